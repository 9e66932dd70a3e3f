#!/usr/bin/env python
"""The tables of tests/test_song_calls_host.py in full (CPU only, from the repo root):

    python tools/song_calls.py --dump DIR               every table -- what each call shape of a compiled song's desk does -- one file per name under DIR
                                                        (a directory outside the repository); dump at two commits and `diff -r` the directories
    python tools/song_calls.py --golden COMMIT          write tests/golden/song_calls.json: one digest and the number of shapes per table, made at COMMIT
                                                        (the commit that is checked out), with no shape listed as reordered
    python tools/song_calls.py --reordered DIR          list in the golden file every line whose answer here differs from the dump under DIR, with the answer
                                                        there; the test then refuses a listed line unless both answers are refusals before a launch"""
import json
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tests import test_song_calls_host as T  # noqa: E402


def main(argv):
    patch = pytest.MonkeyPatch()
    try:
        tables = T.tables(patch)
    finally:
        patch.undo()
    if argv[:1] == ["--dump"] and len(argv) == 2:
        out = Path(argv[1]).resolve()
        if ROOT in out.parents or out == ROOT:
            raise SystemExit("the full tables go to a directory outside the repository")
        out.mkdir(parents=True, exist_ok=True)
        for name, lines in tables.items():
            (out / (name.replace("/", ".") + ".txt")).write_text("\n".join(lines) + "\n")
        print("%d tables, %d shapes under %s" % (len(tables), sum(map(len, tables.values())), out))
    elif argv[:1] == ["--golden"] and len(argv) == 2:
        golden = {"commit": argv[1], "tables": {name: [len(lines), T.digest(lines)] for name, lines in tables.items()}, "reordered": {}}
        T.GOLDEN.write_text(json.dumps(golden, indent=1) + "\n")
    elif argv[:1] == ["--reordered"] and len(argv) == 2:
        golden = json.loads(T.GOLDEN.read_text())
        golden["reordered"] = {}
        for name, lines in tables.items():
            were = (Path(argv[1]) / (name.replace("/", ".") + ".txt")).read_text().split("\n")[:-1]
            if [w.split(" -> ", 1)[0] for w in were] != [n.split(" -> ", 1)[0] for n in lines]:
                raise SystemExit("%s: the two grids differ" % name)
            moved = {}
            for k, (was, now) in enumerate(zip(were, lines)):
                if was != now:
                    moved.setdefault((was.split(" -> ", 1)[1], now.split(" -> ", 1)[1]), []).append(k)
            if moved:
                golden["reordered"][name] = [{"was": was, "now": now, "lines": at} for (was, now), at in sorted(moved.items())]
            ndiffer = sum(map(len, moved.values()))
            print("%-28s %6d shapes, %6d identical, %4d differ" % (name, len(lines), len(lines) - ndiffer, ndiffer))
        T.GOLDEN.write_text(json.dumps(golden, indent=1).replace(",\n    ", ", ") + "\n")
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main(sys.argv[1:])
