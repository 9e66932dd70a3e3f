"""What the desk of a compiled song DOES with a call, written down shape by shape (no GPU; the fake native layer of tests/songhost.py): a
grid of keyword values walked through every door -- ``render`` of a window and of an empty one, ``render_into``, the first item of
``chunks``, ``stems``, ``stems_into``, ``CompiledSequence.level_history`` -- of four songs (stereo, mono, flat, closed), each shape
recorded as what the fake ``N.Sequence.render`` / ``.stems`` was handed plus the type and shape of what came back, or as the exception's
type and message; and the same for ``automation()`` over a grid of lanes, recorded as the packed tables and what the fake
``N.SeqAutomation`` was handed.  tests/golden/song_calls.json holds one digest and the number of shapes per (door, song), made at the
commit it names; ``reordered`` there lists the lines whose answer was changed on purpose since, with the answer there was.
``python tools/song_calls.py`` dumps the full tables."""
import hashlib
import itertools
import json
from pathlib import Path

import numpy as np
import pytest

from synthesizer_amd import _native as N
from synthesizer_amd import mixer
from tests.songhost import RATE, _Auto, _ClipSeq, _fake, _mono, _StemBuf, _stereo

GOLDEN = Path(__file__).resolve().parent / "golden" / "song_calls.json"
nan, inf = float("nan"), float("inf")
FADE = [[(0, 100, 0.5, 1.0)], None, None]

# (label, value, good): a value is good where a stereo song of tracks takes it alone
KEYWORDS = {
    "gains": [("None", None, True), ("good", (0.5, 1.0, 2.0), True), ("short", (0.5, 1.0), False), ("nan", (0.5, nan, 1.0), False)],
    "meters": [("False", False, True), ("True", True, True), ("history", "history", True), ("bad", "History", False)],
    "pans": [("None", None, True), ("nones", [None] * 3, True), ("number", (0.3, None, None), True), ("pair", (None, (0.5, 0.25), None), True),
             ("bad", (None, 1.5, None), False)],
    "master": [("None", None, True), ("one", 1.0, True), ("half", 0.5, True), ("nan", nan, False)],
    "groups": [("None", None, True), ("empty", [], True), ("two", [(0, 1, 0.5), (1, 3, None)], True),
               ("three", [(0, 1, 0.5), (1, 2, None, 0.3), (2, 3, 2.0, (0.5, 0.25))], True), ("overlap", [(0, 2, 1.0), (1, 3, 1.0)], False),
               ("strgain", [(0, 1, "0.5")], False)],
    "automation": [("None", True), ("faders", True), ("master", True), ("group1", True), ("pan", True), ("grouppan1", True), ("other", False),
                   ("closed", False), ("notauto", False)],
    "clips": [("False", False, True), ("True", True, True)],
}
RENDER_KEYS = ("gains", "meters", "pans", "master", "groups", "automation", "clips")
STEMS_KEYS = ("gains", "pans", "master", "groups", "automation")
DOORS = {
    "render": (RENDER_KEYS, lambda cs, kw: cs.render(10, 20, **kw)),
    "render_empty": (RENDER_KEYS, lambda cs, kw: cs.render(3, 0, **kw)),
    "render_into": (RENDER_KEYS, lambda cs, kw: cs.render_into(N.DeviceBuffer(100), 4, 3, 9, **kw)),
    "chunks": (RENDER_KEYS, lambda cs, kw: next(cs.chunks(100, **kw))),
    "stems": (STEMS_KEYS, lambda cs, kw: cs.stems(10, 21, **kw)),
    "stems_into": (STEMS_KEYS, lambda cs, kw: cs.stems_into(N.DeviceBuffer(100000), 6, 300, 3, 9, **kw)),
    "level_history": (STEMS_KEYS, lambda cs, kw: cs.level_history(10, 21, **kw)),
}
SONGS = ("stereo", "mono", "flat", "closed")


class _CallSeq(_ClipSeq):
    """_ClipSeq, whose meters have a row per group as well and which keeps what each stems call was handed, among the renders"""

    def render(self, first_sample, nsamples, out, out_sample=0, **kw):
        if kw.get("meters") is True:
            self.rendered.append((first_sample, nsamples, out_sample, kw))
            return [((0, 0), (0, 0))] * (4 + len(kw.get("groups") or ()))
        return _ClipSeq.render(self, first_sample, nsamples, out, out_sample, **kw)

    def stems(self, first_sample, nsamples, out, out_sample, plane_samples, **kw):
        self.rendered.append(("stems", first_sample, nsamples, out_sample, plane_samples, kw))


def _level_blocks(buf, sample_offset, nframes, nch, width, plane_samples, nplanes, origin_frame, block_frames):
    nblocks = (origin_frame + nframes - 1) // block_frames - origin_frame // block_frames + 1 if nframes > 0 else 0
    return np.zeros((nblocks, nplanes), dtype=N.SEQ_METER_DTYPE)


def _patch(monkeypatch):
    _fake(monkeypatch)
    monkeypatch.setattr(N, "DeviceBuffer", _StemBuf)
    monkeypatch.setattr(N, "Sequence", _CallSeq)
    monkeypatch.setattr(N, "SeqAutomation", _Auto)
    monkeypatch.setattr(N, "pcm_level_blocks", _level_blocks)
    del _Auto.made[:]


def _tracks(nch, width=2):
    a = _stereo(1000, width) if nch == 2 else _mono(1000, width)
    return mixer.compile_tracks([[(0.0, a), (0.5, a, 0.5)], [], [(0.25, a)]], RATE, nch, width, name="tune")


def _make_song(which):
    """the song, and its ``automation=`` values by label (those it cannot make are left out)"""
    other = _tracks(2)
    autos = {"None": None, "other": other.automation(FADE), "closed": other.automation(FADE), "notauto": "x"}
    autos["closed"].close()
    if which == "flat":
        return mixer.compile_sequence([(0.0, _stereo())], RATE, 2), autos
    cs = _tracks(1 if which == "mono" else 2)
    piece = [(0, 10, 0.5, 1.0)]
    autos.update(faders=cs.automation(FADE), master=cs.automation(FADE, master=piece), group1=cs.automation(FADE, groups=[None, piece]))
    if which != "mono":
        autos.update(pan=cs.automation(FADE, pans=[[(0, 10, -1.0, 1.0)], None, None]), grouppan1=cs.automation(FADE, group_pans=[None, [(0, 10, 0.0, 1.0)]]))
    if which == "closed":
        cs.close()
    return cs, autos


def _values(key, autos):
    if key == "automation":
        return [(label, autos[label], good) for label, good in KEYWORDS[key] if label in autos]
    return KEYWORDS[key]


def _shapes(keys, autos):
    """the product of the good values, and every pair of keywords through all of their values -- the others at their defaults and at a
    full desk: pairs of wrong values are what the order of the checks decides"""
    values = [_values(k, autos) for k in keys]
    seen = set(itertools.product(*[[i for i, v in enumerate(vs) if v[2]] for vs in values]))
    full = {"gains": 1, "meters": 1, "pans": 2, "master": 2, "groups": 3, "automation": 1 if "faders" in autos else 0, "clips": 0}
    for base in ([0] * len(keys), [full[k] for k in keys]):
        for a, b in itertools.combinations(range(len(keys)), 2):
            for i, j in itertools.product(range(len(values[a])), range(len(values[b]))):
                shape = list(base)
                shape[a], shape[b] = i, j
                seen.add(tuple(shape))
    return values, sorted(seen)


def _canon(v, handles):
    if isinstance(v, dict):
        return "{" + ", ".join("%s=%s" % (k, _canon(v[k], handles)) for k in sorted(v)) + "}"
    if isinstance(v, (list, tuple)):
        return ("[%s]" if isinstance(v, list) else "(%s)") % ", ".join(_canon(x, handles) for x in v)
    if isinstance(v, _Auto):
        return "<SeqAutomation %s>" % handles.get(id(v), "?")
    if isinstance(v, np.ndarray):
        return "<%s %s %s>" % (v.dtype.str if v.dtype.names is None else "rows", v.shape, hashlib.sha256(v.tobytes()).hexdigest()[:16])
    if isinstance(v, mixer.Sample):
        return "Sample(%r, %d frames, %d ch, width %d)" % (v.name, len(v), v.nchannels, v.samplewidth)
    if isinstance(v, mixer.SongHistory):
        return "%r rows=%s clipped=%s ngroups=%d total=%r" % (v, v.peak.shape, None if v.clipped() is None else v.clipped().shape, v.ngroups, v.total())
    if isinstance(v, mixer.SongStems):
        return "%r plane_frames=%r buffer=%r" % (v, v._plane_frames, None if v._buffer is None else v._buffer.nbytes)
    return "%s %r" % (type(v).__name__, v) if isinstance(v, (float, np.generic)) else repr(v)


def _record(call, seq, handles):
    del seq.rendered[:]
    try:
        got = call()
    except Exception as e:      # noqa: BLE001 -- every refusal is a record
        return "%s: %s | handed %s" % (type(e).__name__, e, _canon(list(seq.rendered), handles))
    return "%s %s | handed %s" % (type(got).__name__, _canon(got, handles), _canon(list(seq.rendered), handles))


def render_table(monkeypatch, door, which):
    """the lines ``shape -> record`` of one door of one song"""
    _patch(monkeypatch)
    cs, autos = _make_song(which)
    handles = {id(a._auto): label for label, a in autos.items() if isinstance(a, mixer.Automation) and a._auto is not None}
    keys, go = DOORS[door]
    values, shapes = _shapes(keys, autos)
    seq, lines = cs._seq if cs._seq is not None else _CallSeq(*[None] * 6), []
    for shape in shapes:
        picked = [vs[i] for vs, i in zip(values, shape)]
        kw = {k: p[1] for k, p in zip(keys, picked)}
        lines.append("%s -> %s" % (" ".join("%s=%s" % (k, p[0]) for k, p in zip(keys, picked)), _record(lambda: go(cs, kw), seq, handles)))
    return lines


piece, unity = (0, 100, 0.5, 1.0), (200, 300, 1.0, 1.0)
LANES = {
    "lanes": [("nones", [None] * 3), ("fade", [[piece], None, None]), ("unity", [[piece, unity, (400, 500, 1, 0)], None, [unity]]),
              ("short", [None] * 2), ("high", [None, [(0, 10, 1.5, 1.0)], None]), ("overlap", [[piece, (50, 150, 0.5, 0.5)], None, None]),
              ("number", 5), ("past", [None, None, [(0, 10 ** 6, 0.0, 1.0)]])],
    "master": [("None", None), ("fade", [piece]), ("unity", [unity]), ("nan", [(0, 10, nan, 1.0)])],
    "groups": [("None", None), ("second", [None, [piece, unity]]), ("nine", [None] * 9), ("str", [[(0, 10, "a", 1.0)]])],
    "pans": [("None", None), ("nones", [None] * 3), ("sweep", [[(0, 10, -1.0, 1.0), (20, 30, 0.0, 0.0)], None, None]), ("short", [None]),
             ("low", [None, [(0, 10, -1.5, 0.0)], None])],
    "group_pans": [("None", None), ("second", [None, [(5, 10, 0.0, 1.0)]]), ("bool", [[(True, 10, 0.0, 1.0)]])],
}
LANE_SONGS = {"stereo": lambda: _tracks(2), "mono": lambda: _tracks(1), "wide": lambda: _tracks(2, 4), "three_bytes": lambda: _tracks(2, 3),
              "flat": lambda: mixer.compile_sequence([(0.0, _stereo())], RATE, 2), "closed": lambda: _tracks(2)}


def automation_table(monkeypatch, which):
    """the lines ``lanes -> record`` of ``automation()`` of one song, over the whole grid"""
    _patch(monkeypatch)
    cs = LANE_SONGS[which]()
    if which == "closed":
        cs.close()
    lines = []
    for picked in itertools.product(*LANES.values()):
        kw = {k: p[1] for k, p in zip(LANES, picked)}
        del _Auto.made[:]
        try:
            a = cs.automation(kw.pop("lanes"), **kw)
            made = [("same segments" if h.segments is a.segments else "other segments", h.seg_first, h.rest) for h in _Auto.made]
            got = _canon(dict(pieces=a.pieces, segments=a.segments, seg_first=a.seg_first, master=a.master, groups=a.groups, pans=a.pans,
                              group_pans=a.group_pans, pan_segments=a.pan_segments, pan_first=a.pan_first, rides=a.rides, pan_rides=a.pan_rides,
                              made=made), {})
        except Exception as e:      # noqa: BLE001
            got = "%s: %s | made %d" % (type(e).__name__, e, len(_Auto.made))
        lines.append("%s -> %s" % (" ".join("%s=%s" % (k, p[0]) for k, p in zip(LANES, picked)), got))
    return lines


def tables(monkeypatch):
    """every table by name: ``door/song`` and ``automation/song``"""
    out = {"%s/%s" % (door, which): render_table(monkeypatch, door, which) for door in DOORS for which in SONGS}
    out.update({"automation/%s" % which: automation_table(monkeypatch, which) for which in LANE_SONGS})
    return out


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def as_it_was(name, lines, reordered):
    """``lines`` with the answers there were put back where ``reordered`` lists a line: ``{table: [{"was": answer, "now": answer, "lines":
    [index, ...]}, ...]}``; a listed line must give ``now``, and both answers must be refusals before anything is handed on -- the one
    kind of change the list may hold: a call wrong in two ways, of which ``render`` and ``chunks`` now name the groups first"""
    out = list(lines)
    for entry in reordered.get(name, []):
        was, now = entry["was"], entry["now"]
        assert all(a.split(": ")[0].endswith("Error") and a.endswith(" | handed []") for a in (was, now)), (name, was, now)
        assert "group" in now and ("pan" in was or "master" in was), (name, was, now)      # the groups' check moved in front of these two
        for k in entry["lines"]:
            shape, got = lines[k].split(" -> ", 1)
            assert got == now, "%s: %s gives %r, listed as %r" % (name, shape, got, now)
            out[k] = "%s -> %s" % (shape, was)
    return out


@pytest.fixture(scope="module")
def recorded():
    patch = pytest.MonkeyPatch()
    try:
        return tables(patch)
    finally:
        patch.undo()


def test_every_call_shape_does_what_it_did(recorded):
    golden = json.loads(GOLDEN.read_text())
    assert sorted(recorded) == sorted(golden["tables"])
    wrong = []
    for name, lines in recorded.items():
        was = as_it_was(name, lines, golden["reordered"])
        if [len(lines), digest(was)] != golden["tables"][name]:
            wrong.append(name)
    assert not wrong, ("these tables differ from the recorded ones: %s.  `python tools/song_calls.py --dump DIR` writes the full tables, one "
                       "file per name, to a directory outside the repository: run it at commit %s and here, and diff the two directories"
                       % (", ".join(wrong), golden["commit"]))


def test_the_grid_holds_what_it_should(recorded):
    assert len(recorded) == len(DOORS) * len(SONGS) + len(LANE_SONGS)
    stereo = recorded["render/stereo"]
    for key, values in KEYWORDS.items():
        for v in values:
            assert any("%s=%s " % (key, v[0]) in line + " " for line in stereo), (key, v[0])
    # every pair of wrong values is there, both ways round a check could fall
    assert any(line.startswith("gains=None meters=False pans=bad master=None groups=overlap ") for line in stereo)
    assert any(line.startswith("gains=nan meters=bad ") for line in stereo)
    assert all("closed" in line.split(" -> ")[1] for door in DOORS for line in recorded["%s/closed" % door])
    launched = [line for line in stereo if not line.endswith("handed []")]
    assert len(launched) > 1000 and all("Error" not in line.split(" | ")[0] for line in launched)
