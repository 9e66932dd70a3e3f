#!/usr/bin/env python3
"""Compare the kernels of two device-assembly files, kernel by kernel.

    hipcc --offload-arch=gfx950 <the flags of synthesizer_amd/build.py> --cuda-device-only -S csrc/X.hip -o parent.s    (at the parent)
    hipcc ...                                                                                 -o here.s      (in this tree)
    python tools/kernel_diff.py parent.s here.s [--rename map.json] [--show N]

Prints one line -- parent kernels / kernels here / identical / differing / missing / added -- and the names behind the last three.
A kernel is a symbol with an .amdhsa_kernel block.  Two kernels are identical where BOTH agree: the body (the lines from the symbol's
label to its end, comments stripped, function-local labels numbered in order of appearance) and the .amdhsa_* block (registers, LDS,
scratch, kernel-argument size).  Kernels are matched by DEMANGLED name; --rename gives a JSON object of old -> new spellings of
template arguments (whole words), applied to the parent's demangled names, for a change that renames types and nothing else.  The
kernel's own mangled name inside its text counts as "itself".  Text is compared and nothing else: no instruction is looked for.
Exit status 0 where every parent kernel is identical here and none was added, 1 otherwise."""
from __future__ import annotations

import argparse
import difflib
import json
import re
import shutil
import subprocess
import sys

LOCAL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")             # .LBB12_3, .Ltmp7, .LJTI4_0, .Lfunc_end12


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin") or shutil.which("c++filt")
    if not tool or not names:
        return list(names)                                   # (no demangler: a rename map cannot apply, equal names still match)
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return [re.sub(r">\s+(?=>)", ">", name) for name in out[:len(names)]]       # (a demangler's "> >" is ">>")


def clean(lines, own):
    """The lines as compared: no comments, no blank lines, the kernel's own symbol as @SELF, local labels by order of appearance."""
    seen = {}

    def label(m):
        return seen.setdefault(m.group(0), ".L%d" % len(seen))

    out = []
    for line in lines:
        line = line.split(";", 1)[0].strip()
        if line:
            out.append(LOCAL.sub(label, line.replace(own, "@SELF")))
    return out


def kernels(path):
    """{mangled name: (body lines, .amdhsa lines)} of one assembly file."""
    text = open(path, errors="replace").read().split("\n")
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line) for line in text) if m]
    wanted = set(names)
    found = {}
    i = 0
    while i < len(text):
        line = text[i]
        m = re.match(r"(\S+):\s*(?:;.*)?$", line)
        if m and m.group(1) in wanted and m.group(1) not in found:
            name, j = m.group(1), i + 1
            while j < len(text) and not re.match(r"\s*\.amdhsa_kernel\s", text[j]) and not re.match(r"\.Lfunc_end\d+:", text[j]):
                j += 1
            body = [t for t in text[i + 1:j] if not re.match(r"\s*\.(section|p2align|text)\b", t)]
            while j < len(text) and not re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(name) + r"\s*$", text[j]):
                j += 1
            k = j
            while k < len(text) and not re.match(r"\s*\.end_amdhsa_kernel", text[k]):
                k += 1
            found[name] = (clean(body, name), clean(text[j + 1:k], name))
            i = k
        i += 1
    missing = wanted - set(found)
    if missing:
        sys.exit("%s: %d kernels with a descriptor and no body, e.g. %s" % (path, len(missing), sorted(missing)[0]))
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("here")
    ap.add_argument("--rename", help="JSON object: old spelling -> new spelling, applied to the parent's demangled names")
    ap.add_argument("--show", type=int, default=20, help="how many names of each kind to print (default 20)")
    ap.add_argument("--diff", help="print the unified diff of the kernel whose (new) demangled name contains this text")
    args = ap.parse_args()
    rename = json.load(open(args.rename)) if args.rename else {}
    sides = []
    for path, renamed in ((args.parent, True), (args.here, False)):
        ks = kernels(path)
        mangled = sorted(ks)
        by_name = {}
        for sym, name in zip(mangled, demangle(mangled)):
            if renamed:
                for old in sorted(rename, key=len, reverse=True):
                    name = re.sub(r"(?<![\w])" + re.escape(old) + r"(?![\w<])", rename[old], name)
            if name in by_name:
                sys.exit("%s: two kernels demangle to %s" % (path, name))
            by_name[name] = ks[sym]
        sides.append(by_name)
    parent, here = sides
    same, body, desc = [], [], []
    for name in sorted(set(parent) & set(here)):
        b, d = parent[name][0] == here[name][0], parent[name][1] == here[name][1]
        (same if b and d else body if not b else desc).append(name)
    missing, added = sorted(set(parent) - set(here)), sorted(set(here) - set(parent))
    print("parent kernels %d   kernels here %d   identical %d   differing %d   missing %d   added %d"
          % (len(parent), len(here), len(same), len(body) + len(desc), len(missing), len(added)))
    print("bodies equal %d of %d matched, .amdhsa_* blocks equal %d of %d matched"
          % (len(same) + len(desc), len(same) + len(body) + len(desc), len(same) + len([n for n in body if parent[n][1] == here[n][1]]), len(same) + len(body) + len(desc)))
    for title, names in (("differing in the body", body), ("differing in the .amdhsa_* block alone", desc), ("missing here", missing), ("added here", added)):
        for name in names[:args.show]:
            print("  %s: %s" % (title, name))
        if len(names) > args.show:
            print("  %s: ... and %d more" % (title, len(names) - args.show))
    if args.diff:
        for name in sorted(set(parent) & set(here)):
            if args.diff in name:
                for part, what in ((0, "body"), (1, ".amdhsa")):
                    sys.stdout.write("\n".join(difflib.unified_diff(parent[name][part], here[name][part], "parent " + what, "here " + what, lineterm="", n=2)) + "\n")
                break
    return 0 if not (body or desc or missing or added) else 1


if __name__ == "__main__":
    sys.exit(main())
