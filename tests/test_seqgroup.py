"""The checks and the packing of a group list as synthesizer_amd/csrc/seqgroup.hpp states them for sequence.hip (shg::check, shg::pack,
shg::group_of), built for the host with g++ -std=c++17 -Wall: the byte-per-track table against a Python restatement for 0, 1 and 8
groups, every refusal at its boundary (``end == ntracks`` passes, ``end == ntracks + 1`` does not; ranges that touch pass, ranges that
overlap by one do not).  The same cases run inside the C++ file against its own restatement (sg_selfcheck), which a stand-alone build
of it with a ``main`` runs as a program.  Equality, no tolerance.  No GPU."""
import ctypes
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
U32 = ctypes.c_uint32
FLAGS = ["-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math"]
OK, COUNT, RANGE_EMPTY, RANGE_BEYOND, RANGE_ORDER, GAIN_NOT_FINITE, PAN_NOT_FINITE, PAN_NOT_STEREO = range(8)     # shg::Refusal
NONE = 255
nan, inf = float("nan"), float("inf")


@pytest.fixture(scope="module")
def sg(tmp_path_factory):
    out = tmp_path_factory.mktemp("seqgroup") / "libseqgroup.so"
    subprocess.run(["g++"] + FLAGS + ["-shared", "-fPIC", str(ROOT / "tests" / "cpu_seqgroup.cpp"), "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    lib.sg_check.argtypes = [ctypes.POINTER(ctypes.c_double), U32, U32, ctypes.c_int, ctypes.POINTER(U32)]
    lib.sg_pack.argtypes = [ctypes.POINTER(ctypes.c_double), U32, U32, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double),
                            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(U32)]
    lib.sg_pack.restype = U32
    return lib


def rows(groups):
    flat = [float(v) for g in groups for v in g]
    return (ctypes.c_double * max(1, len(flat)))(*flat)


def check(sg, groups, ntracks, nch=2):
    entry = U32(99)
    why = sg.sg_check(rows(groups), len(groups), ntracks, nch, ctypes.byref(entry))
    return (why, entry.value) if why else (OK, None)


def pack(sg, groups, ntracks):
    of = ctypes.create_string_buffer(32)
    gains, pans, count = (ctypes.c_double * 8)(), (ctypes.c_double * 16)(), U32()
    row0 = sg.sg_pack(rows(groups), len(groups), ntracks, of, gains, pans, ctypes.byref(count))
    return list(of.raw), list(gains), list(pans), count.value, row0


def restated(groups, ntracks):
    """the table as the issue states it: a byte per track naming its group or none, 8 gains, 16 pan factors, the count"""
    of = [NONE] * 32
    for i, (first, end, _g, _l, _r) in enumerate(groups):
        for t in range(first, end):
            of[t] = i
    gains = [g[2] for g in groups] + [1.0] * (8 - len(groups))
    pans = [f for g in groups for f in g[3:5]] + [1.0] * (16 - 2 * len(groups))
    return of, gains, pans, len(groups), ntracks + 1


LISTS = {
    "none": ([], 6),
    "one": ([(2, 5, 0.5, 1.0, 1.0)], 6),
    "one over everything": ([(0, 32, -1.5, 0.25, 2.0)], 32),
    "eight of four": ([(4 * i, 4 * i + 4, 0.5 + 0.125 * i, 1.0 - 0.125 * i, 0.25 * i) for i in range(8)], 32),
    "eight with loose tracks between": ([(3 * i + 1, 3 * i + 3, 1.0 + i, 1.0, 1.0) for i in range(8)], 25),
    "touching, across a word of the table": ([(3, 4, 0.0, 0.0, 0.0), (4, 9, 2.0, 1.0, 0.5)], 9),
}


def test_the_cases_inside_the_cpp_file_hold(sg):
    assert sg.sg_selfcheck() == 0
    assert sg.sg_table_bytes() == 232                           # 32 + 64 + 128 + 8 bytes of kernel arguments


@pytest.mark.parametrize("name", list(LISTS))
def test_the_packed_table_names_every_tracks_group(sg, name):
    groups, ntracks = LISTS[name]
    assert pack(sg, groups, ntracks) == restated(groups, ntracks)
    if groups:
        assert check(sg, groups, ntracks) == (OK, None)


def test_every_refusal_at_its_boundary(sg):
    one = (1.0, 1.0, 1.0)
    assert check(sg, [], 6) == (COUNT, 0)
    assert check(sg, [(i, i + 1) + one for i in range(8)], 8) == (OK, None)
    assert check(sg, [(i, i + 1) + one for i in range(9)], 9) == (COUNT, 0)
    assert check(sg, [(0, 6) + one], 6) == (OK, None)                       # end == ntracks
    assert check(sg, [(0, 7) + one], 6) == (RANGE_BEYOND, 0)                # end == ntracks + 1
    assert check(sg, [(0, 2) + one, (5, 7) + one], 6) == (RANGE_BEYOND, 1)
    assert check(sg, [(0, 33) + one], 40) == (RANGE_BEYOND, 0)              # the table holds 32 tracks
    assert check(sg, [(3, 3) + one], 6) == (RANGE_EMPTY, 0)
    assert check(sg, [(4, 3) + one], 6) == (RANGE_EMPTY, 0)
    assert check(sg, [(0, 3) + one, (3, 6) + one], 6) == (OK, None)         # touching
    assert check(sg, [(0, 3) + one, (2, 6) + one], 6) == (RANGE_ORDER, 1)   # overlapping by one
    assert check(sg, [(3, 6) + one, (0, 3) + one], 6) == (RANGE_ORDER, 1)   # out of order
    for bad in (nan, inf, -inf):
        assert check(sg, [(0, 3, bad, 1.0, 1.0)], 6) == (GAIN_NOT_FINITE, 0)
        assert check(sg, [(0, 3) + one, (3, 4, 1.0, bad, 1.0)], 6) == (PAN_NOT_FINITE, 1)
        assert check(sg, [(0, 3, 1.0, 1.0, bad)], 6, nch=1) == (PAN_NOT_FINITE, 0)
    assert check(sg, [(0, 3, 2.0, 1.0, 1.0)], 6, nch=1) == (OK, None)       # a mono song has group faders
    assert check(sg, [(0, 3, 2.0, 1.0, 0.5)], 6, nch=1) == (PAN_NOT_STEREO, 0)
    assert check(sg, [(0, 3, 2.0, 0.999, 1.0)], 6, nch=4) == (PAN_NOT_STEREO, 0)
    assert check(sg, [(0, 3, 0.0, 0.0, 0.0)], 6) == (OK, None)              # a silent group is a legal one


def test_a_program_of_its_own_runs_the_same_cases(tmp_path):
    """the file with its ``main``, as a stand-alone build takes it (with sanitizers, where they are wanted: host code alone)"""
    exe = tmp_path / "cpu_seqgroup"
    subprocess.run(["g++"] + FLAGS + ["-DSEQGROUP_MAIN", str(ROOT / "tests" / "cpu_seqgroup.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "0 mismatches" in p.stdout, p.stdout + p.stderr
