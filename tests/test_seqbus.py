"""The pure check of an automation table and the numbering of the lanes of the buses, as synthesizer_amd/csrc/seqauto.hpp states them for
sequence.hip (sha::check, sha::master_lane, sha::group_lane, sha::lanes), built for the host with g++ -O2 -std=c++17 -Wall -Werror: every
refusal in the order the check reports them, on a track's lane, the master's and a group's; accepted tables with 0 and 8 group lanes; the
lanes in the meter table's row order.  The same cases run inside the C++ file (sb_selfcheck), which a stand-alone build of it with a
``main`` runs as a program.  Equality, no tolerance.  No GPU."""
import ctypes
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
U32 = ctypes.c_uint32
FLAGS = ["-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math"]
OK, FIRST_ENDS, FIRST_DECREASES, RESERVED, ENDS, KIND, MUL, ORIGIN, NUMSAMPLES, VOLUME = range(10)      # sha::Refusal
nan, inf = float("nan"), float("inf")
SONG = 1000


@pytest.fixture(scope="module")
def sb(tmp_path_factory):
    out = tmp_path_factory.mktemp("seqbus") / "libseqbus.so"
    subprocess.run(["g++"] + FLAGS + ["-shared", "-fPIC", str(ROOT / "tests" / "cpu_seqbus.cpp"), "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    lib.sb_check.argtypes = [ctypes.POINTER(ctypes.c_double), U32, ctypes.POINTER(U32), U32, ctypes.c_double, ctypes.POINTER(U32), ctypes.POINTER(U32)]
    for name in ("sb_master_lane", "sb_group_lane", "sb_lanes", "sb_max_group_lanes"):
        getattr(lib, name).restype = U32
    lib.sb_master_lane.argtypes = [U32]
    lib.sb_group_lane.argtypes = [U32, U32]
    lib.sb_lanes.argtypes = [U32, U32]
    return lib


def move(a, b, v0, v1, **kw):
    """(end, origin, mul, slope, numsamples, offset, kind, reserved) of a move over samples [a, b)"""
    row = dict(end=b, origin=a, mul=1.0, slope=v1 - v0, numsamples=float(b - a), offset=v0, kind=1, reserved=0)
    row.update(kw)
    return tuple(row[f] for f in ("end", "origin", "mul", "slope", "numsamples", "offset", "kind", "reserved"))


def gap(b, **kw):
    return move(0, b, 0.0, 0.0, **dict(dict(numsamples=0.0, kind=0), **kw))


def check(sb, lanes, song=SONG, first=None):
    """lanes: a list of segment rows per lane"""
    rows = [float(v) for lane in lanes for seg in lane for v in seg]
    if first is None:
        first = [0]
        for lane in lanes:
            first.append(first[-1] + len(lane))
    lane, segment = U32(99), U32(99)
    why = sb.sb_check((ctypes.c_double * max(1, len(rows)))(*rows), len(rows) // 8, (U32 * len(first))(*first), len(first) - 1, float(song),
                      ctypes.byref(lane), ctypes.byref(segment))
    return (why, lane.value, segment.value) if why else (OK, None, None)


def table(nlanes, lane=None, segment=None, bad=None):
    """every lane a gap to 100 and a move over [100, 200), with ``bad`` in place of one segment"""
    lanes = [[gap(100), move(100, 200, 0.25, 1.0)] for _ in range(nlanes)]
    if lane is not None:
        lanes[lane][segment] = bad
    return lanes


def test_the_cases_inside_the_cpp_file_hold(sb):
    assert sb.sb_selfcheck() == 0
    assert sb.sb_max_group_lanes() == 8


def test_the_lanes_stand_in_the_meter_tables_row_order(sb):
    for ntracks in (1, 3, 6, 32):
        row0 = ntracks + 1                                      # the meter row of group 0, which the kernels know
        assert sb.sb_master_lane(row0) == ntracks
        assert [sb.sb_group_lane(row0, g) for g in range(8)] == [ntracks + 1 + g for g in range(8)]
        assert sb.sb_lanes(ntracks, 0) == ntracks + 1 and sb.sb_lanes(ntracks, 8) == ntracks + 9


@pytest.mark.parametrize("ngroups", [0, 8])
def test_tables_with_no_and_with_eight_group_lanes_pass(sb, ngroups):
    nlanes = 3 + 1 + ngroups
    assert check(sb, table(nlanes)) == (OK, None, None)
    assert check(sb, [[] for _ in range(nlanes)]) == (OK, None, None)                       # no segment at all
    lanes = [[] for _ in range(nlanes)]
    lanes[-1] = [move(0, SONG, 1.0, 0.0)]                                                   # the last lane alone, over the whole song
    assert check(sb, lanes) == (OK, None, None)
    lanes[-1] = [move(0, SONG + 1, 1.0, 0.0)]
    assert check(sb, lanes) == (ENDS, nlanes - 1, 0)


@pytest.mark.parametrize("lane", [1, 3, 11])                    # of 3 tracks and 8 groups: a track's, the master's, the last group's
def test_every_refusal_in_its_order(sb, lane):
    n = 12

    def one(segment, bad):
        return check(sb, table(n, lane, segment, bad))
    good = dict(a=100, b=200, v0=0.25, v1=1.0)
    assert one(1, move(**good, reserved=1, end=50)) == (RESERVED, lane, 1)                  # in front of the end that does not ascend
    assert one(1, move(**good, end=100, kind=2)) == (ENDS, lane, 1)                         # ... which stands in front of the kind
    assert one(1, move(**good, end=SONG + 1)) == (ENDS, lane, 1)
    assert one(1, move(100, SONG, 0.25, 1.0)) == (OK, None, None)                           # to the song's last sample
    assert one(0, gap(0)) == (ENDS, lane, 0)
    assert one(1, move(**good, kind=2, mul=0.5)) == (KIND, lane, 1)
    assert one(1, move(**good, mul=0.5, origin=4)) == (MUL, lane, 1)
    assert one(0, gap(100, mul=0.999)) == (MUL, lane, 0)
    assert one(1, move(**good, origin=99, numsamples=1.0)) == (ORIGIN, lane, 1)
    assert one(0, move(0, 100, 0.5, 0.5)) == (OK, None, None)
    assert one(0, move(0, 100, 0.5, 0.5, origin=1)) == (ORIGIN, lane, 0)
    assert one(1, move(**good, numsamples=99.0, offset=2.0)) == (NUMSAMPLES, lane, 1)
    assert one(1, move(**good, numsamples=nan)) == (NUMSAMPLES, lane, 1)
    assert one(1, move(**good, numsamples=100.5)) == (OK, None, None)
    assert one(1, move(**good, numsamples=inf)) == (VOLUME, lane, 1)
    for offset in (-0.001, 1.001, nan, inf):
        assert one(1, move(**good, offset=offset, slope=0.0)) == (VOLUME, lane, 1)
    for slope in (0.751, -0.251, nan, -inf):
        assert one(1, move(**good, slope=slope)) == (VOLUME, lane, 1)
    assert one(1, move(**good, slope=-0.25)) == (OK, None, None)                            # to exactly 0.0


def test_the_offsets_are_held_in_front_of_every_segment(sb):
    lanes = [[move(0, 100, 0.5, 1.0, reserved=1)], [move(0, 100, 0.5, 1.0)]]
    assert check(sb, lanes, first=[1, 2, 2])[0] == FIRST_ENDS
    assert check(sb, lanes, first=[0, 1, 1])[0] == FIRST_ENDS
    assert check(sb, lanes, first=[0, 2, 1, 2])[:2] == (FIRST_DECREASES, 2)
    assert check(sb, lanes)[:2] == (RESERVED, 0)


def test_a_program_of_its_own_runs_the_same_cases(tmp_path):
    """the file with its ``main``, as a stand-alone build takes it (with sanitizers, where they are wanted: host code alone)"""
    exe = tmp_path / "cpu_seqbus"
    subprocess.run(["g++"] + FLAGS + ["-DSEQBUS_MAIN", str(ROOT / "tests" / "cpu_seqbus.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "0 mismatches" in p.stdout, p.stdout + p.stderr
