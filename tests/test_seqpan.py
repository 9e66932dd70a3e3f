"""The pan lane's statements as synthesizer_amd/csrc/seqpan.hpp makes them for sequence.hip (shp::check, shp::shape_from, shp::track_lane,
shp::group_lane), built for the host with g++ -O2 -std=c++17 -Wall -Werror: the lane statement, run tile by tile as the kernels run it,
against a plain Python loop over the frames -- ``Sample.pan(lfo=...)``'s expression where a move holds the frame, ``audioop.mul`` per
side where none does -- on lanes that take each of the three paths; every refusal of the check in the order it reports them; the pan
lanes behind the fader lanes' offsets.  The same and more (random lanes, origins past 2^31 samples, the endpoints at extreme samples) run
inside the C++ file (sp_selfcheck), which a stand-alone build of it with a ``main`` runs as a program.  Equality, no tolerance.  No GPU."""
import audioop
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
U32 = ctypes.c_uint32
FLAGS = ["-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math"]
OK, FIRST_ENDS, FIRST_DECREASES, RESERVED, ENDS, ODD, KIND, MUL, ORIGIN, NUMSAMPLES, RANGE = range(11)      # shp::Refusal
nan, inf = float("nan"), float("inf")
SONG = 1000                                                     # samples: 500 frames


@pytest.fixture(scope="module")
def sp(tmp_path_factory):
    out = tmp_path_factory.mktemp("seqpan") / "libseqpan.so"
    subprocess.run(["g++"] + FLAGS + ["-shared", "-fPIC", str(ROOT / "tests" / "cpu_seqpan.cpp"), "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    lib.sp_check.argtypes = [ctypes.POINTER(ctypes.c_double), U32, ctypes.POINTER(U32), U32, ctypes.c_double, ctypes.POINTER(U32), ctypes.POINTER(U32)]
    lib.sp_shape.argtypes = [ctypes.POINTER(ctypes.c_double), U32, ctypes.POINTER(ctypes.c_int), U32, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                             ctypes.c_double]
    for name in ("sp_track_lane", "sp_group_lane", "sp_lanes", "sp_kind"):
        getattr(lib, name).restype = U32
    lib.sp_track_lane.argtypes = [U32, U32]
    lib.sp_group_lane.argtypes = [U32, U32]
    lib.sp_lanes.argtypes = [U32, U32]
    return lib


def move(a, b, p0, p1, **kw):
    """(end, origin, mul, slope, numsamples, offset, kind, reserved) of a pan move over FRAMES [a, b)"""
    row = dict(end=2 * b, origin=2 * a, mul=1.0, slope=p1 - p0, numsamples=float(b - a), offset=p0, kind=3, reserved=0)
    row.update(kw)
    return tuple(row[f] for f in ("end", "origin", "mul", "slope", "numsamples", "offset", "kind", "reserved"))


def gap(b, **kw):
    return move(0, b, 0.0, 0.0, **dict(dict(numsamples=0.0, kind=0), **kw))


def check(sp, lanes, song=SONG, first=None):
    rows = [float(v) for lane in lanes for seg in lane for v in seg]
    if first is None:
        first = [0]
        for lane in lanes:
            first.append(first[-1] + len(lane))
    lane, segment = U32(99), U32(99)
    why = sp.sp_check((ctypes.c_double * max(1, len(rows)))(*rows), len(rows) // 8, (U32 * len(first))(*first), len(first) - 1, float(song),
                      ctypes.byref(lane), ctypes.byref(segment))
    return (why, lane.value, segment.value) if why else (OK, None, None)


def table(nlanes, lane=None, segment=None, bad=None):
    """every lane a gap to frame 50 and a move over frames [50, 100), with ``bad`` in place of one segment"""
    lanes = [[gap(50), move(50, 100, -0.25, 1.0)] for _ in range(nlanes)]
    if lane is not None:
        lanes[lane][segment] = bad
    return lanes


def test_the_cases_inside_the_cpp_file_hold(sp):
    assert sp.sp_selfcheck() == 0
    assert sp.sp_kind() == 3


def test_the_pan_lanes_stand_behind_the_fader_lanes_offsets(sp):
    for ntracks in (1, 3, 6, 32):
        row0 = ntracks + 1                                      # the meter row of group 0, which the kernels know
        fader_offsets = ntracks + 1 + 8 + 1                     # tracks, the master, eight groups, the end
        assert [sp.sp_track_lane(row0, t) for t in range(ntracks)] == [fader_offsets + t for t in range(ntracks)]
        assert [sp.sp_group_lane(row0, g) for g in range(8)] == [fader_offsets + ntracks + g for g in range(8)]
        assert sp.sp_lanes(ntracks, 0) == ntracks and sp.sp_lanes(ntracks, 8) == ntracks + 8


# ---- the lane statement against a plain loop over the frames ----------------------------------------------------------------------------------
def straight(x, pieces, left, right, width):
    """the chain's pan step in Python ints and floats: a piece's frames by Sample.pan(lfo=...)'s expression, the rest by audioop.mul per side"""
    dtype = {1: np.int8, 2: "<i2", 4: "<i4"}[width]
    y = list(x)
    for c, f in ((0, left), (1, right)):
        if f != 1.0:
            y[c::2] = np.frombuffer(audioop.mul(np.asarray(x[c::2], dtype=dtype).tobytes(), width, f), dtype=dtype).tolist()
    for a, b, p0, p1 in pieces:
        n = b - a
        for k in range(n):
            p = k * (p1 - p0) / n + p0
            y[2 * (a + k)] = int(x[2 * (a + k)] * (1.0 - p) / 2.0)
            y[2 * (a + k) + 1] = int(x[2 * (a + k) + 1] * (1.0 + p) / 2.0)
    return y


def rows_of(pieces):
    rows, at = [], 0
    for a, b, p0, p1 in pieces:
        if a > at:
            rows.append(gap(a))
        rows.append(move(a, b, p0, p1))
        at = b
    return rows


LANES = {
    "no segment": (),
    "one move over everything": ((0, 4096, -1.0, 1.0),),
    "moves on tile edges": ((512, 1024, 1.0, -1.0), (1024, 2048, 0.3, 0.3)),
    "across edges, adjacent with a jump, one frame, holds": ((3, 4, 0.5, 0.5), (500, 530, 0.8, -0.3), (530, 1500, 0.9, -1.0), (1500, 1501, 0.0, 0.0),
                                                             (2047, 2049, -1.0, -1.0), (2100, 2200, 1.0, 1.0), (3000, 3001, 0.0, 0.0)),
    "a gap that ends on a tile's edge": ((1024, 1030, 0.1, 0.2), (2050, 2060, 0.0, 0.0)),
}


@pytest.mark.parametrize("lane_width, width", [(4, 1), (8, 2), (4, 4)])
@pytest.mark.parametrize("name", sorted(LANES))
def test_the_lane_statement_is_the_plain_loop_over_the_frames(sp, name, lane_width, width):
    pieces = LANES[name]
    nsamples = 5 * 2048                                         # five tiles of 2048 samples, ten of 1024; the lanes end inside
    rng = np.random.default_rng(len(name) + 10 * width)
    lo, hi = -2 ** (8 * width - 1), 2 ** (8 * width - 1) - 1
    x = rng.integers(lo, hi + 1, nsamples).tolist()
    x[0:6] = [lo, lo, hi, hi, -1, -1]
    x[2 * 1024:2 * 1024 + 4] = [lo, hi, hi, lo]
    rows = [float(v) for seg in rows_of(pieces) for v in seg]
    for left, right in ((1.0, 1.0), (0.35, 0.65), (1.5, 0.0)):
        got = (ctypes.c_int * nsamples)(*x)
        assert sp.sp_shape((ctypes.c_double * max(1, len(rows)))(*rows), len(rows) // 8, got, nsamples, lane_width, width, left, right) == 0
        assert list(got) == straight(x, pieces, left, right, width), (name, left, right)


# ---- the check --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ngroups", [0, 8])
def test_tables_with_no_and_with_eight_group_lanes_pass(sp, ngroups):
    nlanes = 3 + ngroups
    assert check(sp, table(nlanes)) == (OK, None, None)
    assert check(sp, [[] for _ in range(nlanes)]) == (OK, None, None)
    lanes = [[] for _ in range(nlanes)]
    lanes[-1] = [move(0, SONG // 2, 1.0, -1.0)]                 # the last lane alone, over the whole song
    assert check(sp, lanes) == (OK, None, None)
    lanes[-1] = [move(0, SONG // 2 + 1, 1.0, -1.0)]
    assert check(sp, lanes) == (ENDS, nlanes - 1, 0)


@pytest.mark.parametrize("lane", [1, 10])                       # of 3 tracks and 8 groups: a track's, the last group's
def test_every_refusal_in_its_order(sp, lane):
    n = 11

    def one(segment, bad):
        return check(sp, table(n, lane, segment, bad))
    good = dict(a=50, b=100, p0=-0.25, p1=1.0)
    assert one(1, move(**good, reserved=1, end=50)) == (RESERVED, lane, 1)                  # in front of the end that does not ascend
    assert one(1, move(**good, end=100, kind=1)) == (ENDS, lane, 1)                         # ... which stands in front of the kind
    assert one(1, move(**good, end=SONG + 2)) == (ENDS, lane, 1)
    assert one(1, move(50, SONG // 2, -0.25, 1.0)) == (OK, None, None)                      # to the song's last frame
    assert one(0, gap(0)) == (ENDS, lane, 0)
    assert one(1, move(**good, end=199, kind=1)) == (ODD, lane, 1)                          # half a frame, in front of the kind
    assert one(0, gap(50, end=99)) == (ODD, lane, 0)
    for kind in (1, 2, 4):
        assert one(1, move(**good, kind=kind, mul=0.5)) == (KIND, lane, 1)                  # a fade is no pan move
    assert one(1, move(**good, mul=0.5, origin=4)) == (MUL, lane, 1)
    assert one(0, gap(50, mul=0.999)) == (MUL, lane, 0)
    assert one(1, move(**good, origin=98, numsamples=1.0)) == (ORIGIN, lane, 1)
    assert one(0, move(0, 50, 0.5, 0.5)) == (OK, None, None)
    assert one(0, move(0, 50, 0.5, 0.5, origin=2)) == (ORIGIN, lane, 0)
    assert one(1, move(**good, numsamples=49.0, offset=2.0)) == (NUMSAMPLES, lane, 1)       # its FRAMES are 50
    assert one(1, move(**good, numsamples=nan)) == (NUMSAMPLES, lane, 1)
    assert one(1, move(**good, numsamples=50.5)) == (OK, None, None)
    assert one(1, move(**good, numsamples=inf)) == (RANGE, lane, 1)
    for offset in (-1.001, 1.001, nan, inf):
        assert one(1, move(**good, offset=offset, slope=0.0)) == (RANGE, lane, 1)
    for slope in (1.251, -0.751, nan, -inf):
        assert one(1, move(**good, slope=slope)) == (RANGE, lane, 1)
    assert one(1, move(**good, slope=-0.75)) == (OK, None, None)                            # to exactly -1.0
    assert one(1, move(50, 100, -1.0, 1.0)) == one(1, move(50, 100, 1.0, -1.0)) == (OK, None, None)


def test_the_offsets_are_held_in_front_of_every_segment(sp):
    lanes = [[move(0, 50, 0.5, 1.0, reserved=1)], [move(0, 50, 0.5, 1.0)]]
    assert check(sp, lanes, first=[1, 2, 2])[0] == FIRST_ENDS
    assert check(sp, lanes, first=[0, 1, 1])[0] == FIRST_ENDS
    assert check(sp, lanes, first=[0, 2, 1, 2])[:2] == (FIRST_DECREASES, 2)
    assert check(sp, lanes)[:2] == (RESERVED, 0)


def test_a_program_of_its_own_runs_the_same_cases(tmp_path):
    """the file with its ``main``, as a stand-alone build takes it (with sanitizers, where they are wanted: host code alone)"""
    exe = tmp_path / "cpu_seqpan"
    subprocess.run(["g++"] + FLAGS + ["-DSEQPAN_MAIN", str(ROOT / "tests" / "cpu_seqpan.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "0 mismatches" in p.stdout, p.stdout + p.stderr
