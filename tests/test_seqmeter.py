"""csrc/seqmeter.hpp -- the level meters of a song of tracks -- built for the host with g++, against Python integers: a lane's partial row
(per channel the peak, max |x|, and the exact sum of x * x as sq_hi * 2^32 + sq_lo) from its 4 or 8 samples cut to a window, the
combination of two partial rows, and the split of x * x.  No GPU."""
import ctypes as C
import random
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


class Row(C.Structure):
    _fields_ = [("peak", C.c_uint32 * 2), ("sq_hi", C.c_uint64 * 2), ("sq_lo", C.c_uint64 * 2)]


@pytest.fixture(scope="module")
def sm(tmp_path_factory):
    out = tmp_path_factory.mktemp("seqmeter") / "libseqmeter.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", str(ROOT / "tests" / "cpu_seqmeter.cpp"), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.sm_row_bytes.restype = lib.sm_magnitude.restype = C.c_uint32
    lib.sm_magnitude.argtypes = [C.c_int64]
    lib.sm_square.argtypes = [C.c_int, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.sm_square.restype = None
    lib.sm_lane.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Row)]
    lib.sm_lane.restype = None
    lib.sm_fold.argtypes = [C.POINTER(Row), C.POINTER(Row)]
    lib.sm_fold.restype = None
    return lib


def lane(sm, width, x, s0, lo, hi, nch):
    r = Row()
    sm.sm_lane(int(width >= 3), len(x), (C.c_int64 * len(x))(*x), s0, lo, hi, nch, C.byref(r))
    return r


def value(r):
    """(peaks, sums) of a row, the sums as Python ints"""
    return (r.peak[0], r.peak[1]), ((r.sq_hi[0] << 32) + r.sq_lo[0], (r.sq_hi[1] << 32) + r.sq_lo[1])


def want(x, s0, lo, hi, nch):
    peak, sq = [0, 0], [0, 0]
    for j, v in enumerate(x):
        if lo <= s0 + j < hi:
            c = (s0 + j) & 1 if nch == 2 else 0
            peak[c] = max(peak[c], abs(v))
            sq[c] += v * v
    return tuple(peak), tuple(sq)


def lane_samples(width):
    return 8 if width == 2 else 4


def test_a_row_is_forty_bytes_as_the_header_says(sm):
    assert sm.sm_row_bytes() == 40 == C.sizeof(Row)
    header = (ROOT / "include" / "synthhip.h").read_text()
    assert "} sh_seq_meter;" in header and "uint32_t peak[2];" in header and "uint64_t sq_hi[2];" in header and "uint64_t sq_lo[2];" in header


@pytest.mark.parametrize("x", [-2 ** 31, 2 ** 31 - 1, -2 ** 23, -128, 0, 1, -1, -32768, 32767])
def test_the_magnitude_and_the_split_of_the_extremes(sm, x):
    assert sm.sm_magnitude(x) == abs(x)                                    # |-2^31| is 2^31: never taken in int32
    for wide in (0, 1):
        hi, lo = C.c_uint64(), C.c_uint64()
        sm.sm_square(wide, abs(x), C.byref(hi), C.byref(lo))
        assert (hi.value << 32) + lo.value == x * x
        assert (hi.value, lo.value) == ((x * x >> 32, x * x & 0xFFFFFFFF) if wide else (0, x * x))


def test_the_largest_square_is_two_to_the_62(sm):
    hi, lo = C.c_uint64(), C.c_uint64()
    sm.sm_square(1, sm.sm_magnitude(-2 ** 31), C.byref(hi), C.byref(lo))
    assert (hi.value, lo.value) == (2 ** 30, 0) and (hi.value << 32) + lo.value == 2 ** 62


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_random_lanes_and_every_cut(sm, width, nch):
    rng = random.Random(10 * width + nch)
    n, top = lane_samples(width), 2 ** (8 * width - 1)
    extremes = [v for v in (-2 ** 31, 2 ** 31 - 1, -2 ** 23, -128, -top, top - 1) if -top <= v < top]
    for k in range(60):
        x = [rng.choice(extremes) if rng.random() < 0.3 else rng.randrange(-top, top) for _ in range(n)]
        s0 = rng.randrange(0, 1 << 20) * n
        for a in range(n + 1):
            for b in range(a, n + 1):                                       # empty, single-sample and whole cuts among them
                assert value(lane(sm, width, x, s0, s0 + a, s0 + b, nch)) == want(x, s0, s0 + a, s0 + b, nch), (x, a, b)
        assert value(lane(sm, width, x, s0, 0, 2 ** 32 - 65536, nch)) == want(x, s0, 0, 2 ** 32, nch)       # a lane wholly inside
        assert value(lane(sm, width, x, s0, s0 + n, s0 + n + 5, nch)) == ((0, 0), (0, 0))                # and one wholly outside
    if nch == 1:
        assert value(lane(sm, width, [top - 1] * n, 0, 0, n, 1))[0][1] == 0                               # a mono song's second channel reads 0


def test_a_narrow_width_keeps_one_sum(sm):
    for width in (1, 2):
        r = lane(sm, width, [-(2 ** (8 * width - 1))] * lane_samples(width), 0, 0, 8, 2)
        assert (r.sq_hi[0], r.sq_hi[1]) == (0, 0) and r.sq_lo[0] == r.sq_lo[1] == (lane_samples(width) // 2) * 4 ** (8 * width - 1)


def test_a_lane_of_full_scale_at_width_four(sm):
    r = lane(sm, 4, [-2 ** 31] * 4, 8, 8, 12, 1)
    assert value(r) == ((2 ** 31, 0), (4 * 2 ** 62, 0)) and (r.sq_hi[0], r.sq_lo[0]) == (4 * 2 ** 30, 0)
    r = lane(sm, 4, [-2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1], 8, 8, 12, 2)
    assert value(r) == ((2 ** 31, 2 ** 31 - 1), (2 * 2 ** 62, 2 * (2 ** 31 - 1) ** 2))


@pytest.mark.parametrize("k", [1, 2, 3, 6, 10])
def test_two_to_the_k_partial_rows_fold_to_one_row_in_any_order(sm, k):
    rng = random.Random(k)
    rows, total_peak, total_sq = [], [0, 0], [0, 0]
    for i in range(2 ** k):
        x = [rng.choice([-2 ** 31, 2 ** 31 - 1, rng.randrange(-2 ** 31, 2 ** 31)]) for _ in range(4)]
        rows.append(lane(sm, 4, x, 4 * i, 0, 2 ** 31, 2))
        (p, s) = want(x, 4 * i, 0, 2 ** 31, 2)
        total_peak = [max(total_peak[c], p[c]) for c in (0, 1)]
        total_sq = [total_sq[c] + s[c] for c in (0, 1)]
    if k >= 3:
        assert max(total_sq) >= 2 ** 64                                     # past one 64-bit sum: the two sums carry it
    orders = [list(range(2 ** k)), list(range(2 ** k))[::-1], rng.sample(range(2 ** k), 2 ** k)]
    got = []
    for order in orders:
        acc = Row()
        for i in order:
            sm.sm_fold(C.byref(acc), C.byref(rows[i]))
        got.append(((acc.peak[0], acc.peak[1]), (acc.sq_hi[0], acc.sq_hi[1]), (acc.sq_lo[0], acc.sq_lo[1])))
        assert value(acc) == (tuple(total_peak), tuple(total_sq))
    tree = [Row.from_buffer_copy(bytes(r)) for r in rows]                   # the butterfly of a wave reduction
    m = 1
    while m < 2 ** k:
        for i in range(0, 2 ** k - m, 2 * m):
            sm.sm_fold(C.byref(tree[i]), C.byref(tree[i + m]))
        m *= 2
    got.append(((tree[0].peak[0], tree[0].peak[1]), (tree[0].sq_hi[0], tree[0].sq_hi[1]), (tree[0].sq_lo[0], tree[0].sq_lo[1])))
    assert all(g == got[0] for g in got)                                    # field by field, not only the value


def test_the_program_of_its_own(tmp_path):
    """cpu_seqmeter.cpp with its own main: the form a sanitizer build runs (here built plainly)"""
    exe = tmp_path / "seqmeter"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-DSEQMETER_MAIN", str(ROOT / "tests" / "cpu_seqmeter.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert out.startswith("seqmeter: ") and out.rstrip().endswith("ok")
