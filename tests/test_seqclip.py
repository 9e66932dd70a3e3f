"""csrc/seqclip.hpp -- what an OVER of a compiled song's level history is: the predicate of a saturating add that clamps, the predicate of
a multiply that clamps (floor(p) outside the range), the 16-bit form the kernels evaluate on packed samples, a lane's count cut to the
window, the fold and the row -- built for the host with g++, against Python integers.  tests/cpu_seqclip.cpp also builds as a program of
its own (-DSEQCLIP_MAIN), which is built and run once here without a sanitizer.  No GPU."""
import ctypes as C
import math
import random
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HI = {1: 127, 2: 32767, 3: 8388607, 4: 2147483647}
LO = {w: -HI[w] - 1 for w in HI}


class Row(C.Structure):
    _fields_ = [("peak", C.c_uint32 * 2), ("sq_hi", C.c_uint64 * 2), ("sq_lo", C.c_uint64 * 2), ("clipped", C.c_uint32 * 2)]


@pytest.fixture(scope="module")
def sc(tmp_path_factory):
    out = tmp_path_factory.mktemp("seqclip") / "libseqclip.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", str(ROOT / "tests" / "cpu_seqclip.cpp"), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.sc_add_clamps.argtypes = [C.c_int, C.c_longlong, C.c_longlong]
    lib.sc_mul_clamps.argtypes = [C.c_int, C.c_double]
    for f in (lib.sc_add_clamps16, lib.sc_sat16, lib.sc_wrap16):
        f.argtypes = [C.c_int, C.c_int]
    lib.sc_disagree16.argtypes = [C.c_int, C.c_int]
    lib.sc_disagree16.restype = C.c_uint64
    lib.sc_lane8.argtypes = [C.POINTER(C.c_short), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.sc_lane4.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.sc_fold_counts.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.sc_fold_rows.argtypes = [C.POINTER(Row), C.POINTER(Row)]
    lib.sc_row_size.restype = lib.sc_clipped_offset.restype = C.c_uint32
    for f in (lib.sc_lane8, lib.sc_lane4, lib.sc_fold_counts, lib.sc_fold_rows):
        f.restype = None
    return lib


def test_the_add_at_width_1_over_every_pair_of_saturated_values(sc):
    for a in range(-128, 128):
        for x in range(-128, 128):
            assert bool(sc.sc_add_clamps(1, a, x)) == (a + x > 127 or a + x < -128), (a, x)


@pytest.mark.parametrize("width", [2, 3, 4])
def test_the_add_at_the_rails(sc, width):
    hi, lo = HI[width], LO[width]
    near = [lo, lo + 1, lo + 2, -2, -1, 0, 1, 2, hi - 2, hi - 1, hi]
    for a in near:
        for x in near:
            assert bool(sc.sc_add_clamps(width, a, x)) == (a + x > hi or a + x < lo), (a, x)
    assert not sc.sc_add_clamps(width, hi, 0) and sc.sc_add_clamps(width, hi, 1) and not sc.sc_add_clamps(width, hi - 1, 1)
    assert not sc.sc_add_clamps(width, lo, 0) and sc.sc_add_clamps(width, lo, -1) and not sc.sc_add_clamps(width, lo + 1, -1)
    assert sc.sc_add_clamps(width, hi, hi) and sc.sc_add_clamps(width, lo, lo) and not sc.sc_add_clamps(width, hi, lo)


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_the_multiply_around_the_rails(sc, width):
    hi, lo = float(HI[width]), float(LO[width])
    for p, want in ((hi, False), (hi + 0.25, False), (hi + 0.5, False), (math.nextafter(hi + 1.0, 0.0), False),      # (HI, HI + 1) floors to HI
                    (hi + 1.0, True), (hi + 1.5, True), (2 * hi, True), (hi - 0.5, False), (0.0, False), (-0.5, False),
                    (lo, False), (lo + 0.5, False), (math.nextafter(lo, -math.inf), True), (lo - 0.25, True), (lo - 1.0, True), (lo - 1.5, True),
                    (2 * lo, True)):
        assert bool(sc.sc_mul_clamps(width, p)) == want == (math.floor(p) > hi or math.floor(p) < lo), (width, p)
    # as products of a sample and a factor: HI * 1.00001 and friends
    rng = random.Random(11)
    for _ in range(2000):
        x = rng.choice([HI[width], LO[width], rng.randrange(LO[width], HI[width] + 1)])
        f = rng.choice([1.5, -1.0, 0.999, 1.0 + 2.0 ** -20, 2.0, -2.0, 0.5, 1.0 / 3.0])
        p = float(x) * f
        assert bool(sc.sc_mul_clamps(width, p)) == (math.floor(p) > HI[width] or math.floor(p) < LO[width]), (x, f)


def test_the_16_bit_form_is_the_exact_sum_out_of_range(sc):
    """saturating sum != wrapping sum iff the exact sum is out of range: every a against x on a stride of 61 from the lower rail on
    (1075 values) and against the 64 values at each rail"""
    assert sc.sc_disagree16(-32768, 61) == 0
    for x in list(range(-32768, -32768 + 64)) + list(range(32767 - 63, 32768)):
        assert sc.sc_disagree16(x, 1 << 20) == 0
    for a, x in ((32767, 1), (32767, 32767), (-32768, -1), (-32768, -32768), (1, 32767), (-1, -32768)):
        assert sc.sc_add_clamps16(a, x) and sc.sc_sat16(a, x) in (32767, -32768) and sc.sc_wrap16(a, x) == ((a + x + 32768) % 65536) - 32768
    for a, x in ((32767, 0), (32766, 1), (-32768, 0), (-32767, -1), (32767, -32768), (0, 0)):
        assert not sc.sc_add_clamps16(a, x) and sc.sc_sat16(a, x) == sc.sc_wrap16(a, x) == a + x


def test_a_lane_counts_its_flagged_samples_inside_the_window_by_channel(sc):
    rng = random.Random(5)
    out = (C.c_uint32 * 2)()
    for _ in range(3000):
        flags = [rng.choice([0, 0, -1, 1]) for _ in range(8)]
        s0 = 8 * rng.randrange(0, 40)
        lo = rng.randrange(0, 330)
        hi = lo + rng.randrange(0, 30)
        nch = rng.choice([1, 2])
        want8, want4 = [0, 0], [0, 0]
        for j in range(8):
            if lo <= s0 + j < hi and flags[j]:
                want8[j & 1 if nch == 2 else 0] += 1
                if j < 4:
                    want4[j & 1 if nch == 2 else 0] += 1
        sc.sc_lane8((C.c_short * 8)(*flags), s0, lo, hi, nch, out)
        assert list(out) == want8
        sc.sc_lane4(sum((1 if flags[j] else 0) << j for j in range(4)), s0, lo, hi, nch, out)
        assert list(out) == want4
    # the cut: a lane across the window's first sample, across its last, outside it, and a mono song filling channel 0
    all8 = (C.c_short * 8)(*[-1] * 8)
    for s0, lo, hi, nch, want in ((8, 11, 100, 2, [2, 3]), (8, 0, 13, 2, [3, 2]), (8, 16, 40, 2, [0, 0]), (8, 0, 8, 2, [0, 0]), (8, 8, 16, 2, [4, 4]),
                                  (8, 8, 16, 1, [8, 0]), (8, 9, 10, 1, [1, 0]), (8, 9, 10, 2, [0, 1])):
        sc.sc_lane8(all8, s0, lo, hi, nch, out)
        assert list(out) == want, (s0, lo, hi, nch)


def test_counts_fold_in_any_order(sc):
    rng = random.Random(3)
    parts = [[rng.randrange(0, 2049), rng.randrange(0, 2049)] for _ in range(40)]
    totals = []
    for _ in range(5):
        rng.shuffle(parts)
        acc = (C.c_uint32 * 2)(0, 0)
        for p in parts:
            sc.sc_fold_counts(acc, (C.c_uint32 * 2)(*p))
        totals.append(list(acc))
    assert all(t == [sum(p[0] for p in parts), sum(p[1] for p in parts)] for t in totals)
    # rows: the levels fold as the meters' do, the counts add
    a, b = Row(), Row()
    a.peak[:], a.sq_hi[:], a.sq_lo[:], a.clipped[:] = [5, 9], [1, 2], [3, 4], [7, 0]
    b.peak[:], b.sq_hi[:], b.sq_lo[:], b.clipped[:] = [8, 2], [10, 20], [30, 40], [1, 11]
    sc.sc_fold_rows(C.byref(a), C.byref(b))
    assert (list(a.peak), list(a.sq_hi), list(a.sq_lo), list(a.clipped)) == ([8, 9], [11, 22], [33, 44], [8, 11])


def test_a_row_is_48_bytes_the_counts_behind_the_levels(sc):
    assert sc.sc_row_size() == 48 == C.sizeof(Row) and sc.sc_clipped_offset() == 40 == Row.clipped.offset


def test_the_file_is_a_program_of_its_own_as_well(tmp_path):
    exe = tmp_path / "cpu_seqclip"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DSEQCLIP_MAIN", str(ROOT / "tests" / "cpu_seqclip.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("seqclip: ") and p.stdout.strip().endswith("ok"), p.stdout + p.stderr
