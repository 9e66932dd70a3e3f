"""csrc/pcmfir.hpp -- the contract of sh_pcm_convolve: the constants and their mirrors in the binding, the result's length, the one
rounding at the rails, every refusal of check in its order, and the whole call as a host loop divided as the kernel divides it --
built for the host with g++, against ``numpy.convolve`` on int64 and audioop's fbound written out (tests/firref.py), at widths 1 and 2,
mono, stereo under a mono response and stereo under a stereo one; windows; the same bytes from the tiles taken backwards; the three
ties to the live ``audioop``.  tests/cpu_pcmfir.cpp also builds as a program of its own (-DPCMFIR_MAIN), which is built and run once
here without a sanitizer.  No GPU."""
import audioop
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from synthesizer_amd import _native as N
from tests import firref

ROOT = Path(__file__).resolve().parents[1]
REFUSALS = ("OK", "BAD_WIDTH", "BAD_CHANNELS", "BAD_IR_CHANNELS", "NO_TAPS", "TOO_MANY_TAPS", "BAD_FACTOR", "BAD_WINDOW", "IN_RANGE", "IR_RANGE",
            "OUT_RANGE", "OVERLAP")


@pytest.fixture(scope="module")
def pf(tmp_path_factory):
    out = tmp_path_factory.mktemp("pcmfir") / "libpcmfir.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", str(ROOT / "tests" / "cpu_pcmfir.cpp"), "-o", str(out)],
                   check=True)
    lib = C.CDLL(str(out))
    u64, u32, i64 = C.c_uint64, C.c_uint32, C.c_int64
    lib.pf_constants.restype, lib.pf_constants.argtypes = None, [C.POINTER(u32)]
    lib.pf_result_frames.restype, lib.pf_result_frames.argtypes = u64, [u64, u64]
    lib.pf_scale.restype, lib.pf_scale.argtypes = C.c_int32, [i64, C.c_double, C.c_int]
    lib.pf_padded_taps.restype, lib.pf_padded_taps.argtypes = u32, [u32]
    lib.pf_check.restype, lib.pf_check.argtypes = C.c_int, [C.c_int, C.c_int, C.c_int, u64, u64, C.c_double, u64, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    lib.pf_host_convolve.restype = None
    lib.pf_host_convolve.argtypes = [C.c_char_p, C.c_char_p, C.c_int, u64, u32, C.c_int, C.c_int, C.c_double, u64, u64, C.c_char_p, C.c_int]
    return lib


def host(pf, x, h, factor, width, first=0, count=None, backwards=False):
    """frames [first, first + count) of x (n, nch) under h (m, hch) by the header's host loop, as int64 (count, nch)"""
    n, nch = x.shape
    total = n + len(h) - 1 if n else 0
    count = total - first if count is None else count
    out = C.create_string_buffer(max(1, count * nch * width))
    pf.pf_host_convolve(firref.pcm(x, width), firref.pcm(h, width), width, n, len(h), nch, h.shape[1], factor, first, count, out, int(backwards))
    return np.frombuffer(out.raw[:count * nch * width], dtype=firref.DTYPES[width]).astype(np.int64).reshape(count, nch)


def test_the_constants_are_the_bindings_and_the_bound_holds(pf):
    got = (C.c_uint32 * 5)()
    pf.pf_constants(got)
    max_taps, tile, chunk, lane, unroll = list(got)
    assert (max_taps, tile, chunk) == (N.PCM_FIR_MAX_TAPS, N.PCM_FIR_TILE_FRAMES, N.PCM_FIR_TAP_CHUNK) == (2 ** 22, 2048, 1024)
    assert tile == 256 * lane and chunk % unroll == 0
    assert max_taps * 2 ** 30 == 2 ** 52 < 2 ** 53                 # |acc| <= m * 2^30: every partial sum is a float64
    assert float(2 ** 52) + 1.0 != float(2 ** 52) and float(-2 ** 52) - 1.0 != float(-2 ** 52)
    assert [pf.pf_padded_taps(m) for m in (1, 7, 8, 9, 2 ** 22)] == [8, 8, 8, 16, 2 ** 22]


def test_the_results_length(pf):
    assert [pf.pf_result_frames(n, m) for n, m in ((0, 5), (1, 1), (1, 5), (7, 1), (100, 30), (2 ** 40, 2 ** 22))] == [0, 1, 5, 7, 129, 2 ** 40 + 2 ** 22 - 1]


@pytest.mark.parametrize("width", [1, 2])
def test_scale_is_fbound_at_the_rails_and_for_both_signs_of_zero(pf, width):
    lo, hi = firref.lo_hi(width)
    span = hi - lo + 1                                          # 2^(8 width)
    # p in (HI, HI + 1): 2 HI + 1 halves; p in (LO - 1, LO + 1): LO -+ a half; then the exact rails and their inner neighbours
    assert pf.pf_scale(2 * hi + 1, 0.5, width) == hi and pf.pf_scale(2 * hi + 2, 0.5, width) == hi and pf.pf_scale(span * span, 1.0, width) == hi
    assert pf.pf_scale(2 * lo - 1, 0.5, width) == lo and pf.pf_scale(2 * lo + 1, 0.5, width) == lo and pf.pf_scale(-span * span, 1.0, width) == lo
    assert pf.pf_scale(hi, 1.0, width) == hi and pf.pf_scale(lo, 1.0, width) == lo and pf.pf_scale(lo + 1, 1.0, width) == lo + 1
    assert pf.pf_scale(2 * hi - 1, 0.5, width) == hi - 1 and pf.pf_scale(2 * lo + 3, 0.5, width) == lo + 1      # floor, not truncation
    assert pf.pf_scale(0, 1.0, width) == 0 and pf.pf_scale(0, -1.0, width) == 0                                 # +0.0 and -0.0
    assert pf.pf_scale(-1, 0.5, width) == -1 and pf.pf_scale(1, 0.5, width) == 0 and pf.pf_scale(1, -0.5, width) == -1
    for acc, f in ((2 * hi + 1, 0.5), (2 * lo - 1, 0.5), (2 * lo + 1, 0.5), (-3, 0.5), (12345, 1.0 / 7.0), (-12345, 1.0 / 7.0), (0, -1.0)):
        assert pf.pf_scale(acc, f, width) == int(firref.fbound(float(acc) * f, width))
        dt = firref.DTYPES[width]                               # audioop.mul is this rounding of ONE sample
        if lo <= acc <= hi:
            assert pf.pf_scale(acc, f, width) == int(np.frombuffer(audioop.mul(np.array([acc], dtype=dt).tobytes(), width, f), dtype=dt)[0])


def test_every_refusal_in_its_order(pf):
    def check(width=2, nch=2, ir_nch=1, n=100, m=10, factor=0.5, first=0, count=109, a=(0x1000, 400, 0), h=(0x2000, 20, 0), o=(0x3000, 436, 0)):
        op = lambda t: (C.c_uint64 * 3)(*t)
        return REFUSALS[pf.pf_check(width, nch, ir_nch, n, m, factor, first, count, op(a), op(h), op(o))]
    assert check() == "OK"
    assert check(width=3) == check(width=4) == check(width=0) == "BAD_WIDTH" and check(width=1, a=(0x1000, 200, 0), h=(0x2000, 10, 0), o=(0x3000, 218, 0)) == "OK"
    assert check(nch=0) == check(nch=3) == "BAD_CHANNELS"
    assert check(nch=1, ir_nch=2) == check(ir_nch=0) == check(ir_nch=3) == "BAD_IR_CHANNELS"
    assert check(ir_nch=2, h=(0x2000, 40, 0)) == "OK" and check(nch=1, a=(0x1000, 200, 0), o=(0x3000, 218, 0)) == "OK"
    assert check(m=0) == "NO_TAPS"
    assert check(m=2 ** 22 + 1) == "TOO_MANY_TAPS"
    assert check(factor=float("inf")) == check(factor=float("-inf")) == check(factor=float("nan")) == "BAD_FACTOR"
    assert check(factor=0.0) == check(factor=-1e300) == "OK"
    assert check(count=110) == check(first=1) == check(first=110, count=0) == check(first=2 ** 64 - 1, count=2) == "BAD_WINDOW"
    assert check(n=0, count=1) == "BAD_WINDOW" and check(n=0, count=0, a=(0x1000, 0, 0)) == "OK"
    assert check(first=109, count=0) == "OK" and check(first=108, count=1) == "OK"
    assert check(a=(0x1000, 399, 0)) == check(a=(0x1000, 404, 6)) == check(a=(0x1000, 400, 401)) == "IN_RANGE"
    assert check(a=(0x1000, 404, 4)) == check(a=(0x1000, 500, 3)) == "OK"            # (any byte: no alignment is asked for)
    assert check(h=(0x2000, 19, 0)) == check(h=(0x2000, 30, 12)) == check(h=(0x2000, 20, 1)) == "IR_RANGE"
    assert check(o=(0x3000, 435, 0)) == check(o=(0x3000, 440, 6)) == check(o=(0x3000, 436, 1)) == "OUT_RANGE"
    assert check(o=(0x3000, 440, 4)) == check(o=(0x3000, 440, 3)) == "OK"
    assert check(o=(0x1000 + 398, 436, 0)) == check(o=(0x1000 - 434, 436, 0)) == check(o=(0x1000, 400, 0), count=100) == "OVERLAP"
    assert check(o=(0x2000 + 18, 436, 0)) == check(o=(0x2000 - 434, 436, 0)) == "OVERLAP"
    assert check(o=(0x1000 + 400, 436, 0)) == check(o=(0x1000 - 436, 436, 0)) == "OK"              # side by side is no overlap
    assert check(o=(0x1000, 400, 0), first=5, count=0) == "OK"                                     # an empty window writes nothing
    assert check(a=(0x1000, 400, 0), h=(0x1000, 20, 0)) == "OK"                                    # the inputs may share their bytes
    # the order: each refusal hides the ones behind it
    bad = dict(width=3, nch=3, ir_nch=3, m=0, factor=float("nan"), count=10 ** 6, a=(0x1000, 1, 0), h=(0x2000, 1, 0), o=(0x1000, 1, 0))
    order = ["width", "nch", "ir_nch", "m", "factor", "count", "a", "h", "o"]
    want = ["BAD_WIDTH", "BAD_CHANNELS", "BAD_IR_CHANNELS", "NO_TAPS", "BAD_FACTOR", "BAD_WINDOW", "IN_RANGE", "IR_RANGE", "OUT_RANGE"]
    for k, name in enumerate(order):
        assert check(**{key: bad[key] for key in order[k:]}) == want[k], name
    assert check(m=2 ** 22 + 1, factor=float("nan")) == "TOO_MANY_TAPS"


CASES = [(1, 1), (2, 1), (2, 2)]                                # (channels, channels of the response)


@pytest.mark.parametrize("width", [1, 2])
@pytest.mark.parametrize("nch,hch", CASES)
def test_the_host_loop_equals_numpy_convolve_and_fbound_forwards_and_backwards(pf, width, nch, hch):
    rng = np.random.default_rng(100 * width + 10 * nch + hch)
    T, K = N.PCM_FIR_TILE_FRAMES, N.PCM_FIR_TAP_CHUNK
    shapes = [(1, 1), (1, 9), (2, 2), (17, 3), (300, 40), (40, 300), (T - 1, 7), (T + 1, 8), (9, K + 1), (2 * T + 3, K - 1), (700, 2 * K + 5), (4000, 700)]
    for n, m in shapes:
        x, h = firref.rand_frames(rng, width, n, nch), firref.rand_frames(rng, width, m, hch)
        for factor in (1.0 / (1 << (8 * width - 1)), 1.0 / (1 << (8 * width + 2)), 1.0):
            want = firref.convolve(x, h, factor, width)
            assert want.shape == (n + m - 1, nch)
            assert np.array_equal(host(pf, x, h, factor, width), want), (n, m, factor)
            assert np.array_equal(host(pf, x, h, factor, width, backwards=True), want), (n, m, factor)
    lo, hi = firref.lo_hi(width)
    assert want.min() == lo and want.max() == hi                   # (the last shape at factor 1.0 reaches both rails)
    assert host(pf, np.zeros((0, nch), dtype=np.int64), firref.rand_frames(rng, width, 5, hch), 1.0, width).shape == (0, nch)


def test_the_host_loop_and_the_numpy_reference_are_both_held_against_python_integers(pf):
    rng = np.random.default_rng(5)
    x, h = firref.rand_frames(rng, 2, 600, 1), firref.rand_frames(rng, 2, 90, 1)
    xs, hs = [int(v) for v in x[:, 0]], [int(v) for v in h[:, 0]]
    want = [sum(hs[k] * xs[i - k] for k in range(len(hs)) if 0 <= i - k < len(xs)) for i in range(len(xs) + len(hs) - 1)]
    assert firref.sums(x, h)[:, 0].tolist() == want
    # 90 products of at most 2^30 stay below 2^37: at 2^-22 nothing clips, and the floor of an integer over a power of two is a shift
    assert max(abs(v) for v in want) < 2 ** 37
    assert host(pf, x, h, 2.0 ** -22, 2)[:, 0].tolist() == [v >> 22 for v in want]


@pytest.mark.parametrize("width", [1, 2])
def test_a_window_is_that_slice_of_the_whole_result(pf, width):
    rng = np.random.default_rng(7 + width)
    T = N.PCM_FIR_TILE_FRAMES
    x, h = firref.rand_frames(rng, width, T + 300, 2), firref.rand_frames(rng, width, 77, 2)
    factor = 1.0 / (1 << (8 * width + 1))
    whole = firref.convolve(x, h, factor, width)
    for first, count in ((0, 1), (0, T), (5, T), (T - 1, 2), (T + 299, 77), (len(whole) - 1, 1), (1000, 0), (len(whole), 0), (3, len(whole) - 3)):
        assert np.array_equal(host(pf, x, h, factor, width, first, count), whole[first:first + count]), (first, count)
        assert np.array_equal(host(pf, x, h, factor, width, first, count, backwards=True), whole[first:first + count]), (first, count)


@pytest.mark.parametrize("width", [1, 2])
def test_the_three_ties_to_audioop(pf, width):
    """one tap is audioop.mul; a 1 at tap k is k frames of silence in front; two taps of 1 are audioop.add with the delayed copy"""
    rng = np.random.default_rng(20 + width)
    dt = firref.DTYPES[width]
    x = firref.rand_frames(rng, width, 500, 1)
    raw = firref.pcm(x, width)
    for f in (1.0, 0.5, -0.75, 1.9, -2.0, 1.0 / 3.0):
        want = np.frombuffer(audioop.mul(raw, width, f), dtype=dt).astype(np.int64)
        assert np.array_equal(host(pf, x, np.array([[1]], dtype=np.int64), f, width)[:, 0], want), f
    for k in (1, 7, 64):
        h = np.zeros((k + 1, 1), dtype=np.int64)
        h[k] = 1
        assert host(pf, x, h, 1.0, width)[:, 0].astype(dt).tobytes() == bytes(k * width) + raw
        h[0] = 1
        delayed, padded = bytes(k * width) + raw, raw + bytes(k * width)
        assert host(pf, x, h, 1.0, width)[:, 0].astype(dt).tobytes() == audioop.add(padded, delayed, width)


def test_the_file_is_a_program_of_its_own_as_well(tmp_path):
    exe = tmp_path / "cpu_pcmfir"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-DPCMFIR_MAIN", str(ROOT / "tests" / "cpu_pcmfir.cpp"), "-o", str(exe)],
                   check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("pcmfir: ") and p.stdout.strip().endswith("ok"), p.stdout + p.stderr
