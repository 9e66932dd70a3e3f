"""csrc/pcmresample.hpp -- the contract of sh_pcm_resample_fir: the constants and their mirrors in the binding, the result's length
(with n * L near 2^64), every refusal of check in its order, the plan (the tables e and p, the rows' length, every output owned exactly
once, the last short chunk, the padding of the staged span) and the whole call as a host loop divided as the kernel divides it -- built
for the host with g++, against tests/resampleref.py (``numpy.convolve`` over int64 per phase, held by the zero-stuffed form, and
audioop's fbound written out).  tests/cpu_pcmresample.cpp also builds as a program of its own (-DPCMRESAMPLE_MAIN), which is built and
run once here without a sanitizer.  No GPU."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from synthesizer_amd import _native as N
from tests import firref, resampleref

ROOT = Path(__file__).resolve().parents[1]
REFUSALS = ("OK", "BAD_WIDTH", "BAD_CHANNELS", "NO_TAPS", "TOO_MANY_TAPS", "BAD_RATIO", "BAD_UP", "BAD_STRIDE", "BAD_DELAY", "BAD_FACTOR", "BAD_WINDOW",
            "IN_RANGE", "TAPS_RANGE", "OUT_RANGE", "OVERLAP")
RATIOS = [(1, 1), (2, 1), (1, 2), (3, 2), (2, 3), (7, 8), (8, 1), (1, 8), (5, 3), (4, 6), (160, 147), (147, 160), (80, 441)]
PLAN = ("c", "P", "Mp", "chunks", "e_lo", "e_span", "spread", "steps", "pad", "q_waves", "rounds", "blocks", "step_chunk", "staged")


@pytest.fixture(scope="module")
def pr(tmp_path_factory):
    out = tmp_path_factory.mktemp("pcmresample") / "libpcmresample.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", str(ROOT / "tests" / "cpu_pcmresample.cpp"), "-o",
                    str(out)], check=True)
    lib = C.CDLL(str(out))
    u64, u32, i64 = C.c_uint64, C.c_uint32, C.c_int64
    lib.pr_constants.restype, lib.pr_constants.argtypes = None, [C.POINTER(u32)]
    lib.pr_result_frames.restype, lib.pr_result_frames.argtypes = u64, [u64, u32, u32]
    lib.pr_stride_fits.restype, lib.pr_stride_fits.argtypes = C.c_int, [u32, u32]
    lib.pr_bank_ways.restype, lib.pr_bank_ways.argtypes = u32, [u32, u32]
    lib.pr_staged_at.restype, lib.pr_staged_at.argtypes = u32, [u32, u32, u32]
    lib.pr_check.restype = C.c_int
    lib.pr_check.argtypes = [C.c_int, C.c_int, u64, u64, u32, u32, u32, C.c_double, u64, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    lib.pr_plan.restype, lib.pr_plan.argtypes = None, [u32, u32, u32, u32, u32, C.POINTER(u32)]
    lib.pr_tables.restype, lib.pr_tables.argtypes = None, [u32, u32, u32, u32, C.POINTER(u64), C.POINTER(u32), C.POINTER(u64)]
    lib.pr_row_tap.restype, lib.pr_row_tap.argtypes = i64, [u32] * 8
    lib.pr_workgroups.restype, lib.pr_workgroups.argtypes = u64, [u64, u64, u32, u32, u32, u32, u32]
    lib.pr_host_resample.restype = None
    lib.pr_host_resample.argtypes = [C.c_char_p, C.c_char_p, C.c_int, u64, u32, u32, u32, u32, C.c_int, C.c_double, u64, u64, C.c_char_p, C.c_int, C.POINTER(u32)]
    return lib


def plan(pr, m, L, M, delay, nbytes=2):
    got = (C.c_uint32 * 14)()
    pr.pr_plan(m, L, M, delay, nbytes, got)
    return dict(zip(PLAN, list(got)))


def host(pr, x, h, L, M, delay, factor, width, first=0, count=None, backwards=False, owners=False):
    """frames [first, first + count) of x (n, nch) under the taps h by the header's host loop, as int64 (count, nch)"""
    n, nch = x.shape
    total = resampleref.result_frames(n, L, M)
    count = total - first if count is None else count
    out = C.create_string_buffer(max(1, count * nch * width))
    own = (C.c_uint32 * max(1, count * nch))() if owners else None
    pr.pr_host_resample(firref.pcm(x, width), np.asarray(h).astype(np.int16).tobytes(), width, n, len(h), L, M, delay, nch, factor, first, count, out,
                        int(backwards), own)
    got = np.frombuffer(out.raw[:count * nch * width], dtype=firref.DTYPES[width]).astype(np.int64).reshape(count, nch)
    return (got, list(own)[:count * nch]) if owners else got


def test_the_constants_are_the_bindings(pr):
    got = (C.c_uint32 * 8)()
    pr.pr_constants(got)
    assert list(got) == [N.PCM_RESAMPLE_MAX_TAPS, N.PCM_RESAMPLE_MAX_UP, N.PCM_RESAMPLE_LANE_OUTPUTS, N.PCM_RESAMPLE_BLOCK_GROUPS, N.PCM_RESAMPLE_WAVES,
                         N.PCM_RESAMPLE_STEP_CHUNK, N.PCM_RESAMPLE_STEP_UNROLL, N.PCM_RESAMPLE_STAGED_SAMPLES] == [2 ** 22, 4096, 8, 64, 4, 1024, 2, 32768]
    assert N.PCM_RESAMPLE_MAX_TAPS == N.PCM_FIR_MAX_TAPS and N.PCM_RESAMPLE_MAX_TAPS * 2 ** 30 == 2 ** 52       # pcmfir.hpp's bound, term for term
    assert N.PCM_RESAMPLE_STEP_CHUNK % N.PCM_RESAMPLE_STEP_UNROLL == 0
    for L in (1, 2, 3, 7, 8, 9, 160, 4096):
        c = N.pcm_resample_copies(L)
        assert plan(pr, 5, L, 3, 0)["c"] == c and c * L >= 8 and (c == 1 or (c - 1) * L < 8)
    # the ratios a sampler meets fit one step; the strides beyond the staged span do not, in the header and in its mirror alike
    for L, M, fits in ((160, 147, True), (147, 160, True), (320, 147, True), (1, 6, True), (80, 441, True), (1, 8, True), (8, 503, True), (8, 504, False),
                       (1, 63, False), (1, 62, True), (4096, 1, True), (3, 168, False)):
        assert bool(pr.pr_stride_fits(L, M)) == N.pcm_resample_stride_fits(L, M) == fits, (L, M)


def test_the_results_length_with_products_near_two_to_the_64(pr):
    cases = [(0, 5, 3), (1, 1, 1), (1, 5, 1), (1, 1, 5), (7, 3, 2), (100, 160, 147), (44100, 160, 147), (48000, 147, 160), (2 ** 40, 4096, 4095),
             (2 ** 52 - 1, 4095, 4096), (2 ** 52, 4096, 3), (2 ** 63, 3, 3), (2 ** 64 - 1, 1, 1), (2 ** 64 - 1, 4096, 4096), (2 ** 64 - 1, 5, 7),
             (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1), (2 ** 62, 3, 1)]
    for n, L, M in cases:
        assert pr.pr_result_frames(n, L, M) == -(-n * L // M), (n, L, M)
    assert pr.pr_result_frames(2 ** 63, 2, 1) == pr.pr_result_frames(2 ** 64 - 1, 4096, 1) == 2 ** 64 - 1        # no uint64 holds it: saturated
    assert pr.pr_result_frames(5, 0, 3) == pr.pr_result_frames(5, 3, 0) == 0


def test_every_refusal_in_its_order(pr):
    def check(width=2, nch=2, n=147, m=10, up=160, down=147, delay=4, factor=0.5, first=0, count=160, a=(0x1000, 588, 0), h=(0x2000, 20, 0), o=(0x3000, 640, 0)):
        op = lambda t: (C.c_uint64 * 3)(*t)
        return REFUSALS[pr.pr_check(width, nch, n, m, up, down, delay, factor, first, count, op(a), op(h), op(o))]
    assert check() == "OK"
    assert check(width=3) == check(width=4) == check(width=0) == "BAD_WIDTH" and check(width=1, a=(0x1000, 294, 0), o=(0x3000, 320, 0)) == "OK"
    assert check(nch=0) == check(nch=3) == "BAD_CHANNELS" and check(nch=1, a=(0x1000, 294, 0), o=(0x3000, 320, 0)) == "OK"
    assert check(m=0) == "NO_TAPS"
    assert check(m=2 ** 22 + 1) == "TOO_MANY_TAPS" and check(m=2 ** 22, h=(0x10000000, 2 ** 23, 0)) == "OK"
    assert check(up=0) == check(down=0) == check(up=0, down=0) == "BAD_RATIO"
    assert check(up=4097) == "BAD_UP" and check(up=4096) == "OK"
    assert check(up=8, down=504) == check(up=1, down=63) == check(up=4096, down=2 ** 32 - 1) == "BAD_STRIDE"
    assert check(up=8, down=503, count=3) == check(up=1, down=62, count=3) == "OK"
    assert check(delay=10) == check(delay=2 ** 32 - 1) == "BAD_DELAY" and check(delay=9) == check(delay=0) == "OK"
    assert check(factor=float("inf")) == check(factor=float("-inf")) == check(factor=float("nan")) == "BAD_FACTOR"
    assert check(factor=0.0) == check(factor=-1e300) == "OK"
    assert check(count=161) == check(first=1) == check(first=161, count=0) == check(first=2 ** 64 - 1, count=2) == "BAD_WINDOW"
    assert check(n=0, count=1) == "BAD_WINDOW" and check(n=0, count=0, a=(0x1000, 0, 0)) == "OK"
    assert check(first=160, count=0) == "OK" and check(first=159, count=1) == "OK"
    assert check(a=(0x1000, 587, 0)) == check(a=(0x1000, 590, 4)) == check(a=(0x1000, 588, 589)) == "IN_RANGE"
    assert check(a=(0x1000, 592, 4)) == check(a=(0x1000, 600, 3)) == "OK"            # (any byte: no alignment is asked for)
    assert check(h=(0x2000, 19, 0)) == check(h=(0x2000, 30, 12)) == check(h=(0x2000, 20, 1)) == "TAPS_RANGE"
    assert check(width=1, a=(0x1000, 294, 0), o=(0x3000, 320, 0), h=(0x2000, 19, 0)) == "TAPS_RANGE"          # the taps are 16 bits at every width
    assert check(o=(0x3000, 639, 0)) == check(o=(0x3000, 644, 6)) == check(o=(0x3000, 640, 1)) == "OUT_RANGE"
    assert check(o=(0x3000, 644, 4)) == check(o=(0x3000, 644, 3)) == "OK"
    assert check(o=(0x1000 + 586, 640, 0)) == check(o=(0x1000 - 638, 640, 0)) == check(o=(0x1000, 588, 0), count=147) == "OVERLAP"
    assert check(o=(0x2000 + 18, 640, 0)) == check(o=(0x2000 - 638, 640, 0)) == "OVERLAP"
    assert check(o=(0x1000 + 588, 640, 0)) == check(o=(0x1000 - 640, 640, 0)) == "OK"              # side by side is no overlap
    assert check(o=(0x1000, 588, 0), first=5, count=0) == "OK"                                     # an empty window writes nothing
    assert check(a=(0x1000, 588, 0), h=(0x1000, 20, 0)) == "OK"                                    # the inputs may share their bytes
    # the order: each refusal hides the ones behind it
    bad = dict(width=3, nch=3, m=0, up=0, delay=10, factor=float("nan"), count=10 ** 6, a=(0x1000, 1, 0), h=(0x2000, 1, 0), o=(0x1000, 1, 0))
    order = ["width", "nch", "m", "up", "delay", "factor", "count", "a", "h", "o"]
    want = ["BAD_WIDTH", "BAD_CHANNELS", "NO_TAPS", "BAD_RATIO", "BAD_DELAY", "BAD_FACTOR", "BAD_WINDOW", "IN_RANGE", "TAPS_RANGE", "OUT_RANGE"]
    for k, name in enumerate(order):
        assert check(**{key: bad[key] for key in order[k:]}) == want[k], name
    assert check(m=2 ** 22 + 1, up=0) == "TOO_MANY_TAPS" and check(up=4097, down=10 ** 6, delay=10) == "BAD_UP"
    assert check(up=8, down=504, delay=10) == "BAD_STRIDE"


@pytest.mark.parametrize("L,M", RATIOS)
def test_the_plan_its_tables_and_its_rows(pr, L, M):
    R = N.PCM_RESAMPLE_LANE_OUTPUTS
    for m in sorted({1, 2, max(L - 1, 1), L, L + 1, 8 * L + 3}):
        for delay in sorted({0, (m - 1) // 2, m - 1}):
            pl = plan(pr, m, L, M, delay)
            c, P = pl["c"], pl["P"]
            assert (c, P, pl["Mp"], pl["chunks"]) == (N.pcm_resample_copies(L), c * L, c * M, -(-P // R))
            e, p, E = (C.c_uint64 * P)(), (C.c_uint32 * P)(), (C.c_uint64 * pl["chunks"])()
            pr.pr_tables(L, M, delay, P, e, p, E)
            assert list(e) == [(rho * M + delay) // L for rho in range(P)] and list(p) == [(rho * M + delay) % L for rho in range(P)]
            assert list(E) == [max(e[q * R:q * R + R]) for q in range(pl["chunks"])]
            # b = g M' + e[rho] and p = p[rho] for every output of some groups: the tables do not depend on g
            for g in (0, 1, 5, 1000):
                for rho in range(P):
                    j = P * g + rho
                    assert ((j * M + delay) // L, (j * M + delay) % L) == (g * pl["Mp"] + e[rho], p[rho])
            spread = max(E[q] - min(e[q * R:q * R + R]) for q in range(pl["chunks"]))
            assert (pl["e_lo"], pl["e_span"], pl["spread"]) == (e[0], e[P - 1] - e[0], spread) and spread <= -(-R * M // L) + 1
            need = -(-m // L) + spread
            assert pl["steps"] % N.PCM_RESAMPLE_STEP_UNROLL == 0 and need <= pl["steps"] < need + N.PCM_RESAMPLE_STEP_UNROLL
            # the rows: every tap of a residue's phase exactly once, at the step its offset puts it, in rising order; the residues of
            # the last short chunk past P have no taps at all
            for q in sorted({0, pl["chunks"] // 2, pl["chunks"] - 1}):
                for r in range(R):
                    rho = q * R + r
                    taps = [pr.pr_row_tap(q, rho, t, P, L, M, delay, m) for t in range(pl["steps"])]
                    if rho >= P:
                        assert set(taps) == {-1}
                        continue
                    d = E[q] - e[rho]
                    assert [k for k in taps if k >= 0] == list(range(p[rho], m, L)) and all(k == -1 for k in taps[:d])
                    assert all(taps[t] == p[rho] + (t - d) * L for t in range(d, pl["steps"]) if taps[t] >= 0)
            assert pr.pr_row_tap(0, 0, pl["steps"], P, L, M, delay, m) == -1
            # the waves: min(chunks, 4) share out the chunks; with fewer than four chunks the others take further blocks
            assert pl["q_waves"] == min(pl["chunks"], 4) and pl["rounds"] == -(-pl["chunks"] // pl["q_waves"])
            assert 1 <= pl["blocks"] <= 4 // pl["q_waves"] and (pl["chunks"] < 4 or pl["blocks"] == 1)
            assert pl["step_chunk"] == min(pl["steps"], N.PCM_RESAMPLE_STEP_CHUNK)                 # (every ratio of the list fits whole chunks)
            groups = pl["blocks"] * N.PCM_RESAMPLE_BLOCK_GROUPS
            last = (groups - 1) * pl["Mp"] + pl["e_span"] + pl["step_chunk"] - 1
            assert pl["staged"] == pr.pr_staged_at(last, pl["Mp"], pl["pad"]) + 1 <= N.PCM_RESAMPLE_STAGED_SAMPLES


def test_the_last_short_chunk_and_the_blocks_of_a_small_up(pr):
    assert [plan(pr, 9, L, 1, 0)[k] for L in (1, 2, 3, 7, 8, 9, 24, 25, 160) for k in ("P", "chunks", "q_waves", "blocks")] == [
        8, 1, 1, 4, 8, 1, 1, 4, 9, 2, 2, 2, 14, 2, 2, 2, 8, 1, 1, 4, 9, 2, 2, 2, 24, 3, 3, 1, 25, 4, 4, 1, 160, 20, 4, 1]
    # a long stride leaves a small up fewer blocks than waves, and a stride at the limit fewer steps than STEP_CHUNK
    assert plan(pr, 9, 8, 100, 0)["blocks"] == 4 and plan(pr, 9, 8, 200, 0)["blocks"] == 2 and plan(pr, 9, 8, 400, 0)["blocks"] == 1
    pl = plan(pr, 2 ** 20, 8, 503, 0)
    assert pl["steps"] > 1024 and pl["step_chunk"] < 1024 and pl["step_chunk"] % N.PCM_RESAMPLE_STEP_UNROLL == 0 and pl["staged"] <= 32768
    assert plan(pr, 2 ** 20, 8, 503, 0)["step_chunk"] >= 256                                     # (room for some hundred steps at the least)


def test_the_staged_span_is_padded_where_the_stride_meets_few_banks(pr):
    """ARITHMETIC on the bank formula (byte address / 4) mod 32 over lanes 0 .. 31, not a counter reading"""
    assert pr.pr_bank_ways(160, 2) == 16 and pr.pr_bank_ways(160, 4) == 32 and pr.pr_bank_ways(64, 2) == 32 and pr.pr_bank_ways(147, 4) == 1
    assert pr.pr_bank_ways(147, 2) <= 2 and pr.pr_bank_ways(2, 2) == 1 and pr.pr_bank_ways(1, 1) == 1
    for Mp, nbytes in ((160, 2), (147, 2), (48, 2), (441, 2), (8, 2), (64, 2), (160, 4), (160, 1), (6, 2), (320, 2)):
        pl = plan(pr, 100, 8, Mp, 0, nbytes)
        assert pl["Mp"] == Mp and pr.pr_bank_ways(Mp + pl["pad"], nbytes) <= 2 and pl["pad"] < 4, (Mp, nbytes)
        if pr.pr_bank_ways(Mp, nbytes) == 1:
            assert pl["pad"] == 0
    # rows of M' frames with pad unused ones behind each: lane l at o frames into its own reads l (M' + pad) + o + (o / M') pad
    for Mp, pad in ((160, 2), (6, 1), (147, 0)):
        for l in (0, 1, 63):
            for o in (0, 1, Mp - 1, Mp, 3 * Mp + 5):
                assert pr.pr_staged_at(l * Mp + o, Mp, pad) == l * (Mp + pad) + o + o // Mp * pad
    assert len({pr.pr_staged_at(j, 6, 1) for j in range(1000)}) == 1000


def test_both_forms_of_the_reference_agree_and_are_held_against_python_integers():
    rng = np.random.default_rng(11)
    for L, M in RATIOS[:10] + [(16, 7)]:
        for m in (1, L + 1, 4 * L + 3):
            x, h = firref.rand_frames(rng, 2, 90, 2), resampleref.rand_taps(rng, m)
            for delay in sorted({0, (m - 1) // 2, m - 1}):
                a, b = resampleref.sums(x, h, L, M, delay), resampleref.sums_stuffed(x, h, L, M, delay)
                assert a.shape == (-(-90 * L // M), 2) and np.array_equal(a, b), (L, M, m, delay)
    L, M, delay = 5, 3, 4
    x, h = firref.rand_frames(rng, 2, 40, 1), resampleref.rand_taps(rng, 23)
    u = [0] * (40 * L)
    u[::L] = [int(v) for v in x[:, 0]]
    want = [sum(int(h[k]) * u[j * M + delay - k] for k in range(23) if 0 <= j * M + delay - k < len(u)) for j in range(-(-40 * L // M))]
    assert resampleref.sums(x, h, L, M, delay)[:, 0].tolist() == want


@pytest.mark.parametrize("width,nch", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_the_host_loop_equals_the_reference(pr, width, nch):
    """every ratio, tap count, delay and length of the grid; the small cases against the zero-stuffed form as well"""
    rng = np.random.default_rng(100 * width + nch)
    factors = (2.0 ** -14, 2.0 ** -(8 * width + 10), 1.0)
    k, seen = 0, set()
    for L, M in RATIOS:
        c = N.pcm_resample_copies(L)
        xs = {g: firref.rand_frames(rng, width, g * c * M, nch) for g in (1, 2, 63, 64, 65)}          # g groups' worth of input
        for m in sorted({1, 2, max(L - 1, 1), L, L + 1, 8 * L + 3}):
            h = resampleref.rand_taps(rng, m)
            for delay in sorted({0, (m - 1) // 2, m - 1}):
                for g, x in xs.items():
                    factor = factors[k % 3]
                    k += 1
                    want = resampleref.resample(x, h, L, M, delay, factor, width)
                    assert want.shape == (g * c * L, nch)
                    seen |= {int(want.min()), int(want.max())}
                    got, owners = host(pr, x, h, L, M, delay, factor, width, owners=True)
                    assert np.array_equal(got, want), (L, M, m, delay, g)
                    assert set(owners) == {1}, (L, M, m, delay, g)                                  # every output owned exactly once
                    if g <= 2:
                        assert np.array_equal(want, resampleref.resample(x, h, L, M, delay, factor, width, stuffed=True))
                        assert np.array_equal(host(pr, x, h, L, M, delay, factor, width, backwards=True), want)
    lo, hi = firref.lo_hi(width)
    assert lo in seen and hi in seen                               # (the cases at factor 1.0 reach both rails)


@pytest.mark.parametrize("width", [1, 2])
def test_rows_longer_than_a_chunk_of_steps_and_an_input_that_is_no_whole_group(pr, width):
    rng = np.random.default_rng(40 + width)
    K = N.PCM_RESAMPLE_STEP_CHUNK
    for L, M, m, n in ((1, 1, 2 * K + 5, 700), (2, 3, 2 * K + 1, 1000), (3, 2, 3 * K + 7, 333), (160, 147, 160 * K + 9, 401), (7, 8, 50, 1001), (5, 3, 1, 7)):
        x, h = firref.rand_frames(rng, width, n, 2), resampleref.rand_taps(rng, m)
        delay = (m - 1) // 2
        want = resampleref.resample(x, h, L, M, delay, 2.0 ** -17, width)
        assert plan(pr, m, L, M, delay, width)["steps"] > K or m <= 50
        assert np.array_equal(host(pr, x, h, L, M, delay, 2.0 ** -17, width), want), (L, M, m)
        assert np.array_equal(host(pr, x, h, L, M, delay, 2.0 ** -17, width, backwards=True), want), (L, M, m)
    assert host(pr, np.zeros((0, 2), dtype=np.int64), h, 5, 3, 0, 1.0, width).shape == (0, 2)


@pytest.mark.parametrize("width", [1, 2])
def test_a_window_is_that_slice_of_the_whole_result(pr, width):
    rng = np.random.default_rng(7 + width)
    for L, M in ((160, 147), (1, 6), (3, 2)):
        P = N.pcm_resample_copies(L) * L
        per = 64 * P * plan(pr, 77, L, M, 30, width)["blocks"]                                   # the outputs of one workgroup
        n = -(-(per + 300) * M // L)
        x, h = firref.rand_frames(rng, width, n, 2), resampleref.rand_taps(rng, 77)
        whole = resampleref.resample(x, h, L, M, 30, 2.0 ** -15, width)
        for first, count in ((0, 1), (0, per), (5, per), (per - 1, 2), (P + 3, 2 * P), (len(whole) - 1, 1), (1000, 0), (len(whole), 0), (3, len(whole) - 3)):
            got, owners = host(pr, x, h, L, M, 30, 2.0 ** -15, width, first, count, owners=True)
            assert np.array_equal(got, whole[first:first + count]) and set(owners) <= {1}, (L, M, first, count)
            assert np.array_equal(host(pr, x, h, L, M, 30, 2.0 ** -15, width, first, count, backwards=True), whole[first:first + count])


def test_the_file_is_a_program_of_its_own_as_well(tmp_path):
    exe = tmp_path / "cpu_pcmresample"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-DPCMRESAMPLE_MAIN", str(ROOT / "tests" / "cpu_pcmresample.cpp"),
                    "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("pcmresample: ") and p.stdout.strip().endswith("ok"), p.stdout + p.stderr
