"""csrc/pcmlimit.hpp -- the contract of sh_pcm_limit: the constants and their mirrors in the binding; slope, reach and carry_tiles;
the required gain by long division against the operator; every refusal of check in its order; the carries folded from given summaries,
the sums that pass 2^32 included; and the whole call as a host loop divided as the kernels divide it (summaries, carries, tiles) --
built for the host with g++, against the reference of tests/limitref.py, whose numpy form is held to the definition by brute force
first -- at widths 1, 2 and 4, mono and stereo; windows; the same bytes from the tiles taken backwards.  tests/cpu_pcmlimit.cpp also
builds as a program of its own (-DPCMLIMIT_MAIN), which is built and run once here without a sanitizer.  No GPU."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from synthesizer_amd import _native as N
from tests import limitref

ROOT = Path(__file__).resolve().parents[1]
ONE = limitref.ONE
REFUSALS = ("OK", "BAD_WIDTH", "BAD_CHANNELS", "BAD_CEILING", "BAD_ATTACK", "BAD_RELEASE", "BAD_WINDOW", "IN_RANGE", "OUT_RANGE", "GAIN_RANGE", "OUT_OVERLAP",
            "GAIN_OVERLAP", "NO_DESTINATION")


@pytest.fixture(scope="module")
def pl(tmp_path_factory):
    out = tmp_path_factory.mktemp("pcmlimit") / "libpcmlimit.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", str(ROOT / "tests" / "cpu_pcmlimit.cpp"), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    u64, u32, i32 = C.c_uint64, C.c_uint32, C.c_int32
    lib.pl_constants.restype, lib.pl_constants.argtypes = None, [C.POINTER(u32)]
    for name in ("pl_slope", "pl_reach", "pl_carry_tiles"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = u32, [u32]
    lib.pl_hi.restype, lib.pl_hi.argtypes = u32, [C.c_int]
    lib.pl_required_gain.restype, lib.pl_required_gain.argtypes = u32, [u32, u32]
    lib.pl_apply_gain.restype, lib.pl_apply_gain.argtypes = i32, [i32, u32]
    lib.pl_plan.restype, lib.pl_plan.argtypes = None, [u64, u32, u32, u64, u64, C.POINTER(u64)]
    lib.pl_check.restype, lib.pl_check.argtypes = C.c_int, [C.c_int, C.c_int, u64, u64, u64, u64, u64, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    lib.pl_carries.restype, lib.pl_carries.argtypes = None, [u64, u32, u32, u64, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    lib.pl_host_limit.restype = None
    lib.pl_host_limit.argtypes = [C.c_char_p, C.c_int, u64, C.c_int, u32, u32, u32, u64, u64, C.c_char_p, C.POINTER(u32), C.c_int]
    return lib


def host(pl, x, width, ceiling, attack, release, first=0, count=None, backwards=False):
    """frames [first, first + count) of the limited x (n, nch) by the header's host loop: (y int64 (count, nch), G int64 (count,))"""
    n, nch = x.shape
    count = n - first if count is None else count
    out = C.create_string_buffer(max(1, count * nch * width))
    gain = (C.c_uint32 * max(1, count))()
    pl.pl_host_limit(limitref.pcm(x, width), width, n, nch, ceiling, attack, release, first, count, out, gain, int(backwards))
    y = np.frombuffer(out.raw[:count * nch * width], dtype=limitref.DTYPES[width]).astype(np.int64).reshape(count, nch)
    return y, np.array(gain[:count], dtype=np.int64)


def test_the_numpy_reference_is_the_definition_by_brute_force():
    rng = np.random.default_rng(1)
    for k in range(60):
        width, nch = (1, 2, 4)[k % 3], 1 + k % 2
        n = int(rng.integers(1, 65))
        ceiling = int(rng.integers(1, limitref.hi_of(width) + 1))
        attack, release = (int(v) for v in rng.choice([0, 1, 2, 3, 5, 17, 64, 1000], 2))
        x = limitref.noise_with_peaks(rng, width, n, nch, ceiling, peaks=np.flatnonzero(rng.integers(0, 6, n) == 0))
        assert limitref.gain(x, ceiling, attack, release).tolist() == limitref.gain_brute(x, ceiling, attack, release), (k, n, attack, release)
    x = np.array([[-2 ** 31], [5], [2 ** 31 - 1]], dtype=np.int64)          # the rails of width 4: |-2^31| is 2^31
    assert limitref.required_gain(x, 1).tolist() == [0, ONE // 5, ONE // (2 ** 31 - 1)] and limitref.required_gain(x, 2 ** 31 - 1).tolist() == [ONE - 1, ONE, ONE]


def test_the_constants_are_the_bindings(pl):
    got = (C.c_uint32 * 4)()
    pl.pl_constants(got)
    one, max_frames, tile, lane = list(got)
    assert (one, max_frames, tile) == (N.PCM_LIMIT_ONE, N.PCM_LIMIT_MAX_FRAMES, N.PCM_LIMIT_TILE_FRAMES) == (2 ** 30, 2 ** 20, 2048) and tile == 256 * lane
    assert [pl.pl_hi(w) for w in (1, 2, 4)] == [127, 32767, 2 ** 31 - 1] == [limitref.hi_of(w) for w in (1, 2, 4)]
    assert (2 ** 31 - 1) * ONE < 2 ** 61 and 2 ** 31 * ONE <= 2 ** 61            # C * ONE and |x * G|
    assert ONE + 2 ** 21 * ONE < 2 ** 52                                        # a term of G: at most 51 bits and a carry


def test_slope_reach_and_carry_tiles(pl):
    T = N.PCM_LIMIT_TILE_FRAMES
    frames = (0, 1, 2, 3, 2 ** 20)
    assert [pl.pl_slope(f) for f in frames] == [ONE, ONE, 2 ** 29, 357913942, 1024] == [limitref.slope(f) for f in frames]
    assert [pl.pl_reach(f) for f in frames] == [1, 1, 2, 3, 2 ** 20] == [limitref.reach(f) for f in frames]
    assert [pl.pl_carry_tiles(f) for f in frames] == [0, 0, 1, 1, 512]
    for f in (5, 7, 1000, T - 1, T, T + 1, T + 2, T + 3, 2 * T + 3, 48000, 2 ** 20 - 1):
        s, reach = pl.pl_slope(f), pl.pl_reach(f)
        assert s == -(-ONE // f) and reach == -(-ONE // s) <= f
        assert (reach - 1) * s < ONE <= reach * s                              # the last distance that can lower G, and the first that cannot
        k = pl.pl_carry_tiles(f)                                               # tiles k apart are (k - 1) T + 1 frames apart at the least
        assert (k - 1) * T + 1 <= reach - 1 < k * T + 1
    assert max(pl.pl_carry_tiles(f) for f in range(0, 2 ** 20 + 1, 4093)) <= 512 and pl.pl_carry_tiles(2 ** 20) == 512


def test_the_required_gain_by_long_division_is_the_operators(pl):
    rng = np.random.default_rng(2)
    cases = [(1, 1), (2, 1), (2 ** 31, 1), (2 ** 31, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 2), (128, 127), (32768, 1), (32768, 32767), (3, 2), (5, 5), (0, 1), (7, 100)]
    cases += [(int(p), int(c)) for p, c in zip(rng.integers(0, 2 ** 31 + 1, 2000), rng.integers(1, 2 ** 31, 2000))]
    for p, c in cases:
        assert pl.pl_required_gain(p, c) == (ONE if p <= c else (c * ONE) // p), (p, c)
    for x, g in [(-2 ** 31, ONE), (-2 ** 31, 0), (-2 ** 31, 1), (2 ** 31 - 1, ONE - 1), (-1, ONE - 1), (-1, 1), (1, ONE - 1), (-32768, ONE // 3), (-7, 3 * (ONE // 4))]:
        assert pl.pl_apply_gain(x, g) == (x * g) >> 30, (x, g)                 # floor, not truncation


def test_every_refusal_in_its_order(pl):
    def check(width=2, nch=2, n=100, ceiling=20000, attack=10, release=100, first=0, count=100, a=(0x1000, 400, 0, 1), o=(0x3000, 400, 0, 1), p=(0x5000, 400, 0, 1)):
        op = lambda t: (C.c_uint64 * 4)(*t)
        return REFUSALS[pl.pl_check(width, nch, n, ceiling, attack, release, first, count, op(a), op(o), op(p))]
    none = (0, 0, 0, 0)
    assert check() == "OK"
    assert check(width=3) == check(width=0) == check(width=8) == "BAD_WIDTH"
    assert check(width=1, ceiling=127) == check(width=4, ceiling=2 ** 31 - 1, a=(0x1000, 800, 0, 1), o=(0x3000, 800, 0, 1)) == "OK"
    assert check(nch=0) == check(nch=3) == "BAD_CHANNELS" and check(nch=1) == "OK"
    assert check(ceiling=0) == check(ceiling=32768) == check(width=1, ceiling=128) == check(width=4, ceiling=2 ** 31) == check(ceiling=2 ** 32 + 5) == "BAD_CEILING"
    assert check(ceiling=1) == check(ceiling=32767) == "OK"
    assert check(attack=2 ** 20 + 1) == check(attack=2 ** 32) == "BAD_ATTACK" and check(release=2 ** 20 + 1) == "BAD_RELEASE"
    assert check(attack=2 ** 20, release=2 ** 20) == check(attack=0, release=0) == "OK"
    assert check(count=101) == check(first=1) == check(first=101, count=0) == check(first=2 ** 64 - 1, count=2) == "BAD_WINDOW"
    assert check(first=100, count=0) == check(first=99, count=1) == check(n=0, count=0, a=(0x1000, 0, 0, 1)) == "OK"
    assert check(a=(0x1000, 399, 0, 1)) == check(a=(0x1000, 404, 6, 1)) == check(a=(0x1000, 400, 401, 1)) == "IN_RANGE"
    assert check(a=(0x1000, 404, 4, 1)) == check(a=(0x1000, 500, 3, 1)) == "OK"                    # (any byte: no alignment is asked for)
    assert check(o=(0x3000, 399, 0, 1)) == check(o=(0x3000, 404, 6, 1)) == "OUT_RANGE" and check(o=(0x3000, 403, 3, 1)) == "OK"
    assert check(p=(0x5000, 399, 0, 1)) == check(p=(0x5000, 404, 5, 1)) == "GAIN_RANGE" and check(p=(0x5000, 401, 1, 1)) == "OK"
    assert check(o=(0x3000, 40, 0, 1), p=(0x5000, 40, 0, 1), first=90, count=10) == "OK"            # a window's destinations hold the window alone
    # in place: exactly the window's own bytes and nothing else
    assert check(o=(0x1000, 400, 0, 1)) == check(o=(0x1000, 400, 40, 1), first=10, count=90) == check(o=(0x1000 + 40, 360, 0, 1), first=10, count=90) == "OK"
    assert check(o=(0x1000, 400, 36, 1), first=10, count=90) == check(o=(0x1000, 400, 44, 1), first=10, count=89) == check(o=(0x1000, 400, 0, 1), first=10, count=90) == "OUT_OVERLAP"
    assert check(o=(0x1000 + 398, 400, 0, 1)) == check(o=(0x1000 - 398, 400, 0, 1)) == check(o=(0x1000, 400, 1, 1), count=99) == "OUT_OVERLAP"
    assert check(o=(0x1000 + 400, 400, 0, 1)) == check(o=(0x1000 - 400, 400, 0, 1)) == "OK"         # side by side is no overlap
    assert check(o=(0x1000 + 2, 400, 0, 1), first=50, count=0) == "OK"                              # an empty window writes nothing
    assert check(p=(0x1000 + 399, 400, 0, 1)) == check(p=(0x1000 - 399, 400, 0, 1)) == check(p=(0x3000 + 399, 400, 0, 1)) == check(p=(0x3000, 400, 0, 1)) == "GAIN_OVERLAP"
    assert check(p=(0x1000 + 300, 400, 0, 1), first=0, count=10, o=(0x3000, 40, 0, 1)) == "GAIN_OVERLAP"                 # the WHOLE input counts, not its window
    assert check(p=(0x1000 + 400, 400, 0, 1)) == check(p=(0x3000 + 400, 400, 0, 1)) == "OK"
    assert check(o=none) == check(p=none) == "OK" and check(o=none, p=none) == "NO_DESTINATION"
    assert check(o=none, p=(0x1000, 400, 0, 1)) == "GAIN_OVERLAP" and check(o=(0x1000, 400, 0, 1), p=none) == "OK"
    # the order: each refusal hides the ones behind it
    bad = dict(width=3, nch=3, ceiling=0, attack=2 ** 21, release=2 ** 21, count=10 ** 6, a=(0x1000, 1, 0, 1), o=(0x1000, 1, 0, 1), p=(0x1000, 1, 0, 1))
    order = ["width", "nch", "ceiling", "attack", "release", "count", "a", "o", "p"]
    want = ["BAD_WIDTH", "BAD_CHANNELS", "BAD_CEILING", "BAD_ATTACK", "BAD_RELEASE", "BAD_WINDOW", "IN_RANGE", "OUT_RANGE", "GAIN_RANGE"]
    for k, name in enumerate(order):
        assert check(**{key: bad[key] for key in order[k:]}) == want[k], name
    assert check(o=(0x1000 + 2, 400, 0, 1), p=(0x1000, 400, 0, 1)) == "OUT_OVERLAP" and check(ceiling=0, o=none, p=none) == "BAD_CEILING"
    assert check(count=101, o=none, p=none) == "BAD_WINDOW" and check(a=(0x1000, 1, 0, 1), o=none, p=none) == "IN_RANGE"


def test_the_plan_of_a_window(pl):
    T = N.PCM_LIMIT_TILE_FRAMES

    def plan(n, attack, release, first, count):
        got = (C.c_uint64 * 8)()
        pl.pl_plan(n, attack, release, first, count, got)
        return list(got)
    assert plan(1, 0, 0, 0, 1) == [ONE, ONE, 0, 0, 0, 1, 0, 1]
    assert plan(10 * T, 0, 0, 3 * T - 1, 2) == [ONE, ONE, 0, 0, 2, 2, 2, 2]
    assert plan(10 * T, 2, 3, 3 * T, T) == [2 ** 29, 357913942, 1, 1, 3, 1, 2, 3]
    assert plan(10 * T + 1, T + 2, 2 * T + 3, 5 * T + 7, 1) == [limitref.slope(T + 2), limitref.slope(2 * T + 3), 2, 3, 5, 1, 2, 6]
    assert plan(10 * T + 1, 2 ** 20, 2 ** 20, 5 * T + 7, 1)[2:] == [512, 512, 5, 1, 0, 11]                    # cut to the sample's 11 tiles
    assert plan(2000 * T, 2 ** 20, 2 ** 20, 1000 * T, 3 * T + 1)[2:] == [512, 512, 1000, 4, 488, 512 + 4 + 512]


def test_the_carry_sums_pass_32_bits_and_are_capped(pl):
    """fold the carries from given summaries: sums of a summary and a distance times a slope, the distance up to 2^20 frames; at the
    steepest slope that still carries (2^29, a tile apart) and at the longest reach (513 tiles in all)"""
    T = N.PCM_LIMIT_TILE_FRAMES

    def carries(n, attack, release, u, fs, bs):
        got = (C.c_uint32 * 2)()
        pl.pl_carries(n, attack, release, u, (C.c_uint32 * len(fs))(*fs), (C.c_uint32 * len(bs))(*bs), got)
        return list(got)
    # a slope of ONE: no tile carries, whatever the summaries hold
    assert carries(3 * T, 0, 1, 1, [0], [0]) == [ONE, ONE]
    # a slope of 2^29: the neighbour alone, one frame away
    assert carries(3 * T, 2, 2, 1, [5, 0, 7], [9, 0, 11]) == [5 + 2 ** 29, 11 + 2 ** 29]
    assert carries(3 * T, 2, 2, 1, [2 ** 29, 0, 7], [9, 0, 2 ** 29 + 1]) == [ONE, ONE]                        # capped
    assert carries(3 * T, 2, 2, 0, [5, 6], [0, 8]) == [ONE, 8 + 2 ** 29] and carries(3 * T, 2, 2, 2, [5, 6], [0, 8]) == [5 + 2 ** 29, ONE]
    # T + 2 frames: a reach of T + 2, so the next tile but one carries, at its nearest frame alone: (T + 1) * s is all but ONE
    s = limitref.slope(T + 2)
    assert (T + 1) * s < ONE < (T + 2) * s and pl.pl_carry_tiles(T + 2) == 2
    assert carries(9 * T, T + 2, T + 2, 4, [0, ONE, 0, 0, 0], [0, 0, 0, 0, 0]) == [(T + 1) * s, s]
    assert carries(9 * T, T + 2, T + 2, 4, [2, 3, 0, 0, 0], [0, 0, 0, ONE, 1]) == [3 + s, 1 + (T + 1) * s]
    # 2^20 frames: 512 tiles a side; the farthest summary of 0 gives (511 T + 1) * 1024 < ONE, a product of a 20-bit distance and a slope
    n, u = 1200 * T, 600
    fs, bs = [ONE] * 1025, [ONE] * 1025
    fs[0], bs[1024] = 0, 17
    assert carries(n, 2 ** 20, 2 ** 20, u, fs, bs) == [(511 * T + 1) * 1024, 17 + (511 * T + 1) * 1024]
    fs[0], fs[1], bs[1024], bs[1000] = ONE, ONE - 1, ONE, 1000
    assert carries(n, 2 ** 20, 2 ** 20, u, fs, bs) == [ONE, 1000 + (487 * T + 1) * 1024]


def test_s_of_two_to_the_30_across_two_tiles(pl):
    """attack and release of 0 and 1 frames: the slope is 2^30, and a frame T away lies 2^41 up the ramp -- in 32 bits that wraps to 0
    and the peak's gain would come back a tile later.  Peaks at a tile's last frame and at the next one's first."""
    T = N.PCM_LIMIT_TILE_FRAMES
    x = np.full((2 * T + 5, 1), 100, dtype=np.int64)
    x[T - 1], x[T], x[0], x[2 * T + 4] = 30000, -32768, 20000, 32767
    for attack, release in ((0, 0), (1, 1), (0, 1), (1, 0)):
        y, G = host(pl, x, 2, 1000, attack, release)
        g = limitref.required_gain(x, 1000)
        assert G.tolist() == g.tolist() and (G < ONE).sum() == 4 and np.array_equal(y, (x * g[:, None]) >> 30)
    for attack, release in ((2, 2), (2, 0), (0, 3), (3, 2)):
        y, G = host(pl, x, 2, 1000, attack, release)
        wy, wG = limitref.limit(x, 1000, attack, release)
        assert np.array_equal(G, wG) and np.array_equal(y, wy) and (G == ONE).sum() > 2 * T - 20


CASES = [(w, nch) for w in (1, 2, 4) for nch in (1, 2)]


@pytest.mark.parametrize("width,nch", CASES)
def test_the_host_loop_equals_the_reference_forwards_and_backwards(pl, width, nch):
    rng = np.random.default_rng(100 * width + nch)
    T = N.PCM_LIMIT_TILE_FRAMES
    spans = [0, 1, 2, 7, T - 1, T, T + 1, 2 * T + 3]
    hi = limitref.hi_of(width)
    for k, n in enumerate((1, 2, 64, T - 1, T, T + 1, 3 * T + 5)):
        for j in range(4):
            attack, release = spans[(k + 3 * j) % 8], spans[(2 * k + j + 1) % 8]
            ceiling = (hi, hi // 2, max(hi // 10, 1), max(hi // 100, 1))[j]
            x = limitref.noise_with_peaks(rng, width, n, nch, ceiling)
            wy, wG = limitref.limit(x, ceiling, attack, release)
            assert int(np.abs(wy).max()) <= ceiling
            for backwards in (False, True):
                y, G = host(pl, x, width, ceiling, attack, release, backwards=backwards)
                assert np.array_equal(G, wG) and np.array_equal(y, wy), (n, attack, release, ceiling, backwards)
    assert (wG == ONE).any() and (wG < ONE).any()                              # (the longest case: frames at unity and frames below)
    assert host(pl, np.zeros((0, nch), dtype=np.int64), width, 1, 5, 5)[0].shape == (0, nch)


@pytest.mark.parametrize("width", [1, 2, 4])
def test_the_rails(pl, width):
    hi = limitref.hi_of(width)
    x = np.array([[-hi - 1, 0], [hi, -hi - 1], [0, 0], [-1, 1], [hi, hi]], dtype=np.int64)
    for ceiling in (1, hi):
        for attack, release in ((0, 0), (2, 3)):
            y, G = host(pl, x, width, ceiling, attack, release)
            wy, wG = limitref.limit(x, ceiling, attack, release)
            assert np.array_equal(y, wy) and np.array_equal(G, wG) and int(np.abs(y).max()) <= ceiling
    y, G = host(pl, x, width, hi, 0, 0)                                        # -2^(8w-1) under C = HI: all but unity, and the frame at HI untouched
    assert G.tolist() == [(hi * ONE) // (hi + 1)] * 2 + [ONE] * 3 and y[0, 0] >= -hi and y[4].tolist() == [hi, hi]
    assert host(pl, x, width, 1, 0, 0)[0][2:4].tolist() == [[0, 0], [-1, 1]]


@pytest.mark.parametrize("width", [1, 2, 4])
def test_a_window_is_that_slice_of_the_whole_result(pl, width):
    rng = np.random.default_rng(7 + width)
    T = N.PCM_LIMIT_TILE_FRAMES
    n, ceiling = 3 * T + 300, limitref.hi_of(width) // 3
    x = limitref.noise_with_peaks(rng, width, n, 2, ceiling, peaks=[0, T - 3, T - 1, T, 2 * T + 99, 2 * T + 111, n - 1])
    wy, wG = limitref.limit(x, ceiling, T + 1, 2 * T + 3)
    pairs = ((0, 1), (0, T), (5, T), (T - 1, 2), (T, 1), (T - 2, 1), (T + 1, T - 2), (2 * T + 100, 11), (n - 1, 1), (1000, 0), (n, 0), (3, n - 3))
    for first, count in pairs:
        for backwards in (False, True):
            y, G = host(pl, x, width, ceiling, T + 1, 2 * T + 3, first, count, backwards)
            assert np.array_equal(y, wy[first:first + count]) and np.array_equal(G, wG[first:first + count]), (first, count, backwards)


def test_the_file_is_a_program_of_its_own_as_well(tmp_path):
    exe = tmp_path / "cpu_pcmlimit"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DPCMLIMIT_MAIN", str(ROOT / "tests" / "cpu_pcmlimit.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("pcmlimit: ") and p.stdout.strip().endswith("ok"), p.stdout + p.stderr
