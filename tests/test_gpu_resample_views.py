"""The resampler (csrc/resample.hip, csrc/ratecv.hpp) through windows of larger buffers.

resample_launch sends every call whose input or output pointer is off the 16-byte grid to RT_GENERIC with vec = 1, and the four
routes that take the aligned calls of mono and stereo layouts (RT_PERIOD, RT_SMALL, RT_LDS, RT_FRAMES) store 16 bytes per thread
and stage whole input vectors.  Every case here runs with both windows on the grid, with the input off it, the output off it and
both off it; the output window is 64 bytes longer than the result, and pcm_view_call (tests/helpers.py) asserts that the surplus
and everything around the window keep their sentinel and that the input's parent is untouched.

References, neither of them the library: live audioop.ratecv for the integer widths, oracle.pcm_oracle.ratecv_f32 (bit for bit) for
float32.  The route every case is meant to reach is part of its id and is asserted on the host with the CPU build of ratecv.hpp
(tests/test_ratecv_plan.py: rc), given the same `aligned` flag the launch code computes.
"""
import audioop
import ctypes as C

import numpy as np
import pytest

from oracle import pcm_oracle as P
from tests.helpers import pcm_view_call
from tests.test_gpu_pcm_views import _check
from tests.test_ratecv_plan import rc  # noqa: F401  (the fixture: tests/cpu_ratecv.cpp built with g++)

pytestmark = pytest.mark.gpu

ROUTES = {"NONE": 0, "GENERIC": 1, "FRAMES": 2, "LDS": 3, "SMALL": 4, "PERIOD": 5}          # shr::Route
SURPLUS = 64                                               # bytes of output window behind frame nout
PERIOD_FRAMES = [12345, 40001]                             # at least three interior chunks and a tail
# 12 345 frames of MONO 96000 -> 44100 are 5671 output frames, fewer than three chunks of the period kernel: that case reaches PERIOD
# from 30 001 frames on, and 12 345 stays in as a case of its own, named for the route it takes just below the threshold
PERIOD_FRAMES_MONO_DOWN = [30001, 40001]
BELOW_PERIOD = ("SMALL", 2, 0, 1, 96000, 44100)
BELOW_PERIOD_FRAMES = [12345]
# (route, width, is_float, channels, inrate, outrate)
CASES = [
    ("PERIOD", 2, 0, 1, 44100, 48000), ("PERIOD", 2, 0, 2, 44100, 48000), ("PERIOD", 2, 0, 1, 96000, 44100), ("PERIOD", 2, 0, 2, 96000, 44100),
    ("SMALL", 2, 0, 1, 8000, 8001), ("SMALL", 1, 0, 2, 48000, 44100),
    ("LDS", 4, 0, 1, 44100, 48000), ("LDS", 4, 1, 2, 44100, 48000),
    ("FRAMES", 4, 0, 1, 192000, 8000), ("FRAMES", 2, 0, 4, 1000003, 999983),
    ("GENERIC", 2, 0, 3, 44100, 48000), ("GENERIC", 2, 0, 8, 44100, 48000),
    BELOW_PERIOD,
]


def expected_route(case, frames):
    """the route the case's id names, at every length the case runs"""
    return case[0]


def case_id(c):
    return "%s%s-%s%d-%dch-%d-%d" % (c[0], "-below-PERIOD" if c is BELOW_PERIOD else "", "f" if c[2] else "i", 8 * c[1], c[3], c[4], c[5])


def host_plan(rc, width, is_float, nch, inrate, outrate, aligned, frames):  # noqa: F811
    """the 19 numbers of the launch's plan for the whole output of `frames` input frames"""
    v = np.zeros(19, dtype=np.uint64)
    nout = P.ratecv_out_frames(frames, inrate, outrate)
    rc.rc_plan(width, is_float, nch, inrate, outrate, int(aligned), 0, 0, nout, 0, frames, v.ctypes.data)
    return [int(x) for x in v]


def frame_counts(rc, case):  # noqa: F811
    """PERIOD: its two lengths.  The others: 1, 2, 9, one workgroup's worth of output (256 x frames per thread of the aligned plan)
    minus and plus one frame, and 20 011"""
    route, width, is_float, nch, inrate, outrate = case
    if case is BELOW_PERIOD:
        return list(BELOW_PERIOD_FRAMES)
    if route == "PERIOD":
        return list(PERIOD_FRAMES_MONO_DOWN if case[3:] == (1, 96000, 44100) else PERIOD_FRAMES)
    fr = host_plan(rc, width, is_float, nch, inrate, outrate, True, 20011)[2]
    wg = max(3, 256 * fr * inrate // outrate)               # input frames that give about 256 * fr output frames
    return sorted({1, 2, 9, wg - 1, wg + 1, 20011})


def pcm(rng, width, is_float, n):
    """n samples; the extremes first, so that the first interpolations run between them"""
    if is_float:
        x = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        x[:4] = np.array([1.0, -1.0, -1.0, 1.0], dtype=np.float32)[:min(4, n)]
        return x
    lo, hi = -(1 << (8 * width - 1)), (1 << (8 * width - 1)) - 1
    x = rng.integers(lo, hi + 1, n, dtype=np.int64)
    x[:6] = np.array([hi, lo, lo, hi, hi, hi])[:min(6, n)]
    return x.astype({1: "<i1", 2: "<i2", 4: "<i4"}[width])


def reference(x, width, is_float, nch, inrate, outrate):
    if is_float:
        return P.ratecv_f32(x.reshape(-1, nch), inrate, outrate).tobytes()
    return audioop.ratecv(x.tobytes(), width, nch, inrate, outrate, None)[0]


def off_grid(fb):
    """one frame's worth of bytes off the grid where that is off it, else one sample's natural alignment"""
    return fb if fb % 16 else 4


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_resample_through_windows(gpu, rc, case):  # noqa: F811
    L = gpu.lib()
    route, width, is_float, nch, inrate, outrate = case
    fb = width * nch
    rng = np.random.default_rng(sum(case[1:]))
    for frames in frame_counts(rc, case):
        nout = P.ratecv_out_frames(frames, inrate, outrate)
        assert L.sh_resample_out_frames(frames, inrate, outrate) == nout
        if nout and expected_route(case, frames):
            assert host_plan(rc, width, is_float, nch, inrate, outrate, True, frames)[0] == ROUTES[expected_route(case, frames)], (case_id(case), frames)
        assert not nout or host_plan(rc, width, is_float, nch, inrate, outrate, False, frames)[0] == ROUTES["GENERIC"]
        x = pcm(rng, width, is_float, frames * nch)
        want = reference(x, width, is_float, nch, inrate, outrate)
        assert len(want) == nout * fb
        a = off_grid(width)
        results = {}
        for ai, ao in ((0, 0), (a, 0), (0, a), (a, 16 - a), (8, 8)):
            got_frames = C.c_size_t(12345)
            rc_, got = pcm_view_call(gpu, [(x.tobytes(), ai)], nout * fb, ao,
                                     lambda iv, ov: L.sh_resample(iv[0].handle, frames, nch, width, is_float, inrate, outrate, ov.handle, C.byref(got_frames)),
                                     out_view_nbytes=nout * fb + SURPLUS)
            assert got_frames.value == nout
            _check(rc_, got, want, (case_id(case), frames, ai, ao))
            results[(ai, ao)] = got
        assert len(set(results.values())) == 1


@pytest.mark.parametrize("nch", [1, 2])
def test_resample_24_bit_through_windows(gpu, nch):
    """width 3 goes through k_unpack24 / k_pack24 around the 32-bit path: the input window at every residue mod 4 and 13, the output
    window at 0 and 5"""
    L = gpu.lib()
    rng = np.random.default_rng(24 + nch)
    for inrate, outrate in ((44100, 48000), (3, 7)):
        for frames in (1, 9, 1025, 4099):
            v = rng.integers(-(1 << 23), 1 << 23, frames * nch, dtype=np.int64)
            v[:4] = np.array([0x7FFFFF, -0x800000, -0x800000, 0x7FFFFF])[:min(4, v.size)]
            raw = (v.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()
            want = audioop.ratecv(raw, 3, nch, inrate, outrate, None)[0]
            nout = len(want) // (3 * nch)
            assert nout == P.ratecv_out_frames(frames, inrate, outrate)
            for ai in (0, 1, 2, 3, 13):
                for ao in (0, 5):
                    rc_, got = pcm_view_call(gpu, [(raw, ai)], len(want), ao,
                                             lambda iv, ov: L.sh_resample(iv[0].handle, frames, nch, 3, 0, inrate, outrate, ov.handle, None),
                                             out_view_nbytes=len(want) + SURPLUS)
                    _check(rc_, got, want, ("24 bits", nch, inrate, outrate, frames, ai, ao))


RANGES = [(16, 100), (3984, 48), (4000 - 16, 8000), (4096, 1), (1920, 2100)]       # tests/test_gpu_pcm.py: _RESAMPLE_CHILD


@pytest.mark.parametrize("nch", [1, 2])
def test_resample_range_through_windows(gpu, nch):
    """sh_resample_range on the ranges of tests/test_gpu_pcm.py (starts inside a chunk of the period kernel, ends on and just behind a
    chunk edge, and the range up to the last output frame): the held input a window on the grid and 2 bytes off it, the output a
    window longer than out_n"""
    L = gpu.lib()
    rng = np.random.default_rng(60 + nch)
    frames = 40001
    for inrate, outrate in ((44100, 48000), (96000, 44100)):
        x = pcm(rng, 2, 0, frames * nch)
        want = audioop.ratecv(x.tobytes(), 2, nch, inrate, outrate, None)[0]
        nout = len(want) // (2 * nch)
        for out_first, out_n in RANGES + [(nout - nout % 16 - 160, 160 + nout % 16)]:
            if out_first + out_n > nout:
                continue
            a, b = C.c_size_t(), C.c_size_t()
            gpu.check(L.sh_resample_span(frames, inrate, outrate, out_first, out_n, C.byref(a), C.byref(b)))
            held = x[a.value * nch:(a.value + b.value) * nch].tobytes()
            piece = want[out_first * 2 * nch:(out_first + out_n) * 2 * nch]
            for ai, ao in ((0, 0), (2, 0), (0, 2), (2, 8)):
                rc_, got = pcm_view_call(gpu, [(held, ai)], len(piece), ao,
                                         lambda iv, ov: L.sh_resample_range(iv[0].handle, a.value, b.value, nch, 2, 0, inrate, outrate, out_first, out_n, ov.handle),
                                         out_view_nbytes=len(piece) + SURPLUS)
                _check(rc_, got, piece, ("range", nch, inrate, outrate, out_first, out_n, ai, ao))
