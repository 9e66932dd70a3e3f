"""The per-sample arithmetic of audioop.ratecv as synthesizer_amd/csrc/ratecv.hpp states it for resample.hip and for the resampled events
of sequence.hip (shr::position / step / index, shr::small_int, shr::shifted_int), built for the host with g++ -ffp-contract=off and held
to live ``audioop.ratecv``: every width, mono and stereo, the speeds a sampler uses at the usual rates, and rate pairs whose reduced
outrate is 65536 or more (the float64 route at widths 1 and 2).  Equality, no tolerance.  No GPU."""
import audioop
import ctypes
import subprocess
from math import gcd
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
U64 = ctypes.c_uint64
SPEEDS = [0.1, 0.5, 2 ** (-5 / 12), 0.9999, 2 ** (1 / 12), 1.5, 3.3, 10]
RATES = [8000, 22050, 44100, 48000]
# (inrate, outrate) with a reduced outrate >= 65536: 96 kHz against a rate coprime to it, both ways round, and a sampler's 96 kHz * 2^(7/12)
BIG = [(95999, 96000), (143837, 96000), (96000, 95999), (9601, 96000), (959999, 96000), (65537, 65536)]


@pytest.fixture(scope="module")
def sr(tmp_path_factory):
    out = tmp_path_factory.mktemp("seqrate") / "libseqrate.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                    str(ROOT / "tests" / "cpu_seqrate.cpp"), "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    lib.sr_out_frames.argtypes = [U64, U64, U64]
    lib.sr_out_frames.restype = U64
    lib.sr_small.argtypes = [ctypes.c_int, U64, U64]
    lib.sr_resample.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, U64, U64, ctypes.c_char_p, U64, ctypes.c_int, ctypes.c_int]
    return lib


def pcm(rng, width, nsamples) -> bytes:
    """full-scale random samples with runs of the lowest and of the highest value"""
    bits = 8 * width
    v = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), nsamples, dtype=np.int64)
    for _ in range(6):
        at = int(rng.integers(0, max(1, nsamples - 40)))
        v[at:at + int(rng.integers(2, 40))] = -(1 << (bits - 1)) if _ % 2 else (1 << (bits - 1)) - 1
    if width == 3:
        return v.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    return v.astype({1: np.int8, 2: "<i2", 4: "<i4"}[width]).tobytes()


def check(sr, rng, width, nch, inrate, outrate, frames):
    data = pcm(rng, width, frames * nch)
    want = audioop.ratecv(data, width, nch, inrate, outrate, None)[0]
    nout = sr.sr_out_frames(frames, inrate, outrate)
    assert nout * width * nch == len(want), (width, nch, inrate, outrate, frames)
    routes = [0, 1] if sr.sr_small(width, inrate, outrate) else [0]
    for use_small in routes:
        for run in (1, 4, 8):
            got = ctypes.create_string_buffer(len(want) + 1)
            sr.sr_resample(data, width, nch, inrate, outrate, got, nout, run, use_small)
            assert got.raw[:len(want)] == want, (width, nch, inrate, outrate, frames, use_small, run)
    return routes


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_the_speeds_of_a_sampler_at_the_usual_rates(sr, width, nch):
    rng = np.random.default_rng(10 * width + nch)
    small = 0
    for rate in RATES:
        for speed in SPEEDS:
            inrate = int(rate * speed)
            assert inrate != rate
            small += 1 in check(sr, rng, width, nch, inrate, rate, int(rng.integers(700, 1500)))
    assert (small > 0) == (width <= 2)          # the integer route is reached at widths 1 and 2, and only there
    for frames in (0, 1, 2, 3):                 # ratecv of one frame is one frame
        check(sr, rng, width, nch, int(44100 * 1.5), 44100, frames)
        check(sr, rng, width, nch, int(44100 * 0.37), 44100, frames)


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_a_reduced_outrate_of_65536_or_more_takes_the_float64_route(sr, width, nch):
    rng = np.random.default_rng(50 + 10 * width + nch)
    for inrate, outrate in BIG:
        assert outrate // gcd(inrate, outrate) >= 65536 and not sr.sr_small(width, inrate, outrate)
        check(sr, rng, width, nch, inrate, outrate, int(rng.integers(300, 600)))
