"""The per-sample gain of an enveloped event as synthesizer_amd/csrc/seqenv.hpp states it for sequence.hip (she::gain, she::shape_lane),
built for the host with g++ -ffp-contract=off and run over the segment lists that the host-side replay of ``Sample.envelope`` makes
(``synthesizer_amd.sample._envelope_segments``), against ``oracle.sample_oracle.RefSample.envelope``: widths 1, 2 and 4, mono and stereo,
the shapes the kernels use (lanes of 2, 4 and 8 samples; tiles inside one segment and tiles that straddle boundaries; events that start
anywhere in a lane), and the degenerate envelopes.  Equality, no tolerance.  No GPU."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle.sample_oracle import RefSample
from synthesizer_amd import _native as N
from synthesizer_amd.sample import _envelope_segments

ROOT = Path(__file__).resolve().parent.parent
U32 = ctypes.c_uint32
SEG = np.dtype([("mul", "<f8"), ("slope", "<f8"), ("numsamples", "<f8"), ("offset", "<f8"), ("end", "<u4"), ("origin", "<u4"),
                ("kind", "<u4"), ("pad", "<u4")])               # she::Seg


@pytest.fixture(scope="module")
def se(tmp_path_factory):
    out = tmp_path_factory.mktemp("seqenv") / "libseqenv.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                    str(ROOT / "tests" / "cpu_seqenv.cpp"), "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    lib.se_shape.argtypes = [ctypes.c_char_p, ctypes.c_int, U32, ctypes.c_void_p, U32, U32, U32, ctypes.c_int, ctypes.c_char_p]
    lib.se_seg_bytes.restype = ctypes.c_uint
    lib.se_max_segments.restype = ctypes.c_uint
    return lib


def pcm(rng, width, nsamples) -> bytes:
    """full-scale random samples with runs of the lowest and of the highest value and a run of -1 (floor and trunc part there)"""
    bits = 8 * width
    v = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), nsamples, dtype=np.int64)
    for i in range(6):
        at = int(rng.integers(0, max(1, nsamples - 10)))
        v[at:at + int(rng.integers(2, 10))] = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1, -1)[i % 3]
    return v.astype({1: np.int8, 2: "<i2", 4: "<i4"}[width]).tobytes()


def table(segs):
    t = np.zeros(len(segs), dtype=SEG)
    for i, (end, mul, kind, slope, numsamples, offset, origin) in enumerate(segs):
        t[i] = (mul, slope, numsamples, offset, end, origin, kind, 0)
    return t


def shaped(se, data, width, segs, dst, tile, lane):
    n = len(data) // width
    t = table(segs)
    out = ctypes.create_string_buffer(len(data) + 1)
    assert se.se_shape(data, width, n, t.ctypes.data if len(t) else None, len(t), dst, tile, lane, out) == 0
    assert out.raw[len(data)] == 0, "a zero outside the event did not stay zero"
    return out.raw[:len(data)]


def check(se, rng, width, nch, rate, frames, env):
    data = pcm(rng, width, frames * nch)
    want = RefSample(data, width, rate, nch).envelope(*env).frames
    segs = _envelope_segments(len(data), width, nch, rate, *env)
    assert len(segs) <= se.se_max_segments()
    assert all(a[0] < b[0] for a, b in zip(segs, segs[1:])) and (not segs or segs[-1][0] == frames * nch)
    # one tile (everything straddles unless there is one segment), the kernels' tiles, and tiles so small that most lie inside a segment
    for dst, tile, lane in ((0, 1 << 20, 8), (5, 2048, 8), (3, 1024, 4), (6, 1024, 2), (13, 16, 8), (1, 8, 4), (7, 4, 2)):
        got = shaped(se, data, width, segs, dst, tile, lane)
        assert got == want, (width, nch, rate, frames, env, dst, tile, lane, segs)
    return len(segs)


def test_the_segment_record_is_48_bytes(se):
    assert se.se_seg_bytes() == SEG.itemsize == 48
    assert se.se_max_segments() == 7
    assert (N.ENV_NONE, N.ENV_FADE_IN, N.ENV_FADE_OUT) == (0, 1, 2)


@pytest.mark.parametrize("width", [1, 2, 4])
@pytest.mark.parametrize("nch", [1, 2])
def test_the_gain_over_replayed_segments_is_refsample_envelope(se, width, nch):
    rng = np.random.default_rng(100 * width + nch)
    counts = set()
    cases = [
        (8000, 2400, (0.05, 0.05, 0.5, 0.1)),               # the full shape: fade-in, fade-out, sustain, fade-out
        (8000, 2400, (0.0, 0.0, 0.5, 0.0)),                 # a sustain level alone: one segment
        (8000, 2400, (0.1, 0.0, 1.0, 0.0)),                 # an attack alone
        (8000, 2400, (0.0, 0.0, 1.0, 0.05)),                # a release alone
        (8000, 2400, (0.0, 0.1, 0.25, 0.0)),                # a decay alone
        (8000, 3001, (0.0101, 0.0203, 0.7, 0.0507)),        # boundaries off every multiple
        (11025, 3000, (0.07, 0.013, 0.3, 0.11)),
        (44100, 5000, (0.01, 0.02, 0.9, 0.03)),
        (22050, 999, (0.001, 0.0005, 0.6, 0.002)),
    ]
    for rate, frames, env in cases:
        counts.add(check(se, rng, width, nch, rate, frames, env))
    # an attack part whose own duration rounds a frame down (int(rate * (n / rate)) == n - 1): its last frame stays unfaded, five segments
    for rate in (8000, 11025, 44100):
        odd = [n for n in range(1, 3000) if int(rate * (n * width * nch / rate / width / nch)) != n][:3]
        assert odd, rate
        for n in odd:
            assert check(se, rng, width, nch, rate, n + 1500, ((n + 0.5) / rate, 0.01, 0.5, 0.02)) == 5
            counts.add(5)
    for _ in range(40):                                     # random shapes, parts that may be empty or swallow the sample
        rate = int(rng.choice([8000, 11025, 22050, 44100]))
        frames = int(rng.integers(1, 3000))
        dur = frames / rate
        a, d = (float(rng.choice([0.0, rng.uniform(0, dur), rng.uniform(0, 0.3 * dur)])) for _ in range(2))
        left = max(0.0, dur - a - d)
        r = float(rng.choice([0.0, rng.uniform(0, left) * 0.999]))
        s = float(rng.choice([0.0, 1.0, rng.uniform(0, 1)]))
        try:
            _envelope_segments(frames * nch * width, width, nch, rate, a, d, s, r)
        except ValueError:                                  # (the replay refuses what upstream slices from the wrong end)
            continue
        counts.add(check(se, rng, width, nch, rate, frames, (a, d, s, r)))
    assert {1, 2, 3, 4} <= counts and max(counts) >= 5, counts


@pytest.mark.parametrize("width", [1, 2, 4])
@pytest.mark.parametrize("nch", [1, 2])
def test_degenerate_envelopes(se, width, nch):
    rng = np.random.default_rng(7 * width + nch)
    rate, frames = 8000, 1200
    data = pcm(rng, width, frames * nch)
    # nothing at all: the input, and not one segment that does anything
    segs = _envelope_segments(len(data), width, nch, rate, 0.0, 0.0, 1.0, 0.0)
    assert all(s[1] == 1.0 and s[2] == N.ENV_NONE for s in segs)
    assert shaped(se, data, width, segs, 5, 1024, 4) == data == RefSample(data, width, rate, nch).envelope(0.0, 0.0, 1.0, 0.0).frames
    # sustainlevel 0: silence after attack and decay (floor of -x * 0.0 is 0 as well)
    check(se, rng, width, nch, rate, frames, (0.0, 0.0, 0.0, 0.0))
    check(se, rng, width, nch, rate, frames, (0.02, 0.03, 0.0, 0.01))
    # an attack longer than the sample: the whole sample is the fade-in, the other parts are empty
    assert check(se, rng, width, nch, rate, frames, (1.0, 0.0, 1.0, 0.0)) == 1
    check(se, rng, width, nch, rate, frames, (0.15, 0.0, 0.5, 0.0))
    # attack + decay longer than the sample
    check(se, rng, width, nch, rate, frames, (0.1, 0.2, 0.5, 0.0))
    # a one-frame sample
    for env in ((0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.5, 0.0), (1.0, 0.0, 1.0, 0.0), (0.0, 1.0, 0.5, 0.0), (0.0, 0.0, 0.5, 1.0 / rate)):
        check(se, rng, width, nch, rate, 1, env)
    # an empty one
    assert _envelope_segments(0, width, nch, rate, 0.0, 0.0, 0.5, 0.0) == []


def test_a_release_longer_than_the_sustain_is_refused():
    with pytest.raises(ValueError, match="envelope"):
        _envelope_segments(2 * 800, 2, 1, 8000, 0.05, 0.03, 0.5, 0.03)     # 0.1 s: 0.02 s are left, the release wants 0.03
    with pytest.raises(ValueError, match="envelope"):
        _envelope_segments(2 * 800, 2, 1, 8000, 1.0, 0.0, 0.5, 0.001)      # the attack took everything
