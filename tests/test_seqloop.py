"""The virtual-to-source frame mapping of a looped event as synthesizer_amd/csrc/seqloop.hpp states it for sequence.hip, built for the host
with g++ and held to Python's ``v if v < E else S + (v - E) % (E - S)``: from scratch (shl::map) and stepped (shl::at once, then shl::step1 /
shl::step by compare and subtract), loops of 1 to 1000 frames, starts of 0, 1 and 5, every virtual frame up to five passes and a bit, steps
of 1 to 11 frames -- longer than the loop among them -- with and without ratecv's carry, started at every frame.  Equality.  No GPU."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
U32 = ctypes.c_uint32
LOOPS = [1, 2, 3, 7, 8, 9, 1000]
STARTS = [0, 1, 5]


@pytest.fixture(scope="module")
def sl(tmp_path_factory):
    out = tmp_path_factory.mktemp("seqloop") / "libseqloop.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", str(ROOT / "tests" / "cpu_seqloop.cpp"), "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    lib.sl_map.argtypes = [U32, U32, U32, U32, ctypes.c_void_p]
    lib.sl_walk.argtypes = [U32, U32, U32, U32, U32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def want(v, S, E):
    return v if v < E else S + (v - E) % (E - S)


def top(S, L):
    return S + L + 5 * L + 3                                # E + 5 (E - S) + 3


@pytest.mark.parametrize("L", LOOPS)
@pytest.mark.parametrize("S", STARTS)
def test_from_scratch(sl, S, L):
    E = S + L
    n = top(S, L) + 1
    out = np.zeros(n, dtype=np.uint32)
    sl.sl_map(0, n, E, L, out.ctypes.data)
    assert out.tolist() == [want(v, S, E) for v in range(n)]
    assert out[E] == S and out[E - 1] == E - 1              # v == E exactly, and the frame in front of the seam
    assert out.max() == E - 1                               # nothing behind the loop's end is ever read


@pytest.mark.parametrize("L", LOOPS)
@pytest.mark.parametrize("S", STARTS)
def test_stepped_one_frame_at_a_time_from_every_start(sl, S, L):
    E = S + L
    n = top(S, L) + 1
    for v0 in sorted(set(list(range(0, min(n, E + 2 * L + 2))) + [n - 1])) if L < 1000 else (0, 1, E - 1, E, E + 1, E + L - 1, E + L, 2 * E):
        count = n - v0
        v, f = np.zeros(count, dtype=np.uint32), np.zeros(count, dtype=np.uint32)
        carry = np.zeros(count, dtype=np.uint8)
        sl.sl_walk(v0, count, E, L, 1, carry.ctypes.data, v.ctypes.data, f.ctypes.data)
        assert v.tolist() == list(range(v0, n))
        assert f.tolist() == [want(x, S, E) for x in range(v0, n)], (S, L, v0)


@pytest.mark.parametrize("L", LOOPS)
@pytest.mark.parametrize("S", STARTS)
def test_stepped_by_ratecv_steps_with_and_without_the_carry(sl, S, L):
    """a ratecv step is step_q frames, and step_q + 1 when the remainder wraps: steps of 1 .. 11 with a carry never, always and in the
    pattern of a remainder of 3/7 (steps of 0 frames with a carry too: a slowed-down note stays on a frame or moves one on)"""
    E = S + L
    rng = np.random.default_rng(100 * S + L)
    seen_longer = False
    for inc in range(0, 12):
        for pattern in ("never", "always", "3/7", "random"):
            if inc == 0 and pattern == "never":
                continue
            count = 64 if L < 1000 else 700
            if pattern == "never":
                carry = np.zeros(count, dtype=np.uint8)
            elif pattern == "always":
                carry = np.ones(count, dtype=np.uint8)
            elif pattern == "3/7":
                carry = np.array([((3 * (i + 1)) % 7) < 3 for i in range(count)], dtype=np.uint8)
            else:
                carry = rng.integers(0, 2, count).astype(np.uint8)
            for v0 in (0, 1, max(0, E - 2), E - 1, E, E + 1, E + L - 1, E + 3 * L + 1):
                v, f = np.zeros(count, dtype=np.uint32), np.zeros(count, dtype=np.uint32)
                sl.sl_walk(v0, count, E, L, inc, carry.ctypes.data, v.ctypes.data, f.ctypes.data)
                at = v0 + np.concatenate(([0], np.cumsum(inc + carry.astype(np.int64))[:-1]))
                assert v.tolist() == at.tolist()
                assert f.tolist() == [want(int(x), S, E) for x in at], (S, L, inc, pattern, v0)
            seen_longer |= inc > L
    assert seen_longer or L >= 11                           # steps longer than the loop


def test_prev_and_cur_across_the_seam(sl):
    """ratecv's prev and cur are virtual frames j - 1 and j, each mapped on its own: at j == E prev is the loop's last frame and cur its
    first; a loop of one frame maps both to it"""
    for S, L in ((5, 3), (0, 1), (1, 1), (5, 1000)):
        E = S + L
        out = np.zeros(2, dtype=np.uint32)
        sl.sl_map(E - 1, 2, E, L, out.ctypes.data)
        assert out.tolist() == [E - 1, S]
        sl.sl_map(E + L - 1, 2, E, L, out.ctypes.data)
        assert out.tolist() == [E - 1, S]
