"""The composed index map of an event of sh_mix_events_rev -- region, reverse, loop -> stored sample -- as synthesizer_amd/csrc/seqrev.hpp
states it for sequence.hip, built for the host with g++ and held to a brute-force unrolling in Python: the region's samples numbered as
they are stored, turned round with a slice (the order of the SAMPLES, as audioop.reverse), the loop written out frame by frame.  Every
small (F, S, L, V, nch), forwards and reversed, from scratch and stepped.  Equality.  No GPU."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
U32 = ctypes.c_uint32


@pytest.fixture(scope="module")
def sv(tmp_path_factory):
    out = tmp_path_factory.mktemp("seqrev") / "libseqrev.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", str(ROOT / "tests" / "cpu_seqrev.cpp"), "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    lib.sv_map.argtypes = lib.sv_walk.argtypes = [U32] * 6 + [ctypes.c_void_p]
    return lib


def unrolled(reversed_, F, S, L, V, nch):
    """the stored sample (counted from the region's first) behind every sample of the V virtual frames, written out"""
    stored = list(range(F * nch))
    played = stored[::-1] if reversed_ else stored          # audioop.reverse: samples, not frames
    frames = [played[f * nch:(f + 1) * nch] for f in range(F)]
    E = S + L
    out = []
    for v in range(V):
        out += frames[v if (not L or v < E) else S + (v - E) % L]
    return out


def _ask(fn, reversed_, F, E, L, V, nch):
    out = np.full(V * nch, -99, dtype=np.int64)
    fn(reversed_, F, E, L, V, nch, out.ctypes.data)
    return out.tolist()


@pytest.mark.parametrize("nch", [1, 2, 3])
@pytest.mark.parametrize("reversed_", [0, 1])
def test_every_small_region_loop_and_length(sv, reversed_, nch):
    cases = 0
    for F in range(1, 8):
        for V in range(0, F + 1):                           # no loop: a plain cut of the (reversed) region
            assert _ask(sv.sv_map, reversed_, F, 0, 0, V, nch) == unrolled(reversed_, F, 0, 0, V, nch)
        for S in range(F):
            for L in range(1, F - S + 1):
                E = S + L
                for V in range(0, E + 3 * L + 3):
                    want = unrolled(reversed_, F, S, L, V, nch)
                    assert _ask(sv.sv_map, reversed_, F, E, L, V, nch) == want, (F, S, L, V)
                    assert _ask(sv.sv_walk, reversed_, F, E, L, V, nch) == want, (F, S, L, V)
                    assert not want or (0 <= min(want) and max(want) < F * nch)              # nothing outside the region is read
                    cases += 1
    assert cases > 1000


def test_what_a_reversed_stereo_frame_is(sv):
    """played frame 0 of a reversed stereo region of 5 frames is stored frame 4 with its channels swapped: stored samples 9, 8"""
    assert _ask(sv.sv_map, 1, 5, 0, 0, 5, 2) == [9, 8, 7, 6, 5, 4, 3, 2, 1, 0]
    assert _ask(sv.sv_map, 0, 5, 0, 0, 5, 2) == list(range(10))
    # looped: played frames 1 and 2 are the loop; the seam goes from played frame 2 (stored 2: samples 5, 4) to played frame 1 (stored 3: 7, 6)
    assert _ask(sv.sv_map, 1, 5, 3, 2, 6, 2) == [9, 8, 7, 6, 5, 4, 7, 6, 5, 4, 7, 6]


def test_a_reversed_looped_event_plays_only_the_end_of_its_region(sv):
    """its region as the entry point is told is the E frames in front of the loop's end: the same samples as the whole region, moved"""
    F, S, L, V, nch = 9, 2, 3, 14, 2
    E = S + L
    whole = unrolled(1, F, S, L, V, nch)
    part = _ask(sv.sv_map, 1, E, E, L, V, nch)              # the region [F - E, F) as stored
    assert [p + (F - E) * nch for p in part] == whole
