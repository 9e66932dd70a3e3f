"""The references and inputs of tests/test_gpu_pcm_views.py on their own (no GPU): the written-out float expressions produce no
out-of-range value in the clean cases and exactly one, where it is meant to be, in the overflow cases -- so that a refusal (or its
absence) on the device is the kernel's doing, not the inputs' -- and the offsets and lengths cover what that file promises."""
import numpy as np
import pytest

from oracle import pcm_oracle as P
from tests import test_gpu_pcm_views as V


@pytest.mark.parametrize("width", [1, 2, 4])
def test_modulate_and_pan_cases(width):
    vec = 16 // width
    for n in V.lengths(width, channel_op=True):
        for nmod in sorted({7, max(n, 1)}):
            vals, mod, values = V.modulate_case(width, n, nmod)
            assert len(values) == n and V.out_of_range(values, width) == 0 and all(-1.0 <= m <= 1.0 for m in mod)
        for nch in (1, 2):
            vals, pan, values = V.pan_case(width, nch, n)
            assert len(values) == 2 * n and V.out_of_range(values, width) == 0 and all(-1.0 <= p <= 1.0 for p in pan)
    n = 256 * vec + vec + 1
    vals, mod, values = V.modulate_case(width, n, n, overflow=True)
    assert V.out_of_range(values, width) == 1 and V.out_of_range(values[-1:], width) == 1
    for nch in (1, 2):
        vals, pan, values = V.pan_case(width, nch, n, overflow=True)
        assert V.out_of_range(values, width) == 1 and V.out_of_range(values[-2:-1], width) == 1      # the last frame's left value


@pytest.mark.parametrize("width", [1, 2, 4])
def test_fade_reference_stays_in_range(width):
    rng = np.random.default_rng(width)
    for n in V.lengths(width):
        vals = V.rand_vals(rng, width, n)
        for fadeout, slope, offset in V.FADES:
            values = V.fade_values(vals.tolist(), fadeout, slope, offset)
            assert V.out_of_range(values, width) == 0
            assert P.fade(V.encode(vals, width), width, bool(fadeout), slope, offset) == V.encode(values, width)


def test_encode_is_the_oracles():
    rng = np.random.default_rng(0)
    for width in (1, 2, 3, 4):
        vals = V.rand_vals(rng, width, 100)
        assert V.encode(vals, width) == P._encode(vals, width) and P._decode(V.encode(vals, width), width).tolist() == vals.tolist()
        lo, hi = V.lo_hi(width)
        assert {lo, hi, lo + 1, hi - 1} <= set(vals[:8].tolist()) and vals[-8:].tolist() == vals[:8].tolist()[::-1]


def test_offsets_and_lengths_cover_the_classes():
    for width in (1, 2, 3, 4):
        res = V.residues(width)
        assert {r % 16 for r in res} >= {0, width, 8, 16 - width}
        if width == 3:
            assert {r % 4 for r in res} == {0, 1, 2, 3}
        else:
            assert all(r % width == 0 for r in res)             # natural alignment is the caller's duty
        for nw in (1, 2, 3, 4):
            pairs = V.offset_pairs(width, nw)
            assert (0, 0) in pairs
            assert {a for a, o in pairs if o == 0} == set(res) and {o for a, o in pairs if a == 0} == set(V.residues(nw))
            both = [(a, o) for a, o in pairs if a and o]
            assert len(both) >= 3 and all(a % 16 != o % 16 for a, o in both)
        vec = 16 // (4 if width == 3 else width)
        assert set(V.lengths(width)) >= {0, 1, vec - 1, vec, vec + 1, 256 * vec - 1, 256 * vec, 256 * vec + vec + 1, 3 * 256 * vec + 5}
    assert set(V.lengths(3)) >= {2, 3, 5}
