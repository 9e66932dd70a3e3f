"""The exact integer reference of the float64 scans (tests/helpers.py: scan_*), checked without a GPU: against fractions.Fraction,
against a plain sequential float64 cumsum (which must pass the bound), and against a numpy restatement of the kernels' ORDER of
additions -- which passes with the exclusive value taken from the scan itself and fails, on the inputs built for it, with the
`inclusive - own` form the kernels had."""
from fractions import Fraction

import numpy as np
import pytest

from tests import helpers as H


def _hillis_steele(sh):
    """Rows of 256 values -> their inclusive sums in the kernels' order: eight levels, sh[t] += sh[t - o]."""
    sh = sh.copy()
    o = 1
    while o < 256:
        sh[:, o:] = sh[:, o:] + sh[:, :-o]
        o <<= 1
    return sh


def _block_exclusive(x, own_subtracted):
    incl = _hillis_steele(x)
    if own_subtracted:
        return incl - x, incl[:, 255]
    ex = np.zeros_like(incl)
    ex[:, 1:] = incl[:, :-1]
    return ex, incl[:, 255]


def model_scan(x, carry_in, own_subtracted=False):
    """csrc/osc_scan.hip in numpy, addition for addition: -> (out, carry_out).  own_subtracted: block_exclusive_scan_256 returning
    `incl - x` (as it did) instead of its left neighbour's inclusive sum."""
    n = len(x)
    ntiles = -(-n // H.SCAN_TILE)
    v = np.zeros(ntiles * H.SCAN_TILE)
    v[:n] = x
    v = v.reshape(ntiles, 256, 8)
    s = np.zeros((ntiles, 256))
    for j in range(8):
        s = s + v[:, :, j]
    ex, totals = _block_exclusive(s, own_subtracted)
    base = np.empty(ntiles)
    carry = float(carry_in)
    for r0 in range(0, ntiles, 256):
        blk = np.zeros((1, 256))
        cnt = min(256, ntiles - r0)
        blk[0, :cnt] = totals[r0:r0 + cnt]
        bex, btot = _block_exclusive(blk, own_subtracted)
        base[r0:r0 + cnt] = carry + bex[0, :cnt]
        carry = carry + btot[0]
    run = ex + base[:, None]
    out = np.empty((ntiles, 256, 8))
    for j in range(8):
        out[:, :, j] = run
        run = run + v[:, :, j]
    return out.reshape(-1)[:n], carry


def test_exact_prefix_and_bound_against_fractions():
    rng = np.random.default_rng(40)
    for kind in H.SCAN_INPUT_KINDS:
        k, carry_k = H.scan_inputs(kind, 300, rng)
        prefix, total, a, a_total = H.scan_exact(k, carry_k)
        x = H.scan_grid(k)
        step = Fraction(1, 1 << H.SCAN_GRID_BITS)
        run, run_a = Fraction(carry_k) * step, abs(Fraction(carry_k)) * step
        got = np.cumsum(np.concatenate([[H.scan_grid(carry_k)], x]))[:-1]         # a sequential float64 sum: i rounded additions at most
        err = H.scan_error(got, prefix)
        for i in range(300):
            assert Fraction(int(prefix[i])) * step == run and Fraction(int(a[i])) * step == run_a, (kind, i)
            assert Fraction(int(err[i])) * step == abs(Fraction(float(got[i])) - run), (kind, i)
            for depth in (1, 33, 40):
                assert int(H.scan_allowed(a[i:i + 1], depth)[0]) == (depth * int(a[i])) >> 53, (kind, i, depth)
            run += Fraction(float(x[i]))
            run_a += abs(Fraction(float(x[i])))
        assert Fraction(total) * step == run and Fraction(a_total) * step == run_a
        # the plain sequential sum passes the bound at small n: element i has seen i additions
        seq = np.cumsum(np.concatenate([[H.scan_grid(carry_k)], x[:32]]))[:-1]
        assert np.all(H.scan_error(seq, prefix[:32]) <= H.scan_allowed(a[:32], H.scan_depth(32))), kind


def test_grid_conversions_refuse_what_is_off_the_grid():
    with pytest.raises(AssertionError):
        H.scan_grid(np.array([(1 << 60) + 1]))                  # not a float64
    with pytest.raises(AssertionError):
        H.scan_to_grid(np.array([2.0 ** -41]))                  # below the grid step
    with pytest.raises(AssertionError):
        H.scan_to_grid(np.array([np.nan]))
    with pytest.raises(AssertionError):
        H.scan_exact(np.full(4, 1 << 60, dtype=np.int64))       # sum |k| = 2^62
    assert H.scan_allowed(np.array([(1 << 62) - 1]), 40)[0] == (40 * ((1 << 62) - 1)) >> 53


def test_depth_counts():
    assert H.scan_rounds(1) == 1 and H.scan_rounds(524288) == 1 and H.scan_rounds(524289) == 2 and H.scan_rounds(3 * 524288 + 77) == 4
    assert H.scan_depth(2048) == 32 and H.scan_depth(1 << 20) == 33 and H.scan_carry_depth(1 << 20) == 25
    assert H.scan_chain_depth([100]) == H.scan_depth(100)
    assert H.scan_chain_depth([1 << 20, 5, 7]) == 25 + 1 + 1 + 8            # first piece's carry, through the second, into the third
    assert H.scan_chain_depth([5, 1 << 20]) == max(33, 24 + 2 + 8)


@pytest.mark.parametrize("n", [1, 7, 9, 2049, 4101, 524289 + 4096])
def test_the_kernels_order_of_additions_meets_the_counted_bound(n):
    rng = np.random.default_rng(n)
    for kind in H.SCAN_INPUT_KINDS:
        k, carry_k = H.scan_inputs(kind, n, rng)
        prefix, total, a, a_total = H.scan_exact(k, carry_k)
        out, carry = model_scan(H.scan_grid(k), H.scan_grid(carry_k))
        assert np.all(H.scan_error(out, prefix) <= H.scan_allowed(a, H.scan_depth(n))), kind
        assert H.scan_error([carry], [total])[0] <= H.scan_allowed([a_total], H.scan_carry_depth(n))[0], kind


def test_subtracting_the_own_element_breaks_the_bound_and_the_inputs_show_it():
    """What the adversarial input is for: with `inclusive - own` as the exclusive value an output loses the part
    of its prefix that lies below ulp(prefix + own group), and the bound over j < i has no room for that."""
    rng = np.random.default_rng(7)
    n = 3 * H.SCAN_TILE
    for pos in range(8):
        for thread, tile in ((1, 0), (100, 1), (255, 2)):
            k, carry_k, at = H.scan_adversarial(n, tile, thread, pos, 57 + pos % 4, rng, negative=bool(pos & 1))
            prefix, _total, a, _at = H.scan_exact(k, carry_k)
            allowed = H.scan_allowed(a, H.scan_depth(n))
            good, _c = model_scan(H.scan_grid(k), H.scan_grid(carry_k))
            bad, _c = model_scan(H.scan_grid(k), H.scan_grid(carry_k), own_subtracted=True)
            assert np.all(H.scan_error(good, prefix) <= allowed), (pos, thread, tile)
            over = np.flatnonzero(H.scan_error(bad, prefix) > allowed)
            # the thread's own group up to the large value; from tile 1 on the tile's base too (the tile totals go through the same scan)
            assert over.size and (tile or at - pos in over) and np.all(over <= at) and np.all(over >= (at - pos if tile == 0 else tile * H.SCAN_TILE)), (pos, thread, tile, over)
