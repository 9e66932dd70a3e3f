"""sh_scan_f64 and sh_scan_rows_f64 (csrc/osc_scan.hip) against an exact integer reference (tests/helpers.py: scan_*).

Two classes of input.  EXACT: integer-valued doubles, |x| <= 2^20, mixed signs, an integer carry -- every partial sum in any order is
a float64, so every output and every carry must EQUAL the integer cumsum: indexing, tile bases, carries and races have no tolerance
to hide behind.  ROUNDED: values on the grid k * 2^-40, sum |k| < 2^62 -- the exact prefix is an int64, every float64 the kernels can
produce is a multiple of the grid step, and each output's error is known exactly; it must satisfy

    |got_i - exact_i| <= K * 2^-53 * A_i,     A_i = |carry_in| + sum_{j<i} |x_j|,

K = helpers.scan_depth(n) = 31 + ceil(ntiles / 256): the rounded additions on the longest path from an input to an output, counted
from the source (the count is spelled out in scan_depth's docstring; tests/test_scan_reference.py shows on the CPU that the kernels'
order of additions meets it and that a sequential sum does).  K is not fitted to what the device returns.  A_i runs over j < i only:
an exclusive sum that is built from the element's own group (`inclusive - own`, as block_exclusive_scan_256 once returned) fails the
adversarial input -- one value beyond 2^53 grid steps after a run of small ones -- and is meant to.
"""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

ROUND = H.SCAN_TILE * H.SCAN_SUMS_ROUND           # 524 288 values: one round of the tile-sum loop
NS = [0, 1, 7, 8, 9, 2047, 2048, 2049, 4101, ROUND, ROUND + 1, 1 << 20, 3 * ROUND + 77]
SENTINEL = np.float64(-1.2345678912345e300)
PAD = 24


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _scan(N, x, carry_in, want_carry=True):
    """sh_scan_f64 over x -> (out, carry_out); the output buffer is PAD doubles longer than n and that tail must stay untouched."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = x.size
    xb = N.DeviceBuffer.from_array(np.concatenate([x, np.full(PAD, SENTINEL)]))
    ob = N.DeviceBuffer.from_array(np.full(n + PAD, SENTINEL))
    carry = C.c_double(float("nan"))
    N.check(N.lib().sh_scan_f64(xb.handle, n, float(carry_in), ob.handle, C.byref(carry) if want_carry else None))
    got = ob.download(np.float64, n + PAD)
    assert np.array_equal(_bits(got[n:]), _bits(np.full(PAD, SENTINEL))), "sh_scan_f64 wrote past out[n)"
    assert np.array_equal(_bits(xb.download(np.float64, n + PAD)[:n]), _bits(x)), "sh_scan_f64 changed its input"
    xb.free()
    ob.free()
    return got[:n], carry.value


def _scan_rows(N, buf, row0, nrows, n, stride, carry, col0=0):
    """sh_scan_rows_f64 in place on a device buffer of doubles (a window from column col0 on when col0 > 0), carries on the device."""
    target = buf if col0 == 0 else buf.view(col0 * 8, buf.nbytes - col0 * 8)
    return N.lib().sh_scan_rows_f64(target.handle, row0, nrows, n, stride, carry.handle)


def _exact_class(n, rng):
    return rng.integers(-(1 << 20), (1 << 20) + 1, n, dtype=np.int64), int(rng.integers(-(1 << 30), 1 << 30))


def _check_rounded(got, got_carry, k, carry_k, depth, carry_depth, what):
    """Every element and the carry against the bound; prints the worst ratio of error to allowance before asserting."""
    prefix, total, a, a_total = H.scan_exact(k, carry_k)
    err = H.scan_error(got, prefix)
    allowed = H.scan_allowed(a, depth)
    bad = np.flatnonzero(err > allowed)
    if err.size:
        print("%s: n %d, K %d, max error %d grid steps, %d of %d outputs round (allowance > 0)" %
              (what, len(k), depth, int(err.max()), int(np.count_nonzero(allowed)), err.size))
    assert bad.size == 0, "%s: %d outputs over K u A_i, first at %d: error %d > %d grid steps" % (
        what, bad.size, bad[0], err[bad[0]], allowed[bad[0]])
    if got_carry is not None:
        cerr = int(H.scan_error([got_carry], [total])[0])
        assert cerr <= int(H.scan_allowed([a_total], carry_depth)[0]), (what, "carry", cerr)


@pytest.mark.parametrize("n", NS)
def test_scan_exact_class_equals_the_integer_cumsum(gpu, n):
    rng = np.random.default_rng(1000 + n)
    x, carry_in = _exact_class(n, rng)
    got, carry = _scan(gpu, x.astype(np.float64), carry_in)
    want = carry_in + np.concatenate([[0], np.cumsum(x)])
    assert np.array_equal(got, want[:-1].astype(np.float64))
    assert carry == float(want[-1])                         # n == 0: carry_in handed back, nothing written (the tail check in _scan)
    got2, carry2 = _scan(gpu, x.astype(np.float64), carry_in, want_carry=False)      # carry_out may be NULL
    assert np.array_equal(got2, got)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", H.SCAN_INPUT_KINDS)
def test_scan_rounded_class_stays_within_the_counted_bound(gpu, kind, n):
    rng = np.random.default_rng(2000 + n)
    k, carry_k = H.scan_inputs(kind, n, rng)
    got, carry = _scan(gpu, H.scan_grid(k), H.scan_grid(carry_k))
    _check_rounded(got, carry, k, carry_k, H.scan_depth(n), H.scan_carry_depth(n), kind)


def test_scan_adversarial_large_value_after_small_ones(gpu):
    """One value of 2^57 .. 2^60 grid steps (2^17 .. 2^20 as a float64; the prefix in front of it has 53 bits and lies 2^37 below) at
    each position 0..7 of an 8-value group, in threads 1, 2, 100 and 255 of tiles 0, 1 and 2, both signs.  The outputs in front of it,
    in its own group, have a prefix of small values: A_i gives them no allowance at all (K u A_i < one grid step), so they must be
    exact.  `inclusive - own` returns them rounded at ulp(2^57): red on the kernels as they stood."""
    rng = np.random.default_rng(7)
    n = 3 * H.SCAN_TILE + 5
    failures = []
    for pos in range(8):
        for thread in (1, 2, 100, 255):
            for tile in (0, 1, 2):
                k, carry_k, at = H.scan_adversarial(n, tile, thread, pos, 57 + (pos + thread) % 4, rng, negative=bool((pos + tile) & 1))
                got, _carry = _scan(gpu, H.scan_grid(k), H.scan_grid(carry_k))
                prefix, _total, a, _a_total = H.scan_exact(k, carry_k)
                err = H.scan_error(got, prefix)
                over = np.flatnonzero(err > H.scan_allowed(a, H.scan_depth(n)))
                if over.size:
                    failures.append((pos, thread, tile, int(over[0]), int(over.size), int(err[over].max())))
    assert not failures, "%d of 96 cases over the bound; (pos, thread, tile, first index, outputs, worst error in grid steps): %s" % (
        len(failures), failures[:6])


# ---- the rows form ---------------------------------------------------------------------------------------------------------------
ROW_KINDS = ("exact",) + H.SCAN_INPUT_KINDS


def _row_inputs(r, n, rng):
    kind = ROW_KINDS[r % len(ROW_KINDS)]
    if kind == "exact":
        x, c = _exact_class(n, rng)
        return kind, x, c, x.astype(np.float64), float(c)
    k, carry_k = H.scan_inputs(kind, n, rng)
    return kind, k, carry_k, H.scan_grid(k), float(H.scan_grid(carry_k))


def _geometries(n):
    if n <= 4101:
        return [(nrows, row0, n + extra) for nrows in (1, 3, 37) for row0 in (0, 2) for extra in (0, 1, 13)]
    # past one round of the tile-sum loop the host side of a case costs seconds: every value of each parameter once, 37 rows at the largest n
    return [(1, 2, n), (3, 0, n + 13), (37 if n == NS[-1] else 3, 2, n + 1)]


@pytest.mark.parametrize("n", NS)
def test_scan_rows_geometry_sentinels_carries_and_equality_with_the_single_form(gpu, n):
    """Rows row0 .. row0 + nrows - 1 of a matrix with row_stride >= n, in place: each row holds another class of input (exact, then the
    four rounded kinds, by row number) and a carry of its own.  Checked: every element of every row (equality / the bound), the carry
    buffer (the totals), the padding behind each row and the rows around the scanned ones (bit-identical sentinels), and bit-equality
    with sh_scan_f64 of the same row -- both forms add in the same order."""
    N = gpu
    for nrows, row0, stride in _geometries(n):
        if stride == 0:
            stride = 1                                       # n == 0 with row_stride == n: a stride of 0 is no matrix
        rng = np.random.default_rng(3000 + 7 * n + 100 * nrows + row0 + stride)
        total_rows = row0 + nrows + 1
        host = np.full(total_rows * stride, SENTINEL)
        rows = [_row_inputs(r, n, rng) for r in range(nrows)]
        for r, (_kind, _k, _c, x, _cf) in enumerate(rows):
            host[(row0 + r) * stride:(row0 + r) * stride + n] = x
        carries = np.concatenate([[cf for _kd, _k, _c, _x, cf in rows], [SENTINEL, SENTINEL]])
        buf = N.DeviceBuffer.from_array(host)
        cbuf = N.DeviceBuffer.from_array(carries)
        N.check(_scan_rows(N, buf, row0, nrows, n, stride, cbuf))
        got = buf.download(np.float64, host.size)
        got_c = cbuf.download(np.float64, nrows + 2)
        buf.free()
        cbuf.free()
        mask = np.ones(host.size, dtype=bool)
        for r in range(nrows):
            mask[(row0 + r) * stride:(row0 + r) * stride + n] = False
        assert np.array_equal(_bits(got[mask]), _bits(host[mask])), ("padding or a neighbouring row changed", n, nrows, row0, stride)
        assert np.array_equal(_bits(got_c[nrows:]), _bits(carries[nrows:])), "carry buffer written past nrows"
        if n == 0:
            assert np.array_equal(_bits(got_c), _bits(carries))
            continue
        for r, (kind, k, c, x, cf) in enumerate(rows):
            out = got[(row0 + r) * stride:(row0 + r) * stride + n]
            what = "rows n=%d nrows=%d row0=%d stride=%d row %d (%s)" % (n, nrows, row0, stride, r, kind)
            if kind == "exact":
                want = c + np.concatenate([[0], np.cumsum(k)])
                assert np.array_equal(out, want[:-1].astype(np.float64)), what
                assert got_c[r] == float(want[-1]), what
            else:
                _check_rounded(out, got_c[r], k, c, H.scan_depth(n), H.scan_carry_depth(n), what)
            if n <= 4101 or r < 5:
                single, single_carry = _scan(N, x, cf)
                assert np.array_equal(_bits(out), _bits(single)) and _bits([got_c[r]])[0] == _bits([single_carry])[0], what


def test_scan_rows_refuses_what_it_cannot_do_and_touches_nothing(gpu):
    N = gpu
    host = np.full(65536 + 8, SENTINEL)
    carries = np.full(65536 + 8, SENTINEL)
    buf = N.DeviceBuffer.from_array(host)
    cbuf = N.DeviceBuffer.from_array(carries)
    short_c = N.DeviceBuffer.from_array(carries[:2])
    assert N.lib().sh_scan_rows_f64(buf.handle, 0, 65535, 1, 1, cbuf.handle) == N.SH_OK            # the limit itself
    buf.upload(host)
    cbuf.upload(carries)
    cases = [
        ("65 536 rows", (buf, 0, 65536, 1, 1, cbuf)),
        ("rows buffer one value short", (buf, 2, 3, 13109, 13109, cbuf)),              # (2 + 3 - 1) * 13109 + 13109 = 65544 + 1
        ("row_stride below n", (buf, 0, 2, 100, 99, cbuf)),
        ("carry buffer short", (buf, 0, 3, 100, 100, short_c)),
    ]
    for what, (b, row0, nrows, n, stride, c) in cases:
        assert N.lib().sh_scan_rows_f64(b.handle, row0, nrows, n, stride, c.handle) == N.SH_ERR_INVALID, what
        assert np.array_equal(_bits(buf.download(np.float64, host.size)), _bits(host)), what
        assert np.array_equal(_bits(cbuf.download(np.float64, carries.size)), _bits(carries)), what
        assert np.array_equal(_bits(short_c.download(np.float64, 2)), _bits(carries[:2])), what
    assert N.lib().sh_scan_rows_f64(None, 0, 1, 1, 1, cbuf.handle) == N.SH_ERR_INVALID
    assert N.lib().sh_scan_rows_f64(buf.handle, 0, 1, 1, 1, None) == N.SH_ERR_INVALID
    # the single form: a buffer shorter than n values
    assert N.lib().sh_scan_f64(short_c.handle, 3, 0.0, buf.handle, None) == N.SH_ERR_INVALID
    assert N.lib().sh_scan_f64(buf.handle, 3, 0.0, short_c.handle, None) == N.SH_ERR_INVALID
    assert np.array_equal(_bits(short_c.download(np.float64, 2)), _bits(carries[:2]))


# ---- chaining ----------------------------------------------------------------------------------------------------------------------
def _cuts(n, pieces, rng):
    """Sorted cut points of [0, n) into `pieces` pieces: 1, 2047 and 2049 among them as far as they fit, the rest random."""
    fixed = {2: [1], 3: [2047, 2049], 17: [1, 2047, 2049]}[pieces]
    cuts = set(c for c in fixed if 0 < c < n)
    while len(cuts) < pieces - 1:
        cuts.add(int(rng.integers(1, n)))
    return [0] + sorted(cuts) + [n]


@pytest.mark.parametrize("n", [4101, ROUND + 2049, 3 * ROUND + 77])
def test_scan_chained_pieces_against_one_long_scan(gpu, n):
    """[0, n) in one call, then as 2, 3 and 17 pieces (cuts at 1, 2047, 2049 and at random points), each piece's carry_out fed to the
    next call.  Exact class: every piece equals its slice of the whole, and the final carries agree.  Rounded class: every piece stays
    within K u A_i with A_i over the WHOLE range in front of i and K = helpers.scan_chain_depth(pieces so far): the longest path now
    runs through the carries (an input reaches its piece's carry_out in 23 + R additions, crosses each later piece in R more, and
    enters the last through R + 8)."""
    N = gpu
    rng = np.random.default_rng(4000 + n)
    x, carry_in = _exact_class(n, rng)
    whole, whole_carry = _scan(N, x.astype(np.float64), carry_in)
    assert np.array_equal(whole, (carry_in + np.concatenate([[0], np.cumsum(x)]))[:-1].astype(np.float64))
    grid_inputs = [(kind,) + H.scan_inputs(kind, n, rng) for kind in ("modulator", "small_on_large_carry", "log_uniform")]
    for pieces in (2, 3, 17):
        cuts = _cuts(n, pieces, rng)
        carry = float(carry_in)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            got, carry = _scan(N, x[lo:hi].astype(np.float64), carry)
            assert np.array_equal(got, whole[lo:hi]), (pieces, lo, hi)
        assert carry == whole_carry, pieces
        for kind, k, carry_k in grid_inputs:
            prefix, total, a, a_total = H.scan_exact(k, carry_k)
            carry = float(H.scan_grid(carry_k))
            xs = H.scan_grid(k)
            for p, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
                got, carry = _scan(N, xs[lo:hi], carry)
                depth = H.scan_chain_depth(np.diff(cuts[:p + 2]))
                over = np.flatnonzero(H.scan_error(got, prefix[lo:hi]) > H.scan_allowed(a[lo:hi], depth))
                assert over.size == 0, (kind, pieces, lo, hi, depth, over[:4])
            carry_depth = sum(H.scan_carry_depth(hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:]))
            assert H.scan_error([carry], [total])[0] <= H.scan_allowed([a_total], min(carry_depth, 1023))[0], (kind, pieces)


@pytest.mark.parametrize("n", [4101, ROUND + 2049])
def test_scan_rows_chained_pieces_with_the_carry_left_on_the_device(gpu, n):
    """The same for the rows form: five rows (one of each class), scanned whole and as 2, 3 and 17 column ranges with the device carry
    left in place between the calls.  Exact rows: equal to the whole; rounded rows: within the chained bound; every row: bit-equal to
    sh_scan_f64 chained over the same pieces."""
    N = gpu
    rng = np.random.default_rng(5000 + n)
    nrows, stride = len(ROW_KINDS), n + 13
    rows = [_row_inputs(r, n, rng) for r in range(nrows)]
    host = np.full(nrows * stride, SENTINEL)
    for r, (_kind, _k, _c, x, _cf) in enumerate(rows):
        host[r * stride:r * stride + n] = x
    carries = np.array([cf for _kd, _k, _c, _x, cf in rows])
    for pieces in (1, 2, 3, 17):
        cuts = [0, n] if pieces == 1 else _cuts(n, pieces, rng)
        buf = N.DeviceBuffer.from_array(host)
        cbuf = N.DeviceBuffer.from_array(carries)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            N.check(_scan_rows(N, buf, 0, nrows, hi - lo, stride, cbuf, col0=lo))
        got = buf.download(np.float64, host.size).reshape(nrows, stride)
        got_c = cbuf.download(np.float64, nrows)
        buf.free()
        cbuf.free()
        assert np.array_equal(_bits(got[:, n:]), _bits(host.reshape(nrows, stride)[:, n:])), "padding changed"
        for r, (kind, k, c, x, cf) in enumerate(rows):
            if kind == "exact":
                want = c + np.concatenate([[0], np.cumsum(k)])
                assert np.array_equal(got[r, :n], want[:-1].astype(np.float64)) and got_c[r] == float(want[-1]), (pieces, r)
            else:
                prefix, total, a, a_total = H.scan_exact(k, c)
                err = H.scan_error(got[r, :n], prefix)
                for p, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
                    depth = H.scan_chain_depth(np.diff(cuts[:p + 2]))
                    assert np.all(err[lo:hi] <= H.scan_allowed(a[lo:hi], depth)), (kind, pieces, lo, hi, depth)
            carry = cf
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                single, carry = _scan(N, x[lo:hi], carry)
                assert np.array_equal(_bits(got[r, lo:hi]), _bits(single)), (kind, pieces, lo, hi)
            assert _bits([got_c[r]])[0] == _bits([carry])[0], (kind, pieces)
