"""The inputs and references of tests/test_gpu_mixbus.py on their own (no GPU): the exact class is exact in float32 in every order
tried, every voice and the two channels matter to the expected bytes, the special frames are where the module says, the padding is
outside the class, and the rounded class's two_sum reference is math.fsum's."""
import math

import numpy as np
import pytest

from tests import test_gpu_mixbus as M

SMALL = [c for c in M.CASES if c.nv * c.nf <= 4_000_000]


def f32_sum(terms, order):
    """float32 running sum over axis 0 in the given order of voices: one rounded addition per step, as a loop would do it"""
    acc = np.zeros(terms.shape[1:], dtype=np.float32)
    for v in order:
        acc = acc + terms[v]
        assert acc.dtype == np.float32
    return acc


def case_ints(c):
    return M.exact_ints(c.nv, c.nf, M.IDS.index(c.id))


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.id)
def test_float32_sums_are_the_integer_sum_in_any_order(c):
    a, b, T = M.grid_bits(c.nv)
    assert a + b == T == 24 - math.ceil(math.log2(c.nv)) and c.nv << T <= 1 << 24
    k, j, _ = case_ints(c)
    assert np.abs(k).max() <= 1 << a and np.abs(j).max() <= 1 << b
    x, g = M.to_f32(k, a), M.to_f32(j, b)
    want = M.to_f32(M.exact_sum(k, j), T)
    terms = x[:, :, None] * g[:, None, :]                      # float32 products: exact, at most 2^T units each
    assert terms.dtype == np.float32 and np.array_equal(np.ldexp(terms.astype(np.float64), T), k[:, :, None].astype(np.int64) * j[:, None, :])
    rng = np.random.default_rng(c.nv)
    for order in (range(c.nv), range(c.nv - 1, -1, -1), rng.permutation(c.nv)):
        assert f32_sum(terms, order).tobytes() == want.tobytes(), c.id
    # the magnitudes any grouping can meet stay inside 2^24 units
    assert int(np.abs(k.astype(np.int64)).T.dot(np.abs(j.astype(np.int64))).max()) <= 1 << 24


@pytest.mark.parametrize("c", M.CASES, ids=lambda c: c.id)
def test_every_voice_and_both_channels_matter(c):
    a, b, T = M.grid_bits(c.nv)
    k, j, _ = case_ints(c)
    s = M.exact_sum(k, j)
    want = M.to_f32(s, T)
    assert not np.any((want == 0) & np.signbit(want))           # an exact zero is +0, as a sum from +0 gives it
    # swapping left with right
    assert M.to_f32(s[:, ::-1], T).tobytes() != want.tobytes()
    # removing one voice: the expected integers without its terms
    for v in range(c.nv):
        kv = k[v].astype(np.int64)
        without = s - np.stack([kv * int(j[v, 0]), kv * int(j[v, 1])], axis=1)
        assert M.to_f32(without, T).tobytes() != want.tobytes(), (c.id, v)
    # the special frames: +-nvoices on the right, the extremes under gain +-1 in the first frames
    for f, sign in M.special_frames(c.nf).items():
        assert s[f, 1] == sign * (c.nv << T) and np.all(np.abs(k[:, f]) == 1 << a)
    if c.nf > 5:
        assert (k[0, 2], k[0, 3]) == (1 << a, -(1 << a)) and abs(j[0, 1]) == 1 << b
    # the last voice: one grid unit per left term outside the full-scale frames; gains of both signs and zero
    rest = np.setdiff1d(np.arange(c.nf), list(M.special_frames(c.nf)) + ([2, 3] if c.nv == 1 else []))
    assert np.all(np.abs(k[c.nv - 1, rest].astype(np.int64) * int(j[c.nv - 1, 0])) == 1)
    if c.nv >= 4:
        assert {int(j[0, 0]), int(j[1, 0]), int(j[2, 0])} == {1 << b, -(1 << b), 0} and {-(1 << b), 1 << b} == set(j[:, 1].tolist())


def test_padding_is_outside_the_class_and_between_the_rows():
    c = M.BY_ID["split-wide-stride"]
    buf, gains, want = M.exact_case(c)
    assert buf.size == (c.nv - 1) * c.stride + c.nf
    rows = np.concatenate([buf, np.zeros(c.stride - c.nf, np.float32)]).reshape(c.nv, c.stride)
    pad = rows[:-1, c.nf:]
    assert np.isnan(pad).any() and np.isinf(pad).any() and np.isnan(pad[:, 0]).all()          # the float behind every row but the last: NaN
    a, _b, _T = M.grid_bits(c.nv)
    finite = pad[np.isfinite(pad)].astype(np.float64)
    assert np.all((np.ldexp(finite, a) % 1 != 0) | (np.abs(finite) > 1))
    assert np.all(np.isfinite(rows[:, :c.nf])) and np.all(np.isfinite(want))
    for cc in M.CASES:
        assert cc.stride >= cc.nf


def test_bound_terms():
    assert M.gamma(1) == 41 * 2.0 ** -24 / (1 - 41 * 2.0 ** -24) and M.gamma(1024) == 1064 * 2.0 ** -24 / (1 - 1064 * 2.0 ** -24)
    # r covers every tree the kernels form: a group's wave walks at most ceil(n / 8) of its n voices, 7 cross-wave adds, groups - 1 adds
    from tests.test_mixbus_plan import group_sizes  # noqa: F401
    for c in M.CASES:
        if c.groups:
            assert -(-max(c.groups) // 8) + 7 + len(c.groups) - 1 <= c.nv + 8 + 32 and len(c.groups) <= 32


@pytest.mark.parametrize("kind", ["uniform", "log-uniform"])
def test_two_sum_reference_is_fsum(kind):
    for nv, nf in ((1, 7), (9, 257), (250, 100), (1024, 40)):
        x, g = M.rounded_inputs(kind, nv, nf, nv)
        assert x.dtype == np.float32 and g.dtype == np.float32 and np.abs(x).max() <= 1 and np.abs(g).max() <= 1
        if kind == "log-uniform":
            assert np.abs(x).min() >= 2.0 ** -40 and np.abs(g).min() >= 2.0 ** -40 and (x < 0).any() and (x > 0).any()
        S, A = M.rounded_reference(x, g)
        for f in range(nf):
            for ch in range(2):
                terms = [float(x[v, f]) * float(g[v, ch]) for v in range(nv)]           # exact in float64
                s, a_ = math.fsum(terms), math.fsum(abs(t) for t in terms)
                # fsum is correctly rounded; two_sum's collected errors are themselves summed in float64: one ulp at the most
                assert abs(S[f, ch] - s) <= 2.0 ** -52 * abs(s) and abs(A[f, ch] - a_) <= 2.0 ** -52 * a_, (nv, f, ch)


def test_finalize_inputs_hold_what_they_promise():
    x = M.finalize_inputs(255, 255)
    with np.errstate(over="ignore"):
        y = x.astype(np.float32)
    bits = y.view(np.uint32)
    fmax = np.finfo(np.float32).max
    # halfway cases above an even and above an odd neighbour; results on both sides

    def tie(xi, yi):
        if not np.isfinite(yi) or float(yi) == xi:
            return False
        other = float(np.nextafter(yi, np.float32(np.copysign(np.inf, xi - float(yi)))))
        return np.isfinite(other) and abs(xi - float(yi)) == abs(other - xi)          # (exact in float64 for these magnitudes)
    with np.errstate(over="ignore"):
        mids = [i for i in range(255) if abs(x[i]) > 1e-30 and tie(x[i], y[i])]
    assert len(mids) >= 8 and all(bits[i] % 2 == 0 for i in mids)                # ties went to even ...
    assert any(abs(y[i]) > abs(x[i]) for i in mids) and any(abs(y[i]) < abs(x[i]) for i in mids)      # ... up and down
    assert np.any((y == 2.0) & (x < 2.0)) and np.any((y == 1.0) & (x < 1.0))                       # up into the next binade
    sub = (y != 0) & (np.abs(y) < np.finfo(np.float32).tiny)
    assert sub.sum() >= 5 and np.any((y == 0) & (x != 0)) and np.any(y == np.float32(2.0 ** -126))
    assert np.any((y == fmax) & (x > float(fmax))) and np.any(np.isposinf(y) & np.isfinite(x)) and np.any(np.isneginf(y) & np.isfinite(x))
    assert np.any(np.isnan(y)) and np.any((y == 0) & np.signbit(y) & (x == 0)) and np.any((y == 0) & ~np.signbit(y) & (x == 0))
    for n in (1, 255, 257, 70001):
        assert M.finalize_inputs(n, n).shape == (n,)
