"""sh_mix_bus_f32 (csrc/osc_mixbus.hip: k_mix_bus_f32, k_mix_bus_direct, k_bus_sum) and sh_bus_finalize against references that do not
come from the library, on every kernel route and through windows of larger buffers.

EXACT CLASS.  Voices k 2^-a, gains j 2^-b with integers |k| <= 2^a, |j| <= 2^b and a + b = T = 24 - ceil(log2 nvoices): every product
and every partial sum of products, in any grouping, is a whole number of grid units 2^-T of magnitude at most nvoices 2^T <= 2^24 --
a float32, exactly, under fmaf and under plain additions alike.  The expected bus is the int64 sum, scaled; the comparison is of bytes.
Layout of a case (exact_case): the RIGHT gains are all +-1 with random signs, the LEFT gains random grid values with both signs and
zero; frame 0 and the last frame have every voice at sgn(right gain) (right sum exactly +nvoices: 2^24 units when nvoices is a power
of two), frame 1 the opposite (-nvoices); frames 2 and 3 have voice 0 at +1 and -1; the LAST voice is k = +-1 under a left gain of
one unit, so each of its left terms is one grid unit (except in the three full-scale frames) and dropping it from a sum shows.
tests/test_mixbus_refs.py checks these inputs without a GPU.

ROUNDED CLASS.  Uniform [-1, 1] and log-uniform [2^-40, 1] float32 inputs; S = sum g x and A = sum |g x| per output from exact
float64 products summed with two_sum per voice (vectorised; tests/test_mixbus_refs.py holds it against math.fsum), and
|got - S| <= gamma_r A + nv 2^-52 A with gamma_r = r 2^-24 / (1 - r 2^-24), r = nvoices + 8 + 32: one rounding per term, at most 7
cross-wave additions, at most 31 additions over the groups' partial buses.  Every test prints its worst |got - S| / (gamma_r A).

Every case is named for the route it takes, and the route is asserted with the CPU build of csrc/mixbus_plan.hpp
(tests/test_mixbus_plan.py: mb).  With stride > nframes the padding between the rows holds NaN, infinities and values off the grid.
"""
from collections import namedtuple

import numpy as np
import pytest

from tests.helpers import pcm_view_call
from tests.test_mixbus_plan import launches, mb, route  # noqa: F401  (mb: the fixture, tests/cpu_mixbus.cpp built with g++)

pytestmark = pytest.mark.gpu

Case = namedtuple("Case", "id nv nf stride route groups")
BIG = 1 << 24
CASES = [
    # split kernel, loops (groups: the voices of each group)
    Case("split-loop8-1group", 63, 1000, 1000, "split", (63,)),
    Case("split-loop8-2groups", 120, 1000, 1000, "split", (60, 60)),
    Case("split-loop8-4groups", 250, 1000, 1000, "split", (63, 63, 63, 61)),
    Case("split-loop41-1group", 33, 1000, 1000, "split", (33,)),
    Case("split-loop41-8groups", 257, 1024, 1024, "split", (33,) * 7 + (26,)),
    Case("split-32groups", 1024, 3000, 3000, "split", (32,) * 32),
    # split kernel, lane branches
    Case("split-ragged3-of-4", 33, 1003, 1004, "split", (33,)),
    Case("split-ragged1-of-4", 120, 1001, 1004, "split", (60, 60)),
    Case("split-ragged2-of-4", 8, 254, 256, "split", (8,)),
    Case("split-scalar-stride", 64, 4099, 4099, "split", (32, 32)),
    Case("split-wide-stride", 9, 257, 4096, "split", (9,)),
    Case("split-edge-1", 5, 1, 4, "split", (5,)),
    Case("split-edge-255", 8, 255, 256, "split", (8,)),
    Case("split-edge-256", 8, 256, 256, "split", (8,)),
    Case("split-edge-257", 9, 257, 260, "split", (9,)),
    Case("split-one-voice-one-frame", 1, 1, 1, "split", (1,)),
    Case("split-3x7", 3, 7, 7, "split", (3,)),
    Case("split-below-direct", 9, 392960, 392960, "split", (9,)),
    # direct kernel
    Case("direct-remainder-only", 3, 393216, 393216, "direct", None),
    Case("direct-no-remainder", 4, 393216, 393216, "direct", None),
    Case("direct", 9, 393216, 393216, "direct", None),
    Case("direct-ragged-smallest", 9, 392961, 392964, "direct", None),
    Case("direct-ragged", 5, 500003, 500004, "direct", None),
    Case("direct-nt", 86, 392964, 392964, "direct-nt", None),
    Case("chunked", 2, BIG + 261, BIG + 264, "chunked", None),
]
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]
# the cases that also run through windows: one or more of every route; (voices residue, bus residue) pairs
WINDOW_IDS = ["split-ragged3-of-4", "split-ragged1-of-4", "split-scalar-stride", "split-wide-stride", "split-loop8-4groups",
              "direct-ragged-smallest", "direct-nt", "chunked"]
ALL_RESIDUES = [(av, ab) for av in (0, 4, 8, 12) for ab in (0, 8)]
WINDOWS = [(cid, av, ab) for cid in WINDOW_IDS for av, ab in ALL_RESIDUES]
SURPLUS = 64
PADDING = np.array([np.nan, np.inf, -np.inf, 3.0e38, 1.0 + 2.0 ** -20, -7.25e10], dtype=np.float32)


# ---- inputs and references -----------------------------------------------------------------------------------------------------------
def grid_bits(nv):
    """(a, b, T): T = 24 - ceil(log2 nv) split between the voices and the gains"""
    T = 24 - (nv - 1).bit_length()
    a = (T + 1) // 2
    return a, T - a, T


def special_frames(nf):
    """{frame: sign} of the frames whose right sum is sign * nvoices"""
    out = {0: 1}
    if nf > 1:
        out[1] = -1
        out[nf - 1] = 1 if nf > 2 else -1
    return out


def exact_ints(nv, nf, seed):
    """(k [nv, nf] int32, j [nv, 2] int32, T): the integers of the exact class"""
    a, b, T = grid_bits(nv)
    rng = np.random.default_rng(seed)
    k = rng.integers(-(1 << a), (1 << a) + 1, (nv, nf), dtype=np.int32)
    j = np.empty((nv, 2), dtype=np.int32)
    j[:, 0] = rng.integers(-(1 << b), (1 << b) + 1, nv)
    j[:, 1] = rng.choice(np.array([-1, 1], dtype=np.int32), nv) << b
    for v, val in zip(range(nv - 1), (1 << b, -(1 << b), 0)):          # both extremes and zero among the left gains
        j[v, 0] = val
    # the last voice: +-1 under a left gain of one unit
    k[nv - 1] = rng.choice(np.array([-1, 1], dtype=np.int32), nf)
    j[nv - 1, 0] = -1 if nv % 2 else 1
    if nf > 3:
        k[0, 2], k[0, 3] = 1 << a, -(1 << a)
    for f, sign in special_frames(nf).items():
        k[:, f] = sign * np.sign(j[:, 1]) << a
    return k, j, T


def exact_sum(k, j):
    """int64 [nf, 2]: sum over the voices of k j"""
    s = np.zeros((k.shape[1], 2), dtype=np.int64)
    for v in range(k.shape[0]):
        kv = k[v].astype(np.int64)
        s[:, 0] += kv * int(j[v, 0])
        s[:, 1] += kv * int(j[v, 1])
    return s


def to_f32(ints, bits):
    f = ints.astype(np.float32)
    assert np.array_equal(f.astype(np.int64), ints)
    return np.ldexp(f, -bits)


def rows_buffer(x, stride):
    """[nv, nf] float32 -> the flat buffer of (nv - 1) stride + nf floats, PADDING between the rows"""
    nv, nf = x.shape
    if stride == nf:
        return np.ascontiguousarray(x).reshape(-1)
    full = np.empty((nv, stride), dtype=np.float32)
    full[:, :nf] = x
    full[:, nf:] = np.resize(PADDING, stride - nf)
    return full.reshape(-1)[:(nv - 1) * stride + nf].copy()


_EXACT = {}


def exact_case(c):
    """(voices buffer, gains [nv, 2], expected [nf, 2]) float32; kept, read-only, for the cases that run more than once"""
    if c.id in _EXACT:
        return _EXACT[c.id]
    a, b, T = grid_bits(c.nv)
    k, j, _ = exact_ints(c.nv, c.nf, IDS.index(c.id))
    out = (rows_buffer(to_f32(k, a), c.stride), to_f32(j, b), to_f32(exact_sum(k, j), T))
    if c.id in WINDOW_IDS:
        for arr in out:
            arr.setflags(write=False)
        _EXACT[c.id] = out
    return out


def two_sum_add(s, e, t):
    """s + t without rounding error: the rounded sum into s, what the rounding lost added to e (Knuth's two_sum), in place"""
    n = s + t
    bb = n - s
    e += (s - (n - bb)) + (t - bb)
    s[...] = n


def rounded_inputs(kind, nv, nf, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        x = rng.uniform(-1.0, 1.0, (nv, nf)).astype(np.float32)
        g = rng.uniform(-1.0, 1.0, (nv, 2)).astype(np.float32)
    else:
        x = (np.exp2(rng.uniform(-40.0, 0.0, (nv, nf))) * rng.choice([-1.0, 1.0], (nv, nf))).astype(np.float32)
        g = (np.exp2(rng.uniform(-40.0, 0.0, (nv, 2))) * rng.choice([-1.0, 1.0], (nv, 2))).astype(np.float32)
    return x, g


def rounded_reference(x, g):
    """(S, A) float64 [nf, 2].  The product of two float32 is a float64 exactly; the products are summed voice by voice with
    two_sum, the errors apart (their own sum is rounded: 2^-53 of something already 2^-53 of A), and added at the end."""
    nf = x.shape[1]
    s, e = np.zeros((4, nf)), np.zeros((4, nf))
    g64 = g.astype(np.float64)
    for v in range(x.shape[0]):
        xv = x[v].astype(np.float64)
        t = np.stack([xv * g64[v, 0], xv * g64[v, 1]])
        two_sum_add(s, e, np.concatenate([t, np.abs(t)]))
    s += e
    return np.ascontiguousarray(s[:2].T), np.ascontiguousarray(s[2:].T)


def gamma(nv):
    r = nv + 8 + 32
    return r * 2.0 ** -24 / (1.0 - r * 2.0 ** -24)


# ---- calls -----------------------------------------------------------------------------------------------------------------------------
def mix(N, buf, gains, nv, nf, stride):
    """fresh allocations: (rc, bus [nf, 2])"""
    vb, gb = N.DeviceBuffer.from_array(buf), N.DeviceBuffer.from_array(gains)
    bus = N.DeviceBuffer(nf * 8)
    try:
        rc = N.lib().sh_mix_bus_f32(vb.handle, nv, stride, nf, gb.handle, bus.handle)
        return rc, bus.download(np.float32, nf * 2).reshape(nf, 2)
    finally:
        for b in (vb, gb, bus):
            b.free()


def assert_route(mb, c, av=0, ab=0):  # noqa: F811
    ls = launches(mb, c.nv, c.nf, c.stride, av, ab)
    if av % 16 or ab % 16:
        assert all(not p["direct"] and (not p["vec"] or (p["groups"] > 1 and av % 16 == 0)) for _o, _n, p in ls), c.id
    elif c.route == "chunked":
        assert [route(p) for _o, _n, p in ls] == ["direct", "split"]
    else:
        assert [route(p) for _o, _n, p in ls] == [c.route] and ls[0][2]["vec"] == 1


def first_difference(got, want):
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    return "" if bad.size == 0 else "%d frames differ, first %d: got %r want %r" % (bad.size, bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("cid", IDS)
def test_exact_class_on_every_route(gpu, mb, cid):  # noqa: F811
    c = BY_ID[cid]
    assert_route(mb, c)
    buf, gains, want = exact_case(c)
    rc, got = mix(gpu, buf, gains, c.nv, c.nf, c.stride)
    assert rc == 0
    assert got.tobytes() == want.tobytes(), first_difference(got, want)


@pytest.mark.parametrize("kind", ["uniform", "log-uniform"])
@pytest.mark.parametrize("cid", IDS)
def test_rounded_class_within_the_counted_bound(gpu, mb, cid, kind):  # noqa: F811
    c = BY_ID[cid]
    assert_route(mb, c)
    x, g = rounded_inputs(kind, c.nv, c.nf, 1000 + IDS.index(cid))
    S, A = rounded_reference(x, g)
    rc, got = mix(gpu, rows_buffer(x, c.stride), g, c.nv, c.nf, c.stride)
    assert rc == 0
    err = np.abs(got.astype(np.float64) - S)
    assert np.all(np.isfinite(got)) and np.all(A > 0)
    ratio = float(np.max(err / (gamma(c.nv) * A)))
    print("%s %s: worst |got - S| / (gamma_r A) = %.4f (r = %d)" % (cid, kind, ratio, c.nv + 40))
    bad = np.argwhere(err > gamma(c.nv) * A + c.nv * 2.0 ** -52 * A)
    assert bad.size == 0, "%d outputs outside the bound, first (frame, channel) %s" % (len(bad), bad[0])


@pytest.mark.parametrize("cid,av,ab", WINDOWS, ids=["%s-v%d-b%d" % w for w in WINDOWS])
def test_exact_class_through_windows(gpu, mb, cid, av, ab):  # noqa: F811
    """voices, gains and bus as windows of sentinel-filled parents: the voices at residue av, the bus at ab (64 bytes longer than the
    result), the gains on and off the 16-byte grid by turns.  The bytes are those of the exact reference at every residue; the
    surplus, the guards and the input parents are untouched (pcm_view_call).  Off the grid no launch is direct (host plan)."""
    c = BY_ID[cid]
    assert_route(mb, c, av, ab)
    buf, gains, want = exact_case(c)
    L = gpu.lib()
    rc, res = pcm_view_call(gpu, [(buf.tobytes(), av), (gains.tobytes(), 8 if av in (4, 12) else 0)], c.nf * 8, ab,
                            lambda v, o: L.sh_mix_bus_f32(v[0].handle, c.nv, c.stride, c.nf, v[1].handle, o.handle), out_view_nbytes=c.nf * 8 + SURPLUS)
    assert rc == 0
    got = np.frombuffer(res, dtype=np.float32).reshape(c.nf, 2)
    assert res == want.tobytes(), first_difference(got, want)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_bus_untouched(gpu):
    L = gpu.lib()
    nv, nf, stride = 9, 257, 260
    c = Case("refusal", nv, nf, stride, "split", (9,))
    a, b, T = grid_bits(nv)
    k, j, _ = exact_ints(nv, nf, 77)
    buf, gains = rows_buffer(to_f32(k, a), stride), to_f32(j, b)
    want = to_f32(exact_sum(k, j), T)

    def run(vbytes=None, gbytes=None, obytes=None, ag=0, args=None, expect_ok=False, null=None):
        nv_, stride_, nf_ = args or (nv, stride, nf)

        def call(v, o):
            hs = [v[0].handle, v[1].handle, o.handle]
            if null is not None:
                hs[null] = None
            return L.sh_mix_bus_f32(hs[0], nv_, stride_, nf_, hs[1], hs[2])
        rc, _ = pcm_view_call(gpu, [(buf.tobytes(), 0, vbytes), (gains.tobytes(), ag, gbytes)], nf * 8, 0, call, out_view_nbytes=obytes, untouched=True)
        if expect_ok:
            assert rc == 0
        else:
            assert rc == gpu.SH_ERR_INVALID
    run(args=(nv, nf - 1, nf))                               # stride < nframes
    run(vbytes=buf.nbytes - 4)                               # one float short of (nvoices - 1) stride + nframes
    run(obytes=nf * 8 - 8)                                   # a bus one frame short
    run(gbytes=nv * 8 - 4)                                   # gains too small
    run(ag=4)                                                # gains off the 8-byte grid
    run(ag=12)
    run(args=(0, stride, nf))                                # no voices
    for null in (0, 1, 2):
        run(null=null)
    run(args=(nv, stride, 0), expect_ok=True)                # no frames: OK, nothing written
    # (and the same buffers, accepted: the refusals above are not the call's normal answer)
    rc, res = pcm_view_call(gpu, [(buf.tobytes(), 0), (gains.tobytes(), 8)], nf * 8, 0,
                            lambda v, o: L.sh_mix_bus_f32(v[0].handle, nv, stride, nf, v[1].handle, o.handle))
    assert rc == 0 and res == want.tobytes(), c.id


# ---- sh_bus_finalize ---------------------------------------------------------------------------------------------------------------------
def finalize_inputs(n, seed):
    """n float64 values: the rounding cases first (as many as fit), then uniform values over many binades"""
    f32 = np.float32
    fmax = float(np.finfo(f32).max)
    sub = 2.0 ** -149
    special = []
    for lo in (f32(1.0), np.nextafter(f32(1.0), f32(2)), f32(0.1), np.nextafter(f32(0.1), f32(1)), f32(-3.5), np.nextafter(f32(-3.5), f32(-4))):
        hi = np.nextafter(lo, f32(np.sign(lo) * np.inf))
        mid = (float(lo) + float(hi)) / 2.0                                  # halfway, exactly; lo's last bit is 0 in one case and 1 in the next
        special += [mid, np.nextafter(mid, 0.0), np.nextafter(mid, np.sign(mid) * np.inf)]
    special += [2.0 - 2.0 ** -24, 2.0 - 2.0 ** -25, -(2.0 - 2.0 ** -24), 1.0 - 2.0 ** -25, 1.0 - 2.0 ** -26, 4.0 - 2.0 ** -40]      # up into the next binade (three of them ties)
    special += [sub, 0.5 * sub, np.nextafter(0.5 * sub, 1.0), 0.75 * sub, 1.5 * sub, 2.5 * sub, -1.5 * sub, 2.0 ** -126 - 2.0 ** -150, 2.0 ** -126 - 2.0 ** -151,
                3.0 * 2.0 ** -140, 2.0 ** -200, -2.0 ** -200]                 # float32 subnormals and what rounds to them or to zero
    half = fmax + 2.0 ** 103                                                  # halfway between FLT_MAX and 2^128: to even, which is infinity
    special += [fmax, np.nextafter(half, 0.0), half, -np.nextafter(half, 0.0), -half, 1.0e39, -1.0e39, 1.0e308, np.inf, -np.inf]
    special += [0.0, -0.0, np.nan]
    special = np.array(special, dtype=np.float64)
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, n) * np.exp2(rng.integers(-30, 30, n))
    m = min(n, len(special))
    # (a single value: the halfway case above an odd neighbour)
    x[:m] = special[:m] if n > 1 else special[3:4]
    return x


@pytest.mark.parametrize("n", [1, 255, 257, 70001])
@pytest.mark.parametrize("window", [False, True])
def test_bus_finalize_rounds_to_nearest_even(gpu, n, window):
    """float64 -> float32 bit for bit against numpy's conversion (IEEE round to nearest, ties to even, overflow to infinity, gradual
    underflow); through windows the float64 input sits 8 bytes and the float32 output 4 bytes off the 16-byte grid."""
    L = gpu.lib()
    x = finalize_inputs(n, n)
    with np.errstate(over="ignore"):
        want = x.astype(np.float32)
    rc, res = pcm_view_call(gpu, [(x.tobytes(), 8 if window else 0)], n * 4, 4 if window else 0,
                            lambda v, o: L.sh_bus_finalize(v[0].handle, n, o.handle), out_view_nbytes=n * 4 + SURPLUS)
    assert rc == 0
    got = np.frombuffer(res, dtype=np.float32)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, "value %d: %r -> got %r want %r" % (bad[0], x[bad[0]], got[bad[0]], want[bad[0]])
