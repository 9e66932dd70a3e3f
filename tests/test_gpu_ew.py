"""sh_ew_f64 (csrc/osc_scan.hip: k_ew_f64), bit for bit against numpy / Python scalar arithmetic.

Every op is one or two IEEE operations, so the comparison is equality of the uint64 views (NaN where the reference has NaN): the sign
of zero, subnormals, infinities and the largest finite values included.  AXPY is a + fl(b * p0), the product rounded first
(include/synthhip.h) -- checked on operands where a fused multiply-add gives another result.  CLIP is the oracle's own expression,
max(min(v, maximum), minimum), with Python's rule for ties and NaN (the first argument stays).  Also: element offsets on all four
operands, the three kinds of destination (float64, float32, the host through scratch) and their round-to-nearest-even float32
values, the in-place aliasing the callers use, and the refusals.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = [0, 1, 255, 256, 257, 70001]
A_OFF, B_OFF, OUT64_OFF, OUT32_OFF = 3, 5, 7, 11            # non-zero and odd
PAD = 16
SENT64 = np.float64(-1.2345678912345e300)
SENT32 = np.float32(-1.2345679e30)
DBL_MAX = np.finfo(np.float64).max
FLT_MAX = float(np.finfo(np.float32).max)

SPECIALS = np.array([
    0.0, -0.0, 5e-324, -5e-324, 2.2250738585072009e-308, -2.2250738585072009e-308, 2.2250738585072014e-308, 1e-310,
    math.inf, -math.inf, math.nan, DBL_MAX, -DBL_MAX, np.nextafter(DBL_MAX, 0.0), 0.5 * DBL_MAX,
    1.0, -1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), np.nextafter(-1.0, 0.0), np.nextafter(-1.0, -2.0),
    np.nextafter(0.0, 1.0), 0.5, -0.5, 2.0, -2.0, 1.5, 1e-300, 1e300, -1e300,
    # float32 rounding: ties (to even), just off the ties, the overflow threshold, float32 subnormals
    1.0 + 2.0 ** -24, 1.0 + 3.0 * 2.0 ** -24, np.nextafter(1.0 + 2.0 ** -24, 2.0), np.nextafter(1.0 + 2.0 ** -24, 0.0),
    FLT_MAX, FLT_MAX + 2.0 ** 103, np.nextafter(FLT_MAX + 2.0 ** 103, 0.0), -(FLT_MAX + 2.0 ** 103), 2.0 ** 128,
    2.0 ** -149, 2.0 ** -150, np.nextafter(2.0 ** -150, 1.0), 3.0 * 2.0 ** -150, 2.0 ** -126, np.nextafter(2.0 ** -126, 0.0), -2.0 ** -151,
], dtype=np.float64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want):
    """Bit-equal, NaN matching NaN (its payload is not specified)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    view = np.uint64 if got.dtype == np.float64 else np.uint32
    return np.all((np.isnan(got) & np.isnan(want)) | (got.view(view) == want.view(view)))


def _first_diff(got, want):
    view = np.uint64 if got.dtype == np.float64 else np.uint32
    bad = np.flatnonzero(~((np.isnan(got) & np.isnan(want)) | (got.view(view) == want.view(view))))
    return [(int(i), float(got[i]), float(want[i])) for i in bad[:5]], int(bad.size)


def _operands(n, seed=0):
    """a, b of n values: every pair of SPECIALS first, then random values over the whole exponent range and around +-1."""
    rng = np.random.default_rng(seed)
    m = SPECIALS.size
    a = np.repeat(SPECIALS, m)
    b = np.tile(SPECIALS, m)
    extra = max(0, 70001 - a.size)
    wide = np.ldexp(rng.uniform(1.0, 2.0, extra), rng.integers(-1070, 1024, extra)) * rng.choice([-1.0, 1.0], extra)
    near = rng.uniform(-2.0, 2.0, extra)
    a = np.concatenate([a, np.where(rng.random(extra) < 0.5, wide, near)])
    b = np.concatenate([b, np.where(rng.random(extra) < 0.5, np.roll(wide, 1), np.roll(near, 1))])
    if n == 1:
        return a[1:2].copy(), b[2:3].copy()                     # (-0.0 with 5e-324)
    return a[:n].copy(), b[:n].copy()


def _run(N, op, a, b, n, p0=0.0, p1=0.0, dest="f64"):
    """One call with odd offsets on every operand and sentinel padding around every range.  -> (out64 or None, out32 or None)."""
    L = N.lib()
    ab = N.DeviceBuffer.from_array(np.concatenate([np.full(A_OFF, SENT64), a if a is not None else [], np.full(PAD, SENT64)]))
    bb = N.DeviceBuffer.from_array(np.concatenate([np.full(B_OFF, SENT64), b if b is not None else [], np.full(PAD, SENT64)]))
    h64 = np.full(OUT64_OFF + n + PAD, SENT64)
    h32 = np.full(OUT32_OFF + n + PAD, SENT32)
    o64 = N.DeviceBuffer.from_array(h64)
    o32 = N.DeviceBuffer.from_array(h32)
    host = np.full(n + PAD, SENT32)
    use64, use32, usehost = dest in ("f64", "both"), dest in ("f32", "both"), dest == "host"
    N.check(L.sh_ew_f64(op, ab.handle if a is not None else None, A_OFF, bb.handle if b is not None else None, B_OFF, n, p0, p1,
                        o64.handle if use64 else None, OUT64_OFF, o32.handle if use32 else None, OUT32_OFF,
                        host.ctypes.data if usehost else None))
    g64 = o64.download(np.float64, h64.size)
    g32 = o32.download(np.float32, h32.size)
    for buf in (ab, bb, o64, o32):
        buf.free()
    keep64 = np.ones(h64.size, dtype=bool)
    keep32 = np.ones(h32.size, dtype=bool)
    if use64:
        keep64[OUT64_OFF:OUT64_OFF + n] = False
    if use32:
        keep32[OUT32_OFF:OUT32_OFF + n] = False
    assert np.array_equal(g64.view(np.uint64)[keep64], h64.view(np.uint64)[keep64]), "float64 destination written outside [off, off + n)"
    assert np.array_equal(g32.view(np.uint32)[keep32], h32.view(np.uint32)[keep32]), "float32 destination written outside [off, off + n)"
    assert np.array_equal(host[n:].view(np.uint32), np.full(PAD, SENT32).view(np.uint32)), "host destination written past n"
    out32 = g32[OUT32_OFF:OUT32_OFF + n] if use32 else (host[:n] if usehost else None)
    return (g64[OUT64_OFF:OUT64_OFF + n] if use64 else None), out32


def _check(N, op, a, b, want, p0=0.0, p1=0.0, what=""):
    n = want.size
    with np.errstate(all="ignore"):
        want32 = want.astype(np.float32)                        # round to nearest even; beyond FLT_MAX + half an ulp: inf
    for dest in ("f64", "f32", "both", "host"):
        g64, g32 = _run(N, op, a, b, n, p0, p1, dest)
        if g64 is not None:
            assert _same(g64, want), (what, dest, n) + _first_diff(g64, want)
        if g32 is not None:
            assert _same(g32, want32), (what, dest, n, "float32") + _first_diff(g32, want32)


@pytest.mark.parametrize("n", NS)
def test_single_ieee_operations(gpu, n):
    """ADD, MUL, ABS, COPY, FILL: one IEEE operation (or none) each."""
    N = gpu
    a, b = _operands(n)
    with np.errstate(all="ignore"):
        _check(N, N.SH_EW_ADD, a, b, a + b, what="ADD")
        _check(N, N.SH_EW_MUL, a, b, a * b, what="MUL")
        _check(N, N.SH_EW_ABS, a, None, np.abs(a), what="ABS")
        _check(N, N.SH_EW_COPY, a, None, a.copy(), what="COPY")
        for p0 in (0.0, -0.0, 1.0 + 2.0 ** -24, -DBL_MAX, 5e-324, math.inf):
            _check(N, N.SH_EW_FILL, None, None, np.full(n, p0), p0=p0, what="FILL %r" % p0)


def _fma_exact(a, b, c):
    """a * b + c rounded once (Fraction -> float is correctly rounded), for finite operands."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


@pytest.mark.parametrize("n", NS)
def test_axpy_rounds_the_product_first(gpu, n):
    """a + fl(b * p0).  The first 1000 operands are built so that a fused multiply-add answers differently: a = -fl(b * p0), where the
    unfused form gives 0 and the fused one the product's rounding error -- asserted on the CPU for at least 900 of them."""
    N = gpu
    rng = np.random.default_rng(6)
    a, b = _operands(n, seed=6)
    for p0 in (1.0 / 3.0, -0.7, 1e-3, 0.0, -0.0, math.inf, 1.0):
        m = min(n, 1000)
        b[:m] = rng.uniform(1.0, 2.0, m)
        a[:m] = -(b[:m] * p0) if math.isfinite(p0) else 1.0
        with np.errstate(all="ignore"):
            want = a + b * p0                                   # two numpy operations: the product is a float64 before the sum
        if n >= 1000 and p0 in (1.0 / 3.0, -0.7, 1e-3):
            fused = np.array([_fma_exact(float(b[i]), p0, float(a[i])) for i in range(m)])
            differ = int(np.count_nonzero(fused != want[:m]))
            assert differ >= 900, (p0, differ)
        _check(N, N.SH_EW_AXPY, a, b, want, p0=p0, what="AXPY %r" % p0)


@pytest.mark.parametrize("n", NS)
def test_nextup_is_nextafter_towards_infinity(gpu, n):
    N = gpu
    a, _b = _operands(n)
    with np.errstate(over="ignore"):
        want = np.nextafter(a, np.inf)
    _check(N, N.SH_EW_NEXTUP, a, None, want, what="NEXTUP")


def test_nextup_edges(gpu):
    N = gpu
    a = np.array([-0.0, 0.0, -5e-324, 5e-324, DBL_MAX, -DBL_MAX, math.inf, -math.inf, math.nan, 2.2250738585072009e-308,
                  -2.2250738585072014e-308, 1.0, -1.0, np.nextafter(2.0, 0.0)])
    with np.errstate(over="ignore"):
        want = np.nextafter(a, np.inf)
    assert want[0] == 5e-324 and want[1] == 5e-324 and want[4] == math.inf and want[5] == -np.nextafter(DBL_MAX, 0.0)
    assert want[9] == 2.2250738585072014e-308 and want[10] == -2.2250738585072009e-308 and want[6] == math.inf
    _check(N, N.SH_EW_NEXTUP, a, None, want, what="NEXTUP edges")


def _clip_reference(a, lo, hi):
    """ClipFilter in the oracle: max(min(v, maximum), minimum) on Python floats -- min and max keep their FIRST argument on a tie
    (-0.0 against 0.0) and when the comparison is false because of a NaN."""
    return np.array([max(min(float(v), hi), lo) for v in a], dtype=np.float64)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-0.0, 1.0), (-1.0, 0.0), (-1.0, -0.0), (-0.25, 0.75)])
def test_clip_is_the_oracles_expression(gpu, lo, hi, n):
    N = gpu
    a, _b = _operands(n, seed=2)
    if n > 300:                                                 # values straddling the limits, and the limits themselves
        edge = [lo, hi, -lo, -hi, np.nextafter(lo, -np.inf), np.nextafter(lo, np.inf), np.nextafter(hi, -np.inf), np.nextafter(hi, np.inf),
                0.0, -0.0, math.nan, -math.nan, math.inf, -math.inf]
        a[:len(edge)] = edge
    elif n == 1:
        a[0] = -0.0
    want = _clip_reference(a, lo, hi)
    _check(N, N.SH_EW_CLIP, a, None, want, p0=lo, p1=hi, what="CLIP (%r, %r)" % (lo, hi))


def test_clip_signed_zero_and_nan_by_name(gpu):
    """ClipFilter(src, 0.0, 1.0) as a half-wave rectifier: a source sample of -0.0 stays -0.0 in the oracle (min(-0.0, 1.0) = -0.0,
    max(-0.0, 0.0) = -0.0: a tie keeps the first argument) and a NaN stays NaN."""
    N = gpu
    a = np.array([-0.0, 0.0, math.nan, -1.0, 2.0, 1.0, 0.5])
    want = _clip_reference(a, 0.0, 1.0)
    assert math.copysign(1.0, want[0]) == -1.0 and math.isnan(want[2]) and list(want[3:]) == [0.0, 1.0, 1.0, 0.5]
    g64, _ = _run(N, N.SH_EW_CLIP, a, None, a.size, 0.0, 1.0, "f64")
    assert math.copysign(1.0, g64[0]) == -1.0, "clip(-0.0, 0.0, 1.0) = %r, the oracle has -0.0" % g64[0]
    assert math.isnan(g64[2]), "clip(NaN, 0.0, 1.0) = %r, the oracle has NaN" % g64[2]
    assert _same(g64, want)
    want = _clip_reference(a, -1.0, 0.0)                        # the upper limit a zero: min(0.0, -0.0)... keeps the sample's zero
    g64, _ = _run(N, N.SH_EW_CLIP, a, None, a.size, -1.0, 0.0, "f64")
    assert _same(g64, want), (g64, want)


@pytest.mark.parametrize("n", [1, 257, 70001])
def test_in_place_aliasing_as_the_callers_use_it(gpu, n):
    """AXPY with a == b == out at one offset (the FM time-step weights: m += m (w - 1)) and MUL with out == b (the gain row)."""
    N = gpu
    L = N.lib()
    rng = np.random.default_rng(n)
    m = rng.uniform(-1.0, 1.0, n + 9)
    wm1 = 2.0 ** -30 + 2.0 ** -52
    buf = N.DeviceBuffer.from_array(m)
    N.check(L.sh_ew_f64(N.SH_EW_AXPY, buf.handle, 5, buf.handle, 5, n, wm1, 0.0, buf.handle, 5, None, 0, None))
    want = m.copy()
    want[5:5 + n] = m[5:5 + n] + m[5:5 + n] * wm1
    assert np.array_equal(_bits(buf.download(np.float64, n + 9)), _bits(want))
    src = rng.uniform(-1.0, 1.0, n)
    gain = rng.uniform(0.0, 2.0, n + 3)
    sb, gb = N.DeviceBuffer.from_array(src), N.DeviceBuffer.from_array(gain)
    N.check(L.sh_ew_f64(N.SH_EW_MUL, sb.handle, 0, gb.handle, 3, n, 0.0, 0.0, gb.handle, 3, None, 0, None))
    want = gain.copy()
    want[3:] = src * gain[3:]
    assert np.array_equal(_bits(gb.download(np.float64, n + 3)), _bits(want))
    assert np.array_equal(_bits(sb.download(np.float64, n)), _bits(src))


def test_refusals(gpu):
    N = gpu
    L = N.lib()
    a = N.DeviceBuffer.from_array(np.full(100, SENT64))
    o64 = N.DeviceBuffer.from_array(np.full(100, SENT64))
    o32 = N.DeviceBuffer.from_array(np.full(100, SENT32))
    host = np.full(100, SENT32)
    INV = N.SH_ERR_INVALID
    assert L.sh_ew_f64(8, a.handle, 0, a.handle, 0, 10, 0.0, 0.0, o64.handle, 0, None, 0, None) == INV              # unknown op
    assert L.sh_ew_f64(-1, a.handle, 0, a.handle, 0, 10, 0.0, 0.0, o64.handle, 0, None, 0, None) == INV
    assert L.sh_ew_f64(N.SH_EW_COPY, a.handle, 0, None, 0, 10, 0.0, 0.0, None, 0, None, 0, None) == INV             # no destination
    assert L.sh_ew_f64(N.SH_EW_COPY, a.handle, 0, None, 0, 0, 0.0, 0.0, None, 0, None, 0, None) == INV              # ... even for n == 0
    assert L.sh_ew_f64(N.SH_EW_COPY, a.handle, 91, None, 0, 10, 0.0, 0.0, o64.handle, 0, None, 0, None) == INV      # a: 91 + 10 > 100
    assert L.sh_ew_f64(N.SH_EW_COPY, a.handle, 101, None, 0, 0, 0.0, 0.0, o64.handle, 0, None, 0, None) == INV      # a_off past the end
    assert L.sh_ew_f64(N.SH_EW_COPY, None, 0, None, 0, 10, 0.0, 0.0, o64.handle, 0, None, 0, None) == INV           # a missing
    assert L.sh_ew_f64(N.SH_EW_ADD, a.handle, 0, a.handle, 95, 10, 0.0, 0.0, o64.handle, 0, None, 0, None) == INV   # b
    assert L.sh_ew_f64(N.SH_EW_ADD, a.handle, 0, None, 0, 10, 0.0, 0.0, o64.handle, 0, None, 0, None) == INV        # b missing
    assert L.sh_ew_f64(N.SH_EW_COPY, a.handle, 0, None, 0, 10, 0.0, 0.0, o64.handle, 91, None, 0, None) == INV      # out_f64
    assert L.sh_ew_f64(N.SH_EW_COPY, a.handle, 0, None, 0, 10, 0.0, 0.0, None, 0, o32.handle, 91, None) == INV      # out_f32
    assert L.sh_ew_f64(N.SH_EW_COPY, a.handle, 0, None, 0, 10, 0.0, 0.0, o64.handle, 0, o32.handle, 91, host.ctypes.data) == INV
    assert L.sh_ew_f64(N.SH_EW_COPY, a.handle, 90, None, 0, 10, 0.0, 0.0, o64.handle, 90, o32.handle, 90, None) == N.SH_OK   # the last that fits
    assert np.array_equal(o64.download(np.float64, 90).view(np.uint64), np.full(90, SENT64).view(np.uint64))
    assert np.array_equal(o32.download(np.float32, 90).view(np.uint32), np.full(90, SENT32).view(np.uint32))
    assert np.array_equal(host.view(np.uint32), np.full(100, SENT32).view(np.uint32))
    assert L.sh_ew_f64(N.SH_EW_FILL, None, 0, None, 0, 0, 1.0, 0.0, o64.handle, 100, None, 0, None) == N.SH_OK      # n == 0 at the very end
