"""The audioop-exact PCM entry points (csrc/pcm_ops.hip, sh_pcm_add of csrc/pcm.hip) through windows of larger buffers.

Which path of these kernels runs -- 16-byte vectors, the scalar tail, the all-scalar fallback, the dword or the byte-wise 24-bit
packer -- is decided by the ADDRESS the entry point is handed.  A Sample's storage is always a fresh allocation, so the Sample-level
tests only ever pass 16-byte-aligned pointers and destinations of exactly the result's size.  Here every operand is a
DeviceBuffer.view at a chosen residue mod 16 inside a sentinel-filled parent (tests/helpers.py: pcm_view_call), which asserts for
every call that the device pointer has the intended residue, that no byte outside the destination window changed and that the
inputs are untouched.

References, all on the CPU: the live audioop module; oracle.pcm_oracle.fade; Python's own float expressions written out for
modulate / pan_lfo / to_f64; exact Python integers for the sums of squares.  Every PCM comparison is byte equality.  The only
tolerance: a sum of squares that no float64 holds exactly (width 4 and raw 24-bit values once the sum reaches 2^53) is a float64 sum
of n non-negative once-rounded terms in an order of the library's choosing, so |got - exact| <= gamma * exact with
gamma = (n+1) u / (1 - (n+1) u), u = 2^-53 (Higham, Accuracy and Stability, section 4.2); below 2^53 every order of additions is
exact and equality is asserted.  (The entry points return the sum as a double, so "exact" cannot be asked of a 62-bit integer:
the width-3 cases therefore run a second set of values below 2^17, whose sums stay below 2^53 at every length and are exact on
every path.)  Lengths are the ones where a kernel changes path: V-1, V, V+1, 256 V +- 1, ... with V = 16 / width samples per
vector; 8192 +- 1 and k 8192 + r for the statistics (4 loads in flight x 256 lanes x 8 int16).
"""
import audioop
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from oracle import pcm_oracle as P
from tests.helpers import PCM_OUT_SENTINEL, pcm_view_call

pytestmark = pytest.mark.gpu

CORNERS24 = [0x7FFFFF, -0x800000, -0x7FFFFF, 0x7FFFFE, 0, -1, 3, -3]          # (tests/test_gpu_pcm24.py: CORNERS)
STATS_LENGTHS = [1, 7, 8191, 8192, 8193, 3 * 8192 + 5, 70001]
STATS_FRAMES = [1, 3, 4095, 4096, 4097, (3 * 8192 + 5) // 2, 35001]


def lo_hi(width):
    return -(1 << (8 * width - 1)), (1 << (8 * width - 1)) - 1


def encode(vals, width):
    v = np.asarray(vals, dtype=np.int64)
    if width == 3:
        u = v & 0xFFFFFF
        return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()
    return v.astype({1: "<i1", 2: "<i2", 4: "<i4"}[width]).tobytes()


def rand_vals(rng, width, n, scale=1.0):
    """n full-range values (int64), the corner values of the existing tests' _rand / CORNERS at the front and again at the very end
    (the end is where the scalar tails and the last partial 24-bit group work)."""
    lo, hi = lo_hi(width)
    v = (rng.integers(lo, hi + 1, n, dtype=np.int64) * scale).astype(np.int64)
    corners = np.array(CORNERS24 if width == 3 else [hi, lo, lo + 1, hi - 1, 0, -1, 3, -3], dtype=np.int64)
    if scale == 1.0:
        k = min(n, 8)
        v[:k] = corners[:k]
        if n >= 16:
            v[n - 8:] = corners[::-1]
    return v


def lengths(width, channel_op=False):
    V = 16 // (4 if width == 3 else width)
    ns = {0, 1, V - 1, V, V + 1, 256 * V - 1, 256 * V, 256 * V + V + 1, 3 * 256 * V + 5}
    if width == 3:
        ns |= {2, 3, 5}                                     # the four-sample groups of k_unpack24 / k_pack24
    if channel_op:
        ns |= {128 * V - 1, 128 * V, 128 * V + 1}           # 256 lanes x V / 2 frames: the channel kernels' workgroup
    return sorted(ns)


def residues(width):
    """Window offsets: 0, one sample, 8 and 16 - one sample mod 16; width 3 (any byte) also 1 and 2 mod 4."""
    return [0, 3, 8, 13, 1, 2] if width == 3 else [0, width, 8, 16 - width]


def offset_pairs(width_in, width_out=None):
    """(a_in, a_out): aligned/aligned, offset/aligned, aligned/offset, both offset at different residues; every residue on each side."""
    ri, ro = residues(width_in), residues(width_in if width_out is None else width_out)
    pairs = [(0, 0)] + [(r, 0) for r in ri[1:]] + [(0, r) for r in ro[1:]]
    for k, r in enumerate(ri[1:]):
        o = next(x for x in ro[1 + (k + 1) % (len(ro) - 1):] + ro[1:] if x % 16 != r % 16)
        pairs.append((r, o))
    return pairs


def _check(rc, got, want, what):
    assert rc == 0, (what, rc)
    if got != want:
        g, w = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
        bad = np.flatnonzero(g != w)
        raise AssertionError("%r: %d of %d bytes differ, first at byte %d (got %d, want %d)" % (what, bad.size, w.size, bad[0], g[bad[0]], w[bad[0]]))


# ---- the written-out references of the float expressions (checked on their own, without a GPU, by tests/test_pcm_view_refs.py) ----

def modulate_values(vals, mod):
    """Sample.modulate_amp's expression, written out as tests/test_gpu_sample_edit.py's oracle does: int(v * m[i % nmod])."""
    nmod = len(mod)
    return [int(v * mod[i % nmod]) for i, v in enumerate(vals)]


def pan_values(vals, nch, pan):
    """Sample.pan(lfo=...)'s expression: frame i -> int(l * (1 - p) / 2), int(r * (1 + p) / 2); a mono source feeds both sides."""
    out = []
    for i, p in enumerate(pan):
        l, r = vals[i * nch], vals[i * nch + nch - 1]
        out.append(int(l * (1 - p) / 2))
        out.append(int(r * (1 + p) / 2))
    return out


def out_of_range(values, width):
    lo, hi = lo_hi(width)
    return sum(1 for t in values if not lo <= t <= hi)


def modulate_case(width, n, nmod, overflow=False, seed=0):
    """-> (vals, mod, values): random full-range samples and factors in (-1, 1) (1.0, 0.0, -0.999, 0.5 first): no product leaves the
    range.  overflow: the LAST sample is the largest value and its factor 1.5 (nmod = n): exactly one product out of range."""
    rng = np.random.default_rng(1000 * width + n + 7 * nmod + seed)
    vals = rand_vals(rng, width, n).tolist()
    mod = rng.uniform(-1.0, 1.0, nmod)
    mod[:min(4, nmod)] = (1.0, 0.0, -0.999, 0.5)[:min(4, nmod)]
    mod = mod.tolist()
    if overflow:
        assert nmod == n and n > 0
        vals[-1], mod[-1] = lo_hi(width)[1], 1.5
    return vals, mod, modulate_values(vals, mod)


def pan_case(width, nch, n, overflow=False, seed=0):
    """-> (vals, pan, values): positions in (-1, 1) (-1.0, 1.0, 0.0, 0.999999 first): both gains lie in [0, 1].  overflow: the last
    frame holds the largest value (left; the right one 3 when stereo) at position -1.5: left = 1.25 max is out of range, right is not."""
    rng = np.random.default_rng(2000 * width + 100 * nch + n + seed)
    vals = rand_vals(rng, width, n * nch).tolist()
    pan = rng.uniform(-1.0, 1.0, n)
    pan[:min(4, n)] = (-1.0, 1.0, 0.0, 0.999999)[:min(4, n)]
    pan = pan.tolist()
    if overflow:
        assert n > 0
        vals[(n - 1) * nch] = lo_hi(width)[1]
        vals[(n - 1) * nch + nch - 1] = lo_hi(width)[1] if nch == 1 else 3
        pan[-1] = -1.5
    return vals, pan, pan_values(vals, nch, pan)


FADES = ((1, 0.9, 0.0), (0, 0.8, 0.2))                       # (fadeout, slope, offset): Sample.fadeout(.., 0.1), Sample.fadein(.., 0.2)


def fade_values(vals, fadeout, slope, offset):
    n = float(len(vals))
    return [int(v * ((1.0 - i * slope / n) if fadeout else (i * slope / n + offset))) for i, v in enumerate(vals)]


def f64_buffer(values):
    return np.asarray(values, dtype=np.float64).tobytes()


# ---- audioop's elementwise family ------------------------------------------------------------------------------------------

MUL_FACTORS = (1.5, -1.0, -0.333, 2.5)                      # 1.5 and 2.5 saturate full-range samples; two are negative
OWN_OFFSET_PAIRS_24 = [(0, 0), (3, 0), (0, 3), (3, 6), (9, 3), (6, 9)]      # sh_pcm_mul's own offsets are whole 24-bit samples


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_mul(gpu, width):
    """audioop.mul, the data placed by windows and by sh_pcm_mul's own in_off / out_off: both must give audioop's bytes."""
    L = gpu.lib()
    rng = np.random.default_rng(width)
    for n in lengths(width):
        raw = encode(rand_vals(rng, width, n), width)
        want = {f: audioop.mul(raw, width, f) for f in MUL_FACTORS}
        for f in MUL_FACTORS:
            for ai, ao in offset_pairs(width):
                rc, got = pcm_view_call(gpu, [(raw, ai)], len(raw), ao,
                                        lambda iv, ov: L.sh_pcm_mul(iv[0].handle, 0, len(raw), width, f, ov.handle, 0))
                _check(rc, got, want[f], ("views", width, n, f, ai, ao))
            for ai, ao in (OWN_OFFSET_PAIRS_24 if width == 3 else offset_pairs(width)):
                rc, got = pcm_view_call(gpu, [(b"\x33" * ai + raw, 0)], ao + len(raw), 0,
                                        lambda iv, ov: L.sh_pcm_mul(iv[0].handle, ai, len(raw), width, f, ov.handle, ao))
                _check(rc, got, bytes([PCM_OUT_SENTINEL]) * ao + want[f], ("own offsets", width, n, f, ai, ao))


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_bias(gpu, width):
    L = gpu.lib()
    rng = np.random.default_rng(10 + width)
    for n in lengths(width):
        raw = encode(rand_vals(rng, width, n), width)
        for b in (1, -1, 12345, lo_hi(width)[1]):
            want = audioop.bias(raw, width, b)
            for ai, ao in offset_pairs(width):
                rc, got = pcm_view_call(gpu, [(raw, ai)], len(raw), ao, lambda iv, ov: L.sh_pcm_bias(iv[0].handle, len(raw), width, b, ov.handle))
                _check(rc, got, want, (width, n, b, ai, ao))


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_reverse(gpu, width):
    L = gpu.lib()
    rng = np.random.default_rng(20 + width)
    for n in lengths(width):
        raw = encode(rand_vals(rng, width, n), width)
        want = audioop.reverse(raw, width)
        for ai, ao in offset_pairs(width):
            rc, got = pcm_view_call(gpu, [(raw, ai)], len(raw), ao, lambda iv, ov: L.sh_pcm_reverse(iv[0].handle, len(raw), width, ov.handle))
            _check(rc, got, want, (width, n, ai, ao))


@pytest.mark.parametrize("width", [1, 2, 4])
def test_reverse_refuses_the_same_view(gpu, width):
    L = gpu.lib()
    raw = encode(rand_vals(np.random.default_rng(width), width, 40), width)
    for a in residues(width):
        rc, _ = pcm_view_call(gpu, [(raw, a)], None, 0, lambda iv, ov: L.sh_pcm_reverse(iv[0].handle, len(raw), width, iv[0].handle))
        assert rc == gpu.SH_ERR_INVALID, (width, a, rc)          # (and pcm_view_call found the parent unchanged)


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_tomono(gpu, width):
    L = gpu.lib()
    rng = np.random.default_rng(30 + width)
    for n in lengths(width, channel_op=True):               # frames
        raw = encode(rand_vals(rng, width, 2 * n), width)
        for lf, rf in ((1.0, 1.0), (0.5, 0.25), (-1.0, 0.7)):       # (1, 1) saturates full-range frames
            want = audioop.tomono(raw, width, lf, rf)
            for ai, ao in offset_pairs(width):
                rc, got = pcm_view_call(gpu, [(raw, ai)], n * width, ao, lambda iv, ov: L.sh_pcm_tomono(iv[0].handle, n, width, lf, rf, ov.handle))
                _check(rc, got, want, (width, n, lf, rf, ai, ao))


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_tostereo(gpu, width):
    L = gpu.lib()
    rng = np.random.default_rng(40 + width)
    for n in lengths(width, channel_op=True):               # frames
        raw = encode(rand_vals(rng, width, n), width)
        for lf, rf in ((1.0, 1.0), (0.5, 0.25), (2.0, -1.0)):       # 2.0 saturates
            want = audioop.tostereo(raw, width, lf, rf)
            for ai, ao in offset_pairs(width):
                rc, got = pcm_view_call(gpu, [(raw, ai)], 2 * n * width, ao, lambda iv, ov: L.sh_pcm_tostereo(iv[0].handle, n, width, lf, rf, ov.handle))
                _check(rc, got, want, (width, n, lf, rf, ai, ao))


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_add(gpu, width):
    """audioop.add; the second operand at an offset of its own."""
    L = gpu.lib()
    rng = np.random.default_rng(50 + width)
    rs = residues(width)
    for n in lengths(width):
        a, b = encode(rand_vals(rng, width, n), width), encode(rand_vals(rng, width, n)[::-1], width)
        want = audioop.add(a, b, width)
        for k, (ai, ao) in enumerate(offset_pairs(width)):
            for ab in (rs[k % len(rs)], rs[(k + 2) % len(rs)]):
                rc, got = pcm_view_call(gpu, [(a, ai), (b, ab)], len(a), ao,
                                        lambda iv, ov: L.sh_pcm_add(iv[0].handle, 0, iv[1].handle, 0, len(a), width, ov.handle, 0))
                _check(rc, got, want, (width, n, ai, ab, ao))
        # sh_pcm_add's own offsets, each a whole number of samples (at width 3: 3, 6, 0 -- whose bitwise OR is no multiple of 3)
        rc, got = pcm_view_call(gpu, [(b"\x33" * width + a, 0), (b"\x44" * 2 * width + b, 0)], len(a), 0,
                                lambda iv, ov: L.sh_pcm_add(iv[0].handle, width, iv[1].handle, 2 * width, len(a), width, ov.handle, 0))
        _check(rc, got, want, ("own offsets", width, n))


@pytest.mark.parametrize("new_width", [1, 2, 3, 4])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_lin2lin(gpu, width, new_width):
    L = gpu.lib()
    rng = np.random.default_rng(60 + 4 * width + new_width)
    for n in sorted(set(lengths(width)) | set(lengths(new_width))):
        raw = encode(rand_vals(rng, width, n), width)
        want = audioop.lin2lin(raw, width, new_width)
        for ai, ao in offset_pairs(width, new_width):
            rc, got = pcm_view_call(gpu, [(raw, ai)], n * new_width, ao, lambda iv, ov: L.sh_pcm_lin2lin(iv[0].handle, n, width, new_width, ov.handle))
            _check(rc, got, want, (width, new_width, n, ai, ao))


# ---- the float expressions of Sample ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [1, 2, 4])
def test_fade(gpu, width):
    L = gpu.lib()
    rng = np.random.default_rng(70 + width)
    for n in lengths(width):
        raw = encode(rand_vals(rng, width, n), width)
        for fadeout, slope, offset in FADES:
            want = P.fade(raw, width, bool(fadeout), slope, offset)
            for ai, ao in offset_pairs(width):
                rc, got = pcm_view_call(gpu, [(raw, ai)], len(raw), ao,
                                        lambda iv, ov: L.sh_pcm_fade(iv[0].handle, 0, len(raw), width, fadeout, slope, offset, ov.handle, 0))
                _check(rc, got, want, (width, n, fadeout, ai, ao))


@pytest.mark.parametrize("width", [1, 2, 4])
def test_modulate(gpu, width):
    """int(v * m[i % nmod]); the float64 factors in a window of their own (offsets in multiples of 8)."""
    L = gpu.lib()
    V = 16 // width
    for n in lengths(width):
        for nmod in sorted({7, max(n, 1)}):                 # cycled (or longer than the sample), and one factor per sample
            vals, mod, values = modulate_case(width, n, nmod)
            assert out_of_range(values, width) == 0
            raw, want, m = encode(vals, width), encode(values, width), f64_buffer(mod)
            for k, (ai, ao) in enumerate(offset_pairs(width)):
                rc, got = pcm_view_call(gpu, [(raw, ai), (m, (0, 8, 24)[k % 3])], len(raw), ao,
                                        lambda iv, ov: L.sh_pcm_modulate(iv[0].handle, len(raw), width, iv[1].handle, nmod, ov.handle))
                _check(rc, got, want, (width, n, nmod, ai, ao))
    # the one out-of-range product in the last sample of the scalar tail of an off-grid window: refused; then a clean call succeeds
    n = 256 * V + V + 1
    vals, mod, values = modulate_case(width, n, n, overflow=True)
    assert out_of_range(values, width) == 1 and out_of_range(values[-1:], width) == 1
    raw, m = encode(vals, width), f64_buffer(mod)
    call = lambda iv, ov: L.sh_pcm_modulate(iv[0].handle, len(raw), width, iv[1].handle, n, ov.handle)
    rc, _ = pcm_view_call(gpu, [(raw, width), (m, 8)], len(raw), 16 - width, call)
    assert rc == gpu.SH_ERR_OVERFLOW, rc
    vals, mod, values = modulate_case(width, n, n)
    raw, m = encode(vals, width), f64_buffer(mod)
    rc, got = pcm_view_call(gpu, [(raw, width), (m, 8)], len(raw), 16 - width, call)
    _check(rc, got, encode(values, width), ("after an overflow", width))


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("width", [1, 2, 4])
def test_pan_lfo(gpu, width, nch):
    L = gpu.lib()
    V = 16 // width
    for n in lengths(width, channel_op=True):               # frames
        vals, pan, values = pan_case(width, nch, n)
        assert out_of_range(values, width) == 0
        raw, want, p = encode(vals, width), encode(values, width), f64_buffer(pan)
        for k, (ai, ao) in enumerate(offset_pairs(width)):
            rc, got = pcm_view_call(gpu, [(raw, ai), (p, (8, 0, 24)[k % 3])], 2 * n * width, ao,
                                    lambda iv, ov: L.sh_pcm_pan_lfo(iv[0].handle, n, width, nch, iv[1].handle, ov.handle))
            _check(rc, got, want, (width, nch, n, ai, ao))
    n = 256 * V + V + 1
    vals, pan, values = pan_case(width, nch, n, overflow=True)
    assert out_of_range(values, width) == 1 and out_of_range(values[-2:-1], width) == 1
    raw, p = encode(vals, width), f64_buffer(pan)
    call = lambda iv, ov: L.sh_pcm_pan_lfo(iv[0].handle, n, width, nch, iv[1].handle, ov.handle)
    rc, _ = pcm_view_call(gpu, [(raw, width), (p, 8)], 2 * n * width, 16 - width, call)
    assert rc == gpu.SH_ERR_OVERFLOW, rc
    vals, pan, values = pan_case(width, nch, n)
    raw, p = encode(vals, width), f64_buffer(pan)
    rc, got = pcm_view_call(gpu, [(raw, width), (p, 8)], 2 * n * width, 16 - width, call)
    _check(rc, got, encode(values, width), ("after an overflow", width, nch))


@pytest.mark.parametrize("width", [1, 2, 4])
def test_to_f64(gpu, width):
    """float(v) / divisor, as float64 bit patterns."""
    L = gpu.lib()
    rng = np.random.default_rng(90 + width)
    for n in lengths(width):
        vals = rand_vals(rng, width, n)
        raw = encode(vals, width)
        for divisor in (float(1 << (8 * width - 1)), float(lo_hi(width)[1]), 3.0):
            want = (vals.astype(np.float64) / np.float64(divisor)).tobytes()
            for ai in residues(width):
                for ao in (0, 8):
                    rc, got = pcm_view_call(gpu, [(raw, ai)], 8 * n, ao, lambda iv, ov: L.sh_pcm_to_f64(iv[0].handle, n, width, divisor, ov.handle))
                    _check(rc, got, want, (width, n, divisor, ai, ao))


# ---- statistics ---------------------------------------------------------------------------------------------------------------

def _assert_sumsq(got, exact, n, what):
    """exact below 2^53: integers of which every partial sum is a float64, in any order -> equality.  Otherwise the derived bound."""
    if exact < 1 << 53:
        assert Fraction(got) == exact, (what, got, exact)
    else:
        gamma = Fraction(n + 1, (1 << 53) - (n + 1))
        assert abs(Fraction(got) - exact) <= gamma * exact, (what, got, exact, float(abs(Fraction(got) - exact) / exact), float(gamma))


def _stats_sets(rng, width, n, tail_index):
    """-> [(label, values)]: full-range random values; the single largest magnitude (the most negative value, over half-scale
    noise) at index 0, at the last sample, at the first sample of the scalar tail of an aligned window; for widths 3 and 4 also
    values below 2^17, whose sum of squares is exact in float64 at every length."""
    lo = lo_hi(width)[0]
    sets = [("full", rand_vals(rng, width, n))]
    for label, at in (("first", 0), ("last", n - 1), ("tail", tail_index)):
        if at is not None and 0 <= at < n:
            v = rand_vals(rng, width, n, scale=0.5)
            v[at] = lo
            sets.append((label, v))
    if width >= 3:
        sets.append(("small", rng.integers(-(1 << 17) + 1, 1 << 17, n, dtype=np.int64)))
    return sets


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_stats(gpu, width):
    """sh_pcm_stats: audioop.max, and the sum of squares from exact Python integers.  On a window off the 16-byte grid the whole
    buffer goes through the grid-strided scalar loop of k_pcm_stats (the raw 24-bit samples through k_unpack24's byte path)."""
    L = gpu.lib()
    rng = np.random.default_rng(100 + width)
    V = 16 // (4 if width == 3 else width)
    for n in STATS_LENGTHS:
        tail = (n // V) * V
        for label, vals in _stats_sets(rng, width, n, tail if tail < n else None):
            raw = encode(vals, width)
            want_max = audioop.max(raw, width)
            exact = sum(v * v for v in vals.tolist())
            if label != "full" and label != "small":
                assert want_max == 1 << (8 * width - 1)
            for a in residues(width):
                mx, sq = C.c_uint32(12345), C.c_double(-1.0)
                rc, _ = pcm_view_call(gpu, [(raw, a)], None, 0, lambda iv, ov: L.sh_pcm_stats(iv[0].handle, len(raw), width, C.byref(mx), C.byref(sq)))
                assert rc == 0 and mx.value == want_max, (width, n, label, a, rc, mx.value, want_max)
                if width <= 2:
                    assert Fraction(sq.value) == exact, (width, n, label, a, sq.value, exact)
                else:
                    _assert_sumsq(sq.value, exact, n, (width, n, label, a))


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_stats_stereo(gpu, width):
    """sh_pcm_stats_stereo: per channel.  The extreme sits in ONE channel and the other channel is at a quarter of the level, so
    exchanged channels cannot pass."""
    L = gpu.lib()
    rng = np.random.default_rng(200 + width)
    V = 16 // (4 if width == 3 else width)
    lo = lo_hi(width)[0]
    for n in STATS_FRAMES:                                  # frames
        tail = (2 * n // V) * V // 2                        # first frame of the scalar tail of an aligned window
        sets = []
        x = rand_vals(rng, width, 2 * n)
        x[1::2] = (x[1::2] * 0.25).astype(np.int64)
        sets.append(("full", x))
        for label, at, ch in (("first L", 0, 0), ("last R", n - 1, 1), ("tail L", tail, 0), ("tail R", tail, 1)):
            if 0 <= at < n:
                x = rand_vals(rng, width, 2 * n, scale=0.5)
                x[1 - ch::2] = (x[1 - ch::2] * 0.25).astype(np.int64)
                x[2 * at + ch] = lo
                sets.append((label, x))
        if width >= 3:
            x = rng.integers(-(1 << 17) + 1, 1 << 17, 2 * n, dtype=np.int64)
            x[0::2] = x[0::2] // 4
            sets.append(("small", x))
        for label, x in sets:
            raw = encode(x, width)
            want_max = [audioop.max(encode(x[c::2], width), width) for c in range(2)]
            exact = [sum(v * v for v in x[c::2].tolist()) for c in range(2)]
            assert want_max[0] != want_max[1] and exact[0] != exact[1]
            for a in residues(width):
                mx, sq = (C.c_uint32 * 2)(12345, 12345), (C.c_double * 2)(-1.0, -1.0)
                rc, _ = pcm_view_call(gpu, [(raw, a)], None, 0, lambda iv, ov: L.sh_pcm_stats_stereo(iv[0].handle, n, width, mx, sq))
                assert rc == 0 and [mx[0], mx[1]] == want_max, (width, n, label, a, rc, [mx[0], mx[1]], want_max)
                for c in range(2):
                    if width <= 2:
                        assert Fraction(sq[c]) == exact[c], (width, n, label, a, c, sq[c], exact[c])
                    else:
                        _assert_sumsq(sq[c], exact[c], n, (width, n, label, a, c))


EVERY_WORKGROUP = 512 * 8192 + 3 * 8192 + 5                # samples: all 512 workgroups live, some with one turn more, one partial turn, a scalar tail


def _exact_sumsq(v):
    """The sum of squares of int64 values below 2^31 in magnitude as a Python integer: the squares' 32-bit halves, each summed in uint64
    (4.2 M x 2^32 < 2^64)."""
    sq = v * v
    return (int((sq >> 32).sum(dtype=np.uint64)) << 32) + int((sq & 0xFFFFFFFF).sum(dtype=np.uint64))


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("width", [2, 3, 4])
def test_stats_every_workgroup(gpu, width, nch):
    """The one kernel and its fold with every workgroup at work: 512 records (the fold's second round, b += 256), full turns of four
    loads and a partial one at width 2, a scalar tail -- on an aligned window and on one a sample off (all scalar).  "small": values
    below 2^15, the right channel at a quarter of the left's range; 4.2 M x 2^30 < 2^53, so every order of additions must return the
    exact sum -- a dropped or doubled element cannot hide.  "full": full-range values without the most negative one, which is then
    placed once, in the right (or only) channel of the first frame of an aligned window's scalar tail (the last frame where whole vectors
    leave no tail: stereo at widths 3 and 4); the bound is _assert_sumsq's."""
    L = gpu.lib()
    rng = np.random.default_rng(300 + 10 * width + nch)
    lo, hi = lo_hi(width)
    V = 16 // (4 if width == 3 else width)
    nframes = EVERY_WORKGROUP // nch
    n = nframes * nch
    small = rng.integers(-(1 << 15) + 1, 1 << 15, n, dtype=np.int64)
    small[nch - 1::nch] //= 4 if nch == 2 else 1
    full = rng.integers(lo + 1, hi + 1, n, dtype=np.int64)
    full[min(n // V * V, n - nch) + nch - 1] = lo
    for label, x in (("small", small), ("full", full)):
        raw = encode(x, width)
        exact = [_exact_sumsq(x[c::nch]) for c in range(nch)]
        want_max = [audioop.max(encode(x[c::nch], width), width) for c in range(nch)]
        if label == "small":
            assert max(exact) < 1 << 53
        else:
            assert want_max[nch - 1] == 1 << (8 * width - 1) and (nch == 1 or want_max[0] < want_max[1])
        for a in (0, width):
            mx, sq = (C.c_uint32 * 2)(12345, 12345), (C.c_double * 2)(-1.0, -1.0)
            if nch == 1:
                call = lambda iv, ov: L.sh_pcm_stats(iv[0].handle, len(raw), width, mx, sq)
            else:
                call = lambda iv, ov: L.sh_pcm_stats_stereo(iv[0].handle, nframes, width, mx, sq)
            rc, _ = pcm_view_call(gpu, [(raw, a)], None, 0, call)
            assert rc == 0 and list(mx)[:nch] == want_max, (width, nch, label, a, rc, list(mx), want_max)
            for c in range(nch):
                if width == 2:
                    assert Fraction(sq[c]) == exact[c], (width, nch, label, a, c, sq[c], exact[c])
                else:
                    _assert_sumsq(sq[c], exact[c], nframes, (width, nch, label, a, c))


# ---- refusals: bounds are the WINDOW's, not the allocation's ---------------------------------------------------------------------

def _requests(N, n=40):
    """(label, [(nbytes, sample bytes) per input], (out nbytes, out sample bytes) or None, call, the refusal's code)."""
    L = N.lib()
    INV = N.SH_ERR_INVALID
    for w in (1, 2, 3, 4):
        yield "mul/%d" % w, [(n * w, w)], (n * w, w), (lambda iv, ov, w=w: L.sh_pcm_mul(iv[0].handle, 0, n * w, w, 0.5, ov.handle, 0)), INV
        yield "bias/%d" % w, [(n * w, w)], (n * w, w), (lambda iv, ov, w=w: L.sh_pcm_bias(iv[0].handle, n * w, w, 5, ov.handle)), INV
        yield "reverse/%d" % w, [(n * w, w)], (n * w, w), (lambda iv, ov, w=w: L.sh_pcm_reverse(iv[0].handle, n * w, w, ov.handle)), INV
        yield "tomono/%d" % w, [(2 * n * w, w)], (n * w, w), (lambda iv, ov, w=w: L.sh_pcm_tomono(iv[0].handle, n, w, 0.5, 0.5, ov.handle)), INV
        yield "tostereo/%d" % w, [(n * w, w)], (2 * n * w, w), (lambda iv, ov, w=w: L.sh_pcm_tostereo(iv[0].handle, n, w, 0.5, 0.5, ov.handle)), INV
        # (sh_pcm_add reports a range outside a buffer with audioop.add's own complaint, SH_ERR_LENGTH: include/synthhip.h)
        yield "add/%d" % w, [(n * w, w), (n * w, w)], (n * w, w), (lambda iv, ov, w=w: L.sh_pcm_add(iv[0].handle, 0, iv[1].handle, 0, n * w, w, ov.handle, 0)), N.SH_ERR_LENGTH
        for nw in (1, 2, 3, 4):
            yield "lin2lin/%d/%d" % (w, nw), [(n * w, w)], (n * nw, nw), (lambda iv, ov, w=w, nw=nw: L.sh_pcm_lin2lin(iv[0].handle, n, w, nw, ov.handle)), INV
        yield "stats/%d" % w, [(n * w, w)], None, (lambda iv, ov, w=w: L.sh_pcm_stats(iv[0].handle, n * w, w, None, None)), INV
        yield "stats_stereo/%d" % w, [(2 * n * w, w)], None, (lambda iv, ov, w=w: L.sh_pcm_stats_stereo(iv[0].handle, n, w, None, None)), INV
        if w == 3:
            continue
        yield "fade/%d" % w, [(n * w, w)], (n * w, w), (lambda iv, ov, w=w: L.sh_pcm_fade(iv[0].handle, 0, n * w, w, 1, 0.9, 0.0, ov.handle, 0)), INV
        yield "modulate/%d" % w, [(n * w, w), (n * 8, 8)], (n * w, w), (lambda iv, ov, w=w: L.sh_pcm_modulate(iv[0].handle, n * w, w, iv[1].handle, n, ov.handle)), INV
        for nch in (1, 2):
            yield ("pan_lfo/%d/%d" % (w, nch), [(n * w * nch, w), (n * 8, 8)], (2 * n * w, w),
                   (lambda iv, ov, w=w, nch=nch: L.sh_pcm_pan_lfo(iv[0].handle, n, w, nch, iv[1].handle, ov.handle)), INV)
        yield "to_f64/%d" % w, [(n * w, w)], (n * 8, 8), (lambda iv, ov, w=w: L.sh_pcm_to_f64(iv[0].handle, n, w, 2.0, ov.handle)), INV


def test_refusals_are_checked_against_the_window(gpu):
    """A window one sample shorter than the request -- each input in turn, then the destination -- inside a parent that holds the
    whole request: refused, and the destination's parent still holds its sentinel everywhere."""
    for label, ins, out, call, code in _requests(gpu):
        data = [bytes(nbytes) for nbytes, _ in ins]          # zeros: no request can overflow
        out_nbytes = None if out is None else out[0]
        rc, _ = pcm_view_call(gpu, [(d, 0) for d in data], out_nbytes, 0, call)
        assert rc == 0, (label, "the whole request", rc)
        for k, (nbytes, sample) in enumerate(ins):
            short = [(d, 0, nbytes - sample if j == k else None) for j, d in enumerate(data)]
            rc, _ = pcm_view_call(gpu, short, out_nbytes, 0, call, untouched=True)
            assert rc == code, (label, "input %d short" % k, rc)
        if out is not None:
            rc, _ = pcm_view_call(gpu, [(d, 0) for d in data], out_nbytes, 0, call, out_view_nbytes=out_nbytes - out[1], untouched=True)
            assert rc == code, (label, "output short", rc)
    # the statistics leave the caller's results alone when they refuse
    L = gpu.lib()
    mx, sq = C.c_uint32(12345), C.c_double(-1.0)
    rc, _ = pcm_view_call(gpu, [(bytes(80), 0, 78)], None, 0, lambda iv, ov: L.sh_pcm_stats(iv[0].handle, 80, 2, C.byref(mx), C.byref(sq)))
    assert rc == gpu.SH_ERR_INVALID and mx.value == 12345 and sq.value == -1.0
