"""The quantisers (csrc/pcm.hip: sh_quantize_f32, sh_quantize_f64, sh_quantize_clip_f32) through windows of larger buffers.

The 16-bit forms choose between a vector kernel (16 bytes in, 8 or 4 bytes out per load) and the one-sample kernel from the two
ADDRESSES, and cut the request into a vector part and a scalar tail; the other widths run the one-sample kernel.  Every operand
here is a DeviceBuffer.view at a chosen residue inside a sentinel-filled parent (tests/helpers.py: pcm_view_call).

Reference, not the library: the expression tests/test_gpu_osc.py and tests/test_gpu_huge.py compare against,
``np.trunc(scale * v.astype(np.float64))`` cast to the width's integer (int(scale * v) of sample.py, truncation toward zero; the
product in float64), and for the clip form ``np.where(isnan(p), 0, np.clip(np.trunc(p), -32768, 32767))``.  Byte equality.

An input parent holds 1e30 -- which no width can hold -- immediately in front of and behind the requested range: a kernel that looks
at one value outside [in_off, in_off + n) raises the overflow flag, which the call (or the next sh_overflow_check) reports.
"""
import numpy as np
import pytest

from tests.helpers import PCM_OUT_SENTINEL, pcm_view_call
from tests.test_gpu_pcm_views import _check, residues

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 3, 4, 5, 1023, 1024, 1025, 2048 + 3]
WIDTHS = [1, 2, 4]
BAD = 1.0e30
INT = {1: "<i1", 2: "<i2", 4: "<i4"}


def scale_of(width):
    return float((1 << (8 * width - 1)) - 1)


def values(ftype, width, n, seed=0):
    """n values in (-1, 1) of `ftype`; the corners 1, -1, 0, -0 and the largest value below 1 first and again at the very end"""
    rng = np.random.default_rng(100 * width + n + seed + (7 if ftype == np.float64 else 0))
    v = rng.uniform(-1.0, 1.0, n).astype(ftype)
    corners = np.array([1.0, -1.0, 0.0, -0.0, np.nextafter(ftype(1.0), ftype(0.0)), 0.5, -0.25, 1e-9], dtype=ftype)
    k = min(n, 8)
    v[:k] = corners[:k]
    if n >= 16:
        v[n - 8:] = corners[::-1]
    return v


def reference(v, width):
    return np.trunc(scale_of(width) * v.astype(np.float64)).astype(INT[width]).tobytes()


def reference_clip(v, scale):
    p = scale * v.astype(np.float64)
    return np.where(np.isnan(p), 0.0, np.clip(np.trunc(p), -32768.0, 32767.0)).astype("<i2").tobytes()


def in_residues(ftype):
    """the input window on the 16-byte grid and one value's natural alignment off it"""
    return [0, 4] if ftype == np.float32 else [0, 8]


def _entry(L, ftype):
    return L.sh_quantize_f32 if ftype == np.float32 else L.sh_quantize_f64


@pytest.mark.parametrize("ftype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("width", WIDTHS)
def test_quantize_through_windows(gpu, width, ftype):
    """the request placed by the windows, in_off = out_off = 0; 1e30 on both sides of it"""
    L = gpu.lib()
    entry = _entry(L, ftype)
    bad = np.array([BAD], dtype=ftype).tobytes()
    for n in LENGTHS:
        v = values(ftype, width, n)
        want = reference(v, width)
        for ai in in_residues(ftype):
            for ao in residues(width):
                rc, got = pcm_view_call(gpu, [(v.tobytes(), ai)], n * width, ao,
                                        lambda iv, ov: entry(iv[0].handle, 0, n, scale_of(width), width, ov.handle, 0), guards=[(bad, bad)])
                _check(rc, got, want, (width, n, ai, ao))
                assert L.sh_overflow_check() == gpu.SH_OK, (width, n, ai, ao)


@pytest.mark.parametrize("ftype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("width", WIDTHS)
def test_quantize_own_offsets(gpu, width, ftype):
    """the same ranges named by in_off / out_off inside on-grid windows: the same bytes, the output in front of out_off untouched,
    and the 1e30 at in_off - 1 and in_off + n (inside the window this time) not looked at"""
    L = gpu.lib()
    entry = _entry(L, ftype)
    size = np.dtype(ftype).itemsize
    for n in LENGTHS:
        v = values(ftype, width, n, seed=1)
        want = reference(v, width)
        for ai in in_residues(ftype):
            for ao in residues(width):
                in_off, out_off = 1 + ai // size, ao // width
                padded = np.concatenate([np.full(in_off, BAD, dtype=ftype), v, np.full(2, BAD, dtype=ftype)])
                rc, got = pcm_view_call(gpu, [(padded.tobytes(), 0)], (out_off + n) * width, 0,
                                        lambda iv, ov: entry(iv[0].handle, in_off, n, scale_of(width), width, ov.handle, out_off))
                _check(rc, got, bytes([PCM_OUT_SENTINEL]) * (out_off * width) + want, ("own offsets", width, n, in_off, out_off))
                assert L.sh_overflow_check() == gpu.SH_OK, (width, n, in_off, out_off)


@pytest.mark.parametrize("ftype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("width", WIDTHS)
def test_quantize_overflow_in_the_last_element(gpu, width, ftype):
    """1e30 as the LAST element inside the range: SH_ERR_OVERFLOW at every length and residue; a clean call after it succeeds"""
    L = gpu.lib()
    entry = _entry(L, ftype)
    for n in LENGTHS[1:]:
        v = values(ftype, width, n, seed=2)
        v[-1] = BAD
        for ai in in_residues(ftype):
            for ao in (residues(width)[0], residues(width)[1]):
                rc, _ = pcm_view_call(gpu, [(v.tobytes(), ai)], n * width, ao,
                                      lambda iv, ov: entry(iv[0].handle, 0, n, scale_of(width), width, ov.handle, 0))
                assert rc == gpu.SH_ERR_OVERFLOW, (width, n, ai, ao, rc)
                assert L.sh_overflow_check() == gpu.SH_OK, "the flag stuck"
    v = values(ftype, width, 1025, seed=3)
    rc, got = pcm_view_call(gpu, [(v.tobytes(), in_residues(ftype)[1])], 1025 * width, residues(width)[1],
                            lambda iv, ov: entry(iv[0].handle, 0, 1025, scale_of(width), width, ov.handle, 0))
    _check(rc, got, reference(v, width), ("after an overflow", width))


def test_quantize_clip_through_windows(gpu):
    """sh_quantize_clip_f32 (the real-time mixer's ring slots: multiples of nframes * bytes_per_frame, 4-byte aligned at best):
    saturates, NaN gives 0, never refuses and never raises the flag -- whatever lies around the range"""
    L = gpu.lib()
    bad = np.array([BAD], dtype=np.float32).tobytes()
    scale = 40000.0                                         # 1.0 -> 40000: beyond int16 on both sides
    for n in LENGTHS:
        v = values(np.float32, 2, n, seed=4)
        if n:
            v[n // 2] = np.float32("nan")
            v[-1] = np.float32(BAD)
        if n > 4:
            v[1], v[n - 2] = np.float32(-BAD), np.float32("inf")
        want = reference_clip(v, scale)
        if n > 8:
            assert want.count(np.int16(32767).tobytes()) and want.count(np.int16(-32768).tobytes())
        for ai in in_residues(np.float32) + [8, 12]:
            for ao in residues(2) + [4, 6]:
                rc, got = pcm_view_call(gpu, [(v.tobytes(), ai)], n * 2, ao,
                                        lambda iv, ov: L.sh_quantize_clip_f32(iv[0].handle, n, scale, ov.handle), guards=[(bad, bad)])
                _check(rc, got, want, ("clip", n, ai, ao))
                assert L.sh_overflow_check() == gpu.SH_OK, ("clip", n, ai, ao)


def test_refusals_are_checked_against_the_window(gpu):
    """a window one value shorter than the request, inside a parent that holds all of it: refused, nothing written"""
    L = gpu.lib()
    n = 40
    for ftype in (np.float32, np.float64):
        size = np.dtype(ftype).itemsize
        data = np.zeros(n, dtype=ftype).tobytes()
        for width in WIDTHS:
            call = lambda iv, ov: _entry(L, ftype)(iv[0].handle, 0, n, scale_of(width), width, ov.handle, 0)
            rc, _ = pcm_view_call(gpu, [(data, 0, size * (n - 1))], n * width, 0, call, untouched=True)
            assert rc == gpu.SH_ERR_INVALID, (ftype, width, "input short", rc)
            rc, _ = pcm_view_call(gpu, [(data, 0)], n * width, 0, call, out_view_nbytes=(n - 1) * width, untouched=True)
            assert rc == gpu.SH_ERR_INVALID, (ftype, width, "output short", rc)
            off = lambda iv, ov: _entry(L, ftype)(iv[0].handle, 1, n, scale_of(width), width, ov.handle, 0)
            rc, _ = pcm_view_call(gpu, [(data, 0)], n * width, 0, off, untouched=True)
            assert rc == gpu.SH_ERR_INVALID, (ftype, width, "in_off pushes the range out", rc)
    data = np.zeros(n, dtype=np.float32).tobytes()
    clip = lambda iv, ov: L.sh_quantize_clip_f32(iv[0].handle, n, 32767.0, ov.handle)
    rc, _ = pcm_view_call(gpu, [(data, 0, 4 * (n - 1))], 2 * n, 0, clip, untouched=True)
    assert rc == gpu.SH_ERR_INVALID
    rc, _ = pcm_view_call(gpu, [(data, 0)], 2 * n, 0, clip, out_view_nbytes=2 * (n - 1), untouched=True)
    assert rc == gpu.SH_ERR_INVALID
