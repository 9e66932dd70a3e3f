"""The reference of the convolution tests (tests/test_pcmfir.py, tests/test_gpu_convolve.py): ``numpy.convolve`` of each channel's
samples as int64 -- exact for these sizes, every partial sum below 2^53 and far below 2^63 -- and audioop's ``fbound`` written out in
numpy; full-range random PCM with both rails at the front and at the end.  A helper module: it holds no test."""
import numpy as np

DTYPES = {1: np.int8, 2: np.int16}


def lo_hi(width):
    return -(1 << (8 * width - 1)), (1 << (8 * width - 1)) - 1


def rand_vals(rng, width, n):
    """n full-range values (int64) with the rails and their neighbours at the front and again at the very end"""
    lo, hi = lo_hi(width)
    v = rng.integers(lo, hi + 1, n, dtype=np.int64)
    corners = np.array([hi, lo, lo + 1, hi - 1, 0, -1, 3, -3], dtype=np.int64)
    k = min(n, 8)
    v[:k] = corners[:k]
    if n >= 16:
        v[n - 8:] = corners[::-1]
    return v


def rand_frames(rng, width, n, nch):
    """(n, nch) int64, each channel rand_vals of its own"""
    return np.stack([rand_vals(rng, width, n) for _ in range(nch)], axis=1) if n else np.zeros((0, nch), dtype=np.int64)


def fbound(p, width):
    """audioop's fbound on float64 values: above HI gives HI, below LO + 1.0 gives LO, otherwise floor"""
    lo, hi = lo_hi(width)
    p = np.asarray(p, dtype=np.float64)
    p = np.where(p > float(hi), float(hi), np.where(p < float(lo) + 1.0, float(lo), p))
    return np.floor(p).astype(np.int64)


def sums(x, h):
    """the exact sums: x (n, nch) int64 under h (m, hch) int64, hch 1 or nch -> (n + m - 1, nch) int64 (0 frames where n == 0)"""
    n, nch = x.shape
    if n == 0:
        return np.zeros((0, nch), dtype=np.int64)
    return np.stack([np.convolve(x[:, c], h[:, c if h.shape[1] == 2 else 0]) for c in range(nch)], axis=1).astype(np.int64)


def convolve(x, h, factor, width):
    """the whole result as int64 samples (frames, nch): the exact sums, one float64 multiply each, fbound"""
    return fbound(sums(x, h).astype(np.float64) * np.float64(factor), width)


def pcm(values, width):
    """int64 samples (any shape, frames first) as interleaved little-endian PCM bytes"""
    return np.ascontiguousarray(values).astype(DTYPES[width]).tobytes()
