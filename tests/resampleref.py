"""The reference of the resample_fir tests (tests/test_pcmresample.py, tests/test_resample_fir_host.py, tests/test_gpu_resample_fir.py):
the exact sums of a rational resampler with integer taps -- zero-stuff by L, filter, keep every M-th -- in two independent forms, both
``numpy.convolve`` over int64, and audioop's ``fbound`` from tests/firref.py.  ``sums`` runs one convolution per residue of the output
frame mod L with that residue's phase ``h[p::L]``; ``sums_stuffed`` stuffs the zeros into memory and convolves once, which is only
for small cases and holds the first form.  A helper module: it holds no test."""
import numpy as np

from tests import firref


def result_frames(n, L, M):
    return -(-n * L // M)


def sums(x, h, L, M, delay):
    """x (n, nch) int64, h (m,) int64 -> the exact sums (ceil(n L / M), nch) int64"""
    n, nch = x.shape
    total = result_frames(n, L, M)
    out = np.zeros((total, nch), dtype=np.int64)
    for r in range(min(L, total)):
        p, b0 = (r * M + delay) % L, (r * M + delay) // L
        hp = np.asarray(h[p::L], dtype=np.int64)
        js = np.arange(r, total, L)
        if len(hp) == 0:
            continue
        b = b0 + M * np.arange(len(js), dtype=np.int64)               # frame j = r + L i reads conv(x, hp)[b0 + M i]
        for c in range(nch):
            full = np.convolve(x[:, c].astype(np.int64), hp)
            ok = b < len(full)
            out[js[ok], c] = full[b[ok]]
    return out


def sums_stuffed(x, h, L, M, delay):
    """the same sums with the zeros stuffed into memory and ONE convolution per channel"""
    n, nch = x.shape
    total = result_frames(n, L, M)
    out = np.zeros((total, nch), dtype=np.int64)
    idx = np.arange(total, dtype=np.int64) * M + delay
    for c in range(nch):
        u = np.zeros(n * L, dtype=np.int64)
        u[::L] = x[:, c]
        full = np.convolve(u, np.asarray(h, dtype=np.int64)) if n else np.zeros(0, dtype=np.int64)
        ok = idx < len(full)
        out[ok, c] = full[idx[ok]]
    return out


def resample(x, h, L, M, delay, factor, width, stuffed=False):
    """the whole result as int64 samples (frames, nch): the exact sums, one float64 multiply each, fbound"""
    s = (sums_stuffed if stuffed else sums)(x, h, L, M, delay)
    return firref.fbound(s.astype(np.float64) * np.float64(factor), width)


def rand_taps(rng, m):
    """m full-range int16 taps (int64) with both rails"""
    return firref.rand_vals(rng, 2, m)


def lowpass_taps(up, down, zero_crossings=16, beta=8.6):
    """the default bank's formula, restated: a Kaiser-windowed sinc cut at the lower of the two Nyquist frequencies, unity 2**14"""
    q = max(up, down)
    m = 2 * zero_crossings * q + 1
    k = np.arange(m, dtype=np.float64)
    return np.rint(2.0 ** 14 * (up / q) * np.sinc((k - (m - 1) / 2) / q) * np.kaiser(m, beta)).astype(np.int16)
