"""The reference of the limiter tests (tests/test_pcmlimit.py, tests/test_gpu_limit.py), never the code under test, in two forms: the
definition by brute force in Python ints, O(n^2), for short inputs; and the numpy form -- ``F = i * s + minimum.accumulate(g - i * s)``
in int64 and its mirror image, then ``min``, then ``(x * G) >> 30`` -- which tests/test_pcmlimit.py holds to the brute force first.
Quiet noise with sparse peaks as input: every case has frames at unity and frames below it.  A helper module: it holds no test."""
import numpy as np

ONE = 1 << 30
DTYPES = {1: np.int8, 2: np.int16, 4: np.int32}


def hi_of(width):
    return (1 << (8 * width - 1)) - 1


def slope(f):
    return ONE if f <= 1 else -(-ONE // f)


def reach(f):
    return -(-ONE // slope(f))


def required_gain(x, ceiling):
    """g per frame of x (n, nch) int64, as int64"""
    p = np.abs(x.astype(np.int64)).max(axis=1)
    return np.where(p <= ceiling, ONE, (ceiling * ONE) // np.maximum(p, 1)).astype(np.int64)


def gain_brute(x, ceiling, attack, release):
    """G by the definition, in Python ints: every pair of frames"""
    g = [int(v) for v in required_gain(x, ceiling)]
    s_a, s_r, n = slope(attack), slope(release), len(g)
    return [min([ONE] + [g[j] + (j - i) * s_a for j in range(i, n)] + [g[j] + (i - j) * s_r for j in range(i)]) for i in range(n)]


def gain(x, ceiling, attack, release):
    """G (n,) int64 by two prefix minima"""
    g = required_gain(x, ceiling)
    n = len(g)
    if n == 0:
        return g
    i = np.arange(n, dtype=np.int64)
    s_a, s_r = slope(attack), slope(release)
    forward = i * s_r + np.minimum.accumulate(g - i * s_r)
    backward = (np.minimum.accumulate((g + i * s_a)[::-1])[::-1]) - i * s_a
    return np.minimum(ONE, np.minimum(forward, backward))


def limit(x, ceiling, attack, release):
    """(y (n, nch) int64, G (n,) int64)"""
    G = gain(x, ceiling, attack, release)
    return (x.astype(np.int64) * G[:, None]) >> 30, G


def noise_with_peaks(rng, width, n, nch, ceiling, peaks=None, mild=False):
    """(n, nch) int64: noise of at most a quarter of the ceiling, and at `peaks` (frames; None: one in about 300, at least one where n
    allows it) a sample between the ceiling and the rails on one channel, of either sign -- `mild`: about a tenth above the ceiling at the most,
    so that the gain is back at unity within an eighth of the reach"""
    hi = hi_of(width) if not mild else min(hi_of(width), ceiling + ceiling // 10 + 1)
    quiet = max(ceiling // 4, 1)
    x = rng.integers(-quiet, quiet + 1, (n, nch), dtype=np.int64)
    if peaks is None:
        peaks = np.flatnonzero(rng.integers(0, 300, n) == 0)
        if peaks.size == 0 and n:
            peaks = np.array([int(rng.integers(0, n))])
    for i in peaks:
        v = int(rng.integers(min(ceiling + 1, hi), hi + 1))
        x[i, int(rng.integers(0, nch))] = v if rng.integers(0, 2) else -v - 1
    return x


def pcm(values, width):
    """int64 samples (any shape, frames first) as interleaved little-endian PCM bytes"""
    return np.ascontiguousarray(values).astype(DTYPES[width]).tobytes()
