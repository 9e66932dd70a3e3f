"""The four entry points of the placed-sample mixer agree with each other: a list that a lower feature level can express gives the same
track bytes through every level above it -- sh_mix_events, sh_mix_events_rate, sh_mix_events_pan (src_channels 2) and sh_mix_events_env
(seg_count 0) -- and those bytes are live ``audioop``'s (the oracle of tests/test_gpu_panned.py: ratecv, tostereo, mul, add with
saturation at every event, in list order).  Small on purpose: a stereo track of two tiles and a tail, sources of a few hundred frames."""
import audioop
import ctypes as C
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.test_gpu_panned import factors, oracle
from tests.test_gpu_sequence import OTHER_SCHEME, ROOT, _pcm

pytestmark = pytest.mark.gpu

RATE = 8192                                                # a power of two: seconds = frame / RATE is exact
FACTORS = [None, 0.5, 1.9, -1.0, 0.37, 1.9]                # None: exactly 1.0; 1.9 on sources at 0.9 of full scale saturates
SPEEDS = [0.5, 1.7, 0.999, 2.5]
PANS = [(1.0, 0.0), 0.3, (-0.5, 0.8), (1.5, 1.2), -1.0]


@functools.lru_cache(maxsize=None)
def lists(width):
    """(sources, base, A, B, C, want_A, want_B, want_C); an event is (first track SAMPLE, source, factor | None, speed | None, pan | None),
    sources 0 - 2 stereo (300, 200 and 1 frames), 3 and 4 mono (250 and 120 frames)"""
    rng = np.random.default_rng(500 + width)
    tile, lane = (2048, 8) if width == 2 else (1024, 4)
    ntrack = 2 * tile + (1002 if width == 2 else 502)      # 5098 / 2550 samples: two tiles and a tail that is no multiple of 8
    assert ntrack == (5098 if width == 2 else 2550) and ntrack % 8
    sources = [_pcm(rng, width, 2 * n, 0.9) for n in (300, 200, 1)] + [_pcm(rng, width, n, 0.9) for n in (250, 120)]
    base = _pcm(rng, width, ntrack, 0.4)
    # A: plain.  aligned; misaligned against the lane's 16 bytes (2, 4 and 6 samples off); shorter than a lane; across both tile edges; up
    # to the last track sample; ten events on tile 0 (the plain 16-bit loop: two batches of four and a remainder)
    places = [(0, 0), (18, 1), (50, 2), (100, 1), (230, 1), (310, 1), (420, 1), (512, 1), (590, 1), (622, 1), (tile - 300, 0), (2 * tile - 100, 1),
              (ntrack - 400, 1), (ntrack - 2, 2)]
    A = [(p, i, FACTORS[k % len(FACTORS)], None, None) for k, (p, i) in enumerate(places)]
    assert {p % 8 for p, *_ in A} >= {0, 2, 4, 6} and sum(1 for p, *_ in A if p < tile) >= 9
    assert any(p < tile < p + len(sources[i]) // width for p, i, *_ in A) and any(p + len(sources[i]) // width == ntrack for p, i, *_ in A)
    assert any(len(sources[i]) // width < lane for _p, i, *_ in A) and {f for _p, _i, f, *_ in A} >= {None, 0.5, 1.9}
    # B: resampled stereo events between A's; C: mono events with left / right, plain and resampled, between B's
    B = []
    for k, ev in enumerate(A):
        B.append(ev)
        if k % 2 == 0:
            speed = SPEEDS[(k // 2) % len(SPEEDS)]
            B.append(([6, 316, tile - 150, 1500, 2 * tile - 398][(k // 2) % 5], 1 if speed < 0.9 else 0, FACTORS[(k + 1) % len(FACTORS)], speed, None))
    C_ = []
    for k, ev in enumerate(B):
        C_.append(ev)
        if k % 2 == 1:
            C_.append(([4, 250, tile - 122, 1700, 2 * tile - 600, 36][(k // 2) % 6], 3 + (k // 2) % 2, FACTORS[(k + 2) % len(FACTORS)],
                       [None, 0.5, 1.7][(k // 2) % 3], PANS[(k // 2) % len(PANS)]))
    assert any(e[3] and e[3] < 1 for e in B) and any(e[3] and e[3] > 1 for e in B)
    mono = [e for e in C_ if e[4] is not None]
    assert any(e[3] is None for e in mono) and any(e[3] for e in mono) and len(A) < len(B) < len(C_)
    wants = []
    for lst in (A, B, C_):
        want = oracle(base, [(p // 2 / RATE, sources[i], f, None, sp, pan) for p, i, f, sp, pan in lst], width, RATE)
        assert len(want) == len(base)                      # every event fits: the entry points do not grow a track
        wants.append(want)
    return (sources, base, A, B, C_) + tuple(wants)


def _rows(lst, sources, width):
    """(dst_sample, nsamples, src_frames, factor, left, right, src, inrate, outrate, src_channels) per event"""
    rows = []
    for p, i, f, speed, pan in lst:
        nch = 1 if pan is not None else 2
        frames = len(sources[i]) // (width * nch)
        inrate = RATE if speed is None else int(RATE * speed)
        out_frames = frames if inrate == RATE else len(audioop.ratecv(sources[i], width, nch, inrate, RATE, None)[0]) // (width * nch)
        left, right = factors(pan) if pan is not None else (0.0, 0.0)
        rows.append((p, 2 * out_frames, frames if inrate != RATE else 0, 1.0 if f is None else f, left, right, i, inrate, RATE, nch))
    return rows


def _run(N, level, rows, bufs, base, width):
    """the track bytes after one call of the entry point of `level` on a fresh copy of base"""
    if level == "plain":
        t = np.array([(d, 0, n, f, s, 0) for d, n, _sf, f, _l, _r, s, _i, _o, _c in rows], dtype=N.MIX_EVENT_DTYPE)
    elif level == "rate":
        t = np.array([(d, 0, n, sf, f, s, i, o, 0) for d, n, sf, f, _l, _r, s, i, o, _c in rows], dtype=N.MIX_EVENT_RATE_DTYPE)
    elif level == "pan":
        t = np.array([(d, 0, n, sf, f, l, r, s, i, o, c, 0) for d, n, sf, f, l, r, s, i, o, c in rows], dtype=N.MIX_EVENT_PAN_DTYPE)
    else:
        t = np.array([(d, 0, n, sf, f, l, r, s, i, o, c, 0, 0, 0) for d, n, sf, f, l, r, s, i, o, c in rows], dtype=N.MIX_EVENT_ENV_DTYPE)
    arr = (C.c_void_p * len(bufs))(*[b.handle for b in bufs])
    track = N.DeviceBuffer.from_bytes(base)
    ns = len(base) // width
    lib = N.lib()
    if level == "plain":
        rc = lib.sh_mix_events(arr, len(bufs), t.ctypes.data, len(t), width, track.handle, ns)
    elif level == "rate":
        rc = lib.sh_mix_events_rate(arr, len(bufs), t.ctypes.data, len(t), width, 2, track.handle, ns)
    elif level == "pan":
        rc = lib.sh_mix_events_pan(arr, len(bufs), t.ctypes.data, len(t), width, track.handle, ns)
    else:
        rc = lib.sh_mix_events_env(arr, len(bufs), t.ctypes.data, len(t), None, 0, width, 2, track.handle, ns)
    assert rc == N.SH_OK, (level, lib.sh_last_error())
    return track.download_bytes(len(base))


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_the_levels_agree(gpu, width):
    N = gpu
    sources, base, A, B, C_, want_a, want_b, want_c = lists(width)
    bufs = [N.DeviceBuffer.from_bytes(b) for b in sources]
    env = [] if width == 3 else ["env"]                    # an envelope's fades have no 24-bit form
    for name, lst, want, levels in (("A", A, want_a, ["plain", "rate", "pan"] + env), ("B", B, want_b, ["rate", "pan"] + env),
                                    ("C", C_, want_c, ["pan"] + env)):
        rows = _rows(lst, sources, width)
        got = {level: _run(N, level, rows, bufs, base, width) for level in levels}
        for level in levels:
            assert got[level] == got[levels[0]], "list %s, width %d: %s differs from %s" % (name, width, level, levels[0])
            assert got[level] == want, "list %s, width %d: %s differs from audioop" % (name, width, level)
    assert want_a != base and want_b != want_a and want_c != want_b


def test_the_levels_agree_under_the_other_alignment_scheme(gpu):
    """SYNTHHIP_SEQ_ALIGN is read once per process (sh_init): the 16-bit case again in a child under the scheme that is not the default"""
    env = dict(os.environ, SYNTHHIP_SEQ_ALIGN=OTHER_SCHEME)
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        str(Path(__file__).resolve()) + "::test_the_levels_agree[2]"], cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "1 passed" in p.stdout and "failed" not in p.stdout, p.stdout[-3000:] + p.stderr[-1000:]
