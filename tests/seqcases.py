"""What the GPU tests of the placed-sample mixer share beyond the reference (tests/seqref.py): the one packer and the one caller of the
sh_mix_events* entry points, both read off the product's level ladder (N.MIX_LEVELS); the child process under the other alignment
scheme; lists with samples in place of instruments; and the compiled songs that the compiled, tracks, meters and far-offset files render.

The modules of this family import from here, from tests.seqref and from tests.helpers, never from one another.

Adding a level: add its stage and its wrong orders to seqref.source (STEPS, MOVED) and a row to seqref.WRONG, and use event_table /
mix_events with the new N.MIX_LEVELS entry.  No new packer, caller or oracle loop."""
import audioop
import ctypes as C
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

from tests.seqref import LANE, OTHER_SCHEME, TILE, factors, mix, out_frames, pcm

ROOT = Path(__file__).resolve().parent.parent
RATE = 8192                                                 # of the songs below (a power of two: frame / RATE seconds are exact)
LOOPS = [1, 2, 3, 7, 8, 9, 65]                              # frames of a loop
STARTS = [0, 1, 5]
SPEEDS = [None, 0.1, 0.37, 0.999, 1.001, 2.5, 10]
LENGTHS = [1, 7, 8, 9, 15, 16, 17, 65]                      # frames of a region
FACTORS = [(0.75, -0.25), (1.0, 0.0), (0.5, 0.5), (0.0, 1.0), (1.5, 1.2), (1.0, 1.0), (0.3, 1.0)]      # of `channels`


# ---- tables and entry points --------------------------------------------------------------------------------------------------------------
def _level(N, level):
    return N.MIX_LEVELS[N.SEQ_LEVELS.index(level) if isinstance(level, str) else level]


def _table(dtype, rows):
    t = np.zeros(len(rows), dtype=dtype)
    for k, r in enumerate(rows):
        t[k] = tuple(r) + (0,) * (len(dtype.names) - len(r))
    return t


def event_table(N, level, rows):
    """rows: the fields of the level's event struct in order, the tail may be left out"""
    return _table(_level(N, level).dtype, rows)


def segment_table(N, rows):
    """rows: (end, origin, mul, slope, numsamples, offset, kind[, reserved])"""
    return _table(N.ENV_SEGMENT_DTYPE, rows)


def mix_events(N, level, srcs, table, segments, width, nchannels, track, track_samples):
    """one call of the level's entry point; `segments` and `nchannels` go to the entry points that take them"""
    lv = _level(N, level)
    args = [(C.c_void_p * max(1, len(srcs)))(*[b.handle for b in srcs]), len(srcs), table.ctypes.data if len(table) else None, len(table)]
    if lv.segments:
        args += [segments.ctypes.data if segments is not None and len(segments) else None, len(segments) if segments is not None else 0]
    args += [width, nchannels] if lv.nchannels else [width]
    return getattr(N.lib(), lv.entry)(*args, track.handle if track is not None else None, track_samples)


def seq_create(N, srcs, events, segments, width, nchannels, track_samples):
    arr = (C.c_void_p * max(1, len(srcs)))(*[b.handle for b in srcs])
    h = C.c_void_p()
    rc = N.lib().sh_seq_create(arr, len(srcs), events.ctypes.data if len(events) else None, len(events),
                               segments.ctypes.data if segments is not None and len(segments) else None,
                               len(segments) if segments is not None else 0, width, nchannels, track_samples, C.byref(h))
    return rc, h


def in_a_child_under_the_other_alignment_scheme(path, ids):
    """SYNTHHIP_SEQ_ALIGN is read once per process (sh_init): the named cases of the file again, in a fresh child under the scheme that is
    not the default"""
    env = dict(os.environ, SYNTHHIP_SEQ_ALIGN=OTHER_SCHEME)
    me = str(Path(path).resolve())
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider"] + [me + "::" + i for i in ids],
                       cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "%d passed" % len(ids) in p.stdout and "failed" not in p.stdout, p.stdout[-3000:] + p.stderr[-1000:]


def spy(N, monkeypatch):
    """the names of the sh_mix_events* entry points that Python calls reach from here on"""
    calls = []
    real = N.lib()

    class Spy:
        def __getattr__(self, name):
            if name.startswith("sh_mix_events"):
                calls.append(name)
            return getattr(real, name)
    monkeypatch.setattr(N, "lib", lambda: Spy())
    return calls


# ---- lists: events name an instrument by its index; instruments are (bytes, channels) ---------------------------------------------------
def sample_of(data: bytes, width, rate, nch):
    from synthesizer_amd.sample import Sample
    return Sample.from_raw_frames(data, width, rate, nch)


def named(instruments, events):
    return [(e[0], instruments[e[1]][0]) + tuple(e[2:]) for e in events]


def with_samples(samples, events):
    return [(e[0], samples[e[1]]) + tuple(e[2:]) for e in events]


def as_samples(instruments, width, rate):
    return [sample_of(b, width, rate, c) for b, c in instruments]


# ---- the song of the plain file, which the sampler's and the panned one's build on ------------------------------------------------------
SONG_RATE, SONG_NCH = 48000, 2
VOLUMES = [1.0, 1.0, 0.5, 0.8, -1.0, 0.0, 1.7]


def hits_song(nevents=3000, span=20.0):
    rng = np.random.default_rng(0)
    instruments = []
    for seconds in (0.05, 0.12, 0.25, 0.4):
        n = int(SONG_RATE * seconds)
        decay = np.exp(-3.0 * np.arange(n) / n)[:, None]
        noise = rng.uniform(-1.0, 1.0, (n, SONG_NCH))
        instruments.append((noise * decay * 0.5 * 32767).astype("<i2").tobytes())
    starts = rng.integers(0, int(SONG_RATE * span), nevents) / SONG_RATE
    starts[:50] = starts[0]
    which = rng.integers(0, 4, nevents)
    volumes = rng.choice(VOLUMES, nevents)
    return instruments, [(float(starts[k]), int(which[k]), float(volumes[k])) for k in range(nevents)]


# ---- the shaped notes of the envelope file, which the loop file plays unlooped -------------------------------------------------------------
SHAPED_RATE = 8000
_SHAPED = {}


def shaped_notes(width, nch, seed=0, scale=0.6):
    """(instruments, events): instruments are (bytes, channels) -- mono ones first, then (a stereo track) stereo ones; events are (seconds,
    instrument, volume, other_seconds, speed, pan, envelope), 64 of them going twice through the 32 on/off patterns of envelope, speed,
    pan, volume and other_seconds (a mono track has no pan: 16 patterns, four times), the envelopes 4-tuples and 5-tuples in turn, their
    times odd fractions of the note, and then the edge shapes.  Made once per (width, nch, seed, scale) and never changed."""
    key = (width, nch, seed, scale)
    if key in _SHAPED:
        return _SHAPED[key]
    rate = SHAPED_RATE
    speeds = [0.5, 2 ** (3 / 12), 0.8, 2.0, 1.5, 2 ** (-5 / 12)]
    vols = [0.5, 1.7, -1.0, 0.8, 1.9, -1.3]
    pans = [0.3, (1.0, 0.0), -0.65, (-0.5, 0.8), (1.5, 1.2), 1.0]
    levels = [0.5, 0.7, 1.0, 0.0, 0.25, 0.93]
    rng = np.random.default_rng(1000 * seed + 10 * width + nch)
    track_frames = 4 * TILE[width] // nch
    lengths = [400, 800, 1203, 1600] + ([3200] if width == 2 else [])      # frames: 0.05 - 0.2 s; a 16-bit track has room for 0.4 s as well
    instruments = [(pcm(rng, width, n, scale), 1) for n in lengths]
    if nch == 2:
        instruments += [(pcm(rng, width, 2 * n, scale), 2) for n in lengths]
    events = []

    def add(k, env_on, speed_on, pan_on, vol_on, cut_on, env=None, which=None, frame=None):
        speed = speeds[k % len(speeds)] if speed_on else None
        i = (k + k // 32) % len(lengths) if which is None else which
        out = out_frames(lengths[i], int(rate * speed), rate) if speed else lengths[i]
        if out > track_frames * 3 // 4:                     # too long for this track at this speed: the shortest instrument
            i = 0
            out = out_frames(lengths[0], int(rate * speed), rate) if speed else lengths[0]
        if env_on and env is None:
            dur = out / rate
            level = levels[k % len(levels)]
            if (k // 32) % 2:                               # a note length: the release ends the note before the instrument does
                dur = 0.61 * dur
                env = (0.113 * dur, 0.171 * dur, level, 0.233 * dur, dur)
            else:
                env = (0.113 * dur, 0.171 * dur, level, 0.233 * dur)
        if env is not None and len(env) == 5:
            out = min(out, int(rate * env[4]))
        cut = 0.37 * out / rate if cut_on else None
        if frame is None:
            frame = int(rng.integers(0, track_frames - out + 1))
        pan = pans[k % len(pans)] if pan_on else None
        events.append((frame / rate, i + (len(lengths) if nch == 2 and pan is None else 0), vols[k % len(vols)] if vol_on else None, cut, speed, pan, env))

    for k in range(64):
        add(k, k & 1, k & 2, (k & 4) and nch == 2, k & 8, k & 16)
    # the edge shapes: an attack part whose duration rounds a frame down (an unfaded frame at its tail: 8000 * (1001 / 8000) < 1001), an
    # attack longer than the note, a level of 0, an envelope that does nothing, a sustain level alone, no release, across a tile edge
    assert int(rate * (1001 * width / rate / width)) == 1000
    add(64, 1, 0, nch == 2, 1, 0, env=(1001.5 / rate, 0.01, 0.5, 0.01), which=2)
    add(65, 1, 0, 0, 0, 0, env=(1.0, 0.0, 1.0, 0.0), which=0)
    add(66, 1, 1, nch == 2, 0, 0, env=(0.004, 0.003, 0.0, 0.0), which=1)
    add(67, 1, 0, 0, 1, 0, env=(0.0, 0.0, 1.0, 0.0), which=1)
    add(68, 1, 0, 0, 0, 1, env=(0.0, 0.0, 0.37, 0.0), which=3)
    add(69, 1, 1, 0, 1, 0, env=(0.013, 0.0, 0.8, 0.0, 0.031), which=0)
    add(70, 1, 0, nch == 2, 0, 0, env=(0.0201, 0.0107, 0.6, 0.0153), which=1, frame=TILE[width] // nch - 215)
    _SHAPED[key] = (instruments, events)
    return _SHAPED[key]


# ---- lists that a lower level can express, through the levels above it -----------------------------------------------------------------------
LEVEL_ROW = ("dst_sample", "nsamples", "src_frames", "factor", "left", "right", "src", "inrate", "outrate", "src_channels")


@functools.lru_cache(maxsize=None)
def lists(width):
    """(sources, base, A, B, C, want_A, want_B, want_C); an event is (first track SAMPLE, source, factor | None, speed | None, pan | None),
    sources 0 - 2 stereo (300, 200 and 1 frames), 3 and 4 mono (250 and 120 frames); the track is stereo"""
    factors_ = [None, 0.5, 1.9, -1.0, 0.37, 1.9]            # None: exactly 1.0; 1.9 on sources at 0.9 of full scale saturates
    speeds = [0.5, 1.7, 0.999, 2.5]
    pans = [(1.0, 0.0), 0.3, (-0.5, 0.8), (1.5, 1.2), -1.0]
    rng = np.random.default_rng(500 + width)
    tile, lane = TILE[width], LANE[width]
    ntrack = 2 * tile + (1002 if width == 2 else 502)      # 5098 / 2550 samples: two tiles and a tail that is no multiple of 8
    assert ntrack == (5098 if width == 2 else 2550) and ntrack % 8
    sources = [pcm(rng, width, 2 * n, 0.9) for n in (300, 200, 1)] + [pcm(rng, width, n, 0.9) for n in (250, 120)]
    base = pcm(rng, width, ntrack, 0.4)
    # A: plain.  aligned; misaligned against the lane's 16 bytes (2, 4 and 6 samples off); shorter than a lane; across both tile edges; up
    # to the last track sample; ten events on tile 0 (the plain 16-bit loop: two batches of four and a remainder)
    places = [(0, 0), (18, 1), (50, 2), (100, 1), (230, 1), (310, 1), (420, 1), (512, 1), (590, 1), (622, 1), (tile - 300, 0), (2 * tile - 100, 1),
              (ntrack - 400, 1), (ntrack - 2, 2)]
    A = [(p, i, factors_[k % len(factors_)], None, None) for k, (p, i) in enumerate(places)]
    assert {p % 8 for p, *_ in A} >= {0, 2, 4, 6} and sum(1 for p, *_ in A if p < tile) >= 9
    assert any(p < tile < p + len(sources[i]) // width for p, i, *_ in A) and any(p + len(sources[i]) // width == ntrack for p, i, *_ in A)
    assert any(len(sources[i]) // width < lane for _p, i, *_ in A) and {f for _p, _i, f, *_ in A} >= {None, 0.5, 1.9}
    # B: resampled stereo events between A's; C: mono events with left / right, plain and resampled, between B's
    B = []
    for k, ev in enumerate(A):
        B.append(ev)
        if k % 2 == 0:
            speed = speeds[(k // 2) % len(speeds)]
            B.append(([6, 316, tile - 150, 1500, 2 * tile - 398][(k // 2) % 5], 1 if speed < 0.9 else 0, factors_[(k + 1) % len(factors_)], speed, None))
    C_ = []
    for k, ev in enumerate(B):
        C_.append(ev)
        if k % 2 == 1:
            C_.append(([4, 250, tile - 122, 1700, 2 * tile - 600, 36][(k // 2) % 6], 3 + (k // 2) % 2, factors_[(k + 2) % len(factors_)],
                       [None, 0.5, 1.7][(k // 2) % 3], pans[(k // 2) % len(pans)]))
    assert any(e[3] and e[3] < 1 for e in B) and any(e[3] and e[3] > 1 for e in B)
    mono = [e for e in C_ if e[4] is not None]
    assert any(e[3] is None for e in mono) and any(e[3] for e in mono) and len(A) < len(B) < len(C_)
    wants = []
    for lst in (A, B, C_):
        want = mix(base, [(p // 2 / RATE, sources[i], f, None, sp, pan) for p, i, f, sp, pan in lst], width, RATE, 2)
        assert len(want) == len(base)                      # every event fits: the entry points do not grow a track
        wants.append(want)
    return (sources, base, A, B, C_) + tuple(wants)


def rows_of(lst, sources, width):
    """LEVEL_ROW per event of one of the lists"""
    rows = []
    for p, i, f, speed, pan in lst:
        nch = 1 if pan is not None else 2
        frames = len(sources[i]) // (width * nch)
        inrate = RATE if speed is None else int(RATE * speed)
        out = frames if inrate == RATE else len(audioop.ratecv(sources[i], width, nch, inrate, RATE, None)[0]) // (width * nch)
        left, right = factors(pan) if pan is not None else (0.0, 0.0)
        rows.append((p, 2 * out, frames if inrate != RATE else 0, 1.0 if f is None else f, left, right, i, inrate, RATE, nch))
    return rows


def call_level(N, level, rows, bufs, width, track, track_samples):
    """one call of the entry point of `level` on the stereo `track`: the rows in that level's layout -- the columns it has, the rest zero"""
    t = np.zeros(len(rows), dtype=_level(N, level).dtype)
    for name, column in zip(LEVEL_ROW, zip(*rows)):
        if name in t.dtype.names:
            t[name] = column
    return mix_events(N, level, bufs, t, None, width, 2, track, track_samples)


# ---- the compiled songs: one list per feature level ------------------------------------------------------------------------------------------
LEVELS = ["plain", "rate", "pan", "env", "loop", "rev", "downmix", "balance"]       # the last two: CHAN into a mono and in a stereo song
LEVEL_NAME = {"downmix": "chan", "balance": "chan"}
HELD = (600, 300, 97)                                       # frames: a loud instrument and two of the siblings' sizes
assert {2.5, 0.37, 1.001, 0.999} <= set(SPEEDS) and {9, 65} <= set(LOOPS) and 65 in LENGTHS


def _nch(level):
    return 2 if level in ("pan", "balance") else 1


def _ev(frame, inst, volume=None, other_frames=None, speed=None, pan=None, envelope=None, loop=None, region=None, reverse=None, channels=None):
    return (frame / RATE, inst, volume, None if other_frames is None else other_frames / RATE, speed, pan, envelope, loop, region, reverse, channels)


def _envelope(out):
    dur = (0.61 * out + 0.37) / RATE                        # the siblings' proportions: attack, decay, a sustain, a release that ends the note
    return (0.113 * dur, 0.171 * dur, 0.5, 0.233 * dur, dur)


def _stage(level, k, width):
    """what stage event k (0: at the song's start, 1: across the pile-up window's start, 2: in tile 3, 3: inside the pile-up) carries"""
    if level == "plain":
        return {}
    if level == "rate":
        return dict(speed=[2.5, 0.37, 1.001, 0.999][k])
    if level == "pan":
        return dict(pan=[0.3, (1.5, 1.2), -1.0, (1.0, 1.0)][k], speed=0.37 if k == 1 else None)
    if level == "env":
        return dict(envelope=_envelope([300, 300, 300, 200][k]))
    if level == "loop":
        return dict(loop=[(230 / RATE, 295 / RATE, 350 / RATE), (5 / RATE, 70 / RATE, 260 / RATE), (1 / RATE, 10 / RATE, 400 / RATE), (0.0, 9 / RATE, 700 / RATE)][k],
                    speed=2.5 if k == 0 else None)
    if level == "rev":
        return dict(reverse=True, region=(12 / RATE, 250 / RATE) if k == 0 else None, loop=(5 / RATE, 70 / RATE, 260 / RATE) if k == 1 else None)
    kw = dict(channels=FACTORS[[0, 4, 6, 5][k]], speed=0.37 if k == 1 else None, reverse=k == 2)
    if width != 3 and k == 1:
        kw["envelope"] = _envelope(out_frames(HELD[2], int(RATE * 0.37), RATE))
    return kw


@functools.lru_cache(maxsize=None)
def song(level, width):
    """(instruments as (bytes, channels), events, nch, expected bytes of the whole song, total samples), made once"""
    nch = _nch(level)
    T, L = TILE[width], LANE[width]
    F = T // nch
    src_ch = 2 if level in ("downmix", "balance") else 1 if level == "pan" else nch
    rng = np.random.default_rng(100 * LEVELS.index(level) + 10 + width)
    instruments = [(pcm(rng, width, HELD[0] * src_ch, 1.0), src_ch), (pcm(rng, width, HELD[1] * src_ch, 0.6), src_ch),
                   (pcm(rng, width, HELD[2] * src_ch, 0.6), src_ch)]
    rest = {"pan": dict(pan=(1.0, 1.0)), "downmix": dict(channels=(1.0, 1.0))}.get(level, {})      # what every other row needs to be legal
    w0 = (T + 3 * L) // nch                                 # the frame the pile-up window starts on
    tail = (37 * L + 3) // nch                              # frames of tile 3: the song ends mid-lane
    stretched = level in ("rate", "loop", "pan", "rev", "downmix", "balance")
    events = [
        _ev(0, 1, 0.8, **_stage(level, 0, width)),                                          # across samples 3 and L + 1
        _ev(F - 300, 0, 0.5, **rest),                                                       # starts in tile 0, runs through [T - 1, T + 1)
        _ev(w0 - 100, 2 if stretched else 1, None, **_stage(level, 1, width)),              # its stage straddles the pile-up window's start
        _ev(w0 + 10, 0, 1.7, 200, **rest),                                                  # three loud notes on one another
        _ev(w0 + 13, 0, -1.0, 200, **dict(rest, **_stage(level, 3, width))),
        _ev(w0 + 17, 0, 1.7, 200, **rest),
        _ev(3 * F, 1, 1.2, tail, **_stage(level, 2, width)),                                # tile 3, from its first sample on
    ]
    want = mix(b"", named(instruments, events), width, RATE, nch)
    return instruments, events, nch, want, len(want) // width


def windows(level, width, total):
    T, L = TILE[width], LANE[width]
    w = [(0, total), (3, total - 5), (T - 1, T + 1), (L + 1, L + 2), (2 * T + 5, 3 * T - 7), (T + 3 * L, 3 * T + L)]
    if level == "balance":
        w.append((T + 3 * L + 1, 3 * T + L))               # an odd first sample in a stereo song: left and right stay where the song has them
    return w


def check_song(level, width):
    """what the list must hold, on the CPU with audioop alone, before the GPU is asked"""
    instruments, events, nch, want, total = song(level, width)
    T, L = TILE[width], LANE[width]
    assert 3 * T < total < 4 * T and total % L != 0, (total, T, L)                          # four tiles, ending mid-lane in tile 3
    assert want[2 * T * width:3 * T * width] == bytes(T * width)                            # tile 2: no event touches it
    lo, hi = T + 3 * L, 3 * T + L                                                           # the pile-up window
    pile = want[lo * width:hi * width]
    assert abs(audioop.max(pile, width)) >= 2 ** (8 * width - 1) - 1, "nothing saturates"
    assert audioop.minmax(pile, width)[1] == 2 ** (8 * width - 1) - 1 or audioop.minmax(pile, width)[0] == -2 ** (8 * width - 1)
    back = mix(b"", named(instruments, events[::-1]), width, RATE, nch)
    assert len(back) == len(want) and back[lo * width:hi * width] != pile, "list order does not matter"
    for a, b in windows(level, width, total):
        idle = 2 * T <= a and b <= 3 * T
        assert (want[a * width:b * width] == bytes((b - a) * width)) == idle, (a, b)


def compiled_raw(N, level, width):
    """the song through the C entry point: the product's packer makes the table (an input), N.Sequence is sh_seq_create's thin wrapper"""
    from synthesizer_amd.sample import Sample
    instruments, events, nch, want, total = song(level, width)
    samples = as_samples(instruments, width, RATE)
    track = Sample(samplerate=RATE, nchannels=nch, samplewidth=width)
    bufs, table, segtab, nbytes = track._compile_events(with_samples(samples, events))
    assert nbytes == len(want)
    return N.Sequence(bufs, table, segtab, width, nch, total), samples


def render_window(N, seq, width, a, b, out_sample):
    """(the rendered bytes, the 64 bytes in front of them, the 64 behind) of a window rendered into a 0x5A-filled buffer"""
    n = b - a
    inner = (out_sample + n) * width
    parent = N.DeviceBuffer.from_bytes(b"\x5a" * (64 + inner + 64))
    out = parent.view(64, inner)
    seq.render(a, n, out, out_sample)
    got = parent.download_bytes(64 + inner + 64)
    at = 64 + out_sample * width
    return got[at:at + n * width], got[at - 64:at], got[at + n * width:]


# ---- songs of tracks ----------------------------------------------------------------------------------------------------------------------
GAINS = [(0.5, 1.0, -1.7), (0.0, 1.0, 0.0), (1.0, 1.0, 1.0), (0.999, 2.5, 0.37)]


def subs_of(instruments, tracks, width, nch):
    """every track on its own, event after event: the one place the event chain is evaluated"""
    return [mix(b"", named(instruments, t), width, RATE, nch) for t in tracks]


def master(subs, gains, width):
    """the reference chain behind the sub-mixes: mul (none at 1.0), pad, add, in track order"""
    total = max([len(s) for s in subs] + [0])
    out = bytes(total)
    for sub, g in zip(subs, [1.0] * len(subs) if gains is None else gains):
        if g != 1.0:
            sub = audioop.mul(sub, width, g)
        out = audioop.add(out, sub + bytes(total - len(sub)), width)
    return out


def ints(data, width):
    if width == 3:
        a = np.frombuffer(data, dtype=np.uint8).reshape(-1, 3).astype(np.int64)
        v = a[:, 0] | (a[:, 1] << 8) | (a[:, 2] << 16)
        return np.where(v >= 1 << 23, v - (1 << 24), v)
    return np.frombuffer(data, dtype={1: np.int8, 2: "<i2", 4: "<i4"}[width]).astype(np.int64)


class WithGains:
    """N.Sequence behind render_window, which calls render(first, n, out, out_sample)"""

    def __init__(self, seq, gains):
        self.seq, self.gains = seq, gains

    def render(self, a, n, out, out_sample):
        self.seq.render(a, n, out, out_sample, gains=self.gains)


def raw_tracks(N, instruments, tracks, nch, width):
    """the song through the C entry point: the product's packer makes the table (an input), N.Sequence is sh_seq_create_tracks' thin wrapper"""
    from synthesizer_amd.sample import Sample
    samples = as_samples(instruments, width, RATE)
    track = Sample(samplerate=RATE, nchannels=nch, samplewidth=width)
    bufs, table, segtab, nbytes = track._compile_events(with_samples(samples, [e for t in tracks for e in t]))
    first = [0]
    for t in tracks:
        first.append(first[-1] + len(t))
    return N.Sequence(bufs, table, segtab, width, nch, nbytes // width, track_first=first), samples


@functools.lru_cache(maxsize=None)
def bus_song(width):
    """(instruments, tracks, the sub-mixes, total samples), made once.  Mono.  Track 0 and track 1 pile the loud instrument up inside
    [T + 3 L, 3 T + L) with opposite signs; track 2 is absent from that tile, and tile 3 holds nothing but the last track's note; tile 2 is
    idle and the song ends mid-lane."""
    T, L = TILE[width], LANE[width]
    rng = np.random.default_rng(900 + width)
    instruments = [(pcm(rng, width, HELD[0], 1.0), 1), (pcm(rng, width, HELD[1], 0.6), 1), (pcm(rng, width, HELD[2], 0.6), 1)]
    w0, tail = T + 3 * L, 37 * L + 3
    tracks = [
        [_ev(0, 1, 0.8), _ev(T - 300, 0, 0.5), _ev(w0 + 10, 0, 1.7, 200), _ev(w0 + 13, 0, 1.7, 200)],
        [_ev(w0 - 100, 1, None), _ev(w0 + 10, 0, -1.7, 200), _ev(w0 + 17, 0, -1.7, 200)],
        [_ev(5, 2, 1.3), _ev(3 * T, 1, 1.2, tail)],
    ]
    subs = subs_of(instruments, tracks, width, 1)
    total = max(len(s) for s in subs) // width
    assert 3 * T < total < 4 * T and total % L != 0
    return instruments, tracks, subs, total


# ---- level meters: the reference rows -------------------------------------------------------------------------------------------------------
U32, MASK = np.uint64(32), np.uint64(0xFFFFFFFF)
_POST = {}


def row_of(x, a, nch):
    """the row of song samples a .. a + len(x): ((peak, peak), (sum, sum)), the sums Python ints formed from two uint64 sums"""
    peak, sq = [0, 0], [0, 0]
    for c in range(2 if nch == 2 else 1):
        v = x[(c - a) % 2::2] if nch == 2 else x            # song sample a + i is channel (a + i) & 1
        if len(v):
            m = np.abs(v).astype(np.uint64)                  # |-2^31| = 2^31, taken in int64
            s = m * m                                        # <= 2^62
            peak[c] = int(m.max())
            sq[c] = (int((s >> U32).sum(dtype=np.uint64)) << 32) + int((s & MASK).sum(dtype=np.uint64))
    return tuple(peak), tuple(sq)


def post_fader(key, subs, gains, width):
    """(the tracks as the master takes them, the master), as int64 arrays of the song's length; made once per song and gain vector"""
    if (key, gains) not in _POST:
        total = max([len(s) for s in subs] + [0])
        scaled = []
        for sub, g in zip(subs, [1.0] * len(subs) if gains is None else gains):
            if g != 1.0:
                sub = audioop.mul(sub, width, g)
            scaled.append(ints(sub + bytes(total - len(sub)), width))
        _POST[(key, gains)] = (scaled, ints(master(subs, gains, width), width), master(subs, gains, width))
    return _POST[(key, gains)]


def reference(key, subs, gains, width, nch, a, b):
    scaled, mast, _bytes = post_fader(key, subs, gains, width)
    return [row_of(x[a:b], a, nch) for x in scaled] + [row_of(mast[a:b], a, nch)]


def the_song(kind, width):
    """(instruments, tracks, nch, the sub-mixes, total samples, level)"""
    if kind == "bus":
        instruments, tracks, subs, total = bus_song(width)
        return instruments, tracks, 1, subs, total, "plain"
    instruments, events, nch, _flat, total = song(kind, width)
    tracks = [events[0::3], events[1::3], events[2::3]]         # the list dealt over three tracks
    key = ("subs", kind, width)
    if key not in _POST:
        _POST[key] = subs_of(instruments, tracks, width, nch)
    return instruments, tracks, nch, _POST[key], total, LEVEL_NAME.get(kind, kind)


def metered(N, seq, width, a, b, gains, out_sample=0):
    """(rows, the rendered bytes, the guards intact) of a metered render into a 0x5A-filled buffer"""
    n = b - a
    inner = (out_sample + n) * width
    parent = N.DeviceBuffer.from_bytes(b"\x5a" * (64 + inner + 64))
    rows = seq.render(a, n, parent.view(64, inner), out_sample, gains=gains, meters=True)
    got = parent.download_bytes(64 + inner + 64)
    at = 64 + out_sample * width
    return rows, got[at:at + n * width], got[:at] == b"\x5a" * at and got[at + n * width:] == b"\x5a" * 64
