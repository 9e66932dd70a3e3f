"""GPU parity of an ADSR envelope per event in Sample.mix_at_many / mixer.sequence / sh_mix_events_env -- shaped notes in one launch --
against live ``audioop`` and upstream's ``array`` fades written out here: ``ratecv``, the cut to the note's length, the envelope (split,
``mul`` of the sustain and release parts, the ramps ``int(x * f)`` counting samples, join), ``tostereo``, ``mul``, the cut, ``add`` with
saturation at every event, in list order, on byte slices; the arithmetic of the loop of ``copy().speed().clip().envelope().stereo()``,
``at_volume`` and ``mix_at`` it replaces.  Expected bytes never come from the product.  Rate 8000, instruments of 0.05 - 0.4 s, tracks of
four tiles (a 16-bit tile is 2048 samples, the others 1024)."""
import array
import audioop
import ctypes as C
import math

import numpy as np
import pytest

from oracle.sample_oracle import RefSample
from tests.test_gpu_sequence import _pcm, _sample

pytestmark = pytest.mark.gpu

RATE = 8000
TILE = {1: 1024, 2: 2048, 4: 1024}                          # track samples per workgroup
LANE = {1: 4, 2: 8, 4: 4}                                   # track samples per lane
TYPECODE = {1: "b", 2: "h", 4: "i"}
RIGHT, AFTER_MUL, AFTER_STEREO, RAMPS_FLOORED, SUSTAIN_TRUNCATED, K_FRAMES = range(6)
WRONG = {"envelope after mul": AFTER_MUL, "envelope after tostereo": AFTER_STEREO, "ramps floored": RAMPS_FLOORED,
         "sustain truncated": SUSTAIN_TRUNCATED, "k counts frames": K_FRAMES}


def envelope_bytes(frames: bytes, width, nch, rate, attack, decay, sustainlevel, release, variant=RIGHT) -> bytes:
    """upstream's Sample.envelope on a byte string (split, amplify, fadein, fadeout, join as they stand), or one of the WRONG readings
    of its rounding"""
    fb = width * nch

    def frame_idx(seconds):
        return fb * int(rate * seconds)

    def duration(b):
        return len(b) / rate / width / nch

    def split(b, seconds):
        end = frame_idx(seconds)
        return (b[:end], b[end:]) if end != len(b) else (b, b"")

    def amplify(b, factor):
        if variant != SUSTAIN_TRUNCATED:
            return audioop.mul(b, width, factor)            # clamp, then floor
        a = array.array(TYPECODE[width], b)
        for k in range(len(a)):
            a[k] = int(a[k] * factor)
        return a.tobytes()

    def ramped(b, f):
        a = array.array(TYPECODE[width], b)
        numsamples = len(b) / width
        for k in range(int(numsamples)):
            v = a[k] * (f(k // nch, numsamples / nch) if variant == K_FRAMES else f(k, numsamples))
            a[k] = math.floor(v) if variant == RAMPS_FLOORED else int(v)
        return a.tobytes()

    def fadeout(b, seconds, target_volume):
        seconds = min(seconds, duration(b))
        i = frame_idx(duration(b) - seconds)
        decrease = 1.0 - target_volume
        return b[:i] + ramped(b[i:], lambda k, n: 1.0 - k * decrease / n)

    def fadein(b, seconds, start_volume=0.0):
        seconds = min(seconds, duration(b))
        i = frame_idx(seconds)
        increase = 1.0 - start_volume
        return ramped(b[:i], lambda k, n: k * increase / n + start_volume) + b[i:]

    A, D = split(frames, attack)
    D, S = split(D, decay)
    if sustainlevel < 1:
        S = amplify(S, sustainlevel)
    assert duration(S) - release >= 0, "upstream slices from the wrong end here; the product refuses it"
    S, R = split(S, duration(S) - release)
    if attack > 0:
        A = fadein(A, attack)
    if decay > 0:
        D = fadeout(D, decay, sustainlevel)
    if release > 0:
        R = fadeout(R, release, 0.0)
    return A + D + S + R


def factors(pan):
    if isinstance(pan, tuple):
        return float(pan[0]), float(pan[1])
    return (1.0 - pan) / 2.0, (1.0 + pan) / 2.0           # Sample.pan upstream


def shaped_source(frames, width, rate, nch, volume, other_seconds, speed, pan, env, order=RIGHT) -> bytes:
    """what mix_at is handed for one event: ratecv, the cut to the note's length, the envelope, tostereo, mul, the cut -- or a WRONG order"""
    snch = nch if pan is None else 1
    inrate = rate if speed is None else int(rate * speed)
    if inrate != rate:
        frames = audioop.ratecv(frames, width, snch, inrate, rate, None)[0]

    def shape(b, c):
        if env is None:
            return b
        if len(env) == 5:
            b = b[:width * c * int(rate * env[4])]              # clip(0.0, length)
        return envelope_bytes(b, width, c, rate, *env[:4], variant=order if order in (RAMPS_FLOORED, SUSTAIN_TRUNCATED, K_FRAMES) else RIGHT)

    if order not in (AFTER_MUL, AFTER_STEREO):
        frames = shape(frames, snch)
    if pan is not None:
        frames = audioop.tostereo(frames, width, *factors(pan))
    if order == AFTER_STEREO:
        frames = shape(frames, nch)
    if volume is not None:
        frames = audioop.mul(frames, width, volume)
    if order == AFTER_MUL:
        frames = shape(frames, nch)
    if other_seconds:
        frames = frames[:width * nch * int(rate * other_seconds)]
    return frames


def oracle(track: bytes, events, width, rate, nch, order=RIGHT) -> bytes:
    """events: (seconds, source bytes, volume | None, other_seconds | None, speed | None, pan | None, envelope | None) -- a source with a
    pan is mono, one without has the track's channels -- applied one after another like upstream's mix_at"""
    fb = width * nch
    t = bytearray(track)
    for seconds, frames, volume, other_seconds, speed, pan, env in events:
        frames = shaped_source(frames, width, rate, nch, volume, other_seconds, speed, pan, env, order)
        start = fb * int(rate * seconds)
        end = start + len(frames)
        if end > len(t):
            t.extend(bytes(end - len(t)))
        t[start:end] = audioop.add(bytes(t[start:end]), frames, width)
    return bytes(t)


def _differs(a: bytes, b: bytes) -> int:
    assert len(a) == len(b)
    return int(np.count_nonzero(np.frombuffer(a, dtype=np.uint8) != np.frombuffer(b, dtype=np.uint8)))


def _out_frames(n, inrate, rate):
    return (n - 1) * rate // inrate + 1 if n else 0


LENGTHS = [400, 800, 1203, 1600]                            # frames: 0.05 - 0.2 s; a 16-bit track has room for 3200, 0.4 s, as well
SPEEDS = [0.5, 2 ** (3 / 12), 0.8, 2.0, 1.5, 2 ** (-5 / 12)]
VOLS = [0.5, 1.7, -1.0, 0.8, 1.9, -1.3]
PANS = [0.3, (1.0, 0.0), -0.65, (-0.5, 0.8), (1.5, 1.2), 1.0]
LEVELS = [0.5, 0.7, 1.0, 0.0, 0.25, 0.93]
_CACHE = {}


def notes(width, nch, seed=0, scale=0.6):
    """(instruments, events): instruments are (bytes, channels) -- mono ones first, then (a stereo track) stereo ones; events are (seconds,
    instrument, volume, other_seconds, speed, pan, envelope), 64 of them going twice through the 32 on/off patterns of envelope, speed,
    pan, volume and other_seconds (a mono track has no pan: 16 patterns, four times), the envelopes 4-tuples and 5-tuples in turn, their
    times odd fractions of the note, and then the edge shapes.  Made once per (width, nch, seed, scale) and never changed."""
    key = (width, nch, seed, scale)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(1000 * seed + 10 * width + nch)
    track_frames = 4 * TILE[width] // nch
    lengths = LENGTHS + ([3200] if width == 2 else [])
    instruments = [(_pcm(rng, width, n, scale), 1) for n in lengths]
    if nch == 2:
        instruments += [(_pcm(rng, width, 2 * n, scale), 2) for n in lengths]
    events = []

    def add(k, env_on, speed_on, pan_on, vol_on, cut_on, env=None, which=None, frame=None):
        speed = SPEEDS[k % len(SPEEDS)] if speed_on else None
        i = (k + k // 32) % len(lengths) if which is None else which
        out = _out_frames(lengths[i], int(RATE * speed), RATE) if speed else lengths[i]
        if out > track_frames * 3 // 4:                     # too long for this track at this speed: the shortest instrument
            i = 0
            out = _out_frames(lengths[0], int(RATE * speed), RATE) if speed else lengths[0]
        if env_on and env is None:
            dur = out / RATE
            level = LEVELS[k % len(LEVELS)]
            if (k // 32) % 2:                               # a note length: the release ends the note before the instrument does
                dur = 0.61 * dur
                env = (0.113 * dur, 0.171 * dur, level, 0.233 * dur, dur)
            else:
                env = (0.113 * dur, 0.171 * dur, level, 0.233 * dur)
        if env is not None and len(env) == 5:
            out = min(out, int(RATE * env[4]))
        cut = 0.37 * out / RATE if cut_on else None
        if frame is None:
            frame = int(rng.integers(0, track_frames - out + 1))
        pan = PANS[k % len(PANS)] if pan_on else None
        events.append((frame / RATE, i + (len(lengths) if nch == 2 and pan is None else 0), VOLS[k % len(VOLS)] if vol_on else None, cut, speed, pan, env))

    for k in range(64):
        add(k, k & 1, k & 2, (k & 4) and nch == 2, k & 8, k & 16)
    # the edge shapes: an attack part whose duration rounds a frame down (an unfaded frame at its tail: 8000 * (1001 / 8000) < 1001), an
    # attack longer than the note, a level of 0, an envelope that does nothing, a sustain level alone, no release, across a tile edge
    assert int(RATE * (1001 * width / RATE / width)) == 1000
    add(64, 1, 0, nch == 2, 1, 0, env=(1001.5 / RATE, 0.01, 0.5, 0.01), which=2)
    add(65, 1, 0, 0, 0, 0, env=(1.0, 0.0, 1.0, 0.0), which=0)
    add(66, 1, 1, nch == 2, 0, 0, env=(0.004, 0.003, 0.0, 0.0), which=1)
    add(67, 1, 0, 0, 1, 0, env=(0.0, 0.0, 1.0, 0.0), which=1)
    add(68, 1, 0, 0, 0, 1, env=(0.0, 0.0, 0.37, 0.0), which=3)
    add(69, 1, 1, 0, 1, 0, env=(0.013, 0.0, 0.8, 0.0, 0.031), which=0)
    add(70, 1, 0, nch == 2, 0, 0, env=(0.0201, 0.0107, 0.6, 0.0153), which=1, frame=TILE[width] // nch - 215)
    _CACHE[key] = (instruments, events)
    return _CACHE[key]


def named(instruments, events):
    return [(s, instruments[i][0], v, o, sp, p, e) for s, i, v, o, sp, p, e in events]


def as_samples(instruments, width):
    return [_sample(b, width, RATE, c) for b, c in instruments]


def boundaries(event, instruments, width, nch):
    """(first track sample, track samples, [track samples where a part of the envelope begins]) of an event, in plain integers"""
    seconds, i, _v, other_seconds, speed, pan, env = event
    data, snch = instruments[i]
    frames = len(data) // (width * snch)
    if speed:
        frames = _out_frames(frames, int(RATE * speed), RATE)
    if env is not None and len(env) == 5:
        frames = min(frames, int(RATE * env[4]))
    taken = min(frames, int(RATE * other_seconds)) if other_seconds else frames
    dst = nch * int(RATE * seconds)
    marks = []
    if env is not None:
        a = min(int(RATE * env[0]), frames)
        d = min(int(RATE * env[1]), frames - a)
        s_all = frames - a - d
        s = min(int(RATE * (s_all / RATE - env[3])), s_all)
        marks = [dst + nch * f for f in (a, a + d, a + d + s) if 0 < f < taken]
    return dst, nch * taken, marks


def assert_the_list_has_the_hard_places(instruments, events, width, nch):
    tile, lane = TILE[width], LANE[width]
    spans = [boundaries(e, instruments, width, nch) for e in events if e[6] is not None]
    assert any(dst % 8 for dst, _n, _m in spans), "no enveloped event starts off a multiple of eight samples"
    assert any(m % 8 for _d, _n, marks in spans for m in marks), "no segment boundary off a multiple of eight samples"
    assert any(m % lane for _d, _n, marks in spans for m in marks), "no segment boundary inside a lane's vector"
    assert any(dst // tile != (dst + n - 1) // tile for dst, n, _m in spans if n), "no enveloped event across a tile edge"
    assert max(dst + n for dst, n, _m in spans) <= 4 * tile and max(dst + n for dst, n, _m in spans) > tile     # two to four tiles


def test_the_written_out_envelope_is_refsample_envelope():
    rng = np.random.default_rng(5)
    for width in (1, 2, 4):
        for nch in (1, 2):
            for env in ((0.01, 0.02, 0.5, 0.03), (1001.5 / RATE, 0.01, 0.7, 0.02), (0.0, 0.0, 1.0, 0.0), (1.0, 0.0, 1.0, 0.0), (0.0, 0.05, 0.0, 0.01)):
                data = _pcm(rng, width, 1500 * nch)
                assert envelope_bytes(data, width, nch, RATE, *env) == RefSample(data, width, RATE, nch).envelope(*env).frames


# ---- 1: the definition -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filled", [False, True])
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("width", [1, 2, 4])
def test_mix_at_many_with_envelopes_is_the_oracle_loop(gpu, width, nch, filled):
    instruments, events = notes(width, nch)
    assert_the_list_has_the_hard_places(instruments, events, width, nch)
    base = _pcm(np.random.default_rng(width + nch), width, 4 * TILE[width], 0.3) if filled else b""
    want = oracle(base, named(instruments, events), width, RATE, nch)
    assert 2 * TILE[width] * width < len(want) <= 4 * TILE[width] * width
    samples = as_samples(instruments, width)
    got = _sample(base, width, RATE, nch).mix_at_many([(s, samples[i], v, o, sp, p, e) for s, i, v, o, sp, p, e in events])
    assert len(got) * width * nch == len(want)
    assert bytes(got.view_frame_data()) == want
    for (b, c), smp in zip(instruments, samples):
        assert bytes(smp.view_frame_data()) == b and smp.nchannels == c                 # the instruments are untouched


# ---- 2: every combination --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 4])
def test_envelope_crossed_with_speed_pan_volume_and_other_seconds(gpu, width):
    from synthesizer_amd import mixer
    instruments, events = notes(width, 2)
    patterns = {(e[6] is not None, e[4] is not None, e[5] is not None, e[2] is not None, e[3] is not None) for e in events[:64]}
    assert len(patterns) == 32
    shaped = [e for e in events[:64] if e[6] is not None]
    assert {len(e[6]) for e in shaped if e[5] is not None and e[4] is not None} == {4, 5}
    assert {(len(e[6]), e[4] is not None, e[5] is not None, e[2] is not None, e[3] is not None) for e in shaped} == \
        {(n, a, b, c, d) for n in (4, 5) for a in (False, True) for b in (False, True) for c in (False, True) for d in (False, True)}
    want = oracle(b"", named(instruments, events[:64]), width, RATE, 2)
    samples = as_samples(instruments, width)
    got = mixer.sequence([(s, samples[i], v, o, sp, p, e) for s, i, v, o, sp, p, e in events[:64]], RATE, 2, width, name="shaped")
    assert got.name == "shaped" and (got.samplerate, got.nchannels, got.samplewidth) == (RATE, 2, width)
    assert bytes(got.view_frame_data()) == want


# ---- 3: the order and the rounding can be told from the wrong ones ---------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 4])
def test_the_oracle_tells_the_right_chain_from_every_wrong_one(gpu, width):
    instruments, events = notes(width, 2)
    want = oracle(b"", named(instruments, events), width, RATE, 2)
    wrong = {name: _differs(want, oracle(b"", named(instruments, events), width, RATE, 2, order)) for name, order in WRONG.items()}
    print("width %d: bytes of %d that differ from the wrong readings: %s" % (width, len(want), wrong))
    assert all(n > 0 for n in wrong.values()), wrong
    samples = as_samples(instruments, width)
    got = _sample(b"", width, RATE, 2).mix_at_many([(s, samples[i], v, o, sp, p, e) for s, i, v, o, sp, p, e in events])
    assert bytes(got.view_frame_data()) == want


# ---- 4: saturation in list order -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 4])
def test_loud_enveloped_events_saturate_in_list_order(gpu, width):
    instruments, events = notes(width, 2, seed=4, scale=1.0)
    events = [(s, i, (1.9 if k % 2 else -1.9), o, sp, p, e) for k, (s, i, _v, o, sp, p, e) in enumerate(events) if e is not None]
    want = oracle(b"", named(instruments, events), width, RATE, 2)
    back = oracle(b"", named(instruments, events[::-1]), width, RATE, 2)
    v = np.frombuffer(want, dtype={1: np.int8, 2: "<i2", 4: "<i4"}[width])
    hi = 2 ** (8 * width - 1) - 1
    assert (v == hi).any() and (v == -hi - 1).any()
    assert len(back) == len(want) and _differs(want, back) > 0                           # saturating at every event: the order matters
    samples = as_samples(instruments, width)
    got = _sample(b"", width, RATE, 2).mix_at_many([(s, samples[i], v_, o, sp, p, e) for s, i, v_, o, sp, p, e in events])
    assert bytes(got.view_frame_data()) == want
    got = _sample(b"", width, RATE, 2).mix_at_many([(s, samples[i], v_, o, sp, p, e) for s, i, v_, o, sp, p, e in events[::-1]])
    assert bytes(got.view_frame_data()) == back


# ---- 5: the product's own loop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width, nch", [(2, 2), (1, 1), (4, 2)])
def test_the_same_bytes_as_the_loop_of_speed_clip_envelope_stereo_at_volume_and_mix_at(gpu, width, nch):
    instruments, events = notes(width, nch)
    samples = as_samples(instruments, width)
    base = _pcm(np.random.default_rng(9), width, 4 * TILE[width], 0.3)
    loop = _sample(base, width, RATE, nch)
    for seconds, i, volume, other_seconds, speed, pan, envelope in events:
        o = samples[i]
        if speed is not None:
            o = o.copy().speed(speed)
        if envelope is not None:
            o = o.copy()
            if len(envelope) == 5:
                o.clip(0.0, envelope[4])
            o.envelope(*envelope[:4])
        if pan is not None:
            o = o.copy().stereo(*pan) if isinstance(pan, tuple) else o.copy().pan(pan)
        if volume is not None:
            o = o.at_volume(volume)
        loop.mix_at(seconds, o, other_seconds)
    many = _sample(base, width, RATE, nch).mix_at_many([(s, samples[i], v, o, sp, p, e) for s, i, v, o, sp, p, e in events])
    assert len(many) == len(loop)
    assert bytes(many.view_frame_data()) == bytes(loop.view_frame_data()) == oracle(base, named(instruments, events), width, RATE, nch)


# ---- 6: a mixed list, and the track as a source ----------------------------------------------------------------------------------------
def test_enveloped_and_plain_events_in_one_list_and_the_track_as_a_source(gpu, monkeypatch):
    N = gpu
    width, nch = 2, 2
    instruments, events = notes(width, nch)
    assert any(e[6] is None for e in events) and any(e[6] is not None for e in events)
    samples = as_samples(instruments, width)
    calls = []
    real = N.lib()

    class Spy:
        def __getattr__(self, name):
            if name.startswith("sh_mix_events"):
                calls.append(name)
            return getattr(real, name)
    monkeypatch.setattr(N, "lib", lambda: Spy())
    base = _pcm(np.random.default_rng(3), width, 4 * TILE[width], 0.3)
    t = _sample(base, width, RATE, nch)
    first, last = events[:30], events[30:50]
    env = (0.02, 0.03, 0.5, 0.05, 0.2)
    t.mix_at_many([(s, samples[i], v, o, sp, p, e) for s, i, v, o, sp, p, e in first] + [(0.05, t, 0.4, None, 1.5, None, env)] +
                  [(s, samples[i], v, o, sp, p, e) for s, i, v, o, sp, p, e in last])
    assert calls == ["sh_mix_events_env", "sh_mix_events_env"]                           # the list is cut at the track; one launch per side
    mid = oracle(base, named(instruments, first), width, RATE, nch)
    mid = oracle(mid, [(0.05, mid, 0.4, None, 1.5, None, env)], width, RATE, nch)
    assert bytes(t.view_frame_data()) == oracle(mid, named(instruments, last), width, RATE, nch)
    # a list without an envelope goes where it went before
    del calls[:]
    plain = [(s, samples[i], v, o, sp, p) for s, i, v, o, sp, p, e in events if e is None]
    got = _sample(base, width, RATE, nch).mix_at_many(plain + [(0.1, samples[5], 0.5, None, None, None, None)])
    assert calls == ["sh_mix_events_pan"]
    assert bytes(got.view_frame_data()) == oracle(base, named(instruments, [e for e in events if e[6] is None] + [(0.1, 5, 0.5, None, None, None, None)]), width, RATE, nch)


# ---- 7: the entry point's refusals -----------------------------------------------------------------------------------------------------
def _events(N, rows):
    """rows: (dst_sample, src_sample, nsamples, src_frames, factor, left, right, src, inrate, outrate, src_channels, seg_first, seg_count[, reserved])"""
    t = np.zeros(len(rows), dtype=N.MIX_EVENT_ENV_DTYPE)
    for k, r in enumerate(rows):
        t[k] = tuple(r) + (0,) * (14 - len(r))
    return t


def _segments(N, rows):
    """rows: (end, origin, mul, slope, numsamples, offset, kind[, reserved])"""
    t = np.zeros(len(rows), dtype=N.ENV_SEGMENT_DTYPE)
    for k, r in enumerate(rows):
        t[k] = tuple(r) + (0,) * (8 - len(r))
    return t


def _mix_events_env(N, srcs, events, segments, width, nchannels, track, track_samples):
    arr = (C.c_void_p * max(1, len(srcs)))(*[b.handle for b in srcs])
    return N.lib().sh_mix_events_env(arr, len(srcs), events.ctypes.data if len(events) else None, len(events),
                                     segments.ctypes.data if len(segments) else None, len(segments), width, nchannels,
                                     track.handle if track is not None else None, track_samples)


def test_the_entry_point_refuses_on_the_host_and_leaves_the_track(gpu):
    N = gpu
    rng = np.random.default_rng(26)
    src, base = _pcm(rng, 2, 1000), _pcm(rng, 2, 5000)
    s, t = N.DeviceBuffer.from_bytes(src), N.DeviceBuffer.from_bytes(base)
    nan, inf = float("nan"), float("inf")
    good = [(100, 0, 1.0, 1.0, 100.0, 0.0, 1), (300, 100, 0.5, 0.0, 0.0, 0.0, 0), (500, 300, 0.5, 1.0, 200.0, 0.0, 2)]
    ok = (100, 0, 1000, 500, 0.5, 0.3, 0.7, 0, 8000, 8000, 1, 0, 3)       # 500 mono frames through tostereo: 500 source samples
    ok2 = (100, 0, 500, 0, 0.5, nan, nan, 0, 8000, 8000, 2, 0, 3)         # 250 stereo frames: 500 source samples
    bad = {
        # what the entry points before it refuse
        "source index": ([ok, (0, 0, 10, 5, 1.0, 1.0, 1.0, 1, 8000, 8000, 1, 0, 0)], good),
        "range outside its source": ([ok, (0, 996, 10, 0, 1.0, 1.0, 1.0, 0, 8000, 8000, 1, 0, 0)], good),
        "range outside the track": ([ok, (4992, 0, 10, 5, 1.0, 1.0, 1.0, 0, 8000, 8000, 1, 0, 0)], good),
        "nan factor": ([ok, (0, 0, 10, 5, nan, 1.0, 1.0, 0, 8000, 8000, 1, 0, 0)], good),
        "reserved": ([ok, (0, 0, 10, 5, 1.0, 1.0, 1.0, 0, 8000, 8000, 1, 0, 0, 7)], good),
        "inrate 0": ([ok, (0, 0, 10, 5, 1.0, 1.0, 1.0, 0, 0, 8000, 1, 0, 0)], good),
        "src_channels 0": ([ok, (0, 0, 10, 5, 1.0, 1.0, 1.0, 0, 8000, 8000, 0, 0, 0)], good),
        "src_channels 3": ([(0, 0, 12, 6, 1.0, 1.0, 1.0, 0, 8000, 8000, 3, 0, 0)], good),
        "nan left": ([ok, (0, 0, 10, 5, 1.0, nan, 1.0, 0, 8000, 8000, 1, 0, 0)], good),
        "odd dst_sample": ([ok, (1, 0, 10, 5, 1.0, 1.0, 1.0, 0, 8000, 8000, 1, 0, 0)], good),
        "more samples than src_frames resample to": ([ok, (0, 0, 20, 5, 1.0, 1.0, 1.0, 0, 4000, 8000, 1, 0, 0)], good),
        # and what the segments add
        "eight segments": ([ok, (0, 0, 1000, 0, 1.0, 1.0, 1.0, 0, 8000, 8000, 1, 0, 8)], [(10 * (k + 1), 0, 0.5, 0.0, 0.0, 0.0, 0) for k in range(8)]),
        "segments outside the table": ([ok, (0, 0, 1000, 0, 1.0, 1.0, 1.0, 0, 8000, 8000, 1, 2, 2)], good),
        "seg_first outside the table": ([(0, 0, 1000, 0, 1.0, 1.0, 1.0, 0, 8000, 8000, 1, 4, 1)], good),
        "ends that descend": ([ok2[:12] + (0,), ok], [good[0], (50, 100, 0.5, 0.0, 0.0, 0.0, 0), good[2]]),
        "an end beyond the mono event's source samples": ([(100, 0, 998, 0, 0.5, 0.3, 0.7, 0, 8000, 8000, 1, 0, 3)], good),
        "an end beyond the stereo event's source samples": ([(100, 0, 498, 0, 0.5, 0.3, 0.7, 0, 8000, 8000, 2, 0, 3)], good),
        "an end beyond the resampled event's source samples": ([(0, 0, 18, 5, 1.0, 1.0, 1.0, 0, 4000, 8000, 1, 0, 1)], [(10, 0, 0.5, 0.0, 0.0, 0.0, 0)]),
        "an origin beyond them": ([ok], [good[0], good[1], (500, 501, 0.5, 1.0, 200.0, 0.0, 2)]),
        "nan mul": ([ok], [(100, 0, nan, 1.0, 100.0, 0.0, 1)] + good[1:]),
        "infinite slope": ([ok], [(100, 0, 1.0, inf, 100.0, 0.0, 1)] + good[1:]),
        "infinite numsamples": ([ok], [(100, 0, 1.0, 1.0, inf, 0.0, 1)] + good[1:]),
        "nan offset": ([ok], [(100, 0, 1.0, 1.0, 100.0, nan, 1)] + good[1:]),
        "a ramp over no samples": ([ok], [(100, 0, 1.0, 1.0, 0.0, 0.0, 1)] + good[1:]),
        "a ramp over minus one sample": ([ok], good[:2] + [(500, 300, 0.5, 1.0, -1.0, 0.0, 2)]),
        "kind 3": ([ok], good[:2] + [(500, 300, 0.5, 1.0, 200.0, 0.0, 3)]),
        "a segment's reserved": ([ok], good[:2] + [(500, 300, 0.5, 1.0, 200.0, 0.0, 2, 1)]),
    }
    for what, (rows, segs) in bad.items():
        assert _mix_events_env(N, [s], _events(N, rows), _segments(N, segs), 2, 2, t, 5000) == N.SH_ERR_INVALID, what
        err = N.lib().sh_last_error()
        assert err.startswith(b"sh_mix_events_env") and b"event %d" % (len(rows) - 1) in err, (what, err)       # the event is named
        assert t.download_bytes(len(base)) == base, what
    for width in (0, 3, 5, -2):
        assert _mix_events_env(N, [s], _events(N, [ok]), _segments(N, good), width, 2, t, 5000) == N.SH_ERR_INVALID
    assert _mix_events_env(N, [s], _events(N, [ok]), _segments(N, good), 2, 0, t, 5000) == N.SH_ERR_INVALID
    assert _mix_events_env(N, [s], _events(N, [ok]), _segments(N, good), 2, 1, t, 5000) == N.SH_OK       # a mono track: a mono event of it, no tostereo
    t = N.DeviceBuffer.from_bytes(base)
    assert _mix_events_env(N, [s, t], _events(N, [ok]), _segments(N, good), 2, 2, t, 5000) == N.SH_ERR_INVALID     # a source that is the track
    assert _mix_events_env(N, [s], _events(N, [ok]), _segments(N, good), 2, 2, t, 5001) == N.SH_ERR_INVALID
    assert t.download_bytes(len(base)) == base                                                         # nothing was launched
    assert _mix_events_env(N, [s], _events(N, []), _segments(N, []), 2, 2, t, 5000) == N.SH_OK
    assert t.download_bytes(len(base)) == base
    # and what it accepts: the mono event through tostereo, then the stereo one, both shaped by the same three segments
    assert _mix_events_env(N, [s], _events(N, [ok, ok2]), _segments(N, good), 2, 2, t, 5000) == N.SH_OK, N.lib().sh_last_error()

    def by_hand(data):
        a = array.array("h", data)
        for p in range(500):
            x = a[p]
            if p < 100:
                x = int(x * (p * 1.0 / 100.0 + 0.0))
            else:
                x = math.floor(max(-32768.0, min(32767.0, x * 0.5)))
                if p >= 300:
                    x = int(x * (1.0 - (p - 300) * 1.0 / 200.0))
            a[p] = x
        return a.tobytes()
    want = bytearray(base)
    want[200:2200] = audioop.add(base[200:2200], audioop.mul(audioop.tostereo(by_hand(src[:1000]), 2, 0.3, 0.7), 2, 0.5), 2)
    want[200:1200] = audioop.add(bytes(want[200:1200]), audioop.mul(by_hand(src[:1000]), 2, 0.5), 2)
    assert t.download_bytes(len(base)) == bytes(want)
