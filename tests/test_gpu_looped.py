"""GPU parity of a sustain loop per event in Sample.mix_at_many / mixer.sequence / sh_mix_events_loop -- notes longer than their recording,
in one launch -- against bytes unrolled on the host by the frame formula (virtual frame v is frame v of the source while v < E, frame
S + (v - E) % (E - S) after it; tests/seqref.py: unroll) and then the rest of its chain (source, mix) with live ``audioop``: ``ratecv`` over the
unrolled frames, the cut, the envelope, ``tostereo``, ``mul``, the cut, ``add`` with saturation at every event, in list order.  Expected
bytes never come from the product.  Rate 8192 (a power of two: frame / RATE seconds are exact), sources of a few hundred frames, tracks
of three tiles (a 16-bit tile is 2048 samples, the others 1024)."""
import audioop
from math import gcd

import numpy as np
import pytest

from tests.seqcases import (LOOPS, SHAPED_RATE, SPEEDS, STARTS, as_samples, call_level, event_table, in_a_child_under_the_other_alignment_scheme, lists,
                            mix_events, named, rows_of, sample_of, shaped_notes, spy, with_samples)
from tests.seqref import LANE, TILE, differs, discriminates, mix, out_frames, pcm, unroll, unroll_frames

pytestmark = pytest.mark.gpu

RATE = 8192


# ---- 1: plain looped events, through the entry point (track offsets count samples there) -------------------------------------------------
def plain_cases(width, nch):
    """(sources, rows as (dst_sample, source, S, L, V, factor)): every loop length at every track offset 0 .. 15, the starts, the four
    kinds of V and the volumes in turn; then notes over three tiles"""
    rng = np.random.default_rng(10 * width + nch)
    tile = TILE[width]
    sources = [pcm(rng, width, nch * n, 0.5) for n in (300, 211)]
    rows = []
    k = 0
    for L in LOOPS:
        for off in range(16):
            S = STARTS[k % 3]
            E = S + L
            V = [E - 1, E, E + 1, E + 3 * L + max(1, L // 2)][(k // 3) % 4]
            if k % 5 == 0:                                  # a long head: the loop at the end of the recording
                S = (300, 211)[k % 2] - L
                E = S + L
                V = E + 2 * L + L // 3 + 1
            base = [40, tile - 96, 2 * tile - 24, tile + 500][k % 4]
            rows.append((base + off, k % 2, S, L, V, [1.0, 0.5, 1.0, -0.8][k % 4]))
            k += 1
    # one tile wholly in the head, one with the seam, one wholly behind it: a head that starts in tile 0 and ends in tile 1
    for j, (L, S) in enumerate(zip(LOOPS, [0, 1, 5, 0, 1, 5, 200])):
        frames = (tile + 600) // nch
        rows.append((tile - 2 * (60 + j) + (j % 2 if nch == 1 else 0), 0, 300 - L if j % 2 else S, L, frames, 0.25))
    return sources, rows


def plain_want(base, sources, rows, width, nch):
    t = bytearray(base)
    fb = width * nch
    for dst, i, S, L, V, factor in rows:
        F = len(sources[i]) // fb
        assert S + L <= F
        data = unroll(sources[i], width, nch, RATE, (S / RATE, (S + L) / RATE, V / RATE))
        assert len(data) == V * fb
        if factor != 1.0:
            data = audioop.mul(data, width, factor)
        a, b = dst * width, dst * width + len(data)
        t[a:b] = audioop.add(bytes(t[a:b]), data, width)
    return bytes(t)


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_plain_looped_events_at_every_offset(gpu, width, nch):
    N = gpu
    tile, lane = TILE[width], LANE[width]
    sources, rows = plain_cases(width, nch)
    ntrack = 3 * tile - 6
    base = pcm(np.random.default_rng(width), width, ntrack, 0.3)
    # the list has the hard places
    seams = [(dst + (S + L) * nch) % lane for dst, _i, S, L, V, _f in rows if V > S + L]
    assert set(seams) == set(range(lane)), "the seam does not meet a lane's samples at every position"
    assert {dst % 16 for dst, *_ in rows} == set(range(16)) and {L for _d, _i, _S, L, _V, _f in rows} == set(LOOPS)
    assert {S for _d, _i, S, *_ in rows} >= set(STARTS)
    kinds = {(V < S + L, V == S + L, V == S + L + 1, V > S + 3 * L) for _d, _i, S, L, V, _f in rows}
    assert len(kinds) == 4
    whole = [(dst, S, L, V) for dst, _i, S, L, V, _f in rows if dst < tile < dst + (S + L) * nch and dst + V * nch > 2 * tile]
    assert whole, "no note with its head across the first tile edge and its loop over the third tile"
    assert all(dst + V * nch <= ntrack for dst, _i, _S, _L, V, _f in rows)
    want = plain_want(base, sources, rows, width, nch)
    bufs = [N.DeviceBuffer.from_bytes(b) for b in sources]
    track = N.DeviceBuffer.from_bytes(base)
    table = event_table(N, "loop", [(dst, 0, V * nch, V, f, 0.0, 0.0, i, RATE, RATE, nch, 0, 0, 0, S, L) for dst, i, S, L, V, f in rows])
    assert mix_events(N, "loop", bufs, table, None, width, nch, track, ntrack) == N.SH_OK, N.lib().sh_last_error()
    got = track.download_bytes(len(base))
    assert got == want, "%d bytes differ" % differs(got, want)
    # on the parent the eighth element does nothing: the bytes of the unlooped notes are others
    assert want != plain_want(base, sources, [(d, i, S, L, min(V, S + L), f) for d, i, S, L, V, f in rows], width, nch)


def test_plain_looped_events_under_the_other_alignment_scheme(gpu):
    """SYNTHHIP_SEQ_ALIGN is read once per process (sh_init): the 16-bit cases again in a child under the scheme that is not the default"""
    in_a_child_under_the_other_alignment_scheme(__file__, ["test_plain_looped_events_at_every_offset[2-1]", "test_plain_looped_events_at_every_offset[2-2]",
                                                           "test_loops_crossed_with_speed_pan_envelope_volume_and_other_seconds[2]"])


# ---- 2: crossed with the rest, through Sample.mix_at_many ---------------------------------------------------------------------------------
_CACHE = {}


def notes(width, nch=2, seed=0, scale=0.6, loud=False):
    """(instruments as (bytes, channels), events as (seconds, instrument, volume, other_seconds, speed, pan, envelope, loop)): the seven
    speeds times the seven loop lengths, pan, envelope (with a note length), volume and other_seconds on and off.  Made once, never changed."""
    key = (width, nch, seed, scale, loud)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(1000 * seed + 10 * width + nch)
    track_frames = 3 * TILE[width] // nch
    lengths = [300, 211, 97]
    instruments = [(pcm(rng, width, n, scale), 1) for n in lengths]
    if nch == 2:
        instruments += [(pcm(rng, width, 2 * n, scale), 2) for n in lengths]
    events = []
    for k in range(98):
        speed = SPEEDS[k % 7]
        L = LOOPS[(k // 7) % 7]
        i = k % 3
        S = STARTS[k % 3] if k % 4 else lengths[i] - L - (k % 2)     # a short head, or the loop at the end of the recording
        E = S + L
        out = 150 + (37 * k) % 600                          # frames the note lands on, about
        inrate = RATE if speed is None else int(RATE * speed)
        V = max(2, out * inrate // RATE)
        out = out_frames(V, inrate, RATE)
        pan = [0.3, (1.0, 0.0), -0.65, (1.5, 1.2)][k % 4] if (k & 1) and nch == 2 else None
        env = None
        if (k & 2) and width != 3:
            dur = (0.61 * out + 0.37) / RATE                # the note's length falls inside a loop pass for most of them
            env = (0.113 * dur, 0.171 * dur, [0.5, 0.7, 1.0, 0.0, 0.25][k % 5], 0.233 * dur, dur)
            out = min(out, int(RATE * dur))
        volume = ([1.9, -1.9] if loud else [0.5, 1.7, -1.0, 0.8])[k % (2 if loud else 4)] if (k & 4) or loud else None
        cut = (0.37 * out + 1) / RATE if k & 8 else None
        frame = int(rng.integers(0, track_frames - out + 1))
        events.append((frame / RATE, i + (3 if nch == 2 and pan is None else 0), volume, cut, speed, pan, env, (S / RATE, E / RATE, V / RATE)))
    _CACHE[key] = (instruments, events)
    return _CACHE[key]


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_loops_crossed_with_speed_pan_envelope_volume_and_other_seconds(gpu, width):
    from synthesizer_amd import mixer
    instruments, events = notes(width)
    crossed = {(e[4], round(RATE * (e[7][1] - e[7][0]))) for e in events}
    assert crossed == {(sp, L) for sp in SPEEDS for L in LOOPS}          # speed 10 over the 3-frame loop and 0.1 over the 1-frame loop among them
    assert {(e[5] is not None, e[6] is not None, e[2] is not None, e[3] is not None) for e in events} >= \
        {(a, b and width != 3, c, d) for a in (False, True) for b in (False, True) for c in (False, True) for d in (False, True)}
    if width != 3:                                          # a note length that falls inside a loop pass, behind the head
        assert any(e[6] is not None and e[4] is None and int(RATE * e[6][4]) > round(RATE * e[7][1]) and
                   (int(RATE * e[6][4]) - round(RATE * e[7][1])) % round(RATE * (e[7][1] - e[7][0])) for e in events)
    want = mix(b"", named(instruments, events), width, RATE, 2)
    assert 2 * TILE[width] * width < len(want) <= 3 * TILE[width] * width
    unlooped = mix(b"", [e[:7] + (None,) for e in named(instruments, events)], width, RATE, 2) if width == 3 else None
    assert unlooped is None or unlooped != want
    samples = as_samples(instruments, width, RATE)
    got = mixer.sequence(with_samples(samples, events), RATE, 2, width, name="held")
    assert got.name == "held" and len(got) * 2 * width == len(want)
    assert bytes(got.view_frame_data()) == want, "%d bytes differ" % differs(bytes(got.view_frame_data()), want)
    for (b, c), smp in zip(instruments, samples):
        assert bytes(smp.view_frame_data()) == b and smp.nchannels == c                 # the instruments are untouched


@pytest.mark.parametrize("nch", [1, 2])
def test_a_looped_note_at_a_reduced_outrate_of_65536_or_more(gpu, nch):
    """96 kHz against int(96000 * speed) coprime to it: the float64 route (shr::shifted_int) of the 16-bit kernel over virtual frames"""
    rate = 96000
    rng = np.random.default_rng(7 + nch)
    instruments = [(pcm(rng, 2, nch * n, 1.0), nch) for n in (9, 700, 301)]
    speeds = [2 ** (7 / 12), 0.5, 0.999999, None, 1.00002, 2 ** (-7 / 12)]
    assert sum(1 for sp in speeds if sp and rate // gcd(int(rate * sp), rate) >= 65536) >= 3
    events = []
    for k in range(36):
        i = k % 3
        F = (9, 700, 301)[i]
        L = LOOPS[k % 7] if i else [1, 2, 3][k % 3]
        S = min(STARTS[k % 3], F - L) if k % 2 else F - L
        events.append((int(rng.integers(0, 3000)) / rate, i, [None, 0.7, -1.3][k % 3], None, speeds[k % 6], None, None,
                       ((S + 0.5) / rate, (S + L + 0.5) / rate, (900.5 + 13 * k) / rate)))
    base = pcm(rng, 2, nch * 5000, 0.5)
    want = mix(base, named(instruments, events), 2, rate, nch)
    samples = as_samples(instruments, 2, rate)
    got = sample_of(base, 2, rate, nch).mix_at_many(with_samples(samples, events))
    assert bytes(got.view_frame_data()) == want


# ---- 3: the order ------------------------------------------------------------------------------------------------------------------------
def order_notes(width):
    """every event has a loop, a speed and an envelope that the resampled recording holds, so that every wrong order can be formed"""
    rng = np.random.default_rng(40 + width)
    instruments = [(pcm(rng, width, 400, 0.6), 1), (pcm(rng, width, 2 * 300, 0.6), 2)]
    events = []
    for k in range(24):
        i = k % 2
        speed = [0.5, 0.8, 1.5, 2 ** (3 / 12)][k % 4]
        S, L = [40, 41, 45][k % 3], LOOPS[2 + k % 5]
        dur = 0.02 + 0.0005 * k                             # the resampled recording holds the envelope too: the wrong order can be formed
        env = (0.113 * dur, 0.171 * dur, 0.5, 0.233 * dur, dur)
        events.append((int(rng.integers(0, 900)) / RATE, i, [None, 0.7][k % 2], None, speed, 0.3 if i == 0 else None, env,
                       (S / RATE, (S + L) / RATE, (500 + 11 * k) / RATE)))
    return instruments, events


@pytest.mark.parametrize("width", [1, 2, 4])
def test_the_oracle_tells_the_right_order_from_each_wrong_one(gpu, width):
    instruments, events = order_notes(width)
    want = mix(b"", named(instruments, events), width, RATE, 2)
    discriminates(want, named(instruments, events), width, RATE, 2, "loop")
    samples = as_samples(instruments, width, RATE)
    got = sample_of(b"", width, RATE, 2).mix_at_many(with_samples(samples, events))
    assert bytes(got.view_frame_data()) == want


# ---- 4: saturation in list order -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_loud_looped_events_saturate_in_list_order(gpu, width):
    instruments, events = notes(width, 2, seed=4, scale=1.0, loud=True)
    want = mix(b"", named(instruments, events), width, RATE, 2)
    back = mix(b"", named(instruments, events[::-1]), width, RATE, 2)
    if width == 3:
        v = np.frombuffer(want, dtype=np.uint8).reshape(-1, 3)
        assert (v == (255, 255, 127)).all(axis=1).any() and (v == (0, 0, 128)).all(axis=1).any()
    else:
        v = np.frombuffer(want, dtype={1: np.int8, 2: "<i2", 4: "<i4"}[width])
        hi = 2 ** (8 * width - 1) - 1
        assert (v == hi).any() and (v == -hi - 1).any()
    assert len(back) == len(want) and differs(want, back) > 0                           # saturating at every event: the order matters
    samples = as_samples(instruments, width, RATE)
    got = sample_of(b"", width, RATE, 2).mix_at_many(with_samples(samples, events))
    assert bytes(got.view_frame_data()) == want
    got = sample_of(b"", width, RATE, 2).mix_at_many(with_samples(samples, events[::-1]))
    assert bytes(got.view_frame_data()) == back


# ---- 5: the product's own loop of calls ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width, nch", [(2, 2), (1, 1), (3, 2), (4, 2)])
def test_the_same_bytes_as_the_loop_of_clip_join_speed_envelope_stereo_at_volume_and_mix_at(gpu, width, nch):
    instruments, events = notes(width, nch)
    events = events[::2][:28] + events[1::2][:14]
    samples = as_samples(instruments, width, RATE)
    base = pcm(np.random.default_rng(9), width, 3 * TILE[width], 0.3)
    loop_ = sample_of(base, width, RATE, nch)
    for seconds, i, volume, other_seconds, speed, pan, envelope, loop in events:
        ls, le, length = loop
        o = samples[i].copy().clip(0.0, le)
        body = samples[i].copy().clip(ls, le)
        while o.duration < length:
            o.join(body)
        o.clip(0.0, length)
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
        loop_.mix_at(seconds, o, other_seconds)
    many = sample_of(base, width, RATE, nch).mix_at_many(with_samples(samples, events))
    assert len(many) == len(loop_)
    assert bytes(many.view_frame_data()) == bytes(loop_.view_frame_data()) == mix(base, named(instruments, events), width, RATE, nch)


# ---- 6: the levels ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 4])
def test_a_list_of_env_gives_the_same_bytes_through_the_loop_entry_point(gpu, width):
    N = gpu
    sources, base, _A, _B, C_, _wa, _wb, want_c = lists(width)
    bufs = [N.DeviceBuffer.from_bytes(b) for b in sources]
    rows = rows_of(C_, sources, width)
    got = {}
    for level in ("env", "loop"):
        track = N.DeviceBuffer.from_bytes(base)
        assert call_level(N, level, rows, bufs, width, track, len(base) // width) == N.SH_OK, (level, N.lib().sh_last_error())
        got[level] = track.download_bytes(len(base))
    assert got["loop"] == got["env"] == want_c


def test_a_list_without_a_loop_reaches_the_entry_point_it_reached_before(gpu, monkeypatch):
    N = gpu
    instruments, events = notes(2)
    samples = as_samples(instruments, 2, RATE)
    calls = spy(N, monkeypatch)
    e_instruments, e_events = shaped_notes(2, 2)            # the envelope file's list: envelopes that fit the recordings as they are
    e_samples = as_samples(e_instruments, 2, SHAPED_RATE)
    unlooped = [(s_, e_samples[i], v, o, sp, p, e, None) for s_, i, v, o, sp, p, e in e_events]
    got = sample_of(b"", 2, SHAPED_RATE, 2).mix_at_many(unlooped)
    assert calls == ["sh_mix_events_env"]
    assert bytes(got.view_frame_data()) == mix(b"", named(e_instruments, e_events), 2, SHAPED_RATE, 2)
    del calls[:]
    sample_of(b"", 2, SHAPED_RATE, 2).mix_at_many([e[:6] + (None, None) for e in unlooped])
    assert calls == ["sh_mix_events_pan"]
    del calls[:]
    sample_of(b"", 2, RATE, 2).mix_at_many(with_samples(samples, events[:40]))
    assert calls == ["sh_mix_events_loop"]


# ---- 7: the track as a looped source ---------------------------------------------------------------------------------------------------------
def test_looped_and_unlooped_events_in_one_list_and_the_track_as_a_looped_source(gpu, monkeypatch):
    N = gpu
    width, nch = 2, 2
    instruments, events = notes(width, nch)
    events = [e if k % 3 else e[:6] + (None, None) for k, e in enumerate(events)]      # (an envelope sized for the held note does not fit the recording)
    assert any(e[7] is None for e in events[:50]) and any(e[7] is not None and e[6] is not None for e in events[:50])
    samples = as_samples(instruments, width, RATE)
    calls = spy(N, monkeypatch)
    base = pcm(np.random.default_rng(3), width, 3 * TILE[width], 0.3)
    t = sample_of(base, width, RATE, nch)
    first, last = events[:30], events[30:50]
    env = (0.02, 0.03, 0.5, 0.05, 0.2)
    own = (0.05, None, 0.4, None, 1.5, None, env, (100 / RATE, 171 / RATE, 0.4))
    t.mix_at_many(with_samples(samples, first) + [own[:1] + (t,) + own[2:]] + with_samples(samples, last))
    assert calls == ["sh_mix_events_loop", "sh_mix_events_loop"]                         # the list is cut at the track; one launch per side
    mid = mix(base, named(instruments, first), width, RATE, nch)
    mid = mix(mid, [own[:1] + (mid,) + own[2:]], width, RATE, nch)
    assert bytes(t.view_frame_data()) == mix(mid, named(instruments, last), width, RATE, nch)


def test_the_track_as_a_looped_source_is_clamped_to_what_the_events_before_left(gpu):
    """the track starts empty and the events before grow it: loop_end is clamped to the track as it is when the event runs -- inside the
    grown part, and beyond its end -- not to what it held when the list was read"""
    width, nch = 2, 2
    instruments, events = notes(width, nch)
    samples = as_samples(instruments, width, RATE)
    first, last = events[:30], events[30:40]
    mid = mix(b"", named(instruments, first), width, RATE, nch)
    frames = len(mid) // (width * nch)
    assert frames > 1000
    inside = (0.05, None, 0.4, None, 1.5, None, (0.02, 0.03, 0.5, 0.05, 0.2), (100 / RATE, 171 / RATE, 0.4))
    beyond = (0.01, None, -0.7, 0.3, None, None, None, ((frames - 300) / RATE, (frames + 500) / RATE, (frames + 900) / RATE))
    t = sample_of(b"", width, RATE, nch)
    t.mix_at_many(with_samples(samples, first) + [inside[:1] + (t,) + inside[2:], beyond[:1] + (t,) + beyond[2:]] + with_samples(samples, last))
    want = mix(mid, [inside[:1] + (mid,) + inside[2:]], width, RATE, nch)
    assert len(want) // (width * nch) < frames + 500                                     # the second loop's end lies beyond the track still
    want = mix(want, [beyond[:1] + (want,) + beyond[2:]], width, RATE, nch)
    want = mix(want, named(instruments, last), width, RATE, nch)
    assert bytes(t.view_frame_data()) == want
    # a loop that is empty in the track as the events before left it: found when that event runs
    t = sample_of(b"", width, RATE, nch)
    with pytest.raises(ValueError, match="mix_at_many: loop"):
        t.mix_at_many(with_samples(samples, first) + [(0.0, t, None, None, None, None, None, ((frames + 10) / RATE, (frames + 90) / RATE, 3.0))])
    assert bytes(t.view_frame_data()) == mid


# ---- 8: the entry point ------------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_refuses_on_the_host_and_leaves_the_track(gpu):
    N = gpu
    rng = np.random.default_rng(26)
    src, base = pcm(rng, 2, 1000), pcm(rng, 2, 5000)
    s, t = N.DeviceBuffer.from_bytes(src), N.DeviceBuffer.from_bytes(base)
    nan = float("nan")
    segs = np.zeros(1, dtype=N.ENV_SEGMENT_DTYPE)
    segs[0] = (100, 0, 0.5, 0.0, 0.0, 0.0, 0, 0)
    # 500 stereo frames in the source; a good looped row: frames 100 .. 300 held for 900 frames
    ok = (100, 0, 1800, 900, 0.5, 0.0, 0.0, 0, 8000, 8000, 2, 0, 0, 0, 100, 200)
    mono = (100, 0, 1800, 900, 0.5, 0.3, 0.7, 0, 8000, 8000, 1, 0, 0, 0, 100, 200)     # 1000 mono frames through tostereo
    bad = {
        # what sh_mix_events_env refuses
        "source index": (ok[:7] + (1,) + ok[8:]),
        "nan factor": (ok[:4] + (nan,) + ok[5:]),
        "reserved": (ok[:13] + (7,) + ok[14:]),
        "inrate 0": (ok[:8] + (0,) + ok[9:]),
        "src_channels 3": (ok[:10] + (3,) + ok[11:]),
        "nan left": (mono[:5] + (nan,) + mono[6:]),
        "odd dst_sample of a mono source": ((101,) + mono[1:]),
        "range outside the track": ((4000,) + ok[1:]),
        "an unlooped row's range outside its source": (0, 996, 10, 0, 1.0, 0.0, 0.0, 0, 8000, 8000, 2, 0, 0, 0, 0, 0),
        "an unlooped row's src_frames outside its source": (0, 0, 10, 501, 1.0, 0.0, 0.0, 0, 4000, 8000, 2, 0, 0, 0, 0, 0),
        "segments outside the table": (ok[:11] + (1, 1) + ok[13:]),
        # and what the loop adds
        "the loop beyond the source": (ok[:14] + (400, 101)),
        "loop_start beyond the source": (ok[:14] + (501, 1)),
        "the loop beyond what src_sample leaves": ((100, 200) + ok[2:14] + (300, 101)),
        "src_sample off whole frames": ((100, 1) + ok[2:]),
        "nsamples off whole frames": (ok[:2] + (1799,) + ok[3:]),
        "more samples than the virtual frames hold": (ok[:2] + (1802,) + ok[3:]),
        "more samples than the virtual frames resample to": (ok[:2] + (2 * 1800,) + ok[3:8] + (4000,) + ok[9:]),     # 900 frames at half speed: 1799
        "more virtual samples than 32 bits index": (ok[:3] + (0xFFFF0000 // 2 + 1,) + ok[4:]),
    }
    for what, row in bad.items():
        rows = [ok, row]
        assert mix_events(N, "loop", [s], event_table(N, "loop", rows), segs, 2, 2, t, 5000) == N.SH_ERR_INVALID, what
        err = N.lib().sh_last_error()
        assert err.startswith(b"sh_mix_events_loop") and b"event 1" in err, (what, err)      # the event is named
        assert t.download_bytes(len(base)) == base, what
    # width 3 with segments; width 3 without them may loop
    s3, t3 = N.DeviceBuffer.from_bytes(bytes(3000)), N.DeviceBuffer.from_bytes(bytes(15000))
    shaped = ok[:11] + (0, 1) + ok[13:]
    assert mix_events(N, "loop", [s3], event_table(N, "loop", [ok, shaped]), segs, 3, 2, t3, 5000) == N.SH_ERR_INVALID
    assert b"event 1" in N.lib().sh_last_error()
    assert t3.download_bytes(15000) == bytes(15000)
    assert mix_events(N, "loop", [s3], event_table(N, "loop", [ok]), None, 3, 2, t3, 5000) == N.SH_OK, N.lib().sh_last_error()
    for width in (0, 5, -2):
        assert mix_events(N, "loop", [s], event_table(N, "loop", [ok]), None, width, 2, t, 5000) == N.SH_ERR_INVALID
    assert mix_events(N, "loop", [s], event_table(N, "loop", [ok]), None, 2, 0, t, 5000) == N.SH_ERR_INVALID
    assert mix_events(N, "loop", [s, t], event_table(N, "loop", [ok]), None, 2, 2, t, 5000) == N.SH_ERR_INVALID      # a source that is the track
    assert mix_events(N, "loop", [s], event_table(N, "loop", [ok]), None, 2, 2, t, 5001) == N.SH_ERR_INVALID
    assert mix_events(N, "loop", [s], event_table(N, "loop", []), None, 2, 2, t, 5000) == N.SH_OK
    assert t.download_bytes(len(base)) == base                                                         # nothing was launched
    # and what it accepts: the stereo note, then the mono one through tostereo
    assert mix_events(N, "loop", [s], event_table(N, "loop", [ok, mono]), None, 2, 2, t, 5000) == N.SH_OK, N.lib().sh_last_error()
    want = bytearray(base)
    held = audioop.mul(unroll_frames(src, 4, 100, 300, 900), 2, 0.5)
    want[200:3800] = audioop.add(base[200:3800], held, 2)
    held = unroll_frames(src, 2, 100, 300, 900)
    held = audioop.mul(audioop.tostereo(held, 2, 0.3, 0.7), 2, 0.5)
    want[200:3800] = audioop.add(bytes(want[200:3800]), held, 2)
    assert t.download_bytes(len(base)) == bytes(want)
