"""GPU parity of a region and of reversed playback per event in Sample.mix_at_many / mixer.sequence / sh_mix_events_rev -- slices of a
recording, forwards or backwards, in one launch -- against live ``audioop`` on byte slices: the region cut as ``clip`` cuts it
(``data[fb * int(rate * start):fb * int(rate * end)]``), ``audioop.reverse`` of the slice (the order of the SAMPLES), and then
the rest of the chain of tests/seqref.py (source, mix) as it stands: the loop unrolled over the clipped, reversed frames, ``ratecv``,
the cut, the envelope, ``tostereo``, ``mul``, the cut, ``add`` with saturation at every event, in list order.  Expected bytes never come
from the product.  Rate 8192, sources of a few hundred frames, tracks of three tiles, as that file has them."""
import audioop

import numpy as np
import pytest

from tests.seqcases import (LENGTHS, LOOPS, SPEEDS, STARTS, as_samples, event_table, in_a_child_under_the_other_alignment_scheme, mix_events, named,
                            sample_of, spy, with_samples)
from tests.seqref import LANE, TILE, differs, discriminates, mix, out_frames, pcm, unroll

pytestmark = pytest.mark.gpu

RATE = 8192


# ---- 1: plain reversed events, through the entry point (track offsets count samples there) -------------------------------------------------
def plain_cases(width, nch):
    """(sources, rows as (dst_sample, source, first frame, frames, samples taken, factor)): every region length at every track offset
    0 .. 15, the starts, regions on the buffer's first and last sample and the factors in turn; then notes over three tiles"""
    rng = np.random.default_rng(20 * width + nch)
    tile = TILE[width]
    held = (300, 211, (tile + 700) // nch)                  # frames
    sources = [pcm(rng, width, nch * n, 0.5) for n in held]
    rows = []
    k = 0
    lengths = LENGTHS if nch == 1 else LENGTHS + [(n + 1) // 2 for n in LENGTHS]      # stereo: that many frames, and that many samples' worth
    for F in lengths:
        for off in range(16):
            i = k % 2
            a = STARTS[k % 3]
            if k % 5 == 0:
                a = held[i] - F                             # the region ends on the buffer's last sample
            if k % 5 == 1:
                a = 0                                       # and starts on its first
            n = F * nch if k % 7 != 3 or F == 1 else (F - 1) * nch        # (a cut: the first samples of the REVERSED region)
            base = [40, tile - 96, 2 * tile - 24, tile + 500][k % 4]
            rows.append((base + off, i, a, F, n, [1.0, 0.5, -0.8][k % 3]))
            k += 1
    for j in range(6):                                      # from tile 0 over tile 1 into tile 2
        F = held[2] - j - (0 if j % 2 else 5)
        a = held[2] - F if j % 2 else (0, 5)[j // 2 % 2]
        rows.append((tile - 300 - 2 * j + (j % 2 if nch == 1 else 0), 2, a, F, F * nch, 0.25))
    return sources, rows


def plain_want(base, sources, rows, width, nch, reverse=True):
    t = bytearray(base)
    fb = width * nch
    for dst, i, a, F, n, factor in rows:
        assert (a + F) * fb <= len(sources[i])
        data = sources[i][a * fb:(a + F) * fb]
        if reverse:
            data = audioop.reverse(data, width)
        data = data[:n * width]
        if factor != 1.0:
            data = audioop.mul(data, width, factor)
        lo, hi = dst * width, dst * width + len(data)
        t[lo:hi] = audioop.add(bytes(t[lo:hi]), data, width)
    return bytes(t)


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_plain_reversed_events_at_every_offset(gpu, width, nch):
    N = gpu
    tile, lane = TILE[width], LANE[width]
    sources, rows = plain_cases(width, nch)
    held = [len(b) // (width * nch) for b in sources]
    ntrack = 3 * tile - 6
    base = pcm(np.random.default_rng(width), width, ntrack, 0.3)
    # the list has the hard places
    for F in LENGTHS:
        assert {dst % 16 for dst, _i, _a, f, _n, _x in rows if f == F} == set(range(16))
    for F in LENGTHS:                                       # per region length: the three starts, a region on the buffer's last sample, one on its first
        mine = [(i, a) for _d, i, a, f, _n, _x in rows if f == F]
        assert {a for _i, a in mine} >= set(STARTS), F
        assert any(a + F == held[i] for i, a in mine) and any(a == 0 for _i, a in mine), F
    assert {x for *_r, x in rows} >= {1.0, 0.5, -0.8}
    assert any(dst < tile and dst + n > 2 * tile for dst, _i, _a, _F, n, _x in rows), "no note from tile 0 into tile 2"
    assert {(dst + n) % lane for dst, _i, _a, _F, n, _x in rows} == set(range(lane))        # an event's end at every position of a lane
    assert all(dst + n <= ntrack for dst, _i, _a, _F, n, _x in rows)
    want = plain_want(base, sources, rows, width, nch)
    assert want != plain_want(base, sources, rows, width, nch, reverse=False)             # what the parent mixes: the flag does something
    bufs = [N.DeviceBuffer.from_bytes(b) for b in sources]
    track = N.DeviceBuffer.from_bytes(base)
    table = event_table(N, "rev", [(dst, a * nch, n, F, f, 0.0, 0.0, i, RATE, RATE, nch, 0, 0, 0, 0, 0, 1) for dst, i, a, F, n, f in rows])
    assert mix_events(N, "rev", bufs, table, None, width, nch, track, ntrack) == N.SH_OK, N.lib().sh_last_error()
    got = track.download_bytes(len(base))
    assert got == want, "%d bytes differ" % differs(got, want)
    # and the same rows without the flag are rows of sh_mix_events_loop: the region forwards
    track = N.DeviceBuffer.from_bytes(base)
    table["flags"] = 0
    assert mix_events(N, "rev", bufs, table, None, width, nch, track, ntrack) == N.SH_OK, N.lib().sh_last_error()
    assert track.download_bytes(len(base)) == plain_want(base, sources, rows, width, nch, reverse=False)


def test_reversed_events_under_the_other_alignment_scheme(gpu):
    """SYNTHHIP_SEQ_ALIGN is read once per process (sh_init): the 16-bit cases again in a child under the scheme that is not the default"""
    in_a_child_under_the_other_alignment_scheme(__file__, ["test_plain_reversed_events_at_every_offset[2-1]", "test_plain_reversed_events_at_every_offset[2-2]",
                                                           "test_reversed_crossed_with_the_rest_of_the_chain[2]"])


# ---- 2: crossed with the rest, through Sample.mix_at_many ---------------------------------------------------------------------------------
_CACHE = {}
HELD = [300, 211, 97]                                       # frames of the instruments, mono and (a stereo track) stereo


def notes(width, nch=2, seed=0, scale=0.6, loud=False):
    """(instruments as (bytes, channels), events as (seconds, instrument, volume, other_seconds, speed, pan, envelope, loop, region,
    reverse)).  Events 0 .. 48: reversed regions under the seven speeds times the seven loop lengths.  Events 49 .. 97, seven each under
    the seven speeds: reversed without a loop (the whole sample; a region), a region forwards (looped; plain), reversed and looped
    without a region, neither (a looped note as it was), reversed with a region to the sample's end.  Pan, envelope (with a note
    length), volume and other_seconds on and off across them.  Made once, never changed."""
    key = (width, nch, seed, scale, loud)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(2000 * seed + 10 * width + nch)
    track_frames = 3 * TILE[width] // nch
    instruments = [(pcm(rng, width, n, scale), 1) for n in HELD]
    if nch == 2:
        instruments += [(pcm(rng, width, 2 * n, scale), 2) for n in HELD]
    events = []
    for k in range(98):
        speed = SPEEDS[k % 7]
        kind = 7 if k < 49 else (k - 49) // 7               # 7: reversed, region, loop
        reverse = [True, 1, None, False, "backwards", 0, True, True][kind]
        looped = kind in (2, 4, 5, 7)
        i = 2 if kind in (0, 6) else k % 3
        first = ([0, 1, 5, 12] if looped else [0, 1, 5, 40])[k % 4]
        if kind in (0, 4, 5):
            region, R = None, HELD[i]
        elif kind == 6:
            region, R = (first / RATE, None), HELD[i] - first
        else:
            R = HELD[i] - first - [0, 3, 7][k % 3] if looped else 20 + (7 * k) % 41
            region = (first / RATE, (first + R) / RATE)
        inrate = RATE if speed is None else int(RATE * speed)
        loop = None
        if looped:
            L = LOOPS[(k // 7) % 7]
            S = STARTS[k % 3] if k % 4 else R - L - (k % 2)           # a short head, or the loop at the end of what is played
            V = max(2, (150 + (37 * k) % 600) * inrate // RATE)
            loop = (S / RATE, (S + L) / RATE, V / RATE)
            R = V
        out = out_frames(R, inrate, RATE)
        pan = [0.3, (1.0, 0.0), -0.65, (1.5, 1.2)][k % 4] if (k & 1) and nch == 2 else None
        env = None
        if (k & 2) and width != 3:
            dur = (0.61 * out + 0.37) / RATE
            env = (0.113 * dur, 0.171 * dur, [0.5, 0.7, 1.0, 0.0, 0.25][k % 5], 0.233 * dur, dur)
            out = min(out, int(RATE * dur))
        volume = ([1.9, -1.9] if loud else [0.5, 1.7, -1.0, 0.8])[k % (2 if loud else 4)] if (k & 4) or loud else None
        other_seconds = (0.37 * out + 1) / RATE if k & 8 else None
        frame = int(rng.integers(0, track_frames - out + 1))
        events.append((frame / RATE, i + (3 if nch == 2 and pan is None else 0), volume, other_seconds, speed, pan, env, loop, region, reverse))
    _CACHE[key] = (instruments, events)
    return _CACHE[key]


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_reversed_crossed_with_the_rest_of_the_chain(gpu, width):
    from synthesizer_amd import mixer
    instruments, events = notes(width)
    turned = [e for e in events if e[9]]
    assert {e[4] for e in turned if e[7] is None} == set(SPEEDS)                                      # reversed with each speed
    assert {(e[4], round(RATE * (e[7][1] - e[7][0]))) for e in turned if e[7] is not None} >= {(sp, L) for sp in SPEEDS for L in LOOPS}
    assert any(e[5] is not None for e in turned) and any(e[5] is None for e in turned)                # mono panned, and stereo
    assert any(e[6] is not None and len(e[6]) == 5 for e in turned) or width == 3                     # an envelope and a length
    assert any(e[8] is not None and not e[9] for e in events) and any(e[8] is None and not e[9] for e in events)
    assert any(e[8] is not None and e[8][1] is None for e in turned)
    if width == 3:
        assert any(e[7] is not None for e in turned)                                                  # 24-bit, reversed and looped
    want = mix(b"", named(instruments, events), width, RATE, 2)
    assert 2 * TILE[width] * width < len(want) <= 3 * TILE[width] * width
    # on the parent the ninth and tenth element do nothing: other bytes
    assert want != mix(b"", [e[:8] + (None, None) for e in named(instruments, events)], width, RATE, 2)
    discriminates(want, named(instruments, events), width, RATE, 2, "rev")
    samples = as_samples(instruments, width, RATE)
    got = mixer.sequence(with_samples(samples, events), RATE, 2, width, name="turned")
    assert got.name == "turned" and len(got) * 2 * width == len(want)
    assert bytes(got.view_frame_data()) == want, "%d bytes differ" % differs(bytes(got.view_frame_data()), want)
    for (b, c), smp in zip(instruments, samples):
        assert bytes(smp.view_frame_data()) == b and smp.nchannels == c                 # the instruments are untouched


@pytest.mark.parametrize("nch", [1, 2])
def test_reversed_into_a_track_that_holds_something(gpu, nch, monkeypatch):
    N = gpu
    instruments, events = notes(2, nch)
    base = pcm(np.random.default_rng(5), 2, 3 * TILE[2], 0.3)
    want = mix(base, named(instruments, events), 2, RATE, nch)
    calls = spy(N, monkeypatch)
    got = sample_of(base, 2, RATE, nch).mix_at_many(with_samples(as_samples(instruments, 2, RATE), events))
    assert calls == ["sh_mix_events_rev"]                                                # one launch
    assert bytes(got.view_frame_data()) == want


# ---- 3: what reversed means for a stereo sample ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_a_reversed_stereo_sample_comes_backwards_with_left_and_right_swapped(gpu, width):
    """audioop.reverse turns the order of the SAMPLES round: frame f of the reversed region is frame F - 1 - f of the region with its
    channels in the other order.  Stated on the frames themselves, with numpy, and held against audioop and the product."""
    rng = np.random.default_rng(60 + width)
    F, a, b = 200, 30, 171
    data = pcm(rng, width, 2 * F, 0.9)
    frames = np.frombuffer(data, dtype=np.uint8).reshape(F, 2, width)                    # frame, channel, byte
    swapped = frames[a:b][::-1, ::-1, :].tobytes()                                       # frames backwards AND left <-> right
    framewise = frames[a:b][::-1, :, :].tobytes()                                        # what a frame-wise reversal would be
    assert swapped == audioop.reverse(data[a * 2 * width:b * 2 * width], width) != framewise
    event = (8 / RATE, sample_of(data, width, RATE, 2), None, None, None, None, None, None, (a / RATE, b / RATE), True)
    got = bytes(sample_of(b"", width, RATE, 2).mix_at_many([event]).view_frame_data())
    assert got == bytes(8 * 2 * width) + swapped
    left_in = frames[a:b, 0, :].tobytes()
    got_frames = np.frombuffer(got, dtype=np.uint8).reshape(-1, 2, width)[8:]
    assert got_frames[::-1, 1, :].tobytes() == left_in                                   # the source's left channel plays on the right
    # a mono sample panned: nothing to swap, the frames come backwards
    mono = pcm(rng, width, F, 0.9)
    m = np.frombuffer(mono, dtype=np.uint8).reshape(F, width)
    want = audioop.tostereo(m[a:b][::-1].tobytes(), width, 1.0, 0.0)
    got = sample_of(b"", width, RATE, 2).mix_at_many([(0.0, sample_of(mono, width, RATE, 1), None, None, None, (1.0, 0.0), None, None, (a / RATE, b / RATE), True)])
    assert bytes(got.view_frame_data()) == want


# ---- 4: a region without a reversal, at every level -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_a_region_forwards_goes_to_the_entry_point_of_its_level(gpu, width, monkeypatch):
    N = gpu
    rng = np.random.default_rng(70 + width)
    mono, stereo = pcm(rng, width, 300, 0.6), pcm(rng, width, 2 * 211, 0.6)
    env = (0.002, 0.003, 0.5, 0.004, 0.02) if width != 3 else None
    region, tail = (5 / RATE, 190 / RATE), (100 / RATE, None)
    tiers = [
        ("sh_mix_events", [(0.01, 1, 0.5, None, None, None, None, None, region, None), (0.3, 1, None, 0.01, None, None, None, None, tail, False)]),
        ("sh_mix_events_rate", [(0.01, 1, 0.5, None, 0.37, None, None, None, region, None), (0.1, 1, None, None, 2.5, None, None, None, tail, None)]),
        ("sh_mix_events_pan", [(0.01, 0, 0.5, None, 0.37, 0.3, None, None, region, None), (0.1, 1, None, None, None, None, None, None, tail, None)]),
        ("sh_mix_events_env", [(0.01, 0, 0.5, None, 1.001, 0.3, env, None, region, None), (0.1, 1, None, None, None, None, env, None, tail, None)]),
        ("sh_mix_events_loop", [(0.01, 0, 0.5, None, 0.999, 0.3, env, (0.01, 0.5, 0.09), region, None), (0.1, 1, None, None, None, None, None, None, tail, None)]),
    ]
    instruments = [(mono, 1), (stereo, 2)]
    calls = spy(N, monkeypatch)
    for entry, events in tiers:
        if width == 3 and entry == "sh_mix_events_env":
            continue                                        # (no envelope at 24 bits: the list would be the pan level's again)
        del calls[:]
        want = mix(b"", named(instruments, events), width, RATE, 2)
        assert want != mix(b"", [e[:8] + (None, None) for e in named(instruments, events)], width, RATE, 2)
        got = sample_of(b"", width, RATE, 2).mix_at_many(with_samples(as_samples(instruments, width, RATE), events))
        assert calls == [entry]
        assert bytes(got.view_frame_data()) == want, entry
    # an empty region: nothing is mixed, the track grows to the event's start
    del calls[:]
    got = sample_of(b"", width, RATE, 2).mix_at_many([(0.01, sample_of(stereo, width, RATE, 2), None, None, None, None, None, None, (0.5, 0.6), True)])
    assert bytes(got.view_frame_data()) == bytes(2 * width * int(RATE * 0.01))


# ---- 5: the order ------------------------------------------------------------------------------------------------------------------------
def order_notes(width):
    """every event has a region, a reversal, a loop and a speed, so that every wrong order can be formed for every event"""
    rng = np.random.default_rng(80 + width)
    instruments = [(pcm(rng, width, 400, 0.6), 1), (pcm(rng, width, 2 * 300, 0.6), 2)]
    events = []
    for k in range(24):
        i = k % 2
        speed = [0.5, 0.8, 1.5, 2 ** (3 / 12)][k % 4]
        S, L = [40, 41, 45][k % 3], LOOPS[2 + k % 5]
        events.append((int(rng.integers(0, 900)) / RATE, i, [None, 0.7][k % 2], None, speed, 0.3 if i == 0 else None, None,
                       (S / RATE, (S + L) / RATE, (300 + 11 * k) / RATE), ((3 + k) / RATE, (250 - 2 * k) / RATE), True))
    return instruments, events


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_the_oracle_tells_the_right_order_from_each_wrong_one(gpu, width):
    instruments, events = order_notes(width)
    want = mix(b"", named(instruments, events), width, RATE, 2)
    discriminates(want, named(instruments, events), width, RATE, 2, "rev")
    got = sample_of(b"", width, RATE, 2).mix_at_many(with_samples(as_samples(instruments, width, RATE), events))
    assert bytes(got.view_frame_data()) == want


# ---- 6: saturation in list order -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_loud_reversed_events_saturate_in_list_order(gpu, width):
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


# ---- 7: the product's own loop of calls ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width, nch", [(2, 2), (1, 1), (3, 2), (4, 2)])
def test_the_same_bytes_as_the_documented_loop_of_sample_calls(gpu, width, nch):
    instruments, events = notes(width, nch)
    events = events[:21:2] + events[49::3]
    samples = as_samples(instruments, width, RATE)
    base = pcm(np.random.default_rng(9), width, 3 * TILE[width], 0.3)
    loop_ = sample_of(base, width, RATE, nch)
    for seconds, i, volume, other_seconds, speed, pan, envelope, loop, region, reverse in events:
        other = samples[i]
        o = other
        if region is not None:
            o = other.copy().clip(region[0], other.duration if region[1] is None else region[1])
        if reverse:
            o = o.copy().reverse()
        if loop is not None:
            ls, le, length = loop
            body = o.copy().clip(ls, le)
            o = o.copy().clip(0.0, le)
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


# ---- 8: the track as a source ------------------------------------------------------------------------------------------------------------------
def test_the_track_as_a_reversed_region_of_itself(gpu, monkeypatch):
    N = gpu
    width, nch = 2, 2
    instruments, events = notes(width, nch)
    samples = as_samples(instruments, width, RATE)
    calls = spy(N, monkeypatch)
    base = pcm(np.random.default_rng(3), width, 3 * TILE[width], 0.3)
    t = sample_of(base, width, RATE, nch)
    first, last = events[:30], events[30:50]
    own = (0.05, None, 0.4, None, 1.5, None, (0.02, 0.03, 0.5, 0.05, 0.2), (100 / RATE, 171 / RATE, 0.4), (0.01, 0.1), True)
    tail = (0.02, None, -0.6, 0.05, None, None, None, None, (0.3, None), True)           # to the end of the track as it is then
    t.mix_at_many(with_samples(samples, first) + [own[:1] + (t,) + own[2:], tail[:1] + (t,) + tail[2:]] + with_samples(samples, last))
    assert calls == ["sh_mix_events_rev", "sh_mix_events_rev"]                           # the list is cut at the track; one launch per side
    mid = mix(base, named(instruments, first), width, RATE, nch)
    mid = mix(mid, [own[:1] + (mid,) + own[2:]], width, RATE, nch)
    assert mid != mix(mid, [own[:1] + (mid,) + own[2:8] + (None, None)], width, RATE, nch)
    mid = mix(mid, [tail[:1] + (mid,) + tail[2:]], width, RATE, nch)
    assert bytes(t.view_frame_data()) == mix(mid, named(instruments, last), width, RATE, nch)


# ---- 9: the entry point ------------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_refuses_on_the_host_and_leaves_the_track(gpu):
    N = gpu
    rng = np.random.default_rng(27)
    src, base = pcm(rng, 2, 1000), pcm(rng, 2, 5000)
    s, t = N.DeviceBuffer.from_bytes(src), N.DeviceBuffer.from_bytes(base)
    nan = float("nan")
    segs = np.zeros(1, dtype=N.ENV_SEGMENT_DTYPE)
    segs[0] = (100, 0, 0.5, 0.0, 0.0, 0.0, 0, 0)
    # 500 stereo frames in the source.  A good reversed row: frames 100 .. 400 backwards; a good reversed looped row: the 300 frames from
    # frame 150 on played backwards, played frames 100 .. 300 held for 900 frames
    ok = (100, 200, 600, 300, 0.5, 0.0, 0.0, 0, 8000, 8000, 2, 0, 0, 0, 0, 0, 1)
    held = (100, 300, 1800, 900, 0.5, 0.0, 0.0, 0, 8000, 8000, 2, 0, 0, 0, 100, 200, 1)
    mono = (100, 100, 600, 300, 0.5, 0.3, 0.7, 0, 8000, 8000, 1, 0, 0, 0, 0, 0, 1)     # 1000 mono frames through tostereo
    bad = {
        # what sh_mix_events_loop refuses
        "source index": (ok[:7] + (1,) + ok[8:], b"no source"),
        "nan factor": (ok[:4] + (nan,) + ok[5:], b"factor is not finite"),
        "reserved": (ok[:13] + (7,) + ok[14:], b"reserved must be 0"),
        "inrate 0": (ok[:8] + (0,) + ok[9:], b"sampling rate"),
        "src_channels 3": (ok[:10] + (3,) + ok[11:], b"src_channels 3"),
        "nan left": (mono[:5] + (nan,) + mono[6:], b"left / right"),
        "odd dst_sample of a mono source": ((101,) + mono[1:], b"whole stereo frames"),
        "range outside the track": ((4500,) + ok[1:], b"range outside the track"),
        "an unflagged row's range outside its source": ((0, 996, 10, 0, 1.0, 0.0, 0.0, 0, 8000, 8000, 2, 0, 0, 0, 0, 0, 0), b"range outside its source"),
        "segments outside the table": (ok[:11] + (1, 1) + ok[13:], b"segments outside the table"),
        "the loop beyond the source": (held[:14] + (400, 101, 1), b"loop outside its source"),
        "a looped row's nsamples off whole frames": (held[:2] + (1799,) + held[3:], b"whole frames"),
        # and what the flags add
        "an unknown flag bit": (ok[:16] + (3,), b"unknown flags"),
        "an unknown flag bit alone": (ok[:16] + (2,), b"unknown flags"),
        "a high flag bit": (ok[:16] + (0x80000001,), b"unknown flags"),
        "a reversed region off whole frames": (ok[:1] + (201,) + ok[2:], b"region starts on a whole frame"),
        "a reversed region beyond its source": (ok[:3] + (401,) + ok[4:], b"reversed region outside its source"),
        "a reversed region beyond what src_sample leaves": (ok[:1] + (800, 200, 101) + ok[4:], b"reversed region outside its source"),
        "a reversed resampled region beyond its source": (ok[:3] + (401,) + ok[4:8] + (4000,) + ok[9:], b"reversed region outside its source"),
        "more samples than the reversed region holds": (ok[:2] + (602,) + ok[3:], b"more samples than src_frames hold"),
    }
    for what, (row, message) in bad.items():
        rows = [ok, row]
        assert mix_events(N, "rev", [s], event_table(N, "rev", rows), segs, 2, 2, t, 5000) == N.SH_ERR_INVALID, what
        err = N.lib().sh_last_error()
        assert err.startswith(b"sh_mix_events_rev") and b"event 1" in err and message in err, (what, err)
        assert t.download_bytes(len(base)) == base, what
    # width 3 with segments; width 3 without them may play backwards
    s3, t3 = N.DeviceBuffer.from_bytes(bytes(3000)), N.DeviceBuffer.from_bytes(bytes(15000))
    shaped = ok[:11] + (0, 1) + ok[13:]
    assert mix_events(N, "rev", [s3], event_table(N, "rev", [ok, shaped]), segs, 3, 2, t3, 5000) == N.SH_ERR_INVALID
    assert b"event 1" in N.lib().sh_last_error()
    assert t3.download_bytes(15000) == bytes(15000)
    assert mix_events(N, "rev", [s3], event_table(N, "rev", [ok]), None, 3, 2, t3, 5000) == N.SH_OK, N.lib().sh_last_error()
    for width in (0, 5, -2):
        assert mix_events(N, "rev", [s], event_table(N, "rev", [ok]), None, width, 2, t, 5000) == N.SH_ERR_INVALID
    assert mix_events(N, "rev", [s], event_table(N, "rev", [ok]), None, 2, 0, t, 5000) == N.SH_ERR_INVALID
    assert mix_events(N, "rev", [s, t], event_table(N, "rev", [ok]), None, 2, 2, t, 5000) == N.SH_ERR_INVALID        # a source that is the track
    assert mix_events(N, "rev", [s], event_table(N, "rev", [ok]), None, 2, 2, t, 5001) == N.SH_ERR_INVALID
    assert mix_events(N, "rev", [s], event_table(N, "rev", []), None, 2, 2, t, 5000) == N.SH_OK
    assert t.download_bytes(len(base)) == base                                                          # nothing was launched
    # and what it accepts: the reversed region, the reversed held note, then the mono one through tostereo
    assert mix_events(N, "rev", [s], event_table(N, "rev", [ok, held, mono]), None, 2, 2, t, 5000) == N.SH_OK, N.lib().sh_last_error()
    want = bytearray(base)
    x = audioop.mul(audioop.reverse(src[400:1600], 2), 2, 0.5)
    want[200:1400] = audioop.add(base[200:1400], x, 2)
    turned = audioop.reverse(src[600:1800], 2)              # the 300 frames from frame 150 on
    x = audioop.mul(unroll(turned, 2, 2, RATE, (100 / RATE, 300 / RATE, 900 / RATE)), 2, 0.5)
    want[200:3800] = audioop.add(bytes(want[200:3800]), x, 2)
    x = audioop.mul(audioop.tostereo(audioop.reverse(src[200:800], 2), 2, 0.3, 0.7), 2, 0.5)
    want[200:1400] = audioop.add(bytes(want[200:1400]), x, 2)
    assert t.download_bytes(len(base)) == bytes(want)
