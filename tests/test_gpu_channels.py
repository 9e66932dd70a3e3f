"""GPU parity of ``channels`` per event in Sample.mix_at_many / mixer.sequence / sh_mix_events_chan -- a stereo sample downmixed into a mono
track (audioop.tomono) or balanced in a stereo one, in one launch -- against live ``audioop`` on byte slices.  The reference is
tests/seqref.py (source, mix): the chain as it stands, run over the STEREO source up to the envelope, then the new step --
``audioop.tomono(data, w, lf, rf)`` for a downmix; for a balance ``tomono(1, 0)`` -> ``mul(lf)`` -> ``tostereo(1, 0)`` added with
``audioop.add`` to its right-hand twin -- then ``mul``, the cut of ``other_seconds`` in TRACK samples, ``add`` with saturation at every
event, in list order.  Expected bytes never come from the product.  Rate 8192, sources of a few hundred frames, tracks of three tiles, as
the sibling files have them."""
import audioop

import numpy as np
import pytest

from tests.helpers import pcm_track_call
from tests.seqcases import (FACTORS, LENGTHS, LOOPS, SPEEDS, STARTS, as_samples, event_table, in_a_child_under_the_other_alignment_scheme, mix_events,
                            named, sample_of, spy, with_samples)
from tests.seqref import LANE, TILE, balance, differs, discriminates, mix, out_frames, pcm, weigh

pytestmark = pytest.mark.gpu

RATE = 8192
HELD = [300, 211, 97]                                       # frames of the instruments, stereo and mono


# ---- 1: plain downmixes and balances, through the entry point (track offsets count samples there) -------------------------------------------
_PLAIN = {}


def plain_cases(width, nch):
    """(sources, base, rows as (dst_sample, source, src_sample, nsamples, factor, lf, rf), expected bytes), made once.  Every length at
    every source residue 0 .. 15, the lane residues of the start in turn; an event that ends one short of, at and one past each tile
    boundary; notes from tile 0 into tile 2.  Source 0 is loud (saturation under lf = rf = 1), the others hold odd negatives enough."""
    if (width, nch) in _PLAIN:
        return _PLAIN[(width, nch)]
    rng = np.random.default_rng(30 * width + nch)
    tile, lane = TILE[width], LANE[width]
    per = 2 // nch                                          # source samples per track sample
    held = (400, 311, tile * per + 900)                     # samples
    sources = [pcm(rng, width, held[0], 1.0), pcm(rng, width, held[1], 0.5), pcm(rng, width, held[2], 0.5)]
    ntrack = 3 * tile - 6
    base = pcm(np.random.default_rng(width), width, ntrack, 0.3)
    rows = []
    k = 0
    for F in LENGTHS:                                       # frames
        n = F * nch
        for off in range(16):
            i = k % 2
            a = [32, 64, 48][k % 3] + off
            if k % 5 == 0:
                a = held[i] - per * n - (held[i] - per * n - off) % 16          # as far back as the residue allows
            if k % 5 == 1:
                a = off
            dst = [40, tile - 96, 2 * tile - 24, tile + 500][k % 4] + (k // 3) % lane
            if nch == 2:
                dst -= dst % 2                              # a balance starts on a whole stereo frame
            lf, rf = [(1.0, 1.0), (0.5, 0.5), (1.0, 0.0), (0.0, 1.0), (0.75, -0.25), (1.5, 1.2)][k % 6]
            rows.append((dst, i, a, n, [1.0, 0.5, -0.8][k % 3], lf, rf))
            k += 1
    for edge in (tile, 2 * tile):                           # ends one short of, at and one past a tile boundary
        for d in (-1, 0, 1):
            rows.append((edge - 34, 1, 7 + d, 34 + d, 1.0, 0.5, 0.5))
    for j in range(6):                                      # from tile 0 over tile 1 into tile 2
        n = tile + 300 + 2 * j
        rows.append((tile - 200 - 2 * j, 2, j, n, 0.25, [0.5, 1.0][j % 2], [0.5, 0.3][j % 2]))
    want = bytearray(base)
    for dst, i, a, n, factor, lf, rf in rows:
        assert (a + per * n) * width <= len(sources[i]) and dst + n <= ntrack
        data = weigh(sources[i][a * width:(a + per * n) * width], width, nch, lf, rf)
        if factor != 1.0:
            data = audioop.mul(data, width, factor)
        lo, hi = dst * width, dst * width + len(data)
        assert hi - lo == n * width
        want[lo:hi] = audioop.add(bytes(want[lo:hi]), data, width)
    _PLAIN[(width, nch)] = (sources, base, rows, bytes(want))
    return _PLAIN[(width, nch)]


def _plain_table(N, rows, nch):
    flag = N.MIX_EVENT_DOWNMIX if nch == 1 else N.MIX_EVENT_BALANCE
    return event_table(N, "chan", [(dst, a, n, 0, f, lf, rf, i, RATE, RATE, 2, 0, 0, 0, 0, 0, flag) for dst, i, a, n, f, lf, rf in rows])


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_plain_downmix_and_balance_at_every_offset(gpu, width, nch):
    N = gpu
    tile, lane = TILE[width], LANE[width]
    sources, base, rows, want = plain_cases(width, nch)
    per = 2 // nch
    ntrack = len(base) // width
    # the list has the hard places
    starts = set(range(lane)) if nch == 1 else set(range(0, lane, 2))
    assert {dst % lane for dst, *_r in rows} == starts
    for F in LENGTHS:
        mine = [r for r in rows[:16 * len(LENGTHS)] if r[3] == F * nch]
        assert {a % 16 for _d, _i, a, *_r in mine} == set(range(16)), F
    # where the source's samples lie against the lane's: every shift of the funnel, and the aligned case
    assert {(a - per * dst) % (per * lane) for dst, _i, a, *_r in rows} == set(range(per * lane))
    for edge in (tile, 2 * tile):
        assert {dst + n - edge for dst, _i, _a, n, *_r in rows} >= {-1, 0, 1}
    assert any(dst < tile and dst + n > 2 * tile for dst, _i, _a, n, *_r in rows), "no note from tile 0 into tile 2"
    assert {(lf, rf) for *_r, lf, rf in rows} >= {(1.0, 1.0), (0.5, 0.5), (1.0, 0.0), (0.0, 1.0)}
    # the factors do what they are there for: lf = rf = 1 saturates (a downmix), 0.5 floors an odd negative
    hi = 2 ** (8 * width - 1) - 1
    for dst, i, a, n, f, lf, rf in rows:
        if i == 0 and n >= 16 and (lf, rf) == (1.0, 1.0) and nch == 1:
            x = weigh(sources[i][a * width:(a + 2 * n) * width], width, 1, 1.0, 1.0)
            if audioop.max(x, width) >= hi:
                break
    else:
        assert nch == 2, "no downmix saturates"
    v = np.frombuffer(sources[1], dtype=np.uint8).reshape(-1, width)
    assert ((v[:, 0] & 1) == 1).any() and (v[:, -1] >= 128).any()
    assert want != base
    wrong = bytearray(base)                                 # what the rows are without their mode: other bytes (a mono track refuses them)
    bufs = [N.DeviceBuffer.from_bytes(b) for b in sources]
    track = N.DeviceBuffer.from_bytes(base)
    table = _plain_table(N, rows, nch)
    assert mix_events(N, "chan", bufs, table, None, width, nch, track, ntrack) == N.SH_OK, N.lib().sh_last_error()
    got = track.download_bytes(len(base))
    assert got == want, "%d bytes differ" % differs(got, want)
    # the same rows without the mode: a stereo source in a mono track is refused; in a stereo track they are rows of sh_mix_events_rev
    track = N.DeviceBuffer.from_bytes(base)
    table["flags"] = 0
    if nch == 1:
        assert mix_events(N, "chan", bufs, table, None, width, nch, track, ntrack) == N.SH_ERR_INVALID
        assert track.download_bytes(len(base)) == base
    else:
        for dst, i, a, n, f, _lf, _rf in rows:
            data = sources[i][a * width:(a + n) * width]
            data = audioop.mul(data, width, f) if f != 1.0 else data
            wrong[dst * width:(dst + n) * width] = audioop.add(bytes(wrong[dst * width:(dst + n) * width]), data, width)
        assert mix_events(N, "chan", bufs, table, None, width, nch, track, ntrack) == N.SH_OK, N.lib().sh_last_error()
        assert track.download_bytes(len(base)) == bytes(wrong) != want


def test_channels_under_the_other_alignment_scheme(gpu):
    """SYNTHHIP_SEQ_ALIGN is read once per process (sh_init): the 16-bit cases again in a child under the scheme that is not the default"""
    in_a_child_under_the_other_alignment_scheme(__file__, ["%s[2-%d]" % (t, n) for t in ("test_plain_downmix_and_balance_at_every_offset", "test_channels_crossed_with_the_rest_of_the_chain")
                                                           for n in (1, 2)])


# ---- 2, 3: each stage with the new one, through Sample.mix_at_many; the order ------------------------------------------------------------------
_CACHE = {}


def notes(width, nch, seed=0):
    """(instruments as (bytes, channels): 0 .. 2 stereo, 3 .. 5 mono; events as (seconds, instrument, volume, other_seconds, speed, pan,
    envelope, loop, region, reverse, channels)).  84 events under the seven speeds: five of every six weigh a stereo instrument, the
    sixth is the track's other kind of row (a panned mono instrument or a plain stereo one in a stereo track, a plain mono one in a mono
    track); region, reverse, loop, envelope (with a note length), volume and other_seconds on and off across them.  Made once."""
    key = (width, nch, seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(3000 * seed + 10 * width + nch)
    track_frames = 3 * TILE[width] // nch
    instruments = [(pcm(rng, width, 2 * n, 0.6), 2) for n in HELD] + [(pcm(rng, width, n, 0.6), 1) for n in HELD]
    events = []
    for k in range(84):
        speed = SPEEDS[k % 7]
        weighed = k % 6 != 5
        i = k % 3
        R = HELD[i]
        region = None
        if k % 4 in (1, 2):
            first = [0, 1, 5, 12][(k // 4) % 4]
            if k % 4 == 1:
                R = R - first - [0, 3, 7][k % 3]
                region = (first / RATE, (first + R) / RATE)
            else:
                R = R - first
                region = (first / RATE, None)
        reverse = bool(k % 3 != 1)
        inrate = RATE if speed is None else int(RATE * speed)
        loop = None
        looped = k % 5 in (0, 3)
        if speed == 0.1 and not looped:                     # ten times as long: a short slice, so that the note fits the track
            first, R = [0, 1, 5, 12][(k // 4) % 4], 20 + (7 * k) % 41
            region = (first / RATE, (first + R) / RATE)
        if looped:
            L = LOOPS[(k // 5) % 7]
            S = STARTS[k % 3] if k % 2 else R - L - (k % 3)             # a short head, or the loop at the end of what is played
            V = max(2, (150 + (37 * k) % 500) * inrate // RATE)
            loop = (S / RATE, (S + L) / RATE, V / RATE)
            R = V
        out = out_frames(R, inrate, RATE)
        env = None
        if (k & 2) and width != 3:
            dur = (0.61 * out + 0.37) / RATE
            env = (0.113 * dur, 0.171 * dur, [0.5, 0.7, 1.0, 0.0, 0.25][k % 5], 0.233 * dur, dur)
            out = min(out, int(RATE * dur))
        volume = [0.5, 1.7, -1.0, 0.8][k % 4] if k & 4 else None
        other_seconds = (0.37 * out + 1) / RATE if k & 8 else None
        frame = int(rng.integers(0, track_frames - out + 1))
        pan = None
        if weighed:
            channels = FACTORS[k % 7]
        else:
            channels = None
            if nch == 1 or k % 12 == 5:
                i += 3                                      # a mono instrument: plain in a mono track, panned in a stereo one
                pan = [0.3, (1.5, 1.2)][k % 2] if nch == 2 else None
        events.append((frame / RATE, i, volume, other_seconds, speed, pan, env, loop, region, reverse, channels))
    _CACHE[key] = (instruments, events)
    return _CACHE[key]


def _has_every_stage(events, width, nch):
    mine = [e for e in events if e[10] is not None]
    assert any(e[4] is not None and e[4] < 1 for e in mine) and any(e[4] is not None and e[4] > 1 for e in mine)      # ratecv up and down
    assert any(e[6] is not None and e[6][0] > 0 for e in mine) or width == 3                                          # ramps
    assert any(e[7] is not None for e in mine)                                                                        # a loop
    assert any(e[8] is not None and e[9] and e[10][0] != e[10][1] for e in mine)                                      # region, reverse, lf != rf
    assert any(e[3] is not None for e in mine) and any(e[2] is not None for e in mine)                                # other_seconds, volume
    assert any(e[7] is not None and e[9] and e[4] is not None and (e[6] is not None or width == 3) for e in mine)      # all of them at once
    others = [e for e in events if e[10] is None]
    if nch == 2:
        assert any(e[5] is not None for e in others) and any(e[5] is None for e in others)                            # pan rows and plain stereo rows
    else:
        assert others and all(e[1] >= 3 for e in others)                                                              # plain mono rows


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_channels_crossed_with_the_rest_of_the_chain(gpu, width, nch, monkeypatch):
    """a track that grows: every kind of row in one list, one launch"""
    N = gpu
    from synthesizer_amd import mixer
    instruments, events = notes(width, nch)
    _has_every_stage(events, width, nch)
    want = mix(b"", named(instruments, events), width, RATE, nch)
    assert 2 * TILE[width] * width < len(want) <= 3 * TILE[width] * width
    discriminates(want, named(instruments, events), width, RATE, nch, "chan")
    samples = as_samples(instruments, width, RATE)
    calls = spy(N, monkeypatch)
    got = mixer.sequence(with_samples(samples, events), RATE, nch, width, name="weighed")
    assert calls == ["sh_mix_events_chan"]                                               # one launch
    assert got.name == "weighed" and got.nchannels == nch and len(got) * nch * width == len(want)
    assert bytes(got.view_frame_data()) == want, "%d bytes differ" % differs(bytes(got.view_frame_data()), want)
    for (b, c), smp in zip(instruments, samples):
        assert bytes(smp.view_frame_data()) == b and smp.nchannels == c                 # the instruments are untouched


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("width", [2, 3])
def test_channels_into_a_track_that_holds_something(gpu, width, nch, monkeypatch):
    """mixed in place over a base that is not silence"""
    N = gpu
    instruments, events = notes(width, nch, seed=1)
    base = pcm(np.random.default_rng(5), width, 3 * TILE[width], 0.3)
    want = mix(base, named(instruments, events), width, RATE, nch)
    discriminates(want, named(instruments, events), width, RATE, nch, "chan", base)
    calls = spy(N, monkeypatch)
    got = sample_of(base, width, RATE, nch).mix_at_many(with_samples(as_samples(instruments, width, RATE), events))
    assert calls == ["sh_mix_events_chan"]
    assert bytes(got.view_frame_data()) == want


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_each_stage_alone_with_a_downmix_and_with_a_balance(gpu, width):
    """one stage and the new step per list, so that a failure names its stage"""
    rng = np.random.default_rng(90 + width)
    src = pcm(rng, width, 2 * 300, 0.9)
    env = (0.004, 0.006, 0.5, 0.008, 0.03)
    stages = {
        "speed up": dict(speed=2.5), "speed down": dict(speed=0.37),
        "envelope": dict(envelope=env),
        "loop": dict(loop=(5 / RATE, 70 / RATE, 500 / RATE)),
        "region reversed": dict(region=(12 / RATE, 250 / RATE), reverse=True),
        "reversed": dict(reverse=True),
        "other_seconds": dict(other_seconds=101 / RATE),
        "volume": dict(volume=-1.7),
    }
    for nch in (1, 2):
        for what, kw in stages.items():
            if what == "envelope" and width == 3:
                continue
            e = (9 / RATE, None, kw.get("volume"), kw.get("other_seconds"), kw.get("speed"), None, kw.get("envelope"), kw.get("loop"),
                 kw.get("region"), kw.get("reverse"), (0.75, -0.5))
            want = mix(b"", [e[:1] + (src,) + e[2:]], width, RATE, nch)
            assert want != mix(b"", [e[:1] + (src,) + e[2:10] + ((1.0, 0.0),)], width, RATE, nch)
            got = sample_of(b"", width, RATE, nch).mix_at_many([e[:1] + (sample_of(src, width, RATE, 2),) + e[2:]])
            assert bytes(got.view_frame_data()) == want, (what, nch)
    # (1.0, 0.0) into a mono track is Sample.left(); (1.0, 1.0) in a stereo one the plain event
    got = sample_of(b"", width, RATE, 1).mix_at_many([(0.0, sample_of(src, width, RATE, 2), None, None, None, None, None, None, None, None, (1.0, 0.0))])
    assert bytes(got.view_frame_data()) == audioop.tomono(src, width, 1, 0) == bytes(sample_of(src, width, RATE, 2).left().view_frame_data())
    got = sample_of(b"", width, RATE, 2).mix_at_many([(0.0, sample_of(src, width, RATE, 2), None, None, None, None, None, None, None, None, (1.0, 1.0))])
    assert bytes(got.view_frame_data()) == src


@pytest.mark.parametrize("width, nch", [(2, 1), (2, 2), (3, 1), (1, 2), (4, 1)])
def test_the_same_bytes_as_the_documented_loop_of_sample_calls(gpu, width, nch):
    instruments, events = notes(width, nch)
    events = events[:84:5]
    samples = as_samples(instruments, width, RATE)
    base = pcm(np.random.default_rng(9), width, 3 * TILE[width], 0.3)
    loop_ = sample_of(base, width, RATE, nch)
    for seconds, i, volume, other_seconds, speed, pan, envelope, loop, region, reverse, channels in events:
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
        if channels is not None:
            lf, rf = channels
            o = o.copy().mono(lf, rf) if nch == 1 else o.copy().stereo(lf, rf)
        if volume is not None:
            o = o.at_volume(volume)
        loop_.mix_at(seconds, o, other_seconds)
    many = sample_of(base, width, RATE, nch).mix_at_many(with_samples(samples, events))
    assert len(many) == len(loop_)
    assert bytes(many.view_frame_data()) == bytes(loop_.view_frame_data()) == mix(base, named(instruments, events), width, RATE, nch)


def test_the_track_as_its_own_balanced_source(gpu, monkeypatch):
    N = gpu
    width, nch = 2, 2
    instruments, events = notes(width, nch)
    samples = as_samples(instruments, width, RATE)
    calls = spy(N, monkeypatch)
    base = pcm(np.random.default_rng(3), width, 3 * TILE[width], 0.3)
    t = sample_of(base, width, RATE, nch)
    first, last = events[:20], events[20:40]
    own = (0.05, None, 0.4, 0.1, 1.5, None, None, None, (0.01, 0.2), True, (0.75, -0.25))
    t.mix_at_many(with_samples(samples, first) + [own[:1] + (t,) + own[2:]] + with_samples(samples, last))
    assert calls == ["sh_mix_events_chan", "sh_mix_events_chan"]                         # the list is cut at the track; one launch per side
    mid = mix(base, named(instruments, first), width, RATE, nch)
    mid = mix(mid, [own[:1] + (mid,) + own[2:]], width, RATE, nch)
    assert bytes(t.view_frame_data()) == mix(mid, named(instruments, last), width, RATE, nch)


# ---- 4: the entry point --------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_refuses_on_the_host_and_leaves_the_track(gpu):
    N = gpu
    rng = np.random.default_rng(28)
    src, base = pcm(rng, 2, 1000), pcm(rng, 2, 5000)
    s, t = N.DeviceBuffer.from_bytes(src), N.DeviceBuffer.from_bytes(base)
    nan = float("nan")
    D, B, R = N.MIX_EVENT_DOWNMIX, N.MIX_EVENT_BALANCE, N.MIX_EVENT_REVERSED
    segs = np.zeros(1, dtype=N.ENV_SEGMENT_DTYPE)
    segs[0] = (100, 0, 0.5, 0.0, 0.0, 0.0, 0, 0)
    # 500 stereo frames in the source.  Good rows: frames 100 .. 400 downmixed to 300 mono samples; the same backwards; balanced
    down = (100, 200, 300, 300, 0.5, 0.75, -0.25, 0, 8000, 8000, 2, 0, 0, 0, 0, 0, D)
    back = down[:16] + (D | R,)
    bal = (100, 200, 600, 300, 0.5, 0.75, -0.25, 0, 8000, 8000, 2, 0, 0, 0, 0, 0, B)
    plain = (0, 10, 20, 0, 1.0, 0.0, 0.0, 0, 8000, 8000, 1, 0, 0, 0, 0, 0, 0)            # a mono source in the mono track
    for nch, ok, bad in ((1, down, {
        # what sh_mix_events_rev refuses
        "source index": (down[:7] + (1,) + down[8:], b"no source"),
        "nan factor": (down[:4] + (nan,) + down[5:], b"factor is not finite"),
        "reserved": (down[:13] + (7,) + down[14:], b"reserved must be 0"),
        "inrate 0": (down[:8] + (0,) + down[9:], b"sampling rate"),
        "a stereo source in a mono track without the mode": (down[:16] + (0,), b"src_channels 2"),
        "range outside the track": ((4800,) + down[1:], b"range outside the track"),
        "range outside its source": (down[:1] + (402,) + down[2:], b"range outside its source"),
        "twice the samples outside its source": (down[:2] + (401,) + down[3:], b"range outside its source"),
        "segments outside the table": (down[:11] + (1, 1) + down[13:], b"segments outside the table"),
        "a segment beyond the event's stereo samples": (down[:2] + (49,) + down[3:11] + (0, 1) + down[13:], b"beyond the event's source samples"),
        "a reversed region beyond its source": (back[:3] + (401,) + back[4:], b"reversed region outside its source"),
        "more samples than the reversed region holds": (back[:2] + (301,) + back[3:], b"more samples than src_frames hold"),
        # and what the modes add
        "an unknown flag bit": (down[:16] + (D | 8,), b"unknown flags"),
        "a high flag bit": (down[:16] + (0x80000000 | D,), b"unknown flags"),
        "both modes": (down[:16] + (D | B,), b"downmix and balance"),
        "a downmix of a mono source": (down[:10] + (1,) + down[11:], b"stereo source"),
        "a balance into a mono track": (down[:16] + (B,), b"a balance needs a stereo track"),
        "nan left": (down[:5] + (nan,) + down[6:], b"left / right"),
        "infinite right": (down[:6] + (float("inf"),) + down[7:], b"left / right"),
        "a downmix beyond 32-bit source coordinates": ((2 ** 31 - 32768 - 299,) + down[1:], b"2^31 - 32768"),
        "a downmix with 2^31 samples": (down[:2] + (2 ** 31,) + down[3:], b"2^31 - 32768"),
    }), (2, bal, {
        "a downmix into a stereo track": (bal[:16] + (D,), b"a downmix needs a mono track"),
        "a balance of a mono source": (bal[:10] + (1,) + bal[11:], b"stereo source"),
        "a balance on an odd sample": ((101,) + bal[1:], b"whole stereo frame"),
        "nan right": (bal[:6] + (nan,) + bal[7:], b"left / right"),
        "an unknown flag bit": (bal[:16] + (B | 16,), b"unknown flags"),
        "range outside its source": (bal[:1] + (402,) + bal[2:], b"range outside its source"),
    })):
        for what, (row, message) in bad.items():
            assert mix_events(N, "chan", [s], event_table(N, "chan", [ok, row]), segs, 2, nch, t, 5000) == N.SH_ERR_INVALID, what
            err = N.lib().sh_last_error()
            assert err.startswith(b"sh_mix_events_chan") and b"event 1" in err and message in err, (what, err)
            assert t.download_bytes(len(base)) == base, what
    # sh_mix_events_rev keeps refusing the new bits
    for nch, row in ((1, down), (2, bal), (2, bal[:16] + (B | R,))):
        assert mix_events(N, "rev", [s], event_table(N, "rev", [row]), None, 2, nch, t, 5000) == N.SH_ERR_INVALID
        assert b"event 0" in N.lib().sh_last_error() and b"unknown flags" in N.lib().sh_last_error()
        assert t.download_bytes(len(base)) == base
    # width 3 with segments; width 3 without them may be downmixed
    s3, t3 = N.DeviceBuffer.from_bytes(bytes(3000)), N.DeviceBuffer.from_bytes(bytes(15000))
    shaped = down[:11] + (0, 1) + down[13:]
    assert mix_events(N, "chan", [s3], event_table(N, "chan", [down, shaped]), segs, 3, 1, t3, 5000) == N.SH_ERR_INVALID
    assert b"event 1" in N.lib().sh_last_error()
    assert t3.download_bytes(15000) == bytes(15000)
    assert mix_events(N, "chan", [s3], event_table(N, "chan", [down]), None, 3, 1, t3, 5000) == N.SH_OK, N.lib().sh_last_error()
    for width in (0, 5, -2):
        assert mix_events(N, "chan", [s], event_table(N, "chan", [down]), None, width, 1, t, 5000) == N.SH_ERR_INVALID
    assert mix_events(N, "chan", [s], event_table(N, "chan", [down]), None, 2, 0, t, 5000) == N.SH_ERR_INVALID
    assert mix_events(N, "chan", [s, t], event_table(N, "chan", [down]), None, 2, 1, t, 5000) == N.SH_ERR_INVALID       # a source that is the track
    assert mix_events(N, "chan", [s], event_table(N, "chan", [down]), None, 2, 1, t, 5001) == N.SH_ERR_INVALID
    assert mix_events(N, "chan", [s], event_table(N, "chan", []), None, 2, 1, t, 5000) == N.SH_OK
    assert t.download_bytes(len(base)) == base                                                           # nothing was launched
    # and what it accepts: the downmix, the downmix backwards, a plain mono row beside them; then the balance in a stereo track
    assert mix_events(N, "chan", [s], event_table(N, "chan", [down, back, plain]), None, 2, 1, t, 5000) == N.SH_OK, N.lib().sh_last_error()
    want = bytearray(base)
    x = audioop.mul(audioop.tomono(src[400:1600], 2, 0.75, -0.25), 2, 0.5)
    want[200:800] = audioop.add(base[200:800], x, 2)
    x = audioop.mul(audioop.tomono(audioop.reverse(src[400:1600], 2), 2, 0.75, -0.25), 2, 0.5)
    want[200:800] = audioop.add(bytes(want[200:800]), x, 2)
    want[0:40] = audioop.add(bytes(want[0:40]), src[20:60], 2)
    assert t.download_bytes(len(base)) == bytes(want)
    t = N.DeviceBuffer.from_bytes(base)
    assert mix_events(N, "chan", [s], event_table(N, "chan", [bal, bal[:16] + (B | R,)]), None, 2, 2, t, 5000) == N.SH_OK, N.lib().sh_last_error()
    want = bytearray(base)
    want[200:1400] = audioop.add(base[200:1400], audioop.mul(balance(src[400:1600], 2, 0.75, -0.25), 2, 0.5), 2)
    x = audioop.mul(balance(audioop.reverse(src[400:1600], 2), 2, 0.75, -0.25), 2, 0.5)
    want[200:1400] = audioop.add(bytes(want[200:1400]), x, 2)
    assert t.download_bytes(len(base)) == bytes(want)


# ---- 5: the track as a window at an odd sample residue ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2])
def test_the_track_as_an_unaligned_window(gpu, nch):
    """section 1's 16-bit rows into a DeviceBuffer.view three samples off a 16-byte boundary inside a sentinel-filled parent
    (tests/helpers.py: pcm_track_call asserts the residue, the guards around the window and the untouched sources)"""
    N = gpu
    width = 2
    sources, base, rows, want = plain_cases(width, nch)
    ns = len(base) // width
    table = _plain_table(N, rows, nch)
    rc, got = pcm_track_call(N, sources, base, 3 * width, lambda bufs, win, par: mix_events(N, "chan", bufs, table, None, width, nch, win, ns),
                             surplus=16 * width)
    assert rc == N.SH_OK, N.lib().sh_last_error()
    assert got == want, "%d bytes differ" % differs(got, want)
