"""GPU parity of an ADSR envelope per event in Sample.mix_at_many / mixer.sequence / sh_mix_events_env -- shaped notes in one launch --
against live ``audioop`` and upstream's ``array`` fades written out (tests/seqref.py: envelope_bytes, source, mix): ``ratecv``, the cut
to the note's length, the envelope (split, ``mul`` of the sustain and release parts, the ramps ``int(x * f)`` counting samples, join),
``tostereo``, ``mul``, the cut, ``add`` with saturation at every event, in list order, on byte slices; the arithmetic of the loop of
``copy().speed().clip().envelope().stereo()``, ``at_volume`` and ``mix_at`` it replaces.  Expected bytes never come from the product.
Rate 8000, instruments of 0.05 - 0.4 s, tracks of four tiles (a 16-bit tile is 2048 samples, the others 1024)."""
import array
import audioop
import math

import numpy as np
import pytest

from oracle.sample_oracle import RefSample
from tests.seqcases import SHAPED_RATE as RATE, as_samples, event_table, mix_events, named, sample_of, segment_table, shaped_notes as notes, spy
from tests.seqref import LANE, TILE, WRONG, differs, envelope_bytes, mix, out_frames, pcm

pytestmark = pytest.mark.gpu


def boundaries(event, instruments, width, nch):
    """(first track sample, track samples, [track samples where a part of the envelope begins]) of an event, in plain integers"""
    seconds, i, _v, other_seconds, speed, pan, env = event
    data, snch = instruments[i]
    frames = len(data) // (width * snch)
    if speed:
        frames = out_frames(frames, int(RATE * speed), RATE)
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
                data = pcm(rng, width, 1500 * nch)
                assert envelope_bytes(data, width, nch, RATE, *env) == RefSample(data, width, RATE, nch).envelope(*env).frames


# ---- 1: the definition -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filled", [False, True])
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("width", [1, 2, 4])
def test_mix_at_many_with_envelopes_is_the_oracle_loop(gpu, width, nch, filled):
    instruments, events = notes(width, nch)
    assert_the_list_has_the_hard_places(instruments, events, width, nch)
    base = pcm(np.random.default_rng(width + nch), width, 4 * TILE[width], 0.3) if filled else b""
    want = mix(base, named(instruments, events), width, RATE, nch)
    assert 2 * TILE[width] * width < len(want) <= 4 * TILE[width] * width
    samples = as_samples(instruments, width, RATE)
    got = sample_of(base, width, RATE, nch).mix_at_many([(s, samples[i], v, o, sp, p, e) for s, i, v, o, sp, p, e in events])
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
    want = mix(b"", named(instruments, events[:64]), width, RATE, 2)
    samples = as_samples(instruments, width, RATE)
    got = mixer.sequence([(s, samples[i], v, o, sp, p, e) for s, i, v, o, sp, p, e in events[:64]], RATE, 2, width, name="shaped")
    assert got.name == "shaped" and (got.samplerate, got.nchannels, got.samplewidth) == (RATE, 2, width)
    assert bytes(got.view_frame_data()) == want


# ---- 3: the order and the rounding can be told from the wrong ones ---------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 4])
def test_the_oracle_tells_the_right_chain_from_every_wrong_one(gpu, width):
    instruments, events = notes(width, 2)
    want = mix(b"", named(instruments, events), width, RATE, 2)
    wrong = {order: differs(want, mix(b"", named(instruments, events), width, RATE, 2, order)) for order in WRONG["env"]}
    print("width %d: bytes of %d that differ from the wrong readings: %s" % (width, len(want), wrong))
    assert all(n > 0 for n in wrong.values()), wrong
    samples = as_samples(instruments, width, RATE)
    got = sample_of(b"", width, RATE, 2).mix_at_many([(s, samples[i], v, o, sp, p, e) for s, i, v, o, sp, p, e in events])
    assert bytes(got.view_frame_data()) == want


# ---- 4: saturation in list order -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 4])
def test_loud_enveloped_events_saturate_in_list_order(gpu, width):
    instruments, events = notes(width, 2, seed=4, scale=1.0)
    events = [(s, i, (1.9 if k % 2 else -1.9), o, sp, p, e) for k, (s, i, _v, o, sp, p, e) in enumerate(events) if e is not None]
    want = mix(b"", named(instruments, events), width, RATE, 2)
    back = mix(b"", named(instruments, events[::-1]), width, RATE, 2)
    v = np.frombuffer(want, dtype={1: np.int8, 2: "<i2", 4: "<i4"}[width])
    hi = 2 ** (8 * width - 1) - 1
    assert (v == hi).any() and (v == -hi - 1).any()
    assert len(back) == len(want) and differs(want, back) > 0                           # saturating at every event: the order matters
    samples = as_samples(instruments, width, RATE)
    got = sample_of(b"", width, RATE, 2).mix_at_many([(s, samples[i], v_, o, sp, p, e) for s, i, v_, o, sp, p, e in events])
    assert bytes(got.view_frame_data()) == want
    got = sample_of(b"", width, RATE, 2).mix_at_many([(s, samples[i], v_, o, sp, p, e) for s, i, v_, o, sp, p, e in events[::-1]])
    assert bytes(got.view_frame_data()) == back


# ---- 5: the product's own loop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width, nch", [(2, 2), (1, 1), (4, 2)])
def test_the_same_bytes_as_the_loop_of_speed_clip_envelope_stereo_at_volume_and_mix_at(gpu, width, nch):
    instruments, events = notes(width, nch)
    samples = as_samples(instruments, width, RATE)
    base = pcm(np.random.default_rng(9), width, 4 * TILE[width], 0.3)
    loop = sample_of(base, width, RATE, nch)
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
    many = sample_of(base, width, RATE, nch).mix_at_many([(s, samples[i], v, o, sp, p, e) for s, i, v, o, sp, p, e in events])
    assert len(many) == len(loop)
    assert bytes(many.view_frame_data()) == bytes(loop.view_frame_data()) == mix(base, named(instruments, events), width, RATE, nch)


# ---- 6: a mixed list, and the track as a source ----------------------------------------------------------------------------------------
def test_enveloped_and_plain_events_in_one_list_and_the_track_as_a_source(gpu, monkeypatch):
    N = gpu
    width, nch = 2, 2
    instruments, events = notes(width, nch)
    assert any(e[6] is None for e in events) and any(e[6] is not None for e in events)
    samples = as_samples(instruments, width, RATE)
    calls = spy(N, monkeypatch)
    base = pcm(np.random.default_rng(3), width, 4 * TILE[width], 0.3)
    t = sample_of(base, width, RATE, nch)
    first, last = events[:30], events[30:50]
    env = (0.02, 0.03, 0.5, 0.05, 0.2)
    t.mix_at_many([(s, samples[i], v, o, sp, p, e) for s, i, v, o, sp, p, e in first] + [(0.05, t, 0.4, None, 1.5, None, env)] +
                  [(s, samples[i], v, o, sp, p, e) for s, i, v, o, sp, p, e in last])
    assert calls == ["sh_mix_events_env", "sh_mix_events_env"]                           # the list is cut at the track; one launch per side
    mid = mix(base, named(instruments, first), width, RATE, nch)
    mid = mix(mid, [(0.05, mid, 0.4, None, 1.5, None, env)], width, RATE, nch)
    assert bytes(t.view_frame_data()) == mix(mid, named(instruments, last), width, RATE, nch)
    # a list without an envelope goes where it went before
    del calls[:]
    plain = [(s, samples[i], v, o, sp, p) for s, i, v, o, sp, p, e in events if e is None]
    got = sample_of(base, width, RATE, nch).mix_at_many(plain + [(0.1, samples[5], 0.5, None, None, None, None)])
    assert calls == ["sh_mix_events_pan"]
    assert bytes(got.view_frame_data()) == mix(base, named(instruments, [e for e in events if e[6] is None] + [(0.1, 5, 0.5, None, None, None, None)]), width, RATE, nch)


# ---- 7: the entry point's refusals -----------------------------------------------------------------------------------------------------
def test_the_entry_point_refuses_on_the_host_and_leaves_the_track(gpu):
    N = gpu
    rng = np.random.default_rng(26)
    src, base = pcm(rng, 2, 1000), pcm(rng, 2, 5000)
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
        assert mix_events(N, "env", [s], event_table(N, "env", rows), segment_table(N, segs), 2, 2, t, 5000) == N.SH_ERR_INVALID, what
        err = N.lib().sh_last_error()
        assert err.startswith(b"sh_mix_events_env") and b"event %d" % (len(rows) - 1) in err, (what, err)       # the event is named
        assert t.download_bytes(len(base)) == base, what
    for width in (0, 3, 5, -2):
        assert mix_events(N, "env", [s], event_table(N, "env", [ok]), segment_table(N, good), width, 2, t, 5000) == N.SH_ERR_INVALID
    assert mix_events(N, "env", [s], event_table(N, "env", [ok]), segment_table(N, good), 2, 0, t, 5000) == N.SH_ERR_INVALID
    assert mix_events(N, "env", [s], event_table(N, "env", [ok]), segment_table(N, good), 2, 1, t, 5000) == N.SH_OK       # a mono track: a mono event of it, no tostereo
    t = N.DeviceBuffer.from_bytes(base)
    assert mix_events(N, "env", [s, t], event_table(N, "env", [ok]), segment_table(N, good), 2, 2, t, 5000) == N.SH_ERR_INVALID     # a source that is the track
    assert mix_events(N, "env", [s], event_table(N, "env", [ok]), segment_table(N, good), 2, 2, t, 5001) == N.SH_ERR_INVALID
    assert t.download_bytes(len(base)) == base                                                         # nothing was launched
    assert mix_events(N, "env", [s], event_table(N, "env", []), segment_table(N, []), 2, 2, t, 5000) == N.SH_OK
    assert t.download_bytes(len(base)) == base
    # and what it accepts: the mono event through tostereo, then the stereo one, both shaped by the same three segments
    assert mix_events(N, "env", [s], event_table(N, "env", [ok, ok2]), segment_table(N, good), 2, 2, t, 5000) == N.SH_OK, N.lib().sh_last_error()

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
