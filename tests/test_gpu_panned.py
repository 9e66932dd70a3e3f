"""GPU parity of a pan per event in Sample.mix_at_many / mixer.sequence / sh_mix_events_pan -- mono instruments placed in the stereo field
of a stereo track, in one launch -- against live ``audioop``: ``ratecv`` of the mono frames, then ``tostereo``, then ``mul``, then the cut,
then ``add`` with saturation at every event, in list order, on byte slices; the arithmetic of the loop of ``copy().speed().stereo()``,
``at_volume`` and ``mix_at`` it replaces (tests/seqref.py: source, mix, and the three wrong orders of the pan level).  Expected bytes never
come from the product."""
import audioop
from math import gcd

import numpy as np
import pytest

from tests.seqcases import SONG_RATE as RATE, VOLUMES, event_table, in_a_child_under_the_other_alignment_scheme, mix_events, sample_of
from tests.seqref import WRONG, differs, mix, pcm

pytestmark = pytest.mark.gpu

# float pans (Sample.pan's), pairs with a 0 (stereo_mix's "into one channel only"), negative factors, factors above 1
PANS = [0.0, -1.0, 0.3, (1.0, 0.0), (-0.5, 0.8), (1.5, 1.2), 1.0, (0.0, 0.7), -0.65, (0.4, -1.0), (2.0, 0.25), (1.0, 1.0)]


def panned_song(nevents=3000, span=20.0):
    """the plain file's song (tests/seqcases.py: hits_song) with mono instruments (0 .. 3) and two stereo ones (4, 5) into a stereo track: a speed 2^(k/12) per
    event, a quarter of them None; a pan per event of a mono instrument, cycling through PANS"""
    rng = np.random.default_rng(0)
    instruments = []
    for seconds, nch in ((0.05, 1), (0.12, 1), (0.25, 1), (0.4, 1), (0.08, 2), (0.3, 2)):
        n = int(RATE * seconds)
        decay = np.exp(-3.0 * np.arange(n) / n)[:, None]
        instruments.append((rng.uniform(-1.0, 1.0, (n, nch)) * decay * 0.5 * 32767).astype("<i2").tobytes())
    starts = rng.integers(0, int(RATE * span), nevents) / RATE
    starts[:50] = starts[0]
    which = rng.integers(0, 6, nevents)
    volumes = rng.choice(VOLUMES, nevents)
    k = rng.integers(-12, 13, nevents)
    plain = rng.integers(0, 4, nevents) == 0
    events = []
    for n in range(nevents):
        i = int(which[n])
        events.append((float(starts[n]), i, float(volumes[n]), None, None if plain[n] else float(2.0 ** (int(k[n]) / 12)),
                       PANS[n % len(PANS)] if i < 4 else None))
    return instruments, events


# ---- 1: a stereo song ------------------------------------------------------------------------------------------------------------------
def test_a_stereo_song_of_mono_instruments(gpu):
    from synthesizer_amd import mixer
    instruments, events = panned_song()
    named = [(s, instruments[i], v, o, sp, p) for s, i, v, o, sp, p in events]
    want = mix(b"", named, 2, RATE, 2)
    # the oracle must be able to tell the order ratecv -> tostereo -> mul from the three wrong ones
    wrong = {order: differs(want, mix(b"", named, 2, RATE, 2, order)) for order in WRONG["pan"]}
    off_vector = sum(1 for e in events if (2 * int(RATE * e[0])) % 8)
    panned = sum(1 for e in events if e[5] is not None)
    resampled = sum(1 for e in events if e[5] is not None and e[4] is not None and int(RATE * e[4]) != RATE)
    print("panned song: %d bytes, %d of %d events panned (%d of them resampled), bytes that differ from the wrong orders: %s, "
          "%d starts off a multiple of eight samples" % (len(want), panned, len(events), resampled, wrong, off_vector))
    assert all(n > 0 for n in wrong.values()), wrong
    assert off_vector > 0 and 0 < resampled < panned < len(events)
    assert {type(e[5]) for e in events} == {float, tuple, type(None)}
    samples = [sample_of(b, 2, RATE, 1 if i < 4 else 2) for i, b in enumerate(instruments)]
    got = mixer.sequence([(s, samples[i], v, o, sp, p) for s, i, v, o, sp, p in events], RATE, 2, 2, name="panned")
    assert got.name == "panned" and (got.samplerate, got.nchannels, got.samplewidth) == (RATE, 2, 2)
    assert len(got) * 4 == len(want)
    assert bytes(got.view_frame_data()) == want


# ---- 2: the definition -----------------------------------------------------------------------------------------------------------------
def test_the_same_bytes_as_the_loop_of_speed_stereo_at_volume_and_mix_at(gpu):
    from synthesizer_amd.sample import Sample
    instruments, events = panned_song(300, 3.0)
    samples = [sample_of(b, 2, RATE, 1 if i < 4 else 2) for i, b in enumerate(instruments)]
    evs = []
    for k, (s, i, v, _o, sp, p) in enumerate(events):
        evs.append((s, samples[i], None if k % 5 == 0 else v, 0.03 if k % 7 == 0 else None, 1.0 if k % 13 == 0 else sp, p))
    for k in (10, next(k for k in range(11, 300) if evs[k][5] is not None)):
        evs[k] = (0.0,) + evs[k][1:]
    panned = [e for e in evs if e[5] is not None]
    assert any(e[2] is None for e in panned) and any(e[3] for e in panned) and any(e[0] == 0.0 for e in panned)
    assert any(e[4] is None for e in panned) and any(e[4] == 1.0 for e in panned) and any(e[4] not in (None, 1.0) and e[3] for e in panned)
    assert 0 < len(panned) < len(evs)
    base = pcm(np.random.default_rng(1), 2, 2 * RATE, 0.3)
    loop = sample_of(base, 2, RATE, 2)
    for seconds, other, volume, other_seconds, speed, pan in evs:
        o = other
        if speed is not None:
            o = o.copy().speed(speed)
        if pan is not None:
            o = o.copy().stereo(*pan) if isinstance(pan, tuple) else o.copy().pan(pan)
        if volume is not None:
            o = o.at_volume(volume)
        loop.mix_at(seconds, o, other_seconds)
    many = sample_of(base, 2, RATE, 2).mix_at_many(evs)
    assert isinstance(many, Sample) and len(many) == len(loop) > RATE and many.nchannels == 2
    assert bytes(many.view_frame_data()) == bytes(loop.view_frame_data())
    want = mix(base, [(s, instruments[samples.index(o)], v, os_, sp, p) for s, o, v, os_, sp, p in evs], 2, RATE, 2)
    assert bytes(many.view_frame_data()) == want
    for i, (b, smp) in enumerate(zip(instruments, samples)):
        assert bytes(smp.view_frame_data()) == b and smp.nchannels == (1 if i < 4 else 2)       # the instruments are untouched


# ---- 3: widths, every offset -----------------------------------------------------------------------------------------------------------
SPEEDS = [None, 0.1, 0.37, 0.999, 1.001, 2.5, 10]
VOLS = [None, 1.0, 0.5, -1.0, 1.9, 0.0, -0.37]
PAIRS = [0.25, (1.0, 0.0), (-0.5, 0.8), (1.5, 1.2), (0.0, -1.0)]


def _every_offset(width, rate, seed):
    rng = np.random.default_rng(seed)
    tile = 2048 if width == 2 else 1024                     # track samples; half as many stereo frames
    lengths = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 64, 100, tile // 2 - 1, tile // 2, tile // 2 + 1, tile - 1, tile, tile + 1, 3 * tile + 5]
    sources = [pcm(rng, width, n, 0.4) for n in lengths] + [pcm(rng, width, 2 * n, 0.4) for n in (5, 300, tile + 3)]    # the last three: stereo
    track_frames = 6 * tile
    base = pcm(rng, width, 2 * track_frames, 0.4)
    events = []
    for k in range(735):
        i = k % len(lengths) if k % 6 else len(lengths) + (k // 6) % 3
        frame = int(rng.integers(0, 5 * tile // 16)) * 8 + (k // 3) % 8       # sample offsets 0, 2 .. 14 against the track's 16-sample grid
        if k % 9 == 0:
            frame = (int(rng.integers(1, 10)) * tile) // 2 - int(rng.integers(0, 3))      # across a tile edge
        if k % 50 == 49:
            frame = 6 * tile + tile // 2 + k                 # beyond the end: the track grows
        nframes = len(sources[i]) // (width * (2 if i >= len(lengths) else 1))
        other_seconds = (nframes // 2) / rate if k % 11 == 0 and nframes > 1 else None
        events.append((frame / rate, i, VOLS[k % 7], other_seconds, SPEEDS[(k // 7) % 7], PAIRS[k % 5] if i < len(lengths) else None))
    panned = [e for e in events if e[5] is not None]
    assert {(2 * int(rate * e[0])) % 16 for e in panned} == set(range(0, 16, 2))
    assert {(e[4], e[2]) for e in panned} == {(sp, v) for sp in SPEEDS for v in VOLS}
    assert {(e[4], e[5]) for e in panned} == {(sp, p) for sp in SPEEDS for p in PAIRS}
    assert {(e[2], e[5]) for e in panned} == {(v, p) for v in VOLS for p in PAIRS}
    assert {e[1] for e in panned} == set(range(len(lengths))) and len(panned) < len(events)
    return sources, len(lengths), base, events


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_widths_speeds_volumes_factors_and_every_offset(gpu, width):
    rate = 8192                                        # (a power of two: seconds = frame / rate is exact)
    sources, nmono, base, events = _every_offset(width, rate, 300 + width)
    want = mix(base, [(s, sources[i], v, o, sp, p) for s, i, v, o, sp, p in events], width, rate, 2)
    samples = [sample_of(b, width, rate, 1 if i < nmono else 2) for i, b in enumerate(sources)]
    got = sample_of(base, width, rate, 2).mix_at_many([(s, samples[i], v, o, sp, p) for s, i, v, o, sp, p in events])
    assert len(got) * width * 2 == len(want) > len(base)
    assert bytes(got.view_frame_data()) == want


# ---- 4: the float64 route at 16 bits ---------------------------------------------------------------------------------------------------
def test_a_reduced_outrate_of_65536_or_more_at_16_bits(gpu):
    """96 kHz against int(96000 * speed) coprime to it: the float64 route of the 16-bit kernel on panned events, beside the integer one"""
    rate = 96000
    rng = np.random.default_rng(78)
    sources = [pcm(rng, 2, n, 1.0) for n in (1, 9, 700, 5000)]
    base = pcm(rng, 2, 2 * 30000, 0.5)
    speeds = [2 ** (7 / 12), 0.5, 0.999999, None, 1.00002, 2 ** (-7 / 12)]
    assert sum(1 for sp in speeds if sp and rate // gcd(int(rate * sp), rate) >= 65536) >= 3
    assert any(sp and int(rate * sp) != rate and rate // gcd(int(rate * sp), rate) < 65536 for sp in speeds)
    events = [(int(rng.integers(0, 28000)) / rate, k % 4, [None, 0.7, -1.3][k % 3], None, speeds[k % 6], PANS[k % len(PANS)]) for k in range(96)]
    want = mix(base, [(s, sources[i], v, o, sp, p) for s, i, v, o, sp, p in events], 2, rate, 2)
    samples = [sample_of(b, 2, rate, 1) for b in sources]
    got = sample_of(base, 2, rate, 2).mix_at_many([(s, samples[i], v, o, sp, p) for s, i, v, o, sp, p in events])
    assert bytes(got.view_frame_data()) == want


# ---- 5: the C entry point --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_the_entry_point_with_sub_ranges_of_sources(gpu, width):
    """src_sample != 0, sources that are views into one buffer off the 16-byte grid, mono and stereo, plain and resampled rows in one
    table, events that stop before the (resampled) source ends"""
    N = gpu
    rng = np.random.default_rng(240 + width)
    nsrc_samples, ntrack, outrate = 9000, 30000, 44100
    src = pcm(rng, width, nsrc_samples, 0.5)
    base = pcm(rng, width, ntrack, 0.5)
    whole = N.DeviceBuffer.from_bytes(src)
    view = whole.view(6 * width, (nsrc_samples - 6) * width)          # a source whose device memory starts off the 16-byte grid
    inrates = [outrate, 22050, 44099, 48000, 4410, 441000, 62366]
    pairs = [(0.35, 0.65), (1.0, 0.0), (-0.5, 1.5), (0.0, 2.0)]
    rows, want = [], bytearray(base)
    for k in range(320):
        which = k % 2
        nch = 2 if k % 5 == 4 else 1
        inrate = inrates[k % 7]
        left, right = pairs[k % 4] if nch == 1 else (float("nan"), float("inf"))      # (a stereo row ignores them)
        first = (int(rng.integers(0, 200)) * 16 + k % 16) // nch * nch
        start = first + (6 if which else 0)
        if inrate == outrate:
            n = [1, 4, 5, 8, 23, 700, 2048, 4100][(k // 7) % 8] * (2 if nch == 1 else 1)       # track samples
            src_frames = 0                                               # (ignored)
            frames = src[start * width:(start + n // (2 // nch)) * width]
        else:
            src_frames = [1, 2, 9, 300, 1200][(k // 7) % 5]
            frames = audioop.ratecv(src[start * width:(start + src_frames * nch) * width], width, nch, inrate, outrate, None)[0]
            nf = len(frames) // (width * nch)
            if k % 3 == 0:
                nf = (nf + 1) // 2                                       # stops early
            nf = min(nf, 9000)
            n = 2 * nf
            frames = frames[:nf * nch * width]
        if nch == 1:
            frames = audioop.tostereo(frames, width, left, right)
        assert len(frames) == n * width
        d = min(int(rng.integers(0, (ntrack - n) // 16)) * 16 + (k // 16) * (2 if nch == 1 else 1), ntrack - n) // (2 // nch) * (2 // nch)
        factor = [1.0, 0.75, -1.0, 1.0][k % 4]
        rows.append((d, first, n, src_frames, factor, left, right, which, inrate, outrate, nch))
        if factor != 1.0:
            frames = audioop.mul(frames, width, factor)
        want[d * width:(d + n) * width] = audioop.add(bytes(want[d * width:(d + n) * width]), frames, width)
    for nch in (1, 2):
        assert any(r[8] == r[9] and r[10] == nch and r[1] and r[7] for r in rows) and any(r[8] != r[9] and r[10] == nch and r[1] and r[7] for r in rows)
    track = N.DeviceBuffer.from_bytes(base)
    assert mix_events(N, "pan", [whole, view], event_table(N, "pan", rows), None, width, None, track, ntrack) == N.SH_OK, N.lib().sh_last_error()
    assert track.download_bytes(len(base)) == bytes(want)


def test_the_entry_point_refuses_on_the_host(gpu):
    N = gpu
    rng = np.random.default_rng(26)
    src, base = pcm(rng, 2, 1000), pcm(rng, 2, 5000)
    s, t = N.DeviceBuffer.from_bytes(src), N.DeviceBuffer.from_bytes(base)
    nan, inf = float("nan"), float("inf")
    ok = (100, 0, 1000, 500, 0.5, 0.3, 0.7, 0, 22050, 44100, 1)        # 500 mono frames at half speed: 999 frames, 500 of them taken
    ok2 = (100, 0, 1000, 500, 0.5, nan, nan, 0, 22050, 44100, 2)       # 500 stereo frames; left and right are ignored
    plain = (100, 0, 1000, 0, 0.5, 0.3, 0.7, 0, 44100, 44100, 1)
    bad = {
        # what sh_mix_events_rate refuses, on mono and on stereo events
        "source index": [ok, (0, 0, 10, 5, 1.0, 1.0, 1.0, 1, 22050, 44100, 1)],
        "plain range outside its source": [ok, (0, 996, 10, 0, 1.0, 1.0, 1.0, 0, 44100, 44100, 1)],            # 5 frames, 4 left
        "plain stereo range outside its source": [ok, (0, 995, 10, 0, 1.0, 1.0, 1.0, 0, 44100, 44100, 2)],
        "source start outside": [(0, 1002, 0, 0, 1.0, 1.0, 1.0, 0, 22050, 44100, 1)],
        "range outside the track": [ok, (4992, 0, 10, 5, 1.0, 1.0, 1.0, 0, 22050, 44100, 1)],
        "start outside the track": [(5002, 0, 0, 0, 1.0, 1.0, 1.0, 0, 22050, 44100, 1)],
        "nan factor": [ok, (0, 0, 10, 5, nan, 1.0, 1.0, 0, 22050, 44100, 1)],
        "infinite factor": [(0, 0, 10, 5, -inf, 1.0, 1.0, 0, 22050, 44100, 2)],
        "reserved": [ok, (0, 0, 10, 5, 1.0, 1.0, 1.0, 0, 22050, 44100, 1, 7)],
        "inrate 0": [ok, (0, 0, 10, 5, 1.0, 1.0, 1.0, 0, 0, 44100, 1)],
        "outrate 0": [plain, (0, 0, 10, 5, 1.0, 1.0, 1.0, 0, 44100, 0, 1)],
        "both rates 0": [(0, 0, 10, 5, 1.0, 1.0, 1.0, 0, 0, 0, 2)],
        "inrate 2^31": [(0, 0, 10, 5, 1.0, 1.0, 1.0, 0, 2 ** 31, 44100, 1)],
        "outrate 2^31": [(0, 0, 10, 5, 1.0, 1.0, 1.0, 0, 44100, 2 ** 31, 1)],
        "stereo src_sample off a frame": [ok2, (0, 1, 10, 5, 1.0, 1.0, 1.0, 0, 22050, 44100, 2)],
        "stereo nsamples off a frame": [ok2, (0, 0, 9, 5, 1.0, 1.0, 1.0, 0, 22050, 44100, 2)],
        "nsamples beyond what src_frames yields": [ok, (0, 0, 20, 5, 1.0, 1.0, 1.0, 0, 22050, 44100, 1)],     # 5 frames -> 9 frames = 18 samples
        "stereo nsamples beyond what src_frames yields": [ok, (0, 0, 20, 5, 1.0, 1.0, 1.0, 0, 22050, 44100, 2)],
        "nsamples of no frames": [(0, 0, 2, 0, 1.0, 1.0, 1.0, 0, 22050, 44100, 1)],
        "src_frames beyond the source": [ok, (0, 0, 10, 1001, 1.0, 1.0, 1.0, 0, 22050, 44100, 1)],
        "src_frames beyond the source from src_sample on": [(0, 1, 10, 1000, 1.0, 1.0, 1.0, 0, 22050, 44100, 1)],
        "stereo src_frames beyond the source": [ok2, (0, 0, 10, 501, 1.0, 1.0, 1.0, 0, 22050, 44100, 2)],
        # and what a pan adds
        "src_channels 0": [ok, (0, 0, 10, 5, 1.0, 1.0, 1.0, 0, 22050, 44100, 0)],
        "src_channels 3": [(0, 0, 12, 6, 1.0, 1.0, 1.0, 0, 22050, 44100, 3)],
        "nan left": [ok, (0, 0, 10, 5, 1.0, nan, 1.0, 0, 22050, 44100, 1)],
        "infinite right": [(0, 0, 10, 5, 1.0, 1.0, inf, 0, 44100, 44100, 1)],
        "minus infinite left": [(0, 0, 10, 5, 1.0, -inf, 0.0, 0, 22050, 44100, 1)],
        "odd dst_sample": [ok, (1, 0, 10, 5, 1.0, 1.0, 1.0, 0, 22050, 44100, 1)],
        "odd dst_sample, plain": [(7, 0, 10, 0, 1.0, 1.0, 1.0, 0, 44100, 44100, 1)],
        "odd nsamples": [ok, (0, 0, 9, 5, 1.0, 1.0, 1.0, 0, 22050, 44100, 1)],
        "odd nsamples, plain": [ok2, (0, 0, 11, 0, 1.0, 1.0, 1.0, 0, 44100, 44100, 1)],
    }
    for what, rows in bad.items():
        assert mix_events(N, "pan", [s], event_table(N, "pan", rows), None, 2, None, t, 5000) == N.SH_ERR_INVALID, what
        assert N.lib().sh_last_error().startswith(b"sh_mix_events_pan"), what
    for width in (0, 5, -2):
        assert mix_events(N, "pan", [s], event_table(N, "pan", [ok]), None, width, None, t, 5000) == N.SH_ERR_INVALID
    assert mix_events(N, "pan", [s, t], event_table(N, "pan", [ok]), None, 2, None, t, 5000) == N.SH_ERR_INVALID             # a source that is the track
    assert mix_events(N, "pan", [t.view(200, 400)], event_table(N, "pan", [(0, 0, 10, 5, 1.0, 1.0, 1.0, 0, 22050, 44100, 1)]), None, 2, None, t, 5000) == N.SH_ERR_INVALID
    assert mix_events(N, "pan", [s], event_table(N, "pan", [ok]), None, 2, None, t, 5001) == N.SH_ERR_INVALID                # the track range outside its buffer
    assert mix_events(N, "pan", [s], event_table(N, "pan", [ok]), None, 2, None, None, 0) == N.SH_ERR_INVALID
    assert t.download_bytes(len(base)) == base                                                       # nothing was launched
    assert mix_events(N, "pan", [s], event_table(N, "pan", []), None, 2, None, t, 5000) == N.SH_OK
    empty_ends = [(5000, 1000, 0, 0, 1.0, 1.0, 1.0, 0, 22050, 44100, 1), (5000, 1000, 0, 0, 1.0, 1.0, 1.0, 0, 44100, 44100, 2), (0, 0, 0, 0, 1.0, 0.5, 0.5, 0, 44100, 44100, 1)]
    assert mix_events(N, "pan", [s], event_table(N, "pan", empty_ends), None, 2, None, t, 5000) == N.SH_OK                   # empty ranges at the very ends
    assert t.download_bytes(len(base)) == base
    # exactly what 5 mono frames yield (9 frames = 18 track samples), a stereo row with NaN for the factors it ignores, a plain mono row
    rows = [ok, (18, 0, 18, 5, 1.0, -1.0, 2.0, 0, 22050, 44100, 1), ok2, (4000, 500, 1000, 0, 1.0, 1.0, 0.0, 0, 44100, 44100, 1)]
    assert mix_events(N, "pan", [s], event_table(N, "pan", rows), None, 2, None, t, 5000) == N.SH_OK, N.lib().sh_last_error()
    want = bytearray(base)
    want[200:2200] = audioop.add(base[200:2200], audioop.mul(audioop.tostereo(audioop.ratecv(src, 2, 1, 22050, 44100, None)[0][:1000], 2, 0.3, 0.7), 2, 0.5), 2)
    want[36:72] = audioop.add(bytes(want[36:72]), audioop.tostereo(audioop.ratecv(src[:10], 2, 1, 22050, 44100, None)[0], 2, -1.0, 2.0), 2)
    want[200:2200] = audioop.add(bytes(want[200:2200]), audioop.mul(audioop.ratecv(src, 2, 2, 22050, 44100, None)[0][:2000], 2, 0.5), 2)
    want[8000:10000] = audioop.add(bytes(want[8000:10000]), audioop.tostereo(src[1000:2000], 2, 1.0, 0.0), 2)
    assert t.download_bytes(len(base)) == bytes(want)


# ---- 6: in place, steady state, locks --------------------------------------------------------------------------------------------------
def test_in_place_and_the_refusals_of_mix_at_many(gpu):
    rate = 8192
    rng = np.random.default_rng(6)
    a, b, c = pcm(rng, 2, 2 * 8192, 0.6), pcm(rng, 2, 3000, 0.6), pcm(rng, 2, 500, 0.6)
    B, Cc = (sample_of(x, 2, rate, 1) for x in (b, c))
    # growth: a slowed-down sample runs beyond the end, another starts beyond it
    evs = [(0.9, B, None, None, 0.5, 0.5), (0.5, Cc, 0.5, None, 2.0, (0.0, 1.0)), (3.0, Cc, None, None, None, -1.0)]
    t = sample_of(a, 2, rate, 2).mix_at_many(evs)
    want = mix(a, [(0.9, b, None, None, 0.5, 0.5), (0.5, c, 0.5, None, 2.0, (0.0, 1.0)), (3.0, c, None, None, None, -1.0)], 2, rate, 2)
    assert len(want) > 4 * 3 * 8192 and len(t) * 4 == len(want) and bytes(t.view_frame_data()) == want
    # no growth: in place, the same device buffer object before and after; the sources untouched
    t = sample_of(a, 2, rate, 2).to_device()
    dev = t._device()
    evs = [(0.25, B, None, None, 1.5, 0.1), (0.0, Cc, -1.0, None, None, (1.0, 0.0)), (0.9, Cc, None, 0.01, 0.5, (1.2, -0.3))]
    t.mix_at_many(evs)
    assert t._device() is dev
    assert bytes(t.view_frame_data()) == mix(a, [(0.25, b, None, None, 1.5, 0.1), (0.0, c, -1.0, None, None, (1.0, 0.0)),
                                                   (0.9, c, None, 0.01, 0.5, (1.2, -0.3))], 2, rate, 2)
    assert bytes(B.view_frame_data()) == b and bytes(Cc.view_frame_data()) == c and B.nchannels == Cc.nchannels == 1
    # the refusals: ValueError, and nothing mixed before the error
    S = sample_of(a[:400], 2, rate, 2)
    t = sample_of(a, 2, rate, 2)
    for bad in ((0.2, S, None, None, None, 0.5), (0.2, t, None, None, None, 0.5), (0.2, B, None, None, None, 1.5), (0.2, B, None, None, None, -1.01),
                (0.2, B, None, None, None, float("nan")), (0.2, B, None, None, None, (1.0, float("inf"))), (0.2, B, None, None, None, (float("nan"), 0.0)),
                (0.2, B, None, None, None, (1.0,)), (0.2, B, None, None, None, (1.0, 0.5, 0.5)), (0.2, B, None, None, None, ())):
        with pytest.raises(ValueError, match="mix_at_many"):
            t.mix_at_many([(0.1, B, None, None, 0.5, 0.0), bad])
    with pytest.raises(ValueError, match="mix_at_many"):
        sample_of(b, 2, rate, 1).mix_at_many([(0.1, Cc, None, None, None, 0.0)])      # a track that is not stereo
    with pytest.raises(AssertionError):
        t.mix_at_many([(0.1, B, None, None, 0.5, 0.0), (0.2, B)])                   # a mono sample without a pan: mix_at's assertion, as before
    assert bytes(t.view_frame_data()) == a and len(t) == 8192
    with pytest.raises(RuntimeError):
        sample_of(a, 2, rate, 2).lock().mix_at_many([(0.1, B, None, None, 0.5, 0.0)])
    got = sample_of(a, 2, rate, 2).mix_at_many([(0.1, B.lock(), 0.5, None, 0.5, -0.25)])     # a locked SOURCE is only read
    assert bytes(got.view_frame_data()) == mix(a, [(0.1, b, 0.5, None, 0.5, -0.25)], 2, rate, 2)
    assert bytes(B.view_frame_data()) == b
    # `other is self` cuts the list as before; the panned events on both sides of it are batches of their own
    t = sample_of(a, 2, rate, 2)
    t.mix_at_many([(0.1, B, 0.9, None, 1.25, 0.3), (0.05, t, 0.5, 0.2, 0.8), (0.3, Cc, None, None, None, (0.0, 1.0))])
    mid = mix(a, [(0.1, b, 0.9, None, 1.25, 0.3)], 2, rate, 2)
    mid = mix(mid, [(0.05, mid, 0.5, 0.2, 0.8, None)], 2, rate, 2)
    assert bytes(t.view_frame_data()) == mix(mid, [(0.3, c, None, None, None, (0.0, 1.0))], 2, rate, 2)


def test_a_second_call_with_the_same_shapes_allocates_nothing(gpu):
    N = gpu
    instruments, events = panned_song(400, 2.0)
    samples = [sample_of(b, 2, RATE, 1 if i < 4 else 2).to_device() for i, b in enumerate(instruments)]
    evs = [(s, samples[i], v, o, sp, p) for s, i, v, o, sp, p in events]
    track = sample_of(bytes(4 * RATE * 3), 2, RATE, 2).to_device()
    dev = track._device()
    track.mix_at_many(evs)
    N.sync()
    before = N.debug_counters()
    track.mix_at_many(evs)
    after = N.debug_counters()
    assert after["device_allocs"] == before["device_allocs"] and after["device_frees"] == before["device_frees"]
    assert after["stream_syncs"] == before["stream_syncs"] and after["pool_hits"] == before["pool_hits"]
    assert track._device() is dev
    want = mix(bytes(4 * RATE * 3), [(s, instruments[i], v, o, sp, p) for s, i, v, o, sp, p in events] * 2, 2, RATE, 2)
    assert bytes(track.view_frame_data()) == want


# ---- 7: the other way of reading misaligned event samples ------------------------------------------------------------------------------
def test_both_alignment_schemes_give_the_same_bytes():
    """SYNTHHIP_SEQ_ALIGN is read once per process (sh_init): the song, the 16-bit route tests, every offset and the sub-ranges of sources
    again under the scheme that is not the default."""
    in_a_child_under_the_other_alignment_scheme(__file__, ["test_a_stereo_song_of_mono_instruments", "test_a_reduced_outrate_of_65536_or_more_at_16_bits"] +
                                                ["%s[%d]" % (t, w) for t in ("test_widths_speeds_volumes_factors_and_every_offset", "test_the_entry_point_with_sub_ranges_of_sources")
                                                  for w in (1, 2, 3, 4)])
