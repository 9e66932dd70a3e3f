"""GPU parity of a playback speed per event in Sample.mix_at_many / mixer.sequence / sh_mix_events_rate -- a sampler: one recorded note
at many pitches, in one launch -- against live ``audioop``: ``ratecv``, then ``mul``, then the cut, then ``add`` with saturation at every
event, in list order, on byte slices; the arithmetic of the loop of ``copy().speed()``, ``at_volume`` and ``mix_at`` it replaces.
The reference is tests/seqref.py (source, mix).  Expected bytes never come from the product."""
import audioop
import subprocess
from math import gcd

import numpy as np
import pytest

from tests.seqcases import ROOT, SONG_NCH as NCH, SONG_RATE as RATE, event_table, hits_song as song, mix_events, sample_of
from tests.seqref import MUL_BEFORE_RATECV, SELF, mix, pcm

pytestmark = pytest.mark.gpu


def sampler_song(nevents=3000, span=20.0):
    """the plain file's song (tests/seqcases.py: hits_song) with a speed per event: 2^(k/12), k in [-12, 12], a quarter of them None"""
    instruments, events = song(nevents, span)
    rng = np.random.default_rng(7)
    k = rng.integers(-12, 13, nevents)
    plain = rng.integers(0, 4, nevents) == 0
    return instruments, [(s, i, v, None, None if plain[n] else float(2.0 ** (int(k[n]) / 12))) for n, (s, i, v) in enumerate(events)]


# ---- 1: the sampler song ---------------------------------------------------------------------------------------------------------------
def test_the_sampler_song(gpu):
    from synthesizer_amd import mixer
    instruments, events = sampler_song()
    named = [(s, instruments[i], v, o, sp) for s, i, v, o, sp in events]
    want = mix(b"", named, 2, RATE, NCH)
    # the oracle must be able to tell the feature from its absence and from the wrong order
    without = mix(b"", [(s, b, v, o, None) for s, b, v, o, _sp in named], 2, RATE, NCH)
    wrong_order = mix(b"", named, 2, RATE, NCH, MUL_BEFORE_RATECV)
    w = np.frombuffer(want, dtype="<i2")
    n = min(len(want), len(without)) // 2
    differs_without = int(np.count_nonzero(w[:n] != np.frombuffer(without, dtype="<i2")[:n])) + abs(len(want) - len(without))
    differs_wrong_order = int(np.count_nonzero(w != np.frombuffer(wrong_order, dtype="<i2")))
    off_vector = sum(1 for s, _i, _v, _o, _sp in events if (NCH * int(RATE * s)) % 8)
    resampled = sum(1 for e in events if e[4] is not None and int(RATE * e[4]) != RATE)
    print("sampler song: %d samples, %d of %d events resampled, %d samples differ from the list without speeds, %d from ratecv(mul(x)), "
          "%d starts off a multiple of eight samples" % (len(w), resampled, len(events), differs_without, differs_wrong_order, off_vector))
    assert len(wrong_order) == len(want)
    assert differs_without > 0 and differs_wrong_order > 0 and off_vector > 0 and 0 < resampled < len(events)
    samples = [sample_of(b, 2, RATE, NCH) for b in instruments]
    got = mixer.sequence([(s, samples[i], v, o, sp) for s, i, v, o, sp in events], RATE, NCH, 2, name="sampler")
    assert got.name == "sampler" and (got.samplerate, got.nchannels, got.samplewidth) == (RATE, NCH, 2)
    assert len(got) * 2 * NCH == len(want)
    assert bytes(got.view_frame_data()) == want


# ---- 2: the definition -----------------------------------------------------------------------------------------------------------------
def test_the_same_bytes_as_the_loop_of_speed_at_volume_and_mix_at(gpu):
    from synthesizer_amd.sample import Sample
    instruments, events = sampler_song(300, 3.0)
    samples = [sample_of(b, 2, RATE, NCH) for b in instruments]
    evs = []
    for k, (s, i, v, _o, sp) in enumerate(events):
        evs.append((s, samples[i], None if k % 5 == 0 else v, 0.03 if k % 7 == 0 else None, 1.0 if k % 13 == 0 else sp))
    evs[10] = (0.0,) + evs[10][1:]
    assert any(e[4] is None for e in evs) and any(e[4] == 1.0 for e in evs) and any(e[4] not in (None, 1.0) and e[3] for e in evs)
    base = pcm(np.random.default_rng(1), 2, NCH * RATE, 0.3)
    loop = sample_of(base, 2, RATE, NCH)
    for seconds, other, volume, other_seconds, speed in evs:
        o = other
        if speed is not None:
            o = o.copy().speed(speed)
        if volume is not None:
            o = o.at_volume(volume)
        loop.mix_at(seconds, o, other_seconds)
    many = sample_of(base, 2, RATE, NCH).mix_at_many(evs)
    assert isinstance(many, Sample) and len(many) == len(loop) > RATE
    assert bytes(many.view_frame_data()) == bytes(loop.view_frame_data())
    want = mix(base, [(s, instruments[samples.index(o)], v, os_, sp) for s, o, v, os_, sp in evs], 2, RATE, NCH)
    assert bytes(many.view_frame_data()) == want
    for b, smp in zip(instruments, samples):
        assert bytes(smp.view_frame_data()) == b                 # the instruments are untouched


# ---- 3: widths, channels, every offset ---------------------------------------------------------------------------------------------------
SPEEDS = [None, 0.1, 0.37, 0.999, 1.001, 2.5, 10]


def _every_offset(width, nch, rate, seed):
    rng = np.random.default_rng(seed)
    tile = 2048 if width == 2 else 1024
    lengths = [1, 2, 7, 8, 9, 15, 16, 17, 31, 64, 100, tile - 1, tile, tile + 1, 3 * tile + 5, 5 * tile]
    sources = [pcm(rng, width, nch * ((n + nch - 1) // nch), 0.4) for n in lengths]
    track_frames = 12 * tile
    base = pcm(rng, width, nch * track_frames, 0.4)
    events = []
    for k in range(320):
        i = k % len(sources)
        # sample offsets 0 .. 15 against the track's 16-sample grid, for every source, near tile edges and anywhere
        off = (k // len(sources)) % 16 if nch == 1 else (k // len(sources)) % 8
        frame = int(rng.integers(0, 10 * tile // 16)) * (16 // nch) + off
        if k % 9 == 0:
            frame = (int(rng.integers(1, 10)) * tile) // nch - int(rng.integers(0, 3))
        if k % 50 == 49:
            frame = 13 * tile + k                      # beyond the end: the track grows
        volume = [None, 1.0, 0.5, -1.0, 1.9, 0.0, -0.37][k % 7]
        speed = SPEEDS[(k // 3) % 7]                   # (k % 7 drives the volume: every speed meets every volume and every source)
        nframes = len(sources[i]) // (width * nch)
        other_seconds = (nframes // 2) / rate if k % 11 == 0 and nframes > 1 else None
        events.append((frame / rate, i, volume, other_seconds, speed))
    assert {(nch * int(rate * s)) % 16 for s, _i, _v, _o, _sp in events} == set(range(0, 16, nch))
    assert {sp for _s, _i, _v, _o, sp in events} == set(SPEEDS)
    return sources, base, events


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_widths_channels_speeds_and_every_offset(gpu, width, nch):
    rate = 8192                                        # (a power of two: seconds = frame / rate is exact)
    sources, base, events = _every_offset(width, nch, rate, 100 * width + nch)
    want = mix(base, [(s, sources[i], v, o, sp) for s, i, v, o, sp in events], width, rate, nch)
    samples = [sample_of(b, width, rate, nch) for b in sources]
    got = sample_of(base, width, rate, nch).mix_at_many([(s, samples[i], v, o, sp) for s, i, v, o, sp in events])
    assert len(got) * width * nch == len(want) > len(base)
    assert bytes(got.view_frame_data()) == want


@pytest.mark.parametrize("nch", [1, 2])
def test_a_reduced_outrate_of_65536_or_more_at_16_bits(gpu, nch):
    """96 kHz against int(96000 * speed) coprime to it: the float64 route of the 16-bit kernel, beside events of the integer route"""
    rate = 96000
    rng = np.random.default_rng(77 + nch)
    sources = [pcm(rng, 2, nch * n, 1.0) for n in (1, 9, 700, 5000)]
    base = pcm(rng, 2, nch * 30000, 0.5)
    speeds = [2 ** (7 / 12), 0.5, 0.999999, None, 1.00002, 2 ** (-7 / 12)]
    assert sum(1 for sp in speeds if sp and rate // gcd(int(rate * sp), rate) >= 65536) >= 3
    assert any(sp and int(rate * sp) != rate and rate // gcd(int(rate * sp), rate) < 65536 for sp in speeds)
    events = [(int(rng.integers(0, 28000)) / rate, k % 4, [None, 0.7, -1.3][k % 3], None, speeds[k % 6]) for k in range(96)]
    want = mix(base, [(s, sources[i], v, o, sp) for s, i, v, o, sp in events], 2, rate, nch)
    samples = [sample_of(b, 2, rate, nch) for b in sources]
    got = sample_of(base, 2, rate, nch).mix_at_many([(s, samples[i], v, o, sp) for s, i, v, o, sp in events])
    assert bytes(got.view_frame_data()) == want


# ---- 4: the C entry point --------------------------------------------------------------------------------------------------------------
FIELDS = ["dst_sample", "src_sample", "nsamples", "src_frames", "factor", "src", "inrate", "outrate", "reserved"]


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_the_entry_point_with_sub_ranges_of_sources(gpu, width, nch):
    """src_sample != 0, sources that are views into one buffer off the 16-byte grid, plain and resampled rows in one list, events that
    stop before the resampled source ends"""
    N = gpu
    rng = np.random.default_rng(140 + 10 * width + nch)
    nsrc_samples, ntrack, outrate = 9000, 30000, 44100
    src = pcm(rng, width, nsrc_samples, 0.5)
    base = pcm(rng, width, ntrack, 0.5)
    whole = N.DeviceBuffer.from_bytes(src)
    view = whole.view(6 * width, (nsrc_samples - 6) * width)          # a source whose device memory starts off the 16-byte grid
    inrates = [outrate, 22050, 44099, 48000, 4410, 441000, 62366]
    rows, want = [], bytearray(base)
    for k in range(256):
        which = k % 2
        inrate = inrates[k % 7]
        first = (int(rng.integers(0, 200)) * 16 + k % 16) // nch * nch
        start = first + (6 if which else 0)
        if inrate == outrate:
            n = [1, 5, 8, 23, 700, 2048, 4100][(k // 7) % 7]
            src_frames = 0                                               # (ignored)
            frames = src[start * width:(start + n) * width]
        else:
            src_frames = [1, 2, 9, 300, 1200][(k // 7) % 5]
            whole_res = audioop.ratecv(src[start * width:(start + src_frames * nch) * width], width, nch, inrate, outrate, None)[0]
            n = len(whole_res) // width
            if k % 3 == 0:
                n = (n // nch + 1) // 2 * nch                            # stops early
            n = min(n, 20000 // nch * nch)
            frames = whole_res[:n * width]
        d = min(int(rng.integers(0, (ntrack - n) // 16)) * 16 + k // 16, ntrack - n)
        factor = [1.0, 0.75, -1.0, 1.0][k % 4]
        rows.append((d, first, n, src_frames, factor, which, inrate, outrate))
        if factor != 1.0:
            frames = audioop.mul(frames, width, factor)
        want[d * width:(d + n) * width] = audioop.add(bytes(want[d * width:(d + n) * width]), frames, width)
    assert any(r[6] == r[7] for r in rows) and any(r[6] != r[7] and r[1] and r[5] for r in rows)
    track = N.DeviceBuffer.from_bytes(base)
    assert mix_events(N, "rate", [whole, view], event_table(N, "rate", rows), None, width, nch, track, ntrack) == N.SH_OK, N.lib().sh_last_error()
    assert track.download_bytes(len(base)) == bytes(want)


def test_the_entry_point_refuses_on_the_host(gpu):
    N = gpu
    rng = np.random.default_rng(16)
    src, base = pcm(rng, 2, 1000), pcm(rng, 2, 5000)
    s, t = N.DeviceBuffer.from_bytes(src), N.DeviceBuffer.from_bytes(base)
    ok = (100, 0, 1000, 500, 0.5, 0, 22050, 44100)        # 500 stereo frames at half speed: 999 frames, 500 of them taken
    plain = (100, 0, 1000, 0, 0.5, 0, 44100, 44100)
    bad = {
        # what sh_mix_events refuses
        "source index": [ok, (0, 0, 10, 5, 1.0, 1, 22050, 44100)],
        "plain range outside its source": [ok, (0, 995, 10, 0, 1.0, 0, 44100, 44100)],
        "source start outside": [(0, 1002, 0, 0, 1.0, 0, 22050, 44100)],
        "range outside the track": [ok, (4994, 0, 10, 5, 1.0, 0, 22050, 44100)],
        "start outside the track": [(5002, 0, 0, 0, 1.0, 0, 22050, 44100)],
        "nan factor": [ok, (0, 0, 10, 5, float("nan"), 0, 22050, 44100)],
        "infinite factor": [(0, 0, 10, 5, float("-inf"), 0, 22050, 44100)],
        "reserved": [ok, (0, 0, 10, 5, 1.0, 0, 22050, 44100, 7)],
        # and what a rate adds
        "inrate 0": [ok, (0, 0, 10, 5, 1.0, 0, 0, 44100)],
        "outrate 0": [plain, (0, 0, 10, 5, 1.0, 0, 44100, 0)],
        "both rates 0": [(0, 0, 10, 5, 1.0, 0, 0, 0)],
        "inrate 2^31": [(0, 0, 10, 5, 1.0, 0, 2 ** 31, 44100)],
        "outrate 2^31": [(0, 0, 10, 5, 1.0, 0, 44100, 2 ** 31)],
        "src_sample off a frame": [ok, (0, 1, 10, 5, 1.0, 0, 22050, 44100)],
        "nsamples off a frame": [ok, (0, 0, 9, 5, 1.0, 0, 22050, 44100)],
        "nsamples beyond what src_frames yields": [ok, (0, 0, 20, 5, 1.0, 0, 22050, 44100)],       # 5 frames -> 9 frames = 18 samples
        "nsamples of no frames": [(0, 0, 2, 0, 1.0, 0, 22050, 44100)],
        "src_frames beyond the source": [ok, (0, 0, 10, 501, 1.0, 0, 22050, 44100)],
        "src_frames beyond the source from src_sample on": [(0, 2, 10, 500, 1.0, 0, 22050, 44100)],
    }
    for what, rows in bad.items():
        assert mix_events(N, "rate", [s], event_table(N, "rate", rows), None, 2, 2, t, 5000) == N.SH_ERR_INVALID, what
        assert N.lib().sh_last_error().startswith(b"sh_mix_events_rate"), what
    for width in (0, 5, -2):
        assert mix_events(N, "rate", [s], event_table(N, "rate", [ok]), None, width, 2, t, 5000) == N.SH_ERR_INVALID
    for nch in (0, -1):
        assert mix_events(N, "rate", [s], event_table(N, "rate", [ok]), None, 2, nch, t, 5000) == N.SH_ERR_INVALID
    assert mix_events(N, "rate", [s, t], event_table(N, "rate", [ok]), None, 2, 2, t, 5000) == N.SH_ERR_INVALID             # a source that is the track
    assert mix_events(N, "rate", [t.view(200, 400)], event_table(N, "rate", [(0, 0, 10, 5, 1.0, 0, 22050, 44100)]), None, 2, 2, t, 5000) == N.SH_ERR_INVALID
    assert mix_events(N, "rate", [s], event_table(N, "rate", [ok]), None, 2, 2, t, 5001) == N.SH_ERR_INVALID                # the track range outside its buffer
    assert mix_events(N, "rate", [s], event_table(N, "rate", [ok]), None, 2, 2, None, 0) == N.SH_ERR_INVALID
    assert t.download_bytes(len(base)) == base                                                           # nothing was launched
    assert mix_events(N, "rate", [s], event_table(N, "rate", []), None, 2, 2, t, 5000) == N.SH_OK
    assert mix_events(N, "rate", [s], event_table(N, "rate", [(5000, 1000, 0, 0, 1.0, 0, 22050, 44100)]), None, 2, 2, t, 5000) == N.SH_OK   # empty ranges at the very ends
    assert t.download_bytes(len(base)) == base
    assert mix_events(N, "rate", [s], event_table(N, "rate", [ok, (18, 0, 18, 5, 1.0, 0, 22050, 44100)]), None, 2, 2, t, 5000) == N.SH_OK   # exactly what 5 frames yield
    want = bytearray(base)
    want[200:2200] = audioop.add(base[200:2200], audioop.mul(audioop.ratecv(src, 2, 2, 22050, 44100, None)[0][:2000], 2, 0.5), 2)
    want[36:72] = audioop.add(bytes(want[36:72]), audioop.ratecv(src[:20], 2, 2, 22050, 44100, None)[0], 2)
    assert t.download_bytes(len(base)) == bytes(want)


def test_the_event_struct_matches_the_header(gpu, tmp_path):
    N = gpu
    src = tmp_path / "ev.c"
    src.write_text('#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%%zu", sizeof(sh_mix_event_rate));\n%s\nreturn 0;}\n'
                   % (ROOT / "include" / "synthhip.h", "\n".join('printf(" %%zu", offsetof(sh_mix_event_rate, %s));' % f for f in FIELDS)))
    exe = tmp_path / "ev"
    subprocess.run(["gcc", "-std=c99", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    D = N.MIX_EVENT_RATE_DTYPE
    assert got == [D.itemsize] + [D.fields[f][1] for f in FIELDS] == [56, 0, 8, 16, 24, 32, 40, 44, 48, 52]
    assert D.names == tuple(FIELDS)


# ---- 5: growth, in place, the corner cases ----------------------------------------------------------------------------------------------
def test_growth_in_place_and_the_corner_cases(gpu):
    from synthesizer_amd import mixer
    rate = 8192
    rng = np.random.default_rng(5)
    a, b, c = pcm(rng, 2, 8192, 0.6), pcm(rng, 2, 3000, 0.6), pcm(rng, 2, 500, 0.6)
    B, Cc = (sample_of(x, 2, rate, 1) for x in (b, c))
    # growth: a slowed-down sample runs beyond the end, another starts beyond it
    evs = [(0.9, B, None, None, 0.5), (0.5, Cc, 0.5, None, 2.0), (3.0, Cc, None, None, 0.75)]
    t = sample_of(a, 2, rate, 1).mix_at_many(evs)
    want = mix(a, [(0.9, b, None, None, 0.5), (0.5, c, 0.5, None, 2.0), (3.0, c, None, None, 0.75)], 2, rate, 1)
    assert len(want) > 2 * 3 * 8192 and len(t) * 2 == len(want) and bytes(t.view_frame_data()) == want
    # no growth: in place, the same device buffer object before and after; the sources untouched
    t = sample_of(a, 2, rate, 1).to_device()
    dev = t._device()
    evs = [(0.25, B, None, None, 1.5), (0.0, Cc, -1.0, None, 0.3), (0.9, Cc, None, 0.01, 0.5)]
    t.mix_at_many(evs)
    assert t._device() is dev
    assert bytes(t.view_frame_data()) == mix(a, [(0.25, b, None, None, 1.5), (0.0, c, -1.0, None, 0.3), (0.9, c, None, 0.01, 0.5)], 2, rate, 1)
    assert bytes(B.view_frame_data()) == b and bytes(Cc.view_frame_data()) == c
    # zero-length and one-frame sources: ratecv of nothing is nothing, of one frame one frame
    empty, one = sample_of(b"", 2, rate, 1), sample_of(b[:2], 2, rate, 1)
    t = sample_of(a, 2, rate, 1)
    t.mix_at_many([(0.5, empty, None, None, 0.5), (0.25, one, None, None, 0.1), (0.26, one, 0.5, None, 10), (0.0, empty, 0.5, None, 3.0)])
    want = mix(a, [(0.25, b[:2], None, None, 0.1), (0.26, b[:2], 0.5, None, 10)], 2, rate, 1)
    assert len(t) == 8192 and bytes(t.view_frame_data()) == want and want != a
    assert audioop.ratecv(b[:2], 2, 1, 819, rate, None)[0] == b[:2]
    t.mix_at_many([(1.5, empty, None, None, 2.0)])       # a zero-length event beyond the end still grows the track, as mix_at does
    assert len(t) == 12288 and bytes(t.view_frame_data()) == want + bytes(2 * 4096)
    assert len(mixer.sequence([(0.0, empty, None, None, 0.5)], rate, 1)) == 0
    # `other is self` with a speed, in the middle of a list: it reads the track as the events before it left it
    t = sample_of(a, 2, rate, 1)
    t.mix_at_many([(0.1, B, 0.9, None, 1.25), (0.05, t, 0.5, 0.2, 0.8), (0.3, Cc), (0.0, t, None, None, 2.0), (0.7, Cc, 1.5, None, 0.6)])
    assert bytes(t.view_frame_data()) == mix(a, [(0.1, b, 0.9, None, 1.25), (0.05, SELF, 0.5, 0.2, 0.8), (0.3, c, None, None, None),
                                                   (0.0, SELF, None, None, 2.0), (0.7, c, 1.5, None, 0.6)], 2, rate, 1)
    # a speed outside Sample.speed's range, or none at all: ValueError, and nothing mixed before the error
    t = sample_of(a, 2, rate, 1)
    for speed in (0, 0.0, -1, 0.05, 11, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError):
            t.mix_at_many([(0.1, B, None, None, 0.5), (0.2, B, None, None, speed)])
    assert bytes(t.view_frame_data()) == a and len(t) == 8192
    with pytest.raises(RuntimeError):
        sample_of(a, 2, rate, 1).lock().mix_at_many([(0.1, B, None, None, 0.5)])
    got = sample_of(a, 2, rate, 1).mix_at_many([(0.1, B.lock(), 0.5, None, 0.5)])      # a locked SOURCE is only read
    assert bytes(got.view_frame_data()) == mix(a, [(0.1, b, 0.5, None, 0.5)], 2, rate, 1)
    # a plain list, and the same list with speed None / 1.0 / one that leaves the rate as it is spelled out: the same bytes
    x = sample_of(a, 2, rate, 1).mix_at_many([(0.2, B), (0.21, Cc, 0.5), (0.3, B, None, 0.1)])
    y = sample_of(a, 2, rate, 1).mix_at_many([(0.2, B, None, None, None), (0.21, Cc, 0.5, None, 1.0), (0.3, B, None, 0.1, 1.00001)])
    assert int(rate * 1.00001) == rate
    assert bytes(x.view_frame_data()) == bytes(y.view_frame_data()) == mix(a, [(0.2, b, None, None, None), (0.21, c, 0.5, None, None),
                                                                                    (0.3, b, None, 0.1, None)], 2, rate, 1)
    # the boundaries of the range are inside it
    z = sample_of(a, 2, rate, 1).mix_at_many([(0.2, Cc, None, None, 0.1), (0.21, Cc, 0.5, None, 10.0)])
    assert bytes(z.view_frame_data()) == mix(a, [(0.2, c, None, None, 0.1), (0.21, c, 0.5, None, 10.0)], 2, rate, 1)


def test_sequence_against_the_reference_sample(gpu):
    from oracle.sample_oracle import RefSample
    from synthesizer_amd import mixer
    rate, nch = 22050, 2
    rng = np.random.default_rng(18)
    hits = [pcm(rng, 2, nch * n, 0.7) for n in (300, 2500, 9000)]
    events = [(float(rng.uniform(0, 1.5)), int(rng.integers(0, 3)), [None, 0.6, 1.3, -0.9][k % 4], [None, None, 0.05][k % 3],
               [None, 2 ** (3 / 12), 0.5, 1.0, 2 ** (-10 / 12), 4.0][k % 6 if k % 5 else 0]) for k in range(120)]
    events[3] = (0.0,) + events[3][1:]
    ref = RefSample(b"", 2, rate, nch)
    refs = [RefSample(h, 2, rate, nch) for h in hits]
    for seconds, i, volume, other_seconds, speed in events:
        o = refs[i]
        if speed is not None:
            o = o.copy().speed(speed)
        if volume is not None:
            o = o.at_volume(volume)
        ref.mix_at(seconds, o, other_seconds)
    samples = [sample_of(h, 2, rate, nch) for h in hits]
    got = mixer.sequence([(s, samples[i], v, o, sp) for s, i, v, o, sp in events], rate, nch)
    assert len(got) == len(ref) and bytes(got.view_frame_data()) == ref.frames


# ---- 6: steady state --------------------------------------------------------------------------------------------------------------------
def test_a_second_call_with_the_same_shapes_allocates_nothing(gpu):
    N = gpu
    instruments, events = sampler_song(400, 2.0)
    samples = [sample_of(b, 2, RATE, NCH).to_device() for b in instruments]
    evs = [(s, samples[i], v, o, sp) for s, i, v, o, sp in events]
    track = sample_of(bytes(2 * NCH * RATE * 3), 2, RATE, NCH).to_device()
    dev = track._device()
    track.mix_at_many(evs)
    N.sync()
    before = N.debug_counters()
    track.mix_at_many(evs)
    after = N.debug_counters()
    assert after["device_allocs"] == before["device_allocs"] and after["device_frees"] == before["device_frees"]
    assert after["stream_syncs"] == before["stream_syncs"] and after["pool_hits"] == before["pool_hits"]
    assert track._device() is dev
    want = mix(bytes(2 * NCH * RATE * 3), [(s, instruments[i], v, o, sp) for s, i, v, o, sp in events] * 2, 2, RATE, NCH)
    assert bytes(track.view_frame_data()) == want
