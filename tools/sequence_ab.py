#!/usr/bin/env python
"""Sample.mix_at_many against the loop of Sample.mix_at calls it replaces, timed in one process on the same inputs (GPU box, repo
root), every row checked against live audioop (mul, add on byte slices, event by event) before it is timed.

Rows: the song of tests/test_gpu_sequence.py stretched to 120 s with 4096 / 32 768 events; Sample.echo-shaped lists (8 events); 64
events that each cover a whole 10-s stereo track at start 0 -- beside mixer.mix_samples of the same 64 tracks, the aligned gather
fold.  Per row: wall ms of the loop and of mix_at_many (median of repeated passes, each bracketed by a device sync), their ratio,
the device time of the one call (events around it: table copy + kernel) and its logical bytes/s = (sum of event bytes + active-tile
bytes read and written) / device time -- which may exceed the HBM peak when the instruments are served by L2.
SYNTHHIP_SEQ_ALIGN=1: the 16-bit kernel's other way of reading misaligned event samples (include/synthhip.h).

--sampler: events with a playback speed (sh_mix_events_rate) instead -- the 120-s song with 4096 / 32 768 events, each at 2^(k/12),
k in [-12, 12], a quarter of them plain; the same song all downward (speed <= 1) and all upward (speed >= 2); a chord (one 1-s
instrument, 64 notes at one start).  The loop is copy().speed().at_volume() + mix_at per event, timed TWICE (its run-to-run spread is the
yardstick for "not slower"); live audioop.ratecv / mul / add is the check.  --sampler --trace: each row's one call five times and nothing
else, for rocprofv3 --kernel-trace --stats.

--pan: a stereo sampler song (sh_mix_events_pan) -- the 120-s song with 4096 / 32 768 events, MONO instruments, each event at 2^(k/12)
(a quarter plain) and at its own place in the stereo field (floats and factor pairs).  Three forms of the same bytes, checked against
live audioop.ratecv / tostereo / mul / add: (a) one mix_at_many with pans; (b) the loop of copy().speed().stereo() / at_volume / mix_at
it replaces; (c) what there was before pans: a stereo copy of the instrument per distinct (instrument, speed, pan), made once, then
one mix_at_many of plain stereo events -- with the time to make the copies and the device bytes they take.  --pan --trace: (a)'s and (c)'s
one call five times each, for rocprofv3 --kernel-trace.

--env: shaped notes (sh_mix_events_env) -- the sampler song with an ADSR envelope on every note (attack, decay and release 10 %, 15 % and
25 % of the note, sustain level 0.7) and a note length (60 % of the resampled instrument) on every other one.  One mix_at_many against the
loop of copy().speed().clip().envelope() / at_volume / mix_at it replaces, both checked against live audioop.ratecv / mul / add and the
fades in float64 (numpy, the expression order of upstream's int(x * f)).  Then the device time of the one call for the same notes with
(1) no envelope at all (sh_mix_events_rate, the route such a list took before), (2) an envelope that does nothing, (3) a sustain level
alone -- every tile inside one segment, the uniform path -- and (4) the full envelope: what the walk over the segments and the ramps cost.
--env --trace: those four calls five times each and nothing else, for rocprofv3 --kernel-trace.

--loop: held notes (sh_mix_events_loop) -- the sampler song with every note looped to a length beyond its recording (the region from
50 % to 90 % of the instrument, held until the note is 1.5, 2 or 2.5 times the instrument long) and an envelope with a note length (80 %
of the resampled held note) on every note.  Three forms of the same bytes, checked against the frames unrolled in numpy and then live
audioop.ratecv / mul / add and the fades in float64: (a) one mix_at_many with loops; (b) the loop of clip / join / speed / clip / envelope
/ at_volume / mix_at it replaces; (c) what there was before loops: an unrolled copy per distinct (instrument, length), made once, then one
mix_at_many of enveloped events.  --loop --trace: (a)'s and (c)'s one call five times each, for rocprofv3 --kernel-trace.

--reverse: the held notes of --loop with every other note played BACKWARDS (sh_mix_events_rev), every other one of those from a region
(10 % to 95 % of the instrument) -- a reversed cymbal at many places and pitches.  Three forms of the same bytes, checked against
audioop.reverse of the byte slice, the frames unrolled in numpy and then live audioop.ratecv / mul / add and the fades in float64: (a) one
mix_at_many with regions and reversals; (b) the loop of copy().clip().reverse() / clip / join / speed / clip / envelope / at_volume /
mix_at it replaces; (c) what there was before: a reversed copy per distinct (instrument, region), made once, then one mix_at_many of looped
events through sh_mix_events_loop -- with both calls' device times: what the reversal in the kernel costs or saves.  Then the same notes with
no region and no reversal, the list as --loop has it (sh_mix_events_loop: kernels this entry point does not touch), for a run of this commit
against a run of its parent.  --reverse --trace: (a)'s and (c)'s one call five times each, for rocprofv3 --kernel-trace; then the plain
song (no speed, no loop: the vector fetch) with every other note reversed against pre-reversed copies played forwards by the same kernel,
five calls each.

--channels: the held, shaped song of --reverse, its instruments stereo, with ``channels`` per note (sh_mix_events_chan).  Two variants:
a MONO track with a downmix (audioop.tomono) on every note, and a stereo track with a balance on every other note.  (a) one mix_at_many
against the loop of copy().clip().reverse() / ... / envelope / mono() or stereo() / at_volume / mix_at it replaces, the same bytes (the
tests hold both against live audioop); (b) the one call against the same notes from copies converted BEFORE the chain -- one mono() or
stereo() copy per distinct (instrument, factors) -- through sh_mix_events_rev: the time between two events on the stream around the call
here (table packing, table copy and kernel), the kernels' own times under --trace.  For a downmix that is not like for like and not the
same bytes (the copy is mono before ratecv and the envelope: half the samples to fetch, resample and shape): the ratio is the price of
doing the downmix in the lane.  Then (c) the --reverse list without any ``channels`` (sh_mix_events_rev, kernels this entry point does
not touch), five medians of 15 calls, for a run of this commit against a run of its parent.  --channels --trace: per variant (a)'s one
call five times, then (b)'s converted copies five times, then (c)'s list five times, and nothing else, for rocprofv3 --kernel-trace.

--plan: the songs of --channels (both variants) and of --env, 4096 / 32 768 notes, compiled once (mixer.compile_sequence) and rendered
from the resident plan.  Per song: the one call it stands beside -- mixer.sequence (a new track) and mix_at_many in place, wall ms and the
time between two events on the stream -- then the compile time, CompiledSequence.render() (a new Sample) and render_into (in place) of the
whole song, wall and between two events on the stream (one launch and nothing else: the kernel), and the song streamed in windows of 4096
frames (85.3 ms at 48 kHz), a device sync per window: ms per window aligned, the same windows three frames on into a buffer one sample off,
and the share of the 85.3 ms a window takes.  The rendered bytes are held against mixer.sequence's first.  On a tree without
compile_sequence only the first part runs -- that is the yardstick: the parent commit's tool has no --plan, so THIS file is run with
the parent's package on the path, SEQUENCE_AB_TREE=<a built checkout of the parent commit> python tools/sequence_ab.py --plan, on the
same box in the same session, twice (the spread of the two runs is the noise).  --plan --trace: per song
mix_at_many in place five times, then the whole-song render_into five times, and nothing else, for rocprofv3 --kernel-trace --stats.

--tracks: the songs of --plan, their notes dealt over 8 tracks (note k to track k % 8), with mixed gains.  Per song, the time between two
events on the stream (five medians of 15) of a render of the whole song and the wall time per window of 4096 frames (a device sync per
window; every 16th window of the song) for: (a) mixer.compile_tracks' handle, one launch with the gains in its arguments; (b) the way there
was before -- one CompiledSequence per track, each rendered, amplified and mixed into a master: 8 renders, up to 8 amplifies, 8 mixes, 8
tracks materialised per window -- held to (a)'s bytes first; (c) a flat compile_sequence of the same notes, the same work without the bus
(other bytes: the flat list is another chain); (d) (a) with one track muted, and one stem.  On a tree without compile_tracks only (c)
runs: SEQUENCE_AB_TREE=<a built checkout of the parent commit> python tools/sequence_ab.py --tracks is the parent's own figure for (c).

--meters: the stereo songs of --tracks (8 tracks, 4096 / 32 768 notes) with the desk's level meters.  Wall time with a device synchronise,
medians, of the whole song and per window of 4096 frames, for: (a) render(gains=), the path without meters; (b) render(gains=,
meters=True), the rows from the same launch; (c) what a caller did before -- render(gains=), then stem, amplify and the Sample's peak and
sum-of-squares statistics for each of the 8 tracks, then the same on the master -- held to (b)'s rows first, as (b)'s bytes are to (a)'s.
--meters-trace NEVENTS: twenty whole-song renders each of (a) and (b) of the first song and nothing else, for rocprofv3 --kernel-trace.

--desk: the stereo chan song of --meters (8 tracks, 4096 / 32 768 notes) with a pan pot per track and a master fader.  Wall time with a
device synchronise, medians, of the whole song and per window of 4096 frames, for: (a) render(gains=, pans=, master=), the one launch;
(b) the caller's way without it -- eight stems, each amplified and balanced (Sample.stereo), mixed in track order, the mix amplified --
held to (a)'s bytes first; (c) render(gains=) alone, the launch (a) adds its two steps to.  On a tree without pans= only (c) runs:
SEQUENCE_AB_TREE=<a built checkout of the parent commit> python tools/sequence_ab.py --desk is the parent's own figure for (c).

--auto: the song of --desk with fader automation: every track has a fade-in over its first 2 to 9 seconds, a long hold at unity and a
fade-out over its last 3 to 10.  Wall time with a device synchronise, medians, of the whole song and per window of 4096 frames, for:
(a) render(gains=, pans=, master=, automation=), the one launch; (b) the caller's way -- per track a stem, amplify, per move the whole
move's stem amplified and faded (Sample.fadein / fadeout), clipped to the window and joined between what lies around it, then stereo, mix
and the master's amplify -- held to (a)'s bytes first, whole song and a window three frames off inside a fade; (c) render(gains=, pans=,
master=) without automation.  On a tree without automation= only (c) runs: SEQUENCE_AB_TREE=<a built checkout of the parent commit>
python tools/sequence_ab.py --auto is the parent's own figure for (c), row (d).  --auto-trace NEVENTS: twenty whole-song renders each of
(c) and (a) and nothing else, for rocprofv3 --kernel-trace.

--groups: the song of --desk with group buses: its 8 tracks in 3 groups (tracks 1-2, 3-4, 6-7, each with a gain, two with a pan) and 2
loose tracks.  Wall time with a device synchronise, medians, of the whole song and per window of 4096 frames, for: (a) render(gains=,
pans=, master=, groups=), the one launch; (b) the caller's way -- every group rendered with every other track muted, amplify and stereo
on it, the stretches of loose tracks in between rendered the same way, everything mixed in order, the master's amplify -- held to (a)'s
bytes first; (c) render(gains=, pans=, master=) without groups.  On a tree without groups= only (c) runs: SEQUENCE_AB_TREE=<a built
checkout of the parent commit> python tools/sequence_ab.py --groups is the parent's own figure for (c), row (d).

--buses: the song of --groups with a ride on each group's bus and a master fade-in / hold / fade-out (automation(lanes, master=,
groups=)).  The same three rows: (a) render(gains=, pans=, master=, groups=, automation=), the one launch; (b) the caller's way -- every
group's stem with the other tracks muted, amplify, Sample.fadein / fadeout over the whole piece, clip, join, stereo, mix, the master's
amplify, then the master's fades in PCM steps the same way -- held to (a)'s bytes first; (c) render(gains=, pans=, master=, groups=)
without bus lanes.  On a tree whose automation() has no master= only (c) runs: SEQUENCE_AB_TREE=<a built checkout of the parent commit>
python tools/sequence_ab.py --buses is the parent's own figure for (c), row (d).

--pans: the song of --buses, bus lanes and all, with a pan sweep on every track and on one group (automation(lanes, master=, groups=, pans=,
group_pans=)).  (a) render(gains=, pans=, master=, groups=, automation=<bus lanes and pan lanes>), the one launch; (b) the caller's way --
every track's stem, clipped at every move, Sample.pan(lfo=ramp) on the clips a piece covers and stereo on the rest, joined, mixed into
its group's bus or the master, the buses' amplify, fades, pan steps the same way, the master's amplify and fades -- held to (a)'s bytes
first; (c) the same render with an Automation that has the bus lanes and no pan lanes.  On a tree whose automation() has no pans= only (c)
runs: SEQUENCE_AB_TREE=<a built checkout of the parent commit> python tools/sequence_ab.py --pans is the parent's own figure for (c), row (d).

--history: the song of --groups (the stereo chan song, 8 tracks, 3 groups, the desk) and its levels over time.  Wall time with a device
synchronise, medians, of the whole song, for: (a) one render(meters="history", ...), the one launch, the table of blocks read back; (b) the
caller's way today -- chunks(block_frames, meters=True, ...) over the whole song, one metered render per block -- whose master rows are
held to (a)'s first; (c) the same render with meters=True.  On a tree without meters="history" only (c) runs: SEQUENCE_AB_TREE=<a built
checkout of the parent commit> python tools/sequence_ab.py --history is the parent's own figure for (c), row (d).
--clips: the song of --history and the overs of its level history.  Wall time with a device synchronise, medians, and the time between two
events on the stream, of the whole song and of a 4096-frame window, for: (a) render_into(meters="history", clips=True, ...); (c) the same
call without clips; and meters=True.  On a tree without clips= only (c) and meters=True run: SEQUENCE_AB_TREE=<a built checkout of the parent
commit> python tools/sequence_ab.py --clips is the parent's own figure for both, row (d).  --clips-trace: (a) and (c) a few times each and
nothing else, for a kernel trace in a run of its own.
--stems: the song of --pans (8 tracks, 3 groups, bus rides and pan rides) and the samples of every bus.  Wall time with a device
synchronise, medians, and the time between two events on the stream, of the whole song and of a 4096-frame window, for: (a) one
stems_into, 12 planes from one launch; (b) the caller's way -- 12 renders with everything else muted, the tracks through a second desk and
a second Automation that holds their lanes alone, the groups through a third one without the master's lane -- into the same planes, held
to (a)'s bytes first; (c) render_into with the same desk.  On a tree without stems_into only (c) runs: SEQUENCE_AB_TREE=<a built checkout
of the parent commit> python tools/sequence_ab.py --stems is the parent's own figure for (c), row (d).  --stems-trace: (a), (b) and (c)
five times each and nothing else, for a kernel trace in a run of its own."""
import audioop
import os
import sys
import time
from pathlib import Path

import numpy as np

# the yardstick of --plan, --tracks, --desk, --auto, --groups, --buses, --pans and --history is another checkout's package (SEQUENCE_AB_TREE); every other mode measures this tree, whatever the environment says
sys.path.insert(0, (("--plan" in sys.argv[1:] or "--tracks" in sys.argv[1:] or "--desk" in sys.argv[1:] or "--auto" in sys.argv[1:] or "--groups" in sys.argv[1:] or "--buses" in sys.argv[1:] or "--pans" in sys.argv[1:] or "--history" in sys.argv[1:] or "--clips" in sys.argv[1:] or "--stems" in sys.argv[1:]) and os.environ.get("SEQUENCE_AB_TREE")) or str(Path(__file__).resolve().parent.parent))
from synthesizer_amd import _native as N  # noqa: E402
from synthesizer_amd import mixer  # noqa: E402
from synthesizer_amd.sample import Sample  # noqa: E402

RATE, NCH, WIDTH = 48000, 2, 2
TILE = 2048


def instruments(rng):
    out = []
    for seconds in (0.05, 0.12, 0.25, 0.4):
        n = int(RATE * seconds)
        decay = np.exp(-3.0 * np.arange(n) / n)[:, None]
        out.append((rng.uniform(-1.0, 1.0, (n, NCH)) * decay * 0.5 * 32767).astype("<i2").tobytes())
    return out


def song(nevents, span):
    rng = np.random.default_rng(0)
    inst = instruments(rng)
    starts = rng.integers(0, int(RATE * span), nevents) / RATE
    starts[:50] = starts[0]
    which = rng.integers(0, 4, nevents)
    volumes = rng.choice([1.0, 1.0, 0.5, 0.8, -1.0, 0.0, 1.7], nevents)
    return b"", inst, [(float(starts[k]), int(which[k]), float(volumes[k])) for k in range(nevents)]


def echo_list():
    rng = np.random.default_rng(1)
    base = rng.integers(-12000, 12000, NCH * RATE * 5, dtype=np.int16).tobytes()
    tail = base[-NCH * WIDTH * RATE:]                       # the last second, 8 times, 0.3 s apart, each 0.7 of the one before
    return base, [tail], [(4.0 + 0.3 * (k + 1), 0, 0.7 ** (k + 1)) for k in range(8)]


def whole_tracks():
    rng = np.random.default_rng(2)
    tracks = [rng.integers(-3000, 3000, NCH * RATE * 10, dtype=np.int16).tobytes() for _ in range(64)]
    return b"", tracks, [(0.0, k, None) for k in range(64)]


def oracle(base, sources, events):
    fb = WIDTH * NCH
    t = bytearray(base)
    for seconds, i, volume in events:
        frames = sources[i] if volume is None else audioop.mul(sources[i], WIDTH, volume)
        start = fb * int(RATE * seconds)
        end = start + len(frames)
        if end > len(t):
            t.extend(bytes(end - len(t)))
        t[start:end] = audioop.add(bytes(t[start:end]), frames, WIDTH)
    return bytes(t)


def logical_bytes(sources, events, total_bytes):
    active = np.zeros(total_bytes // WIDTH // TILE + 1, dtype=bool)
    ev_bytes = 0
    for seconds, i, _v in events:
        s = NCH * int(RATE * seconds)
        n = len(sources[i]) // WIDTH
        if n:
            active[s // TILE:(s + n - 1) // TILE + 1] = True
            ev_bytes += n * WIDTH
    return ev_bytes + 2 * int(active.sum()) * TILE * WIDTH


def sampler_song(nevents, span, lo=-12, hi=12, plain_share=4):
    base, inst, events = song(nevents, span)
    rng = np.random.default_rng(7)
    k = rng.integers(lo, hi + 1, nevents)
    plain = rng.integers(0, plain_share, nevents) == 0 if plain_share else np.zeros(nevents, dtype=bool)
    return base, inst, [(s, i, v, None if plain[n] else float(2.0 ** (int(k[n]) / 12))) for n, (s, i, v) in enumerate(events)]


def chord():
    rng = np.random.default_rng(3)
    n = RATE
    note = (rng.uniform(-1.0, 1.0, (n, NCH)) * np.exp(-3.0 * np.arange(n) / n)[:, None] * 0.2 * 32767).astype("<i2").tobytes()
    return b"", [note], [(0.5, 0, 0.3, float(2.0 ** ((k % 37 - 12) / 12))) for k in range(64)]


def sampler_oracle(base, sources, events):
    fb = WIDTH * NCH
    t = bytearray(base)
    for seconds, i, volume, speed in events:
        frames = sources[i]
        if speed is not None and int(RATE * speed) != RATE:
            frames = audioop.ratecv(frames, WIDTH, NCH, int(RATE * speed), RATE, None)[0]
        if volume is not None:
            frames = audioop.mul(frames, WIDTH, volume)
        start = fb * int(RATE * seconds)
        end = start + len(frames)
        if end > len(t):
            t.extend(bytes(end - len(t)))
        t[start:end] = audioop.add(bytes(t[start:end]), frames, WIDTH)
    return bytes(t)


def sampler_main():
    N.ensure_init(0)
    print("sampler_ab: SYNTHHIP_SEQ_ALIGN=%s  %s" % (os.environ.get("SYNTHHIP_SEQ_ALIGN", "0"), N.device_info()["name"]), flush=True)
    rows = [("sampler song 120 s, 4096 events", sampler_song(4096, 120.0), 2), ("sampler song 120 s, 32768 events", sampler_song(32768, 120.0), 1),
            ("  all downward (speed <= 1), 4096", sampler_song(4096, 120.0, -12, -1, 0), 2),
            ("  all upward (speed >= 2), 4096", sampler_song(4096, 120.0, 12, 24, 0), 2),
            ("chord: 64 notes of one 1-s sample", chord(), 5)]
    for name, (base, sources, events), loop_passes in rows:
        samples = [Sample.from_raw_frames(b, WIDTH, RATE, NCH).to_device() for b in sources]
        start = Sample.from_raw_frames(base, WIDTH, RATE, NCH).to_device()
        evs = [(s, samples[i], v, None, sp) for s, i, v, sp in events]
        want = sampler_oracle(base, sources, events)
        parity = bytes(start.copy().mix_at_many(evs).view_frame_data()) == want
        if "--trace" in sys.argv[1:]:           # under rocprofv3 --kernel-trace --stats: the one call only, five times per row
            track = Sample.from_raw_frames(bytes(len(want)), WIDTH, RATE, NCH).to_device()
            for _ in range(5):
                track.mix_at_many(evs)
            N.sync()
            print("%-34s traced   parity %s" % (name, "ok" if parity else "FAILED"), flush=True)
            continue

        def loop():
            t = start.copy()
            for seconds, other, volume, _o, speed in evs:
                o = other if speed is None else other.copy().speed(speed)
                t.mix_at(seconds, o if volume is None else o.at_volume(volume))

        def many():
            start.copy().mix_at_many(evs)

        loop_ms = [median_wall(loop, 1, loop_passes), median_wall(loop, 0, loop_passes)]
        many_ms = median_wall(many, 3, 9)
        track = Sample.from_raw_frames(bytes(len(want)), WIDTH, RATE, NCH).to_device()
        for _ in range(3):
            track.mix_at_many(evs)
        dev = []
        for _ in range(9):
            N.sync()
            N.timer_start()
            track.mix_at_many(evs)
            dev.append(N.timer_stop())
        dev_ms = sorted(dev)[len(dev) // 2]
        print("%-34s loop %9.3f / %9.3f ms   mix_at_many %8.3f ms   ratio %6.1fx   device (in place) %7.4f ms   %.2f us per event   parity %s"
              % (name, loop_ms[0], loop_ms[1], many_ms, min(loop_ms) / many_ms, dev_ms, 1e3 * dev_ms / len(evs), "ok" if parity else "FAILED"), flush=True)


PANS = [0.0, -1.0, 0.3, (1.0, 0.0), (-0.5, 0.8), (1.5, 1.2), 1.0, (0.0, 0.7), -0.65, (0.4, -1.0), (2.0, 0.25), (1.0, 1.0)]


def pan_factors(pan):
    return (float(pan[0]), float(pan[1])) if isinstance(pan, tuple) else ((1.0 - pan) / 2.0, (1.0 + pan) / 2.0)


def pan_song(nevents, span):
    """sampler_song with the left channel of its instruments as mono instruments and a pan per event"""
    _base, inst, events = sampler_song(nevents, span)
    mono = [np.frombuffer(b, dtype="<i2")[0::2].tobytes() for b in inst]
    return mono, [(s, i, v, sp, PANS[n % len(PANS)]) for n, (s, i, v, sp) in enumerate(events)]


def pan_oracle(sources, events):
    t = bytearray()
    for seconds, i, volume, speed, pan in events:
        frames = sources[i]
        if speed is not None and int(RATE * speed) != RATE:
            frames = audioop.ratecv(frames, WIDTH, 1, int(RATE * speed), RATE, None)[0]
        frames = audioop.tostereo(frames, WIDTH, *pan_factors(pan))
        if volume is not None:
            frames = audioop.mul(frames, WIDTH, volume)
        start = 2 * WIDTH * int(RATE * seconds)
        end = start + len(frames)
        if end > len(t):
            t.extend(bytes(end - len(t)))
        t[start:end] = audioop.add(bytes(t[start:end]), frames, WIDTH)
    return bytes(t)


def pan_main():
    N.ensure_init(0)
    print("sequence_pan_ab: SYNTHHIP_SEQ_ALIGN=%s  %s" % (os.environ.get("SYNTHHIP_SEQ_ALIGN", "0"), N.device_info()["name"]), flush=True)
    for nevents, loop_passes in ((4096, 3), (32768, 1)):
        sources, events = pan_song(nevents, 120.0)
        samples = [Sample.from_raw_frames(b, WIDTH, RATE, 1).to_device() for b in sources]
        evs = [(s, samples[i], v, None, sp, p) for s, i, v, sp, p in events]
        want = pan_oracle(sources, events)

        def empty():
            return Sample(samplerate=RATE, nchannels=2, samplewidth=WIDTH)

        def many():                                         # (a)
            return empty().mix_at_many(evs)

        def loop():                                         # (b)
            t = empty()
            for seconds, other, volume, _o, speed, pan in evs:
                o = other if speed is None else other.copy().speed(speed)
                o = o.copy().stereo(*pan_factors(pan))
                t.mix_at(seconds, o if volume is None else o.at_volume(volume))
            return t

        def materialise():                                  # (c), first half: one stereo copy per distinct (instrument, speed, pan)
            made = {}
            for _s, i, _v, sp, p in events:
                if (i, sp, p) not in made:
                    o = samples[i] if sp is None else samples[i].copy().speed(sp)
                    made[(i, sp, p)] = o.copy().stereo(*pan_factors(p))
            return made

        def materialised():                                 # (c)
            made = materialise()
            return empty().mix_at_many([(s, made[(i, sp, p)], v) for s, i, v, sp, p in events])

        if "--trace" in sys.argv[1:]:           # under rocprofv3 --kernel-trace: (a)'s one call, then (c)'s, five times each and nothing else
            made = materialise()
            stereo_evs = [(s, made[(i, sp, p)], v) for s, i, v, sp, p in events]
            for lst in (evs, stereo_evs):
                track = Sample.from_raw_frames(bytes(len(want)), WIDTH, RATE, 2).to_device()
                for _ in range(5):
                    track.mix_at_many(lst)
                N.sync()
            print("pan song 120 s, %5d events   traced" % nevents, flush=True)
            continue
        parity = [bytes(f().view_frame_data()) == want for f in (many, loop, materialised)]
        made = materialise()
        extra = sum(len(o) * 2 * WIDTH for o in made.values())
        stereo_evs = [(s, made[(i, sp, p)], v) for s, i, v, sp, p in events]
        many_ms = median_wall(many, 3, 9)
        loop_ms = median_wall(loop, 0, loop_passes)
        mat_ms = median_wall(materialised, 1, 5)
        mat_only_ms = median_wall(materialise, 1, 5)
        mat_mix_ms = median_wall(lambda: empty().mix_at_many(stereo_evs), 3, 9)
        dev = {}
        for name, lst in (("a", evs), ("c", stereo_evs)):  # the one call on a track that is long enough: device time (table copy + kernel)
            track = Sample.from_raw_frames(bytes(len(want)), WIDTH, RATE, 2).to_device()
            for _ in range(3):
                track.mix_at_many(lst)
            runs = []
            for _ in range(9):
                N.sync()
                N.timer_start()
                track.mix_at_many(lst)
                runs.append(N.timer_stop())
            dev[name] = sorted(runs)[len(runs) // 2]
        print("pan song 120 s, %5d events   (a) mix_at_many with pans %9.3f ms   (b) loop %10.3f ms   (c) stereo copies + mix_at_many %9.3f ms "
              "(= %d copies %.3f ms, %.1f MB extra on the device, + the one call %.3f ms)   a/c %.2fx   b/a %.1fx   device, in place: (a) %.4f ms  (c) %.4f ms   "
              "parity a, b, c: %s" % (nevents, many_ms, loop_ms, mat_ms, len(made), mat_only_ms, extra / 1e6, mat_mix_ms, mat_ms / many_ms, loop_ms / many_ms,
                                      dev["a"], dev["c"], " ".join("ok" if x else "FAILED" for x in parity)), flush=True)


def env_song(nevents, span):
    """sampler_song with an envelope per event, in proportion to the note; every other note shorter than its instrument"""
    base, inst, events = sampler_song(nevents, span)
    out = []
    for n, (s, i, v, sp) in enumerate(events):
        frames = len(inst[i]) // (WIDTH * NCH)
        if sp is not None and int(RATE * sp) != RATE:
            frames = (frames - 1) * RATE // int(RATE * sp) + 1
        d = frames / RATE * (0.6 if n % 2 else 1.0)
        out.append((s, i, v, sp, (0.1 * d, 0.15 * d, 0.7, 0.25 * d) + ((d,) if n % 2 else ())))
    return base, inst, out


def np_envelope(frames, attack, decay, sustainlevel, release):
    """upstream's Sample.envelope on 16-bit bytes: the splits and audioop.mul as they stand, the ramps of fadein / fadeout in numpy float64
    (k * slope / numsamples, 1.0 - ramp or ramp + 0.0, the product, trunc: the same IEEE operations in the same order)"""
    fb = WIDTH * NCH

    def frame_idx(seconds):
        return fb * int(RATE * seconds)

    def duration(b):
        return len(b) / RATE / WIDTH / NCH

    def split(b, seconds):
        end = frame_idx(seconds)
        return (b[:end], b[end:]) if end != len(b) else (b, b"")

    def ramped(b, slope, fadeout):
        x = np.frombuffer(b, dtype="<i2").astype(np.float64)
        ramp = np.arange(len(x), dtype=np.float64) * slope / (len(b) / WIDTH)
        return np.trunc(x * ((1.0 - ramp) if fadeout else (ramp + 0.0))).astype("<i2").tobytes()

    def fadeout(b, seconds, target):
        i = frame_idx(duration(b) - min(seconds, duration(b)))
        return b[:i] + ramped(b[i:], 1.0 - target, True)

    A, D = split(frames, attack)
    D, S = split(D, decay)
    if sustainlevel < 1:
        S = audioop.mul(S, WIDTH, sustainlevel)
    S, R = split(S, duration(S) - release)
    if attack > 0:
        i = frame_idx(min(attack, duration(A)))
        A = ramped(A[:i], 1.0, False) + A[i:]
    if decay > 0:
        D = fadeout(D, decay, sustainlevel)
    if release > 0:
        R = fadeout(R, release, 0.0)
    return A + D + S + R


def env_oracle(base, sources, events):
    fb = WIDTH * NCH
    t = bytearray(base)
    for seconds, i, volume, speed, env in events:
        frames = sources[i]
        if speed is not None and int(RATE * speed) != RATE:
            frames = audioop.ratecv(frames, WIDTH, NCH, int(RATE * speed), RATE, None)[0]
        if env is not None:
            if len(env) == 5:
                frames = frames[:fb * int(RATE * env[4])]
            frames = np_envelope(frames, *env[:4])
        if volume is not None:
            frames = audioop.mul(frames, WIDTH, volume)
        start = fb * int(RATE * seconds)
        end = start + len(frames)
        if end > len(t):
            t.extend(bytes(end - len(t)))
        t[start:end] = audioop.add(bytes(t[start:end]), frames, WIDTH)
    return bytes(t)


def env_main():
    N.ensure_init(0)
    print("sequence_env_ab: SYNTHHIP_SEQ_ALIGN=%s  %s" % (os.environ.get("SYNTHHIP_SEQ_ALIGN", "0"), N.device_info()["name"]), flush=True)
    for nevents, loop_passes in ((4096, 2), (32768, 1)):
        base, sources, events = env_song(nevents, 120.0)
        samples = [Sample.from_raw_frames(b, WIDTH, RATE, NCH).to_device() for b in sources]
        start = Sample.from_raw_frames(base, WIDTH, RATE, NCH).to_device()
        evs = [(s, samples[i], v, None, sp, None, e) for s, i, v, sp, e in events]
        want = env_oracle(base, sources, events)

        def many():
            return start.copy().mix_at_many(evs)

        def loop():
            t = start.copy()
            for seconds, other, volume, _o, speed, _p, env in evs:
                o = other if speed is None else other.copy().speed(speed)
                o = o.copy()
                if len(env) == 5:
                    o.clip(0.0, env[4])
                o.envelope(*env[:4])
                t.mix_at(seconds, o if volume is None else o.at_volume(volume))
            return t

        # the one call in place, on a track that is long enough: device time (table copy + kernel), the same notes four ways
        forms = [("no envelope (rate route)", [e[:5] for e in evs]),
                 ("envelope that does nothing", [e[:6] + ((0.0, 0.0, 1.0, 0.0) + e[6][4:],) for e in evs]),
                 ("sustain level alone", [e[:6] + ((0.0, 0.0, 0.7, 0.0) + e[6][4:],) for e in evs]),
                 ("full envelope", evs)]
        if "--trace" in sys.argv[1:]:           # under rocprofv3 --kernel-trace: each form's one call five times, in this order, and nothing else
            for _name, lst in forms:
                track = Sample.from_raw_frames(bytes(len(want)), WIDTH, RATE, NCH).to_device()
                for _ in range(5):
                    track.mix_at_many(lst)
                N.sync()
            print("env song 120 s, %5d events   traced: %s" % (nevents, ", ".join(n for n, _l in forms)), flush=True)
            continue
        parity = [bytes(f().view_frame_data()) == want for f in (many, loop)]
        many_ms = median_wall(many, 3, 9)
        loop_ms = [median_wall(loop, 0, loop_passes), median_wall(loop, 0, loop_passes)]
        dev = []
        for _name, lst in forms:
            track = Sample.from_raw_frames(bytes(len(want)), WIDTH, RATE, NCH).to_device()
            for _ in range(3):
                track.mix_at_many(lst)
            runs = []
            for _ in range(15):
                N.sync()
                N.timer_start()
                track.mix_at_many(lst)
                runs.append(N.timer_stop())
            runs.sort()
            dev.append((runs[len(runs) // 2], runs[0], runs[-1]))
        print("env song 120 s, %5d events   mix_at_many with envelopes %9.3f ms   loop %10.3f / %10.3f ms   ratio %6.1fx   parity one call, loop: %s"
              % (nevents, many_ms, loop_ms[0], loop_ms[1], min(loop_ms) / many_ms, " ".join("ok" if x else "FAILED" for x in parity)), flush=True)
        for (name, _lst), (med, lo, hi) in zip(forms, dev):
            print("    device, in place, %-28s median %8.4f ms   (min %8.4f, max %8.4f of 15)   %.3f us per event" % (name + ":", med, lo, hi, 1e3 * med / nevents), flush=True)


HELD = (1.5, 2.0, 2.5)


def loop_song(nevents, span):
    """sampler_song with a loop and an envelope with a note length per event"""
    base, inst, events = sampler_song(nevents, span)
    out = []
    for n, (s, i, v, sp) in enumerate(events):
        dur = len(inst[i]) // (WIDTH * NCH) / RATE
        loop = (0.5 * dur, 0.9 * dur, HELD[n % 3] * dur)
        frames = int(RATE * loop[2])
        if sp is not None and int(RATE * sp) != RATE:
            frames = (frames - 1) * RATE // int(RATE * sp) + 1
        d = 0.8 * frames / RATE
        out.append((s, i, v, sp, (0.1 * d, 0.15 * d, 0.7, 0.25 * d, d), loop))
    return base, inst, out


def unrolled(frames, loop):
    fb = WIDTH * NCH
    a = np.frombuffer(frames, dtype=np.uint8).reshape(-1, fb)
    S, E, V = int(RATE * loop[0]), min(int(RATE * loop[1]), len(a)), int(RATE * loop[2])
    v = np.arange(V)
    return a[np.where(v < E, v, S + (v - E) % (E - S))].tobytes()


def loop_main():
    N.ensure_init(0)
    print("sequence_loop_ab: SYNTHHIP_SEQ_ALIGN=%s  %s" % (os.environ.get("SYNTHHIP_SEQ_ALIGN", "0"), N.device_info()["name"]), flush=True)
    for nevents, loop_passes in ((4096, 2), (32768, 1)):
        base, sources, events = loop_song(nevents, 120.0)
        samples = [Sample.from_raw_frames(b, WIDTH, RATE, NCH).to_device() for b in sources]
        start = Sample.from_raw_frames(base, WIDTH, RATE, NCH).to_device()
        evs = [(s, samples[i], v, None, sp, None, e, lp) for s, i, v, sp, e, lp in events]
        held = {(i, lp): unrolled(sources[i], lp) for _s, i, _v, _sp, _e, lp in events}
        keys = list(held)
        want = env_oracle(base, [held[k] for k in keys], [(s, keys.index((i, lp)), v, sp, e) for s, i, v, sp, e, lp in events])

        def many():                                         # (a)
            return start.copy().mix_at_many(evs)

        def loop():                                         # (b)
            t = start.copy()
            for seconds, other, volume, _o, speed, _p, env, (ls, le, length) in evs:
                o = other.copy().clip(0.0, le)
                body = other.copy().clip(ls, le)
                while o.duration < length:
                    o.join(body)
                o.clip(0.0, length)
                if speed is not None:
                    o = o.copy().speed(speed)
                o = o.copy()
                o.clip(0.0, env[4])
                o.envelope(*env[:4])
                t.mix_at(seconds, o if volume is None else o.at_volume(volume))
            return t

        def materialise():                                  # (c), first half: one unrolled copy per distinct (instrument, length)
            made = {}
            for i, (ls, le, length) in keys:
                o = samples[i].copy().clip(0.0, le)
                body = samples[i].copy().clip(ls, le)
                while o.duration < length:
                    o.join(body)
                made[(i, (ls, le, length))] = o.clip(0.0, length)
            return made

        def materialised():                                 # (c)
            made = materialise()
            return start.copy().mix_at_many([(s, made[(i, lp)], v, None, sp, None, e) for s, i, v, sp, e, lp in events])

        made = materialise()
        copy_evs = [(s, made[(i, lp)], v, None, sp, None, e) for s, i, v, sp, e, lp in events]
        if "--trace" in sys.argv[1:]:           # under rocprofv3 --kernel-trace: (a)'s one call, then (c)'s, five times each and nothing else
            for lst in (evs, copy_evs):
                track = Sample.from_raw_frames(bytes(len(want)), WIDTH, RATE, NCH).to_device()
                for _ in range(5):
                    track.mix_at_many(lst)
                N.sync()
            print("loop song 120 s, %5d events   traced: looped, then pre-unrolled copies" % nevents, flush=True)
            continue
        parity = [bytes(f().view_frame_data()) == want for f in (many, loop, materialised)]
        extra = sum(len(o) * NCH * WIDTH for o in made.values())
        many_ms = median_wall(many, 3, 9)
        loop_ms = median_wall(loop, 0, loop_passes)
        mat_ms = median_wall(materialised, 1, 5)
        mat_only_ms = median_wall(materialise, 1, 5)
        mat_mix_ms = median_wall(lambda: start.copy().mix_at_many(copy_evs), 3, 9)
        dev = {}
        for name, lst in (("a", evs), ("c", copy_evs)):     # the one call on a track that is long enough: device time (table copy + kernel)
            track = Sample.from_raw_frames(bytes(len(want)), WIDTH, RATE, NCH).to_device()
            for _ in range(3):
                track.mix_at_many(lst)
            runs = []
            for _ in range(15):
                N.sync()
                N.timer_start()
                track.mix_at_many(lst)
                runs.append(N.timer_stop())
            dev[name] = sorted(runs)[len(runs) // 2]
        print("loop song 120 s, %5d events   (a) mix_at_many with loops %9.3f ms   (b) loop of calls %10.3f ms   (c) unrolled copies + mix_at_many "
              "%9.3f ms (= %d copies %.3f ms, %.1f MB extra on the device, + the one call %.3f ms)   a/c %.2fx   b/a %.1fx   device, in place: "
              "(a) %.4f ms  (c) %.4f ms   parity a, b, c: %s" % (nevents, many_ms, loop_ms, mat_ms, len(made), mat_only_ms, extra / 1e6, mat_mix_ms,
                                                                  many_ms / mat_ms, loop_ms / many_ms, dev["a"], dev["c"],
                                                                  " ".join("ok" if x else "FAILED" for x in parity)), flush=True)


def rev_song(nevents, span):
    """loop_song with every other note reversed, every other one of those from a region; the loop sits in what is played"""
    base, inst, events = loop_song(nevents, span)
    out = []
    for n, (s, i, v, sp, e, lp) in enumerate(events):
        dur = len(inst[i]) // (WIDTH * NCH) / RATE
        reverse = n % 2 == 1
        region = (0.1 * dur, 0.95 * dur) if n % 4 == 3 else None
        out.append((s, i, v, sp, e, lp, region, reverse))
    return base, inst, out


def played(frames, region, reverse):
    fb = WIDTH * NCH
    if region is not None:
        frames = frames[fb * int(RATE * region[0]):fb * int(RATE * region[1])]
    return audioop.reverse(frames, WIDTH) if reverse else frames


def plain_trace(nevents):
    """The plain reversed fetch in one kernel, for --reverse --trace: the plain song (no speed, no loop) with every other note reversed,
    then the same bytes from pre-reversed copies played forwards -- with one empty reversed event, so that both lists go to
    sh_mix_events_rev and the vector fetch of a reversed event stands against that of a forward one in k_seq_16<REV>.  Both checked
    against live audioop first; five calls each."""
    base, sources, events = song(nevents, 120.0)
    both = sources + [audioop.reverse(b, WIDTH) for b in sources]
    want = oracle(base, both, [(s, i + (len(sources) if k % 2 else 0), v) for k, (s, i, v) in enumerate(events)])
    samples = [Sample.from_raw_frames(b, WIDTH, RATE, NCH).to_device() for b in both]
    none = (None,) * 5
    turned = [(s, samples[i], v) + none + (None, k % 2 == 1) for k, (s, i, v) in enumerate(events)]
    copies = [(s, samples[i + (len(sources) if k % 2 else 0)], v) for k, (s, i, v) in enumerate(events)]
    copies.append((0.0, samples[0], None) + none + ((0.0, 0.0), True))
    parity = []
    for lst in (turned, copies):
        track = Sample.from_raw_frames(bytes(len(want)), WIDTH, RATE, NCH).to_device()
        parity.append(bytes(track.copy().mix_at_many(lst).view_frame_data()) == want)
        for _ in range(5):
            track.mix_at_many(lst)
        N.sync()
    print("plain song 120 s, %5d events   traced: every other note reversed in the kernel, then forwards from pre-reversed copies, both "
          "through sh_mix_events_rev   parity: %s" % (nevents, " ".join("ok" if x else "FAILED" for x in parity)), flush=True)


def rev_main():
    N.ensure_init(0)
    info = N.device_info()
    print("sequence_rev_ab: SYNTHHIP_SEQ_ALIGN=%s  %s" % (os.environ.get("SYNTHHIP_SEQ_ALIGN", "0"), info["name"] or info["arch"]), flush=True)
    for nevents, loop_passes in ((4096, 2), (32768, 1)):
        base, sources, events = rev_song(nevents, 120.0)
        samples = [Sample.from_raw_frames(b, WIDTH, RATE, NCH).to_device() for b in sources]
        start = Sample.from_raw_frames(base, WIDTH, RATE, NCH).to_device()
        evs = [(s, samples[i], v, None, sp, None, e, lp, rg, rv) for s, i, v, sp, e, lp, rg, rv in events]
        plain_evs = [ev[:8] for ev in evs]                  # the list without a region or a reversal: sh_mix_events_loop, as before
        turned = {(i, rg, rv): played(sources[i], rg, rv) for _s, i, _v, _sp, _e, _lp, rg, rv in events}
        held = {(i, rg, rv, lp): unrolled(turned[(i, rg, rv)], lp) for _s, i, _v, _sp, _e, lp, rg, rv in events}
        keys = list(held)
        want = env_oracle(base, [held[k] for k in keys], [(s, keys.index((i, rg, rv, lp)), v, sp, e) for s, i, v, sp, e, lp, rg, rv in events])

        def many():                                         # (a)
            return start.copy().mix_at_many(evs)

        def loop():                                         # (b)
            t = start.copy()
            for seconds, other, volume, _o, speed, _p, env, (ls, le, length), region, reverse in evs:
                o = other
                if region is not None:
                    o = other.copy().clip(region[0], region[1])
                if reverse:
                    o = o.copy().reverse()
                body = o.copy().clip(ls, le)
                o = o.copy().clip(0.0, le)
                while o.duration < length:
                    o.join(body)
                o.clip(0.0, length)
                if speed is not None:
                    o = o.copy().speed(speed)
                o = o.copy()
                o.clip(0.0, env[4])
                o.envelope(*env[:4])
                t.mix_at(seconds, o if volume is None else o.at_volume(volume))
            return t

        def materialise():                                  # (c), first half: one clipped, reversed copy per distinct (instrument, region)
            made = {}
            for i, rg, rv in turned:
                o = samples[i]
                if rg is not None:
                    o = o.copy().clip(rg[0], rg[1])
                made[(i, rg, rv)] = o.copy().reverse() if rv else o
            return made

        def materialised():                                 # (c)
            made = materialise()
            return start.copy().mix_at_many([(s, made[(i, rg, rv)], v, None, sp, None, e, lp) for s, i, v, sp, e, lp, rg, rv in events])

        made = materialise()
        copy_evs = [(s, made[(i, rg, rv)], v, None, sp, None, e, lp) for s, i, v, sp, e, lp, rg, rv in events]
        if "--trace" in sys.argv[1:]:           # under rocprofv3 --kernel-trace: (a)'s one call, then (c)'s, five times each and nothing else
            for lst in (evs, copy_evs):
                track = Sample.from_raw_frames(bytes(len(want)), WIDTH, RATE, NCH).to_device()
                for _ in range(5):
                    track.mix_at_many(lst)
                N.sync()
            print("rev song 120 s, %5d events   traced: reversed in the kernel, then pre-reversed copies" % nevents, flush=True)
            plain_trace(nevents)
            continue
        parity = [bytes(f().view_frame_data()) == want for f in (many, loop, materialised)]
        extra = sum(len(o) * NCH * WIDTH for k, o in made.items() if k[1] is not None or k[2])
        many_ms = median_wall(many, 3, 9)
        loop_ms = median_wall(loop, 0, loop_passes)
        mat_ms = median_wall(materialised, 1, 5)
        mat_only_ms = median_wall(materialise, 1, 5)
        mat_mix_ms = median_wall(lambda: start.copy().mix_at_many(copy_evs), 3, 9)
        plain_ms = median_wall(lambda: start.copy().mix_at_many(plain_evs), 3, 9)
        dev = {}
        for name, lst in (("a", evs), ("c", copy_evs), ("p", plain_evs)):     # the one call on a track that is long enough: device time (table copy + kernel)
            track = Sample.from_raw_frames(bytes(len(want)), WIDTH, RATE, NCH).to_device()
            for _ in range(3):
                track.mix_at_many(lst)
            runs = []
            for _ in range(15):
                N.sync()
                N.timer_start()
                track.mix_at_many(lst)
                runs.append(N.timer_stop())
            dev[name] = sorted(runs)[len(runs) // 2]
        print("rev song 120 s, %5d events   (a) mix_at_many, every other note reversed %9.3f ms   (b) loop of calls %10.3f ms   (c) reversed copies + "
              "mix_at_many %9.3f ms (= %d copies %.3f ms, %.2f MB extra on the device, + the one call %.3f ms)   a/c %.2fx   b/a %.1fx   device, in "
              "place: (a) sh_mix_events_rev %.4f ms  (c) sh_mix_events_loop %.4f ms   parity a, b, c: %s"
              % (nevents, many_ms, loop_ms, mat_ms, len(made), mat_only_ms, extra / 1e6, mat_mix_ms, many_ms / mat_ms, loop_ms / many_ms, dev["a"],
                 dev["c"], " ".join("ok" if x else "FAILED" for x in parity)), flush=True)
        print("rev song 120 s, %5d events   the list without a region or a reversal (sh_mix_events_loop)   mix_at_many %9.3f ms   device, in place "
              "%.4f ms" % (nevents, plain_ms, dev["p"]), flush=True)


CHANNELS = ((0.75, 0.25), (0.5, 0.5), (1.0, 0.0), (0.3, -0.9))


def device_ms(track, lst, warm=3, runs=15):
    """the one call on a track that is long enough: the time between two events on the stream around it (the host's packing of the
    tables, their copy and the kernel), the median of `runs`"""
    for _ in range(warm):
        track.mix_at_many(lst)
    out = []
    for _ in range(runs):
        N.sync()
        N.timer_start()
        track.mix_at_many(lst)
        out.append(N.timer_stop())
    return sorted(out)[len(out) // 2]


def chan_main():
    N.ensure_init(0)
    info = N.device_info()
    print("sequence_chan_ab: SYNTHHIP_SEQ_ALIGN=%s  %s" % (os.environ.get("SYNTHHIP_SEQ_ALIGN", "0"), info["name"] or info["arch"]), flush=True)
    trace = "--trace" in sys.argv[1:]
    for nevents, loop_passes in ((4096, 2), (32768, 1)):
        base, sources, events = rev_song(nevents, 120.0)
        samples = [Sample.from_raw_frames(b, WIDTH, RATE, NCH).to_device() for b in sources]
        rev_evs = [(s, samples[i], v, None, sp, None, e, lp, rg, rv) for s, i, v, sp, e, lp, rg, rv in events]
        frames = len(Sample.from_raw_frames(base, WIDTH, RATE, NCH).to_device().mix_at_many(rev_evs))      # the song's length: every variant's
        for what, nch, every in (("downmix on every note, mono track", 1, 1), ("balance on every other note, stereo track", 2, 2)):
            chans = [CHANNELS[k % 4] if k % every == 0 else None for k in range(nevents)]
            evs = [ev + (ch,) for ev, ch in zip(rev_evs, chans)]
            start = Sample.from_raw_frames(base, WIDTH, RATE, nch).to_device()
            made = {}                                       # (b): converted first, one copy per distinct (instrument, factors)
            for (_s, i, *_r), ch in zip(events, chans):
                if ch is not None and (i, ch) not in made:
                    made[(i, ch)] = samples[i].copy().mono(*ch) if nch == 1 else samples[i].copy().stereo(*ch)
            copy_evs = [ev[:1] + (made[(i, ch)] if ch is not None else ev[1],) + ev[2:] for ev, (_s, i, *_r), ch in zip(rev_evs, events, chans)]
            track = Sample.from_raw_frames(bytes(frames * nch * WIDTH), WIDTH, RATE, nch).to_device()
            if trace:               # under rocprofv3 --kernel-trace: (a)'s one call, then (b)'s converted copies, five times each and nothing else
                for lst in (evs, copy_evs):
                    for _ in range(5):
                        track.mix_at_many(lst)
                    N.sync()
                print("chan song 120 s, %5d events, %s   traced: sh_mix_events_chan, then %d converted copies through sh_mix_events_rev"
                      % (nevents, what, len(made)), flush=True)
                continue

            def many():                                     # (a)
                return start.copy().mix_at_many(evs)

            def loop():                                     # (a)'s yardstick
                t = start.copy()
                for seconds, other, volume, _o, speed, _p, env, (ls, le, length), region, reverse, ch in evs:
                    o = other
                    if region is not None:
                        o = other.copy().clip(region[0], region[1])
                    if reverse:
                        o = o.copy().reverse()
                    body = o.copy().clip(ls, le)
                    o = o.copy().clip(0.0, le)
                    while o.duration < length:
                        o.join(body)
                    o.clip(0.0, length)
                    if speed is not None:
                        o = o.copy().speed(speed)
                    o = o.copy()
                    o.clip(0.0, env[4])
                    o.envelope(*env[:4])
                    if ch is not None:
                        o = o.copy().mono(*ch) if nch == 1 else o.copy().stereo(*ch)
                    t.mix_at(seconds, o if volume is None else o.at_volume(volume))
                return t

            got = many()
            parity = len(got) == frames and bytes(got.view_frame_data()) == bytes(loop().view_frame_data())
            del got
            many_ms = median_wall(many, 3, 9)
            loop_ms = median_wall(loop, 0, loop_passes)
            dev_chan = device_ms(track, evs)
            dev_copies = device_ms(track, copy_evs)
            print("chan song 120 s, %5d events, %s   (a) mix_at_many %9.3f ms   loop of calls %10.3f ms   loop / one call %.1fx   (b) in place, "
                  "between two events on the stream: sh_mix_events_chan %.4f ms   %d converted copies through sh_mix_events_rev %.4f ms   "
                  "chan / copies %.2fx   parity one call, loop: %s"
                  % (nevents, what, many_ms, loop_ms, loop_ms / many_ms, dev_chan, len(made), dev_copies, dev_chan / dev_copies,
                     "ok" if parity else "FAILED"), flush=True)
        track = Sample.from_raw_frames(bytes(frames * NCH * WIDTH), WIDTH, RATE, NCH).to_device()         # (c): no channels anywhere, a stereo track
        if trace:
            for _ in range(5):
                track.mix_at_many(rev_evs)
            N.sync()
            print("chan song 120 s, %5d events   traced: the list without channels (sh_mix_events_rev)" % nevents, flush=True)
            continue
        meds = [device_ms(track, rev_evs) for _ in range(5)]
        print("chan song 120 s, %5d events   (c) the list without channels (sh_mix_events_rev)   in place, between two events on the stream, "
              "five medians of 15: %s ms" % (nevents, " ".join("%.4f" % m for m in meds)), flush=True)


def plan_main():
    N.ensure_init(0)
    has = hasattr(mixer, "compile_sequence")
    trace = "--trace" in sys.argv[1:]
    info = N.device_info()
    print("sequence_plan_ab: SYNTHHIP_SEQ_ALIGN=%s  %s  compile_sequence: %s" % (os.environ.get("SYNTHHIP_SEQ_ALIGN", "0"), info["name"] or info["arch"],
                                                                               "yes" if has else "no (the yardstick)"), flush=True)
    win = 4096
    for nevents in (4096, 32768):
        songs = []
        _base, sources, events = rev_song(nevents, 120.0)
        samples = [Sample.from_raw_frames(b, WIDTH, RATE, NCH).to_device() for b in sources]
        rev_evs = [(s, samples[i], v, None, sp, None, e, lp, rg, rv) for s, i, v, sp, e, lp, rg, rv in events]
        for what, nch, every in (("chan, downmix on every note, mono track", 1, 1), ("chan, balance on every other note, stereo track", 2, 2)):
            songs.append((what, nch, [ev + (CHANNELS[k % 4] if k % every == 0 else None,) for k, ev in enumerate(rev_evs)]))
        _base, inst, shaped = env_song(nevents, 120.0)
        env_samples = [Sample.from_raw_frames(b, WIDTH, RATE, NCH).to_device() for b in inst]
        songs.append(("env, stereo track", NCH, [(s, env_samples[i], v, None, sp, None, e) for s, i, v, sp, e in shaped]))
        for what, nch, evs in songs:
            whole = mixer.sequence(evs, RATE, nch, WIDTH)
            frames, fb = len(whole), nch * WIDTH
            track = Sample.from_raw_frames(bytes(frames * fb), WIDTH, RATE, nch).to_device()
            cs = mixer.compile_sequence(evs, RATE, nch, WIDTH) if has else None
            out = N.DeviceBuffer(frames * fb + 16) if has else None
            if trace:
                for _ in range(5):
                    track.mix_at_many(evs)
                N.sync()
                for _ in range(5 if has else 0):
                    cs.render_into(out, 0, 0, frames)
                N.sync()
                print("plan song 120 s, %5d events, %s   traced: mix_at_many in place x 5%s" % (nevents, what, ", render_into of the whole song x 5" if has else ""), flush=True)
                continue
            seq_ms = median_wall(lambda: mixer.sequence(evs, RATE, nch, WIDTH), 2, 7)
            many_ms = median_wall(lambda: track.mix_at_many(evs), 2, 7)
            many_dev = device_ms(track, evs, warm=1, runs=7)
            print("plan song 120 s, %5d events, %s, %d frames   mixer.sequence %9.3f ms   mix_at_many in place %9.3f ms, between two events on "
                  "the stream %9.4f ms" % (nevents, what, frames, seq_ms, many_ms, many_dev), flush=True)
            if not has:
                continue
            want = bytes(whole.view_frame_data())
            parity = bytes(cs.render().view_frame_data()) == want
            compile_ms = median_wall(lambda: mixer.compile_sequence(evs, RATE, nch, WIDTH).close(), 1, 3)
            render_ms = median_wall(lambda: cs.render(), 3, 15)
            into_ms = median_wall(lambda: cs.render_into(out, 0, 0, frames), 3, 15)
            devs = []
            for _ in range(5):                              # five medians of 15: their spread is the noise
                runs = []
                for _ in range(15):
                    N.sync()
                    N.timer_start()
                    cs.render_into(out, 0, 0, frames)
                    runs.append(N.timer_stop())
                devs.append(sorted(runs)[7])
            nwin = (frames - 3) // win

            def stream(shift, at):
                for k in range(nwin):
                    cs.render_into(out, at, k * win + shift, win)
                    N.sync()

            got = b"".join(bytes(c.view_frame_data()) for c in cs.chunks(win))
            parity = parity and got == want
            aligned_ms = median_wall(lambda: stream(0, 0), 1, 5) / nwin
            off_ms = median_wall(lambda: stream(3, WIDTH), 1, 5) / nwin
            i = cs.info()
            print("plan song 120 s, %5d events, %s   level %s, %d tiles (%d active), %d pairs, %.2f MB resident   compile %9.3f ms   render() %8.4f ms "
                  "(mixer.sequence / render() %.0fx)   render_into %8.4f ms (mix_at_many / render_into %.0fx)   between two events on the stream, five "
                  "medians of 15: %s ms   windows of %d frames, %d of them: aligned %.4f ms each (%.3f %% of the 85.3 ms), three frames on into a buffer "
                  "one sample off %.4f ms (%.2fx)   parity whole, chunks: %s"
                  % (nevents, what, cs.level, i["ntiles"], i["active_tiles"], i["pairs"], i["device_bytes"] / 1e6, compile_ms, render_ms, seq_ms / render_ms,
                     into_ms, many_ms / into_ms, " ".join("%.4f" % d for d in devs), win, nwin, aligned_ms, 100 * aligned_ms / (win / RATE * 1e3), off_ms,
                     off_ms / aligned_ms, "ok" if parity else "FAILED"), flush=True)
            cs.close()


TRACK_GAINS = (1.0, 0.5, 0.8, 1.7, -1.0, 0.25, 1.0, 0.999)


def five_medians(fn, runs=15):
    """the time between two events on the stream around fn, five medians of `runs`: their spread is the noise"""
    out = []
    for _ in range(5):
        one = []
        for _ in range(runs):
            N.sync()
            N.timer_start()
            fn()
            one.append(N.timer_stop())
        out.append(sorted(one)[runs // 2])
    return out


def tracks_main():
    N.ensure_init(0)
    has = hasattr(mixer, "compile_tracks")
    info = N.device_info()
    print("sequence_tracks_ab: SYNTHHIP_SEQ_ALIGN=%s  %s  compile_tracks: %s" % (os.environ.get("SYNTHHIP_SEQ_ALIGN", "0"), info["name"] or info["arch"],
                                                                                 "yes" if has else "no (the yardstick: (c) alone)"), flush=True)
    win, ntracks = 4096, len(TRACK_GAINS)
    fmt = lambda v: " ".join("%.4f" % x for x in v)        # noqa: E731
    for nevents in (4096, 32768):
        songs = []
        _base, sources, events = rev_song(nevents, 120.0)
        samples = [Sample.from_raw_frames(b, WIDTH, RATE, NCH).to_device() for b in sources]
        rev_evs = [(s, samples[i], v, None, sp, None, e, lp, rg, rv) for s, i, v, sp, e, lp, rg, rv in events]
        for what, nch, every in (("chan, downmix on every note, mono track", 1, 1), ("chan, balance on every other note, stereo track", 2, 2)):
            songs.append((what, nch, [ev + (CHANNELS[k % 4] if k % every == 0 else None,) for k, ev in enumerate(rev_evs)]))
        _base, inst, shaped = env_song(nevents, 120.0)
        env_samples = [Sample.from_raw_frames(b, WIDTH, RATE, NCH).to_device() for b in inst]
        songs.append(("env, stereo track", NCH, [(s, env_samples[i], v, None, sp, None, e) for s, i, v, sp, e in shaped]))
        for what, nch, evs in songs:
            fb = nch * WIDTH
            flat = mixer.compile_sequence(evs, RATE, nch, WIDTH)
            frames = flat.frames
            out = N.DeviceBuffer(frames * fb + 16)
            wins = list(range(0, (frames - 3) // win, 16))

            def stream(render):
                for k in wins:
                    render(k * win, win)
                    N.sync()

            c_whole = five_medians(lambda: flat.render_into(out, 0, 0, frames))
            c_win = median_wall(lambda: stream(lambda a, n: flat.render_into(out, 0, a, n)), 1, 5) / len(wins)
            print("tracks song 120 s, %5d events, %s, %d frames   (c) flat compile_sequence: whole song, between two events on the stream, five "
                  "medians of 15: %s ms   a window of %d frames: %.4f ms" % (nevents, what, frames, fmt(c_whole), win, c_win), flush=True)
            if not has:
                flat.close()
                continue
            dealt = [evs[t::ntracks] for t in range(ntracks)]
            t0 = time.perf_counter()
            bus = mixer.compile_tracks(dealt, RATE, nch, WIDTH)
            compile_ms = (time.perf_counter() - t0) * 1e3
            singles = [mixer.compile_sequence(t, RATE, nch, WIDTH) for t in dealt]
            assert bus.frames == frames

            def old_way(a, n):
                master = Sample(samplerate=RATE, nchannels=nch, samplewidth=WIDTH)
                for cs, g in zip(singles, TRACK_GAINS):
                    m = min(n, max(0, cs.frames - a))
                    if m <= 0:
                        continue
                    sub = cs.render(a, m)
                    if g != 1.0:
                        sub.amplify(g)
                    master.mix(sub)
                return master

            got = bytes(bus.render(gains=TRACK_GAINS).view_frame_data())
            want = bytes(old_way(0, frames).view_frame_data())
            parity = got == want + bytes(len(got) - len(want))
            mid = (frames // 2) // win * win
            parity = parity and bytes(bus.render(mid + 3, win, gains=TRACK_GAINS).view_frame_data()) == got[(mid + 3) * fb:(mid + 3 + win) * fb]
            a_whole = five_medians(lambda: bus.render_into(out, 0, 0, frames, gains=TRACK_GAINS))
            a_win = median_wall(lambda: stream(lambda a, n: bus.render_into(out, 0, a, n, gains=TRACK_GAINS)), 1, 5) / len(wins)
            b_whole = five_medians(lambda: old_way(0, frames), runs=5)
            b_wall = median_wall(lambda: old_way(0, frames), 1, 5)
            b_win = median_wall(lambda: stream(old_way), 1, 5) / len(wins)
            muted = tuple(0.0 if t == 3 else g for t, g in enumerate(TRACK_GAINS))
            one_hot = tuple(1.0 if t == 0 else 0.0 for t in range(ntracks))
            d_muted = five_medians(lambda: bus.render_into(out, 0, 0, frames, gains=muted))
            d_stem = five_medians(lambda: bus.render_into(out, 0, 0, frames, gains=one_hot))
            unity = five_medians(lambda: bus.render_into(out, 0, 0, frames))
            i, nruns = bus.info(), bus._seq.tracks()[1]
            med = lambda v: sorted(v)[len(v) // 2]         # noqa: E731
            print("tracks song 120 s, %5d events, %s   %d tracks, level %s, %d tiles, %d pairs, %d runs, %.2f MB resident, compile %.1f ms   "
                  "(a) one launch, mixed gains: whole song %s ms   a window %.4f ms   (b) %d handles rendered, amplified, mixed: whole song, between two "
                  "events on the stream, five medians of 5: %s ms (wall %.3f ms)   a window %.4f ms   (d) track 3 muted: %s ms   a stem: %s ms   every "
                  "gain 1.0: %s ms   (a) / (b) whole %.3f, window %.3f   (a) / (c) whole %.3f, window %.3f   parity (a) against (b), whole and window: %s"
                  % (nevents, what, ntracks, bus.level, i["ntiles"], i["pairs"], nruns, i["device_bytes"] / 1e6, compile_ms, fmt(a_whole), a_win, ntracks,
                     fmt(b_whole), b_wall, b_win, fmt(d_muted), fmt(d_stem), fmt(unity), med(a_whole) / med(b_whole), a_win / b_win,
                     med(a_whole) / med(c_whole), a_win / c_win, "ok" if parity else "FAILED"), flush=True)
            for cs in singles + [bus, flat]:
                cs.close()


def meters_songs(nevents):
    """the stereo songs of --tracks: (what, nch, events)"""
    _base, sources, events = rev_song(nevents, 120.0)
    samples = [Sample.from_raw_frames(b, WIDTH, RATE, NCH).to_device() for b in sources]
    rev_evs = [(s, samples[i], v, None, sp, None, e, lp, rg, rv) for s, i, v, sp, e, lp, rg, rv in events]
    songs = [("chan, balance on every other note, stereo track", 2, [ev + (CHANNELS[k % 4] if k % 2 == 0 else None,) for k, ev in enumerate(rev_evs)])]
    _base, inst, shaped = env_song(nevents, 120.0)
    env_samples = [Sample.from_raw_frames(b, WIDTH, RATE, NCH).to_device() for b in inst]
    songs.append(("env, stereo track", NCH, [(s, env_samples[i], v, None, sp, None, e) for s, i, v, sp, e in shaped]))
    return songs


def meters_main():
    """--meters: the level meters of a song of tracks from the render's own launch.  (a) render(gains=), the code path without meters;
    (b) render(gains=, meters=True); (c) what a caller did without them: render(gains=), then per track stem, amplify and the Sample's
    peak and sum-of-squares calls, then the same on the master -- held to (b)'s rows first.  Wall time with a device synchronise (b and c
    wait for their figures anyway), medians; whole song and 4096-frame windows.  --meters-trace NEVENTS: whole-song renders of (a) and (b)
    alone, for a kernel trace of its own."""
    N.ensure_init(0)
    info = N.device_info()
    trace = "--meters-trace" in sys.argv[1:]
    sizes = (int(sys.argv[sys.argv.index("--meters-trace") + 1]),) if trace else (4096, 32768)
    print("sequence_meters_ab: SYNTHHIP_SEQ_ALIGN=%s  %s%s" % (os.environ.get("SYNTHHIP_SEQ_ALIGN", "0"), info["name"] or info["arch"],
                                                            "  (trace run: 20 whole-song renders each of (a) and (b))" if trace else ""), flush=True)
    win, ntracks = 4096, len(TRACK_GAINS)
    for nevents in sizes:
        for what, nch, evs in meters_songs(nevents)[:1 if trace else None]:
            fb = nch * WIDTH
            bus = mixer.compile_tracks([evs[t::ntracks] for t in range(ntracks)], RATE, nch, WIDTH)
            frames = bus.frames
            out = N.DeviceBuffer(frames * fb + 16)
            if trace:
                for _ in range(20):
                    bus.render_into(out, 0, 0, frames, gains=TRACK_GAINS)
                    bus.render_into(out, 0, 0, frames, gains=TRACK_GAINS, meters=True)
                N.sync()
                print("meters trace, %5d events, %s, %d frames, level %s: done" % (nevents, what, frames, bus.level), flush=True)
                bus.close()
                continue
            wins = list(range(0, (frames - 3) // win, 16))

            def caller(a, n):
                """(c): the rows as ((peaks), (sums)) per track and for the master"""
                rows = []
                master = bus.render(a, n, gains=TRACK_GAINS)
                for t, g in enumerate(TRACK_GAINS):
                    sub = bus.stem(t, a, n)
                    if g != 1.0:
                        sub.amplify(g)
                    rows.append(sub._channel_stats())
                rows.append(master._channel_stats())
                return rows

            def same(lv, rows):
                got = [(r.peak, r.sum_squares) for r in lv.tracks + [lv.master]]
                return all(p == rp and all(abs(float(s[c]) - rs[c]) <= 1e-12 * max(1.0, rs[c]) for c in (0, 1)) for (p, s), (rp, rs) in zip(got, rows))

            mid = (frames // 2) // win * win
            parity = same(bus.render(gains=TRACK_GAINS, meters=True)[1], caller(0, frames)) and same(bus.render(mid, win, gains=TRACK_GAINS, meters=True)[1], caller(mid, win))
            plain, lv = bus.render(mid, win, gains=TRACK_GAINS), bus.render(mid, win, gains=TRACK_GAINS, meters=True)
            parity = parity and bytes(plain.view_frame_data()) == bytes(lv[0].view_frame_data())

            def stream(render):
                for k in wins:
                    render(k * win, win)
                    N.sync()

            a_whole = median_wall(lambda: bus.render_into(out, 0, 0, frames, gains=TRACK_GAINS), 2, 15)
            b_whole = median_wall(lambda: bus.render_into(out, 0, 0, frames, gains=TRACK_GAINS, meters=True), 2, 15)
            c_whole = median_wall(lambda: caller(0, frames), 1, 5)
            a_dev = five_medians(lambda: bus.render_into(out, 0, 0, frames, gains=TRACK_GAINS))
            b_dev = five_medians(lambda: bus.render_into(out, 0, 0, frames, gains=TRACK_GAINS, meters=True))
            a_win = median_wall(lambda: stream(lambda a, n: bus.render_into(out, 0, a, n, gains=TRACK_GAINS)), 1, 5) / len(wins)
            b_win = median_wall(lambda: stream(lambda a, n: bus.render_into(out, 0, a, n, gains=TRACK_GAINS, meters=True)), 1, 5) / len(wins)
            c_win = median_wall(lambda: stream(caller), 1, 3) / len(wins)
            fmt = lambda v: " ".join("%.4f" % x for x in v)    # noqa: E731
            print("meters song 120 s, %5d events, %s, %d tracks, level %s, %d frames   whole song, wall with a synchronise, median: (a) render(gains=) "
                  "%.4f ms   (b) render(gains=, meters=True) %.4f ms   (c) render, 8 stems, amplify, statistics %.3f ms   between two events on the "
                  "stream, five medians of 15: (a) %s ms   (b) %s ms   a window of %d frames, wall: (a) %.4f ms   (b) %.4f ms   (c) %.3f ms   "
                  "(b) / (a) whole %.3f, window %.3f   (b) / (c) whole %.4f, window %.4f   (c) against (b)'s rows, and (b)'s bytes against (a)'s: %s"
                  % (nevents, what, ntracks, bus.level, frames, a_whole, b_whole, c_whole, fmt(a_dev), fmt(b_dev), win, a_win, b_win, c_win,
                     b_whole / a_whole, b_win / a_win, b_whole / c_whole, b_win / c_win, "ok" if parity else "FAILED"), flush=True)
            bus.close()


DESK_PANS = (0.3, None, (1.5, 0.25), -1.0, (0.999, 0.37), 0.0, None, -0.37)
DESK_MASTER = 0.7


def desk_main():
    """--desk: a pan per track and a master fader in the render's own launch.  (a) render(gains=, pans=, master=); (b) what a caller did
    without them: eight stems, amplify, stereo, mix, amplify -- held to (a)'s bytes first; (c) render(gains=) alone.  Wall time with a
    device synchronise, medians; whole song and 4096-frame windows.  A tree whose render has no pans= runs (c) alone."""
    import inspect
    N.ensure_init(0)
    info = N.device_info()
    has = "pans" in inspect.signature(mixer.CompiledSequence.render).parameters
    print("sequence_desk_ab: SYNTHHIP_SEQ_ALIGN=%s  %s  pans= and master=: %s" % (os.environ.get("SYNTHHIP_SEQ_ALIGN", "0"), info["name"] or info["arch"],
                                                                                "yes" if has else "no (the yardstick: (c) alone)"), flush=True)
    win, ntracks = 4096, len(TRACK_GAINS)
    factors = [None if p is None else pan_factors(p) for p in DESK_PANS]
    for nevents in (4096, 32768):
        what, nch, evs = meters_songs(nevents)[0]
        fb = nch * WIDTH
        bus = mixer.compile_tracks([evs[t::ntracks] for t in range(ntracks)], RATE, nch, WIDTH)
        frames = bus.frames
        out = N.DeviceBuffer(frames * fb + 16)
        wins = list(range(0, (frames - 3) // win, 16))

        def stream(render):
            for k in wins:
                render(k * win, win)
                N.sync()

        c_whole = median_wall(lambda: bus.render_into(out, 0, 0, frames, gains=TRACK_GAINS), 2, 15)
        c_dev = five_medians(lambda: bus.render_into(out, 0, 0, frames, gains=TRACK_GAINS))
        c_win = median_wall(lambda: stream(lambda a, n: bus.render_into(out, 0, a, n, gains=TRACK_GAINS)), 1, 5) / len(wins)
        fmt = lambda v: " ".join("%.4f" % x for x in v)    # noqa: E731
        head = "desk song 120 s, %5d events, %s, %d tracks, level %s, %d frames   " % (nevents, what, ntracks, bus.level, frames)
        tail = "(c) render(gains=): whole song, wall with a synchronise, median %.4f ms   between two events on the stream, five medians of 15: %s ms   " \
               "a window of %d frames, wall %.4f ms" % (c_whole, fmt(c_dev), win, c_win)
        if not has:
            print(head + tail, flush=True)
            bus.close()
            continue

        def caller(a, n):
            """(b): the window as a caller made it with stems"""
            master = Sample(samplerate=RATE, nchannels=nch, samplewidth=WIDTH)
            for t, g in enumerate(TRACK_GAINS):
                sub = bus.stem(t, a, n)
                if g != 1.0:
                    sub.amplify(g)
                if factors[t] is not None:
                    sub.stereo(*factors[t])
                master.mix(sub)
            return master.amplify(DESK_MASTER)

        desk = dict(gains=TRACK_GAINS, pans=DESK_PANS, master=DESK_MASTER)
        mid = (frames // 2) // win * win
        parity = bytes(bus.render(**desk).view_frame_data()) == bytes(caller(0, frames).view_frame_data()) and \
            bytes(bus.render(mid + 3, win, **desk).view_frame_data()) == bytes(caller(mid + 3, win).view_frame_data())
        a_whole = median_wall(lambda: bus.render_into(out, 0, 0, frames, **desk), 2, 15)
        a_dev = five_medians(lambda: bus.render_into(out, 0, 0, frames, **desk))
        a_win = median_wall(lambda: stream(lambda a, n: bus.render_into(out, 0, a, n, **desk)), 1, 5) / len(wins)
        b_whole = median_wall(lambda: caller(0, frames), 1, 5)
        b_win = median_wall(lambda: stream(caller), 1, 3) / len(wins)
        print(head + "(a) render(gains=, pans=, master=): whole song, wall with a synchronise, median %.4f ms   between two events on the stream, five "
              "medians of 15: %s ms   a window, wall %.4f ms   (b) 8 stems, amplify, stereo, mix, amplify: whole song, wall %.3f ms   a window, wall "
              "%.3f ms   %s   (a) / (b) whole %.4f, window %.4f   (a) / (c) whole %.3f, window %.3f   (a)'s bytes against (b)'s, whole and window: %s"
              % (a_whole, fmt(a_dev), a_win, b_whole, b_win, tail, a_whole / b_whole, a_win / b_win, a_whole / c_whole, a_win / c_win,
                 "ok" if parity else "FAILED"), flush=True)
        bus.close()


def auto_lanes(frames):
    """a fade-in, a long hold at unity and a fade-out on every track: whole seconds, so that Sample.fadein's seconds are exact frames"""
    return [[(0, (2 + t) * RATE, t / 8.0, 1.0), (frames - (3 + t) * RATE, frames, 1.0, t / 10.0)] for t in range(len(TRACK_GAINS))]


def auto_main():
    """--auto: fader automation in the render's own launch.  (a) render(gains=, pans=, master=, automation=); (b) the caller's way with
    stems, Sample.fadein / fadeout, clip and join -- held to (a)'s bytes first; (c) render(gains=, pans=, master=).  Wall time with a
    device synchronise, medians; whole song and 4096-frame windows.  A tree whose render has no automation= runs (c) alone."""
    import inspect
    N.ensure_init(0)
    info = N.device_info()
    has = "automation" in inspect.signature(mixer.CompiledSequence.render).parameters
    trace = "--auto-trace" in sys.argv[1:]
    sizes = (int(sys.argv[sys.argv.index("--auto-trace") + 1]),) if trace else (4096, 32768)
    print("sequence_auto_ab: SYNTHHIP_SEQ_ALIGN=%s  %s  automation=: %s%s" % (os.environ.get("SYNTHHIP_SEQ_ALIGN", "0"), info["name"] or info["arch"],
          "yes" if has else "no (the yardstick: (c) alone)", "  (trace run: 20 whole-song renders each of (c) and (a))" if trace else ""), flush=True)
    win, ntracks = 4096, len(TRACK_GAINS)
    factors = [None if p is None else pan_factors(p) for p in DESK_PANS]
    desk = dict(gains=TRACK_GAINS, pans=DESK_PANS, master=DESK_MASTER)
    for nevents in sizes:
        what, nch, evs = meters_songs(nevents)[0]
        fb = nch * WIDTH
        bus = mixer.compile_tracks([evs[t::ntracks] for t in range(ntracks)], RATE, nch, WIDTH)
        frames = bus.frames
        out = N.DeviceBuffer(frames * fb + 16)
        wins = list(range(0, (frames - 3) // win, 16))

        def stream(render):
            for k in wins:
                render(k * win, win)
                N.sync()

        if trace:
            auto = bus.automation(auto_lanes(frames))
            for _ in range(20):
                bus.render_into(out, 0, 0, frames, **desk)
                bus.render_into(out, 0, 0, frames, automation=auto, **desk)
            N.sync()
            print("auto trace, %5d events, %s, %d frames, level %s: done" % (nevents, what, frames, bus.level), flush=True)
            auto.close()
            bus.close()
            continue
        c_whole = median_wall(lambda: bus.render_into(out, 0, 0, frames, **desk), 2, 15)
        c_dev = five_medians(lambda: bus.render_into(out, 0, 0, frames, **desk))
        c_win = median_wall(lambda: stream(lambda a, n: bus.render_into(out, 0, a, n, **desk)), 1, 5) / len(wins)
        fmt = lambda v: " ".join("%.4f" % x for x in v)    # noqa: E731
        head = "auto song 120 s, %5d events, %s, %d tracks, level %s, %d frames   " % (nevents, what, ntracks, bus.level, frames)
        tail = "(c) render(gains=, pans=, master=): whole song, wall with a synchronise, median %.4f ms   between two events on the stream, five medians " \
               "of 15: %s ms   a window of %d frames, wall %.4f ms" % (c_whole, fmt(c_dev), win, c_win)
        if not has:
            print(head + tail, flush=True)
            bus.close()
            continue
        lanes = auto_lanes(frames)
        auto = bus.automation(lanes)
        at = lambda f: (f + 0.5) / RATE                     # noqa: E731  (seconds that Sample.frame_idx turns back into frame f)

        def caller(a, n):
            """(b): the window as a caller made it with stems and Sample's fades"""
            master = Sample(samplerate=RATE, nchannels=nch, samplewidth=WIDTH)
            for t, g in enumerate(TRACK_GAINS):
                sub = bus.stem(t, a, n)
                if g != 1.0:
                    sub.amplify(g)
                for pa, pb, v0, v1 in lanes[t]:
                    lo, hi = max(a, pa), min(a + n, pb)
                    if lo >= hi:
                        continue
                    move = bus.stem(t, pa, pb - pa)         # the whole move: k counts from its first sample, numsamples is its length
                    if g != 1.0:
                        move.amplify(g)
                    move.fadein(move.duration, v0) if v1 == 1.0 else move.fadeout(move.duration, v1)
                    move.clip(at(lo - pa), at(hi - pa))
                    behind = sub.copy().clip(at(hi - a), at(n))
                    sub.clip(0.0, at(lo - a)).join(move).join(behind)
                if factors[t] is not None:
                    sub.stereo(*factors[t])
                master.mix(sub)
            return master.amplify(DESK_MASTER)

        inside = lanes[3][0][1] // 2 // win * win + 3       # a window three frames off inside track 3's fade-in (and others')
        assert any(pa < inside and inside + win < pb for lane in lanes for pa, pb, _v0, _v1 in lane)
        parity = bytes(bus.render(automation=auto, **desk).view_frame_data()) == bytes(caller(0, frames).view_frame_data()) and \
            bytes(bus.render(inside, win, automation=auto, **desk).view_frame_data()) == bytes(caller(inside, win).view_frame_data())
        differs = bytes(bus.render(inside, win, automation=auto, **desk).view_frame_data()) != bytes(bus.render(inside, win, **desk).view_frame_data())
        a_whole = median_wall(lambda: bus.render_into(out, 0, 0, frames, automation=auto, **desk), 2, 15)
        a_dev = five_medians(lambda: bus.render_into(out, 0, 0, frames, automation=auto, **desk))
        a_win = median_wall(lambda: stream(lambda a, n: bus.render_into(out, 0, a, n, automation=auto, **desk)), 1, 5) / len(wins)
        b_whole = median_wall(lambda: caller(0, frames), 1, 3)
        b_win = median_wall(lambda: stream(caller), 1, 3) / len(wins)
        print(head + "(a) render(gains=, pans=, master=, automation=): whole song, wall with a synchronise, median %.4f ms   between two events on the "
              "stream, five medians of 15: %s ms   a window, wall %.4f ms   (b) stems, amplify, fadein / fadeout, clip, join, stereo, mix, amplify: whole "
              "song, wall %.3f ms   a window, wall %.3f ms   %s   (a) / (b) whole %.4f, window %.4f   (a) / (c) whole %.3f, window %.3f   (a)'s bytes "
              "against (b)'s, whole and a window inside a fade: %s   (a) differs from (c) there: %s"
              % (a_whole, fmt(a_dev), a_win, b_whole, b_win, tail, a_whole / b_whole, a_win / b_win, a_whole / c_whole, a_win / c_win,
                 "ok" if parity else "FAILED", "yes" if differs else "NO"), flush=True)
        assert parity and differs
        auto.close()
        bus.close()


GROUPS = [(1, 3, 0.8, (0.999, 0.37)), (3, 5, 1.3, -0.37), (6, 8, 0.6, None)]       # 8 tracks: three groups, tracks 0 and 5 loose


def groups_main():
    """--groups: group buses in the render's own launch.  (a) render(gains=, pans=, master=, groups=); (b) the caller's way: every group
    rendered with every other track muted, amplify and stereo on it, the stretches of loose tracks in between rendered the same way, all
    mixed in order, then the master's gain -- held to (a)'s bytes first; (c) render(gains=, pans=, master=).  Wall time with a device
    synchronise, medians; whole song and 4096-frame windows.  A tree whose render has no groups= runs (c) alone."""
    import inspect
    N.ensure_init(0)
    info = N.device_info()
    has = "groups" in inspect.signature(mixer.CompiledSequence.render).parameters
    print("sequence_groups_ab: SYNTHHIP_SEQ_ALIGN=%s  %s  groups=: %s" % (os.environ.get("SYNTHHIP_SEQ_ALIGN", "0"), info["name"] or info["arch"],
          "yes" if has else "no (the yardstick: (c) alone)"), flush=True)
    win, ntracks = 4096, len(TRACK_GAINS)
    desk = dict(gains=TRACK_GAINS, pans=DESK_PANS, master=DESK_MASTER)
    # the desk in order: (first, end, gain, factors) of a group, (first, end, None, None) of a stretch of loose tracks
    parts, at = [], 0
    for first, end, g, pan in GROUPS:
        if first > at:
            parts.append((at, first, None, None))
        parts.append((first, end, g, None if pan is None else pan_factors(pan)))
        at = end
    if at < ntracks:
        parts.append((at, ntracks, None, None))
    for nevents in (4096, 32768):
        what, nch, evs = meters_songs(nevents)[0]
        fb = nch * WIDTH
        bus = mixer.compile_tracks([evs[t::ntracks] for t in range(ntracks)], RATE, nch, WIDTH)
        frames = bus.frames
        out = N.DeviceBuffer(frames * fb + 16)
        wins = list(range(0, (frames - 3) // win, 16))

        def stream(render):
            for k in wins:
                render(k * win, win)
                N.sync()

        c_whole = median_wall(lambda: bus.render_into(out, 0, 0, frames, **desk), 2, 15)
        c_dev = five_medians(lambda: bus.render_into(out, 0, 0, frames, **desk))
        c_win = median_wall(lambda: stream(lambda a, n: bus.render_into(out, 0, a, n, **desk)), 1, 5) / len(wins)
        fmt = lambda v: " ".join("%.4f" % x for x in v)    # noqa: E731
        head = "groups song 120 s, %5d events, %s, %d tracks, level %s, %d frames   " % (nevents, what, ntracks, bus.level, frames)
        tail = "(c) render(gains=, pans=, master=): whole song, wall with a synchronise, median %.4f ms   between two events on the stream, five medians " \
               "of 15: %s ms   a window of %d frames, wall %.4f ms" % (c_whole, fmt(c_dev), win, c_win)
        if not has:
            print(head + tail, flush=True)
            bus.close()
            continue

        def caller(a, n):
            """(b): the window as a caller made it: one render per group or stretch, the others muted"""
            master = Sample(samplerate=RATE, nchannels=nch, samplewidth=WIDTH)
            for first, end, g, factors in parts:
                solo = [TRACK_GAINS[t] if first <= t < end else 0.0 for t in range(ntracks)]
                part = bus.render(a, n, gains=solo, pans=DESK_PANS)
                if g is not None and g != 1.0:
                    part.amplify(g)
                if factors is not None:
                    part.stereo(*factors)
                master.mix(part)
            return master.amplify(DESK_MASTER)

        mid = (frames // 2) // win * win
        parity = bytes(bus.render(groups=GROUPS, **desk).view_frame_data()) == bytes(caller(0, frames).view_frame_data()) and \
            bytes(bus.render(mid + 3, win, groups=GROUPS, **desk).view_frame_data()) == bytes(caller(mid + 3, win).view_frame_data())
        differs = bytes(bus.render(groups=GROUPS, **desk).view_frame_data()) != bytes(bus.render(**desk).view_frame_data())
        a_whole = median_wall(lambda: bus.render_into(out, 0, 0, frames, groups=GROUPS, **desk), 2, 15)
        a_dev = five_medians(lambda: bus.render_into(out, 0, 0, frames, groups=GROUPS, **desk))
        a_win = median_wall(lambda: stream(lambda a, n: bus.render_into(out, 0, a, n, groups=GROUPS, **desk)), 1, 5) / len(wins)
        b_whole = median_wall(lambda: caller(0, frames), 1, 5)
        b_win = median_wall(lambda: stream(caller), 1, 3) / len(wins)
        print(head + "(a) render(gains=, pans=, master=, groups=): whole song, wall with a synchronise, median %.4f ms   between two events on the "
              "stream, five medians of 15: %s ms   a window, wall %.4f ms   (b) %d renders with the others muted, amplify, stereo, mix, amplify: whole "
              "song, wall %.3f ms   a window, wall %.3f ms   %s   (a) / (b) whole %.4f, window %.4f   (a) / (c) whole %.3f, window %.3f   (a)'s bytes "
              "against (b)'s, whole and window: %s   (a) differs from (c): %s"
              % (a_whole, fmt(a_dev), a_win, len(parts), b_whole, b_win, tail, a_whole / b_whole, a_win / b_win, a_whole / c_whole, a_win / c_win,
                 "ok" if parity else "FAILED", "yes" if differs else "NO"), flush=True)
        assert parity and differs
        bus.close()


def bus_lanes(frames):
    """(the groups' lanes, the master's lane): a ride on each group of GROUPS -- a fade-out, a fade-in, a fade-in and a fade-out -- and on
    the master a fade-in, a hold at unity (no piece) and the fade-out of the whole song; whole seconds, so that Sample.fadein's seconds
    are exact frames, and every piece ends or starts at 1.0, so that Sample.fadein / fadeout state it"""
    groups = [[(20 * RATE, 30 * RATE, 1.0, 0.25)], [(10 * RATE, 25 * RATE, 0.3, 1.0)], [(0, 8 * RATE, 0.0, 1.0), (frames - 10 * RATE, frames, 1.0, 0.5)]]
    return groups, [(0, 4 * RATE, 0.0, 1.0), (frames - 6 * RATE, frames, 1.0, 0.0)]


def buses_main():
    """--buses: rides of the group buses and of the master in the render's own launch, on the song of --groups.  (a) render(gains=, pans=,
    master=, groups=, automation=<a ride on each group, a master fade-in / hold / fade-out>); (b) the caller's way: every group's stem with
    the other tracks muted, amplify, the ride with Sample.fadein / fadeout over the whole piece, clip and join, stereo, mix, the master's
    amplify, then the master's fades the same way -- held to (a)'s bytes first; (c) render(gains=, pans=, master=, groups=) without bus
    lanes.  Wall time with a device synchronise, medians; whole song and 4096-frame windows.  A tree whose automation() has no master=
    runs (c) alone: the parent's figure, row (d)."""
    import inspect
    N.ensure_init(0)
    info = N.device_info()
    has = "master" in inspect.signature(mixer.CompiledSequence.automation).parameters
    print("sequence_buses_ab: SYNTHHIP_SEQ_ALIGN=%s  %s  automation(master=, groups=): %s" % (
        os.environ.get("SYNTHHIP_SEQ_ALIGN", "0"), info["name"] or info["arch"], "yes" if has else "no (the yardstick: (c) alone)"), flush=True)
    win, ntracks = 4096, len(TRACK_GAINS)
    desk = dict(gains=TRACK_GAINS, pans=DESK_PANS, master=DESK_MASTER, groups=GROUPS)
    parts, at_track = [], 0                                     # the desk in order: (first, end, gain, factors, which group) or a loose stretch
    for k, (first, end, g, pan) in enumerate(GROUPS):
        if first > at_track:
            parts.append((at_track, first, None, None, None))
        parts.append((first, end, g, None if pan is None else pan_factors(pan), k))
        at_track = end
    if at_track < ntracks:
        parts.append((at_track, ntracks, None, None, None))
    for nevents in (4096, 32768):
        what, nch, evs = meters_songs(nevents)[0]
        fb = nch * WIDTH
        bus = mixer.compile_tracks([evs[t::ntracks] for t in range(ntracks)], RATE, nch, WIDTH)
        frames = bus.frames
        out = N.DeviceBuffer(frames * fb + 16)
        wins = list(range(0, (frames - 3) // win, 16))

        def stream(render):
            for k in wins:
                render(k * win, win)
                N.sync()

        c_whole = median_wall(lambda: bus.render_into(out, 0, 0, frames, **desk), 2, 15)
        c_dev = five_medians(lambda: bus.render_into(out, 0, 0, frames, **desk))
        c_win = median_wall(lambda: stream(lambda a, n: bus.render_into(out, 0, a, n, **desk)), 1, 5) / len(wins)
        fmt = lambda v: " ".join("%.4f" % x for x in v)    # noqa: E731
        head = "buses song 120 s, %5d events, %s, %d tracks, level %s, %d frames   " % (nevents, what, ntracks, bus.level, frames)
        tail = "(c) render(gains=, pans=, master=, groups=): whole song, wall with a synchronise, median %.4f ms   between two events on the stream, " \
               "five medians of 15: %s ms   a window of %d frames, wall %.4f ms" % (c_whole, fmt(c_dev), win, c_win)
        if not has:
            print(head + tail, flush=True)
            bus.close()
            continue
        glanes, mlane = bus_lanes(frames)
        auto = bus.automation([None] * ntracks, master=mlane, groups=glanes)
        at = lambda f: (f + 0.5) / RATE                     # noqa: E731  (seconds that Sample.frame_idx turns back into frame f)

        def rode(sample, a, n, pieces, whole):
            """``sample``, frames [a, a + n) of a bus behind its gain, with the pieces that reach into it: each faded over its WHOLE length
            (``whole(pa, length)`` makes that stretch of the bus) -- k counts from the piece's first sample --, clipped and joined in"""
            for pa, pb, v0, v1 in pieces:
                lo, hi = max(a, pa), min(a + n, pb)
                if lo >= hi:
                    continue
                move = whole(pa, pb - pa)
                move.fadein(move.duration, v0) if v1 == 1.0 else move.fadeout(move.duration, v1)
                move.clip(at(lo - pa), at(hi - pa))
                behind = sample.copy().clip(at(hi - a), at(n))
                sample.clip(0.0, at(lo - a)).join(move).join(behind)
            return sample

        def stem(first, end, g, a, n):
            solo = [TRACK_GAINS[t] if first <= t < end else 0.0 for t in range(ntracks)]
            part = bus.render(a, n, gains=solo, pans=DESK_PANS)
            return part.amplify(g) if g is not None and g != 1.0 else part

        def mixdown(a, n):
            """the master behind its gain and in front of its ride: one render per group or stretch, the others muted"""
            master = Sample(samplerate=RATE, nchannels=nch, samplewidth=WIDTH)
            for first, end, g, factors, k in parts:
                part = stem(first, end, g, a, n)
                if k is not None:
                    part = rode(part, a, n, glanes[k], lambda pa, length: stem(first, end, g, pa, length))
                if factors is not None:
                    part.stereo(*factors)
                master.mix(part)
            return master.amplify(DESK_MASTER)

        def caller(a, n):
            """(b): the window as a caller made it"""
            return rode(mixdown(a, n), a, n, mlane, mixdown)

        inside = (2 * RATE) // win * win + 3                    # a window three frames off inside the master's fade-in and group 2's
        assert mlane[0][0] < inside and inside + win < mlane[0][1] and glanes[2][0][0] < inside and inside + win < glanes[2][0][1]
        render = lambda *w: bytes(bus.render(*w, automation=auto, **desk).view_frame_data())      # noqa: E731
        parity = render() == bytes(caller(0, frames).view_frame_data()) and render(inside, win) == bytes(caller(inside, win).view_frame_data())
        differs = render(inside, win) != bytes(bus.render(inside, win, **desk).view_frame_data())
        a_whole = median_wall(lambda: bus.render_into(out, 0, 0, frames, automation=auto, **desk), 2, 15)
        a_dev = five_medians(lambda: bus.render_into(out, 0, 0, frames, automation=auto, **desk))
        a_win = median_wall(lambda: stream(lambda a, n: bus.render_into(out, 0, a, n, automation=auto, **desk)), 1, 5) / len(wins)
        b_whole = median_wall(lambda: caller(0, frames), 1, 3)
        b_win = median_wall(lambda: stream(caller), 1, 3) / len(wins)
        print(head + "(a) render(gains=, pans=, master=, groups=, automation=<bus lanes>): whole song, wall with a synchronise, median %.4f ms   between "
              "two events on the stream, five medians of 15: %s ms   a window, wall %.4f ms   (b) %d stems with the others muted, amplify, fadein / "
              "fadeout, clip, join, stereo, mix, amplify, the master's fades: whole song, wall %.3f ms   a window, wall %.3f ms   %s   (a) / (b) whole "
              "%.4f, window %.4f   (a) / (c) whole %.3f, window %.3f   (a)'s bytes against (b)'s, whole and a window inside two fades: %s   (a) differs "
              "from (c) there: %s"
              % (a_whole, fmt(a_dev), a_win, len(parts), b_whole, b_win, tail, a_whole / b_whole, a_win / b_win, a_whole / c_whole, a_win / c_win,
                 "ok" if parity else "FAILED", "yes" if differs else "NO"), flush=True)
        assert parity and differs
        auto.close()
        bus.close()


def pan_lanes(ntracks):
    """(the tracks' pan lanes, the groups' pan lanes): every track travels across the stereo field once, over a stretch of its own and
    in alternating directions; group 1 of GROUPS sweeps from left of centre to right of it"""
    tracks = [[((5 + 3 * t) * RATE, (35 + 9 * t) * RATE, -1.0 if t % 2 else 1.0, 1.0 if t % 2 else -1.0)] for t in range(ntracks)]
    return tracks, [None, [(12 * RATE, 60 * RATE, -0.8, 0.6)], None]


def pans_main():
    """--pans: pan rides of the tracks and of a group in the render's own launch, on the song of --buses with its bus lanes.  (a) render(gains=,
    pans=, master=, groups=, automation=<bus lanes and pan lanes>); (b) the caller's way: every track's stem, clipped at every move,
    Sample.pan(lfo=ramp) on the clips a piece covers, stereo on the rest, join, mix, and the buses' steps of --buses with the group's pan
    step the same way -- held to (a)'s bytes first; (c) the same render with an Automation without pan lanes.  Wall time with a device
    synchronise, medians; whole song and 4096-frame windows.  A tree whose automation() has no pans= runs (c) alone: the parent's figure,
    row (d)."""
    import inspect
    N.ensure_init(0)
    info = N.device_info()
    has = "pans" in inspect.signature(mixer.CompiledSequence.automation).parameters
    print("sequence_pans_ab: SYNTHHIP_SEQ_ALIGN=%s  %s  automation(pans=, group_pans=): %s" % (
        os.environ.get("SYNTHHIP_SEQ_ALIGN", "0"), info["name"] or info["arch"], "yes" if has else "no (the yardstick: (c) alone)"), flush=True)
    win, ntracks = 4096, len(TRACK_GAINS)
    desk = dict(gains=TRACK_GAINS, pans=DESK_PANS, master=DESK_MASTER, groups=GROUPS)
    parts, at_track = [], 0                                     # the desk in order: (first, end, gain, static pan, which group) or a loose stretch
    for k, (first, end, g, pan) in enumerate(GROUPS):
        if first > at_track:
            parts.append((at_track, first, None, None, None))
        parts.append((first, end, g, pan, k))
        at_track = end
    if at_track < ntracks:
        parts.append((at_track, ntracks, None, None, None))
    for nevents in (4096, 32768):
        what, nch, evs = meters_songs(nevents)[0]
        fb = nch * WIDTH
        bus = mixer.compile_tracks([evs[t::ntracks] for t in range(ntracks)], RATE, nch, WIDTH)
        frames = bus.frames
        out = N.DeviceBuffer(frames * fb + 16)
        wins = list(range(0, (frames - 3) // win, 16))
        glanes, mlane = bus_lanes(frames)
        plain = bus.automation([None] * ntracks, master=mlane, groups=glanes)

        def stream(render):
            for k in wins:
                render(k * win, win)
                N.sync()

        c_whole = median_wall(lambda: bus.render_into(out, 0, 0, frames, automation=plain, **desk), 2, 15)
        c_dev = five_medians(lambda: bus.render_into(out, 0, 0, frames, automation=plain, **desk))
        c_win = median_wall(lambda: stream(lambda a, n: bus.render_into(out, 0, a, n, automation=plain, **desk)), 1, 5) / len(wins)
        fmt = lambda v: " ".join("%.4f" % x for x in v)    # noqa: E731
        head = "pans song 120 s, %5d events, %s, %d tracks, level %s, %d frames   " % (nevents, what, ntracks, bus.level, frames)
        tail = "(c) render(gains=, pans=, master=, groups=, automation=<bus lanes>): whole song, wall with a synchronise, median %.4f ms   between two " \
               "events on the stream, five medians of 15: %s ms   a window of %d frames, wall %.4f ms" % (c_whole, fmt(c_dev), win, c_win)
        if not has:
            print(head + tail, flush=True)
            plain.close()
            bus.close()
            continue
        tpans, gpans = pan_lanes(ntracks)
        auto = bus.automation([None] * ntracks, master=mlane, groups=glanes, pans=tpans, group_pans=gpans)
        at = lambda f: (f + 0.5) / RATE                     # noqa: E731  (seconds that Sample.frame_idx turns back into frame f)

        def panned(sample, a, n, pieces, pan):
            """``sample``, frames [a, a + n) of a track or a bus in front of its pan step: clipped at every move, Sample.pan(lfo=ramp) on the
            clips a piece covers -- the ramp's values counted from the piece's first frame --, the static pan on the rest, joined"""
            clips, pos = [], a

            def rest(lo, hi):
                clip = sample.copy().clip(at(lo - a), at(hi - a))
                clips.append(clip if pan is None else clip.stereo(*pan_factors(pan)))
            for pa, pb, p0, p1 in pieces or ():
                lo, hi = max(a, pa), min(a + n, pb)
                if lo >= hi:
                    continue
                if lo > pos:
                    rest(pos, lo)
                length = pb - pa
                ramp = [k * (p1 - p0) / length + p0 for k in range(lo - pa, hi - pa)]
                clips.append(sample.copy().clip(at(lo - a), at(hi - a)).pan(lfo=ramp))
                pos = hi
            if pos < a + n:
                rest(pos, a + n)
            whole = clips[0]
            for clip in clips[1:]:
                whole.join(clip)
            return whole

        def rode(sample, a, n, pieces, whole):
            """--buses' way of a fader ride: each piece that reaches into the window faded over its WHOLE length, clipped and joined in"""
            for pa, pb, v0, v1 in pieces:
                lo, hi = max(a, pa), min(a + n, pb)
                if lo >= hi:
                    continue
                move = whole(pa, pb - pa)
                move.fadein(move.duration, v0) if v1 == 1.0 else move.fadeout(move.duration, v1)
                move.clip(at(lo - pa), at(hi - pa))
                behind = sample.copy().clip(at(hi - a), at(n))
                sample.clip(0.0, at(lo - a)).join(move).join(behind)
            return sample

        def track(t, a, n):
            """track t as its bus takes it: its stem at its gain, then its pan step"""
            return panned(bus.render(a, n, gains=[TRACK_GAINS[t] if u == t else 0.0 for u in range(ntracks)]), a, n, tpans[t], DESK_PANS[t])

        def scaled(first, end, g, a, n):
            """a group's bus behind its gain, in front of its ride"""
            grp = Sample(samplerate=RATE, nchannels=nch, samplewidth=WIDTH)
            for t in range(first, end):
                grp.mix(track(t, a, n))
            return grp.amplify(g) if g != 1.0 else grp

        def mixdown(a, n):
            """the master behind its gain and in front of its ride"""
            master = Sample(samplerate=RATE, nchannels=nch, samplewidth=WIDTH)
            for first, end, g, pan, k in parts:
                if k is None:
                    for t in range(first, end):
                        master.mix(track(t, a, n))
                    continue
                grp = rode(scaled(first, end, g, a, n), a, n, glanes[k], lambda pa, length: scaled(first, end, g, pa, length))
                master.mix(panned(grp, a, n, gpans[k], pan))
            return master.amplify(DESK_MASTER)

        def caller(a, n):
            """(b): the window as a caller made it"""
            return rode(mixdown(a, n), a, n, mlane, mixdown)

        inside = (22 * RATE) // win * win + 3                   # a window three frames off inside group 0's fade, group 1's sweep and five tracks' sweeps
        assert glanes[0][0][0] < inside and inside + win < glanes[0][0][1] and gpans[1][0][0] < inside and inside + win < gpans[1][0][1]
        assert sum(lane[0][0] < inside and inside + win < lane[0][1] for lane in tpans) >= 4
        render = lambda *w: bytes(bus.render(*w, automation=auto, **desk).view_frame_data())      # noqa: E731
        parity = render() == bytes(caller(0, frames).view_frame_data()) and render(inside, win) == bytes(caller(inside, win).view_frame_data())
        differs = render(inside, win) != bytes(bus.render(inside, win, automation=plain, **desk).view_frame_data())
        a_whole = median_wall(lambda: bus.render_into(out, 0, 0, frames, automation=auto, **desk), 2, 15)
        a_dev = five_medians(lambda: bus.render_into(out, 0, 0, frames, automation=auto, **desk))
        a_win = median_wall(lambda: stream(lambda a, n: bus.render_into(out, 0, a, n, automation=auto, **desk)), 1, 5) / len(wins)
        b_whole = median_wall(lambda: caller(0, frames), 0, 3)
        b_win = median_wall(lambda: stream(caller), 0, 3) / len(wins)
        print(head + "(a) render(gains=, pans=, master=, groups=, automation=<bus lanes and pan lanes>): whole song, wall with a synchronise, median "
              "%.4f ms   between two events on the stream, five medians of 15: %s ms   a window, wall %.4f ms   (b) %d stems, clip, Sample.pan(lfo=ramp), "
              "stereo, join, mix, the buses' amplify, fades and pan steps, the master's amplify and fades: whole song, wall %.3f ms   a window, wall "
              "%.3f ms   %s   (a) / (b) whole %.5f, window %.4f   (a) / (c) whole %.3f, window %.3f   (a)'s bytes against (b)'s, whole and a window "
              "inside the sweeps: %s   (a) differs from (c) there: %s"
              % (a_whole, fmt(a_dev), a_win, ntracks, b_whole, b_win, tail, a_whole / b_whole, a_win / b_win, a_whole / c_whole, a_win / c_win,
                 "ok" if parity else "FAILED", "yes" if differs else "NO"), flush=True)
        assert parity and differs
        auto.close()
        plain.close()
        bus.close()


def history_main():
    """--history: the levels of the whole song per block of the song's tile grid.  (a) render_into(meters="history", gains=, pans=, master=,
    groups=), the one launch; (b) the caller's way today: chunks(block_frames, meters=True, ...) over the whole song, one metered render
    per block -- its master rows held to (a)'s first; (c) render_into(meters=True, ...) of the whole song.  Wall time with a device
    synchronise, medians.  A tree without meters="history" runs (c) alone."""
    N.ensure_init(0)
    info = N.device_info()
    has = hasattr(mixer, "SongHistory")
    print("sequence_history_ab: SYNTHHIP_SEQ_ALIGN=%s  %s  meters=\"history\": %s" % (os.environ.get("SYNTHHIP_SEQ_ALIGN", "0"), info["name"] or info["arch"],
          "yes" if has else "no (the yardstick: (c) alone)"), flush=True)
    ntracks = len(TRACK_GAINS)
    desk = dict(gains=TRACK_GAINS, pans=DESK_PANS, master=DESK_MASTER, groups=GROUPS)
    for nevents in (4096, 32768):
        what, nch, evs = meters_songs(nevents)[0]
        fb = nch * WIDTH
        bus = mixer.compile_tracks([evs[t::ntracks] for t in range(ntracks)], RATE, nch, WIDTH)
        frames = bus.frames
        out = N.DeviceBuffer(frames * fb + 16)
        c_whole = median_wall(lambda: bus.render_into(out, 0, 0, frames, meters=True, **desk), 2, 15)
        c_dev = five_medians(lambda: bus.render_into(out, 0, 0, frames, meters=True, **desk))
        fmt = lambda v: " ".join("%.4f" % x for x in v)    # noqa: E731
        head = "history song 120 s, %5d events, %s, %d tracks, %d groups, level %s, %d frames   " % (nevents, what, ntracks, len(GROUPS), bus.level, frames)
        tail = "(c) render(meters=True, gains=, pans=, master=, groups=): whole song, wall with a synchronise, median %.4f ms   between two events on " \
               "the stream, five medians of 15: %s ms" % (c_whole, fmt(c_dev))
        if not has:
            print(head + tail, flush=True)
            bus.close()
            continue
        block = TILE // nch

        def caller():
            """(b): a metered render per block, the levels kept"""
            return [lv for _s, lv in bus.chunks(block, meters=True, **desk)]

        h = bus.render_into(out, 0, 0, frames, meters="history", **desk)
        theirs = caller()
        parity = h.nblocks == len(theirs) and all(h[j] == lv for j, lv in enumerate(theirs)) and h.total() == bus.render_into(out, 0, 0, frames, meters=True, **desk)
        a_whole = median_wall(lambda: bus.render_into(out, 0, 0, frames, meters="history", **desk), 2, 15)
        a_dev = five_medians(lambda: bus.render_into(out, 0, 0, frames, meters="history", **desk))
        a_raw = median_wall(lambda: bus._handle().render(0, frames * nch, out, 0, gains=list(TRACK_GAINS), meters="history", pans=bus._pans(DESK_PANS),
                                                         master=DESK_MASTER, groups=bus._groups(GROUPS)), 2, 15)
        b_whole = median_wall(caller, 1, 3)
        print(head + "(a) render(meters=\"history\", gains=, pans=, master=, groups=): %d blocks of %d frames, %d rows each: whole song, wall with a "
              "synchronise, median %.4f ms (the entry point alone, without the SongHistory: %.4f ms)   between two events on the stream, five medians "
              "of 15: %s ms   (b) chunks(%d, meters=True, ...), %d metered renders: whole song, wall %.3f ms   %s   (a) / (b) %.5f   (a) / (c) %.3f   "
              "(a)'s blocks against (b)'s levels and its total against (c)'s: %s"
              % (h.nblocks, block, ntracks + 1 + len(GROUPS), a_whole, a_raw, fmt(a_dev), block, len(theirs), b_whole, tail, a_whole / b_whole,
                 a_whole / c_whole, "ok" if parity else "FAILED"), flush=True)
        assert parity
        bus.close()


def clips_main(trace=False):
    """--clips: what the overs cost.  (a) render_into(meters="history", clips=True, gains=, pans=, master=, groups=) of the whole song and of a
    4096-frame window; (c) the same call without clips; (m) meters=True.  A tree without clips= runs (c) and (m) alone."""
    import inspect
    N.ensure_init(0)
    info = N.device_info()
    has = "clips" in inspect.signature(mixer.CompiledSequence.render_into).parameters
    print("sequence_clips_ab: SYNTHHIP_SEQ_ALIGN=%s  %s  clips=: %s" % (os.environ.get("SYNTHHIP_SEQ_ALIGN", "0"), info["name"] or info["arch"],
          "yes" if has else "no (the yardstick: (c) and meters=True alone)"), flush=True)
    ntracks = len(TRACK_GAINS)
    desk = dict(gains=TRACK_GAINS, pans=DESK_PANS, master=DESK_MASTER, groups=GROUPS)
    fmt = lambda v: " ".join("%.4f" % x for x in v)        # noqa: E731
    for nevents in (4096, 32768):
        what, nch, evs = meters_songs(nevents)[0]
        fb = nch * WIDTH
        bus = mixer.compile_tracks([evs[t::ntracks] for t in range(ntracks)], RATE, nch, WIDTH)
        frames = bus.frames
        out = N.DeviceBuffer(frames * fb + 16)
        win = 4096
        at = (22 * RATE) // win * win + 3                      # a window three frames off the tile grid, inside the song
        whole = lambda **kw: bus.render_into(out, 0, 0, frames, **kw, **desk)       # noqa: E731
        window = lambda **kw: bus.render_into(out, 0, at, win, **kw, **desk)        # noqa: E731
        if trace:
            for _ in range(5):
                whole(meters="history", clips=True)
                whole(meters="history")
                window(meters="history", clips=True)
                window(meters="history")
            N.sync()
            bus.close()
            continue
        head = "clips song 120 s, %5d events, %s, %d tracks, %d groups, level %s, %d frames   " % (nevents, what, ntracks, len(GROUPS), bus.level, frames)
        rows = []
        for name, kw in (("(c) render(meters=\"history\", ...)", dict(meters="history")), ("(m) render(meters=True, ...)", dict(meters=True))) + \
                ((("(a) render(meters=\"history\", clips=True, ...)", dict(meters="history", clips=True)),) if has else ()):
            rows.append((name, median_wall(lambda: whole(**kw), 2, 15), five_medians(lambda: whole(**kw)), median_wall(lambda: window(**kw), 2, 15),
                         five_medians(lambda: window(**kw))))
        text = "   ".join("%s: whole song, wall with a synchronise, median %.4f ms, between two events on the stream, five medians of 15: %s ms; a window of "
                          "%d frames, wall %.4f ms, events %s ms" % (name, w, fmt(wd), win, x, fmt(xd)) for name, w, wd, x, xd in rows)
        if has:
            h, plain = whole(meters="history", clips=True), whole(meters="history")
            counted = h.clipped().sum(axis=0)
            parity = plain.clipped() is None and h.total() == plain.total() and all(h[j] == plain[j] for j in range(0, h.nblocks, 97))
            text += "   (a) / (c) whole %.3f, window %.3f   overs of the whole song per row (left, right): %s   (a)'s levels against (c)'s: %s" % (
                rows[2][1] / rows[0][1], rows[2][3] / rows[0][3], counted.tolist(), "ok" if parity else "FAILED")
            assert parity
        print(head + text, flush=True)
        bus.close()


def stems_main(trace=False):
    """--stems: every bus of the desk from one launch, on the song of --pans (8 tracks, 3 groups, bus lanes and pan lanes).  (a) one
    stems_into of the whole song and of a 4096-frame window; (b) the caller's way: one render per row with everything else muted -- a track
    through a second desk (no groups, no master gain) and a second Automation holding the tracks' lanes alone, a group through a third
    Automation without the master's lane, the master as it is -- into the same planes, held to (a)'s bytes first; (c) render_into with the
    same desk.  Wall time with a device synchronise, medians of 15.  A tree without stems_into runs (c) alone: the parent's figure, row (d).
    --stems-trace: each call five times and nothing else, for a kernel trace."""
    N.ensure_init(0)
    info = N.device_info()
    has = hasattr(mixer.CompiledSequence, "stems_into")
    print("sequence_stems_ab: SYNTHHIP_SEQ_ALIGN=%s  %s  stems_into: %s" % (os.environ.get("SYNTHHIP_SEQ_ALIGN", "0"), info["name"] or info["arch"],
          "yes" if has else "no (the yardstick: (c) alone)"), flush=True)
    win, ntracks = 4096, len(TRACK_GAINS)
    desk = dict(gains=TRACK_GAINS, pans=DESK_PANS, master=DESK_MASTER, groups=GROUPS)
    nrows = ntracks + 1 + len(GROUPS)
    fmt = lambda v: " ".join("%.4f" % x for x in v)        # noqa: E731
    for nevents in (4096, 32768):
        what, nch, evs = meters_songs(nevents)[0]
        fb = nch * WIDTH
        bus = mixer.compile_tracks([evs[t::ntracks] for t in range(ntracks)], RATE, nch, WIDTH)
        frames = bus.frames
        glanes, mlane = bus_lanes(frames)
        tpans, gpans = pan_lanes(ntracks)
        auto = bus.automation([None] * ntracks, master=mlane, groups=glanes, pans=tpans, group_pans=gpans)
        at = (22 * RATE) // win * win + 3                      # a window three frames off the tile grid, inside the sweeps
        out = N.DeviceBuffer(frames * fb + 16)
        c_whole = lambda: bus.render_into(out, 0, 0, frames, automation=auto, **desk)      # noqa: E731
        c_win = lambda: bus.render_into(out, 0, at, win, automation=auto, **desk)           # noqa: E731
        head = "stems song 120 s, %5d events, %s, %d tracks, %d groups, %d rows, level %s, %d frames   " % (
            nevents, what, ntracks, len(GROUPS), nrows, bus.level, frames)
        if not has:
            if not trace:
                print(head + "(c) render_into(gains=, pans=, master=, groups=, automation=): whole song, wall with a synchronise, median %.4f ms, between "
                      "two events on the stream, five medians of 15: %s ms; a window of %d frames, wall %.4f ms, events %s ms"
                      % (median_wall(c_whole, 2, 15), fmt(five_medians(c_whole)), win, median_wall(c_win, 2, 15), fmt(five_medians(c_win))), flush=True)
            auto.close()
            bus.close()
            continue
        plane = bus.stems_plane_frames(frames, nch, WIDTH)
        wplane = bus.stems_plane_frames(win, nch, WIDTH)
        planes = N.DeviceBuffer(nrows * plane * fb)
        theirs = N.DeviceBuffer(nrows * plane * fb)
        a_whole = lambda: bus.stems_into(planes, 0, plane, 0, frames, automation=auto, **desk)     # noqa: E731
        a_win = lambda: bus.stems_into(planes, 0, wplane, at, win, automation=auto, **desk)         # noqa: E731
        # (b): the second desk and the second and third Automation a caller has to build
        tracks_only = bus.automation([None] * ntracks, pans=tpans)
        no_master = bus.automation([None] * ntracks, groups=glanes, pans=tpans, group_pans=gpans)

        def caller(a, n, stride):
            for t in range(ntracks):                            # a track as its bus takes it: no groups, no master gain, its own lanes
                bus.render_into(theirs, t * stride * fb, a, n, gains=[TRACK_GAINS[t] if u == t else 0.0 for u in range(ntracks)], pans=DESK_PANS,
                                automation=tracks_only)
            bus.render_into(theirs, ntracks * stride * fb, a, n, automation=auto, **desk)
            for k, (first, end, _g, _pan) in enumerate(GROUPS):  # a group as the master takes it: its tracks alone, no master gain, no master ride
                bus.render_into(theirs, (ntracks + 1 + k) * stride * fb, a, n, gains=[TRACK_GAINS[u] if first <= u < end else 0.0 for u in range(ntracks)],
                                pans=DESK_PANS, groups=GROUPS, automation=no_master)
        b_whole = lambda: caller(0, frames, plane)              # noqa: E731
        b_win = lambda: caller(at, win, wplane)                 # noqa: E731
        if trace:
            for _ in range(5):
                a_whole(), b_whole(), c_whole(), a_win(), b_win(), c_win()
            N.sync()
        else:
            parity = True
            for mine, other, n, stride in ((a_win, b_win, win, wplane), (a_whole, b_whole, frames, plane)):
                planes.zero()
                theirs.zero()
                mine()
                other()
                N.sync()
                size = ((nrows - 1) * stride + n) * fb
                step = 1 << 26
                for off in range(0, size, step):
                    parity = parity and planes.download_bytes(min(step, size - off), off) == theirs.download_bytes(min(step, size - off), off)
            c_whole()                                           # (planes holds (a)'s whole song: its master plane against the render's bytes)
            N.sync()
            head_bytes = min(1 << 24, frames * fb)
            master_same = planes.download_bytes(head_bytes, ntracks * plane * fb) == out.download_bytes(head_bytes)
            rows =[(name, median_wall(w, 2, 15), five_medians(w), median_wall(x, 2, 15), five_medians(x)) for name, w, x in (
                ("(a) stems_into: %d planes, one launch" % nrows, a_whole, a_win), ("(b) %d renders with mutes, a second desk, three Automations" % nrows, b_whole, b_win),
                ("(c) render_into with the same desk", c_whole, c_win))]
            text = "   ".join("%s: whole song, wall with a synchronise, median %.4f ms, between two events on the stream, five medians of 15: %s ms; a window "
                              "of %d frames, wall %.4f ms, events %s ms" % (name, w, fmt(wd), win, x, fmt(xd)) for name, w, wd, x, xd in rows)
            print(head + text + "   (a) / (b) whole %.3f, window %.3f   (a) / (c) whole %.3f, window %.3f   bytes written by (a): whole %.1f MB, window %.3f MB   "
                  "(b)'s bytes against (a)'s, whole and window, every plane: %s   (a)'s master plane against (c)'s bytes: %s"
                  % (rows[0][1] / rows[1][1], rows[0][3] / rows[1][3], rows[0][1] / rows[2][1], rows[0][3] / rows[2][3], nrows * frames * fb / 1e6,
                     nrows * win * fb / 1e6, "ok" if parity else "FAILED", "ok" if master_same else "FAILED"), flush=True)
            assert parity and master_same
        for h in (tracks_only, no_master, auto):
            h.close()
        bus.close()


def median_wall(fn, warm, passes):
    for _ in range(warm):
        fn()
    N.sync()
    runs = []
    for _ in range(passes):
        N.sync()
        t0 = time.perf_counter()
        fn()
        N.sync()
        runs.append((time.perf_counter() - t0) * 1e3)
    return sorted(runs)[len(runs) // 2]


def main():
    N.ensure_init(0)
    print("sequence_ab: SYNTHHIP_SEQ_ALIGN=%s  %s" % (os.environ.get("SYNTHHIP_SEQ_ALIGN", "0"), N.device_info()["name"]), flush=True)
    rows = [("song 120 s, 4096 events", song(4096, 120.0), 3), ("song 120 s, 32768 events", song(32768, 120.0), 2),
            ("echo-shaped, 8 events", echo_list(), 7), ("64 x whole 10-s track", whole_tracks(), 5)]
    for name, (base, sources, events), loop_passes in rows:
        samples = [Sample.from_raw_frames(b, WIDTH, RATE, NCH).to_device() for b in sources]
        start = Sample.from_raw_frames(base, WIDTH, RATE, NCH).to_device()
        evs = [(s, samples[i], v) for s, i, v in events]
        got = start.copy().mix_at_many(evs)
        want = oracle(base, sources, events)
        parity = bytes(got.view_frame_data()) == want
        del got

        def loop():
            t = start.copy()
            for seconds, other, volume in evs:
                t.mix_at(seconds, other if volume is None else other.at_volume(volume))

        def many():
            start.copy().mix_at_many(evs)

        loop_ms = median_wall(loop, 1, loop_passes)
        many_ms = median_wall(many, 3, 9)
        # the one call on its own, on a track that is already long enough (in place): device time between two events on the stream
        track = Sample.from_raw_frames(bytes(len(want)), WIDTH, RATE, NCH).to_device()
        for _ in range(3):
            track.mix_at_many(evs)
        dev = []
        for _ in range(9):
            N.sync()
            N.timer_start()
            track.mix_at_many(evs)
            dev.append(N.timer_stop())
        dev_ms = sorted(dev)[len(dev) // 2]
        lb = logical_bytes(sources, events, len(want))
        print("%-26s loop %9.3f ms   mix_at_many %8.3f ms   ratio %7.1fx   device (in place) %7.4f ms   logical %.3f TB/s (%.1f MB)   parity %s"
              % (name, loop_ms, many_ms, loop_ms / many_ms, dev_ms, lb / (dev_ms * 1e-3) / 1e12, lb / 1e6, "ok" if parity else "FAILED"), flush=True)
        if name.startswith("64 x"):
            mixed = mixer.mix_samples(samples)
            same = bytes(mixed.view_frame_data()) == want
            g = []
            for _ in range(3):
                mixer.mix_samples(samples)
            for _ in range(9):
                N.sync()
                N.timer_start()
                mixer.mix_samples(samples)
                g.append(N.timer_stop())
            g_ms = sorted(g)[len(g) // 2]
            gb = 65 * len(want)
            print("%-26s mixer.mix_samples (aligned gather fold) device %7.4f ms   %.3f TB/s of its %.1f MB   same bytes %s"
                  % ("", g_ms, gb / (g_ms * 1e-3) / 1e12, gb / 1e6, "ok" if same else "FAILED"), flush=True)


if __name__ == "__main__":
    stems_main("--stems-trace" in sys.argv[1:]) if "--stems" in sys.argv[1:] or "--stems-trace" in sys.argv[1:] else clips_main("--clips-trace" in sys.argv[1:]) if "--clips" in sys.argv[1:] or "--clips-trace" in sys.argv[1:] else history_main() if "--history" in sys.argv[1:] else pans_main() if "--pans" in sys.argv[1:] else buses_main() if "--buses" in sys.argv[1:] else groups_main() if "--groups" in sys.argv[1:] else auto_main() if "--auto" in sys.argv[1:] or "--auto-trace" in sys.argv[1:] else desk_main() if "--desk" in sys.argv[1:] else meters_main() if "--meters" in sys.argv[1:] or "--meters-trace" in sys.argv[1:] else tracks_main() if "--tracks" in sys.argv[1:] else plan_main() if "--plan" in sys.argv[1:] else chan_main() if "--channels" in sys.argv[1:] else rev_main() if "--reverse" in sys.argv[1:] else loop_main() if "--loop" in sys.argv[1:] else env_main() if "--env" in sys.argv[1:] else pan_main() if "--pan" in sys.argv[1:] else sampler_main() if "--sampler" in sys.argv[1:] else main()
