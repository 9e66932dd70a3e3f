#!/usr/bin/env python3
"""Levels over time of plain PCM and of a song's stems: sh_pcm_level_blocks against the ways a caller had.

    python tools/level_blocks_ab.py            the table below
    python tools/level_blocks_ab.py --trace    each (a) five times and nothing else, for rocprofv3 --kernel-trace --stats -- python ...
    python tools/level_blocks_ab.py --extents [--trace]    the waveform extremes of the same two buffers (extents() below; profiles/waveform_ab.txt)

Wall time with a device synchronise, medians of 15 after a warm-up of every shape; the compared variants run by turns in one process.
(a)  one level_history at 1024-frame blocks: of a 120-s, 48-kHz stereo 16-bit Sample, and of the 12-plane stems buffer of the --stems
     song of tools/sequence_ab.py (8 tracks, 3 groups, bus rides and pan rides).
(b)  the caller's way today: a view and level_db_peak per block (per block and row for the stems).  Its per-block cost is taken from
     300 blocks and SCALED to the whole length; it is not run in full.
(c)  sh_pcm_stats_stereo over the same bytes: it reads what (a) reads and writes one row.  Measured with this tree's library, whose
     k_pcm_stats is the parent commit's instruction for instruction (tools/kernel_diff.py), so the figure is the parent's as well.
(a2) CompiledSequence.level_history of the --pans song (rides and pan rides) against chunks(1024, meters=True) of the same desk, run in
     full once, and against render(meters="history") of the --groups desk (no rides) of the same song, for scale.
The kernel's own time comes from the --trace run under rocprofv3; (a)'s bytes over that time stand against the HBM peak."""
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import sequence_ab as S  # noqa: E402  (the songs, desks and timers of the sequence tools; it puts this tree's package on the path)
from synthesizer_amd import _native as N  # noqa: E402
from synthesizer_amd import mixer  # noqa: E402
from synthesizer_amd.sample import Sample  # noqa: E402

RATE, WIDTH, BLOCK, SCALED_FROM = 48000, 2, 1024, 300
C = N.C


def by_turns(variants, warm=2, passes=15):
    """{name: (median ms, min ms, max ms)}: every variant warmed up, then one pass of each by turns, `passes` times"""
    for fn in variants.values():
        for _ in range(warm):
            fn()
    N.sync()
    runs = {name: [] for name in variants}
    for _ in range(passes):
        for name, fn in variants.items():
            N.sync()
            t0 = time.perf_counter()
            fn()
            N.sync()
            runs[name].append((time.perf_counter() - t0) * 1e3)
    return {name: (float(np.median(v)), min(v), max(v)) for name, v in runs.items()}


def per_block_caller(rows, frames, fb):
    """(b): ms per block of a view and level_db_peak per block and row, over SCALED_FROM blocks spread across the length"""
    nblocks = frames // BLOCK
    picks = [int(k * (nblocks - 1) / (SCALED_FROM - 1)) for k in range(SCALED_FROM)]

    def one_pass():
        for j in picks:
            for buf, off in rows:
                s = Sample(samplerate=RATE, nchannels=2, samplewidth=WIDTH)
                s._set_device(buf.view(off + j * BLOCK * fb, BLOCK * fb), BLOCK * fb)
                s.level_db_peak
    one_pass()
    N.sync()
    t0 = time.perf_counter()
    one_pass()
    N.sync()
    return (time.perf_counter() - t0) * 1e3 / SCALED_FROM


def stats_stereo(buf, nframes):
    mx, sq = (C.c_uint32 * 2)(), (C.c_double * 2)()
    return lambda: N.check(N.lib().sh_pcm_stats_stereo(buf.handle, nframes, WIDTH, mx, sq))


def show(title, nbytes, got):
    for name, (med, lo, hi) in got.items():
        print("  %-68s median %8.4f ms  (min %.4f, max %.4f)   %7.1f GB/s of %d bytes by wall" % (title + name, med, lo, hi, nbytes / med / 1e6, nbytes), flush=True)


def main(trace=False):
    N.ensure_init(0)
    info = N.device_info()
    print("level_blocks_ab: %s" % (info["name"] or info["arch"]), flush=True)
    fb = 2 * WIDTH
    frames = 120 * RATE
    pcm = np.random.default_rng(0).integers(-32768, 32768, size=2 * frames, dtype=np.int16)
    sample = Sample.from_raw_frames(pcm.tobytes(), WIDTH, RATE, 2).to_device()
    a_sample = lambda: sample.level_history(BLOCK)               # noqa: E731
    # the --stems song and its desk
    ntracks = len(S.TRACK_GAINS)
    what, nch, evs = S.meters_songs(4096)[0]
    bus = mixer.compile_tracks([evs[t::ntracks] for t in range(ntracks)], RATE, nch, WIDTH)
    glanes, mlane = S.bus_lanes(bus.frames)
    tpans, gpans = S.pan_lanes(ntracks)
    auto = bus.automation([None] * ntracks, master=mlane, groups=glanes, pans=tpans, group_pans=gpans)
    desk = dict(gains=S.TRACK_GAINS, pans=S.DESK_PANS, master=S.DESK_MASTER, groups=S.GROUPS)
    stems = bus.stems(automation=auto, **desk)
    nrows, plane = len(stems), stems._plane_frames
    a_stems = lambda: stems.level_history(BLOCK)                 # noqa: E731
    if trace:
        for fn in (a_sample, a_stems):
            for _ in range(5):
                fn()
        N.sync()
        return
    h = a_sample()
    assert h.total().master.peak == sample._channel_stats()[0], "the history's total is not the whole sample's peak"
    print("(a) / (c)  a Sample of 120 s, 48 kHz, stereo, 16 bits: %d frames, %d blocks of %d frames" % (frames, len(h), BLOCK), flush=True)
    show("", frames * fb, by_turns({"(a) Sample.level_history(1024): one launch, the table copied back": a_sample,
                                    "(c) sh_pcm_stats_stereo over the same bytes: one row": stats_stereo(sample._device(), frames)}))
    per = per_block_caller([(sample._device(), 0)], frames, fb)
    print("  (b) a view and level_db_peak per block: %.4f ms per block over %d blocks, SCALED to %d blocks: %.1f ms" % (per, SCALED_FROM, len(h), per * len(h)), flush=True)
    hs = a_stems()
    print("(a) / (c)  the stems of the --stems song (%s): %d planes of %d frames, %d blocks of %d frames" % (what, nrows, bus.frames, len(hs), BLOCK), flush=True)
    show("", nrows * bus.frames * fb, by_turns({"(a) SongStems.level_history(1024): one launch over %d planes" % nrows: a_stems,
                                               "(c) sh_pcm_stats_stereo over the planes' buffer: one row": stats_stereo(stems._buffer, nrows * plane)}))
    per = per_block_caller([(stems._buffer, r * plane * fb) for r in range(nrows)], bus.frames, fb)
    print("  (b) a view and level_db_peak per block and row: %.4f ms per block (%d rows) over %d blocks, SCALED to %d blocks: %.1f ms"
          % (per, nrows, SCALED_FROM, len(hs), per * len(hs)), flush=True)
    # (a2): the whole route for a desk that rides
    a2 = lambda: bus.level_history(block_frames=BLOCK, automation=auto, **desk)      # noqa: E731
    plain = lambda: bus.render(meters="history", **desk)        # noqa: E731
    print("(a2) the --pans song, %d frames: stems + level_history (two launches), and for scale render(meters=\"history\") of the --groups desk (no rides)" % bus.frames, flush=True)
    show("", nrows * bus.frames * fb, by_turns({"(a2) CompiledSequence.level_history(block_frames=1024, rides and pan rides)": a2,
                                               "     render(meters=\"history\"), the --groups desk, one launch": plain}, passes=9))
    for _ in zip(range(200), bus.chunks(BLOCK, meters=True, automation=auto, **desk)):
        pass
    N.sync()
    t0 = time.perf_counter()
    count = sum(1 for _ in bus.chunks(BLOCK, meters=True, automation=auto, **desk))
    N.sync()
    print("  chunks(1024, meters=True) of the same desk, in full, once: %d chunks, %.1f ms" % (count, (time.perf_counter() - t0) * 1e3), flush=True)
    auto.close()
    bus.close()


def numpy_extents(pcm, block):
    """the caller's way: (lo, hi), each (nblocks, channels), of a [frames, channels] array by reshape, min and max per block"""
    whole = len(pcm) // block
    body = pcm[:whole * block].reshape(whole, block, pcm.shape[1])
    lo, hi = body.min(axis=1), body.max(axis=1)
    if len(pcm) % block:                                        # the last, partial block
        lo, hi = np.vstack([lo, pcm[whole * block:].min(axis=0)]), np.vstack([hi, pcm[whole * block:].max(axis=0)])
    return lo, hi


def extents(trace=False):
    """--extents: the waveform extremes (sh_pcm_extent_blocks) of main()'s two buffers at 1024-frame blocks.
    (a)  waveform(1024): of the Sample, and of the 12-plane stems buffer in one launch.
    (b)  the caller's way today: get_frames_numpy() of the same PCM (of each of the twelve stems), reshaped, min / max per block.  The
         PCM lies in device memory and nowhere else, so every pass downloads it: a fresh Sample over a view of the same bytes, which
         holds no host copy.  (b)'s table is held to (a)'s first.
    (c)  --extents --trace: each waveform and each level_history five times and nothing else, for rocprofv3 --kernel-trace --stats in a
         run of its own: k_pcm_extent_blocks next to k_pcm_level_blocks on the same buffers in the same session."""
    N.ensure_init(0)
    info = N.device_info()
    print("level_blocks_ab --extents: %s" % (info["name"] or info["arch"]), flush=True)
    fb = 2 * WIDTH
    frames = 120 * RATE
    pcm = np.random.default_rng(0).integers(-32768, 32768, size=2 * frames, dtype=np.int16)
    sample = Sample.from_raw_frames(pcm.tobytes(), WIDTH, RATE, 2).to_device()
    ntracks = len(S.TRACK_GAINS)
    what, nch, evs = S.meters_songs(4096)[0]
    bus = mixer.compile_tracks([evs[t::ntracks] for t in range(ntracks)], RATE, nch, WIDTH)
    glanes, mlane = S.bus_lanes(bus.frames)
    tpans, gpans = S.pan_lanes(ntracks)
    auto = bus.automation([None] * ntracks, master=mlane, groups=glanes, pans=tpans, group_pans=gpans)
    stems = bus.stems(automation=auto, gains=S.TRACK_GAINS, pans=S.DESK_PANS, master=S.DESK_MASTER, groups=S.GROUPS)
    nrows, plane = len(stems), stems._plane_frames
    a_sample = lambda: sample.waveform(BLOCK)                   # noqa: E731
    a_stems = lambda: stems.waveform(BLOCK)                     # noqa: E731
    if trace:
        for fn in (a_sample, lambda: sample.level_history(BLOCK), a_stems, lambda: stems.level_history(BLOCK)):
            for _ in range(5):
                fn()
        N.sync()
        return

    def fresh(buf, offset, nframes):
        """the same bytes as a Sample that holds no host copy"""
        s = Sample(samplerate=RATE, nchannels=2, samplewidth=WIDTH)
        s._set_device(buf.view(offset, nframes * fb), nframes * fb)
        return s
    b_sample = lambda: numpy_extents(fresh(sample._device(), 0, frames).get_frames_numpy(), BLOCK)      # noqa: E731
    b_stems = lambda: [numpy_extents(fresh(stems._buffer, r * plane * fb, bus.frames).get_frames_numpy(), BLOCK) for r in range(nrows)]      # noqa: E731
    w, (lo, hi) = a_sample(), b_sample()
    assert np.array_equal(w.lo[:, 0], lo) and np.array_equal(w.hi[:, 0], hi), "the Sample: numpy's table is not waveform's"
    ws, per_row = a_stems(), b_stems()
    for r, (lo, hi) in enumerate(per_row):
        assert np.array_equal(ws.lo[:, r], lo) and np.array_equal(ws.hi[:, r], hi), "stem %d: numpy's table is not waveform's" % r
    assert np.array_equal(w.peaks(), sample.level_history(BLOCK).peaks()) and np.array_equal(ws.peaks(), stems.level_history(BLOCK).peaks())
    print("(a) / (b)  a Sample of 120 s, 48 kHz, stereo, 16 bits: %d frames, %d blocks of %d frames; (b)'s table equals (a)'s" % (frames, len(w), BLOCK), flush=True)
    show("", frames * fb, by_turns({"(a) Sample.waveform(1024): one launch, the table copied back": a_sample,
                                    "(b) get_frames_numpy() of the same PCM, reshape, min / max per block": b_sample,
                                    "    Sample.level_history(1024), for scale": lambda: sample.level_history(BLOCK)}))
    print("(a) / (b)  the stems of the --stems song (%s): %d planes of %d frames, %d blocks of %d frames; (b)'s tables equal (a)'s"
          % (what, nrows, bus.frames, len(ws), BLOCK), flush=True)
    show("", nrows * bus.frames * fb, by_turns({"(a) SongStems.waveform(1024): one launch over %d planes" % nrows: a_stems,
                                               "(b) get_frames_numpy() of each of the %d stems, reshape, min / max" % nrows: b_stems,
                                               "    SongStems.level_history(1024), for scale": lambda: stems.level_history(BLOCK)}, warm=1))
    auto.close()
    bus.close()


if __name__ == "__main__":
    if "--extents" in sys.argv[1:]:
        extents("--trace" in sys.argv[1:])
    else:
        main("--trace" in sys.argv[1:])
