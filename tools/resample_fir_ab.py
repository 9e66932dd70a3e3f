#!/usr/bin/env python3
"""A band-limited rate conversion of a song in device memory: sh_pcm_resample_fir against the way a caller had.

    python tools/resample_fir_ab.py [--out FILE]                  rows (a), (b), (c); FILE (profiles/resample_fir_ab.txt) is written anew
    python tools/resample_fir_ab.py --quick LABEL [--out FILE]    (a) alone, appended to FILE under LABEL: row (e), for a diagnostic build
                                                                  named by SYNTHHIP_LIB (-DSH_FIRP_STAGE_F32) and for the shipped one
    python tools/resample_fir_ab.py --trace                       each (a) five times and nothing else, for
                                                                  rocprofv3 --kernel-trace --stats -f csv -- python ...   (no counters)
    python tools/resample_fir_ab.py --kernel CSV [--out FILE]     row (d): k_firp's time from that run's kernel_stats CSV, appended

Wall time with a device synchronise, medians of 15 after a warm-up, the variants by turns in one process.
(a)  one mixer.resample_fir_into of the 120-s stereo 16-bit Sample: 44.1 -> 48, 48 -> 44.1 and 44.1 -> 96 kHz with the default taps
     (mixer.lowpass_taps: 32 zero crossings of a Kaiser-windowed sinc), and 48 -> 8 kHz.
(b)  the caller's way today: get_frames_numpy() of the same PCM, numpy.convolve in int64 per phase and channel, the scale step,
     Sample.from_array, to_device.  Its bytes are held to (a)'s first.  It is run ONCE on a 5-second slice and SCALED to the whole length.
(c)  Sample.resample (audioop.ratecv's linear interpolation) of the same input: other bytes, context only -- what the better filter costs.
(d)  the kernel alone, from the --trace run under rocprofv3: USEFUL multiply-adds a second -- frames out x channels x taps / up, the rows'
     zero padding not counted -- and their share of the v_fma_f64 issue peak, 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3 T a second.
(e)  the shape: (a)'s calls with the diagnostic build and with the shipped one, by wall."""
import csv
import math
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from synthesizer_amd import _native as N  # noqa: E402
from synthesizer_amd import mixer  # noqa: E402
from synthesizer_amd.sample import Sample  # noqa: E402

WIDTH, SECONDS, SLICE_SECONDS = 2, 120, 5
ROWS = ((44100, 48000), (48000, 44100), (44100, 96000), (48000, 8000))
PEAK = 256 * 4 * 16 * 2.4e9


class Report:
    """lines to the terminal and to the profile"""

    def __init__(self, path, anew):
        self.file = open(path, "w" if anew else "a")

    def __call__(self, line):
        print(line, flush=True)
        self.file.write(line + "\n")
        self.file.flush()


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


def ratio(rate_in, rate_out):
    g = math.gcd(rate_in, rate_out)
    return rate_out // g, rate_in // g


def useful_macs(rate_in, rate_out, frames_in, nch=2):
    up, down = ratio(rate_in, rate_out)
    return float(-(-frames_in * up // down)) * nch * (2 * 16 * max(up, down) + 1) / up


def callers_way(buf, nframes, rate_in, rate_out):
    """(b): the device bytes through numpy and back to the device; the new Sample"""
    up, down = ratio(rate_in, rate_out)
    s = Sample(samplerate=rate_in, nchannels=2, samplewidth=WIDTH)
    s._set_device(buf.view(0, nframes * 2 * WIDTH), nframes * 2 * WIDTH)
    x = s.get_frames_numpy().astype(np.int64).reshape(-1, 2)
    h = mixer.lowpass_taps(up, down).astype(np.int64)
    delay, total = (len(h) - 1) // 2, -(-nframes * up // down)
    acc = np.zeros((total, 2), dtype=np.int64)
    for r in range(min(up, total)):
        p, b0 = (r * down + delay) % up, (r * down + delay) // up
        js = np.arange(r, total, up)
        b = b0 + down * np.arange(len(js), dtype=np.int64)
        for c in range(2):
            full = np.convolve(x[:, c], h[p::up])
            ok = b < len(full)
            acc[js[ok], c] = full[b[ok]]
    p = acc.astype(np.float64) * 2.0 ** -14
    p = np.where(p > 32767.0, 32767.0, np.where(p < -32767.0, -32768.0, p))
    return Sample.from_array(np.floor(p).astype(np.int16).reshape(-1), rate_out, 2).to_device()


def kernel_rows(path, say):
    """(d) from a rocprofv3 kernel_stats CSV: the rows whose name holds k_firp and not k_firp_rows"""
    work = 5 * sum(useful_macs(a, b, SECONDS * a) for a, b in ROWS)
    found = [row for row in csv.DictReader(open(path)) if "k_firp" in row.get("Name", "") and "k_firp_rows" not in row.get("Name", "")]
    calls, total_ns = sum(int(r["Calls"]) for r in found), sum(float(r["TotalDurationNs"]) for r in found)
    if calls != 5 * len(ROWS):
        say("(d)  %d dispatches of k_firp in %s, not the %d of --trace: no figure" % (calls, path, 5 * len(ROWS)))
        return
    rate = work / (total_ns * 1e-9)
    say("(d)  the kernel alone (rocprofv3 --kernel-trace --stats, a run of its own, no counters): %d dispatches of k_firp<short, 2>, %.3f ms in all"
        % (calls, total_ns / 1e6))
    say("     %.3e useful multiply-adds in all (real taps, not the rows' zero padding): %.2f T a second, %.1f %% of the v_fma_f64 issue peak of 39.3 T"
        % (work, rate / 1e12, 100.0 * rate / PEAK))


def main(argv):
    out = ROOT / "profiles" / "resample_fir_ab.txt"
    if "--out" in argv:
        out = Path(argv[argv.index("--out") + 1])
    mode = argv[0] if argv and argv[0] in ("--quick", "--trace", "--kernel") else ""
    if mode == "--kernel":
        kernel_rows(argv[1], Report(out, False))
        return
    N.ensure_init(0)
    info = N.device_info()
    rng = np.random.default_rng(0)
    samples, calls = {}, {}
    dst = N.DeviceBuffer(SECONDS * 96000 * 2 * WIDTH + 64)
    for rate_in, rate_out in ROWS:
        if rate_in not in samples:
            pcm = rng.integers(-32768, 32768, size=2 * SECONDS * rate_in, dtype=np.int16)
            samples[rate_in] = Sample.from_raw_frames(pcm.tobytes(), WIDTH, rate_in, 2).to_device()
        up, down = ratio(rate_in, rate_out)
        taps = Sample.from_raw_frames(mixer.lowpass_taps(up, down).tobytes(), 2, rate_out, 1).to_device()      # (designed and uploaded once, outside the clock)
        calls["(a) resample_fir_into, %d -> %d Hz (%d/%d, %d taps)" % (rate_in, rate_out, up, down, len(taps))] = (
            lambda s=samples[rate_in], r=rate_out, t=taps: mixer.resample_fir_into(dst, 0, s, r, t))
    if mode == "--trace":
        for fn in calls.values():
            for _ in range(5):
                fn()
        N.sync()
        return
    say = Report(out, mode == "")
    if mode == "--quick":
        named = os.environ.get("SYNTHHIP_LIB")
        say("(e)  %s%s" % (argv[1], " (the build named by SYNTHHIP_LIB)" if named else ""))
        for (name, (med, lo, hi)), (a, b) in zip(by_turns(calls).items(), ROWS):
            say("     %-64s median %9.3f ms  (min %.3f, max %.3f)" % (name, med, lo, hi))
        return
    say("resample_fir_ab: %s; %d outputs a lane, blocks of %d groups, chunks of %d steps" % (info["name"] or info["arch"], N.PCM_RESAMPLE_LANE_OUTPUTS,
                                                                                          N.PCM_RESAMPLE_BLOCK_GROUPS, N.PCM_RESAMPLE_STEP_CHUNK))
    say("(a)  a Sample of %d s, stereo, 16 bits; by wall, with a synchronise, medians of 15" % SECONDS)
    variants = dict(calls)
    for rate_in, rate_out in ROWS:
        variants["(c) Sample.resample, %d -> %d Hz" % (rate_in, rate_out)] = lambda s=samples[rate_in], r=rate_out: s.copy().resample(r)
    got = by_turns(variants)
    for (name, (med, lo, hi)), (a, b) in zip(list(got.items())[:len(ROWS)], ROWS):
        rate = useful_macs(a, b, SECONDS * a) / (med * 1e-3)
        say("  %-64s median %9.3f ms  (min %.3f, max %.3f)   %.2f T useful multiply-adds/s by wall" % (name, med, lo, hi, rate / 1e12))
    say("(b)  the caller's way today, once each: get_frames_numpy, numpy.convolve per phase and channel in int64, the scale step, from_array, to_device")
    lost = []
    for (name, (a_ms, _lo, _hi)), (rate_in, rate_out) in zip(list(got.items())[:len(ROWS)], ROWS):
        nframes = SLICE_SECONDS * rate_in
        N.sync()
        t0 = time.perf_counter()
        theirs = callers_way(samples[rate_in]._device(), nframes, rate_in, rate_out)
        N.sync()
        ms = (time.perf_counter() - t0) * 1e3
        piece = Sample(samplerate=rate_in, nchannels=2, samplewidth=WIDTH)
        piece._set_device(samples[rate_in]._device().view(0, nframes * 2 * WIDTH), nframes * 2 * WIDTH)
        ours = mixer.resample_fir(piece, rate_out)
        assert len(ours) == len(theirs) and bytes(ours.view_frame_data()) == bytes(theirs.view_frame_data()), "(b)'s bytes are not (a)'s: %s" % name
        whole = ms * SECONDS / SLICE_SECONDS
        say("  (b) %d -> %d Hz: %11.1f ms for a %d-second slice (its bytes equal (a)'s of the slice), SCALED to %d s: %.0f ms; (a) %.3f ms: %.0f times as fast"
            % (rate_in, rate_out, ms, SLICE_SECONDS, SECONDS, whole, a_ms, whole / a_ms))
        if not a_ms < whole:
            lost.append(name)
    say("     (a) beats (b) on every row" if not lost else "     (a) does NOT beat (b) on: %s" % ", ".join(lost))
    say("(c)  Sample.resample of the same input (a copy of it first; audioop.ratecv's linear interpolation: other bytes, context only)")
    for name, (med, lo, hi) in list(got.items())[len(ROWS):]:
        say("  %-64s median %9.3f ms  (min %.3f, max %.3f)" % (name, med, lo, hi))


if __name__ == "__main__":
    main(sys.argv[1:])
