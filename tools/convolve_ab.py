#!/usr/bin/env python3
"""An impulse response over a song in device memory: sh_pcm_convolve against the way a caller had.

    python tools/convolve_ab.py [--out FILE]                  rows (a) and (b); FILE (profiles/convolve_ab.txt) is written anew
    python tools/convolve_ab.py --quick LABEL [--out FILE]    (a) alone, two lines per call appended to FILE under LABEL: row (d), for
                                                              a diagnostic build named by SYNTHHIP_LIB (-DSH_FIR_LANE_FRAMES=4,
                                                              -DSH_FIR_TAP_CHUNK=512 / 2048) and for the shipped one
    python tools/convolve_ab.py --trace                       each (a) five times and nothing else, for
                                                              rocprofv3 --kernel-trace --stats -f csv -- python ...   (no counters)
    python tools/convolve_ab.py --kernel CSV [--out FILE]     row (c): k_fir's average time from that run's kernel_stats CSV, appended
    python tools/convolve_ab.py --clock [--out FILE]          the 48 000-tap call in a loop under tools/clock_power.py's sampler, appended

Wall time with a device synchronise, medians of 15 after a warm-up, the variants by turns in one process.
(a)  one mixer.convolve_into of the 120-s, 48-kHz stereo 16-bit Sample: a mono response of 4 800 taps, one of 48 000, a stereo one of
     48 000.
(b)  the caller's way today: get_frames_numpy() of the same PCM (a fresh Sample over the device bytes, which holds no host copy),
     numpy.convolve per channel in int64, the scale step, Sample.from_array, to_device.  Its bytes are held to (a)'s first.  numpy's
     direct form runs about 2e9 multiply-adds a second on one core, so (b) is run ONCE, not fifteen times: the short response in
     full, the long ones on a 5-second slice, SCALED to the whole length.
(c)  the kernel alone, from the --trace run under rocprofv3: multiply-adds a second and the fraction of the v_fma_f64 issue peak, 256
     CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3 T lane-operations a second.  The three calls of (a) are one kernel, k_fir<short, 2>, so
     the CSV's row is their average: 15 dispatches, (frames + taps - 1) * taps * 2 multiply-adds each.
(d)  the shape: (a)'s three calls with each diagnostic build and with the shipped one, by wall."""
import csv
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

RATE, WIDTH, SECONDS, SLICE_SECONDS = 48000, 2, 120, 5
FRAMES = SECONDS * RATE
TAPS = (("a mono response of 4 800 taps", 4800, 1), ("a mono response of 48 000 taps", 48000, 1), ("a stereo response of 48 000 taps", 48000, 2))
PEAK = 256 * 4 * 16 * 2.4e9
FACTOR = 1.0 / (1 << 22)


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


def macs(taps, nch=2, frames=FRAMES):
    return float(frames + taps - 1) * taps * nch


def responses(rng):
    """the three responses of (a): decaying noise, full scale in front"""
    def one(taps, nch):
        env = np.exp(-6.0 * np.arange(taps) / taps)[:, None]
        v = np.rint(rng.uniform(-1.0, 1.0, size=(taps, nch)) * env * 32767.0).astype(np.int16)
        return Sample.from_raw_frames(v.tobytes(), WIDTH, RATE, nch).to_device()
    return [(what, one(taps, nch)) for what, taps, nch in TAPS]


def callers_way(buf, nframes, ir):
    """(b): the device bytes through numpy and back to the device; the new Sample"""
    s = Sample(samplerate=RATE, nchannels=2, samplewidth=WIDTH)
    s._set_device(buf.view(0, nframes * 2 * WIDTH), nframes * 2 * WIDTH)
    x = s.get_frames_numpy().astype(np.int64).reshape(-1, 2)
    h = ir.get_frames_numpy().astype(np.int64).reshape(-1, ir.nchannels)
    acc = np.stack([np.convolve(x[:, c], h[:, c if ir.nchannels == 2 else 0]) for c in range(2)], axis=1)
    p = acc.astype(np.float64) * FACTOR
    p = np.where(p > 32767.0, 32767.0, np.where(p < -32767.0, -32768.0, p))
    return Sample.from_array(np.floor(p).astype(np.int16).reshape(-1), RATE, 2).to_device()


def kernel_row(path, say):
    """(c) from a rocprofv3 kernel_stats CSV: the row whose name holds k_fir and not k_fir_taps"""
    for row in csv.DictReader(open(path)):
        name = row.get("Name", "")
        if "k_fir" in name and "k_fir_taps" not in name:
            calls, total_ns = int(row["Calls"]), float(row["TotalDurationNs"])
            work = 5 * sum(macs(taps, 2) for _w, taps, _n in TAPS)
            if calls != 15:
                say("(c)  %d dispatches of k_fir in %s, not the 15 of --trace: no figure" % (calls, path))
                return
            rate = work / (total_ns * 1e-9)
            say("(c)  the kernel alone (rocprofv3 --kernel-trace --stats, a run of its own, no counters): 15 dispatches of %s, %.3f ms in all "
                "(average %.3f ms, min %.3f, max %.3f)" % (name.replace("void (anonymous namespace)::", "").split("(")[0], total_ns / 1e6, float(row["AverageNs"]) / 1e6, float(row["MinNs"]) / 1e6, float(row["MaxNs"]) / 1e6))
            say("     %.3e multiply-adds in all: %.2f T multiply-adds a second, %.1f %% of the v_fma_f64 issue peak of 39.3 T lane-operations a second"
                % (work, rate / 1e12, 100.0 * rate / PEAK))
            return
    say("(c)  no k_fir row in %s" % path)


def main(argv):
    out = ROOT / "profiles" / "convolve_ab.txt"
    if "--out" in argv:
        out = Path(argv[argv.index("--out") + 1])
    mode = argv[0] if argv and argv[0] in ("--quick", "--trace", "--kernel", "--clock") else ""
    if mode == "--kernel":
        kernel_row(argv[1], Report(out, False))
        return
    N.ensure_init(0)
    info = N.device_info()
    named = os.environ.get("SYNTHHIP_LIB")
    rng = np.random.default_rng(0)
    pcm = rng.integers(-32768, 32768, size=2 * FRAMES, dtype=np.int16)
    sample = Sample.from_raw_frames(pcm.tobytes(), WIDTH, RATE, 2).to_device()
    irs = responses(rng)
    dst = N.DeviceBuffer((FRAMES + 48000) * 2 * WIDTH)
    calls = {"(a) convolve_into, %s" % what: (lambda ir=ir: mixer.convolve_into(dst, 0, sample, ir, FACTOR)) for what, ir in irs}
    if mode == "--trace":
        for fn in calls.values():
            for _ in range(5):
                fn()
        N.sync()
        return
    say = Report(out, mode == "")
    if mode == "--clock":
        sys.path.insert(0, str(ROOT / "tools"))
        import clock_power
        fn = list(calls.values())[1]
        fn()
        N.sync()
        sampler = clock_power.Sampler(period=0.05, pci=N.device_pci())
        sampler.start()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 3.0:
            for _ in range(10):
                fn()
            N.sync()
        sampler.stop_flag = True
        sampler.join()
        rows = [r for r in sampler.rows if r[0] - t0 > 0.5]
        say("     the clock: the 48 000-tap mono call in a loop for 3 s: sclk median %.0f MHz, package power median %.0f W (%d samples)"
            % (np.median([r[1] for r in rows]), np.median([r[2] for r in rows]), len(rows)))
        return
    if mode == "--quick":
        label = argv[1]
        got = by_turns(calls)
        say("(d)  %s%s" % (label, " (the build named by SYNTHHIP_LIB; the binding's tile and chunk are the shipped ones and do not describe it)" if named else ""))
        for (name, (med, lo, hi)), (what, taps, nch) in zip(got.items(), TAPS):
            say("     %-52s median %9.3f ms  (min %.3f, max %.3f)   %.2f T multiply-adds/s by wall" % (name, med, lo, hi, macs(taps) / (med * 1e-3) / 1e12))
        return
    say("convolve_ab: %s, tiles of %d frames, chunks of %d taps" % (info["name"] or info["arch"], N.PCM_FIR_TILE_FRAMES, N.PCM_FIR_TAP_CHUNK))
    say("(a)  a Sample of %d s, %d Hz, stereo, 16 bits: %d frames; by wall, with a synchronise, medians of 15" % (SECONDS, RATE, FRAMES))
    got = by_turns(calls)
    for (name, (med, lo, hi)), (what, taps, nch) in zip(got.items(), TAPS):
        rate = macs(taps) / (med * 1e-3)
        say("  %-52s median %9.3f ms  (min %.3f, max %.3f)   %.2f T multiply-adds/s by wall, %.1f %% of the issue peak" % (name, med, lo, hi, rate / 1e12, 100.0 * rate / PEAK))
    say("(b)  the caller's way today, once each: get_frames_numpy, numpy.convolve per channel in int64, the scale step, from_array, to_device")
    fb = 2 * WIDTH
    lost = []
    for k, (what, ir) in enumerate(irs):
        nframes = FRAMES if k == 0 else SLICE_SECONDS * RATE
        N.sync()
        t0 = time.perf_counter()
        theirs = callers_way(sample._device(), nframes, ir)
        N.sync()
        ms = (time.perf_counter() - t0) * 1e3
        piece = Sample(samplerate=RATE, nchannels=2, samplewidth=WIDTH)
        piece._set_device(sample._device().view(0, nframes * fb), nframes * fb)
        ours = mixer.convolve(piece, ir, FACTOR)
        assert len(ours) == len(theirs) and bytes(ours.view_frame_data()) == bytes(theirs.view_frame_data()), "(b)'s bytes are not (a)'s: %s" % what
        a_ms = got["(a) convolve_into, %s" % what][0]
        whole = ms * FRAMES / nframes
        if k == 0:
            say("  %-52s %11.1f ms in full; its bytes equal (a)'s; (a) %.3f ms: %.0f times as fast" % ("(b) " + what, ms, a_ms, ms / a_ms))
        else:
            say("  %-52s %11.1f ms for a %d-second slice (its bytes equal (a)'s of the slice), SCALED to %d s: %.0f ms; (a) %.3f ms: %.0f times as fast"
                % ("(b) " + what, ms, SLICE_SECONDS, SECONDS, whole, a_ms, whole / a_ms))
        if not a_ms < whole:
            lost.append(what)
    say("     (a) beats (b) on every row" if not lost else "     (a) does NOT beat (b) on: %s" % ", ".join(lost))


if __name__ == "__main__":
    main(sys.argv[1:])
