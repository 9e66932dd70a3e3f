#!/usr/bin/env python3
"""A look-ahead peak limiter over a song in device memory: sh_pcm_limit against the way a caller had.

    python tools/limit_ab.py [--out FILE]                  rows (a) and (b); FILE (profiles/limit_ab.txt) is written anew
    python tools/limit_ab.py --trace                       each call of (a) five times and nothing else, for
                                                           rocprofv3 --kernel-trace --stats -f csv -- python ...   (no counters)
    python tools/limit_ab.py --kernel CSV [--out FILE]     row (c): the kernels' average times from that run's kernel_stats CSV, appended
    python tools/limit_ab.py --resources LOG [--out FILE]  the registers, LDS and waves per SIMD of the kernels, from the remarks of
                                                           hipcc -Rpass-analysis=kernel-resource-usage on csrc/pcm_limit.hip, appended

Wall time with a device synchronise, medians of 15 after a warm-up, the variants by turns in one process.
(a)  one mixer.limit_into of the 120-s, 48-kHz stereo 16-bit Sample at a ceiling of 16384, attack 240 and release 9600 frames: into a
     buffer of its own, in place, and with the gain plane (the C entry point with both destinations).
(b)  the caller's way today: get_frames_numpy() of the same PCM (a fresh Sample over the device bytes, which holds no host copy), the
     numpy prefix-minimum form of tests/limitref.py, Sample.from_array, to_device.  Its bytes are held to (a)'s first.
(c)  the kernels alone, from the --trace run under rocprofv3, as bytes moved against the 8 TB/s HBM peak: k_limit_tiles reads the
     PCM once, k_limit_apply reads it once more and writes it (and 4 bytes a frame of gains where the plane is asked for): three bytes
     moved per byte of PCM."""
import csv
import re
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from synthesizer_amd import _native as N  # noqa: E402
from synthesizer_amd import mixer  # noqa: E402
from synthesizer_amd.sample import Sample  # noqa: E402
from tests import limitref  # noqa: E402

RATE, WIDTH, SECONDS = 48000, 2, 120
FRAMES = SECONDS * RATE
CEILING, ATTACK, RELEASE = 16384, 240, 9600
PCM_BYTES = FRAMES * 2 * WIDTH
HBM_PEAK = 8e12
TRACE_CALLS = 5


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


def song(rng):
    """120 s of stereo noise at about -15 dBFS rms: some 0.6 % of its samples pass the ceiling of -6 dBFS"""
    return np.clip(np.rint(rng.normal(0.0, 6000.0, size=(FRAMES, 2))), -32768, 32767).astype(np.int16)


def callers_way(buf):
    """(b): the device bytes through numpy and back to the device; the new Sample"""
    s = Sample(samplerate=RATE, nchannels=2, samplewidth=WIDTH)
    s._set_device(buf.view(0, PCM_BYTES), PCM_BYTES)
    x = s.get_frames_numpy().astype(np.int64).reshape(-1, 2)
    y, _G = limitref.limit(x, CEILING, ATTACK, RELEASE)
    return Sample.from_array(y.astype(np.int16).reshape(-1), RATE, 2).to_device()


def kernel_rows(path, say):
    """(c) from a rocprofv3 kernel_stats CSV: the three kernels of the stereo 16-bit calls"""
    moved = {"k_limit_tiles": (PCM_BYTES, 2 * TRACE_CALLS, "reads the PCM"), "k_limit_apply<short, 2, false>": (2 * PCM_BYTES, TRACE_CALLS, "reads and writes the PCM"),
             "k_limit_apply<short, 2, true>": (2 * PCM_BYTES + 4 * FRAMES, TRACE_CALLS, "reads and writes the PCM, writes the gains")}
    rows = list(csv.DictReader(open(path)))
    say("(c)  the kernels alone (rocprofv3 --kernel-trace --stats, a run of its own, no counters), %d bytes of PCM:" % PCM_BYTES)
    total = 0.0
    for key, (nbytes, calls, what) in moved.items():
        hit = [r for r in rows if key.replace(" ", "") in r.get("Name", "").replace(" ", "")]
        if len(hit) != 1 or int(hit[0]["Calls"]) != calls:
            say("     %s: %d rows, %s dispatches, not the %d of --trace: no figure" % (key, len(hit), hit[0]["Calls"] if hit else "no", calls))
            continue
        avg = float(hit[0]["AverageNs"])
        total += avg if "true" not in key else 0.0
        say("     %-32s average %8.1f us (min %.1f, max %.1f): %s, %d bytes: %.2f TB/s, %.1f %% of the 8 TB/s HBM peak"
            % (key, avg / 1e3, float(hit[0]["MinNs"]) / 1e3, float(hit[0]["MaxNs"]) / 1e3, what, nbytes, nbytes / avg / 1e3, 100.0 * nbytes / (avg * 1e-9) / HBM_PEAK))
    if total:
        say("     one call without the plane, both kernels: %.1f us for 3 x %d bytes: %.2f TB/s, %.1f %% of the peak"
            % (total / 1e3, PCM_BYTES, 3 * PCM_BYTES / total / 1e3, 100.0 * 3 * PCM_BYTES / (total * 1e-9) / HBM_PEAK))


def resource_rows(path, say):
    """the kernels' registers, LDS and occupancy from hipcc's kernel-resource-usage remarks (mangled names: a = int8, s = int16, i = int32)"""
    say("     the kernels' resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950); no kernel has scratch or spills:")
    name, row, worst = None, {}, 0
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name, row = m.group(1), {}
            continue
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            row[m.group(1).split(" [")[0]] = int(m.group(2))
            if len(row) == 7:
                worst = max(worst, row["ScratchSize"] + row["SGPRs Spill"] + row["VGPRs Spill"])
                kind = re.search(r"k_limit_(tiles|apply)I([asi])Li([12])E(?:Lb([01]))?", name)
                say("       k_limit_%-5s %-5s %s%s  %3d VGPRs, %3d SGPRs, %3d bytes of LDS, %d waves per SIMD, scratch %d, spills %d"
                    % (kind.group(1), {"a": "int8", "s": "int16", "i": "int32"}[kind.group(2)], "mono  " if kind.group(3) == "1" else "stereo",
                       "" if kind.group(4) is None else (", gains" if kind.group(4) == "1" else "       "), row["VGPRs"], row["TotalSGPRs"], row["LDS Size"], row["Occupancy"],
                       row["ScratchSize"], row["SGPRs Spill"] + row["VGPRs Spill"]))
                name = None
    assert worst == 0, "a kernel of pcm_limit.hip has scratch or spills"


def main(argv):
    out = ROOT / "profiles" / "limit_ab.txt"
    if "--out" in argv:
        out = Path(argv[argv.index("--out") + 1])
    mode = argv[0] if argv and argv[0] in ("--trace", "--kernel", "--resources") else ""
    if mode == "--kernel":
        kernel_rows(argv[1], Report(out, False))
        return
    if mode == "--resources":
        resource_rows(argv[1], Report(out, False))
        return
    N.ensure_init(0)
    info = N.device_info()
    pcm = song(np.random.default_rng(0))
    sample = Sample.from_raw_frames(pcm.tobytes(), WIDTH, RATE, 2).to_device()
    src, L = sample._device(), N.lib()
    dst, plane, own = N.DeviceBuffer(PCM_BYTES), N.DeviceBuffer(4 * FRAMES), N.DeviceBuffer.from_array(pcm)

    def both():
        N.check(L.sh_pcm_limit(src.handle, 0, FRAMES, 2, WIDTH, CEILING, ATTACK, RELEASE, 0, FRAMES, dst.handle, 0, plane.handle, 0))

    def in_place():                                             # (after the first pass it limits what is limited already: the same traffic)
        N.check(L.sh_pcm_limit(own.handle, 0, FRAMES, 2, WIDTH, CEILING, ATTACK, RELEASE, 0, FRAMES, own.handle, 0, None, 0))
    calls = {"(a) limit_into, a buffer of its own": lambda: mixer.limit_into(dst, 0, sample, CEILING, ATTACK, RELEASE), "(a) in place": in_place,
             "(a) with the gain plane": both}
    if mode == "--trace":
        for name, fn in calls.items():
            if "in place" not in name:
                for _ in range(TRACE_CALLS):
                    fn()
        N.sync()
        return
    say = Report(out, True)
    say("limit_ab: %s, tiles of %d frames; a ceiling of %d, attack %d and release %d frames" % (info["name"] or info["arch"], N.PCM_LIMIT_TILE_FRAMES, CEILING, ATTACK, RELEASE))
    G = mixer.limit_gain(sample, CEILING, ATTACK, RELEASE)
    say("(a)  a Sample of %d s, %d Hz, stereo, 16 bits: %d frames, %d bytes; %.2f %% of its frames pass the ceiling, %.1f %% are at unity; by wall, with a synchronise, "
        "medians of 15" % (SECONDS, RATE, FRAMES, PCM_BYTES, 100.0 * float((np.abs(pcm.astype(np.int32)).max(axis=1) > CEILING).mean()), 100.0 * float((G == 1 << 30).mean())))
    got = by_turns(calls)
    for name, (med, lo, hi) in got.items():
        moved = 3 * PCM_BYTES + (4 * FRAMES if "plane" in name else 0)
        say("  %-40s median %8.3f ms  (min %.3f, max %.3f)   %.2f TB/s by wall" % (name, med, lo, hi, moved / (med * 1e-3) / 1e12))
    say("(b)  the caller's way today, once: get_frames_numpy, two prefix minima in int64 (tests/limitref.py), from_array, to_device")
    N.sync()
    t0 = time.perf_counter()
    theirs = callers_way(src)
    N.sync()
    ms = (time.perf_counter() - t0) * 1e3
    ours = mixer.limit(sample, CEILING, ATTACK, RELEASE)
    assert len(ours) == len(theirs) and bytes(ours.view_frame_data()) == bytes(theirs.view_frame_data()), "(b)'s bytes are not (a)'s"
    lost = []
    for name, (med, _lo, _hi) in got.items():
        say("  %-40s %10.1f ms; its bytes equal (a)'s; %s %.3f ms: %.0f times as fast" % ("(b) numpy", ms, name, med, ms / med))
        if not med < ms:
            lost.append(name)
    say("     (a) beats (b) on every row" if not lost else "     (a) does NOT beat (b) on: %s" % ", ".join(lost))


if __name__ == "__main__":
    main(sys.argv[1:])
