"""Host time per event of Sample.mix_at_many -- the checks and the table packing, which is where the call's time goes --
under a library that answers 0 to everything: no GPU, repeatable.  Four lists of 32 768 events over 120 s, 8 instruments of 20 000 frames,
16-bit: plain stereo events; a speed per event; mono events with speed, pan and envelope; stereo events with speed, envelope, loop, region,
alternating reverse and channels.  Seven runs per list, a fresh track per run, a fresh process per run and tree, this tree and
EVENT_HOST_TREE=<a checkout of the commit to compare with> taking turns.  Per list: median (min .. max) in microseconds per event for
both, and whether this tree's median lies within the other's own min-to-max spread above the other's median."""
import json
import os
import random
import statistics
import subprocess
import sys
import time
from pathlib import Path

HERE = str(Path(__file__).resolve().parent.parent)
NEVENTS, SPAN, RATE, RUNS = 32768, 120.0, 44100, 7
NAMES = ("plain", "speed", "speed + pan + envelope", "speed + envelope + loop + region + reverse + channels")


def one_run(tree):
    sys.path.insert(0, tree)
    from synthesizer_amd import _native as N
    from synthesizer_amd.sample import Sample

    class Buf:
        handle = None

        def __init__(self, nbytes=0):
            self.nbytes = nbytes
        from_bytes = classmethod(lambda cls, data: cls(len(data)))
        zero = lambda self, *_a: None
    lib = type("Lib", (), {"__getattr__": lambda self, name: lambda *_a: 0})()
    N.lib, N.DeviceBuffer = (lambda: lib), Buf
    rng = random.Random(7)
    mono = [Sample.from_raw_frames(bytes(2 * 20000), 2, RATE, 1) for _ in range(8)]
    stereo = [Sample.from_raw_frames(bytes(4 * 20000), 2, RATE, 2) for _ in range(8)]
    at = [rng.random() * SPAN for _ in range(NEVENTS)]
    speed = [2 ** (int(rng.random() * 25 - 12) / 12) for _ in range(NEVENTS)]
    env, loop, region = (0.01, 0.02, 0.6, 0.05), (0.05, 0.2, 0.5), (0.02, 0.4)
    lists = [[(t, stereo[k % 8]) for k, t in enumerate(at)],
             [(t, stereo[k % 8], None, None, speed[k]) for k, t in enumerate(at)],
             [(t, mono[k % 8], 0.5, None, speed[k], (k % 9 - 4) / 4, env) for k, t in enumerate(at)],
             [(t, stereo[k % 8], 0.5, None, speed[k], None, env, loop, region, k % 2, (0.75, 0.5)) for k, t in enumerate(at)]]
    out = []
    for events in lists:
        track = Sample(samplerate=RATE, nchannels=2, samplewidth=2)
        t0 = time.perf_counter()
        track.mix_at_many(events)
        out.append((time.perf_counter() - t0) / NEVENTS * 1e6)
    print(json.dumps(out))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--run":
        return one_run(sys.argv[2])
    trees = {"this tree": HERE}
    if os.environ.get("EVENT_HOST_TREE"):
        trees = {"other tree": os.environ["EVENT_HOST_TREE"], "this tree": HERE}
    times = {name: [] for name in trees}
    for _ in range(RUNS):
        for name, tree in trees.items():
            times[name].append(json.loads(subprocess.run([sys.executable, __file__, "--run", tree], check=True, capture_output=True, text=True).stdout))
    for k, what in enumerate(NAMES):
        print(what)
        for name in trees:
            runs = [r[k] for r in times[name]]
            print("  %-10s median %6.2f us/event  (min %6.2f .. max %6.2f)" % (name, statistics.median(runs), min(runs), max(runs)))
        if len(trees) == 2:
            other, this = [r[k] for r in times["other tree"]], [r[k] for r in times["this tree"]]
            bound = statistics.median(other) + max(other) - min(other)
            print("  this tree's median %.2f %s the bound %.2f (the other's median + its spread)" % (
                statistics.median(this), "is within" if statistics.median(this) <= bound else "EXCEEDS", bound))


if __name__ == "__main__":
    main()
