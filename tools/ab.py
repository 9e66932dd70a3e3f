#!/usr/bin/env python
"""A/B plumbing for kernel work (GPU box, from the repo root):

    python tools/ab.py build NAME [extra hipcc flags ...]   a VARIANT of libsynthhip.so beside the shipped one: synthesizer_amd/build/libsynthhip_NAME.so
                                                           (load it with SYNTHHIP_LIB=<that path>; e.g. -DSH_DIAG for tools/headline_phases.py)
    python tools/ab.py time LIB [LIB ...]                   the headline (us per block: median pass, best pass) under each library, two streams and one
    python tools/ab.py config CONFIG LIB [LIB ...]          bench.py --only-config CONFIG (config2 / config3 / staggered) under each library
    python tools/ab.py shapes [WFM[:groups] ...]            the headline under SYNTHHIP_VARIANT (and SYNTHHIP_GROUPS) settings of ONE library
    python tools/ab.py diff                                 how far the shape switches move a result: float64 bus of one block, headline and config 3
    python tools/ab.py mix LIB [LIB ...]                    sh_mix_bus_f32 on the benchmark's mix row (1024 x 480 000: k_mix_bus_direct, streaming loads) and on the
                                                           two-step render's (1024 x 48 000: k_mix_bus_f32 in 8 groups + k_bus_sum) under each library, the libraries
                                                           by turns, four processes each: ms per call, median of 7 timings per process
    python tools/ab.py pcm LIB [LIB ...]                    the benchmark's rows of the elementwise and statistics PCM entry points (900 MB int16, 1200 MB float) and
                                                           sh_pcm_stats at width 4 under each library, by turns, four processes each: ms per call, median of 7 loops
    python tools/ab.py mixcalls                             one call of each of those shapes and of a short direct one (for a kernel trace; SYNTHHIP_LIB picks the library)

(Round 5: build_variant.py, variant_diff.py, variants.py and the ab_*.sh wrappers in one file.)"""
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def build(argv):
    from synthesizer_amd import build as B
    name, extra = argv[0], argv[1:]
    out = B.HERE / "build" / ("libsynthhip_%s.so" % name)
    objdir = B.HERE / "build" / ("obj_" + name)
    objdir.mkdir(parents=True, exist_ok=True)
    defs = ['-DSH_SOURCE_HASH="%s"' % B.source_hash()] + extra
    jobs = []
    for src in B.SOURCES:
        obj = objdir / (src + ".o")
        jobs.append((src, obj, subprocess.Popen([B.HIPCC] + B.FLAGS + defs + ["-c", str(B.CSRC / src), "-o", str(obj)])))
    bad = [s for s, _o, p in jobs if p.wait() != 0]
    if bad:
        sys.exit("failed: " + " ".join(bad))
    subprocess.run([B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC"] + [str(o) for _s, o, _p in jobs] + ["-o", str(out), "-ldl"], check=True)
    import shutil
    shutil.rmtree(objdir, ignore_errors=True)
    print(out)


def _bench(args, env):
    p = subprocess.run([sys.executable, "bench.py"] + args, env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    try:
        return json.loads(p.stdout.strip().splitlines()[-1])
    except Exception:
        print("bench.py failed: %s %s" % (p.stdout[-300:], p.stderr[-300:]), flush=True)
        return None


def time_libs(argv):
    for lib in argv:
        for no_overlap in ("0", "1"):
            d = _bench(["--no-pcm-rows", "--no-two-step", "--no-configs", "--cpu-frames", "0", "--min-seconds", "0.6"],
                       {"SYNTHHIP_ALLOW_STALE": "1", "SYNTHHIP_LIB": lib, "SYNTHHIP_NO_OVERLAP": no_overlap})
            if d:
                print("%s no_overlap %s: %.2f %.2f us per block (median pass, best pass)" % (lib, no_overlap, d["ms_per_step"] * 1e3, d["passes"]["min_ms_per_step"] * 1e3), flush=True)


def config(argv):
    cfg, libs = argv[0], argv[1:]
    for lib in libs:
        d = _bench(["--only-config", cfg], {"SYNTHHIP_ALLOW_STALE": "1", "SYNTHHIP_LIB": lib})
        if d:
            for name, row in d["configs"].items():
                print("%s %s: %s" % (lib, name, {k: v for k, v in row.items() if isinstance(v, (int, float))}), flush=True)


def shapes(argv):
    for v in argv or ["4163", "484", "444", "844", "484:8", "484:16"]:
        var, _, groups = v.partition(":")
        env = {"SYNTHHIP_VARIANT": var}
        if groups:
            env["SYNTHHIP_GROUPS"] = groups
        d = _bench(["--steps", "40", "--warmup", "3", "--no-two-step", "--no-configs", "--no-pcm-rows", "--cpu-frames", "0", "--min-seconds", "0.5"], env)
        if d:
            print("variant %s: %.0f Msamples/s, %.4f ms/launch" % (v, d["value"], d["roofline"]["avg_launch_ms"]), flush=True)


_DIFF_CHILD = r'''
import sys; sys.path.insert(0, ".")
import numpy as np
from synthesizer_amd import _native as N
from synthesizer_amd import oscillators as G, workloads as W
from synthesizer_amd.mixer import VoiceBank
N.ensure_init(0)
out = {}
for name, (v, g) in (("add", W.additive_voices(G, 1024, 48000, seed=0, partials=16, adsr={"sustain": 1e9})), ("fm", W.fm_voices(G, 1024, 48000, seed=1))):
    bank = VoiceBank(v, gains=g)
    b = N.DeviceBuffer(48000 * 16)
    bank.render_device(48000, 100 * 48000, bus_f64=b)
    out[name] = b.download(np.float64, 96000)
np.savez(sys.argv[1], **out)
'''


def diff(argv):
    import numpy as np
    res = {}
    for name, env in (("default", {}), ("v484", {"SYNTHHIP_VARIANT": "484"}), ("v444", {"SYNTHHIP_VARIANT": "444"}), ("nosplit", {"SYNTHHIP_NO_SPLIT": "1"}),
                      ("g8", {"SYNTHHIP_GROUPS": "8"})):
        path = "/tmp/vd_%s.npz" % name
        subprocess.run([sys.executable, "-c", _DIFF_CHILD, path], env=dict(os.environ, **env), check=True)
        res[name] = np.load(path)
    for name in res:
        for k in ("add", "fm"):
            print(name, k, "max |diff| %.3e" % np.max(np.abs(res[name][k] - res["default"][k])), "scale %.3f" % np.max(np.abs(res["default"][k])))


_MIX_CHILD = r'''
import sys, time; sys.path.insert(0, ".")
import numpy as np
from synthesizer_amd import _native as N
N.ensure_init(0)
L = N.lib()
timed = sys.argv[1] == "time"
for nv, nf in ((1024, 480000), (1024, 48000)) + (() if timed else ((9, 393216),)):
    v = N.DeviceBuffer(nv * nf * 4); v.zero()
    g = N.DeviceBuffer.from_array(np.random.default_rng(0).uniform(0, 1, nv * 2).astype(np.float32))
    bus = N.DeviceBuffer(nf * 8)
    call = lambda: N.check(L.sh_mix_bus_f32(v.handle, nv, nf, nf, g.handle, bus.handle))
    call(); N.sync()
    if timed:
        reps = 20 if nf > 100000 else 200
        ms = []
        for _ in range(7):
            t = time.perf_counter()
            for _k in range(reps):
                call()
            N.sync()
            ms.append((time.perf_counter() - t) / reps * 1e3)
        print("%d x %d: %.4f ms (median of 7; min %.4f max %.4f)" % (nv, nf, sorted(ms)[3], min(ms), max(ms)), flush=True)
    for b in (v, g, bus):
        b.free()
'''


_PCM_CHILD = r'''
import sys, ctypes, statistics; sys.path.insert(0, ".")
import numpy as np
from synthesizer_amd import _native as N
N.ensure_init(0)
L = N.lib()
n, nq, nq64 = 900_000_000, 300_000_000, 150_000_000          # bench.py pcm_rows: the same calls on the same sizes
chunks, src, dst = N.DeviceBuffer(2 * n), N.DeviceBuffer(4 * nq), N.DeviceBuffer(2 * nq)
pcm = np.random.default_rng(1).integers(-3000, 3000, 1 << 24).astype(np.int16)
flt = np.random.default_rng(0).uniform(-1, 1, 1 << 24).astype(np.float32)
for buf, img in ((chunks, pcm), (src, flt)):
    for off in range(0, buf.nbytes, img.nbytes):
        buf.upload(img[:min(len(img), (buf.nbytes - off) // img.itemsize)], off)
mx, sq = (ctypes.c_uint32 * 2)(), (ctypes.c_double * 2)()
rows = (("pcm_stats_i16_900MB", lambda: L.sh_pcm_stats(chunks.handle, n, 2, mx, sq)),
        ("pcm_stats_stereo_i16_900MB", lambda: L.sh_pcm_stats_stereo(chunks.handle, n // 4, 2, mx, sq)),
        ("pcm_stats_i32_900MB", lambda: L.sh_pcm_stats(chunks.handle, n, 4, mx, sq)),
        ("pcm_mul_i16_900MB", lambda: L.sh_pcm_mul(chunks.handle, 0, n, 2, 0.7071, src.handle, 0)),
        ("pcm_tomono_i16_900MB", lambda: L.sh_pcm_tomono(chunks.handle, n // 4, 2, 0.5, 0.5, src.handle)),
        ("pcm_add_i16_900MB", lambda: L.sh_pcm_add(chunks.handle, 0, chunks.handle, n, n, 2, src.handle, 0)),
        ("quantize_f32_to_i16_1200MB", lambda: L.sh_quantize_f32(src.handle, 0, nq, 32767.0, 2, dst.handle, 0)),
        ("quantize_f64_to_i16_1200MB", lambda: L.sh_quantize_f64(src.handle, 0, nq64, 32767.0, 2, dst.handle, 0)))
for name, call in rows[:3] + rows[6:] + rows[3:6]:             # (the rows that overwrite src after the ones that read it)
    N.check(call()); N.sync()
    ms = []
    for _ in range(7):
        N.timer_start()
        for _k in range(5):
            N.check(call())
        ms.append(N.timer_stop() / 5)
    print("%s: %.4f ms (median of 7; min %.4f max %.4f)" % (name, statistics.median(ms), min(ms), max(ms)), flush=True)
'''


def _by_turns(child, argv):
    for rep in range(4):
        for lib in argv:
            p = subprocess.run([sys.executable, "-c", child, "time"], env=dict(os.environ, SYNTHHIP_ALLOW_STALE="1", SYNTHHIP_LIB=lib),
                               capture_output=True, text=True, timeout=300)
            if p.returncode:
                sys.exit("failed under %s (%d): %s" % (lib, p.returncode, p.stderr[-300:]))
            for line in p.stdout.splitlines():
                print("%s process %d: %s" % (Path(lib).name, rep, line), flush=True)


def mix(argv):
    _by_turns(_MIX_CHILD, argv)


def pcm(argv):
    _by_turns(_PCM_CHILD, argv)


def mixcalls(argv):
    sys.argv = ["mixcalls", "calls"]                       # in this process: a kernel trace follows it without following children
    exec(_MIX_CHILD, {"__name__": "__mixcalls__"})


COMMANDS = {"build": build, "time": time_libs, "config": config, "shapes": shapes, "diff": diff, "mix": mix, "pcm": pcm, "mixcalls": mixcalls}

if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] not in COMMANDS:
        sys.exit(__doc__)
    COMMANDS[sys.argv[1]](sys.argv[2:])
