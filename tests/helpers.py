"""Shared helpers for the parity tests (oracle side)."""
import math

import numpy as np


def rms(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0.0
    return float(np.sqrt(np.mean((a - b) ** 2)))


def accumulated(t0, inc, start, n, chunk=1 << 22):
    """t_start .. t_{start+n-1} of the float64 running sum t += inc (sequential, exact):
    numpy's cumsum is a plain left-to-right loop."""
    t = float(t0)
    done = 0
    while done < start:
        m = min(chunk, start - done)
        a = np.full(m + 1, inc, dtype=np.float64)
        a[0] = t
        t = float(np.cumsum(a)[-1])
        done += m
    a = np.full(n, inc, dtype=np.float64)
    a[0] = t
    return np.cumsum(a)


def ulp32_diff(a, b):
    """distance in float32 ulps between two float32 arrays"""
    a = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


# ---- the C oracle over many voices, in parallel (a window late in the notes costs the oracle every sample before it) ----

def _oracle_window_worker(args):
    kind, n_total, seed, adsr, lo, hi, step, start, n = args
    from oracle import c_oracle as CO
    from oracle import synth_oracle as O
    from synthesizer_amd.workloads import additive_voices, fm_voices
    if kind == "additive":
        voices, gains = additive_voices(O, n_total, 48000, seed=seed, partials=16, adsr=adsr)
    else:
        voices, gains = fm_voices(O, n_total, 48000, seed=seed)
    idx = list(range(lo, hi, step))
    rows = np.stack([CO.render(voices[i], start + n)[start:] for i in idx])
    return CO.mix_bus(rows, [gains[i] for i in idx])


def oracle_bus_window(kind, n_total, seed, adsr, indices, start, n, max_procs=64):
    """float64 stereo bus [n, 2] of the voices `indices` (a range) of the workload (`kind`, n_total, seed, adsr) over the frames
    [start, start + n), by the C oracle run from frame 0, the voices dealt to up to max_procs processes (the partial buses of
    the processes are added in voice order: float64 summation order differs from one long sum by ~1e-16)."""
    import multiprocessing as mp
    import os
    idx = list(indices)
    lo, hi, step = idx[0], idx[-1] + 1, (idx[1] - idx[0]) if len(idx) > 1 else 1
    assert idx == list(range(lo, hi, step))
    nproc = max(1, min(os.cpu_count() or 1, max_procs, len(idx)))
    per = -(-len(idx) // nproc)
    jobs = []
    for p in range(nproc):
        part = idx[p * per:(p + 1) * per]
        if part:
            jobs.append((kind, n_total, seed, adsr, part[0], part[-1] + 1, step, start, n))
    if len(jobs) == 1:
        return _oracle_window_worker(jobs[0])
    with mp.get_context("spawn").Pool(len(jobs)) as pool:
        parts = pool.map(_oracle_window_worker, jobs, chunksize=1)
    bus = parts[0].copy()
    for p in parts[1:]:
        bus += p
    return bus


# ---- the int16 boundary guard at a chosen tolerance (tests/test_gpu_guard_contract.py, tests/test_host_logic.py) ----
# A bank's packed arrays with every polynomial / Clenshaw Harmonics voice's fast form moved away from its term-by-term list by a
# chosen amount, and the voice's declared tolerance raised to cover it: the contract of include/synthhip.h (ABI 6) then says that
# every int16 route still gives the LIST's integers.

def repeated_list(harmonics, copies):
    """[(k, a / copies) x copies for each (k, a)]: a longer list whose sum is the same series (each partial `copies` times in a row)."""
    return [(float(k), float(a) / copies) for k, a in harmonics for _ in range(copies)]


def adsr_over(mod, osc, sustain_level, attack=0.01, decay=0.05, sustain=1.0e6, release=0.2):
    """mod.EnvelopeFilter over osc with any sustain level: the classes take levels in [0, 1] (as upstream's does), the records and the C
    oracle any -- a level above 1 makes the envelope's largest gain, and with it the guard's reach, exceed the source's."""
    env = mod.EnvelopeFilter(osc, attack, decay, sustain, 1.0, release)
    env._sustain_level = sustain_level
    return env


def guard_gmax(voice):
    """The largest envelope gain of a packed voice (the factor pack_voices scales its guard by)."""
    env = voice["env"]
    return max(1.0, abs(float(env["sustain_level"]))) if int(env["enabled"]) else 1.0


def perturbed_voice_indices(voices):
    from synthesizer_amd import _native as N
    return [i for i in range(len(voices))
            if int(voices["kind"][i]) == N.SH_HARMONICS and int(voices["fm_mode"][i]) == N.SH_FM_NONE and int(voices["harm_dense"][i]) in (1, 2)]


def perturb_packed(packed, tq, scale, guard_list=None):
    """(voices, segs, coefs, partials) of pack_voices with the fast form of every polynomial / Clenshaw Harmonics voice moved by up to
    tq / |scale| (scale * the sample moves by up to tq integers): delta = tq / (|scale| |amplitude| gmax) added to the polynomial's
    constant term (coefs[harm_offset + 15], highest power first: the sample moves by sin(t) delta |amplitude| g) or to a_1 of the
    Clenshaw form (the last coefficient, k = K .. 1).  Each such voice gets a coefficient block of its own, so delta fits its amplitude;
    its guard_c is raised by |amplitude| gmax |delta| (1 + 2^-20).  guard_list: the guard list of every guarded voice replaced by this
    one (a list of the same sum, e.g. repeated_list), guard_t / guard_c recomputed for it.  tq = 0 and no guard_list: unchanged."""
    from fractions import Fraction
    from synthesizer_amd import oscillators as G
    voices, segs, coefs, partials = packed
    if tq == 0 and guard_list is None:
        return packed
    voices = voices.copy()
    coefs = [float(c) for c in coefs]
    partials = partials.copy()
    if guard_list is not None:
        from synthesizer_amd import _native as N
        g_off = len(partials)
        extra = np.zeros(len(guard_list), dtype=N.PARTIAL_DTYPE)
        for j, (k, a) in enumerate(guard_list):
            extra[j] = (float(k), float(a))
        partials = np.concatenate([partials, extra])
    for i in perturbed_voice_indices(voices):
        off, cnt, dense = int(voices["harm_offset"][i]), int(voices["harm_count"][i]), int(voices["harm_dense"][i])
        block = coefs[off:off + cnt]
        amp, gmax = abs(float(voices["amplitude"][i])), guard_gmax(voices[i])
        guarded = int(voices["guard_count"][i]) != 0
        if guard_list is not None and guarded:
            bounds = G.guard_bounds(guard_list, tuple(block) if dense == 2 else None, tuple(block) if dense == 1 else None)
            gt, gc = G.guard_tolerance(bounds, guard_list, float(voices["amplitude"][i]), float(voices["bias"][i]), gmax)
            voices["guard_offset"][i], voices["guard_count"][i] = g_off, len(guard_list)
            voices["guard_t"][i], voices["guard_c"][i] = gt, gc
        if tq == 0:
            continue
        voices["harm_offset"][i] = len(coefs)
        j = 15 if dense == 2 else cnt - 1
        old = block[j]
        block[j] = old + tq / (abs(scale) * amp * gmax)
        coefs.extend(block)
        moved = abs(float(Fraction(block[j]) - Fraction(old)))
        if guarded:
            voices["guard_c"][i] = float(voices["guard_c"][i]) + amp * gmax * moved * (1.0 + 2.0 ** -20)
            assert float(voices["guard_c"][i]) < 1.0
    return voices, segs, np.array(coefs, dtype=np.float64), partials


def fast_form_longdouble(coef_block, dense, t):
    """The fast form of a packed Harmonics voice at phases t, at unit amplitude, in long double: sin(t) P(cos t) (polynomial, highest
    power first) or sum_k a_k sin(k t) (Clenshaw coefficients, k = K .. 1) -- of the exact products k t."""
    t = np.asarray(t, dtype=np.longdouble)
    c = [np.longdouble(x) for x in coef_block]
    if dense == 2:
        ct = np.cos(t)
        p = np.zeros_like(t)
        for x in c:
            p = p * ct + x
        return np.sin(t) * p
    K = len(c)
    out = np.zeros_like(t)
    for j, a in enumerate(c):
        if a:
            out += a * np.sin(np.longdouble(K - j) * t)
    return out


def range_rule_maps(rows, n):
    """The chain map over int16 rows in voice order, as the library MAKES maps (the range rule, bytes of sh_chain_map):
    add = the exact sum, saturated at +-2^17 once; lo / hi = the sequential fold of clamp(bound + s, -32768, 32767) from
    (-32768, 32767) -- the chain applied to -32768 and to 32767.  `rows`: an iterable of n int16 values each."""
    from synthesizer_amd import chainmaps as CM
    add = np.zeros(n, dtype=np.int64)
    lo = np.full(n, -32768, dtype=np.int64)
    hi = np.full(n, 32767, dtype=np.int64)
    for r in rows:
        s = np.asarray(r, dtype=np.int16).astype(np.int64)
        add += s
        lo = np.clip(lo + s, -32768, 32767)
        hi = np.clip(hi + s, -32768, 32767)
    out = np.empty(n, dtype=CM.CHAIN_MAP_DTYPE)
    out["add"] = np.clip(add, -CM.ADD_MAX, CM.ADD_MAX)
    out["lo"] = lo
    out["hi"] = hi
    return out
