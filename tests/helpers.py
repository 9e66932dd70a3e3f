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


# ---- the float64 scans (sh_scan_f64, sh_scan_rows_f64) against exact integers ---------------------------------------------
# Inputs live on a fixed-point grid: x_j = k_j * 2^-SCAN_GRID_BITS with integer k_j and sum |k_j| (carry included) < 2^62.  The
# exact prefix is then an int64, every float64 any order of additions can produce is a multiple of the grid step, and
# np.ldexp(got, SCAN_GRID_BITS) is that multiple without rounding: the error of every output is known exactly, in integers.
SCAN_GRID_BITS = 40
SCAN_TILE = 2048            # csrc/osc_scan.hip: values per workgroup (256 threads x 8)
SCAN_SUMS_ROUND = 256       # tile totals scanned per round of k_scan_sums / k_scan_rows_sums


def scan_grid(k):
    """Integers k -> the float64 values k * 2^-40 (asserted exact: every k must be a float64 itself)."""
    k = np.asarray(k, dtype=np.int64)
    f = k.astype(np.float64)
    assert np.all(np.abs(f) < 2.0 ** 62) and np.array_equal(f.astype(np.int64), k), "a grid integer that is not a float64"
    return np.ldexp(f, -SCAN_GRID_BITS)


def scan_to_grid(values):
    """float64 values -> their grid integers (int64), asserting that each is finite, on the grid and inside int64."""
    v = np.asarray(values, dtype=np.float64)
    g = np.ldexp(v, SCAN_GRID_BITS)
    assert np.all(np.isfinite(g)) and np.all(np.abs(g) < 2.0 ** 63), "not finite, or far outside the grid's range"
    assert np.all(g == np.rint(g)), "a value that no sum of grid values can be"
    return g.astype(np.int64)


def scan_exact(k, carry_k=0):
    """Exact exclusive prefix in grid integers: (prefix[i] = carry + sum_{j<i} k_j, total, A[i] = |carry| + sum_{j<i} |k_j|, A_total).
    Asserts that sum |k| stays below 2^62, so that int64 holds every partial sum."""
    k = np.asarray(k, dtype=np.int64)
    carry_k = int(carry_k)
    mag = np.abs(k)
    # (a float64 estimate of the sum, good to 1e-12, against a limit 1e-3 below 2^62: the int64 sums that follow cannot wrap)
    assert abs(carry_k) + float(np.sum(mag.astype(np.float64))) < 0.999 * 2.0 ** 62, "sum |k| reaches 2^62"
    incl = np.cumsum(k, dtype=np.int64)
    incl_a = np.cumsum(mag, dtype=np.int64)
    prefix = np.empty(k.size, dtype=np.int64)
    a = np.empty(k.size, dtype=np.int64)
    if k.size:
        prefix[0], a[0] = carry_k, abs(carry_k)
        prefix[1:] = incl[:-1] + carry_k
        a[1:] = incl_a[:-1] + abs(carry_k)
    total = carry_k + (int(incl[-1]) if k.size else 0)
    return prefix, total, a, abs(carry_k) + (int(incl_a[-1]) if k.size else 0)


def scan_error(got, prefix):
    """|got_i - exact_i| in grid steps, exactly (int64)."""
    return np.abs(scan_to_grid(got) - np.asarray(prefix, dtype=np.int64))


def scan_allowed(a, depth):
    """floor(depth * 2^-53 * A_i) in grid steps, exactly, for A_i < 2^62 and depth < 1024 (int64 throughout): the first-order bound of
    a sum whose every path from an input to the output holds at most `depth` rounded additions, |got - exact| <= depth u A with
    u = 2^-53.  (The second-order term depth^2 u^2 A is below 2^-30 of a grid step here, and the errors are whole grid steps.)"""
    a = np.asarray(a, dtype=np.int64)
    assert 0 < depth < 1024
    return depth * (a >> 53) + ((depth * (a & ((1 << 53) - 1))) >> 53)


def scan_rounds(n):
    """Rounds of the tile-sum loop for n values: ceil(ntiles / 256)."""
    ntiles = -(-int(n) // SCAN_TILE)
    return max(1, -(-ntiles // SCAN_SUMS_ROUND))


def scan_depth(n):
    """K of one call over n values: rounded additions on the longest path from an input to an output, counted from csrc/osc_scan.hip.
      7   the 8 values of a thread, summed in order (the first add, to 0.0, is exact)
      8   Hillis-Steele levels over the 256 thread sums: the tile's total
      8   Hillis-Steele levels over the round's tile totals: the round's total
      R-1 `carry = c + total` once per round, from the input's round to the one before the output's (R = scan_rounds(n))
      1   sums[i] = c + ex: the tile's base
      1   the thread's exclusive value + the tile's base (k_scan_apply)
      7   the running adds over the thread's own 8 values
    = 31 + R.  Shorter paths: a tile of the output's own round 32, the output's own tile 23, carry_in R + 8."""
    return 31 + scan_rounds(n)


def scan_carry_depth(n):
    """The same count for carry_out of one call: 7 + 8 + 8, then at most R carry adds: 23 + R (carry_in itself: R)."""
    return 23 + scan_rounds(n)


def scan_chain_depth(piece_lengths):
    """K for the outputs of the LAST of several calls chained by their carries (each carry_out fed to the next call as carry_in): an
    input of piece q reaches piece q's carry_out in scan_carry_depth(n_q) additions, passes every piece between in scan_rounds(n_m)
    more, and reaches an output of the last piece through its carry path, scan_rounds(n_p) + 8; an input of the last piece itself
    has scan_depth(n_p).  The longest of these."""
    lens = [int(x) for x in piece_lengths if int(x) > 0]
    if not lens:
        return 1
    last = lens[-1]
    best = scan_depth(last)
    through = 0
    for n_q in reversed(lens[:-1]):
        best = max(best, scan_carry_depth(n_q) + through + scan_rounds(last) + 8)
        through += scan_rounds(n_q)
    return best


SCAN_INPUT_KINDS = ("uniform", "modulator", "small_on_large_carry", "log_uniform")


def scan_inputs(kind, n, rng):
    """-> (k, carry_k): grid integers of one of the rounded-class inputs, n values, sum |k| + |carry| < 2^62."""
    one = 1 << SCAN_GRID_BITS
    if kind == "uniform":                       # uniform in (-1, 1)
        return rng.integers(-one + 1, one, n, dtype=np.int64), int(rng.integers(-one, one))
    if kind == "modulator":                     # all positive: 0.3 + 0.2 sin, 5 Hz at 48 kHz
        t = np.arange(n, dtype=np.float64)
        return np.rint((0.3 + 0.2 * np.sin(2.0 * math.pi * 5.0 / 48000.0 * t + 0.7)) * one).astype(np.int64), int(0.25 * one)
    if kind == "small_on_large_carry":          # values around 1e-6 on a carry of about 1e6
        return rng.integers(-2 * int(1e-6 * one), 2 * int(1e-6 * one) + 1, n, dtype=np.int64), (int(1.0e6 * one) >> 8 << 8) + 12345 * 256       # (a float64: ulp 2^8 grid steps up there)
    if kind == "log_uniform":                   # magnitudes log-uniform over the grid's whole range, random signs
        # the mean of such a draw is 2^top / (top ln 2): top = 65 - log2 n keeps the sum near 2^60 (scan_exact checks it); the carry
        # is below 2^60.  Partial sums beyond 2^53 grid steps are where additions round: from a few thousand values on this input
        # is exact, and the bound asks for equality by itself.
        top = min(59.0, 65.0 - math.log2(max(n, 1)))
        mag = np.floor(np.exp2(rng.uniform(0.0, top, n))).astype(np.int64)      # (float64 first: every magnitude is a float64)
        return mag * rng.choice(np.array([-1, 1], dtype=np.int64), n), -int(np.floor(2.0 ** rng.uniform(0.0, 60.0)))
    raise ValueError(kind)


def scan_adversarial(n, tile, thread, pos, big_log2, rng, negative=False):
    """A run of small values (|k| < 2^20) with ONE value of 2^big_log2 grid steps (big_log2 >= 53: beyond the 53 bits of the prefix in
    front of it) at position `pos` of the 8-value group of thread `thread` in tile `tile`.  Every output in front of the large value
    has a prefix of small values only, and the bound over j < i gives it no room for the large one.  The values of the tile in front
    of that group sum to an odd number of grid steps, so a sum that rounds them against the large value cannot come out exact by luck."""
    assert 53 <= big_log2 <= 60 and 0 <= pos < 8 and 0 < thread < 256
    k = rng.integers(1, 1 << 20, n, dtype=np.int64) * rng.choice(np.array([-1, 1, 1], dtype=np.int64), n)
    at = tile * SCAN_TILE + thread * 8 + pos
    assert at < n
    k[at] = -(1 << big_log2) if negative else 1 << big_log2
    group = at - pos
    if int(k[tile * SCAN_TILE:group].sum()) % 2 == 0:
        k[group - 1] += 1
    return k, int(rng.integers(1, 1 << 20)), at


# ---- the PCM entry points through windows of larger buffers (tests/test_gpu_pcm_views.py) -----------------------------------
# Every operand lives in a DeviceBuffer.view of a parent that is filled with a sentinel byte and keeps PCM_GUARD bytes free on both
# sides of the window; the window starts `a` bytes after a 16-byte boundary of the parent, so `a` mod 16 is the residue of the device
# pointer the kernels see.
PCM_GUARD = 64
PCM_IN_SENTINEL = 0xA5
PCM_OUT_SENTINEL = 0x5A


def pcm_view_call(N, inputs, out_nbytes, a_out, call, out_view_nbytes=None, untouched=False, guards=None):
    """Run `call(in_views, out_view) -> rc` on windows of sentinel-filled parents and return (rc, the out_nbytes result bytes).

    inputs: a list of (data, a) or (data, a, view_nbytes): `data` (bytes) is uploaded at byte PCM_GUARD + a of its parent and the
    window covers it (or only its first view_nbytes bytes: a window shorter than the request, inside a parent that holds all of it).
    out_nbytes / a_out: the same for the destination (None: the call has none, out_view is None); out_view_nbytes: a shorter window,
    or a longer one whose bytes behind out_nbytes must keep their sentinel.
    Asserted after the call: every window's device pointer has the residue its case intended, mod 16; every input parent is
    unchanged; the destination parent still holds its sentinel outside the window -- everywhere with untouched=True (a refusal).
    guards: per input None or (before, after), bytes written over the sentinel immediately in front of and behind `data` (at most
    PCM_GUARD each): what a kernel that reads outside its range would see."""
    import ctypes as C
    L = N.lib()
    parents, views, images = [], [], []
    for k, item in enumerate(inputs):
        data, a = bytes(item[0]), int(item[1])
        vbytes = len(data) if len(item) < 3 or item[2] is None else int(item[2])
        img = np.full(PCM_GUARD + a + max(len(data), vbytes) + PCM_GUARD, PCM_IN_SENTINEL, dtype=np.uint8)
        img[PCM_GUARD + a:PCM_GUARD + a + len(data)] = np.frombuffer(data, dtype=np.uint8)
        if guards is not None and guards[k] is not None:
            before, after = bytes(guards[k][0]), bytes(guards[k][1])
            assert len(before) <= PCM_GUARD and len(after) <= PCM_GUARD
            img[PCM_GUARD + a - len(before):PCM_GUARD + a] = np.frombuffer(before, dtype=np.uint8)
            img[PCM_GUARD + a + len(data):PCM_GUARD + a + len(data) + len(after)] = np.frombuffer(after, dtype=np.uint8)
        parent = N.DeviceBuffer.from_array(img)
        view = parent.view(PCM_GUARD + a, vbytes)
        assert (C.cast(L.sh_buf_devptr(view.handle), C.c_void_p).value or 0) % 16 == a % 16, "input window not at the intended residue"
        parents.append(parent)
        views.append(view)
        images.append(img)
    out_parent = out_view = out_img = None
    if out_nbytes is not None:
        vbytes = out_nbytes if out_view_nbytes is None else int(out_view_nbytes)
        out_img = np.full(PCM_GUARD + a_out + max(out_nbytes, vbytes) + PCM_GUARD, PCM_OUT_SENTINEL, dtype=np.uint8)
        out_parent = N.DeviceBuffer.from_array(out_img)
        out_view = out_parent.view(PCM_GUARD + a_out, vbytes)
        assert (C.cast(L.sh_buf_devptr(out_view.handle), C.c_void_p).value or 0) % 16 == a_out % 16, "output window not at the intended residue"
    try:
        rc = call(views, out_view)
        N.sync()
        for parent, img in zip(parents, images):
            assert parent.download(np.uint8, img.size).tobytes() == img.tobytes(), "an input parent was written to"
        result = None
        if out_parent is not None:
            got = out_parent.download(np.uint8, out_img.size)
            # (a window longer than the result: its surplus behind out_nbytes is guard as well)
            lo, hi = PCM_GUARD + a_out, PCM_GUARD + a_out + (0 if untouched else min(out_view.nbytes, out_nbytes))
            stray = np.flatnonzero(np.concatenate([got[:lo], got[hi:]]) != PCM_OUT_SENTINEL)
            assert stray.size == 0, "destination parent written outside the window: byte %d relative to the window's start, %d bytes in all" % (
                int(stray[0]) - lo if stray[0] < lo else int(stray[0]) - lo + (hi - lo), stray.size)
            result = got[lo:lo + out_nbytes].tobytes()
        return rc, result
    finally:
        for v in views + ([out_view] if out_view is not None else []):
            v.free()
        for p in parents + ([out_parent] if out_parent is not None else []):
            p.free()


def pcm_track_call(N, sources, base, a, call, surplus=0, untouched=False):
    """The in-place form (the placed-sample mixer): `base` (bytes) is uploaded at byte PCM_GUARD + a of a parent filled with
    PCM_OUT_SENTINEL, the window covers it and `surplus` bytes behind it; `sources` (bytes each) are fresh buffers.  Runs
    `call(source_buffers, window, parent) -> rc` and returns (rc, the len(base) bytes of the track).  Asserted after the call: the
    window's pointer has residue a mod 16; the parent still holds its sentinel in front of the window, in the window's surplus and
    behind it; every source is unchanged; with untouched=True (a refusal) the track's bytes are still `base`."""
    import ctypes as C
    L = N.lib()
    base = bytes(base)
    img = np.full(PCM_GUARD + a + len(base) + surplus + PCM_GUARD, PCM_OUT_SENTINEL, dtype=np.uint8)
    lo, hi = PCM_GUARD + a, PCM_GUARD + a + len(base)
    img[lo:hi] = np.frombuffer(base, dtype=np.uint8)
    parent = N.DeviceBuffer.from_array(img)
    window = parent.view(lo, len(base) + surplus)
    bufs = [N.DeviceBuffer.from_bytes(bytes(b)) for b in sources]
    try:
        assert (C.cast(L.sh_buf_devptr(window.handle), C.c_void_p).value or 0) % 16 == a % 16, "track window not at the intended residue"
        rc = call(bufs, window, parent)
        N.sync()
        for k, (buf, b) in enumerate(zip(bufs, sources)):
            assert buf.download_bytes(len(b)) == bytes(b), "source %d was written to" % k
        got = parent.download(np.uint8, img.size)
        stray = np.flatnonzero(np.concatenate([got[:lo], got[hi:]]) != PCM_OUT_SENTINEL)
        assert stray.size == 0, "track parent written outside track_samples: byte %d relative to the window's start, %d bytes in all" % (
            int(stray[0]) - lo if stray[0] < lo else int(stray[0]) - lo + (hi - lo), stray.size)
        result = got[lo:hi].tobytes()
        if untouched:
            assert result == base, "a refused call wrote into the track"
        return rc, result
    finally:
        window.free()
        parent.free()
        for b in bufs:
            b.free()
