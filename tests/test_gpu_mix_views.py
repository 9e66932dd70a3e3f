"""The placed-sample mixer (csrc/sequence.hip) and the saturating chain (csrc/pcm.hip) through windows of larger buffers.

Both families choose their kernel path from the ADDRESS they are handed -- seq_launch's `aligned`, the chain's direct loops against
its split kernels, RowSrc's vector load, the gather's `whole` per batch of four sources, the vector store of split_store -- and every
other test hands them fresh 16-byte-aligned allocations of exactly the right size.  Here the track, the chunk rows, the pan factors,
the gather's sources and the outputs are DeviceBuffer.view windows at chosen residues mod 16 inside sentinel-filled parents
(tests/helpers.py: pcm_view_call, pcm_track_call), which assert the pointer's residue, untouched inputs and untouched bytes around
every window.

References, none of them the library: tests/seqref.py (mix) over the lists of tests/seqcases.py (lists) and the shaped lists below for
the track; the loop of live audioop.add / audioop.tostereo for the chain
(tests/test_gpu_realtime_mixer.py: _audioop_fold).  Every comparison is byte equality.  tests/test_mix_view_refs.py checks the case
tables below without a GPU.
"""
import audioop
import ctypes as C
import functools

import numpy as np
import pytest

from tests.helpers import PCM_GUARD, PCM_OUT_SENTINEL, pcm_track_call, pcm_view_call
from tests.seqcases import RATE, as_samples, call_level, in_a_child_under_the_other_alignment_scheme, lists, named, rows_of, sample_of, with_samples
from tests.seqref import mix, out_frames, pcm, source
from tests.test_gpu_pcm_views import _check, residues
from tests.test_gpu_realtime_mixer import _audioop_fold, _rand_pcm

pytestmark = pytest.mark.gpu

SURPLUS = 16                                               # samples of window behind track_samples


# ---- 1: the track as a window -----------------------------------------------------------------------------------------------------
LEVELS = {"A": ["plain", "rate", "pan", "env"], "B": ["rate", "pan", "env"], "C": ["pan", "env"]}


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_track_windows_plain_rate_pan_env(gpu, width):
    """the lists of tests/seqcases.py into a track window at every residue, track_samples the window and 16 samples
    short of it: audioop's bytes, the same at every residue, nothing written around the track"""
    N = gpu
    sources, base, A, B, C_, want_a, want_b, want_c = lists(width)
    ns = len(base) // width
    for name, lst, want in (("A", A, want_a), ("B", B, want_b), ("C", C_, want_c)):
        rows = rows_of(lst, sources, width)
        for level in LEVELS[name]:
            if level == "env" and width == 3:               # an envelope's fades have no 24-bit form
                continue
            for a in residues(width):
                for surplus in (0, SURPLUS * width):
                    rc, got = pcm_track_call(N, sources, base, a, lambda bufs, win, par: call_level(N, level, rows, bufs, width, win, ns), surplus=surplus)
                    _check(rc, got, want, (name, level, width, a, surplus))


# the shaped lists of LOOP and REV: (instrument, volume, other_seconds, speed, pan, envelope?, loop as (S, L, V frames) | None,
# region as (first, frames | None) | None, reverse, where), instruments 0 - 2 mono (300, 211, 97 frames), 3 and 4 stereo (300, 211);
# where: a track frame, or "end" (the event ends on the last track sample)
HELD = [300, 211, 97]
SHAPED = {
    "loop": [
        (0, None, None, 0.37, 0.3, False, (5, 65, 420), None, False, 100),                   # looped and resampled, over the first tile edge (16 bits)
        (3, 0.5, None, None, None, False, (1, 8, 600), None, False, 500),                   # stereo, over the first tile edge of the other widths
        (1, 1.7, None, 1.7, (1.0, 0.0), True, None, None, False, 30),                       # an envelope (widths 1, 2, 4) on a resampled note
        (2, None, None, 2.5, -0.65, True, (0, 9, 700), None, False, 900),                   # looped, resampled and shaped
        (4, -1.0, None, None, None, False, (0, 1, 1), None, False, 77),                     # one frame: shorter than a lane
        (4, 0.8, None, None, None, False, (12, 7, 333), None, False, "end"),                # up to the last track sample
    ],
    "rev": [
        (0, None, None, 0.37, 0.3, False, (5, 65, 420), None, False, 100),                   # looped and resampled, forwards
        (3, 0.5, None, None, None, False, None, (5, 115), True, 500),                       # reversed from a region, stereo
        (1, 1.7, None, 1.7, (1.0, 0.0), True, None, (40, None), True, 30),                  # reversed to the sample's end, resampled, an envelope
        (2, None, None, 2.5, -0.65, True, (0, 9, 700), (3, 60), True, 900),                 # region, reversed, looped, resampled, shaped
        (4, -1.0, None, None, None, False, None, (7, 1), True, 77),                         # one frame: shorter than a lane
        (4, 0.8, (0.37 * 150 + 1) / RATE, None, None, False, None, (12, 150), True, "end"),        # cut by other_seconds, up to the last track sample
    ],
}


@functools.lru_cache(maxsize=None)
def shaped(kind, width):
    """-> (instruments as (bytes, channels), base, events of ten fields in the ladder's order (8-tuples for "loop"), audioop's
    bytes, [(first track sample, samples) per event]).  Made once, never changed."""
    rng = np.random.default_rng(900 + 10 * width + (kind == "rev"))
    sources, base = lists(width)[:2]
    track_frames = len(base) // (2 * width)
    instruments = [(pcm(rng, width, n, 0.6), 1) for n in HELD] + [(pcm(rng, width, 2 * n, 0.6), 2) for n in HELD[:2]]
    events, spans = [], []
    for i, volume, other_seconds, speed, pan, shaped_, loop, region, reverse, where in SHAPED[kind]:
        data, snch = instruments[i]
        assert (pan is not None) == (snch == 1)
        frames = len(data) // (width * snch)
        reg = None if region is None else (region[0] / RATE, None if region[1] is None else (region[0] + region[1]) / RATE)
        R = frames if region is None else (frames - region[0] if region[1] is None else region[1])
        lp = None if loop is None else (loop[0] / RATE, (loop[0] + loop[1]) / RATE, loop[2] / RATE)
        inrate = RATE if speed is None else int(RATE * speed)
        out = out_frames(R if loop is None else loop[2], inrate, RATE)
        env = None
        if shaped_ and width != 3:
            dur = (0.61 * out + 0.37) / RATE
            env = (0.113 * dur, 0.171 * dur, 0.5, 0.233 * dur, dur)
        played = source(data, width, RATE, 2, volume=volume, other_seconds=other_seconds, speed=speed, pan=pan, env=env, loop=lp, region=reg, reverse=reverse)
        out = len(played) // (2 * width)
        frame = track_frames - out if where == "end" else where
        assert 0 <= frame and frame + out <= track_frames
        events.append((frame / RATE, i, volume, other_seconds, speed, pan, env, lp, reg, reverse))
        spans.append((2 * frame, 2 * out))
    want = mix(base, named(instruments, events), width, RATE, 2)
    if kind == "loop":
        assert all(e[8] is None and not e[9] for e in events)
        events = [e[:8] for e in events]
    assert len(want) == len(base) and want != base
    return instruments, base, events, want, spans


def _recorded_call(N, monkeypatch, kind, width):
    """Sample.mix_at_many of the shaped list with the library watched: -> (the entry point's name, its arguments with the tables
    copied, the samples that own the source buffers).  The arguments are what a caller of the C entry point would write by hand."""
    instruments, base, events, want, _spans = shaped(kind, width)
    calls = []
    real = N.lib()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith("sh_mix_events"):
                return fn

            def watched(*args):
                srcs, nsrc, tab, ntab, seg, nseg, w, nch, _track, ns = args
                dt = N.MIX_EVENT_REV_DTYPE if name == "sh_mix_events_rev" else N.MIX_EVENT_LOOP_DTYPE
                table = np.frombuffer(C.string_at(tab, ntab * dt.itemsize), dtype=dt).copy()
                segs = np.frombuffer(C.string_at(seg, nseg * N.ENV_SEGMENT_DTYPE.itemsize), dtype=N.ENV_SEGMENT_DTYPE).copy() if nseg else None
                calls.append((name, (srcs, nsrc, table, segs, w, nch, ns)))
                return fn(*args)
            return watched
    samples = as_samples(instruments, width, RATE)
    with monkeypatch.context() as m:
        m.setattr(N, "lib", lambda: Spy())
        got = sample_of(base, width, RATE, 2).mix_at_many(with_samples(samples, events))
    assert [c[0] for c in calls] == ["sh_mix_events_" + kind], calls
    assert bytes(got.view_frame_data()) == want               # (a fresh aligned track: what the other tests already cover)
    return calls[0][0], calls[0][1], samples


@pytest.mark.parametrize("kind", ["loop", "rev"])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_track_windows_loop_rev(gpu, monkeypatch, width, kind):
    """a short list with loops, regions, reversal, speeds, pans and (widths 1, 2, 4) envelopes into a track window at every residue"""
    N = gpu
    instruments, base, events, want, _spans = shaped(kind, width)
    name, (srcs, nsrc, table, segs, w, nch, ns), samples = _recorded_call(N, monkeypatch, kind, width)
    assert (w, nch, ns) == (width, 2, len(base) // width) and (segs is not None) == (width != 3)
    entry = getattr(N.lib(), name)

    def call(_bufs, win, _par):
        return entry(srcs, nsrc, table.ctypes.data, len(table), segs.ctypes.data if segs is not None else None,
                     len(segs) if segs is not None else 0, w, nch, win.handle, ns)
    for a in residues(width):
        for surplus in (0, SURPLUS * width):
            rc, got = pcm_track_call(N, [], base, a, call, surplus=surplus)
            _check(rc, got, want, (kind, width, a, surplus))
    for (b, c), smp in zip(instruments, samples):
        assert bytes(smp.view_frame_data()) == b and smp.nchannels == c                 # the instruments are untouched


def test_track_windows_under_the_other_alignment_scheme(gpu):
    """SYNTHHIP_SEQ_ALIGN is read once per process (sh_init): the 16-bit cases again in a child under the scheme that is not the default"""
    in_a_child_under_the_other_alignment_scheme(__file__, ["test_track_windows_plain_rate_pan_env[2]", "test_track_windows_loop_rev[2-loop]",
                                                           "test_track_windows_loop_rev[2-rev]"])


# ---- 2: refusals are checked against the window and track_samples -------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_track_refusals_against_the_window(gpu, width):
    """The track of a call is its first track_samples samples (include/synthhip.h: no source may be, or overlap, the track): a source
    in the same parent in front of the window, or in the window's surplus BEHIND track_samples, is legal and is mixed in; one sample
    into [0, track_samples) from either side is refused.  track_samples beyond the window and an event beyond track_samples (in a
    window that has room) are refused.  A refusal writes nothing."""
    N = gpu
    lib = N.lib()
    rng = np.random.default_rng(width)
    ns = 200
    base = pcm(rng, width, ns, 0.4)
    src = pcm(rng, width, 8, 0.4)

    def plain(events, track_samples, extra=()):
        def call(bufs, win, par):
            views = [par.view(off, nbytes) for off, nbytes in extra]
            try:
                arr = (C.c_void_p * (len(bufs) + len(views)))(*[b.handle for b in list(bufs) + views])
                t = np.array(events, dtype=N.MIX_EVENT_DTYPE)
                return lib.sh_mix_events(arr, len(arr), t.ctypes.data, len(t), width, win.handle, track_samples)
            finally:
                for v in views:
                    v.free()
        return call
    for a in residues(width):
        lo = PCM_GUARD + a
        # a source inside the track's parent, in front of the window: legal (it holds the sentinel: 8 samples of it are mixed in)
        sentinel = bytes([PCM_OUT_SENTINEL]) * (8 * width)
        want = bytearray(base)
        want[10 * width:18 * width] = audioop.add(bytes(want[10 * width:18 * width]), sentinel, width)
        want[192 * width:] = audioop.add(bytes(want[192 * width:]), src, width)
        events = [(10, 0, 8, 1.0, 1, 0), (192, 0, 8, 1.0, 0, 0)]                        # the second: up to the last track sample
        rc, got = pcm_track_call(N, [src], base, a, plain(events, ns, extra=[(lo - 8 * width, 8 * width)]), surplus=SURPLUS * width)
        _check(rc, got, bytes(want), ("a source in front of the window", width, a))
        # ... and behind track_samples, in the window's surplus
        rc, got = pcm_track_call(N, [src], base, a, plain(events, ns, extra=[(lo + ns * width, 8 * width)]), surplus=SURPLUS * width)
        _check(rc, got, bytes(want), ("a source behind track_samples", width, a))
        # one sample into the track: refused
        for off in (lo - 7 * width, lo + (ns - 1) * width):
            rc, _ = pcm_track_call(N, [src], base, a, plain(events, ns, extra=[(off, 8 * width)]), surplus=SURPLUS * width, untouched=True)
            assert rc == N.SH_ERR_INVALID, ("a source that overlaps the track", width, a, off - lo, rc)
        # track_samples one beyond the window
        rc, _ = pcm_track_call(N, [src], base, a, plain(events[1:], ns + 1), untouched=True)
        assert rc == N.SH_ERR_INVALID, ("track_samples beyond the window", width, a, rc)
        # an event that ends one sample beyond track_samples, in a window that has room for it
        rc, _ = pcm_track_call(N, [src], base, a, plain([(193, 0, 8, 1.0, 0, 0)], ns), surplus=SURPLUS * width, untouched=True)
        assert rc == N.SH_ERR_INVALID, ("an event beyond track_samples", width, a, rc)


# ---- 3: the strided chain -----------------------------------------------------------------------------------------------------------
CHAIN_RESIDUES = [0, 2, 8, 14]
CHAIN_PAIRS = [(0, 0), (2, 0), (8, 0), (14, 0), (0, 2), (0, 8), (0, 14), (2, 8), (8, 14), (14, 2)]      # (chunks, out)
CHAIN_PAIRS_LONG = [(0, 0), (2, 0), (0, 8), (14, 2), (8, 14)]          # every class and every residue on each side
TAIL = 8 + 3
# (id, voices, samples, long): the route boundaries of sh_mix_chain_i16 / sh_mix_chain_pan_i16, each with the ragged tail
CHAIN_SHAPES = [
    ("9v-4107", 9, 4096 + TAIL, False),                     # under 64 voices: two waves
    ("64v-4107", 64, 4096 + TAIL, False),                   # at least 64: eight waves, one column
    ("9v-640x512", 9, 640 * 512 + TAIL, True),              # the four-samples-per-lane direct loop when on the grid
    ("9v-1536x512", 9, 1536 * 512 + TAIL, True),            # the eight-samples-per-lane direct loop when on the grid
    ("64v-512x512", 64, 512 * 512 + TAIL, True),            # eight waves, two columns
]


def chain_rows(nv, nsamples, seed):
    rng = np.random.default_rng(seed)
    return [(rng.integers(-32768, 32768, nsamples) * 0.6).astype(np.int16) for _ in range(nv)]      # loud: the order shows


def strided(rows, stride, fill=0x1111):
    """the rows at `stride` samples, junk between them, nothing behind the last row"""
    n = len(rows[0])
    buf = np.full((len(rows) - 1) * stride + n, fill, dtype=np.int16)
    for v, x in enumerate(rows):
        buf[v * stride:v * stride + n] = x
    return buf.tobytes()


@pytest.mark.parametrize("name, nv, nsamples, long_", CHAIN_SHAPES, ids=[s[0] for s in CHAIN_SHAPES])
def test_chain_i16_through_windows(gpu, name, nv, nsamples, long_):
    L = gpu.lib()
    rows = chain_rows(nv, nsamples, nv + nsamples)
    want = _audioop_fold(rows, nsamples)
    grid = (nsamples + 7) // 8 * 8
    for stride in (grid, grid + 3):
        data = strided(rows, stride)
        pairs = CHAIN_PAIRS if not long_ else (CHAIN_PAIRS_LONG if stride == grid else [(0, 0), (2, 8)])
        for ac, ao in pairs:
            rc, got = pcm_view_call(gpu, [(data, ac)], 2 * nsamples, ao, lambda iv, ov: L.sh_mix_chain_i16(iv[0].handle, nv, stride, nsamples, ov.handle))
            _check(rc, got, want, ("sh_mix_chain_i16", name, stride - grid, ac, ao))
        rc, got = pcm_view_call(gpu, [(data, 2)], 2 * nsamples, 8, lambda iv, ov: L.sh_mix_chain(iv[0].handle, nv, stride, nsamples, 2, ov.handle))
        _check(rc, got, want, ("sh_mix_chain, width 2", name, stride - grid))


@pytest.mark.parametrize("name, nv, nframes, long_", CHAIN_SHAPES, ids=[s[0] for s in CHAIN_SHAPES])
def test_chain_pan_i16_through_windows(gpu, name, nv, nframes, long_):
    """the rows as mono voices that enter as audioop.tostereo(row, lf, rf); the factors in a window of their own"""
    L = gpu.lib()
    rows = chain_rows(nv, nframes, 7 * nv + nframes)
    fac = np.random.default_rng(nv).uniform(0.2, 1.6, size=(nv, 2))
    stereo = [np.frombuffer(audioop.tostereo(x.tobytes(), 2, float(lf), float(rf)), dtype=np.int16) for x, (lf, rf) in zip(rows, fac)]
    want = _audioop_fold(stereo, 2 * nframes)
    del stereo
    facb = fac.reshape(-1).tobytes()
    grid = (nframes + 7) // 8 * 8
    call = lambda stride: lambda iv, ov: L.sh_mix_chain_pan_i16(iv[0].handle, nv, stride, nframes, iv[1].handle, ov.handle)
    for stride in (grid, grid + 3):
        data = strided(rows, stride)
        pairs = CHAIN_PAIRS if not long_ else (CHAIN_PAIRS_LONG if stride == grid else [(0, 0), (2, 8)])
        for ac, ao in pairs:
            rc, got = pcm_view_call(gpu, [(data, ac), (facb, 0)], 4 * nframes, ao, call(stride))
            _check(rc, got, want, ("sh_mix_chain_pan_i16", name, stride - grid, ac, ao))
    # the factors 8 bytes off the grid: the same bytes, with everything else on the grid (the direct loop's condition but for them) and off it
    for ac, ao in ((0, 0), (8, 2)):
        rc, got = pcm_view_call(gpu, [(data if ac else strided(rows, grid), ac), (facb, 8)], 4 * nframes, ao, call(grid + 3 if ac else grid))
        _check(rc, got, want, ("factors at residue 8", name, ac, ao))


def test_chain_refuses_misaligned_factors(gpu):
    """factors_lr is read as doubles by wave-uniform loads: a window 2 or 4 bytes off their grid is refused by the four strided entry
    points that take one (chain_rows_check), nothing written"""
    L = gpu.lib()
    nv, nframes = 9, 1000 + TAIL
    rows = chain_rows(nv, nframes, 5)
    data = strided(rows, nframes)
    facb = np.random.default_rng(1).uniform(0.2, 1.6, size=2 * nv).tobytes()
    for af in (2, 4, 10, 12):
        rc, _ = pcm_view_call(gpu, [(data, 0), (facb, af)], 4 * nframes, 0,
                              lambda iv, ov: L.sh_mix_chain_pan_i16(iv[0].handle, nv, nframes, nframes, iv[1].handle, ov.handle), untouched=True)
        assert rc == gpu.SH_ERR_INVALID, ("sh_mix_chain_pan_i16", af, rc)
        rc, _ = pcm_view_call(gpu, [(data, 0), (facb, af)], 16 * nframes, 0,
                              lambda iv, ov: L.sh_mix_chain_pan_i16_parts(iv[0].handle, nv, nframes, nframes, iv[1].handle, ov.handle), untouched=True)
        assert rc == gpu.SH_ERR_INVALID, ("sh_mix_chain_pan_i16_parts", af, rc)


@pytest.mark.parametrize("width", [1, 3, 4])
def test_chain_of_the_other_widths_through_windows(gpu, width):
    """sh_mix_chain at 8, 24 and 32 bits: strides and windows at every residue a sample of that width can have"""
    L = gpu.lib()
    rng = np.random.default_rng(300 + width)
    nsamples = 1024 + TAIL
    for nv in (9, 70):
        rows = [_rand_pcm(rng, nsamples, width, 0.6) for _ in range(nv)]
        want = rows[0]
        for r in rows[1:]:
            want = audioop.add(want, r, width)
        for stride in (nsamples, nsamples + 3):
            data = (b"\x11" * ((stride - nsamples) * width)).join(rows)
            rs = residues(width)
            for k, ac in enumerate(rs):
                for ao in (rs[k], rs[(k + 1) % len(rs)]):
                    rc, got = pcm_view_call(gpu, [(data, ac)], nsamples * width, ao, lambda iv, ov: L.sh_mix_chain(iv[0].handle, nv, stride, nsamples, width, ov.handle))
                    _check(rc, got, want, ("sh_mix_chain", width, nv, stride - nsamples, ac, ao))


# ---- 4: the gather ------------------------------------------------------------------------------------------------------------------
OUT_OFFS = [0, 1, 4, 7]
SRC_OFFS = [0, 1, 5]
DIRECT_N = 1536 * 512 + TAIL


def direct_case():
    """the nine sources of the k_mix_chain_gather_direct case as (samples, sample offset, window residue): batch 0 one off-grid source,
    one that ends inside the LAST whole wave's 1 KB, 24 samples short of it (a kernel that took `whole` from another source of the batch
    would read 48 bytes over its end there, inside the parent's guard, and nowhere else: the wave behind it is the ragged tail of every
    source), two whole ones, a whole one first; batch 1 on the grid and whole; the remainder off the grid"""
    n = DIRECT_N
    return [(n, 0, 0), (n, 1, 0), (1536 * 512 - 24, 0, 0), (n, 8, 0),
            (n, 0, 0), (n, 0, 0), (n, 8, 0), (n, 0, 0),
            (n, 5, 8)]


def small_case(nsrc, nsamples, res=tuple(CHAIN_RESIDUES)):
    """ragged sources, the sample offsets and window residues in turn; one empty, one of a single sample, the longest whole"""
    lens = [nsamples, nsamples - 5, 100, 0, nsamples // 2 + 1, nsamples, 8, 1, nsamples - 1]
    return [(lens[v % len(lens)], SRC_OFFS[v % 3], res[(v // 3) % len(res)]) for v in range(nsrc)]


def _gather(gpu, case, nsamples, width, out_offs, seed, what):
    L = gpu.lib()
    rng = np.random.default_rng(seed)
    raws = [_rand_pcm(rng, n, width, 0.6) for n, _off, _a in case]
    want = bytes(nsamples * width)
    for r in raws:
        want = audioop.add(want, r + bytes(nsamples * width - len(r)), width)
    inputs = [(b"\x33" * (off * width) + r, a) for r, (_n, off, a) in zip(raws, case)]
    offs = (C.c_size_t * len(case))(*[off for _n, off, _a in case])
    cnt = (C.c_uint32 * len(case))(*[n for n, _off, _a in case])
    for out_off in out_offs:
        def call(iv, ov):
            bufs = (C.c_void_p * len(iv))(*[v.handle for v in iv])
            if width == 2:
                return L.sh_mix_chain_gather_i16(bufs, offs, cnt, len(iv), nsamples, ov.handle, out_off)
            return L.sh_mix_chain_gather(bufs, offs, cnt, len(iv), nsamples, width, ov.handle, out_off)
        rc, got = pcm_view_call(gpu, inputs, (out_off + nsamples) * width, 0, call)
        _check(rc, got, bytes([PCM_OUT_SENTINEL]) * (out_off * width) + want, (what, width, out_off))


@pytest.mark.parametrize("nsrc", [5, 64, 70])
def test_gather_i16_tables(gpu, nsrc):
    """the table in the kernel arguments (at most 64 sources; 64: eight waves) and in scratch (70)"""
    _gather(gpu, small_case(nsrc, 1024 + TAIL), 1024 + TAIL, 2, OUT_OFFS, nsrc, "gather %d" % nsrc)


def test_gather_i16_direct(gpu):
    """k_mix_chain_gather_direct: two full batches of four sources and a remainder; the output on the grid and off it"""
    _gather(gpu, direct_case(), DIRECT_N, 2, [0, 7], 9, "gather direct")


@pytest.mark.parametrize("width", [1, 3, 4])
def test_gather_of_the_other_widths(gpu, width):
    for nsrc in (5, 70):
        _gather(gpu, small_case(nsrc, 1024 + TAIL, tuple(residues(width))), 1024 + TAIL, width, OUT_OFFS, 10 * width + nsrc, "gather %d" % nsrc)
