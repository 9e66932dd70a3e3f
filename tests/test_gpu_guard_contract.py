"""The int16 boundary guard at chosen tolerances, on every int16 route and kernel shape (include/synthhip.h, ABI 6).

The contract: wherever a Harmonics voice's fast form (polynomial or Clenshaw) lies within guard_t |t| + guard_c of its list's term-by-term
sum, every int16 route gives the LIST's integers.  At the natural tolerance (< 1e-9) the guard is barely exercised -- a handful of
crossings in 67 M samples (tests/test_gpu_guard.py).  Here the fast form is MADE to differ from its list: tests/helpers.perturb_packed moves
each voice's polynomial constant term (or a_1 of the Clenshaw form) so that scale * the sample moves by up to `tq` integers, and raises
guard_c to cover it (tests/test_guard_premise.py holds that premise on the host, without a GPU).
The expected rows depend on the list alone: the C oracle's quantised samples, and the live audioop chains over them.

Tolerances reach every branch of the guard: the 2^-32 grid of the lean kernels (1e-6 .. 0.124), "redo everything" (>= 1/8), and the band
around the integer 0 that is only skipped while tq < 1/2.  Lists of 255 and 272 entries cover the lean record's 8-bit length field.
The same perturbed bank built with params.int16_guard = False must differ in many samples: the guard is what makes the rows right.
"""
import audioop

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

SR = 48000
NEAR = 1e-9
H16 = [(k, 1.0 / k) for k in range(1, 17)]
H15 = [(k, 1.0 / k) for k in range(1, 16)]
# a list whose wave crosses zero where sin(t) does not vanish: the 1/k series is positive on (0, pi) and crosses at t = 0 and pi only,
# where the fixture's move (a multiple of sin t) vanishes too -- this one puts moved samples next to the integer 0
Z5 = [(1, 0.2), (5, 1.0), (11, -0.4), (16, 0.25)]
TOLERANCES = [0.0, 1e-6, 1e-3, 0.05, 0.124, 0.126, 0.49, 0.51, 2.0, 40.0]
S10 = 10 * SR + 777
S300 = 300 * SR


def _bank(name):
    """(make(module) -> voices, gains, rows the oracle decides (the Harmonics voices), guard list for the device's voices or None)."""
    rng = np.random.default_rng(17)

    def harmonics(mod, lists, amps, env=None, long=None):
        out = []
        for j, (harm, amp) in enumerate(zip(lists, amps)):
            f = float(np.exp(np.log(55.0) + (np.log(3520.0) - np.log(55.0)) * ((j * 0.618034) % 1.0)))
            o = mod.Harmonics(f, long if (long is not None and mod.__name__.startswith("oracle")) else harm, amplitude=float(amp),
                              phase=(0.37 * j) % 1.0, samplerate=SR)
            out.append(H.adsr_over(mod, o, env) if env is not None else o)
        return out

    nv = 8
    amps = rng.uniform(0.15, 0.5, nv) * np.where(np.arange(nv) % 3 == 1, -1.0, 1.0)     # (every third voice of negative amplitude)
    gains = [(float(rng.uniform(0.2, 1.0)), float(rng.uniform(0.2, 1.0))) for _ in range(nv)]
    mixed_lists = [H16, Z5] * (nv // 2)
    if name == "lean":
        return (lambda mod: harmonics(mod, mixed_lists, amps)), gains, list(range(nv)), None
    if name == "adsr":                       # sustain level 1.5: the envelope's largest gain (gmax) scales the guard
        a = amps * 0.6
        return (lambda mod: harmonics(mod, mixed_lists, a, env=1.5)), gains, list(range(nv)), None
    if name == "clenshaw":
        lists = [[(1, 1.0), (33, 0.3)], [(k, 1.0 / k) for k in range(1, 41)]] * (nv // 2)
        return (lambda mod: harmonics(mod, lists, amps * 0.7)), gains, list(range(nv)), None
    if name == "mixed":                      # Harmonics interleaved with FM Sine voices: the lean lists of k_generate_lists
        def make(mod):
            hv = harmonics(mod, mixed_lists, amps)
            if mod.__name__.startswith("oracle"):
                return hv
            fm = [mod.Sine(200.0 + 10 * k, 0.3, fm_lfo=mod.Sine(3.0, 0.02, samplerate=SR), samplerate=SR) for k in range(nv)]
            return [x for pair in zip(hv, fm) for x in pair]
        return make, gains + gains, list(range(0, 2 * nv, 2)), None
    if name in ("list255", "list272"):       # the voices' guard lists: 15 x 17 = 255 (fits the lean record) and 16 x 17 = 272 entries
        base = H15 if name == "list255" else H16
        long = H.repeated_list(base, 17)
        n4 = 4
        return (lambda mod: harmonics(mod, [base] * n4, amps[:n4], long=long)), gains[:n4], list(range(n4)), long
    raise KeyError(name)


CASES = [
    # (bank, start, frames, scale): the frames pick the materialisation kernel -- 1000 k_generate<1>, 3000 <2>, 10 000 the lists or
    # the lean kernel, 70 001 two segments with a partial last tile, 2^20 the fused mixdown's folded stretches
    ("lean", S10, 1000, 32767.0),
    ("lean", S300, 3000, 32767.0),
    ("lean", 0, 10000, 32767.0),
    ("lean", S300, 70001, 32767.0),
    ("lean", S300, 1 << 20, 32767.0),
    ("lean", S10, 10000, 20000.0),
    ("adsr", 0, 3000, 32767.0),
    ("adsr", S10, 70001, 32767.0),
    ("mixed", S300, 10000, 32767.0),
    ("clenshaw", S300, 1000, 32767.0),
    ("clenshaw", S10, 70001, 32767.0),
    ("list255", S300, 70001, 32767.0),
    ("list272", S300, 70001, 32767.0),
    ("list272", S10, 3000, 32767.0),
]


def _oracle(make, start, n, scale):
    """(int16 rows, mask of samples within NEAR of a truncation boundary) of the oracle's voices."""
    from oracle import c_oracle as CO
    from oracle import synth_oracle as O
    rows, near = [], []
    for o in make(O):
        inner = o._source if isinstance(o, O.EnvelopeFilter) else o
        if isinstance(o, O.EnvelopeFilter) and (start - 2) / SR <= o._attack + o._decay:
            v = CO.render(o, start + n)[start:]
        else:
            v = CO.render_window(o, start, n)
        assert inner.fm is None
        y = scale * v
        r = np.rint(y)
        d = np.abs(y - r)
        d[r == 0] = 1.0                                        # (no boundary at 0: truncation toward zero)
        rows.append(CO.quantise(v, scale).astype(np.int16))
        near.append(d < NEAR)
    return np.stack(rows), np.stack(near)


def _chain(rows):
    mixed = rows[0].tobytes()
    for r in rows[1:]:
        mixed = audioop.add(mixed, r.tobytes(), 2)
    return np.frombuffer(mixed, dtype=np.int16)


def _chain_stereo(rows, gains):
    mixed = None
    for r, (gl, gr) in zip(rows, gains):
        s = audioop.tostereo(r.tobytes(), 2, gl, gr)
        mixed = s if mixed is None else audioop.add(mixed, s, 2)
    return np.frombuffer(mixed, dtype=np.int16)


def _bad(got, want, allowed):
    """samples that differ where no allowance covers them (allowed: a one-step difference at an oracle sample within NEAR of a boundary)"""
    d = got != want
    if not d.any():
        return 0
    ok = allowed & (np.abs(got.astype(np.int32) - want.astype(np.int32)) <= 1)
    return int(np.count_nonzero(d & ~ok))


@pytest.mark.parametrize("bank,start,n,scale", CASES, ids=["%s-%d-%s-%d" % (b, n, "0" if s == 0 else ("10s" if s == S10 else "300s"), sc) for b, s, n, sc in CASES])
def test_every_int16_route_gives_the_lists_integers(gpu, monkeypatch, bank, start, n, scale):
    N = gpu
    from synthesizer_amd import mixer, params
    from synthesizer_amd import oscillators as G
    from synthesizer_amd.mixer import VoiceBank, apply_chain_parts, compose_chain_parts
    make, gains, hrows, glist = _bank(bank)
    want_h, near_h = _oracle(make, start, n, scale)
    nv = len(gains)
    orig_pack = mixer.pack_voices
    failures = []
    print("\n%s start %d frames %d scale %g: %d oracle samples within %.0e of a truncation boundary"
          % (bank, start, n, scale, int(near_h.sum()), NEAR))

    def build(tq, guard=True, voices=None, gains_=None):
        monkeypatch.setattr(mixer, "pack_voices", lambda specs, g=None: H.perturb_packed(orig_pack(specs, g), tq, scale, glist))
        params.int16_guard = guard
        try:
            return VoiceBank(voices if voices is not None else make(G), gains=gains_ if gains_ is not None else gains)
        finally:
            params.int16_guard = True
            monkeypatch.setattr(mixer, "pack_voices", orig_pack)

    for tq in TOLERANCES:
        b = build(tq)
        stride_rows, stride = b.generate_i16_device(n, start, scale)
        got = stride_rows.download(np.int16, nv * stride).reshape(nv, stride)[:, :n].copy()
        stride_rows.free()
        # the rows the oracle decides come from it; the others (FM voices: a bound, not equality) from the device
        want = got.copy()
        allowed = np.zeros(want.shape, dtype=bool)
        want[hrows] = want_h
        allowed[hrows] = near_h
        counts = {"rows": _bad(got, want, allowed)}
        frame_ok = allowed.any(axis=0)
        mono = _chain(want)
        counts["mono_fused"] = _bad(np.frombuffer(b.mixdown_i16_device(n, start, scale).download_bytes(n * 2), dtype=np.int16), mono, frame_ok)
        fused = N.lib().sh_get_option(N.SH_INFO_LAST_MIXDOWN_FUSED)
        counts["mono_two_step"] = _bad(np.frombuffer(b.mixdown_i16_device(n, start, scale, two_step=True).download_bytes(n * 2), dtype=np.int16),
                                       mono, frame_ok)
        stereo = _chain_stereo(want, gains)
        st_ok = np.repeat(frame_ok, 2)
        counts["stereo"] = _bad(np.frombuffer(b.mixdown_stereo_i16_device(n, start, scale).download_bytes(n * 4), dtype=np.int16), stereo, st_ok)
        # the parts route: the voices in two shards (banks of their own), each leaving its chain maps; applied in order, and composed first
        voices = make(G)
        cut = nv // 2 + 1
        shards = [build(tq, voices=voices[:cut], gains_=gains[:cut]), build(tq, voices=voices[cut:], gains_=gains[cut:])]
        parts = [s.mixdown_i16_parts_device(n, start, scale) for s in shards]
        counts["parts"] = _bad(np.frombuffer(apply_chain_parts(parts, n).download_bytes(n * 2), dtype=np.int16), mono, frame_ok)
        counts["parts_composed"] = _bad(np.frombuffer(apply_chain_parts([compose_chain_parts(parts, n)], n).download_bytes(n * 2), dtype=np.int16),
                                        mono, frame_ok)
        sparts = [s.mixdown_i16_parts_device(n, start, scale, stereo=True) for s in shards]
        counts["parts_stereo"] = _bad(np.frombuffer(apply_chain_parts(sparts, 2 * n).download_bytes(n * 4), dtype=np.int16), stereo, st_ok)
        for p in parts + sparts:
            p.free()
        line = "  tq %-6g fused stretches %d: %s" % (tq, fused, " ".join("%s %d" % kv for kv in counts.items()))
        # teeth: the same perturbed bank without the guard lists differs from the list's integers in many samples
        if tq >= 1e-3:
            plain = build(tq, guard=False)
            prow, pstride = plain.generate_i16_device(n, start, scale)
            pgot = prow.download(np.int16, nv * pstride).reshape(nv, pstride)[:, :n][hrows]
            prow.free()
            off = int(np.count_nonzero(pgot != want_h))
            expect = int(0.1 * (2.0 / np.pi) * min(tq, 1.0) * want_h.size)     # (a tenth of the crossings sin(t) * tq makes on average)
            line += "; guard off: %d differ (bound %d)" % (off, expect if expect >= 5 else 0)
            if expect >= 5 and off < expect:
                failures.append("tq %g: without the guard only %d samples differ (< %d): the perturbation did not take" % (tq, off, expect))
        print(line)
        for route, c in counts.items():
            if c:
                failures.append("tq %g %s: %d int16 samples differ from the list's" % (tq, route, c))
    assert not failures, "\n".join(failures)
    if bank == "lean" and n == 1 << 20:
        assert fused > 0, "the 2^20-frame lean window took no fused stretch"

