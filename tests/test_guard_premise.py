"""The premise of tests/test_gpu_guard_contract.py, on the host (no GPU): a bank whose fast forms were moved away from their lists by
tests/helpers.perturb_packed still declares a tolerance that covers the move, so the contract of include/synthhip.h (ABI 6) -- the list's
integers wherever the fast form lies within guard_t |t| + guard_c of the list's term-by-term sum -- is what the GPU test expects, not an
artefact of the fixture.  And pack_voices never hands the library a polynomial or Clenshaw voice with a guard list over 255 entries."""
import math

import numpy as np
import pytest

from oracle import c_oracle as CO
from oracle import synth_oracle as O
from synthesizer_amd import _native as N
from synthesizer_amd import oscillators as G
from tests import helpers as H

SR = 48000
H16 = [(k, 1.0 / k) for k in range(1, 17)]
H15 = [(k, 1.0 / k) for k in range(1, 16)]
TOLERANCES = [0.0, 1e-6, 1e-3, 0.05, 0.124, 0.126, 0.49, 0.51, 2.0, 40.0]

# (name, list of the device's voice, list of the oracle's voice / the guard list, amplitude, sustain level or None)
VOICES = [
    ("poly 1/k x16", H16, None, 0.4, None),
    ("poly, negative amplitude", H16, None, -0.3, None),
    ("poly crossing zero off t = 0, pi", [(1, 0.2), (5, 1.0), (11, -0.4), (16, 0.25)], None, 0.3, None),
    ("poly under an ADSR, sustain 1.5", H16, None, 0.25, 1.5),
    ("Clenshaw 1 + 33", [(1, 1.0), (33, 0.3)], None, 0.35, None),
    ("Clenshaw dense to 40", [(k, 1.0 / k) for k in range(1, 41)], None, 0.3, None),
    ("poly, guard list 15 x 17 = 255", H15, H.repeated_list(H15, 17), 0.4, None),
    ("poly, guard list 16 x 17 = 272", H16, H.repeated_list(H16, 17), 0.4, None),
]


def _voice(mod, harm, amp, sustain):
    o = mod.Harmonics(440.0, harm, amplitude=amp, phase=0.2, samplerate=SR)
    return H.adsr_over(mod, o, sustain) if sustain is not None else o


@pytest.mark.parametrize("scale", [32767.0, 20000.0])
@pytest.mark.parametrize("name,harm,glist,amp,sustain", VOICES, ids=[v[0] for v in VOICES])
def test_perturbed_fast_form_stays_within_its_declared_tolerance(name, harm, glist, amp, sustain, scale):
    """|altered fast form - the list's term-by-term sum| <= the altered guard_t |t| + guard_c at 4000 frames 10 s and 300 s into the note,
    for every tolerance of the GPU test; and where the fast form was moved, it did move (by at least half of tq / scale somewhere)."""
    n = 4000
    packed = G.pack_voices([_voice(G, harm, amp, sustain).spec()])
    assert int(packed[0]["guard_count"][0]) == len(harm) and int(packed[0]["harm_dense"][0]) in (1, 2)
    osc = O.Harmonics(440.0, glist if glist is not None else harm, amplitude=amp, phase=0.2, samplerate=SR)
    g = 1.0 if sustain is None else sustain
    worst = 0.0
    for start in (10 * SR + 777, 300 * SR):
        t = H.accumulated(osc._phase * 2.0 * math.pi, O._increment(osc.frequency, SR, True), start, n)
        ref = CO.render_window(_voice(O, glist if glist is not None else harm, amp, sustain), start, n).astype(np.longdouble)
        for tq in TOLERANCES:
            voices, _segs, coefs, _parts = H.perturb_packed(packed, tq, scale, glist)
            v = voices[0]
            off, cnt, dense = int(v["harm_offset"]), int(v["harm_count"]), int(v["harm_dense"])
            if glist is not None:
                assert int(v["guard_count"]) == len(glist)
            fast = H.fast_form_longdouble(coefs[off:off + cnt], dense, t) * np.longdouble(amp) * np.longdouble(g)
            dist = np.abs(fast - ref)
            bound = float(v["guard_t"]) * np.abs(t).astype(np.longdouble) + float(v["guard_c"])
            worst = max(worst, float(np.max(dist / bound)))
            assert np.all(dist <= bound), (name, start, tq, float(np.max(dist - bound)))
            if tq > 0:
                assert float(np.max(dist)) >= 0.5 * tq / scale * g / H.guard_gmax(v), (name, start, tq)
    print("%s, scale %g: distance / declared tolerance at most %.3f" % (name, scale, worst))


def test_pack_voices_never_emits_a_guard_list_over_255():
    """The lean records hold a guard list's length in eight bits: Harmonics.spec() sums a longer list term by term instead (harm_dense 0,
    no guard).  255 entries keep the fast form and its guard; 256 and more, polynomial- or Clenshaw-capable, do not."""
    cases = [(H.repeated_list(H15, 17), 255, 2), (H.repeated_list(H16, 16), 256, None), (H.repeated_list(H16, 17), 272, None),
             ([(k % 40 + 1, 1.0 / (k + 1)) for k in range(255)], 255, 1), ([(k % 40 + 1, 1.0 / (k + 1)) for k in range(300)], 300, None)]
    specs = [G.Harmonics(330.0, harm, amplitude=0.3, samplerate=SR).spec() for harm, _n, _d in cases]
    voices = G.pack_voices(specs)[0]
    for i, (harm, length, dense) in enumerate(cases):
        assert len(harm) == length
        gcount, hd = int(voices["guard_count"][i]), int(voices["harm_dense"][i])
        if hd in (1, 2):
            assert gcount <= 255, (length, gcount)
        if dense is None:
            assert hd == 0 and gcount == 0, (length, hd, gcount)
        else:
            assert hd == dense and gcount == length, (length, hd, gcount)
    # and the same for whole tables of such voices, whatever the amplitude or envelope
    rng = np.random.default_rng(3)
    specs = []
    for j in range(64):
        m = int(rng.integers(1, 400))
        harm = [(int(rng.integers(1, 41)), float(rng.uniform(-1, 1))) for _ in range(m)]
        o = G.Harmonics(float(rng.uniform(55, 3520)), harm, amplitude=float(rng.uniform(-1, 1)), samplerate=SR)
        specs.append((G.EnvelopeFilter(o, 0.01, 0.05, 1.0, float(rng.uniform(0.2, 1.0)), 0.1) if j % 2 else o).spec())
    voices = G.pack_voices(specs)[0]
    fast = np.isin(voices["harm_dense"], (1, 2))
    assert fast.any() and int(np.max(voices["guard_count"][fast])) <= 255
    assert np.all(voices["guard_count"][~fast] == 0) and np.all(voices["kind"] == N.SH_HARMONICS)
