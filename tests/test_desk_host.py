"""What the ``pans`` and ``master`` keywords of a compiled song of tracks need of the host alone (no GPU): every check and message raised
before the native layer is reached, a pan number turned into ``Sample.pan``'s factors bit for bit, what render hands on, and that
``None`` / 1.0 leave the entry points there were to be called.  The bytes: tests/test_gpu_desk.py."""
import ctypes as C
from pathlib import Path

import pytest

from synthesizer_amd import _native as N
from synthesizer_amd import mixer
from tests.songhost import RATE, _calls, _fake, _Lib, _mono, _Seq, _stereo

nan, inf = float("nan"), float("inf")


def _song(monkeypatch, nch=2):
    _fake(monkeypatch)
    monkeypatch.setattr(N, "Sequence", _Seq)
    a = _stereo(1000) if nch == 2 else _mono(1000)
    return mixer.compile_tracks([[(0.0, a), (0.5, a, 0.5)], [], [(0.25, a)]], RATE, nch)


@pytest.mark.parametrize("bad, message", [
    ((None, None), "2 pans for 3 tracks"),
    ((None,) * 4, "4 pans for 3 tracks"),
    ((), "0 pans for 3 tracks"),
    (0.5, "pans is a sequence, one entry per track"),
    ("abc", "pans is a sequence, one entry per track"),
    ((None, 1.0001, None), "pan 1 must be between -1 and 1"),
    ((-1.5, None, None), "pan 0 must be between -1 and 1"),
    ((None, None, nan), "pan 2 must be between -1 and 1"),
    ((None, inf, None), "pan 1 must be between -1 and 1"),
    ((None, "x", None), r"pan 1 is None, a number or a pair \(left_factor, right_factor\)"),
    ((None, (0.5,), None), r"pan 1 is not a pair \(left_factor, right_factor\) of finite numbers"),
    ((None, (0.5, 0.5, 0.5), None), r"pan 1 is not a pair \(left_factor, right_factor\) of finite numbers"),
    (([0.5, nan], None, None), r"pan 0 is not a pair \(left_factor, right_factor\) of finite numbers"),
    ((None, None, (inf, 0.0)), r"pan 2 is not a pair \(left_factor, right_factor\) of finite numbers"),
    ((None, None, ("a", 0.0)), r"pan 2 is not a pair \(left_factor, right_factor\) of finite numbers"),
    ((None, (None, 1.0), None), r"pan 1 is not a pair \(left_factor, right_factor\) of finite numbers"),
])
def test_pans_are_checked_before_anything_is_rendered(monkeypatch, bad, message):
    cs = _song(monkeypatch)
    for call in _calls(cs, pans=bad) + _calls(cs, pans=bad, gains=(1.0, 0.5, 1.0), master=0.5, meters=True):
        with pytest.raises(ValueError, match="CompiledSequence: " + message):
            call()
    assert cs._seq.rendered == []


@pytest.mark.parametrize("bad, message", [(nan, "master is not finite"), (inf, "master is not finite"), (-inf, "master is not finite"),
                                          ("x", "master is a number"), ((0.5,), "master is a number")])
def test_the_master_is_checked_before_anything_is_rendered(monkeypatch, bad, message):
    cs = _song(monkeypatch)
    for call in _calls(cs, master=bad) + _calls(cs, master=bad, pans=(0.3, None, None)):
        with pytest.raises(ValueError, match="CompiledSequence: " + message):
            call()
    assert cs._seq.rendered == []


def test_a_song_without_tracks_and_a_song_that_is_not_stereo(monkeypatch):
    _fake(monkeypatch)
    monkeypatch.setattr(N, "Sequence", _Seq)
    flat = mixer.compile_sequence([(0.0, _stereo())], RATE, 2)
    for call in _calls(flat, pans=(0.3,)) + _calls(flat, pans=()):
        with pytest.raises(ValueError, match=r"CompiledSequence: pans need a song of tracks \(compile_tracks\); this one has none"):
            call()
    for call in _calls(flat, master=0.5) + _calls(flat, master=1.0):
        with pytest.raises(ValueError, match=r"CompiledSequence: master needs a song of tracks \(compile_tracks\); this one has none"):
            call()
    assert flat._seq.rendered == []
    mono = _song(monkeypatch, nch=1)
    for call in _calls(mono, pans=(None, None, None)) + _calls(mono, pans=(0.3, None, None), master=0.5):
        with pytest.raises(ValueError, match="CompiledSequence: pans need a stereo song, this one has 1 channels"):
            call()
    assert mono._seq.rendered == []
    mono.render(2, 5, master=0.5, gains=(1.0, 2.0, 3.0))        # a mono song has a master fader
    assert mono._seq.rendered == [(2, 5, 0, dict(gains=[1.0, 2.0, 3.0], pans=None, master=0.5))]


def test_a_pan_number_becomes_sample_pans_factors_bit_for_bit(monkeypatch):
    cs = _song(monkeypatch)
    import numpy as np
    for p in (0.3, -0.37, 1.0, -1.0, 0.0, 0.1, 1 / 3, -1e-17, 5e-324, 0.999, 1, np.float32(0.3)):
        cs.render(0, 10, pans=(p, None, (1.5, -0.25)))
        handed = cs._seq.rendered[-1][3]["pans"]
        pf = float(p)
        assert handed == [(1.0 - pf) / 2.0, (1.0 + pf) / 2.0, 1.0, 1.0, 1.5, -0.25] and all(type(f) is float for f in handed)
        assert [f.hex() for f in handed[:2]] == [((1.0 - pf) / 2.0).hex(), ((1.0 + pf) / 2.0).hex()]      # Sample.pan's own expression
    from synthesizer_amd.sample import _pan_factors
    cs.render(0, 10, pans=(0.3, 0.0, -1.0))
    assert cs._seq.rendered[-1][3]["pans"] == [f for p in (0.3, 0.0, -1.0) for f in _pan_factors(p, 1, 2)]
    assert cs._seq.rendered[-1][3]["pans"][2:4] == [0.5, 0.5]   # centre halves both sides, as upstream's pan


def test_what_render_hands_on(monkeypatch):
    cs = _song(monkeypatch)
    seq = cs._seq
    # None, all-None, (1.0, 1.0) and a master of None or exactly 1.0: no step, the calls there were, without the new keywords
    cs.render(10, 20)
    cs.render(10, 20, pans=None, master=None)
    cs.render(10, 20, pans=[None] * 3, master=1.0)
    cs.render(10, 20, gains=(0.5, 1.0, 2.0), pans=((1.0, 1.0), None, [1, 1]), master=1)
    cs.render(10, 20, gains=(0.5, 1.0, 2.0), pans=[None] * 3, meters=True)
    assert seq.rendered == [(20, 40, 0, {}), (20, 40, 0, {}), (20, 40, 0, {}), (20, 40, 0, dict(gains=[0.5, 1.0, 2.0])),
                            (20, 40, 0, dict(gains=[0.5, 1.0, 2.0], meters=True))]      # (a stereo song: two samples a frame)
    del seq.rendered[:]
    # a step somewhere: both keywords, the pans flat, left then right per track, (1.0, 1.0) where there is none
    cs.render(10, 20, pans=(None, (0.0, 0.0), (-0.5, 1.0)))
    cs.render(10, 20, master=-1.3)
    cs.render_into(N.DeviceBuffer(100), 4, 3, 9, gains=(0.0, 1.0, 1.0), pans=(1.0, None, None), master=0.7)
    out, levels = cs.render(0, 8, pans=(-1.0, None, None), master=0.0, meters=True)
    list(cs.chunks(cs.frames - 1, gains=(1.0,) * 3, pans=(None, None, 0.0), master=2))
    assert seq.rendered == [
        (20, 40, 0, dict(gains=None, pans=[1.0, 1.0, 0.0, 0.0, -0.5, 1.0], master=None)),
        (20, 40, 0, dict(gains=None, pans=None, master=-1.3)),
        (6, 18, 2, dict(gains=[0.0, 1.0, 1.0], pans=[0.0, 1.0, 1.0, 1.0, 1.0, 1.0], master=0.7)),
        (0, 16, 0, dict(gains=None, meters=True, pans=[1.0, 0.0, 1.0, 1.0, 1.0, 1.0], master=0.0)),
        (0, 2 * cs.frames - 2, 0, dict(gains=[1.0] * 3, pans=[1.0, 1.0, 1.0, 1.0, 0.5, 0.5], master=2.0)),
        (2 * cs.frames - 2, 2, 0, dict(gains=[1.0] * 3, pans=[1.0, 1.0, 1.0, 1.0, 0.5, 0.5], master=2.0)),
    ]
    assert isinstance(levels, mixer.SongLevels) and len(levels.tracks) == 3
    del seq.rendered[:]
    cs.stem(2, 5, 7)                                            # stem stays: gain 1.0, no pan, no master
    assert seq.rendered == [(10, 14, 0, dict(gains=[0.0, 0.0, 1.0]))]
    cs.close()
    for call in _calls(cs, pans=(0.3, None, None)) + _calls(cs, master=0.5):
        with pytest.raises(ValueError, match="closed"):
            call()


def test_the_binding_calls_the_new_entry_point_only_when_a_step_is_given(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(N, "lib", lambda: lib)
    seq = N.Sequence.__new__(N.Sequence)
    seq._h, seq._sources = C.c_void_p(1), []

    class Out:
        handle = C.c_void_p(2)
    seq.render(5, 6, Out, 7)
    seq.render(5, 6, Out, 7, gains=[1.0, 2.0, 3.0])
    seq.render(5, 6, Out, 7, gains=[1.0, 2.0, 3.0], meters=True)
    assert [c[0] for c in lib.calls] == ["sh_seq_render", "sh_seq_render_gains", "sh_seq_get_tracks", "sh_seq_render_meters"]
    del lib.calls[:]
    assert seq.render(5, 6, Out, 7, pans=[0.5, 0.25, 1.0, 1.0, 0.0, -1.0]) is None
    assert seq.render(5, 6, Out, 7, gains=[1.0, 2.0, 3.0], master=0.7) is None
    rows = seq.render(5, 6, Out, 7, gains=[1.0, 2.0, 3.0], pans=[0.5, 0.25, 1.0, 1.0, 0.0, -1.0], master=-1.3, meters=True)
    assert rows == [((0, 0), (0, 0))] * 4
    desk = [c for c in lib.calls if c[0] != "sh_seq_get_tracks"]
    assert [c[0] for c in desk] == ["sh_seq_render_desk"] * 3
    a, b, c = (d[1] for d in desk)
    assert a[1:3] == b[1:3] == c[1:3] == (5, 6) and a[4] == 7
    assert (a[5], a[6], list(a[7]), a[8], a[9], a[10], a[11]) == (None, 0, [0.5, 0.25, 1.0, 1.0, 0.0, -1.0], 6, 1.0, None, 0)
    assert (list(b[5]), b[6], b[7], b[8], b[9], b[10], b[11]) == ([1.0, 2.0, 3.0], 3, None, 0, 0.7, None, 0)
    assert (list(c[5]), c[6], list(c[7]), c[8], c[9], len(c[10]), c[11]) == ([1.0, 2.0, 3.0], 3, [0.5, 0.25, 1.0, 1.0, 0.0, -1.0], 6, -1.3, 4, 4)
    seq.free()                                                  # (while the library is the fake one: the handle is no sh_seq)
    assert lib.calls[-1][0] == "sh_seq_destroy" and not seq._h


def test_the_new_symbol_is_declared_beside_the_ones_it_extends():
    table = N._SIGNATURES
    desk, meters = table["sh_seq_render_desk"][1], table["sh_seq_render_meters"][1]
    assert len(desk) == 12 and desk[:7] == meters[:7] and desk[7:10] == [C.POINTER(C.c_double), C.c_uint32, C.c_double] and desk[10:] == meters[7:]
    header = (Path(__file__).resolve().parents[1] / "include" / "synthhip.h").read_text()
    assert "int sh_seq_render_desk(" in header and "#define SH_ABI_VERSION 6" in header
