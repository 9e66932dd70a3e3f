"""What fader automation of a compiled song of tracks needs of the host alone (no GPU): every check of ``CompiledSequence.automation``
and of the ``automation=`` keyword raised before the native layer is reached, the records packed as the kernels read them, pieces at
exactly 1.0 dropped, what render hands on, the reference expression against ``oracle.pcm_oracle.fade`` and ``RefSample.fadein`` /
``fadeout``, and the range claim that lets the kernels do without a clamp.  The bytes: tests/test_gpu_automation.py."""
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest

from oracle import pcm_oracle
from oracle.sample_oracle import RefSample
from synthesizer_amd import _native as N
from synthesizer_amd import mixer
from tests.songhost import RATE, _calls, _clip, _fake, _Lib, _mono, _piece, _Seq, _stereo

nan, inf = float("nan"), float("inf")


class _Auto:
    """N.SeqAutomation as the mixer sees it: what it was handed"""
    made = []

    def __init__(self, seq, segments, seg_first):
        self.seq, self.segments, self.seg_first, self.freed = seq, segments, seg_first, False
        _Auto.made.append(self)

    def free(self):
        self.freed = True


def _song(monkeypatch, nch=2, width=2):
    _fake(monkeypatch)
    monkeypatch.setattr(N, "Sequence", _Seq)
    monkeypatch.setattr(N, "SeqAutomation", _Auto)
    del _Auto.made[:]
    a = _stereo(1000, width) if nch == 2 else _mono(1000, width)
    return mixer.compile_tracks([[(0.0, a), (0.5, a, 0.5)], [], [(0.25, a)]], RATE, nch, width)


# ---- the checks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes, message", [
    ((None, None), "2 lanes for 3 tracks"),
    ((None,) * 4, "4 lanes for 3 tracks"),
    (0.5, "lanes is a sequence, one entry per track"),
    ("abc", "lanes is a sequence, one entry per track"),
    ((None, 0.5, None), "track 1: a lane is None or a list of pieces"),
    ((None, "ab", None), "track 1: a lane is None or a list of pieces"),
    (([(0, 10, 0.5)], None, None), r"track 0, piece 0: a piece is \(start_frame, end_frame, from_volume, to_volume\)"),
    ((None, [(0, 10, 0.5, 1.0), (10, 20, 0.5, 1.0, 0.0)], None), r"track 1, piece 1: a piece is \(start_frame, end_frame, from_volume, to_volume\)"),
    ((None, [7], None), r"track 1, piece 0: a piece is \(start_frame, end_frame, from_volume, to_volume\)"),
    ((None, None, [(0, 10, "x", 1.0)]), "track 2, piece 0: a piece is .* four numbers"),
    ((None, None, [(0, 10, 0.5, None)]), "track 2, piece 0: a piece is .* four numbers"),
    (([(0.0, 10, 0.5, 1.0)], None, None), "track 0, piece 0: start_frame and end_frame are integers"),
    (([(0, 10.5, 0.5, 1.0)], None, None), "track 0, piece 0: start_frame and end_frame are integers"),
    (([(True, 10, 0.5, 1.0)], None, None), "track 0, piece 0: start_frame and end_frame are integers"),
    (([(0, "10", 0.5, 1.0)], None, None), "track 0, piece 0: start_frame and end_frame are integers"),
    (([(10, 10, 0.5, 1.0)], None, None), r"track 0, piece 0: frames \[10, 10\): a piece starts at 0 or later and ends behind its start"),
    (([(0, 5, 0.5, 1.0), (12, 10, 0.5, 1.0)], None, None), r"track 0, piece 1: frames \[12, 10\)"),
    (([(-1, 5, 0.5, 1.0)], None, None), r"track 0, piece 0: frames \[-1, 5\)"),
    ((None, [(0, 5001, 0.5, 1.0)], None), r"track 1, piece 0: frames \[0, 5001\) end past the song's 5000 frames"),
    ((None, [(0, 10, 0.5, 1.0), (9, 20, 1.0, 0.5)], None), r"track 1, piece 1: starts at frame 9, before the piece in front of it ends \(10\)"),
    ((None, [(0, 10, 1.0, 1.0), (9, 20, 1.0, 0.5)], None), r"track 1, piece 1: starts at frame 9, before the piece in front of it ends \(10\)"),
    ((None, [(20, 30, 0.5, 1.0), (0, 10, 1.0, 0.5)], None), r"track 1, piece 1: starts at frame 0, before the piece in front of it ends \(30\)"),
    ((None, None, [(0, 10, 1.0001, 1.0)]), "track 2, piece 0: from_volume 1.0001 is not a finite number within 0.0 .. 1.0"),
    ((None, None, [(0, 10, 0.5, -0.1)]), "track 2, piece 0: to_volume -0.1 is not a finite number within 0.0 .. 1.0"),
    ((None, None, [(0, 10, nan, 1.0)]), "track 2, piece 0: from_volume nan is not a finite number within 0.0 .. 1.0"),
    ((None, None, [(0, 10, 0.5, inf)]), "track 2, piece 0: to_volume inf is not a finite number within 0.0 .. 1.0"),
])
def test_lanes_are_checked_before_the_device_is_reached(monkeypatch, lanes, message):
    cs = _song(monkeypatch)
    assert cs.frames == 5000
    with pytest.raises(ValueError, match="CompiledSequence: automation: " + message):
        cs.automation(lanes)
    assert _Auto.made == [] and cs._seq.rendered == []


def test_a_song_without_tracks_a_24_bit_song_and_a_closed_song(monkeypatch):
    _fake(monkeypatch)
    monkeypatch.setattr(N, "Sequence", _Seq)
    monkeypatch.setattr(N, "SeqAutomation", _Auto)
    del _Auto.made[:]
    flat = mixer.compile_sequence([(0.0, _stereo())], RATE, 2)
    with pytest.raises(ValueError, match=r"CompiledSequence: automation needs a song of tracks \(compile_tracks\); this one has none"):
        flat.automation([None])
    for nch in (1, 2):
        wide = _song(monkeypatch, nch=nch, width=3)
        for lanes in ([None] * 3, [[(0, 10, 0.5, 1.0)], None, None], "nonsense"):
            with pytest.raises(NotImplementedError, match="CompiledSequence: automation: width 3: a fade has no 24-bit form"):
                wide.automation(lanes)
    cs = _song(monkeypatch)
    cs.close()
    with pytest.raises(ValueError, match="closed"):
        cs.automation([None] * 3)
    assert _Auto.made == []


@pytest.mark.parametrize("nch", [1, 2])
def test_the_records_are_packed_in_song_samples_and_unity_pieces_are_dropped(monkeypatch, nch):
    cs = _song(monkeypatch, nch=nch)
    lanes = [[(0, 10, 0.25, 1.0), (10, 30, 1.0, 1.0), (30, 31, 0.5, 0.5), (40, 4999, 1.0, 0.1)], None,
             ((5, 6, 1, 1), [7, 9, 0, 0.37], (9, np.int64(5000), np.float32(0.5), 0))]
    auto = cs.automation(lanes)
    assert auto.pieces == (((0, 10, 0.25, 1.0), (30, 31, 0.5, 0.5), (40, 4999, 1.0, 0.1)), (), ((7, 9, 0.0, 0.37), (9, 5000, 0.5, 0.0)))
    assert all(type(v) is float for lane in auto.pieces for p in lane for v in p[2:]) and all(type(f) is int for lane in auto.pieces for p in lane for f in p[:2])
    assert len(_Auto.made) == 1 and _Auto.made[0].seq is cs._seq and _Auto.made[0].segments is auto.segments
    assert auto.seg_first == _Auto.made[0].seg_first == [0, 5, 5, 8]
    g = auto.segments
    assert g.dtype == N.ENV_SEGMENT_DTYPE
    rows = [tuple(g[k][f] for f in ("end", "origin", "mul", "slope", "numsamples", "offset", "kind", "reserved")) for k in range(len(g))]
    c, F, NONE = nch, N.ENV_FADE_IN, N.ENV_NONE
    assert rows == [
        (10 * c, 0, 1.0, 1.0 - 0.25, 10.0 * c, 0.25, F, 0),
        (30 * c, 0, 1.0, 0.0, 0.0, 0.0, NONE, 0),               # the gap: the dropped piece and nothing else
        (31 * c, 30 * c, 1.0, 0.0, 1.0 * c, 0.5, F, 0),         # a hold: slope 0.0
        (40 * c, 0, 1.0, 0.0, 0.0, 0.0, NONE, 0),
        (4999 * c, 40 * c, 1.0, 0.1 - 1.0, 4959.0 * c, 1.0, F, 0),
        (7 * c, 0, 1.0, 0.0, 0.0, 0.0, NONE, 0),                # track 2: the gap in front of its first kept piece
        (9 * c, 7 * c, 1.0, 0.37, 2.0 * c, 0.0, F, 0),
        (5000 * c, 9 * c, 1.0, -0.5, 4991.0 * c, 0.5, F, 0),    # two pieces that meet: no gap
    ]
    assert g["slope"][4].hex() == (0.1 - 1.0).hex()             # v1 - v0 as Python forms it
    # nothing but unity, or nothing at all: an empty table
    for lanes in ([None] * 3, [[(0, 5000, 1.0, 1.0)], [], [(1, 2, 1, 1), (2, 3, 1.0, 1)]]):
        empty = cs.automation(lanes)
        assert empty.pieces == ((), (), ()) and len(empty.segments) == 0 and empty.seg_first == [0, 0, 0, 0]
    # close, with and the last reference free the table once
    made = _Auto.made[0]
    auto.close()
    auto.close()
    assert made.freed
    with pytest.raises(ValueError, match="Automation: closed"):
        cs.render(automation=auto)
    with cs.automation([None] * 3) as inside:
        held = inside._auto
    assert held.freed


# ---- what render hands on ----------------------------------------------------------------------------------------------------------------
def test_the_keyword_is_checked_before_anything_is_rendered_and_handed_on_as_it_is(monkeypatch):
    cs = _song(monkeypatch)
    other = _song(monkeypatch)
    theirs = other.automation([None] * 3)
    for bad in (theirs, "x", 0.5, [None] * 3, object()):
        for call in _calls(cs, automation=bad) + _calls(cs, automation=bad, gains=(1.0, 0.5, 1.0), pans=(0.3, None, None), master=0.5, meters=True):
            with pytest.raises(ValueError, match="CompiledSequence: automation is None or an Automation made by this song's automation"):
                call()
    flat = mixer.compile_sequence([(0.0, _stereo())], RATE, 2)
    for call in _calls(flat, automation=theirs):
        with pytest.raises(ValueError, match="CompiledSequence: automation is None or an Automation made by this song's automation"):
            call()
    assert cs._seq.rendered == [] and flat._seq.rendered == []
    seq = cs._seq
    # None: the calls there were, without the new keyword
    cs.render(10, 20, automation=None)
    cs.render(10, 20, gains=(0.5, 1.0, 2.0), automation=None)
    cs.render(10, 20, gains=(0.5, 1.0, 2.0), pans=(0.0, None, None), master=0.5, automation=None)
    list(cs.chunks(cs.frames, automation=None))
    assert seq.rendered == [(20, 40, 0, {}), (20, 40, 0, dict(gains=[0.5, 1.0, 2.0])),
                            (20, 40, 0, dict(gains=[0.5, 1.0, 2.0], pans=[0.5, 0.5, 1.0, 1.0, 1.0, 1.0], master=0.5)), (0, 2 * cs.frames, 0, {})]
    del seq.rendered[:]
    auto = cs.automation([[(0, 10, 0.5, 1.0)], None, None])
    h = auto._auto
    cs.render(10, 20, automation=auto)
    cs.render_into(N.DeviceBuffer(100), 4, 3, 9, gains=(0.0, 1.0, 1.0), pans=(1.0, None, None), master=0.7, automation=auto)
    out, levels = cs.render(0, 8, master=1.0, meters=True, automation=auto)
    list(cs.chunks(cs.frames - 1, gains=(1.0,) * 3, automation=auto))
    cs.render(3, 0, automation=auto)                            # an empty window: nothing is launched
    assert seq.rendered == [
        (20, 40, 0, dict(gains=None, pans=None, master=None, automation=h)),
        (6, 18, 2, dict(gains=[0.0, 1.0, 1.0], pans=[0.0, 1.0, 1.0, 1.0, 1.0, 1.0], master=0.7, automation=h)),
        (0, 16, 0, dict(gains=None, meters=True, pans=None, master=None, automation=h)),
        (0, 2 * cs.frames - 2, 0, dict(gains=[1.0] * 3, pans=None, master=None, automation=h)),
        (2 * cs.frames - 2, 2, 0, dict(gains=[1.0] * 3, pans=None, master=None, automation=h)),
    ]
    assert isinstance(levels, mixer.SongLevels) and len(levels.tracks) == 3
    del seq.rendered[:]
    cs.stem(2, 5, 7)                                            # stem stays plain
    assert seq.rendered == [(10, 14, 0, dict(gains=[0.0, 0.0, 1.0]))]
    cs.close()
    for call in _calls(cs, automation=auto):
        with pytest.raises(ValueError, match="closed"):
            call()


def test_the_binding_calls_the_new_entry_point_only_with_an_automation(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(N, "lib", lambda: lib)
    monkeypatch.setattr(N, "ensure_init", lambda: None)
    seq = N.Sequence.__new__(N.Sequence)
    seq._h, seq._sources = C.c_void_p(1), []

    class Out:
        handle = C.c_void_p(2)
    seq.render(5, 6, Out, 7)
    seq.render(5, 6, Out, 7, gains=[1.0, 2.0, 3.0])
    seq.render(5, 6, Out, 7, gains=[1.0, 2.0, 3.0], meters=True)
    seq.render(5, 6, Out, 7, pans=[0.5, 0.25, 1.0, 1.0, 0.0, -1.0], master=0.5)
    seq.render(5, 6, Out, 7, master=0.5, automation=None)
    assert [c[0] for c in lib.calls if c[0] != "sh_seq_get_tracks"] == ["sh_seq_render", "sh_seq_render_gains", "sh_seq_render_meters", "sh_seq_render_desk",
                                                                       "sh_seq_render_desk"]
    del lib.calls[:]
    segments = np.zeros(2, dtype=N.ENV_SEGMENT_DTYPE)
    auto = N.SeqAutomation(seq, segments, [0, 2, 2, 2])
    name, args = lib.calls[-1]
    assert name == "sh_seq_auto_create" and args[0] is seq._h and args[1] == segments.ctypes.data and args[2] == 2 and list(args[3]) == [0, 2, 2, 2] and args[4] == 3
    auto._h = C.c_void_p(9)
    del lib.calls[:]
    assert seq.render(5, 6, Out, 7, automation=auto) is None
    assert seq.render(5, 6, Out, 7, gains=[1.0, 2.0, 3.0], master=0.7, automation=auto) is None
    rows = seq.render(5, 6, Out, 7, gains=[1.0, 2.0, 3.0], pans=[0.5, 0.25, 1.0, 1.0, 0.0, -1.0], master=-1.3, meters=True, automation=auto)
    assert rows == [((0, 0), (0, 0))] * 4
    calls = [c for c in lib.calls if c[0] != "sh_seq_get_tracks"]
    assert [c[0] for c in calls] == ["sh_seq_render_auto"] * 3
    a, b, c = (d[1] for d in calls)
    assert a[1:3] == b[1:3] == c[1:3] == (5, 6) and a[4] == 7 and a[12] is b[12] is c[12] is auto._h
    assert (a[5], a[6], a[7], a[8], a[9], a[10], a[11]) == (None, 0, None, 0, 1.0, None, 0)
    assert (list(b[5]), b[6], b[7], b[8], b[9], b[10], b[11]) == ([1.0, 2.0, 3.0], 3, None, 0, 0.7, None, 0)
    assert (list(c[5]), c[6], list(c[7]), c[8], c[9], len(c[10]), c[11]) == ([1.0, 2.0, 3.0], 3, [0.5, 0.25, 1.0, 1.0, 0.0, -1.0], 6, -1.3, 4, 4)
    auto.free()
    assert lib.calls[-1][0] == "sh_seq_auto_destroy" and not auto._h
    seq.free()


def test_the_new_symbols_are_declared_beside_the_one_they_extend():
    table = N._SIGNATURES
    desk, auto = table["sh_seq_render_desk"][1], table["sh_seq_render_auto"][1]
    assert len(auto) == 13 and auto[:12] == desk and auto[12] == C.c_void_p
    assert table["sh_seq_auto_destroy"][1] == [C.c_void_p] and len(table["sh_seq_auto_create"][1]) == 6
    header = (Path(__file__).resolve().parents[1] / "include" / "synthhip.h").read_text()
    for name in ("int sh_seq_auto_create(", "int sh_seq_auto_destroy(", "int sh_seq_render_auto("):
        assert name in header
    assert "#define SH_ABI_VERSION 6" in header and N.SH_ABI_VERSION == 6      # new symbols only: no struct changed


# ---- the reference expression ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("width", [1, 2, 4])
def test_the_expression_is_the_oracles_fade_and_refsamples_fadein_and_fadeout(width):
    rng = np.random.default_rng(70 + width)
    dtype = {1: np.int8, 2: "<i2", 4: "<i4"}[width]
    for nch in (1, 2):
        for frames in (1, 2, 7, 100, 1000):
            assert int(RATE * (frames / RATE)) == frames               # (the fades below cover the whole clip)
            n = frames * nch
            v = _clip(rng, width, n)
            data = v.astype(dtype).tobytes()
            for v0, v1 in [(0.0, 1.0), (1.0, 0.0), (0.25, 0.9), (0.9, 0.1), (0.37, 0.37), (0.0, 0.0), (1.0, 1.0), (float(rng.uniform()), float(rng.uniform()))]:
                got = np.asarray(_piece(v.tolist(), n, v0, v1), dtype=np.int64).astype(dtype).tobytes()
                assert got == pcm_oracle.fade(data, width, False, v1 - v0, v0), (width, nch, frames, v0, v1)
                if v1 == 1.0:                                   # Sample.fadein(seconds, v0) of the clip: the whole clip is the fade
                    assert got == RefSample(data, width, RATE, nch).fadein(frames / RATE + 1.0, v0).frames
                if v0 == 1.0:                                   # Sample.fadeout(seconds, v1): 1.0 - k * decrease / n is the same double
                    assert got == RefSample(data, width, RATE, nch).fadeout(frames / RATE + 1.0, v1).frames
                    assert got == pcm_oracle.fade(data, width, True, 1.0 - v1, 0.0)


def test_the_factor_stays_between_its_volumes_and_the_result_inside_the_width():
    """float64 arrays: numpy's elementwise IEEE arithmetic is Python's float arithmetic, operation for operation"""
    rng = np.random.default_rng(2024)
    count = 200000
    sizes = np.array([1, 2, 3, 7, 1000, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 5, 2 ** 32 - 65536 - 1, 2 ** 32 - 65536], dtype=np.int64)
    n = np.where(np.arange(count) % 3 == 0, rng.integers(1, 2 ** 32 - 65536, count), sizes[np.arange(count) % len(sizes)])
    k = np.choose(np.arange(count) % 4, [np.zeros(count, dtype=np.int64), n - 1, n // 2, (rng.uniform(size=count) * n).astype(np.int64)])
    assert ((0 <= k) & (k < n)).all() and n.max() == 2 ** 32 - 65536 and (n >= 2 ** 32 - 65536 - 1).sum() > 1000

    def volumes():
        u = rng.uniform(size=count)
        return np.choose(rng.integers(0, 5, count), [np.zeros(count), np.ones(count), u, u * 1e-9, 1.0 - u * 1e-12])
    v0, v1 = volumes(), volumes()
    nf = n.astype(np.float64)                                   # numsamples, a float
    f = k.astype(np.float64) * (v1 - v0) / nf + v0
    assert ((np.minimum(v0, v1) <= f) & (f <= np.maximum(v0, v1))).all()
    for i in range(0, count, 997):                              # and Python's own floats agree with the arrays
        assert int(k[i]) * (float(v1[i]) - float(v0[i])) / float(int(n[i])) + float(v0[i]) == float(f[i])
    for width in (1, 2, 4):
        top = float(1 << (8 * width - 1))
        for x in (-top, top - 1.0):
            y = np.trunc(x * f)
            assert ((-top <= y) & (y <= top - 1.0)).all()
    # the fade-out form is the same double: negation is exact
    t = rng.uniform(size=count)
    assert (1.0 - k.astype(np.float64) * (1.0 - t) / nf == k.astype(np.float64) * (t - 1.0) / nf + 1.0).all()
    assert math.isfinite(float(f.max()))
