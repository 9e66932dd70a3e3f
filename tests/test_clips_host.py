"""What the overs of a compiled song's level history -- ``clips=True`` on ``CompiledSequence.render``, ``render_into`` and ``chunks``,
``Levels.clipped``, ``SongHistory.clipped()`` -- need of the host alone (no GPU; the fake native layer of tests/songhost.py): what
is refused before a launch, that ``clips=False`` hands on exactly the keywords there were, which entry point the binding reaches, and the
arithmetic of ``SongHistory`` with counts (``total``, ``fold``, ``clipped()``, ``Levels`` equality with and without counts).  The counts
themselves: tests/test_gpu_clips.py."""
import ctypes as C
import random
from pathlib import Path

import numpy as np
import pytest

from synthesizer_amd import _native as N
from synthesizer_amd import mixer
from tests.songhost import RATE, _Auto, _calls, _ClipSeq, _fake, _Lib, _mono, _stereo
from tests.test_history_host import hand_made


def _song(monkeypatch, nch=2):
    _fake(monkeypatch)
    monkeypatch.setattr(N, "Sequence", _ClipSeq)
    monkeypatch.setattr(N, "SeqAutomation", _Auto)
    del _Auto.made[:]
    a = _stereo(1000) if nch == 2 else _mono(1000)
    return mixer.compile_tracks([[(0.0, a), (0.5, a, 0.5)], [], [(0.25, a)]], RATE, nch)


# ---- what is refused before a launch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meters", [False, True])
def test_clips_need_a_history(monkeypatch, meters):
    cs = _song(monkeypatch)
    for call in _calls(cs, clips=True, meters=meters) + _calls(cs, clips=True, meters=meters, gains=(1.0, 0.5, 1.0), master=0.5):
        with pytest.raises(ValueError, match="CompiledSequence: clips=True counts the overs per block of a level history: it needs meters=\"history\""):
            call()
    assert cs._seq.rendered == []
    for bad in ("History", 1, None):                            # the meters= message keeps its wording
        for call in _calls(cs, clips=True, meters=bad):
            with pytest.raises(ValueError, match="CompiledSequence: meters is True, False or \"history\""):
                call()
    assert cs._seq.rendered == []


def test_a_flat_song_and_odd_blocks_are_refused(monkeypatch):
    _fake(monkeypatch)
    monkeypatch.setattr(N, "Sequence", _ClipSeq)
    flat = mixer.compile_sequence([(0.0, _stereo())], RATE, 2)
    for call in _calls(flat, clips=True, meters="history"):
        with pytest.raises(ValueError, match=r"CompiledSequence: meters need a song of tracks \(compile_tracks\); this one has none"):
            call()
    for call in _calls(flat, clips=True):
        with pytest.raises(ValueError, match="clips=True counts the overs per block of a level history"):
            call()
    assert flat._seq.rendered == []
    from synthesizer_amd.sample import Sample
    three = Sample.from_raw_frames(bytes(2 * 3 * 100), 2, RATE, 3)
    odd = mixer.compile_tracks([[(0.0, three)], []], RATE, 3)
    for call in _calls(odd, clips=True, meters="history"):
        with pytest.raises(ValueError, match="a level history needs blocks of whole frames"):
            call()
    assert odd._seq.rendered == []


def test_overs_through_bus_rides_or_pan_rides_are_not_built(monkeypatch):
    cs = _song(monkeypatch)
    three = [(0, 1, 0.5), (1, 2, 1.0), (2, 3, 0.25)]
    faders = cs.automation([[(0, 100, 0.5, 1.0)], None, None])
    for auto in (cs.automation([None] * 3, master=[(0, 10, 0.5, 1.0)]), cs.automation([None] * 3, groups=[None, [(0, 5, 0.5, 0.5)]]),
                 cs.automation([None] * 3, pans=[[(0, 10, 0.5, -1.0)], None, None]), cs.automation([None] * 3, group_pans=[[(0, 10, 0.5, -1.0)]])):
        for call in _calls(cs, meters="history", clips=True, automation=auto, groups=three):
            with pytest.raises(NotImplementedError, match="CompiledSequence: overs are not counted through rides of buses and pans yet"):
                call()
    assert cs._seq.rendered == []
    _out, h = cs.render(0, 10, meters="history", clips=True, automation=faders, groups=three)      # the tracks' fader moves are fine
    assert isinstance(h, mixer.SongHistory) and cs._seq.rendered[-1][3]["automation"] is _Auto.made[0] and cs._seq.rendered[-1][3]["clips"] is True
    assert h.clipped().shape == (1, 7, 2)


# ---- what each value hands on -----------------------------------------------------------------------------------------------------------
def test_clips_false_hands_on_exactly_the_keywords_there_were(monkeypatch):
    cs = _song(monkeypatch)
    seq = cs._seq
    for kw in ({}, dict(clips=False)):
        del seq.rendered[:]
        cs.render(10, 20, **kw)
        cs.render(10, 20, gains=(0.5, 1.0, 2.0), meters=True, **kw)
        cs.render_into(N.DeviceBuffer(100), 4, 3, 9, master=0.7, meters=True, **kw)
        out, h = cs.render(1000, 3000, gains=(0.5, 1.0, 2.0), meters="history", **kw)
        h2 = cs.render_into(N.DeviceBuffer(100), 4, 3, 9, pans=(0.0, None, None), groups=[(0, 2, 0.5)], meters="history", **kw)
        parts = list(cs.chunks(2500, meters="history", **kw))
        assert seq.rendered == [(20, 40, 0, {}), (20, 40, 0, dict(gains=[0.5, 1.0, 2.0], meters=True)),
                                (6, 18, 2, dict(gains=None, meters=True, pans=None, master=0.7)),
                                (2000, 6000, 0, dict(gains=[0.5, 1.0, 2.0], meters="history")),
                                (6, 18, 2, dict(gains=None, meters="history", pans=[0.5, 0.5, 1.0, 1.0, 1.0, 1.0], master=None, groups=[(0, 2, 0.5, 1.0, 1.0)])),
                                (0, 5000, 0, dict(gains=None, meters="history")), (5000, 5000, 0, dict(gains=None, meters="history"))]
        assert h.clipped() is None and h2.clipped() is None and all(p[1].clipped() is None for p in parts)
        assert all(lv.clipped is None for block in h for lv in block.tracks + [block.master]) and h.total().master.clipped is None


def test_clips_true_hands_on_the_history_keywords_and_clips(monkeypatch):
    cs = _song(monkeypatch)
    seq = cs._seq
    out, h = cs.render(1000, 3000, gains=(0.5, 1.0, 2.0), meters="history", clips=True)
    assert isinstance(out, mixer.Sample) and isinstance(h, mixer.SongHistory) and h.starts == [1000, 1024, 2048, 3072]
    h2 = cs.render_into(N.DeviceBuffer(100), 4, 3, 9, pans=(0.0, None, None), groups=[(0, 2, 0.5)], meters="history", clips=True)
    parts = list(cs.chunks(2500, meters="history", clips=True))
    assert seq.rendered == [(2000, 6000, 0, dict(gains=[0.5, 1.0, 2.0], meters="history", clips=True)),
                            (6, 18, 2, dict(gains=None, meters="history", pans=[0.5, 0.5, 1.0, 1.0, 1.0, 1.0], master=None, groups=[(0, 2, 0.5, 1.0, 1.0)],
                                            clips=True)),
                            (0, 5000, 0, dict(gains=None, meters="history", clips=True)), (5000, 5000, 0, dict(gains=None, meters="history", clips=True))]
    # the counts the fake wrote: 10 * song block + row on the left, 1 on the right
    got = h.clipped()
    assert isinstance(got, np.ndarray) and got.shape == (4, 4, 2) and got[:, :, 0].tolist() == [[10 * b + r for r in range(4)] for b in range(4)]
    assert got[:, :, 1].tolist() == [[1] * 4] * 4
    assert [lv.clipped for lv in h[2].tracks] == [(20, 1), (21, 1), (22, 1)] and h[2].master.clipped == (23, 1)
    assert all(type(v) is int for v in h[2].master.clipped)
    assert h.total().master.clipped == (3 + 13 + 23 + 33, 4) and h.total().tracks[0].clipped == (60, 4)
    assert h2.clipped().shape == (1, 5, 2) and h2[0].groups[0].clipped == (4, 1)
    assert [p[1].clipped().shape for p in parts] == [(3, 4, 2), (3, 4, 2)]
    del seq.rendered[:]
    # an empty window: nothing is launched, a history without blocks that still has counts
    out, e = cs.render(3, 0, meters="history", clips=True)
    assert len(out) == 0 and e.nblocks == 0 and e.clipped().shape == (0, 4, 2) and e.total().master.clipped == (0, 0) and seq.rendered == []
    assert cs.render_into(N.DeviceBuffer(100), 0, 3, 0, meters="history", clips=True).clipped().shape == (0, 4, 2) and seq.rendered == []


def test_the_binding_reaches_the_new_entry_point_for_clips_alone(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(N, "lib", lambda: lib)
    seq = N.Sequence.__new__(N.Sequence)
    seq._h, seq._sources, seq._width = C.c_void_p(1), [], 2

    class Out:
        handle = C.c_void_p(2)
    gains, pans, groups = [1.0, 2.0, 3.0], [0.5, 0.25, 1.0, 1.0, 0.0, -1.0], [(0, 1, 0.5, 1.0, 1.0), (1, 3, 1.0, 0.5, 0.25)]
    a = seq.render(2040, 2060, Out, 7, meters="history")
    b = seq.render(2040, 2060, Out, 7, meters="history", clips=False)
    c = seq.render(2040, 2060, Out, 7, meters="history", clips=True)
    d = seq.render(4096, 2048, Out, 0, gains=gains, pans=pans, master=0.5, groups=groups, meters="history", clips=True)
    e = seq.render(4096, 0, Out, 0, meters="history", clips=True)
    calls = [c_ for c_ in lib.calls if c_[0] != "sh_seq_get_tracks"]
    assert [c_[0] for c_ in calls] == ["sh_seq_render_history"] * 2 + ["sh_seq_render_clips"] * 3
    assert a.dtype == b.dtype == N.SEQ_METER_DTYPE
    for got, shape in ((c, (3, 4)), (d, (1, 6)), (e, (0, 4))):
        assert isinstance(got, np.ndarray) and got.dtype == N.SEQ_METER_CLIPS_DTYPE and got.shape == shape and got.dtype.itemsize == 48
    assert [len(c_[1]) for c_ in calls] == [16] * 5 and calls[2][1][:10] == calls[0][1][:10] and calls[2][1][11:] == calls[0][1][11:]
    assert C.addressof(calls[2][1][10].contents) == c.ctypes.data and isinstance(calls[2][1][10].contents, N.SeqMeterClips)
    args = calls[3][1]
    assert (list(args[5]), args[6], list(args[7]), args[8], args[9], args[11], args[12], args[13], args[15]) == (gains, 3, pans, 6, 0.5, 6, 1, None, 2)
    assert (calls[4][1][10], calls[4][1][11], calls[4][1][12]) == (None, 4, 0)
    del lib.calls[:]
    for meters in (False, True):                                # clips without a history: refused in the binding as well, nothing called
        with pytest.raises(ValueError, match="Sequence.render: clips=True counts per block of a history"):
            seq.render(5, 6, Out, 7, gains=gains, meters=meters, clips=True)
    assert lib.calls == []
    seq.free()


def test_the_new_symbol_is_declared_beside_the_one_it_extends():
    table = N._SIGNATURES
    hist, clips = table["sh_seq_render_history"][1], table["sh_seq_render_clips"][1]
    assert len(clips) == len(hist) == 16 and clips[:10] == hist[:10] and clips[11:] == hist[11:]
    assert clips[10] == C.POINTER(N.SeqMeterClips) and hist[10] == C.POINTER(N.SeqMeter)
    header = (Path(__file__).resolve().parents[1] / "include" / "synthhip.h").read_text()
    assert "int sh_seq_render_clips(" in header and "} sh_seq_meter_clips;" in header and "#define SH_ABI_VERSION 6" in header and N.SH_ABI_VERSION == 6
    assert N.SEQ_METER_CLIPS_DTYPE.itemsize == C.sizeof(N.SeqMeterClips) == 48
    fields = ("peak", "sq_hi", "sq_lo", "clipped")
    assert [N.SEQ_METER_CLIPS_DTYPE.fields[f][1] for f in fields] == [getattr(N.SeqMeterClips, f).offset for f in fields] == [0, 8, 24, 40]
    assert [N.SEQ_METER_CLIPS_DTYPE.fields[f][1] for f in fields[:3]] == [N.SEQ_METER_DTYPE.fields[f][1] for f in fields[:3]]


# ---- SongHistory arithmetic with counts ---------------------------------------------------------------------------------------------------
def counted(nblocks, nrows, seed, mono=False):
    rng = random.Random(seed)
    return [[[rng.choice([0, rng.randrange(1025)]), 0 if mono else rng.randrange(1025)] for _r in range(nrows)] for _b in range(nblocks)]


def test_total_and_fold_add_the_counts():
    bf = 512
    peak, sq = hand_made(9, 4, 4, seed=9)
    clips = counted(9, 4, 21)
    start, end = 5 * bf + 100, 13 * bf + 7
    h = mixer.SongHistory(peak, sq, start // bf, bf, start, end - start, 4, 2, RATE, 1, clipped=clips)
    assert h.clipped().tolist() == clips and h.clipped().shape == (9, 4, 2)
    got = h.clipped()
    got[:] = 0
    assert h.clipped().tolist() == clips                        # a copy, as peaks()
    for j in range(9):
        rows = h[j].tracks + [h[j].master] + h[j].groups
        assert [lv.clipped for lv in rows] == [tuple(clips[j][r]) for r in range(4)] and all(type(v) is int for lv in rows for v in lv.clipped)
    total = h.total()
    assert [lv.clipped for lv in total.tracks + [total.master] + total.groups] == [tuple(sum(clips[b][r][c] for b in range(9)) for c in range(2)) for r in range(4)]
    f = h.fold(4)                                               # song blocks 5 .. 13 by index // 4: [5, 8), [8, 12), [12, 14)
    for k, (a, b) in enumerate([(0, 3), (3, 7), (7, 9)]):
        assert f.clipped()[k].tolist() == [[sum(clips[j][r][c] for j in range(a, b)) for c in range(2)] for r in range(4)]
        assert f[k].master.clipped == tuple(sum(clips[j][2][c] for j in range(a, b)) for c in range(2))
    assert f.total() == h.total() and f.total().master.clipped == h.total().master.clipped
    assert h.fold(2).fold(2).clipped().tolist() == f.clipped().tolist() and h.fold(1000).clipped()[0].tolist() == h.clipped().sum(axis=0).tolist()
    with pytest.raises(ValueError, match="SongHistory: clipped"):
        mixer.SongHistory(peak, sq, start // bf, bf, start, end - start, 4, 2, RATE, 1, clipped=[b[:3] for b in clips])


def test_a_mono_song_has_the_mono_rule_of_peak():
    mpeak, msq = hand_made(3, 4, 2, seed=4, mono=True)
    clips = counted(3, 4, 8, mono=True)
    m = mixer.SongHistory(mpeak, msq, 0, 2048, 0, 3 * 2048, 2, 1, RATE, clipped=clips)
    assert m.clipped()[:, :, 0].tolist() == m.clipped()[:, :, 1].tolist() == [[row[0] for row in block] for block in clips]
    assert m[1].master.clipped == (clips[1][3][0],) * 2 and m.total().master.clipped == (sum(b[3][0] for b in clips),) * 2


def test_levels_compare_counts_only_where_both_sides_have_them():
    a = mixer.Levels((5, 6), (25, 36), 10, 2, 2, RATE)
    b = mixer.Levels((5, 6), (25, 36), 10, 2, 2, RATE, clipped=(3, 0))
    c = mixer.Levels((5, 6), (25, 36), 10, 2, 2, RATE, clipped=(3, 1))
    d = mixer.Levels((5, 6), (25, 36), 10, 2, 2, RATE, clipped=(3, 0))
    assert a.clipped is None and b.clipped == (3, 0) and a == b and b == a and a == c and b == d and b != c and not (b == c) and not (a != b)
    assert mixer.Levels((5, 7), (25, 36), 10, 2, 2, RATE, clipped=(3, 0)) != b and "clipped=(3, 0)" in repr(b) and "clipped" not in repr(a)
    mono = mixer.Levels((5, 0), (25, 0), 10, 2, 1, RATE, clipped=(4, 0))
    assert mono.clipped == (4, 4) and mono.peak == (5, 5)
    # a history with counts against the levels there were: total() == the window's SongLevels, a block seen with and without counts
    peak, sq = hand_made(4, 4, 2, seed=1)
    clips = counted(4, 4, 2)
    with_counts = mixer.SongHistory(peak, sq, 0, 1024, 700, 2800, 2, 2, RATE, clipped=clips)
    without = mixer.SongHistory(peak, sq, 0, 1024, 700, 2800, 2, 2, RATE)
    assert with_counts.total() == without.total() and all(with_counts[j] == without[j] for j in range(4))
    window = mixer.SongLevels([(lv.peak, lv.sum_squares) for lv in without.total().tracks + [without.total().master]], 2800, 2, 2, RATE)
    assert with_counts.total() == window and window == with_counts.total()
    other = mixer.SongHistory(peak, sq, 0, 1024, 700, 2800, 2, 2, RATE, clipped=[[[v + 1 for v in row] for row in block] for block in clips])
    assert with_counts[1] != other[1] and with_counts.total() != other.total()
