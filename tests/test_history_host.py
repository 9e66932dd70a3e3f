"""What the level history of a compiled song of tracks -- ``CompiledSequence.render(meters="history")`` and ``mixer.SongHistory`` -- needs of
the host alone (no GPU; the fakes of tests/songhost.py): ``SongHistory`` built from hand-made
rows against Python integers (indexing, ``starts``, the frames of partial edge blocks, ``total()``, ``fold(n)`` from a window that starts
mid-group, ``peaks()``, a mono song's ``left == right``), the validation of ``meters=``, and which entry points and keywords
``meters=True``, ``meters=False`` and ``meters="history"`` reach.  The levels themselves: tests/test_gpu_history.py."""
import ctypes as C
import random
from pathlib import Path

import numpy as np
import pytest

from synthesizer_amd import _native as N
from synthesizer_amd import mixer
from tests.songhost import RATE, _Auto, _calls, _fake, _Lib, _mono, _Seq, _stereo


# ---- hand-made rows -------------------------------------------------------------------------------------------------------------------
def hand_made(nblocks, nrows, width, seed=0, mono=False):
    """(peak, sum_squares) as nested lists of Python ints, (nblocks, nrows, 2); wide sums pass 2^64"""
    rng = random.Random(seed)
    top = 2 ** (8 * width - 1)
    peak = [[[rng.choice([0, rng.randrange(top + 1)]), 0 if mono else rng.randrange(top + 1)] for _r in range(nrows)] for _b in range(nblocks)]
    sq = [[[p * p * rng.randrange(1, 1024), q * q * rng.randrange(1, 1024)] for p, q in block] for block in peak]
    return peak, sq


def history(peak, sq, start, frames, block_frames=1024, width=2, nch=2, ngroups=0):
    return mixer.SongHistory(peak, sq, start // block_frames, block_frames, start, frames, width, nch, RATE, ngroups)


def rows_of(levels):
    return [(lv.peak, lv.sum_squares, lv.frames) for lv in levels.tracks + [levels.master] + levels.groups]


def test_blocks_index_as_song_levels_with_their_own_frames():
    # frames [700, 3500) in blocks of 1024: block 0 is [700, 1024), then two whole ones, then [3072, 3500)
    peak, sq = hand_made(4, 6, 2, seed=1)
    h = history(peak, sq, 700, 2800, ngroups=2)
    assert (h.nblocks, len(h), h.block_frames, h.start_frame, h.frames) == (4, 4, 1024, 700, 2800)
    assert h.starts == [700, 1024, 2048, 3072] and h.block_counts == [324, 1024, 1024, 428]
    assert h.history is h or len(h.history) == 4
    for j in range(4):
        lv = h.history[j]
        assert isinstance(lv, mixer.SongLevels) and len(lv.tracks) == 3 and len(lv.groups) == 2
        assert rows_of(lv) == [(tuple(peak[j][r]), tuple(sq[j][r]), h.block_counts[j]) for r in range(6)]
        assert all(type(v) is int for row in rows_of(lv) for pair in row[:2] for v in pair)
        assert lv == h[j] and rows_of(h[j - 4]) == rows_of(lv)
    # rms is over the block's own frames: a partial block is not read as a whole one
    assert h[0].master.rms == (int((sq[0][3][0] / 324) ** 0.5), int((sq[0][3][1] / 324) ** 0.5))
    assert h[0].master.duration == 324 / RATE and h[1].master.duration == 1024 / RATE
    assert [lv.master.frames for lv in h] == h.block_counts
    for bad in (4, -5):
        with pytest.raises(IndexError):
            h[bad]


def test_the_blocks_must_be_the_windows():
    peak, sq = hand_made(4, 4, 2)
    for start, frames in ((700, 2300), (700, 3400), (0, 2800), (1024, 2800)):       # three blocks, five, another first block
        with pytest.raises(ValueError, match="SongHistory"):
            mixer.SongHistory(peak, sq, 0, 1024, start, frames, 2, 2, RATE)
    with pytest.raises(ValueError, match="SongHistory"):
        mixer.SongHistory(peak, [b[:3] for b in sq], 0, 1024, 700, 2800, 2, 2, RATE)
    one = history([[[5, 6]] * 4], [[[25, 36]] * 4], 1023, 1)                         # one frame: one block
    assert one.starts == [1023] and one.block_counts == [1] and one[0].master.frames == 1
    whole = history([[[5, 6]] * 4], [[[25, 36]] * 4], 1024, 1024)                    # exactly one block
    assert whole.starts == [1024] and whole.block_counts == [1024]


@pytest.mark.parametrize("width", [2, 4])
def test_the_total_is_the_fold_of_all_blocks_in_python_integers(width):
    peak, sq = hand_made(7, 5, width, seed=width)
    h = history(peak, sq, 300, 6 * 1024 + 50, width=width, ngroups=1)
    assert h.nblocks == 7 and h.block_counts[0] == 724 and h.block_counts[-1] == 350
    total = h.total()
    assert isinstance(total, mixer.SongLevels)
    want = [(tuple(max(peak[b][r][c] for b in range(7)) for c in range(2)), tuple(sum(sq[b][r][c] for b in range(7)) for c in range(2)), 6 * 1024 + 50)
            for r in range(5)]
    assert rows_of(total) == want
    if width == 4:
        assert max(v for row in want for v in row[1]) > 2 ** 64, "no sum passes 2^64"
    # == what a metered render of the window hands back: a SongLevels of the same rows and the window's frames
    same = mixer.SongLevels([(p, s) for p, s, _f in want], 6 * 1024 + 50, width, 2, RATE, 1)
    other = mixer.SongLevels([(p, s) for p, s, _f in want], 6 * 1024 + 49, width, 2, RATE, 1)
    assert total == same and not (total != same) and total != other and total != object()


def test_fold_merges_by_song_block_index_from_a_window_that_starts_mid_group():
    # song blocks 5 .. 13 (nine of them, the first and the last partial); fold(4) merges by index // 4: [5, 8), [8, 12), [12, 14)
    bf = 512
    peak, sq = hand_made(9, 4, 4, seed=9)
    start, end = 5 * bf + 100, 13 * bf + 7
    h = history(peak, sq, start, end - start, block_frames=bf, width=4)
    assert h.first_block == 5 and h.nblocks == 9
    f = h.fold(4)
    assert isinstance(f, mixer.SongHistory) and (f.block_frames, f.first_block, f.nblocks, f.start_frame, f.frames) == (4 * bf, 1, 3, start, end - start)
    groups = [(0, 3), (3, 7), (7, 9)]
    assert f.starts == [start, 8 * bf, 12 * bf] and f.block_counts == [8 * bf - start, 4 * bf, end - 12 * bf]
    for k, (a, b) in enumerate(groups):
        want = [(tuple(max(peak[j][r][c] for j in range(a, b)) for c in range(2)), tuple(sum(sq[j][r][c] for j in range(a, b)) for c in range(2)),
                 sum(h.block_counts[a:b])) for r in range(4)]
        assert rows_of(f[k]) == want
        assert all(type(v) is int for row in rows_of(f[k]) for v in row[1])
    assert f.total() == h.total() and f.fold(1).starts == f.starts
    # the same song blocks from a window that starts a block later: the coarse blocks both hold whole read the same
    g = history(peak[1:], sq[1:], 6 * bf, end - 6 * bf, block_frames=bf, width=4).fold(4)
    assert g.first_block == 1 and g.nblocks == 3 and rows_of(g[1]) == rows_of(f[1]) and rows_of(g[2]) == rows_of(f[2]) and rows_of(g[0]) != rows_of(f[0])
    # fold of a fold is the fold: 2 then 2 against 4, where the groups nest
    assert [rows_of(x) for x in h.fold(2).fold(2)] == [rows_of(x) for x in f]
    everything = h.fold(1000)
    assert everything.nblocks == 1 and everything[0] == h.total()
    for bad in (0, -1):
        with pytest.raises(ValueError, match="SongHistory: fold"):
            h.fold(bad)
    with pytest.raises(TypeError):
        h.fold(2.0)


def test_peaks_for_drawing_and_a_mono_song():
    peak, sq = hand_made(3, 4, 2, seed=3)
    h = history(peak, sq, 0, 3 * 1024)
    p = h.peaks()
    assert isinstance(p, np.ndarray) and p.shape == (3, 4, 2) and p.tolist() == peak
    p[:] = 0
    assert h.peaks().tolist() == peak                           # a copy: drawing code may scale it
    mpeak, msq = hand_made(3, 4, 2, seed=4, mono=True)
    m = history(mpeak, msq, 0, 3 * 2048, block_frames=2048, nch=1)
    assert all(row[1] == 0 for block in mpeak for row in block)
    assert m.peaks()[:, :, 0].tolist() == m.peaks()[:, :, 1].tolist() == [[row[0] for row in block] for block in mpeak]
    for j in range(3):
        for lv, row, s in zip(m[j].tracks + [m[j].master], mpeak[j], msq[j]):
            assert lv.peak == (row[0], row[0]) and lv.sum_squares == (s[0], s[0]) and lv.frames == 2048      # left == right, as Sample has it
    assert m.total().master.peak[0] == m.total().master.peak[1] == max(block[3][0] for block in mpeak)


def test_an_empty_history_reads_zero():
    h = mixer.SongHistory.from_blocks(None, 4, 2048, 77, 0, 2, 2, RATE)
    assert (h.nblocks, h.starts, h.block_counts, list(h)) == (0, [], [], []) and h.peaks().shape == (0, 4, 2)
    assert h.total() == mixer.SongLevels([((0, 0), (0, 0))] * 4, 0, 2, 2, RATE) and h.fold(3).nblocks == 0


def test_from_blocks_forms_the_sums_in_python_integers():
    blocks = np.zeros((2, 4), dtype=N.SEQ_METER_DTYPE)
    blocks["peak"][1, 3] = (2 ** 31, 7)
    blocks["sq_hi"][1, 3] = (2 ** 41, 1)
    blocks["sq_lo"][1, 3] = (2 ** 43 + 5, 2 ** 33)
    blocks["sq_hi"][0, 3] = (2 ** 41, 0)
    h = mixer.SongHistory.from_blocks(blocks, 4, 1024, 512 - 10, 20, 4, 2, RATE)
    assert h.block_frames == 512 and h.starts == [502, 512] and h.block_counts == [10, 10]
    assert h[1].master.peak == (2 ** 31, 7) and h[1].master.sum_squares == ((2 ** 41 << 32) + 2 ** 43 + 5, (1 << 32) + 2 ** 33)
    assert h.total().master.sum_squares[0] == (2 ** 42 << 32) + 2 ** 43 + 5 > 2 ** 64


# ---- meters= ------------------------------------------------------------------------------------------------------------------------------
class _HistSeq(_Seq):
    """tests/songhost._Seq, whose history is the array N.Sequence.render hands back: one row set per song tile of the window"""

    def render(self, first_sample, nsamples, out, out_sample=0, **kw):
        if kw.get("meters") == "history":
            self.rendered.append((first_sample, nsamples, out_sample, kw))
            nblocks = (first_sample + nsamples - 1) // 2048 - first_sample // 2048 + 1
            blocks = np.zeros((nblocks, 4 + len(kw.get("groups") or ())), dtype=N.SEQ_METER_DTYPE)
            blocks["peak"][:, :, 0] = np.arange(nblocks)[:, None] + first_sample // 2048
            return blocks
        return _Seq.render(self, first_sample, nsamples, out, out_sample, **kw)


def _song(monkeypatch, nch=2):
    _fake(monkeypatch)
    monkeypatch.setattr(N, "Sequence", _HistSeq)
    monkeypatch.setattr(N, "SeqAutomation", _Auto)
    del _Auto.made[:]
    a = _stereo(1000) if nch == 2 else _mono(1000)
    return mixer.compile_tracks([[(0.0, a), (0.5, a, 0.5)], [], [(0.25, a)]], RATE, nch)


@pytest.mark.parametrize("bad", ["History", "true", "", 1, 0, 2, None, 1.0, b"history", ("history",), np.True_])
def test_meters_is_a_bool_or_the_word_history(monkeypatch, bad):
    cs = _song(monkeypatch)
    for call in _calls(cs, meters=bad) + _calls(cs, meters=bad, gains=(1.0, 0.5, 1.0), master=0.5):
        with pytest.raises(ValueError, match="CompiledSequence: meters is True, False or \"history\""):
            call()
    assert cs._seq.rendered == []


def test_a_history_needs_tracks_and_blocks_of_whole_frames(monkeypatch):
    _fake(monkeypatch)
    monkeypatch.setattr(N, "Sequence", _HistSeq)
    flat = mixer.compile_sequence([(0.0, _stereo())], RATE, 2)
    for call in _calls(flat, meters="history"):
        with pytest.raises(ValueError, match=r"CompiledSequence: meters need a song of tracks \(compile_tracks\); this one has none"):
            call()
    assert flat._seq.rendered == []
    from synthesizer_amd.sample import Sample
    three = Sample.from_raw_frames(bytes(2 * 3 * 100), 2, RATE, 3)
    odd = mixer.compile_tracks([[(0.0, three)], []], RATE, 3)
    for call in _calls(odd, meters="history"):
        with pytest.raises(ValueError, match="CompiledSequence: a level history needs blocks of whole frames: 3 channels do not divide a block of 2048 samples"):
            call()
    assert odd._seq.rendered == []
    odd.render(0, 10, meters=True)                              # the meters there were take any channel count
    assert odd._seq.rendered == [(0, 30, 0, dict(gains=None, meters=True))]
    cs = _song(monkeypatch)
    for bad, message in (((1.0, 2.0), "2 gains for 3 tracks"), ((1.0, float("nan"), 1.0), "gain 1 is not finite")):
        for call in _calls(cs, meters="history", gains=bad):       # and everything render already refuses
            with pytest.raises(ValueError, match="CompiledSequence: " + message):
                call()
    with pytest.raises(ValueError, match="outside the song's 5000 frames"):
        cs.render(4000, 1001, meters="history")
    assert cs._seq.rendered == []
    cs.close()
    for call in _calls(cs, meters="history"):
        with pytest.raises(ValueError, match="closed"):
            call()


def test_a_history_with_bus_rides_or_pan_rides_is_not_built(monkeypatch):
    cs = _song(monkeypatch)
    three = [(0, 1, 0.5), (1, 2, 1.0), (2, 3, 0.25)]
    faders = cs.automation([[(0, 100, 0.5, 1.0)], None, None])
    for auto in (cs.automation([None] * 3, master=[(0, 10, 0.5, 1.0)]), cs.automation([None] * 3, groups=[None, [(0, 5, 0.5, 0.5)]]),
                 cs.automation([None] * 3, pans=[[(0, 10, 0.5, -1.0)], None, None]), cs.automation([None] * 3, group_pans=[[(0, 10, 0.5, -1.0)]])):
        for call in _calls(cs, meters="history", automation=auto, groups=three):
            with pytest.raises(NotImplementedError, match="CompiledSequence: rides of buses and pans have no level history yet"):
                call()
        cs.render(0, 10, meters=True, automation=auto, groups=three)      # the meters there were take them
    assert [r[3]["meters"] for r in cs._seq.rendered] == [True] * 4
    del cs._seq.rendered[:]
    _out, h = cs.render(0, 10, meters="history", automation=faders, groups=three)      # fader moves of the tracks have a history
    assert isinstance(h, mixer.SongHistory) and cs._seq.rendered[-1][3]["automation"] is _Auto.made[0] and len(h[0].groups) == 3


def test_what_each_value_of_meters_hands_on(monkeypatch):
    cs = _song(monkeypatch)
    seq = cs._seq
    assert cs.frames == 5000
    # False and True: the calls and keywords of the parent commit
    assert isinstance(cs.render(10, 20), mixer.Sample) and isinstance(cs.render(10, 20, meters=False), mixer.Sample)
    out, levels = cs.render(10, 20, gains=(0.5, 1.0, 2.0), meters=True)
    assert isinstance(levels, mixer.SongLevels) and not isinstance(levels, mixer.SongHistory)
    assert cs.render_into(N.DeviceBuffer(100), 4, 3, 9, meters=False) is None
    assert isinstance(cs.render_into(N.DeviceBuffer(100), 4, 3, 9, master=0.7, meters=True), mixer.SongLevels)
    pairs = list(cs.chunks(4999, meters=True))
    assert seq.rendered == [(20, 40, 0, {}), (20, 40, 0, {}), (20, 40, 0, dict(gains=[0.5, 1.0, 2.0], meters=True)), (6, 18, 2, {}),
                            (6, 18, 2, dict(gains=None, meters=True, pans=None, master=0.7)), (0, 9998, 0, dict(gains=None, meters=True)),
                            (9998, 2, 0, dict(gains=None, meters=True))]
    assert [type(lv) for _s, lv in pairs] == [mixer.SongLevels] * 2
    del seq.rendered[:]
    # "history": the same keywords with meters="history", a SongHistory back
    out, h = cs.render(1000, 3000, gains=(0.5, 1.0, 2.0), meters="history")
    assert isinstance(out, mixer.Sample) and isinstance(h, mixer.SongHistory)
    assert (h.block_frames, h.start_frame, h.frames, h.nblocks, h.starts) == (1024, 1000, 3000, 4, [1000, 1024, 2048, 3072])
    assert [lv.tracks[0].peak[0] for lv in h] == [0, 1, 2, 3] and [lv.master.frames for lv in h] == [24, 1024, 1024, 928]
    h2 = cs.render_into(N.DeviceBuffer(100), 4, 3, 9, pans=(0.0, None, None), groups=[(0, 2, 0.5)], meters="history")
    assert isinstance(h2, mixer.SongHistory) and h2.nblocks == 1 and len(h2[0].groups) == 1 and h2.peaks().shape == (1, 5, 2)
    parts = list(cs.chunks(2500, meters="history"))
    assert [type(p[1]) for p in parts] == [mixer.SongHistory] * 2 and [p[1].starts for p in parts] == [[0, 1024, 2048], [2500, 3072, 4096]]
    assert seq.rendered == [(2000, 6000, 0, dict(gains=[0.5, 1.0, 2.0], meters="history")),
                            (6, 18, 2, dict(gains=None, meters="history", pans=[0.5, 0.5, 1.0, 1.0, 1.0, 1.0], master=None, groups=[(0, 2, 0.5, 1.0, 1.0)])),
                            (0, 5000, 0, dict(gains=None, meters="history")), (5000, 5000, 0, dict(gains=None, meters="history"))]
    del seq.rendered[:]
    # an empty window: nothing is launched, a history without blocks
    out, h = cs.render(3, 0, meters="history")
    assert len(out) == 0 and isinstance(h, mixer.SongHistory) and h.nblocks == 0 and h.total() == cs.render(3, 0, meters=True)[1]
    assert cs.render_into(N.DeviceBuffer(100), 0, 3, 0, meters="history").nblocks == 0 and seq.rendered == []


def test_the_binding_reaches_the_new_entry_point_for_a_history_alone(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(N, "lib", lambda: lib)
    seq = N.Sequence.__new__(N.Sequence)
    seq._h, seq._sources, seq._width = C.c_void_p(1), [], 2

    class Out:
        handle = C.c_void_p(2)
    gains, pans, groups = [1.0, 2.0, 3.0], [0.5, 0.25, 1.0, 1.0, 0.0, -1.0], [(0, 1, 0.5, 1.0, 1.0), (1, 3, 1.0, 0.5, 0.25)]
    # False and True: the entry points of the parent commit, with its arguments
    seq.render(5, 6, Out, 7)
    seq.render(5, 6, Out, 7, gains=gains)
    seq.render(5, 6, Out, 7, gains=gains, meters=True)
    seq.render(5, 6, Out, 7, gains=gains, pans=pans, master=-1.3, meters=True)
    seq.render(5, 6, Out, 7, gains=gains, pans=pans, master=-1.3, meters=False)
    seq.render(5, 6, Out, 7, master=0.5, groups=groups, meters=True)
    seq.render(5, 6, Out, 7, master=0.5, groups=groups)
    calls = [c for c in lib.calls if c[0] != "sh_seq_get_tracks"]
    assert [c[0] for c in calls] == ["sh_seq_render", "sh_seq_render_gains", "sh_seq_render_meters", "sh_seq_render_desk", "sh_seq_render_desk",
                                     "sh_seq_render_groups", "sh_seq_render_groups"]
    assert len(calls[2][1]) == 9 and len(calls[2][1][7]) == 4 and calls[2][1][8] == 4
    assert (len(calls[3][1][10]), calls[3][1][11], calls[4][1][10], calls[4][1][11]) == (4, 4, None, 0)
    assert (len(calls[5][1][10]), calls[5][1][11], calls[6][1][10], calls[6][1][11]) == (6, 6, None, 0)
    del lib.calls[:]
    # "history": the new one, and only it, whatever else the render names
    a = seq.render(2040, 2060, Out, 7, meters="history")                            # samples [2040, 4100): tiles 0, 1 and 2
    b = seq.render(5, 6, Out, 7, gains=gains, pans=pans, master=-1.3, meters="history")
    c = seq.render(4096, 2048, Out, 0, master=0.5, groups=groups, meters="history")
    d = seq.render(4096, 0, Out, 0, meters="history")                               # an empty window: no block, NULL rows
    calls = [c_ for c_ in lib.calls if c_[0] != "sh_seq_get_tracks"]
    assert [c_[0] for c_ in calls] == ["sh_seq_render_history"] * 4
    for got, shape in ((a, (3, 4)), (b, (1, 4)), (c, (1, 6)), (d, (0, 4))):
        assert isinstance(got, np.ndarray) and got.dtype == N.SEQ_METER_DTYPE and got.shape == shape
    args = calls[0][1]
    assert len(args) == 16 and args[0] is seq._h and args[1:3] == (2040, 2060) and args[4] == 7
    assert (args[5], args[6], args[7], args[8], args[9]) == (None, 0, None, 0, 1.0) and (args[11], args[12]) == (4, 3) and args[13:] == (None, None, 0)
    assert C.addressof(args[10].contents) == a.ctypes.data
    args = calls[1][1]
    assert (list(args[5]), args[6], list(args[7]), args[8], args[9], args[11], args[12]) == (gains, 3, pans, 6, -1.3, 4, 1) and args[13:] == (None, None, 0)
    args = calls[2][1]
    assert (args[9], args[11], args[12], args[13], args[15]) == (0.5, 6, 1, None, 2) and [(g.first, g.end, g.gain, g.left, g.right) for g in args[14]] == groups
    assert (calls[3][1][10], calls[3][1][11], calls[3][1][12]) == (None, 4, 0)
    for bad in ("History", 1, None, 0.0):
        with pytest.raises(ValueError, match="Sequence.render: meters is True, False or \"history\""):
            seq.render(5, 6, Out, 7, meters=bad)
    assert [c_ for c_ in lib.calls if c_[0] != "sh_seq_get_tracks"] == calls
    seq.free()


def test_the_new_symbol_is_declared_beside_the_one_it_extends():
    table = N._SIGNATURES
    groups, hist = table["sh_seq_render_groups"][1], table["sh_seq_render_history"][1]
    assert len(hist) == len(groups) + 1 == 16 and hist[:12] == groups[:12] and hist[12] == C.c_uint32 and hist[13:] == groups[12:]
    header = (Path(__file__).resolve().parents[1] / "include" / "synthhip.h").read_text()
    assert "int sh_seq_render_history(" in header and "#define SH_ABI_VERSION 6" in header and N.SH_ABI_VERSION == 6      # a new symbol only
    assert N.SEQ_TILE_SAMPLES == {1: 1024, 2: 2048, 3: 1024, 4: 1024} and N.SEQ_METER_DTYPE.itemsize == C.sizeof(N.SeqMeter) == 40
    assert [N.SEQ_METER_DTYPE.fields[f][1] for f in ("peak", "sq_hi", "sq_lo")] == [N.SeqMeter.peak.offset, N.SeqMeter.sq_hi.offset, N.SeqMeter.sq_lo.offset]
