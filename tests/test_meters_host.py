"""What the level meters of a song of tracks -- ``CompiledSequence.render(..., meters=True)``, ``mixer.Levels`` / ``SongLevels`` -- need of
the host alone (no GPU): the ``ValueError``s raised before anything is launched, what ``render`` hands on to the handle, and the
arithmetic of ``Levels`` against ``audioop`` and ``Sample``'s own formulas restated here.  csrc/seqmeter.hpp: tests/test_seqmeter.py."""
import audioop
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest

from synthesizer_amd import _native as N
from synthesizer_amd import mixer
from tests.songhost import RATE, _fake, _mono


class _Seq:
    """N.Sequence's face, with rows that say which call made them"""

    def __init__(self, sources, table, segments, width, nchannels, track_samples, track_first=None):
        self.ntracks = 0 if track_first is None else len(track_first) - 1
        self.rendered = []

    def info(self):
        return {"level": 0, "device_bytes": 0}

    def render(self, first_sample, nsamples, out, out_sample=0, gains=None, meters=False):
        self.rendered.append((first_sample, nsamples, out_sample, gains, meters))
        if meters:
            return [((100 + t, 7), (1000 * (t + 1) * nsamples, 5)) for t in range(self.ntracks + 1)]

    def free(self):
        pass


def _song(monkeypatch, nch=1):
    _fake(monkeypatch)
    monkeypatch.setattr(N, "Sequence", _Seq)
    a = _mono(1000)
    pan = (1.0, 0.5) if nch == 2 else None
    tracks = [[(0.0, a, None, None, None, pan)], [], [(0.25, a, 0.5, None, None, pan)]]
    return mixer.compile_tracks(tracks, RATE, nch), mixer.compile_sequence([(0.0, a, None, None, None, pan)], RATE, nch)


def test_meters_on_a_song_without_tracks_are_refused_before_anything_is_launched(monkeypatch):
    cs, flat = _song(monkeypatch)
    for call in (lambda: flat.render(meters=True), lambda: flat.render(3, 4, meters=True), lambda: next(flat.chunks(10, meters=True)),
                 lambda: flat.render_into(N.DeviceBuffer(100), 0, 0, 10, meters=True)):
        with pytest.raises(ValueError, match=r"CompiledSequence: meters need a song of tracks \(compile_tracks\); this one has none"):
            call()
    assert flat._seq.rendered == []
    flat.render(3, 4)                                                      # and without the keyword it is what it was
    assert flat._seq.rendered == [(3, 4, 0, None, False)]


def test_every_other_refusal_still_comes_first_and_launches_nothing(monkeypatch):
    cs, flat = _song(monkeypatch)
    nan = float("nan")
    for bad, message in (((1.0, 1.0), "2 gains for 3 tracks"), ((1.0, nan, 1.0), "gain 1 is not finite"), (0.5, "gains is a sequence of numbers")):
        with pytest.raises(ValueError, match="CompiledSequence: " + message):
            cs.render(gains=bad, meters=True)
        with pytest.raises(ValueError, match="CompiledSequence: " + message):
            next(cs.chunks(100, gains=bad, meters=True))
    with pytest.raises(ValueError, match="outside the song's"):
        cs.render(cs.frames + 1, 1, meters=True)
    with pytest.raises(ValueError, match="outside the song's"):
        cs.render_into(N.DeviceBuffer(100), 0, 0, cs.frames + 1, meters=True)
    with pytest.raises(ValueError, match="byte_offset 1 is not a whole number"):
        cs.render_into(N.DeviceBuffer(100), 1, 0, 10, meters=True)
    assert cs._seq.rendered == []
    cs.close()
    with pytest.raises(ValueError, match="closed"):
        cs.render(meters=True)


def test_what_a_metered_render_hands_on_and_returns(monkeypatch):
    cs, _flat = _song(monkeypatch)
    seq = cs._seq
    out, lv = cs.render(10, 20, gains=[0.5, 1, np.float32(2.0)], meters=True)
    assert len(out) == 20 and isinstance(lv, mixer.SongLevels) and len(lv.tracks) == 3 and isinstance(lv.master, mixer.Levels)
    assert [t.peak for t in lv.tracks] == [(100, 100), (101, 101), (102, 102)] and lv.master.peak == (103, 103)       # a mono song: left == right
    assert [t.sum_squares for t in lv.tracks] == [(20000, 20000), (40000, 40000), (60000, 60000)] and lv.master.frames == 20
    got = cs.render_into(N.DeviceBuffer(100), 4, 3, 9, meters=True)
    assert isinstance(got, mixer.SongLevels) and got.master.sum_squares == (36000, 36000)
    assert cs.render_into(N.DeviceBuffer(100), 4, 3, 9) is None            # today's path returns what it returned
    pairs = list(cs.chunks(cs.frames - 1, gains=(1.0, 0.0, 1.0), meters=True))
    assert [(len(s), l.master.frames) for s, l in pairs] == [(cs.frames - 1, cs.frames - 1), (1, 1)]
    assert seq.rendered == [(10, 20, 0, [0.5, 1.0, 2.0], True), (3, 9, 2, None, True), (3, 9, 2, None, False),
                            (0, cs.frames - 1, 0, [1.0, 0.0, 1.0], True), (cs.frames - 1, 1, 0, [1.0, 0.0, 1.0], True)]
    # an empty window launches nothing and reads zero everywhere
    out, lv = cs.render(5, 0, meters=True)
    assert len(out) == 0 and len(seq.rendered) == 5 and len(lv.tracks) == 3
    for row in lv.tracks + [lv.master]:
        assert row.peak == row.sum_squares == row.rms == (0, 0) and row.level_db_peak == row.level_db_rms == (-60.0, -60.0)


def test_a_stereo_song_keeps_its_channels_apart(monkeypatch):
    cs, _flat = _song(monkeypatch, nch=2)
    _out, lv = cs.render(0, 50, meters=True)
    assert lv.tracks[1].peak == (101, 7) and lv.tracks[1].sum_squares == (200000, 5) and lv.master.nchannels == 2


def _db(v, width):
    return max(20.0 * math.log((v + 1) / 2 ** (8 * width - 1), 10), -60.0)      # Sample.__db_level's formula, restated


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_the_arithmetic_of_levels_is_audioops_and_samples(width):
    rng = np.random.default_rng(width)
    top = 2 ** (8 * width - 1)
    frames = 333
    x = rng.integers(-top // 3, top // 3, size=2 * frames).astype(np.int64)
    x[4] = -top                                                            # a full-scale sample on the left
    left, right = x[0::2], x[1::2]
    sq = (sum(int(v) ** 2 for v in left), sum(int(v) ** 2 for v in right))
    lv = mixer.Levels((int(np.abs(left).max()), int(np.abs(right).max())), sq, frames, width, 2, RATE)
    assert lv.peak == (top, int(np.abs(right).max())) and lv.sum_squares == sq and all(type(v) is int for v in lv.sum_squares)
    assert lv.rms == (int(math.sqrt(sq[0] / frames)), int(math.sqrt(sq[1] / frames)))
    if width != 3:                                                         # and audioop says the same of the bytes (its sums are exact here: < 2^53)
        dt = {1: np.int8, 2: "<i2", 4: "<i4"}[width]
        raw_l, raw_r = left.astype(dt).tobytes(), right.astype(dt).tobytes()
        if max(sq) < 2 ** 53:
            assert lv.rms == (audioop.rms(raw_l, width), audioop.rms(raw_r, width))
        assert lv.peak == (audioop.max(raw_l, width), audioop.max(raw_r, width))
    assert lv.level_db_peak == (_db(lv.peak[0], width), _db(lv.peak[1], width)) and lv.level_db_peak[0] > 0.0          # (2^(8w-1) + 1) / 2^(8w-1)
    assert lv.level_db_rms == (_db(lv.rms[0], width), _db(lv.rms[1], width))
    assert lv.duration == frames / RATE


def test_the_floor_at_minus_sixty_and_mono(monkeypatch):
    quiet = mixer.Levels((3, 0), (9, 0), 100, 2, 2, RATE)
    assert quiet.level_db_peak == (-60.0, -60.0) and quiet.level_db_rms == (-60.0, -60.0) and quiet.rms == (0, 0)
    at = mixer.Levels((32, 0), (32 * 32 * 100, 0), 100, 2, 2, RATE)       # (32 + 1) / 32768: just above the floor, and the right channel on it
    assert at.level_db_peak[0] == pytest.approx(20 * math.log10(33 / 32768)) and at.level_db_peak[0] > -60.0 and at.level_db_peak[1] == -60.0
    assert at.rms == (32, 0)
    mono = mixer.Levels((1234, 0), (5 * 1234 ** 2, 0), 5, 2, 1, RATE)     # a mono song: the second channel of its row reads 0
    assert mono.peak == (1234, 1234) and mono.rms == (1234, 1234) and mono.level_db_peak[0] == mono.level_db_peak[1] == _db(1234, 2)
    assert mono.sum_squares == (5 * 1234 ** 2,) * 2
    empty = mixer.Levels((0, 0), (0, 0), 0, 2, 1, RATE)
    assert empty.rms == (0, 0) and empty.level_db_rms == (-60.0, -60.0)
    big = mixer.Levels((2 ** 31, 0), (5 * 2 ** 62, 0), 5, 4, 1, RATE)     # past 2^64: Python ints carry it
    assert big.rms == (2 ** 31, 2 ** 31) and big.level_db_peak[0] == _db(2 ** 31, 4) > 0.0


def test_song_levels_feed_a_level_meter():
    from synthesizer_amd.sample import LevelMeter
    lv = mixer.SongLevels([((20000, 10), (8000 * 20000 ** 2, 800)), ((30000, 10), (8000 * 30000 ** 2, 800))], 8000, 2, 2, 8000)
    meter = LevelMeter(rms_mode=False)
    left, peak_left, right, peak_right = meter.update(lv.master)
    assert (left, right) == lv.master.level_db_peak and peak_left == left and right == -60.0 + 0.0
    assert meter._time == 1.0


def test_the_new_symbol_is_declared_beside_the_ones_it_extends():
    table = N._SIGNATURES
    assert len(table["sh_seq_render_meters"][1]) == 9 and table["sh_seq_render_meters"][1][:7] == table["sh_seq_render_gains"][1]
    assert table["sh_seq_render_meters"][1][7] == C.POINTER(N.SeqMeter) and C.sizeof(N.SeqMeter) == 40
    assert [(n, getattr(N.SeqMeter, n).offset) for n, _t in N.SeqMeter._fields_] == [("peak", 0), ("sq_hi", 8), ("sq_lo", 24)]
    header = (Path(__file__).resolve().parents[1] / "include" / "synthhip.h").read_text()
    assert "#define SH_ABI_VERSION 6" in header and "int sh_seq_render_meters(" in header and "} sh_seq_meter;" in header
