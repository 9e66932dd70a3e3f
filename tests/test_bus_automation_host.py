"""What the rides of the buses of a compiled song of tracks -- ``CompiledSequence.automation(lanes, master=, groups=)`` -- need of the host
alone (no GPU; the fakes of tests/test_automation_host.py): every check of the new arguments raised before the native layer is reached, the
lanes packed in the meter table's row order, pieces at exactly 1.0 dropped, an automation without a bus piece made and handed on exactly
as before, a ride on a group refused by a render that does not name the group, and the master's ride over a clip against
``RefSample.fadein`` / ``fadeout``.  The bytes: tests/test_gpu_bus_automation.py."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from oracle.sample_oracle import RefSample
from synthesizer_amd import _native as N
from synthesizer_amd import mixer
from tests.songhost import RATE, _Auto, _calls, _clip, _fake, _Lib, _piece, _rows, _Seq, _song, _stereo

nan, inf = float("nan"), float("inf")


# ---- the checks ---------------------------------------------------------------------------------------------------------------------------
BAD_LANES = [
    (0.5, "a lane is None or a list of pieces"),
    ("ab", "a lane is None or a list of pieces"),
    ([(0, 10, 0.5)], r"piece 0: a piece is \(start_frame, end_frame, from_volume, to_volume\)"),
    ([(0, 10, 0.5, 1.0), (10, 20, 0.5, 1.0, 0.0)], r"piece 1: a piece is \(start_frame, end_frame, from_volume, to_volume\)"),
    ([7], r"piece 0: a piece is \(start_frame, end_frame, from_volume, to_volume\)"),
    ([(0, 10, "x", 1.0)], "piece 0: a piece is .* four numbers"),
    ([(0, 10, 0.5, None)], "piece 0: a piece is .* four numbers"),
    ([(0.0, 10, 0.5, 1.0)], "piece 0: start_frame and end_frame are integers"),
    ([(True, 10, 0.5, 1.0)], "piece 0: start_frame and end_frame are integers"),
    ([(0, "10", 0.5, 1.0)], "piece 0: start_frame and end_frame are integers"),
    ([(10, 10, 0.5, 1.0)], r"piece 0: frames \[10, 10\): a piece starts at 0 or later and ends behind its start"),
    ([(0, 5, 0.5, 1.0), (12, 10, 0.5, 1.0)], r"piece 1: frames \[12, 10\)"),
    ([(-1, 5, 0.5, 1.0)], r"piece 0: frames \[-1, 5\)"),
    ([(0, 5001, 0.5, 1.0)], r"piece 0: frames \[0, 5001\) end past the song's 5000 frames"),
    ([(0, 10, 0.5, 1.0), (9, 20, 1.0, 0.5)], r"piece 1: starts at frame 9, before the piece in front of it ends \(10\)"),
    ([(0, 10, 1.0, 1.0), (9, 20, 1.0, 0.5)], r"piece 1: starts at frame 9, before the piece in front of it ends \(10\)"),
    ([(0, 10, 1.0001, 1.0)], "piece 0: from_volume 1.0001 is not a finite number within 0.0 .. 1.0"),
    ([(0, 10, 0.5, -0.1)], "piece 0: to_volume -0.1 is not a finite number within 0.0 .. 1.0"),
    ([(0, 10, nan, 1.0)], "piece 0: from_volume nan is not a finite number within 0.0 .. 1.0"),
    ([(0, 10, 0.5, inf)], "piece 0: to_volume inf is not a finite number within 0.0 .. 1.0"),
]


@pytest.mark.parametrize("lane, message", BAD_LANES)
def test_a_bus_lane_goes_through_a_track_lanes_checks_and_the_error_names_it(monkeypatch, lane, message):
    cs = _song(monkeypatch)
    assert cs.frames == 5000
    sep = ": " if message.startswith("a lane") else ", "
    with pytest.raises(ValueError, match="CompiledSequence: automation: master" + sep + message):
        cs.automation([None] * 3, master=lane)
    with pytest.raises(ValueError, match="CompiledSequence: automation: group 2" + sep + message):
        cs.automation([None] * 3, groups=[None, [(0, 10, 0.5, 1.0)], lane])
    with pytest.raises(ValueError, match="CompiledSequence: automation: group 0" + sep + message):
        cs.automation([None] * 3, master=[(0, 10, 0.5, 1.0)], groups=(lane,))
    with pytest.raises(ValueError, match="CompiledSequence: automation: track 1" + sep + message):      # a track's lane is reported first
        cs.automation([None, lane, None], master=lane, groups=[lane])
    assert _Auto.made == [] and cs._seq.rendered == []


def test_the_group_lanes_are_a_sequence_of_at_most_eight(monkeypatch):
    cs = _song(monkeypatch)
    for bad in (0.5, "abc", 3):
        with pytest.raises(ValueError, match="CompiledSequence: automation: groups is None or a sequence, one entry per group"):
            cs.automation([None] * 3, groups=bad)
    with pytest.raises(ValueError, match="CompiledSequence: automation: 9 group lanes, at most 8"):
        cs.automation([None] * 3, groups=[None] * 9)
    with pytest.raises(ValueError, match="CompiledSequence: automation: 9 group lanes, at most 8"):
        cs.automation([None] * 3, master=[(0, 10, 0.5, 1.0)], groups=[[(0, 10, 0.5, 1.0)]] * 9)
    assert _Auto.made == []
    assert cs.automation([None] * 3, groups=[[(0, 10, 0.5, 1.0)]] * 8).rides == 8 and _Auto.made[-1].rest == (8,)


def test_width_3_a_song_without_tracks_and_a_closed_song(monkeypatch):
    _fake(monkeypatch)
    monkeypatch.setattr(N, "Sequence", _Seq)
    monkeypatch.setattr(N, "SeqAutomation", _Auto)
    del _Auto.made[:]
    flat = mixer.compile_sequence([(0.0, _stereo())], RATE, 2)
    with pytest.raises(ValueError, match=r"CompiledSequence: automation needs a song of tracks \(compile_tracks\); this one has none"):
        flat.automation([None], master=[(0, 10, 0.5, 1.0)])
    for nch in (1, 2):
        wide = _song(monkeypatch, nch=nch, width=3)
        for kw in (dict(master=[(0, 10, 0.5, 1.0)]), dict(groups=[[(0, 10, 0.5, 1.0)]]), dict(master="nonsense"), dict(master=None, groups=None)):
            with pytest.raises(NotImplementedError, match="CompiledSequence: automation: width 3: a fade has no 24-bit form"):
                wide.automation([None] * 3, **kw)
    cs = _song(monkeypatch)
    cs.close()
    with pytest.raises(ValueError, match="closed"):
        cs.automation([None] * 3, master=[(0, 10, 0.5, 1.0)])
    assert _Auto.made == []


# ---- the packed table ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("nch", [1, 2])
def test_the_lanes_are_packed_in_the_meter_tables_row_order_and_unity_pieces_are_dropped(monkeypatch, nch):
    cs = _song(monkeypatch, nch=nch)
    lanes = [[(0, 10, 0.25, 1.0)], None, [(7, 9, 0, 0.37)]]
    master = [(0, 100, 0.0, 1.0), (100, 4000, 1.0, 1.0), (4000, np.int64(5000), 1, np.float32(0.5))]        # fade-in, hold at 1.0 (dropped), fade-out
    groups = [None, ((5, 6, 1, 1), [20, 30, 0.5, 0.5]), [(0, 5000, 1.0, 1.0)], [(40, 50, 0.9, 0.1), (50, 60, 0.1, 0.9)]]
    auto = cs.automation(lanes, master=master, groups=groups)
    assert auto.pieces == (((0, 10, 0.25, 1.0),), (), ((7, 9, 0.0, 0.37),))
    assert auto.master == ((0, 100, 0.0, 1.0), (4000, 5000, 1.0, 0.5))
    assert auto.groups == ((), ((20, 30, 0.5, 0.5),), (), ((40, 50, 0.9, 0.1), (50, 60, 0.1, 0.9))) and auto.rides == 4
    assert all(type(v) is float for lane in (auto.master,) + auto.groups for p in lane for v in p[2:])
    assert all(type(f) is int for lane in (auto.master,) + auto.groups for p in lane for f in p[:2])
    assert len(_Auto.made) == 1 and _Auto.made[0].seq is cs._seq and _Auto.made[0].segments is auto.segments and _Auto.made[0].rest == (4,)
    # tracks 0 .. 2, the master at 3, group g at 4 + g: ntracks + 1 + ngroups + 1 offsets
    assert auto.seg_first == _Auto.made[0].seg_first == [0, 1, 1, 3, 6, 6, 8, 8, 11]
    c, F, NONE = nch, N.ENV_FADE_IN, N.ENV_NONE
    assert auto.segments.dtype == N.ENV_SEGMENT_DTYPE
    assert _rows(auto.segments) == [
        (10 * c, 0, 1.0, 0.75, 10.0 * c, 0.25, F, 0),           # track 0
        (7 * c, 0, 1.0, 0.0, 0.0, 0.0, NONE, 0),                # track 2: the gap in front of its piece
        (9 * c, 7 * c, 1.0, 0.37, 2.0 * c, 0.0, F, 0),
        (100 * c, 0, 1.0, 1.0, 100.0 * c, 0.0, F, 0),           # the master: the fade-in from frame 0, no gap in front
        (4000 * c, 0, 1.0, 0.0, 0.0, 0.0, NONE, 0),             # a plain segment where the dropped hold stood
        (5000 * c, 4000 * c, 1.0, 0.5 - 1.0, 1000.0 * c, 1.0, F, 0),
        (20 * c, 0, 1.0, 0.0, 0.0, 0.0, NONE, 0),               # group 1
        (30 * c, 20 * c, 1.0, 0.0, 10.0 * c, 0.5, F, 0),        # a hold: slope 0.0
        (40 * c, 0, 1.0, 0.0, 0.0, 0.0, NONE, 0),               # group 3: two pieces that meet, no gap between
        (50 * c, 40 * c, 1.0, 0.1 - 0.9, 10.0 * c, 0.9, F, 0),
        (60 * c, 50 * c, 1.0, 0.9 - 0.1, 10.0 * c, 0.1, F, 0),
    ]
    # a master ride alone: the master's lane and no group lane; a group ride alone: an empty lane for the master
    alone = cs.automation([None] * 3, master=[(10, 20, 0.5, 1.0)])
    assert alone.seg_first == [0, 0, 0, 0, 2] and alone.rides == 0 and _Auto.made[-1].rest == (0,) and alone.groups == ()
    one = cs.automation([None] * 3, groups=[None, [(0, 20, 0.5, 1.0)], None])
    assert one.seg_first == [0, 0, 0, 0, 0, 0, 1, 1] and one.rides == 2 and _Auto.made[-1].rest == (3,) and one.master == ()
    # close, with and the last reference free the table once
    made = _Auto.made[0]
    auto.close()
    auto.close()
    assert made.freed
    with pytest.raises(ValueError, match="Automation: closed"):
        cs.render(automation=auto, groups=[(0, 1, 1.0)] * 1 + [(1, 2, 1.0), (2, 3, 1.0)])


def test_an_automation_without_a_bus_piece_is_made_and_handed_on_as_before(monkeypatch):
    cs = _song(monkeypatch)
    lanes = [[(0, 10, 0.25, 1.0), (30, 31, 0.5, 0.5)], None, [(7, 9, 0, 0.37)]]
    plain = cs.automation(lanes)
    for kw in (dict(master=None, groups=None), dict(master=[], groups=[]), dict(master=[(0, 5000, 1.0, 1.0)], groups=[None, [(3, 4, 1, 1)], []])):
        auto = cs.automation(lanes, **kw)
        assert _Auto.made[-1].rest == ()                        # N.SeqAutomation(seq, segments, seg_first): three arguments
        assert auto.seg_first == plain.seg_first == [0, 3, 3, 5] and _rows(auto.segments) == _rows(plain.segments)
        assert auto.pieces == plain.pieces and auto.master == () and not any(auto.groups) and auto.rides == 0
        del cs._seq.rendered[:]
        h = auto._auto
        cs.render(10, 20, automation=auto)
        cs.render(10, 20, gains=(0.5, 1.0, 2.0), master=0.5, automation=auto)
        cs.render(10, 20, automation=auto, groups=[(0, 2, 0.5)])
        assert cs._seq.rendered == [(20, 40, 0, dict(gains=None, pans=None, master=None, automation=h)),
                                    (20, 40, 0, dict(gains=[0.5, 1.0, 2.0], pans=None, master=0.5, automation=h)),
                                    (20, 40, 0, dict(gains=None, pans=None, master=None, groups=[(0, 2, 0.5, 1.0, 1.0)], automation=h))]
    assert plain.master == () and plain.groups == () and plain.rides == 0
    assert mixer.CompiledSequence._pack_lanes(plain.pieces, 2)[1] == mixer.CompiledSequence._pack_lanes(plain.pieces, 2, (), ((), ()))[1] == [0, 3, 3, 5]


# ---- what render hands on ----------------------------------------------------------------------------------------------------------------
def test_a_ride_on_a_group_needs_a_render_that_names_the_group(monkeypatch):
    cs = _song(monkeypatch)
    auto = cs.automation([None] * 3, groups=[None, [(0, 10, 0.5, 1.0)]])          # rides group 1
    assert auto.rides == 2
    for groups, named in ((None, 0), ([], 0), ([(0, 1, 0.5)], 1)):
        for call in _calls(cs, automation=auto, groups=groups) + _calls(cs, automation=auto, groups=groups, gains=(1.0, 0.5, 1.0), master=0.5, meters=True):
            with pytest.raises(ValueError, match="CompiledSequence: the automation rides group 1, and this render names %d groups" % named):
                call()
    assert cs._seq.rendered == []
    h = auto._auto
    two, three = [(0, 1, 0.5), (1, 3, None)], [(0, 1, 0.5), (1, 2, None), (2, 3, 0.25)]
    cs.render(10, 20, automation=auto, groups=two)
    cs.render_into(N.DeviceBuffer(100), 4, 3, 9, master=0.7, automation=auto, groups=three)      # more groups than it rides
    list(cs.chunks(cs.frames, automation=auto, groups=two))
    cs.render(3, 0, automation=auto, groups=two)                # an empty window: nothing is launched
    g2, g3 = [(0, 1, 0.5, 1.0, 1.0), (1, 3, 1.0, 1.0, 1.0)], [(0, 1, 0.5, 1.0, 1.0), (1, 2, 1.0, 1.0, 1.0), (2, 3, 0.25, 1.0, 1.0)]
    assert cs._seq.rendered == [
        (20, 40, 0, dict(gains=None, pans=None, master=None, groups=g2, automation=h)),
        (6, 18, 2, dict(gains=None, pans=None, master=0.7, groups=g3, automation=h)),
        (0, 2 * cs.frames, 0, dict(gains=None, pans=None, master=None, groups=g2, automation=h)),
    ]
    # a master ride alone needs no groups=, and takes them
    del cs._seq.rendered[:]
    ride = cs.automation([None] * 3, master=[(0, 100, 0.0, 1.0)], groups=[None, None])
    assert ride.rides == 0
    cs.render(10, 20, automation=ride)
    out, levels = cs.render(0, 8, master=-1.3, meters=True, automation=ride)
    cs.render(10, 20, automation=ride, groups=two)
    assert cs._seq.rendered == [
        (20, 40, 0, dict(gains=None, pans=None, master=None, automation=ride._auto)),
        (0, 16, 0, dict(gains=None, meters=True, pans=None, master=-1.3, automation=ride._auto)),
        (20, 40, 0, dict(gains=None, pans=None, master=None, groups=g2, automation=ride._auto)),
    ]
    assert isinstance(levels, mixer.SongLevels) and len(levels.tracks) == 3 and levels.groups == []
    # another song's automation is still refused, whatever it rides
    other = _song(monkeypatch)
    for call in _calls(other, automation=ride) + _calls(other, automation=auto, groups=two):
        with pytest.raises(ValueError, match="CompiledSequence: automation is None or an Automation made by this song's automation"):
            call()


def test_the_binding_calls_the_new_entry_point_only_with_bus_lanes(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(N, "lib", lambda: lib)
    monkeypatch.setattr(N, "ensure_init", lambda: None)
    seq = N.Sequence.__new__(N.Sequence)
    seq._h, seq._sources = C.c_void_p(1), []
    segments = np.zeros(2, dtype=N.ENV_SEGMENT_DTYPE)
    plain = N.SeqAutomation(seq, segments, [0, 2, 2, 2])
    name, args = lib.calls[-1]
    assert name == "sh_seq_auto_create" and len(args) == 6 and args[4] == 3
    buses = N.SeqAutomation(seq, segments, [0, 0, 0, 0, 1, 1, 2], 2)          # 3 tracks, the master, 2 groups
    name, args = lib.calls[-1]
    assert name == "sh_seq_auto_create_buses" and args[0] is seq._h and args[1] == segments.ctypes.data and args[2] == 2
    assert list(args[3]) == [0, 0, 0, 0, 1, 1, 2] and args[4] == 3 and args[5] == 2
    master_only = N.SeqAutomation(seq, segments, [0, 0, 0, 0, 2], 0)
    name, args = lib.calls[-1]
    assert name == "sh_seq_auto_create_buses" and list(args[3]) == [0, 0, 0, 0, 2] and args[4] == 3 and args[5] == 0
    # a render reaches the entry points it reached: sh_seq_render_auto without groups, sh_seq_render_groups with them
    del lib.calls[:]

    class Out:
        handle = C.c_void_p(2)
    master_only._h, buses._h = C.c_void_p(8), C.c_void_p(9)
    seq.render(5, 6, Out, 7, automation=master_only)
    seq.render(5, 6, Out, 7, master=0.5, automation=buses, groups=[(0, 1, 0.5, 1.0, 1.0), (1, 3, 1.0, 0.5, 0.25)])
    calls = [c for c in lib.calls if c[0] != "sh_seq_get_tracks"]
    assert [c[0] for c in calls] == ["sh_seq_render_auto", "sh_seq_render_groups"]
    assert calls[0][1][12] is master_only._h and calls[1][1][12] is buses._h and calls[1][1][14] == 2
    for a in (plain, buses, master_only):
        a.free()
    seq.free()


def test_the_new_symbol_is_declared_beside_the_one_it_extends():
    table = N._SIGNATURES
    create, buses = table["sh_seq_auto_create"][1], table["sh_seq_auto_create_buses"][1]
    assert len(buses) == 7 and buses[:5] == create[:5] and buses[5] == C.c_uint32 and buses[6] == create[5]
    header = (Path(__file__).resolve().parents[1] / "include" / "synthhip.h").read_text()
    assert "int sh_seq_auto_create_buses(" in header
    assert "#define SH_ABI_VERSION 6" in header and N.SH_ABI_VERSION == 6      # a new symbol only: no struct changed


# ---- the reference expression over the mix ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 4])
def test_the_masters_ride_over_a_clip_is_refsamples_fadein_and_fadeout(width):
    """a master piece ending at 1.0 is Sample.fadein(seconds, v0) of that clip of the mix, one starting at 1.0 Sample.fadeout(seconds, v1):
    the chain's expression, with k counting the clip's interleaved samples, on a clip INSIDE a longer mix"""
    rng = np.random.default_rng(170 + width)
    dtype = {1: np.int8, 2: "<i2", 4: "<i4"}[width]
    for nch in (1, 2):
        total = 1500
        mix = _clip(rng, width, total * nch)
        for a, b in ((0, 1000), (250, 1250), (500, 1500), (700, 701)):
            frames = b - a
            assert int(RATE * (frames / RATE)) == frames        # (the fade covers the whole clip)
            clip = mix[a * nch:b * nch]
            data = clip.astype(dtype).tobytes()
            for v0, v1 in [(0.0, 1.0), (0.25, 1.0), (1.0, 0.0), (1.0, 0.37)]:
                rode = mix.tolist()
                n = float(frames * nch)
                for k in range(frames * nch):                   # the chain's ride of the master, in the song
                    rode[a * nch + k] = int(rode[a * nch + k] * (k * (v1 - v0) / n + v0))
                got = np.asarray(rode[a * nch:b * nch], dtype=np.int64).astype(dtype).tobytes()
                assert got == np.asarray(_piece(clip.tolist(), frames * nch, v0, v1), dtype=np.int64).astype(dtype).tobytes()
                assert rode[:a * nch] == mix[:a * nch].tolist() and rode[b * nch:] == mix[b * nch:].tolist()
                if v1 == 1.0:
                    assert got == RefSample(data, width, RATE, nch).fadein(frames / RATE + 1.0, v0).frames, (width, nch, a, b, v0)
                if v0 == 1.0:
                    assert got == RefSample(data, width, RATE, nch).fadeout(frames / RATE + 1.0, v1).frames, (width, nch, a, b, v1)
