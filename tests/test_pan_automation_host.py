"""What the pan rides of a compiled stereo song of tracks -- ``CompiledSequence.automation(lanes, pans=, group_pans=)`` -- need of the host
alone (no GPU; the fakes of tests/songhost.py): every check of the new arguments raised before the native layer is reached,
the pieces packed into rows and offsets, no piece dropped, an automation without a pan piece made and handed on exactly as before, a pan
ride on a group refused by a render that does not name the group, and a piece over a clip against ``RefSample.pan(lfo=...)``.  The bytes:
tests/test_gpu_pan_automation.py."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from oracle.sample_oracle import RefSample
from synthesizer_amd import _native as N
from synthesizer_amd import mixer
from tests.songhost import RATE, _Auto, _calls, _clip, _fake, _Lib, _rows, _Seq, _song, _stereo

nan, inf = float("nan"), float("inf")

# ---- the checks ---------------------------------------------------------------------------------------------------------------------------
BAD_LANES = [
    (0.5, "a lane is None or a list of pieces"),
    ("ab", "a lane is None or a list of pieces"),
    ([(0, 10, 0.5)], r"piece 0: a piece is \(start_frame, end_frame, from_pan, to_pan\)"),
    ([(0, 10, 0.5, 1.0), (10, 20, 0.5, 1.0, 0.0)], r"piece 1: a piece is \(start_frame, end_frame, from_pan, to_pan\)"),
    ([7], r"piece 0: a piece is \(start_frame, end_frame, from_pan, to_pan\)"),
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
    ([(0, 10, 0.0, 0.0), (9, 20, 1.0, 0.5)], r"piece 1: starts at frame 9, before the piece in front of it ends \(10\)"),
    ([(0, 10, 1.0001, 1.0)], "piece 0: from_pan 1.0001 is not a finite number within -1.0 .. 1.0"),
    ([(0, 10, 0.5, -1.1)], "piece 0: to_pan -1.1 is not a finite number within -1.0 .. 1.0"),
    ([(0, 10, nan, 1.0)], "piece 0: from_pan nan is not a finite number within -1.0 .. 1.0"),
    ([(0, 10, 0.5, -inf)], "piece 0: to_pan -inf is not a finite number within -1.0 .. 1.0"),
]


@pytest.mark.parametrize("lane, message", BAD_LANES)
def test_a_pan_lane_is_checked_before_the_device_is_reached_and_the_error_names_it(monkeypatch, lane, message):
    cs = _song(monkeypatch)
    assert cs.frames == 5000
    sep = ": " if message.startswith("a lane") else ", "
    with pytest.raises(ValueError, match="CompiledSequence: automation: track 1 pan" + sep + message):
        cs.automation([None] * 3, pans=[None, lane, None])
    with pytest.raises(ValueError, match="CompiledSequence: automation: group 2 pan" + sep + message):
        cs.automation([None] * 3, group_pans=[None, [(0, 10, 0.5, 1.0)], lane])
    with pytest.raises(ValueError, match="CompiledSequence: automation: track 0 pan" + sep + message):      # a track's lane is reported first
        cs.automation([None] * 3, pans=[lane, None, lane], group_pans=[lane])
    with pytest.raises(ValueError, match="CompiledSequence: automation: master" + sep):                     # and the faders' in front of the pans'
        cs.automation([None] * 3, master=0.5 if message.startswith("a lane") else [(0, 10, 0.5)], pans=[lane, None, None])
    assert _Auto.made == [] and cs._seq.rendered == []


def test_the_pan_lanes_are_one_per_track_and_at_most_eight_group_lanes(monkeypatch):
    cs = _song(monkeypatch)
    for bad in (0.5, "abc", 3):
        with pytest.raises(ValueError, match="CompiledSequence: automation: pans is None or a sequence, one entry per track"):
            cs.automation([None] * 3, pans=bad)
        with pytest.raises(ValueError, match="CompiledSequence: automation: group_pans is None or a sequence, one entry per group"):
            cs.automation([None] * 3, group_pans=bad)
    for bad in ([], [None] * 2, [None] * 4):
        with pytest.raises(ValueError, match="CompiledSequence: automation: %d pan lanes for 3 tracks" % len(bad)):
            cs.automation([None] * 3, pans=bad)
    with pytest.raises(ValueError, match="CompiledSequence: automation: 9 group pan lanes, at most 8"):
        cs.automation([None] * 3, group_pans=[None] * 9)
    assert _Auto.made == []
    auto = cs.automation([None] * 3, group_pans=[[(0, 10, 0.5, -1.0)]] * 8)
    assert auto.pan_rides == 8 and auto.rides == 0 and _Auto.made[-1].rest[0] == 8


def test_a_song_that_is_not_stereo_width_3_a_song_without_tracks_and_a_closed_song(monkeypatch):
    _fake(monkeypatch)
    monkeypatch.setattr(N, "Sequence", _Seq)
    monkeypatch.setattr(N, "SeqAutomation", _Auto)
    del _Auto.made[:]
    piece = [(0, 10, 0.5, 1.0)]
    flat = mixer.compile_sequence([(0.0, _stereo())], RATE, 2)
    with pytest.raises(ValueError, match=r"CompiledSequence: automation needs a song of tracks \(compile_tracks\); this one has none"):
        flat.automation([None], pans=[piece])
    mono = _song(monkeypatch, nch=1)
    for kw in (dict(pans=[piece, None, None]), dict(group_pans=[piece]), dict(pans=[None] * 3), dict(group_pans=[]), dict(pans="nonsense")):
        with pytest.raises(ValueError, match="CompiledSequence: automation: pans need a stereo song, this one has 1 channels"):
            mono.automation([None] * 3, **kw)
    assert mono.automation([None] * 3, pans=None, group_pans=None).pan_segments is None      # (without the arguments a mono song has its faders)
    del _Auto.made[:]
    for nch in (1, 2):
        wide = _song(monkeypatch, nch=nch, width=3)
        for kw in (dict(pans=[piece, None, None]), dict(group_pans=[piece]), dict(pans="nonsense")):
            with pytest.raises(NotImplementedError, match="CompiledSequence: automation: width 3: a fade has no 24-bit form"):
                wide.automation([None] * 3, **kw)
    cs = _song(monkeypatch)
    cs.close()
    with pytest.raises(ValueError, match="closed"):
        cs.automation([None] * 3, pans=[piece, None, None])
    assert _Auto.made == []


# ---- the packed tables ----------------------------------------------------------------------------------------------------------------------
def test_the_pieces_are_packed_into_rows_and_offsets_and_none_is_dropped(monkeypatch):
    cs = _song(monkeypatch)
    lanes = [[(0, 10, 0.25, 1.0)], None, None]
    pans = [[(0, 10, -1.0, 1.0), (10, 11, 0.0, 0.0)], None, [(7, 9, 0, 0.37), (4000, np.int64(5000), 1, np.float32(-0.5))]]
    group_pans = [None, ((5, 6, 0, 0), [20, 30, 0.5, 0.5]), [(0, 5000, 1.0, -1.0)]]
    auto = cs.automation(lanes, master=[(0, 100, 0.0, 1.0)], groups=[[(3, 4, 0.5, 0.5)]], pans=pans, group_pans=group_pans)
    assert auto.pans == (((0, 10, -1.0, 1.0), (10, 11, 0.0, 0.0)), (), ((7, 9, 0.0, 0.37), (4000, 5000, 1.0, -0.5)))
    assert auto.group_pans == ((), ((5, 6, 0.0, 0.0), (20, 30, 0.5, 0.5)), ((0, 5000, 1.0, -1.0),)) and auto.pan_rides == 3 and auto.rides == 1
    assert all(type(v) is float for lane in auto.pans + auto.group_pans for p in lane for v in p[2:])
    assert all(type(f) is int for lane in auto.pans + auto.group_pans for p in lane for f in p[:2])
    made = _Auto.made[-1]
    assert len(_Auto.made) == 1 and made.seq is cs._seq and made.segments is auto.segments
    assert made.rest == (3, auto.pan_segments, auto.pan_first)   # three group lanes: the larger of the two lists
    # the fader lanes in the buses' format, the group lanes that were not given empty: ntracks + 1 + 3 + 1 offsets
    assert auto.seg_first == made.seg_first == [0, 1, 1, 1, 2, 4, 4, 4]
    # the pan lanes: the tracks', then the groups': ntracks + 3 + 1 offsets
    assert auto.pan_first == made.rest[2] == [0, 2, 2, 6, 6, 10, 11]
    P, NONE = N.ENV_PAN, N.ENV_NONE
    assert P == 3 and auto.pan_segments.dtype == N.ENV_SEGMENT_DTYPE
    assert _rows(auto.pan_segments) == [
        (20, 0, 1.0, 2.0, 10.0, -1.0, P, 0),                    # track 0: origin and end in samples, numsamples in FRAMES
        (22, 20, 1.0, 0.0, 1.0, 0.0, P, 0),                     # a hold at 0.0 is a piece of its own
        (14, 0, 1.0, 0.0, 0.0, 0.0, NONE, 0),                   # track 2: the gap in front of its piece
        (18, 14, 1.0, 0.37, 2.0, 0.0, P, 0),
        (8000, 0, 1.0, 0.0, 0.0, 0.0, NONE, 0),
        (10000, 8000, 1.0, -0.5 - 1.0, 1000.0, 1.0, P, 0),
        (10, 0, 1.0, 0.0, 0.0, 0.0, NONE, 0),                   # group 1
        (12, 10, 1.0, 0.0, 1.0, 0.0, P, 0),
        (40, 0, 1.0, 0.0, 0.0, 0.0, NONE, 0),
        (60, 40, 1.0, 0.0, 10.0, 0.5, P, 0),
        (10000, 0, 1.0, -2.0, 5000.0, 1.0, P, 0),               # group 2: over the whole song
    ]
    # pan lanes alone: the fader table holds the empty lanes of the tracks, the master and the groups
    alone = cs.automation([None] * 3, pans=[None, [(1, 2, 0.5, 0.5)], None])
    assert alone.seg_first == [0, 0, 0, 0, 0] and len(alone.segments) == 0 and alone.pan_first == [0, 0, 2, 2] and _Auto.made[-1].rest[0] == 0
    one = cs.automation([None] * 3, groups=[None, None, None], group_pans=[[(0, 20, 0.5, 1.0)]])
    assert one.seg_first == [0] * 8 and one.pan_first == [0, 0, 0, 0, 1, 1, 1] and one.pan_rides == 1 and _Auto.made[-1].rest[0] == 3
    made = _Auto.made[0]
    auto.close()
    auto.close()
    assert made.freed
    with pytest.raises(ValueError, match="Automation: closed"):
        cs.render(automation=auto, groups=[(0, 1, 1.0), (1, 2, 1.0), (2, 3, 1.0)])


def test_an_automation_without_a_pan_piece_packs_and_reaches_what_it_did_before(monkeypatch):
    cs = _song(monkeypatch)
    lanes = [[(0, 10, 0.25, 1.0), (30, 31, 0.5, 0.5)], None, [(7, 9, 0, 0.37)]]
    master, groups = [(0, 100, 0.0, 1.0)], [None, [(5, 9, 0.5, 0.25)]]
    for before_kw in (dict(), dict(master=master), dict(master=master, groups=groups)):
        before = cs.automation(lanes, **before_kw)
        rest = _Auto.made[-1].rest
        for kw in (dict(pans=None, group_pans=None), dict(pans=[None] * 3), dict(pans=[(), None, []], group_pans=[None, ()]), dict(group_pans=[])):
            auto = cs.automation(lanes, **dict(before_kw, **kw))
            assert _Auto.made[-1].rest == rest and len(rest) <= 1      # N.SeqAutomation's arguments as before: no pan table
            assert auto.seg_first == before.seg_first and _rows(auto.segments) == _rows(before.segments)
            assert auto.pan_segments is None and auto.pan_first is None and auto.pan_rides == 0 and not any(auto.pans) and not any(auto.group_pans)
            assert (auto.pieces, auto.master, auto.groups, auto.rides) == (before.pieces, before.master, before.groups, before.rides)
            del cs._seq.rendered[:]
            cs.render(10, 20, automation=auto, groups=[(0, 1, 0.5), (1, 3, None)])
            assert cs._seq.rendered == [(20, 40, 0, dict(gains=None, pans=None, master=None, groups=[(0, 1, 0.5, 1.0, 1.0), (1, 3, 1.0, 1.0, 1.0)],
                                                         automation=auto._auto))]
    assert mixer.CompiledSequence._pack_lanes(before.pieces, 2)[1] == [0, 3, 3, 5]
    assert mixer.CompiledSequence._pack_lanes(before.pieces, 2, buses=True)[1] == [0, 3, 3, 5, 5]


# ---- what render hands on ----------------------------------------------------------------------------------------------------------------
def test_a_pan_ride_on_a_group_needs_a_render_that_names_the_group(monkeypatch):
    cs = _song(monkeypatch)
    auto = cs.automation([None] * 3, group_pans=[None, [(0, 10, 0.5, 1.0)]])          # rides the pan of group 1
    assert auto.pan_rides == 2 and auto.rides == 0
    for groups, named in ((None, 0), ([], 0), ([(0, 1, 0.5)], 1)):
        for call in _calls(cs, automation=auto, groups=groups) + _calls(cs, automation=auto, groups=groups, gains=(1.0, 0.5, 1.0), master=0.5, meters=True):
            with pytest.raises(ValueError, match="CompiledSequence: the automation rides the pan of group 1, and this render names %d groups" % named):
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
    # the tracks' pan rides alone need no groups=, and take them; a fader ride on a group is still asked for first
    del cs._seq.rendered[:]
    tracks_only = cs.automation([None] * 3, pans=[[(0, 100, -1.0, 1.0)], None, None], group_pans=[None, None])
    assert tracks_only.pan_rides == 0
    cs.render(10, 20, automation=tracks_only)
    cs.render(10, 20, automation=tracks_only, groups=two)
    assert cs._seq.rendered == [(20, 40, 0, dict(gains=None, pans=None, master=None, automation=tracks_only._auto)),
                                (20, 40, 0, dict(gains=None, pans=None, master=None, groups=g2, automation=tracks_only._auto))]
    both = cs.automation([None] * 3, groups=[None, None, [(0, 5, 0.5, 0.5)]], group_pans=[[(0, 5, 0.5, 0.5)]])
    with pytest.raises(ValueError, match="CompiledSequence: the automation rides group 2, and this render names 2 groups"):
        cs.render(automation=both, groups=two)
    with pytest.raises(ValueError, match="CompiledSequence: the automation rides group 2, and this render names 0 groups"):
        cs.render(automation=both)
    cs.render(0, 5, automation=both, groups=three)


def test_the_binding_calls_the_new_entry_point_only_with_a_pan_table(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(N, "lib", lambda: lib)
    monkeypatch.setattr(N, "ensure_init", lambda: None)
    seq = N.Sequence.__new__(N.Sequence)
    seq._h, seq._sources = C.c_void_p(1), []
    segments, pan_segments = np.zeros(2, dtype=N.ENV_SEGMENT_DTYPE), np.zeros(3, dtype=N.ENV_SEGMENT_DTYPE)
    plain = N.SeqAutomation(seq, segments, [0, 2, 2, 2])
    assert lib.calls[-1][0] == "sh_seq_auto_create"
    buses = N.SeqAutomation(seq, segments, [0, 0, 0, 0, 1, 1, 2], 2)
    assert lib.calls[-1][0] == "sh_seq_auto_create_buses"
    pans = N.SeqAutomation(seq, segments, [0, 0, 0, 0, 1, 1, 2], 2, pan_segments, [0, 1, 1, 1, 3, 3])      # 3 tracks, the master, 2 groups
    name, args = lib.calls[-1]
    assert name == "sh_seq_auto_create_pans" and len(args) == 10 and args[0] is seq._h and args[1] == segments.ctypes.data and args[2] == 2
    assert list(args[3]) == [0, 0, 0, 0, 1, 1, 2] and args[4] == 3 and args[5] == 2
    assert args[6] == pan_segments.ctypes.data and args[7] == 3 and list(args[8]) == [0, 1, 1, 1, 3, 3]
    del lib.calls[:]

    class Out:
        handle = C.c_void_p(2)
    pans._h = C.c_void_p(9)
    seq.render(5, 6, Out, 7, automation=pans)
    seq.render(5, 6, Out, 7, master=0.5, automation=pans, groups=[(0, 1, 0.5, 1.0, 1.0), (1, 3, 1.0, 0.5, 0.25)])
    calls = [c for c in lib.calls if c[0] != "sh_seq_get_tracks"]
    assert [c[0] for c in calls] == ["sh_seq_render_auto", "sh_seq_render_groups"]
    assert calls[0][1][12] is pans._h and calls[1][1][12] is pans._h and calls[1][1][14] == 2
    for a in (plain, buses, pans):
        a.free()
    seq.free()


def test_the_new_symbol_is_declared_beside_the_one_it_extends():
    table = N._SIGNATURES
    buses, pans = table["sh_seq_auto_create_buses"][1], table["sh_seq_auto_create_pans"][1]
    assert len(pans) == 10 and pans[:6] == buses[:6] and pans[6:9] == [buses[1], C.c_uint32, buses[3]] and pans[9] == buses[6]
    header = (Path(__file__).resolve().parents[1] / "include" / "synthhip.h").read_text()
    assert "int sh_seq_auto_create_pans(" in header and "#define SH_ENV_PAN 3u" in header
    assert "#define SH_ABI_VERSION 6" in header and N.SH_ABI_VERSION == 6      # a new symbol only: no struct changed


# ---- the reference expression over a clip ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 4])
def test_a_piece_over_a_clip_is_refsamples_pan_with_an_lfo(width):
    """a piece over frames [a, b) is Sample.pan(lfo=[k * (p1 - p0) / n + p0 ...]) of that clip: the chain's expression, with k counting the
    clip's FRAMES, on a clip INSIDE a longer track; the result stays inside the width's range at both ends of the pot"""
    rng = np.random.default_rng(270 + width)
    dtype = {1: np.int8, 2: "<i2", 4: "<i4"}[width]
    total = 1500
    track = _clip(rng, width, total * 2)
    lo, hi = -2 ** (8 * width - 1), 2 ** (8 * width - 1) - 1
    track[200:208] = [lo, lo, hi, hi, lo, hi, -1, -1]
    for a, b in ((0, 1000), (100, 1250), (500, 1500), (700, 701)):
        n = b - a
        data = track[2 * a:2 * b].astype(dtype).tobytes()
        for p0, p1 in [(-1.0, 1.0), (1.0, -1.0), (0.0, 0.0), (0.3, -0.77), (1.0, 1.0), (-1.0, -1.0)]:
            rode = track.tolist()
            for k in range(n):                                  # the chain's pan ride, in the song
                p = k * (p1 - p0) / n + p0
                rode[2 * (a + k)] = int(rode[2 * (a + k)] * (1.0 - p) / 2.0)
                rode[2 * (a + k) + 1] = int(rode[2 * (a + k) + 1] * (1.0 + p) / 2.0)
            assert lo <= min(rode) and max(rode) <= hi
            got = np.asarray(rode[2 * a:2 * b], dtype=np.int64).astype(dtype).tobytes()
            assert got == RefSample(data, width, RATE, 2).pan(lfo=[k * (p1 - p0) / n + p0 for k in range(n)]).frames, (width, a, b, p0, p1)
            assert rode[:2 * a] == track[:2 * a].tolist() and rode[2 * b:] == track[2 * b:].tolist()
