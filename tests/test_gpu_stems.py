"""GPU parity of the STEMS of a compiled song of tracks -- CompiledSequence.stems / stems_into, N.Sequence.stems, sh_seq_render_stems --
byte for byte against live ``audioop``: every plane of a stems call is the bus the neighbouring files' reference chains already hold --
``grouped()`` of tests/test_gpu_groups.py returns (the tracks as their bus takes them, the groups as the master takes them, the master's
bytes, ...), ``chain()`` of tests/test_gpu_pan_automation.py the same three with fader rides, bus rides and pan rides -- so plane t is
``posts[t]``, plane ntracks is ``out`` and plane ntracks + 1 + g is ``buses[g]``, all zeros where ``rows_of`` of those files says ZERO (a
track of a silent group, whose events are skipped).  Expected bytes never come from the product; the two places where the product is
held against itself (section 5) say so.  Rate 8192 and songs of two to four tiles, as in the neighbouring files."""
import audioop
import ctypes as C
import gc

import numpy as np
import pytest

from tests.seqcases import (GAINS, RATE, _ev, as_samples, in_a_child_under_the_other_alignment_scheme, ints, raw_tracks, row_of, subs_of, the_song,
                            with_samples)
from tests.seqref import LANE, TILE, differs, pcm
from tests.test_gpu_automation import native_auto as fader_auto
from tests.test_gpu_bus_automation import native_auto as bus_auto
from tests.test_gpu_bus_automation import song_of as bus_song_of
from tests.test_gpu_groups import LISTS, MUTED, SETTINGS, flat, grouped, lanes_of, native, silent, six
from tests.test_gpu_pan_automation import KIND, chain
from tests.test_gpu_pan_automation import native_auto as pan_auto
from tests.test_gpu_pan_automation import song_of
from tests.test_gpu_sequence_far import _Pack, base_of, far_bytes, far_sequence

gpu_test = pytest.mark.gpu
WIDTHS = [1, 2, 3, 4]
GAP = 24                                                    # samples between two planes where the stride is larger than the window
DESKS = [(gains, pans, master_gain, LISTS[name]) for gains, pans, master_gain, name in SETTINGS] + [(None, None, None, MUTED)]


# ---- the reference: the planes of a call, in plane order -----------------------------------------------------------------------------------
def planes_of(posts, buses, out, groups):
    """the tracks, the master, the groups -- a track of a silent group all zeros, as its events are skipped"""
    mute = {t for g in groups or () if silent(g) for t in range(g[0], g[1])}
    return [bytes(len(out)) if t in mute else p for t, p in enumerate(posts)] + [out] + list(buses)


def want_six(kind, width, desk, lanes=None):
    gains, pans, master_gain, groups = desk
    _instruments, _tracks, subs, _total = six(kind, width)
    posts, buses, out, _raw = grouped((kind, width), subs, gains, pans, groups, master_gain, width, lanes=lanes)
    return planes_of(posts, buses, out, groups)


def windows(width, total):
    """the whole song; from mid-tile on an odd sample to mid-tile; one tile with a few samples on either side"""
    T, L = TILE[width], LANE[width]
    return [(0, total), (T + 3 * L + 1, 3 * T + L), (T - 3, 2 * T + 5)]


# ---- the product's side ----------------------------------------------------------------------------------------------------------------------
def stems(N, seq, width, a, b, nrows, out_sample=0, gap=0, **desk):
    """(the planes' bytes in plane order, the guards intact: in front, behind and in every gap) of a stems call into a 0x5A-filled buffer"""
    n = b - a
    plane = n + gap
    inner = (out_sample + (nrows - 1) * plane + n) * width
    parent = N.DeviceBuffer.from_bytes(b"\x5a" * (64 + inner + 64))
    seq.stems(a, n, parent.view(64, inner), out_sample, plane, **desk)
    got = parent.download_bytes(64 + inner + 64)
    at = 64 + out_sample * width
    outs = [got[at + r * plane * width:at + (r * plane + n) * width] for r in range(nrows)]
    guards = got[:at] == b"\x5a" * at and got[at + ((nrows - 1) * plane + n) * width:] == b"\x5a" * 64 and \
        all(got[at + (r * plane + n) * width:at + (r + 1) * plane * width] == b"\x5a" * (gap * width) for r in range(nrows - 1))
    return outs, guards


def check(N, seq, width, want, wins, what, **desk):
    """every plane of every window, at out_sample 0 and 1, with a stride equal to the window and one GAP samples larger"""
    for a, b in wins:
        for out_sample in (0, 1):
            for gap in (0, GAP):
                got, guards = stems(N, seq, width, a, b, len(want), out_sample, gap, **desk)
                for r, (g, w) in enumerate(zip(got, want)):
                    assert g == w[a * width:b * width], "%s, window [%d, %d) at %d, gap %d, plane %d of %d: %d bytes differ" % (
                        what, a, b, out_sample, gap, r, len(want), differs(g, w[a * width:b * width]))
                assert guards, (what, a, b, out_sample, gap)


def desk_kw(desk, auto=None):
    gains, pans, master_gain, groups = desk
    return dict(gains=None if gains is None else list(gains), pans=flat(pans), master=master_gain, groups=native(groups) if groups else None, automation=auto)


# ---- 0: the cases are not vacuous (the reference alone, no device) -------------------------------------------------------------------------
def test_the_cases_tell_stems_from_what_a_caller_had():
    width = 2
    T = TILE[width]
    top = 2 ** (8 * width - 1)
    for kind in ("pile", "balance"):
        _instruments, _tracks, subs, total = six(kind, width)
        desk = DESKS[0]
        gains, pans, master_gain, groups = desk
        want = want_six(kind, width, desk)
        assert len(want) == 6 + 1 + len(groups) and all(len(p) == total * width for p in want)
        # a grouped track's plane is NOT its solo render through the full desk (the group's gain and pan and the master's gain stand behind it)
        t = groups[0][0]
        solo = tuple(g if k == t else 0.0 for k, g in enumerate(gains))
        assert want[t] != grouped((kind, width, "solo"), subs, solo, pans, groups, master_gain, width)[2] and any(want[t])
        # and some track's plane is not stem(t)'s chain, the raw track at gain 1.0
        assert any(want[k] != subs[k] + bytes(total * width - len(subs[k])) for k in range(6))
        # all planes differ pairwise where they sound
        sounding = [p for p in want if any(p)]
        assert len(sounding) >= 8 and len(set(sounding)) == len(sounding)
        # one tile is idle for everyone
        assert all(p[2 * T * width:3 * T * width] == bytes(T * width) for p in want)
        # a sounding track has a tile with no run of its own while another track sounds there
        by_tile = [[any(p[k * T * width:(k + 1) * T * width]) for k in range(4)] for p in want[:6]]
        assert any(any(row) and not row[k] and any(other[k] for other in by_tile) for row in by_tile for k in range(4))
    # some plane is at a rail where the master is not (the pile-up: a track or a group saturates on its own)
    want = [ints(p, width) for p in want_six("pile", width, DESKS[0])]
    master = want[6]
    assert any(np.any(((p == top - 1) | (p == -top)) & (master != top - 1) & (master != -top)) for r, p in enumerate(want) if r != 6)
    # one track is muted and one group is silent: their planes, and the planes of the silent group's tracks, are zeros; the others sound
    muted = want_six("pile", width, DESKS[1])
    assert DESKS[1][0][1] == 0.0 and not any(muted[1]) and any(muted[0])
    gone = want_six("pile", width, DESKS[3])
    assert [any(p) for p in gone] == [False, False, True, False, False, True, True, False, False]


# ---- 1: the six-track songs and their group settings, windows, strides and guards -------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", ["pile", "pan", "balance"])
def test_every_plane_is_its_bus_byte_for_byte(gpu, kind, width):
    N = gpu
    instruments, tracks, subs, total = six(kind, width)
    seq, _samples = raw_tracks(N, instruments, tracks, 2, width)
    assert seq.tracks()[0] == 6
    lanes = lanes_of(width, total)
    auto = fader_auto(N, seq, lanes, 2) if width != 3 else None           # (no automation at width 3)
    wins = windows(width, total)
    assert wins[1][0] % 2 == 1 and wins[1][0] % TILE[width] and wins[1][1] % TILE[width] and wins[2][0] < TILE[width] < 2 * TILE[width] < wins[2][1]
    for desk in DESKS:
        check(N, seq, width, want_six(kind, width, desk), wins, "%s, desk %s" % (kind, desk), **desk_kw(desk))
        if auto is not None:
            want = want_six(kind, width, desk, lanes)
            assert want != want_six(kind, width, desk) or desk is DESKS[3]      # (the laned tracks of the last desk stand in silent groups)
            check(N, seq, width, want, wins, "%s with fader lanes, desk %s" % (kind, desk), **desk_kw(desk, auto))
    # no groups at all: the tracks and the master
    desk = (DESKS[0][0], DESKS[0][1], 0.7, [])
    want = want_six(kind, width, desk)
    assert len(want) == 7
    check(N, seq, width, want, wins[1:], "%s, no groups" % kind, **desk_kw(desk))
    if auto is not None:
        auto.free()
    seq.free()


# ---- 2: fader rides, bus rides and pan rides ---------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("width", [1, 2, 4])
def test_the_planes_of_a_song_that_rides_its_buses_and_pans(gpu, width):
    N = gpu
    instruments, tracks, subs, total, settings = song_of(width)
    seq, _samples = raw_tracks(N, instruments, tracks, 2, width)
    wins = windows(width, total)
    assert len(settings) == 5 and not settings[3].groups and not any(settings[4].lanes) and any(settings[4].tpans)
    for s in settings:
        posts, buses, out = chain((KIND, width), subs, s, width)
        want = planes_of(posts, buses, out, s.groups)
        assert len(want) == 3 + 1 + len(s.groups or ())
        auto = pan_auto(N, seq, s)
        check(N, seq, width, want, wins, "setting %s" % s.name, gains=None if s.gains is None else list(s.gains), pans=flat(s.pans), master=s.master,
              groups=native(s.groups) if s.groups else None, automation=auto)
        auto.free()
    seq.free()


@gpu_test
@pytest.mark.parametrize("width", [1, 2, 4])
@pytest.mark.parametrize("kind", ["balance", "bus"])
def test_the_planes_of_a_song_that_rides_its_buses_without_pan_pieces(gpu, kind, width):
    """an Automation without pan pieces packs no pan lanes: its table reaches a kernel that reads only the lanes it holds (the fader lanes
    alone are section 1's).  ``bus``: the mono song, which has group faders and rides and no pans"""
    N = gpu
    instruments, tracks, nch, subs, total, settings = bus_song_of(kind, width)
    seq, _samples = raw_tracks(N, instruments, tracks, nch, width)
    for s in (settings[0], settings[4]):
        posts, buses, out, _scaled = s.chain((kind, width), subs, width, nch)
        want = planes_of(posts, buses, out, s.groups)
        assert len(want) == 3 + 1 + len(s.groups) and any(s.glanes) and s.mlane
        auto = bus_auto(N, seq, s, nch)
        check(N, seq, width, want, windows(width, total)[1:], "%s, setting %s" % (kind, s.name), gains=list(s.gains), pans=flat(s.pans), master=s.master,
              groups=native(s.groups), automation=auto)
        auto.free()
    seq.free()


# ---- 3: a mono song of tracks with gains and a master ---------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("width", WIDTHS)
def test_a_mono_song_with_gains_and_a_master(gpu, width):
    N = gpu
    instruments, tracks, nch, subs, total, _level = the_song("bus", width)
    assert nch == 1 and len(tracks) == 3
    seq, _samples = raw_tracks(N, instruments, tracks, 1, width)
    for gains, master_gain, groups in ((GAINS[0], 0.7, []), (GAINS[1], None, []), (GAINS[3], -1.3, [(0, 2, 0.6, None)]), (None, None, [])):
        posts, buses, out, _raw = grouped(("bus", width), subs, gains, None, groups, master_gain, width)
        want = planes_of(posts, buses, out, groups)
        check(N, seq, width, want, windows(width, total), "mono, gains %s, master %s" % (gains, master_gain), gains=None if gains is None else list(gains),
              master=master_gain, groups=native(groups) if groups else None)
    seq.free()


# ---- 4: thirty-two tracks in eight groups of four: 41 planes -----------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("width", [2, 4])
def test_forty_one_planes(gpu, width):
    N = gpu
    T = TILE[width]
    rng = np.random.default_rng(3200 + width)                   # the shape of test_thirty_two_tracks_in_eight_groups_of_four
    instruments = [(pcm(rng, width, 2 * 40, 0.9), 2), (pcm(rng, width, 2 * 25, 0.9), 2)]
    tracks = [[_ev(T // 2 + 20 + 3 * t, t % 2, [None, 1.3, 0.8][t % 3])] for t in range(32)]
    gains = tuple([1.0, 0.9, 1.7, -0.6][t % 4] for t in range(32))
    pans = tuple((round(0.05 + 0.045 * t, 3), round(1.4 - 0.06 * t, 3)) for t in range(32))
    groups = [(4 * g, 4 * g + 4, round(0.4 + 0.17 * g, 2), (round(1.2 - 0.11 * g, 2), round(0.3 + 0.09 * g, 2))) for g in range(8)]
    subs = subs_of(instruments, tracks, width, 2)
    total = max(len(s) for s in subs) // width
    assert T < total < 2 * T
    posts, buses, out, _raw = grouped(("forty-one", width), subs, gains, pans, groups, 0.9, width)
    want = planes_of(posts, buses, out, groups)
    assert len(want) == 41 and len(set(want)) == 41             # every plane its own
    seq, _samples = raw_tracks(N, instruments, tracks, 2, width)
    for a, b in ((0, total), (T + 37, total - 3)):
        for gap in (0, GAP):
            got, guards = stems(N, seq, width, a, b, 41, 1, gap, gains=list(gains), pans=flat(pans), master=0.9, groups=native(groups))
            assert [g == w[a * width:b * width] for g, w in zip(got, want)] == [True] * 41 and guards, (a, b, gap)
    seq.free()


# ---- 5: the product against itself (and only here): the master's plane is render_into's bytes, each plane's statistics its meter row -------------
@gpu_test
@pytest.mark.parametrize("width", WIDTHS)
def test_the_planes_are_what_the_meters_of_the_same_call_read(gpu, width):
    from synthesizer_amd import mixer
    N = gpu
    instruments, tracks, subs, total = six("pile", width)
    samples = as_samples(instruments, width, RATE)
    T, L = TILE[width], LANE[width]
    with mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, 2, width) as cs:
        for gains, pans, master_gain, name in SETTINGS:
            kw = dict(gains=gains, pans=pans, master=master_gain, groups=LISTS[name])
            for a, n in ((0, cs.frames), ((T + 3 * L) // 2 + 1, 700)):
                st = cs.stems(a, n, **kw)
                buf = N.DeviceBuffer.from_bytes(b"\x5a" * (n * 2 * width))
                levels = cs.render_into(buf, 0, a, n, meters=True, **kw)
                assert bytes(st.master.view_frame_data()) == buf.download_bytes(n * 2 * width)
                rows = levels.tracks + [levels.master] + levels.groups
                assert len(rows) == len(st.rows())
                for r, (sample, row) in enumerate(zip(st.rows(), rows)):
                    data = bytes(sample.view_frame_data())
                    assert row_of(ints(data, width), 0, 2) == (row.peak, row.sum_squares), (name, a, n, r)
                    assert audioop.max(data, width) == max(row.peak)


# ---- 6: 16 bits under the other alignment scheme -----------------------------------------------------------------------------------------------
@gpu_test
def test_the_planes_at_16_bits_under_the_other_alignment_scheme(gpu):
    in_a_child_under_the_other_alignment_scheme(__file__, ["test_every_plane_is_its_bus_byte_for_byte[balance-2]"])


# ---- 7: a song whose coordinates lie past 2^31 samples ---------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("width", [2, 4])
def test_a_window_of_a_song_past_two_to_the_thirty_one(gpu, width):
    N = gpu
    instruments, tracks, subs, total = six("pile", width)
    T, L = TILE[width], LANE[width]
    B = base_of("mid", width)
    assert B + T == 2 ** 31
    (args, kw), _samples = raw_tracks(_Pack, instruments, tracks, 2, width)
    seq, _table = far_sequence(N, args, B, track_first=kw["track_first"])
    assert seq.tracks()[0] == 6 and seq.info()["track_samples"] == B + total
    desk = DESKS[0]
    near = want_six("pile", width, desk)
    for a, b in ((B + T + 3 * L + 1, B + 3 * T + L), (2 ** 31 - 5, 2 ** 31 + 7), (B - 5, B + L + 2)):
        for out_sample, gap in ((0, 0), (1, GAP)):
            got, guards = stems(N, seq, width, a, b, len(near), out_sample, gap, **desk_kw(desk))
            for r, (g, w) in enumerate(zip(got, near)):
                assert g == far_bytes(w, B, a, b, width), (a - B, b - B, out_sample, gap, r)
            assert guards, (a - B, b - B, out_sample, gap)
    seq.free()


# ---- 8: through the mixer ------------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("width", WIDTHS)
def test_the_mixer_returns_samples_that_are_views_of_one_buffer(gpu, width):
    from synthesizer_amd import mixer
    N = gpu
    instruments, tracks, subs, total = six("balance", width)
    samples = as_samples(instruments, width, RATE)
    gains, pans, master_gain, groups = DESKS[0]
    lanes = lanes_of(width, total)
    with mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, 2, width, name="six") as cs:
        auto = cs.automation(lanes) if width != 3 else None
        want = want_six("balance", width, DESKS[0], lanes if auto is not None else None)
        kw = dict(gains=gains, pans=pans, master=master_gain, groups=groups, automation=auto)
        for a, n in ((0, cs.frames), (333, 1001), (5, 1)):
            st = cs.stems(a, n, **kw)
            assert isinstance(st, mixer.SongStems) and (st.start_frame, st.frames) == (a, n) and len(st.tracks) == 6 and len(st.groups) == len(groups)
            assert [s.name for s in st.rows()] == ["six:track %d" % t for t in range(6)] + ["six:master"] + ["six:group %d" % g for g in range(len(groups))]
            rows = st.rows()
            del st
            gc.collect()                                        # the Samples outlive the SongStems: each keeps the one buffer alive
            for r, (s, w) in enumerate(zip(rows, want)):
                assert (s.samplerate, s.nchannels, s.samplewidth, len(s)) == (RATE, 2, width, n)
                assert bytes(s.view_frame_data()) == w[2 * a * width:2 * (a + n) * width], (a, n, r)
            last = rows[-1]
            del rows, s
            gc.collect()
            assert bytes(last.view_frame_data()) == want[-1][2 * a * width:2 * (a + n) * width]
        # stems_into a caller's buffer, one sample in, planes further apart than the window
        a, n, plane = 333, 700, 712
        nrows = len(want)
        size = width + ((nrows - 1) * plane + n) * 2 * width + width
        buf = N.DeviceBuffer.from_bytes(b"\x5a" * size)
        assert cs.stems_into(buf, width, plane, a, n, **kw) is None
        back = buf.download_bytes(size)
        for r, w in enumerate(want):
            at = width + r * plane * 2 * width
            assert back[at:at + n * 2 * width] == w[2 * a * width:2 * (a + n) * width], r
            behind = back[at + n * 2 * width:at + plane * 2 * width]      # the gap, or behind the last plane the one sample that is left
            assert behind == b"\x5a" * ((plane - n) * 2 * width if r < nrows - 1 else width), r
        assert back[:width] == b"\x5a" * width
        # an empty window: empty Samples, nothing written
        e = cs.stems(7, 0, **kw)
        assert len(e.rows()) == nrows and all(len(s) == 0 for s in e.rows()) and e.frames == 0
        assert cs.stems_into(buf, 0, 0, 7, 0, **kw) is None and buf.download_bytes(size) == back
        if auto is not None:
            auto.close()


# ---- 9: what the entry point refuses, and what it takes ----------------------------------------------------------------------------------------
@gpu_test
def test_the_entry_point_refuses_on_the_host_and_writes_nothing(gpu):
    N = gpu
    lib = N.lib()
    from synthesizer_amd import mixer
    from synthesizer_amd.sample import Sample
    instruments, tracks, subs, total = six("pile", 2)
    seq, samples = raw_tracks(N, instruments, tracks, 2, 2)
    bufs, table, segtab, nbytes = Sample(samplerate=RATE, nchannels=2, samplewidth=2)._compile_events(with_samples(samples, [e for t in tracks for e in t]))
    flat_song = N.Sequence(bufs, table, segtab, 2, 2, nbytes // 2)
    segments, first = mixer.CompiledSequence._pack_lanes(((), ((10, 90, 0.2, 0.9),), (), (), (), ()), 2, (), ((), ((0, 5, 0.5, 0.5),)), buses=True)
    rides = N.SeqAutomation(seq, segments, first, 2)            # rides group 1
    size = 40000
    out = N.DeviceBuffer.from_bytes(b"\x5a" * size)             # 20 000 samples
    src0 = samples[0]._device()
    dbl = lambda *v: (C.c_double * len(v))(*v)                 # noqa: E731
    grp = lambda *g: (N.SeqGroup * max(1, len(g)))(*[N.SeqGroup(*x) for x in g])      # noqa: E731
    ones, twelve = dbl(*[1.0] * 6), dbl(*[0.5, 0.5] * 6)
    good = grp((0, 2, 0.8, 1.0, 1.0), (3, 5, 1.3, 0.5, 0.25))

    def call(song=seq, a=0, n=100, o=out.handle, at=0, plane=100, nplanes=9, gains=ones, ngains=6, pans=twelve, npans=12, master_gain=1.0, automation=None,
             groups=good, ngroups=2):
        return song.handle if song is not None else None, a, n, o, at, plane, nplanes, gains, ngains, pans, npans, master_gain, automation, groups, ngroups
    for what, args, message in (
        # its own
        ("planes for the tracks and the master alone", call(nplanes=7), b"7 planes for 6 tracks, the master and 2 groups"),
        ("a plane too many", call(nplanes=10), b"10 planes for 6 tracks, the master and 2 groups"),
        ("planes closer than the window", call(plane=99), b"planes 99 samples apart for a window of 100: they would overlap"),
        ("a last plane that ends one sample past out", call(n=2000, plane=2250, at=1), b"the last of 9 planes ends outside out"),
        ("a first plane past out", call(at=20001, n=0, plane=0), b"the last of 9 planes ends outside out"),
        ("a flat song", call(song=flat_song, gains=None, ngains=0, pans=None, npans=0, nplanes=1, groups=None, ngroups=0), b"a flat song has no stems"),
        ("planes whose span holds a source", call(o=src0.handle, n=10, plane=10), b"the span of the 9 planes overlaps a source of the song"),
        # and what sh_seq_render_groups refuses
        ("a range past the song", call(a=total - 10, n=11, plane=11), b"range outside the song"),
        ("too few gains", call(ngains=5), b"5 gains for 6 tracks"),
        ("a pan factor too few", call(npans=11), b"11 pan factors for 6 tracks"),
        ("a gain that is no number", call(gains=dbl(1.0, float("inf"), 1.0, 1.0, 1.0, 1.0)), b"gain 1 is not finite"),
        ("a master that is no number", call(master_gain=float("nan")), b"master gain is not finite"),
        ("NULL gains that are counted", call(gains=None), b"NULL argument"),
        ("a NULL song", call(song=None), b"NULL argument"),
        ("a NULL out", call(o=None), b"NULL argument"),
        ("nine groups", call(groups=grp(*[(i, i + 1, 1.0, 1.0, 1.0) for i in range(6)] * 2), ngroups=9, nplanes=16), b"9 groups, 0 to 8"),
        ("NULL groups that are counted", call(groups=None), b"NULL argument"),
        ("an empty range", call(groups=grp((0, 2, 0.8, 1.0, 1.0), (3, 3, 1.0, 1.0, 1.0))), b"group 1: tracks [3, 3): an empty range"),
        ("ranges that overlap by one", call(groups=grp((0, 3, 0.8, 1.0, 1.0), (2, 5, 1.0, 1.0, 1.0))), b"group 1: starts at track 2, in front of the end"),
        ("a group gain that is no number", call(groups=grp((0, 2, float("nan"), 1.0, 1.0)), ngroups=1, nplanes=8), b"group 0: gain is not finite"),
        ("an automation that rides a group the call does not name", call(automation=rides.handle, groups=grp((0, 2, 0.8, 1.0, 1.0)), ngroups=1, nplanes=8),
         b"the automation rides group 1, and this call names 1 groups"),
    ):
        assert lib.sh_seq_render_stems(*args) == N.SH_ERR_INVALID, what
        err = lib.sh_last_error()
        assert err.startswith(b"sh_seq_render_stems") and message in err, (what, err)
    assert out.download_bytes(size) == b"\x5a" * size
    # a source that lies in the GAP between two planes is inside the span: neither plane touches it, the span's check alone sees it
    notes = (np.arange(32, dtype="<i2") + 1000).tobytes()
    held = N.DeviceBuffer.from_bytes(b"\x5a" * 300 + notes + b"\x5a" * (4096 - 364))      # the source: samples [150, 182) of `held`
    inst = Sample.from_raw_frames(notes, 2, RATE, 2)
    inst._set_device(held.view(300, 64), 64)
    bufs1, table1, segtab1, nbytes1 = Sample(samplerate=RATE, nchannels=2, samplewidth=2)._compile_events([(0.0, inst)])
    one = N.Sequence(bufs1, table1, segtab1, 2, 2, nbytes1 // 2, track_first=[0, 1])
    assert nbytes1 == 64 and one.tracks()[0] == 1
    assert lib.sh_seq_render_stems(one.handle, 0, 32, held.handle, 100, 100, 2, None, 0, None, 0, 1.0, None, None, 0) == N.SH_ERR_INVALID      # [100, 232)
    assert b"the span of the 2 planes overlaps a source of the song" in lib.sh_last_error()
    assert held.download_bytes(4096) == b"\x5a" * 300 + notes + b"\x5a" * (4096 - 364)
    assert lib.sh_seq_render_stems(one.handle, 0, 32, held.handle, 200, 100, 2, None, 0, None, 0, 1.0, None, None, 0) == N.SH_OK      # behind the source
    assert held.download_bytes(4096) == b"\x5a" * 300 + notes + b"\x5a" * 36 + notes + b"\x5a" * 136 + notes + b"\x5a" * (4096 - 664)
    # what it takes: NULL gains and pans, no groups, nsamples == 0; and a call writes exactly its planes
    assert lib.sh_seq_render_stems(*call(n=0, plane=0, gains=None, ngains=0, pans=None, npans=0, groups=None, ngroups=0, nplanes=7)) == N.SH_OK
    assert out.download_bytes(size) == b"\x5a" * size
    groups = [(0, 2, 0.8, (0.999, 0.37)), (2, 6, 1.3, None)]
    assert lib.sh_seq_render_stems(*call(n=1000, plane=1100, at=3, gains=None, ngains=0, pans=None, npans=0, groups=grp(*native(groups)))) == N.SH_OK
    posts, buses, master, _raw = grouped(("pile", 2), subs, None, None, groups, None, 2)
    got = out.download_bytes(size)
    want = bytearray(b"\x5a" * size)
    for r, p in enumerate(planes_of(posts, buses, master, groups)):
        want[2 * (3 + 1100 * r):2 * (3 + 1100 * r + 1000)] = p[:2000]
    assert got == bytes(want)
    rides.free()
    for s in (seq, flat_song, one):
        s.free()
