"""GPU parity of the group buses of a compiled song of tracks -- CompiledSequence.render(groups=) / N.Sequence.render(groups=) /
sh_seq_render_groups -- byte for byte against live ``audioop``.  The reference chain is ``grouped`` below, the only definition of
correct::

    master = silence
    for t: sub = the track folded on its own (tests/seqcases.subs_of); its gain, its fader moves, its pan (the desk's and the automation's)
           if t lies in group g:
               if t == first_g: bus = silence
               bus = audioop.add(bus, sub)                           # the group saturates ON ITS OWN, at every track
               if t == end_g - 1:
                   if gain_g != 1.0: bus = audioop.mul(bus, gain_g)
                   if pan_g is not None: bus = Sample.stereo(lf_g, rf_g) of a stereo sample (tests/seqref.balance)
                   master = audioop.add(master, bus)                 # where the group's LAST track stands
           else: master = audioop.add(master, sub)
    if master_gain != 1.0: master = audioop.mul(master, master_gain)

Expected bytes never come from the product.  Rate 8192 and four-tile songs (at most 8192 samples): the events of the neighbouring files'
stereo songs dealt over six tracks, and a six-track pile-up of its own in which a group saturates in front of its gain."""
import audioop
import ctypes as C
import functools

import numpy as np
import pytest

from tests.seqcases import (HELD, RATE, _ev, as_samples, in_a_child_under_the_other_alignment_scheme, ints, raw_tracks, render_window, row_of,
                            song, subs_of, windows, with_samples)
from tests.seqref import LANE, TILE, differs, factors, pcm
from tests.test_gpu_automation import ride
from tests.test_gpu_desk import TRUNCATED, flat, mul, stereo

pytestmark = pytest.mark.gpu

ZERO = ((0, 0), (0, 0))
KINDS = ["pan", "balance", "pile"]                          # the neighbours' two stereo songs over six tracks, and the pile-up of this file
WIDTHS = [1, 2, 3, 4]
RIGHT, PER_TRACK, FLAT, LATE, PAN_FIRST = "right", "the group's gain on each track", "the flat desk", "the group behind all tracks", \
    "the group's pan in front of its gain"
WRONG = (PER_TRACK, FLAT, LATE, PAN_FIRST, TRUNCATED)
GAINS6 = [(0.5, 1.0, -1.7, 0.999, 1.0, 0.8), (1.0, 0.0, 1.0, 2.5, 0.37, 1.0)]
PANS6 = [(0.3, None, (1.5, 0.25), None, -0.37, (0.999, 0.37)), (None, (0.0, 0.0), None, (-0.5, 1.0), None, 1.0)]
# (first_track, end_track, gain, pan): one group; three with loose tracks in front, between and behind; one track; all tracks
LISTS = {
    "one": [(3, 6, 0.7, None)],
    "three": [(1, 3, 1.3, (0.999, 0.37)), (3, 4, -0.8, None), (4, 5, 0.6, -0.37)],
    "one track": [(2, 3, 0.37, (1.5, 0.25))],
    "all": [(0, 6, 0.9, 0.3)],
    "two around a loose track": [(0, 2, 0.8, (0.999, 0.37)), (3, 5, 1.3, (0.37, 0.999))],
}


# ---- the songs ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def six(kind, width):
    """(instruments, six tracks, the sub-mixes, total samples); stereo"""
    T, L = TILE[width], LANE[width]
    if kind != "pile":
        instruments, events, nch, _flat, total = song(kind, width)
        assert nch == 2
        tracks = [events[t::6] for t in range(6)]               # the list dealt over six tracks: the three loud notes are tracks 3, 4 and 5
    else:
        # tracks 0 and 1 (a group) pile the loud instrument up at the same frames with the same sign, track 2 (loose) has it there with the
        # opposite sign, tracks 3 and 4 (a group) pile it up again, track 5 (loose) has the opposite sign once more, so that the master
        # saturates on the way and the place where a group enters it shows.  Tile 2 is idle; the song ends mid-lane.
        rng = np.random.default_rng(1700 + width)
        instruments = [(pcm(rng, width, 2 * HELD[0], 1.0), 2), (pcm(rng, width, 2 * HELD[1], 0.6), 2), (pcm(rng, width, 2 * HELD[2], 0.6), 2)]
        w0, tail, F = (T + 3 * L) // 2, (37 * L + 3) // 2, T // 2
        tracks = [
            [_ev(0, 1, 0.8), _ev(w0 + 10, 0, 1.7, 200)],
            [_ev(F - 300, 0, 0.5), _ev(w0 + 10, 0, 1.7, 200)],
            [_ev(w0 + 10, 0, -1.7, 200)],
            [_ev(w0 - 100, 1, None), _ev(w0 + 10, 0, 1.7, 200)],
            [_ev(w0 + 10, 0, 1.2, 200)],
            [_ev(5, 2, 1.3), _ev(w0 + 10, 0, -1.7, 200), _ev(3 * F, 1, 1.2, tail)],
        ]
    subs = subs_of(instruments, tracks, width, 2)
    total = max(len(s) for s in subs) // width
    assert 3 * T < total < 4 * T and total % L != 0 and total % 2 == 0
    return instruments, tracks, subs, total


def pair(pan):
    return None if pan is None else factors(tuple(pan) if isinstance(pan, (tuple, list)) else pan)


def native(groups):
    """the list as the C entry point takes it: (first, end, gain, left, right)"""
    return [(f, e, 1.0 if g is None else g) + ((1.0, 1.0) if p is None else pair(p)) for f, e, g, p in groups]


def silent(group):
    _f, _e, g, p = group
    return g == 0.0 or (p is not None and pair(p) == (0.0, 0.0))


# ---- the reference -----------------------------------------------------------------------------------------------------------------------
_GROUPED = {}


def grouped(key, subs, gains, pans, groups, master_gain, width, how=RIGHT, lanes=None):
    """(the tracks as their bus takes them; the groups as the master takes them; the master's bytes; the groups in front of their gain),
    made once per key and setting.  ``how``: the chain, or one of its wrong forms."""
    groups = tuple(groups)
    at = (key, gains, pans, groups, master_gain, how, lanes)
    if at in _GROUPED:
        return _GROUPED[at]
    total = max([len(s) for s in subs] + [0])
    of = {t: k for k, (first, end, _g, _p) in enumerate(groups) for t in range(first, end)}

    def fader(data, k, rounding=RIGHT):                        # a group's gain, then its pan
        _first, _end, g, pan = groups[k]
        g, pan = 1.0 if g is None else g, pair(pan)
        if how == PAN_FIRST and pan is not None:
            return mul(stereo(data, width, *pan), width, g)
        data = mul(data, width, g, rounding)
        return data if pan is None else stereo(data, width, *pan, rounding)

    out, posts, buses, raw, late, bus = bytes(total), [], [None] * len(groups), [None] * len(groups), [], None
    for t, sub in enumerate(subs):
        sub = sub + bytes(total - len(sub))
        sub = mul(sub, width, 1.0 if gains is None else gains[t])
        if lanes is not None and lanes[t]:
            sub = ride(sub, width, 2, lanes[t])
        if pans is not None and pans[t] is not None:
            sub = stereo(sub, width, *pair(pans[t]))
        k = of.get(t)
        if k is not None and how in (PER_TRACK, FLAT):
            sub = fader(sub, k)
        posts.append(sub)
        if k is None or how == FLAT:
            out = audioop.add(out, sub, width)
            continue
        first, end = groups[k][:2]
        if t == first:
            bus = bytes(total)
        bus = audioop.add(bus, sub, width)                      # saturating at every track of the group
        if t == end - 1:
            raw[k] = bus
            if how != PER_TRACK:
                bus = fader(bus, k, TRUNCATED if how == TRUNCATED else RIGHT)
            buses[k] = bus
            if how == LATE:
                late.append(bus)
            else:
                out = audioop.add(out, bus, width)              # where the group's last track stands
    for bus in late:
        out = audioop.add(out, bus, width)
    if master_gain is not None:
        out = mul(out, width, master_gain)
    _GROUPED[at] = (posts, buses, out, raw)
    return _GROUPED[at]


def rows_of(key, subs, gains, pans, groups, master_gain, width, a, b, lanes=None):
    """ntracks + 1 + ngroups rows: the tracks as their bus takes them (zero in a silent group, whose events are skipped), the master, the
    groups as the master takes them"""
    posts, buses, out, _raw = grouped(key, subs, gains, pans, groups, master_gain, width, lanes=lanes)
    mute = {t for g in groups if silent(g) for t in range(g[0], g[1])}
    return [ZERO if t in mute else row_of(ints(p, width)[a:b], a, 2) for t, p in enumerate(posts)] + [row_of(ints(out, width)[a:b], a, 2)] + \
        [row_of(ints(bus, width)[a:b], a, 2) for bus in buses]


class WithGroups:
    """N.Sequence behind render_window, which calls render(first, n, out, out_sample): through sh_seq_render_groups"""

    def __init__(self, seq, gains, pans, master_gain, groups, auto=None):
        self.seq, self.gains, self.pans, self.master, self.groups, self.auto = seq, gains, flat(pans), master_gain, native(groups), auto

    def render(self, a, n, out, out_sample):
        self.seq.render(a, n, out, out_sample, gains=self.gains, pans=self.pans, master=self.master, groups=self.groups, automation=self.auto)


def metered(N, seq, width, a, b, gains, pans, master_gain, groups, out_sample=0):
    """(rows, the rendered bytes, the guards intact) of a metered render with groups into a 0x5A-filled buffer"""
    n = b - a
    inner = (out_sample + n) * width
    parent = N.DeviceBuffer.from_bytes(b"\x5a" * (64 + inner + 64))
    rows = seq.render(a, n, parent.view(64, inner), out_sample, gains=gains, meters=True, pans=flat(pans), master=master_gain, groups=native(groups))
    got = parent.download_bytes(64 + inner + 64)
    at = 64 + out_sample * width
    return rows, got[at:at + n * width], got[:at] == b"\x5a" * at and got[at + n * width:] == b"\x5a" * 64


def lanes_of(width, total):
    """fader moves for tracks 1, 3 and 4, in song frames: a fade across the pile-up window's start, a hold, a fade to the song's end"""
    T, L = TILE[width], LANE[width]
    w = (T + 3 * L) // 2
    return ((), ((w - 40, w + 60, 0.2, 0.9), (w + 60, w + 90, 0.5, 0.5)), (), ((0, total // 2, 0.9, 0.15),), ((w + 5, w + 150, 1.0, 0.3),), ())


# ---- 1: the reference tells the chain from its wrong forms (no device) ----------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_reference_differs_from_every_wrong_form_inside_the_pile_up(kind, width):
    _instruments, _tracks, subs, total = six(kind, width)
    T, L = TILE[width], LANE[width]
    lo, hi = (T + 3 * L) * width, (3 * T + L) * width
    top = 2 ** (8 * width - 1)
    groups = LISTS["two around a loose track"] if kind == "pile" else LISTS["three"]
    # first with no step on the tracks or the master, so that whatever differs is a group's step and where it stands; then on a full desk
    for gains, pans, master_gain in ((None, None, None), (GAINS6[0], PANS6[0], 0.7)):
        want = grouped((kind, width), subs, gains, pans, groups, master_gain, width)[2]
        found = {how: differs(want[lo:hi], grouped((kind, width), subs, gains, pans, groups, master_gain, width, how)[2][lo:hi]) for how in WRONG}
        print("%s, width %d, gains %s, pans %s: bytes of the pile-up window that differ: %s" % (kind, width, gains, pans, found))
        assert all(n > 0 for n in found.values()), found
    if kind == "pile":
        raw = grouped((kind, width), subs, None, None, groups, None, width)[3]
        for bus in raw:                                         # each group saturates in front of its gain
            low, high = audioop.minmax(bus[lo:hi], width)
            assert high == top - 1 and low == -top, "a group does not saturate on its own"
        # and a loose track of the opposite sign stands between the two: the master's order shows
        assert found[LATE] > 0


# ---- 2: the whole song, through the mixer ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", KINDS[:2])
def test_the_whole_song_is_the_reference_chain_byte_for_byte(gpu, kind, width):
    from synthesizer_amd import mixer
    instruments, tracks, subs, total = six(kind, width)
    samples = as_samples(instruments, width, RATE)
    lanes = lanes_of(width, total)
    with mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, 2, width) as cs:
        assert cs.ntracks == 6 and cs.frames * 2 == total
        auto = cs.automation(lanes) if width != 3 else None
        for name in ("one", "three", "one track", "all"):
            groups = LISTS[name]
            for gains, pans, master_gain in ((None, None, None), (GAINS6[0], PANS6[0], 0.7), (GAINS6[1], PANS6[1], -1.3), (GAINS6[0], None, None)):
                want = grouped((kind, width), subs, gains, pans, groups, master_gain, width)[2]
                got = bytes(cs.render(gains=gains, pans=pans, master=master_gain, groups=groups).view_frame_data())
                assert got == want, "groups %s, gains %s, pans %s, master %s: %d bytes differ" % (name, gains, pans, master_gain, differs(got, want))
                if auto is not None:
                    want = grouped((kind, width), subs, gains, pans, groups, master_gain, width, lanes=lanes)[2]
                    got = bytes(cs.render(gains=gains, pans=pans, master=master_gain, groups=groups, automation=auto).view_frame_data())
                    assert got == want, "groups %s with automation, gains %s, pans %s, master %s: %d bytes differ" % (
                        name, gains, pans, master_gain, differs(got, want))
        if auto is not None:
            assert grouped((kind, width), subs, None, None, LISTS["three"], None, width, lanes=lanes)[2] != \
                grouped((kind, width), subs, None, None, LISTS["three"], None, width)[2]
            auto.close()


# ---- 3: windows, through the C entry point ----------------------------------------------------------------------------------------------
SETTINGS = [(GAINS6[0], PANS6[0], 0.7, "three"), (GAINS6[1], PANS6[1], -1.3, "two around a loose track"), (None, None, None, "all")]


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", ["balance", "pile"])
def test_every_window_holds_its_slice_and_nothing_beside_it_is_written(gpu, kind, width):
    N = gpu
    instruments, tracks, subs, total = six(kind, width)
    wins = windows("balance", width, total)
    assert any(a % 2 for a, _b in wins), "no window starts on an odd sample"
    seq, _samples = raw_tracks(N, instruments, tracks, 2, width)
    assert seq.tracks()[0] == 6
    for gains, pans, master_gain, name in SETTINGS:
        groups = LISTS[name]
        want = grouped((kind, width), subs, gains, pans, groups, master_gain, width)[2]
        for a, b in wins:
            for out_sample in (0, 1):
                got, front, back = render_window(N, WithGroups(seq, gains, pans, master_gain, groups), width, a, b, out_sample)
                assert got == want[a * width:b * width], (gains, pans, master_gain, name, a, b, out_sample, differs(got, want[a * width:b * width]))
                assert front == b"\x5a" * 64 and back == b"\x5a" * 64, (a, b, out_sample)
    seq.free()


def test_the_windows_at_16_bits_under_the_other_alignment_scheme(gpu):
    in_a_child_under_the_other_alignment_scheme(
        __file__, ["test_every_window_holds_its_slice_and_nothing_beside_it_is_written[%s-2]" % kind for kind in ("balance", "pile")])


# ---- 4: meters ---------------------------------------------------------------------------------------------------------------------------
MUTED = [(0, 2, 0.0, (0.999, 0.37)), (3, 5, 1.3, (0.0, 0.0))]       # a group at gain 0.0, a group at pan (0.0, 0.0)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", ["balance", "pile"])
def test_the_rows_of_the_groups_follow_the_masters(gpu, kind, width):
    from synthesizer_amd import mixer
    N = gpu
    instruments, tracks, subs, total = six(kind, width)
    T, L = TILE[width], LANE[width]
    wins = [(0, total), (T + 3 * L + 1, 3 * T + L), (2 * T + 5, 3 * T - 7), (T - 1, T + 1)]      # whole, odd, idle, across a tile's edge
    seq, samples = raw_tracks(N, instruments, tracks, 2, width)
    for gains, pans, master_gain, name in SETTINGS:
        groups = LISTS[name]
        want_bytes = grouped((kind, width), subs, gains, pans, groups, master_gain, width)[2]
        for a, b in wins:
            want = rows_of((kind, width), subs, gains, pans, groups, master_gain, width, a, b)
            assert len(want) == 6 + 1 + len(groups)
            for out_sample in (0, 1):
                rows, got, guards = metered(N, seq, width, a, b, gains, pans, master_gain, groups, out_sample)
                assert rows == want, "gains %s, pans %s, master %s, groups %s, window [%d, %d) at %d:\n%s\n%s" % (
                    gains, pans, master_gain, name, a, b, out_sample, rows, want)
                assert got == want_bytes[a * width:b * width] and guards, (gains, pans, master_gain, name, a, b, out_sample)
            assert got == render_window(N, WithGroups(seq, gains, pans, master_gain, groups), width, a, b, 1)[0]      # the unmetered render's bytes
            if 2 * T <= a and b <= 3 * T:
                assert rows == [ZERO] * (7 + len(groups))       # the idle tile: nothing sounds
    # a group at gain 0.0 and one with pan (0.0, 0.0) read zero, and so do their tracks; the loose tracks and the master sound
    want = rows_of((kind, width), subs, None, None, MUTED, None, width, 0, total)
    rows, got, guards = metered(N, seq, width, 0, total, None, None, None, MUTED)
    assert rows == want and guards and got == grouped((kind, width), subs, None, None, MUTED, None, width)[2]
    assert rows[0] == rows[1] == rows[3] == rows[4] == rows[7] == rows[8] == ZERO and rows[2] != ZERO and rows[5] != ZERO and rows[6] != ZERO
    seq.free()
    # chunks of a length that is no multiple of the lane width join to the whole, and the third chunk's rows are right
    frames = 333
    assert (2 * frames) % LANE[width]
    gains, pans, master_gain, name = SETTINGS[0]
    groups = LISTS[name]
    with mixer.compile_tracks([with_samples(as_samples(instruments, width, RATE), t) for t in tracks], RATE, 2, width) as cs:
        pairs = list(cs.chunks(frames, gains=gains, pans=pans, master=master_gain, groups=groups, meters=True))
        assert len(pairs) == -(-cs.frames // frames) > 4
        assert b"".join(bytes(s.view_frame_data()) for s, _l in pairs) == grouped((kind, width), subs, gains, pans, groups, master_gain, width)[2]
        third = rows_of((kind, width), subs, gains, pans, groups, master_gain, width, 4 * frames, 6 * frames)
        levels = pairs[2][1]
        assert len(levels.tracks) == 6 and len(levels.groups) == len(groups)
        assert [(r.peak, r.sum_squares) for r in levels.tracks + [levels.master] + levels.groups] == third


# ---- 5: identities -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_groups_that_do_nothing_change_no_byte(gpu, width):
    from synthesizer_amd import mixer
    instruments, tracks, subs, total = six("pile", width)
    T, L = TILE[width], LANE[width]
    gains, pans = GAINS6[0], PANS6[0]
    with mixer.compile_tracks([with_samples(as_samples(instruments, width, RATE), t) for t in tracks], RATE, 2, width) as cs:
        plain = bytes(cs.render(gains=gains, pans=pans, master=0.7).view_frame_data())
        assert bytes(cs.render(gains=gains, pans=pans, master=0.7, groups=None).view_frame_data()) == plain
        assert bytes(cs.render(gains=gains, pans=pans, master=0.7, groups=[]).view_frame_data()) == plain
        for t in range(6):                                      # a one-track group at gain 1.0: the track's own bus
            assert bytes(cs.render(gains=gains, pans=pans, master=0.7, groups=[(t, t + 1, 1.0)]).view_frame_data()) == plain, t
            assert bytes(cs.render(gains=gains, pans=pans, master=0.7, groups=[(t, t + 1, None, (1.0, 1.0))]).view_frame_data()) == plain, t
        # a group over all tracks at gain g, no master: the master's fader at g
        for g in (0.7, -1.3, 0.0):
            assert bytes(cs.render(gains=gains, pans=pans, groups=[(0, 6, g)]).view_frame_data()) == \
                bytes(cs.render(gains=gains, pans=pans, master=g).view_frame_data()), g
        # a group at gain 1.0 in a window where nothing saturates: the ungrouped render (the whole song is NOT: the group clips on its own)
        top = 2 ** (8 * width - 1)
        a, n = 104, T // 2 - 300 - 108                          # frames of tile 0 behind track 5's first note, in front of track 1's
        ungrouped = grouped(("pile", width), subs, None, None, [], None, width)[2]
        low, high = audioop.minmax(ungrouped[2 * a * width:2 * (a + n) * width], width)
        assert n > 0 and -top < low < 0 < high < top - 1
        for groups in ([(3, 5, 1.0)], [(0, 2, 1.0), (3, 6, None, None)]):
            assert bytes(cs.render(a, n, groups=groups).view_frame_data()) == bytes(cs.render(a, n).view_frame_data())
            assert bytes(cs.render(groups=groups).view_frame_data()) != bytes(cs.render().view_frame_data())
            assert bytes(cs.render(groups=groups).view_frame_data()) == grouped(("pile", width), subs, None, None, [g + (None,) * (4 - len(g)) for g in groups],
                                                                                None, width)[2]
        # a group's bus alone is the render with its tracks soloed
        buses = grouped(("pile", width), subs, None, None, [(0, 2, 1.0, None)], None, width)[3]
        assert bytes(cs.render(gains=[1.0, 1.0, 0.0, 0.0, 0.0, 0.0]).view_frame_data()) == buses[0]


# ---- 6: thirty-two tracks in eight groups of four -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [2, 4])
def test_thirty_two_tracks_in_eight_groups_of_four(gpu, width):
    N = gpu
    T, L = TILE[width], LANE[width]
    rng = np.random.default_rng(3200 + width)
    instruments = [(pcm(rng, width, 2 * 40, 0.9), 2), (pcm(rng, width, 2 * 25, 0.9), 2)]
    tracks = [[_ev(T // 2 + 20 + 3 * t, t % 2, [None, 1.3, 0.8][t % 3])] for t in range(32)]      # one short event each, all in tile 1, overlapping
    gains = tuple([1.0, 0.9, 1.7, -0.6][t % 4] for t in range(32))
    pans = tuple((round(0.05 + 0.045 * t, 3), round(1.4 - 0.06 * t, 3)) for t in range(32))
    groups = [(4 * g, 4 * g + 4, round(0.4 + 0.17 * g, 2), (round(1.2 - 0.11 * g, 2), round(0.3 + 0.09 * g, 2))) for g in range(8)]
    assert len({g[2:] for g in groups}) == 8
    subs = subs_of(instruments, tracks, width, 2)
    total = max(len(s) for s in subs) // width
    assert T < total < 2 * T and min(int(RATE * t[0][0]) * 2 for t in tracks) >= T
    key = ("thirty-two", width)
    _posts, _buses, want, raw = grouped(key, subs, gains, pans, groups, 0.9, width)
    top = 2 ** (8 * width - 1)
    assert any(audioop.minmax(b, width)[1] == top - 1 or audioop.minmax(b, width)[0] == -top for b in raw)      # a group saturates on the way
    assert differs(want, grouped(key, subs, gains, pans, groups, 0.9, width, PER_TRACK)[2]) > 0
    seq, _samples = raw_tracks(N, instruments, tracks, 2, width)
    assert seq.tracks()[0] == 32
    for a, b in ((0, total), (T + 37, total - 3)):
        got, front, back = render_window(N, WithGroups(seq, list(gains), pans, 0.9, groups), width, a, b, 1)
        assert got == want[a * width:b * width] and front == back == b"\x5a" * 64, (a, b)
        rows, got, guards = metered(N, seq, width, a, b, list(gains), pans, 0.9, groups)
        assert len(rows) == 41
        assert rows == rows_of(key, subs, gains, pans, groups, 0.9, width, a, b) and got == want[a * width:b * width] and guards, (a, b)
        assert len(set(rows[33:])) == 8                           # every group's own row
    seq.free()


# ---- 7: what the C entry point refuses ---------------------------------------------------------------------------------------------------
def test_the_entry_point_refuses_on_the_host_and_writes_nothing(gpu):
    N = gpu
    lib = N.lib()
    from synthesizer_amd import mixer
    from synthesizer_amd.sample import Sample
    instruments, tracks, subs, total = six("pile", 2)
    seq, samples = raw_tracks(N, instruments, tracks, 2, 2)
    bufs, table, segtab, nbytes = Sample(samplerate=RATE, nchannels=2, samplewidth=2)._compile_events(with_samples(samples, [e for t in tracks for e in t]))
    flat_song = N.Sequence(bufs, table, segtab, 2, 2, nbytes // 2)
    rng = np.random.default_rng(7)
    m_instruments = [(pcm(rng, 2, 300, 0.6), 1)]
    m_tracks = [[_ev(10 * t, 0, 0.8)] for t in range(6)]
    mono, _m = raw_tracks(N, m_instruments, m_tracks, 1, 2)
    i3, t3, _s3, _total3 = six("pile", 3)
    three, _s = raw_tracks(N, i3, t3, 2, 3)
    segments, first = mixer.CompiledSequence._pack_lanes(((), ((10, 90, 0.2, 0.9),), (), (), (), ()), 2)
    auto = N.SeqAutomation(seq, segments, first)
    out = N.DeviceBuffer.from_bytes(b"\x5a" * 4000)
    rows = (N.SeqMeter * 10)()
    C.memset(rows, 0xAB, C.sizeof(rows))
    untouched = bytes(rows)
    dbl = lambda *v: (C.c_double * len(v))(*v)                 # noqa: E731
    grp = lambda *g: (N.SeqGroup * max(1, len(g)))(*[N.SeqGroup(*x) for x in g])      # noqa: E731
    nan, inf = float("nan"), float("inf")
    ones, twelve = dbl(*[1.0] * 6), dbl(*[0.5, 0.5] * 6)
    good = grp((0, 2, 0.8, 1.0, 1.0), (3, 5, 1.3, 0.5, 0.25))

    def call(song=seq, a=0, n=100, o=out.handle, at=0, gains=ones, ngains=6, pans=twelve, npans=12, master_gain=1.0, meters=None, nmeters=0,
             automation=None, groups=good, ngroups=2):
        return song.handle if song is not None else None, a, n, o, at, gains, ngains, pans, npans, master_gain, meters, nmeters, automation, groups, ngroups
    for what, args, message in (
        # what sh_seq_render_desk and sh_seq_render_auto refuse
        ("a mono song with pans", call(song=mono, groups=grp((0, 2, 0.8, 1.0, 1.0)), ngroups=1), b"pans need a stereo song, this one has 1 channels"),
        ("a flat song", call(song=flat_song, gains=None, ngains=0, pans=None, npans=0), b"the song has no tracks"),
        ("too few gains", call(ngains=5), b"5 gains for 6 tracks"),
        ("a pan factor too few", call(npans=11), b"11 pan factors for 6 tracks"),
        ("a pan that is no number", call(pans=dbl(*[0.5, 0.5, 1.0, nan] + [1.0] * 8)), b"pan 1: right factor is not finite"),
        ("a master that is no number", call(master_gain=nan), b"master gain is not finite"),
        ("a gain that is no number", call(gains=dbl(1.0, inf, 1.0, 1.0, 1.0, 1.0)), b"gain 1 is not finite"),
        ("NULL pans that are counted", call(pans=None), b"NULL argument"),
        ("NULL gains that are counted", call(gains=None), b"NULL argument"),
        ("NULL rows that are counted", call(nmeters=9), b"NULL argument"),
        ("a NULL song", call(song=None), b"NULL argument"),
        ("a NULL out", call(o=None), b"NULL argument"),
        ("a range past the song", call(a=total - 10, n=11), b"range outside the song"),
        ("a range past out", call(n=2000, at=1), b"range outside out"),
        ("an automation made for another song", call(song=mono, pans=None, npans=0, automation=auto.handle, groups=grp((0, 2, 0.8, 1.0, 1.0)), ngroups=1),
         b"the automation was made for another song"),
        # and its own
        ("no groups", call(ngroups=0), b"0 groups, 1 to 8"),
        ("nine groups", call(groups=grp(*[(i, i + 1, 1.0, 1.0, 1.0) for i in range(6)] * 2), ngroups=9), b"9 groups, 1 to 8"),
        ("NULL groups", call(groups=None), b"NULL argument"),
        ("an empty range", call(groups=grp((0, 2, 0.8, 1.0, 1.0), (3, 3, 1.0, 1.0, 1.0))), b"group 1: tracks [3, 3): an empty range"),
        ("a range turned round", call(groups=grp((4, 2, 0.8, 1.0, 1.0)), ngroups=1), b"group 0: tracks [4, 2): an empty range"),
        ("a range past the tracks", call(groups=grp((0, 2, 0.8, 1.0, 1.0), (3, 7, 1.0, 1.0, 1.0))), b"group 1: tracks [3, 7) of 6"),
        ("ranges that overlap by one", call(groups=grp((0, 3, 0.8, 1.0, 1.0), (2, 5, 1.0, 1.0, 1.0))), b"group 1: starts at track 2, in front of the end"),
        ("ranges out of order", call(groups=grp((3, 5, 0.8, 1.0, 1.0), (0, 2, 1.0, 1.0, 1.0))), b"group 1: starts at track 0, in front of the end"),
        ("a group gain that is no number", call(groups=grp((0, 2, nan, 1.0, 1.0)), ngroups=1), b"group 0: gain is not finite"),
        ("an infinite group gain", call(groups=grp((0, 2, 0.8, 1.0, 1.0), (3, 5, -inf, 1.0, 1.0))), b"group 1: gain is not finite"),
        ("a group factor that is no number", call(groups=grp((0, 2, 0.8, 1.0, nan)), ngroups=1), b"group 0: left / right is not finite"),
        ("an infinite group factor", call(groups=grp((0, 2, 0.8, inf, 1.0)), ngroups=1), b"group 0: left / right is not finite"),
        ("a group pan on a mono song", call(song=mono, pans=None, npans=0, groups=grp((0, 2, 0.8, 1.0, 1.0), (2, 3, 1.0, 0.5, 1.0))),
         b"group 1: a pan needs a stereo song, this one has 1 channels"),
        ("rows for the tracks and the master alone", call(meters=rows, nmeters=7), b"7 rows for 6 tracks, the master and 2 groups"),
        ("a row too many", call(meters=rows, nmeters=10), b"10 rows for 6 tracks, the master and 2 groups"),
        ("rows that are not counted", call(meters=rows, nmeters=0), b"0 rows for 6 tracks, the master and 2 groups"),
        ("an automation handle at width 3", call(song=three, automation=auto.handle, gains=None, ngains=0, pans=None, npans=0),
         b"width 3: a fader move's fade has no 24-bit form"),
    ):
        assert lib.sh_seq_render_groups(*args) == N.SH_ERR_INVALID, what
        err = lib.sh_last_error()
        assert err.startswith(b"sh_seq_render_groups") and message in err, (what, err)
        assert bytes(rows) == untouched, what
    assert out.download_bytes(4000) == b"\x5a" * 4000
    # and what it takes: NULL gains and NULL pans with groups alone, unmetered; touching ranges; a group that ends on the last track
    groups = [(0, 2, 0.8, (0.999, 0.37)), (2, 6, 1.3, None)]
    assert lib.sh_seq_render_groups(*call(n=1000, gains=None, ngains=0, pans=None, npans=0, groups=grp(*native(groups)))) == N.SH_OK
    want = grouped(("pile", 2), subs, None, None, groups, None, 2)[2]
    assert out.download_bytes(2000) == want[:2000] and out.download_bytes(2000, 2000) == b"\x5a" * 2000 and bytes(rows) == untouched
    # a mono song has group faders, and an empty window zeroes the rows, the groups' as well
    assert lib.sh_seq_render_groups(*call(song=mono, n=0, gains=None, ngains=0, pans=None, npans=0, meters=rows, nmeters=9,
                                          groups=grp((0, 2, 0.8, 1.0, 1.0), (2, 3, 1.0, 1.0, 1.0)))) == N.SH_OK
    assert bytes(rows) == bytes(9 * 40) + untouched[9 * 40:]
    auto.free()
    for s in (seq, flat_song, mono, three):
        s.free()
