"""GPU parity of the rides of the BUSES of a compiled song of tracks -- CompiledSequence.automation(lanes, master=, groups=) and
render(automation=, groups=) / N.SeqAutomation(..., ngroups) / sh_seq_auto_create_buses, sh_seq_render_auto, sh_seq_render_groups -- byte
for byte against the chain below, the only definition of correct, written here with Python ints and floats over the sub-mixes of
tests/seqcases.subs_of and live ``audioop``.  With ``ride(x, pieces)`` ::

    for (a, b, v0, v1) in pieces:                                    # song frames
        n = float((b - a) * nch)
        for k in range((b - a) * nch):                               # k counts interleaved SAMPLES from the piece's first, in the SONG
            x[a * nch + k] = int(x[a * nch + k] * (k * (v1 - v0) / n + v0))      # a Python float product, truncated toward zero

the song is ::

    master = silence
    for t: sub = the track folded on its own; audioop.mul(gains[t]); ride(sub, lanes[t]); Sample.stereo(pans[t])
           if t lies in group g:
               bus = silence at first_g;  bus = audioop.add(bus, sub)
               if t == end_g - 1:
                   if gain_g != 1.0: bus = audioop.mul(bus, gain_g)  # over the saturated sum
                   ride(bus, group_lanes[g])                         # behind the group's gain, in front of its pan
                   if pan_g is not None: bus = Sample.stereo(lf_g, rf_g)
                   master = audioop.add(master, bus)
           else: master = audioop.add(master, sub)
    if master_gain != 1.0: master = audioop.mul(master, master_gain)
    ride(master, master_lane)                                        # behind the master's gain, on the saturated master

Expected bytes never come from the product.  Rate 8192 and the three-track, four-tile songs of the neighbouring files (at most 8192
samples), one mono ("bus") and one stereo ("balance"); the search has a song of its own, long enough for 513 pieces.  Of the wrong forms,
"k counts frames" and "the group's ride behind its pan" exist in a stereo song alone."""
import audioop
import ctypes as C
import math

import numpy as np
import pytest

from tests.seqcases import (GAINS, RATE, _ev, as_samples, in_a_child_under_the_other_alignment_scheme, ints, raw_tracks, render_window, row_of,
                            subs_of, the_song, windows, with_samples)
from tests.seqref import LANE, TILE, balance, differs, factors, pcm

pytestmark = pytest.mark.gpu

KINDS = ["bus", "balance"]                                  # a mono and a stereo song
WIDTHS = [1, 2, 4]
ZERO = ((0, 0), (0, 0))
RIGHT, GROUP_RIDE_FIRST, GROUP_RIDE_BEHIND_PAN, PER_TRACK, MASTER_RIDE_FIRST, FLOORED, MUL_HOLD, K_WINDOW, K_FRAMES = \
    "right", "the group's ride in front of its gain", "the group's ride behind its pan", "the group's ride on each of its tracks", \
    "the master's ride in front of the master's gain", "floor instead of truncation", "audioop.mul for a hold", \
    "k counted from the window's start", "k counts frames"
WRONG = (GROUP_RIDE_FIRST, GROUP_RIDE_BEHIND_PAN, PER_TRACK, MASTER_RIDE_FIRST, FLOORED, MUL_HOLD, K_WINDOW, K_FRAMES)
STEREO_ONLY = (GROUP_RIDE_BEHIND_PAN, K_FRAMES)
HOW_A_PIECE_IS_READ = (FLOORED, MUL_HOLD, K_WINDOW, K_FRAMES)     # the forms that change the ride's own expression: on both bus levels


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def to_bytes(v, width):
    return np.asarray(v, dtype=np.int64).astype({1: np.int8, 2: "<i2", 4: "<i4"}[width]).tobytes()


def ride(data, width, nch, pieces, how=RIGHT, window=0):
    """the chain's ``ride`` on bytes of the song's length: Python ints and floats, sample by sample; or a wrong reading of a piece"""
    if not pieces:
        return data
    v = ints(data, width).tolist()
    for a, b, v0, v1 in pieces:
        if how == MUL_HOLD and v0 == v1:
            v[a * nch:b * nch] = ints(audioop.mul(to_bytes(v[a * nch:b * nch], width), width, v0), width).tolist()
            continue
        n = float((b - a) * nch)
        for k in range((b - a) * nch):
            at = a * nch + k
            if how == K_FRAMES:
                f = (k // nch) * (v1 - v0) / float(b - a) + v0
            elif how == K_WINDOW:
                if at < window:
                    continue
                f = (at - max(a * nch, window)) * (v1 - v0) / n + v0
            else:
                f = k * (v1 - v0) / n + v0
            y = v[at] * f                                       # a Python float product
            v[at] = math.floor(y) if how == FLOORED else int(y)      # truncated toward zero
    return to_bytes(v, width)


def pair(pan):
    return None if pan is None else factors(tuple(pan) if isinstance(pan, (tuple, list)) else pan)


def flat(pans):
    """pans as the C entry point takes them: left then right per track, (1.0, 1.0) where there is none"""
    return None if pans is None else [f for p in pans for f in ((1.0, 1.0) if p is None else pair(p))]


def native(groups):
    """the list as the C entry point takes it: (first, end, gain, left, right)"""
    return [(f, e, 1.0 if g is None else g) + ((1.0, 1.0) if p is None else pair(p)) for f, e, g, p in groups]


def mul(data, width, factor):
    return data if factor is None or factor == 1.0 else audioop.mul(data, width, factor)


_CHAIN = {}


def chain(key, subs, gains, lanes, pans, groups, master_gain, glanes, mlane, width, nch, how=RIGHT, window=0):
    """(the tracks as their bus takes them; the groups as the master takes them; the master's bytes; the groups behind their gain and in
    front of their ride), made once per key and setting.  ``lanes``: the tracks'; ``glanes``: one per group, or None; ``mlane``: the
    master's, or None.  ``how``: the chain, or one of its wrong forms."""
    groups = tuple(groups or ())
    at = (key, gains, lanes, pans, groups, master_gain, glanes, mlane, how, window)
    if at in _CHAIN:
        return _CHAIN[at]
    total = max([len(s) for s in subs] + [0])
    of = {t: k for k, (first, end, _g, _p) in enumerate(groups) for t in range(first, end)}
    read = how if how in HOW_A_PIECE_IS_READ else RIGHT
    out, posts, buses, scaled, bus = bytes(total), [], [None] * len(groups), [None] * len(groups), None
    for t, sub in enumerate(subs):
        sub = sub + bytes(total - len(sub))
        sub = mul(sub, width, None if gains is None else gains[t])
        sub = ride(sub, width, nch, None if lanes is None else lanes[t])
        if pans is not None and pans[t] is not None:
            sub = balance(sub, width, *pair(pans[t]))
        k = of.get(t)
        if k is None:
            posts.append(sub)
            out = audioop.add(out, sub, width)
            continue
        first, end, g, pan = groups[k]
        pieces = None if glanes is None or k >= len(glanes) else glanes[k]
        posts.append(sub)
        if how == PER_TRACK:
            sub = ride(sub, width, nch, pieces)
        if t == first:
            bus = bytes(total)
        bus = audioop.add(bus, sub, width)                      # saturating at every track of the group
        if t == end - 1:
            if how == GROUP_RIDE_FIRST:
                bus = ride(bus, width, nch, pieces)
            bus = mul(bus, width, g)
            scaled[k] = bus
            if how not in (GROUP_RIDE_FIRST, GROUP_RIDE_BEHIND_PAN, PER_TRACK):
                bus = ride(bus, width, nch, pieces, read, window)
            if pan is not None:
                bus = balance(bus, width, *pair(pan))
            if how == GROUP_RIDE_BEHIND_PAN:
                bus = ride(bus, width, nch, pieces)
            buses[k] = bus
            out = audioop.add(out, bus, width)                  # where the group's last track stands
    if how == MASTER_RIDE_FIRST:
        out = ride(out, width, nch, mlane)
    out = mul(out, width, master_gain)
    if how != MASTER_RIDE_FIRST:
        out = ride(out, width, nch, mlane, read, window)
    _CHAIN[at] = (posts, buses, out, scaled)
    return _CHAIN[at]


def silent(group):
    _f, _e, g, p = group
    return g == 0.0 or (p is not None and pair(p) == (0.0, 0.0))


def rows_of(key, subs, s, width, nch, a, b):
    """ntracks + 1 + ngroups rows: the tracks as their bus takes them (zero in a silent group, whose events are skipped), the master over
    the stored bytes, the groups as the master takes them, behind their ride and pan"""
    posts, buses, out, _scaled = chain(key, subs, s.gains, s.lanes, s.pans, s.groups, s.master, s.glanes, s.mlane, width, nch)
    mute = {t for g in s.groups or () if silent(g) for t in range(g[0], g[1])}
    return [ZERO if t in mute else row_of(ints(p, width)[a:b], a, nch) for t, p in enumerate(posts)] + [row_of(ints(out, width)[a:b], a, nch)] + \
        [row_of(ints(bus, width)[a:b], a, nch) for bus in buses]


# ---- the pieces, in song frames, chosen for where a lane can go wrong (tests/test_gpu_automation.py's lane_sets, for a bus) --------------
def parts(width, nch, total):
    """{name: one lane}; sample positions below are even, so they are whole frames of a stereo song as well"""
    T, L = TILE[width], LANE[width]
    w = T + 3 * L                                               # the pile-up window's first sample

    def fr(*pieces):
        assert all(a % nch == 0 and b % nch == 0 for a, b, _v0, _v1 in pieces)
        return tuple((a // nch, b // nch, v0, v1) for a, b, v0, v1 in pieces)
    return {
        "edges": fr((L + 2, 5 * L + 2, 0.2, 0.9), (5 * L + 2, 9 * L - 2, 0.9, 0.1),       # starts and ends mid-lane; two pieces meet mid-lane
                    (10 * L, 14 * L, 1.0, 0.3),                                          # on lane boundaries (a fade-out)
                    (15 * L + 2, 15 * L + 2 + nch, 0.25, 0.75),                          # one frame
                    (16 * L + 2, 18 * L, 0.5, 0.5), (18 * L + nch, 20 * L + 2, 0.37, 0.37),     # one frame apart; holds
                    (T, 2 * T, 0.3, 1.0),                                                # on tile boundaries (a fade-in)
                    (3 * T + 2 * L + 2, total, 0.8, 0.0)),                               # to the song's last frame
        "holds": fr((w - 80, w - 40, 0.0, 0.6), (w - 40, w, 1.0, 1.0), (w, w + 30, 0.6, 0.2), (w + 30, w + 60, 0.0, 0.0),      # a hold at 0.0
                    (w + 60, w + 200, 0.0, 0.37), (w + 200, w + 260, 0.37, 0.37), (w + 260, w + 300, 1.0, 1.0), (w + 300, w + 340, 1.0, 0.5)),
        "across": fr((T - 2 * L - 2, 3 * T + 3 * L + 2, 0.1, 1.0)),                      # one piece across three tiles
        "whole": fr((0, total, 0.9, 0.15)),                                              # over the whole song
        None: None,
    }


class Setting:
    """one desk: the tracks' gains, lanes and pans, the group list with the groups' lanes, the master's gain and lane"""

    def __init__(self, name, gains, lanes, pans, groups, master, glanes, mlane):
        self.name, self.gains, self.lanes, self.pans, self.groups, self.master, self.glanes, self.mlane = name, gains, lanes, pans, groups, master, glanes, mlane

    def chain(self, key, subs, width, nch, how=RIGHT, window=0):
        return chain(key, subs, self.gains, self.lanes, self.pans, self.groups, self.master, self.glanes, self.mlane, width, nch, how, window)


PANS = [(0.3, None, (1.5, 0.25)), (None, (0.999, 0.37), -0.37)]
# (first_track, end_track, gain, pan): tracks 0-1 with a gain above 1 and a pan, track 2 loose; tracks 1-2, so that the group closes behind
# the last run; two groups of one track, the second without an event in some tile of either song
LISTS = {
    "front": [(0, 2, 1.9, (0.999, 0.37))],
    "back": [(1, 3, -1.6, -0.37)],
    "idle": [(0, 1, 0.8, (1.5, 0.25)), (2, 3, 1.3, None)],
}
# (the list, gains, which of PANS, master, the tracks' lanes, the groups' lanes, the master's lane): every kind of piece on a group's
# lane and on the master's; in each a fade that starts in front of the pile-up window and a hold inside it, a master gain, a group gain
SETTINGS = [
    ("front", GAINS[0], 0, 0.7, ("whole", None, "edges"), ("edges",), "holds"),
    ("front", GAINS[3], 1, -1.3, (None, None, None), ("holds",), "across"),
    ("back", GAINS[3], 0, -1.3, ("across", "holds", None), ("whole",), "holds"),
    ("back", GAINS[0], 1, 0.7, (None, "edges", "whole"), ("holds",), "edges"),
    ("idle", GAINS[0], 1, -1.3, ("edges", "whole", "edges"), ("edges", "across"), "holds"),
    ("idle", GAINS[3], 0, 0.7, (None, "across", None), ("holds", "whole"), "edges"),
]


def song_of(kind, width):
    """(instruments, tracks, nch, the sub-mixes, total samples, the settings)"""
    instruments, tracks, nch, subs, total, _level = the_song(kind, width)
    assert total % nch == 0 and len(tracks) == 3
    p = parts(width, nch, total)
    settings = []
    for k, (name, gains, which, master_gain, lanes, glanes, mlane) in enumerate(SETTINGS):
        groups = tuple((f, e, g, pan if nch == 2 else None) for f, e, g, pan in LISTS[name])      # (a mono song has group faders, no pans)
        settings.append(Setting("%d: %s" % (k, name), gains, tuple(p[x] for x in lanes), PANS[which] if nch == 2 else None, groups, master_gain,
                                tuple(p[x] for x in glanes), p[mlane]))
    return instruments, tracks, nch, subs, total, settings


def native_auto(N, seq, s, nch, ntracks=3):
    """the lanes through sh_seq_auto_create_buses: the product's packer makes the table (an input)"""
    from synthesizer_amd import mixer
    lanes = tuple(() if lane is None else lane for lane in (s.lanes or (None,) * ntracks))
    segments, first = mixer.CompiledSequence._pack_lanes(lanes, nch, s.mlane or (), tuple(() if g is None else g for g in s.glanes or ()))
    assert len(first) == ntracks + 1 + len(s.glanes or ()) + 1
    return N.SeqAutomation(seq, segments, first, len(s.glanes or ()))


class WithBuses:
    """N.Sequence behind render_window, which calls render(first, n, out, out_sample): through sh_seq_render_groups (sh_seq_render_auto
    where the setting names no group)"""

    def __init__(self, seq, s, auto):
        self.seq, self.s, self.auto = seq, s, auto

    def render(self, a, n, out, out_sample, **kw):
        s = self.s
        return self.seq.render(a, n, out, out_sample, gains=None if s.gains is None else list(s.gains), pans=flat(s.pans), master=s.master,
                               groups=native(s.groups) if s.groups else None, automation=self.auto, **kw)


def metered(N, seq, s, auto, width, a, b, out_sample=0):
    """(rows, the rendered bytes, the guards intact) of a metered render into a 0x5A-filled buffer"""
    n = b - a
    inner = (out_sample + n) * width
    parent = N.DeviceBuffer.from_bytes(b"\x5a" * (64 + inner + 64))
    rows = WithBuses(seq, s, auto).render(a, n, parent.view(64, inner), out_sample, meters=True)
    got = parent.download_bytes(64 + inner + 64)
    at = 64 + out_sample * width
    return rows, got[at:at + n * width], got[:at] == b"\x5a" * at and got[at + n * width:] == b"\x5a" * 64


# ---- 1: the inputs tell the chain from its wrong forms (no device) -------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_inputs_tell_the_chain_from_every_wrong_form_inside_the_pile_up(kind, width):
    _instruments, _tracks, nch, subs, total, settings = song_of(kind, width)
    T, L = TILE[width], LANE[width]
    lo, hi = T + 3 * L, 3 * T + L                               # the pile-up window: it starts inside a fade of every setting
    top = 2 ** (8 * width - 1)
    clipped = 0
    for s in settings:
        assert s.master not in (None, 1.0) and all(g[2] != 1.0 for g in s.groups) and (nch == 1 or any(g[3] is not None for g in s.groups))
        bus_lanes = [lane for lane in s.glanes + (s.mlane,) if lane]
        assert any(a * nch < lo < b * nch and v0 != v1 for lane in bus_lanes for a, b, v0, v1 in lane), "no fade of a bus starts in front of the window"
        assert any(lo <= a * nch and b * nch <= hi and v0 == v1 for lane in bus_lanes for a, b, v0, v1 in lane), "no hold of a bus inside the window"
        _posts, _buses, want, scaled = s.chain((kind, width), subs, width, nch)
        plain = chain((kind, width), subs, s.gains, s.lanes, s.pans, s.groups, s.master, None, None, width, nch)[2]
        assert differs(want[lo * width:hi * width], plain[lo * width:hi * width]) > 0
        found = {}
        for how in WRONG:
            if nch == 1 and how in STEREO_ONLY:
                continue
            other = s.chain((kind, width), subs, width, nch, how, lo)[2]
            found[how] = differs(want[lo * width:hi * width], other[lo * width:hi * width])
        print("%s, width %d, setting %s: bytes of the pile-up window that differ: %s" % (kind, width, s.name, found))
        assert all(n > 0 for n in found.values()), (s.name, found)
        for k, (first, end, g, _pan) in enumerate(s.groups):     # a group gain above 1 saturates the bus in front of its ride
            if abs(g) > 1.0:
                low, high = audioop.minmax(scaled[k][lo * width:hi * width], width)
                clipped += high == top - 1 or low == -top
    assert clipped >= 2, "no group saturates behind its gain"


# ---- 2: the whole song, chunks and render_into, through the mixer ---------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_whole_song_chunks_and_an_odd_offset_are_the_reference_chain_byte_for_byte(gpu, kind, width):
    from synthesizer_amd import mixer
    N = gpu
    instruments, tracks, nch, subs, total, settings = song_of(kind, width)
    samples = as_samples(instruments, width, RATE)
    frames = 333
    assert (nch * frames) % LANE[width]
    with mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, nch, width) as cs:
        assert cs.ntracks == 3 and cs.frames * nch == total
        for s in settings:
            want = s.chain((kind, width), subs, width, nch)[2]
            groups = [g for g in s.groups]
            with cs.automation(s.lanes, master=s.mlane, groups=s.glanes) as auto:
                assert auto.rides == len(s.glanes) and auto.master
                kw = dict(gains=s.gains, pans=s.pans, master=s.master, groups=groups, automation=auto)
                got = bytes(cs.render(**kw).view_frame_data())
                assert got == want, "setting %s: %d bytes differ" % (s.name, differs(got, want))
                parts_ = list(cs.chunks(frames, **kw))           # chunks that cut pieces and are no multiple of the lane width
                assert len(parts_) == -(-cs.frames // frames) > 4 and b"".join(bytes(p.view_frame_data()) for p in parts_) == want, s.name
                # render_into one sample off, of a window that starts mid-lane
                a, n = (TILE[width] + 3 * LANE[width]) // nch + 1, 700
                buf = N.DeviceBuffer.from_bytes(b"\x5a" * (n * nch * width + 2 * width))
                assert cs.render_into(buf, width, a, n, **kw) is None
                back = buf.download_bytes(n * nch * width + 2 * width)
                assert back[width:-width] == want[a * nch * width:(a + n) * nch * width] and back[:width] == back[-width:] == b"\x5a" * width, s.name
        # a master ride without groups=: the fade-in, hold and fade-out of the whole mix
        s = settings[0]
        fade = ((0, 300, 0.0, 1.0), (300, cs.frames - 500, 0.8, 0.8), (cs.frames - 500, cs.frames, 1.0, 0.0))
        want = chain((kind, width), subs, s.gains, s.lanes, s.pans, None, s.master, None, fade, width, nch)[2]
        with cs.automation(s.lanes, master=fade) as auto:
            assert bytes(cs.render(gains=s.gains, pans=s.pans, master=s.master, automation=auto).view_frame_data()) == want
            levels = cs.render(gains=s.gains, pans=s.pans, master=s.master, automation=auto, meters=True)[1]
            m = row_of(ints(want, width), 0, nch)
            assert (levels.master.peak, levels.master.sum_squares) == (m if nch == 2 else ((m[0][0],) * 2, (m[1][0],) * 2)) and levels.groups == []
        with cs.automation([None] * 3, master=fade) as auto:    # and with nothing else on the desk
            assert bytes(cs.render(automation=auto).view_frame_data()) == chain((kind, width), subs, None, None, None, None, None, None, fade, width, nch)[2]
        # a group at gain 0.0 with a ride gives zeros: its tracks are skipped, the loose track and the master's ride stay
        muted = [(0, 2, 0.0, None)]
        want = chain((kind, width), subs, s.gains, None, None, muted, None, (s.glanes[0],), fade, width, nch)[2]
        assert want == ride(mul(subs[2] + bytes(len(want) - len(subs[2])), width, s.gains[2]), width, nch, fade)
        with cs.automation([None] * 3, master=fade, groups=[s.glanes[0]]) as auto:
            out, levels = cs.render(gains=s.gains, groups=muted, automation=auto, meters=True)
            assert bytes(out.view_frame_data()) == want
            assert [(r.peak, r.sum_squares) for r in levels.tracks[:2] + levels.groups] == [ZERO] * 3 and levels.tracks[2].peak != (0, 0)
            with pytest.raises(ValueError, match="the automation rides group 0, and this render names 0 groups"):
                cs.render(automation=auto)


# ---- 3: windows, through the C entry points -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_window_holds_its_slice_and_nothing_beside_it_is_written(gpu, kind, width):
    N = gpu
    instruments, tracks, nch, subs, total, settings = song_of(kind, width)
    wins = windows("balance", width, total)
    assert any(a % 2 for a, _b in wins), "no window starts on an odd sample"
    seq, _samples = raw_tracks(N, instruments, tracks, nch, width)
    for s in settings:
        assert any(a * nch < w0 < b * nch for lane in s.glanes + (s.mlane,) for a, b, _v0, _v1 in lane or () for w0, _w1 in wins), "no window starts inside a piece"
        auto = native_auto(N, seq, s, nch)
        want = s.chain((kind, width), subs, width, nch)[2]
        for a, b in wins:
            for out_sample in (0, 1):
                got, front, back = render_window(N, WithBuses(seq, s, auto), width, a, b, out_sample)
                assert got == want[a * width:b * width], (s.name, a, b, out_sample, differs(got, want[a * width:b * width]))
                assert front == b"\x5a" * 64 and back == b"\x5a" * 64, (a, b, out_sample)
        auto.free()
    seq.free()


def test_the_windows_at_16_bits_under_the_other_alignment_scheme(gpu):
    in_a_child_under_the_other_alignment_scheme(
        __file__, ["test_every_window_holds_its_slice_and_nothing_beside_it_is_written[%s-2]" % kind for kind in KINDS])


# ---- 4: meters ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_rows_read_a_group_behind_its_ride_and_the_master_over_the_stored_bytes(gpu, kind, width):
    N = gpu
    instruments, tracks, nch, subs, total, settings = song_of(kind, width)
    T, L = TILE[width], LANE[width]
    wins = [(0, total), (T + 3 * L + 1, 3 * T + L), (2 * T + 5, 3 * T - 7), (T - 1, T + 1)]      # whole, odd, idle, across a tile's edge
    seq, _samples = raw_tracks(N, instruments, tracks, nch, width)
    for s in settings:
        auto = native_auto(N, seq, s, nch)
        want_bytes = s.chain((kind, width), subs, width, nch)[2]
        unridden = Setting(s.name, s.gains, s.lanes, s.pans, s.groups, s.master, None, None)
        whole = rows_of((kind, width), subs, s, width, nch, 0, total)
        plain = rows_of((kind, width), subs, unridden, width, nch, 0, total)
        assert whole[:3] == plain[:3] and whole[3] != plain[3] and whole[4:] != plain[4:]      # the buses' rows move, the tracks' do not
        for a, b in wins:
            want = rows_of((kind, width), subs, s, width, nch, a, b)
            assert len(want) == 3 + 1 + len(s.groups)
            for out_sample in (0, 1):
                rows, got, guards = metered(N, seq, s, auto, width, a, b, out_sample)
                assert rows == want, "setting %s, window [%d, %d) at %d:\n%s\n%s" % (s.name, a, b, out_sample, rows, want)
                assert got == want_bytes[a * width:b * width] and guards, (s.name, a, b, out_sample)
            if 2 * T <= a and b <= 3 * T:
                assert rows == [ZERO] * (4 + len(s.groups))     # the idle tile: a ride over zeros is zero
        auto.free()
    # a master ride through sh_seq_render_auto: ntracks + 1 rows
    s = settings[1]
    alone = Setting("master alone", s.gains, s.lanes, s.pans, (), s.master, (), s.mlane)
    auto = native_auto(N, seq, alone, nch)
    for a, b in wins[:2]:
        rows, got, guards = metered(N, seq, alone, auto, width, a, b, 1)
        assert rows == rows_of((kind, width), subs, alone, width, nch, a, b) and len(rows) == 4 and guards
        assert got == alone.chain((kind, width), subs, width, nch)[2][a * width:b * width]
    auto.free()
    seq.free()


# ---- 5: the search: a master lane of 513 pieces ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("width", WIDTHS)
def test_a_master_lane_of_513_three_frame_pieces_with_one_frame_gaps(gpu, width, nch):
    N = gpu
    T, L = TILE[width], LANE[width]
    rng = np.random.default_rng(6130 + 10 * width + nch)
    frames = 513 * 4 + 41                                       # the pieces end 42 frames before the song does
    instruments = [(pcm(rng, width, frames * nch, 0.9), nch), (pcm(rng, width, 500 * nch, 0.9), nch)]
    tracks = [[_ev(0, 0, 0.8)], [_ev(300, 1, 1.2)]]
    subs = subs_of(instruments, tracks, width, nch)
    total = max(len(s) for s in subs) // width
    assert total == frames * nch and total > T and total % L
    vols = [0.0, 0.25, 0.5, 0.37, 1.0, 0.9, 0.1]
    many = tuple((4 * i, 4 * i + 3, vols[i % 7], vols[(3 * i + 1) % 7]) for i in range(513))
    assert len(many) == 513 and all(many[i + 1][0] - many[i][1] == 1 for i in range(512))
    key = ("search", width, nch)
    s = Setting("513", (1.7, 0.8), (((100, 700, 1.0, 0.2),), None), None, ((0, 2, 0.9, None),), 0.9, (((50, 900, 0.3, 1.0),),), many)
    want = s.chain(key, subs, width, nch)[2]
    assert differs(want, chain(key, subs, s.gains, s.lanes, None, s.groups, s.master, s.glanes, None, width, nch)[2]) > total // 4
    seq, _samples = raw_tracks(N, instruments, tracks, nch, width)
    auto = native_auto(N, seq, s, nch, ntracks=2)
    for a, b in ((0, total), (T - 3, T + L + 1), (total - T - 5, total), (3 * nch * 4 + 1, total - 7)):
        for out_sample in (0, 1):
            got, front, back = render_window(N, WithBuses(seq, s, auto), width, a, b, out_sample)
            assert got == want[a * width:b * width], (a, b, out_sample, differs(got, want[a * width:b * width]))
            assert front == back == b"\x5a" * 64
    rows, got, guards = metered(N, seq, s, auto, width, 0, total)
    assert rows == rows_of(key, subs, s, width, nch, 0, total) and got == want and guards
    auto.free()
    seq.free()


# ---- 6: far out --------------------------------------------------------------------------------------------------------------------------
MAX = 2 ** 32 - 65536                                       # shq::MAX_TRACK_SAMPLES


class _Pack:
    """stands where the native module stands in raw_tracks and keeps what it would hand N.Sequence (tests/test_gpu_sequence_far.py's way)"""

    @staticmethod
    def Sequence(*args, **kw):
        return args, kw


@pytest.mark.parametrize("kind, width, base, which", [("balance", 2, "top", 4), ("bus", 4, "mid", 0)])
def test_bus_pieces_whose_origin_lies_past_2_31_samples(gpu, kind, width, base, which):
    """the near song B samples further out, its pieces B / nch frames further out: the far window [B + a, B + b) holds the near bytes
    [a, b), because k and n are relative to the piece"""
    N = gpu
    instruments, tracks, nch, subs, total, settings = song_of(kind, width)
    T, L = TILE[width], LANE[width]
    B = {"mid": 2 ** 31 - T, "top": MAX - 4 * T}[base]
    assert B % T == 0 and B % 2 == 0
    (args, kw), _samples = raw_tracks(_Pack, instruments, tracks, nch, width)
    bufs, table, segtab, _w, _nch, packed = args
    assert packed == total
    shifted = table.copy()
    shifted["dst_sample"] += np.uint64(B)
    seq = N.Sequence(bufs, shifted, segtab, width, nch, B + total, track_first=kw["track_first"])
    s = settings[which]

    def far(lane):
        return None if lane is None else tuple((a + B // nch, b + B // nch, v0, v1) for a, b, v0, v1 in lane)
    moved = Setting(s.name, s.gains, tuple(far(x) for x in s.lanes), s.pans, s.groups, s.master, tuple(far(x) for x in s.glanes), far(s.mlane))
    wins = [(T + 3 * L, 3 * T + L), (T + 3 * L + 71, T + 3 * L + 150), (3 * T + 3 * L, total), (T - 5, T + L + 3)]
    assert any(a * nch > 2 ** 31 and a * nch < B + w0 < b * nch for lane in moved.glanes + (moved.mlane,) for a, b, _v0, _v1 in lane for w0, _w1 in wins), \
        "no window starts inside a bus piece whose origin lies past 2^31"
    auto = native_auto(N, seq, moved, nch)
    want = s.chain((kind, width), subs, width, nch)[2]
    for a, b in wins:
        got, front, back = render_window(N, WithBuses(seq, moved, auto), width, B + a, B + b, 1)
        assert got == want[a * width:b * width], "window B + [%d, %d): %d bytes differ" % (a, b, differs(got, want[a * width:b * width]))
        assert front == back == b"\x5a" * 64
    rows = metered(N, seq, moved, auto, width, B + wins[0][0], B + wins[0][1])[0]
    assert rows == rows_of((kind, width), subs, s, width, nch, *wins[0])
    auto.free()
    seq.free()


# ---- 7: what the C entry points refuse, and a handle without a bus segment -------------------------------------------------------------------
def test_the_entry_points_refuse_on_the_host_and_a_handle_without_bus_segments_renders_as_before(gpu):
    N = gpu
    lib = N.lib()
    from synthesizer_amd import mixer
    instruments, tracks, nch, subs, total, settings = song_of("balance", 2)
    seq, _samples = raw_tracks(N, instruments, tracks, 2, 2)

    def create(rows_, first, ntracks=3, ngroups=0, song=seq):
        t = np.zeros(len(rows_), dtype=N.ENV_SEGMENT_DTYPE)
        for k, r in enumerate(rows_):
            t[k] = tuple(r) + (0,) * (8 - len(r))
        h = C.c_void_p()
        rc = lib.sh_seq_auto_create_buses(song.handle, t.ctypes.data if len(t) else None, len(t), (C.c_uint32 * len(first))(*first), ntracks, ngroups, C.byref(h))
        assert not h.value or rc == N.SH_OK
        if h.value:
            lib.sh_seq_auto_destroy(h)
        return rc, lib.sh_last_error()
    good = (100, 0, 1.0, 0.5, 100.0, 0.25, 1)
    assert create([good], [0, 0, 0, 0, 1])[0] == N.SH_OK                                # the master's lane, no group lane
    assert create([good], [0, 0, 0, 0, 0] + [0] * 7 + [1], ngroups=8)[0] == N.SH_OK    # the last of eight group lanes
    nan = float("nan")
    for what, rows_, first, kw, message in (
        ("nine group lanes", [good], [0] * 13 + [1], dict(ngroups=9), b"9 group lanes, 0 to 8"),
        ("another track count", [good], [0, 0, 0, 1], dict(ntracks=2), b"2 lanes for 3 tracks"),
        ("a first that does not end at the table", [good], [0, 0, 0, 0, 0], {}, b"seg_first starts at 0 and ends at nsegments"),
        ("a first that decreases at a group", [good, good], [0, 0, 0, 2, 1, 2], dict(ngroups=1), b"seg_first decreases at group 0"),
        ("a reserved word on the master", [good + (1,)], [0, 0, 0, 0, 1], {}, b"master: segment 0: reserved must be 0"),
        ("an end past the song on a group", [(total + 2, 0, 1.0, 0.5, total + 2.0, 0.25, 1)], [0, 0, 0, 0, 0, 0, 1], dict(ngroups=2),
         b"group 1: segment 0: ends not ascending or beyond the song"),
        ("a fade-out segment", [(100, 0, 1.0, 0.5, 100.0, 0.0, 2)], [0, 0, 0, 0, 1], {}, b"master: segment 0: kind 2 not 0 or 1"),
        ("a mul", [(100, 0, 0.5, 0.5, 100.0, 0.25, 1)], [0, 0, 0, 0, 0, 1], dict(ngroups=1), b"group 0: segment 0: mul must be 1.0"),
        ("an origin that is not the first sample", [(100, 4, 1.0, 0.5, 100.0, 0.25, 1)], [0, 0, 0, 0, 1], {}, b"master: segment 0: a move's origin is its first sample"),
        ("numsamples too small", [good, (200, 100, 1.0, 0.5, 99.0, 0.25, 1)], [0, 0, 0, 0, 2], {}, b"master: segment 1: numsamples shorter than the move"),
        ("a volume above 1", [(100, 0, 1.0, 0.8, 100.0, 0.25, 1)], [0, 0, 0, 0, 0, 1], dict(ngroups=1), b"group 0: segment 0: a volume is not finite or outside 0 .. 1"),
        ("a volume that is no number", [(100, 0, 1.0, 0.0, 100.0, nan, 1)], [0, 0, 0, 0, 1], {}, b"master: segment 0: a volume is not finite or outside 0 .. 1"),
    ):
        rc, err = create(rows_, first, **kw)
        assert rc == N.SH_ERR_INVALID and err.startswith(b"sh_seq_auto_create_buses") and message in err, (what, err)
    # a ride on a group that the call does not name: refused, nothing written
    s = settings[4]                                             # rides groups 0 and 1
    auto = native_auto(N, seq, s, 2)
    out = N.DeviceBuffer.from_bytes(b"\x5a" * 4000)
    one = (N.SeqGroup * 1)(N.SeqGroup(0, 1, 0.8, 1.0, 1.0))
    assert lib.sh_seq_render_auto(seq.handle, 0, 1000, out.handle, 0, None, 0, None, 0, 1.0, None, 0, auto.handle) == N.SH_ERR_INVALID
    assert b"sh_seq_render_auto: the automation rides group 1" in lib.sh_last_error()
    assert lib.sh_seq_render_groups(seq.handle, 0, 1000, out.handle, 0, None, 0, None, 0, 1.0, None, 0, auto.handle, one, 1) == N.SH_ERR_INVALID
    assert b"sh_seq_render_groups: the automation rides group 1, and this call names 1 groups" in lib.sh_last_error()
    assert out.download_bytes(4000) == b"\x5a" * 4000
    auto.free()
    # a handle of sh_seq_auto_create_buses without a segment on a bus lane renders what sh_seq_auto_create's renders, with and without groups
    lanes = tuple(() if lane is None else lane for lane in s.lanes)
    segments, first = mixer.CompiledSequence._pack_lanes(lanes, 2)
    plain = N.SeqAutomation(seq, segments, first)
    empty = N.SeqAutomation(seq, segments, first + [first[-1]] * 3, 2)
    for groups in ((), s.groups):
        base = Setting("no bus lanes", s.gains, s.lanes, s.pans, groups, s.master, None, None)
        want = base.chain(("balance", 2), subs, 2, 2)[2]
        for auto in (plain, empty):
            got, front, back = render_window(N, WithBuses(seq, base, auto), 2, 3, total - 5, 1)
            assert got == want[3 * 2:(total - 5) * 2] and front == back == b"\x5a" * 64
    plain.free()
    empty.free()
    seq.free()
