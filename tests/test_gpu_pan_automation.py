"""GPU parity of the PAN RIDES of a compiled stereo song of tracks -- CompiledSequence.automation(lanes, pans=, group_pans=) and
render(automation=, groups=) / N.SeqAutomation(..., pan_segments, pan_first) / sh_seq_auto_create_pans, sh_seq_render_auto,
sh_seq_render_groups -- byte for byte against the chain below, the only definition of correct, written here with Python ints and floats
over the sub-mixes of tests/seqcases.subs_of and live ``audioop``.  With ``ride(x, pieces)`` the fader moves of
tests/test_gpu_bus_automation.py and ``pan_step(x, pieces, static)`` ::

    y = Sample.stereo(x, *static)                                    # outside the pieces: the static pan (none where static is None)
    for (a, b, p0, p1) in pieces:                                    # song frames
        n = b - a
        for k in range(n):                                           # k counts FRAMES from the piece's first, in the SONG
            p = k * (p1 - p0) / n + p0                               # Python floats, in this order
            L, R = x[a + k]
            y[a + k] = (int(L * (1.0 - p) / 2.0), int(R * (1.0 + p) / 2.0))      # Sample.pan(lfo=...): truncated toward zero

the song is ::

    master = silence
    for t: sub = the track folded on its own; audioop.mul(gains[t]); ride(sub, lanes[t]); pan_step(sub, pan_lanes[t], pans[t])
           if t lies in group g:
               bus = silence at first_g;  bus = audioop.add(bus, sub)
               if t == end_g - 1:
                   if gain_g != 1.0: bus = audioop.mul(bus, gain_g)
                   ride(bus, group_lanes[g]); pan_step(bus, group_pan_lanes[g], pan_g)
                   master = audioop.add(master, bus)
           else: master = audioop.add(master, sub)
    if master_gain != 1.0: master = audioop.mul(master, master_gain)
    ride(master, master_lane)

and a track or group whose static factors are both exactly 0.0 gives silence whatever its pan lane holds (its events are skipped).
Expected bytes never come from the product.  Rate 8192 and the stereo three-track, four-tile song of the neighbouring files (at most 8192
samples); the search has a song of its own, long enough for 513 pieces."""
import ctypes as C
import math

import audioop
import numpy as np
import pytest

from tests.seqcases import (GAINS, RATE, _ev, as_samples, in_a_child_under_the_other_alignment_scheme, ints, raw_tracks, render_window, row_of,
                            subs_of, the_song, windows, with_samples)
from tests.seqref import LANE, TILE, balance, differs, pcm
from tests.test_gpu_bus_automation import LISTS, MAX, PANS, WithBuses, _Pack, flat, metered, mul, native, pair, ride, to_bytes
from tests.test_gpu_bus_automation import parts as fader_parts

pytestmark = pytest.mark.gpu

KIND = "balance"                                            # the stereo song
WIDTHS = [1, 2, 4]
ZERO = ((0, 0), (0, 0))
RIGHT, K_SAMPLES, N_SAMPLES, FLOORED, STEREO_HOLD, ON_TOP, SWAPPED, BEFORE_GAIN, BEFORE_FADER, GROUP_BEFORE_GAIN, GROUP_BEFORE_RIDE = \
    "right", "k and n counted in samples", "n counted in samples", "floor instead of truncation", "Sample.stereo for a hold", \
    "the ride on top of the static pan", "left and right swapped", "the ride in front of the gain", "the ride in front of the fader move", \
    "the group's pan ride in front of its gain", "the group's pan ride in front of its fader ride"
HOW_A_PIECE_IS_READ = (K_SAMPLES, N_SAMPLES, FLOORED, STEREO_HOLD, ON_TOP, SWAPPED)      # on both levels
WRONG = HOW_A_PIECE_IS_READ + (BEFORE_GAIN, BEFORE_FADER, GROUP_BEFORE_GAIN, GROUP_BEFORE_RIDE)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def pan_step(data, width, pieces, static, how=RIGHT):
    """the chain's ``pan_step`` on stereo bytes of the song's length: Python ints and floats, frame by frame; or a wrong reading of a piece"""
    base = data if static is None else balance(data, width, *pair(static))
    if not pieces:
        return base
    x, y = ints(data, width).tolist(), ints(base, width).tolist()
    src = y[:] if how == ON_TOP else x
    for a, b, p0, p1 in pieces:
        if how == STEREO_HOLD and p0 == p1:
            y[2 * a:2 * b] = ints(balance(to_bytes(x[2 * a:2 * b], width), width, (1.0 - p0) / 2.0, (1.0 + p0) / 2.0), width).tolist()
            continue
        n = b - a
        for k in range(n):
            pl = pr = k * (p1 - p0) / n + p0
            if how == K_SAMPLES:
                pl, pr = (2 * k) * (p1 - p0) / (2 * n) + p0, (2 * k + 1) * (p1 - p0) / (2 * n) + p0
            elif how == N_SAMPLES:
                pl = pr = k * (p1 - p0) / (2 * n) + p0
            if how == SWAPPED:
                pl, pr = -pl, -pr
            left, right = src[2 * (a + k)] * (1.0 - pl) / 2.0, src[2 * (a + k) + 1] * (1.0 + pr) / 2.0
            y[2 * (a + k)] = math.floor(left) if how == FLOORED else int(left)
            y[2 * (a + k) + 1] = math.floor(right) if how == FLOORED else int(right)
    return to_bytes(y, width)


class Setting:
    """one desk: the tracks' gains, fader lanes, static pans and pan lanes, the group list with the groups' fader and pan lanes, the master's
    gain and lane"""

    def __init__(self, name, gains, lanes, pans, groups, master, glanes, mlane, tpans, gpans):
        self.name, self.gains, self.lanes, self.pans, self.groups, self.master, self.glanes, self.mlane = name, gains, lanes, pans, groups, master, glanes, mlane
        self.tpans, self.gpans = tpans, gpans

    def without_pan_lanes(self):
        return Setting(self.name + ", no pan lanes", self.gains, self.lanes, self.pans, self.groups, self.master, self.glanes, self.mlane, None, None)


_CHAIN = {}


def chain(key, subs, s, width, how=RIGHT):
    """(the tracks as their bus takes them; the groups as the master takes them; the master's bytes), made once per key, setting and form"""
    at = (key, s.name, how)
    if at in _CHAIN:
        return _CHAIN[at]
    groups = tuple(s.groups or ())
    total = max(len(x) for x in subs)
    of = {t: k for k, (first, end, _g, _p) in enumerate(groups) for t in range(first, end)}
    read = how if how in HOW_A_PIECE_IS_READ else RIGHT
    out, posts, buses, bus = bytes(total), [], [None] * len(groups), None
    for t, sub in enumerate(subs):
        sub = sub + bytes(total - len(sub))
        gain = None if s.gains is None else s.gains[t]
        lane = None if s.lanes is None else s.lanes[t]
        plane = None if s.tpans is None else s.tpans[t]
        static = None if s.pans is None else s.pans[t]
        if how == BEFORE_GAIN:
            sub = ride(mul(pan_step(sub, width, plane, static), width, gain), width, 2, lane)
        elif how == BEFORE_FADER:
            sub = ride(pan_step(mul(sub, width, gain), width, plane, static), width, 2, lane)
        else:
            sub = pan_step(ride(mul(sub, width, gain), width, 2, lane), width, plane, static, read)
        if static is not None and pair(static) == (0.0, 0.0):      # muted by its static factors: skipped, pan lane or not
            sub = bytes(total)
        posts.append(sub)
        k = of.get(t)
        if k is None:
            out = audioop.add(out, sub, width)
            continue
        first, end, g, pan = groups[k]
        glane = None if s.glanes is None or k >= len(s.glanes) else s.glanes[k]
        gplane = None if s.gpans is None or k >= len(s.gpans) else s.gpans[k]
        if t == first:
            bus = bytes(total)
        bus = audioop.add(bus, sub, width)
        if t == end - 1:
            if how == GROUP_BEFORE_GAIN:
                bus = ride(mul(pan_step(bus, width, gplane, pan), width, g), width, 2, glane)
            elif how == GROUP_BEFORE_RIDE:
                bus = ride(pan_step(mul(bus, width, g), width, gplane, pan), width, 2, glane)
            else:
                bus = pan_step(ride(mul(bus, width, g), width, 2, glane), width, gplane, pan, read)
            if pan is not None and pair(pan) == (0.0, 0.0):
                bus = bytes(total)
            buses[k] = bus
            out = audioop.add(out, bus, width)
    out = ride(mul(out, width, s.master), width, 2, s.mlane)
    _CHAIN[at] = (posts, buses, out)
    return _CHAIN[at]


def silent(group):
    _f, _e, g, p = group
    return g == 0.0 or (p is not None and pair(p) == (0.0, 0.0))


def rows_of(key, subs, s, width, a, b):
    """ntracks + 1 + ngroups rows: the tracks behind their pan step (zero where muted or in a silent group), the master over the stored
    bytes, the groups behind their ride and pan step"""
    posts, buses, out = chain(key, subs, s, width)
    mute = {t for g in s.groups or () if silent(g) for t in range(g[0], g[1])}
    return [ZERO if t in mute else row_of(ints(p, width)[a:b], a, 2) for t, p in enumerate(posts)] + [row_of(ints(out, width)[a:b], a, 2)] + \
        [row_of(ints(bus, width)[a:b], a, 2) for bus in buses]


# ---- the pan pieces, in song frames, chosen for where a pan lane can go wrong ----------------------------------------------------------------
def pan_parts(width, total):
    T, L = TILE[width], LANE[width]
    F, frames = T // 2, total // 2
    w = (T + 3 * L) // 2                                        # the pile-up window's first frame
    return {
        "edges": ((3, 4, 0.5, 0.5),                             # one frame
                  (10, 200, -1.0, 1.0),                         # wholly inside tile 0: from one end to the other
                  (F - 150, F + 4, 1.0, -1.0),                  # across a tile's edge
                  (F + 4, w + 20, 0.8, -0.3),                   # adjacent, with a jump in pan; the pile-up window starts inside it
                  (w + 20, w + 60, 0.0, 0.0),                   # a hold at 0.0, adjacent
                  (w + 70, w + 110, -1.0, -1.0), (w + 120, w + 160, 1.0, 1.0),      # holds at both ends
                  (w + 170, w + 230, -0.6, 0.9),
                  (3 * F + 5, frames, 0.3, -1.0)),              # to the song's last frame
        "holds": ((w - 30, w + 40, 0.0, 0.0), (w + 40, w + 41, 1.0, 1.0), (w + 100, w + 180, -0.37, -0.37), (3 * F, 3 * F + 60, 0.0, 0.0)),
        "across": ((F - 40, 3 * F + 20, -0.9, 0.7),),           # one piece across three tiles
        "whole": ((0, frames, 0.9, -0.15),),
        None: None,
    }


# (the group list, gains, which of PANS, master, the tracks' fader lanes, the groups' fader lanes, the master's lane, the tracks' pan lanes,
# the groups' pan lanes).  PANS[0] gives track 0 a static pan 0.3 and track 2 the pair (1.5, 0.25) outside their pieces.
SETTINGS = [
    ("front", GAINS[0], 0, 0.7, ("whole", None, "edges"), ("edges",), "holds", ("edges", "whole", "holds"), ("across",)),
    ("back", GAINS[3], 1, -1.3, (None, "holds", None), ("whole",), None, (None, "across", "edges"), ("holds",)),
    ("idle", GAINS[0], 1, -1.3, ("edges", "whole", "edges"), ("edges", "across"), "holds", ("holds", "edges", "whole"), ("edges", "whole")),
    (None, GAINS[3], 0, 0.7, (None, "across", None), (), "edges", ("edges", None, "across"), ()),       # no group: sh_seq_render_auto
    ("front", None, 1, None, (None, None, None), (None,), None, ("whole", "edges", None), ("edges",)),   # pan lanes and nothing else that moves
]


def song_of(width):
    """(instruments, tracks, the sub-mixes, total samples, the settings)"""
    instruments, tracks, nch, subs, total, _level = the_song(KIND, width)
    assert nch == 2 and total % 2 == 0 and len(tracks) == 3 and 3 * TILE[width] < total < 4 * TILE[width]
    assert any(int(v) < 0 for sub in subs for v in ints(sub, width)[:64])
    f, p = fader_parts(width, 2, total), pan_parts(width, total)
    settings = []
    for k, (name, gains, which, master_gain, lanes, glanes, mlane, tpans, gpans) in enumerate(SETTINGS):
        settings.append(Setting("%d: %s" % (k, name), gains, tuple(f[x] for x in lanes), PANS[which], tuple(LISTS[name]) if name else (), master_gain,
                                tuple(f[x] for x in glanes), f[mlane], tuple(p[x] for x in tpans), tuple(p[x] for x in gpans)))
    return instruments, tracks, subs, total, settings


def native_auto(N, seq, s, ntracks=3):
    """the lanes through sh_seq_auto_create_pans: the product's packers make the tables (inputs)"""
    from synthesizer_amd import mixer
    ngroups = max(len(s.glanes or ()), len(s.gpans or ()))

    def lanes_of(lanes, n):
        lanes = tuple(() if lane is None else lane for lane in lanes or ())
        return lanes + ((),) * (n - len(lanes))
    segments, first = mixer.CompiledSequence._pack_lanes(lanes_of(s.lanes, ntracks), 2, s.mlane or (), lanes_of(s.glanes, ngroups), buses=True)
    pan_segments, pan_first = mixer.CompiledSequence._pack_pan_lanes(lanes_of(s.tpans, ntracks), lanes_of(s.gpans, ngroups))
    assert len(first) == ntracks + 1 + ngroups + 1 and len(pan_first) == ntracks + ngroups + 1
    return N.SeqAutomation(seq, segments, first, ngroups, pan_segments, pan_first)


def inside(pieces_of_lanes, total):
    """a mask over the song's samples: the frames of every piece of the given lanes"""
    m = np.zeros(total, dtype=bool)
    for lane in pieces_of_lanes:
        for a, b, _p0, _p1 in lane or ():
            m[2 * a:2 * b] = True
    return m


# ---- 1: the inputs tell the chain from its wrong forms (no device) -------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_the_inputs_tell_the_chain_from_every_wrong_form_inside_the_pieces(width):
    _instruments, _tracks, subs, total, settings = song_of(width)
    T, L = TILE[width], LANE[width]
    for s in (settings[0], settings[2]):
        assert s.master not in (None, 1.0) and all(g[2] != 1.0 for g in s.groups) and any(g[3] is not None for g in s.groups)
        lanes = [lane for lane in s.tpans + s.gpans if lane]
        assert any(p0 == p1 == 0.0 for lane in lanes for _a, _b, p0, p1 in lane) and any(b - a == 1 for lane in lanes for a, b, _p0, _p1 in lane)
        assert any(2 * a < T + 3 * L < 2 * b for lane in lanes for a, b, _p0, _p1 in lane), "no piece holds the pile-up window's start"
        assert any(a2[0] == a1[1] and a2[2] != a1[3] for lane in lanes for a1, a2 in zip(lane, lane[1:])), "no two adjacent pieces with a jump"
        assert any(2 * a // T != (2 * b - 1) // T for lane in lanes for a, b, _p0, _p1 in lane), "no piece across a tile's edge"
        want = ints(chain((KIND, width), subs, s, width)[2], width)
        plain = ints(chain((KIND, width), subs, s.without_pan_lanes(), width)[2], width)
        track_frames, group_frames = inside(s.tpans, total), inside(s.gpans, total)
        holds = inside([[p for p in lane if p[2] == p[3]] for lane in lanes], total)
        assert np.count_nonzero((want != plain) & (track_frames | group_frames)) > total // 8
        found = {}
        for how in WRONG:
            other = ints(chain((KIND, width), subs, s, width, how)[2], width)
            where = holds if how == STEREO_HOLD else group_frames if how in (GROUP_BEFORE_GAIN, GROUP_BEFORE_RIDE) else track_frames | group_frames
            found[how] = int(np.count_nonzero((want != other) & where))
        print("width %d, setting %s: samples inside the pieces that differ: %s" % (width, s.name, found))
        assert all(n > 0 for n in found.values()), (s.name, found)
    # a hold at 0.0 against the static pan 0.0: every negative odd sample differs, and nothing else
    x = np.arange(-40, 41).repeat(2).tolist()
    held = ints(pan_step(to_bytes(x, width), width, ((0, len(x) // 2, 0.0, 0.0),), None), width)
    static = ints(pan_step(to_bytes(x, width), width, None, 0.0), width)
    assert [int(v) for v in np.array(x)[held != static]] == [v for v in x if v < 0 and v % 2]


# ---- 2: the whole song, chunks and render_into, through the mixer ---------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_the_whole_song_chunks_and_an_odd_offset_are_the_reference_chain_byte_for_byte(gpu, width):
    from synthesizer_amd import mixer
    N = gpu
    instruments, tracks, subs, total, settings = song_of(width)
    samples = as_samples(instruments, width, RATE)
    frames = 333                                                # cuts inside pieces, no multiple of the lane width
    assert (2 * frames) % LANE[width]
    with mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, 2, width) as cs:
        assert cs.ntracks == 3 and cs.frames * 2 == total
        for s in settings:
            want = chain((KIND, width), subs, s, width)[2]
            assert want != chain((KIND, width), subs, s.without_pan_lanes(), width)[2]
            with cs.automation(s.lanes, master=s.mlane, groups=s.glanes, pans=s.tpans, group_pans=s.gpans) as auto:
                assert auto.pan_rides == len(s.gpans) and auto.pan_segments is not None
                kw = dict(gains=s.gains, pans=s.pans, master=s.master, groups=list(s.groups), automation=auto)
                got = bytes(cs.render(**kw).view_frame_data())
                assert got == want, "setting %s: %d bytes differ" % (s.name, differs(got, want))
                parts_ = list(cs.chunks(frames, **kw))
                joined = b"".join(bytes(p.view_frame_data()) for p in parts_)
                assert len(parts_) == -(-cs.frames // frames) > 4 and joined == want and joined == got, s.name
                a, n = (TILE[width] + 3 * LANE[width]) // 2 + 1, 700      # render_into one sample off, of a window that starts mid-piece
                buf = N.DeviceBuffer.from_bytes(b"\x5a" * (n * 2 * width + 2 * width))
                assert cs.render_into(buf, width, a, n, **kw) is None
                back = buf.download_bytes(n * 2 * width + 2 * width)
                assert back[width:-width] == want[a * 2 * width:(a + n) * 2 * width] and back[:width] == back[-width:] == b"\x5a" * width, s.name
                levels = cs.render(meters=True, **kw)[1]
                rows = rows_of((KIND, width), subs, s, width, 0, total)
                assert [(r.peak, r.sum_squares) for r in levels.tracks + [levels.master] + levels.groups] == rows, s.name
        with cs.automation([None] * 3, group_pans=[None, settings[0].gpans[0]]) as auto:
            with pytest.raises(ValueError, match="the automation rides the pan of group 1, and this render names 1 groups"):
                cs.render(automation=auto, groups=[(0, 1, 1.0)])
            with pytest.raises(ValueError, match="the automation rides the pan of group 1, and this render names 0 groups"):
                next(cs.chunks(100, automation=auto))


# ---- 3: windows, through the C entry points -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_every_window_holds_its_slice_and_nothing_beside_it_is_written(gpu, width):
    N = gpu
    instruments, tracks, subs, total, settings = song_of(width)
    T, L = TILE[width], LANE[width]
    w = (T + 3 * L) // 2
    wins = windows(KIND, width, total) + [(2 * (w + 30), 2 * (w + 31)), (2 * (w + 25) + 1, 2 * (w + 50) - 1), (2 * 100, 2 * (T // 2 + 2))]
    assert any(a % 2 for a, _b in wins) and any(b - a == 2 for a, b in wins) and any(a // T != (b - 1) // T and b - a < T for a, b in wins)
    seq, _samples = raw_tracks(N, instruments, tracks, 2, width)
    for s in settings:
        lanes = [lane for lane in s.tpans + s.gpans if lane]
        assert any(2 * a < w0 < 2 * b for lane in lanes for a, b, _p0, _p1 in lane for w0, _w1 in wins), "no window starts inside a piece"
        assert any(2 * a < w1 < 2 * b for lane in lanes for a, b, _p0, _p1 in lane for _w0, w1 in wins), "no window ends inside a piece"
        auto = native_auto(N, seq, s)
        want = chain((KIND, width), subs, s, width)[2]
        for a, b in wins:
            for out_sample in (0, 1):
                got, front, back = render_window(N, WithBuses(seq, s, auto), width, a, b, out_sample)
                assert got == want[a * width:b * width], (s.name, a, b, out_sample, differs(got, want[a * width:b * width]))
                assert front == b"\x5a" * 64 and back == b"\x5a" * 64, (a, b, out_sample)
        auto.free()
    seq.free()


def test_the_windows_at_16_bits_under_the_other_alignment_scheme(gpu):
    in_a_child_under_the_other_alignment_scheme(__file__, ["test_every_window_holds_its_slice_and_nothing_beside_it_is_written[2]"])


# ---- 4: meters ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_the_rows_are_read_behind_the_pan_rides_and_what_is_muted_stays_skipped(gpu, width):
    N = gpu
    instruments, tracks, subs, total, settings = song_of(width)
    T, L = TILE[width], LANE[width]
    wins = [(0, total), (T + 3 * L + 1, 3 * T + L), (2 * T + 5, 3 * T - 7), (T - 1, T + 1)]      # whole, odd, idle, across a tile's edge
    seq, _samples = raw_tracks(N, instruments, tracks, 2, width)
    for s in settings:
        auto = native_auto(N, seq, s)
        want_bytes = chain((KIND, width), subs, s, width)[2]
        whole, plain = rows_of((KIND, width), subs, s, width, 0, total), rows_of((KIND, width), subs, s.without_pan_lanes(), width, 0, total)
        assert all((whole[t] != plain[t]) == bool(s.tpans[t]) for t in range(3)) and whole[3] != plain[3]      # a ridden track's row moves
        for a, b in wins:
            want = rows_of((KIND, width), subs, s, width, a, b)
            assert len(want) == 3 + 1 + len(s.groups)
            for out_sample in (0, 1):
                rows, got, guards = metered(N, seq, s, auto, width, a, b, out_sample)
                assert rows == want, "setting %s, window [%d, %d) at %d:\n%s\n%s" % (s.name, a, b, out_sample, rows, want)
                assert got == want_bytes[a * width:b * width] and guards, (s.name, a, b, out_sample)
            if 2 * T <= a and b <= 3 * T:
                assert rows == [ZERO] * (4 + len(s.groups))     # the idle tile: a pan ride over zeros is zero
        auto.free()
    # a track with static factors (0.0, 0.0) and a group at gain 0.0: skipped and zero, pan lanes or not
    base = settings[2]                                          # groups (0, 1) and (2, 3), pan lanes on every track and both groups
    muted = Setting("muted", base.gains, base.lanes, ((0.0, 0.0), (0.0, 0.0), -0.37), ((0, 1, 0.8, (1.5, 0.25)), (2, 3, 0.0, None)), base.master,
                    base.glanes, base.mlane, base.tpans, base.gpans)
    auto = native_auto(N, seq, muted)
    rows, got, guards = metered(N, seq, muted, auto, width, 0, total, 1)
    assert rows == [ZERO] * 6 and got == bytes(total * width) and guards
    assert rows == rows_of((KIND, width), subs, muted, width, 0, total) and got == chain((KIND, width), subs, muted, width)[2]
    half = Setting("half muted", base.gains, base.lanes, (0.3, (0.0, 0.0), None), ((0, 1, 0.8, (1.5, 0.25)), (2, 3, 0.0, None)), base.master,
                   base.glanes, base.mlane, base.tpans, base.gpans)
    auto2 = native_auto(N, seq, half)
    rows, got, guards = metered(N, seq, half, auto2, width, 0, total)
    want = rows_of((KIND, width), subs, half, width, 0, total)
    assert rows == want and want[1] == want[2] == want[5] == ZERO and want[0] != ZERO and want[4] != ZERO and guards
    assert got == chain((KIND, width), subs, half, width)[2]
    auto.free()
    auto2.free()
    seq.free()


# ---- 5: the search: pan lanes of 513 pieces, on a track and on a group ------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_pan_lanes_of_513_three_frame_pieces_with_one_frame_gaps(gpu, width):
    N = gpu
    T, L = TILE[width], LANE[width]
    rng = np.random.default_rng(7130 + 10 * width)
    frames = 513 * 4 + 41                                       # the pieces end 42 frames before the song does
    instruments = [(pcm(rng, width, frames * 2, 0.9), 2), (pcm(rng, width, 500 * 2, 0.9), 2)]
    tracks = [[_ev(0, 0, 0.8)], [_ev(300, 1, 1.2)]]
    subs = subs_of(instruments, tracks, width, 2)
    total = max(len(s) for s in subs) // width
    assert total == frames * 2 and total > 2 * T and total % L
    pans = [0.0, -0.25, 0.5, 0.37, 1.0, -0.9, 0.1, -1.0]
    many = tuple((4 * i, 4 * i + 3, pans[i % 8], pans[(3 * i + 1) % 8]) for i in range(513))
    other = tuple((4 * i + 1, 4 * i + 4, pans[(i + 3) % 8], pans[(5 * i) % 8]) for i in range(513))
    assert len(many) == 513 and all(many[i + 1][0] - many[i][1] == 1 for i in range(512))
    key = ("search", width)
    s = Setting("513", (1.7, 0.8), (((100, 700, 1.0, 0.2),), None), (0.3, None), ((0, 2, 0.9, (0.999, 0.37)),), 0.9, (((50, 900, 0.3, 1.0),),), None,
                (many, None), (other,))
    want = chain(key, subs, s, width)[2]
    assert differs(want, chain(key, subs, s.without_pan_lanes(), width)[2]) > total // 4
    seq, _samples = raw_tracks(N, instruments, tracks, 2, width)
    auto = native_auto(N, seq, s, ntracks=2)
    for a, b in ((0, total), (T - 3, T + L + 1), (total - T - 5, total), (25, total - 7)):
        for out_sample in (0, 1):
            got, front, back = render_window(N, WithBuses(seq, s, auto), width, a, b, out_sample)
            assert got == want[a * width:b * width], (a, b, out_sample, differs(got, want[a * width:b * width]))
            assert front == back == b"\x5a" * 64
    rows, got, guards = metered(N, seq, s, auto, width, 0, total)
    assert rows == rows_of(key, subs, s, width, 0, total) and got == want and guards
    auto.free()
    seq.free()


# ---- 6: far out --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width, base, which", [(2, "top", 2), (4, "mid", 0)])
def test_pan_pieces_whose_origin_lies_past_2_31_samples(gpu, width, base, which):
    """the near song B samples further out, its pieces B / 2 frames further out: the far window [B + a, B + b) holds the near bytes [a, b),
    because k and n are relative to the piece"""
    N = gpu
    instruments, tracks, subs, total, settings = song_of(width)
    T, L = TILE[width], LANE[width]
    B = {"mid": 2 ** 31 - T, "top": MAX - 4 * T}[base]
    assert B % T == 0 and B % 2 == 0
    (args, kw), _samples = raw_tracks(_Pack, instruments, tracks, 2, width)
    bufs, table, segtab, _w, _nch, packed = args
    assert packed == total
    shifted = table.copy()
    shifted["dst_sample"] += np.uint64(B)
    seq = N.Sequence(bufs, shifted, segtab, width, 2, B + total, track_first=kw["track_first"])
    s = settings[which]

    def far(lane):
        return None if lane is None else tuple((a + B // 2, b + B // 2, v0, v1) for a, b, v0, v1 in lane)
    moved = Setting(s.name, s.gains, tuple(far(x) for x in s.lanes), s.pans, s.groups, s.master, tuple(far(x) for x in s.glanes), far(s.mlane),
                    tuple(far(x) for x in s.tpans), tuple(far(x) for x in s.gpans))
    wins = [(T + 3 * L, 3 * T + L), (T + 3 * L + 71, T + 3 * L + 150), (3 * T + 3 * L, total), (T - 5, T + L + 3)]
    assert any(2 * a > 2 ** 31 and 2 * a < B + w0 < 2 * b for lane in moved.tpans + moved.gpans for a, b, _p0, _p1 in lane or () for w0, _w1 in wins), \
        "no window starts inside a pan piece whose origin lies past 2^31"
    auto = native_auto(N, seq, moved)
    want = chain((KIND, width), subs, s, width)[2]
    for a, b in wins:
        got, front, back = render_window(N, WithBuses(seq, moved, auto), width, B + a, B + b, 1)
        assert got == want[a * width:b * width], "window B + [%d, %d): %d bytes differ" % (a, b, differs(got, want[a * width:b * width]))
        assert front == back == b"\x5a" * 64
    rows = metered(N, seq, moved, auto, width, B + wins[0][0], B + wins[0][1])[0]
    assert rows == rows_of((KIND, width), subs, s, width, *wins[0])
    auto.free()
    seq.free()


# ---- 7: routing, and what the C entry points refuse ---------------------------------------------------------------------------------------------
def test_an_automation_without_pan_pieces_reaches_the_entry_points_it_reached(gpu, monkeypatch):
    from synthesizer_amd import mixer
    N = gpu
    instruments, tracks, subs, total, settings = song_of(2)
    samples = as_samples(instruments, 2, RATE)
    calls, real = [], N.lib()

    class Spy:
        def __getattr__(self, name):
            if name.startswith("sh_seq_auto_create") or name.startswith("sh_seq_render"):
                calls.append(name)
            return getattr(real, name)
    s = settings[0]
    with mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, 2, 2) as cs:
        monkeypatch.setattr(N, "lib", lambda: Spy())
        for kw, create in ((dict(), "sh_seq_auto_create"), (dict(pans=[None] * 3, group_pans=[None, ()]), "sh_seq_auto_create"),
                           (dict(master=s.mlane, pans=[(), None, ()]), "sh_seq_auto_create_buses"),
                           (dict(pans=s.tpans), "sh_seq_auto_create_pans")):
            del calls[:]
            with cs.automation(s.lanes, **kw) as auto:
                cs.render(gains=s.gains, automation=auto)
                cs.render(gains=s.gains, automation=auto, groups=list(s.groups))
            assert calls == [create, "sh_seq_render_auto", "sh_seq_render_groups"], (kw, calls)
        monkeypatch.undo()
        with cs.automation(s.lanes) as before, cs.automation(s.lanes, pans=[None] * 3, group_pans=[()]) as after:
            assert before.seg_first == after.seg_first and before.segments.tobytes() == after.segments.tobytes() and after.pan_segments is None
            assert bytes(cs.render(gains=s.gains, pans=s.pans, automation=after).view_frame_data()) == \
                bytes(cs.render(gains=s.gains, pans=s.pans, automation=before).view_frame_data())


def test_the_entry_points_refuse_on_the_host_and_a_handle_without_pan_segments_renders_as_before(gpu):
    N = gpu
    lib = N.lib()
    from synthesizer_amd import mixer
    instruments, tracks, subs, total, settings = song_of(2)
    seq, _samples = raw_tracks(N, instruments, tracks, 2, 2)
    mono_instruments, mono_tracks, _nch, _subs, _total, _level = the_song("bus", 2)
    mono, _mono_samples = raw_tracks(N, mono_instruments, mono_tracks, 1, 2)

    def table(rows_):
        t = np.zeros(len(rows_), dtype=N.ENV_SEGMENT_DTYPE)
        for k, r in enumerate(rows_):
            t[k] = tuple(r) + (0,) * (8 - len(r))
        return t

    def create(rows_, first, ngroups=0, song=seq, faders=(), seg_first=None):
        t, f = table(rows_), table(faders)
        seg_first = [0] * (3 + 1 + ngroups + 1) if seg_first is None else seg_first
        h = C.c_void_p()
        rc = lib.sh_seq_auto_create_pans(song.handle, f.ctypes.data if len(f) else None, len(f), (C.c_uint32 * len(seg_first))(*seg_first), 3, ngroups,
                                         t.ctypes.data if len(t) else None, len(t), (C.c_uint32 * len(first))(*first), C.byref(h))
        assert not h.value or rc == N.SH_OK
        if h.value:
            lib.sh_seq_auto_destroy(h)
        return rc, lib.sh_last_error()
    good = (100, 0, 1.0, 0.5, 50.0, -0.25, 3)                   # (end, origin, mul, slope, numsamples, offset, kind): frames [0, 50)
    assert create([good], [0, 1, 1, 1])[0] == N.SH_OK                                   # track 0's pan lane, no group lane
    assert create([good], [0, 0, 0, 0] + [0] * 7 + [1], ngroups=8)[0] == N.SH_OK        # the last of eight group pan lanes
    assert create([], [0, 0, 0, 0])[0] == N.SH_OK                                       # no pan segment at all
    nan = float("nan")
    for what, rows_, first, kw, message in (
        ("a song that is not stereo", [good], [0, 1, 1, 1], dict(song=mono), b"a pan needs a stereo song, this one has 1 channels"),
        ("nine group lanes", [good], [0] * 12 + [1], dict(ngroups=9), b"9 group lanes, 0 to 8"),
        ("a fader table that is refused", [good], [0, 1, 1, 1], dict(faders=[(100, 0, 1.0, 0.5, 100.0, 0.25, 3)], seg_first=[0, 1, 1, 1, 1]),
         b"track 0: segment 0: kind 3 not 0 or 1"),
        ("a first that does not end at the table", [good], [0, 0, 0, 0], {}, b"pan_first starts at 0 and ends at npan_segments"),
        ("a first that decreases at a group", [good, good], [0, 0, 0, 2, 1, 2], dict(ngroups=2), b"pan_first decreases at group 1 pan"),
        ("a reserved word", [good + (1,)], [0, 0, 1, 1], {}, b"track 1 pan: segment 0: reserved must be 0"),
        ("an end past the song on a group", [(total + 2, 0, 1.0, 0.5, total / 2 + 1.0, -0.25, 3)], [0, 0, 0, 0, 0, 1], dict(ngroups=2),
         b"group 1 pan: segment 0: ends not ascending or beyond the song"),
        ("half a frame", [(101, 0, 1.0, 0.5, 50.5, -0.25, 3)], [0, 1, 1, 1], {}, b"track 0 pan: segment 0: an odd end"),
        ("a fade-in segment", [(100, 0, 1.0, 0.5, 50.0, 0.0, 1)], [0, 1, 1, 1], {}, b"track 0 pan: segment 0: kind 1 not 0 or 3"),
        ("a mul", [(100, 0, 0.5, 0.5, 50.0, -0.25, 3)], [0, 0, 0, 0, 1], dict(ngroups=1), b"group 0 pan: segment 0: mul must be 1.0"),
        ("an origin that is not the first sample", [(100, 4, 1.0, 0.5, 50.0, -0.25, 3)], [0, 1, 1, 1], {}, b"track 0 pan: segment 0: a move's origin is its first sample"),
        ("numsamples too small", [good, (200, 100, 1.0, 0.5, 49.0, -0.25, 3)], [0, 2, 2, 2], {}, b"track 0 pan: segment 1: numsamples smaller than the move's frames"),
        ("a pan above 1", [(100, 0, 1.0, 1.3, 50.0, -0.25, 3)], [0, 0, 0, 0, 1], dict(ngroups=1), b"group 0 pan: segment 0: a pan is not finite or outside -1 .. 1"),
        ("a pan below -1", [(100, 0, 1.0, 0.0, 50.0, -1.01, 3)], [0, 0, 0, 1], {}, b"track 2 pan: segment 0: a pan is not finite or outside -1 .. 1"),
        ("a pan that is no number", [(100, 0, 1.0, 0.0, 50.0, nan, 3)], [0, 1, 1, 1], {}, b"track 0 pan: segment 0: a pan is not finite or outside -1 .. 1"),
    ):
        rc, err = create(rows_, first, **kw)
        assert rc == N.SH_ERR_INVALID and err.startswith(b"sh_seq_auto_create_pans") and message in err, (what, err)
    # a pan ride on a group that the call does not name: refused, nothing written
    s = settings[2]                                             # pan lanes on groups 0 and 1
    auto = native_auto(N, seq, s)
    out = N.DeviceBuffer.from_bytes(b"\x5a" * 4000)
    one = (N.SeqGroup * 1)(N.SeqGroup(0, 1, 0.8, 1.0, 1.0))
    only_pans = native_auto(N, seq, Setting("pans alone", None, None, None, (), None, (), None, (), (None, s.gpans[1])))
    for handle in (auto, only_pans):
        assert lib.sh_seq_render_auto(seq.handle, 0, 1000, out.handle, 0, None, 0, None, 0, 1.0, None, 0, handle.handle) == N.SH_ERR_INVALID
        assert b"sh_seq_render_auto: the automation rides" in lib.sh_last_error() and b"group 1" in lib.sh_last_error()
        assert lib.sh_seq_render_groups(seq.handle, 0, 1000, out.handle, 0, None, 0, None, 0, 1.0, None, 0, handle.handle, one, 1) == N.SH_ERR_INVALID
        assert b"sh_seq_render_groups: the automation rides" in lib.sh_last_error() and b"group 1, and this call names 1 groups" in lib.sh_last_error()
    assert b"rides the pan of group 1" in lib.sh_last_error()
    assert out.download_bytes(4000) == b"\x5a" * 4000
    auto.free()
    only_pans.free()
    # a handle of sh_seq_auto_create_pans without a pan segment renders what the handles before it render, with and without groups
    for base in (settings[0], settings[3]):
        bare = base.without_pan_lanes()
        lanes = tuple(() if lane is None else lane for lane in bare.lanes)
        glanes = tuple(() if lane is None else lane for lane in bare.glanes)
        segments, first = mixer.CompiledSequence._pack_lanes(lanes, 2, bare.mlane or (), glanes)
        before = N.SeqAutomation(seq, segments, first, len(glanes))
        empty = native_auto(N, seq, bare)
        want = chain((KIND, 2), subs, bare, 2)[2]
        for handle in (before, empty):
            got, front, back = render_window(N, WithBuses(seq, bare, handle), 2, 3, total - 5, 1)
            assert got == want[3 * 2:(total - 5) * 2] and front == back == b"\x5a" * 64
        before.free()
        empty.free()
    seq.free()
    mono.free()
