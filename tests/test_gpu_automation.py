"""GPU parity of fader automation in a compiled song of tracks -- CompiledSequence.automation(lanes) and render(automation=) /
N.Sequence.render(automation=) / sh_seq_auto_create, sh_seq_render_auto -- byte for byte against the chain below, the only definition of
correct, written here with Python ints and floats over the sub-mixes of tests/seqcases.subs_of and live ``audioop``::

    master = silence
    for t: sub = the track folded on its own
           if gains[t] != 1.0: sub = audioop.mul(sub, gains[t])
           for (a, b, v0, v1) in pieces[t]:                          # song frames
               n = float((b - a) * nch)
               for k in range((b - a) * nch):                        # k counts SAMPLES from the piece's first, interleaved
                   sub[a * nch + k] = int(sub[a * nch + k] * (k * (v1 - v0) / n + v0))
           if pans[t] is not None: sub = Sample.stereo(lf, rf) of a stereo sample (tests/seqref.balance)
           master = audioop.add(master, sub)
    if master_gain != 1.0: master = audioop.mul(master, master_gain)

Expected bytes never come from the product.  Rate 8192 and the three-track, four-tile songs of the neighbouring files (at most 8192
samples), one mono ("bus") and one stereo ("balance"); the search has a song of its own, long enough for 513 pieces.  Of the wrong forms,
"k counts frames" and "the fade behind the pan" exist in a stereo song alone (a mono song's frames are its samples, and it has no pan)."""
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
PANS = [(0.3, None, (1.5, 0.25)), (None, (0.999, 0.37), -0.37), (-1.0, 1.0, 0.0), ((1.0, 1.0), (0.0, 0.0), (-0.5, 1.0))]      # the desk file's
MASTERS = [None, 0.7, -1.3]
RIGHT, FADE_FIRST, FLOORED, MUL_HOLD, K_FRAMES, K_WINDOW, BEHIND_PAN = "right", "the fade in front of the gain", "floor instead of truncation", \
    "audioop.mul for a hold", "k counts frames", "k counted from the window's start", "the fade behind the pan"
WRONG = (FADE_FIRST, FLOORED, MUL_HOLD, K_FRAMES, K_WINDOW, BEHIND_PAN)
STEREO_ONLY = (K_FRAMES, BEHIND_PAN)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def to_bytes(v, width):
    return np.asarray(v, dtype=np.int64).astype({1: np.int8, 2: "<i2", 4: "<i4"}[width]).tobytes()


def ride(data, width, nch, pieces, how=RIGHT, window=0):
    """the fader moves of one track on its bytes (of the song's length): Python ints and floats, sample by sample"""
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


def flat(pans):
    """pans as the C entry point takes them: left then right per track, (1.0, 1.0) where there is none"""
    if pans is None:
        return None
    return [f for p in pans for f in ((1.0, 1.0) if p is None else factors(tuple(p) if isinstance(p, (tuple, list)) else p))]


_CHAIN = {}


def chain(key, subs, gains, lanes, pans, master_gain, width, nch, how=RIGHT, window=0):
    """(the tracks as the master takes them, as bytes of the song's length; the master's bytes), made once per key and setting"""
    at = (key, gains, lanes, pans, master_gain, how, window)
    if at in _CHAIN:
        return _CHAIN[at]
    total = max([len(s) for s in subs] + [0])
    out, posts = bytes(total), []
    for t, sub in enumerate(subs):
        sub = sub + bytes(total - len(sub))
        g = 1.0 if gains is None else gains[t]
        pieces = () if lanes is None or lanes[t] is None else lanes[t]
        pan = None if pans is None or pans[t] is None else factors(tuple(pans[t]) if isinstance(pans[t], (tuple, list)) else pans[t])
        if how == FADE_FIRST:
            sub = ride(sub, width, nch, pieces)
        if g != 1.0:
            sub = audioop.mul(sub, width, g)
        if how not in (FADE_FIRST, BEHIND_PAN):
            sub = ride(sub, width, nch, pieces, how, window)
        if pan is not None:
            sub = balance(sub, width, *pan)
        if how == BEHIND_PAN:
            sub = ride(sub, width, nch, pieces)
        posts.append(sub)
        out = audioop.add(out, sub, width)
    if master_gain is not None and master_gain != 1.0:
        out = audioop.mul(out, width, master_gain)
    _CHAIN[at] = (posts, out)
    return _CHAIN[at]


def rows_of(key, subs, gains, lanes, pans, master_gain, width, nch, a, b):
    posts, out = chain(key, subs, gains, lanes, pans, master_gain, width, nch)
    return [row_of(ints(p, width)[a:b], a, nch) for p in posts] + [row_of(ints(out, width)[a:b], a, nch)]


# ---- the pieces, in song frames, chosen for where a lane can go wrong -------------------------------------------------------------------
def lane_sets(width, nch, total):
    """{name: one lane per track}; sample positions below are even, so they are whole frames of a stereo song as well"""
    T, L = TILE[width], LANE[width]
    w = T + 3 * L                                               # the pile-up window's first sample

    def fr(*pieces):
        assert all(a % nch == 0 and b % nch == 0 for a, b, _v0, _v1 in pieces)
        return tuple((a // nch, b // nch, v0, v1) for a, b, v0, v1 in pieces)
    edges = fr((L + 2, 5 * L + 2, 0.2, 0.9), (5 * L + 2, 9 * L - 2, 0.9, 0.1),        # starts and ends mid-lane; two pieces meet mid-lane
               (10 * L, 14 * L, 1.0, 0.3),                                           # on lane boundaries (a fade-out)
               (15 * L + 2, 15 * L + 2 + nch, 0.25, 0.75),                           # one frame
               (16 * L + 2, 18 * L, 0.5, 0.5), (18 * L + nch, 20 * L + 2, 0.37, 0.37),      # one frame apart; holds
               (T, 2 * T, 0.3, 1.0),                                                 # on tile boundaries (a fade-in)
               (3 * T + 2 * L + 2, total, 0.8, 0.0))                                 # to the song's last frame
    holds = fr((w - 80, w - 40, 0.0, 0.6), (w - 40, w, 1.0, 1.0), (w, w + 30, 0.6, 0.2), (w + 30, w + 60, 0.0, 0.0), (w + 60, w + 200, 0.0, 0.37),
               (w + 200, w + 260, 0.37, 0.37), (w + 260, w + 300, 1.0, 1.0), (w + 300, w + 340, 1.0, 0.5))
    across = fr((T - 2 * L - 2, 3 * T + 3 * L + 2, 0.1, 1.0))                         # across three tiles
    whole = fr((0, total, 0.9, 0.15))
    return {"edges": (edges, whole, edges), "across": (across, holds, holds), "one": (None, across, None)}


SETS = ["edges", "across"]


def song_of(kind, width):
    instruments, tracks, nch, subs, total, level = the_song(kind, width)
    assert total % nch == 0
    return instruments, tracks, nch, subs, total, lane_sets(width, nch, total)


class WithAuto:
    """N.Sequence behind render_window, which calls render(first, n, out, out_sample): through sh_seq_render_auto"""

    def __init__(self, seq, gains, pans, master_gain, auto):
        self.seq, self.gains, self.pans, self.master, self.auto = seq, gains, flat(pans), master_gain, auto

    def render(self, a, n, out, out_sample):
        self.seq.render(a, n, out, out_sample, gains=self.gains, pans=self.pans, master=self.master, automation=self.auto)


def native_auto(N, seq, lanes, nch):
    """the lanes through sh_seq_auto_create: the product's packer makes the table (an input)"""
    from synthesizer_amd import mixer
    segments, first = mixer.CompiledSequence._pack_lanes(tuple(() if lane is None else lane for lane in lanes), nch)
    return N.SeqAutomation(seq, segments, first)


def metered(N, seq, width, a, b, gains, pans, master_gain, auto, out_sample=0):
    """(rows, the rendered bytes, the guards intact) of a metered render with automation into a 0x5A-filled buffer"""
    n = b - a
    inner = (out_sample + n) * width
    parent = N.DeviceBuffer.from_bytes(b"\x5a" * (64 + inner + 64))
    rows = seq.render(a, n, parent.view(64, inner), out_sample, gains=gains, meters=True, pans=flat(pans), master=master_gain, automation=auto)
    got = parent.download_bytes(64 + inner + 64)
    at = 64 + out_sample * width
    return rows, got[at:at + n * width], got[:at] == b"\x5a" * at and got[at + n * width:] == b"\x5a" * 64


# ---- 1: the inputs tell the chain from its wrong forms -------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_inputs_tell_the_chain_from_every_wrong_form(kind, width):
    _instruments, _tracks, nch, subs, total, sets = song_of(kind, width)
    T, L = TILE[width], LANE[width]
    lo, hi = T + 3 * L, 3 * T + L                               # the pile-up window: it starts inside the pieces that start on T and before it
    top = 2 ** (8 * width - 1)
    pans = PANS[0] if nch == 2 else None
    for name in SETS:
        lanes = sets[name]
        assert any(a * nch < lo < b * nch for lane in lanes for a, b, _v0, _v1 in lane or ())
        for gains in (GAINS[0], GAINS[3]):
            key = (kind, width)
            want = chain(key, subs, gains, lanes, pans, 0.7, width, nch)[1]
            assert want != chain(key, subs, gains, None, pans, 0.7, width, nch)[1]
            found = {}
            for how in WRONG:
                if nch == 1 and how in STEREO_ONLY:
                    continue
                other = chain(key, subs, gains, lanes, pans, 0.7, width, nch, how, lo)[1]
                found[how] = differs(want[lo * width:hi * width], other[lo * width:hi * width]) if how == K_WINDOW else differs(want, other)
            print("%s, width %d, set %s, gains %s: bytes that differ: %s" % (kind, width, name, gains, found))
            assert all(n > 0 for n in found.values()), found
    # a gain above 1 and a negative one saturate a track in front of its moves, inside a piece
    for gains in (GAINS[0], GAINS[3]):
        hit = False
        for t, sub in enumerate(subs):
            scaled = ints(audioop.mul(sub, width, gains[t]), width)
            for a, b, _v0, _v1 in sets["edges"][t]:
                part = scaled[a * nch:b * nch]
                hit = hit or (len(part) and (part.max() == top - 1 or part.min() == -top))
        assert hit, "no track saturates behind its gain inside a piece"


# ---- 2: the whole song, through the mixer ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_whole_song_is_the_reference_chain_byte_for_byte(gpu, kind, width):
    from synthesizer_amd import mixer
    instruments, tracks, nch, subs, total, sets = song_of(kind, width)
    samples = as_samples(instruments, width, RATE)
    with mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, nch, width) as cs:
        assert cs.ntracks == 3 and cs.frames * nch == total
        for name in SETS + ["one"]:
            lanes = sets[name]
            with cs.automation(lanes) as auto:
                assert all(p[2:] != (1.0, 1.0) for lane in auto.pieces for p in lane)
                for gains in (None, GAINS[0], GAINS[3]):
                    for pans in (PANS if nch == 2 else [None]):
                        for master_gain in MASTERS:
                            want = chain((kind, width), subs, gains, lanes, pans, master_gain, width, nch)[1]
                            got = bytes(cs.render(gains=gains, pans=pans, master=master_gain, automation=auto).view_frame_data())
                            assert got == want, "set %s, gains %s, pans %s, master %s: %d bytes differ" % (name, gains, pans, master_gain, differs(got, want))


# ---- 3: windows, through the C entry point ----------------------------------------------------------------------------------------------
SETTINGS = [(GAINS[0], 0, 0.7, "edges"), (GAINS[3], 1, -1.3, "across"), (None, 3, None, "edges")]      # (gains, which of PANS, master, lanes)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_window_holds_its_slice_and_nothing_beside_it_is_written(gpu, kind, width):
    N = gpu
    instruments, tracks, nch, subs, total, sets = song_of(kind, width)
    wins = windows("balance", width, total)
    assert any(a % 2 for a, _b in wins), "no window starts on an odd sample"
    seq, _samples = raw_tracks(N, instruments, tracks, nch, width)
    for gains, which, master_gain, name in SETTINGS:
        pans = PANS[which] if nch == 2 else None
        lanes = sets[name]
        assert any(a * nch < w0 < b * nch for lane in lanes for a, b, _v0, _v1 in lane or () for w0, _w1 in wins), "no window starts inside a piece"
        auto = native_auto(N, seq, lanes, nch)
        want = chain((kind, width), subs, gains, lanes, pans, master_gain, width, nch)[1]
        for a, b in wins:
            for out_sample in (0, 1):
                got, front, back = render_window(N, WithAuto(seq, gains, pans, master_gain, auto), width, a, b, out_sample)
                assert got == want[a * width:b * width], (gains, pans, master_gain, name, a, b, out_sample, differs(got, want[a * width:b * width]))
                assert front == b"\x5a" * 64 and back == b"\x5a" * 64, (a, b, out_sample)
        auto.free()
    seq.free()


def test_the_windows_at_16_bits_under_the_other_alignment_scheme(gpu):
    in_a_child_under_the_other_alignment_scheme(
        __file__, ["test_every_window_holds_its_slice_and_nothing_beside_it_is_written[%s-2]" % kind for kind in KINDS])


# ---- 4: meters ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_rows_read_a_track_behind_its_moves(gpu, kind, width):
    N = gpu
    instruments, tracks, nch, subs, total, sets = song_of(kind, width)
    T, L = TILE[width], LANE[width]
    wins = [(0, total), (T + 3 * L + 1, 3 * T + L), (2 * T + 5, 3 * T - 7), (T - 1, T + 1)]      # whole, odd, idle, across a tile's edge
    seq, _samples = raw_tracks(N, instruments, tracks, nch, width)
    for gains, which, master_gain, name in SETTINGS:
        pans = PANS[which] if nch == 2 else None
        lanes = sets[name]
        auto = native_auto(N, seq, lanes, nch)
        want_bytes = chain((kind, width), subs, gains, lanes, pans, master_gain, width, nch)[1]
        plain_rows = rows_of((kind, width), subs, gains, None, pans, master_gain, width, nch, 0, total)
        assert rows_of((kind, width), subs, gains, lanes, pans, master_gain, width, nch, 0, total) != plain_rows
        for a, b in wins:
            want = rows_of((kind, width), subs, gains, lanes, pans, master_gain, width, nch, a, b)
            for out_sample in (0, 1):
                rows, got, guards = metered(N, seq, width, a, b, gains, pans, master_gain, auto, out_sample)
                assert rows == want, "set %s, gains %s, pans %s, master %s, window [%d, %d) at %d:\n%s\n%s" % (name, gains, pans, master_gain, a, b,
                                                                                                                    out_sample, rows, want)
                assert got == want_bytes[a * width:b * width] and guards, (name, gains, pans, master_gain, a, b, out_sample)
        auto.free()
    # a muted track is still skipped: its row reads zero whatever its lane says
    auto = native_auto(N, seq, sets["edges"], nch)
    rows = metered(N, seq, width, 0, total, [0.0, 1.0, 1.0], None, None, auto)[0]
    assert rows[0] == ((0, 0), (0, 0)) and rows[1][0][0] > 0
    auto.free()
    seq.free()


# ---- 5: equalities -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_moves_that_do_nothing_change_no_byte_and_chunks_are_the_whole(gpu, kind, width):
    from synthesizer_amd import mixer
    instruments, tracks, nch, subs, total, sets = song_of(kind, width)
    samples = as_samples(instruments, width, RATE)
    gains, pans, master_gain = GAINS[3], (PANS[0] if nch == 2 else None), 0.7
    with mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, nch, width) as cs:
        plain = bytes(cs.render(gains=gains, pans=pans, master=master_gain).view_frame_data())
        assert plain == chain((kind, width), subs, gains, None, pans, master_gain, width, nch)[1]
        assert bytes(cs.render(gains=gains, pans=pans, master=master_gain, automation=None).view_frame_data()) == plain
        unity = [[(0, 10, 1.0, 1.0), (10, cs.frames, 1.0, 1.0)], None, [(5, 6, 1.0, 1.0)]]
        for lanes in ([None] * 3, unity):
            with cs.automation(lanes) as auto:
                assert auto.pieces == ((), (), ()) and len(auto.segments) == 0
                assert bytes(cs.render(gains=gains, pans=pans, master=master_gain, automation=auto).view_frame_data()) == plain
                assert bytes(cs.render(automation=auto).view_frame_data()) == bytes(cs.render().view_frame_data())
        # chunks of a length that cuts pieces and is no multiple of the lane width
        frames = 333
        assert (nch * frames) % LANE[width]
        for name in SETS:
            lanes = sets[name]
            assert any(a < c < b for lane in lanes for a, b, _v0, _v1 in lane or () for c in range(frames, cs.frames, frames))
            want = chain((kind, width), subs, gains, lanes, pans, master_gain, width, nch)[1]
            with cs.automation(lanes) as auto:
                parts = list(cs.chunks(frames, gains=gains, pans=pans, master=master_gain, automation=auto))
                assert len(parts) == -(-cs.frames // frames) > 4
                assert b"".join(bytes(p.view_frame_data()) for p in parts) == want
                pairs = list(cs.chunks(frames, gains=gains, pans=pans, master=master_gain, automation=auto, meters=True))
                assert [bytes(s.view_frame_data()) for s, _l in pairs] == [bytes(p.view_frame_data()) for p in parts]
                third = rows_of((kind, width), subs, gains, lanes, pans, master_gain, width, nch, 2 * nch * frames, 3 * nch * frames)
                if nch == 1:                                    # (a mono song's Levels read left == right, as Sample does)
                    third = [((p[0], p[0]), (q[0], q[0])) for p, q in third]
                assert [(r.peak, r.sum_squares) for r in pairs[2][1].tracks + [pairs[2][1].master]] == third
                # stem stays plain
                assert bytes(cs.stem(0).view_frame_data()) == subs[0] + bytes(len(want) - len(subs[0]))


# ---- 6: the search: a track of 513 pieces -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("width", WIDTHS)
def test_a_track_of_513_three_frame_pieces_with_one_frame_gaps(gpu, width, nch):
    N = gpu
    T, L = TILE[width], LANE[width]
    rng = np.random.default_rng(5130 + 10 * width + nch)
    frames = 513 * 4 + 41                                       # the pieces end 42 frames before the song does
    instruments = [(pcm(rng, width, frames * nch, 0.9), nch), (pcm(rng, width, 500 * nch, 0.9), nch)]
    tracks = [[_ev(0, 0, 0.8)], [_ev(300, 1, 1.2)]]
    subs = subs_of(instruments, tracks, width, nch)
    total = max(len(s) for s in subs) // width
    assert total == frames * nch and total > T and total % L
    vols = [0.0, 0.25, 0.5, 0.37, 1.0, 0.9, 0.1]
    many = tuple((4 * i, 4 * i + 3, vols[i % 7], vols[(3 * i + 1) % 7]) for i in range(513))
    lanes = (many, ((100, 700, 1.0, 0.2),))
    assert len(many) == 513 and all(many[i + 1][0] - many[i][1] == 1 for i in range(512))
    key = ("search", width, nch)
    gains, master_gain = (1.7, 0.8), 0.9
    want = chain(key, subs, gains, lanes, None, master_gain, width, nch)[1]
    assert differs(want, chain(key, subs, gains, None, None, master_gain, width, nch)[1]) > total // 4
    seq, _samples = raw_tracks(N, instruments, tracks, nch, width)
    auto = native_auto(N, seq, lanes, nch)
    for a, b in ((0, total), (T - 3, T + L + 1), (total - T - 5, total), (3 * nch * 4 + 1, total - 7)):
        for out_sample in (0, 1):
            got, front, back = render_window(N, WithAuto(seq, list(gains), None, master_gain, auto), width, a, b, out_sample)
            assert got == want[a * width:b * width], (a, b, out_sample, differs(got, want[a * width:b * width]))
            assert front == back == b"\x5a" * 64
    rows, got, guards = metered(N, seq, width, 0, total, list(gains), None, master_gain, auto)
    assert rows == rows_of(key, subs, gains, lanes, None, master_gain, width, nch, 0, total) and got == want and guards
    auto.free()
    seq.free()


# ---- 7: refusals ---------------------------------------------------------------------------------------------------------------------------
def test_width_3_has_no_automation(gpu):
    from synthesizer_amd import mixer
    N = gpu
    instruments, tracks, nch, _subs, total, _level = the_song("bus", 3)
    samples = as_samples(instruments, 3, RATE)
    with mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, nch, 3) as cs:
        with pytest.raises(NotImplementedError, match="width 3"):
            cs.automation([None, [(0, 10, 0.5, 1.0)], None])
        with pytest.raises(NotImplementedError, match="width 3"):
            cs.automation([None] * 3)
        h = C.c_void_p()
        first = (C.c_uint32 * 4)(0, 0, 0, 0)
        assert N.lib().sh_seq_auto_create(cs._seq.handle, None, 0, first, 3, C.byref(h)) == N.SH_ERR_INVALID and not h.value
        assert b"width 3" in N.lib().sh_last_error()


def test_the_entry_points_refuse_on_the_host_and_write_nothing(gpu):
    N = gpu
    lib = N.lib()
    from synthesizer_amd import mixer
    from synthesizer_amd.sample import Sample
    instruments, tracks, nch, subs, total, sets = song_of("balance", 2)
    seq, samples = raw_tracks(N, instruments, tracks, 2, 2)
    auto = native_auto(N, seq, sets["edges"], 2)
    bufs, table, segtab, nbytes = Sample(samplerate=RATE, nchannels=2, samplewidth=2)._compile_events(with_samples(samples, [e for t in tracks for e in t]))
    flat_song = N.Sequence(bufs, table, segtab, 2, 2, nbytes // 2)
    others = []
    for kind, width, cut in (("bus", 2, 0), ("balance", 4, 0), ("balance", 2, 1)):      # other channels, other width, other length ...
        o_instruments, o_tracks, o_nch, _s, o_total, o_sets = song_of(kind, width)
        o_tracks = [t[:len(t) - cut] if k == 0 else t for k, t in enumerate(o_tracks)]     # (the last note of track 0 ends the song)
        o_seq, o_samples = raw_tracks(N, o_instruments, o_tracks, o_nch, width)
        assert cut == 0 or o_seq.info()["track_samples"] < total
        others.append((o_seq, native_auto(N, o_seq, [None] * 3, o_nch), o_samples))
    two_seq, two_samples = raw_tracks(N, instruments, tracks[:2], 2, 2)                 # ... and another track count
    others.append((two_seq, native_auto(N, two_seq, [None] * 2, 2), two_samples))
    out = N.DeviceBuffer.from_bytes(b"\x5a" * 4000)
    rows = (N.SeqMeter * 5)()
    C.memset(rows, 0xAB, C.sizeof(rows))
    untouched = bytes(rows)
    dbl = lambda *v: (C.c_double * len(v))(*v)                 # noqa: E731
    nan = float("nan")
    ones, six = dbl(1.0, 1.0, 1.0), dbl(0.5, 0.5, 1.0, 1.0, 0.0, 1.0)
    cases = [
        ("no automation", (seq.handle, 0, 100, out.handle, 0, ones, 3, six, 6, 1.0, None, 0, None), b"NULL argument"),
        ("a flat song", (flat_song.handle, 0, 100, out.handle, 0, None, 0, None, 0, 0.5, None, 0, auto.handle), b"the song has no tracks"),
        ("too few gains", (seq.handle, 0, 100, out.handle, 0, dbl(1.0, 1.0), 2, six, 6, 1.0, None, 0, auto.handle), b"2 gains for 3 tracks"),
        ("a pan factor too few", (seq.handle, 0, 100, out.handle, 0, ones, 3, six, 5, 1.0, None, 0, auto.handle), b"5 pan factors for 3 tracks"),
        ("a row too few", (seq.handle, 0, 100, out.handle, 0, ones, 3, six, 6, 1.0, rows, 3, auto.handle), b"3 rows for 3 tracks and the master"),
        ("a pan that is no number", (seq.handle, 0, 100, out.handle, 0, ones, 3, dbl(0.5, 0.5, 1.0, nan, 0.0, 1.0), 6, 1.0, rows, 4, auto.handle),
         b"pan 1: right factor is not finite"),
        ("a master that is no number", (seq.handle, 0, 100, out.handle, 0, ones, 3, six, 6, nan, rows, 4, auto.handle), b"master gain is not finite"),
        ("a gain that is no number", (seq.handle, 0, 100, out.handle, 0, dbl(1.0, nan, 1.0), 3, six, 6, 1.0, rows, 4, auto.handle), b"gain 1 is not finite"),
        ("NULL rows that are counted", (seq.handle, 0, 100, out.handle, 0, ones, 3, six, 6, 1.0, None, 4, auto.handle), b"NULL argument"),
        ("a NULL song", (None, 0, 100, out.handle, 0, ones, 3, six, 6, 1.0, None, 0, auto.handle), b"NULL argument"),
        ("a NULL out", (seq.handle, 0, 100, None, 0, ones, 3, six, 6, 1.0, None, 0, auto.handle), b"NULL argument"),
        ("a range past the song", (seq.handle, total - 10, 11, out.handle, 0, ones, 3, six, 6, 0.5, rows, 4, auto.handle), b"range outside the song"),
        ("a range past out", (seq.handle, 0, 2000, out.handle, 1, ones, 3, six, 6, 0.5, None, 0, auto.handle), b"range outside out"),
    ]
    for o_seq, o_auto, _keep in others:
        cases.append(("an automation of another song", (seq.handle, 0, 100, out.handle, 0, ones, 3, None, 0, 1.0, rows, 4, o_auto.handle),
                      b"the automation was made for another song"))
    for what, args, message in cases:
        assert lib.sh_seq_render_auto(*args) == N.SH_ERR_INVALID, what
        err = lib.sh_last_error()
        assert err.startswith(b"sh_seq_render_auto") and message in err, (what, err)
        assert bytes(rows) == untouched, what
    assert out.download_bytes(4000) == b"\x5a" * 4000
    # what sh_seq_auto_create refuses: rows are (end, origin, mul, slope, numsamples, offset, kind, reserved)
    def create(rows_, first, ntracks=3, song=seq):
        t = np.zeros(len(rows_), dtype=N.ENV_SEGMENT_DTYPE)
        for k, r in enumerate(rows_):
            t[k] = tuple(r) + (0,) * (8 - len(r))
        h = C.c_void_p()
        rc = lib.sh_seq_auto_create(song.handle, t.ctypes.data if len(t) else None, len(t), (C.c_uint32 * len(first))(*first), ntracks, C.byref(h))
        assert not h.value or rc == N.SH_OK
        if h.value:
            lib.sh_seq_auto_destroy(h)
        return rc, lib.sh_last_error()
    good = (100, 0, 1.0, 0.5, 100.0, 0.25, 1)
    assert create([good], [0, 1, 1, 1])[0] == N.SH_OK
    for what, rows_, first, kw, message in (
        ("a flat song", [good], [0, 1, 1, 1], dict(song=flat_song), b"the song has no tracks"),
        ("another track count", [good], [0, 1, 1], dict(ntracks=2), b"2 lanes for 3 tracks"),
        ("a first that does not end at the table", [good], [0, 0, 0, 0], {}, b"seg_first starts at 0 and ends at nsegments"),
        ("a first that decreases", [good, good], [0, 2, 1, 2], {}, b"seg_first decreases at track 2"),
        ("a reserved word", [good + (1,)], [0, 1, 1, 1], {}, b"track 0: segment 0: reserved must be 0"),
        ("an end past the song", [(total + 2, 0, 1.0, 0.5, total + 2.0, 0.25, 1)], [0, 0, 1, 1], {}, b"track 1: segment 0: ends not ascending or beyond the song"),
        ("ends that do not ascend", [good, (100, 100, 1.0, 0.0, 0.0, 0.0, 0)], [0, 2, 2, 2], {}, b"track 0: segment 1: ends not ascending"),
        ("a fade-out segment", [(100, 0, 1.0, 0.5, 100.0, 0.0, 2)], [0, 1, 1, 1], {}, b"kind 2 not 0 or 1"),
        ("a mul", [(100, 0, 0.5, 0.5, 100.0, 0.25, 1)], [0, 1, 1, 1], {}, b"mul must be 1.0"),
        ("an origin that is not the first sample", [(100, 4, 1.0, 0.5, 100.0, 0.25, 1)], [0, 1, 1, 1], {}, b"a move's origin is its first sample"),
        ("numsamples too small", [(100, 0, 1.0, 0.5, 99.0, 0.25, 1)], [0, 1, 1, 1], {}, b"numsamples shorter than the move"),
        ("a volume above 1", [(100, 0, 1.0, 0.8, 100.0, 0.25, 1)], [0, 1, 1, 1], {}, b"a volume is not finite or outside 0 .. 1"),
        ("a volume below 0", [(100, 0, 1.0, -0.5, 100.0, 0.25, 1)], [0, 1, 1, 1], {}, b"a volume is not finite or outside 0 .. 1"),
        ("a volume that is no number", [(100, 0, 1.0, 0.0, 100.0, nan, 1)], [0, 1, 1, 1], {}, b"a volume is not finite or outside 0 .. 1"),
    ):
        rc, err = create(rows_, first, **kw)
        assert rc == N.SH_ERR_INVALID and err.startswith(b"sh_seq_auto_create") and message in err, (what, err)
    # and what sh_seq_render_auto takes: NULL gains and NULL pans, a master of 1.0, unmetered -- the moves alone
    assert lib.sh_seq_render_auto(seq.handle, 0, 1000, out.handle, 0, None, 0, None, 0, 1.0, None, 0, auto.handle) == N.SH_OK
    want = chain(("balance", 2), subs, None, sets["edges"], None, None, 2, 2)[1]
    assert out.download_bytes(2000) == want[:2000] and out.download_bytes(2000, 2000) == b"\x5a" * 2000 and bytes(rows) == untouched
    # the mixer refuses an Automation of another song before anything is launched
    with mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, 2, 2) as one, \
            mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, 2, 2) as two:
        with one.automation([None] * 3) as theirs:
            for bad in (theirs, "x", 0.5):
                with pytest.raises(ValueError, match="automation is None or an Automation made by this song"):
                    two.render(automation=bad)
    auto.free()
    for o_seq, o_auto, _keep in others:
        o_auto.free()
        o_seq.free()
    seq.free()
    flat_song.free()


# ---- 8: far out --------------------------------------------------------------------------------------------------------------------------
MAX = 2 ** 32 - 65536                                       # shq::MAX_TRACK_SAMPLES


class _Pack:
    """stands where the native module stands in raw_tracks and keeps what it would hand N.Sequence (tests/test_gpu_sequence_far.py's way)"""

    @staticmethod
    def Sequence(*args, **kw):
        return args, kw


@pytest.mark.parametrize("kind, width, base", [("bus", 2, "top"), ("balance", 4, "top"), ("balance", 2, "mid"), ("bus", 1, "mid")])
def test_a_piece_whose_origin_lies_past_2_31_samples(gpu, kind, width, base):
    """the near song B samples further out, its pieces B / nch frames further out: the far window [B + a, B + b) holds the near bytes [a, b)"""
    N = gpu
    instruments, tracks, nch, subs, total, sets = song_of(kind, width)
    T, L = TILE[width], LANE[width]
    B = {"mid": 2 ** 31 - T, "top": MAX - 4 * T}[base]
    assert B % T == 0 and B % 2 == 0
    (args, kw), _samples = raw_tracks(_Pack, instruments, tracks, nch, width)
    bufs, table, segtab, _w, _nch, packed = args
    assert packed == total
    shifted = table.copy()
    shifted["dst_sample"] += np.uint64(B)
    seq = N.Sequence(bufs, shifted, segtab, width, nch, B + total, track_first=kw["track_first"])
    gains, pans, master_gain = GAINS[3], (PANS[0] if nch == 2 else None), 0.7
    wins = [(T + 3 * L, 3 * T + L), (T + 3 * L + 71, T + 3 * L + 150), (3 * T + 3 * L, total), (T - 5, T + L + 3)]
    for name in SETS:
        lanes = sets[name]
        far = tuple(tuple((a + B // nch, b + B // nch, v0, v1) for a, b, v0, v1 in lane) for lane in lanes)
        assert any(a * nch > 2 ** 31 and a * nch < B + w0 < b * nch for lane in far for a, b, _v0, _v1 in lane for w0, _w1 in wins), \
            "no window starts inside a piece whose origin lies past 2^31"
        auto = native_auto(N, seq, far, nch)
        want = chain((kind, width), subs, gains, lanes, pans, master_gain, width, nch)[1]
        for a, b in wins:
            got, front, back = render_window(N, WithAuto(seq, list(gains), pans, master_gain, auto), width, B + a, B + b, 1)
            assert got == want[a * width:b * width], "set %s, window B + [%d, %d): %d bytes differ" % (name, a, b, differs(got, want[a * width:b * width]))
            assert front == back == b"\x5a" * 64
        rows = metered(N, seq, width, B + wins[0][0], B + wins[0][1], list(gains), pans, master_gain, auto)[0]
        assert rows == rows_of((kind, width), subs, gains, lanes, pans, master_gain, width, nch, *wins[0])
        auto.free()
    seq.free()
