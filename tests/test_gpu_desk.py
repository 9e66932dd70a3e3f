"""GPU parity of the desk of a stereo song of tracks -- a pan pot per track and a master fader at render time:
CompiledSequence.render(gains=, pans=, master=) / N.Sequence.render(pans=, master=) / sh_seq_render_desk -- byte for byte against live
``audioop``.  The reference chain is ``desk`` below, the only definition of correct::

    master = silence
    for t: sub = the track folded on its own (tests/seqcases.subs_of)
           if gains[t] != 1.0: sub = audioop.mul(sub, gains[t])
           if pans[t] is not None: sub = Sample.stereo(lf, rf) of a stereo sample (tests/seqref.balance)
           master = audioop.add(master, sub)
    if master_gain != 1.0: master = audioop.mul(master, master_gain)

Expected bytes never come from the product.  Rate 8192 and the four-tile songs of the neighbouring files (at most 8192 samples)."""
import audioop
import ctypes as C

import numpy as np
import pytest

from tests.seqcases import (GAINS, RATE, _ev, as_samples, in_a_child_under_the_other_alignment_scheme, ints, raw_tracks, render_window, row_of,
                            subs_of, the_song, windows, with_samples)
from tests.seqref import LANE, TILE, balance, differs, factors, pcm

pytestmark = pytest.mark.gpu

ZERO = ((0, 0), (0, 0))
KINDS = ["pan", "balance"]
WIDTHS = [1, 2, 3, 4]
PANS = [(0.3, None, (1.5, 0.25)), (None, (0.999, 0.37), -0.37), (-1.0, 1.0, 0.0), ((1.0, 1.0), (0.0, 0.0), (-0.5, 1.0))]
MASTERS = [None, 0.7, -1.3]
RIGHT, PAN_FIRST, ONE_PRODUCT, SWAPPED, MASTER_PER_TRACK, TRUNCATED = "right", "pan first", "one product", "left and right swapped", \
    "master per track", "truncation instead of floor"
WRONG = (PAN_FIRST, ONE_PRODUCT, SWAPPED, MASTER_PER_TRACK, TRUNCATED)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def to_bytes(v, width):
    v = np.asarray(v, dtype=np.int64)
    if width == 3:
        return v.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    return v.astype({1: np.int8, 2: "<i2", 4: "<i4"}[width]).tobytes()


def mul(data, width, factor, how=RIGHT):
    """audioop.mul, none at exactly 1.0; TRUNCATED: the wrong rounding, toward zero"""
    if factor == 1.0:
        return data
    if how != TRUNCATED:
        return audioop.mul(data, width, factor)
    top = 2 ** (8 * width - 1)
    return to_bytes(np.clip(np.trunc(ints(data, width).astype(np.float64) * factor), -top, top - 1).astype(np.int64), width)


def stereo(data, width, lf, rf, how=RIGHT):
    """Sample.stereo(lf, rf) of a stereo sample"""
    if how != TRUNCATED:
        return balance(data, width, lf, rf)
    v = ints(data, width)
    out = v.copy()
    out[0::2] = ints(mul(to_bytes(v[0::2], width), width, lf, how), width)
    out[1::2] = ints(mul(to_bytes(v[1::2], width), width, rf, how), width)
    return to_bytes(out, width)


def flat(pans):
    """pans as the C entry point takes them: left then right per track, (1.0, 1.0) where there is none"""
    if pans is None:
        return None
    return [f for p in pans for f in ((1.0, 1.0) if p is None else factors(tuple(p) if isinstance(p, (tuple, list)) else p))]


_DESK = {}


def desk(key, subs, gains, pans, master_gain, width, how=RIGHT):
    """(the tracks as the master takes them, post-fader and post-pan, as bytes of the song's length; the master's bytes; the master's bytes
    in front of its gain), made once per key and setting"""
    at = (key, gains, pans, master_gain, how)
    if at in _DESK:
        return _DESK[at]
    total = max([len(s) for s in subs] + [0])
    out, posts = bytes(total), []
    for t, sub in enumerate(subs):
        sub = sub + bytes(total - len(sub))
        g = 1.0 if gains is None else gains[t]
        pan = None if pans is None or pans[t] is None else factors(tuple(pans[t]) if isinstance(pans[t], (tuple, list)) else pans[t])
        if how == SWAPPED and pan is not None:
            pan = pan[::-1]
        if how == ONE_PRODUCT and pan is not None:
            sub = stereo(sub, width, g * pan[0], g * pan[1])
        elif how == PAN_FIRST:
            if pan is not None:
                sub = stereo(sub, width, *pan)
            sub = mul(sub, width, g)
        else:
            sub = mul(sub, width, g, how)                    # the gain first,
            if pan is not None:
                sub = stereo(sub, width, *pan, how)          # then the pan: two roundings
        posts.append(sub)
        if how == MASTER_PER_TRACK and master_gain is not None:
            sub = mul(sub, width, master_gain)
        out = audioop.add(out, sub, width)
    before = out
    if master_gain is not None and how != MASTER_PER_TRACK:
        out = mul(out, width, master_gain, how)              # once, behind the last track
    _DESK[at] = (posts, out, before)
    return _DESK[at]


def rows_of(key, subs, gains, pans, master_gain, width, a, b):
    posts, out, _before = desk(key, subs, gains, pans, master_gain, width)
    return [row_of(ints(p, width)[a:b], a, 2) for p in posts] + [row_of(ints(out, width)[a:b], a, 2)]


class WithDesk:
    """N.Sequence behind render_window, which calls render(first, n, out, out_sample): through sh_seq_render_desk"""

    def __init__(self, seq, gains, pans, master_gain):
        self.seq, self.gains, self.pans, self.master = seq, gains, flat(pans), 1.0 if master_gain is None else master_gain

    def render(self, a, n, out, out_sample):
        self.seq.render(a, n, out, out_sample, gains=self.gains, pans=self.pans, master=self.master)


def metered(N, seq, width, a, b, gains, pans, master_gain, out_sample=0):
    """(rows, the rendered bytes, the guards intact) of a metered desk render into a 0x5A-filled buffer"""
    n = b - a
    inner = (out_sample + n) * width
    parent = N.DeviceBuffer.from_bytes(b"\x5a" * (64 + inner + 64))
    rows = seq.render(a, n, parent.view(64, inner), out_sample, gains=gains, meters=True, pans=flat(pans),
                      master=1.0 if master_gain is None else master_gain)
    got = parent.download_bytes(64 + inner + 64)
    at = 64 + out_sample * width
    return rows, got[at:at + n * width], got[:at] == b"\x5a" * at and got[at + n * width:] == b"\x5a" * 64


# ---- 1: the reference tells the chain from its wrong forms -------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_reference_differs_from_every_wrong_form_inside_the_pile_up(kind, width):
    _instruments, _tracks, nch, subs, total, _level = the_song(kind, width)
    assert nch == 2
    T, L = TILE[width], LANE[width]
    lo, hi = (T + 3 * L) * width, (3 * T + L) * width
    top = 2 ** (8 * width - 1)
    for gains in (GAINS[0], GAINS[3]):
        for pans in PANS[:2]:
            _posts, want, before = desk((kind, width), subs, gains, pans, 0.7, width)
            found = {how: differs(want[lo:hi], desk((kind, width), subs, gains, pans, 0.7, width, how)[1][lo:hi]) for how in WRONG}
            print("%s, width %d, gains %s, pans %s: bytes of the pile-up window that differ: %s" % (kind, width, gains, pans, found))
            assert all(n > 0 for n in found.values()), found
            low, high = audioop.minmax(before[lo:hi], width)
            assert high == top - 1 or low == -top, "the master does not saturate in front of its gain"
            assert audioop.max(want[lo:hi], width) < top - 1      # and its gain, applied once behind, brings it down again


# ---- 2: the whole song, through the mixer ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_whole_song_is_the_reference_chain_byte_for_byte(gpu, kind, width):
    from synthesizer_amd import mixer
    instruments, tracks, nch, subs, total, level = the_song(kind, width)
    samples = as_samples(instruments, width, RATE)
    with mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, 2, width) as cs:
        assert cs.level == level and cs.ntracks == 3 and cs.frames * 2 == total
        for gains in (None, GAINS[0], GAINS[3]):
            for pans in PANS:
                for master_gain in MASTERS:
                    want = desk((kind, width), subs, gains, pans, master_gain, width)[1]
                    got = bytes(cs.render(gains=gains, pans=pans, master=master_gain).view_frame_data())
                    assert got == want, "gains %s, pans %s, master %s: %d bytes differ" % (gains, pans, master_gain, differs(got, want))


# ---- 3: windows, through the C entry point ----------------------------------------------------------------------------------------------
SETTINGS = [(GAINS[0], PANS[0], 0.7), (GAINS[3], PANS[1], -1.3), (None, PANS[3], None)]


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_window_holds_its_slice_and_nothing_beside_it_is_written(gpu, kind, width):
    N = gpu
    instruments, tracks, nch, subs, total, level = the_song(kind, width)
    wins = windows("balance", width, total)
    assert any(a % 2 for a, _b in wins), "no window starts on an odd sample"
    seq, _samples = raw_tracks(N, instruments, tracks, 2, width)
    assert N.SEQ_LEVELS[seq.info()["level"]] == level and seq.tracks()[0] == 3
    for gains, pans, master_gain in SETTINGS:
        want = desk((kind, width), subs, gains, pans, master_gain, width)[1]
        for a, b in wins:
            for out_sample in (0, 1):
                got, front, back = render_window(N, WithDesk(seq, gains, pans, master_gain), width, a, b, out_sample)
                assert got == want[a * width:b * width], (gains, pans, master_gain, a, b, out_sample)
                assert front == b"\x5a" * 64 and back == b"\x5a" * 64, (a, b, out_sample)
    seq.free()


def test_the_windows_at_16_bits_under_the_other_alignment_scheme(gpu):
    in_a_child_under_the_other_alignment_scheme(
        __file__, ["test_every_window_holds_its_slice_and_nothing_beside_it_is_written[%s-2]" % kind for kind in KINDS])


# ---- 4: meters ---------------------------------------------------------------------------------------------------------------------------
METERED = [(GAINS[0], ((0.0, 0.0), -1.0, (1.5, 0.25)), 0.7), (GAINS[3], PANS[0], -1.3), (None, PANS[1], None)]


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_rows_are_post_pan_and_the_masters_row_is_over_the_stored_bytes(gpu, kind, width):
    N = gpu
    instruments, tracks, nch, subs, total, _level = the_song(kind, width)
    T, L = TILE[width], LANE[width]
    wins = [(0, total), (T + 3 * L + 1, 3 * T + L), (2 * T + 5, 3 * T - 7), (T - 1, T + 1)]      # whole, odd, idle, across a tile's edge
    seq, _samples = raw_tracks(N, instruments, tracks, 2, width)
    for gains, pans, master_gain in METERED:
        want_bytes = desk((kind, width), subs, gains, pans, master_gain, width)[1]
        for a, b in wins:
            want = rows_of((kind, width), subs, gains, pans, master_gain, width, a, b)
            for out_sample in (0, 1):
                rows, got, guards = metered(N, seq, width, a, b, gains, pans, master_gain, out_sample)
                assert rows == want, "gains %s, pans %s, master %s, window [%d, %d) at %d:\n%s\n%s" % (gains, pans, master_gain, a, b, out_sample, rows, want)
                assert got == want_bytes[a * width:b * width] and guards, (gains, pans, master_gain, a, b, out_sample)
            assert got == render_window(N, WithDesk(seq, gains, pans, master_gain), width, a, b, 1)[0]       # the unmetered render's bytes
            if 2 * T <= a and b <= 3 * T:
                assert rows == [ZERO] * 4                       # the idle tile: nothing sounds
    # a track whose pans are (0.0, 0.0) reads zero; a hard-left track's right channel reads peak 0, its left one sounds
    gains, pans, master_gain = METERED[0]
    rows = metered(N, seq, width, 0, total, gains, pans, master_gain)[0]
    assert rows[0] == ZERO and rows[1][0][1] == 0 and rows[1][1][1] == 0 and rows[1][0][0] > 0 and rows[2][0][1] > 0 and rows[3][0][0] > 0
    seq.free()


# ---- 5: identities -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_steps_that_do_nothing_change_no_byte_and_chunks_are_the_whole(gpu, width):
    from synthesizer_amd import mixer
    N = gpu
    instruments, tracks, nch, subs, total, _level = the_song("balance", width)
    samples = as_samples(instruments, width, RATE)
    gains = GAINS[3]
    with mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, 2, width) as cs:
        plain = bytes(cs.render(gains=gains).view_frame_data())
        assert plain == desk(("balance", width), subs, gains, None, None, width)[1]
        assert bytes(cs.render(gains=gains, pans=[None] * 3, master=None).view_frame_data()) == plain
        assert bytes(cs.render(gains=gains, pans=[(1.0, 1.0)] * 3, master=1.0).view_frame_data()) == plain
        one = bytes(cs.render(gains=gains, pans=((1.0, 1.0), 0.3, None), master=0.7).view_frame_data())
        assert one == bytes(cs.render(gains=gains, pans=(None, 0.3, None), master=0.7).view_frame_data()) != plain
        # the same through the kernels of the desk: every factor 1.0 is the render with gains
        got = render_window(N, WithDesk(cs._seq, list(gains), [None] * 3, None), width, 0, total, 0)[0]
        assert got == plain
        # master=0.0: silence, every byte written
        for a, b in ((0, total), (TILE[width] + 3, 2 * TILE[width] + 1)):
            got, front, back = render_window(N, WithDesk(cs._seq, list(gains), PANS[0], 0.0), width, a, b, 1)
            assert got == bytes((b - a) * width) and front == back == b"\x5a" * 64
        # chunks of a length that is no multiple of the lane width
        frames = 333
        assert (2 * frames) % LANE[width]
        for pans, master_gain in ((PANS[1], -1.3), (PANS[0], None)):
            parts = list(cs.chunks(frames, gains=gains, pans=pans, master=master_gain))
            assert len(parts) == -(-cs.frames // frames) > 4
            assert b"".join(bytes(p.view_frame_data()) for p in parts) == desk(("balance", width), subs, gains, pans, master_gain, width)[1]
            pairs = list(cs.chunks(frames, gains=gains, pans=pans, master=master_gain, meters=True))
            assert [bytes(s.view_frame_data()) for s, _l in pairs] == [bytes(p.view_frame_data()) for p in parts]
            third = rows_of(("balance", width), subs, gains, pans, master_gain, width, 4 * frames, 6 * frames)
            assert [(r.peak, r.sum_squares) for r in pairs[2][1].tracks + [pairs[2][1].master]] == third


# ---- 6: thirty-two tracks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [2, 4])
def test_thirty_two_tracks_each_with_its_own_pair_of_factors(gpu, width):
    N = gpu
    T, L = TILE[width], LANE[width]
    rng = np.random.default_rng(320 + width)
    instruments = [(pcm(rng, width, 2 * 40, 0.9), 2), (pcm(rng, width, 2 * 25, 0.9), 2)]
    tracks = [[_ev(T // 2 + 20 + 3 * t, t % 2, [None, 1.3, 0.8][t % 3])] for t in range(32)]      # one short event each, all in tile 1, overlapping
    pans = tuple((round(0.05 + 0.045 * t, 3), round(1.4 - 0.06 * t, 3)) for t in range(32))
    gains = tuple([1.0, 0.9, 1.7, -0.6][t % 4] for t in range(32))
    assert len(set(pans)) == 32
    subs = subs_of(instruments, tracks, width, 2)
    total = max(len(s) for s in subs) // width
    assert T < total < 2 * T and min(int(RATE * t[0][0]) * 2 for t in tracks) >= T
    key = ("thirty-two", width)
    posts, want, before = desk(key, subs, gains, pans, 0.9, width)
    top = 2 ** (8 * width - 1)
    assert audioop.minmax(before, width)[1] == top - 1 or audioop.minmax(before, width)[0] == -top      # the master saturates on the way
    shifted = desk(key, subs, gains, pans[1:] + pans[:1], 0.9, width)[1]
    assert differs(want, shifted) > 0 and differs(want, desk(key, subs, gains, pans, 0.9, width, SWAPPED)[1]) > 0
    seq, _samples = raw_tracks(N, instruments, tracks, 2, width)
    assert seq.tracks()[0] == 32
    for a, b in ((0, total), (T + 37, total - 3)):
        got, front, back = render_window(N, WithDesk(seq, list(gains), pans, 0.9), width, a, b, 1)
        assert got == want[a * width:b * width] and front == back == b"\x5a" * 64, (a, b)
        rows, got, guards = metered(N, seq, width, a, b, list(gains), pans, 0.9)
        assert rows == rows_of(key, subs, gains, pans, 0.9, width, a, b) and got == want[a * width:b * width] and guards, (a, b)
        assert len({r for r in rows[:32]}) == 32                  # every track's own row
    seq.free()


# ---- 7: what the C entry point refuses ---------------------------------------------------------------------------------------------------
def test_the_entry_point_refuses_on_the_host_and_writes_nothing(gpu):
    N = gpu
    lib = N.lib()
    from synthesizer_amd.sample import Sample
    instruments, tracks, nch, subs, total, _level = the_song("balance", 2)
    seq, samples = raw_tracks(N, instruments, tracks, 2, 2)
    bufs, table, segtab, nbytes = Sample(samplerate=RATE, nchannels=2, samplewidth=2)._compile_events(with_samples(samples, [e for t in tracks for e in t]))
    flat_song = N.Sequence(bufs, table, segtab, 2, 2, nbytes // 2)
    m_instruments, m_tracks, _nch, _subs, _total, _lv = the_song("bus", 2)
    mono, _m = raw_tracks(N, m_instruments, m_tracks, 1, 2)
    out = N.DeviceBuffer.from_bytes(b"\x5a" * 4000)
    rows = (N.SeqMeter * 5)()
    C.memset(rows, 0xAB, C.sizeof(rows))
    untouched = bytes(rows)
    dbl = lambda *v: (C.c_double * len(v))(*v)                 # noqa: E731
    nan, inf = float("nan"), float("inf")
    ones, six = dbl(1.0, 1.0, 1.0), dbl(0.5, 0.5, 1.0, 1.0, 0.0, 1.0)
    for what, args, message in (
        ("a mono song with pans", (mono.handle, 0, 100, out.handle, 0, ones, 3, six, 6, 1.0, None, 0), b"pans need a stereo song, this one has 1 channels"),
        ("a flat song", (flat_song.handle, 0, 100, out.handle, 0, None, 0, None, 0, 0.5, None, 0), b"the song has no tracks"),
        ("a flat song with pans", (flat_song.handle, 0, 100, out.handle, 0, None, 0, six, 6, 1.0, None, 0), b"the song has no tracks"),
        ("too few gains", (seq.handle, 0, 100, out.handle, 0, dbl(1.0, 1.0), 2, six, 6, 1.0, None, 0), b"2 gains for 3 tracks"),
        ("a pan factor too few", (seq.handle, 0, 100, out.handle, 0, ones, 3, six, 5, 1.0, None, 0), b"5 pan factors for 3 tracks"),
        ("one pan per track", (seq.handle, 0, 100, out.handle, 0, ones, 3, ones, 3, 1.0, None, 0), b"3 pan factors for 3 tracks"),
        ("a row too few", (seq.handle, 0, 100, out.handle, 0, ones, 3, six, 6, 1.0, rows, 3), b"3 rows for 3 tracks and the master"),
        ("a row too many", (seq.handle, 0, 100, out.handle, 0, ones, 3, six, 6, 1.0, rows, 5), b"5 rows for 3 tracks and the master"),
        ("rows that are not counted", (seq.handle, 0, 100, out.handle, 0, ones, 3, six, 6, 1.0, rows, 0), b"0 rows for 3 tracks and the master"),
        ("a pan that is no number", (seq.handle, 0, 100, out.handle, 0, ones, 3, dbl(0.5, 0.5, 1.0, nan, 0.0, 1.0), 6, 1.0, rows, 4), b"pan 1: right factor is not finite"),
        ("an infinite pan", (seq.handle, 0, 100, out.handle, 0, None, 0, dbl(0.5, 0.5, 1.0, 1.0, -inf, 1.0), 6, 1.0, None, 0), b"pan 2: left factor is not finite"),
        ("a master that is no number", (seq.handle, 0, 100, out.handle, 0, ones, 3, six, 6, nan, rows, 4), b"master gain is not finite"),
        ("an infinite master", (seq.handle, 0, 100, out.handle, 0, None, 0, None, 0, inf, None, 0), b"master gain is not finite"),
        ("a gain that is no number", (seq.handle, 0, 100, out.handle, 0, dbl(1.0, nan, 1.0), 3, six, 6, 1.0, rows, 4), b"gain 1 is not finite"),
        ("NULL pans that are counted", (seq.handle, 0, 100, out.handle, 0, ones, 3, None, 6, 1.0, None, 0), b"NULL argument"),
        ("NULL gains that are counted", (seq.handle, 0, 100, out.handle, 0, None, 3, six, 6, 1.0, None, 0), b"NULL argument"),
        ("NULL rows that are counted", (seq.handle, 0, 100, out.handle, 0, ones, 3, six, 6, 1.0, None, 4), b"NULL argument"),
        ("a NULL song", (None, 0, 100, out.handle, 0, ones, 3, six, 6, 1.0, None, 0), b"NULL argument"),
        ("a NULL out", (seq.handle, 0, 100, None, 0, ones, 3, six, 6, 1.0, None, 0), b"NULL argument"),
        ("a range past the song", (seq.handle, total - 10, 11, out.handle, 0, ones, 3, six, 6, 0.5, rows, 4), b"range outside the song"),
        ("a range past out", (seq.handle, 0, 2000, out.handle, 1, ones, 3, six, 6, 0.5, None, 0), b"range outside out"),
    ):
        assert lib.sh_seq_render_desk(*args) == N.SH_ERR_INVALID, what
        err = lib.sh_last_error()
        assert err.startswith(b"sh_seq_render_desk") and message in err, (what, err)
        assert bytes(rows) == untouched, what
    assert out.download_bytes(4000) == b"\x5a" * 4000
    # and what it takes: NULL gains and NULL pans with a master alone, unmetered
    assert lib.sh_seq_render_desk(seq.handle, 0, 1000, out.handle, 0, None, 0, None, 0, 0.7, None, 0) == N.SH_OK
    want = desk(("balance", 2), subs, None, None, 0.7, 2)[1]
    assert out.download_bytes(2000) == want[:2000] and out.download_bytes(2000, 2000) == b"\x5a" * 2000 and bytes(rows) == untouched
    # a mono song has a master fader, and an empty window zeroes the rows
    assert lib.sh_seq_render_desk(mono.handle, 0, 0, out.handle, 0, None, 0, None, 0, 0.7, rows, 4) == N.SH_OK
    assert bytes(rows) == bytes(4 * 40) + untouched[4 * 40:]
    for s in (seq, flat_song, mono):
        s.free()
