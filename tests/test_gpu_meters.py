"""GPU parity of the level meters of a song of tracks -- CompiledSequence.render(..., meters=True) / N.Sequence.render(meters=True) /
sh_seq_render_meters -- against live ``audioop`` and integers.  The expected rows come from tests/seqcases.py's per-track reference
(every track folded on its own, ``audioop.mul`` by its gain -- none at exactly 1.0 --, padded with silence; the master ``audioop.add`` in
track order), cut to the window and reduced here with numpy int64 / uint64 and Python ints: per channel (song sample s is channel s & 1
of a stereo song) the peak, max |x|, and the exact sum of x * x.  Expected values never come from the product.  Rate 8192 and the
four-tile songs of the neighbouring files; one song per kernel template: 16-bit plain (k_win_plain16), the 16-bit stereo balance song at
level chan (k_win_16, the next record's index held ahead) and the 16-bit rate song (k_win_16, a whole record held ahead), widths 1, 3, 4
plain (k_win_w), and the stereo balance song at width 4 beside them (two channels of two sums)."""
import audioop
import ctypes as C
import math

import numpy as np
import pytest

from tests.seqcases import (GAINS, RATE, _ev, as_samples, bus_song, in_a_child_under_the_other_alignment_scheme, master, metered, post_fader, raw_tracks,
                            reference, subs_of, the_song, windows, with_samples)
from tests.seqref import LANE, TILE, pcm

pytestmark = pytest.mark.gpu

ZERO = ((0, 0), (0, 0))


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def to_bytes(v, width):
    v = np.asarray(v, dtype=np.int64)
    if width == 3:
        return v.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    return v.astype({1: np.int8, 2: "<i2", 4: "<i4"}[width]).tobytes()


def check_against_audioop(key, subs, gains, width, nch, a, b, rows):
    """where the window is whole frames: the peaks are audioop.max of each channel, and -- wherever the expected sum is below 2^53, where
    audioop's own float sum is exact -- Levels.rms is audioop.rms.  The number of rows that audioop.rms judged."""
    from synthesizer_amd import mixer
    if nch == 2 and (a % 2 or b % 2):
        return 0
    scaled, mast, _bytes = post_fader(key, subs, gains, width)
    judged = 0
    for x, (peak, sq) in zip(scaled + [mast], rows):
        lv = mixer.Levels(peak, sq, (b - a) // nch, width, nch, RATE)
        for c in range(nch):
            data = to_bytes(x[a:b][c::nch], width)           # audioop.tomono(frames, w, 1, 0) / (.., 0, 1): the channel's own samples
            assert lv.peak[c] == audioop.max(data, width), (gains, a, b, c)
            if sq[c] < 2 ** 53:
                assert lv.rms[c] == audioop.rms(data, width), (gains, a, b, c)
                judged += 1
        if nch == 1:
            assert lv.peak[0] == lv.peak[1] and lv.rms[0] == lv.rms[1]
    return judged


# ---- the songs, one per kernel template ----------------------------------------------------------------------------------------------------
SONGS = [("bus", 2), ("balance", 2), ("rate", 2), ("bus", 1), ("bus", 3), ("bus", 4), ("balance", 4)]


def the_windows(kind, width, total):
    """whole song (the heaviest-first permutation), mid-lane start and end, across a tile's edge, one sample, inside the idle tile, the
    pile-up, (balance) an odd first sample; and one lane, and a window that ends at the song's mid-lane end"""
    T, L = TILE[width], LANE[width]
    return windows(kind if kind == "balance" else "plain", width, total) + [(2 * L, 3 * L), (T + 5, total)]


def plain(N, seq, width, a, b, gains):
    out = N.DeviceBuffer.from_bytes(b"\x5a" * ((b - a) * width))
    seq.render(a, b - a, out, 0, gains=gains)
    return out.download_bytes((b - a) * width)


# ---- 1, 2: the rows are the reference's, the bytes those of the render without meters ------------------------------------------------------
@pytest.mark.parametrize("kind, width", SONGS)
def test_rows_equal_the_reference_and_the_bytes_are_the_unmetered_render(gpu, kind, width):
    N = gpu
    instruments, tracks, nch, subs, total, level = the_song(kind, width)
    T = TILE[width]
    wins = the_windows(kind, width, total)
    judged = 0
    for gains in [None] + GAINS:                                # on the CPU first: audioop.rms judges at least one case of this width
        for a, b in wins:
            judged += check_against_audioop((kind, width), subs, gains, width, nch, a, b, reference((kind, width), subs, gains, width, nch, a, b))
    assert judged > 0, "no expected sum of width %d is below 2^53" % width
    assert any(2 * T <= a and b <= 3 * T for a, b in wins) and any(b == total and total % LANE[width] for a, b in wins)
    seq, _samples = raw_tracks(N, instruments, tracks, nch, width)
    assert N.SEQ_LEVELS[seq.info()["level"]] == level and seq.tracks()[0] == 3
    for gains in [None] + GAINS:
        want_bytes = post_fader((kind, width), subs, gains, width)[2]
        for a, b in wins:
            want = reference((kind, width), subs, gains, width, nch, a, b)
            for out_sample in (0, 1):
                rows, got, guards = metered(N, seq, width, a, b, gains, out_sample)
                assert rows == want, "gains %s, window [%d, %d) at out_sample %d:\n%s\n%s" % (gains, a, b, out_sample, rows, want)
                assert got == want_bytes[a * width:b * width] and guards, (gains, a, b, out_sample)
            assert got == plain(N, seq, width, a, b, gains), (gains, a, b)
            if 2 * T <= a and b <= 3 * T:
                assert rows == [ZERO] * 4                       # the idle tile: nothing sounds
    seq.free()


def test_rows_of_every_16_bit_song_under_the_other_alignment_scheme(gpu):
    in_a_child_under_the_other_alignment_scheme(
        __file__, ["test_rows_equal_the_reference_and_the_bytes_are_the_unmetered_render[%s-%d]" % s for s in SONGS if s[1] == 2])


# ---- 3: the edge mask --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_full_scale_samples_beside_the_window_in_its_edge_lanes_do_not_count(gpu, width):
    N = gpu
    T, L = TILE[width], LANE[width]
    top = 2 ** (8 * width - 1)
    a, n = T + 3 * L + 3, T + 2 * L + 2                         # the window: mid-lane at both ends, across a tile's edge
    assert (a - 1) // L == a // L and (a + n) // L == (a + n - 1) // L      # the spikes share the lanes of the window's first and last samples
    rng = np.random.default_rng(70 + width)
    quiet = rng.integers(-top // 8, top // 8, n)
    spiky = to_bytes(np.concatenate([[-top], quiet, [top - 1]]), width)     # full scale at samples a - 1 and a + n, quiet between
    instruments = [(spiky, 1), (pcm(rng, width, 300, 0.1), 1)]
    tracks = [[_ev(a - 1, 0)], [_ev(a - 40, 1, 0.5), _ev(a + n - 100, 1)]]
    subs = subs_of(instruments, tracks, width, 1)
    key = ("edge", width)
    seq, _samples = raw_tracks(N, instruments, tracks, 1, width)
    for gains in (None, (0.5, 1.0), (-1.0, 1.7)):
        scaled, _m, want_bytes = post_fader(key, subs, gains, width)
        g0 = 1.0 if gains is None else abs(gains[0])
        assert abs(int(scaled[0][a - 1])) >= int(g0 * (top - 1)) and abs(int(scaled[0][a + n])) >= int(g0 * (top - 1)) - 1      # the spikes are there,
        want = reference(key, subs, gains, width, 1, a, a + n)
        assert want[0][0][0] <= g0 * (top // 8) + 1 < top - 1, "the reference peak of the window is not below full scale"   # and the window is quiet
        rows, got, guards = metered(N, seq, width, a, a + n, gains)
        assert rows[0][0] == want[0][0], (gains, rows[0], want[0])
        assert rows == want and got == want_bytes[a * width:(a + n) * width] and guards, gains
        wide = reference(key, subs, gains, width, 1, a - 1, a + n + 1)      # one sample more on each side: now they count
        assert wide[0][0][0] > want[0][0][0] and metered(N, seq, width, a - 1, a + n + 1, gains)[0] == wide
    seq.free()


# ---- 4: channels ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how, width", [("channels", 2), ("pan", 4), ("channels", 1)])
def test_a_track_that_sounds_only_left_reads_zero_on_the_right(gpu, how, width):
    from synthesizer_amd import mixer
    T = TILE[width]
    rng = np.random.default_rng(80 + width)
    src_ch = 2 if how == "channels" else 1
    instruments = [(pcm(rng, width, 600 * src_ch, 0.5), src_ch), (pcm(rng, width, 300 * src_ch, 0.4), src_ch)]
    left_only = dict(channels=(1.0, 0.0)) if how == "channels" else dict(pan=(1.0, 0.0))
    both = dict(channels=(0.75, 0.5)) if how == "channels" else dict(pan=(0.5, 1.0))
    F = T // 2
    tracks = [[_ev(3, 0, 0.8, **left_only), _ev(F - 100, 1, None, **left_only), _ev(2 * F + 7, 0, 1.3, **left_only)],
              [_ev(10, 1, None, **both), _ev(F + 50, 0, 0.9, **both)]]
    subs = subs_of(instruments, tracks, width, 2)
    key = (how, width)
    total = max(len(s) for s in subs) // width
    samples = as_samples(instruments, width, RATE)
    with mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, 2, width) as cs:
        assert cs.level == ("chan" if how == "channels" else "pan") and cs.frames == total // 2
        for gains in (None, (1.7, 0.5)):
            for fa, fb in ((0, total // 2), (5, F + 3), (F - 5, F + 60)):
                want = reference(key, subs, gains, width, 2, 2 * fa, 2 * fb)
                assert want[0][0][1] == 0 and want[0][1][1] == 0 and want[0][0][0] > 0 and want[1][0][1] > 0     # on the CPU: silent right, sounding left
                out, lv = cs.render(fa, fb - fa, gains=gains, meters=True)
                assert bytes(out.view_frame_data()) == post_fader(key, subs, gains, width)[2][2 * fa * width:2 * fb * width]
                got = [(r.peak, r.sum_squares) for r in lv.tracks + [lv.master]]
                assert got == want, (gains, fa, fb)
                assert lv.tracks[0].peak[1] == 0 and lv.tracks[0].sum_squares[1] == 0 
                assert lv.tracks[0].level_db_peak[1] == max(20.0 * math.log(1 / 2 ** (8 * width - 1), 10), -60.0)      # silence: (0 + 1) / 2^(8w-1), floored
                assert lv.master.frames == fb - fa and check_against_audioop(key, subs, gains, width, 2, 2 * fa, 2 * fb, got) >= 0
                if width == 2:                                   # and the master reads what Sample reads off the finished window
                    assert lv.master.level_db_peak == out.level_db_peak and lv.master.level_db_rms == out.level_db_rms
        parts = list(cs.chunks(F, gains=(1.7, 0.5), meters=True))
        assert [(r.peak, r.sum_squares) for _s, l in parts for r in [l.master]] == \
            [reference(key, subs, (1.7, 0.5), width, 2, 2 * at, min(2 * (at + F), total))[2] for at in range(0, total // 2, F)]


# ---- 5: no carry-over ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [2, 4])
def test_a_quiet_window_after_a_loud_one_reads_its_own_levels(gpu, width):
    N = gpu
    instruments, tracks, nch, subs, total, _level = the_song("bus", width)
    T, L = TILE[width], LANE[width]
    loud, quiet = (T + 3 * L, 3 * T + L), (3 * T + 20, 3 * T + 90)
    key = ("bus", width)
    r1, r2 = reference(key, subs, None, width, 1, *loud), reference(key, subs, None, width, 1, *quiet)
    assert r1[3][0][0] > r2[3][0][0] > 0 and r1[0][1][0] > r2[0][1][0] == 0 and r1[3][1][0] > r2[3][1][0]     # louder in peak and sum; track 0 silent after
    seq, _samples = raw_tracks(N, instruments, tracks, 1, width)
    assert metered(N, seq, width, *loud, None)[0] == r1
    assert metered(N, seq, width, *quiet, None)[0] == r2
    assert metered(N, seq, width, *loud, None)[0] == r1           # and the same again: the rows of a run do not depend on the run
    seq.free()


# ---- 6: muted and absent tracks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_muted_and_absent_tracks_read_zero(gpu, width):
    N = gpu
    instruments, tracks, nch, subs, total, _level = the_song("bus", width)
    T, L = TILE[width], LANE[width]
    key = ("bus", width)
    seq, _samples = raw_tracks(N, instruments, tracks, 1, width)
    gains = (0.0, 1.0, 0.0)
    for a, b in ((0, total), (T - 300, T + 3 * L + 50)):
        want = reference(key, subs, gains, width, 1, a, b)
        assert want[0] == want[2] == ZERO and want[3] == want[1] != ZERO
        rows, got, guards = metered(N, seq, width, a, b, gains)
        assert rows == want and rows[3] == rows[1] and guards
        assert got == (subs[1] + bytes(total * width))[a * width:b * width]
    a, b = T + 3 * L, 2 * T                                     # track 2 has no event in tile 1: absent, at any gain
    for gains in (None, (0.5, 1.0, -1.7)):
        want = reference(key, subs, gains, width, 1, a, b)
        assert want[2] == ZERO and want[0] != ZERO and want[1] != ZERO
        assert metered(N, seq, width, a, b, gains)[0] == want
    seq.free()


# ---- 7: wide sums --------------------------------------------------------------------------------------------------------------------------
def test_a_sum_of_squares_past_two_to_the_64_at_width_four(gpu):
    N = gpu
    T, L = TILE[4], LANE[4]
    rng = np.random.default_rng(91)
    loud = np.concatenate([[-2 ** 31] * 7, rng.integers(-2 ** 31, 2 ** 31, 500), [-2 ** 31] * 3])
    instruments = [(to_bytes(loud, 4), 1), (pcm(rng, 4, 300, 0.3), 1)]
    tracks = [[_ev(T - 200, 0)], [_ev(T - 100, 1, 0.5), _ev(5, 1)]]
    subs = subs_of(instruments, tracks, 4, 1)
    key = ("wide", 4)
    seq, _samples = raw_tracks(N, instruments, tracks, 1, 4)
    for gains in (None, (1.0, 0.5), (-1.0, 1.0)):
        for a, b in ((T - 202, T + 310), (T - 198, T + 2 * L + 1)):      # the second: five of the first seven inside, across the tile's edge
            x = post_fader(key, subs, gains, 4)[0][0][a:b]
            want = reference(key, subs, gains, 4, 1, a, b)
            assert int(np.count_nonzero(np.abs(x) >= 2 ** 31 - 1)) >= 5 and want[0][1][0] >= 2 ** 64 and want[2][1][0] >= 2 ** 64
            if gains is None:
                assert int(np.count_nonzero(x == -2 ** 31)) >= 5 and want[0][0][0] == 2 ** 31
            rows, _got, guards = metered(N, seq, 4, a, b, gains)
            assert rows == want and guards, (gains, a, b)
    seq.free()


def test_a_sum_of_squares_past_two_to_the_53_at_width_three(gpu):
    N = gpu
    T = TILE[3]
    rng = np.random.default_rng(93)
    loud = rng.choice([-2 ** 23, 2 ** 23 - 1, 2 ** 23 - 3], 600)
    instruments = [(to_bytes(loud, 3), 1), (pcm(rng, 3, 300, 0.3), 1)]
    tracks = [[_ev(T - 250, 0)], [_ev(T - 100, 1, 0.5)]]
    subs = subs_of(instruments, tracks, 3, 1)
    key = ("wide", 3)
    seq, _samples = raw_tracks(N, instruments, tracks, 1, 3)
    a, b = T - 251, T + 350
    for gains in (None, (0.999, 1.0)):
        want = reference(key, subs, gains, 3, 1, a, b)
        assert want[0][1][0] > 2 ** 53 and want[2][1][0] > 2 ** 53
        rows, _got, guards = metered(N, seq, 3, a, b, gains)
        assert rows == want and guards, gains
    seq.free()


# ---- 8: the C entry point --------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_refuses_on_the_host_and_leaves_out_and_rows(gpu):
    N = gpu
    L = N.lib()
    instruments, tracks, subs, total = bus_song(2)
    seq, samples = raw_tracks(N, instruments, tracks, 1, 2)
    from synthesizer_amd.sample import Sample
    bufs, table, segtab, nbytes = Sample(samplerate=RATE, nchannels=1, samplewidth=2)._compile_events(with_samples(samples, [e for t in tracks for e in t]))
    flat = N.Sequence(bufs, table, segtab, 2, 1, nbytes // 2)
    out = N.DeviceBuffer.from_bytes(b"\x5a" * 4000)
    rows = (N.SeqMeter * 5)()
    C.memset(rows, 0xAB, C.sizeof(rows))
    untouched = bytes(rows)
    dbl = lambda *v: (C.c_double * len(v))(*v)                 # noqa: E731
    ones = dbl(1.0, 1.0, 1.0)
    for what, args, message in (
        ("too few gains", (seq.handle, 0, 100, out.handle, 0, dbl(1.0, 1.0), 2, rows, 4), b"2 gains for 3 tracks"),
        ("too many gains", (seq.handle, 0, 100, out.handle, 0, dbl(1.0, 1.0, 1.0, 1.0), 4, rows, 4), b"4 gains for 3 tracks"),
        ("a gain that is no number", (seq.handle, 0, 100, out.handle, 0, dbl(1.0, float("nan"), 1.0), 3, rows, 4), b"gain 1 is not finite"),
        ("an infinite gain", (seq.handle, 0, 100, out.handle, 0, dbl(1.0, 1.0, float("inf")), 3, rows, 4), b"gain 2 is not finite"),
        ("a song without tracks", (flat.handle, 0, 100, out.handle, 0, dbl(1.0), 1, rows, 2), b"the song has no tracks"),
        ("a song without tracks and no gains", (flat.handle, 0, 100, out.handle, 0, None, 0, rows, 1), b"the song has no tracks"),
        ("NULL gains that are counted", (seq.handle, 0, 100, out.handle, 0, None, 3, rows, 4), b"NULL argument"),
        ("a NULL song", (None, 0, 100, out.handle, 0, ones, 3, rows, 4), b"NULL argument"),
        ("a NULL out", (seq.handle, 0, 100, None, 0, ones, 3, rows, 4), b"NULL argument"),
        ("NULL rows", (seq.handle, 0, 100, out.handle, 0, ones, 3, None, 4), b"NULL argument"),
        ("a row too few", (seq.handle, 0, 100, out.handle, 0, ones, 3, rows, 3), b"3 rows for 3 tracks and the master"),
        ("a row too many", (seq.handle, 0, 100, out.handle, 0, ones, 3, rows, 5), b"5 rows for 3 tracks and the master"),
        ("a range past the song", (seq.handle, total - 10, 11, out.handle, 0, ones, 3, rows, 4), b"range outside the song"),
        ("a range past out", (seq.handle, 0, 2000, out.handle, 1, ones, 3, rows, 4), b"range outside out"),
        ("an empty range past the song", (seq.handle, total + 1, 0, out.handle, 0, ones, 3, rows, 4), b"range outside the song"),
    ):
        assert L.sh_seq_render_meters(*args) == N.SH_ERR_INVALID, what
        err = L.sh_last_error()
        assert err.startswith(b"sh_seq_render_meters") and message in err, (what, err)
        assert bytes(rows) == untouched, what
    assert out.download_bytes(4000) == b"\x5a" * 4000
    # an empty window: SH_OK, the rows zeroed, out as it was
    assert L.sh_seq_render_meters(seq.handle, 50, 0, out.handle, 0, ones, 3, rows, 4) == N.SH_OK
    assert bytes(rows) == bytes(4 * 40) + untouched[4 * 40:] and out.download_bytes(4000) == b"\x5a" * 4000
    # NULL gains with ngains 0: every gain 1.0
    C.memset(rows, 0xAB, C.sizeof(rows))
    assert L.sh_seq_render_meters(seq.handle, 0, 1000, out.handle, 0, None, 0, rows, 4) == N.SH_OK
    got = [((r.peak[0], r.peak[1]), ((r.sq_hi[0] << 32) + r.sq_lo[0], (r.sq_hi[1] << 32) + r.sq_lo[1])) for r in rows[:4]]
    assert got == reference(("bus", 2), subs, None, 2, 1, 0, 1000) and bytes(rows)[4 * 40:] == untouched[4 * 40:]
    assert out.download_bytes(2000) == master(subs, None, 2)[:2000] and out.download_bytes(2000, 2000) == b"\x5a" * 2000
    assert all(r.sq_hi[0] == r.sq_hi[1] == 0 for r in rows[:4])    # 16 bits: one sum holds it
    seq.free()
    flat.free()
