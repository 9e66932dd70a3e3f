"""The placed-sample mixer and compiled songs in the UPPER half of their documented range: every kernel of sequence.hip -- the k_seq_*
mixing kernels behind the seven sh_mix_events* entry points and the k_win_* window kernels behind sh_seq_render, sh_seq_render_gains and
sh_seq_render_meters -- with song coordinates past 2^31 samples and up to shq::MAX_TRACK_SAMPLES = 2^32 - 65536, where one `int`, one sum
that wraps or one tile number in the wrong width would go unnoticed by songs of four tiles at sample 0.

Nothing large is computed on the CPU.  The reference chain places an event by padding silence in front of it, so for a base B that is a
multiple of the channel count the bytes of the far window [B + a, B + b) are the bytes [a, b) of the same list placed at 0: the near
songs of tests/seqcases.py that the compiled, tracks and meters files render (the live-``audioop`` reference and their self-check) are
used as they stand, the product's packer makes the table of the NEAR list, and B is added to the table's ``dst_sample`` column -- the
table is an input of the entry points.  Expected bytes come from ``audioop`` alone, never from the product.  A compiled song's length is
only a number and a window of it renders into a small buffer; the mixing kernels get a track of that many bytes of which only the
song's own tiles and a guard on either side are ever uploaded or read back.

The bases, T and L being the tile and lane of the width:
    mid    2^31 - T            the near event that runs through [T - 1, T + 1) crosses sample 2^31; the pile-up lies just above it
    top    MAX - 4 T           the song's four tiles are the last four a song can have
    dm     2^31 - 32768 - n    a downmix song (n samples) ends exactly on the limit the kernels' 2 * dst and 2 * n set; not tile-aligned,
                               so the song's idle tile is no whole tile there and FOUR tiles are active, not three"""
import ctypes as C

import numpy as np
import pytest

from tests.seqcases import (GAINS, HELD, LEVEL_NAME, LEVELS, RATE, WithGains, _ev, as_samples, check_song, compiled_raw, master, metered, mix_events, named,
                            raw_tracks, reference, render_window, seq_create, song, subs_of, the_song, windows, with_samples)
from tests.seqref import LANE, TILE, differs, mix, pcm

pytestmark = pytest.mark.gpu

MAX = 2 ** 32 - 65536                                       # shq::MAX_TRACK_SAMPLES
DM_LIMIT = 2 ** 31 - 32768                                  # where a downmix ends at the latest
FAR_LEVELS = [lv for lv in LEVELS if lv != "downmix"]       # the downmix song has a base of its own
EVERY = [(lv, w) for lv in FAR_LEVELS for w in (1, 2, 3, 4) if (lv, w) != ("env", 3)]       # (no envelope at width 3: the product refuses)


def base_of(name, width, total=None):
    T = TILE[width]
    B = {"mid": 2 ** 31 - T, "top": MAX - 4 * T, "dm": DM_LIMIT - (total or 0)}[name]
    assert name == "dm" or (B % T == 0 and B % 2 == 0)
    return B


class _Pack:
    """Stands where the native module stands in compiled_raw / raw_tracks and keeps what they would hand N.Sequence: the product's packer
    makes the table of the near list once, and it is shifted before an entry point sees it."""

    @staticmethod
    def Sequence(*args, **kw):
        return args, kw


def far_sequence(N, args, B, track_first=None):
    """the packed near song B samples further out: (bufs, table, segtab, width, nch, total) -> a handle of B + total samples"""
    bufs, table, segtab, width, nch, total = args
    shifted = table.copy()
    shifted["dst_sample"] += np.uint64(B)
    return N.Sequence(bufs, shifted, segtab, width, nch, B + total, track_first=track_first), shifted


def far_bytes(want, B, a, b, width):
    """bytes [a, b) of the song placed at B: silence in front of B, then the near song's"""
    lead = max(0, B - a)
    out = (bytes(lead * width) + want)[(a - B + lead) * width:(b - B + lead) * width]
    assert len(out) == (b - a) * width
    return out


def tiles_touched(table, T):
    touched = set()
    for d, n in zip(table["dst_sample"].tolist(), table["nsamples"].tolist()):
        if n:
            touched.update(range(d // T, (d + n - 1) // T + 1))
    return len(touched)


def check_windows(N, seq, width, want, B, wins, out_samples=(0, 1, 8)):
    for a, b in wins:
        exp = far_bytes(want, B, a, b, width)
        for out_sample in out_samples:
            got, front, behind = render_window(N, seq, width, a, b, out_sample)
            assert got == exp, "window [%d, %d) = B + [%d, %d) at out_sample %d: %d bytes differ" % (a, b, a - B, b - B, out_sample, differs(got, exp))
            assert front == b"\x5a" * 64 and behind == b"\x5a" * 64, (a, b, out_sample)


_LAST = {}


def with_last_row(level, width):
    """(instruments, events, nch, expected bytes): the level's near list and one more row of the 97-frame instrument that ends exactly at
    near sample 4 T -- shifted by `top`, the song is MAX samples long.  The row is legal at every level: a mono source of a stereo song
    takes pan's (1.0, 1.0); 97 frames of a stereo song start and end on whole frames."""
    if (level, width) not in _LAST:
        instruments, events, nch, _want, _total = song(level, width)
        T = TILE[width]
        rest = {"pan": dict(pan=(1.0, 1.0))}.get(level, {})
        events = events + [_ev(4 * T // nch - HELD[2], 2, 0.9, **rest)]
        want = mix(b"", named(instruments, events), width, RATE, nch)
        assert len(want) == 4 * T * width
        _LAST[(level, width)] = (instruments, events, nch, want)
    return _LAST[(level, width)]


# ---- (a) windows of a far song through sh_seq_create / sh_seq_render -----------------------------------------------------------------------
@pytest.mark.parametrize("base", ["mid", "top"])
@pytest.mark.parametrize("level, width", EVERY)
def test_windows_of_a_far_song(gpu, level, width, base):
    N = gpu
    check_song(level, width)
    instruments, events, nch, want, total = song(level, width)
    T, L = TILE[width], LANE[width]
    B = base_of(base, width)
    (args, _kw), _samples = compiled_raw(_Pack, level, width)
    seq, table = far_sequence(N, args, B)
    info = seq.info()
    assert N.SEQ_LEVELS[info["level"]] == LEVEL_NAME.get(level, level)
    assert info["track_samples"] == B + total and info["nevents"] == len(events)
    assert info["ntiles"] == -(-(B + total) // T) and info["active_tiles"] == 3 == tiles_touched(table, T)
    wins = [(B + a, B + b) for a, b in windows(level, width, total) if (a, b) != (0, total)] + [(B - 5, B + L + 2)]
    if base == "mid":
        wins.append((2 ** 31 - 1, 2 ** 31 + 1))
        assert B + T == 2 ** 31 and any(d < 2 ** 31 < d + n for d, n in zip(table["dst_sample"].tolist(), table["nsamples"].tolist()))
    else:
        assert B + 4 * T == MAX
    check_windows(N, seq, width, want, B, wins)
    seq.free()


@pytest.mark.parametrize("row", [False, True], ids=["to_the_limit", "and_a_row_above_2_31"])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_windows_of_a_far_downmix_song(gpu, width, row):
    """the last downmix row ends exactly on 2^31 - 32768; `row`: one plain row of a MONO instrument above 2^31 in the same (chan) song"""
    N = gpu
    check_song("downmix", width)
    instruments, events, nch, want, total = song("downmix", width)
    assert nch == 1
    T, L = TILE[width], LANE[width]
    B = base_of("dm", width, total)
    wins = [(B + a, B + b) for a, b in windows("downmix", width, total) if (a, b) != (0, total)] + [(B - 5, B + L + 2)]
    if row:
        at = total + 32768 + T + 7                          # near; far it starts at sample 2^31 + T + 7
        instruments = instruments + [(pcm(np.random.default_rng(7000 + width), width, HELD[2], 0.6), 1)]
        events = events + [_ev(at, 3, 0.8)]
        near = want
        want = mix(b"", named(instruments, events), width, RATE, 1)
        assert want[:len(near)] == near and len(want) == (at + HELD[2]) * width and B + at > 2 ** 31
        wins += [(B + total - 5, B + total + 3), (2 ** 31 - 1, 2 ** 31 + 1), (B + at - 3, B + at + HELD[2]), (B + at + 1, B + at + 2)]
        total = at + HELD[2]
    (args, _kw), _samples = raw_tracks(_Pack, instruments, [events], 1, width)
    assert args[5] == total
    seq, table = far_sequence(N, args, B)
    assert max(d + n for d, n, f in zip(table["dst_sample"].tolist(), table["nsamples"].tolist(), table["flags"].tolist()) if f & N.MIX_EVENT_DOWNMIX) == DM_LIMIT
    info = seq.info()
    assert N.SEQ_LEVELS[info["level"]] == "chan" and info["track_samples"] == B + total and info["nevents"] == len(events)
    # B is no multiple of T: the near song's idle tile [2 T, 3 T) lies across two far tiles, both of which hold events
    assert info["ntiles"] == -(-(B + total) // T) and info["active_tiles"] == tiles_touched(table, T) == (5 if row else 4)
    check_windows(N, seq, width, want, B, wins)
    seq.free()


# ---- (b) a song of exactly MAX samples ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 4])
@pytest.mark.parametrize("level", ["plain", "rate", "balance"])
def test_a_song_of_exactly_the_greatest_length(gpu, level, width):
    N = gpu
    lib = N.lib()
    instruments, events, nch, want = with_last_row(level, width)
    T, L = TILE[width], LANE[width]
    B = base_of("top", width)
    (args, _kw), _samples = raw_tracks(_Pack, instruments, [events], nch, width)
    assert args[5] == 4 * T
    seq, table = far_sequence(N, args, B)
    info = seq.info()
    assert info["track_samples"] == MAX and info["ntiles"] == MAX // T and info["active_tiles"] == 3
    assert want[-L * width:] != bytes(L * width), "the last lane is silent"
    check_windows(N, seq, width, want, B, [(MAX - 1, MAX), (MAX - L - 1, MAX), (MAX - T - 3, MAX)])
    out = N.DeviceBuffer.from_bytes(b"\x5a" * 64)
    assert lib.sh_seq_render(seq.handle, MAX - 1, 2, out.handle, 0) == N.SH_ERR_INVALID
    err = lib.sh_last_error()
    assert err.startswith(b"sh_seq_render") and b"range outside the song" in err, err
    assert out.download_bytes(64) == b"\x5a" * 64
    rc, h = seq_create(N, args[0], table, args[2], width, nch, MAX + 1)
    err = lib.sh_last_error()
    assert rc == N.SH_ERR_INVALID and not h.value and err.startswith(b"sh_seq_create") and b"2^32 - 65536" in err, err
    seq.free()


# ---- (c) the whole far song in one launch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tracks", [False, True], ids=["flat", "two_tracks"])
def test_the_whole_far_song_in_one_launch_on_a_folded_grid(gpu, tracks):
    """sh_seq_render of (0, MAX): the heaviest-first `order` path, and a grid of MAX / 1024 = 4 194 240 workgroups, more than
    GRID_X_MAX = 2^21, folded into two dimensions -- sample 2^31 is tile 2^21, the first workgroup of the second grid row.  Width 1 only:
    at width 2 a song has at most MAX / 2048 = 2 097 120 tiles, just below 2^21, so the 16-bit kernels never run on a folded grid.
    `out` is 4 GiB, set to 0x5A on the device; the silence that the render must write is read back in 64 KiB windows at the head, across
    sample 2^31 and up to the song, and the peak of everything between them (sh_pcm_stats, tested past 2^32 samples) is 0."""
    N = gpu
    lib = N.lib()
    width, T = 1, TILE[1]
    B = base_of("top", width)
    instruments, events, nch, want = with_last_row("plain", width)
    gains = None
    if tracks:
        dealt = [events[0::2], events[1::2]]
        gains = GAINS[0][:2]
        want = master(subs_of(instruments, dealt, width, 1), gains, width)
        assert len(want) == 4 * T and gains == (0.5, 1.0)
    else:
        dealt = [events]
    (args, kw), _samples = raw_tracks(_Pack, instruments, dealt, 1, width)
    seq, _table = far_sequence(N, args, B, kw["track_first"] if tracks else None)
    assert seq.info()["ntiles"] == MAX // T == 4194240 > 2 ** 21 and seq.info()["track_samples"] == MAX and seq.tracks()[0] == (2 if tracks else 0)
    out = N.DeviceBuffer(MAX)
    try:
        out.zero()
        N.check(lib.sh_pcm_bias(out.handle, MAX, 1, 0x5A, out.handle))
        for at in (0, 2 ** 31 - 32, B + 100, MAX - 64):
            assert out.download_bytes(64, at) == b"\x5a" * 64, at
        seq.render(0, MAX, out, 0, gains=gains)
        got = out.download_bytes(4 * T, B)
        assert got == want, "%d bytes of the song differ" % differs(got, want)
        K = 65536
        for at in (0, 2 ** 31 - K // 2, B - K):
            assert out.download_bytes(K, at) == bytes(K), at
        for lo, hi in ((K, 2 ** 31 - K // 2), (2 ** 31 + K // 2, B - K)):
            view = out.view(lo, hi - lo)
            peak, squares = C.c_uint32(1), C.c_double(1.0)
            N.check(lib.sh_pcm_stats(view.handle, hi - lo, 1, C.byref(peak), C.byref(squares)))
            assert peak.value == 0 and squares.value == 0.0, (lo, hi, peak.value)
    finally:
        out.free()
        seq.free()


# ---- (d) tracks and meters far out ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, width, base", [("bus", w, "mid") for w in (1, 2, 3, 4)] + [("bus", 2, "top"), ("bus", 4, "top"), ("balance", 2, "mid"),
                                                                                           ("balance", 4, "mid")])
def test_tracks_and_meters_far_out(gpu, kind, width, base):
    N = gpu
    instruments, tracks, nch, subs, total, level = the_song(kind, width)
    T, L = TILE[width], LANE[width]
    B = base_of(base, width)
    (args, kw), _samples = raw_tracks(_Pack, instruments, tracks, nch, width)
    assert args[5] == total
    seq, _table = far_sequence(N, args, B, kw["track_first"])
    assert N.SEQ_LEVELS[seq.info()["level"]] == level and seq.tracks()[0] == 3 and seq.info()["active_tiles"] == 3
    wins = [(T + 3 * L, 3 * T + L), (T, T + 1), (T - 5, T + L + 3)]         # the pile-up, one sample, mid-lane at both ends across a tile's edge
    if kind == "balance":
        wins.append((T + 3 * L + 1, 3 * T + L))             # left / right parity from (uint64_t)s0 + j
        assert base == "mid" and (B + wins[-1][0]) % 2 == 1 and B + wins[-1][0] > 2 ** 31
    if base == "mid":
        assert B + wins[1][0] == 2 ** 31
    for gains in [None] + GAINS:
        want = master(subs, gains, width)
        for a, b in wins:
            exp = want[a * width:b * width]
            got, front, behind = render_window(N, WithGains(seq, gains), width, B + a, B + b, 1)
            assert got == exp, "gains %s, window B + [%d, %d): %d bytes differ" % (gains, a, b, differs(got, exp))
            assert front == b"\x5a" * 64 and behind == b"\x5a" * 64, (gains, a, b)
            rows, metered_bytes, guards = metered(N, seq, width, B + a, B + b, gains)
            ref = reference((kind, width), subs, gains, width, nch, a, b)
            assert rows == ref, "gains %s, window B + [%d, %d):\n%s\n%s" % (gains, a, b, rows, ref)
            assert metered_bytes == exp and guards, (gains, a, b)
    seq.free()


# ---- (e) the mixing kernels through the seven entry points ---------------------------------------------------------------------------------
def mix_through(N, level, bufs, table, segtab, width, nch, track, track_samples):
    """one call of the level's own entry point: the chan table narrowed to that entry point's struct (the fields it lacks hold nothing in
    a list of its level)"""
    name = LEVEL_NAME.get(level, level)
    dtype = N.MIX_LEVELS[N.SEQ_LEVELS.index(name)].dtype
    t = np.zeros(len(table), dtype=dtype)
    for field in dtype.names:
        t[field] = table[field]
    for field in set(table.dtype.names) - set(dtype.names):
        assert not table[field].any() or field in ("src_frames", "inrate", "outrate", "src_channels"), (level, field)
    return mix_events(N, name, bufs, t, segtab, width, nch, track, track_samples)


@pytest.mark.parametrize("level, width, base", [(lv, w, "mid") for lv, w in EVERY] + [("downmix", w, "dm") for w in (1, 2, 3, 4)] +
                         [(lv, w, "top") for lv, w in EVERY if w in (1, 2)])
def test_the_mixing_kernels_far_out(gpu, level, width, base):
    """a track of (B + total) samples of which only [B - T, B + 4 T) is ever uploaded: a 0x5A guard tile, a quiet base, a guard behind.
    `top`: with the last row the track is MAX samples long and the guard behind lies behind the track's last sample.  The downmix list
    goes out as far as a downmix may (`dm`)."""
    N = gpu
    T = TILE[width]
    if base == "top":
        instruments, events, nch, _silent = with_last_row(level, width)
        total = 4 * T
    else:
        instruments, events, nch, _silent, total = song(level, width)
    B = base_of(base, width, total)
    quiet = pcm(np.random.default_rng(8000 + 10 * LEVELS.index(level) + width), width, total, 0.4)
    want = mix(quiet, named(instruments, events), width, RATE, nch)
    assert len(want) == len(quiet) and want != quiet        # every event fits: the entry points do not grow a track
    (args, _kw), _samples = raw_tracks(_Pack, instruments, [events], nch, width)
    bufs, table, segtab, _w, _nch, packed = args
    assert packed == total and (base != "top" or B + total == MAX) and (base != "dm" or B + total == DM_LIMIT)
    table = table.copy()
    table["dst_sample"] += np.uint64(B)
    front, behind = b"\x5a" * (T * width), b"\x5a" * ((4 * T - total) * width + 64)
    track = N.DeviceBuffer((B + 4 * T) * width + 64)
    try:
        track.upload(np.frombuffer(front + quiet + behind, dtype=np.uint8), (B - T) * width)
        rc = mix_through(N, level, bufs, table, segtab, width, nch, track, B + total)
        assert rc == N.SH_OK, N.lib().sh_last_error()
        got = track.download_bytes(len(front) + len(quiet) + len(behind), (B - T) * width)
    finally:
        track.free()
    mixed = got[len(front):len(front) + len(quiet)]
    assert mixed == want, "%d bytes differ (%d from the untouched base)" % (differs(mixed, want), differs(mixed, quiet))
    assert got[:len(front)] == front and got[len(front) + len(quiet):] == behind


# ---- (f) the product API ------------------------------------------------------------------------------------------------------------------
def test_the_product_compiles_and_renders_a_song_of_the_greatest_length(gpu):
    from synthesizer_amd import mixer
    rng = np.random.default_rng(99)
    instruments = [(pcm(rng, 2, HELD[2], 0.9), 1), (pcm(rng, 2, HELD[1], 0.9), 1)]
    near = [(0, 0, 0.8), (50, 1, 1.7), (400 - HELD[2], 0, None)]
    want = mix(b"", named(instruments, [_ev(*e) for e in near]), 2, RATE, 1)
    assert len(want) == 2 * 400
    B = MAX - 400
    far = [_ev(B + f, i, v) for f, i, v in near]
    assert all(int(RATE * e[0]) == B + f for e, (f, _i, _v) in zip(far, near))      # seconds = frame / 8192 is exact
    samples = as_samples(instruments, 2, RATE)
    with mixer.compile_sequence(with_samples(samples, far), RATE, 1, 2, name="far") as cs:
        assert len(cs) == cs.frames == MAX and cs.level == "plain" and cs.info()["ntiles"] == MAX // TILE[2]
        got = cs.render(MAX - 300, 300)
        assert len(got) == 300 and bytes(got.view_frame_data()) == want[2 * 100:]
        c = 300                                             # as chunks(300) would: its last three starts, the last chunk shorter
        starts = list(range(0, MAX, c)[-3:])
        assert starts[0] < B < starts[1] and MAX - starts[2] == MAX % c != 0
        for at in starts:
            n = min(c, MAX - at)
            part = cs.render(at, n)
            assert len(part) == n and bytes(part.view_frame_data()) == far_bytes(want, B, at, at + n, 2), at
        for a, n in ((MAX - 3, 4), (MAX + 1, None)):
            with pytest.raises(ValueError, match="CompiledSequence"):
                cs.render(a, n)
