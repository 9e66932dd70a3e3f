"""GPU parity of a song made of tracks -- mixer.compile_tracks / CompiledSequence(gains=...) / sh_seq_create_tracks, sh_seq_render_gains --
against live ``audioop`` on byte slices.  The expected bytes are the reference chain: tests/seqref.py's ``mix`` (the whole
event chain, event after event like mix_at) run ONCE PER TRACK, ``audioop.mul`` by the track's gain (none at exactly 1.0), the shorter
tracks padded with silence, ``audioop.add`` in track order -- then sliced per window.  Expected bytes never come from the product.  Rate
8192, instruments of 97 to 600 frames and a song of four tiles that ends mid-lane with one idle tile, as tests/seqcases.py has them.

Gain vectors that hold only 0.0 and 1.0 form no product at all (a gain of 1.0 takes no multiply, one of 0.0 skips the track), so there is
no truncated form for them to differ from: the floor-against-truncation assertion is made for every vector that multiplies."""
import audioop
import ctypes as C

import numpy as np
import pytest

from tests.seqcases import (GAINS, LEVEL_NAME, LEVELS, RATE, WithGains, _ev, as_samples, bus_song, in_a_child_under_the_other_alignment_scheme, ints,
                            master, named, raw_tracks, render_window, song, subs_of, windows, with_samples)
from tests.seqref import LANE, TILE, differs, mix, pcm

pytestmark = pytest.mark.gpu


def full_scale(width):
    return 2 ** (8 * width - 1) - 1


def saturates(data, width):
    lo, hi = audioop.minmax(data, width)
    return hi == full_scale(width) or lo == -full_scale(width) - 1


# ---- 1: grouping decides bytes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_grouping_decides_bytes(gpu, width):
    from synthesizer_amd import mixer
    instruments, tracks, subs, total = bus_song(width)
    T, L = TILE[width], LANE[width]
    lo, hi = (T + 3 * L) * width, (3 * T + L) * width
    grouped = master(subs, None, width)
    flat = mix(b"", named(instruments, [e for t in tracks for e in t]), width, RATE, 1)
    assert len(grouped) == len(flat) == total * width
    assert grouped[lo:hi] != flat[lo:hi], "the chain of sub-mixes is the flat list"
    assert saturates(grouped[lo:hi], width) and saturates(flat[lo:hi], width), "nothing saturates"
    assert all(saturates(s[lo:hi], width) for s in subs[:2])   # the two tracks saturate on their own, and the third is absent from their tile
    assert subs[2][T * width:2 * T * width] == bytes(T * width)
    samples = as_samples(instruments, width, RATE)
    with mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, 1, width, name="bus") as cs:
        assert cs.ntracks == 3 and cs.frames == total and cs.level == "plain"
        got = bytes(cs.render().view_frame_data())
        assert got == grouped, "%d bytes differ from the grouped oracle (%d from the flat one)" % (differs(got, grouped), differs(got, flat))
        assert cs._seq.tracks() == (3, 6)                       # tile 0: all three tracks, tile 1: two, tile 2: none, tile 3: the last
    with mixer.compile_sequence(with_samples(samples, [e for t in tracks for e in t]), RATE, 1, width) as cs:
        assert cs.ntracks is None and cs._seq.tracks() == (0, 0) and bytes(cs.render().view_frame_data()) == flat


# ---- 2: gains ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_gains_and_stems(gpu, width):
    from synthesizer_amd import mixer
    instruments, tracks, subs, total = bus_song(width)
    lo, hi = -full_scale(width) - 1, full_scale(width)
    for gains in GAINS:                                         # on the CPU first: floor, not truncation, decides bytes wherever a product is formed
        floored = truncated = 0
        for sub, g in zip(subs, gains):
            if g in (0.0, 1.0):
                continue
            x = np.clip(ints(sub, width).astype(np.float64) * g, lo, hi)
            assert np.array_equal(np.floor(x).astype(np.int64), ints(audioop.mul(sub, width, g), width))
            truncated += int(np.count_nonzero(np.trunc(x) != np.floor(x)))
            floored += int(np.count_nonzero((x < 0) & (x * 2 == np.floor(x * 2)) & (x != np.floor(x))))
        if any(g not in (0.0, 1.0) for g in gains):
            assert truncated > 0, gains
        if 0.5 in gains:
            assert floored > 0, "no negative product lands on .5"
    samples = as_samples(instruments, width, RATE)
    with mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, 1, width) as cs:
        for gains in GAINS:
            want = master(subs, gains, width)
            got = bytes(cs.render(gains=gains).view_frame_data())
            assert got == want, (gains, differs(got, want))
        assert master(subs, GAINS[0], width) != master(subs, GAINS[3], width) != master(subs, None, width)
        for t, sub in enumerate(subs):
            got = cs.stem(t)
            assert len(got) == total and bytes(got.view_frame_data()) == sub + bytes(total * width - len(sub)), t
        a, n = 1500, 700
        assert bytes(cs.stem(1, a, n).view_frame_data()) == (subs[1] + bytes(total * width))[a * width:(a + n) * width]


# ---- 3: every level and width --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level, width", [(lv, w) for lv in LEVELS for w in (1, 2, 3, 4) if (lv, w) != ("env", 3)])      # (no envelope at width 3)
def test_windows_of_every_level_through_the_entry_point(gpu, level, width):
    N = gpu
    instruments, events, nch, _flat, total = song(level, width)
    tracks = [events[0::3], events[1::3], events[2::3]]         # the list dealt over three tracks: the three loud notes part ways
    subs = subs_of(instruments, tracks, width, nch)
    T = TILE[width]
    seq, _samples = raw_tracks(N, instruments, tracks, nch, width)
    info = seq.info()
    assert N.SEQ_LEVELS[info["level"]] == LEVEL_NAME.get(level, level) and seq.tracks()[0] == 3
    assert info["track_samples"] == total and info["nevents"] == len(events) and info["ntiles"] == 4 and info["active_tiles"] == 3
    for gains in (None, (0.5, 1.0, -1.7)):
        want = master(subs, gains, width)
        assert len(want) == total * width
        for a, b in windows(level, width, total):
            idle = 2 * T <= a and b <= 3 * T
            exp = want[a * width:b * width]
            assert not idle or exp == bytes((b - a) * width), (a, b)
            for out_sample in (0, 1):
                got, front, behind = render_window(N, seq if gains is None else WithGains(seq, gains), width, a, b, out_sample)
                assert got == exp, "gains %s, window [%d, %d) at out_sample %d: %d bytes differ" % (gains, a, b, out_sample, differs(got, exp))
                assert front == b"\x5a" * 64 and behind == b"\x5a" * 64, (gains, a, b, out_sample)
    seq.free()


def test_windows_of_every_level_at_16_bits_under_the_other_alignment_scheme(gpu):
    in_a_child_under_the_other_alignment_scheme(__file__, ["test_windows_of_every_level_through_the_entry_point[%s-2]" % lv for lv in LEVELS])


# ---- 4: run shapes -------------------------------------------------------------------------------------------------------------------------
def test_a_track_with_no_events_at_all(gpu):
    from synthesizer_amd import mixer
    instruments, tracks, subs, total = bus_song(2)
    samples = as_samples(instruments, 2, RATE)
    with mixer.compile_tracks([with_samples(samples, t) for t in (tracks[0], [], tracks[1], tracks[2], [])], RATE, 1) as cs:
        assert cs.ntracks == 5 and cs._seq.tracks() == (5, 6)
        for gains in ((0.5, 123.0, 1.0, -1.7, 0.0), (1.0, 0.0, 1.0, 1.0, -3.0)):
            want = master(subs, (gains[0], gains[2], gains[3]), 2)
            assert bytes(cs.render(gains=gains).view_frame_data()) == want, gains
        assert bytes(cs.stem(1).view_frame_data()) == bytes(2 * total) == bytes(cs.stem(4).view_frame_data())
    with mixer.compile_tracks([[], []], RATE, 1) as cs:         # and a song of nothing
        assert cs.frames == 0 and len(cs.render(gains=(2.0, 3.0))) == 0


def test_runs_of_one_three_four_five_and_nine_events_in_a_plain_16_bit_tile(gpu):
    """k_win_plain16 keeps four records in flight: a run of one batch, of less, of a batch and one, of two and one, in one tile; and the
    same runs in another order, so that each length starts a tile's walk and ends it"""
    from synthesizer_amd import mixer
    rng = np.random.default_rng(41)
    instruments = [(pcm(rng, 2, 300, 0.5), 1), (pcm(rng, 2, 97, 0.9), 1)]
    vols = [None, 0.5, 1.7, -1.0, 0.37]
    k = 0
    tracks = []
    for n in (1, 3, 4, 5, 9):
        tracks.append([_ev(40 + 11 * (k + j), (k + j) % 2, vols[(k + j) % 5]) for j in range(n)])
        k += n
    samples = as_samples(instruments, 2, RATE)
    for order in ((0, 1, 2, 3, 4), (4, 2, 0, 3, 1)):
        dealt = [tracks[i] for i in order]
        subs = subs_of(instruments, dealt, 2, 1)
        with mixer.compile_tracks([with_samples(samples, t) for t in dealt], RATE, 1) as cs:
            assert cs.level == "plain" and cs.info()["ntiles"] == 1 and cs._seq.tracks() == (5, 5)
            for gains in (None, (1.3, -0.5, 1.0, 0.25, 2.0), (0.0, 1.0, 0.0, 1.0, 0.0)):
                want = master(subs, gains, 2)
                assert bytes(cs.render(gains=gains).view_frame_data()) == want, (order, gains)
                assert bytes(cs.render(3, 201, gains=gains).view_frame_data()) == want[6:408], (order, gains)


@pytest.mark.parametrize("width", [2, 4])
def test_thirty_two_tracks_of_one_event_each_on_one_tile(gpu, width):
    from synthesizer_amd import mixer
    rng = np.random.default_rng(43 + width)
    instruments = [(pcm(rng, width, 300, 0.3), 1), (pcm(rng, width, 97, 0.2), 1)]
    tracks = [[_ev(7 * t, t % 2, [None, 0.9, -1.0][t % 3])] for t in range(32)]
    gains = [[1.0, 0.0, 0.5, -1.7, 2.5, 0.999, 0.37, 1.0][t % 8] for t in range(32)]
    subs = subs_of(instruments, tracks, width, 1)
    want = master(subs, gains, width)
    assert saturates(want, width)
    samples = as_samples(instruments, width, RATE)
    with mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, 1, width) as cs:
        assert cs.ntracks == 32 and cs._seq.tracks() == (32, 32)
        assert bytes(cs.render(gains=gains).view_frame_data()) == want
        assert bytes(cs.render().view_frame_data()) == master(subs, None, width)
        assert bytes(cs.stem(31).view_frame_data()) == subs[31] + bytes(len(want) - len(subs[31]))


# ---- 5: one track is the flat list -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", LEVELS)
def test_one_track_is_compile_sequence_of_the_same_list(gpu, level):
    from synthesizer_amd import mixer
    instruments, events, nch, want, total = song(level, 2)
    samples = as_samples(instruments, 2, RATE)
    with mixer.compile_tracks([with_samples(samples, events)], RATE, nch) as one, mixer.compile_sequence(with_samples(samples, events), RATE, nch) as flat:
        assert one.ntracks == 1 and flat.ntracks is None and one.level == flat.level == LEVEL_NAME.get(level, level) and one.frames == flat.frames
        assert bytes(one.render().view_frame_data()) == bytes(flat.render().view_frame_data()) == want
        a, n = 1500 // nch, 333
        assert bytes(one.render(a, n).view_frame_data()) == bytes(flat.render(a, n).view_frame_data()) == want[a * 2 * nch:(a + n) * 2 * nch]


# ---- 6: streaming ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level, width", [("plain", 2), ("balance", 2), ("loop", 3), ("env", 4)])
def test_chunks_with_gains_that_change_between_them(gpu, level, width):
    N = gpu
    from synthesizer_amd import mixer
    instruments, events, nch, _flat, total = song(level, width)
    tracks = [events[0::3], events[1::3], events[2::3]]
    subs = subs_of(instruments, tracks, width, nch)
    samples = as_samples(instruments, width, RATE)
    fb = width * nch
    g1, g2 = (0.5, 1.0, -1.7), (0.999, 0.0, 2.5)
    w1, w2 = master(subs, g1, width), master(subs, g2, width)
    assert w1 != w2
    with mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, nch, width) as cs:
        for c in (100, 1000, TILE[width] // nch):
            parts = list(cs.chunks(c, gains=g1))
            assert [len(p) for p in parts] == [c] * (cs.frames // c) + ([cs.frames % c] if cs.frames % c else [])
            assert b"".join(bytes(p.view_frame_data()) for p in parts) == w1 == bytes(cs.render(gains=g1).view_frame_data()), c
        handle, held = cs._seq.handle.value, cs.info()["device_bytes"]
        c = 700
        out = N.DeviceBuffer(c * fb + 16)
        cs.render_into(out, width, 0, c, gains=g1)              # the warm-up, one sample off the buffer's start
        before = N.debug_counters()
        for k in range(cs.frames // c):                         # a fader moves between two chunks of one handle: nothing recompiled
            want = (w1, w2)[k % 2]
            cs.render_into(out, width, k * c, c, gains=(g1, g2)[k % 2])
            assert out.download_bytes(c * fb, width) == want[k * c * fb:(k + 1) * c * fb], k
        after = N.debug_counters()
        assert all(after[x] == before[x] for x in ("device_allocs", "device_frees")), (before, after)
        assert cs._seq.handle.value == handle and cs.info()["device_bytes"] == held


# ---- 7: refusals -----------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_any_launch(gpu, monkeypatch):
    N = gpu
    from synthesizer_amd import mixer
    instruments, tracks, subs, total = bus_song(2)
    samples = as_samples(instruments, 2, RATE)
    made = []
    real = N.Sequence
    monkeypatch.setattr(N, "Sequence", lambda *a, **k: made.append(a) or real(*a, **k))
    one = with_samples(samples, tracks[0])
    with pytest.raises(ValueError, match="33 tracks, at most 32"):
        mixer.compile_tracks([one] * 33, RATE, 1)
    with pytest.raises(ValueError, match="at least one track"):
        mixer.compile_tracks([], RATE, 1)
    assert made == []
    cs = mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, 1)
    flat = mixer.compile_sequence(one, RATE, 1)
    launched = []
    for c in (cs, flat):
        inner = c._seq.render
        monkeypatch.setattr(c._seq, "render", lambda *a, _inner=inner, **k: launched.append(a) or _inner(*a, **k))
    nan, inf = float("nan"), float("inf")
    for gains in ((1.0, 1.0), (1.0,) * 4, (), (1.0, nan, 1.0), (inf, 1.0, 1.0), (1.0, 1.0, -inf)):
        with pytest.raises(ValueError, match="CompiledSequence"):
            cs.render(gains=gains)
        with pytest.raises(ValueError, match="CompiledSequence"):
            list(cs.chunks(500, gains=gains))
    with pytest.raises(ValueError, match="gains need a song of tracks"):
        flat.render(gains=(1.0,))
    with pytest.raises(ValueError, match="stem needs a song of tracks"):
        flat.stem(0)
    for t in (3, -1):
        with pytest.raises(ValueError, match="outside the song's 3 tracks"):
            cs.stem(t)
    assert launched == []
    assert bytes(cs.stem(2).view_frame_data()) == subs[2] and len(launched) == 1
    cs.close()
    for call in (lambda: cs.render(gains=(1.0, 1.0, 1.0)), lambda: cs.stem(0), lambda: list(cs.chunks(500, gains=(1.0, 1.0, 1.0)))):
        with pytest.raises(ValueError, match="closed"):
            call()
    assert len(launched) == 1
    flat.close()


def test_the_entry_points_refuse_on_the_host_and_leave_out(gpu):
    N = gpu
    L = N.lib()
    instruments, tracks, subs, total = bus_song(2)
    seq, samples = raw_tracks(N, instruments, tracks, 1, 2)
    flat, _s = raw_tracks(N, instruments, tracks, 1, 2)
    flat.free()
    from synthesizer_amd.sample import Sample
    bufs, table, segtab, nbytes = Sample(samplerate=RATE, nchannels=1, samplewidth=2)._compile_events(with_samples(samples, [e for t in tracks for e in t]))
    flat = N.Sequence(bufs, table, segtab, 2, 1, nbytes // 2)
    out = N.DeviceBuffer.from_bytes(b"\x5a" * 4000)
    dbl = lambda *v: (C.c_double * len(v))(*v)                 # noqa: E731
    nan = float("nan")
    for what, args, message in (
        ("too few gains", (seq.handle, 0, 100, out.handle, 0, dbl(1.0, 1.0), 2), b"2 gains for 3 tracks"),
        ("too many gains", (seq.handle, 0, 100, out.handle, 0, dbl(1.0, 1.0, 1.0, 1.0), 4), b"4 gains for 3 tracks"),
        ("a gain that is no number", (seq.handle, 0, 100, out.handle, 0, dbl(1.0, nan, 1.0), 3), b"gain 1 is not finite"),
        ("an infinite gain", (seq.handle, 0, 100, out.handle, 0, dbl(1.0, 1.0, float("inf")), 3), b"gain 2 is not finite"),
        ("a song without tracks", (flat.handle, 0, 100, out.handle, 0, dbl(1.0), 1), b"the song has no tracks"),
        ("NULL gains", (seq.handle, 0, 100, out.handle, 0, None, 3), b"NULL argument"),
        ("a NULL song", (None, 0, 100, out.handle, 0, dbl(1.0, 1.0, 1.0), 3), b"NULL argument"),
        ("a range past the song", (seq.handle, total - 10, 11, out.handle, 0, dbl(1.0, 1.0, 1.0), 3), b"range outside the song"),
        ("a range past out", (seq.handle, 0, 2000, out.handle, 1, dbl(1.0, 1.0, 1.0), 3), b"range outside out"),
    ):
        assert L.sh_seq_render_gains(*args) == N.SH_ERR_INVALID, what
        err = L.sh_last_error()
        assert err.startswith(b"sh_seq_render_gains") and message in err, (what, err)
    assert out.download_bytes(4000) == b"\x5a" * 4000
    # sh_seq_create_tracks: the track count and track_first, in its own name; what sh_seq_create refuses, in front of them
    arr = (C.c_void_p * len(bufs))(*[b.handle for b in bufs])
    u32 = lambda *v: (C.c_uint32 * len(v))(*v)                 # noqa: E731
    n = len(table)

    def create(first, ntracks, width=2, nch=1):
        h = C.c_void_p()
        rc = L.sh_seq_create_tracks(arr, len(bufs), table.ctypes.data, n, first, ntracks, None, 0, width, nch, nbytes // 2, C.byref(h))
        return rc, h, L.sh_last_error()

    for what, first, ntracks, message in (
        ("no track", u32(0), 0, b"at least one track"),
        ("33 tracks", u32(*([0] * 33 + [n])), 33, b"33 tracks, at most 32"),
        ("NULL track_first", None, 3, b"NULL argument"),
        ("a first offset that is not 0", u32(1, 4, 7, n), 3, b"track_first starts at 0 and ends at nevents"),
        ("a last offset that is not nevents", u32(0, 4, 7, n - 1), 3, b"track_first starts at 0 and ends at nevents"),
        ("offsets that decrease", u32(0, 7, 4, n), 3, b"track_first decreases at track 2"),
    ):
        rc, h, err = create(first, ntracks)
        assert rc == N.SH_ERR_INVALID and not h.value and err.startswith(b"sh_seq_create_tracks") and message in err, (what, err)
    rc, h, err = create(u32(0), 0, width=5)                     # sh_seq_create's refusals come first, in its words
    assert rc == N.SH_ERR_INVALID and err == b"sh_seq_create_tracks: width 5 not in {1, 2, 3, 4}"
    rc, h, err = create(u32(0), 0, nch=0)
    assert rc == N.SH_ERR_INVALID and err == b"sh_seq_create_tracks: # of channels should be >= 1"
    rc, h, err = create(u32(0, 4, 7, n), 3)
    assert rc == N.SH_OK and h.value, err
    nt, nr = C.c_uint32(), C.c_uint32()
    assert L.sh_seq_get_tracks(h, C.byref(nt), C.byref(nr)) == N.SH_OK and (nt.value, nr.value) == (3, 6)
    assert L.sh_seq_get_tracks(flat.handle, C.byref(nt), C.byref(nr)) == N.SH_OK and (nt.value, nr.value) == (0, 0)
    assert L.sh_seq_get_tracks(None, C.byref(nt), C.byref(nr)) == N.SH_ERR_INVALID and L.sh_seq_get_tracks(h, None, C.byref(nr)) == N.SH_ERR_INVALID
    # sh_seq_render of a handle with tracks: every gain 1.0, still grouped
    big = N.DeviceBuffer(total * 2)
    assert L.sh_seq_render(h, 0, total, big.handle, 0) == N.SH_OK and big.download_bytes(total * 2) == master(subs, None, 2)
    assert L.sh_seq_destroy(h) == N.SH_OK
    seq.free()
    flat.free()
