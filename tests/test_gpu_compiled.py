"""GPU parity of a compiled song -- mixer.compile_sequence / CompiledSequence / sh_seq_create, sh_seq_render -- against live ``audioop``
on byte slices: a window of the song rendered alone holds the bytes of that slice of the whole song.  The oracle is
tests/seqref.py's ``mix`` (the whole chain, event after event like mix_at), run once per list and SLICED; expected bytes
never come from the product.  Rate 8192, sources of a few hundred frames, as the sibling files have them; a song of four tiles that ends
mid-lane in tile 3 and whose tile 2 no event touches; one list per feature level."""
import audioop
import ctypes as C

import numpy as np
import pytest

from tests.seqcases import (LEVEL_NAME, LEVELS, RATE, _envelope, _ev, as_samples, check_song, compiled_raw, event_table,
                            in_a_child_under_the_other_alignment_scheme, mix_events, named, render_window, seq_create, song, windows, with_samples)
from tests.seqref import TILE, differs, mix, pcm

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("width", [1, 2, 3, 4])
@pytest.mark.parametrize("level", LEVELS)
def test_windows_of_every_level_through_the_entry_point(gpu, level, width):
    N = gpu
    if level == "env" and width == 3:
        from synthesizer_amd import mixer
        instruments, events = song("plain", width)[:2]
        shaped = [events[0][:6] + (_envelope(300),) + events[0][7:]]
        samples = as_samples(instruments, width, RATE)
        with pytest.raises(NotImplementedError, match="3-byte samples"):
            mixer.compile_sequence(with_samples(samples, shaped), RATE, 1, width)
        with pytest.raises(NotImplementedError, match="3-byte samples"):
            mixer.sequence(with_samples(samples, shaped), RATE, 1, width)
        return
    check_song(level, width)
    instruments, events, nch, want, total = song(level, width)
    seq, _samples = compiled_raw(N, level, width)
    info = seq.info()
    assert N.SEQ_LEVELS[info["level"]] == LEVEL_NAME.get(level, level)
    assert info["track_samples"] == total and info["nevents"] == len(events) and info["ntiles"] == 4 and info["active_tiles"] == 3
    for a, b in windows(level, width, total):
        for out_sample in (0, 1, 8):
            got, front, behind = render_window(N, seq, width, a, b, out_sample)
            exp = want[a * width:b * width]
            assert got == exp, "window [%d, %d) at out_sample %d: %d bytes differ" % (a, b, out_sample, differs(got, exp))
            assert front == b"\x5a" * 64 and behind == b"\x5a" * 64, (a, b, out_sample)
    seq.free()


def test_windows_of_every_level_at_16_bits_under_the_other_alignment_scheme(gpu):
    in_a_child_under_the_other_alignment_scheme(__file__, ["test_windows_of_every_level_through_the_entry_point[%s-2]" % lv for lv in LEVELS])


@pytest.mark.parametrize("level, width", [("plain", 2), ("rev", 2), ("downmix", 2), ("balance", 2), ("pan", 1), ("loop", 3), ("env", 4)])
def test_chunks_render_and_the_sequence_they_replace(gpu, level, width):
    from synthesizer_amd import mixer
    instruments, events, nch, want, total = song(level, width)
    samples = as_samples(instruments, width, RATE)
    fb = width * nch
    with mixer.compile_sequence(with_samples(samples, events), RATE, nch, width, name="song") as cs:
        assert cs.level == LEVEL_NAME.get(level, level) and len(cs) == cs.frames == total // nch and cs.duration == cs.frames / RATE
        assert (cs.samplerate, cs.nchannels, cs.samplewidth) == (RATE, nch, width)
        for c in (100, 1000, TILE[width] // nch):
            parts = list(cs.chunks(c))
            assert [len(p) for p in parts] == [c] * (cs.frames // c) + ([cs.frames % c] if cs.frames % c else [])
            assert b"".join(bytes(p.view_frame_data()) for p in parts) == want, c
        whole = mixer.sequence(with_samples(samples, events), RATE, nch, width)
        assert bytes(whole.view_frame_data()) == want
        for a, n in ((0, None), (7, None), (1500 // nch, 333), (cs.frames - 1, 1), (cs.frames, 0), (5, 0)):
            got = cs.render(a, n)
            b = cs.frames if n is None else a + n
            assert got.name == "song" and got.nchannels == nch and got.samplewidth == width and len(got) == b - a
            assert bytes(got.view_frame_data()) == bytes(whole.view_frame_data())[a * fb:b * fb] == want[a * fb:b * fb]
        for a, n in ((-1, None), (0, -1), (cs.frames + 1, None), (cs.frames - 3, 4), (0, cs.frames + 1)):
            with pytest.raises(ValueError, match="CompiledSequence"):
                cs.render(a, n)
    with pytest.raises(ValueError, match="closed"):
        cs.render()


def test_a_song_of_forty_frames_chunk_by_single_frame(gpu):
    from synthesizer_amd import mixer
    rng = np.random.default_rng(77)
    src = [(pcm(rng, 2, 2 * 40, 1.0), 2), (pcm(rng, 2, 2 * 8, 0.6), 2)]
    events = [_ev(0, 0, 1.7), _ev(3, 1, None, speed=0.37, channels=(0.75, -0.25)), _ev(5, 0, -1.0, 30, reverse=True), _ev(15, 1, 1.7)]
    want = mix(b"", named(src, events), 2, RATE, 2)
    assert len(want) == 40 * 4
    cs = mixer.compile_sequence(with_samples(as_samples(src, 2, RATE), events), RATE, 2)
    parts = list(cs.chunks(1))
    assert len(parts) == 40 and all(len(p) == 1 for p in parts)
    assert b"".join(bytes(p.view_frame_data()) for p in parts) == want
    cs.close()
    cs.close()                                              # (twice is once)


def test_the_song_keeps_sounding_as_its_sources_did_when_it_was_compiled(gpu):
    from synthesizer_amd import mixer
    instruments, events, nch, want, total = song("rate", 2)
    samples = as_samples(instruments, 2, RATE)
    cs = mixer.compile_sequence(with_samples(samples, events), RATE, nch, 2)
    samples[0].amplify(0.5)
    samples[1].mix_at(0.0, samples[2])                      # in place, were the buffer not shared
    samples[2].mix_at_many([(0.0, samples[1], 0.5)])
    assert bytes(samples[0].view_frame_data()) == audioop.mul(instruments[0][0], 2, 0.5)
    assert bytes(cs.render().view_frame_data()) == want
    assert bytes(cs.render(100, 3000).view_frame_data()) == want[200:6200]


def test_steady_state_renders_touch_neither_the_driver_nor_the_stream(gpu):
    N = gpu
    from synthesizer_amd import mixer
    instruments, events, nch, want, total = song("downmix", 2)
    cs = mixer.compile_sequence(with_samples(as_samples(instruments, 2, RATE), events), RATE, nch, 2)
    n = 700
    out = N.DeviceBuffer(2 * n + 16)
    cs.render_into(out, 2, 0, n)                            # the warm-up, one sample off the buffer's start
    before = N.debug_counters()
    for k in range(8):
        cs.render_into(out, 2, 611 * k, n)
    after = N.debug_counters()
    assert all(after[c] == before[c] for c in ("device_allocs", "device_frees", "stream_syncs")), (before, after)
    assert out.download_bytes(2 * n, 2) == want[2 * 611 * 7:2 * (611 * 7 + n)]
    with pytest.raises(ValueError, match="byte_offset"):
        cs.render_into(out, 1, 0, n)


def test_render_refuses_on_the_host_and_leaves_out(gpu):
    N = gpu
    L = N.lib()
    seq, samples = compiled_raw(N, "plain", 2)
    total = song("plain", 2)[4]
    out = N.DeviceBuffer.from_bytes(b"\x5a" * 4000)
    src0 = samples[0]._device()
    for what, args, message in (
        ("a range past the song", (seq.handle, total - 10, 11, out.handle, 0), b"range outside the song"),
        ("a start past the song", (seq.handle, total + 1, 0, out.handle, 0), b"range outside the song"),
        ("a range past out", (seq.handle, 0, 2000, out.handle, 1), b"range outside out"),
        ("out_sample past out", (seq.handle, 0, 1, out.handle, 2001), b"range outside out"),
        ("an out that is a source", (seq.handle, 0, 100, src0.handle, 0), b"overlaps a source"),
        ("a NULL song", (None, 0, 10, out.handle, 0), b"NULL argument"),
        ("a NULL out", (seq.handle, 0, 10, None, 0), b"NULL argument"),
    ):
        assert L.sh_seq_render(*args) == N.SH_ERR_INVALID, what
        err = L.sh_last_error()
        assert err.startswith(b"sh_seq_render") and message in err, (what, err)
    assert out.download_bytes(4000) == b"\x5a" * 4000
    assert src0.download_bytes(len(song("plain", 2)[0][0][0])) == song("plain", 2)[0][0][0]
    assert L.sh_seq_render(seq.handle, 5, 0, out.handle, 2000) == N.SH_OK                   # nothing to write: nothing launched
    assert L.sh_seq_render(seq.handle, total, 0, out.handle, 0) == N.SH_OK
    assert out.download_bytes(4000) == b"\x5a" * 4000
    info = N.SeqInfo()
    assert L.sh_seq_get_info(None, C.byref(info)) == N.SH_ERR_INVALID and L.sh_seq_get_info(seq.handle, None) == N.SH_ERR_INVALID
    assert L.sh_seq_destroy(None) == N.SH_OK
    seq.free()


def test_create_refuses_what_the_chan_entry_point_refuses_in_its_words(gpu):
    """one row per family of seq_check_events' refusals, handed to sh_mix_events_chan and to sh_seq_create: the same text under the other name"""
    N = gpu
    s, t = N.DeviceBuffer.from_bytes(bytes(2000)), N.DeviceBuffer.from_bytes(bytes(10000))
    nan = float("nan")
    D, B, R = N.MIX_EVENT_DOWNMIX, N.MIX_EVENT_BALANCE, N.MIX_EVENT_REVERSED
    segs = np.zeros(1, dtype=N.ENV_SEGMENT_DTYPE)
    segs[0] = (100, 0, 0.5, 0.0, 0.0, 0.0, 0, 0)
    down = (100, 200, 300, 300, 0.5, 0.75, -0.25, 0, 8000, 8000, 2, 0, 0, 0, 0, 0, D)
    back = down[:16] + (D | R,)
    bal = (100, 200, 600, 300, 0.5, 0.75, -0.25, 0, 8000, 8000, 2, 0, 0, 0, 0, 0, B)
    looped = (100, 0, 300, 400, 1.0, 0.0, 0.0, 0, 8000, 8000, 1, 0, 0, 0, 5, 50, 0)
    cases = {
        "reserved": (1, down[:13] + (7,) + down[14:]),
        "unknown flags": (1, down[:16] + (D | 8,)),
        "both modes": (1, down[:16] + (D | B,)),
        "a mode on a mono source": (1, down[:10] + (1,) + down[11:]),
        "a balance into a mono song": (1, down[:16] + (B,)),
        "a downmix into a stereo song": (2, bal[:16] + (D,)),
        "a balance on an odd sample": (2, (101,) + bal[1:]),
        "left / right": (1, down[:5] + (nan,) + down[6:]),
        "a downmix beyond 32-bit source coordinates": (1, (2 ** 31 - 32768 - 299,) + down[1:]),
        "factor": (1, down[:4] + (nan,) + down[5:]),
        "no source": (1, down[:7] + (1,) + down[8:]),
        "src_channels": (1, down[:16] + (0,)),
        "sampling rate": (1, down[:8] + (0,) + down[9:]),
        "a mono source on an odd sample of a stereo song": (2, (101, 0, 20, 0, 1.0, 0.5, 0.5, 0, 8000, 8000, 1, 0, 0, 0, 0, 0, 0)),
        "range outside its source": (1, down[:1] + (802,) + down[2:]),
        "a loop on a fraction of a frame": (2, (100, 1, 300, 400, 1.0, 0.0, 0.0, 0, 8000, 8000, 2, 0, 0, 0, 5, 50, 0)),
        "loop outside its source": (1, looped[:14] + (990, 50) + looped[16:]),
        "more samples than the virtual frames hold": (1, looped[:2] + (401,) + looped[3:]),
        "a reversed region beyond its source": (1, back[:3] + (801,) + back[4:]),
        "a resampled event on a fraction of a frame": (2, (100, 1, 300, 400, 1.0, 0.0, 0.0, 0, 8000, 4000, 2, 0, 0, 0, 0, 0, 0)),
        "src_frames outside its source": (1, (100, 0, 30, 1001, 1.0, 0.0, 0.0, 0, 8000, 4000, 1, 0, 0, 0, 0, 0, 0)),
        "more samples than src_frames resample to": (1, (100, 0, 300, 100, 1.0, 0.0, 0.0, 0, 8000, 4000, 1, 0, 0, 0, 0, 0, 0)),
        "too many segments": (1, down[:11] + (0, 1000) + down[13:]),
        "segments outside the table": (1, down[:11] + (1, 1) + down[13:]),
        "a segment beyond the event's samples": (1, down[:2] + (49,) + down[3:11] + (0, 1) + down[13:]),
        "range outside the track": (1, (4800,) + down[1:]),
    }
    for what, (nch, row) in cases.items():
        ok = bal if nch == 2 else down
        table = event_table(N, "chan", [ok, row])
        assert mix_events(N, "chan", [s], table, segs, 2, nch, t, 5000) == N.SH_ERR_INVALID, what
        theirs = N.lib().sh_last_error()
        assert theirs.startswith(b"sh_mix_events_chan: event 1"), (what, theirs)
        rc, h = seq_create(N, [s], table, segs, 2, nch, 5000)
        mine = N.lib().sh_last_error()
        assert rc == N.SH_ERR_INVALID and not h.value, what
        assert mine == theirs.replace(b"sh_mix_events_chan", b"sh_seq_create"), (what, mine, theirs)
    assert t.download_bytes(10000) == bytes(10000)
    # in front of the events: width, channels, NULL; width 3 with segments
    for width, nch, message in ((0, 1, b"width 0"), (5, 1, b"width 5"), (2, 0, b"# of channels")):
        rc, h = seq_create(N, [s], event_table(N, "chan", [down]), None, width, nch, 5000)
        assert rc == N.SH_ERR_INVALID and N.lib().sh_last_error().startswith(b"sh_seq_create") and message in N.lib().sh_last_error()
    assert N.lib().sh_seq_create(None, 0, None, 0, None, 0, 2, 1, 0, None) == N.SH_ERR_INVALID and b"NULL" in N.lib().sh_last_error()
    shaped = down[:11] + (0, 1) + down[13:]
    rc, h = seq_create(N, [s], event_table(N, "chan", [down, shaped]), segs, 3, 1, 5000)
    assert rc == N.SH_ERR_INVALID and N.lib().sh_last_error() == b"sh_seq_create: event 1: width 3: an envelope's fades have no 24-bit form"
    # two faults at once: the one sh_mix_events_chan names is the one named here (width 3 with segments in front of the channel count)
    assert mix_events(N, "chan", [s], event_table(N, "chan", [down, shaped]), segs, 3, 0, t, 3000) == N.SH_ERR_INVALID
    theirs = N.lib().sh_last_error()
    rc, h = seq_create(N, [s], event_table(N, "chan", [down, shaped]), segs, 3, 0, 3000)
    assert rc == N.SH_ERR_INVALID and N.lib().sh_last_error() == theirs.replace(b"sh_mix_events_chan", b"sh_seq_create") and b"width 3" in theirs
    # and what it accepts: the good rows; an empty list is a song of silence
    rc, h = seq_create(N, [s], event_table(N, "chan", [down, back]), None, 2, 1, 5000)
    assert rc == N.SH_OK and h.value, N.lib().sh_last_error()
    assert N.lib().sh_seq_destroy(h) == N.SH_OK
    rc, h = seq_create(N, [s], event_table(N, "chan", []), None, 2, 1, 3000)
    assert rc == N.SH_OK, N.lib().sh_last_error()
    out = N.DeviceBuffer.from_bytes(b"\x5a" * 6000)
    assert N.lib().sh_seq_render(h, 0, 3000, out.handle, 0) == N.SH_OK and out.download_bytes(6000) == bytes(6000)
    assert N.lib().sh_seq_destroy(h) == N.SH_OK
