"""GPU parity of a compiled song -- mixer.compile_sequence / CompiledSequence / sh_seq_create, sh_seq_render -- against live ``audioop``
on byte slices: a window of the song rendered alone holds the bytes of that slice of the whole song.  The oracle is
tests/test_gpu_channels.py's ``oracle`` (the whole chain, event after event like mix_at), run once per list and SLICED; expected bytes
never come from the product.  Rate 8192, sources of a few hundred frames, as the sibling files have them; a song of four tiles that ends
mid-lane in tile 3 and whose tile 2 no event touches; one list per feature level."""
import audioop
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.test_gpu_channels import FACTORS, _chan_table, _mix_events_chan, oracle
from tests.test_gpu_enveloped import _differs
from tests.test_gpu_looped import LANE, LOOPS, RATE, SPEEDS, TILE, _out_frames
from tests.test_gpu_reversed import LENGTHS, as_samples, named, with_samples
from tests.test_gpu_sequence import OTHER_SCHEME, ROOT, _pcm

pytestmark = pytest.mark.gpu

LEVELS = ["plain", "rate", "pan", "env", "loop", "rev", "downmix", "balance"]       # the last two: CHAN into a mono and in a stereo song
LEVEL_NAME = {"downmix": "chan", "balance": "chan"}
HELD = (600, 300, 97)                                       # frames: a loud instrument and two of the siblings' sizes
assert {2.5, 0.37, 1.001, 0.999} <= set(SPEEDS) and {9, 65} <= set(LOOPS) and 65 in LENGTHS


def _nch(level):
    return 2 if level in ("pan", "balance") else 1


def _ev(frame, inst, volume=None, other_frames=None, speed=None, pan=None, envelope=None, loop=None, region=None, reverse=None, channels=None):
    return (frame / RATE, inst, volume, None if other_frames is None else other_frames / RATE, speed, pan, envelope, loop, region, reverse, channels)


def _envelope(out_frames):
    dur = (0.61 * out_frames + 0.37) / RATE                 # the siblings' proportions: attack, decay, a sustain, a release that ends the note
    return (0.113 * dur, 0.171 * dur, 0.5, 0.233 * dur, dur)


def _stage(level, k, width):
    """what stage event k (0: at the song's start, 1: across the pile-up window's start, 2: in tile 3, 3: inside the pile-up) carries"""
    if level == "plain":
        return {}
    if level == "rate":
        return dict(speed=[2.5, 0.37, 1.001, 0.999][k])
    if level == "pan":
        return dict(pan=[0.3, (1.5, 1.2), -1.0, (1.0, 1.0)][k], speed=0.37 if k == 1 else None)
    if level == "env":
        return dict(envelope=_envelope([300, 300, 300, 200][k]))
    if level == "loop":
        return dict(loop=[(230 / RATE, 295 / RATE, 350 / RATE), (5 / RATE, 70 / RATE, 260 / RATE), (1 / RATE, 10 / RATE, 400 / RATE), (0.0, 9 / RATE, 700 / RATE)][k],
                    speed=2.5 if k == 0 else None)
    if level == "rev":
        return dict(reverse=True, region=(12 / RATE, 250 / RATE) if k == 0 else None, loop=(5 / RATE, 70 / RATE, 260 / RATE) if k == 1 else None)
    kw = dict(channels=FACTORS[[0, 4, 6, 5][k]], speed=0.37 if k == 1 else None, reverse=k == 2)
    if width != 3 and k == 1:
        kw["envelope"] = _envelope(_out_frames(HELD[2], int(RATE * 0.37), RATE))
    return kw


_SONGS = {}


def song(level, width):
    """(instruments as (bytes, channels), events, nch, expected bytes of the whole song, total samples), made once"""
    if (level, width) in _SONGS:
        return _SONGS[(level, width)]
    nch = _nch(level)
    T, L = TILE[width], LANE[width]
    F = T // nch
    src_ch = 2 if level in ("downmix", "balance") else 1 if level == "pan" else nch
    rng = np.random.default_rng(100 * LEVELS.index(level) + 10 + width)
    instruments = [(_pcm(rng, width, HELD[0] * src_ch, 1.0), src_ch), (_pcm(rng, width, HELD[1] * src_ch, 0.6), src_ch),
                   (_pcm(rng, width, HELD[2] * src_ch, 0.6), src_ch)]
    rest = {"pan": dict(pan=(1.0, 1.0)), "downmix": dict(channels=(1.0, 1.0))}.get(level, {})      # what every other row needs to be legal
    w0 = (T + 3 * L) // nch                                 # the frame the pile-up window starts on
    tail = (37 * L + 3) // nch                              # frames of tile 3: the song ends mid-lane
    stretched = level in ("rate", "loop", "pan", "rev", "downmix", "balance")
    events = [
        _ev(0, 1, 0.8, **_stage(level, 0, width)),                                          # across samples 3 and L + 1
        _ev(F - 300, 0, 0.5, **rest),                                                       # starts in tile 0, runs through [T - 1, T + 1)
        _ev(w0 - 100, 2 if stretched else 1, None, **_stage(level, 1, width)),              # its stage straddles the pile-up window's start
        _ev(w0 + 10, 0, 1.7, 200, **rest),                                                  # three loud notes on one another
        _ev(w0 + 13, 0, -1.0, 200, **dict(rest, **_stage(level, 3, width))),
        _ev(w0 + 17, 0, 1.7, 200, **rest),
        _ev(3 * F, 1, 1.2, tail, **_stage(level, 2, width)),                                # tile 3, from its first sample on
    ]
    want = oracle(b"", named(instruments, events), width, RATE, nch)
    total = len(want) // width
    _SONGS[(level, width)] = (instruments, events, nch, want, total)
    return _SONGS[(level, width)]


def windows(level, width, total):
    T, L = TILE[width], LANE[width]
    w = [(0, total), (3, total - 5), (T - 1, T + 1), (L + 1, L + 2), (2 * T + 5, 3 * T - 7), (T + 3 * L, 3 * T + L)]
    if level == "balance":
        w.append((T + 3 * L + 1, 3 * T + L))               # an odd first sample in a stereo song: left and right stay where the song has them
    return w


def check_song(level, width):
    """what the list must hold, on the CPU with audioop alone, before the GPU is asked"""
    instruments, events, nch, want, total = song(level, width)
    T, L = TILE[width], LANE[width]
    assert 3 * T < total < 4 * T and total % L != 0, (total, T, L)                          # four tiles, ending mid-lane in tile 3
    assert want[2 * T * width:3 * T * width] == bytes(T * width)                            # tile 2: no event touches it
    lo, hi = T + 3 * L, 3 * T + L                                                           # the pile-up window
    pile = want[lo * width:hi * width]
    assert abs(audioop.max(pile, width)) >= 2 ** (8 * width - 1) - 1, "nothing saturates"
    assert audioop.minmax(pile, width)[1] == 2 ** (8 * width - 1) - 1 or audioop.minmax(pile, width)[0] == -2 ** (8 * width - 1)
    back = oracle(b"", named(instruments, events[::-1]), width, RATE, nch)
    assert len(back) == len(want) and back[lo * width:hi * width] != pile, "list order does not matter"
    for a, b in windows(level, width, total):
        idle = 2 * T <= a and b <= 3 * T
        assert (want[a * width:b * width] == bytes((b - a) * width)) == idle, (a, b)


def compiled_raw(N, level, width):
    """the song through the C entry point: the product's packer makes the table (an input), N.Sequence is sh_seq_create's thin wrapper"""
    from synthesizer_amd.sample import Sample
    instruments, events, nch, want, total = song(level, width)
    samples = as_samples(instruments, width)
    track = Sample(samplerate=RATE, nchannels=nch, samplewidth=width)
    bufs, table, segtab, nbytes = track._compile_events(with_samples(samples, events))
    assert nbytes == len(want)
    return N.Sequence(bufs, table, segtab, width, nch, total), samples


def render_window(N, seq, width, a, b, out_sample):
    """(the rendered bytes, the 64 bytes in front of them, the 64 behind) of a window rendered into a 0x5A-filled buffer"""
    n = b - a
    inner = (out_sample + n) * width
    parent = N.DeviceBuffer.from_bytes(b"\x5a" * (64 + inner + 64))
    out = parent.view(64, inner)
    seq.render(a, n, out, out_sample)
    got = parent.download_bytes(64 + inner + 64)
    at = 64 + out_sample * width
    return got[at:at + n * width], got[at - 64:at], got[at + n * width:]


@pytest.mark.parametrize("width", [1, 2, 3, 4])
@pytest.mark.parametrize("level", LEVELS)
def test_windows_of_every_level_through_the_entry_point(gpu, level, width):
    N = gpu
    if level == "env" and width == 3:
        from synthesizer_amd import mixer
        instruments, events = song("plain", width)[:2]
        shaped = [events[0][:6] + (_envelope(300),) + events[0][7:]]
        samples = as_samples(instruments, width)
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
            assert got == exp, "window [%d, %d) at out_sample %d: %d bytes differ" % (a, b, out_sample, _differs(got, exp))
            assert front == b"\x5a" * 64 and behind == b"\x5a" * 64, (a, b, out_sample)
    seq.free()


def in_a_child_under_the_other_alignment_scheme(path, ids):
    """SYNTHHIP_SEQ_ALIGN is read once per process (sh_init): the named cases of the file again, in a fresh child under the scheme that is
    not the default"""
    env = dict(os.environ, SYNTHHIP_SEQ_ALIGN=OTHER_SCHEME)
    me = str(Path(path).resolve())
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider"] + [me + "::" + i for i in ids],
                       cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "%d passed" % len(ids) in p.stdout and "failed" not in p.stdout, p.stdout[-3000:] + p.stderr[-1000:]


def test_windows_of_every_level_at_16_bits_under_the_other_alignment_scheme(gpu):
    in_a_child_under_the_other_alignment_scheme(__file__, ["test_windows_of_every_level_through_the_entry_point[%s-2]" % lv for lv in LEVELS])


@pytest.mark.parametrize("level, width", [("plain", 2), ("rev", 2), ("downmix", 2), ("balance", 2), ("pan", 1), ("loop", 3), ("env", 4)])
def test_chunks_render_and_the_sequence_they_replace(gpu, level, width):
    from synthesizer_amd import mixer
    instruments, events, nch, want, total = song(level, width)
    samples = as_samples(instruments, width)
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
    src = [(_pcm(rng, 2, 2 * 40, 1.0), 2), (_pcm(rng, 2, 2 * 8, 0.6), 2)]
    events = [_ev(0, 0, 1.7), _ev(3, 1, None, speed=0.37, channels=(0.75, -0.25)), _ev(5, 0, -1.0, 30, reverse=True), _ev(15, 1, 1.7)]
    want = oracle(b"", named(src, events), 2, RATE, 2)
    assert len(want) == 40 * 4
    cs = mixer.compile_sequence(with_samples(as_samples(src, 2), events), RATE, 2)
    parts = list(cs.chunks(1))
    assert len(parts) == 40 and all(len(p) == 1 for p in parts)
    assert b"".join(bytes(p.view_frame_data()) for p in parts) == want
    cs.close()
    cs.close()                                              # (twice is once)


def test_the_song_keeps_sounding_as_its_sources_did_when_it_was_compiled(gpu):
    from synthesizer_amd import mixer
    instruments, events, nch, want, total = song("rate", 2)
    samples = as_samples(instruments, 2)
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
    cs = mixer.compile_sequence(with_samples(as_samples(instruments, 2), events), RATE, nch, 2)
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


def _seq_create(N, srcs, events, segments, width, nchannels, track_samples):
    arr = (C.c_void_p * max(1, len(srcs)))(*[b.handle for b in srcs])
    h = C.c_void_p()
    rc = N.lib().sh_seq_create(arr, len(srcs), events.ctypes.data if len(events) else None, len(events),
                               segments.ctypes.data if segments is not None and len(segments) else None,
                               len(segments) if segments is not None else 0, width, nchannels, track_samples, C.byref(h))
    return rc, h


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
        table = _chan_table(N, [ok, row])
        assert _mix_events_chan(N, [s], table, segs, 2, nch, t, 5000) == N.SH_ERR_INVALID, what
        theirs = N.lib().sh_last_error()
        assert theirs.startswith(b"sh_mix_events_chan: event 1"), (what, theirs)
        rc, h = _seq_create(N, [s], table, segs, 2, nch, 5000)
        mine = N.lib().sh_last_error()
        assert rc == N.SH_ERR_INVALID and not h.value, what
        assert mine == theirs.replace(b"sh_mix_events_chan", b"sh_seq_create"), (what, mine, theirs)
    assert t.download_bytes(10000) == bytes(10000)
    # in front of the events: width, channels, NULL; width 3 with segments
    for width, nch, message in ((0, 1, b"width 0"), (5, 1, b"width 5"), (2, 0, b"# of channels")):
        rc, h = _seq_create(N, [s], _chan_table(N, [down]), None, width, nch, 5000)
        assert rc == N.SH_ERR_INVALID and N.lib().sh_last_error().startswith(b"sh_seq_create") and message in N.lib().sh_last_error()
    assert N.lib().sh_seq_create(None, 0, None, 0, None, 0, 2, 1, 0, None) == N.SH_ERR_INVALID and b"NULL" in N.lib().sh_last_error()
    shaped = down[:11] + (0, 1) + down[13:]
    rc, h = _seq_create(N, [s], _chan_table(N, [down, shaped]), segs, 3, 1, 5000)
    assert rc == N.SH_ERR_INVALID and N.lib().sh_last_error() == b"sh_seq_create: event 1: width 3: an envelope's fades have no 24-bit form"
    # two faults at once: the one sh_mix_events_chan names is the one named here (width 3 with segments in front of the channel count)
    assert _mix_events_chan(N, [s], _chan_table(N, [down, shaped]), segs, 3, 0, t, 3000) == N.SH_ERR_INVALID
    theirs = N.lib().sh_last_error()
    rc, h = _seq_create(N, [s], _chan_table(N, [down, shaped]), segs, 3, 0, 3000)
    assert rc == N.SH_ERR_INVALID and N.lib().sh_last_error() == theirs.replace(b"sh_mix_events_chan", b"sh_seq_create") and b"width 3" in theirs
    # and what it accepts: the good rows; an empty list is a song of silence
    rc, h = _seq_create(N, [s], _chan_table(N, [down, back]), None, 2, 1, 5000)
    assert rc == N.SH_OK and h.value, N.lib().sh_last_error()
    assert N.lib().sh_seq_destroy(h) == N.SH_OK
    rc, h = _seq_create(N, [s], _chan_table(N, []), None, 2, 1, 3000)
    assert rc == N.SH_OK, N.lib().sh_last_error()
    out = N.DeviceBuffer.from_bytes(b"\x5a" * 6000)
    assert N.lib().sh_seq_render(h, 0, 3000, out.handle, 0) == N.SH_OK and out.download_bytes(6000) == bytes(6000)
    assert N.lib().sh_seq_destroy(h) == N.SH_OK
