"""What a sustain loop per event in Sample.mix_at_many needs of the host alone (no GPU): sh_mix_event_loop as the header lays it out
against the numpy dtype the binding packs, the ValueErrors raised before the library is even loaded, and which entry point a list goes
to with which table -- a list without a loop where it went before, with the same table bytes."""
import ctypes as C

import numpy as np
import pytest

from synthesizer_amd import _native as N
from synthesizer_amd.sample import Sample
from tests.songhost import RATE, _mono, _stereo
from tests.test_enveloped_host import EVENT_FIELDS, _fake_library, _layout, _Lib, _no_library

LOOP_FIELDS = EVENT_FIELDS + ["loop_start", "loop_frames"]
nan, inf = float("nan"), float("inf")


def test_the_struct_matches_the_header(tmp_path):
    D = N.MIX_EVENT_LOOP_DTYPE
    assert _layout(tmp_path, "sh_mix_event_loop", LOOP_FIELDS) == [D.itemsize] + [D.fields[f][1] for f in LOOP_FIELDS] \
        == [104, 0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 68, 72, 76, 80, 88, 96]
    assert D.names == tuple(LOOP_FIELDS)
    E = N.MIX_EVENT_ENV_DTYPE                               # sh_mix_event_env's fields where that struct has them
    assert all(D.fields[f] == E.fields[f] for f in E.names)


@pytest.mark.parametrize("what, loop", [
    ("two numbers", (0.01, 0.02)),
    ("four numbers", (0.01, 0.02, 0.5, 0.1)),
    ("none", ()),
    ("a number", 0.5),
    ("a string", "abc"),
    ("a negative loop_start", (-0.01, 0.02, 0.5)),
    ("a negative loop_end", (0.0, -0.02, 0.5)),
    ("a negative length", (0.01, 0.02, -0.5)),
    ("a loop_start that is no number", (nan, 0.02, 0.5)),
    ("an infinite loop_end", (0.01, inf, 0.5)),
    ("a length that is no number", (0.01, 0.02, nan)),
    ("an infinite length", (0.01, 0.02, inf)),
    ("an empty loop", (0.02, 0.02, 0.5)),
    ("a loop that ends before it starts", (0.03, 0.02, 0.5)),
    ("a loop of less than a frame", (0.0100, 0.0101, 0.5)),                       # frames 80 .. 80
    ("a loop behind the sample", (0.5, 0.9, 1.0)),                                # the track's 4000 frames: S = 4000 = E after the clamp
    ("a loop far behind the sample", (0.7, 0.8, 0.9)),
    ("a note beyond what one call addresses", (0.01, 0.02, 2.0 ** 32 / RATE)),
])
def test_mix_at_many_refuses_before_the_library_is_loaded(monkeypatch, what, loop):
    _no_library(monkeypatch)
    track = _stereo(4000)
    for other, pan in ((_stereo(), None), (_mono(), 0.5)):
        with pytest.raises(ValueError, match="mix_at_many: loop"):
            track.mix_at_many([(0.0, _stereo(), 0.5, None, 1.5, None, None, (0.01, 0.02, 0.3)), (0.1, other, None, None, None, pan, None, loop)])
    with pytest.raises(ValueError, match="mix_at_many: loop"):
        track.mix_at_many([(0.1, track, None, None, None, None, None, loop)])   # the track itself: checked with the rest, before anything is mixed
    assert len(track) == 4000 and bytes(track.view_frame_data()) == bytes(16000)


def test_the_addressable_length_counts_samples_not_frames(monkeypatch):
    _no_library(monkeypatch)
    frames = 0xFFFF0000 // 2 + 1                                                  # fits a mono note, not a stereo one
    with pytest.raises(ValueError, match="mix_at_many: loop"):
        _stereo(4000).mix_at_many([(0.0, _stereo(), None, 0.01, None, None, None, (0.01, 0.02, (frames + 0.5) / RATE))])


def test_an_envelope_is_checked_against_the_looped_length(monkeypatch):
    _no_library(monkeypatch)
    track = _mono(8000)
    env = (0.05, 0.05, 0.5, 0.1)                            # needs 0.2 s: the 1000 frames (0.125 s) do not have them, a note looped to 0.5 s has
    with pytest.raises(ValueError, match="mix_at_many: envelope"):
        track.mix_at_many([(0.1, _mono(), None, None, None, None, env)])
    with pytest.raises(ValueError, match="mix_at_many: envelope"):
        track.mix_at_many([(0.1, _mono(), None, None, None, None, env, (0.05, 0.1, 0.15))])
    lib = _fake_library(monkeypatch)
    track.mix_at_many([(0.1, _mono(), None, None, None, None, env, (0.05, 0.1, 0.5))])
    assert [c for c in lib.calls if c.startswith("sh_mix_events")] == ["sh_mix_events_loop"]


class _LoopLib(_Lib):
    """_Lib, which also keeps what sh_mix_events_loop was handed"""
    DTYPES = dict(_Lib.DTYPES, sh_mix_events_loop="MIX_EVENT_LOOP_DTYPE")

    def __getattr__(self, name):
        call = _Lib.__getattr__(self, name)
        if name != "sh_mix_events_loop":
            return call

        def loop_call(*args):
            raw = (C.c_char * (args[5] * N.ENV_SEGMENT_DTYPE.itemsize)).from_address(args[4]) if args[5] else b""
            self.segments.append(np.frombuffer(bytes(raw), dtype=N.ENV_SEGMENT_DTYPE))
            return call(*args)
        return loop_call


def _fake(monkeypatch):
    from tests.test_enveloped_host import _Buf
    lib = _LoopLib()
    monkeypatch.setattr(N, "lib", lambda: lib)
    monkeypatch.setattr(N, "DeviceBuffer", _Buf)
    return lib


def test_a_list_without_a_loop_goes_where_it_went_with_the_same_table(monkeypatch):
    lib = _fake(monkeypatch)
    m, s = _mono(100), _stereo(70)
    env = (0.001, 0.001, 0.5, 0.001)
    lists = [[(0.01, s, 0.5), (0.02, s, None, 0.001)],
             [(0.01, s, 0.5), (0.02, s, None, None, 1.5)],
             [(0.01, m, 0.5, None, None, 0.5), (0.02, s, None, None, 1.5)],
             [(0.01, m, 0.5, None, None, 0.5, env), (0.02, s, None, None, 1.5)]]
    for lst in lists:
        _stereo(4000).mix_at_many(lst)
    names = ["sh_mix_events", "sh_mix_events_rate", "sh_mix_events_pan", "sh_mix_events_env"]
    assert [c for c in lib.calls if c.startswith("sh_mix_events")] == names
    short = [t.tobytes() for t in lib.tables]
    del lib.calls[:], lib.tables[:]
    for lst in lists:                                       # the eighth element, when it is None, changes nothing
        _stereo(4000).mix_at_many([tuple(e) + (None,) * (8 - len(e)) for e in lst])
    assert [c for c in lib.calls if c.startswith("sh_mix_events")] == names
    assert [t.tobytes() for t in lib.tables] == short
    assert [t.dtype for t in lib.tables] == [N.MIX_EVENT_DTYPE, N.MIX_EVENT_RATE_DTYPE, N.MIX_EVENT_PAN_DTYPE, N.MIX_EVENT_ENV_DTYPE]


def test_a_list_with_a_loop_is_one_table_of_loop_rows(monkeypatch):
    lib = _fake(monkeypatch)
    m, s = _mono(1000), _stereo(800)
    track = _stereo(4000)
    track.mix_at_many([
        (0.01, m, 0.5, None, None, 0.5, None, (0.05, 0.1, 0.3)),                  # frames 400 .. 800 looped to 2400 mono frames
        (0.02, s, None, None, 2.0),                                              # no loop: loop_frames 0, the source's own frames
        (0.03, s, None, None, 2.0, None, None, (0.01, 0.5, 0.25)),                # loop_end clamped to the 800 frames; 2000 virtual frames at speed 2
        (0.04, s, None, 0.05, None, None, (0.01, 0.0, 0.25, 0.01, 0.2), (0.0, 0.05, 1.0)),   # 8000 virtual frames, the envelope cuts at 1600, other_seconds at 400
        (0.05, m, None, None, None, (0.0, 1.25), None, (0.0, 0.1, 0.05)),         # V = 400 <= E = 800: a plain cut, still a loop row
    ])
    assert [c for c in lib.calls if c.startswith("sh_mix_events")] == ["sh_mix_events_loop"]          # one batch, one launch
    (t,) = lib.tables
    assert t.dtype == N.MIX_EVENT_LOOP_DTYPE and len(t) == 5
    assert t["loop_start"].tolist() == [400, 0, 80, 0, 0] and t["loop_frames"].tolist() == [400, 0, 720, 400, 800]
    assert t["src_frames"].tolist() == [2400, 800, 2000, 8000, 400]
    assert t["src_channels"].tolist() == [1, 2, 2, 2, 1] and t["src"].tolist() == [0, 1, 1, 1, 0]
    assert t["dst_sample"].tolist() == [160, 320, 480, 640, 800]
    assert t["nsamples"].tolist() == [4800, 800, 2 * ((2000 - 1) * RATE // (2 * RATE) + 1), 800, 800]
    assert t["inrate"].tolist() == [RATE, 2 * RATE, 2 * RATE, RATE, RATE]
    assert t["seg_count"].tolist() == [0, 0, 0, 2, 0] and not t["reserved"].any()
    (g,) = lib.segments                                     # the envelope saw the 1600 frames its length leaves of the 8000 virtual ones
    assert g["end"].tolist() == [160, 800] and g["kind"].tolist() == [N.ENV_FADE_IN, N.ENV_NONE] and g["mul"].tolist() == [1.0, 0.25]


def test_24_bit_samples_may_loop_but_have_no_envelope(monkeypatch):
    lib = _fake(monkeypatch)
    track = _stereo(4000, 3)
    track.mix_at_many([(0.1, _stereo(1000, 3), None, None, 1.5, None, None, (0.05, 0.1, 0.3))])
    assert [c for c in lib.calls if c.startswith("sh_mix_events")] == ["sh_mix_events_loop"]
    with pytest.raises(NotImplementedError):
        _stereo(4000, 3).mix_at_many([(0.1, _stereo(1000, 3), None, None, None, None, (0.01, 0.01, 0.5, 0.01), (0.05, 0.1, 0.3))])
