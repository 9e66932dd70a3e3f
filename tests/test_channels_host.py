"""What ``channels`` per event in Sample.mix_at_many -- a stereo sample downmixed into a mono track or balanced in a stereo one -- needs of
the host alone (no GPU): sh_mix_event_chan as the header lays it out against the numpy dtype the binding packs, the ValueErrors raised
before the library is even loaded, which entry point a list goes to with which table (no ``channels``: where it went, byte for byte), and
the packed rows of a downmix and of a balance, alone and with region + reverse + loop + speed + envelope."""
import ctypes as C

import numpy as np
import pytest

from synthesizer_amd import _native as N
from synthesizer_amd.sample import Sample
from tests.songhost import RATE, _fake, _mono, _stereo
from tests.test_enveloped_host import _layout, _no_library
from tests.test_reversed_host import REV_FIELDS, _RevLib

nan, inf = float("nan"), float("inf")


class _ChanLib(_RevLib):
    """_RevLib, which also keeps what sh_mix_events_chan was handed"""
    DTYPES = dict(_RevLib.DTYPES, sh_mix_events_chan="MIX_EVENT_CHAN_DTYPE")

    def __getattr__(self, name):
        call = _RevLib.__getattr__(self, name)
        if name != "sh_mix_events_chan":
            return call

        def chan_call(*args):
            raw = (C.c_char * (args[5] * N.ENV_SEGMENT_DTYPE.itemsize)).from_address(args[4]) if args[5] else b""
            self.segments.append(np.frombuffer(bytes(raw), dtype=N.ENV_SEGMENT_DTYPE))
            self.args = args[6:8]                           # width, nchannels
            return call(*args)
        return chan_call


def _entries(lib):
    return [c for c in lib.calls if c.startswith("sh_mix_events")]


def _ev(seconds, other, channels, volume=None, other_seconds=None, speed=None, envelope=None, loop=None, region=None, reverse=None, pan=None):
    return (seconds, other, volume, other_seconds, speed, pan, envelope, loop, region, reverse, channels)


def test_the_struct_matches_the_header(tmp_path):
    D = N.MIX_EVENT_CHAN_DTYPE
    assert _layout(tmp_path, "sh_mix_event_chan", REV_FIELDS) == [D.itemsize] + [D.fields[f][1] for f in REV_FIELDS] \
        == [112, 0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 68, 72, 76, 80, 88, 96, 104]
    assert D.names == tuple(REV_FIELDS)
    R = N.MIX_EVENT_REV_DTYPE                               # sh_mix_event_rev's layout
    assert all(D.fields[f] == R.fields[f] for f in R.names)
    assert (N.MIX_EVENT_REVERSED, N.MIX_EVENT_DOWNMIX, N.MIX_EVENT_BALANCE) == (1, 2, 4)
    assert _layout(tmp_path, "sh_mix_event_rev", REV_FIELDS) == _layout(tmp_path, "sh_mix_event_chan", REV_FIELDS)


@pytest.mark.parametrize("what, track, event", [
    ("one number", _mono, lambda: _ev(0.1, _stereo(), (0.5,))),
    ("three numbers", _stereo, lambda: _ev(0.1, _stereo(), [0.5, 0.5, 0.5])),
    ("a number", _mono, lambda: _ev(0.1, _stereo(), 0.5)),
    ("a string", _mono, lambda: _ev(0.1, _stereo(), "ab")),
    ("a pair of strings", _mono, lambda: _ev(0.1, _stereo(), ("a", "b"))),
    ("a pair with None", _stereo, lambda: _ev(0.1, _stereo(), (None, 1))),
    ("a factor that is no number", _mono, lambda: _ev(0.1, _stereo(), (nan, 0.5))),
    ("an infinite factor", _stereo, lambda: _ev(0.1, _stereo(), (0.5, -inf))),
    ("a mono other into a mono track", _mono, lambda: _ev(0.1, _mono(), (0.5, 0.5))),
    ("a mono other into a stereo track", _stereo, lambda: _ev(0.1, _mono(), (0.5, 0.5))),
    ("pan and channels on a stereo other", _stereo, lambda: _ev(0.1, _stereo(), (0.5, 0.5), pan=0.3)),
    ("pan and channels on a mono other", _stereo, lambda: _ev(0.1, _mono(), (0.5, 0.5), pan=(1.0, 0.0))),
    ("pan and channels into a mono track", _mono, lambda: _ev(0.1, _stereo(), (0.5, 0.5), pan=0.0)),
])
def test_mix_at_many_refuses_before_the_library_is_loaded(monkeypatch, what, track, event):
    _no_library(monkeypatch)
    t = track(4000)
    before = bytes(t.view_frame_data())
    good = _ev(0.0, _stereo(), (0.5, 0.25), 0.5, None, 1.5)
    with pytest.raises(ValueError, match="mix_at_many"):
        t.mix_at_many([good, event()])                      # raised with the other checks: nothing was mixed before
    assert len(t) == 4000 and bytes(t.view_frame_data()) == before


def test_mix_at_many_refuses_a_track_that_is_neither_mono_nor_stereo(monkeypatch):
    _no_library(monkeypatch)
    four = Sample.from_raw_frames(bytes(8 * 100), 2, RATE, 4)
    with pytest.raises(ValueError, match="mix_at_many: channels"):
        four.mix_at_many([_ev(0.1, _stereo(), (1.0, 1.0))])
    assert len(four) == 100


def test_a_downmix_the_kernels_cannot_address_is_refused(monkeypatch):
    """2 * (dst_sample + nsamples) in 32 bits: the last event that fits ends 2^31 - 32768 samples in"""
    _no_library(monkeypatch)
    rate = 2 ** 20
    limit = 2 ** 31 - 32768
    t = Sample.from_raw_frames(b"", 1, rate, 1)
    s = Sample.from_raw_frames(bytes(2 * 100), 1, rate, 2)
    with pytest.raises(ValueError, match="mix_at_many: channels"):
        t.mix_at_many([_ev((limit - 99) / rate, s, (0.5, 0.5))])
    assert len(t) == 0
    lib = _fake(monkeypatch)                                # one frame earlier it is the last event that fits: it ends at the limit
    Sample.from_raw_frames(b"", 1, rate, 1).mix_at_many([_ev((limit - 100) / rate, s, (0.5, 0.5))])
    assert _entries(lib) == ["sh_mix_events_chan"]
    assert int(lib.tables[0]["dst_sample"][0]) + int(lib.tables[0]["nsamples"][0]) == limit


def test_a_balance_beyond_the_downmix_limit_is_an_event_like_any_other(monkeypatch):
    """the limit is the downmix's alone: a balance reads one source sample per track sample, so a stereo track takes one that ends
    beyond 2^31 - 32768 samples (here 2^31 + 4096 samples in) as it takes a plain stereo event there"""
    lib = _fake(monkeypatch)
    rate = 2 ** 20
    s = Sample.from_raw_frames(bytes(2 * 100), 1, rate, 2)
    first = 2 ** 30 + 2048 - 100                            # the event's first FRAME; it ends at frame 2^30 + 2048
    Sample.from_raw_frames(b"", 1, rate, 2).mix_at_many([_ev(first / rate, s, (0.5, 0.25))])
    assert _entries(lib) == ["sh_mix_events_chan"]
    (t,) = lib.tables
    assert t["flags"].tolist() == [N.MIX_EVENT_BALANCE] and t["dst_sample"].tolist() == [2 * first] and t["nsamples"].tolist() == [200]
    assert int(t["dst_sample"][0]) + int(t["nsamples"][0]) == 2 ** 31 + 4096 > 2 ** 31 - 32768


def test_without_channels_the_old_assertion_and_the_old_routes_stand(monkeypatch):
    _no_library(monkeypatch)
    with pytest.raises(AssertionError):
        _mono(4000).mix_at_many([(0.1, _stereo())])         # a stereo other in a mono track: mix_at's assertion, as before
    with pytest.raises(AssertionError):
        _mono(4000).mix_at_many([_ev(0.1, _stereo(), None)])
    with pytest.raises(ValueError, match="mix_at_many: pan needs a mono sample"):
        _stereo(4000).mix_at_many([_ev(0.1, _stereo(), None, pan=0.5)])
    lib = _fake(monkeypatch)
    m, s = _mono(1000), _stereo(800)
    env = (0.001, 0.001, 0.5, 0.001)
    lists = [[(0.01, s, 0.5), (0.02, s, None, 0.001)],
             [(0.01, s, 0.5), (0.02, s, None, None, 1.5)],
             [(0.01, m, 0.5, None, None, 0.5), (0.02, s, None, None, 1.5)],
             [(0.01, m, 0.5, None, None, 0.5, env), (0.02, s, None, None, 1.5)],
             [(0.01, m, 0.5, None, None, 0.5, env, (0.05, 0.1, 0.3)), (0.02, s, None, None, 1.5)],
             [(0.01, m, 0.5, None, None, 0.5, env, (0.05, 0.1, 0.3), (0.01, 0.1), True), (0.02, s, None, None, 1.5)]]
    names = ["sh_mix_events", "sh_mix_events_rate", "sh_mix_events_pan", "sh_mix_events_env", "sh_mix_events_loop", "sh_mix_events_rev"]
    for lst in lists:
        _stereo(4000).mix_at_many(lst)
    assert _entries(lib) == names
    short = [t.tobytes() for t in lib.tables]
    del lib.calls[:], lib.tables[:]
    for lst in lists:                                       # the eleventh element said as None: the same tables at the same entry points
        _stereo(4000).mix_at_many([tuple(e) + (None,) * (11 - len(e)) for e in lst])
    assert _entries(lib) == names
    assert [t.tobytes() for t in lib.tables] == short
    assert [t.dtype for t in lib.tables] == [N.MIX_EVENT_DTYPE, N.MIX_EVENT_RATE_DTYPE, N.MIX_EVENT_PAN_DTYPE, N.MIX_EVENT_ENV_DTYPE,
                                             N.MIX_EVENT_LOOP_DTYPE, N.MIX_EVENT_REV_DTYPE]


def test_a_plain_downmix_row(monkeypatch):
    lib = _fake(monkeypatch)
    s, m = _stereo(800), _mono(300)
    track = _mono(1000)
    track.mix_at_many([(0.01, m, 0.5), _ev(0.02, s, (0.75, -0.25)), _ev(0.03, s, [1, 0], -1.0, 0.05)])
    assert _entries(lib) == ["sh_mix_events_chan"] and lib.args == (2, 1)          # one batch, one launch, a mono track
    (t,) = lib.tables
    assert t.dtype == N.MIX_EVENT_CHAN_DTYPE and len(t) == 3
    assert t["flags"].tolist() == [0, N.MIX_EVENT_DOWNMIX, N.MIX_EVENT_DOWNMIX]
    assert t["left"].tolist() == [0.0, 0.75, 1.0] and t["right"].tolist() == [0.0, -0.25, 0.0]
    assert t["src_channels"].tolist() == [1, 2, 2] and t["src"].tolist() == [0, 1, 1]
    assert t["dst_sample"].tolist() == [80, 160, 240]                                # mono track samples
    assert t["nsamples"].tolist() == [300, 800, 400]                                 # MONO samples: a stereo frame each; other_seconds cuts 400
    assert t["src_frames"].tolist() == [300, 800, 800] and t["factor"].tolist() == [0.5, 1.0, -1.0]
    assert not t["src_sample"].any() and not t["loop_frames"].any() and not t["seg_count"].any() and not t["reserved"].any()
    assert len(track) == 1000


def test_a_plain_balance_row(monkeypatch):
    lib = _fake(monkeypatch)
    s, m = _stereo(800), _mono(300)
    track = _stereo(100)
    track.mix_at_many([(0.01, m, 0.5, None, None, 0.5), _ev(0.02, s, (0.75, -0.25)), (0.03, s), _ev(0.03, s, (1.0, 1.0), None, 0.05)])
    assert _entries(lib) == ["sh_mix_events_chan"] and lib.args == (2, 2)
    (t,) = lib.tables
    assert t["flags"].tolist() == [0, N.MIX_EVENT_BALANCE, 0, N.MIX_EVENT_BALANCE]
    assert t["left"].tolist() == [0.25, 0.75, 0.0, 1.0] and t["right"].tolist() == [0.75, -0.25, 0.0, 1.0]      # a pan row keeps tostereo's
    assert t["src_channels"].tolist() == [1, 2, 2, 2]
    assert t["dst_sample"].tolist() == [160, 320, 480, 480] and t["nsamples"].tolist() == [600, 1600, 1600, 800]    # stereo samples
    assert len(track) == 240 + 800


def test_a_downmix_and_a_balance_with_region_reverse_loop_speed_and_envelope(monkeypatch):
    lib = _fake(monkeypatch)
    s = _stereo(1000)
    # region frames 400 .. 800, reversed; loop played frames 160 .. 240 held for 0.3 s = 2400 frames; twice as fast: 1200 frames; an
    # envelope with a length of 0.1 s = 800 frames, of which other_seconds takes 0.05 s = 400
    shaped = dict(volume=0.5, other_seconds=0.05, speed=2.0, envelope=(0.01, 0.0, 0.25, 0.01, 0.1), loop=(0.02, 0.03, 0.3), region=(0.05, 0.1),
                  reverse=True)
    rows = {}
    for nch, track in ((1, _mono(4000)), (2, _stereo(4000))):
        del lib.calls[:], lib.tables[:], lib.segments[:]
        track.mix_at_many([_ev(0.04, s, (0.75, -0.25), **shaped)])
        assert _entries(lib) == ["sh_mix_events_chan"] and lib.args == (2, nch)
        (t,), (g,) = lib.tables, lib.segments
        rows[nch] = (t, g)
        assert t["flags"].tolist() == [N.MIX_EVENT_REVERSED | (N.MIX_EVENT_DOWNMIX if nch == 1 else N.MIX_EVENT_BALANCE)]
        assert t["left"].tolist() == [0.75] and t["right"].tolist() == [-0.25] and t["factor"].tolist() == [0.5]
        assert t["src_channels"].tolist() == [2] and t["inrate"].tolist() == [2 * RATE] and t["outrate"].tolist() == [RATE]
        # in stereo frames / samples, as for any stereo source: the loop_end frames at the region's END, as stored
        assert t["src_sample"].tolist() == [2 * (400 + (400 - 240))]
        assert t["loop_start"].tolist() == [160] and t["loop_frames"].tolist() == [80] and t["src_frames"].tolist() == [2400]
        assert t["dst_sample"].tolist() == [320 * nch] and t["nsamples"].tolist() == [400 * nch]     # TRACK samples: mono for the downmix
        assert t["seg_first"].tolist() == [0] and t["seg_count"].tolist() == [len(g)]
        # the envelope over the source's 1600 stereo samples (800 frames), cut where other_seconds cuts: 800 stereo samples either way
        assert g["end"].tolist() == [160, 800] and g["kind"].tolist() == [N.ENV_FADE_IN, N.ENV_NONE] and g["mul"].tolist() == [1.0, 0.25]
    assert rows[1][1].tobytes() == rows[2][1].tobytes()     # the same segments: they count the stereo source's samples


def test_24_bit_samples_may_be_downmixed_but_have_no_envelope(monkeypatch):
    lib = _fake(monkeypatch)
    _mono(4000, 3).mix_at_many([_ev(0.1, _stereo(1000, 3), (0.5, 0.5), None, None, 1.5, None, (0.05, 0.1, 0.3), (0.0, 0.11), True)])
    assert _entries(lib) == ["sh_mix_events_chan"] and lib.args == (3, 1)
    with pytest.raises(NotImplementedError):
        _mono(4000, 3).mix_at_many([_ev(0.1, _stereo(1000, 3), (0.5, 0.5), envelope=(0.01, 0.01, 0.5, 0.01))])


def test_the_track_as_its_own_balanced_source_goes_through_the_loop_body(monkeypatch):
    """the list is cut at the track; that event is copy().stereo(lf, rf) / mix_at on the host, whatever the library answers"""
    calls = []
    track = _stereo(4000)
    monkeypatch.setattr(Sample, "stereo", lambda self, lf=1.0, rf=1.0: calls.append(("stereo", lf, rf)) or self)
    monkeypatch.setattr(Sample, "mix_at", lambda self, seconds, other, other_seconds=None: calls.append(("mix_at", seconds, other_seconds)) or self)
    monkeypatch.setattr(Sample, "copy", lambda self: self)
    lib = _fake(monkeypatch)
    track.mix_at_many([_ev(0.01, _stereo(100), (0.5, 0.5)), _ev(0.02, track, (0.75, -0.25), None, 0.05)])
    assert _entries(lib) == ["sh_mix_events_chan"]
    assert calls == [("stereo", 0.75, -0.25), ("mix_at", 0.02, 0.05)]
