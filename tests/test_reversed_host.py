"""What a region and reversed playback per event in Sample.mix_at_many need of the host alone (no GPU): sh_mix_event_rev as the header
lays it out against the numpy dtype the binding packs, the ValueErrors raised before the library is even loaded, which entry point a list
goes to with which table -- no region and no reverse: today's tables; regions alone: today's entry point with src_sample and src_frames
filled in; one reversed event: sh_mix_events_rev -- and the region arithmetic (int(rate * s), clamping, end=None)."""
import pytest

from synthesizer_amd import _native as N
from synthesizer_amd.sample import Sample, _region_frames
from tests.songhost import RATE, _mono, _stereo
from tests.test_enveloped_host import _layout, _no_library
from tests.test_looped_host import LOOP_FIELDS, _LoopLib

REV_FIELDS = LOOP_FIELDS + ["flags"]
nan, inf = float("nan"), float("inf")


class _RevLib(_LoopLib):
    DTYPES = dict(_LoopLib.DTYPES, sh_mix_events_rev="MIX_EVENT_REV_DTYPE")


def _fake(monkeypatch):
    from tests.test_enveloped_host import _Buf
    lib = _RevLib()
    monkeypatch.setattr(N, "lib", lambda: lib)
    monkeypatch.setattr(N, "DeviceBuffer", _Buf)
    return lib


def _entries(lib):
    return [c for c in lib.calls if c.startswith("sh_mix_events")]


def test_the_struct_matches_the_header(tmp_path):
    D = N.MIX_EVENT_REV_DTYPE
    assert _layout(tmp_path, "sh_mix_event_rev", REV_FIELDS) == [D.itemsize] + [D.fields[f][1] for f in REV_FIELDS] \
        == [112, 0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 68, 72, 76, 80, 88, 96, 104]
    assert D.names == tuple(REV_FIELDS)
    L = N.MIX_EVENT_LOOP_DTYPE                              # sh_mix_event_loop's fields where that struct has them
    assert all(D.fields[f] == L.fields[f] for f in L.names)
    assert N.MIX_EVENT_REVERSED == 1


@pytest.mark.parametrize("what, region", [
    ("one number", (0.01,)),
    ("three numbers", (0.01, 0.02, 0.03)),
    ("none", ()),
    ("a number", 0.5),
    ("a string", "ab"),
    ("a negative start", (-0.01, 0.02)),
    ("a negative end", (0.0, -0.02)),
    ("a start that is no number", (nan, 0.02)),
    ("an infinite start", (inf, None)),
    ("an end that is no number", (0.01, nan)),
    ("an infinite end", (0.01, inf)),
    ("a start that is a string", ("a", 0.02)),
    ("an end before the start", (0.03, 0.02)),
    ("an end a hair before the start", (0.0200001, 0.02)),
])
def test_mix_at_many_refuses_before_the_library_is_loaded(monkeypatch, what, region):
    _no_library(monkeypatch)
    track = _stereo(4000)
    for reverse in (None, True):
        for other, pan in ((_stereo(), None), (_mono(), 0.5)):
            with pytest.raises(ValueError, match="mix_at_many: region"):
                track.mix_at_many([(0.0, _stereo(), 0.5, None, 1.5, None, None, None, (0.01, 0.02), True),
                                   (0.1, other, None, None, None, pan, None, None, region, reverse)])
        with pytest.raises(ValueError, match="mix_at_many: region"):
            track.mix_at_many([(0.1, track, None, None, None, None, None, None, region, reverse)])      # the track itself: checked with the rest
    assert len(track) == 4000 and bytes(track.view_frame_data()) == bytes(16000)


def test_a_start_behind_the_sample_with_no_end_is_an_end_before_the_start(monkeypatch):
    """clip(start, other.duration) asserts end >= start upstream"""
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match="mix_at_many: region"):
        _stereo(4000).mix_at_many([(0.1, _stereo(1000), None, None, None, None, None, None, (0.2, None))])


def test_an_empty_region_with_a_loop_is_the_loops_no_frame_between(monkeypatch):
    _no_library(monkeypatch)
    for region in ((0.05, 0.05), (0.125, None), (0.125, 0.5), (0.0100, 0.0101)):
        for reverse in (False, True):
            with pytest.raises(ValueError, match="mix_at_many: loop: no frame between"):
                _stereo(4000).mix_at_many([(0.1, _stereo(1000), None, None, None, None, None, (0.0, 0.01, 0.5), region, reverse)])
    # and the loop is clamped to the region's frames, not the sample's: frames 80 .. 160 of the sample hold no frame 100 of their own
    with pytest.raises(ValueError, match="mix_at_many: loop: no frame between"):
        _stereo(4000).mix_at_many([(0.1, _stereo(1000), None, None, None, None, None, (100 / RATE, 0.1, 0.5), (0.01, 0.02))])


def test_the_region_arithmetic():
    """clip's: fb * int(rate * s) under byte-slicing rules, so clamped to the sample; end None is the sample's duration, a float"""
    assert _region_frames((0.01, 0.02), 8000, 1000, 0.125) == (80, 80)
    assert _region_frames([0.01, 0.02], 8000, 1000, 0.125) == (80, 80)
    assert _region_frames((0.0, None), 8000, 1000, 0.125) == (0, 1000)
    assert _region_frames((0.1, None), 8000, 1000, 0.125) == (800, 200)
    assert _region_frames((0.1, 0.5), 8000, 1000, 0.125) == (800, 200)         # the end clamped
    assert _region_frames((0.2, 0.5), 8000, 1000, 0.125) == (1000, 0)          # both clamped: empty, and inside the sample
    assert _region_frames((0.05, 0.05), 8000, 1000, 0.125) == (400, 0)
    assert _region_frames((0.0100, 0.0101), 8000, 1000, 0.125) == (80, 0)      # less than a frame
    assert _region_frames((0.0199, 0.0201), 8000, 1000, 0.125) == (159, 1)     # int() truncates
    assert _region_frames((1, 2), 8000, 100000, 12.5) == (8000, 8000)          # ints are numbers
    # int(rate * (n / rate)) is n - 1 for some n: end=None then stops a frame short, as other.duration does in clip
    rate = 44100
    n = next(n for n in range(1, 4000) if int(rate * (2 * n / rate / 2 / 1)) != n)          # duration: nbytes / rate / width / nchannels
    s = Sample.from_raw_frames(bytes(2 * n), 2, rate, 1)
    assert int(rate * s.duration) == n - 1
    assert _region_frames((0.0, None), rate, n, s.duration) == (0, n - 1)


def test_no_region_and_no_reverse_packs_todays_tables(monkeypatch):
    lib = _fake(monkeypatch)
    m, s = _mono(1000), _stereo(800)
    env = (0.001, 0.001, 0.5, 0.001)
    lists = [[(0.01, s, 0.5), (0.02, s, None, 0.001)],
             [(0.01, s, 0.5), (0.02, s, None, None, 1.5)],
             [(0.01, m, 0.5, None, None, 0.5), (0.02, s, None, None, 1.5)],
             [(0.01, m, 0.5, None, None, 0.5, env), (0.02, s, None, None, 1.5)],
             [(0.01, m, 0.5, None, None, 0.5, env, (0.05, 0.1, 0.3)), (0.02, s, None, None, 1.5)]]
    for lst in lists:
        _stereo(4000).mix_at_many(lst)
    names = ["sh_mix_events", "sh_mix_events_rate", "sh_mix_events_pan", "sh_mix_events_env", "sh_mix_events_loop"]
    assert _entries(lib) == names
    short = [t.tobytes() for t in lib.tables]
    for tail in ((None, None), (None, False), (None, 0), (None, "")):        # reverse is taken by truth value
        del lib.calls[:], lib.tables[:]
        for lst in lists:
            _stereo(4000).mix_at_many([tuple(e) + (None,) * (8 - len(e)) + tail for e in lst])
        assert _entries(lib) == names
        assert [t.tobytes() for t in lib.tables] == short
    assert [t.dtype for t in lib.tables] == [N.MIX_EVENT_DTYPE, N.MIX_EVENT_RATE_DTYPE, N.MIX_EVENT_PAN_DTYPE, N.MIX_EVENT_ENV_DTYPE,
                                             N.MIX_EVENT_LOOP_DTYPE]


def test_regions_alone_go_where_the_list_went_with_src_sample_and_src_frames_filled_in(monkeypatch):
    lib = _fake(monkeypatch)
    m, s = _mono(1000), _stereo(800)
    env = (0.001, 0.001, 0.5, 0.001)
    region = (0.01, 0.05)                                   # frames 80 .. 400
    lists = [[(0.01, s, 0.5), (0.02, s, None, 0.001)],
             [(0.01, s, 0.5), (0.02, s, None, None, 2.0)],
             [(0.01, m, 0.5, None, None, 0.5), (0.02, s, None, None, 2.0)],
             [(0.01, m, 0.5, None, None, 0.5, env), (0.02, s, None, None, 2.0)],
             [(0.01, m, 0.5, None, None, 0.5, env, (0.02, 0.03, 0.3)), (0.02, s, None, None, 2.0)]]
    names = ["sh_mix_events", "sh_mix_events_rate", "sh_mix_events_pan", "sh_mix_events_env", "sh_mix_events_loop"]
    for lst in lists:
        _stereo(4000).mix_at_many(lst)
    plain = list(lib.tables)
    del lib.calls[:], lib.tables[:]
    for lst in lists:                                       # the second event gets the region
        _stereo(4000).mix_at_many([lst[0], tuple(lst[1]) + (None,) * (8 - len(lst[1])) + (region,)])
    assert _entries(lib) == names
    for k, (a, b) in enumerate(zip(plain, lib.tables)):
        assert a.dtype == b.dtype and a[0].tobytes() == b[0].tobytes()               # the same dtype, the other row untouched
        assert b["src_sample"].tolist() == [0, 160]                                  # samples: frame 80 of a stereo source
        if k == 0:
            assert b["nsamples"].tolist() == [1600, 16]                              # other_seconds cuts 8 frames of the 320
        else:
            assert b["src_frames"].tolist()[1] == 320 and b["src_frames"][0] == a["src_frames"][0]
            assert b["nsamples"].tolist()[1] == 2 * ((320 - 1) * RATE // (2 * RATE) + 1)    # ratecv over the region's 320 frames
        changed = {"src_sample", "nsamples", "src_frames"}
        assert all(a[f][1] == b[f][1] for f in a.dtype.names if f not in changed)
    # a region of a looped, panned, enveloped mono event: the loop clamped to the region, the envelope over the held note
    del lib.calls[:], lib.tables[:], lib.segments[:]
    _stereo(4000).mix_at_many([(0.01, m, 0.5, None, None, 0.5, (0.01, 0.0, 0.25, 0.01, 0.2), (0.02, 0.5, 0.3), (0.05, 0.1))])
    (t,) = lib.tables
    assert _entries(lib) == ["sh_mix_events_loop"] and t.dtype == N.MIX_EVENT_LOOP_DTYPE
    assert t["src_sample"].tolist() == [400] and t["loop_start"].tolist() == [160] and t["loop_frames"].tolist() == [240]      # E = min(4000, 400)
    assert t["src_frames"].tolist() == [2400] and t["nsamples"].tolist() == [3200]                      # the envelope's length: 1600 frames
    # an empty region: nothing is mixed and the track grows to the event's start
    del lib.calls[:], lib.tables[:]
    track = _stereo(100)
    track.mix_at_many([(0.05, s, None, None, None, None, None, None, (0.2, 0.3))])
    assert len(track) == 400
    assert lib.tables[0]["nsamples"].tolist() == [0] and lib.tables[0]["src_sample"].tolist() == [1600]


def test_one_reversed_event_and_the_list_goes_to_the_new_entry_point(monkeypatch):
    lib = _fake(monkeypatch)
    m, s = _mono(1000), _stereo(800)
    track = _stereo(4000)
    track.mix_at_many([
        (0.01, s, 0.5),                                                          # no flag: a row of sh_mix_events_loop
        (0.02, s, None, None, 2.0, None, None, None, None, True),                # the whole sample backwards, at speed 2
        (0.03, s, None, None, None, None, None, None, (0.01, 0.05), 1),          # frames 80 .. 400 backwards
        (0.04, m, None, None, None, 0.5, None, (0.02, 0.03, 0.3), (0.05, 0.1), True),     # region 400 .. 800, loop 160 .. 240 of the reversed
        (0.05, m, None, None, None, (0.0, 1.25), None, (0.0, 0.5, 0.01), None, "yes"),    # E clamped to 1000; V = 80: a plain cut, still a loop row
        (0.06, s, None, None, None, None, None, (0.01, 0.02, 0.1), (0.01, 0.05), False),   # a looped region forwards among them
    ])
    assert _entries(lib) == ["sh_mix_events_rev"]                                # one batch, one launch
    (t,) = lib.tables
    assert t.dtype == N.MIX_EVENT_REV_DTYPE and len(t) == 6
    assert t["flags"].tolist() == [0, 1, 1, 1, 1, 0] and not t["reserved"].any()
    # the region as stored, forwards; a reversed looped row: the loop_end frames at the region's END
    assert t["src_sample"].tolist() == [0, 0, 160, 400 + (400 - 240), 0, 160]
    assert t["loop_start"].tolist() == [0, 0, 0, 160, 0, 80] and t["loop_frames"].tolist() == [0, 0, 0, 80, 1000, 80]
    assert t["src_frames"].tolist() == [800, 800, 320, 2400, 80, 800]
    assert t["nsamples"].tolist() == [1600, 2 * ((800 - 1) // 2 + 1), 640, 4800, 160, 1600]
    assert t["src_channels"].tolist() == [2, 2, 2, 1, 1, 2] and t["src"].tolist() == [0, 0, 0, 1, 1, 0]


def test_24_bit_samples_may_play_backwards_but_have_no_envelope(monkeypatch):
    lib = _fake(monkeypatch)
    _stereo(4000, 3).mix_at_many([(0.1, _stereo(1000, 3), None, None, 1.5, None, None, (0.05, 0.1, 0.3), (0.0, 0.11), True)])
    assert _entries(lib) == ["sh_mix_events_rev"]
    with pytest.raises(NotImplementedError):
        _stereo(4000, 3).mix_at_many([(0.1, _stereo(1000, 3), None, None, None, None, (0.01, 0.01, 0.5, 0.01), None, None, True)])
