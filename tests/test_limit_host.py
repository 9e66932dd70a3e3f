"""What ``Sample.limit``, ``mixer.limit``, ``mixer.limit_into`` and ``mixer.limit_gain`` need of the host alone (no GPU; the binding
monkeypatched with the fake native layer of tests/songhost.py): what each call hands to sh_pcm_limit, the seconds-to-frames rule, the
``ceiling_db`` rule, every ``ValueError`` and ``NotImplementedError`` and that each is raised before any call into the library, a
locked input, a shared buffer, an empty window, a loud ``SynthHipError`` without a device, and that the entry point is declared in
the header and bound.  The bytes themselves: tests/test_gpu_limit.py."""
import re
from pathlib import Path

import numpy as np
import pytest

from synthesizer_amd import _native as N
from synthesizer_amd import mixer
from synthesizer_amd.sample import Sample
from tests.songhost import RATE, _Buf, _Lib, _mono, _stereo

ROOT = Path(__file__).resolve().parents[1]


class _Plane(_Buf):
    """a device buffer that can be read back and freed, as limit_gain's plane is"""
    freed = 0

    def __init__(self, nbytes=0):
        _Buf.__init__(self, nbytes)
        self.handle = object()                                  # (one of its own: the tests tell the buffers of a call apart by it)

    def download(self, dtype, count, offset=0):
        return np.zeros(count, dtype=dtype)

    def free(self):
        _Plane.freed += 1


@pytest.fixture
def lib(monkeypatch):
    fake = _Lib()
    monkeypatch.setattr(N, "lib", lambda: fake)
    monkeypatch.setattr(N, "DeviceBuffer", _Plane)
    return fake


def _args(call):
    """a recorded sh_pcm_limit call without its three buffers: (in_off, in_frames, nch, width, ceiling, attack, release, first, nframes,
    out_off, gain_off)"""
    name, a = call
    assert name == "sh_pcm_limit" and len(a) == 14
    return a[1:10] + (a[11], a[13])


def test_a_samples_limit_is_one_call_in_place_over_the_whole_sample(lib):
    s = _stereo(1000)
    buf = s._device()
    assert s.limit(20000) is s
    assert [_args(c) for c in lib.calls] == [(0, 1000, 2, 2, 20000, 40, 1600, 0, 1000, 0, 0)]        # 0.005 s and 0.2 s at 8000 Hz
    name, a = lib.calls[0]
    assert a[0] is buf.handle and a[10] is buf.handle and a[12] is None and s._device() is buf      # out IS the sample's own buffer; no gain plane
    assert len(s) == 1000 and s.nchannels == 2 and s.samplewidth == 2 and s.samplerate == RATE and s.on_device
    del lib.calls[:]
    assert _mono(0).limit(5).limit(ceiling_db=-3) is not None and lib.calls == []                    # nothing in, nothing launched


def test_seconds_become_frames_by_rounding_half_up(lib):
    for rate, attack, release, frames in ((8000, 0.005, 0.2, (40, 1600)), (44100, 0.005, 0.2, (221, 8820)), (48000, 0.0, 0.00001, (0, 0)),
                                          (48000, 0.00002, 0.5 / 48000, (1, 1)), (44100, 0.0001, 1.0, (4, 44100)), (48000, 1.5 / 48000, 2.4 / 48000, (2, 2)),
                                          (48000, 2 ** 20 / 48000, 21.0, (2 ** 20, 1008000)), (8000, 1, 2, (8000, 16000))):
        s = Sample.from_raw_frames(bytes(400), 2, rate, 2)
        assert frames == (int(attack * rate + 0.5), int(release * rate + 0.5))
        s.limit(1000, attack, release)
        assert _args(lib.calls[-1])[4:7] == (1000,) + frames, (rate, attack, release)


def test_ceiling_db_is_relative_to_full_scale_and_truncated(lib):
    for width, db, want in ((2, 0, 32767), (2, -6, 16422), (2, -1.0, 29203), (2, -0.1, 32391), (1, -6, 63), (1, 0.0, 127), (4, 0, 2 ** 31 - 1), (4, -20, 214748364),
                            (2, -90.3, 1)):
        assert want == int((2 ** (8 * width - 1) - 1) * 10 ** (db / 20))
        _mono(100, width=width).limit(ceiling_db=db)
        assert _args(lib.calls[-1])[3:5] == (width, want), (width, db)
    del lib.calls[:]
    for kw in (dict(), dict(ceiling=100, ceiling_db=-3), dict(ceiling_db=0.5), dict(ceiling_db=float("nan")), dict(ceiling_db="-3"), dict(ceiling_db=True),
               dict(ceiling_db=-200), dict(ceiling_db=float("-inf"))):
        with pytest.raises(ValueError, match="limit: "):
            _mono(100).limit(**kw)
    assert lib.calls == []


def test_a_locked_sample_is_refused_in_place_and_fine_as_an_input_and_a_shared_buffer_is_not_written(lib):
    s = _stereo(100).lock()
    with pytest.raises(RuntimeError, match="locked"):
        s.limit(100)
    assert lib.calls == []
    out = mixer.limit(s, 100, 3, 4)
    assert out is not s and len(out) == 100 and (out.nchannels, out.samplewidth, out.samplerate) == (2, 2, RATE)
    name, a = lib.calls[0]
    assert _args(lib.calls[0]) == (0, 100, 2, 2, 100, 3, 4, 0, 100, 0, 0) and a[10] is not a[0] and a[10] is out._device().handle
    del lib.calls[:]
    s = _stereo(100)
    shared = s._share_device()                                  # a mixer streams from it: the limiter writes a buffer of its own
    s.limit(100)
    assert len(lib.calls) == 1 and s._device() is not shared and len(s) == 100


def test_a_window_a_callers_buffer_and_the_gain_trace(lib):
    s = _stereo(1000, width=4)
    out = mixer.limit(s, 2 ** 31 - 1, 0, 2 ** 20, start_frame=100, nframes=200)
    assert len(out) == 200 and [_args(c) for c in lib.calls] == [(0, 1000, 2, 4, 2 ** 31 - 1, 0, 2 ** 20, 100, 200, 0, 0)]
    del lib.calls[:]
    assert len(mixer.limit(s, 1, 2 ** 20, 0, start_frame=990)) == 10 and _args(lib.calls[0])[4:9] == (1, 2 ** 20, 0, 990, 10)
    del lib.calls[:]
    buf = N.DeviceBuffer(10000)
    assert mixer.limit_into(buf, 64, s, 5, 6, 7, 8, 300) == 300
    name, a = lib.calls[0]
    assert a[10] is buf.handle and a[12] is None and _args(lib.calls[0]) == (0, 1000, 2, 4, 5, 6, 7, 8, 300, 64, 0)
    del lib.calls[:]
    freed = _Plane.freed
    G = mixer.limit_gain(s, 5, 6, 7, 8, 300)
    name, a = lib.calls[0]
    assert G.dtype == np.uint32 and G.shape == (300,) and a[10] is None and a[12] is not None and _args(lib.calls[0]) == (0, 1000, 2, 4, 5, 6, 7, 8, 300, 0, 0)
    assert _Plane.freed == freed + 1 and len(mixer.limit_gain(s, 5, 6, 7)) == 1000
    del lib.calls[:]
    # an empty window succeeds and calls nothing
    assert len(mixer.limit(s, 5, 6, 7, start_frame=1000)) == 0 and len(mixer.limit(s, 5, 6, 7, nframes=0)) == 0
    assert mixer.limit_into(buf, 0, s, 5, 6, 7, 500, 0) == 0 and mixer.limit_gain(s, 5, 6, 7, 3, 0).shape == (0,) and lib.calls == []


def test_every_refusal_is_raised_before_any_call_into_the_library(lib):
    s = _stereo(100)
    ways = (lambda a, *r, **kw: mixer.limit(a, *r, **kw), lambda a, *r, **kw: mixer.limit_into(N.DeviceBuffer(4096), 0, a, *r, **kw),
            lambda a, *r, **kw: mixer.limit_gain(a, *r, **kw))
    refusals = [
        (ValueError, "ceiling is an int in \\[1, 32767\\]", lambda who: who(s, 0, 1, 1)),
        (ValueError, "ceiling is an int in \\[1, 32767\\]", lambda who: who(s, 32768, 1, 1)),
        (ValueError, "ceiling is an int in \\[1, 127\\]", lambda who: who(_mono(10, width=1), 128, 1, 1)),
        (ValueError, "ceiling is an int in \\[1, 2147483647\\]", lambda who: who(_mono(10, width=4), 2 ** 31, 1, 1)),
        (ValueError, "ceiling is an int", lambda who: who(s, 100.0, 1, 1)),
        (ValueError, "ceiling is an int", lambda who: who(s, True, 1, 1)),
        (ValueError, "attack_frames is an int in \\[0, 2\\*\\*20", lambda who: who(s, 100, 2 ** 20 + 1, 1)),
        (ValueError, "attack_frames is an int", lambda who: who(s, 100, -1, 1)),
        (ValueError, "attack_frames is an int", lambda who: who(s, 100, 1.0, 1)),
        (ValueError, "release_frames is an int in \\[0, 2\\*\\*20", lambda who: who(s, 100, 1, 2 ** 20 + 1)),
        (ValueError, "release_frames is an int", lambda who: who(s, 100, 1, None)),
        (ValueError, "mono and stereo only", lambda who: who(Sample.from_raw_frames(bytes(60), 2, RATE, 3), 100, 1, 1)),
        (NotImplementedError, "3-byte samples are not built", lambda who: who(_stereo(10, width=3), 100, 1, 1)),
    ]
    for kind, text, how in refusals:
        for who in ways:
            with pytest.raises(kind, match=text):
                how(who)
    for kw in (dict(start_frame=101), dict(start_frame=0, nframes=101), dict(start_frame=100, nframes=1), dict(start_frame=-1), dict(nframes=-1),
               dict(start_frame=1.5), dict(nframes=True)):
        for who, name in zip(ways, ("limit: ", "limit_into: ", "limit_gain: ")):
            with pytest.raises(ValueError, match=name):
                who(s, 100, 1, 1, **kw)
    with pytest.raises(ValueError, match=r"frames \[0, 1\) reach past the sample's 0"):
        mixer.limit(_mono(0), 5, 1, 1, nframes=1)
    # the method: the same refusals, and its own
    with pytest.raises(NotImplementedError, match="3-byte samples are not built"):
        _stereo(10, width=3).limit(100)
    for kw in (dict(ceiling=0), dict(ceiling=32768), dict(ceiling=100.5), dict(ceiling=100, attack=-0.1), dict(ceiling=100, release=float("nan")),
               dict(ceiling=100, attack=float("inf")), dict(ceiling=100, release="1"), dict(ceiling=100, attack=(2 ** 20 + 1) / RATE),
               dict(ceiling=100, release=132.0)):
        with pytest.raises(ValueError, match="limit: "):
            _stereo(100).limit(**kw)
    assert lib.calls == []
    assert _stereo(100).limit(100, 2 ** 20 / RATE, 131.0) is not None and _args(lib.calls[0])[5:7] == (2 ** 20, 131 * RATE)      # the bound itself is taken


def test_without_a_device_the_call_fails_loudly():
    """no fake layer here: the library cannot initialise without a GPU, and says so"""
    if N.lib().sh_device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(N.SynthHipError):
        Sample.from_raw_frames(bytes(400), 2, RATE, 2).limit(1000)
    with pytest.raises(N.SynthHipError):
        mixer.limit_gain(Sample.from_raw_frames(bytes(400), 2, RATE, 2), 1000, 1, 1)


def test_the_entry_point_is_declared_bound_and_built_from_a_unit_of_its_own():
    from synthesizer_amd import build as B
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "synthhip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+sh_pcm_limit\s*\(", text) and "sh_pcm_limit" in N.exported_symbols()
    assert len(N._SIGNATURES["sh_pcm_limit"][1]) == 14
    assert "pcm_limit.hip" in B.SOURCES and "pcmlimit.hpp" in B.HEADERS
    assert N.SH_ABI_VERSION == 6                                # no struct changed
    assert (N.PCM_LIMIT_ONE, N.PCM_LIMIT_TILE_FRAMES, N.PCM_LIMIT_MAX_FRAMES) == (2 ** 30, 2048, 2 ** 20)
