"""What ``Sample.convolve``, ``mixer.convolve`` and ``mixer.convolve_into`` need of the host alone (no GPU; the binding monkeypatched
with the fake native layer of tests/songhost.py): what each call hands to sh_pcm_convolve, every ``ValueError`` and
``NotImplementedError`` and that each is raised before any call into the library, ``tail=False``, the default factor, a locked input,
an empty window, and that the entry point is declared in the header and bound.  The bytes themselves: tests/test_gpu_convolve.py."""
import re
from pathlib import Path

import pytest

from synthesizer_amd import _native as N
from synthesizer_amd import mixer
from synthesizer_amd.sample import Sample
from tests.songhost import RATE, _Buf, _Lib, _mono, _stereo

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture
def lib(monkeypatch):
    fake = _Lib()
    monkeypatch.setattr(N, "lib", lambda: fake)
    monkeypatch.setattr(N, "DeviceBuffer", _Buf)
    return fake


def _args(call):
    """a recorded sh_pcm_convolve call without its three buffers: (in_off, in_frames, nch, width, ir_off, ir_frames, ir_nch, factor, first,
    nframes, out_off)"""
    name, a = call
    assert name == "sh_pcm_convolve" and len(a) == 14
    return a[1:5] + a[6:12] + a[13:]


def test_a_samples_convolve_is_one_call_over_the_whole_result_in_place(lib):
    s, ir = _stereo(1000), _mono(48)
    assert s.convolve(ir) is s
    assert [_args(c) for c in lib.calls] == [(0, 1000, 2, 2, 0, 48, 1, 1.0 / 32768.0, 0, 1047, 0)]
    assert len(s) == 1047 and s.nchannels == 2 and s.samplewidth == 2 and s.samplerate == RATE and s.on_device
    assert len(ir) == 48                                        # the response is read only


def test_tail_false_keeps_the_samples_length_and_the_default_factor_follows_the_width(lib):
    s = _mono(500, width=1)
    s.convolve(_mono(9, width=1), tail=False)
    assert [_args(c) for c in lib.calls] == [(0, 500, 1, 1, 0, 9, 1, 1.0 / 128.0, 0, 500, 0)] and len(s) == 500
    del lib.calls[:]
    s = _stereo(500)
    s.convolve(_stereo(9), 0.25, tail=False)
    assert [_args(c) for c in lib.calls] == [(0, 500, 2, 2, 0, 9, 2, 0.25, 0, 500, 0)] and len(s) == 500
    del lib.calls[:]
    s = _mono(0)
    s.convolve(_mono(9))                                        # nothing in, nothing out, nothing launched
    assert lib.calls == [] and len(s) == 0
    s.convolve(_mono(9), tail=False)
    assert lib.calls == [] and len(s) == 0


def test_a_locked_sample_is_refused_in_place_and_fine_as_an_input(lib):
    s, ir = _stereo(100).lock(), _mono(5).lock()
    with pytest.raises(RuntimeError, match="locked"):
        s.convolve(ir)
    assert lib.calls == []
    out = mixer.convolve(s, ir)
    assert out is not s and len(out) == 104 and len(s) == 100 and out.nchannels == 2 and out.samplewidth == 2 and out.samplerate == RATE
    assert [_args(c) for c in lib.calls] == [(0, 100, 2, 2, 0, 5, 1, 1.0 / 32768.0, 0, 104, 0)]
    out.convolve(ir)                                            # the result is a Sample of its own: writable
    assert len(out) == 108


def test_a_window_of_the_result_and_a_callers_buffer(lib):
    s, ir = _stereo(1000), _stereo(48)
    out = mixer.convolve(s, ir, 0.5, start_frame=100, nframes=200)
    assert len(out) == 200 and [_args(c) for c in lib.calls] == [(0, 1000, 2, 2, 0, 48, 2, 0.5, 100, 200, 0)]
    del lib.calls[:]
    out = mixer.convolve(s, ir, start_frame=1000)               # to the end: the tail
    assert len(out) == 47 and _args(lib.calls[0])[8:10] == (1000, 47)
    del lib.calls[:]
    buf = N.DeviceBuffer(10000)
    assert mixer.convolve_into(buf, 64, s, ir, 1.5, 7, 300) == 300
    name, a = lib.calls[0]
    assert a[12] is buf.handle and _args(lib.calls[0]) == (0, 1000, 2, 2, 0, 48, 2, 1.5, 7, 300, 64)
    del lib.calls[:]
    assert mixer.convolve_into(buf, 0, s, ir) == 1047 and _args(lib.calls[0])[7:] == (1.0 / 32768.0, 0, 1047, 0)
    del lib.calls[:]
    # an empty window succeeds and calls nothing
    assert len(mixer.convolve(s, ir, start_frame=1047)) == 0 and len(mixer.convolve(s, ir, nframes=0)) == 0
    assert mixer.convolve_into(buf, 0, s, ir, None, 500, 0) == 0 and lib.calls == []


def test_every_refusal_is_raised_before_any_call_into_the_library(lib):
    s, m = _stereo(100), _mono(100)
    other_rate = Sample.from_raw_frames(bytes(20), 2, RATE * 2, 1)
    refusals = [
        (ValueError, "samples of 1 bytes, the sample of 2", lambda who: who(s, _mono(5, width=1))),
        (ValueError, "at %d Hz, the sample at %d" % (2 * RATE, RATE), lambda who: who(s, other_rate)),
        (ValueError, r"sample\.stereo\(\)", lambda who: who(m, _stereo(5))),
        (ValueError, "an empty response", lambda who: who(s, _mono(0))),
        (ValueError, "at most 2\\*\\*22", lambda who: who(m, _mono(2 ** 22 + 1))),
        (ValueError, "not finite", lambda who: who(s, _mono(5), float("inf"))),
        (ValueError, "not finite", lambda who: who(s, _mono(5), float("nan"))),
        (NotImplementedError, "3-byte samples", lambda who: who(_stereo(10, width=3), _mono(5, width=3))),
        (NotImplementedError, "4-byte samples", lambda who: who(_stereo(10, width=4), _mono(5, width=4))),
    ]
    for kind, text, how in refusals:
        for who in (mixer.convolve, lambda a, b, *f: a.convolve(b, *f), lambda a, b, *f: mixer.convolve_into(N.DeviceBuffer(4096), 0, a, b, *f)):
            with pytest.raises(kind, match=text):
                how(who)
    windows = [dict(start_frame=105), dict(start_frame=0, nframes=105), dict(start_frame=100, nframes=5), dict(start_frame=-1), dict(nframes=-1),
               dict(start_frame=1.5), dict(nframes=True)]
    for kw in windows:
        with pytest.raises(ValueError, match="convolve: "):
            mixer.convolve(s, _mono(5), **kw)
        with pytest.raises(ValueError, match="convolve_into: "):
            mixer.convolve_into(N.DeviceBuffer(4096), 0, s, _mono(5), None, kw.get("start_frame", 0), kw.get("nframes"))
    with pytest.raises(ValueError, match=r"frames \[0, 1\) reach past the result's 0"):
        mixer.convolve(_mono(0), _mono(5), nframes=1)
    assert lib.calls == []
    assert len(mixer.convolve(m, _mono(2 ** 22))) == 100 + 2 ** 22 - 1 and len(lib.calls) == 1      # the bound itself is taken


def test_the_entry_point_is_declared_bound_and_built_from_a_unit_of_its_own():
    from synthesizer_amd import build as B
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "synthhip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+sh_pcm_convolve\s*\(", text) and "sh_pcm_convolve" in N.exported_symbols()
    assert len(N._SIGNATURES["sh_pcm_convolve"][1]) == 14
    assert "pcm_fir.hip" in B.SOURCES and "pcmfir.hpp" in B.HEADERS
    assert N.SH_ABI_VERSION == 6                                # no struct changed
