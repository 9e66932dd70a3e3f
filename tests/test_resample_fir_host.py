"""What ``Sample.resample_fir``, ``mixer.resample_fir``, ``mixer.resample_fir_into`` and ``mixer.lowpass_taps`` need of the host alone
(no GPU; the binding monkeypatched with the fake native layer of tests/songhost.py): what each door hands to sh_pcm_resample_fir,
every ``ValueError`` and ``NotImplementedError`` and that each is raised before any call into the library, the gcd reduction, the
defaults of ``factor`` and ``delay``, that the entry points are declared in the header and bound and the new files built; and the
default tap bank: its shape, and what it does to sines through the reference alone (tests/resampleref.py), which is run here on the
CPU.  The bytes of the kernel: tests/test_gpu_resample_fir.py."""
import re
from pathlib import Path

import numpy as np
import pytest

from synthesizer_amd import _native as N
from synthesizer_amd import mixer
from synthesizer_amd.sample import Sample
from tests import resampleref
from tests.songhost import RATE, _Buf, _Lib, _mono, _stereo

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture
def lib(monkeypatch):
    fake = _Lib()
    monkeypatch.setattr(N, "lib", lambda: fake)
    monkeypatch.setattr(N, "DeviceBuffer", _Buf)
    return fake


def _args(call):
    """a recorded sh_pcm_resample_fir call without its three buffers: (in_off, in_frames, nch, width, taps_off, ntaps, up, down, delay,
    factor, first, nframes, out_off)"""
    name, a = call
    assert name == "sh_pcm_resample_fir" and len(a) == 16
    return a[1:5] + a[6:14] + a[15:]


def at(rate, n=1000, nch=2, width=2):
    return Sample.from_raw_frames(bytes(nch * width * n), width, rate, nch)


def test_a_samples_resample_fir_is_one_call_over_the_whole_result_in_place(lib):
    s = at(44100, 1470)
    assert s.resample_fir(48000) is s
    m = 2 * 16 * 160 + 1
    assert [_args(c) for c in lib.calls] == [(0, 1470, 2, 2, 0, m, 160, 147, (m - 1) // 2, 2.0 ** -14, 0, 1600, 0)]
    assert len(s) == 1600 and s.samplerate == 48000 and s.nchannels == 2 and s.samplewidth == 2 and s.on_device
    del lib.calls[:]
    assert s.resample_fir(48000) is s and lib.calls == [] and len(s) == 1600                      # the same rate, the default taps: untouched
    s.resample_fir(48000, np.array([3, 5, 7], dtype=np.int16), 0.5, 2)                           # the same rate under taps of the caller's: a filter
    assert [_args(c) for c in lib.calls] == [(0, 1600, 2, 2, 0, 3, 1, 1, 2, 0.5, 0, 1600, 0)] and s.samplerate == 48000
    del lib.calls[:]
    e = at(44100, 0, 1, 1)
    assert e.resample_fir(8000) is e and lib.calls == [] and len(e) == 0 and e.samplerate == 8000  # nothing in, nothing out, nothing launched
    with pytest.raises(RuntimeError, match="locked"):
        at(44100).lock().resample_fir(48000)
    assert lib.calls == []


def test_the_rates_are_reduced_by_their_gcd_and_the_length_is_the_ceiling(lib):
    for rate_in, rate_out, n, up, down in ((44100, 48000, 1001, 160, 147), (48000, 44100, 1001, 147, 160), (44100, 96000, 10, 320, 147), (48000, 8000, 1001, 1, 6),
                                           (44100, 8000, 1001, 80, 441), (8000, 16000, 7, 2, 1), (8000, 12000, 7, 3, 2), (11025, 44100, 3, 4, 1)):
        out = mixer.resample_fir(at(rate_in, n, 1), rate_out)
        m = 2 * 16 * max(up, down) + 1
        total = -(-n * up // down)
        assert _args(lib.calls[-1]) == (0, n, 1, 2, 0, m, up, down, (m - 1) // 2, 2.0 ** -14, 0, total, 0), (rate_in, rate_out)
        assert len(out) == total and out.samplerate == rate_out and out.nchannels == 1 and out.samplewidth == 2


def test_the_taps_the_factor_and_the_delay_of_the_caller(lib):
    s = at(8000, 100, 1, 1).lock()                                  # the input is read only: a locked one is fine
    out = mixer.resample_fir(s, 12000, np.arange(1, 12, dtype=np.int16))
    assert out is not s and len(out) == 150 and len(s) == 100 and out.samplewidth == 1
    assert _args(lib.calls[-1]) == (0, 100, 1, 1, 0, 11, 3, 2, 5, 2.0 ** -14, 0, 150, 0)             # the taps are 16 bits at every width
    mixer.resample_fir(s, 12000, np.arange(1, 13, dtype=np.int16), 0.25)
    assert _args(lib.calls[-1])[5:10] == (12, 3, 2, 5, 0.25)                                        # (m - 1) // 2
    mixer.resample_fir(s, 12000, _mono(12), 1, 0)
    assert _args(lib.calls[-1])[5:10] == (12, 3, 2, 0, 1.0)
    mixer.resample_fir(s, 12000, _mono(12), delay=11)
    assert _args(lib.calls[-1])[5:10] == (12, 3, 2, 11, 2.0 ** -14)
    mixer.resample_fir(s, 12000, _mono(2 ** 22), delay=0)                                           # the bound itself is taken
    assert _args(lib.calls[-1])[5] == 2 ** 22


def test_a_window_of_the_result_and_a_callers_buffer(lib):
    s = at(44100, 1470)
    out = mixer.resample_fir(s, 48000, start_frame=100, nframes=200)
    assert len(out) == 200 and _args(lib.calls[-1])[10:] == (100, 200, 0)
    out = mixer.resample_fir(s, 48000, start_frame=1000)
    assert len(out) == 600 and _args(lib.calls[-1])[10:] == (1000, 600, 0)
    buf = N.DeviceBuffer(10000)
    taps = np.array([1, 2, 3], dtype=np.int16)
    assert mixer.resample_fir_into(buf, 64, s, 48000, taps, 1.5, 1, 7, 300) == 300
    name, a = lib.calls[-1]
    assert a[14] is buf.handle and _args(lib.calls[-1]) == (0, 1470, 2, 2, 0, 3, 160, 147, 1, 1.5, 7, 300, 64)
    assert mixer.resample_fir_into(buf, 0, s, 48000) == 1600 and _args(lib.calls[-1])[10:] == (0, 1600, 0)
    del lib.calls[:]
    # an empty window succeeds and calls nothing
    assert len(mixer.resample_fir(s, 48000, start_frame=1600)) == 0 and len(mixer.resample_fir(s, 48000, nframes=0)) == 0
    assert mixer.resample_fir_into(buf, 0, s, 48000, None, None, None, 500, 0) == 0 and lib.calls == []


def test_every_refusal_is_raised_before_any_call_into_the_library(lib):
    s = at(44100, 147)
    i16 = lambda *v: np.array(v, dtype=np.int16)
    refusals = [
        (ValueError, "samplerate is a positive int", lambda who: who(s, 0)),
        (ValueError, "samplerate is a positive int", lambda who: who(s, 48000.0)),
        (ValueError, "samplerate is a positive int", lambda who: who(s, True)),
        (NotImplementedError, r"3-byte samples.*make_16bit\(\)", lambda who: who(at(44100, 10, 2, 3), 48000)),
        (NotImplementedError, r"4-byte samples.*make_16bit\(\)", lambda who: who(at(44100, 10, 2, 4), 48000)),
        (ValueError, "44100 Hz to 44101 Hz is 44101/44100: up is at most 4096", lambda who: who(s, 44101)),
        (ValueError, "44100 Hz to 700 Hz is 1/63: a stride of 504 frames is too long .*two steps", lambda who: who(s, 700)),
        (ValueError, "one-dimensional int16 array", lambda who: who(s, 48000, np.array([1.0, 2.0]))),
        (ValueError, "one-dimensional int16 array", lambda who: who(s, 48000, np.zeros((2, 2), dtype=np.int16))),
        (ValueError, "numpy int16 array or a 16-bit mono Sample", lambda who: who(s, 48000, [1, 2, 3])),
        (ValueError, "16-bit mono Sample, not 1 bytes and 1 channels", lambda who: who(s, 48000, _mono(5, width=1))),
        (ValueError, "16-bit mono Sample, not 2 bytes and 2 channels .a stereo bank is not built", lambda who: who(s, 48000, _stereo(5))),
        (ValueError, "no taps", lambda who: who(s, 48000, i16())),
        (ValueError, "at most 2\\*\\*22", lambda who: who(s, 48000, _mono(2 ** 22 + 1))),
        (ValueError, "not finite", lambda who: who(s, 48000, None, float("inf"))),
        (ValueError, "not finite", lambda who: who(s, 48000, None, float("nan"))),
        (ValueError, r"delay is an int in \[0, 3\)", lambda who: who(s, 48000, i16(1, 2, 3), None, 3)),
        (ValueError, r"delay is an int in \[0, 3\)", lambda who: who(s, 48000, i16(1, 2, 3), None, -1)),
        (ValueError, r"delay is an int in \[0, 3\)", lambda who: who(s, 48000, i16(1, 2, 3), None, 1.0)),
    ]
    for kind, text, how in refusals:
        for who in (mixer.resample_fir, lambda a, *r: a.resample_fir(*r), lambda a, *r: mixer.resample_fir_into(N.DeviceBuffer(4096), 0, a, *r)):
            with pytest.raises(kind, match=text):
                how(who)
    windows = [dict(start_frame=161), dict(start_frame=0, nframes=161), dict(start_frame=100, nframes=61), dict(start_frame=-1), dict(nframes=-1),
               dict(start_frame=1.5), dict(nframes=True)]
    for kw in windows:
        with pytest.raises(ValueError, match="resample_fir: "):
            mixer.resample_fir(s, 48000, **kw)
        with pytest.raises(ValueError, match="resample_fir_into: "):
            mixer.resample_fir_into(N.DeviceBuffer(4096), 0, s, 48000, **kw)
    with pytest.raises(ValueError, match=r"frames \[0, 1\) reach past the result's 0"):
        mixer.resample_fir(at(44100, 0), 48000, nframes=1)
    with pytest.raises(ValueError, match="mono and stereo only, not 3 channels"):
        mixer.resample_fir(at(44100, 10, 3), 48000)
    assert lib.calls == []


def test_the_entry_points_are_declared_bound_and_built_from_a_unit_of_its_own():
    from synthesizer_amd import build as B
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "synthhip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+sh_pcm_resample_fir\s*\(", text) and re.search(r"\buint64_t\s+sh_pcm_resample_fir_frames\s*\(", text)
    assert {"sh_pcm_resample_fir", "sh_pcm_resample_fir_frames"} <= set(N.exported_symbols())
    assert len(N._SIGNATURES["sh_pcm_resample_fir"][1]) == 16 and len(N._SIGNATURES["sh_pcm_resample_fir_frames"][1]) == 3
    assert "pcm_resample_fir.hip" in B.SOURCES and "pcmresample.hpp" in B.HEADERS
    assert N.SH_ABI_VERSION == 6                                # no struct changed


def test_the_length_function_works_without_a_device():
    L = N.lib()
    for n, up, down in ((0, 3, 2), (1, 1, 1), (44100, 160, 147), (48000, 147, 160), (7, 3, 2), (2 ** 40 + 1, 4096, 4095)):
        assert L.sh_pcm_resample_fir_frames(n, up, down) == -(-n * up // down)


# ---- the default bank
def test_lowpass_taps_shape():
    for up, down in ((160, 147), (147, 160), (320, 147), (1, 6), (2, 1), (1, 1), (80, 441)):
        h = mixer.lowpass_taps(up, down)
        q = max(up, down)
        assert h.dtype == np.int16 and h.shape == (32 * q + 1,) and np.array_equal(h, h[::-1])
        assert np.array_equal(h, resampleref.lowpass_taps(up, down))
        if up >= down:
            assert h.max() == 16384 == h[(len(h) - 1) // 2]
        for p in range(up):                                        # every phase passes DC at unity, to the rounding of its taps
            assert abs(int(h[p::up].astype(np.int64).sum()) - 16384) <= 16, (up, down, p)
    assert len(mixer.lowpass_taps(3, 2, zero_crossings=4)) == 25 and len(mixer.lowpass_taps(2 ** 17 - 1, 1)) == 2 ** 22 - 31
    with pytest.raises(ValueError, match="at most 2\\*\\*22"):
        mixer.lowpass_taps(2 ** 17, 1)
    for bad in ((0, 1), (1, 0), (1.5, 1), (True, 1)):
        with pytest.raises(ValueError, match="positive int"):
            mixer.lowpass_taps(*bad)


def _sine(freq, rate, n, amp=16384.0):
    return amp * np.sin(2.0 * np.pi * freq * np.arange(n) / rate)


def _through(freq, rate_in, rate_out, seconds=0.5):
    """a half-scale sine through the reference with the default bank, factor and delay -> (result, ideal sine at the new rate)"""
    g = np.gcd(rate_in, rate_out)
    up, down = rate_out // g, rate_in // g
    n = int(rate_in * seconds)
    x = np.rint(_sine(freq, rate_in, n)).astype(np.int64).reshape(-1, 1)
    h = mixer.lowpass_taps(up, down).astype(np.int64)
    y = resampleref.resample(x, h, up, down, (len(h) - 1) // 2, 2.0 ** -14, 2)[:, 0]
    return y.astype(np.float64), _sine(freq, rate_out, len(y))


@pytest.mark.parametrize("freq,rate_in,rate_out", [(1000, 44100, 48000), (18000, 44100, 48000), (1000, 48000, 44100), (10000, 44100, 96000)])
def test_a_sine_in_the_passband_meets_the_ideal_sine_at_the_new_rate(freq, rate_in, rate_out):
    """rms error below 3.0 sample steps, the first 2000 frames at each end left out (measured with this reference: 1.41, 1.42, 1.45, 1.30;
    fbound floors, which alone is an offset of half a step and an rms of 0.58)"""
    y, ideal = _through(freq, rate_in, rate_out)
    err = (y - ideal)[2000:-2000]
    rms = float(np.sqrt(np.mean(err ** 2)))
    print("rms error %.3f" % rms)
    assert len(err) > 10000 and rms < 3.0


def test_a_sine_above_the_new_nyquist_frequency_does_not_fold_back():
    """a half-scale 5 kHz sine 48 -> 8 kHz comes out below 16 rms (measured: 3.7), against 11 586 for a tone in the passband"""
    y, _ = _through(5000, 48000, 8000)
    rms = float(np.sqrt(np.mean(y[400:-400] ** 2)))
    print("rms %.3f" % rms)
    assert rms < 16.0
    y, ideal = _through(1000, 48000, 8000)
    assert abs(float(np.sqrt(np.mean(y[400:-400] ** 2))) - 16384 / np.sqrt(2.0)) < 20.0
