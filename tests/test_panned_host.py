"""What a pan per event in Sample.mix_at_many needs of the host alone (no GPU): sh_mix_event_pan as the header lays it out against the
numpy dtype the binding packs, the ValueErrors raised before the library is even loaded, and which entry point a list goes to."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from synthesizer_amd import _native as N
from synthesizer_amd.sample import Sample

ROOT = Path(__file__).resolve().parent.parent
FIELDS = ["dst_sample", "src_sample", "nsamples", "src_frames", "factor", "left", "right", "src", "inrate", "outrate", "src_channels", "reserved"]
RATE = 8000


def test_the_event_struct_matches_the_header(tmp_path):
    src = tmp_path / "ev.c"
    src.write_text('#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%%zu", sizeof(sh_mix_event_pan));\n%s\nreturn 0;}\n'
                   % (ROOT / "include" / "synthhip.h", "\n".join('printf(" %%zu", offsetof(sh_mix_event_pan, %s));' % f for f in FIELDS)))
    exe = tmp_path / "ev"
    subprocess.run(["gcc", "-std=c99", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    D = N.MIX_EVENT_PAN_DTYPE
    assert got == [D.itemsize] + [D.fields[f][1] for f in FIELDS] == [80, 0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 68, 72]
    assert D.names == tuple(FIELDS)
    # the fields it shares with sh_mix_event_rate have that struct's types
    R = N.MIX_EVENT_RATE_DTYPE
    assert all(D.fields[f][0] == R.fields[f][0] for f in R.names)


def _mono(n=100):
    return Sample.from_raw_frames(bytes(2 * n), 2, RATE, 1)


def _stereo(n=100):
    return Sample.from_raw_frames(bytes(4 * n), 2, RATE, 2)


def _no_library(monkeypatch):
    def refuse(*_a, **_k):
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(N, "lib", refuse)
    monkeypatch.setattr(N, "DeviceBuffer", refuse)


@pytest.mark.parametrize("what, event", [
    ("a stereo other", lambda: (0.1, _stereo(), None, None, None, 0.5)),
    ("a float below -1", lambda: (0.1, _mono(), None, None, None, -1.0001)),
    ("a float above 1", lambda: (0.1, _mono(), None, None, None, 2)),
    ("a float that is no number", lambda: (0.1, _mono(), None, None, None, float("nan"))),
    ("an infinite factor", lambda: (0.1, _mono(), None, None, None, (float("inf"), 0.0))),
    ("a factor that is no number", lambda: (0.1, _mono(), 0.5, None, 2.0, (0.5, float("nan")))),
    ("a pair of one", lambda: (0.1, _mono(), None, None, None, (0.5,))),
    ("a pair of three", lambda: (0.1, _mono(), None, None, None, [0.5, 0.5, 0.5])),
])
def test_mix_at_many_refuses_before_the_library_is_loaded(monkeypatch, what, event):
    _no_library(monkeypatch)
    track = _stereo(1000)
    with pytest.raises(ValueError, match="mix_at_many"):
        track.mix_at_many([(0.0, _mono(), 0.5, None, 1.5, -0.5), event()])       # raised with the other checks: nothing was mixed before
    assert len(track) == 1000 and bytes(track.view_frame_data()) == bytes(4000)


def test_mix_at_many_refuses_a_track_that_is_not_stereo(monkeypatch):
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match="mix_at_many"):
        _mono(1000).mix_at_many([(0.1, _mono(), None, None, None, 0.0)])
    four = Sample.from_raw_frames(bytes(8 * 100), 2, RATE, 4)
    with pytest.raises(ValueError, match="mix_at_many"):
        four.mix_at_many([(0.1, _mono(), None, None, None, (1.0, 1.0))])
    track = _stereo(1000)
    with pytest.raises(ValueError, match="mix_at_many"):
        track.mix_at_many([(0.1, track, None, None, None, 0.0)])                 # the track itself is stereo: it cannot carry a pan
    with pytest.raises(AssertionError):
        track.mix_at_many([(0.1, _mono())])                                     # a mono sample without a pan: mix_at's assertion, as before


class _Buf:
    handle = None

    def __init__(self, nbytes=0):
        self.nbytes = nbytes

    @classmethod
    def from_bytes(cls, data):
        return cls(len(data))

    def zero(self, *_a):
        pass


class _Lib:
    """Every entry point answers SH_OK; the calls and the event tables they were handed are kept."""
    def __init__(self):
        self.calls = []
        self.tables = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            if name.startswith("sh_mix_events"):
                dtype = {"sh_mix_events": N.MIX_EVENT_DTYPE, "sh_mix_events_rate": N.MIX_EVENT_RATE_DTYPE, "sh_mix_events_pan": N.MIX_EVENT_PAN_DTYPE}[name]
                raw = (C.c_char * (args[3] * dtype.itemsize)).from_address(args[2])
                self.tables.append(np.frombuffer(bytes(raw), dtype=dtype))
            return 0
        return call


def _fake_library(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(N, "lib", lambda: lib)
    monkeypatch.setattr(N, "DeviceBuffer", _Buf)
    return lib


def test_a_list_without_pans_does_not_reference_the_new_entry_point(monkeypatch):
    lib = _fake_library(monkeypatch)
    a, b = _stereo(50), _stereo(70)
    _stereo(1000).mix_at_many([(0.01, a, 0.5), (0.02, b, None, 0.001), (0.03, a, None, None, None), (0.04, a, None, None, 1.0, None)])
    assert [c for c in lib.calls if c.startswith("sh_mix_events")] == ["sh_mix_events"]
    _stereo(1000).mix_at_many([(0.01, a, 0.5), (0.02, b, None, None, 1.5), (0.03, a, None, None, 0.5, None)])
    assert [c for c in lib.calls if c.startswith("sh_mix_events")] == ["sh_mix_events", "sh_mix_events_rate"]
    assert [t.dtype for t in lib.tables] == [N.MIX_EVENT_DTYPE, N.MIX_EVENT_RATE_DTYPE]


def test_a_list_with_pans_is_one_table_of_mono_and_stereo_rows(monkeypatch):
    lib = _fake_library(monkeypatch)
    m, s = _mono(100), _stereo(70)
    track = _stereo(1000)
    track.mix_at_many([(0.01, m, 0.5, None, None, 0.5), (0.02, s, None, None, 2.0), (0.03, m, None, 0.005, 0.5, (0.0, 1.25)), (0.04, s, -1.0),
                       (0.2, m, None, None, None, -1.0)])
    assert [c for c in lib.calls if c.startswith("sh_mix_events")] == ["sh_mix_events_pan"]          # one batch, one launch
    (t,) = lib.tables
    assert t.dtype == N.MIX_EVENT_PAN_DTYPE and len(t) == 5
    assert t["src_channels"].tolist() == [1, 2, 1, 2, 1] and t["src"].tolist() == [0, 1, 0, 1, 0]
    assert t["left"].tolist() == [0.25, 0.0, 0.0, 0.0, 1.0] and t["right"].tolist() == [0.75, 0.0, 1.25, 0.0, 0.0]
    assert t["factor"].tolist() == [0.5, 1.0, 1.0, -1.0, 1.0]
    assert t["dst_sample"].tolist() == [160, 320, 480, 640, 3200]                                    # stereo track samples: 2 * int(RATE * seconds)
    # track samples per event: 100 mono frames; 70 stereo frames at twice the speed; 199 resampled mono frames cut at 40; 70; 100
    assert t["nsamples"].tolist() == [200, 70, 80, 140, 200]
    assert t["src_frames"].tolist() == [100, 70, 100, 70, 100]
    assert t["inrate"].tolist() == [RATE, 2 * RATE, RATE // 2, RATE, RATE] and set(t["outrate"].tolist()) == {RATE}
    assert not t["reserved"].any() and not t["src_sample"].any()
    assert len(track) == 1700                                                                        # grown to the end of the last event
