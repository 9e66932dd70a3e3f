"""What an envelope per event in Sample.mix_at_many needs of the host alone (no GPU): sh_mix_event_env and sh_env_segment as the header
lays them out against the numpy dtypes the binding packs, the ValueErrors and the NotImplementedError raised before the library is even
loaded, the host's replay of upstream's part boundaries against ``oracle.sample_oracle.RefSample`` where ``int(rate * (n / rate)) != n``,
and which entry point a list goes to with which table."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle.sample_oracle import RefSample
from synthesizer_amd import _native as N
from synthesizer_amd.sample import _envelope_segments
from tests.songhost import RATE, _Buf, _mono, _stereo

ROOT = Path(__file__).resolve().parent.parent
EVENT_FIELDS = ["dst_sample", "src_sample", "nsamples", "src_frames", "factor", "left", "right", "src", "inrate", "outrate", "src_channels",
                "seg_first", "seg_count", "reserved"]
SEGMENT_FIELDS = ["end", "origin", "mul", "slope", "numsamples", "offset", "kind", "reserved"]


def _layout(tmp_path, struct, fields):
    src = tmp_path / (struct + ".c")
    src.write_text('#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%%zu", sizeof(%s));\n%s\nreturn 0;}\n'
                   % (ROOT / "include" / "synthhip.h", struct, "\n".join('printf(" %%zu", offsetof(%s, %s));' % (struct, f) for f in fields)))
    exe = tmp_path / struct
    subprocess.run(["gcc", "-std=c99", str(src), "-o", str(exe)], check=True)
    return [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]


def test_the_structs_match_the_header(tmp_path):
    D = N.MIX_EVENT_ENV_DTYPE
    assert _layout(tmp_path, "sh_mix_event_env", EVENT_FIELDS) == [D.itemsize] + [D.fields[f][1] for f in EVENT_FIELDS] \
        == [88, 0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 68, 72, 76, 80]
    assert D.names == tuple(EVENT_FIELDS)
    P = N.MIX_EVENT_PAN_DTYPE                               # sh_mix_event_pan's fields where that struct has them, up to its reserved
    assert all(D.fields[f] == P.fields[f] for f in P.names if f != "reserved")
    G = N.ENV_SEGMENT_DTYPE
    assert _layout(tmp_path, "sh_env_segment", SEGMENT_FIELDS) == [G.itemsize] + [G.fields[f][1] for f in SEGMENT_FIELDS] == [56, 0, 8, 16, 24, 32, 40, 48, 52]
    assert G.names == tuple(SEGMENT_FIELDS)


def _no_library(monkeypatch):
    def refuse(*_a, **_k):
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(N, "lib", refuse)
    monkeypatch.setattr(N, "DeviceBuffer", refuse)


nan, inf = float("nan"), float("inf")


@pytest.mark.parametrize("what, envelope", [
    ("three numbers", (0.01, 0.01, 0.5)),
    ("six numbers", (0.01, 0.01, 0.5, 0.01, 0.1, 0.0)),
    ("none", ()),
    ("a number", 0.5),
    ("a negative attack", (-0.01, 0.01, 0.5, 0.01)),
    ("a negative decay", (0.01, -0.01, 0.5, 0.01)),
    ("a negative release", (0.01, 0.01, 0.5, -0.01)),
    ("a negative length", (0.01, 0.01, 0.5, 0.0, -0.1)),
    ("an attack that is no number", (nan, 0.01, 0.5, 0.01)),
    ("an infinite decay", (0.01, inf, 0.5, 0.01)),
    ("an infinite release", (0.01, 0.01, 0.5, inf)),
    ("a length that is no number", (0.01, 0.01, 0.5, 0.01, nan)),
    ("an infinite length", (0.01, 0.01, 0.5, 0.01, inf)),
    ("a sustainlevel above 1", (0.01, 0.01, 1.0001, 0.01)),
    ("a negative sustainlevel", (0.01, 0.01, -0.1, 0.01)),
    ("a sustainlevel that is no number", (0.01, 0.01, nan, 0.01)),
    ("a release longer than the sustain", (0.05, 0.05, 0.5, 0.45)),             # 0.125 s: 0.025 s are left; the track's 0.5 s leave 0.4 s
    ("a release longer than what the length leaves", (0.01, 0.01, 0.5, 0.05, 0.06)),
    ("an attack over the whole sample and a release", (1.0, 0.0, 0.5, 0.001)),
])
def test_mix_at_many_refuses_before_the_library_is_loaded(monkeypatch, what, envelope):
    _no_library(monkeypatch)
    track = _stereo(4000)
    for other, pan in ((_stereo(), None), (_mono(), 0.5)):
        with pytest.raises(ValueError, match="mix_at_many"):
            track.mix_at_many([(0.0, _stereo(), 0.5, None, 1.5, None, (0.01, 0.01, 0.5, 0.01)), (0.1, other, None, None, None, pan, envelope)])
    with pytest.raises(ValueError, match="mix_at_many"):
        track.mix_at_many([(0.1, track, None, None, None, None, envelope)])     # the track itself: checked with the rest, before anything is mixed
    assert len(track) == 4000 and bytes(track.view_frame_data()) == bytes(16000)


def test_a_resampled_note_is_checked_at_its_resampled_length(monkeypatch):
    _no_library(monkeypatch)
    track = _mono(8000)
    env = (0.05, 0.05, 0.5, 0.03)                           # fits 1000 frames at half speed (0.25 s), not at speed 1 (0.125 s) or 2
    with pytest.raises(ValueError, match="mix_at_many"):
        track.mix_at_many([(0.1, _mono(), None, None, None, None, env)])
    with pytest.raises(ValueError, match="mix_at_many"):
        track.mix_at_many([(0.1, _mono(), None, None, 2.0, None, env)])
    with pytest.raises(ValueError, match="mix_at_many"):
        track.mix_at_many([(0.1, _mono(), None, None, 0.5, None, env + (0.12,))])        # ... nor at half speed cut to 0.12 s


def test_24_bit_samples_have_no_envelope(monkeypatch):
    _no_library(monkeypatch)
    track = _stereo(4000, 3)
    with pytest.raises(NotImplementedError):
        track.mix_at_many([(0.1, _stereo(1000, 3), None, None, None, None, (0.01, 0.01, 0.5, 0.01))])
    assert bytes(track.view_frame_data()) == bytes(24000)


# ---- the boundaries ----------------------------------------------------------------------------------------------------------------------
def _parts(data, width, nch, rate, attack, decay, sustainlevel, release):
    """the byte lengths of upstream's parts, from RefSample's own split / duration / frame_idx: attack (faded, unfaded tail), decay
    (unfaded head, faded), sustain, release (unfaded head, faded)"""
    A = RefSample(data, width, rate, nch)
    D = A.split(attack)
    S = D.split(decay)
    R = S.split(S.duration - release)
    a_fade = min(A.frame_idx(min(attack, A.duration)), len(A.frames)) if attack > 0 else 0
    d_head = min(D.frame_idx(D.duration - min(decay, D.duration)), len(D.frames)) if decay > 0 else len(D.frames)
    r_head = min(R.frame_idx(R.duration - min(release, R.duration)), len(R.frames)) if release > 0 else len(R.frames)
    return [a_fade, len(A.frames) - a_fade, d_head, len(D.frames) - d_head, len(S.frames), r_head, len(R.frames) - r_head]


def _expected_segments(parts, width, sustainlevel):
    """the parts as (end, mul, kind, numsamples, origin) in samples, empty ones dropped, neighbours without a ramp and with one mul joined"""
    mul = sustainlevel if sustainlevel < 1 else 1.0
    kinds = [N.ENV_FADE_IN, 0, 0, N.ENV_FADE_OUT, 0, 0, N.ENV_FADE_OUT]
    muls = [1.0, 1.0, 1.0, 1.0, mul, mul, mul]
    out, at = [], 0
    for nb, kind, m in zip(parts, kinds, muls):
        if nb:
            if not kind and out and not out[-1][2] and out[-1][1] == m:
                out[-1] = ((at + nb) // width,) + out[-1][1:]
            else:
                out.append(((at + nb) // width, m, kind, float(nb // width) if kind else 0.0, at // width))
        at += nb
    return out


@pytest.mark.parametrize("width, nch", [(1, 1), (2, 1), (2, 2), (4, 2)])
def test_the_replayed_boundaries_are_refsamples_where_the_rounding_bites(width, nch):
    seen_tail = 0
    for rate in (8000, 11025, 22050, 44100):
        odd = [n for n in range(1, 4000) if int(rate * (n / rate)) != n]          # found by search: n frames last a little less than n / rate
        assert odd, rate
        for n in odd[:6] + odd[-2:]:
            for frames, env in ((n + 2000, ((n + 0.5) / rate, 0.01, 0.5, 0.02)),          # an attack part of n frames
                                (n + 2000, (0.01, (n + 0.5) / rate, 0.5, 0.02)),          # a decay part of n frames
                                (n + 200, (0.004, 0.005, 0.7, n / rate)),                 # a release of about n frames
                                (n, (0.001, 0.002, 0.9, 0.003)),                          # a sample of n frames
                                (n, (n / rate, 0.0, 1.0, 0.0)), (n, (0.0, n / rate, 0.3, 0.0))):
                data = bytes(frames * nch * width)
                try:
                    segs = _envelope_segments(len(data), width, nch, rate, *env)
                except ValueError:
                    assert RefSample(data, width, rate, nch).split(env[0]).split(env[1]).duration - env[3] < 0
                    continue
                parts = _parts(data, width, nch, rate, *env)
                assert sum(parts) == len(data)
                want = _expected_segments(parts, width, env[2])
                assert [(s[0], s[1], s[2], s[4], s[6]) for s in segs] == want, (rate, n, frames, env)
                assert all(s[3] == (1.0 - env[2] if k < len(segs) - 1 and s[2] == N.ENV_FADE_OUT and s[1] == 1.0 else 1.0) for k, s in enumerate(segs) if s[2])
                assert all(s[5] == 0.0 for s in segs)
                seen_tail += bool(parts[0] and parts[1])
    assert seen_tail > 0                                    # an unfaded frame at the tail of the attack part did occur


# ---- which entry point, which table -------------------------------------------------------------------------------------------------------
class _Lib:
    """Every entry point answers SH_OK; the calls and the tables they were handed are kept."""
    DTYPES = {"sh_mix_events": "MIX_EVENT_DTYPE", "sh_mix_events_rate": "MIX_EVENT_RATE_DTYPE", "sh_mix_events_pan": "MIX_EVENT_PAN_DTYPE",
              "sh_mix_events_env": "MIX_EVENT_ENV_DTYPE"}

    def __init__(self):
        self.calls = []
        self.tables = []
        self.segments = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            if name in self.DTYPES:
                dtype = getattr(N, self.DTYPES[name])
                raw = (C.c_char * (args[3] * dtype.itemsize)).from_address(args[2])
                self.tables.append(np.frombuffer(bytes(raw), dtype=dtype))
            if name == "sh_mix_events_env":
                raw = (C.c_char * (args[5] * N.ENV_SEGMENT_DTYPE.itemsize)).from_address(args[4]) if args[5] else b""
                self.segments.append(np.frombuffer(bytes(raw), dtype=N.ENV_SEGMENT_DTYPE))
                self.args = args[6:8]
            return 0
        return call


def _fake_library(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(N, "lib", lambda: lib)
    monkeypatch.setattr(N, "DeviceBuffer", _Buf)
    return lib


def test_a_list_without_envelopes_does_not_reference_the_new_entry_point(monkeypatch):
    lib = _fake_library(monkeypatch)
    m, s = _mono(100), _stereo(70)
    _stereo(4000).mix_at_many([(0.01, s, 0.5), (0.02, s, None, 0.001, None, None, None)])
    _stereo(4000).mix_at_many([(0.01, s, 0.5), (0.02, s, None, None, 1.5, None, None)])
    _stereo(4000).mix_at_many([(0.01, m, 0.5, None, None, 0.5, None), (0.02, s, None, None, 1.5)])
    assert [c for c in lib.calls if c.startswith("sh_mix_events")] == ["sh_mix_events", "sh_mix_events_rate", "sh_mix_events_pan"]
    assert [t.dtype for t in lib.tables] == [N.MIX_EVENT_DTYPE, N.MIX_EVENT_RATE_DTYPE, N.MIX_EVENT_PAN_DTYPE]


def test_a_list_with_an_envelope_is_one_table_of_events_and_one_of_segments(monkeypatch):
    lib = _fake_library(monkeypatch)
    m, s = _mono(1000), _stereo(800)
    track = _stereo(4000)
    track.mix_at_many([
        (0.01, m, 0.5, None, None, 0.5, (0.01, 0.02, 0.5, 0.03)),                # 1000 mono frames: 80 | 160 | 520 | 240
        (0.02, s, None, None, 2.0),                                              # no envelope
        (0.03, s, None, None, None, None, (0.0, 0.0, 1.0, 0.0)),                 # an envelope that does nothing: one plain segment
        (0.04, s, -1.0, 0.05, None, None, (0.01, 0.0, 0.25, 0.01, 0.0625)),      # 500 of 800 stereo frames, cut again at 400 inside the sustain
        (0.05, m, None, None, 0.5, (0.0, 1.25), (0.0, 0.0, 0.0, 0.0)),           # silence, resampled and panned
    ])
    assert [c for c in lib.calls if c.startswith("sh_mix_events")] == ["sh_mix_events_env"]          # one batch, one launch
    assert lib.args == (2, 2)                                                                        # width, the track's channels
    (t,), (g,) = lib.tables, lib.segments
    assert t.dtype == N.MIX_EVENT_ENV_DTYPE and len(t) == 5
    assert t["src_channels"].tolist() == [1, 2, 2, 2, 1] and t["src"].tolist() == [0, 1, 1, 1, 0]
    assert t["left"].tolist() == [0.25, 0.0, 0.0, 0.0, 0.0] and t["right"].tolist() == [0.75, 0.0, 0.0, 0.0, 1.25]
    assert t["factor"].tolist() == [0.5, 1.0, 1.0, -1.0, 1.0]
    assert t["dst_sample"].tolist() == [160, 320, 480, 640, 800]
    assert t["nsamples"].tolist() == [2000, 800, 1600, 800, 3998]
    assert t["inrate"].tolist() == [RATE, 2 * RATE, RATE, RATE, RATE // 2] and set(t["outrate"].tolist()) == {RATE}
    assert t["seg_count"].tolist() == [4, 0, 1, 2, 1] and t["seg_first"].tolist() == [0, 0, 4, 5, 7]
    assert not t["reserved"].any() and not g["reserved"].any() and len(g) == 8
    rows = [tuple(r) for r in g[["end", "origin", "mul", "slope", "numsamples", "offset", "kind"]].tolist()]
    assert rows == [
        (80, 0, 1.0, 1.0, 80.0, 0.0, N.ENV_FADE_IN), (240, 80, 1.0, 0.5, 160.0, 0.0, N.ENV_FADE_OUT), (760, 240, 0.5, 0.0, 0.0, 0.0, N.ENV_NONE),
        (1000, 760, 0.5, 1.0, 240.0, 0.0, N.ENV_FADE_OUT),
        (1600, 0, 1.0, 0.0, 0.0, 0.0, N.ENV_NONE),
        # stereo: positions count samples, two per frame; the release (samples 840 .. 1000) fell to other_seconds' cut at sample 800
        (160, 0, 1.0, 1.0, 160.0, 0.0, N.ENV_FADE_IN), (800, 160, 0.25, 0.0, 0.0, 0.0, N.ENV_NONE),
        (1999, 0, 0.0, 0.0, 0.0, 0.0, N.ENV_NONE),
    ]
