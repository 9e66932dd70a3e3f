"""What the stems of a compiled song -- ``CompiledSequence.stems`` and ``stems_into``, ``SongStems``, ``N.Sequence.stems``,
sh_seq_render_stems -- need of the host alone (no GPU; the fake native layer of tests/songhost.py):
that ``stems`` hands on exactly the desk's keywords plus the stride, that the stride it picks keeps every plane on the store's 16-byte
grid, what is refused before any buffer is made, that the new symbol is declared in the header and bound, and that ``stem()`` is still
``render`` with one-hot gains.  The bytes: tests/test_gpu_stems.py."""
import ctypes as C
import re
from pathlib import Path

import pytest

from synthesizer_amd import _native as N
from synthesizer_amd import mixer
from tests.songhost import RATE, _Auto, _fake, _Lib, _mono, _Seq, _StemBuf, _stereo

nan, inf = float("nan"), float("inf")


class _StemSeq(_Seq):
    """tests/songhost._Seq, which also keeps what each stems call was handed"""

    def __init__(self, *a, **kw):
        _Seq.__init__(self, *a, **kw)
        self.stemmed = []

    def stems(self, first_sample, nsamples, out, out_sample, plane_samples, **kw):
        self.stemmed.append((first_sample, nsamples, out, out_sample, plane_samples, kw))


def _song(monkeypatch, nch=2, width=2):
    _fake(monkeypatch)
    monkeypatch.setattr(N, "DeviceBuffer", _StemBuf)
    monkeypatch.setattr(N, "Sequence", _StemSeq)
    monkeypatch.setattr(N, "SeqAutomation", _Auto)
    del _Auto.made[:]
    del _StemBuf.made[:]
    a = _stereo(1000, width) if nch == 2 else _mono(1000, width)
    cs = mixer.compile_tracks([[(0.0, a), (0.5, a, 0.5)], [], [(0.25, a)]], RATE, nch, width, name="tune")
    del _StemBuf.made[:]
    return cs


def _calls(cs, **kw):
    """the ways a keyword reaches a stems call"""
    return (lambda: cs.stems(**kw), lambda: cs.stems(3, 0, **kw), lambda: cs.stems_into(N.DeviceBuffer(100000), 0, 100, 0, 10, **kw))


# ---- what is handed on --------------------------------------------------------------------------------------------------------------------
def test_stems_hands_on_exactly_the_desks_keywords_and_the_stride(monkeypatch):
    cs = _song(monkeypatch)
    seq = cs._seq
    auto = cs.automation([[(0, 100, 0.5, 1.0)], None, None], master=[(0, 10, 0.5, 1.0)])
    got = cs.stems(10, 21, gains=(0.5, 1.0, 2.0), pans=(0.0, None, None), master=0.7, automation=auto, groups=[(0, 2, 0.5)])
    plain = cs.stems(10, 21)
    assert cs.stems_into(N.DeviceBuffer(100000), 6, 300, 3, 9, master=1.0, groups=[]) is None
    assert [(c[0], c[1], c[3], c[4], c[5]) for c in seq.stemmed] == [
        (20, 42, 0, 48, dict(gains=[0.5, 1.0, 2.0], pans=[0.5, 0.5, 1.0, 1.0, 1.0, 1.0], master=0.7, automation=_Auto.made[0], groups=[(0, 2, 0.5, 1.0, 1.0)])),
        (20, 42, 0, 48, dict(gains=None, pans=None, master=None, automation=None, groups=None)),
        (6, 18, 3, 600, dict(gains=None, pans=None, master=None, automation=None, groups=None))]
    assert seq.rendered == []                                   # one stems call each, and no render beside it
    # one buffer per call, of nrows planes of the stride; every Sample a view of it, in plane order
    first, second = seq.stemmed[0][2], seq.stemmed[1][2]
    assert first.nbytes == 5 * 24 * 4 and first.views == [(r * 24 * 4, 21 * 4) for r in range(5)] and first.parent is None
    assert second.nbytes == 4 * 24 * 4 and second.views == [(r * 24 * 4, 21 * 4) for r in range(4)]
    assert isinstance(got, mixer.SongStems) and len(got.tracks) == 3 and len(got.groups) == 1 and len(plain.groups) == 0 and len(got) == 5
    assert got.rows() == got.tracks + [got.master] + got.groups and (got.start_frame, got.frames) == (10, 21)
    assert [s.name for s in got.rows()] == ["tune:track 0", "tune:track 1", "tune:track 2", "tune:master", "tune:group 0"]
    for s in got.rows():
        assert (s.samplerate, s.nchannels, s.samplewidth) == (RATE, 2, 2) and len(s) == 21
    assert "3 tracks" in repr(got) and "[10, 31)" in repr(got)


def test_an_empty_window_gives_empty_samples_and_launches_nothing(monkeypatch):
    cs = _song(monkeypatch)
    e = cs.stems(3, 0, groups=[(0, 1, 0.5), (1, 3, 1.0)])
    assert len(e.tracks) == 3 and len(e.groups) == 2 and e.frames == 0 and all(len(s) == 0 for s in e.rows())
    assert cs.stems_into(N.DeviceBuffer(100), 0, 0, 3, 0) is None
    assert cs._seq.stemmed == [] and cs._seq.rendered == [] and len(_StemBuf.made) == 1      # (the one this test made)


@pytest.mark.parametrize("width", [1, 2, 3, 4])
@pytest.mark.parametrize("nch", [1, 2])
def test_the_stride_keeps_every_plane_aligned(monkeypatch, nch, width):
    cs = _song(monkeypatch, nch, width)
    for nframes in (1, 2, 3, 7, 8, 9, 15, 16, 17, 333, 1000):
        p = mixer.CompiledSequence.stems_plane_frames(nframes, nch, width)
        assert p >= nframes and (p * nch * width) % 16 == 0 and all((q * nch * width) % 16 for q in range(nframes, p)), (nframes, p)
        del cs._seq.stemmed[:]
        cs.stems(5, nframes)
        first, n, buf, out_sample, plane, _kw = cs._seq.stemmed[0]
        assert (first, n, out_sample, plane) == (5 * nch, nframes * nch, 0, p * nch) and buf.nbytes == 4 * p * nch * width
        assert all(off % 16 == 0 for off, _n in buf.views) and [off for off, _n in buf.views] == [r * plane * width for r in range(4)]


# ---- what is refused before any buffer is made ---------------------------------------------------------------------------------------------
def test_a_flat_song_has_no_stems(monkeypatch):
    _fake(monkeypatch)
    monkeypatch.setattr(N, "DeviceBuffer", _StemBuf)
    monkeypatch.setattr(N, "Sequence", _StemSeq)
    flat = mixer.compile_sequence([(0.0, _stereo())], RATE, 2)
    del _StemBuf.made[:]
    for call in (lambda: flat.stems(), lambda: flat.stems(3, 0), lambda: flat.stems(gains=(1.0,)), lambda: flat.stems_into(None, 0, 100, 0, 10)):
        with pytest.raises(ValueError, match=r"CompiledSequence: stems need a song of tracks \(compile_tracks\); this one has none"):
            call()
    assert flat._seq.stemmed == [] and flat._seq.rendered == [] and _StemBuf.made == []


@pytest.mark.parametrize("kw, message", [
    (dict(gains=(1.0, 0.5)), "2 gains for 3 tracks"),
    (dict(gains=(1.0, nan, 1.0)), "gain 1 is not finite"),
    (dict(gains="abc"), "gains is a sequence of numbers, one per track"),
    (dict(pans=(None, None)), "2 pans for 3 tracks"),
    (dict(pans=(None, 1.0001, None)), "pan 1 must be between -1 and 1"),
    (dict(pans=(None, (0.5,), None)), r"pan 1 is not a pair \(left_factor, right_factor\) of finite numbers"),
    (dict(master=inf), "master is not finite"),
    (dict(master="x"), "master is a number"),
    (dict(groups=[(0, 4, 1.0)]), r"group 0: tracks \[0, 4\) outside the song's 3 tracks"),
    (dict(groups=[(1, 1, 1.0)]), r"group 0: tracks \[1, 1\): an empty range"),
    (dict(groups=[(0, 2, 1.0), (1, 3, 1.0)]), "group 1: starts at track 1, before the group in front of it ends"),
    (dict(groups=[(0, 2, nan)]), "group 0: gain is not finite"),
    (dict(groups=[(0, 1, 1.0)] * 9), "9 groups, at most 8"),
    (dict(groups=0.5), "groups is a sequence"),
    (dict(automation="x"), r"automation is None or an Automation made by this song's automation\(\)"),
])
def test_the_desk_is_checked_before_any_buffer_is_made(monkeypatch, kw, message):
    cs = _song(monkeypatch)
    for call in (lambda: cs.stems(**kw), lambda: cs.stems(3, 0, **kw), lambda: cs.stems_into(None, 0, 100, 0, 10, **kw)):
        with pytest.raises(ValueError, match="CompiledSequence: " + message):
            call()
    assert cs._seq.stemmed == [] and cs._seq.rendered == [] and _StemBuf.made == []


def test_an_automation_of_another_song_a_ride_without_its_group_and_a_bad_window(monkeypatch):
    cs = _song(monkeypatch)
    other = _song(monkeypatch)
    foreign = other.automation([[(0, 100, 0.5, 1.0)], None, None])
    rides = cs.automation([None] * 3, groups=[None, [(0, 5, 0.5, 0.5)]])
    pans = cs.automation([None] * 3, group_pans=[[(0, 10, 0.5, -1.0)]])
    del _StemBuf.made[:]
    for call in (lambda: cs.stems(automation=foreign), lambda: cs.stems_into(None, 0, 100, 0, 10, automation=foreign)):
        with pytest.raises(ValueError, match=r"CompiledSequence: automation is None or an Automation made by this song's automation\(\)"):
            call()
    with pytest.raises(ValueError, match="the automation rides group 1, and this render names 1 groups"):
        cs.stems(automation=rides, groups=[(0, 1, 1.0)])
    with pytest.raises(ValueError, match="the automation rides the pan of group 0, and this render names 0 groups"):
        cs.stems(automation=pans)
    for call, message in ((lambda: cs.stems(-1), "start_frame -1 outside the song's"), (lambda: cs.stems(0, cs.frames + 1), r"frames \[0, 5001\) outside the song's 5000 frames"),
                          (lambda: cs.stems_into(None, 1, 100, 0, 10), "byte_offset 1 is not a whole number of 2-byte samples"),
                          (lambda: cs.stems_into(None, 0, 9, 0, 10), "planes 9 frames apart for a window of 10 frames")):
        with pytest.raises(ValueError, match="CompiledSequence: " + message):
            call()
    assert cs._seq.stemmed == [] and _StemBuf.made == []
    # a ride with its group, and pan rides: handed on (stems take every Automation the song can make)
    cs.stems(0, 8, automation=rides, groups=[(0, 1, 1.0), (1, 3, 0.5)])
    cs.stems(0, 8, automation=pans, groups=[(0, 1, 1.0)])
    assert [c[5]["automation"] for c in cs._seq.stemmed] == _Auto.made[-2:] and len(_StemBuf.made) == 2
    for bad in (dict(meters=True), dict(clips=True), dict(meters="history")):      # no meters= and no clips= on these calls
        with pytest.raises(TypeError):
            cs.stems(**bad)
        with pytest.raises(TypeError):
            cs.stems_into(None, 0, 100, 0, 10, **bad)


# ---- the binding and the header -----------------------------------------------------------------------------------------------------------
def test_the_binding_reaches_the_new_entry_point(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(N, "lib", lambda: lib)
    seq = N.Sequence.__new__(N.Sequence)
    seq._h, seq._sources, seq._width = C.c_void_p(1), [], 2

    class Out:
        handle = C.c_void_p(2)

    class Auto:
        handle = C.c_void_p(3)
    gains, pans, groups = [1.0, 2.0, 3.0], [0.5, 0.25, 1.0, 1.0, 0.0, -1.0], [(0, 1, 0.5, 1.0, 1.0), (1, 3, 1.0, 0.5, 0.25)]
    assert seq.stems(2040, 2060, Out, 7, 2064) is None
    assert seq.stems(4096, 2048, Out, 0, 2048, gains=gains, pans=pans, master=0.5, automation=Auto, groups=groups) is None
    calls = [c for c in lib.calls if c[0] != "sh_seq_get_tracks"]
    assert [c[0] for c in calls] == ["sh_seq_render_stems"] * 2 and [len(c[1]) for c in calls] == [15] * 2
    a = calls[0][1]
    assert (a[0].value, a[1], a[2], a[3].value, a[4], a[5], a[6]) == (1, 2040, 2060, 2, 7, 2064, 4) and a[7:] == (None, 0, None, 0, 1.0, None, None, 0)
    b = calls[1][1]
    assert (b[1], b[2], b[4], b[5], b[6]) == (4096, 2048, 0, 2048, 6) and (list(b[7]), b[8], list(b[9]), b[10], b[11], b[12].value, b[14]) == (
        gains, 3, pans, 6, 0.5, 3, 2)
    assert [(g.first, g.end, g.gain, g.left, g.right) for g in b[13]] == groups
    seq.free()


def test_the_new_symbol_is_declared_in_the_header_and_bound():
    table = N._SIGNATURES
    stems, groups = table["sh_seq_render_stems"][1], table["sh_seq_render_groups"][1]
    # sh_seq_render_groups' arguments with plane_samples and nplanes behind out_sample, and without the meters
    assert len(stems) == 15 and stems[:5] == groups[:5] and stems[5:7] == [C.c_size_t, C.c_uint32] and stems[7:12] == groups[5:10] and stems[12:] == groups[12:]
    assert table["sh_seq_render_stems"][0] == C.c_int
    header = (Path(__file__).resolve().parents[1] / "include" / "synthhip.h").read_text()
    assert "#define SH_ABI_VERSION 6" in header and N.SH_ABI_VERSION == 6
    m = re.search(r"int sh_seq_render_stems\(([^;]*)\);", header)
    assert m, "sh_seq_render_stems is not declared"
    params = [re.sub(r"/\*.*?\*/", "", p).split()[-1].lstrip("*") for p in m.group(1).replace("\n", " ").split(",")]
    assert params == ["seq", "first_sample", "nsamples", "out", "out_sample", "plane_samples", "nplanes", "gains", "ngains", "pans", "npans", "master_gain",
                      "automation", "groups", "ngroups"]
    source = (Path(__file__).resolve().parents[1] / "synthesizer_amd" / "csrc" / "sequence.hip").read_text()
    assert "int sh_seq_render_stems(" in source and '#include "seqstem.hpp"' in source


# ---- stem() is what it was ------------------------------------------------------------------------------------------------------------------
def test_stem_still_reaches_render_with_one_hot_gains(monkeypatch):
    cs = _song(monkeypatch)
    cs.stem(1, 10, 20)
    cs.stem(2)
    assert cs._seq.rendered == [(20, 40, 0, dict(gains=[0.0, 1.0, 0.0])), (0, 2 * cs.frames, 0, dict(gains=[0.0, 0.0, 1.0]))]
    assert cs._seq.stemmed == []
