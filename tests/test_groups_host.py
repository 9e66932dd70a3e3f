"""What the ``groups`` keyword of a compiled song of tracks needs of the host alone (no GPU): every check and message raised before the
native layer is reached, the form the list is handed on in, and that ``None`` / an empty list leave the entry points there were to be
called with the keywords they got before.  The bytes: tests/test_gpu_groups.py."""
import ctypes as C
from pathlib import Path

import pytest

from synthesizer_amd import _native as N
from synthesizer_amd import mixer
from tests.songhost import RATE, _calls, _fake, _Lib, _mono, _Seq, _stereo

nan, inf = float("nan"), float("inf")


class _Seq6(_Seq):
    def render(self, first_sample, nsamples, out, out_sample=0, **kw):
        self.rendered.append((first_sample, nsamples, out_sample, kw))
        if kw.get("meters"):
            return [((0, 0), (0, 0))] * (7 + len(kw.get("groups") or ()))


def _song(monkeypatch, nch=2):
    """six tracks"""
    _fake(monkeypatch)
    monkeypatch.setattr(N, "Sequence", _Seq6)
    a = _stereo(1000) if nch == 2 else _mono(1000)
    return mixer.compile_tracks([[(0.0, a), (0.5, a, 0.5)], [], [(0.25, a)], [(0.1, a)], [], [(0.3, a, 0.7)]], RATE, nch)


@pytest.mark.parametrize("bad, message", [
    (5, r"groups is a sequence of \(first_track, end_track, gain\) or \(first_track, end_track, gain, pan\)"),
    ("abc", r"groups is a sequence of \(first_track, end_track, gain\)"),
    ([(0, 1, 1.0)] * 9, "9 groups, at most 8"),
    ([(0, 2)], r"group 0: an entry is \(first_track, end_track, gain\) or \(first_track, end_track, gain, pan\)"),
    ([(0, 2, 1.0, None, 3)], r"group 0: an entry is \(first_track, end_track, gain\)"),
    ([(0, 2, 1.0), 7], r"group 1: an entry is \(first_track, end_track, gain\)"),
    ([(0, 2, 1.0), "abc"], r"group 1: an entry is \(first_track, end_track, gain\)"),
    ([(0.0, 2, 1.0)], "group 0: first_track and end_track are integers"),
    ([(0, 2.5, 1.0)], "group 0: first_track and end_track are integers"),
    ([(0, True, 1.0)], "group 0: first_track and end_track are integers"),
    ([(0, "2", 1.0)], "group 0: first_track and end_track are integers"),
    ([(-1, 2, 1.0)], r"group 0: tracks \[-1, 2\) outside the song's 6 tracks"),
    ([(0, 2, 1.0), (4, 7, 1.0)], r"group 1: tracks \[4, 7\) outside the song's 6 tracks"),
    ([(2, 2, 1.0)], r"group 0: tracks \[2, 2\): an empty range"),
    ([(3, 1, 1.0)], r"group 0: tracks \[3, 1\): an empty range"),
    ([(0, 3, 1.0), (2, 4, 1.0)], r"group 1: starts at track 2, before the group in front of it ends \(3\)"),
    ([(3, 5, 1.0), (0, 2, 1.0)], r"group 1: starts at track 0, before the group in front of it ends \(5\)"),
    ([(0, 2, nan)], "group 0: gain is not finite"),
    ([(0, 2, 1.0), (2, 3, -inf)], "group 1: gain is not finite"),
    ([(0, 2, "x")], "group 0: gain is None or a finite number"),
    ([(0, 2, (1.0,))], "group 0: gain is None or a finite number"),
    ([(0, 2, 1.0, 1.5)], "group 0: pan must be between -1 and 1"),
    ([(0, 2, 1.0, nan)], "group 0: pan must be between -1 and 1"),
    ([(0, 2, 1.0, "x")], r"group 0: pan is None, a number or a pair \(left_factor, right_factor\)"),
    ([(0, 2, 1.0, (0.5,))], r"group 0: pan is not a pair \(left_factor, right_factor\) of finite numbers"),
    ([(0, 2, 1.0, (0.5, inf))], r"group 0: pan is not a pair \(left_factor, right_factor\) of finite numbers"),
    ([(0, 2, 1.0, (None, 0.5))], r"group 0: pan is not a pair \(left_factor, right_factor\) of finite numbers"),
])
def test_groups_are_checked_before_anything_is_rendered(monkeypatch, bad, message):
    cs = _song(monkeypatch)
    for call in _calls(cs, groups=bad) + _calls(cs, groups=bad, gains=(1.0,) * 6, master=0.5, meters=True):
        with pytest.raises(ValueError, match="CompiledSequence: " + message):
            call()
    assert cs._seq.rendered == []


def test_a_song_without_tracks_and_a_song_that_is_not_stereo(monkeypatch):
    _fake(monkeypatch)
    monkeypatch.setattr(N, "Sequence", _Seq6)
    flat = mixer.compile_sequence([(0.0, _stereo())], RATE, 2)
    for call in _calls(flat, groups=[(0, 1, 0.5)]) + _calls(flat, groups=[]):
        with pytest.raises(ValueError, match=r"CompiledSequence: groups need a song of tracks \(compile_tracks\); this one has none"):
            call()
    assert flat._seq.rendered == []
    mono = _song(monkeypatch, nch=1)
    for bad in ([(0, 2, 0.5, 0.3)], [(0, 2, 0.5), (2, 3, 1.0, (1.0, 1.0))]):
        for call in _calls(mono, groups=bad):
            with pytest.raises(ValueError, match="CompiledSequence: group [01]: a pan needs a stereo song, this one has 1 channels"):
                call()
    assert mono._seq.rendered == []
    mono.render(2, 5, groups=[(0, 2, 0.5), (2, 3, None, None)])    # a mono song has group faders
    assert mono._seq.rendered == [(2, 5, 0, dict(gains=None, pans=None, master=None, groups=[(0, 2, 0.5, 1.0, 1.0), (2, 3, 1.0, 1.0, 1.0)]))]


def test_what_render_hands_on(monkeypatch):
    cs = _song(monkeypatch)
    seq = cs._seq
    # None and an empty list: the calls there were, with the keywords they got before
    cs.render(10, 20)
    cs.render(10, 20, groups=None)
    cs.render(10, 20, groups=[])
    cs.render(10, 20, groups=(), gains=(0.5, 1.0, 2.0, 1.0, 1.0, 1.0))
    cs.render(10, 20, groups=[], gains=(0.5, 1.0, 2.0, 1.0, 1.0, 1.0), meters=True)
    cs.render(10, 20, groups=None, master=0.7)
    assert seq.rendered == [(20, 40, 0, {}), (20, 40, 0, {}), (20, 40, 0, {}), (20, 40, 0, dict(gains=[0.5, 1.0, 2.0, 1.0, 1.0, 1.0])),
                            (20, 40, 0, dict(gains=[0.5, 1.0, 2.0, 1.0, 1.0, 1.0], meters=True)), (20, 40, 0, dict(gains=None, pans=None, master=0.7))]
    del seq.rendered[:]
    # a list: five numbers per entry -- integers, the gain (None: 1.0), the two factors ((1.0, 1.0) without a pan; Sample.pan's of a number)
    import numpy as np
    cs.render(10, 20, groups=[(0, 2, 0.5), (np.int64(2), 3, None, 0.3), [4, 6, 2, (1.5, -0.25)]])
    cs.render_into(N.DeviceBuffer(100), 4, 3, 9, gains=(0.0, 1.0, 1.0, 1.0, 1.0, 1.0), pans=(1.0,) + (None,) * 5, master=0.7, groups=[(0, 6, 0.9, None)])
    out, levels = cs.render(0, 8, groups=[(1, 2, 1.0), (5, 6, 0.0, -1.0)], meters=True)
    list(cs.chunks(cs.frames - 1, groups=[(0, 1, -1.5, 0.0)]))
    assert seq.rendered == [
        (20, 40, 0, dict(gains=None, pans=None, master=None,
                         groups=[(0, 2, 0.5, 1.0, 1.0), (2, 3, 1.0, (1.0 - 0.3) / 2.0, (1.0 + 0.3) / 2.0), (4, 6, 2.0, 1.5, -0.25)])),
        (6, 18, 2, dict(gains=[0.0, 1.0, 1.0, 1.0, 1.0, 1.0], pans=[0.0, 1.0] + [1.0] * 10, master=0.7, groups=[(0, 6, 0.9, 1.0, 1.0)])),
        (0, 16, 0, dict(gains=None, meters=True, pans=None, master=None, groups=[(1, 2, 1.0, 1.0, 1.0), (5, 6, 0.0, 1.0, 0.0)])),
        (0, 2 * cs.frames - 2, 0, dict(gains=None, pans=None, master=None, groups=[(0, 1, -1.5, 0.5, 0.5)])),
        (2 * cs.frames - 2, 2, 0, dict(gains=None, pans=None, master=None, groups=[(0, 1, -1.5, 0.5, 0.5)])),
    ]
    handed = seq.rendered[0][3]["groups"]
    assert all(type(g[0]) is int and type(g[1]) is int and all(type(f) is float for f in g[2:]) for g in handed)
    assert isinstance(levels, mixer.SongLevels) and len(levels.tracks) == 6 and len(levels.groups) == 2
    assert "groups=" in repr(levels)
    # an empty window of a metered render: zero rows for the groups as well, nothing launched
    del seq.rendered[:]
    out, levels = cs.render(3, 0, groups=[(1, 2, 1.0), (5, 6, 0.5)], meters=True)
    assert seq.rendered == [] and len(levels.tracks) == 6 and len(levels.groups) == 2 and levels.groups[0].peak == (0, 0)
    # without groups the levels are what they were
    out, levels = cs.render(0, 8, meters=True)
    assert levels.groups == [] and repr(levels) == "SongLevels(tracks=%r, master=%r)" % (levels.tracks, levels.master)
    cs.close()
    for call in _calls(cs, groups=[(0, 1, 0.5)]):
        with pytest.raises(ValueError, match="closed"):
            call()


def test_the_binding_calls_the_new_entry_point_only_when_groups_are_given(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(N, "lib", lambda: lib)
    seq = N.Sequence.__new__(N.Sequence)
    seq._h, seq._sources = C.c_void_p(1), []

    class Out:
        handle = C.c_void_p(2)
    seq.render(5, 6, Out, 7, groups=None)
    seq.render(5, 6, Out, 7, gains=[1.0, 2.0, 3.0], groups=[])
    seq.render(5, 6, Out, 7, gains=[1.0, 2.0, 3.0], master=0.5, groups=None)
    assert [c[0] for c in lib.calls] == ["sh_seq_render", "sh_seq_render_gains", "sh_seq_render_desk"]
    del lib.calls[:]
    assert seq.render(5, 6, Out, 7, groups=[(0, 2, 0.5, 1.0, 1.0)]) is None
    rows = seq.render(5, 6, Out, 7, gains=[1.0, 2.0, 3.0], pans=[0.5, 0.25, 1.0, 1.0, 0.0, -1.0], master=-1.3, meters=True,
                      groups=[(0, 1, 1.0, 0.5, 0.25), (1, 3, -2.0, 1.0, 1.0)])
    assert rows == [((0, 0), (0, 0))] * 6                       # three tracks, the master, two groups
    calls = [c for c in lib.calls if c[0] != "sh_seq_get_tracks"]
    assert [c[0] for c in calls] == ["sh_seq_render_groups"] * 2
    a, b = (c[1] for c in calls)
    assert a[1:3] == b[1:3] == (5, 6) and a[4] == b[4] == 7
    assert (a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[14]) == (None, 0, None, 0, 1.0, None, 0, None, 1)
    assert [(g.first, g.end, g.gain, g.left, g.right) for g in a[13]] == [(0, 2, 0.5, 1.0, 1.0)]
    assert (list(b[5]), b[6], list(b[7]), b[8], b[9], len(b[10]), b[11], b[12], b[14]) == ([1.0, 2.0, 3.0], 3, [0.5, 0.25, 1.0, 1.0, 0.0, -1.0], 6, -1.3, 6, 6, None, 2)
    assert [(g.first, g.end, g.gain, g.left, g.right) for g in b[13]] == [(0, 1, 1.0, 0.5, 0.25), (1, 3, -2.0, 1.0, 1.0)]
    seq.free()                                                  # (while the library is the fake one: the handle is no sh_seq)


def test_the_new_symbol_is_declared_beside_the_one_it_extends():
    table = N._SIGNATURES
    groups, auto = table["sh_seq_render_groups"][1], table["sh_seq_render_auto"][1]
    assert len(groups) == 15 and groups[:13] == auto and groups[13:] == [C.POINTER(N.SeqGroup), C.c_uint32]
    assert C.sizeof(N.SeqGroup) == 32 and N.SeqGroup.gain.offset == 8 and N.SeqGroup.right.offset == 24 and N.SEQ_MAX_GROUPS == 8
    header = (Path(__file__).resolve().parents[1] / "include" / "synthhip.h").read_text()
    assert "int sh_seq_render_groups(" in header and "#define SH_SEQ_MAX_GROUPS 8u" in header and "#define SH_ABI_VERSION 6" in header
    assert mixer.CompiledSequence.MAX_GROUPS == 8
