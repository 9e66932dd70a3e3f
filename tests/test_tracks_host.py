"""What mixer.compile_tracks and the ``gains`` keyword need of the host alone (no GPU): every check and message raised before the library
is even loaded, an error naming the track and the event's index in its own list, the tables handed to sh_seq_create_tracks (the tracks'
events one track behind the other, where each track starts), and what render hands on.  shq::plan_runs: tests/test_seqruns.py."""
from pathlib import Path

import numpy as np
import pytest

from synthesizer_amd import _native as N
from synthesizer_amd import mixer
from synthesizer_amd.sample import Sample
from tests.songhost import RATE, _fake, _mono, _stereo
from tests.test_channels_host import _ev
from tests.test_enveloped_host import _no_library

nan, inf = float("nan"), float("inf")


def test_the_number_of_tracks_is_checked_before_the_library_is_loaded(monkeypatch):
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match="compile_tracks: a song needs at least one track"):
        mixer.compile_tracks([], RATE, 1)
    with pytest.raises(ValueError, match="compile_tracks: 33 tracks, at most 32"):
        mixer.compile_tracks([[(0.0, _mono())]] * 33, RATE, 1)
    with pytest.raises(ValueError, match="compile_tracks: tracks is a sequence of event lists"):
        mixer.compile_tracks(5, RATE, 1)
    assert mixer.CompiledSequence.MAX_TRACKS == 32


@pytest.mark.parametrize("what, nch, event, error, message", [
    ("a negative time", 1, lambda: _ev(-0.1, _mono(), None), ValueError, "mix_at_many: negative time"),
    ("a volume that is no number", 1, lambda: _ev(0.1, _mono(), None, volume=nan), ValueError, "mix_at_many: volume is not finite"),
    ("a speed outside 0.1 .. 10", 1, lambda: _ev(0.1, _mono(), None, speed=11.0), ValueError, "mix_at_many: speed must be"),
    ("a pan into a mono song", 1, lambda: _ev(0.1, _mono(), None, pan=0.3), ValueError, "mix_at_many: pan needs a stereo track"),
    ("a sustain level above 1", 1, lambda: _ev(0.1, _mono(), None, envelope=(0.01, 0.01, 1.5, 0.01)), ValueError, "mix_at_many: envelope: sustainlevel"),
    ("a loop without a frame", 1, lambda: _ev(0.1, _mono(), None, loop=(0.05, 0.05, 1.0)), ValueError, "mix_at_many: loop"),
    ("a region that ends before it starts", 1, lambda: _ev(0.1, _mono(), None, region=(0.05, 0.01)), ValueError, "mix_at_many: region"),
    ("channels on a mono sample", 1, lambda: _ev(0.1, _mono(), (0.5, 0.5)), ValueError, "mix_at_many: channels needs a stereo sample"),
    ("pan and channels", 2, lambda: _ev(0.1, _stereo(), (0.5, 0.5), pan=0.3), ValueError, "mix_at_many: pan and channels"),
])
def test_an_error_names_the_track_and_the_events_index_in_its_own_list(monkeypatch, what, nch, event, error, message):
    _no_library(monkeypatch)
    good = _ev(0.0, _stereo(), (0.5, 0.25), 0.5) if nch == 1 else _ev(0.0, _stereo(), None, 0.5)
    with pytest.raises(error, match="compile_tracks: track 2, event 1: " + message):
        mixer.compile_tracks([[good, good, good], [], [good, event(), event()], [event()]], RATE, nch)
    with pytest.raises(error, match="compile_tracks: track 0, event 0: " + message):
        mixer.compile_tracks([[event()]], RATE, nch)
    with pytest.raises(error, match="^" + message):                      # the same check, in the words of the call it stands beside
        mixer.sequence([good, event()], RATE, nch)


def test_what_sequence_refuses_for_the_format_compile_tracks_refuses(monkeypatch):
    _no_library(monkeypatch)
    s3 = Sample.from_raw_frames(bytes(3 * 100), 3, RATE, 1)
    with pytest.raises(NotImplementedError, match="compile_tracks: track 1, event 0: mix_at_many: envelope: 3-byte samples"):
        mixer.compile_tracks([[(0.0, s3)], [(0.0, s3, None, None, None, None, (0.001, 0.001, 0.5, 0.001))]], RATE, 1, 3)
    with pytest.raises(AssertionError):                                  # mix_at's assertion stays an assertion
        mixer.compile_tracks([[(0.0, _stereo())]], RATE, 1)


class _Seq:
    made = []

    def __init__(self, sources, table, segments, width, nchannels, track_samples, track_first=None):
        self.made.append((sources, table.copy(), None if segments is None else segments.copy(), width, nchannels, track_samples, track_first))
        self.rendered = []

    def info(self):
        return {"level": 0, "device_bytes": 0}

    def render(self, first_sample, nsamples, out, out_sample=0, gains=None):
        self.rendered.append((first_sample, nsamples, out_sample, gains))

    def free(self):
        pass


def _tracks_song(monkeypatch):
    _fake(monkeypatch)
    monkeypatch.setattr(N, "Sequence", _Seq)
    _Seq.made.clear()
    a, b = _mono(1000), _mono(700)
    tracks = [[(0.0, a), (0.5, b, 0.5)], [], [(0.25, a, None, 0.01), (0.0, a, None, None, None, None, (0.01, 0.01, 0.5, 0.01, 0.05))], [(1.0, b, -1.0)]]
    return a, b, tracks, mixer.compile_tracks(tracks, RATE, 1, name="song")


def test_the_tables_are_the_flat_lists_and_track_first_says_where_the_tracks_start(monkeypatch):
    a, b, tracks, cs = _tracks_song(monkeypatch)
    sources, table, segments, width, nchannels, track_samples, track_first = _Seq.made[-1]
    assert track_first == [0, 2, 2, 4, 5] and cs.ntracks == 4 and cs.name == "song"
    flat = mixer.compile_sequence([e for t in tracks for e in t], RATE, 1)
    assert flat.ntracks is None and _Seq.made[-1][6] is None              # compile_sequence's call has no track_first at all
    f_sources, f_table, f_segments = _Seq.made[-1][:3]
    assert table.dtype == N.MIX_EVENT_CHAN_DTYPE and len(table) == len(f_table) == 5 and segments.tobytes() == f_segments.tobytes()
    for f in table.dtype.names:
        assert table[f].tolist() == f_table[f].tolist(), f
    assert len(sources) == len(f_sources) == 2 and (width, nchannels) == (2, 1)
    assert track_samples == cs.frames == flat.frames == RATE + 700        # the song is as long as its longest track
    # a track's own length does not matter, nor does an empty song
    cs = mixer.compile_tracks([[], []], RATE, 2)
    assert cs.ntracks == 2 and cs.frames == 0 and _Seq.made[-1][6] == [0, 0, 0] and len(_Seq.made[-1][1]) == 0
    assert len(cs.render(gains=(0.5, 2.0))) == 0 and list(cs.chunks(10, gains=(0.5, 2.0))) == []


def test_gains_are_checked_and_handed_on_as_floats(monkeypatch):
    a, b, tracks, cs = _tracks_song(monkeypatch)
    seq = cs._seq
    for bad, message in (((1.0, 1.0, 1.0), "3 gains for 4 tracks"), ((1.0,) * 5, "5 gains for 4 tracks"), ((), "0 gains for 4 tracks"),
                         ((1.0, nan, 1.0, 1.0), "gain 1 is not finite"), ((1.0, 1.0, 1.0, -inf), "gain 3 is not finite"),
                         ((1.0, "x", 1.0, 1.0), "gains is a sequence of numbers"), (0.5, "gains is a sequence of numbers")):
        with pytest.raises(ValueError, match="CompiledSequence: " + message):
            cs.render(gains=bad)
        with pytest.raises(ValueError, match="CompiledSequence: " + message):
            cs.render_into(N.DeviceBuffer(100), 0, 0, 10, gains=bad)
        with pytest.raises(ValueError, match="CompiledSequence: " + message):
            next(cs.chunks(100, gains=bad))
    for bad in (-1, 4, 32):
        with pytest.raises(ValueError, match="CompiledSequence: track %d outside the song's 4 tracks" % bad):
            cs.stem(bad)
    assert seq.rendered == []                                             # nothing of the above reached a render
    cs.render(10, 20, gains=[0.5, 1, np.float32(2.0), -1.7])
    cs.render(10, 20)
    cs.stem(2, 5, 7)
    cs.render_into(N.DeviceBuffer(100), 4, 3, 9, gains=(0.0, 0.0, 0.0, 0.0))
    list(cs.chunks(cs.frames - 1, gains=(1.0, 1.0, 1.0, 1.0)))
    assert seq.rendered == [(10, 20, 0, [0.5, 1.0, 2.0, -1.7]), (10, 20, 0, None), (5, 7, 0, [0.0, 0.0, 1.0, 0.0]), (3, 9, 2, [0.0] * 4),
                            (0, cs.frames - 1, 0, [1.0] * 4), (cs.frames - 1, 1, 0, [1.0] * 4)]
    assert all(type(g) is float for r in seq.rendered if r[3] for g in r[3])
    cs.close()
    for call in (lambda: cs.render(gains=(1.0,) * 4), lambda: cs.stem(0), lambda: next(cs.chunks(10, gains=(1.0,) * 4)),
                 lambda: cs.render_into(N.DeviceBuffer(100), 0, 0, 10, gains=(1.0,) * 4)):
        with pytest.raises(ValueError, match="closed"):
            call()


def test_a_song_without_tracks_takes_no_gains(monkeypatch):
    _fake(monkeypatch)
    monkeypatch.setattr(N, "Sequence", _Seq)
    cs = mixer.compile_sequence([(0.0, _mono())], RATE, 1)
    assert cs.ntracks is None
    with pytest.raises(ValueError, match="CompiledSequence: gains need a song of tracks"):
        cs.render(gains=(1.0,))
    with pytest.raises(ValueError, match="CompiledSequence: gains need a song of tracks"):
        next(cs.chunks(10, gains=()))
    with pytest.raises(ValueError, match="CompiledSequence: stem needs a song of tracks"):
        cs.stem(0)
    assert cs._seq.rendered == []
    cs.render(3, 4)                                                       # and without the keyword it is what it was
    assert cs._seq.rendered == [(3, 4, 0, None)]


def test_the_new_symbols_are_declared_beside_the_ones_they_extend():
    import ctypes as C
    table = N._SIGNATURES
    assert [len(table[s][1]) for s in ("sh_seq_create_tracks", "sh_seq_render_gains", "sh_seq_get_tracks")] == [12, 7, 3]
    assert table["sh_seq_create_tracks"][1][:4] == table["sh_seq_create"][1][:4] and table["sh_seq_create_tracks"][1][6:] == table["sh_seq_create"][1][4:]
    assert table["sh_seq_render_gains"][1][:5] == table["sh_seq_render"][1] and table["sh_seq_render_gains"][1][5] == C.POINTER(C.c_double)
    header = (Path(__file__).resolve().parents[1] / "include" / "synthhip.h").read_text()
    assert "#define SH_SEQ_MAX_TRACKS 32u" in header and "#define SH_ABI_VERSION 6" in header
    for s in ("sh_seq_create_tracks", "sh_seq_render_gains", "sh_seq_get_tracks"):
        assert "int %s(" % s in header
