"""What mixer.compile_sequence needs of the host alone (no GPU): sh_seq_info as the header lays it out against the ctypes mirror, every
ValueError / NotImplementedError of Sample.mix_at_many raised by compile_sequence too, before the library is even loaded, and the table it
hands sh_seq_create: sh_mix_event_chan's layout whatever the list holds, the rows being those mix_at_many packs for the same list."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from synthesizer_amd import _native as N
from synthesizer_amd import mixer
from synthesizer_amd.sample import Sample
from tests.songhost import RATE, _fake, _mono, _stereo
from tests.test_abi import HEADER
from tests.test_channels_host import _ev
from tests.test_enveloped_host import _no_library

nan, inf = float("nan"), float("inf")


def test_the_info_struct_matches_the_header(tmp_path):
    fields = [n for n, _t in N.SeqInfo._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%%zu %s\\n", sizeof(sh_seq_info), %s);return 0;}\n'
                   % (HEADER, " ".join(["%zu"] * len(fields)), ", ".join("offsetof(sh_seq_info, %s)" % f for f in fields)))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(N.SeqInfo)] + [getattr(N.SeqInfo, f).offset for f in fields] == [40, 0, 8, 16, 24, 28, 32, 36]
    assert N.SEQ_LEVELS == ("plain", "rate", "pan", "env", "loop", "rev", "chan")


@pytest.mark.parametrize("what, nch, event, error", [
    ("a negative time", 1, lambda: _ev(-0.1, _mono(), None), ValueError),
    ("a volume that is no number", 1, lambda: _ev(0.1, _mono(), None, volume=nan), ValueError),
    ("a speed outside 0.1 .. 10", 1, lambda: _ev(0.1, _mono(), None, speed=11.0), ValueError),
    ("a pan on a stereo sample", 2, lambda: _ev(0.1, _stereo(), None, pan=0.3), ValueError),
    ("a pan into a mono song", 1, lambda: _ev(0.1, _mono(), None, pan=0.3), ValueError),
    ("a pan outside -1 .. 1", 2, lambda: _ev(0.1, _mono(), None, pan=1.5), ValueError),
    ("an envelope of three numbers", 1, lambda: _ev(0.1, _mono(), None, envelope=(0.01, 0.01, 0.5)), ValueError),
    ("a sustain level above 1", 1, lambda: _ev(0.1, _mono(), None, envelope=(0.01, 0.01, 1.5, 0.01)), ValueError),
    ("a loop without a frame", 1, lambda: _ev(0.1, _mono(), None, loop=(0.05, 0.05, 1.0)), ValueError),
    ("a region that ends before it starts", 1, lambda: _ev(0.1, _mono(), None, region=(0.05, 0.01)), ValueError),
    ("channels of one number", 1, lambda: _ev(0.1, _stereo(), (0.5,)), ValueError),
    ("channels that are no numbers", 2, lambda: _ev(0.1, _stereo(), (inf, 0.5)), ValueError),
    ("channels on a mono sample", 1, lambda: _ev(0.1, _mono(), (0.5, 0.5)), ValueError),
    ("pan and channels", 2, lambda: _ev(0.1, _stereo(), (0.5, 0.5), pan=0.3), ValueError),
])
def test_compile_sequence_refuses_before_the_library_is_loaded(monkeypatch, what, nch, event, error):
    _no_library(monkeypatch)
    good = _ev(0.0, _stereo(), (0.5, 0.25), 0.5) if nch == 1 else _ev(0.0, _stereo(), None, 0.5)
    with pytest.raises(error, match="mix_at_many"):
        mixer.compile_sequence([good, event()], RATE, nch)
    with pytest.raises(error, match="mix_at_many"):                      # the same check as the call it stands beside
        mixer.sequence([good, event()], RATE, nch)


def test_what_sequence_refuses_for_the_format_compile_sequence_refuses(monkeypatch):
    _no_library(monkeypatch)
    s3 = Sample.from_raw_frames(bytes(3 * 100), 3, RATE, 1)
    with pytest.raises(NotImplementedError, match="3-byte samples"):
        mixer.compile_sequence([(0.0, s3, None, None, None, None, (0.001, 0.001, 0.5, 0.001))], RATE, 1, 3)
    four = Sample.from_raw_frames(bytes(8 * 100), 2, RATE, 4)
    with pytest.raises(ValueError, match="mix_at_many: channels"):
        mixer.compile_sequence([_ev(0.1, _stereo(), (1.0, 1.0))], RATE, 4)
    with pytest.raises(AssertionError):                                  # mix_at's assertion: a stereo sample in a mono song without channels
        mixer.compile_sequence([(0.0, _stereo())], RATE, 1)
    with pytest.raises(AssertionError):
        mixer.compile_sequence([(0.0, four)], RATE, 2)
    rate = 2 ** 20                                                       # a downmix the kernels cannot address
    s = Sample.from_raw_frames(bytes(2 * 100), 1, rate, 2)
    with pytest.raises(ValueError, match="mix_at_many: channels"):
        mixer.compile_sequence([_ev((2 ** 31 - 32768 - 99) / rate, s, (0.5, 0.5))], rate, 1, 1)


class _Seq:
    made = []

    def __init__(self, sources, table, segments, width, nchannels, track_samples):
        self.made.append((sources, table.copy(), None if segments is None else segments.copy(), width, nchannels, track_samples))

    def info(self):
        return {"level": 0}

    def free(self):
        pass


def test_the_table_is_the_one_mix_at_many_packs_in_the_widest_layout(monkeypatch):
    lib = _fake(monkeypatch)
    monkeypatch.setattr(N, "Sequence", _Seq)
    _Seq.made.clear()
    a, b = _mono(1000), _mono(700)
    lists = {
        "plain": [(0.0, a), (0.5, b, 0.5), (0.25, a, None, 0.01)],
        "rate": [(0.0, a, None, None, 1.5), (0.5, b, 0.5)],
        "env": [(0.0, a, None, None, None, None, (0.01, 0.01, 0.5, 0.01, 0.05)), (0.5, b, 0.5, None, 2.0)],
        "loop": [(0.0, a, None, None, None, None, None, (0.01, 0.02, 0.5)), (0.5, b)],
        "rev": [(0.0, a, None, None, None, None, None, None, (0.01, 0.05), True), (0.5, b)],
    }
    for what, events in lists.items():
        lib.tables.clear()
        lib.segments.clear()
        whole = mixer.sequence(events, RATE, 1)
        cs = mixer.compile_sequence(events, RATE, 1, name=what)
        sources, table, segments, width, nchannels, track_samples = _Seq.made[-1]
        assert table.dtype == N.MIX_EVENT_CHAN_DTYPE and (width, nchannels) == (2, 1) and len(sources) == 2, what
        assert track_samples == len(whole) == cs.frames == len(cs) and cs.duration == cs.frames / RATE and cs.name == what
        (theirs,) = lib.tables                                           # what mix_at_many handed its entry point for the same list
        for f in theirs.dtype.names:
            assert table[f].tolist() == theirs[f].tolist(), (what, f)
        assert (table["inrate"] != 0).all() and (table["outrate"] == RATE).all() and (table["src_channels"] == 1).all(), what
        if lib.segments:
            assert segments.tobytes() == lib.segments[0].tobytes(), what
    # an empty list is a song of no frames
    cs = mixer.compile_sequence([], RATE, 2)
    assert cs.frames == 0 and len(_Seq.made[-1][1]) == 0 and _Seq.made[-1][5] == 0
    assert len(cs.render()) == 0 and list(cs.chunks(10)) == []
    with pytest.raises(ValueError, match="CompiledSequence"):
        cs.render(1)
    with pytest.raises(ValueError, match="chunk_frames"):
        next(cs.chunks(0))
