"""What the level history of plain PCM -- ``mixer.level_history`` / ``Sample.level_history``, ``SongStems.level_history``,
``CompiledSequence.level_history``, ``N.pcm_level_blocks``, sh_pcm_level_blocks -- needs of the host alone (no GPU; the fake native layer
of tests/test_stems_host.py): what is refused before anything is launched, that an empty window gives an empty history and launches
nothing, that a ``SongStems`` that knows its buffer makes ONE call over all planes and one built by hand one call per row, that
``CompiledSequence.level_history`` is ``stems`` and then that, that ``meters="history"`` with a ride still raises what it raised, and that
the new symbol is declared in the header and bound.  The levels: tests/test_gpu_level_blocks.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from synthesizer_amd import _native as N
from synthesizer_amd import mixer
from synthesizer_amd.sample import Sample
from tests.songhost import RATE, _Auto, _fake, _Lib, _mono, _StemBuf, _stereo
from tests.test_stems_host import _song


def _record(monkeypatch):
    """N.pcm_level_blocks without a device: what each call was handed, and a table of the right shape whose peaks say which row they are"""
    calls = []

    def fake(buf, sample_offset, nframes, nch, width, plane_samples, nplanes, origin_frame, block_frames):
        calls.append((buf, sample_offset, nframes, nch, width, plane_samples, nplanes, origin_frame, block_frames))
        nblocks = (origin_frame + nframes - 1) // block_frames - origin_frame // block_frames + 1 if nframes > 0 else 0
        blocks = np.zeros((nblocks, nplanes), dtype=N.SEQ_METER_DTYPE)
        blocks["peak"][:, :, 0] = 100 * (len(calls) - 1) + np.arange(nplanes)[None, :] + 1
        blocks["sq_lo"][:, :, 0] = np.arange(nblocks)[:, None] + 1
        blocks["sq_hi"][:, :, 0] = 1
        return blocks
    monkeypatch.setattr(N, "pcm_level_blocks", fake)
    return calls


# ---- a Sample ------------------------------------------------------------------------------------------------------------------------------
def test_a_samples_history_is_one_call_over_its_buffer(monkeypatch):
    _fake(monkeypatch)
    calls = _record(monkeypatch)
    s = _stereo(1000, 4)
    h = s.level_history(300, origin_frame=250)
    assert isinstance(h, mixer.SongHistory) and len(calls) == 1
    assert calls[0] == (s._device(), 0, 1000, 2, 4, 2000, 1, 250, 300)
    assert (h.nblocks, h.block_frames, h.first_block, h.start_frame, h.frames, h.ngroups) == (5, 300, 0, 250, 1000, 0)
    assert h.starts == [250, 300, 600, 900, 1200] and h.block_counts == [50, 300, 300, 300, 50]
    assert (h.samplewidth, h.nchannels, h.samplerate) == (4, 2, RATE) and h.peak.shape == (5, 1, 2)
    assert h[2].tracks == [] and h[2].groups == [] and h[2].master == mixer.Levels((1, 0), ((1 << 32) + 3, 0), 300, 4, 2, RATE)
    assert h.total().master.sum_squares == ((5 << 32) + 15, 0) and h.fold(2).block_counts == [350, 600, 50]
    m = mixer.level_history(_mono(77), 1000)                     # a mono Sample: left == right, as Levels has it; the default origin
    assert calls[1][2:] == (77, 1, 2, 77, 1, 0, 1000) and m[0].master.peak == (101, 101) and m.peaks()[0, 0].tolist() == [101, 101]


@pytest.mark.parametrize("bad", [0, -3, 1.5, "64", None, True])
def test_block_frames_is_a_positive_int(monkeypatch, bad):
    _fake(monkeypatch)
    calls = _record(monkeypatch)
    for call in (lambda: mixer.level_history(_stereo(10), bad), lambda: _stereo(10).level_history(bad)):
        with pytest.raises(ValueError, match="level_history: block_frames is a positive int"):
            call()
    if bad is not None:                                         # (None is a SongStems' default block)
        st = mixer.SongStems([], _stereo(10), [], 0, 10)
        with pytest.raises(ValueError, match="SongStems: block_frames is a positive int"):
            st.level_history(bad)
    assert calls == []


def test_the_origin_and_the_format_are_checked_before_anything_is_launched(monkeypatch):
    _fake(monkeypatch)
    calls = _record(monkeypatch)
    for bad in (-1, 0.5, "0", None, False):
        with pytest.raises(ValueError, match="level_history: origin_frame is a non-negative int"):
            mixer.level_history(_stereo(10), 4, bad)
    three = Sample.from_raw_frames(bytes(2 * 3 * 10), 2, RATE, 3)
    with pytest.raises(ValueError, match="level_history: a level history needs a mono or stereo sample, this one has 3 channels"):
        three.level_history(4)
    assert calls == []
    assert len(mixer.level_history(_stereo(10), np.int64(4), np.int64(2))) == 3 and len(calls) == 1      # numpy ints are ints


def test_an_empty_sample_has_an_empty_history_and_launches_nothing(monkeypatch):
    _fake(monkeypatch)
    calls = _record(monkeypatch)
    h = Sample(samplerate=RATE, nchannels=2, samplewidth=2).level_history(64, 1000)
    assert len(h) == 0 and h.peak.shape == (0, 1, 2) and h.starts == [] and h.frames == 0 and h.start_frame == 1000
    assert h.total().master == mixer.Levels((0, 0), (0, 0), 0, 2, 2, RATE) and h.fold(3).nblocks == 0 and h.peaks().shape == (0, 1, 2)
    assert calls == []


# ---- the stems of a song -----------------------------------------------------------------------------------------------------------------------
def test_stems_that_know_their_buffer_make_one_call_over_all_planes(monkeypatch):
    cs = _song(monkeypatch)
    calls = _record(monkeypatch)
    st = cs.stems(10, 21, groups=[(0, 2, 0.5)])
    buf = cs._seq.stemmed[0][2]
    h = st.level_history()
    assert len(calls) == 1 and calls[0] == (buf, 0, 21, 2, 2, 48, 5, 10, 1024)      # the planes' stride in samples; the song's tile in frames
    assert (h.nblocks, h.block_frames, h.start_frame, h.frames, h.ngroups, h.peak.shape) == (1, 1024, 10, 21, 1, (1, 5, 2))
    assert [lv.peak[0] for lv in h[0].tracks] == [1, 2, 3] and h[0].master.peak[0] == 4 and [lv.peak[0] for lv in h[0].groups] == [5]
    assert st.level_history(8).block_counts == [6, 8, 7] and calls[1] == (buf, 0, 21, 2, 2, 48, 5, 10, 8)
    assert buf.views == [(r * 24 * 4, 21 * 4) for r in range(5)]                     # no view was cut for it
    # the whole call: stems, then their history -- the desk's keywords reach stems as they reach it alone
    auto = cs.automation([None] * 3, master=[(0, 10, 0.5, 1.0)], group_pans=[[(0, 10, 0.5, -1.0)]])
    del cs._seq.stemmed[:], calls[:]
    h = cs.level_history(3, 40, block_frames=16, gains=(0.5, 1.0, 2.0), master=0.7, automation=auto, groups=[(0, 2, 0.5)])
    assert [(c[0], c[1], c[4]) for c in cs._seq.stemmed] == [(6, 80, 80)] and cs._seq.stemmed[0][5]["automation"] is _Auto.made[-1]
    assert cs._seq.stemmed[0][5]["gains"] == [0.5, 1.0, 2.0] and cs._seq.stemmed[0][5]["master"] == 0.7 and cs._seq.rendered == []
    assert calls == [(cs._seq.stemmed[0][2], 0, 40, 2, 2, 80, 5, 3, 16)] and h.starts == [3, 16, 32] and h.ngroups == 1
    assert cs.level_history().block_frames == 1024 and calls[-1][2:] == (cs.frames, 2, 2, 2 * cs.frames, 4, 0, 1024)


def test_stems_built_by_hand_take_one_call_per_row(monkeypatch):
    cs = _song(monkeypatch)
    calls = _record(monkeypatch)
    st = cs.stems(10, 21, groups=[(0, 2, 0.5)])
    by_hand = mixer.SongStems(st.tracks, st.master, st.groups, 10, 21)
    h = by_hand.level_history(8)
    assert [c[1:] for c in calls] == [(0, 21, 2, 2, 42, 1, 10, 8)] * 5 and [c[0] for c in calls] == [s._device() for s in st.rows()]
    assert h.peak.shape == (3, 5, 2) and h.peak[0, :, 0].tolist() == [1, 101, 201, 301, 401] and h.ngroups == 1      # the rows in plane order
    assert by_hand.level_history().block_frames == 1024          # without the song's tile: the width's, over the channels
    with pytest.raises(ValueError, match="SongStems: buffer and plane_frames come together"):
        mixer.SongStems(st.tracks, st.master, st.groups, 10, 21, buffer=_StemBuf(100))
    with pytest.raises(ValueError, match="SongStems: every stem has the master's format and the window's 21 frames"):
        mixer.SongStems(st.tracks[:2] + [_stereo(20)], st.master, [], 10, 21).level_history(8)


def test_an_empty_window_and_a_bad_block_launch_nothing(monkeypatch):
    cs = _song(monkeypatch)
    calls = _record(monkeypatch)
    e = cs.level_history(3, 0, groups=[(0, 1, 0.5), (1, 3, 1.0)])
    assert len(e) == 0 and e.peak.shape == (0, 6, 2) and e.ngroups == 2 and e.block_frames == 1024 and e.total().master.peak == (0, 0)
    assert len(e.total().tracks) == 3 and len(e.total().groups) == 2
    assert cs.stems(3, 0).level_history(7).nblocks == 0
    for bad in (0, -1, 2.5, "8", True):
        with pytest.raises(ValueError, match="CompiledSequence: block_frames is a positive int"):
            cs.level_history(block_frames=bad)
    with pytest.raises(ValueError, match="CompiledSequence: 2 gains for 3 tracks"):
        cs.level_history(gains=(1.0, 0.5))
    assert calls == [] and cs._seq.stemmed == [] and cs._seq.rendered == [] and _StemBuf.made == []


def test_a_history_from_the_render_with_a_ride_still_raises_what_it_raised(monkeypatch):
    cs = _song(monkeypatch)
    calls = _record(monkeypatch)
    rides = [cs.automation([None] * 3, master=[(0, 50, 0.5, 1.0)]), cs.automation([None] * 3, groups=[[(0, 50, 0.5, 0.5)]]),
             cs.automation([None] * 3, pans=[[(0, 50, 0.5, -1.0)], None, None]), cs.automation([None] * 3, group_pans=[[(0, 50, 0.5, -1.0)]])]
    for auto in rides:
        for call in (lambda: cs.render(meters="history", automation=auto, groups=[(0, 2, 1.0)]),
                     lambda: cs.render_into(N.DeviceBuffer(4000), 0, 0, 100, meters="history", automation=auto, groups=[(0, 2, 1.0)]),
                     lambda: next(cs.chunks(100, meters="history", automation=auto, groups=[(0, 2, 1.0)]))):
            with pytest.raises(NotImplementedError, match=r"CompiledSequence: rides of buses and pans have no level history yet \(meters=\"history\" with an "
                                                          r"Automation that has master, group or pan pieces\)"):
                call()
        with pytest.raises(NotImplementedError, match="overs are not counted through rides of buses and pans yet"):
            cs.render(meters="history", clips=True, automation=auto, groups=[(0, 2, 1.0)])
    assert cs._seq.rendered == [] and calls == []
    for auto in rides:                                          # and the new route takes every one of them
        assert cs.level_history(0, 100, automation=auto, groups=[(0, 2, 1.0)]).peak.shape == (1, 5, 2)
    assert len(calls) == 4 and len(cs._seq.stemmed) == 4 and cs._seq.rendered == []
    assert "level_history" in mixer.CompiledSequence._no_history_of.__doc__ and "level_history(...)" in mixer.CompiledSequence.__doc__


# ---- the binding and the header -----------------------------------------------------------------------------------------------------------
def test_the_binding_reaches_the_new_entry_point(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(N, "lib", lambda: lib)

    class Buf:
        handle = C.c_void_p(7)
    blocks = N.pcm_level_blocks(Buf, 3, 1000, 2, 4, 2008, 5, 250, 300)
    assert blocks.shape == (5, 5) and blocks.dtype == N.SEQ_METER_DTYPE and not blocks["peak"].any()
    empty = N.pcm_level_blocks(Buf, 0, 0, 1, 2, 0, 3, 9, 4)
    assert empty.shape == (0, 3)
    assert [c[0] for c in lib.calls] == ["sh_pcm_level_blocks"] * 2 and [len(c[1]) for c in lib.calls] == [11] * 2
    a = lib.calls[0][1]
    assert (a[0].value,) + tuple(a[1:9]) == (7, 3, 1000, 2, 4, 2008, 5, 250, 300) and a[10] == 5
    assert C.addressof(a[9].contents) == blocks.ctypes.data       # the table itself is filled, no copy
    b = lib.calls[1][1]
    assert tuple(b[1:9]) == (0, 0, 1, 2, 0, 3, 9, 4) and b[9] is None and b[10] == 0


def test_the_new_symbol_is_declared_in_the_header_and_bound():
    res, args = N._SIGNATURES["sh_pcm_level_blocks"]
    assert res == C.c_int and args == [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_uint32, C.c_uint64, C.c_uint64,
                                       C.POINTER(N.SeqMeter), C.c_size_t]
    root = Path(__file__).resolve().parents[1]
    header = (root / "include" / "synthhip.h").read_text()
    assert "#define SH_ABI_VERSION 6" in header and N.SH_ABI_VERSION == 6      # a new symbol only
    m = re.search(r"int sh_pcm_level_blocks\(([^;]*)\);", header)
    assert m, "sh_pcm_level_blocks is not declared"
    params = [p.split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
    assert params == ["in", "sample_offset", "nframes", "nch", "width", "plane_samples", "nplanes", "origin_frame", "block_frames", "rows", "nblocks"]
    source = (root / "synthesizer_amd" / "csrc" / "pcm_ops.hip").read_text()
    assert "int sh_pcm_level_blocks(" in source and '#include "pcmblocks.hpp"' in source and "k_pcm_level_blocks" in source
    hpp = (root / "synthesizer_amd" / "csrc" / "pcmblocks.hpp").read_text()
    assert int(re.search(r"constexpr uint32_t PART_SAMPLES = (\d+);", hpp).group(1)) == N.PCM_PART_SAMPLES >= 4096
