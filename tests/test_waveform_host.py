"""What the waveform extremes of plain PCM -- ``mixer.Waveform``, ``mixer.waveform`` / ``Sample.waveform``, ``SongStems.waveform``,
``CompiledSequence.waveform``, ``N.pcm_extent_blocks``, sh_pcm_extent_blocks -- need of the host alone (no GPU; the fake native layer of
tests/songhost.py): ``Waveform``'s checks, its grid, ``total()``, ``extents()`` and the mono copy, that ``fold(n)`` of two windows of
one signal that start in different blocks is the coarse call's table, ``peaks()``, what is refused before anything is launched, that an
empty window launches nothing, that a ``SongStems`` that knows its buffer makes ONE call over all planes and one built by hand one
call per row, that ``CompiledSequence.waveform`` is ``stems`` and then that, and that the new symbol is declared in the header and
bound.  The extremes themselves: tests/test_gpu_waveform.py."""
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

INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
SIGNAL = np.random.default_rng(7).integers(-30000, 30000, size=(6000, 2)).astype(np.int32)      # one signal by SONG frame, both channels


def blocks_of(origin, n, B):
    return [(max(k * B, origin), min((k + 1) * B, origin + n)) for k in range(origin // B, (origin + n - 1) // B + 1)] if n > 0 else []


def _record(monkeypatch):
    """N.pcm_extent_blocks without a device: what each call was handed, and the table of SIGNAL's frames [origin, origin + n) -- plane
    r reads the signal plus 1000 r, so that a row says which plane it is"""
    calls = []

    def fake(buf, sample_offset, nframes, nch, width, plane_samples, nplanes, origin_frame, block_frames):
        calls.append((buf, sample_offset, nframes, nch, width, plane_samples, nplanes, origin_frame, block_frames))
        cut = blocks_of(origin_frame, nframes, block_frames)
        blocks = np.zeros((len(cut), nplanes), dtype=N.PCM_EXTENT_DTYPE)
        for j, (a, b) in enumerate(cut):
            for r in range(nplanes):
                blocks["lo"][j, r, :nch] = SIGNAL[a:b, :nch].min(axis=0) + 1000 * r
                blocks["hi"][j, r, :nch] = SIGNAL[a:b, :nch].max(axis=0) + 1000 * r
        return blocks
    monkeypatch.setattr(N, "pcm_extent_blocks", fake)
    return calls


# ---- the Waveform ----------------------------------------------------------------------------------------------------------------------------
def test_a_waveform_checks_its_arrays_and_its_grid():
    lo = np.array([[[-5, -1]], [[-7, 2]], [[3, -9]]])
    hi = np.array([[[4, 8]], [[-6, 2]], [[30, -9]]])
    w = mixer.Waveform(lo, hi, 2, 100, 250, 250, 2, 2, RATE)
    assert (len(w), w.nblocks, w.first_block, w.block_frames, w.start_frame, w.frames, w.ngroups) == (3, 3, 2, 100, 250, 250, 0)
    assert (w.samplewidth, w.nchannels, w.samplerate) == (2, 2, RATE) and w.lo.dtype == w.hi.dtype == np.int32 and w.lo.shape == (3, 1, 2)
    assert w.starts == [250, 300, 400] and w.block_counts == [50, 100, 100]
    t_lo, t_hi = w.total()
    assert t_lo.tolist() == [[-7, -9]] and t_hi.tolist() == [[30, 8]]
    e = w.extents()
    assert e.shape == (3, 1, 2, 2) and e[1, 0].tolist() == [[-7, -6], [2, 2]] and e[2, 0, 1].tolist() == [-9, -9]      # [..., channel, (lo, hi)]
    assert w[1].tolist() == e[1].tolist() and w[-1].tolist() == e[2].tolist() and [b.tolist() for b in w] == e.tolist()
    for j in (3, -4):
        with pytest.raises(IndexError, match="Waveform: block"):
            w[j]
    assert "3 blocks of 100 frames" in repr(w) and "[250, 500)" in repr(w)
    with pytest.raises(ValueError, match=r"Waveform: lo and hi are \(nblocks, nrows, 2\) arrays"):
        mixer.Waveform(lo, hi[:2], 2, 100, 250, 250, 2, 2, RATE)
    with pytest.raises(ValueError, match=r"Waveform: lo and hi are \(nblocks, nrows, 2\) arrays"):
        mixer.Waveform(lo[:, :, 0], hi[:, :, 0], 2, 100, 250, 250, 2, 2, RATE)
    with pytest.raises(ValueError, match=r"Waveform: 3 blocks of 100 frames from block 2 for frames \[250, 550\)"):
        mixer.Waveform(lo, hi, 2, 100, 250, 300, 2, 2, RATE)     # four blocks' window
    with pytest.raises(ValueError, match=r"Waveform: 3 blocks of 100 frames from block 1 for frames \[250, 500\)"):
        mixer.Waveform(lo, hi, 1, 100, 250, 250, 2, 2, RATE)     # the first block is the window's
    with pytest.raises(ValueError, match="Waveform: 3 blocks of 0 frames"):
        mixer.Waveform(lo, hi, 0, 0, 0, 0, 2, 2, RATE)


def test_a_mono_waveform_reads_0_in_channel_1_and_draws_channel_0_twice():
    lo = np.array([[[-5, 0]], [[-7, 0]]])
    hi = np.array([[[-4, 0]], [[-6, 0]]])
    w = mixer.Waveform(lo, hi, 0, 10, 0, 20, 1, 1, RATE)
    assert w.lo[:, :, 1].tolist() == [[0], [0]] and w.hi[:, :, 1].tolist() == [[0], [0]]      # the table's rule
    assert w.extents().tolist() == [[[[-5, -4], [-5, -4]]], [[[-7, -6], [-7, -6]]]] and w[0].tolist() == [[[-5, -4], [-5, -4]]]
    assert w.lo[0, 0, 1] == 0                                   # extents() copies: the arrays keep the table's zeros
    assert w.peaks().tolist() == [[[5, 5]], [[7, 7]]]           # left == right, as SongHistory.peaks()
    assert [a.tolist() for a in w.total()] == [[[-7, 0]], [[-4, 0]]]


def test_peaks_are_the_larger_magnitude_and_the_lower_rail_is_one_more_than_the_upper():
    lo = np.array([[[-32768, 3]], [[-2, INT32_MIN]], [[5, -9]]])
    hi = np.array([[[5, 32767]], [[1, INT32_MAX]], [[6, -8]]])
    w = mixer.Waveform(lo, hi, 0, 4, 0, 12, 4, 2, RATE)
    p = w.peaks()
    assert p.dtype == np.uint32 and p.tolist() == [[[32768, 32767]], [[2, 2 ** 31]], [[6, 9]]]


def test_fold_of_two_windows_that_start_in_different_blocks_is_the_coarse_calls_table(monkeypatch):
    _fake(monkeypatch)
    calls = _record(monkeypatch)
    for start, n in ((250, 1000), (610, 777)):                  # one in the third fine block of a coarse one, one in the first
        s = _stereo(n)
        fine, coarse = s.waveform(100, origin_frame=start), mixer.waveform(s, 300, start)
        assert isinstance(fine, mixer.Waveform) and fine.first_block == start // 100 and coarse.first_block == start // 300
        folded = fine.fold(3)
        assert np.array_equal(folded.lo, coarse.lo) and np.array_equal(folded.hi, coarse.hi) and len(folded) == len(coarse) < len(fine)
        assert (folded.first_block, folded.block_frames, folded.starts, folded.block_counts) == (coarse.first_block, 300, coarse.starts, coarse.block_counts)
        assert (folded.start_frame, folded.frames, folded.samplewidth, folded.nchannels, folded.samplerate) == (start, n, 2, 2, RATE)
        assert [a.tolist() for a in folded.total()] == [a.tolist() for a in fine.total()]
        assert [a.tolist() for a in fine.total()] == [[SIGNAL[start:start + n].min(axis=0).tolist()], [SIGNAL[start:start + n].max(axis=0).tolist()]]
        assert np.array_equal(fine.fold(1).lo, fine.lo) and len(fine.fold(10 ** 6)) == 1
        for bad in (0, -2):
            with pytest.raises(ValueError, match=r"Waveform: fold\(n\) needs a positive n"):
                fine.fold(bad)
    # coarse block 3, song frames [900, 1200), lies whole inside both windows: it reads the same from both
    a, b = mixer.waveform(_stereo(1000), 100, 250).fold(3), mixer.waveform(_stereo(777), 100, 610).fold(3)
    assert a.starts[3] == b.starts[1] == 900 and np.array_equal(a.lo[3], b.lo[1]) and np.array_equal(a.hi[3], b.hi[1])
    assert len(calls) == 6


# ---- a Sample --------------------------------------------------------------------------------------------------------------------------------
def test_a_samples_waveform_is_one_call_over_its_buffer(monkeypatch):
    _fake(monkeypatch)
    calls = _record(monkeypatch)
    s = _stereo(1000, 4)
    w = s.waveform(300, origin_frame=250)
    assert isinstance(w, mixer.Waveform) and len(calls) == 1 and calls[0] == (s._device(), 0, 1000, 2, 4, 2000, 1, 250, 300)
    assert (w.nblocks, w.block_frames, w.first_block, w.start_frame, w.frames, w.ngroups) == (5, 300, 0, 250, 1000, 0)
    assert w.starts == [250, 300, 600, 900, 1200] and w.block_counts == [50, 300, 300, 300, 50] and w.lo.shape == (5, 1, 2)
    assert (w.samplewidth, w.nchannels, w.samplerate) == (4, 2, RATE)
    assert w.lo[2, 0].tolist() == SIGNAL[600:900].min(axis=0).tolist() and w.hi[4, 0].tolist() == SIGNAL[1200:1250].max(axis=0).tolist()
    m = mixer.waveform(_mono(77), 1000)                         # a mono Sample, the default origin
    assert calls[1][2:] == (77, 1, 2, 77, 1, 0, 1000) and m.lo[0, 0].tolist() == [int(SIGNAL[:77, 0].min()), 0]
    assert m.extents()[0, 0].tolist() == [[int(SIGNAL[:77, 0].min()), int(SIGNAL[:77, 0].max())]] * 2


@pytest.mark.parametrize("bad", [0, -3, 1.5, "64", None, True])
def test_block_frames_is_a_positive_int(monkeypatch, bad):
    cs = _song(monkeypatch)
    calls = _record(monkeypatch)
    for call in (lambda: mixer.waveform(_stereo(10), bad), lambda: _stereo(10).waveform(bad)):
        with pytest.raises(ValueError, match="waveform: block_frames is a positive int, not %s" % re.escape(repr(bad))):
            call()
    if bad is not None:                                         # (None is the default block of a song's stems)
        with pytest.raises(ValueError, match="SongStems: block_frames is a positive int"):
            mixer.SongStems([], _stereo(10), [], 0, 10).waveform(bad)
        with pytest.raises(ValueError, match="CompiledSequence: block_frames is a positive int"):
            cs.waveform(block_frames=bad)
    assert calls == [] and cs._seq.stemmed == []


def test_the_origin_and_the_format_are_checked_before_anything_is_launched(monkeypatch):
    _fake(monkeypatch)
    calls = _record(monkeypatch)
    for bad in (-1, 0.5, "0", None, False):
        with pytest.raises(ValueError, match="waveform: origin_frame is a non-negative int, not %s" % re.escape(repr(bad))):
            mixer.waveform(_stereo(10), 4, bad)
    three = Sample.from_raw_frames(bytes(2 * 3 * 10), 2, RATE, 3)
    with pytest.raises(ValueError, match="waveform: a waveform needs a mono or stereo sample, this one has 3 channels"):
        three.waveform(4)
    with pytest.raises(ValueError, match="SongStems: a waveform needs a mono or stereo sample, this one has 3 channels"):
        mixer.SongStems([], three, [], 0, 10).waveform(4)
    assert calls == []
    assert len(mixer.waveform(_stereo(10), np.int64(4), np.int64(2))) == 3 and len(calls) == 1      # numpy ints are ints


def test_an_empty_window_gives_an_empty_waveform_and_launches_nothing(monkeypatch):
    cs = _song(monkeypatch)
    calls = _record(monkeypatch)
    w = Sample(samplerate=RATE, nchannels=2, samplewidth=2).waveform(64, 1000)
    assert len(w) == 0 and w.lo.shape == w.hi.shape == (0, 1, 2) and w.starts == [] and w.block_counts == [] and (w.frames, w.start_frame) == (0, 1000)
    assert w.extents().shape == (0, 1, 2, 2) and w.peaks().shape == (0, 1, 2) and w.fold(3).nblocks == 0 and w.fold(3).block_frames == 192
    assert [a.tolist() for a in w.total()] == [[[INT32_MAX, INT32_MAX]], [[INT32_MIN, INT32_MIN]]]      # audioop.minmax of no sample
    e = cs.waveform(3, 0, groups=[(0, 1, 0.5), (1, 3, 1.0)])
    assert len(e) == 0 and e.lo.shape == (0, 6, 2) and e.ngroups == 2 and e.block_frames == 1024
    assert cs.stems(3, 0).waveform(7).nblocks == 0
    assert calls == [] and cs._seq.stemmed == [] and cs._seq.rendered == [] and _StemBuf.made == []


# ---- the stems of a song -----------------------------------------------------------------------------------------------------------------------
def test_stems_that_know_their_buffer_make_one_call_over_all_planes(monkeypatch):
    cs = _song(monkeypatch)
    calls = _record(monkeypatch)
    st = cs.stems(10, 21, groups=[(0, 2, 0.5)])
    buf = cs._seq.stemmed[0][2]
    w = st.waveform()
    assert len(calls) == 1 and calls[0] == (buf, 0, 21, 2, 2, 48, 5, 10, 1024)      # the planes' stride in samples; the song's tile in frames
    assert (w.nblocks, w.block_frames, w.start_frame, w.frames, w.ngroups, w.lo.shape) == (1, 1024, 10, 21, 1, (1, 5, 2))
    assert (w.lo[0, :, 0] - w.lo[0, 0, 0]).tolist() == [0, 1000, 2000, 3000, 4000]      # the rows in plane order: tracks, master, groups
    assert st.waveform(8).block_counts == [6, 8, 7] and calls[1] == (buf, 0, 21, 2, 2, 48, 5, 10, 8)
    assert buf.views == [(r * 24 * 4, 21 * 4) for r in range(5)]                     # no view was cut for it


def test_stems_built_by_hand_take_one_call_per_row(monkeypatch):
    cs = _song(monkeypatch)
    calls = _record(monkeypatch)
    st = cs.stems(10, 21, groups=[(0, 2, 0.5)])
    by_hand = mixer.SongStems(st.tracks, st.master, st.groups, 10, 21)
    w = by_hand.waveform(8)
    assert [c[1:] for c in calls] == [(0, 21, 2, 2, 42, 1, 10, 8)] * 5 and [c[0] for c in calls] == [s._device() for s in st.rows()]
    assert w.lo.shape == (3, 5, 2) and w.ngroups == 1 and w.starts == [10, 16, 24]
    assert by_hand.waveform().block_frames == 1024              # without the song's tile: the width's, over the channels
    with pytest.raises(ValueError, match="SongStems: every stem has the master's format and the window's 21 frames"):
        mixer.SongStems(st.tracks[:2] + [_stereo(20)], st.master, [], 10, 21).waveform(8)


def test_a_songs_waveform_is_one_stems_call_and_one_extents_call(monkeypatch):
    cs = _song(monkeypatch)
    calls = _record(monkeypatch)
    auto = cs.automation([None] * 3, master=[(0, 10, 0.5, 1.0)], group_pans=[[(0, 10, 0.5, -1.0)]])      # a desk that rides: stems takes it
    w = cs.waveform(3, 40, block_frames=16, gains=(0.5, 1.0, 2.0), master=0.7, automation=auto, groups=[(0, 2, 0.5)])
    assert [(c[0], c[1], c[4]) for c in cs._seq.stemmed] == [(6, 80, 80)] and cs._seq.stemmed[0][5]["automation"] is _Auto.made[-1]
    assert cs._seq.stemmed[0][5]["gains"] == [0.5, 1.0, 2.0] and cs._seq.stemmed[0][5]["master"] == 0.7 and cs._seq.rendered == []
    assert calls == [(cs._seq.stemmed[0][2], 0, 40, 2, 2, 80, 5, 3, 16)] and w.starts == [3, 16, 32] and w.ngroups == 1 and w.lo.shape == (3, 5, 2)
    assert cs.waveform().block_frames == 1024 and calls[-1][2:] == (cs.frames, 2, 2, 2 * cs.frames, 4, 0, 1024)
    assert len(cs._seq.stemmed) == 2 and len(calls) == 2
    # what stems refuses, it refuses, before anything is launched
    with pytest.raises(ValueError, match="CompiledSequence: 2 gains for 3 tracks"):
        cs.waveform(gains=(1.0, 0.5))
    for args, kw in (((), dict(gains=(1.0, 0.5))), ((), dict(groups=[(0, 9, 1.0)])), ((), dict(master=float("nan"))),
                     ((cs.frames + 1,), {}), ((0, cs.frames + 1), {})):
        with pytest.raises(Exception) as by_stems:
            cs.stems(*args, **kw)
        with pytest.raises(Exception) as refused:
            cs.waveform(*args, **kw)
        assert type(refused.value) is type(by_stems.value) and str(refused.value) == str(by_stems.value), (args, kw)
    assert len(cs._seq.stemmed) == 2 and len(calls) == 2


# ---- the binding and the header -----------------------------------------------------------------------------------------------------------
def test_the_binding_reaches_the_new_entry_point(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(N, "lib", lambda: lib)

    class Buf:
        handle = C.c_void_p(7)
    blocks = N.pcm_extent_blocks(Buf, 3, 1000, 2, 4, 2008, 5, 250, 300)
    assert blocks.shape == (5, 5) and blocks.dtype == N.PCM_EXTENT_DTYPE and not blocks["lo"].any() and not blocks["hi"].any()
    empty = N.pcm_extent_blocks(Buf, 0, 0, 1, 2, 0, 3, 9, 4)
    assert empty.shape == (0, 3)
    assert [c[0] for c in lib.calls] == ["sh_pcm_extent_blocks"] * 2 and [len(c[1]) for c in lib.calls] == [11] * 2
    a = lib.calls[0][1]
    assert (a[0].value,) + tuple(a[1:9]) == (7, 3, 1000, 2, 4, 2008, 5, 250, 300) and a[10] == 5
    assert C.addressof(a[9].contents) == blocks.ctypes.data       # the table itself is filled, no copy
    b = lib.calls[1][1]
    assert tuple(b[1:9]) == (0, 0, 1, 2, 0, 3, 9, 4) and b[9] is None and b[10] == 0


def test_the_new_symbol_is_declared_in_the_header_and_bound():
    res, args = N._SIGNATURES["sh_pcm_extent_blocks"]
    assert res == C.c_int and args == [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_uint32, C.c_uint64, C.c_uint64,
                                       C.POINTER(N.PcmExtent), C.c_size_t]
    assert args[:9] + args[10:] == N._SIGNATURES["sh_pcm_level_blocks"][1][:9] + N._SIGNATURES["sh_pcm_level_blocks"][1][10:]
    assert N.PCM_EXTENT_DTYPE.itemsize == C.sizeof(N.PcmExtent) == 16
    root = Path(__file__).resolve().parents[1]
    header = (root / "include" / "synthhip.h").read_text()
    assert "#define SH_ABI_VERSION 6" in header and N.SH_ABI_VERSION == 6      # a new symbol only
    m = re.search(r"int sh_pcm_extent_blocks\(([^;]*)\);", header)
    assert m, "sh_pcm_extent_blocks is not declared"
    params = [p.split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
    assert params == ["in", "sample_offset", "nframes", "nch", "width", "plane_samples", "nplanes", "origin_frame", "block_frames", "rows", "nblocks"]
    assert re.search(r"typedef struct sh_pcm_extent \{\s*int32_t lo\[2\];\s*int32_t hi\[2\];\s*\} sh_pcm_extent;", header)
    source = (root / "synthesizer_amd" / "csrc" / "pcm_ops.hip").read_text()
    assert "int sh_pcm_extent_blocks(" in source and '#include "pcmextent.hpp"' in source and "k_pcm_extent_blocks" in source and "k_pcm_extent_fold" in source
    hpp = (root / "synthesizer_amd" / "csrc" / "pcmextent.hpp").read_text()
    assert '#include "pcmblocks.hpp"' in hpp and "PART_SAMPLES =" not in hpp      # it states no geometry of its own
