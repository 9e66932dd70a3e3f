"""
The mixer sum bus.

Two shapes of the same operation:

* ``VoiceBank``: N oscillator voices (the classes of oscillators.py) -> stereo bus.  The voice table
  lives in HBM; ``render`` runs the fused generate-and-mix kernel (no per-voice PCM ever reaches
  HBM), ``generate`` + ``mix_bus`` is the reference-shaped two-step form (voices materialised as
  float32 PCM, then summed) whose mix step is HBM-bound.
* ``mix_samples``: the reference's real-time mixer rule over integer PCM chunks (upstream
  playback.py mixer loop: ``mixed = audioop.add(mixed, chunk, width)`` for every active voice, in
  order) -- an order-dependent chain of saturating adds, reproduced bit-exactly.
* ``RealTimeMixer``: that loop itself, chunk by chunk: samples are added while it runs, may repeat or start a few
  chunks late, and every ``next(chunks())`` folds the current chunk of every active sample, read in place in HBM
  (``sh_mix_chain_gather_i16``: a pointer table instead of a staging copy), into one chunk of output.

``pan`` follows the linear law used throughout: gain_l = (1 - pan) / 2, gain_r = (1 + pan) / 2.
"""
from __future__ import annotations

import ctypes as C
import gc
import math
import operator
import threading
from typing import Callable, Dict, Generator, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from . import _native as N
from . import params
from .oscillators import Oscillator, VoiceSpec, _pwm_widths, _table, pack_voices, time_step_weights
from .sample import Sample

__all__ = ["VoiceBank", "RealTimeMixer", "mix_samples", "sequence", "compile_sequence", "compile_tracks", "CompiledSequence", "Levels", "SongLevels", "SongStems", "Automation", "pan_gains", "compose_chain_parts", "apply_chain_parts", "mixdown_i16_banks"]


def pan_gains(pan: float) -> Tuple[float, float]:
    return (1.0 - pan) / 2.0, (1.0 + pan) / 2.0


class _RowMatrix:
    """The per-launch float64 rows of a VoiceBank (sh_bank_render_rows): rows 0 .. nfm-1 hold the running sums of the fm_lfo
    modulators (rendered, then scanned in place by ONE batched launch, the carries staying on the device from block to
    block), the rows after them pulse widths / rendered voices.  Sources that are single closed-form records are rendered by
    one launch per group (a bank of modulators, sh_bank_generate_f64); anything else -- a modulator that is itself
    modulated by an arbitrary oscillator, a filter graph -- renders into its row on its own."""

    def __init__(self, fm_sources: Sequence[Oscillator], other_sources: Sequence[Oscillator], samplerate: int,
                 other_roles: Optional[Sequence[str]] = None, fm_incs: Optional[Sequence[float]] = None) -> None:
        self.nfm = len(fm_sources)
        self.nrows = len(fm_sources) + len(other_sources)
        self.samplerate = samplerate
        self.fm_rows: List[int] = []
        self.other_rows: List[int] = []
        self._banks: List[Tuple[N.Bank, int, bool]] = []        # (bank of closed-form sources, first row, fm rows?)
        self._pwm_bank_rows: List[int] = []                     # rows of pulse widths among them (params.variants["pulse"])
        self._singles: List[Tuple[Oscillator, int, str]] = []   # (source, row, "fm" | "pwm" | "voice")

        def place(sources, first_row, out_rows, roles):
            bankable, single = [], []
            is_fm = roles is None
            for k, m in enumerate(sources):
                if m.samplerate != samplerate:
                    raise ValueError("a modulator must run at the sample rate of its voice")
                try:
                    sp = m.spec()
                    ok = sp.fm_mode != N.SH_FM_BUFFER and not sp.needs_pwm and m.length is None
                except NotImplementedError:
                    sp, ok = None, False
                (bankable if ok else single).append((k, m, sp))
            rows = [0] * len(sources)
            r = first_row
            if bankable:
                self._banks.append((N.Bank(*pack_voices([sp for _, _, sp in bankable])), r, is_fm))
                for k, _m, _sp in bankable:
                    rows[k] = r
                    if not is_fm and roles[k] == "pwm":
                        self._pwm_bank_rows.append(r)
                    r += 1
            for k, m, _sp in single:
                rows[k] = r
                self._singles.append((m, r, "fm" if is_fm else roles[k]))
                r += 1
            out_rows.extend(rows)

        place(fm_sources, 0, self.fm_rows, None)
        # the time step inc of every fm row's CARRIER (2 pi / sr for Sine / Harmonics, 1 / sr for the turn-based kinds): the row is
        # weighted with the accumulated time's actual steps over inc in front of the scan (oscillators.time_step_weights); runs of
        # neighbouring rows with the same inc are weighted by one call
        self._row_inc: List[float] = [0.0] * self.nfm
        if fm_incs is not None:
            for k, r in enumerate(self.fm_rows):
                self._row_inc[r] = float(fm_incs[k])
        place(other_sources, self.nfm, self.other_rows, list(other_roles) if other_roles is not None else ["voice"] * len(other_sources))
        self._buf: Optional[N.DeviceBuffer] = None
        self._stride = 0
        self._carry: Optional[N.DeviceBuffer] = None
        if self.nfm:
            self._carry = N.DeviceBuffer(self.nfm * 8)
            self._carry.zero()
        self._pos = 0                                           # the carries hold L(_pos)

    def _render(self, start: int, n: int, fm_only: bool = False) -> None:
        """Rows of frames [start, start + n).  fm_only: a replay of the running sums on the way to a later block -- only the fm
        rows carry state from block to block, the others are not touched."""
        L = N.lib()
        for bank, row0, is_fm in self._banks:
            if is_fm or not fm_only:
                N.check(L.sh_bank_generate_f64(bank.handle, start, n, self._buf.handle, row0, self._stride))
        if not fm_only:
            for row in self._pwm_bank_rows:                         # (closed-form pwm sources rendered by the bank launch above)
                _pwm_widths(self._buf, row * self._stride, n)
        for m, row, role in self._singles:
            if fm_only and role != "fm":
                continue
            # a VOICE that ends (an envelope with stop_at_end over a filter graph, a filter over a finite source) is silent from
            # there on, like a fused stop_at_end voice of the same bank; a modulator that ends before its carrier is an error,
            # as upstream (the carrier's next() on it raises)
            avail = n
            if role == "voice" and m.length is not None:
                avail = max(0, min(n, m.length - start))
            if avail:
                m._render_device(start, avail, out_f64=self._buf.view(row * self._stride * 8, avail * 8))
                if role == "pwm":
                    _pwm_widths(self._buf, row * self._stride, avail)
            if avail < n:
                N.check(L.sh_ew_f64(N.SH_EW_FILL, None, 0, None, 0, n - avail, 0.0, 0.0, self._buf.handle, row * self._stride + avail, None, 0, None))
        if self.nfm:
            r0 = 0
            while r0 < self.nfm:
                r1 = r0 + 1
                while r1 < self.nfm and self._row_inc[r1] == self._row_inc[r0]:
                    r1 += 1
                if self._row_inc[r0] != 0.0:
                    runs = time_step_weights(self._row_inc[r0], start, n)
                    if len(runs) == 1 and runs[0][:2] == (0, n):          # one piece of the time table: rows r0 .. r1 - 1 in one call
                        if runs[0][2] != 0.0:
                            o = r0 * self._stride
                            N.check(L.sh_ew_f64(N.SH_EW_AXPY, self._buf.handle, o, self._buf.handle, o, (r1 - r0 - 1) * self._stride + n,
                                                runs[0][2], 0.0, self._buf.handle, o, None, 0, None))
                    else:                                                  # a piece of the time table ends inside the block (rare)
                        for r in range(r0, r1):
                            for off, cnt, wm1 in runs:
                                if wm1 != 0.0:
                                    o = r * self._stride + off
                                    N.check(L.sh_ew_f64(N.SH_EW_AXPY, self._buf.handle, o, self._buf.handle, o, cnt, wm1, 0.0,
                                                        self._buf.handle, o, None, 0, None))
                r0 = r1
            N.check(L.sh_scan_rows_f64(self._buf.handle, 0, self.nfm, n, self._stride, self._carry.handle))
            self._pos = start + n

    def fill(self, start: int, n: int) -> Tuple[N.DeviceBuffer, int]:
        if self._buf is None or n > self._stride:
            self._stride = max(n, 4096)
            self._buf = N.DeviceBuffer(self.nrows * self._stride * 8)
        if self.nfm and start != self._pos:                     # random access into a recurrence: replay the sums up to `start`
            if start < self._pos:
                self._carry.zero()
                self._pos = 0
            while self._pos < start:
                self._render(self._pos, min(self._stride, start - self._pos), fm_only=True)
        self._render(start, n)
        return self._buf, self._stride


class VoiceBank:
    """N oscillator voices summed to one stereo bus on the GPU."""

    def __init__(self, voices: Sequence[Oscillator], gains: Optional[Sequence[Tuple[float, float]]] = None,
                 pans: Optional[Sequence[float]] = None) -> None:
        if not voices:
            raise ValueError("a voice bank needs at least one voice")
        if gains is not None and pans is not None:
            raise ValueError("give gains or pans, not both")
        if pans is not None:
            gains = [pan_gains(p) for p in pans]
        if gains is None:
            gains = [(1.0, 1.0)] * len(voices)
        if len(gains) != len(voices):
            raise ValueError("one (left, right) gain pair per voice")
        rates = {v.samplerate for v in voices}
        if len(rates) != 1:
            raise ValueError("all voices of a bank must share one sample rate")
        self.samplerate = rates.pop()
        self.nvoices = len(voices)
        self.gains = [(float(l), float(r)) for l, r in gains]
        # Voices that read a ROW of a per-launch float64 matrix: a carrier whose fm_lfo is not a closed-form Sine (the row is
        # the running sum of the modulator), a Pulse with a pwm_lfo (pulse width per sample), or a voice that is no single
        # record at all -- a filter graph, an envelope over one -- whose samples are rendered into its row (SH_BUFFER).
        specs: List[VoiceSpec] = []
        fm_src: List[Tuple[int, Oscillator]] = []           # (voice, modulator): rows 0 .. nfm-1, scanned in place
        fm_incs: List[float] = []                           # ... and the time step of the voice (the carrier) itself
        other_src: List[Tuple[str, int, Oscillator]] = []   # ("pwm" | "voice", voice, source): the rows after them
        # (the collector off while the records are made: a table of 200 000 notes is a million live objects, and every generation-2
        # pass walks them all -- 2.5 s with it, 1.35 s without; nothing in the loop makes a cycle)
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            for i, v in enumerate(voices):
                try:
                    sp = v.spec()
                except NotImplementedError:
                    sp = VoiceSpec(kind=N.SH_BUFFER, amplitude=1.0, bias=0.0, fm_mode=N.SH_FM_NONE, carrier=_table(0.0, 0.0))
                    other_src.append(("voice", i, v))
                else:
                    if sp.fm_mode == N.SH_FM_BUFFER:
                        fm_src.append((i, v._fm_source()))
                        fm_incs.append(sp.fm_inc)
                    if sp.needs_pwm:
                        other_src.append(("pwm", i, v._pwm_source()))
                specs.append(sp)
            self._packed = pack_voices(specs, self.gains)
        finally:
            if gc_was_on:
                gc.enable()
        self._bank = N.Bank(*self._packed)
        self._gains_dev: Optional[N.DeviceBuffer] = None
        self._pan_dev: Optional[N.DeviceBuffer] = None
        self._rows: Optional[_RowMatrix] = None
        if fm_src or other_src:
            fm_row = np.full(self.nvoices, -1, dtype=np.int32)
            pwm_row = np.full(self.nvoices, -1, dtype=np.int32)
            self._rows = _RowMatrix([m for _, m in fm_src], [m for _, _, m in other_src], self.samplerate,
                                    other_roles=[what for what, _, _ in other_src], fm_incs=fm_incs)
            for (i, _m), r in zip(fm_src, self._rows.fm_rows):
                fm_row[i] = r
            for (what, i, _m), r in zip(other_src, self._rows.other_rows):
                (pwm_row if what == "pwm" else fm_row)[i] = r
            N.check(N.lib().sh_bank_set_rows(self._bank.handle, fm_row.ctypes.data, pwm_row.ctypes.data))

    # -- fused path ------------------------------------------------------------------------------
    def render_device(self, nframes: int, start: int = 0, bus_f32: Optional[N.DeviceBuffer] = None,
                      bus_f64: Optional[N.DeviceBuffer] = None) -> N.DeviceBuffer:
        """Fused generate-and-mix into device buffers (float32 frames x 2 and/or float64 frames x 2)."""
        if bus_f32 is None and bus_f64 is None:
            bus_f32 = N.DeviceBuffer(nframes * 8)
        if self._rows is not None and nframes:
            rows, stride = self._rows.fill(start, nframes)
            N.check(N.lib().sh_bank_render_rows(self._bank.handle, start, nframes, rows.handle, stride,
                                                bus_f32.handle if bus_f32 is not None else None,
                                                bus_f64.handle if bus_f64 is not None else None))
            return bus_f32 if bus_f32 is not None else bus_f64
        N.check(N.lib().sh_bank_render(self._bank.handle, start, nframes,
                                       bus_f32.handle if bus_f32 is not None else None,
                                       bus_f64.handle if bus_f64 is not None else None))
        return bus_f32 if bus_f32 is not None else bus_f64

    def render_run(self, nframes: int, nblocks: int, start: int = 0, ring: Optional[Sequence[N.DeviceBuffer]] = None,
                   pcm_ring: Optional[Sequence[N.DeviceBuffer]] = None, scale: float = 32767.0) -> Sequence[N.DeviceBuffer]:
        """``nblocks`` consecutive blocks of ``nframes`` frames in ONE call: block k goes to ``ring[k % len(ring)]`` (float32 stereo)
        and / or ``pcm_ring[k % len(pcm_ring)]`` (saturated int16 stereo).  Ring buffers that are consecutive windows of one
        allocation (``VoiceBank.make_ring``) are filled by one launch per stretch: a run of blocks of a small bank costs one
        launch, not one per block.  Without a ring: a fresh contiguous one of ``nblocks`` float32 buffers.  Returns the ring."""
        if self._rows is not None:
            raise NotImplementedError("render_run: a bank with modulation rows renders block by block (render_device)")
        if ring is None and pcm_ring is None:
            ring = self.make_ring(nframes, nblocks)
        n32 = len(ring) if ring is not None else 0
        n16 = len(pcm_ring) if pcm_ring is not None else 0
        if n32 and n16 and n32 != n16:
            raise ValueError("the float32 and the PCM ring must have the same number of slots")
        nring = n32 or n16
        a32 = (C.c_void_p * nring)(*[b.handle for b in ring]) if n32 else None
        a16 = (C.c_void_p * nring)(*[b.handle for b in pcm_ring]) if n16 else None
        N.check(N.lib().sh_bank_render_run(self._bank.handle, start, nframes, nblocks, a32, a16, nring, float(scale)))
        return ring if ring is not None else pcm_ring

    @staticmethod
    def make_ring(nframes: int, nslots: int, bytes_per_frame: int = 8) -> Sequence[N.DeviceBuffer]:
        """``nslots`` bus buffers of ``nframes`` frames that are consecutive windows of ONE allocation (8 bytes per frame: float32
        stereo; 4: int16 stereo PCM): ``render_run`` fills neighbouring slots with one launch."""
        whole = N.DeviceBuffer(nslots * nframes * bytes_per_frame)
        return [whole.view(k * nframes * bytes_per_frame, nframes * bytes_per_frame) for k in range(nslots)]

    def render(self, nframes: int, start: int = 0) -> np.ndarray:
        """Stereo bus as a [nframes, 2] float32 array."""
        if nframes == 0:
            return np.zeros((0, 2), dtype=np.float32)
        buf = self.render_device(nframes, start)
        out = buf.download(np.float32, nframes * 2).reshape(nframes, 2)
        buf.free()
        return out

    def render_pcm_device(self, nframes: int, start: int = 0, scale: float = 32767.0,
                          pcm: Optional[N.DeviceBuffer] = None) -> N.DeviceBuffer:
        """Fused generate-and-mix delivered as saturated int16 stereo PCM (nframes x 2) in a device buffer: the fold of
        the voice groups' partial buses quantises as it goes, so consecutive blocks stay pipelined (no quantise kernel
        between them).  The buffer is complete once any other library call (or ``_native.sync()``) has been made."""
        if pcm is None:
            pcm = N.DeviceBuffer(nframes * 4)
        if self._rows is not None:                       # modulation rows: float32 bus first, then the saturating quantiser
            bus = self.render_device(nframes, start)
            N.check(N.lib().sh_quantize_clip_f32(bus.handle, nframes * 2, float(scale), pcm.handle))
            bus.free()
            return pcm
        N.check(N.lib().sh_bank_render_pcm(self._bank.handle, start, nframes, float(scale), pcm.handle))
        return pcm

    def render_sample(self, nframes: int, start: int = 0, scale: float = 32767.0) -> Sample:
        """Stereo bus quantised to an int16 Sample (saturating: a bus can exceed full scale)."""
        s = Sample(samplerate=self.samplerate, nchannels=2, samplewidth=2)
        if nframes == 0:
            return s
        s._set_device(self.render_pcm_device(nframes, start, scale), nframes * 4)
        return s

    # -- two-step (reference-shaped) path -----------------------------------------------------------
    def generate_device(self, nframes: int, start: int = 0, out: Optional[N.DeviceBuffer] = None,
                        stride: Optional[int] = None) -> N.DeviceBuffer:
        """Every voice as float32 PCM in HBM, voice-major: out[v*stride + i]."""
        stride = nframes if stride is None else stride
        if out is None:
            out = N.DeviceBuffer(self.nvoices * stride * 4)
        if self._rows is not None and nframes:
            # voices that read rows of the launch's float64 matrix (arbitrary fm_lfo / pwm_lfo, filter graphs): the same matrix
            # the fused render fills, read by the general materialisation kernel
            rows, rstride = self._rows.fill(start, nframes)
            N.check(N.lib().sh_bank_generate_rows(self._bank.handle, start, nframes, rows.handle, rstride, out.handle, stride))
            return out
        N.check(N.lib().sh_bank_generate(self._bank.handle, start, nframes, out.handle, stride))
        return out

    def generate(self, nframes: int, start: int = 0) -> np.ndarray:
        buf = self.generate_device(nframes, start)
        out = buf.download(np.float32, self.nvoices * nframes).reshape(self.nvoices, nframes)
        buf.free()
        return out

    # -- two-step, integer: the route upstream itself takes (oscillator block -> Sample.from_osc_block -> mixer) ---------------
    def generate_i16_device(self, nframes: int, start: int = 0, scale: float = 32767.0, out: Optional[N.DeviceBuffer] = None,
                            stride: Optional[int] = None, check: bool = True) -> Tuple[N.DeviceBuffer, int]:
        """Every voice as int16 PCM in HBM, voice-major: out[v*stride + i] = int(scale * sample) -- ``Sample.from_osc_block`` of
        every voice's block in one launch (OverflowError where a sample does not fit).  Returns (buffer, stride); the stride is
        ``nframes`` rounded up to a multiple of 64 unless given (it must be even).  ``check=False`` (a stream of blocks): the
        call only enqueues; ``VoiceBank.overflow_check()`` raises for every block since the last check at once."""
        stride = (nframes + 63) & ~63 if stride is None else stride
        if out is None:
            out = N.DeviceBuffer(max(self.nvoices * stride * 2, 4))
        if nframes == 0:
            return out, stride
        if params.variants["quantise"] == "round":
            # the other reading of the quantiser (round half to even): the fused epilogue truncates, so every voice goes through
            # float64 rows and the library's quantiser, which follows the option (a contingency path: 8 B per voice-sample on the way)
            if self._rows is not None:
                raise NotImplementedError("generate_i16_device under the round() quantise variant: banks with modulation rows")
            r64 = N.DeviceBuffer(self.nvoices * stride * 8)
            N.check(N.lib().sh_bank_generate_f64(self._bank.handle, start, nframes, r64.handle, 0, stride))
            try:
                for v in range(self.nvoices):
                    N.check(N.lib().sh_quantize_f64(r64.handle, v * stride, nframes, float(scale), 2, out.handle, v * stride))
            finally:
                r64.free()
            return out, stride
        if self._rows is not None:
            rows, rstride = self._rows.fill(start, nframes)
            N.check(N.lib().sh_bank_generate_rows_i16(self._bank.handle, start, nframes, rows.handle, rstride, float(scale), out.handle, stride))
        else:
            fn = N.lib().sh_bank_generate_i16 if check else N.lib().sh_bank_generate_i16_async
            N.check(fn(self._bank.handle, start, nframes, float(scale), out.handle, stride))
        return out, stride

    @staticmethod
    def overflow_check() -> None:
        """OverflowError if a ``generate_i16_device(..., check=False)`` since the last check met a sample that does not fit."""
        N.check(N.lib().sh_overflow_check())

    def voice_samples(self, nframes: int, start: int = 0, scale: float = 32767.0) -> List[Sample]:
        """The voices as mono int16 Samples (views of one matrix in HBM): ``[Sample.from_osc_block(voice block) ...]``."""
        buf, stride = self.generate_i16_device(nframes, start, scale)
        out = []
        for v in range(self.nvoices):
            s = Sample(samplerate=self.samplerate, nchannels=1, samplewidth=2)
            if nframes:
                s._set_device(buf.view(v * stride * 2, nframes * 2), nframes * 2)
                s._share_device()                              # (a window of the shared matrix: never written in place)
            out.append(s)
        return out

    def mixdown_i16_device(self, nframes: int, start: int = 0, scale: float = 32767.0,
                           out: Optional[N.DeviceBuffer] = None, check: bool = True, two_step: bool = False) -> N.DeviceBuffer:
        """The mono mixdown the reference's mixer makes of the voices: every voice quantised (``from_osc_block``), then
        ``mixed = audioop.add(mixed, voice, 2)`` down the voices in order.  nframes int16 samples.  The library folds the samples
        into the chain where they are made wherever it can (``sh_bank_mixdown_i16``); ``two_step=True`` materialises the int16 rows
        and runs the chain kernel over them -- the same bytes."""
        if out is None:
            out = N.DeviceBuffer(max(nframes * 2, 4))
        if nframes == 0:
            return out
        if two_step or self._rows is not None or params.variants["quantise"] == "round":
            rows, stride = self.generate_i16_device(nframes, start, scale, check=check)
            N.check(N.lib().sh_mix_chain_i16(rows.handle, self.nvoices, stride, nframes, out.handle))
            rows.free()
            return out
        fn = N.lib().sh_bank_mixdown_i16 if check else N.lib().sh_bank_mixdown_i16_async
        N.check(fn(self._bank.handle, start, nframes, float(scale), out.handle))
        return out

    def mixdown_i16_parts_device(self, nframes: int, start: int = 0, scale: float = 32767.0, stereo: bool = False,
                                 out: Optional[N.DeviceBuffer] = None) -> N.DeviceBuffer:
        """``mixdown_i16_device`` (``stereo``: ``mixdown_stereo_i16_device``) as the chain's MAP instead of its result: one
        ``sh_chain_map`` (chainmaps.CHAIN_MAP_DTYPE, 8 bytes) per int16 value -- nframes maps, or 2 * nframes interleaved L / R.
        The maps of consecutive banks applied in order (``apply_chain_parts``) give the mixdown of their voices concatenated."""
        nvalues = nframes * (2 if stereo else 1)
        if out is None:
            out = N.DeviceBuffer(max(nvalues * 8, 8))
        if nframes == 0:
            return out
        L = N.lib()
        if stereo or self._rows is not None or params.variants["quantise"] == "round":
            rows, stride = self.generate_i16_device(nframes, start, scale)
            try:
                if stereo:
                    N.check(L.sh_mix_chain_pan_i16_parts(rows.handle, self.nvoices, stride, nframes, self.pan_factors_device().handle, out.handle))
                else:
                    N.check(L.sh_mix_chain_i16_parts(rows.handle, self.nvoices, stride, nframes, out.handle))
            finally:
                rows.free()
            return out
        N.check(L.sh_bank_mixdown_i16_parts(self._bank.handle, start, nframes, float(scale), out.handle))
        return out

    def pan_factors_device(self) -> N.DeviceBuffer:
        if self._pan_dev is None:
            self._pan_dev = N.DeviceBuffer.from_array(np.asarray(self.gains, dtype=np.float64).reshape(-1))
        return self._pan_dev

    def mixdown_stereo_i16_device(self, nframes: int, start: int = 0, scale: float = 32767.0,
                                  out: Optional[N.DeviceBuffer] = None) -> N.DeviceBuffer:
        """The stereo mixdown the reference's mixer makes: every voice quantised (``from_osc_block``), placed with
        ``Sample.stereo(left, right)`` (``audioop.tostereo`` with the voice's gains as factors), then the saturating
        ``audioop.add`` chain in voice order.  nframes x 2 int16, interleaved."""
        rows, stride = self.generate_i16_device(nframes, start, scale)
        if out is None:
            out = N.DeviceBuffer(max(nframes * 4, 4))
        if nframes:
            N.check(N.lib().sh_mix_chain_pan_i16(rows.handle, self.nvoices, stride, nframes, self.pan_factors_device().handle, out.handle))
        rows.free()
        return out

    def gains_device(self) -> N.DeviceBuffer:
        if self._gains_dev is None:
            self._gains_dev = N.DeviceBuffer.from_array(np.asarray(self.gains, dtype=np.float32).reshape(-1))
        return self._gains_dev

    def mix_device(self, voices: N.DeviceBuffer, nframes: int, stride: Optional[int] = None,
                   bus_f32: Optional[N.DeviceBuffer] = None) -> N.DeviceBuffer:
        """Sum materialised voices to the stereo bus (HBM-bound: 4*N + 8 bytes per frame)."""
        stride = nframes if stride is None else stride
        if bus_f32 is None:
            bus_f32 = N.DeviceBuffer(nframes * 8)
        N.check(N.lib().sh_mix_bus_f32(voices.handle, self.nvoices, stride, nframes,
                                       self.gains_device().handle, bus_f32.handle))
        return bus_f32

    def render_two_step(self, nframes: int, start: int = 0) -> np.ndarray:
        v = self.generate_device(nframes, start)
        bus = self.mix_device(v, nframes)
        out = bus.download(np.float32, nframes * 2).reshape(nframes, 2)
        v.free()
        bus.free()
        return out


def mix_bus(voices: np.ndarray, gains: Sequence[Tuple[float, float]]) -> np.ndarray:
    """[nvoices, nframes] float32 voices -> [nframes, 2] float32 bus (host arrays in and out)."""
    voices = np.ascontiguousarray(voices, dtype=np.float32)
    nv, nf = voices.shape
    vb = N.DeviceBuffer.from_array(voices)
    gb = N.DeviceBuffer.from_array(np.asarray(gains, dtype=np.float32).reshape(-1))
    bus = N.DeviceBuffer(max(nf, 1) * 8)
    N.check(N.lib().sh_mix_bus_f32(vb.handle, nv, nf, nf, gb.handle, bus.handle))
    out = bus.download(np.float32, nf * 2).reshape(nf, 2)
    for b in (vb, gb, bus):
        b.free()
    return out


def _chain_planes(parts: Union[N.DeviceBuffer, Sequence[N.DeviceBuffer]], nvalues: int) -> Tuple[Optional[N.DeviceBuffer], int, bool]:
    """(buffer of consecutive planes of nvalues maps, number of planes, temporary?): a sequence of buffers is copied into one."""
    if isinstance(parts, N.DeviceBuffer):
        nparts = parts.nbytes // (nvalues * 8) if nvalues else 0
        return parts, nparts, False
    parts = list(parts)
    if not parts or nvalues == 0:
        return None, 0, False
    planes = N.DeviceBuffer(len(parts) * nvalues * 8)
    for k, p in enumerate(parts):
        N.check(N.lib().sh_buf_copy(planes.handle, k * nvalues * 8, p.handle, 0, nvalues * 8))
    return planes, len(parts), True


def compose_chain_parts(parts: Union[N.DeviceBuffer, Sequence[N.DeviceBuffer]], nvalues: int,
                        out: Optional[N.DeviceBuffer] = None) -> N.DeviceBuffer:
    """Chain maps of consecutive voice ranges (a list of buffers of ``nvalues`` maps, or one buffer of such planes back to back),
    folded in order into ONE map per value (``sh_chain_parts_compose``)."""
    planes, nparts, tmp = _chain_planes(parts, nvalues)
    if out is None:
        out = N.DeviceBuffer(max(nvalues * 8, 8))
    N.check(N.lib().sh_chain_parts_compose(planes.handle if planes is not None else None, nparts, nvalues, nvalues, out.handle))
    if tmp:
        planes.free()
    return out


def apply_chain_parts(parts: Union[N.DeviceBuffer, Sequence[N.DeviceBuffer]], nvalues: int,
                      x0: Optional[Union[N.DeviceBuffer, Sample]] = None, out: Optional[N.DeviceBuffer] = None) -> N.DeviceBuffer:
    """Chain maps of consecutive voice ranges applied in order to ``x0`` (nvalues int16 in a device buffer, or a 16-bit Sample's
    frames; None: silence) -> nvalues int16: ``audioop.add(x0, voice)`` down every voice of every range (``sh_chain_parts_apply``)."""
    if isinstance(x0, Sample):
        if x0.samplewidth != 2 or len(x0) * x0.nchannels < nvalues:
            raise ValueError("x0 must be a 16-bit sample of at least nvalues samples")
        x0 = x0._device()
    planes, nparts, tmp = _chain_planes(parts, nvalues)
    if out is None:
        out = N.DeviceBuffer(max(nvalues * 2, 4))
    N.check(N.lib().sh_chain_parts_apply(planes.handle if planes is not None else None, nparts, nvalues, nvalues,
                                         x0.handle if x0 is not None else None, out.handle))
    if tmp:
        planes.free()
    return out


def mixdown_i16_banks(banks: Sequence[VoiceBank], nframes: int, start: int = 0, scale: float = 32767.0,
                      stereo: bool = False) -> Sample:
    """The reference's int16 mixdown of the banks' voices concatenated in order (mono, or ``stereo`` with every voice placed by its
    gains): each bank leaves its chain maps in one plane of a shared buffer, one launch applies the planes to silence.  Covers
    tables of any size (a bank holds at most 32 768 voices for the integer routes)."""
    if not banks:
        raise ValueError("no banks to mix")
    rates = {b.samplerate for b in banks}
    if len(rates) != 1:
        raise ValueError("all banks must share one sample rate")
    nch = 2 if stereo else 1
    s = Sample(samplerate=rates.pop(), nchannels=nch, samplewidth=2)
    nvalues = nframes * nch
    if nframes == 0:
        return s
    planes = N.DeviceBuffer(len(banks) * nvalues * 8)
    for k, b in enumerate(banks):
        b.mixdown_i16_parts_device(nframes, start, scale, stereo, out=planes.view(k * nvalues * 8, nvalues * 8))
    out = apply_chain_parts(planes, nvalues)
    planes.free()
    s._set_device(out, nvalues * 2)
    return s


def _gather(sources: Sequence[Tuple[N.DeviceBuffer, int, int]], nsamples: int, out: N.DeviceBuffer, width: int = 2,
            out_sample_off: int = 0) -> None:
    """out[out_sample_off : +nsamples] = ordered saturating fold of (buffer, first sample, samples available) sources of
    `width`-byte samples: mixed = audioop.add(mixed, chunk, width) down the list."""
    n = len(sources)
    bufs = (C.c_void_p * max(n, 1))(*[b.handle for b, _o, _n in sources])
    offs = (C.c_size_t * max(n, 1))(*[o for _b, o, _n in sources])
    lens = (C.c_uint32 * max(n, 1))(*[min(k, 0xFFFFFFFF) for _b, _o, k in sources])
    N.check(N.lib().sh_mix_chain_gather(bufs, offs, lens, n, nsamples, width, out.handle, out_sample_off))


def mix_samples(samples: Sequence[Sample], name: str = "mix") -> Sample:
    """The real-time mixer's fold over whole samples: pad every voice with silence to the longest,
    then ``mixed = add(mixed, voice)`` in the given order, saturating at every step."""
    if not samples:
        raise ValueError("nothing to mix")
    first = samples[0]
    for s in samples[1:]:
        assert s.samplewidth == first.samplewidth and s.samplerate == first.samplerate and s.nchannels == first.nchannels
    width = first.samplewidth
    nbytes = max(len(s) for s in samples) * width * first.nchannels
    out = Sample(name=name, samplerate=first.samplerate, nchannels=first.nchannels, samplewidth=width)
    if nbytes == 0:
        return out
    nsamples = nbytes // width
    dst = N.DeviceBuffer(nbytes)
    _gather([(s._device(), 0, len(s) * s.nchannels) for s in samples], nsamples, dst, width)
    out._set_device(dst, nbytes)
    return out


def sequence(events: Sequence[tuple], samplerate: int, nchannels: int, samplewidth: int = 2, name: str = "") -> Sample:
    """A track made of placed samples: a new empty ``Sample`` of the given format with ``events`` -- ``(seconds, sample,
    volume=None, sample_seconds=None, speed=None, pan=None, envelope=None, loop=None, region=None, reverse=None, channels=None)`` each -- mixed in by
    ``Sample.mix_at_many``: in list order, saturating at every event; ``region`` -- ``(start, end)``, seconds of the sample's own time, ``end``
    may be None -- plays a slice of the sample and ``reverse`` plays it backwards (``Sample.reverse``: a stereo sample's channels change
    places), both before everything else and without a copy per slice; ``loop`` -- ``(loop_start, loop_end, length)``, seconds of the sample's own time -- holds the
    (clipped, reversed) sample's loop region until the note is ``length`` long, next; ``speed`` plays the sample faster or slower (``Sample.speed``: one recorded note at many pitches),
    ``envelope`` -- ``(attack, decay, sustainlevel, release)`` or with a fifth element, the note's length -- shapes the (resampled, cut)
    sample as ``Sample.envelope`` does, ``pan`` places a mono sample in the stereo field of a stereo track (``Sample.pan``, or the
    factor pair of ``Sample.stereo``), ``channels`` -- ``(left_factor, right_factor)`` -- weighs the two channels of a STEREO sample in
    pan's place (``Sample.mono`` into a mono track, ``Sample.stereo``'s balance in a stereo one), all of them before ``volume`` applies,
    in that order."""
    track = Sample(name=name, samplerate=samplerate, nchannels=nchannels, samplewidth=samplewidth)
    return track.mix_at_many(events)


class Levels:
    """The levels of one track, or of the master, in one rendered window of a song of tracks (``CompiledSequence.render(meters=True)``):
    per channel, as ``(left, right)`` tuples, ``peak`` (``audioop.max``), ``sum_squares`` (the exact integer sum of x * x, a Python int),
    ``rms`` (``int(sqrt(sum_squares / frames))``, as ``Sample.rms`` forms it; 0 for an empty window) and ``level_db_peak`` /
    ``level_db_rms`` by ``Sample.level_db_peak``'s formula, ``20 log10((v + 1) / 2^(8 w - 1))`` and not below -60.  A mono song gives
    ``left == right``, as ``Sample`` does.  It has what ``LevelMeter.update`` reads of a ``Sample`` (the two levels and ``duration``).
    ``clipped``: None, or (a render with ``clips=True``) the OVERS as a ``(left, right)`` tuple of ints, with the mono rule of ``peak``:
    the number of samples at which the row's own arithmetic was clamped (``CompiledSequence`` has the definition).  Two ``Levels``
    compare their counts only where both have them."""

    def __init__(self, peak, sum_squares, frames: int, samplewidth: int, nchannels: int, samplerate: int, clipped=None) -> None:
        both = (lambda v: (int(v[0]), int(v[1]))) if nchannels == 2 else (lambda v: (int(v[0]), int(v[0])))
        self.peak = both(peak)
        self.sum_squares = both(sum_squares)
        self.clipped = None if clipped is None else both(clipped)
        self.frames, self.samplewidth, self.nchannels, self.samplerate = int(frames), int(samplewidth), int(nchannels), int(samplerate)

    @property
    def duration(self) -> float:
        return self.frames / self.samplerate

    @property
    def rms(self) -> Tuple[int, int]:
        if not self.frames:
            return 0, 0
        return int(math.sqrt(self.sum_squares[0] / self.frames)), int(math.sqrt(self.sum_squares[1] / self.frames))

    def _db(self, values) -> Tuple[float, float]:
        maxvalue = 2 ** (8 * self.samplewidth - 1)
        # cut off at -60 dB instead of running down to -infinity
        return max(20.0 * math.log((values[0] + 1) / maxvalue, 10), -60.0), max(20.0 * math.log((values[1] + 1) / maxvalue, 10), -60.0)

    @property
    def level_db_peak(self) -> Tuple[float, float]:
        return self._db(self.peak)

    @property
    def level_db_rms(self) -> Tuple[float, float]:
        return self._db(self.rms)

    def __eq__(self, other) -> bool:
        return isinstance(other, Levels) and (self.peak, self.sum_squares, self.frames, self.samplewidth, self.nchannels) == (
            other.peak, other.sum_squares, other.frames, other.samplewidth, other.nchannels) and (
            self.clipped is None or other.clipped is None or self.clipped == other.clipped)

    def __repr__(self) -> str:
        if self.clipped is not None:
            return "Levels(peak=%r, sum_squares=%r, frames=%d, clipped=%r)" % (self.peak, self.sum_squares, self.frames, self.clipped)
        return "Levels(peak=%r, sum_squares=%r, frames=%d)" % (self.peak, self.sum_squares, self.frames)


class SongLevels:
    """What a metered render returns beside its bytes: ``tracks``, one ``Levels`` per track, POST-fader (over the track as the master takes
    it: folded on its own, times its gain; a muted track reads zero), and ``master``, over the window's output -- all from the one launch
    that rendered the window.  ``groups``: one ``Levels`` per group bus of a render with ``groups=``, over the bus as the master takes it
    (behind the group's gain and pan); empty without groups.  ``rows``: ``N.Sequence.render(meters=True)``'s -- the tracks, the master,
    then the ``ngroups`` groups; a row is ``(peak, sum_squares)`` or, with overs, ``(peak, sum_squares, clipped)``."""

    def __init__(self, rows, frames: int, samplewidth: int, nchannels: int, samplerate: int, ngroups: int = 0) -> None:
        made = [Levels(row[0], row[1], frames, samplewidth, nchannels, samplerate, row[2] if len(row) > 2 else None) for row in rows]
        at = len(made) - 1 - ngroups
        self.tracks: List[Levels] = made[:at]
        self.master: Levels = made[at]
        self.groups: List[Levels] = made[at + 1:]

    def __eq__(self, other) -> bool:
        return isinstance(other, SongLevels) and (self.tracks, self.master, self.groups) == (other.tracks, other.master, other.groups)

    def __repr__(self) -> str:
        if self.groups:
            return "SongLevels(tracks=%r, master=%r, groups=%r)" % (self.tracks, self.master, self.groups)
        return "SongLevels(tracks=%r, master=%r)" % (self.tracks, self.master)


def _grid_blocks(who: str, nblocks: int, first_block: int, block_frames: int, start_frame: int, frames: int) -> Tuple[List[int], List[int]]:
    """the blocks of a window on the song's frame grid, checked: where each block's counted range begins and the frames it counts"""
    end = start_frame + frames
    want = (end - 1) // block_frames - start_frame // block_frames + 1 if frames > 0 else 0
    if block_frames <= 0 or nblocks != want or (nblocks and first_block != start_frame // block_frames):
        raise ValueError("%s: %d blocks of %d frames from block %d for frames [%d, %d)" % (who, nblocks, block_frames, first_block, start_frame, end))
    edges = (first_block + np.arange(nblocks + 1, dtype=np.int64)) * block_frames      # the song's grid, cut to the window
    lows, highs = np.maximum(edges[:-1], start_frame), np.minimum(edges[1:], end)
    return lows.tolist(), (highs - lows).tolist()


def _fold_cuts(first_block: int, nblocks: int, n: int) -> List[int]:
    """where ``nblocks`` blocks from song block ``first_block`` on are cut when merged by ``song block index // n``"""
    return [0] + [j for j in range(1, nblocks) if (first_block + j) % n == 0] + [nblocks]


class SongHistory:
    """The levels of a rendered window OVER TIME (``CompiledSequence.render(meters="history")``): one ``SongLevels`` per BLOCK, all from the
    one launch that rendered the window.  Blocks are anchored to the SONG, not to the window: block index ``i`` covers song frames
    ``[i * block_frames, (i + 1) * block_frames)``, cut to the window, so the first and the last block of a window may be partial and a
    block that lies whole inside two windows reads the same from both.  As rendered, ``block_frames`` is one tile of the song's grid
    (2048 samples at 16 bits, 1024 at the other widths, over the channels); ``fold(n)`` gives coarser ones.

    ``start_frame``, ``frames``: the window.  ``nblocks`` (``len()``).  ``starts[j]``: the song frame where block ``j``'s counted range
    begins.  ``history[j]`` (``self[j]``): block ``j``'s ``SongLevels``, whose ``Levels.frames`` is the number of frames counted in that
    block, so ``rms`` is right in a partial one.  ``total()``: the window's ``SongLevels``, equal to what ``meters=True`` returns for it.
    ``peaks()``: the peaks as a numpy array ``(nblocks, nrows, 2)``, rows in table order (tracks, master, groups), for drawing; a mono
    song has ``left == right`` there as in ``Levels``.  ``peak`` (uint32) and ``sum_squares`` (Python ints) are the arrays behind them,
    shaped ``(nblocks, nrows, 2)``, a mono song's channel 1 reading 0.  A rendered history keeps the table as it came back (``parts``:
    the two 64-bit sums of every row) and forms Python ints where they are asked for -- a block that is indexed, ``total()``,
    ``fold(n)``, ``sum_squares`` -- so that the render's call costs no pass over the table in Python.
    A history rendered with ``clips=True`` carries the OVERS as well: ``clipped()`` is a numpy array ``(nblocks, nrows, 2)`` of counts,
    rows and the mono rule as ``peaks()`` has them (None without counts); every block's ``Levels.clipped`` holds its row's, and
    ``total()`` and ``fold(n)`` add the counts."""

    def __init__(self, peak, sum_squares, first_block: int, block_frames: int, start_frame: int, frames: int, samplewidth: int, nchannels: int,
                 samplerate: int, ngroups: int = 0, parts=None, clipped=None) -> None:
        self.peak = np.asarray(peak, dtype=np.uint32)
        self._clipped = None if clipped is None else np.asarray(clipped, dtype=np.uint64)       # (a mono song's channel 1 reads 0, as peak's)
        if self._clipped is not None and self._clipped.shape != self.peak.shape:
            raise ValueError("SongHistory: clipped is an (nblocks, nrows, 2) array as peak is")
        self._parts = None if parts is None else (np.asarray(parts[0], dtype=np.uint64), np.asarray(parts[1], dtype=np.uint64))
        self._sq = None if sum_squares is None else np.asarray(sum_squares, dtype=object)
        held = [a.shape for a in (self._sq,) + (self._parts or ()) if a is not None]
        if self.peak.ndim != 3 or self.peak.shape[2] != 2 or not held or any(shape != self.peak.shape for shape in held):
            raise ValueError("SongHistory: peak and sum_squares are (nblocks, nrows, 2) arrays")
        self.first_block, self.block_frames = int(first_block), int(block_frames)
        self.start_frame, self.frames = int(start_frame), int(frames)
        self.samplewidth, self.nchannels, self.samplerate, self.ngroups = int(samplewidth), int(nchannels), int(samplerate), int(ngroups)
        self.nblocks = int(self.peak.shape[0])
        self.starts, self.block_counts = _grid_blocks("SongHistory", self.nblocks, self.first_block, self.block_frames, self.start_frame, self.frames)
        self.history = self

    @classmethod
    def from_blocks(cls, blocks, nrows: int, tile_samples: int, start_frame: int, frames: int, samplewidth: int, nchannels: int, samplerate: int,
                    ngroups: int = 0, clips: bool = False) -> "SongHistory":
        """``of_blocks`` on the grid of a song's tile: ``tile_samples`` samples over the channels"""
        return cls.of_blocks(blocks, nrows, tile_samples // nchannels, start_frame, frames, samplewidth, nchannels, samplerate, ngroups, clips)

    @classmethod
    def of_blocks(cls, blocks, nrows: int, block_frames: int, start_frame: int, frames: int, samplewidth: int, nchannels: int, samplerate: int,
                  ngroups: int = 0, clips: bool = False) -> "SongHistory":
        """``blocks``: an array ``(nblocks, nrows)`` of sh_seq_meter rows on the grid of ``block_frames`` -- ``N.Sequence.render(meters=
        "history")``'s or ``N.pcm_level_blocks``' (with ``clips=True`` the render's are sh_seq_meter_clips rows: the field ``clipped`` says
        so) -- or None for an empty window, whose history has counts where ``clips``"""
        counted = clips if blocks is None else "clipped" in (blocks.dtype.names or ())
        first = start_frame // block_frames
        if blocks is None or not len(blocks):
            empty = np.zeros((0, nrows, 2), dtype=np.uint64)
            return cls(empty, None, first, block_frames, start_frame, frames, samplewidth, nchannels, samplerate, ngroups, parts=(empty, empty),
                       clipped=empty if counted else None)
        peak, hi, lo = blocks["peak"], blocks["sq_hi"], blocks["sq_lo"]
        clipped = blocks["clipped"] if counted else None
        if frames * nchannels >= 1 << 32:
            # _sums adds a table's two 64-bit sums 2^20 blocks at a time in uint64, which holds while a channel of the window has fewer
            # than 2^32 samples (a sum is below 2^32 a sample); a longer window hands over Python ints
            return cls(peak, (hi.astype(object) << 32) + lo.astype(object), first, block_frames, start_frame, frames, samplewidth, nchannels,
                       samplerate, ngroups, clipped=clipped)
        return cls(peak, None, first, block_frames, start_frame, frames, samplewidth, nchannels, samplerate, ngroups, parts=(hi, lo), clipped=clipped)

    @property
    def sum_squares(self) -> np.ndarray:
        if self._sq is None:                                    # Python ints: a sum passes 2^64 at width 4
            self._sq = (self._parts[0].astype(object) << 32) + self._parts[1].astype(object)
        return self._sq

    def __len__(self) -> int:
        return self.nblocks

    def _rows(self, peak, sq, clipped=None) -> list:
        if clipped is not None:
            return [((int(p[0]), int(p[1])), (int(q[0]), int(q[1])), (int(c[0]), int(c[1]))) for p, q, c in zip(peak, sq, clipped)]
        return [((int(p[0]), int(p[1])), (int(q[0]), int(q[1]))) for p, q in zip(peak, sq)]

    def __getitem__(self, j: int) -> SongLevels:
        j = operator.index(j)
        if j < -self.nblocks or j >= self.nblocks:
            raise IndexError("SongHistory: block %d of %d" % (j, self.nblocks))
        j %= self.nblocks
        sq = self._sq[j] if self._sq is not None else [((int(h[0]) << 32) + int(lo[0]), (int(h[1]) << 32) + int(lo[1]))
                                                       for h, lo in zip(self._parts[0][j], self._parts[1][j])]
        return SongLevels(self._rows(self.peak[j], sq, None if self._clipped is None else self._clipped[j]), self.block_counts[j], self.samplewidth,
                          self.nchannels, self.samplerate, self.ngroups)

    def __iter__(self):
        return (self[j] for j in range(self.nblocks))

    def _sums(self, a: int, b: int) -> np.ndarray:
        """the sums of blocks ``[a, b)`` added up, ``(nrows, 2)`` Python ints.  A rendered table's two 64-bit parts are added apart, 2^20
        blocks at a time in uint64 (a block is at most 2048 samples: a part stays below 2^43, 2^20 of them below 2^63), then as ints."""
        if self._sq is not None:
            return self._sq[a:b].sum(axis=0)
        hi = lo = np.zeros(self.peak.shape[1:], dtype=object)
        for at in range(a, b, 1 << 20):
            hi = hi + self._parts[0][at:min(b, at + (1 << 20))].sum(axis=0, dtype=np.uint64).astype(object)
            lo = lo + self._parts[1][at:min(b, at + (1 << 20))].sum(axis=0, dtype=np.uint64).astype(object)
        return (hi << 32) + lo

    def total(self) -> SongLevels:
        """the whole window's levels: max of the peaks, sum of the sums (an empty window: every level 0)"""
        if not self.nblocks:
            zero = ((0, 0), (0, 0)) if self._clipped is None else ((0, 0), (0, 0), (0, 0))
            return SongLevels([zero] * self.peak.shape[1], 0, self.samplewidth, self.nchannels, self.samplerate, self.ngroups)
        counts = None if self._clipped is None else self._clipped.sum(axis=0, dtype=np.uint64)
        return SongLevels(self._rows(self.peak.max(axis=0), self._sums(0, self.nblocks), counts), self.frames, self.samplewidth, self.nchannels,
                          self.samplerate, self.ngroups)

    def fold(self, n: int) -> "SongHistory":
        """Blocks ``n`` times as long: the blocks merged by ``song block index // n``, so that the result does not depend on where the
        window began -- peaks take the max, sums add as Python ints, frames add."""
        n = operator.index(n)
        if n <= 0:
            raise ValueError("SongHistory: fold(n) needs a positive n")
        if not self.nblocks:
            return SongHistory(self.peak, self.sum_squares, 0, self.block_frames * n, self.start_frame, self.frames, self.samplewidth, self.nchannels,
                               self.samplerate, self.ngroups, clipped=self._clipped)
        first = self.first_block // n
        cuts = _fold_cuts(self.first_block, self.nblocks, n)
        peak = np.stack([self.peak[a:b].max(axis=0) for a, b in zip(cuts, cuts[1:])])
        sq = np.stack([self._sums(a, b) for a, b in zip(cuts, cuts[1:])])
        counts = None if self._clipped is None else np.stack([self._clipped[a:b].sum(axis=0, dtype=np.uint64) for a, b in zip(cuts, cuts[1:])])
        return SongHistory(peak, sq, first, self.block_frames * n, self.start_frame, self.frames, self.samplewidth, self.nchannels, self.samplerate,
                           self.ngroups, clipped=counts)

    def peaks(self) -> np.ndarray:
        out = self.peak.copy()
        if self.nchannels != 2:
            out[:, :, 1] = out[:, :, 0]
        return out

    def clipped(self) -> Optional[np.ndarray]:
        """the overs per block, row and channel (a history rendered with ``clips=True``; None otherwise)"""
        if self._clipped is None:
            return None
        out = self._clipped.copy()
        if self.nchannels != 2:
            out[:, :, 1] = out[:, :, 0]
        return out

    def __repr__(self) -> str:
        return "SongHistory(%d blocks of %d frames, frames [%d, %d))" % (self.nblocks, self.block_frames, self.start_frame, self.start_frame + self.frames)


class Waveform:
    """The waveform EXTREMES of a window OVER TIME, for drawing (``Sample.waveform``, ``SongStems.waveform``, ``CompiledSequence.waveform``):
    per block, row and channel the smallest and the largest sample, ``lo`` and ``hi`` -- ``audioop.minmax`` of that channel's samples in
    that block, signed values of the sample width -- read off the samples in device memory in one launch.  What a peak row cannot say is
    here: a DC offset, a half-wave, which way a transient points.  Blocks are anchored to the SONG as ``SongHistory``'s are: block index
    ``i`` covers song frames ``[i * block_frames, (i + 1) * block_frames)`` cut to the window, so the first and the last block may be
    partial and a block that lies whole inside two windows reads the same from both.

    ``lo``, ``hi``: int32 arrays ``(nblocks, nrows, 2)``, rows in table order (tracks, master, groups; one row for a ``Sample``), a
    mono input's channel 1 reading 0.  ``start_frame``, ``frames``, ``first_block``, ``block_frames``, ``nblocks`` (``len()``),
    ``starts``, ``block_counts``, ``samplewidth``, ``nchannels``, ``samplerate``, ``ngroups``: as ``SongHistory`` has them.
    ``extents()``: ``(nblocks, nrows, 2, 2)`` as ``[..., channel, (lo, hi)]``, a mono input's channel 1 a copy of channel 0 -- the pairs
    to draw; ``self[j]``: block ``j``'s ``(nrows, 2, 2)`` of them.  ``peaks()``: ``max(-lo, hi)`` as uint32, ``SongHistory.peaks()`` of
    the same call (``|-32768|`` is 32768).  ``total()``: the window's ``(lo, hi)``, each ``(nrows, 2)``.  ``fold(n)``: blocks ``n`` times
    as long, the zoom."""

    def __init__(self, lo, hi, first_block: int, block_frames: int, start_frame: int, frames: int, samplewidth: int, nchannels: int,
                 samplerate: int, ngroups: int = 0) -> None:
        self.lo, self.hi = np.asarray(lo, dtype=np.int32), np.asarray(hi, dtype=np.int32)
        if self.lo.ndim != 3 or self.lo.shape[2] != 2 or self.hi.shape != self.lo.shape:
            raise ValueError("Waveform: lo and hi are (nblocks, nrows, 2) arrays")
        self.first_block, self.block_frames = int(first_block), int(block_frames)
        self.start_frame, self.frames = int(start_frame), int(frames)
        self.samplewidth, self.nchannels, self.samplerate, self.ngroups = int(samplewidth), int(nchannels), int(samplerate), int(ngroups)
        self.nblocks = int(self.lo.shape[0])
        self.starts, self.block_counts = _grid_blocks("Waveform", self.nblocks, self.first_block, self.block_frames, self.start_frame, self.frames)

    @classmethod
    def of_blocks(cls, blocks, nrows: int, block_frames: int, start_frame: int, frames: int, samplewidth: int, nchannels: int, samplerate: int,
                  ngroups: int = 0) -> "Waveform":
        """``blocks``: ``N.pcm_extent_blocks``' array ``(nblocks, nrows)`` of sh_pcm_extent rows on the grid of ``block_frames``, or None
        for an empty window"""
        if blocks is None or not len(blocks):
            empty = np.zeros((0, nrows, 2), dtype=np.int32)
            return cls(empty, empty, start_frame // block_frames, block_frames, start_frame, frames, samplewidth, nchannels, samplerate, ngroups)
        return cls(blocks["lo"], blocks["hi"], start_frame // block_frames, block_frames, start_frame, frames, samplewidth, nchannels, samplerate, ngroups)

    def __len__(self) -> int:
        return self.nblocks

    def _both(self, a: np.ndarray) -> np.ndarray:
        """a copy with a mono input's channel 0 in channel 1 as well"""
        out = a.copy()
        if self.nchannels != 2:
            out[..., 1] = out[..., 0]
        return out

    def extents(self) -> np.ndarray:
        return np.stack([self._both(self.lo), self._both(self.hi)], axis=-1)

    def __getitem__(self, j: int) -> np.ndarray:
        j = operator.index(j)
        if j < -self.nblocks or j >= self.nblocks:
            raise IndexError("Waveform: block %d of %d" % (j, self.nblocks))
        j %= self.nblocks
        return np.stack([self._both(self.lo[j]), self._both(self.hi[j])], axis=-1)

    def __iter__(self):
        return (self[j] for j in range(self.nblocks))

    def peaks(self) -> np.ndarray:
        return self._both(np.maximum(-self.lo.astype(np.int64), self.hi.astype(np.int64)).astype(np.uint32))

    def _identity(self) -> Tuple[np.ndarray, np.ndarray]:
        """``audioop.minmax`` of no sample per row and channel -- the identity of min and max -- a mono input's channel 1 reading 0"""
        lo = np.full(self.lo.shape[1:], np.iinfo(np.int32).max, dtype=np.int32)
        hi = np.full(self.lo.shape[1:], np.iinfo(np.int32).min, dtype=np.int32)
        if self.nchannels != 2:
            lo[:, 1] = hi[:, 1] = 0
        return lo, hi

    def total(self) -> Tuple[np.ndarray, np.ndarray]:
        """the whole window's ``(lo, hi)``, each ``(nrows, 2)``: min of the lows, max of the highs (an empty window: what
        ``audioop.minmax`` gives for no sample, 2^31 - 1 and -2^31)"""
        if not self.nblocks:
            return self._identity()
        return self.lo.min(axis=0), self.hi.max(axis=0)

    def fold(self, n: int) -> "Waveform":
        """Blocks ``n`` times as long: the blocks merged by ``song block index // n``, so that the result does not depend on where the
        window began -- min of ``lo``, max of ``hi``."""
        n = operator.index(n)
        if n <= 0:
            raise ValueError("Waveform: fold(n) needs a positive n")
        if not self.nblocks:
            return Waveform(self.lo, self.hi, 0, self.block_frames * n, self.start_frame, self.frames, self.samplewidth, self.nchannels,
                            self.samplerate, self.ngroups)
        cuts = _fold_cuts(self.first_block, self.nblocks, n)
        lo = np.stack([self.lo[a:b].min(axis=0) for a, b in zip(cuts, cuts[1:])])
        hi = np.stack([self.hi[a:b].max(axis=0) for a, b in zip(cuts, cuts[1:])])
        return Waveform(lo, hi, self.first_block // n, self.block_frames * n, self.start_frame, self.frames, self.samplewidth, self.nchannels,
                        self.samplerate, self.ngroups)

    def __repr__(self) -> str:
        return "Waveform(%d blocks of %d frames, frames [%d, %d))" % (self.nblocks, self.block_frames, self.start_frame, self.start_frame + self.frames)


def _block_frames(who: str, block_frames) -> int:
    if isinstance(block_frames, bool) or not isinstance(block_frames, (int, np.integer)) or block_frames <= 0:
        raise ValueError("%s: block_frames is a positive int, not %r" % (who, block_frames))
    return int(block_frames)


def _origin_frame(who: str, origin_frame) -> int:
    if isinstance(origin_frame, bool) or not isinstance(origin_frame, (int, np.integer)) or origin_frame < 0:
        raise ValueError("%s: origin_frame is a non-negative int, not %r" % (who, origin_frame))
    return int(origin_frame)


def _levels_format(who: str, sample: Sample, what: str = "a level history") -> None:
    if sample.nchannels not in (1, 2):
        raise ValueError("%s: %s needs a mono or stereo sample, this one has %d channels" % (who, what, sample.nchannels))
    if sample.samplewidth not in (1, 2, 3, 4):
        raise ValueError("%s: %s needs samples of 1 to 4 bytes, these have %d" % (who, what, sample.samplewidth))


def level_history(sample: Sample, block_frames: int, origin_frame: int = 0) -> SongHistory:
    """The levels of any ``Sample`` (a recording, a resampled file, a finished mix) OVER TIME, in one launch: a ``SongHistory`` with one
    row per block, the master's -- ``history[j].master`` is the ``Levels`` of block ``j``: per channel ``peak`` (``audioop.max``) and the
    exact integer ``sum_squares``, at every width.  Frame ``i`` of the sample stands at frame ``origin_frame + i`` of a grid of
    ``block_frames`` frames, so the first and the last block may be partial and the halves of a sample cut on a block boundary give the
    blocks of the whole.  ``total()``, ``fold(n)``, ``peaks()`` and ``starts`` are ``SongHistory``'s.  Mono and stereo only."""
    block_frames = _block_frames("level_history", block_frames)
    origin_frame = _origin_frame("level_history", origin_frame)
    _levels_format("level_history", sample)
    frames = len(sample)
    nch, width = sample.nchannels, sample.samplewidth
    blocks = N.pcm_level_blocks(sample._device(), 0, frames, nch, width, frames * nch, 1, origin_frame, block_frames) if frames else None
    return SongHistory.of_blocks(blocks, 1, block_frames, origin_frame, frames, width, nch, sample.samplerate)


def waveform(sample: Sample, block_frames: int, origin_frame: int = 0) -> Waveform:
    """The waveform extremes of any ``Sample`` OVER TIME, in one launch: a ``Waveform`` with one row per block -- per channel the
    smallest and the largest sample of block ``j`` (``audioop.minmax``) in ``lo[j, 0]`` and ``hi[j, 0]``, at every width -- on
    ``level_history``'s grid: frame ``i`` of the sample stands at frame ``origin_frame + i`` of a grid of ``block_frames`` frames.  One
    block per pixel column draws the overview; ``fold(n)`` zooms out.  Mono and stereo only."""
    block_frames = _block_frames("waveform", block_frames)
    origin_frame = _origin_frame("waveform", origin_frame)
    _levels_format("waveform", sample, "a waveform")
    frames = len(sample)
    nch, width = sample.nchannels, sample.samplewidth
    blocks = N.pcm_extent_blocks(sample._device(), 0, frames, nch, width, frames * nch, 1, origin_frame, block_frames) if frames else None
    return Waveform.of_blocks(blocks, 1, block_frames, origin_frame, frames, width, nch, sample.samplerate)


def _convolve_call(who: str, sample: Sample, ir: Sample, factor, start_frame, nframes) -> Tuple[float, int, int]:
    """what a convolution refuses, before any call into the library: ``(factor, start_frame, nframes)`` of the checked call"""
    if sample.nchannels not in (1, 2) or ir.nchannels not in (1, 2):
        raise ValueError("%s: mono and stereo only, not %d channels under a response of %d" % (who, sample.nchannels, ir.nchannels))
    if sample.samplewidth in (3, 4):
        raise NotImplementedError("%s: %d-byte samples are not built: the exact sum needs more than a float64 there (make_16bit() first)"
                                  % (who, sample.samplewidth))
    if sample.samplewidth not in (1, 2):
        raise ValueError("%s: samples of 1 or 2 bytes, not %d" % (who, sample.samplewidth))
    if ir.samplewidth != sample.samplewidth:
        raise ValueError("%s: the response has samples of %d bytes, the sample of %d" % (who, ir.samplewidth, sample.samplewidth))
    if ir.samplerate != sample.samplerate:
        raise ValueError("%s: the response is at %d Hz, the sample at %d (resample one of them)" % (who, ir.samplerate, sample.samplerate))
    if ir.nchannels == 2 and sample.nchannels == 1:
        raise ValueError("%s: a stereo response over a mono sample: make the sample stereo first (sample.stereo())" % who)
    if len(ir) == 0:
        raise ValueError("%s: an empty response" % who)
    if len(ir) > N.PCM_FIR_MAX_TAPS:
        raise ValueError("%s: a response of %d frames: at most 2**22 = %d keep the sum exact" % (who, len(ir), N.PCM_FIR_MAX_TAPS))
    factor = 1.0 / 2 ** (8 * sample.samplewidth - 1) if factor is None else float(factor)
    if not math.isfinite(factor):
        raise ValueError("%s: the factor %r is not finite" % (who, factor))
    total = len(sample) + len(ir) - 1 if len(sample) else 0
    if isinstance(start_frame, bool) or not isinstance(start_frame, (int, np.integer)) or start_frame < 0:
        raise ValueError("%s: start_frame is a non-negative int, not %r" % (who, start_frame))
    if nframes is None:
        nframes = max(total - start_frame, 0)
    if isinstance(nframes, bool) or not isinstance(nframes, (int, np.integer)) or nframes < 0:
        raise ValueError("%s: nframes is a non-negative int or None, not %r" % (who, nframes))
    if start_frame + nframes > total:
        raise ValueError("%s: frames [%d, %d) reach past the result's %d" % (who, start_frame, start_frame + nframes, total))
    return factor, int(start_frame), int(nframes)


def convolve_into(buf: N.DeviceBuffer, byte_offset: int, sample: Sample, ir: Sample, factor: Optional[float] = None, start_frame: int = 0,
                  nframes: Optional[int] = None) -> int:
    """Frames ``[start_frame, start_frame + nframes)`` of ``convolve(sample, ir, factor)`` into the caller's device buffer from byte
    ``byte_offset`` on (``nframes`` None: to the result's end); returns the frames written.  Asynchronous; the buffer may not overlap
    ``sample``'s or ``ir``'s."""
    factor, start_frame, nframes = _convolve_call("convolve_into", sample, ir, factor, start_frame, nframes)
    if nframes:
        N.check(N.lib().sh_pcm_convolve(sample._device().handle, 0, len(sample), sample.nchannels, sample.samplewidth, ir._device().handle, 0, len(ir),
                                        ir.nchannels, factor, start_frame, nframes, buf.handle, byte_offset))
    return nframes


def convolve(sample: Sample, ir: Sample, factor: Optional[float] = None, start_frame: int = 0, nframes: Optional[int] = None) -> Sample:
    """``sample`` through the impulse response ``ir`` -- a room, a plate, a cabinet, any FIR filter -- as a new ``Sample``, computed in HBM
    in the direct form and EXACT: per channel, frame ``i`` is ``fbound(factor * sum of ir[k] * sample[i - k])``, the sum the exact integer
    and ``fbound`` ``audioop.mul``'s last step (clamp, then floor), so the bytes are those of ``numpy.convolve`` on int64 and that one
    rounding.  The whole result has ``len(sample) + len(ir) - 1`` frames; ``start_frame`` and ``nframes`` choose a window of it, whose bytes
    are that slice of the whole result's.  ``factor`` None: ``1 / 2 ** (8 * samplewidth - 1)``, a response at full scale being about
    unity.  A mono response goes over every channel; a stereo one needs a stereo sample, left over left and right over right.  Widths 1
    and 2, up to 2**22 taps.  The input is read only: a locked one is fine."""
    factor, start_frame, nframes = _convolve_call("convolve", sample, ir, factor, start_frame, nframes)
    out = Sample(name=sample.name, samplerate=sample.samplerate, nchannels=sample.nchannels, samplewidth=sample.samplewidth)
    if nframes:
        nbytes = nframes * sample.nchannels * sample.samplewidth
        buf = N.DeviceBuffer(nbytes)
        convolve_into(buf, 0, sample, ir, factor, start_frame, nframes)
        out._set_device(buf, nbytes)
    return out


def _limit_call(who: str, sample: Sample, ceiling, attack_frames, release_frames, start_frame, nframes) -> Tuple[int, int, int, int, int]:
    """what a limiter refuses, before any call into the library: ``(ceiling, attack_frames, release_frames, start_frame, nframes)`` of
    the checked call"""
    if sample.nchannels not in (1, 2):
        raise ValueError("%s: mono and stereo only, not %d channels" % (who, sample.nchannels))
    if sample.samplewidth == 3:
        raise NotImplementedError("%s: 3-byte samples are not built" % who)
    if sample.samplewidth not in (1, 2, 4):
        raise ValueError("%s: samples of 1, 2 or 4 bytes, not %d" % (who, sample.samplewidth))
    hi = 2 ** (8 * sample.samplewidth - 1) - 1
    if isinstance(ceiling, bool) or not isinstance(ceiling, (int, np.integer)) or not 1 <= ceiling <= hi:
        raise ValueError("%s: the ceiling is an int in [1, %d] (sample steps), not %r" % (who, hi, ceiling))
    for name, v in (("attack_frames", attack_frames), ("release_frames", release_frames)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= N.PCM_LIMIT_MAX_FRAMES:
            raise ValueError("%s: %s is an int in [0, 2**20 = %d], not %r" % (who, name, N.PCM_LIMIT_MAX_FRAMES, v))
    total = len(sample)
    if isinstance(start_frame, bool) or not isinstance(start_frame, (int, np.integer)) or start_frame < 0:
        raise ValueError("%s: start_frame is a non-negative int, not %r" % (who, start_frame))
    if nframes is None:
        nframes = max(total - start_frame, 0)
    if isinstance(nframes, bool) or not isinstance(nframes, (int, np.integer)) or nframes < 0:
        raise ValueError("%s: nframes is a non-negative int or None, not %r" % (who, nframes))
    if start_frame + nframes > total:
        raise ValueError("%s: frames [%d, %d) reach past the sample's %d" % (who, start_frame, start_frame + nframes, total))
    return int(ceiling), int(attack_frames), int(release_frames), int(start_frame), int(nframes)


def limit_into(buf: N.DeviceBuffer, byte_offset: int, sample: Sample, ceiling: int, attack_frames: int, release_frames: int, start_frame: int = 0,
               nframes: Optional[int] = None) -> int:
    """Frames ``[start_frame, start_frame + nframes)`` of ``limit(sample, ceiling, attack_frames, release_frames)`` into the caller's
    device buffer from byte ``byte_offset`` on (``nframes`` None: to the sample's end); returns the frames written.  Asynchronous; the
    buffer may not overlap ``sample``'s -- except as exactly the window's own bytes of it, which is the call in place."""
    ceiling, attack_frames, release_frames, start_frame, nframes = _limit_call("limit_into", sample, ceiling, attack_frames, release_frames, start_frame, nframes)
    if nframes:
        N.check(N.lib().sh_pcm_limit(sample._device().handle, 0, len(sample), sample.nchannels, sample.samplewidth, ceiling, attack_frames, release_frames,
                                     start_frame, nframes, buf.handle, byte_offset, None, 0))
    return nframes


def limit(sample: Sample, ceiling: int, attack_frames: int, release_frames: int, start_frame: int = 0, nframes: Optional[int] = None) -> Sample:
    """``sample`` under a look-ahead peak limiter -- a brick wall at ``ceiling`` sample steps -- as a new ``Sample``, computed in HBM and
    EXACT in integers.  With ``ONE = 2**30``, per frame: ``p`` the largest magnitude of the frame's channels (one gain per frame, so
    the stereo image holds), ``g = ONE`` where ``p <= ceiling``, else ``ceiling * ONE // p``; the gain ``G[i]`` is the smallest of
    ``ONE``, ``g[j] + (j - i) * s_a`` over the frames ``j >= i`` and ``g[j] + (i - j) * s_r`` over the frames ``j < i`` -- a linear ramp down
    over about ``attack_frames`` in front of a peak, a linear ramp up over about ``release_frames`` behind it, ``s = ONE`` for 0 or 1
    frames and else ``ceil(ONE / frames)``; and the sample is ``(x * G[i]) >> 30``.  No sample of the result exceeds the ceiling in
    magnitude, and a frame whose gain is ``ONE`` is untouched.  ``start_frame`` and ``nframes`` choose a window, whose bytes are that slice
    of the whole result's: peaks outside the window still shape the gain inside it.  Widths 1, 2 and 4; attack and release up to
    2**20 frames.  The input is read only: a locked one is fine."""
    ceiling, attack_frames, release_frames, start_frame, nframes = _limit_call("limit", sample, ceiling, attack_frames, release_frames, start_frame, nframes)
    out = Sample(name=sample.name, samplerate=sample.samplerate, nchannels=sample.nchannels, samplewidth=sample.samplewidth)
    if nframes:
        nbytes = nframes * sample.nchannels * sample.samplewidth
        buf = N.DeviceBuffer(nbytes)
        limit_into(buf, 0, sample, ceiling, attack_frames, release_frames, start_frame, nframes)
        out._set_device(buf, nbytes)
    return out


def limit_gain(sample: Sample, ceiling: int, attack_frames: int, release_frames: int, start_frame: int = 0, nframes: Optional[int] = None) -> np.ndarray:
    """The gain-reduction trace of ``limit``: ``G`` over the window as a numpy ``uint32`` array, one value per frame, ``2**30`` being unity
    (``G / 2**30`` is what a meter draws).  Nothing of the sample is written.  Synchronous: the array is copied back."""
    ceiling, attack_frames, release_frames, start_frame, nframes = _limit_call("limit_gain", sample, ceiling, attack_frames, release_frames, start_frame, nframes)
    if not nframes:
        return np.zeros(0, dtype=np.uint32)
    plane = N.DeviceBuffer(nframes * 4)
    try:
        N.check(N.lib().sh_pcm_limit(sample._device().handle, 0, len(sample), sample.nchannels, sample.samplewidth, ceiling, attack_frames, release_frames,
                                     start_frame, nframes, None, 0, plane.handle, 0))
        return plane.download(np.uint32, nframes)
    finally:
        plane.free()


def lowpass_taps(up: int, down: int, zero_crossings: int = 16, beta: float = 8.6) -> np.ndarray:
    """The default tap bank of ``resample_fir`` for the ratio ``up / down``, designed on the host: a Kaiser-windowed sinc cut at the lower
    of the two Nyquist frequencies, as int16 with unity at ``2**14`` -- ``q = max(up, down)``, ``m = 2 * zero_crossings * q + 1`` taps,
    ``h[k] = rint(2**14 * (up / q) * sinc((k - (m - 1) / 2) / q) * kaiser(m, beta)[k])``.  Symmetric; its largest tap is 16384 where
    ``up >= down``.  With ``factor = 2**-14`` and ``delay = (m - 1) // 2`` the converted signal keeps its level and its place in time."""
    for name, v in (("up", up), ("down", down), ("zero_crossings", zero_crossings)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError("lowpass_taps: %s is a positive int, not %r" % (name, v))
    q = max(int(up), int(down))
    m = 2 * int(zero_crossings) * q + 1
    if m > N.PCM_RESAMPLE_MAX_TAPS:
        raise ValueError("lowpass_taps: %d taps: at most 2**22 = %d keep the sum exact" % (m, N.PCM_RESAMPLE_MAX_TAPS))
    k = np.arange(m, dtype=np.float64)
    return np.rint(2.0 ** 14 * (int(up) / q) * np.sinc((k - (m - 1) / 2) / q) * np.kaiser(m, float(beta))).astype(np.int16)


def _resample_fir_call(who: str, sample: Sample, samplerate, taps, factor, delay, start_frame, nframes):
    """what a conversion refuses, before any call into the library: ``(up, down, taps, factor, delay, start_frame, nframes)`` of the checked
    call, ``taps`` a 16-bit mono ``Sample``"""
    if isinstance(samplerate, bool) or not isinstance(samplerate, (int, np.integer)) or samplerate < 1:
        raise ValueError("%s: samplerate is a positive int, not %r" % (who, samplerate))
    if sample.nchannels not in (1, 2):
        raise ValueError("%s: mono and stereo only, not %d channels" % (who, sample.nchannels))
    if sample.samplewidth in (3, 4):
        raise NotImplementedError("%s: %d-byte samples are not built: the exact sum needs more than a float64 there (make_16bit() first)"
                                  % (who, sample.samplewidth))
    if sample.samplewidth not in (1, 2):
        raise ValueError("%s: samples of 1 or 2 bytes, not %d" % (who, sample.samplewidth))
    g = math.gcd(int(samplerate), sample.samplerate)
    up, down = int(samplerate) // g, sample.samplerate // g
    if up > N.PCM_RESAMPLE_MAX_UP:
        raise ValueError("%s: %d Hz to %d Hz is %d/%d: up is at most %d (convert in two steps)" % (who, sample.samplerate, samplerate, up, down, N.PCM_RESAMPLE_MAX_UP))
    if not N.pcm_resample_stride_fits(up, down):
        raise ValueError("%s: %d Hz to %d Hz is %d/%d: a stride of %d frames is too long for one step (convert in two steps)"
                         % (who, sample.samplerate, samplerate, up, down, N.pcm_resample_copies(up) * down))
    if taps is None:
        taps = lowpass_taps(up, down)
    if isinstance(taps, np.ndarray):
        if taps.dtype != np.int16 or taps.ndim != 1:
            raise ValueError("%s: taps are a one-dimensional int16 array, not %s of %d dimensions" % (who, taps.dtype, taps.ndim))
        taps = Sample.from_raw_frames(np.ascontiguousarray(taps).tobytes(), 2, int(samplerate), 1)
    elif not isinstance(taps, Sample):
        raise ValueError("%s: taps are None, a numpy int16 array or a 16-bit mono Sample, not %r" % (who, type(taps).__name__))
    elif taps.samplewidth != 2 or taps.nchannels != 1:
        raise ValueError("%s: taps are a 16-bit mono Sample, not %d bytes and %d channels (a stereo bank is not built)" % (who, taps.samplewidth, taps.nchannels))
    m = len(taps)
    if m == 0:
        raise ValueError("%s: no taps" % who)
    if m > N.PCM_RESAMPLE_MAX_TAPS:
        raise ValueError("%s: %d taps: at most 2**22 = %d keep the sum exact" % (who, m, N.PCM_RESAMPLE_MAX_TAPS))
    factor = 2.0 ** -14 if factor is None else float(factor)
    if not math.isfinite(factor):
        raise ValueError("%s: the factor %r is not finite" % (who, factor))
    if delay is None:
        delay = (m - 1) // 2
    if isinstance(delay, bool) or not isinstance(delay, (int, np.integer)) or not 0 <= delay < m:
        raise ValueError("%s: delay is an int in [0, %d), not %r" % (who, m, delay))
    total = -(-len(sample) * up // down)
    if isinstance(start_frame, bool) or not isinstance(start_frame, (int, np.integer)) or start_frame < 0:
        raise ValueError("%s: start_frame is a non-negative int, not %r" % (who, start_frame))
    if nframes is None:
        nframes = max(total - start_frame, 0)
    if isinstance(nframes, bool) or not isinstance(nframes, (int, np.integer)) or nframes < 0:
        raise ValueError("%s: nframes is a non-negative int or None, not %r" % (who, nframes))
    if start_frame + nframes > total:
        raise ValueError("%s: frames [%d, %d) reach past the result's %d" % (who, start_frame, start_frame + nframes, total))
    return up, down, taps, factor, int(delay), int(start_frame), int(nframes)


def resample_fir_into(buf: N.DeviceBuffer, byte_offset: int, sample: Sample, samplerate: int, taps=None, factor: Optional[float] = None,
                      delay: Optional[int] = None, start_frame: int = 0, nframes: Optional[int] = None) -> int:
    """Frames ``[start_frame, start_frame + nframes)`` of ``resample_fir(sample, samplerate, taps, factor, delay)`` into the caller's device
    buffer from byte ``byte_offset`` on (``nframes`` None: to the result's end); returns the frames written.  Asynchronous; the buffer may
    not overlap ``sample``'s or the taps'."""
    up, down, taps, factor, delay, start_frame, nframes = _resample_fir_call("resample_fir_into", sample, samplerate, taps, factor, delay, start_frame, nframes)
    if nframes:
        N.check(N.lib().sh_pcm_resample_fir(sample._device().handle, 0, len(sample), sample.nchannels, sample.samplewidth, taps._device().handle, 0, len(taps),
                                            up, down, delay, factor, start_frame, nframes, buf.handle, byte_offset))
    return nframes


def resample_fir(sample: Sample, samplerate: int, taps=None, factor: Optional[float] = None, delay: Optional[int] = None, start_frame: int = 0,
                 nframes: Optional[int] = None) -> Sample:
    """``sample`` converted to ``samplerate`` by a band-limited, rational resampler, as a new ``Sample``, computed in HBM and EXACT: with
    ``up / down`` the two rates over their gcd, per channel frame ``j`` is ``fbound(factor * sum of taps[k] * u[j * down + delay - k])``, ``u``
    being the sample with ``up - 1`` zeros behind every frame -- the sum the exact integer, ``fbound`` ``audioop.mul``'s last step -- so the
    bytes are those of ``numpy.convolve`` on int64 over the stuffed signal, every ``down``-th frame of it, and that one rounding.  The whole
    result has ``ceil(len(sample) * up / down)`` frames; ``start_frame`` and ``nframes`` choose a window, whose bytes are that slice of the whole
    result's.  ``taps`` None: ``lowpass_taps(up, down)``; otherwise a numpy int16 array or a 16-bit mono ``Sample`` of up to 2**22 taps, one
    bank for every channel.  ``factor`` None: ``2**-14``, the default bank's unity; ``delay`` None: ``(len(taps) - 1) // 2``, a symmetric
    bank's centre.  Widths 1 and 2; ``up`` at most 4096.  The input is read only: a locked one is fine.  (``Sample.resample`` and ``speed``
    remain ``audioop.ratecv``'s linear interpolation, byte for byte.)"""
    up, down, taps, factor, delay, start_frame, nframes = _resample_fir_call("resample_fir", sample, samplerate, taps, factor, delay, start_frame, nframes)
    out = Sample(name=sample.name, samplerate=int(samplerate), nchannels=sample.nchannels, samplewidth=sample.samplewidth)
    if nframes:
        nbytes = nframes * sample.nchannels * sample.samplewidth
        buf = N.DeviceBuffer(nbytes)
        resample_fir_into(buf, 0, sample, samplerate, taps, factor, delay, start_frame, nframes)
        out._set_device(buf, nbytes)
    return out


class SongStems:
    """The stems of a window of a song of tracks, made by ``CompiledSequence.stems``: every bus of the desk as a ``Sample`` of the window's
    length, all from one launch into one device buffer.  ``tracks[t]``: track ``t`` as its bus takes it -- behind its gain, its fader moves
    and its pan or pan ride; ``groups[g]``: group ``g``'s bus as the master takes it -- behind its gain, its ride and its pan or pan ride;
    ``master``: the bytes ``render`` returns for the same arguments.  Each is exactly the samples over which ``meters=True`` of the same call
    reads its row; a muted or skipped track or group is silence.  Every ``Sample`` is a view of the one buffer and keeps it alive on its
    own, so it outlives this object.  ``level_history(block_frames)``: the levels of every stem per block of the song's frame grid, a
    ``SongHistory`` with the rows and the meaning of ``render(meters="history")`` -- one launch over all planes where the object knows
    its buffer (``buffer``, ``plane_frames``: the one device buffer and the planes' stride in frames; ``tile_frames``: the song's tile
    in frames, the default block -- ``CompiledSequence.stems`` hands them on), one launch per row where it was built by hand.
    ``waveform(block_frames)``: the smallest and the largest sample of every stem per block of the same grid, a ``Waveform``, by the
    same route."""

    def __init__(self, tracks: Sequence[Sample], master: Sample, groups: Sequence[Sample], start_frame: int, frames: int, *,
                 buffer: Optional[N.DeviceBuffer] = None, plane_frames: Optional[int] = None, tile_frames: Optional[int] = None) -> None:
        self.tracks = list(tracks)
        self.master = master
        self.groups = list(groups)
        self.start_frame = int(start_frame)
        self.frames = int(frames)
        if (buffer is None) != (plane_frames is None):
            raise ValueError("SongStems: buffer and plane_frames come together")
        self._buffer = buffer
        self._plane_frames = None if plane_frames is None else int(plane_frames)
        self._tile_frames = None if tile_frames is None else int(tile_frames)

    def level_history(self, block_frames: Optional[int] = None) -> SongHistory:
        """The levels of every stem OVER TIME: a ``SongHistory`` whose rows are the tracks, the master and the groups, block ``i`` covering
        song frames ``[i * block_frames, (i + 1) * block_frames)`` cut to the window (``block_frames`` None: the song's tile, the block
        of ``render(meters="history")``).  Exact integers read off the stems' own samples (sh_pcm_level_blocks)."""
        blocks, nrows, block_frames = self._per_block(N.pcm_level_blocks, block_frames, "a level history")
        master = self.master
        return SongHistory.of_blocks(blocks, nrows, block_frames, self.start_frame, self.frames, master.samplewidth, master.nchannels, master.samplerate,
                                     len(self.groups))

    def waveform(self, block_frames: Optional[int] = None) -> Waveform:
        """The waveform extremes of every stem OVER TIME, for drawing: a ``Waveform`` whose rows are the tracks, the master and the groups,
        on ``level_history``'s grid and with its default block -- per block, row and channel the smallest and the largest sample, read
        off the stems' own samples (sh_pcm_extent_blocks): one launch over all planes where the object knows its buffer, one per row
        where it was built by hand."""
        blocks, nrows, block_frames = self._per_block(N.pcm_extent_blocks, block_frames, "a waveform")
        master = self.master
        return Waveform.of_blocks(blocks, nrows, block_frames, self.start_frame, self.frames, master.samplewidth, master.nchannels, master.samplerate,
                                  len(self.groups))

    def _per_block(self, table, block_frames: Optional[int], what: str) -> tuple:
        """the checked call behind ``level_history`` and ``waveform``: ``table`` -- ``N.pcm_level_blocks`` or ``N.pcm_extent_blocks`` -- over
        all planes of the one buffer, or row by row; (its array ``(nblocks, nrows)`` or None for an empty window, nrows, the block)"""
        master = self.master
        nch, width = master.nchannels, master.samplewidth
        if block_frames is None:
            block_frames = self._tile_frames if self._tile_frames is not None else max(1, N.SEQ_TILE_SAMPLES[width] // nch)
        block_frames = _block_frames("SongStems", block_frames)
        _levels_format("SongStems", master, what)
        rows = self.rows()
        if any((s.nchannels, s.samplewidth, len(s)) != (nch, width, self.frames) for s in rows):
            raise ValueError("SongStems: every stem has the master's format and the window's %d frames" % self.frames)
        blocks = None
        if self.frames:
            if self._buffer is not None:
                blocks = table(self._buffer, 0, self.frames, nch, width, self._plane_frames * nch, len(rows), self.start_frame, block_frames)
            else:
                blocks = np.concatenate([table(s._device(), 0, self.frames, nch, width, self.frames * nch, 1, self.start_frame, block_frames)
                                         for s in rows], axis=1)
        return blocks, len(rows), block_frames

    def rows(self) -> list:
        """all of them in plane order, which is the meter rows': the tracks, the master, the groups"""
        return self.tracks + [self.master] + self.groups

    def __len__(self) -> int:
        return len(self.tracks) + 1 + len(self.groups)

    def __repr__(self) -> str:
        return "SongStems(%d tracks, the master, %d groups, frames [%d, %d))" % (len(self.tracks), len(self.groups), self.start_frame,
                                                                                  self.start_frame + self.frames)


class Automation:
    """The fader moves of a song of tracks, made by ``CompiledSequence.automation(lanes)`` and given to that song's ``render``,
    ``render_into`` and ``chunks`` as ``automation=``: per track a list of pieces ``(start_frame, end_frame, from_volume, to_volume)``,
    packed as segments in song samples and uploaded ONCE into a small device table that this object owns.  ``pieces`` has the checked
    lanes (a tuple of tuples per track, pieces at exactly (1.0, 1.0) dropped), ``segments`` and ``seg_first`` the packed table.
    ``master`` and ``groups`` hold the checked lanes of the BUSES (``automation(lanes, master=, groups=)``): the master's pieces and a
    tuple per group lane; ``rides`` is one past the last group lane that kept a piece, 0 where none did -- a render with this object
    names at least that many groups.
    ``pans`` and ``group_pans`` hold the checked PAN lanes (``automation(lanes, pans=, group_pans=)``): a tuple of pieces ``(start_frame,
    end_frame, from_pan, to_pan)`` per track and per group lane, none dropped; ``pan_segments`` and ``pan_first`` their packed table
    (None where no pan lane holds a piece: the object is then the one there was); ``pan_rides`` is one past the last group pan lane
    that holds a piece -- a render names at least that many groups as well.
    ``close()`` (or the ``with`` block, or the last reference) frees the table."""

    def __init__(self, song: "CompiledSequence", pieces: tuple, segments: np.ndarray, seg_first: list, master: tuple = (),
                 groups: tuple = (), pans: tuple = (), group_pans: tuple = (), pan_segments: Optional[np.ndarray] = None,
                 pan_first: Optional[list] = None) -> None:
        self._auto = None
        self._song = song
        self.pieces, self.segments, self.seg_first = pieces, segments, seg_first
        self.master, self.groups = master, groups
        self.pans, self.group_pans, self.pan_segments, self.pan_first = pans, group_pans, pan_segments, pan_first
        self.rides = max([g + 1 for g, lane in enumerate(groups) if lane] + [0])      # one past the last group that has a piece
        self.pan_rides = max([g + 1 for g, lane in enumerate(group_pans) if lane] + [0])
        if pan_segments is not None:                            # pan lanes: the entry point that takes them, the buses' lanes in front
            self._auto = N.SeqAutomation(song._handle(), segments, seg_first, len(seg_first) - 2 - len(pieces), pan_segments, pan_first)
        elif master or self.rides:                              # the lanes of the buses behind the tracks': the entry point that takes them
            self._auto = N.SeqAutomation(song._handle(), segments, seg_first, len(groups))
        else:
            self._auto = N.SeqAutomation(song._handle(), segments, seg_first)

    @property
    def rides_buses(self) -> bool:
        """whether a piece rides a bus or a pan: the master's fader, a group's, a track's pan or a group's"""
        return bool(self.master or self.rides or self.pan_segments is not None)

    def _handle(self) -> "N.SeqAutomation":
        if self._auto is None:
            raise ValueError("Automation: closed")
        return self._auto

    def close(self) -> None:
        if self._auto is not None:
            self._auto.free()
            self._auto = None

    def __enter__(self) -> "Automation":
        return self

    def __exit__(self, *_exc) -> None:
        self.close()

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:
            pass


class _LaneKind(NamedTuple):
    """what a lane of an ``Automation`` rides: the word in its pieces' names and messages, the low end of its range (the high end is
    1.0), and whether a piece at exactly (1.0, 1.0) is dropped"""
    name: str
    low: float
    drops_unity: bool


_FADER_LANE = _LaneKind("volume", 0.0, True)        # a hold at 1.0 is no step
_PAN_LANE = _LaneKind("pan", -1.0, False)           # every piece kept: a hold at any pan stands in place of the static one


def _pan_factors(pan, who: str, index: int, strings: bool = True) -> Tuple[float, float]:
    """one pan entry of a desk that is not None (None is (1.0, 1.0), at the caller) -- a number -1 .. 1 or a pair of factors -- as
    ``(left_factor, right_factor)``; ``who % index`` opens the messages (``pan 2``, ``group 1: pan``), and where ``strings`` is False a ``str`` is no number"""
    if isinstance(pan, (tuple, list)):
        try:
            factors = (float(pan[0]), float(pan[1])) if len(pan) == 2 else None
        except (TypeError, ValueError):
            factors = None
        if factors is None or not (math.isfinite(factors[0]) and math.isfinite(factors[1])):
            raise ValueError("CompiledSequence: " + who % index + " is not a pair (left_factor, right_factor) of finite numbers")
        return factors
    try:
        if not strings and isinstance(pan, (str, bytes)):
            raise TypeError
        pan = float(pan)
    except (TypeError, ValueError):
        raise ValueError("CompiledSequence: " + who % index + " is None, a number or a pair (left_factor, right_factor)") from None
    if not -1.0 <= pan <= 1.0:
        raise ValueError("CompiledSequence: " + who % index + " must be between -1 and 1")
    return (1.0 - pan) / 2.0, (1.0 + pan) / 2.0             # Sample.pan: Python floats, on the host


class _DeskCall(NamedTuple):
    """The desk of one call of a compiled song, checked (``CompiledSequence._desk_call``): ``gains`` None or a list of floats, ``meters``
    False, True or "history", ``pans`` None or the flat factors, ``master`` None or a float, ``automation`` None or the ``Automation``,
    ``groups`` None or the table's rows, ``clips`` a bool, ``ngroups`` the number of groups -- None wherever the desk has no such step."""
    gains: Optional[list]
    meters: Union[bool, str]
    pans: Optional[list]
    master: Optional[float]
    automation: Optional[Automation]
    groups: Optional[list]
    clips: bool
    ngroups: int

    def render_keywords(self) -> dict:
        """The keywords ``N.Sequence.render`` is handed, which pick its entry point: none at all for a plain render; ``gains`` (and
        ``meters`` where asked for) alone where the desk has no step; else ``pans`` and ``master`` with them, ``groups`` and ``automation``
        only where there are some; ``clips`` only where asked for."""
        gains, meters, pans, master, automation, groups, clips, _ = self
        if pans is None and master is None and automation is None and groups is None:
            if gains is None and not meters:
                return {}                                       # a plain render: the entry point there was before there were tracks
            keywords = {"gains": gains}
        else:
            keywords = {"gains": gains, "pans": pans, "master": master}
            if groups is not None:
                keywords["groups"] = groups
            if automation is not None:
                keywords["automation"] = automation._handle()
        if meters:
            keywords["meters"] = meters
        if clips:
            keywords["clips"] = True
        return keywords

    def stems_keywords(self) -> dict:
        """the keywords ``N.Sequence.stems`` is handed: always all five"""
        return {"gains": self.gains, "pans": self.pans, "master": self.master, "groups": self.groups,
                "automation": None if self.automation is None else self.automation._handle()}


class CompiledSequence:
    """A list of placed samples compiled once and rendered as often, and in whatever windows, as a player asks: ``render`` of frames
    ``[a, b)`` holds, byte for byte, frames ``[a, b)`` of ``sequence(events, ...)``, in one launch that copies no table.  Made by
    ``compile_sequence``.  The song sounds as its samples did WHEN IT WAS COMPILED: they are taken with ``Sample._share_device()``
    (as ``RealTimeMixer.add_sample`` takes them), so a sample that is amplified or mixed into afterwards writes a buffer of its own, and
    this object holds the buffers it reads.  ``close()`` (or the ``with`` block, or the last reference) frees the device tables.
    A song of TRACKS (``compile_tracks``; ``ntracks`` is their number, None for ``compile_sequence``'s songs) is, byte for byte, ::

        master = Sample(...)                                # empty, the song's format
        for t, events in enumerate(tracks):
            sub = sequence(events, ...)                     # list order, saturating at every event
            if gains[t] != 1.0:
                sub.amplify(gains[t])                       # audioop.mul: clamp, then floor
            master.mix(sub)                                 # audioop.add, saturating; the shorter one padded with silence

    -- which is NOT the flat list: a track saturates on its own before its gain applies, and the master at every track -- with
    ``gains`` given when a window is RENDERED: ``render``, ``render_into`` and ``chunks`` take ``gains=`` (one finite float per
    track; None: all 1.0) and ``stem`` renders one track alone.  Mute, solo and fader moves compile nothing, upload nothing and
    materialise no track: still one launch per window.
    The desk's PAN POTS and MASTER FADER, of a stereo song of tracks: the same calls take ``pans=`` (one entry per track: None, a number
    -1 .. 1 -- ``Sample.pan``'s factors ``((1 - p) / 2, (1 + p) / 2)``, centre halves both sides -- or a pair ``(left_factor,
    right_factor)`` of finite floats) and ``master=`` (one finite float), and the chain is, byte for byte, ::

        master = Sample(...)
        for t, events in enumerate(tracks):
            sub = sequence(events, ...)
            if gains[t] != 1.0:
                sub.amplify(gains[t])                       # audioop.mul: clamp, then floor
            if pans[t] is not None:
                sub.stereo(lf_t, rf_t)                      # a stereo sample's balance: (fbound(L * lf), fbound(R * rf))
            master.mix(sub)                                 # audioop.add, saturating
        if master_gain != 1.0:
            master.amplify(master_gain)                     # once, behind the last track

    -- two roundings per track, the gain first (not one product ``g * lf``, not the pan first), and the master's gain on the
    saturated master, not on each track.  A factor of exactly 1.0 takes no multiply: ``None`` and ``(1.0, 1.0)`` give the same bytes.
    Still one launch per window, nothing uploaded; ``stem`` stays at gain 1.0 without pan or master.
    The desk's METERS: ``render``, ``render_into`` and ``chunks`` take ``meters=True`` and give, from that same launch, a
    ``SongLevels`` -- the levels of every track post-fader and of the master in the window just rendered, exact in integers -- beside
    the same bytes; with ``pans`` a track's levels are post-fader and post-pan, with ``master`` the master's are over the bytes
    returned.  A handle serves one metered render at a time.  Not built: pre-fader meters (they would read a muted track's
    events), meters of a song without tracks.
    The desk's LEVEL HISTORY: ``meters="history"`` gives, still from that one launch, a ``SongHistory`` instead -- the same levels per
    BLOCK of the window, a block being one tile of the SONG's grid (1024 frames of a 16-bit stereo song, 62 to 125 ms at the tests'
    rate, 10 to 21 ms at 48 kHz) cut to the window: ``history[j]`` is the ``SongLevels`` that ``meters=True`` gives for block ``j``'s
    own frames, ``total()`` the one it gives for the window, ``fold(n)`` coarser blocks, ``peaks()`` an array to draw.  Blocks are
    anchored to the song, so a block that lies whole inside two windows reads the same from both.  With gains, pans, master, groups
    and the tracks' fader moves.  Not built (``NotImplementedError``): a history with an ``Automation`` that rides a bus or a pan; a
    history without rendering the bytes.  The route for a desk that RIDES, and for blocks of any size: ``level_history(...)`` --
    ``stems(...)`` of the same desk, every one the song can make, and then ``SongStems.level_history``, the levels per block read off
    the stems' own samples: two launches, the same rows in the same order (tracks, master, groups), ``total()`` what ``meters=True``
    gives.
    The desk's OVERS: with ``meters="history"`` the same calls take ``clips=True``, and the ``SongHistory`` then says, still from that one
    launch, which bus clipped and where: ``clipped()`` per block, row (tracks, master, groups) and channel, ``Levels.clipped`` in every
    block's levels, ``total()`` and ``fold(n)`` adding the counts.  ``clipped`` is the number of samples of that channel in the block at
    which AT LEAST ONE of the row's OWN steps was clamped -- a step is clamped where the value it would have produced without the clamp
    lies outside the width's range ``[LO, HI]`` --, a sample counting ONCE per row however many steps clamped at it.  A track's steps:
    every saturating add of an event's samples into its sub-mix (``mix_at``'s ``audioop.add``), its ``amplify(gain)``, its static pan
    factors.  A group's: every saturating add of a track into its bus, its ``amplify(gain)``, its pan factors.  The master's: every
    saturating add of a track or a group into it, its ``amplify(master_gain)``.  An add clamps where the exact integer sum of the
    saturated accumulator and the addend is ``> HI`` or ``< LO``; a multiply by a factor ``f != 1.0`` clamps where ``floor(p) > HI`` or
    ``floor(p) < LO``, ``p`` being the float64 product ``audioop.mul`` forms (a product in ``(HI, HI + 1)`` floors to ``HI`` and is no
    over).  A row counts its own stage only: a track that clipped does not make its group or the master count.  Not counted: what an
    event does to its own samples before the add (its volume, pan, channel factors, envelope -- the sample as placed) and the tracks'
    fader moves, which cannot leave the range.  A muted or skipped track or group and an idle tile count 0; a mono song fills channel
    0.  The bytes, the peaks and the sums are those of the call without ``clips``.  ``clips=True`` without ``meters="history"`` is a
    ``ValueError``.  Not built (``NotImplementedError``): overs of an event's own chain, overs with bus or pan rides.
    The desk's STEMS: ``stems(start_frame, nframes, gains=, pans=, master=, automation=, groups=)`` hands over the SAMPLES those rows are
    read over -- a ``SongStems`` of one ``Sample`` per track (as its bus takes it: behind its gain, its fader moves and its pan or pan
    ride), one per group (its bus as the master takes it: saturated at every track, behind its gain, its ride and its pan or pan ride) and
    the master (``render``'s bytes) -- from ONE launch that walks every event once, into one device buffer the ``Sample``s are views of;
    ``stems_into`` writes the planes into a caller's buffer.  Plane ``r`` holds exactly what ``meters=True`` of the same call reads row
    ``r`` over; a muted or skipped track or group is silence; every byte of every plane is written and none beside them.  With every desk
    the song can make: gains, pans, master, groups, fader moves, bus rides, pan rides; widths 1 to 4 (no automation at width 3), mono
    and stereo.  ``stem(t)`` is something else: the raw track at gain 1.0, no desk.  Not built: stems together with meters, a history or
    overs in the same launch; ``chunks`` of stems; pre-fader stems; the raw group bus in front of its gain.
    The desk's FADER AUTOMATION: ``automation(lanes)`` takes, per track, None or a list of pieces ``(start_frame, end_frame, from_volume,
    to_volume)`` in SONG frames -- ascending, not overlapping, volumes finite and within 0.0 .. 1.0 (a static gain above 1 stays with
    ``gains``) -- and uploads them once; ``render``, ``render_into`` and ``chunks`` take the ``Automation`` it returns as
    ``automation=``, and the chain is, byte for byte, ::

        master = Sample(...)
        for t, events in enumerate(tracks):
            sub = sequence(events, ...)
            if gains[t] != 1.0:
                sub.amplify(gains[t])
            for (a, b, v0, v1) in pieces[t]:                # the fader moves: behind the gain, in front of the pan
                n = (b - a) * nchannels                     # numsamples, a float
                for k in range(n):                          # k counts SAMPLES from the piece's first, interleaved
                    x = sub[a * nchannels + k]
                    sub[a * nchannels + k] = int(x * (k * (v1 - v0) / n + v0))    # a Python float product, truncated toward zero
            if pans[t] is not None:
                sub.stereo(lf_t, rf_t)
            master.mix(sub)
        if master_gain != 1.0:
            master.amplify(master_gain)

    -- ``Sample.fadein``'s expression: a piece with ``to_volume == 1.0`` is ``Sample.fadein(seconds, from_volume)`` of that clip of the
    track and one with ``from_volume == 1.0`` is ``Sample.fadeout(seconds, to_volume)``, byte for byte.  A HOLD (``from_volume ==
    to_volume``) is ``int(x * v)``, the fade's truncation toward zero, NOT ``audioop.mul``'s floor: it differs from a gain of ``v`` on
    negative samples.  Outside its pieces a track is untouched, and pieces at exactly (1.0, 1.0) are dropped.  A window's bytes are
    that slice of the whole song's whatever the window: positions count from the piece's first sample in the song.  Post-fader meters read
    a track behind its moves, as the master takes it; a muted track is still skipped; ``stem`` stays plain.  Still one launch per window
    and nothing uploaded by a render.  Width 3 has no automation (``NotImplementedError``: upstream's fades have no 24-bit form, as for
    envelopes).
    The desk's GROUP BUSES: ``groups=`` of ``render``, ``render_into`` and ``chunks`` is a list of at most 8 entries ``(first_track,
    end_track, gain)`` or ``(first_track, end_track, gain, pan)`` -- runs of consecutive tracks ``[first_track, end_track)``, ascending
    and not overlapping; ``gain`` a finite number or None for 1.0; ``pan`` what one entry of ``pans`` may be, on stereo songs only.  A
    track outside every entry goes straight to the master.  The chain is, byte for byte, ::

        master = Sample(...)
        for t, events in enumerate(tracks):
            sub = sequence(events, ...)                     # then its gain, its fader moves and its pan, as above
            if t lies in group g:
                if t == first_g:
                    bus = Sample(...)
                bus.mix(sub)                                # the group saturates ON ITS OWN, at every track
                if t == end_g - 1:
                    if gain_g != 1.0:
                        bus.amplify(gain_g)                 # audioop.mul: ONE rounding over the saturated sum
                    if pan_g is not None:
                        bus.stereo(lf_g, rf_g)
                    master.mix(bus)                         # the group enters the master where its LAST track stands
            else:
                master.mix(sub)
        if master_gain != 1.0:
            master.amplify(master_gain)

    -- not a gain on each track (``floor(g * (a + b)) != floor(g * a) + floor(g * b)``) and not the flat list (the group clips before
    the master sees it).  A group whose gain is exactly 0.0, or whose pan factors are both exactly 0.0, skips its tracks' events as a
    muted track does; its levels and its tracks' read zero.  With ``meters=True`` ``SongLevels.groups`` holds one ``Levels`` per group,
    over the bus as the master takes it, behind its gain and pan; a track's levels stay what its bus takes of it.  A group's bus alone
    is already ``render(gains=<solo of its tracks>)``.  Still one launch per window and nothing uploaded by a render; ``groups=None``
    or an empty list is the render without groups.
    The desk's BUS RIDES: ``automation(lanes, master=, groups=)`` takes a lane for the master and one per group as well -- ``master`` None
    or a list of pieces, ``groups`` None or at most 8 entries, each None or a list of pieces, entry ``g`` riding the bus of entry ``g`` of
    whatever ``groups=`` a render names -- checked as a track's lane is and uploaded in the same table.  With ``ride(x, pieces)`` the
    fader moves' expression above, the chain is, byte for byte, ::

        master = Sample(...)
        for t, events in enumerate(tracks):
            sub = sequence(events, ...)                     # then its gain, its fader moves and its pan, as above
            if t lies in group g:
                if t == first_g:
                    bus = Sample(...)
                bus.mix(sub)
                if t == end_g - 1:
                    if gain_g != 1.0:
                        bus.amplify(gain_g)                 # audioop.mul over the saturated sum
                    ride(bus, group_lanes[g])               # the group's ride: behind its gain, in front of its pan
                    if pan_g is not None:
                        bus.stereo(lf_g, rf_g)
                    master.mix(bus)
            else:
                master.mix(sub)
        if master_gain != 1.0:
            master.amplify(master_gain)
        ride(master, master_lane)                           # the master's ride: behind its gain, on the saturated master

    -- a fade of the drum bus is not a fade of each drum (the group saturates on its own, and ``int((a + b) * f)`` is not ``int(a * f) +
    int(b * f)``), and a master piece ending at 1.0 is ``Sample.fadein(seconds, from_volume)`` of that clip of the MIX, one starting at
    1.0 ``Sample.fadeout(seconds, to_volume)``: the fade-out of a whole song.  Positions are song frames, so a window, a chunk or a
    ``render_into`` at an odd sample offset holds that slice of the whole song's bytes.  With ``meters=True`` a group's levels are read
    behind its ride and pan, the master's over the bytes returned.  A group at gain 0.0 or pan (0.0, 0.0) still skips its tracks' events.
    An ``Automation`` that rides group ``g`` needs a render whose ``groups=`` has more than ``g`` entries (``ValueError`` before anything
    is launched); a master ride alone needs no ``groups=``.  One without a piece on a bus lane is the ``Automation`` there was.  Still one
    launch per window and nothing uploaded by a render.
    The desk's PAN RIDES, of a stereo song: ``automation(lanes, pans=, group_pans=)`` takes pan lanes as well -- ``pans`` None or one
    entry per track, ``group_pans`` None or at most 8 entries (entry ``g`` riding the pan of entry ``g`` of a render's ``groups=``), each
    None or a list of pieces ``(start_frame, end_frame, from_pan, to_pan)`` in SONG frames, ascending, not overlapping, pans finite and
    within -1.0 .. 1.0 -- uploaded once in the same table.  The chain is the one above with the two pan steps replaced where a piece
    covers a frame, byte for byte ::

        def pan_ride(x, pieces, lf, rf):                    # x: a track behind its gain and fader moves, a bus behind its gain and ride
            y = x.copy().stereo(lf, rf)                     # outside the pieces: the static pan, as ever
            for (a, b, p0, p1) in pieces:
                n = b - a                                   # FRAMES
                for k in range(n):                          # k counts FRAMES from the piece's first
                    p = k * (p1 - p0) / n + p0              # Python floats, in this order
                    L, R = x[a + k]
                    y[a + k] = (int(L * (1.0 - p) / 2.0), int(R * (1.0 + p) / 2.0))    # truncated toward zero
            return y

    -- a piece is ``Sample.pan(lfo=[k * (p1 - p0) / n + p0 for k in range(n)])`` of that clip.  The ride REPLACES the static pan inside
    its frames; it is not applied on top of it: the pot has one position.  No piece is dropped: a HOLD (``p0 == p1``) is
    ``int(x * (1 -+ p) / 2)``, truncated toward zero, NOT ``Sample.stereo``'s floor -- a hold at 0.0 differs from the static pan 0.0
    on every negative odd sample.  A track or group whose STATIC factors are both exactly 0.0, or whose gain is 0.0, is still skipped
    entirely, pieces or not.  With ``meters=True`` a track's levels are read behind its pan ride, a group's behind its ride and its
    pan ride, the master's over the bytes returned.  Positions are song frames: a window, a chunk or a ``render_into`` at an odd sample
    offset holds that slice of the whole song's bytes.  An ``Automation`` that rides the pan of group ``g`` needs a render whose
    ``groups=`` has more than ``g`` entries (``ValueError`` before anything is launched); one without a pan piece is the
    ``Automation`` there was.  Still one launch per window and nothing uploaded by a render.  Not built: groups inside groups, a
    ``stem`` of a group, automation at width 3."""

    MAX_TRACKS = 32

    def __init__(self, events: Optional[Sequence[tuple]], samplerate: int, nchannels: int, samplewidth: int = 2, name: str = "",
                 tracks: Optional[Sequence[Sequence[tuple]]] = None) -> None:
        self._seq = None
        self.name = name
        self.ntracks = None
        self.samplerate, self.nchannels, self.samplewidth = int(samplerate), int(nchannels), int(samplewidth)
        track = Sample(name=name, samplerate=samplerate, nchannels=nchannels, samplewidth=samplewidth)
        self._fb = self.samplewidth * self.nchannels
        if tracks is None:
            bufs, table, segtab, nbytes = track._compile_events(events)    # every ValueError of mix_at_many, before the device is reached
            self.frames = nbytes // self._fb
            self._nevents = len(table)
            self._seq = N.Sequence(bufs, table, segtab, self.samplewidth, self.nchannels, nbytes // self.samplewidth)
        else:
            bufs, table, segtab, nbytes, track_first = self._check_tracks(track, tracks)
            self.frames = nbytes // self._fb
            self._nevents = len(table)
            self._seq = N.Sequence(bufs, table, segtab, self.samplewidth, self.nchannels, nbytes // self.samplewidth, track_first=track_first)
            self.ntracks = len(track_first) - 1
        self.level = N.SEQ_LEVELS[self._seq.info()["level"]]

    @classmethod
    def _check_tracks(cls, track: Sample, tracks) -> tuple:
        """compile_tracks' checks, all of them before the device is reached: the number of tracks, then every track's list through
        mix_at_many's checks, an error naming the track and the event's index in its own list; then _compile_events' tables of the tracks'
        events one track behind the other, and where each track starts among them."""
        if isinstance(tracks, (str, bytes)) or not hasattr(tracks, "__len__"):
            raise ValueError("compile_tracks: tracks is a sequence of event lists")
        if len(tracks) == 0:
            raise ValueError("compile_tracks: a song needs at least one track")
        if len(tracks) > cls.MAX_TRACKS:
            raise ValueError("compile_tracks: %d tracks, at most %d" % (len(tracks), cls.MAX_TRACKS))
        track._check_gpu_width("mix_at")
        checked, track_first = [], [0]
        for t, events in enumerate(tracks):
            events = list(events)
            try:
                checked.extend(track._check_events(events))
            except (ValueError, NotImplementedError) as first:
                for k, ev in enumerate(events):             # which event: the checks take one event at a time
                    try:
                        track._check_events([ev])
                    except (ValueError, NotImplementedError) as e:
                        raise type(e)("compile_tracks: track %d, event %d: %s" % (t, k, e)) from None
                raise type(first)("compile_tracks: track %d: %s" % (t, first)) from None
            track_first.append(len(checked))
        return track._compile_checked(checked) + (track_first,)

    def _gains(self, gains) -> Optional[list]:
        """``gains`` as render hands them on: None, or ``ntracks`` finite floats -- checked before anything is launched"""
        if gains is None:
            return None
        if self.ntracks is None:
            raise ValueError("CompiledSequence: gains need a song of tracks (compile_tracks); this one has none")
        try:
            out = [float(g) for g in gains]
        except (TypeError, ValueError):
            raise ValueError("CompiledSequence: gains is a sequence of numbers, one per track") from None
        if len(out) != self.ntracks:
            raise ValueError("CompiledSequence: %d gains for %d tracks" % (len(out), self.ntracks))
        for t, g in enumerate(out):
            if not math.isfinite(g):
                raise ValueError("CompiledSequence: gain %d is not finite" % t)
        return out

    def _meters(self, meters) -> bool:
        """``meters`` as render hands it on -- checked before anything is launched"""
        if not isinstance(meters, bool) and not (isinstance(meters, str) and meters == "history"):
            raise ValueError("CompiledSequence: meters is True, False or \"history\", not %r" % (meters,))
        if meters and self.ntracks is None:
            raise ValueError("CompiledSequence: meters need a song of tracks (compile_tracks); this one has none")
        if meters == "history" and N.SEQ_TILE_SAMPLES[self.samplewidth] % self.nchannels:
            raise ValueError("CompiledSequence: a level history needs blocks of whole frames: %d channels do not divide a block of %d samples"
                             % (self.nchannels, N.SEQ_TILE_SAMPLES[self.samplewidth]))
        return meters

    @staticmethod
    def _no_history_of(meters, automation) -> None:
        """a level history with an ``Automation`` that rides a bus or a pan: not built in the riding kernels -- said before anything is
        launched.  The route for such a desk is ``level_history(...)``: its stems, and their levels per block (two launches)."""
        if meters == "history" and automation is not None and automation.rides_buses:
            raise NotImplementedError("CompiledSequence: rides of buses and pans have no level history yet (meters=\"history\" with an "
                                      "Automation that has master, group or pan pieces)")

    @staticmethod
    def _clips(clips, meters, automation) -> bool:
        """``clips`` as render hands it on: the overs are counted per block of a level history and, as the history, not through rides of
        buses and pans -- said before anything is launched"""
        if not clips:
            return False
        if meters != "history":
            raise ValueError("CompiledSequence: clips=True counts the overs per block of a level history: it needs meters=\"history\"")
        if automation is not None and automation.rides_buses:
            raise NotImplementedError("CompiledSequence: overs are not counted through rides of buses and pans yet (clips=True with an "
                                      "Automation that has master, group or pan pieces)")
        return True

    def _history(self, blocks, start_frame: int, nframes: int, ngroups: int, clips: bool = False) -> SongHistory:
        return SongHistory.of_blocks(blocks, self.ntracks + 1 + ngroups, N.SEQ_TILE_SAMPLES[self.samplewidth] // self.nchannels, start_frame, nframes,
                                     self.samplewidth, self.nchannels, self.samplerate, ngroups, clips=clips)

    def _pans(self, pans) -> Optional[list]:
        """``pans`` as render hands them on: None (no track has a pan step), or ``2 * ntracks`` finite floats, left then right per track,
        (1.0, 1.0) where the entry is None -- checked before anything is launched"""
        if pans is None:
            return None
        if self.ntracks is None:
            raise ValueError("CompiledSequence: pans need a song of tracks (compile_tracks); this one has none")
        if self.nchannels != 2:
            raise ValueError("CompiledSequence: pans need a stereo song, this one has %d channels" % self.nchannels)
        if isinstance(pans, (str, bytes)) or not hasattr(pans, "__len__"):
            raise ValueError("CompiledSequence: pans is a sequence, one entry per track")
        if len(pans) != self.ntracks:
            raise ValueError("CompiledSequence: %d pans for %d tracks" % (len(pans), self.ntracks))
        out = [f for t, pan in enumerate(pans) for f in ((1.0, 1.0) if pan is None else _pan_factors(pan, "pan %d", t))]
        return None if out.count(1.0) == len(out) else out        # (every factor == 1.0: no track has a pan step)

    def _master(self, master) -> Optional[float]:
        """``master`` as render hands it on: None (no step: None or exactly 1.0) or a finite float -- checked before anything is launched"""
        if master is None:
            return None
        if self.ntracks is None:
            raise ValueError("CompiledSequence: master needs a song of tracks (compile_tracks); this one has none")
        try:
            master = float(master)
        except (TypeError, ValueError):
            raise ValueError("CompiledSequence: master is a number") from None
        if not math.isfinite(master):
            raise ValueError("CompiledSequence: master is not finite")
        return None if master == 1.0 else master

    MAX_GROUPS = N.SEQ_MAX_GROUPS

    def _groups(self, groups) -> Optional[list]:
        """``groups`` as render hands them on: None (None or an empty list: no group bus), or a list of ``(first_track, end_track, gain,
        left_factor, right_factor)`` -- integers and finite floats, (1.0, 1.0) where the entry has no pan -- checked before anything is
        launched"""
        if groups is None:
            return None
        if self.ntracks is None:
            raise ValueError("CompiledSequence: groups need a song of tracks (compile_tracks); this one has none")
        if isinstance(groups, (str, bytes)) or not hasattr(groups, "__len__"):
            raise ValueError("CompiledSequence: groups is a sequence of (first_track, end_track, gain) or (first_track, end_track, gain, pan)")
        if len(groups) > self.MAX_GROUPS:
            raise ValueError("CompiledSequence: %d groups, at most %d" % (len(groups), self.MAX_GROUPS))
        out, prev, where = [], 0, "CompiledSequence: group %d: "
        for k, entry in enumerate(groups):
            if isinstance(entry, (str, bytes)) or not hasattr(entry, "__len__") or len(entry) not in (3, 4):
                raise ValueError(where % k + "an entry is (first_track, end_track, gain) or (first_track, end_track, gain, pan)")
            try:
                if isinstance(entry[0], bool) or isinstance(entry[1], bool):
                    raise TypeError
                first, end = operator.index(entry[0]), operator.index(entry[1])
            except TypeError:
                raise ValueError(where % k + "first_track and end_track are integers") from None
            if first < 0 or end > self.ntracks:
                raise ValueError(where % k + "tracks [%d, %d) outside the song's %d tracks" % (first, end, self.ntracks))
            if first >= end:
                raise ValueError(where % k + "tracks [%d, %d): an empty range" % (first, end))
            if first < prev:
                raise ValueError(where % k + "starts at track %d, before the group in front of it ends (%d)" % (first, prev))
            gain = 1.0 if entry[2] is None else entry[2]
            try:
                if isinstance(gain, (str, bytes)):
                    raise TypeError
                gain = float(gain)
            except (TypeError, ValueError):
                raise ValueError(where % k + "gain is None or a finite number") from None
            if not math.isfinite(gain):
                raise ValueError(where % k + "gain is not finite")
            pan = entry[3] if len(entry) == 4 else None
            if pan is None:
                factors = (1.0, 1.0)
            elif self.nchannels != 2:
                raise ValueError(where % k + "a pan needs a stereo song, this one has %d channels" % self.nchannels)
            else:
                factors = _pan_factors(pan, "group %d: pan", k, strings=False)
            prev = end
            out.append((first, end, gain, factors[0], factors[1]))
        return out or None

    def _automation(self, automation, groups=None) -> Optional[Automation]:
        """``automation`` as a call takes it: None, or an open ``Automation`` that THIS song made; one that rides group ``g`` needs a
        render that names more than ``g`` groups (``groups``: what ``_groups`` made of the render's) -- checked before anything is
        launched"""
        if automation is None:
            return None
        if not isinstance(automation, Automation) or automation._song is not self:
            raise ValueError("CompiledSequence: automation is None or an Automation made by this song's automation()")
        automation._handle()
        if automation.rides > len(groups or ()):
            raise ValueError("CompiledSequence: the automation rides group %d, and this render names %d groups" % (automation.rides - 1, len(groups or ())))
        if automation.pan_rides > len(groups or ()):
            raise ValueError("CompiledSequence: the automation rides the pan of group %d, and this render names %d groups"
                             % (automation.pan_rides - 1, len(groups or ())))
        return automation

    def _desk_call(self, gains, meters, pans, master, automation, groups, clips, *, stems: bool = False) -> _DeskCall:
        """Every check of a call's desk, once and in one order, whichever door the call came through -- before a buffer is made or
        anything is launched: the song is open, (``stems``) has tracks, then gains, meters, groups, pans, master, the automation against
        the checked groups, clips, and the history that rides do not have."""
        self._handle()
        if stems and self.ntracks is None:
            raise ValueError("CompiledSequence: stems need a song of tracks (compile_tracks); this one has none")
        gains = self._gains(gains)
        meters = self._meters(meters)
        groups = self._groups(groups)
        call = _DeskCall(gains, meters, self._pans(pans), self._master(master), self._automation(automation, groups), groups,
                         self._clips(clips, meters, automation), len(groups or ()))
        self._no_history_of(meters, automation)
        return call

    def automation(self, lanes, master=None, groups=None, pans=None, group_pans=None) -> Automation:
        """The fader moves of this song of tracks (``CompiledSequence`` has the chain): ``lanes`` has one entry per track, None or a list
        of pieces ``(start_frame, end_frame, from_volume, to_volume)`` -- song frames, ascending, not overlapping, ``start < end <=
        len(song)``, volumes finite and within 0.0 .. 1.0.  A hold (``from_volume == to_volume``) is ``int(x * v)``: the fade's truncation
        toward zero, not ``audioop.mul``'s floor.  ``master``: None or such a list for the master, behind its gain.  ``groups``: None or a
        sequence of at most 8 entries, each None or such a list; entry ``g`` rides the bus of entry ``g`` of whatever ``groups=`` a render
        names, behind the group's gain and in front of its pan.  Everything is checked before the device is reached, a ``ValueError``
        naming the track (``master``, ``group g``) and the piece; pieces at exactly (1.0, 1.0) are dropped; the rest are uploaded once into
        a table the returned ``Automation`` owns.  ``pans`` (None or one entry per track) and ``group_pans`` (None or at most 8 entries,
        entry ``g`` for the pan of group ``g``), of a stereo song: each entry None or a list of pieces ``(start_frame, end_frame,
        from_pan, to_pan)``, pans finite and within -1.0 .. 1.0 -- ``Sample.pan(lfo=...)`` of a linear sweep, in place of the static pan
        inside the piece; a ``ValueError`` names ``track t pan`` or ``group g pan`` and the piece, and no piece is dropped."""
        self._handle()
        pieces, master, groups = self._check_lanes(lanes, master, groups)
        pans, group_pans = self._check_pan_lanes(pans, group_pans)
        if not any(pans) and not any(group_pans):               # no pan piece: what was packed, and the entry points reached, before
            segments, seg_first = self._pack_lanes(pieces, self.nchannels, master, groups)
            return Automation(self, pieces, segments, seg_first, master, groups, pans, group_pans)
        ngroups = max(len(groups), len(group_pans))             # both sets of lanes for the same groups, the missing ones empty
        segments, seg_first = self._pack_lanes(pieces, self.nchannels, master, groups + ((),) * (ngroups - len(groups)), buses=True)
        pan_segments, pan_first = self._pack_pan_lanes(pans or ((),) * self.ntracks, group_pans + ((),) * (ngroups - len(group_pans)))
        return Automation(self, pieces, segments, seg_first, master, groups, pans, group_pans, pan_segments, pan_first)

    def _check_pan_lanes(self, pans, group_pans) -> tuple:
        """(the tracks' pan lanes, the groups' pan lanes), checked: ``()`` for None, else every lane through ``_check_lane``"""
        if pans is None and group_pans is None:
            return (), ()
        if self.nchannels != 2:
            raise ValueError("CompiledSequence: automation: pans need a stereo song, this one has %d channels" % self.nchannels)
        if pans is not None:
            if isinstance(pans, (str, bytes)) or not hasattr(pans, "__len__"):
                raise ValueError("CompiledSequence: automation: pans is None or a sequence, one entry per track")
            if len(pans) != self.ntracks:
                raise ValueError("CompiledSequence: automation: %d pan lanes for %d tracks" % (len(pans), self.ntracks))
        if group_pans is not None:
            if isinstance(group_pans, (str, bytes)) or not hasattr(group_pans, "__len__"):
                raise ValueError("CompiledSequence: automation: group_pans is None or a sequence, one entry per group")
            if len(group_pans) > self.MAX_GROUPS:
                raise ValueError("CompiledSequence: automation: %d group pan lanes, at most %d" % (len(group_pans), self.MAX_GROUPS))
        return (tuple(self._check_lane("track %d pan" % t, lane, _PAN_LANE) for t, lane in enumerate(pans or ())),
                tuple(self._check_lane("group %d pan" % g, lane, _PAN_LANE) for g, lane in enumerate(group_pans or ())))

    @staticmethod
    def _pack_pan_lanes(pans: tuple, group_pans: tuple) -> tuple:
        """the checked pan lanes as sh_env_segment rows in song SAMPLES of a stereo song, the tracks' one behind the other and then the
        groups', and where each lane's start: a piece over frames ``[a, b)`` is a pan move (kind ``ENV_PAN``, origin ``2 a``, end ``2 b``,
        numsamples ``b - a`` -- its FRAMES --, slope ``p1 - p0``, offset ``p0``, mul 1.0), a plain segment fills the gap in front of it"""
        rows, seg_first = CompiledSequence._lane_rows(tuple(pans) + tuple(group_pans), 2, 1, N.ENV_PAN)
        return CompiledSequence._segments(rows), seg_first

    def _check_lanes(self, lanes, master=None, groups=None) -> tuple:
        """(the tracks' lanes, the master's lane, the groups' lanes), checked: every lane through ``_check_lane``"""
        if self.ntracks is None:
            raise ValueError("CompiledSequence: automation needs a song of tracks (compile_tracks); this one has none")
        if self.samplewidth == 3:
            raise NotImplementedError("CompiledSequence: automation: width 3: a fade has no 24-bit form")
        if isinstance(lanes, (str, bytes)) or not hasattr(lanes, "__len__"):
            raise ValueError("CompiledSequence: automation: lanes is a sequence, one entry per track")
        if len(lanes) != self.ntracks:
            raise ValueError("CompiledSequence: automation: %d lanes for %d tracks" % (len(lanes), self.ntracks))
        if groups is not None:
            if isinstance(groups, (str, bytes)) or not hasattr(groups, "__len__"):
                raise ValueError("CompiledSequence: automation: groups is None or a sequence, one entry per group")
            if len(groups) > self.MAX_GROUPS:
                raise ValueError("CompiledSequence: automation: %d group lanes, at most %d" % (len(groups), self.MAX_GROUPS))
        return (tuple(self._check_lane("track %d" % t, lane) for t, lane in enumerate(lanes)), self._check_lane("master", master),
                tuple(self._check_lane("group %d" % g, lane) for g, lane in enumerate(groups or ())))

    def _check_lane(self, who: str, lane, what: _LaneKind = _FADER_LANE) -> tuple:
        """one lane -- a track's, the master's or a group's, of faders or (``what``) of pans -- as a tuple of pieces ``(start_frame,
        end_frame, from_volume, to_volume)`` or ``(start_frame, end_frame, from_pan, to_pan)``, integers and floats; a fader's pieces at
        exactly (1.0, 1.0) are dropped, every pan piece is kept (a hold at 0.0 is a step of its own); ``who`` names it in the errors"""
        if lane is None:
            return ()
        if isinstance(lane, (str, bytes)) or not hasattr(lane, "__iter__"):
            raise ValueError("CompiledSequence: automation: %s: a lane is None or a list of pieces" % who)
        form = "a piece is (start_frame, end_frame, from_%s, to_%s)" % (what.name, what.name)
        kept, prev = [], 0
        for k, piece in enumerate(lane):
            where = "CompiledSequence: automation: %s, piece %d: " % (who, k)
            if isinstance(piece, (str, bytes)) or not hasattr(piece, "__len__") or len(piece) != 4:
                raise ValueError(where + form)
            try:
                if isinstance(piece[0], bool) or isinstance(piece[1], bool):
                    raise TypeError
                a, b = operator.index(piece[0]), operator.index(piece[1])
            except TypeError:
                raise ValueError(where + "start_frame and end_frame are integers") from None
            try:
                v0, v1 = float(piece[2]), float(piece[3])
            except (TypeError, ValueError):
                raise ValueError(where + form + ", four numbers") from None
            if a < 0 or a >= b:
                raise ValueError(where + "frames [%d, %d): a piece starts at 0 or later and ends behind its start" % (a, b))
            if b > self.frames:
                raise ValueError(where + "frames [%d, %d) end past the song's %d frames" % (a, b, self.frames))
            if a < prev:
                raise ValueError(where + "starts at frame %d, before the piece in front of it ends (%d)" % (a, prev))
            for end, v in (("from", v0), ("to", v1)):
                if not math.isfinite(v) or not what.low <= v <= 1.0:
                    raise ValueError(where + "%s_%s %r is not a finite number within %r .. 1.0" % (end, what.name, v, what.low))
            prev = b
            if not (what.drops_unity and v0 == 1.0 and v1 == 1.0):
                kept.append((a, b, v0, v1))
        return tuple(kept)

    @staticmethod
    def _lane_rows(lanes, samples_per_frame: int, unit: int, kind: int) -> tuple:
        """checked lanes as sh_env_segment rows in song SAMPLES, one lane behind the other, and where each lane's start: a piece over
        frames ``[a, b)`` is a move of ``kind`` (origin its first sample, numsamples ``(b - a) * unit``, slope ``v1 - v0``, offset ``v0``,
        mul 1.0), a plain segment fills the gap in front of it"""
        rows, seg_first = [], [0]
        for lane in lanes:
            at = 0
            for a, b, v0, v1 in lane:
                if a * samples_per_frame > at:
                    rows.append((a * samples_per_frame, 0, 1.0, 0.0, 0.0, 0.0, N.ENV_NONE))
                rows.append((b * samples_per_frame, a * samples_per_frame, 1.0, v1 - v0, float((b - a) * unit), v0, kind))
                at = b * samples_per_frame
            seg_first.append(len(rows))
        return rows, seg_first

    @staticmethod
    def _segments(rows: list) -> np.ndarray:
        segments = np.zeros(len(rows), dtype=N.ENV_SEGMENT_DTYPE)
        for name, column in zip(("end", "origin", "mul", "slope", "numsamples", "offset", "kind"), zip(*rows) if rows else [()] * 7):
            segments[name] = column
        return segments

    @staticmethod
    def _pack_lanes(pieces: tuple, nchannels: int, master: tuple = (), groups: tuple = (), buses: bool = False) -> tuple:
        """the checked lanes as sh_env_segment rows in song SAMPLES, the tracks' one behind the other, and where each track's start: a
        piece is a fade-in segment (origin its first sample, numsamples its length, slope ``v1 - v0``, offset ``v0``, mul 1.0), a plain
        segment fills the gap in front of it.  Where a bus lane -- the master's or a group's -- holds a piece, the lanes of the buses
        follow the tracks' in the meter table's row order: the master's at ``ntracks``, group ``g``'s at ``ntracks + 1 + g``; where none
        does, the table is the tracks' alone -- unless ``buses`` asks for the lanes of the buses anyway (an ``Automation`` with pan
        lanes: its entry point takes them)"""
        if buses or master or any(groups):
            pieces = tuple(pieces) + (master,) + tuple(groups)
        rows, seg_first = CompiledSequence._lane_rows(pieces, nchannels, nchannels, N.ENV_FADE_IN)
        return CompiledSequence._segments(rows), seg_first

    def _levels(self, rows, nframes: int, ngroups: int = 0) -> SongLevels:
        if rows is None:                                        # an empty window: nothing was launched, every level 0
            rows = [((0, 0), (0, 0))] * (self.ntracks + 1 + ngroups)
        if ngroups:
            return SongLevels(rows, nframes, self.samplewidth, self.nchannels, self.samplerate, ngroups)
        return SongLevels(rows, nframes, self.samplewidth, self.nchannels, self.samplerate)

    @property
    def duration(self) -> float:
        return self.frames / self.samplerate

    def __len__(self) -> int:
        return self.frames

    def info(self) -> dict:
        """sh_seq_info: events, tiles, active tiles, (event, tile) pairs, device bytes, level"""
        return self._handle().info()

    def _handle(self) -> "N.Sequence":
        if self._seq is None:
            raise ValueError("CompiledSequence: closed")
        return self._seq

    def _range(self, start_frame: int, nframes: Optional[int]) -> Tuple[int, int]:
        start_frame = int(start_frame)
        if start_frame < 0 or start_frame > self.frames:
            raise ValueError("CompiledSequence: start_frame %d outside the song's %d frames" % (start_frame, self.frames))
        nframes = self.frames - start_frame if nframes is None else int(nframes)
        if nframes < 0 or nframes > self.frames - start_frame:
            raise ValueError("CompiledSequence: frames [%d, %d) outside the song's %d frames" % (start_frame, start_frame + nframes, self.frames))
        return start_frame, nframes

    def render_into(self, buf: N.DeviceBuffer, byte_offset: int, start_frame: int, nframes: int, gains: Optional[Sequence[float]] = None,
                    meters: bool = False, pans: Optional[Sequence] = None, master: Optional[float] = None,
                    automation: Optional[Automation] = None, groups: Optional[Sequence] = None, clips: bool = False) -> Union[None, SongLevels, SongHistory]:
        """Frames ``[start_frame, start_frame + nframes)`` of the song into ``buf`` from ``byte_offset`` (a whole number of samples) on:
        every byte of the range is written, whatever ``buf`` held.  ``gains``: one per track of a song of tracks.  ``meters=True``: the
        same bytes, and the window's ``SongLevels`` returned, from the same launch (the call then waits for it).  ``pans``, ``master``:
        a pan per track and the master's gain of a stereo song of tracks (``CompiledSequence``), in that same launch.  ``automation``:
        None or an ``Automation`` made by this song's ``automation()``: its fader moves, in that same launch.  ``groups``: None or the
        group buses (``CompiledSequence``), in that same launch; the levels then hold a ``Levels`` per group as well.
        ``meters="history"``: the same bytes, and the window's ``SongHistory`` returned -- its levels per block of the song's tile grid,
        still from that one launch.  ``clips=True`` (with ``meters="history"``): the history carries the overs per block as well
        (``CompiledSequence``), still from that one launch."""
        call = self._desk_call(gains, meters, pans, master, automation, groups, clips)
        start_frame, nframes = self._range(start_frame, nframes)
        if byte_offset < 0 or byte_offset % self.samplewidth:
            raise ValueError("CompiledSequence: byte_offset %d is not a whole number of %d-byte samples" % (byte_offset, self.samplewidth))
        return self._render_into(buf, byte_offset, start_frame, nframes, call)

    def _render_into(self, buf: Optional[N.DeviceBuffer], byte_offset: int, start_frame: int, nframes: int, call: _DeskCall):
        """the one launch of a checked call over a checked window, and what its meters give -- of an empty window, for which nothing is
        launched (``buf`` may be None), every level 0 and a history without blocks"""
        got = None
        if nframes:
            got = self._handle().render(start_frame * self.nchannels, nframes * self.nchannels, buf, byte_offset // self.samplewidth,
                                        **call.render_keywords())
        if call.meters == "history":
            return self._history(got, start_frame, nframes, call.ngroups, call.clips)
        if call.meters:
            return self._levels(got, nframes, call.ngroups)
        return None

    def _render(self, start_frame: int, nframes: int, call: _DeskCall):
        """a checked call over a checked window into a new ``Sample``, with its levels where the call has meters"""
        out = Sample(name=self.name, samplerate=self.samplerate, nchannels=self.nchannels, samplewidth=self.samplewidth)
        buf = N.DeviceBuffer(nframes * self._fb) if nframes else None
        levels = self._render_into(buf, 0, start_frame, nframes, call)
        if buf is not None:
            out._set_device(buf, nframes * self._fb)
        return (out, levels) if call.meters else out

    def render(self, start_frame: int = 0, nframes: Optional[int] = None, gains: Optional[Sequence[float]] = None, meters: bool = False,
               pans: Optional[Sequence] = None, master: Optional[float] = None, automation: Optional[Automation] = None,
               groups: Optional[Sequence] = None, clips: bool = False):
        """A new ``Sample``: frames ``[start_frame, start_frame + nframes)`` of the song; ``nframes`` None: to the end.  ``gains``: one
        per track of a song of tracks (None: all 1.0).  ``meters=True``: ``(Sample, SongLevels)``, both from the one launch;
        ``meters="history"``: ``(Sample, SongHistory)``, the levels per block of the song's tile grid, from the one launch as well.  ``pans``:
        one entry per track of a stereo song of tracks (None, a number -1 .. 1 or a pair of factors); ``master``: the master's gain;
        ``automation``: this song's fader moves (``automation()``); ``groups``: at most 8 entries ``(first_track, end_track, gain)`` or
        ``(first_track, end_track, gain, pan)``, the group buses (``CompiledSequence`` has the chain).  ``clips=True`` (with
        ``meters="history"``): the ``SongHistory`` carries the overs per block."""
        call = self._desk_call(gains, meters, pans, master, automation, groups, clips)     # (checked before the buffer is made)
        return self._render(*self._range(start_frame, nframes), call)

    def stem(self, track: int, start_frame: int = 0, nframes: Optional[int] = None) -> Sample:
        """One track of a song of tracks alone, at gain 1.0, as long as the window: ``render`` with one-hot gains."""
        self._handle()
        if self.ntracks is None:
            raise ValueError("CompiledSequence: stem needs a song of tracks (compile_tracks); this one has none")
        track = int(track)
        if track < 0 or track >= self.ntracks:
            raise ValueError("CompiledSequence: track %d outside the song's %d tracks" % (track, self.ntracks))
        return self.render(start_frame, nframes, gains=[1.0 if t == track else 0.0 for t in range(self.ntracks)])

    @staticmethod
    def stems_plane_frames(nframes: int, nchannels: int, samplewidth: int) -> int:
        """The smallest plane stride, in frames, that is at least ``nframes`` and keeps every plane on the store's 16-byte grid
        (csrc/seqstem.hpp: the stride in bytes a multiple of 16): the 16-bit kernels then store whole vectors in every plane."""
        fb = nchannels * samplewidth
        unit = 16 // math.gcd(16, fb)
        return (nframes + unit - 1) // unit * unit

    def stems_into(self, buf: N.DeviceBuffer, byte_offset: int, plane_frames: int, start_frame: int, nframes: int,
                   gains: Optional[Sequence[float]] = None, pans: Optional[Sequence] = None, master: Optional[float] = None,
                   automation: Optional[Automation] = None, groups: Optional[Sequence] = None) -> None:
        """The stems of frames ``[start_frame, start_frame + nframes)`` into ``buf``: ``ntracks + 1 + len(groups)`` planes of ``nframes``
        frames, plane ``r`` from ``byte_offset + r * plane_frames`` frames on (``plane_frames >= nframes``), in the meter rows' order --
        the tracks, the master, the groups (``SongStems`` says what each holds).  Every byte of every plane is written, whatever ``buf``
        held, and none between or around them.  One launch; the desk's keywords are ``render``'s."""
        call = self._desk_call(gains, False, pans, master, automation, groups, False, stems=True)
        start_frame, nframes = self._range(start_frame, nframes)
        plane_frames = int(plane_frames)
        if byte_offset < 0 or byte_offset % self.samplewidth:
            raise ValueError("CompiledSequence: byte_offset %d is not a whole number of %d-byte samples" % (byte_offset, self.samplewidth))
        if plane_frames < nframes:
            raise ValueError("CompiledSequence: planes %d frames apart for a window of %d frames" % (plane_frames, nframes))
        return self._stems_into(buf, byte_offset, plane_frames, start_frame, nframes, call)

    def _stems_into(self, buf: N.DeviceBuffer, byte_offset: int, plane_frames: int, start_frame: int, nframes: int, call: _DeskCall) -> None:
        """the one launch of a checked stems call over a checked window; none for an empty one"""
        if nframes:
            self._handle().stems(start_frame * self.nchannels, nframes * self.nchannels, buf, byte_offset // self.samplewidth,
                                 plane_frames * self.nchannels, **call.stems_keywords())

    def stems(self, start_frame: int = 0, nframes: Optional[int] = None, gains: Optional[Sequence[float]] = None, pans: Optional[Sequence] = None,
              master: Optional[float] = None, automation: Optional[Automation] = None, groups: Optional[Sequence] = None) -> SongStems:
        """The stems of frames ``[start_frame, start_frame + nframes)`` (``nframes`` None: to the end) of a song of tracks: a
        ``SongStems`` -- every track as its bus takes it, every group's bus as the master takes it, and the master, each a ``Sample`` of
        the window's length -- from ONE launch that walks every event once, into one device buffer the ``Sample``s share.  The desk's
        keywords are ``render``'s, and each stem is exactly what ``meters=True`` of the same call reads its row over.  (``stem(t)`` is
        something else: the raw track at gain 1.0, without the desk.)"""
        call = self._desk_call(gains, False, pans, master, automation, groups, False, stems=True)
        return self._stems(*self._range(start_frame, nframes), call)

    def _stems(self, start_frame: int, nframes: int, call: _DeskCall) -> SongStems:
        """a checked stems call over a checked window into one new buffer, every stem a view of it"""
        ngroups = call.ngroups
        nrows = self.ntracks + 1 + ngroups
        names = ["%s:track %d" % (self.name, t) for t in range(self.ntracks)] + ["%s:master" % self.name] + ["%s:group %d" % (self.name, g) for g in range(ngroups)]
        outs = [Sample(name=n, samplerate=self.samplerate, nchannels=self.nchannels, samplewidth=self.samplewidth) for n in names]
        buf = plane_frames = None
        if nframes:
            plane_frames = self.stems_plane_frames(nframes, self.nchannels, self.samplewidth)
            buf = N.DeviceBuffer(nrows * plane_frames * self._fb)
            self._stems_into(buf, 0, plane_frames, start_frame, nframes, call)
            for r, out in enumerate(outs):
                out._set_device(buf.view(r * plane_frames * self._fb, nframes * self._fb), nframes * self._fb)
        return SongStems(outs[:self.ntracks], outs[self.ntracks], outs[self.ntracks + 1:], start_frame, nframes, buffer=buf, plane_frames=plane_frames,
                         tile_frames=max(1, N.SEQ_TILE_SAMPLES[self.samplewidth] // self.nchannels))

    def level_history(self, start_frame: int = 0, nframes: Optional[int] = None, block_frames: Optional[int] = None,
                      gains: Optional[Sequence[float]] = None, pans: Optional[Sequence] = None, master: Optional[float] = None,
                      automation: Optional[Automation] = None, groups: Optional[Sequence] = None) -> SongHistory:
        """The levels of frames ``[start_frame, start_frame + nframes)`` OVER TIME for EVERY desk ``stems`` takes, rides of buses and pan
        rides included: ``stems(...)`` followed by ``SongStems.level_history(block_frames)`` -- two launches.  The ``SongHistory`` has the
        shape and the meaning of ``render(meters="history")``'s (rows: tracks, master, groups; ``total()`` what ``meters=True`` gives);
        ``block_frames`` None: the song's tile in frames, else any positive int.  The bytes are not returned: ``stems`` keeps them."""
        if block_frames is not None:
            block_frames = _block_frames("CompiledSequence", block_frames)
        call = self._desk_call(gains, False, pans, master, automation, groups, False, stems=True)
        return self._stems(*self._range(start_frame, nframes), call).level_history(block_frames)

    def waveform(self, start_frame: int = 0, nframes: Optional[int] = None, block_frames: Optional[int] = None,
                 gains: Optional[Sequence[float]] = None, pans: Optional[Sequence] = None, master: Optional[float] = None,
                 automation: Optional[Automation] = None, groups: Optional[Sequence] = None) -> Waveform:
        """The waveform extremes of frames ``[start_frame, start_frame + nframes)`` OVER TIME, for drawing, for EVERY desk ``stems`` takes:
        ``stems(...)`` followed by ``SongStems.waveform(block_frames)`` -- two launches.  The ``Waveform``'s rows are the tracks, the
        master and the groups, its blocks ``level_history``'s (``block_frames`` None: the song's tile in frames, else any positive
        int).  The bytes are not returned: ``stems`` keeps them."""
        if block_frames is not None:
            block_frames = _block_frames("CompiledSequence", block_frames)
        call = self._desk_call(gains, False, pans, master, automation, groups, False, stems=True)
        return self._stems(*self._range(start_frame, nframes), call).waveform(block_frames)

    def chunks(self, chunk_frames: int, gains: Optional[Sequence[float]] = None, meters: bool = False, pans: Optional[Sequence] = None,
               master: Optional[float] = None, automation: Optional[Automation] = None, groups: Optional[Sequence] = None,
               clips: bool = False) -> Generator:
        """The song as consecutive ``Sample``s of ``chunk_frames`` frames, the last one shorter.  ``gains``, ``pans``, ``master``,
        ``automation``, ``groups``: as ``render``'s (the joined chunks are the whole render's bytes whatever ``chunk_frames`` cuts).
        ``meters=True``: ``(Sample, SongLevels)`` pairs; ``meters="history"``: ``(Sample, SongHistory)`` pairs, with ``clips=True`` each
        with its overs."""
        chunk_frames = int(chunk_frames)
        if chunk_frames <= 0:
            raise ValueError("CompiledSequence: chunk_frames must be positive")
        call = self._desk_call(gains, meters, pans, master, automation, groups, clips)     # once, for every chunk
        for at in range(0, self.frames, chunk_frames):
            yield self._render(at, min(chunk_frames, self.frames - at), call)

    def close(self) -> None:
        if self._seq is not None:
            self._seq.free()
            self._seq = None

    def __enter__(self) -> "CompiledSequence":
        return self

    def __exit__(self, *_exc) -> None:
        self.close()

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:
            pass


def compile_sequence(events: Sequence[tuple], samplerate: int, nchannels: int, samplewidth: int = 2, name: str = "") -> CompiledSequence:
    """``sequence``'s arguments, compiled and kept instead of rendered once: the events are checked (the ``ValueError`` /
    ``NotImplementedError`` cases of ``Sample.mix_at_many``, raised before anything reaches the device), packed, planned tile by tile
    and uploaded ONCE; ``CompiledSequence.render`` / ``render_into`` / ``chunks`` then give any window of the song in one launch.  An
    event whose sample is the track itself has no meaning here (there is no track yet)."""
    return CompiledSequence(events, samplerate, nchannels, samplewidth, name)


def compile_tracks(tracks: Sequence[Sequence[tuple]], samplerate: int, nchannels: int, samplewidth: int = 2, name: str = "") -> CompiledSequence:
    """A song made of tracks, compiled once: ``tracks`` is a sequence of event lists (1 to 32 of them, a list may be empty), each list
    exactly what ``sequence`` takes and checked as ``sequence`` checks it, before anything reaches the device -- an error names the track
    and the event's index in its own list.  The song is as long as its longest track.  Every track is folded on its own and the tracks are
    mixed in order, each at a gain given when a window is rendered (``CompiledSequence``): ``render(gains=...)``, ``render_into``,
    ``chunks`` and ``stem`` mute, solo and balance the tracks in the one launch a window takes, with nothing compiled again.  A stereo
    song's tracks have a pan pot each and the song a master fader, given the same way: ``render(gains=..., pans=..., master=...)`` is
    ``sub.amplify(gain)``, then ``sub.stereo(left_factor, right_factor)``, per track, the saturating ``mix`` in track order and one
    ``master.amplify(master_gain)`` behind the last track (``CompiledSequence`` has the chain)."""
    return CompiledSequence(None, samplerate, nchannels, samplewidth, name, tracks=tracks)


class _MixSource:
    """One playing sample: its PCM in HBM (a repeating one carries one extra chunk of its own start behind its end,
    so every chunk is one contiguous range), the play position, and how many silent chunks come first."""

    def __init__(self, name: str, buf: N.DeviceBuffer, nbytes: int, loop_bytes: int, delay: int) -> None:
        self.name = name
        self.buf = buf
        self.nbytes = nbytes            # one-shot: length; repeating: length of the looped data (before the extra chunk)
        self.loop_bytes = loop_bytes    # 0 = one-shot
        self.pos = 0
        self.delay = delay
        self.acquired = False           # ordered behind its producers on the mixer's real-time lane (RealTimeMixer.chunks)


class RealTimeMixer:
    """Real-time sample mixer: samples play from the moment they are added; every turn of ``chunks()`` yields
    ``chunksize`` bytes, the saturating sum -- in the order the samples were added -- of the current chunk of every
    active sample.  A sample that ran out is dropped (``all_played_callback`` fires when the last one goes); with
    nothing playing the mixer yields silence.  Samples must be in the mixer's format (``samplewidth`` bytes per sample, 16-bit
    by default; 8-, 24- and 32-bit mixers fold with the same rule, ``audioop.add(mixed, chunk, samplewidth)``).  Mirrors upstream ``synthplayer/playback.py`` ``RealTimeMixer`` ([RECALL], tree not
    mounted): ``add_sample`` / ``remove_sample`` / ``clear_sources`` / ``chunks``.

    The PCM stays in HBM: ``add_sample`` uploads (or reuses the resident buffer of) the sample once, a chunk turn is
    one kernel over a pointer table plus ``chunksize`` bytes back to the host.  ``chunks_device()`` yields the device
    buffer instead, for a consumer that keeps going on the GPU (level metering, resampling)."""

    use_lane = True           # chunks() on the mixer's real-time lane; False: through the library's lock and stream (rounds 1-5; the A/B of tests/test_gpu_realtime_mixer.py)

    def __init__(self, chunksize: int, all_played_callback: Optional[Callable[[], None]] = None, samplewidth: int = 2) -> None:
        if samplewidth not in (1, 2, 3, 4):
            raise ValueError("samplewidth must be 1, 2, 3 or 4")
        if chunksize <= 0 or chunksize % samplewidth:
            raise ValueError("chunksize must be a positive whole number of samples")
        self.chunksize = chunksize
        self.samplewidth = samplewidth
        self.all_played_callback = all_played_callback or (lambda: None)
        self.add_lock = threading.Lock()
        self.chunks_mixed = 0
        self.active_samples: Dict[int, _MixSource] = {}
        self.sample_counter = 0
        self._out = [N.DeviceBuffer(chunksize), N.DeviceBuffer(chunksize)]      # the consumer may still hold the last one
        self._lane: Optional[N.RtLane] = None                                    # created by the first chunks() turn

    def add_sample(self, sample: Sample, repeat: bool = False, chunk_delay: int = 0, sid: Optional[int] = None) -> int:
        """Start playing a sample; returns its id.  ``repeat`` loops it forever, ``chunk_delay`` holds it back."""
        if sample.samplewidth != self.samplewidth:
            raise ValueError("sample width must be %d" % self.samplewidth)
        nbytes = len(sample) * sample.samplewidth * sample.nchannels
        if repeat and nbytes:
            # upstream: data repeated up to at least one chunk, then one more chunk of its start appended
            reps = -(-self.chunksize // nbytes) if nbytes < self.chunksize else 1
            loop = nbytes * reps
            buf = N.DeviceBuffer(loop + self.chunksize)
            src = sample._device()
            for r in range(reps):
                N.check(N.lib().sh_buf_copy(buf.handle, r * nbytes, src.handle, 0, nbytes))
            N.check(N.lib().sh_buf_copy(buf.handle, loop, buf.handle, 0, self.chunksize))
            source = _MixSource(sample.name, buf, loop, loop, chunk_delay)
        else:
            # the Sample's own buffer, read in place: _share_device() tells the Sample never to write it in place from now on
            # (Sample.mix adds in place when nothing grows -- it would change, and race with, the audio being streamed)
            source = _MixSource(sample.name, sample._share_device(), nbytes, 0, chunk_delay)
        with self.add_lock:
            self.sample_counter += 1
            sid = sid or self.sample_counter
            self.active_samples[sid] = source
            return sid

    def remove_sample(self, sid_or_name: Union[int, str]) -> None:
        with self.add_lock:
            if isinstance(sid_or_name, int):
                self.active_samples.pop(sid_or_name, None)
            else:
                for sid in [i for i, src in self.active_samples.items() if src.name == sid_or_name]:
                    del self.active_samples[sid]

    def clear_sources(self) -> None:
        with self.add_lock:
            self.active_samples.clear()
        self.all_played_callback()

    def _advance(self, lane: Optional[N.RtLane] = None) -> list:
        """One turn of the play positions: the (buffer, first sample, samples available) of every source that sounds in this chunk.
        With a real-time lane: a source the lane has not seen yet is ordered behind its producers first (sh_rt_acquire)."""
        with self.add_lock:
            active = list(self.active_samples.items())
        if lane is not None:
            for _sid, src in active:
                if not src.acquired:
                    lane.acquire(src.buf)
                    src.acquired = True
        sources = []
        finished = []
        for sid, src in active:
            if src.delay > 0:
                src.delay -= 1
                continue
            w = self.samplewidth
            if src.loop_bytes:
                sources.append((src.buf, src.pos // w, self.chunksize // w))
                src.pos = (src.pos + self.chunksize) % src.loop_bytes
            elif src.pos < src.nbytes:
                n = min(self.chunksize, src.nbytes - src.pos)
                sources.append((src.buf, src.pos // w, n // w))
                src.pos += self.chunksize
            else:
                finished.append(sid)
        if finished:
            with self.add_lock:
                for sid in finished:
                    self.active_samples.pop(sid, None)
                empty = not self.active_samples
            if empty:
                self.all_played_callback()
        return sources

    def _turn(self) -> N.DeviceBuffer:
        sources = self._advance()
        out = self._out[self.chunks_mixed & 1]
        _gather(sources, self.chunksize // self.samplewidth, out, self.samplewidth)
        self.chunks_mixed += 1
        return out

    def _turn_host(self) -> bytes:
        """One chunk on the mixer's REAL-TIME LANE (sh_rt_*): a stream, a lock and buffers of the mixer's own -- the turn neither takes the
        library's lock nor queues behind what other threads have enqueued (a bank streaming its blocks, Sample operations); the same
        fold kernels as ``_turn``: bit-identical chunks.  A source is ordered behind its producers once, before its first turn."""
        if self._lane is None:
            self._lane = N.RtLane(self.chunksize, max_sources=32768)
        sources = self._advance(self._lane)
        chunk = self._lane.mix_turn(sources, self.chunksize // self.samplewidth, self.samplewidth)
        self.chunks_mixed += 1
        return chunk

    def chunks_device(self) -> Generator[N.DeviceBuffer, None, None]:
        """Endless stream of mixed chunks left in HBM (valid until the turn after the next)."""
        while True:
            yield self._turn()

    def chunks(self) -> Generator[memoryview, None, None]:
        """Endless stream of mixed chunks, ``chunksize`` bytes each (on the mixer's real-time lane: see ``_turn_host``)."""
        while True:
            yield memoryview(self._turn_host() if self.use_lane else self._turn().download_bytes(self.chunksize))
