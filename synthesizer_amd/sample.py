"""
Sample: signed-integer PCM container with the hot-path operations of upstream
``synthplayer/sample.py`` (tree not mounted at /root/reference): ``from_osc_block`` (quantise),
``mix`` / ``mix_at`` (saturating add) and ``resample`` (linear interpolation), plus the
constructors/accessors a caller needs around them.  The arithmetic upstream delegates to CPython's
``audioop`` (add, ratecv) runs here as HIP kernels over PCM that stays resident in HBM; results are
bit-exact with ``audioop`` (tests/test_gpu_pcm.py).

Frames live either on the host (``bytes``) or on the device (``DeviceBuffer``); operations move them
to the device once and leave them there, accessors bring them back lazily.  There is no CPU
implementation of the arithmetic in this package.

Also here (the elementwise operations upstream delegates to audioop):
amplify / amplify_max / invert (``audioop.mul``), bias, reverse, mono / left / right (``tomono``),
stereo / pan (``tostereo``), normalize / make_16bit / make_32bit (``lin2lin``), peak / rms, fadein / fadeout.
Editing operations composed from those on device-resident PCM: clip / split / join / add_silence / delay,
speed (``ratecv``), at_volume, echo, envelope (ADSR), modulate_amp (sample- or oscillator-driven).
Level metering: ``level_db_peak`` / ``level_db_rms`` (both channels from ONE pass over the interleaved PCM, where
upstream makes two ``tomono`` copies and reads each) and the stateful ``LevelMeter``.
24-bit samples (width 3): everything upstream delegates to audioop; not the per-sample ``array`` operations (fades,
modulate_amp, pan with an lfo), which have no 24-bit form upstream either.
"""
from __future__ import annotations

import array
import ctypes as C
import math
import wave
from typing import BinaryIO, Iterable, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from . import params
from . import _native as N

__all__ = ["Sample", "LevelMeter"]

_TYPECODE = {1: "b", 2: "h", 4: "i"}
_NPTYPE = {1: np.int8, 2: np.int16, 4: np.int32}
_MAX_CALL_SAMPLES = 0xFFFF0000                              # shq::MAX_TRACK_SAMPLES: positions are 32 bits on the device


_MAX_DOWNMIX_SOURCE_SAMPLES = 0xFFFF0000                    # sh_mix_events_chan: 2 * (dst_sample + nsamples) of a downmix, in 32 bits


def _ratecv_out_frames(in_frames: int, inrate: int, outrate: int) -> int:
    """Frames ``audioop.ratecv`` makes of ``in_frames`` (sh_resample_out_frames, in Python integers): output frame m exists while
    ceil(m inrate / outrate) <= in_frames - 1."""
    return (in_frames - 1) * outrate // inrate + 1 if in_frames else 0


def _envelope_segments(nbytes: int, width: int, nchannels: int, rate: int, attack: float, decay: float, sustainlevel: float,
                       release: float) -> list:
    """What ``Sample.envelope(attack, decay, sustainlevel, release)`` does to a sample of ``nbytes`` bytes, as consecutive segments
    ``(end, mul, kind, slope, numsamples, offset, origin)`` in SAMPLES (sh_env_segment): upstream's split / amplify / fadein /
    fadeout / join replayed in Python floats as they stand -- ``frame_idx(s) = fb * int(rate * s)``, ``duration = nbytes / rate /
    width / nchannels``, ``min(seconds, duration)``, ``frame_idx(duration - seconds)``, ``S.duration - release`` -- so that a frame the
    rounding leaves unfaded at the tail of the attack or the head of the decay or release part stays unfaded here.  Empty segments are
    dropped and neighbours without a ramp and with the same mul are one.  ValueError where upstream's ``S.duration - release`` is
    negative (it slices from the wrong end then)."""
    fb = width * nchannels

    def frame_idx(seconds):
        return fb * int(rate * seconds)

    def duration(nb):
        return nb / rate / width / nchannels

    a_len = min(frame_idx(attack), nbytes)                  # self.split(attack): frames[:end] | frames[end:]
    d_len = min(frame_idx(decay), nbytes - a_len)           # D.split(decay)
    s_all = nbytes - a_len - d_len                          # S, the release still in it: all of it through audioop.mul
    rest = duration(s_all) - release
    if rest < 0:
        raise ValueError("mix_at_many: envelope: the release (%r s) is longer than what attack and decay leave (%r s)" % (release, duration(s_all)))
    s_len = min(frame_idx(rest), s_all)                     # S.split(S.duration - release)
    r_len = s_all - s_len
    mul = float(sustainlevel) if sustainlevel < 1 else 1.0
    parts = []                                              # (first byte, bytes, mul, kind, slope, offset)
    a_fade = 0
    if attack > 0:                                          # fadein: begin = frames[:frame_idx(min(seconds, duration))]
        a_fade = min(frame_idx(min(attack, duration(a_len))), a_len)
        parts.append((0, a_fade, 1.0, N.ENV_FADE_IN, 1.0 - 0.0, 0.0))
    parts.append((a_fade, a_len - a_fade, 1.0, N.ENV_NONE, 0.0, 0.0))
    d_head = d_len
    if decay > 0:                                           # fadeout: end = frames[frame_idx(duration - min(seconds, duration)):]
        d_head = min(frame_idx(duration(d_len) - min(decay, duration(d_len))), d_len)
    parts.append((a_len, d_head, 1.0, N.ENV_NONE, 0.0, 0.0))
    parts.append((a_len + d_head, d_len - d_head, 1.0, N.ENV_FADE_OUT, 1.0 - float(sustainlevel), 0.0))
    r_head = r_len
    if release > 0:
        r_head = min(frame_idx(duration(r_len) - min(release, duration(r_len))), r_len)
    s_at = a_len + d_len
    parts.append((s_at, s_len + r_head, mul, N.ENV_NONE, 0.0, 0.0))
    parts.append((s_at + s_len + r_head, r_len - r_head, mul, N.ENV_FADE_OUT, 1.0 - 0.0, 0.0))
    segs = []
    for first, nb, m, kind, slope, offset in parts:
        if not nb:
            continue
        end = (first + nb) // width
        if kind == N.ENV_NONE and segs and segs[-1][2] == N.ENV_NONE and segs[-1][1] == m:
            segs[-1] = (end,) + segs[-1][1:]
        else:
            segs.append((end, m, kind, slope, float(nb // width) if kind else 0.0, offset, first // width))
    return segs


def _loop_frames(loop, rate: int, frames: Optional[int], nchannels: int) -> tuple:
    """``(loop_start, loop_end, length)`` in seconds of a sample of ``frames`` frames as ``(S, E - S, V)`` in frames: ``S = int(rate *
    loop_start)`` and ``E = min(int(rate * loop_end), frames)`` as ``clip`` cuts them, ``V = int(rate * length)``; ``frames`` None: E is
    not clamped (the track as its own source: it is clamped to what the track holds when the event runs).  Its ValueErrors: not three
    numbers, one that is not finite or negative, an empty loop after the clamp to the sample, more than one call can address."""
    if not isinstance(loop, (tuple, list)) or len(loop) != 3:
        raise ValueError("mix_at_many: loop is (loop_start, loop_end, length)")
    try:
        good = all(math.isfinite(v) and v >= 0 for v in loop)
    except TypeError:
        good = False
    if not good:
        raise ValueError("mix_at_many: loop: loop_start, loop_end and length are finite and not negative")
    start, end, virtual = int(rate * loop[0]), int(rate * loop[1]), int(rate * loop[2])
    if frames is not None:
        end = min(end, frames)
    if start >= end:
        raise ValueError("mix_at_many: loop: no frame between loop_start (frame %d) and loop_end (frame %d)" % (start, end))
    if virtual * nchannels > _MAX_CALL_SAMPLES:
        raise ValueError("mix_at_many: loop: a note of %d frames is more than one call can address" % virtual)
    return start, end - start, virtual


def _region_frames(region, rate: int, frames: Optional[int], duration: float) -> tuple:
    """``(start, end)`` in seconds of a sample of ``frames`` frames as ``(first frame, frames)``, as ``clip(start, end)`` cuts them:
    ``int(rate * start)`` and ``int(rate * end)`` under byte-slicing rules, so both clamped to the sample; ``end`` None: the sample's
    ``duration``, a float, through the same ``int(rate * duration)``.  ``frames`` None (the track as its own source: it is cut when the
    event runs): only the checks.  Its ValueErrors: not a pair, a start or end that is not finite or is negative, ``end < start``."""
    if not isinstance(region, (tuple, list)) or len(region) != 2:
        raise ValueError("mix_at_many: region is (start, end), end may be None")
    start, end = region
    if end is None:
        end = duration if frames is not None else start
    try:
        good = math.isfinite(start) and start >= 0 and math.isfinite(end) and end >= 0
    except TypeError:
        good = False
    if not good:
        raise ValueError("mix_at_many: region: start and end are finite and not negative")
    if end < start:
        raise ValueError("mix_at_many: region: end (%r s) lies before start (%r s)" % (end, start))
    if frames is None:
        return 0, 0
    first, last = min(int(rate * start), frames), min(int(rate * end), frames)
    return first, last - first


def _channel_weights(channels, other_nchannels: int, track_nchannels: int) -> tuple:
    """``channels`` of an event as ``(left_factor, right_factor)`` in floats, for a stereo ``other`` and a mono or stereo track"""
    if not isinstance(channels, (tuple, list)) or len(channels) != 2:
        raise ValueError("mix_at_many: channels is a pair (left_factor, right_factor)")
    try:
        weights = (float(channels[0]), float(channels[1]))
    except (TypeError, ValueError):
        raise ValueError("mix_at_many: channels is a pair of numbers, not %r" % (tuple(channels),)) from None
    if not (math.isfinite(weights[0]) and math.isfinite(weights[1])):
        raise ValueError("mix_at_many: channels factor is not finite")
    if other_nchannels != 2:
        raise ValueError("mix_at_many: channels needs a stereo sample, this one has %d channels" % other_nchannels)
    if track_nchannels not in (1, 2):
        raise ValueError("mix_at_many: channels needs a mono or stereo track, this one has %d channels" % track_nchannels)
    return weights


def _pan_factors(pan, other_nchannels: int, track_nchannels: int) -> tuple:
    """``pan`` of an event -- a float -1 .. 1 or the pair itself -- as ``audioop.tostereo``'s ``(left_factor, right_factor)``, for a mono
    ``other`` and a stereo track"""
    if other_nchannels != 1:
        raise ValueError("mix_at_many: pan needs a mono sample, this one has %d channels" % other_nchannels)
    if track_nchannels != 2:
        raise ValueError("mix_at_many: pan needs a stereo track, this one has %d channels" % track_nchannels)
    if isinstance(pan, (tuple, list)):
        if len(pan) != 2:
            raise ValueError("mix_at_many: pan is a number or a pair (left_factor, right_factor)")
        factors = (float(pan[0]), float(pan[1]))
    else:
        if not -1.0 <= pan <= 1.0:
            raise ValueError("mix_at_many: pan must be between -1 and 1")
        factors = ((1.0 - pan) / 2.0, (1.0 + pan) / 2.0)    # Sample.pan: Python floats, on the host
    if not (math.isfinite(factors[0]) and math.isfinite(factors[1])):
        raise ValueError("mix_at_many: pan factor is not finite")
    return factors


def _envelope_rows(envelope, frames: int, width: int, nchannels: int, rate: int) -> tuple:
    """``envelope`` of an event whose (resampled) ``other`` has ``frames`` frames of ``nchannels`` channels: (the frames the note's length
    leaves, _envelope_segments' rows over them)"""
    if width == 3:
        raise NotImplementedError("mix_at_many: envelope: 3-byte samples are not supported (fades have no 24-bit form)")
    if not isinstance(envelope, (tuple, list)) or len(envelope) not in (4, 5):
        raise ValueError("mix_at_many: envelope is (attack, decay, sustainlevel, release) or (attack, decay, sustainlevel, release, length)")
    if not all(math.isfinite(v) and v >= 0 for v in envelope[:2] + envelope[3:]):
        raise ValueError("mix_at_many: envelope: attack, decay, release and length are finite and not negative")
    if not 0 <= envelope[2] <= 1:
        raise ValueError("mix_at_many: envelope: sustainlevel must be between 0 and 1")
    if len(envelope) == 5:                                  # clip(0.0, length): frames[0:frame_idx(length)] of the other's own frames
        frames = min(frames, int(rate * envelope[4]))
    return frames, _envelope_segments(frames * width * nchannels, width, nchannels, rate, *envelope[:4])


class _Event(NamedTuple):
    """One checked event of mix_at_many, as Sample._check_events leaves it.  What the caller gave, then what the checks made of it."""
    seconds: float
    other: "Sample"
    volume: Optional[float]
    other_seconds: Optional[float]
    speed: Optional[float]
    start: int                                              # the first byte of the track it touches
    nbytes: int                                             # bytes of the track it covers: resampled, stereo if panned, mono if downmixed, cut
    inrate: int                                             # != the track's rate: ``other`` is resampled from it, and nbytes counts resampled bytes
    pan: Optional[tuple]                                    # audioop.tostereo's (left, right): ``other`` is mono, the track stereo
    loop: Optional[tuple]                                   # (loop_start, loop_frames, virtual frames), in frames of the region
    region: Optional[tuple]                                 # (first frame, frames) of ``other``: what nbytes, loop and segments were counted over
    reverse: bool
    weights: Optional[tuple]                                # ``channels``: a downmix in a mono track, a balance in a stereo one
    envelope: Optional[tuple]                               # as the caller gave it
    segments: Optional[list]                                # _envelope_segments' rows, over the uncut note
    level: int                                              # the highest rung of N.MIX_LEVELS that an attribute of this event needs
    own_region: Optional[tuple]                             # ``other`` is the track itself: the caller's (start, end) in SECONDS, cut when the event runs


_new_event = tuple.__new__                                  # (as _Event._make builds one: a third of the time of _Event(...) per event)
_NO_MORE = (None,) * 9                                      # what an event shorter than the full 11 leaves unsaid


class Sample:
    """Audio sample data: interleaved little-endian signed PCM."""

    norm_samplerate = params.norm_samplerate
    norm_nchannels = params.norm_nchannels
    norm_samplewidth = params.norm_samplewidth

    def __init__(self, wave_file: Optional[Union[str, BinaryIO]] = None, name: str = "", samplerate: int = 0,
                 nchannels: int = 0, samplewidth: int = 0) -> None:
        self.name = name
        self.__locked = False
        self.__samplerate = samplerate or params.norm_samplerate
        self.__nchannels = nchannels or params.norm_nchannels
        self.__samplewidth = samplewidth or params.norm_samplewidth
        self.__frames: Optional[bytes] = b""
        self.__dev: Optional[N.DeviceBuffer] = None
        self.__dev_shared = False      # somebody else (a playing mixer source) reads __dev: never write it in place
        self.__nbytes = 0
        self.filename = None
        if wave_file:
            self.load_wav(wave_file)
            if isinstance(wave_file, str):
                self.filename = wave_file

    # -- storage -------------------------------------------------------------------------------
    def _set_host(self, frames: bytes) -> None:
        self.__frames = bytes(frames)
        self.__dev = None
        self.__dev_shared = False
        self.__nbytes = len(self.__frames)

    def _set_device(self, buf: N.DeviceBuffer, nbytes: int) -> None:
        if buf is not self.__dev:
            self.__dev_shared = False  # a fresh buffer is this Sample's own again
        self.__frames = None
        self.__dev = buf
        self.__nbytes = nbytes

    def _share_device(self) -> N.DeviceBuffer:
        """The device buffer, handed to a reader that keeps it (RealTimeMixer.add_sample streams from it): from now on every
        operation of this Sample writes a buffer of its own -- the in-place form of mix / mix_at is off until the data moves."""
        buf = self._device()
        self.__dev_shared = True
        return buf

    def _host(self) -> bytes:
        if self.__frames is None:
            self.__frames = self.__dev.download_bytes(self.__nbytes) if self.__nbytes else b""
        return self.__frames

    def _device(self) -> N.DeviceBuffer:
        if self.__dev is None:
            self.__dev = N.DeviceBuffer.from_bytes(self.__frames or b"")
        return self.__dev

    def to_device(self) -> "Sample":
        """Make the PCM resident in HBM (drops nothing; the host copy is kept until modified)."""
        self._device()
        return self

    @property
    def on_device(self) -> bool:
        return self.__dev is not None

    # -- constructors --------------------------------------------------------------------------
    @classmethod
    def from_raw_frames(cls, frames: Union[bytes, memoryview, bytearray], samplewidth: int, samplerate: int,
                        numchannels: int, name: str = "") -> "Sample":
        assert samplewidth in (1, 2, 3, 4) and numchannels >= 1 and samplerate > 1
        s = cls(name=name, samplerate=samplerate, nchannels=numchannels, samplewidth=samplewidth)
        frames = bytes(frames)
        if len(frames) % (samplewidth * numchannels):
            raise ValueError("frames data is not a whole number of frames")
        s._set_host(frames)
        return s

    @classmethod
    def from_array(cls, array_or_list: Union[Sequence[int], array.array, np.ndarray], samplerate: int,
                   numchannels: int, name: str = "") -> "Sample":
        if isinstance(array_or_list, np.ndarray):
            width = array_or_list.dtype.itemsize
            assert array_or_list.dtype.kind == "i" and width in (1, 2, 4)
            frames = np.ascontiguousarray(array_or_list).astype(array_or_list.dtype.newbyteorder("<")).tobytes()
        else:
            if isinstance(array_or_list, list):
                try:
                    array_or_list = array.array("h", array_or_list)       # OverflowError when out of range
                except OverflowError:
                    array_or_list = array.array("i", array_or_list)
            width = array_or_list.itemsize
            frames = array_or_list.tobytes()
        return cls.from_raw_frames(frames, width, samplerate, numchannels, name)

    @classmethod
    def from_osc_block(cls, block: Union[Iterable[float], np.ndarray], samplerate: int,
                       amplitude_scale: Optional[float] = None, samplewidth: int = 0) -> "Sample":
        """Quantise one oscillator block (mono): ``int(amplitude_scale * v)`` per sample, truncating
        toward zero, OverflowError when a value does not fit -- upstream Sample.from_osc_block."""
        width = samplewidth or params.norm_samplewidth
        if width not in (1, 2, 4):
            raise NotImplementedError("from_osc_block: sample width %d" % width)
        if amplitude_scale is None:
            amplitude_scale = 2 ** (8 * width - 1) - 1
        arr = block if isinstance(block, np.ndarray) else np.asarray(list(block), dtype=np.float64)
        if arr.dtype not in (np.float32, np.float64):
            arr = arr.astype(np.float64)
        n = int(arr.size)
        s = cls(samplerate=samplerate, nchannels=1, samplewidth=width)
        if n == 0:
            return s
        src = N.DeviceBuffer.from_array(arr.reshape(-1))
        dst = N.DeviceBuffer(n * width)
        fn = N.lib().sh_quantize_f32 if arr.dtype == np.float32 else N.lib().sh_quantize_f64
        N.check(fn(src.handle, 0, n, float(amplitude_scale), width, dst.handle, 0))
        src.free()
        s._set_device(dst, n * width)
        return s

    @classmethod
    def from_osc_device(cls, block_f64: N.DeviceBuffer, n: int, samplerate: int,
                        amplitude_scale: Optional[float] = None, samplewidth: int = 0, free_block: bool = True) -> "Sample":
        """from_osc_block for a float64 block that already lives in HBM (an oscillator's ``_render_f64_device``): the
        quantiser reads the float64 samples the reference would have yielded, nothing is rounded to float32 on the way."""
        width = samplewidth or params.norm_samplewidth
        if width not in (1, 2, 4):
            raise NotImplementedError("from_osc_block: sample width %d" % width)
        if amplitude_scale is None:
            amplitude_scale = 2 ** (8 * width - 1) - 1
        s = cls(samplerate=samplerate, nchannels=1, samplewidth=width)
        if n:
            dst = N.DeviceBuffer(n * width)
            try:
                N.check(N.lib().sh_quantize_f64(block_f64.handle, 0, n, float(amplitude_scale), width, dst.handle, 0))
            finally:
                if free_block:
                    block_f64.free()
            s._set_device(dst, n * width)
        return s

    # -- accessors -------------------------------------------------------------------------------
    @property
    def samplewidth(self) -> int:
        return self.__samplewidth

    @property
    def samplerate(self) -> int:
        return self.__samplerate

    @samplerate.setter
    def samplerate(self, rate: int) -> None:
        assert rate > 0
        self.__samplerate = int(rate)

    @property
    def nchannels(self) -> int:
        return self.__nchannels

    @property
    def duration(self) -> float:
        return self.__nbytes / self.__samplerate / self.__samplewidth / self.__nchannels

    @property
    def maximum(self) -> int:
        return 2 ** (8 * self.__samplewidth - 1) - 1

    def __len__(self) -> int:
        """Number of frames."""
        return self.__nbytes // self.__samplewidth // self.__nchannels

    def __eq__(self, other) -> bool:
        if not isinstance(other, Sample):
            return False
        return (self.__samplewidth == other.__samplewidth and self.__samplerate == other.__samplerate and
                self.__nchannels == other.__nchannels and self._host() == other._host())

    def __repr__(self) -> str:
        return "<Sample '%s' at 0x%x, %g seconds, %d channels, %d bits, rate %d>" % (
            self.name, id(self), self.duration, self.__nchannels, 8 * self.__samplewidth, self.__samplerate)

    def frame_idx(self, seconds: float) -> int:
        """Byte index of the frame at the given time."""
        return self.__nchannels * self.__samplewidth * int(self.__samplerate * seconds)

    def view_frame_data(self) -> memoryview:
        return memoryview(self._host())

    def get_frame_array(self) -> array.array:
        if self.__samplewidth not in _TYPECODE:
            raise NotImplementedError("get_frame_array: sample width %d" % self.__samplewidth)
        return array.array(_TYPECODE[self.__samplewidth], self._host())

    def get_frames_numpy(self) -> np.ndarray:
        """[frames, channels] integer array (copy)."""
        if self.__samplewidth == 3:                   # 24-bit little endian -> int32
            b = np.frombuffer(self._host(), dtype=np.uint8).reshape(-1, 3).astype(np.int32)
            v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
            return (v - ((v & 0x800000) << 1)).reshape(-1, self.__nchannels)
        return np.frombuffer(self._host(), dtype=_NPTYPE[self.__samplewidth]).reshape(-1, self.__nchannels).copy()

    def get_frames_as_floats(self) -> Sequence[float]:
        maxsize = 2 ** (8 * self.__samplewidth - 1)
        return [v / maxsize for v in self.get_frame_array()]

    def copy(self) -> "Sample":
        cpy = Sample(name=self.name, samplerate=self.__samplerate, nchannels=self.__nchannels,
                     samplewidth=self.__samplewidth)
        if self.__dev is not None and self.__frames is None:        # resident in HBM only: copy it there
            buf = N.DeviceBuffer(self.__nbytes)
            if self.__nbytes:
                N.check(N.lib().sh_buf_copy(buf.handle, 0, self.__dev.handle, 0, self.__nbytes))
            cpy._set_device(buf, self.__nbytes)
        else:
            cpy._set_host(self._host())
        cpy.filename = self.filename
        return cpy

    def chunked_frame_data(self, chunksize: int, repeat: bool = False, stopcondition=lambda: False):
        """Generator over the frame bytes in chunks of ``chunksize`` bytes (the last one of a one-shot sample may be
        shorter); with ``repeat`` the data wraps around forever and every chunk is full."""
        frames = self._host()
        if repeat:
            if not frames:
                return
            if len(frames) < chunksize:
                frames = frames * math.ceil(chunksize / len(frames))
            length = len(frames)
            mdata = memoryview(frames + frames[:chunksize])
            i = 0
            while not stopcondition():
                yield mdata[i: i + chunksize]
                i = (i + chunksize) % length
        else:
            mdata = memoryview(frames)
            i = 0
            while i < len(mdata) and not stopcondition():
                yield mdata[i: i + chunksize]
                i += chunksize

    def lock(self) -> "Sample":
        self.__locked = True
        return self

    def _check_writable(self) -> None:
        if self.__locked:
            raise RuntimeError("cannot modify a locked sample")

    # -- WAV in/out (host only, stdlib wave) -----------------------------------------------------
    def load_wav(self, file_or_stream: Union[str, BinaryIO]) -> "Sample":
        self._check_writable()
        with wave.open(file_or_stream) as w:
            if not 2 <= w.getsampwidth() <= 4:
                raise IOError("only supports sample sizes of 2, 3 or 4 bytes")
            if not 1 <= w.getnchannels() <= 2:
                raise IOError("only supports mono or stereo channels")
            self.__nchannels = w.getnchannels()
            self.__samplerate = w.getframerate()
            self.__samplewidth = w.getsampwidth()
            self._set_host(w.readframes(w.getnframes()))
        return self

    def write_wav(self, file_or_stream: Union[str, BinaryIO]) -> None:
        with wave.open(file_or_stream, "wb") as out:
            out.setparams((self.__nchannels, self.__samplewidth, self.__samplerate, 0, "NONE", "not compressed"))
            out.writeframes(self._host())

    # -- editing: slices and concatenations of device-resident PCM -------------------------------------
    def __assemble(self, parts: Sequence[tuple]) -> None:
        """frames = concatenation of parts; a part is (sample, first_byte, nbytes) or (None, 0, nbytes) for silence."""
        total = sum(p[2] for p in parts)
        dst = N.DeviceBuffer(total)
        L = N.lib()
        at = 0
        for src, first, nbytes in parts:
            if nbytes:
                if src is None:
                    dst.zero(at, nbytes)
                else:
                    N.check(L.sh_buf_copy(dst.handle, at, src._device().handle, first, nbytes))
            at += nbytes
        self._set_device(dst, total)

    def add_silence(self, seconds: float, at_start: bool = False) -> "Sample":
        """Add silence at the end (or at the start)."""
        self._check_writable()
        pad = self.frame_idx(seconds)
        if pad:
            me = (self, 0, self.__nbytes)
            keep = self.__dev          # keep the source alive while it is being copied
            self.__assemble([(None, 0, pad), me] if at_start else [me, (None, 0, pad)])
            del keep
        return self

    def clip(self, start_seconds: float, end_seconds: float) -> "Sample":
        """Keep only the given time range."""
        self._check_writable()
        assert end_seconds >= start_seconds
        start, end = self.frame_idx(start_seconds), self.frame_idx(end_seconds)
        if start != 0 or end != self.__nbytes:
            start, end, _ = slice(start, end).indices(self.__nbytes)      # byte-string slicing rules, as upstream
            keep = self.__dev
            self.__assemble([(self, start, max(0, end - start))])
            del keep
        return self

    def split(self, seconds: float) -> "Sample":
        """Keep the first part and return the chopped-off rest as a new sample."""
        self._check_writable()
        end = self.frame_idx(seconds)
        rest = Sample(name=self.name, samplerate=self.__samplerate, nchannels=self.__nchannels, samplewidth=self.__samplewidth)
        if end != self.__nbytes:
            end = slice(end, None).indices(self.__nbytes)[0]               # byte-string slicing rules, as upstream
            rest.__assemble([(self, end, self.__nbytes - end)])
            keep = self.__dev
            self.__assemble([(self, 0, end)])
            del keep
        return rest

    def join(self, other: "Sample") -> "Sample":
        """Append another sample to this one."""
        self._check_writable()
        assert self.samplewidth == other.samplewidth
        assert self.samplerate == other.samplerate
        assert self.nchannels == other.nchannels
        if other.__nbytes:
            keep = self.__dev
            self.__assemble([(self, 0, self.__nbytes), (other, 0, other.__nbytes)])
            del keep
        return self

    def delay(self, seconds: float, keep_length: bool = False) -> "Sample":
        """Delay the sample (insert silence at the start); a negative delay skips a bit from the start instead."""
        self._check_writable()
        if seconds > 0:
            if keep_length:
                num_frames = len(self)
                self.add_silence(seconds, at_start=True)
                self.clip(0, num_frames / self.samplerate)
            else:
                self.add_silence(seconds, at_start=True)
        elif seconds < 0:
            seconds = -seconds
            if keep_length:
                self.add_silence(seconds)
            self.clip(seconds, self.duration)
        return self

    def speed(self, speed: float) -> "Sample":
        """Change the playback speed (and the pitch) without changing the sample rate: frames are interpolated with
        ``audioop.ratecv(frames, width, nchannels, int(samplerate*speed), samplerate, None)``."""
        self._check_writable()
        assert speed > 0
        if speed == 1.0:
            return self
        if speed > 10.0 or speed < 0.1:
            raise ValueError("speed must be between 0.1 and 10")
        rate = self.__samplerate
        self.__samplerate = int(rate * speed)
        self.resample(rate)
        return self

    def at_volume(self, volume: float) -> "Sample":
        """A copy of the sample at the given volume 0..1 (works on locked samples: the original is untouched)."""
        cpy = self.copy()
        cpy.amplify(volume)
        return cpy

    def echo(self, length: float, amount: int, delay: float, decay: float) -> "Sample":
        """Add `amount` echos of the last `length` seconds, `delay` seconds apart, each `decay` times the previous
        volume.  Echos too quiet for the sample width are skipped."""
        self._check_writable()
        self._check_gpu_width("echo")
        if amount > 0:
            length = max(0, self.duration - length)
            echo = Sample(name=self.name, samplerate=self.__samplerate, nchannels=self.__nchannels, samplewidth=self.__samplewidth)
            first = slice(self.frame_idx(length), None).indices(self.__nbytes)[0]      # frames[frame_idx(length):], as upstream
            echo.__assemble([(self, first, self.__nbytes - first)])
            echo_amp = decay
            for _ in range(amount):
                if echo_amp < 1.0 / (2 ** (8 * self.__samplewidth - 1)):
                    break       # an echo nobody can hear
                length += delay
                echo = echo.copy().amplify(echo_amp)
                self.mix_at(length, echo)
                echo_amp *= decay
        return self

    def envelope(self, attack: float, decay: float, sustainlevel: float, release: float) -> "Sample":
        """Apply an ADSR volume envelope; attack, decay and release in seconds, sustainlevel a factor."""
        self._check_writable()
        assert attack >= 0 and decay >= 0 and release >= 0
        assert 0 <= sustainlevel <= 1
        D = self.split(attack)          # self is now the attack part
        S = D.split(decay)
        if sustainlevel < 1:
            S.amplify(sustainlevel)
        R = S.split(S.duration - release)
        if attack > 0:
            self.fadein(attack)
        if decay > 0:
            D.fadeout(decay, sustainlevel)
        if release > 0:
            R.fadeout(release)
        self.join(D).join(S).join(R)
        return self

    def modulate_amp(self, modulation_source) -> "Sample":
        """Amplitude modulation: every sample becomes int(sample * factor).  The factors come from an oscillator
        (its block stream from the start), from another Sample or a sequence of numbers (cycled, scaled so that its
        largest absolute value is 1.0), or from any iterable of floats."""
        self._check_writable()
        self._check_gpu_width("modulate_amp")
        n = self.__nbytes // self.__samplewidth
        if not n:
            return self
        L = N.lib()
        from .oscillators import Oscillator
        if isinstance(modulation_source, Sample):
            modulation_source._check_gpu_width("modulate_amp")
            nmod = modulation_source.__nbytes // modulation_source.__samplewidth
            if not nmod:
                raise ValueError("modulation sample is empty")
            biggest = modulation_source.peak()
            mod = N.DeviceBuffer(nmod * 8)
            N.check(L.sh_pcm_to_f64(modulation_source._device().handle, nmod, modulation_source.__samplewidth, float(biggest), mod.handle))
        elif isinstance(modulation_source, Oscillator):
            nmod = n
            mod = modulation_source._render_f64_device(0, n)
        else:
            if isinstance(modulation_source, (list, tuple, array.array, np.ndarray)):
                values = np.asarray(modulation_source, dtype=np.float64)
                if not len(values):
                    raise ValueError("modulation sequence is empty")
                biggest = max(values.max(), abs(values.min()))
                values = values / biggest
            else:
                import itertools
                values = np.fromiter(itertools.islice(iter(modulation_source), n), dtype=np.float64)
                if len(values) < n:
                    raise ValueError("modulation iterator ran out after %d of %d samples" % (len(values), n))
            nmod = len(values)
            mod = N.DeviceBuffer(nmod * 8)
            mod.upload(values)
        dst = N.DeviceBuffer(self.__nbytes)
        N.check(L.sh_pcm_modulate(self._device().handle, self.__nbytes, self.__samplewidth, mod.handle, nmod, dst.handle))
        self._set_device(dst, self.__nbytes)
        return self

    # -- the hot path ----------------------------------------------------------------------------
    # 24-bit samples: every operation upstream hands to audioop (which reads 3-byte samples) runs on the GPU too; the ones
    # upstream does sample by sample through ``array`` (fades, modulate_amp, pan with an lfo, from_osc_block) have no 24-bit
    # form there either (no array typecode) and none here
    _WIDTH3_OK = frozenset(("mix", "mix_at", "amplify", "peak", "rms", "level_db", "bias", "reverse", "mono", "stereo", "normalize",
                            "make_32bit", "make_16bit", "resample", "echo"))

    def _check_gpu_width(self, what: str) -> None:
        if self.__samplewidth == 3 and what in self._WIDTH3_OK:
            return
        if self.__samplewidth not in (1, 2, 4):
            raise NotImplementedError("%s: %d-byte samples are not supported on the GPU path" % (what, self.__samplewidth))

    def mix(self, other: "Sample", other_seconds: Optional[float] = None, pad_shortest: bool = True) -> "Sample":
        """Mix another sample into this one (saturating add).  The shorter operand is zero-padded
        unless pad_shortest is False, in which case unequal lengths are an error (audioop.add)."""
        self._check_writable()
        assert self.samplewidth == other.samplewidth
        assert self.samplerate == other.samplerate
        assert self.nchannels == other.nchannels
        self._check_gpu_width("mix")
        n1 = self.__nbytes
        n2 = other.__nbytes if not other_seconds else min(other.__nbytes, other.frame_idx(other_seconds))
        if not pad_shortest and n1 != n2:
            raise ValueError("Lengths should be the same")
        self.__mix_region(other, 0, n2, max(n1, n2))
        return self

    def mix_at(self, seconds: float, other: "Sample", other_seconds: Optional[float] = None) -> "Sample":
        """Mix another sample into this one starting at the given time; grows as needed."""
        if seconds == 0.0:
            return self.mix(other, other_seconds)
        self._check_writable()
        assert self.samplewidth == other.samplewidth
        assert self.samplerate == other.samplerate
        assert self.nchannels == other.nchannels
        self._check_gpu_width("mix_at")
        start = self.frame_idx(seconds)
        n2 = other.frame_idx(other_seconds) if other_seconds else other.__nbytes
        n2 = min(n2, other.__nbytes)
        self.__mix_region(other, start, n2, max(self.__nbytes, start + n2))
        return self

    def __mix_region(self, other: "Sample", start: int, n2: int, total: int) -> None:
        """self[start:start+n2] = sat_add(self[start:start+n2] (zero-extended), other[:n2]); length -> total."""
        L = N.lib()
        n1 = self.__nbytes
        aliased = other is self and start != 0              # overlapping source and destination at shifted offsets inside one kernel
        if total == n1 and n1 and self._device().nbytes >= n1 and not self.__dev_shared and not aliased:
            # nothing grows (the mixer's common case: equal lengths, or mix_at inside the sample): add in place -- the kernel is
            # elementwise and declared without __restrict__ for exactly this -- 3 bytes moved per output byte instead of 5 (allocate,
            # copy self, add).  A Sample's device buffer is its own (copy() copies), so nobody else sees the write; a lock()ed
            # sample never gets here (_check_writable); one that a mixer streams from (_share_device) and a mix_at of the sample
            # into itself at an offset take the copying form below.
            if n2:
                N.check(L.sh_pcm_add(self.__dev.handle, start, other._device().handle, 0, n2, self.__samplewidth, self.__dev.handle, start))
            self._set_device(self.__dev, n1)            # (drops the host copy: it is stale now)
            return
        dst = N.DeviceBuffer(total)
        if total > n1:
            dst.zero(n1, total - n1)
        if n1:
            N.check(L.sh_buf_copy(dst.handle, 0, self._device().handle, 0, n1))
        if n2:
            N.check(L.sh_pcm_add(dst.handle, start, other._device().handle, 0, n2, self.__samplewidth, dst.handle, start))
        self._set_device(dst, total)

    def mix_at_many(self, events: Iterable[tuple]) -> "Sample":
        """Mix a list of placed samples into this one: ``events`` holds ``(seconds, other, volume=None, other_seconds=None,
        speed=None, pan=None, envelope=None, loop=None, region=None, reverse=None, channels=None)``, and the result is, byte for byte, what ::

            for seconds, other, volume, other_seconds, speed, pan, envelope, loop, region, reverse, channels in events:
                o = other
                if region is not None:                  # (start, end) in seconds of other's own time; end may be None
                    o = other.copy().clip(region[0], other.duration if region[1] is None else region[1])
                if reverse:                             # audioop.reverse: the order of the SAMPLES, channels included
                    o = o.copy().reverse()
                if loop is not None:                    # a sustain loop: a note longer than its recording, in o's time
                    ls, le, length = loop               # seconds of o's own time, before speed
                    body = o.copy().clip(ls, le)
                    o = o.copy().clip(0.0, le)
                    while o.duration < length:
                        o.join(body)
                    o.clip(0.0, length)
                if speed is not None:
                    o = o.copy().speed(speed)           # audioop.ratecv(frames, width, nchannels, int(rate * speed), rate, None)
                if envelope is not None:
                    o = o.copy()
                    if len(envelope) == 5:
                        o.clip(0.0, envelope[4])        # the note's length, cut BEFORE the envelope: the release ends the note
                    o.envelope(*envelope[:4])           # on the (resampled, cut) frames, before tostereo
                if pan is not None:
                    o = o.copy().stereo(left, right)    # audioop.tostereo of the (resampled, shaped) MONO frames
                if channels is not None:                # a STEREO other, weighed per channel; never beside a pan
                    lf, rf = channels
                    if self.nchannels == 1:
                        o = o.copy().mono(lf, rf)       # audioop.tomono: floor(fbound(l * lf + r * rf))
                    else:
                        o = o.copy().stereo(lf, rf)     # (floor(fbound(L * lf)), floor(fbound(R * rf)))
                if volume is not None:
                    o = o.at_volume(volume)             # audioop.mul, after the resample, the envelope and tostereo
                self.mix_at(seconds, o, other_seconds)  # other_seconds cuts the resampled (stereo) sample

        leaves -- ``audioop.ratecv``, the cut, the envelope, ``audioop.tostereo`` and ``audioop.mul`` per event, in that order,
        ``audioop.add`` with saturation at every event, in list order, the track grown to the furthest end -- in one launch
        (sh_mix_events; sh_mix_events_rate when an event has a speed: a sampler, one recorded note at many pitches; sh_mix_events_pan
        when one has a pan: mono instruments placed in the stereo field of a stereo track, beside stereo ones; sh_mix_events_env when
        one has an envelope: shaped notes) and with at most one allocation (none when nothing grows).  ``envelope`` is ``(attack, decay,
        sustainlevel, release)`` or ``(attack, decay, sustainlevel, release, length)``, seconds and a factor 0 .. 1, with the bytes of
        ``Sample.envelope``: the sustain and release parts through ``audioop.mul`` (clamp, floor; not at all when the level is 1), the
        ramps ``int(x * f)`` (truncated) with ``f`` counting SAMPLES, so the two channels of a stereo frame get different factors and a
        panned event is ramped over its mono samples; the part boundaries are upstream's float arithmetic, replayed on the host.  Parts
        longer than the sample are what they are upstream (empty parts, an attack over the whole sample).  Its ValueErrors: a tuple
        that is not 4 or 5 long, a negative or non-finite attack, decay, release or length, a sustainlevel outside 0 .. 1, a release
        longer than what attack and decay leave of the sample (upstream slices from the wrong end then); 24-bit samples raise
        NotImplementedError (upstream's fades have no 24-bit form).  A speed
        of None or 1.0, or one with ``int(rate * speed) == rate``, is none.  ``pan`` is a float -1 .. 1, ``(left, right)`` =
        ``((1 - pan) / 2, (1 + pan) / 2)`` as ``Sample.pan`` has them, or the pair ``(left_factor, right_factor)`` of ``Sample.stereo``
        itself (a 0 on one side: ``stereo_mix``'s "into the left / right channel only"); it needs a mono ``other`` and a stereo track.
        A ValueError, raised before anything is mixed: negative times, non-finite volumes, a speed that is not finite or outside
        0.1 .. 10; a pan on a stereo ``other`` or into a track that is not stereo, a pan outside -1 .. 1, a pair of another length
        than two, a factor that is not finite.  A mono ``other`` without a pan in a stereo track fails the assertion of ``mix_at``.
        ``loop`` is ``(loop_start, loop_end, length)``: with ``S = int(rate * loop_start)``, ``E = min(int(rate * loop_end), frames)``
        and ``V = int(rate * length)`` the note has V virtual frames, frame v of ``other`` while ``v < E`` and frame ``S + (v - E) % (E -
        S)`` after it; ``ratecv`` runs over the virtual frames (across the seam), the envelope sees V frames, nothing is unrolled in
        memory, and a list with a loop goes to sh_mix_events_loop, still one launch.  ``V <= E`` is a plain cut.  24-bit samples may
        loop.  Its ValueErrors, raised before anything is mixed: not three numbers, one that is not finite or is negative, ``S >= E``,
        ``V`` times the channel count beyond what one call can address.  Where ``other`` is this sample, E is clamped to what the track
        holds when that event runs, so an empty loop there is found only then, after the events before it have been mixed.
        ``region`` plays a slice of ``other`` -- one hit out of a drum break, a recording without its attack -- with ``clip``'s
        arithmetic: frames ``[int(rate * start), int(rate * end))``, both clamped to the sample, nothing copied, no source slot per
        slice.  ``reverse``, taken by truth value, plays the (clipped) sound backwards as ``Sample.reverse`` does: ``audioop.reverse``
        turns the order of the SAMPLES round, so sample ``i`` of the reversed region is sample ``R - 1 - i`` of the region -- for a
        stereo ``other`` the frames come backwards AND left and right change places; a panned event's ``other`` is mono, so nothing
        is swapped there.  Both come FIRST: the loop's S, E and V count frames of the clipped, reversed sound and E is clamped to the
        region's frames, ``ratecv`` runs over these frames with its ``prev`` 0 at the region's first frame, the envelope sees what
        they resample to.  A list with regions goes where it went without them (``src_sample`` and ``src_frames`` say the slice); one
        reversed event and the list goes to sh_mix_events_rev, still one launch.  An empty region is an empty ``other``: nothing is
        mixed and the track grows to the event's start; with a loop it is the loop's "no frame between" ValueError.  The region's
        ValueErrors, raised before anything is mixed: not a pair, a start or end that is not finite or is negative, ``end < start``.
        Where ``other`` is this sample, the region is cut from the track as it is when that event runs, so an ``end`` of None (the
        track's duration then) that lies before ``start`` is found only then, after the events before it have been mixed.
        ``channels`` is the pair ``(left_factor, right_factor)`` for a STEREO ``other``, where ``pan``'s step stands: behind the envelope,
        in front of the volume.  In a mono track it is ``Sample.mono``: a stereo drum break or pad into a mono track, without a converted
        copy per pair of factors; ``(1.0, 0.0)`` is ``Sample.left()``.  In a stereo track it is ``Sample.stereo`` of a stereo sample, a
        balance; ``(1.0, 1.0)`` is the plain event.  Everything in front of it runs over the stereo sample as it does without it: region,
        reverse (left and right change places there, so ``left_factor`` then weighs what was recorded on the right), loop, ``ratecv``
        with two channels, the cut, the envelope, whose ramps count SAMPLES, so the two samples of a frame get different factors before
        they are summed.  Everything behind it counts what ``mix_at`` is handed: ``volume`` multiplies the mono or balanced samples, and
        ``other_seconds`` and the event's end count the track's samples.  All four widths (an envelope still has no 24-bit form).  One
        such event and the list goes to sh_mix_events_chan, still one launch, the rest as rows without a mode.  Its ValueErrors, raised
        before anything is mixed: not a pair, a factor that is not finite, an ``other`` that is not stereo, a track that is neither
        mono nor stereo, a ``pan`` on the same event, a downmix that ends more than 2^31 - 32768 samples into the track (the kernels
        address its stereo samples, two per track sample, in 32 bits).  Without ``channels`` a stereo ``other`` in a mono track fails
        the assertion of ``mix_at``, as before.
        An event whose ``other`` is this sample reads it as the events before it left it: the list is cut there, and that one event
        goes through the loop's body above, region, reverse and a balance included (a downmix cannot occur there)."""
        self._check_writable()
        self._check_gpu_width("mix_at")
        batch = []                                                              # the events since the last one whose other is this sample
        for e in self._check_events(events):
            if e.other is not self:
                batch.append(e)
                continue
            self.__mix_events(batch)                                            # it reads the track as the events before it left it
            batch = []
            other = e.other                                                     # (never panned: a panned event's other is mono, its track stereo)
            if e.own_region is not None:                                        # copy().clip() of the track as it is NOW
                first, end = e.own_region
                if end is None:
                    end = other.duration
                if end < first:
                    raise ValueError("mix_at_many: region: end (%r s: the track as the events before left it) lies before start (%r s)"
                                     % (end, first))
                other = other.copy().clip(first, end)
            if e.reverse:
                other = other.copy().reverse()
            if e.loop is not None:                                              # clip(0.0, loop_end) of the track (its region, reversed) as it is NOW
                first, last = e.loop[0], min(e.loop[0] + e.loop[1], len(other))
                if first >= last:
                    raise ValueError("mix_at_many: loop: no frame between loop_start (frame %d) and loop_end (frame %d) of the track "
                                     "as the events before left it" % (first, last))
                other = other.__unrolled(first, last - first, e.loop[2])
            if e.inrate != self.__samplerate:
                other = other.copy().speed(e.speed)
            if e.envelope is not None:
                other = other.copy()
                if len(e.envelope) == 5:
                    other.clip(0.0, e.envelope[4])
                other.envelope(*e.envelope[:4])
            if e.weights is not None:                                           # (the track is stereo here: a balance)
                other = other.copy().stereo(*e.weights)
            self.mix_at(e.seconds, other if e.volume is None else other.at_volume(e.volume), e.other_seconds)
        self.__mix_events(batch)
        return self

    def _check_events(self, events: Iterable[tuple]) -> list:
        """Every event of a list for mix_at_many checked against this track's format, before anything is mixed or reaches the device: one
        _Event each.  The one statement of mix_at_many's ValueErrors (Sample.mix_at_many, mixer.compile_sequence and mixer.compile_tracks
        all go through it); the order of the checks is the order in which an event's faults are reported."""
        w, nch, rate = self.__samplewidth, self.__nchannels, self.__samplerate
        fb = w * nch
        checked = []                                        # everything is checked before anything is mixed
        for ev in events:
            seconds, other, volume, other_seconds, speed, pan, envelope, loop, region, reverse, channels = (*ev, *_NO_MORE)[:11]
            reverse = bool(reverse)
            assert self.samplewidth == other.samplewidth
            assert self.samplerate == other.samplerate
            weights = None
            if channels is not None:
                if pan is not None:
                    raise ValueError("mix_at_many: pan and channels on one event: pan places a mono sample, channels weighs a stereo one")
                weights = _channel_weights(channels, other.nchannels, nch)
            elif pan is None:
                assert self.nchannels == other.nchannels
            else:
                pan = _pan_factors(pan, other.nchannels, nch)
            if seconds < 0 or (other_seconds is not None and other_seconds < 0):
                raise ValueError("mix_at_many: negative time")
            if volume is not None and not math.isfinite(volume):
                raise ValueError("mix_at_many: volume is not finite")
            inrate = rate
            if speed is not None and speed != 1.0:
                if not math.isfinite(speed) or speed < 0.1 or speed > 10.0:
                    raise ValueError("mix_at_many: speed must be between 0.1 and 10")
                inrate = int(rate * speed)                                      # Sample.speed: Python floats, on the host
                if inrate <= 0:
                    raise ValueError("mix_at_many: speed %r leaves no sample rate" % (speed,))
            start = fb * int(rate * seconds)                                    # frame_idx(seconds): Python floats, on the host
            frames = other.__nbytes // (w * other.nchannels)                    # (a panned event: the mono frames, a track frame each)
            own = other is self                                                 # the track as its own source: cut and clamped when the event runs
            own_region = None
            if region is not None:                                              # the event has the region's frames from here on
                cut = _region_frames(region, rate, None if own else frames, other.duration)
                if own:
                    own_region, region = region, None
                else:
                    region, frames = cut, cut[1]
            if loop is not None:                                                # the note has V frames from here on
                loop = _loop_frames(loop, rate, None if own else frames, other.nchannels)
                frames = loop[2]
            if inrate != rate:
                frames = _ratecv_out_frames(frames, inrate, rate)
            segments = None
            if envelope is not None:
                frames, segments = _envelope_rows(envelope, frames, w, other.nchannels, rate)
            have = fb * frames                                                  # a frame of other (resampled, shaped) is a frame of the track
            n2 = min(fb * int(rate * other_seconds), have) if other_seconds else have      # frame_idx(other_seconds) of what mix_at is handed
            if weights is not None and nch == 1 and 2 * ((start + n2) // w) > _MAX_DOWNMIX_SOURCE_SAMPLES:
                raise ValueError("mix_at_many: channels: a downmix ends at most %d samples into the track (its stereo samples are addressed "
                                 "in 32 bits)" % (_MAX_DOWNMIX_SOURCE_SAMPLES // 2))
            level = (N.LEVEL_CHAN if weights is not None else N.LEVEL_REV if reverse else N.LEVEL_LOOP if loop is not None else
                     N.LEVEL_ENV if segments is not None else N.LEVEL_PAN if pan is not None else N.LEVEL_RATE if inrate != rate else N.LEVEL_PLAIN)
            checked.append(_new_event(_Event, (seconds, other, volume, other_seconds, speed, start, n2, inrate, pan, loop, region, reverse, weights,
                                               envelope, segments, level, own_region)))
        return checked

    def _compile_events(self, events: Iterable[tuple]) -> tuple:
        """What mixer.compile_sequence hands sh_seq_create, this sample being the empty track that says the format: mix_at_many's checks,
        then (the sources' device buffers, shared; the table in sh_mix_event_chan's layout; the segment table; the song's bytes)."""
        self._check_gpu_width("mix_at")
        return self._compile_checked(self._check_events(events))

    def _compile_checked(self, checked: list) -> tuple:
        """_compile_events behind its checks (mixer.compile_tracks checks track by track and hands the tracks' events on as one list, one
        row per event)."""
        if not checked:
            return [], np.zeros(0, dtype=N.MIX_LEVELS[N.LEVEL_CHAN].dtype), None, 0
        bufs, table, segtab, _level = self._pack_events(checked, widest=True, share=True)
        return bufs, table, segtab, max(e.start + e.nbytes for e in checked)

    def __unrolled(self, loop_start: int, loop_frames: int, nframes: int) -> "Sample":
        """A copy with the loop written out: frames [0, loop_start + loop_frames), then frames [loop_start, loop_start + loop_frames)
        again and again, ``nframes`` in all -- what a looped event of mix_at_many plays, for the one whose source is the track itself."""
        fb = self.__samplewidth * self.__nchannels
        head, body, total = (loop_start + loop_frames) * fb, loop_frames * fb, nframes * fb
        parts = [(self, 0, min(head, total))]
        at = head
        while at < total:
            parts.append((self, loop_start * fb, min(body, total - at)))
            at += body
        out = Sample(name=self.name, samplerate=self.__samplerate, nchannels=self.__nchannels, samplewidth=self.__samplewidth)
        out.__assemble(parts)
        return out

    def _pack_events(self, batch: Sequence[_Event], widest: bool = False, share: bool = False) -> tuple:
        """Checked events as the table an entry point reads, packed column by column (whole-array numpy operations, not a row per event):
        (the sources' device buffers, the table, the segment table | None, the level).  The level is the highest of the rows' levels and
        the table has that rung's layout, the narrowest that holds the list; ``widest``: the top rung, whatever the list holds
        (sh_seq_create takes that one layout and finds the level itself).  A column group is filled from the rung up that first has it.
        ``share``: the sources' buffers are taken with _share_device, for a reader that keeps them."""
        col = dict(zip(_Event._fields, zip(*batch)))         # the records' fields as columns
        w, nch, rate = self.__samplewidth, self.__nchannels, self.__samplerate
        level = N.LEVEL_CHAN if widest else max(col["level"])
        others, pans, weights = col["other"], col["pan"], col["weights"]
        nbytes = np.array(col["nbytes"], dtype=np.uint64)
        slot = {}                                           # id(other) -> (index into srcs, other): one dict lookup per event, no more
        for o in others:
            slot.setdefault(id(o), (len(slot), o))
        uniq = [o for _k, o in slot.values()]
        bufs = [o._share_device() if share else o._device() for o in uniq]
        src = np.fromiter((slot[id(o)][0] for o in others), dtype=np.uint32, count=len(others))
        table = np.zeros(len(batch), dtype=N.MIX_LEVELS[level].dtype)
        table["dst_sample"] = np.array(col["start"], dtype=np.uint64) // w
        table["nsamples"] = nbytes // w
        table["factor"] = [1.0 if v is None else float(v) for v in col["volume"]]
        table["src"] = src
        if level >= N.LEVEL_RATE:
            frames = np.array([o.__nbytes // (w * o.nchannels) for o in uniq], dtype=np.uint64)
            table["src_frames"] = frames[src]
            table["inrate"] = np.array(col["inrate"], dtype=np.uint64)
            table["outrate"] = rate
        if level >= N.LEVEL_PAN:
            table["src_channels"] = np.array([o.nchannels for o in uniq], dtype=np.uint32)[src]
            lr = np.array([p if p is not None else (0.0, 0.0) for p in pans], dtype=np.float64)
            table["left"] = lr[:, 0]
            table["right"] = lr[:, 1]
        regions = col["region"]
        if regions.count(None) != len(regions):             # a slice of other: where it starts, and the frames every count above was made over
            at = [i for i, rg in enumerate(regions) if rg is not None]
            src_nch = np.array([o.nchannels for o in uniq], dtype=np.uint64)[src]
            rg = np.array([regions[i] for i in at], dtype=np.uint64)
            table["src_sample"][at] = rg[:, 0] * src_nch[at]
            if level >= N.LEVEL_RATE:
                table["src_frames"][at] = rg[:, 1]
        if level >= N.LEVEL_LOOP:                           # (a row without a loop: loop_frames == 0)
            lp = np.array([l if l is not None else (0, 0, 0) for l in col["loop"]], dtype=np.uint64)
            table["loop_start"] = lp[:, 0]
            table["loop_frames"] = lp[:, 1]
        if level >= N.LEVEL_REV:                            # a reversed row names its region as stored, forwards -- a looped one the part of
            rv = np.flatnonzero(col["reverse"])             # it in front of the loop's end, which is all it plays: its region starts there
            table["flags"][rv] = N.MIX_EVENT_REVERSED
            back = rv[lp[rv, 1] != 0]
            table["src_sample"][back] += (table["src_frames"][back] - lp[back, 0] - lp[back, 1]) * table["src_channels"][back]
        if level >= N.LEVEL_CHAN:                           # a stereo source weighed per channel: tomono into a mono track, a balance in a stereo one
            for i, lf_rf in enumerate(weights):
                if lf_rf is not None:
                    table["flags"][i] |= N.MIX_EVENT_DOWNMIX if nch == 1 else N.MIX_EVENT_BALANCE
                    table["left"][i], table["right"][i] = lf_rf
        if level >= N.LEVEL_LOOP:
            table["src_frames"] = np.where(lp[:, 1] != 0, lp[:, 2], table["src_frames"])      # a looped row: the note's virtual frames
        segtab = None
        if level >= N.LEVEL_ENV:                            # the envelopes' rows, cut here where the event is
            rows = []
            for i, g in enumerate(col["segments"]):
                if g is None:
                    continue
                taken = int(nbytes[i]) // w // (2 if pans[i] is not None else 1)       # the event's source samples, after other_seconds' cut
                if weights[i] is not None and nch == 1:
                    taken *= 2                                                          # (a downmix: two stereo samples per track sample)
                mine = [(min(r[0], taken),) + r[1:] for r in g]
                mine = [r for k, r in enumerate(mine) if r[0] > (mine[k - 1][0] if k else 0)]      # (what the cut leaves nothing of)
                table["seg_first"][i] = len(rows)
                table["seg_count"][i] = len(mine)
                rows.extend(mine)
            segtab = np.zeros(len(rows), dtype=N.ENV_SEGMENT_DTYPE)
            for name, column in zip(("end", "mul", "kind", "slope", "numsamples", "offset", "origin"), zip(*rows) if rows else [()] * 7):
                segtab[name] = column
        return bufs, table, segtab, level

    def __mix_events(self, batch: Sequence[_Event]) -> None:
        """Checked events -- none of them this sample's own -- folded in order, in one launch; length -> the furthest end."""
        if not batch:
            return
        w = self.__samplewidth
        n1 = self.__nbytes
        total = max(n1, max(e.start + e.nbytes for e in batch))                 # the furthest end
        if total == 0:
            return
        if total == n1 and self._device().nbytes >= n1 and not self.__dev_shared:
            track = self.__dev                              # in place, under __mix_region's conditions
        else:
            track = N.DeviceBuffer(total)
            if total > n1:
                track.zero(n1, total - n1)
            if n1:
                N.check(N.lib().sh_buf_copy(track.handle, 0, self._device().handle, 0, n1))
        bufs, table, segtab, level = self._pack_events(batch)
        rung = N.MIX_LEVELS[level]
        args = [(C.c_void_p * len(bufs))(*[b.handle for b in bufs]), len(bufs), table.ctypes.data, len(table)]
        if rung.segments:
            args += [segtab.ctypes.data, len(segtab)]
        args.append(w)
        if rung.nchannels:
            args.append(self.__nchannels)
        N.check(getattr(N.lib(), rung.entry)(*args, track.handle, total // w))
        self._set_device(track, total)                      # (in place: drops the host copy, it is stale now)

    # -- elementwise operations (upstream: thin wrappers over audioop) ---------------------------------
    def __unary(self, fn_name: str, out_nbytes: int, *args) -> "Sample":
        """frames = op(frames): run sh_<fn_name>(in, ..., out) into a fresh device buffer."""
        dst = N.DeviceBuffer(out_nbytes)
        N.check(getattr(N.lib(), fn_name)(self._device().handle, *args, dst.handle))
        self._set_device(dst, out_nbytes)
        return self

    def amplify(self, factor: float) -> "Sample":
        """Amplify (or attenuate, or with a negative factor invert) the sample: audioop.mul."""
        self._check_writable()
        self._check_gpu_width("amplify")
        n = self.__nbytes
        dst = N.DeviceBuffer(n)
        N.check(N.lib().sh_pcm_mul(self._device().handle, 0, n, self.__samplewidth, float(factor), dst.handle, 0))
        self._set_device(dst, n)
        return self

    def convolve(self, ir: "Sample", factor: Optional[float] = None, tail: bool = True) -> "Sample":
        """Run the sample through the impulse response ``ir`` (a room, a plate, a cabinet, any FIR filter), in place and exact:
        ``mixer.convolve(self, ir, factor)``'s bytes.  ``factor`` None: ``1 / 2 ** (8 * samplewidth - 1)``.  ``tail=True`` keeps the
        ``len(ir) - 1`` frames that ring on behind the sample's end, ``tail=False`` the first ``len(self)`` frames.  Widths 1 and 2."""
        self._check_writable()
        self._check_gpu_width("convolve")
        from .mixer import convolve                             # (lazily: mixer imports this module)
        out = convolve(self, ir, factor, 0, None if tail else len(self))
        if len(out):
            self._set_device(out._device(), len(out) * self.__nchannels * self.__samplewidth)
        else:
            self._set_host(b"")
        return self

    def limit(self, ceiling: Optional[int] = None, attack: float = 0.005, release: float = 0.2, ceiling_db: Optional[float] = None) -> "Sample":
        """A look-ahead peak limiter -- a brick wall -- over the sample, in place in HBM and exact in integers:
        ``mixer.limit(self, ceiling, attack_frames, release_frames)``'s bytes.  No sample of the result exceeds the ceiling in magnitude;
        the gain comes down on a linear ramp over ``attack`` seconds in front of a peak and back up over ``release`` seconds behind it,
        one gain for both channels; frames that need no reduction are untouched.  Seconds become frames by
        ``int(seconds * samplerate + 0.5)``.  Exactly one of ``ceiling`` (an int, in sample steps) and ``ceiling_db`` (at most 0, relative
        to full scale: ``int(HI * 10 ** (ceiling_db / 20))``) is given.  Widths 1, 2 and 4."""
        self._check_writable()
        if self.__samplewidth == 3:
            raise NotImplementedError("limit: 3-byte samples are not built")
        if (ceiling is None) == (ceiling_db is None):
            raise ValueError("limit: exactly one of ceiling and ceiling_db is given")
        if ceiling is None:
            if isinstance(ceiling_db, bool) or not isinstance(ceiling_db, (int, float, np.integer, np.floating)) or not ceiling_db <= 0:
                raise ValueError("limit: ceiling_db is a number of at most 0, not %r" % (ceiling_db,))
            ceiling = int((2 ** (8 * self.__samplewidth - 1) - 1) * 10.0 ** (float(ceiling_db) / 20.0))
        frames = []
        for name, seconds in (("attack", attack), ("release", release)):
            if isinstance(seconds, bool) or not isinstance(seconds, (int, float, np.integer, np.floating)) or not 0 <= seconds < float("inf"):
                raise ValueError("limit: %s is a non-negative number of seconds, not %r" % (name, seconds))
            frames.append(int(seconds * self.__samplerate + 0.5))
        from .mixer import limit, limit_into, _limit_call       # (lazily: mixer imports this module)
        _limit_call("limit", self, ceiling, frames[0], frames[1], 0, None)
        n = self.__nbytes
        if not n:
            return self
        if self._device().nbytes >= n and not self.__dev_shared:
            # in place: the kernel reads a tile's frames before it writes them and no others (csrc/pcm_limit.hip), and a Sample's
            # device buffer is its own -- under mix's conditions (one that a mixer streams from takes the copying form below)
            limit_into(self.__dev, 0, self, ceiling, frames[0], frames[1])
            self._set_device(self.__dev, n)                     # (drops the host copy: it is stale now)
        else:
            self._set_device(limit(self, ceiling, frames[0], frames[1])._device(), n)
        return self

    def peak(self) -> int:
        """Maximum absolute sample value (audioop.max)."""
        self._check_gpu_width("peak")
        mx = C.c_uint32()
        N.check(N.lib().sh_pcm_stats(self._device().handle, self.__nbytes, self.__samplewidth, C.byref(mx), None))
        return int(mx.value)

    def rms(self) -> int:
        """Root mean square of the samples, truncated (audioop.rms)."""
        self._check_gpu_width("rms")
        n = self.__nbytes // self.__samplewidth
        if n == 0:
            return 0
        sq = C.c_double()
        N.check(N.lib().sh_pcm_stats(self._device().handle, self.__nbytes, self.__samplewidth, None, C.byref(sq)))
        from math import sqrt
        return int(sqrt(sq.value / float(n)))

    def level_history(self, block_frames: int, origin_frame: int = 0):
        """The levels over time, per block of ``block_frames`` frames, in one launch: ``mixer.level_history(self, ...)``'s ``SongHistory``
        (one row per block, ``history[j].master``; exact integer sums at every width)."""
        from .mixer import level_history                        # (lazily: mixer imports this module)
        return level_history(self, block_frames, origin_frame)

    def waveform(self, block_frames: int, origin_frame: int = 0):
        """The waveform extremes over time, per block of ``block_frames`` frames, in one launch, for drawing: ``mixer.waveform(self,
        ...)``'s ``Waveform`` (per block and channel the smallest and the largest sample, ``audioop.minmax``, at every width)."""
        from .mixer import waveform                             # (lazily: mixer imports this module)
        return waveform(self, block_frames, origin_frame)

    def _channel_stats(self) -> Tuple[Tuple[int, int], Tuple[float, float]]:
        """((max|L|, max|R|), (sum L^2, sum R^2)) of a stereo sample, one pass on the device."""
        mx = (C.c_uint32 * 2)()
        sq = (C.c_double * 2)()
        N.check(N.lib().sh_pcm_stats_stereo(self._device().handle, len(self), self.__samplewidth, mx, sq))
        return (int(mx[0]), int(mx[1])), (float(sq[0]), float(sq[1]))

    def __db_level(self, rms_mode: bool) -> Tuple[float, float]:
        self._check_gpu_width("level_db")
        maxvalue = 2 ** (8 * self.__samplewidth - 1)
        if self.__nchannels == 1:
            left = right = ((self.rms() if rms_mode else self.peak()) + 1) / maxvalue
        elif self.__nchannels == 2:
            (ml, mr), (sl, sr) = self._channel_stats()
            if rms_mode:
                n = len(self)
                ml, mr = (int(math.sqrt(sl / float(n))), int(math.sqrt(sr / float(n)))) if n else (0, 0)
            left, right = (ml + 1) / maxvalue, (mr + 1) / maxvalue
        else:
            raise ValueError("level metering needs a mono or stereo sample")
        # cut off at -60 dB instead of running down to -infinity
        return max(20.0 * math.log(left, 10), -60.0), max(20.0 * math.log(right, 10), -60.0)

    def __db_level_mono(self, rms_mode: bool) -> float:
        self._check_gpu_width("level_db")
        maxvalue = 2 ** (8 * self.__samplewidth - 1)
        level = ((self.rms() if rms_mode else self.peak()) + 1) / maxvalue
        return max(20.0 * math.log(level, 10), -60.0)

    @property
    def level_db_peak(self) -> Tuple[float, float]:
        """Peak level in dB (0 = full scale) of the (left, right) channel, not lower than -60."""
        return self.__db_level(False)

    @property
    def level_db_rms(self) -> Tuple[float, float]:
        """RMS level in dB of the (left, right) channel, not lower than -60."""
        return self.__db_level(True)

    @property
    def level_db_peak_mono(self) -> float:
        return self.__db_level_mono(False)

    @property
    def level_db_rms_mono(self) -> float:
        return self.__db_level_mono(True)

    def amplify_max(self) -> "Sample":
        """Amplify to the maximum volume without clipping."""
        self._check_writable()
        max_amp = self.peak()
        max_target = 2 ** (8 * self.__samplewidth - 1) - 2
        if max_amp > 0:
            self.amplify(max_target / max_amp)
        return self

    def invert(self) -> "Sample":
        return self.amplify(-1)

    def bias(self, bias: int) -> "Sample":
        """Add a constant to every sample (wrapping, like audioop.bias)."""
        self._check_writable()
        self._check_gpu_width("bias")
        return self.__unary("sh_pcm_bias", self.__nbytes, self.__nbytes, self.__samplewidth, int(bias))

    def reverse(self) -> "Sample":
        """Reverse the sound (audioop.reverse: the order of the samples, channels included)."""
        self._check_writable()
        self._check_gpu_width("reverse")
        return self.__unary("sh_pcm_reverse", self.__nbytes, self.__nbytes, self.__samplewidth)

    def mono(self, left_factor: float = 1.0, right_factor: float = 1.0) -> "Sample":
        """Stereo -> mono with per-channel factors (audioop.tomono)."""
        self._check_writable()
        if self.__nchannels == 1:
            return self
        if self.__nchannels != 2:
            raise ValueError("sample must be stereo or mono already")
        self._check_gpu_width("mono")
        nframes = len(self)
        self.__unary("sh_pcm_tomono", nframes * self.__samplewidth, nframes, self.__samplewidth, float(left_factor), float(right_factor))
        self.__nchannels = 1
        return self

    def left(self) -> "Sample":
        return self.mono(1.0, 0)

    def right(self) -> "Sample":
        return self.mono(0, 1.0)

    def stereo(self, left_factor: float = 1.0, right_factor: float = 1.0) -> "Sample":
        """Mono -> stereo with per-channel factors (audioop.tostereo); a stereo sample gets its channels scaled."""
        self._check_writable()
        self._check_gpu_width("stereo")
        if self.__nchannels == 2:
            # upstream: left().amplify(lf) mixed with right().amplify(rf) -> (fbound(L*lf), fbound(R*rf))
            right = self.copy().right().amplify(right_factor).stereo(0, 1.0)
            self.left().amplify(left_factor).stereo(1.0, 0)
            return self.mix(right)
        if self.__nchannels != 1:
            raise ValueError("sample must be mono or stereo already")
        nframes = len(self)
        self.__unary("sh_pcm_tostereo", nframes * 2 * self.__samplewidth, nframes, self.__samplewidth, float(left_factor), float(right_factor))
        self.__nchannels = 2
        return self

    def stereo_mix(self, other: "Sample", other_channel: str, other_mix_factor: float = 1.0, mix_at: float = 0.0,
                   other_seconds: Optional[float] = None) -> "Sample":
        """Mix a mono sample into the left ("L") or right ("R") channel of this one, scaled by ``other_mix_factor``,
        starting at ``mix_at`` seconds.  A mono self first becomes the opposite channel of a stereo sample."""
        self._check_writable()
        assert other.nchannels == 1
        assert other.samplerate == self.__samplerate
        assert other.samplewidth == self.__samplewidth
        assert other_channel in ("L", "R")
        if self.__nchannels == 1:
            if other_channel == "L":
                self.stereo(left_factor=0, right_factor=1)
            else:
                self.stereo(left_factor=1, right_factor=0)
        other = other.copy()
        if other_channel == "L":
            other.stereo(left_factor=other_mix_factor, right_factor=0)
        else:
            other.stereo(left_factor=0, right_factor=other_mix_factor)
        return self.mix_at(mix_at, other, other_seconds)

    def pan(self, panning: float = 0.0, lfo=None) -> "Sample":
        """Linear stereo panning, -1.0 (left) .. 1.0 (right); the sample becomes stereo.  With an ``lfo`` (an
        oscillator, or any iterable of floats: one value per frame) the position follows it instead: the left side of
        frame i becomes int(l * (1 - p) / 2), the right side int(r * (1 + p) / 2)."""
        if lfo is None:
            assert -1.0 <= panning <= 1.0
            left_volume = (1.0 - panning) / 2.0
            right_volume = (1.0 + panning) / 2.0
            return self.stereo(left_volume, right_volume)     # a stereo source keeps its channels apart, like the lfo form
        self._check_writable()
        self._check_gpu_width("pan")
        if self.__nchannels not in (1, 2):
            raise ValueError("pan needs a mono or stereo sample")
        n = len(self)
        from .oscillators import Oscillator
        if isinstance(lfo, Oscillator):
            mod = lfo._render_f64_device(0, n) if n else N.DeviceBuffer(0)
        else:
            import itertools
            values = np.fromiter(itertools.islice(iter(lfo), n), dtype=np.float64)
            if len(values) < n:
                raise ValueError("pan lfo ran out after %d of %d frames" % (len(values), n))
            mod = N.DeviceBuffer(n * 8)
            if n:
                mod.upload(values)
        nbytes = n * 2 * self.__samplewidth
        dst = N.DeviceBuffer(nbytes)
        N.check(N.lib().sh_pcm_pan_lfo(self._device().handle, n, self.__samplewidth, self.__nchannels, mod.handle, dst.handle))
        self.__nchannels = 2
        self._set_device(dst, nbytes)
        return self

    def __lin2lin(self, new_width: int) -> None:
        n = self.__nbytes // self.__samplewidth
        self.__unary("sh_pcm_lin2lin", n * new_width, n, self.__samplewidth, new_width)
        self.__samplewidth = new_width

    def normalize(self) -> "Sample":
        """Bring the sample to the default rate, width and channel count (params.norm_*)."""
        self._check_writable()
        self._check_gpu_width("normalize")
        self.resample(params.norm_samplerate)
        if self.__samplewidth != params.norm_samplewidth:
            self.__lin2lin(params.norm_samplewidth)
        if self.__nchannels == 1 and params.norm_nchannels == 2:
            self.stereo(1, 1)
        return self

    def make_32bit(self, scale_amplitude: bool = True) -> "Sample":
        """Convert to 32-bit samples; without scaling the integer values are kept as they were."""
        self._check_writable()
        self._check_gpu_width("make_32bit")
        old = self.__samplewidth
        if old != 4:
            self.__lin2lin(4)
            if not scale_amplitude:
                self.amplify(1.0 / 2 ** (8 * (4 - old)))
        return self

    def make_16bit(self, maximize_amplitude: bool = True) -> "Sample":
        """Convert to 16-bit samples, optionally maximising the amplitude first."""
        self._check_writable()
        self._check_gpu_width("make_16bit")
        assert self.__samplewidth >= 2
        if maximize_amplitude:
            self.amplify_max()
        if self.__samplewidth > 2:
            self.__lin2lin(2)
        return self

    def __fade(self, first_byte: int, nbytes: int, fadeout: bool, slope: float, offset: float) -> None:
        n = self.__nbytes
        dst = N.DeviceBuffer(n)
        L = N.lib()
        if n:
            N.check(L.sh_buf_copy(dst.handle, 0, self._device().handle, 0, n))
        if nbytes:
            N.check(L.sh_pcm_fade(self._device().handle, first_byte, nbytes, self.__samplewidth, 1 if fadeout else 0,
                                  float(slope), float(offset), dst.handle, first_byte))
        self._set_device(dst, n)

    def fadeout(self, seconds: float, target_volume: float = 0.0) -> "Sample":
        """Fade the end of the sample out to the target volume: int(sample_i * (1 - i*decrease/numsamples))."""
        self._check_writable()
        self._check_gpu_width("fadeout")
        seconds = min(seconds, self.duration)
        i = self.frame_idx(self.duration - seconds)
        self.__fade(i, self.__nbytes - i, True, 1.0 - target_volume, 0.0)
        return self

    def fadein(self, seconds: float, start_volume: float = 0.0) -> "Sample":
        """Fade the start of the sample in from the start volume: int(sample_i * (i*increase/numsamples + start))."""
        self._check_writable()
        self._check_gpu_width("fadein")
        seconds = min(seconds, self.duration)
        i = self.frame_idx(seconds)
        self.__fade(0, i, False, 1.0 - start_volume, start_volume)
        return self

    def resample(self, samplerate: int) -> "Sample":
        """Resample to a different rate without changing pitch/duration: linear interpolation with
        the arithmetic of ``audioop.ratecv(frames, width, nchannels, rate, samplerate, None)``."""
        self._check_writable()
        if samplerate == self.__samplerate:
            return self
        self._check_gpu_width("resample")
        L = N.lib()
        nin = len(self)
        nout = L.sh_resample_out_frames(nin, self.__samplerate, samplerate)
        fb = self.__samplewidth * self.__nchannels
        dst = N.DeviceBuffer(nout * fb)
        out_frames = C.c_size_t()
        if nin:
            N.check(L.sh_resample(self._device().handle, nin, self.__nchannels, self.__samplewidth, 0,
                                  self.__samplerate, samplerate, dst.handle, C.byref(out_frames)))
        self._set_device(dst, nout * fb)
        self.__samplerate = samplerate
        return self

    def resample_fir(self, samplerate: int, taps=None, factor: Optional[float] = None, delay: Optional[int] = None) -> "Sample":
        """Resample to a different rate through a band-limited polyphase FIR, in place and exact: ``mixer.resample_fir(self, samplerate,
        taps, factor, delay)``'s bytes (``taps`` None: ``mixer.lowpass_taps`` of the ratio, a Kaiser-windowed sinc).  No tone above the
        new Nyquist frequency folds back and the top of the band keeps its level, which ``resample`` -- ``audioop.ratecv``'s linear
        interpolation, byte for byte -- does not promise.  The same rate with ``taps`` None leaves the sample as it is.  Widths 1 and 2."""
        self._check_writable()
        if samplerate == self.__samplerate and taps is None:
            return self
        from .mixer import resample_fir                         # (lazily: mixer imports this module; it refuses widths 3 and 4)
        out = resample_fir(self, samplerate, taps, factor, delay)
        if len(out):
            self._set_device(out._device(), len(out) * self.__nchannels * self.__samplewidth)
        else:
            self._set_host(b"")
        self.__samplerate = int(samplerate)
        return self


class LevelMeter:
    """Sound level tracker on the decibel scale (0 dB = full scale) with peak hold: a peak stays for 0.4 s of audio,
    then falls by 30 dB per second until the level catches up.  ``update`` takes one chunk; the real-time mixer feeds
    it every mixed chunk.  (Upstream ``synthplayer/sample.py`` class ``LevelMeter``, [RECALL], tree not mounted.)"""

    def __init__(self, rms_mode: bool = False, lowest: float = -60.0) -> None:
        assert -60.0 <= lowest < 0.0
        self._rms = rms_mode
        self._lowest = lowest
        self.reset()

    def reset(self) -> None:
        self.peak_left = self.peak_right = self._lowest
        self._peak_left_hold = self._peak_right_hold = 0.0
        self.level_left = self.level_right = self._lowest
        self._time = 0.0

    def update(self, sample: Sample) -> Tuple[float, float, float, float]:
        """Feed one chunk; returns (level left, peak left, level right, peak right)."""
        left, right = sample.level_db_rms if self._rms else sample.level_db_peak
        left = max(left, self._lowest)
        right = max(right, self._lowest)
        time = self._time + sample.duration
        if (time - self._peak_left_hold) > 0.4:
            self.peak_left -= sample.duration * 30.0
        if left >= self.peak_left:
            self.peak_left = left
            self._peak_left_hold = time
        if (time - self._peak_right_hold) > 0.4:
            self.peak_right -= sample.duration * 30.0
        if right >= self.peak_right:
            self.peak_right = right
            self._peak_right_hold = time
        self.level_left = left
        self.level_right = right
        self._time = time
        return left, self.peak_left, right, self.peak_right

    def print(self, bar_width: int = 60, stereo: bool = False) -> None:
        """One line of text bars for the current levels (carriage return, no newline)."""
        def bar(level: float, peak: float, width: int) -> str:
            filled = int(width * (level - self._lowest) / -self._lowest)
            mark = min(width - 1, max(0, int(width * (peak - self._lowest) / -self._lowest)))
            cells = ["#"] * filled + ["-"] * (width - filled)
            cells[mark] = ":"
            return "".join(cells)
        if stereo:
            half = bar_width // 2
            print(" %s| L-R |%s" % (bar(self.level_left, self.peak_left, half)[::-1], bar(self.level_right, self.peak_right, half)), end="\r")
        else:
            level, peak = (self.level_left + self.level_right) / 2, (self.peak_left + self.peak_right) / 2
            print(" %d dB |%s| 0 dB" % (int(self._lowest), bar(level, peak, bar_width)), end="\r")
