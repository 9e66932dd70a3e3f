"""ctypes binding of libsynthhip.so (include/synthhip.h).

There is no CPU fallback: every arithmetic entry point of this package goes through the HIP
library.  If the shared object is missing or no GPU is visible the calls raise -- loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import NamedTuple, Optional

import numpy as np

HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("SYNTHHIP_LIB", HERE / "libsynthhip.so"))

SH_OK = 0
SH_ERR_INVALID, SH_ERR_HIP, SH_ERR_NOMEM, SH_ERR_NOTINIT, SH_ERR_OVERFLOW, SH_ERR_RCCL, SH_ERR_LENGTH = -1, -2, -3, -4, -5, -6, -7
SH_SINE, SH_SAWTOOTH, SH_SQUARE, SH_PULSE, SH_HARMONICS, SH_TRIANGLE, SH_LINEAR, SH_NOISE, SH_BUFFER = range(9)
SH_EW_ADD, SH_EW_MUL, SH_EW_CLIP, SH_EW_ABS, SH_EW_COPY, SH_EW_FILL, SH_EW_AXPY, SH_EW_NEXTUP = range(8)
SH_OPT_QUANTISE_ROUND = 1
SH_INFO_LAST_MIXDOWN_FUSED = 2
SH_FM_NONE, SH_FM_SINE, SH_FM_BUFFER = range(3)
SH_DIST_ID_BYTES = 128


class SynthHipError(RuntimeError):
    def __init__(self, code: int, message: str) -> None:
        super().__init__("libsynthhip error %d: %s" % (code, message))
        self.code = code


class NativeLibraryMissing(ImportError):
    pass


# numpy structured dtypes that mirror the C structs byte for byte (align=True = C layout)
SEGMENT_DTYPE = np.dtype([("n0", "<u8"), ("t0", "<f8"), ("dt", "<f8")], align=True)
PARTIAL_DTYPE = np.dtype([("k", "<f8"), ("amp", "<f8")], align=True)
ENVELOPE_DTYPE = np.dtype([
    ("n_attack_end", "<u8"), ("n_decay_end", "<u8"), ("n_sustain_end", "<u8"), ("n_release_end", "<u8"),
    ("attack_slope", "<f8"), ("decay_slope", "<f8"), ("sustain_level", "<f8"), ("release_slope", "<f8"),
    ("tail_amp", "<f8"), ("enabled", "<i4"), ("has_tail", "<i4")], align=True)
VOICE_DTYPE = np.dtype([
    ("kind", "<i4"), ("fm_mode", "<i4"),
    ("amplitude", "<f8"), ("bias", "<f8"), ("pulsewidth", "<f8"),
    ("seg_offset", "<u4"), ("seg_count", "<u4"),
    ("harm_offset", "<u4"), ("harm_count", "<u4"), ("harm_dense", "<i4"), ("flip", "<i4"),
    ("frequency", "<f8"), ("fm_phase0", "<f8"), ("fm_inc", "<f8"),
    ("time_seg_offset", "<u4"), ("time_seg_count", "<u4"),
    ("lfo_a", "<f8"), ("lfo_d", "<f8"), ("lfo_amp", "<f8"), ("lfo_bias", "<f8"), ("lfo_K", "<f8"), ("lfo_C0", "<f8"),
    ("env", ENVELOPE_DTYPE),
    ("gain_l", "<f4"), ("gain_r", "<f4"),
    ("noise_seed", "<u8"), ("noise_hold", "<u4"), ("reserved0", "<u4"), ("start_frame", "<u8"),
    ("guard_t", "<f8"), ("guard_c", "<f8"), ("guard_offset", "<u4"), ("guard_count", "<u4")], align=True)

MIX_EVENT_DTYPE = np.dtype([("dst_sample", "<u8"), ("src_sample", "<u8"), ("nsamples", "<u8"), ("factor", "<f8"),
                            ("src", "<u4"), ("reserved", "<u4")], align=True)          # sh_mix_event
MIX_EVENT_RATE_DTYPE = np.dtype([("dst_sample", "<u8"), ("src_sample", "<u8"), ("nsamples", "<u8"), ("src_frames", "<u8"), ("factor", "<f8"),
                                 ("src", "<u4"), ("inrate", "<u4"), ("outrate", "<u4"), ("reserved", "<u4")], align=True)   # sh_mix_event_rate
MIX_EVENT_PAN_DTYPE = np.dtype([("dst_sample", "<u8"), ("src_sample", "<u8"), ("nsamples", "<u8"), ("src_frames", "<u8"), ("factor", "<f8"),
                                ("left", "<f8"), ("right", "<f8"), ("src", "<u4"), ("inrate", "<u4"), ("outrate", "<u4"),
                                ("src_channels", "<u4"), ("reserved", "<u4")], align=True)                                   # sh_mix_event_pan
MIX_EVENT_ENV_DTYPE = np.dtype([("dst_sample", "<u8"), ("src_sample", "<u8"), ("nsamples", "<u8"), ("src_frames", "<u8"), ("factor", "<f8"),
                                ("left", "<f8"), ("right", "<f8"), ("src", "<u4"), ("inrate", "<u4"), ("outrate", "<u4"),
                                ("src_channels", "<u4"), ("seg_first", "<u4"), ("seg_count", "<u4"), ("reserved", "<u4")], align=True)   # sh_mix_event_env
MIX_EVENT_LOOP_DTYPE = np.dtype([(n, MIX_EVENT_ENV_DTYPE.fields[n][0]) for n in MIX_EVENT_ENV_DTYPE.names] +
                                [("loop_start", "<u8"), ("loop_frames", "<u8")], align=True)                                 # sh_mix_event_loop
MIX_EVENT_REV_DTYPE = np.dtype([(n, MIX_EVENT_LOOP_DTYPE.fields[n][0]) for n in MIX_EVENT_LOOP_DTYPE.names] + [("flags", "<u4")], align=True)   # sh_mix_event_rev
MIX_EVENT_REVERSED = 1                                                                                                       # sh_mix_event_rev.flags
MIX_EVENT_CHAN_DTYPE = np.dtype([(n, MIX_EVENT_REV_DTYPE.fields[n][0]) for n in MIX_EVENT_REV_DTYPE.names], align=True)       # sh_mix_event_chan
MIX_EVENT_DOWNMIX, MIX_EVENT_BALANCE = 2, 4                                                                                  # sh_mix_event_chan.flags
ENV_SEGMENT_DTYPE = np.dtype([("end", "<u8"), ("origin", "<u8"), ("mul", "<f8"), ("slope", "<f8"), ("numsamples", "<f8"), ("offset", "<f8"),
                              ("kind", "<u4"), ("reserved", "<u4")], align=True)                                             # sh_env_segment
ENV_PAN = 3                                     # sh_env_segment.kind of a pan move (SH_ENV_PAN; sh_seq_auto_create_pans' pan lanes only)
ENV_NONE, ENV_FADE_IN, ENV_FADE_OUT = 0, 1, 2                                                                              # sh_env_segment.kind

# sizes the C side must agree with (checked against the library's view in tests via sh_bank_create)
assert SEGMENT_DTYPE.itemsize == 24 and PARTIAL_DTYPE.itemsize == 16 and ENVELOPE_DTYPE.itemsize == 80
assert VOICE_DTYPE.itemsize == 272, VOICE_DTYPE.itemsize
assert MIX_EVENT_DTYPE.itemsize == 40 and MIX_EVENT_RATE_DTYPE.itemsize == 56 and MIX_EVENT_PAN_DTYPE.itemsize == 80
assert MIX_EVENT_ENV_DTYPE.itemsize == 88 and ENV_SEGMENT_DTYPE.itemsize == 56 and MIX_EVENT_LOOP_DTYPE.itemsize == 104
assert MIX_EVENT_REV_DTYPE.itemsize == 112 and MIX_EVENT_CHAN_DTYPE.itemsize == 112


class Counters(C.Structure):
    _fields_ = [("device_allocs", C.c_uint64), ("device_frees", C.c_uint64), ("stream_syncs", C.c_uint64), ("pool_hits", C.c_uint64),
                ("segmented_launches", C.c_uint64), ("tiled_launches", C.c_uint64), ("tiled_predicted", C.c_uint64)]


class SeqInfo(C.Structure):                                                          # sh_seq_info
    _fields_ = [("track_samples", C.c_uint64), ("pairs", C.c_uint64), ("device_bytes", C.c_uint64), ("nevents", C.c_uint32),
                ("ntiles", C.c_uint32), ("active_tiles", C.c_uint32), ("level", C.c_uint32)]


class SeqMeter(C.Structure):                                                         # sh_seq_meter
    _fields_ = [("peak", C.c_uint32 * 2), ("sq_hi", C.c_uint64 * 2), ("sq_lo", C.c_uint64 * 2)]


class SeqGroup(C.Structure):                                                         # sh_seq_group
    _fields_ = [("first", C.c_uint32), ("end", C.c_uint32), ("gain", C.c_double), ("left", C.c_double), ("right", C.c_double)]


SEQ_METER_DTYPE = np.dtype([("peak", "<u4", (2,)), ("sq_hi", "<u8", (2,)), ("sq_lo", "<u8", (2,))])      # sh_seq_meter, 40 bytes, no padding
assert SEQ_METER_DTYPE.itemsize == C.sizeof(SeqMeter) == 40
class SeqMeterClips(C.Structure):                                                    # sh_seq_meter_clips
    _fields_ = SeqMeter._fields_ + [("clipped", C.c_uint32 * 2)]


SEQ_METER_CLIPS_DTYPE = np.dtype(SEQ_METER_DTYPE.descr + [("clipped", "<u4", (2,))])    # sh_seq_meter_clips, 48 bytes, no padding
assert SEQ_METER_CLIPS_DTYPE.itemsize == C.sizeof(SeqMeterClips) == 48
class PcmExtent(C.Structure):                                                        # sh_pcm_extent
    _fields_ = [("lo", C.c_int32 * 2), ("hi", C.c_int32 * 2)]


PCM_EXTENT_DTYPE = np.dtype([("lo", "<i4", (2,)), ("hi", "<i4", (2,))])               # sh_pcm_extent, 16 bytes, no padding
assert PCM_EXTENT_DTYPE.itemsize == C.sizeof(PcmExtent) == 16
SEQ_MAX_GROUPS = 8                                                                    # SH_SEQ_MAX_GROUPS
SEQ_TILE_SAMPLES = {1: 1024, 2: 2048, 3: 1024, 4: 1024}                               # shq::tile_samples(width): a block of a level history
SEQ_LEVELS = ("plain", "rate", "pan", "env", "loop", "rev", "chan")                   # SH_SEQ_LEVEL_*
PCM_PART_SAMPLES = 8192                                                               # shpb::PART_SAMPLES (csrc/pcmblocks.hpp): a block up to this long is one part
PCM_FIR_MAX_TAPS = 1 << 22                                                            # shpf::MAX_TAPS (csrc/pcmfir.hpp): up to here the float64 sum is the integer sum
PCM_FIR_TILE_FRAMES = 2048                                                            # shpf::TILE_FRAMES: the output frames of one workgroup of sh_pcm_convolve
PCM_FIR_TAP_CHUNK = 1024                                                              # shpf::TAP_CHUNK: the taps under one staged span of the input
PCM_RESAMPLE_MAX_TAPS = 1 << 22                                                       # shpr::MAX_TAPS (csrc/pcmresample.hpp)
PCM_RESAMPLE_MAX_UP = 4096                                                            # shpr::MAX_UP: the largest `up` of sh_pcm_resample_fir
PCM_RESAMPLE_LANE_OUTPUTS = 8                                                         # shpr::LANE_OUTPUTS: R, the outputs of one lane
PCM_RESAMPLE_BLOCK_GROUPS = 64                                                        # shpr::BLOCK_GROUPS: the groups (of P = copies * up outputs) of one wave
PCM_RESAMPLE_WAVES = 4                                                                # shpr::WAVES: of a workgroup; with fewer than 4 residue chunks it owns up to 4 blocks
PCM_RESAMPLE_STEP_CHUNK = 1024                                                        # shpr::STEP_CHUNK: the steps under one staged span of the input
PCM_RESAMPLE_STEP_UNROLL = 2                                                          # shpr::STEP_UNROLL: the rows' length is a multiple of it
PCM_RESAMPLE_STAGED_SAMPLES = 32768                                                   # shpr::STAGED_SAMPLES: the staged span's bound
PCM_LIMIT_ONE = 1 << 30                                                               # shpl::ONE (csrc/pcmlimit.hpp): unity of sh_pcm_limit's gains
PCM_LIMIT_TILE_FRAMES = 2048                                                          # shpl::TILE_FRAMES: the frames of one workgroup of sh_pcm_limit, on the sample's own grid
PCM_LIMIT_MAX_FRAMES = 1 << 20                                                        # shpl::MAX_FRAMES: the longest attack and the longest release


def pcm_resample_copies(up: int) -> int:
    """shpr::copies: the periods of `up` outputs that make one group (P = copies * up >= 8 outputs, a stride of copies * down frames)"""
    return 1 if up >= PCM_RESAMPLE_LANE_OUTPUTS else -(-PCM_RESAMPLE_LANE_OUTPUTS // up)


def pcm_resample_stride_fits(up: int, down: int) -> bool:
    """shpr::stride_fits: whether the 64 lanes of a wave, copies * down frames apart, lie inside one staged span"""
    return (PCM_RESAMPLE_BLOCK_GROUPS - 1) * pcm_resample_copies(up) * down + PCM_RESAMPLE_STEP_CHUNK <= PCM_RESAMPLE_STAGED_SAMPLES


class MixLevel(NamedTuple):
    """One rung of the placed-sample mixer's ladder: the table layout a list of that level is packed in, the entry point that reads it,
    and which of the three signatures the entry point has (``segments``: the segment table and its length behind the event table;
    ``nchannels``: the track's channel count behind the sample width)."""
    name: str
    dtype: np.dtype
    entry: str
    segments: bool
    nchannels: bool


# in SEQ_LEVELS' order: a list's level is the highest rung one of its events needs, and every layout holds the columns of those below it
MIX_LEVELS = (MixLevel("plain", MIX_EVENT_DTYPE, "sh_mix_events", False, False),
              MixLevel("rate", MIX_EVENT_RATE_DTYPE, "sh_mix_events_rate", False, True),
              MixLevel("pan", MIX_EVENT_PAN_DTYPE, "sh_mix_events_pan", False, False),
              MixLevel("env", MIX_EVENT_ENV_DTYPE, "sh_mix_events_env", True, True),
              MixLevel("loop", MIX_EVENT_LOOP_DTYPE, "sh_mix_events_loop", True, True),
              MixLevel("rev", MIX_EVENT_REV_DTYPE, "sh_mix_events_rev", True, True),
              MixLevel("chan", MIX_EVENT_CHAN_DTYPE, "sh_mix_events_chan", True, True))
assert tuple(level.name for level in MIX_LEVELS) == SEQ_LEVELS
LEVEL_PLAIN, LEVEL_RATE, LEVEL_PAN, LEVEL_ENV, LEVEL_LOOP, LEVEL_REV, LEVEL_CHAN = range(len(MIX_LEVELS))


class DevInfo(C.Structure):
    _fields_ = [("name", C.c_char * 128), ("arch", C.c_char * 32), ("compute_units", C.c_int32),
                ("clock_mhz", C.c_int32), ("hbm_bytes", C.c_uint64), ("wavefront", C.c_int32), ("device", C.c_int32)]


# every symbol include/synthhip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_SIGNATURES = {
    "sh_init": (C.c_int, [C.c_int]),
    "sh_shutdown": (C.c_int, []),
    "sh_is_initialized": (C.c_int, []),
    "sh_device_count": (C.c_int, []),
    "sh_device_info": (C.c_int, [C.POINTER(DevInfo)]),
    "sh_device_pci": (C.c_int, [C.c_char_p, C.c_int]),
    "sh_last_error": (C.c_char_p, []),
    "sh_version": (C.c_char_p, []),
    "sh_abi": (C.c_int, [C.POINTER(C.c_uint32), C.c_int]),
    "sh_sync": (C.c_int, []),
    "sh_set_option": (C.c_int, [C.c_int, C.c_int]),
    "sh_get_option": (C.c_int, [C.c_int]),
    "sh_debug_counters": (C.c_int, [C.POINTER(Counters)]),
    "sh_buf_alloc": (C.c_int, [C.c_size_t, C.POINTER(_P)]),
    "sh_buf_free": (C.c_int, [_P]),
    "sh_buf_view": (C.c_int, [_P, C.c_size_t, C.c_size_t, C.POINTER(_P)]),
    "sh_buf_size": (C.c_size_t, [_P]),
    "sh_buf_devptr": (_P, [_P]),
    "sh_buf_upload": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t]),
    "sh_buf_download": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t]),
    "sh_buf_fill_zero": (C.c_int, [_P, C.c_size_t, C.c_size_t]),
    "sh_buf_copy": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t, C.c_size_t]),
    "sh_timer_start": (C.c_int, []),
    "sh_timer_stop": (C.c_int, [C.POINTER(C.c_float)]),
    "sh_bank_create": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, C.POINTER(_P)]),
    "sh_bank_destroy": (C.c_int, [_P]),
    "sh_bank_launch_stats": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "sh_bank_nvoices": (C.c_uint32, [_P]),
    "sh_osc_render": (C.c_int, [_P, C.c_uint32, _P, _P, C.c_uint64, C.c_uint32, _P, _P, C.c_size_t, _P]),
    "sh_ew_f64": (C.c_int, [C.c_int, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_double, C.c_double, _P, C.c_size_t, _P, C.c_size_t, _P]),
    "sh_scan_f64": (C.c_int, [_P, C.c_uint32, C.c_double, _P, C.POINTER(C.c_double)]),
    "sh_bank_generate": (C.c_int, [_P, C.c_uint64, C.c_uint32, _P, C.c_size_t]),
    "sh_bank_render": (C.c_int, [_P, C.c_uint64, C.c_uint32, _P, _P]),
    "sh_bank_render_pcm": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_double, _P]),
    "sh_bank_render_run": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(_P), C.POINTER(_P), C.c_uint32, C.c_double]),
    "sh_bank_set_rows": (C.c_int, [_P, _P, _P]),
    "sh_bank_generate_f64": (C.c_int, [_P, C.c_uint64, C.c_uint32, _P, C.c_size_t, C.c_size_t]),
    "sh_scan_rows_f64": (C.c_int, [_P, C.c_size_t, C.c_uint32, C.c_uint32, C.c_size_t, _P]),
    "sh_bank_render_rows": (C.c_int, [_P, C.c_uint64, C.c_uint32, _P, C.c_size_t, _P, _P]),
    "sh_bank_generate_rows": (C.c_int, [_P, C.c_uint64, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t]),
    "sh_bank_generate_i16": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_double, _P, C.c_size_t]),
    "sh_bank_generate_i16_async": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_double, _P, C.c_size_t]),
    "sh_overflow_check": (C.c_int, []),
    "sh_bank_mixdown_i16": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_double, _P]),
    "sh_bank_mixdown_i16_async": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_double, _P]),
    "sh_bank_generate_rows_i16": (C.c_int, [_P, C.c_uint64, C.c_uint32, _P, C.c_size_t, C.c_double, _P, C.c_size_t]),
    "sh_mix_bus_f32": (C.c_int, [_P, C.c_uint32, C.c_size_t, C.c_uint32, _P, _P]),
    "sh_mix_chain_i16": (C.c_int, [_P, C.c_uint32, C.c_size_t, C.c_uint32, _P]),
    "sh_mix_chain_pan_i16": (C.c_int, [_P, C.c_uint32, C.c_size_t, C.c_uint32, _P, _P]),
    "sh_bank_mixdown_i16_parts": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_double, _P]),
    "sh_bank_mixdown_i16_parts_async": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_double, _P]),
    "sh_mix_chain_i16_parts": (C.c_int, [_P, C.c_uint32, C.c_size_t, C.c_uint32, _P]),
    "sh_mix_chain_pan_i16_parts": (C.c_int, [_P, C.c_uint32, C.c_size_t, C.c_uint32, _P, _P]),
    "sh_chain_parts_compose": (C.c_int, [_P, C.c_uint32, C.c_size_t, C.c_uint32, _P]),
    "sh_chain_parts_apply": (C.c_int, [_P, C.c_uint32, C.c_size_t, C.c_uint32, _P, _P]),
    "sh_mix_chain_gather_i16": (C.c_int, [C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, _P, C.c_size_t]),
    "sh_mix_chain": (C.c_int, [_P, C.c_uint32, C.c_size_t, C.c_uint32, C.c_int, _P]),
    "sh_mix_chain_gather": (C.c_int, [C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_int, _P, C.c_size_t]),
    "sh_mix_events": (C.c_int, [C.POINTER(_P), C.c_uint32, _P, C.c_uint32, C.c_int, _P, C.c_size_t]),
    "sh_mix_events_rate": (C.c_int, [C.POINTER(_P), C.c_uint32, _P, C.c_uint32, C.c_int, C.c_int, _P, C.c_size_t]),
    "sh_mix_events_pan": (C.c_int, [C.POINTER(_P), C.c_uint32, _P, C.c_uint32, C.c_int, _P, C.c_size_t]),
    "sh_mix_events_env": (C.c_int, [C.POINTER(_P), C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, C.c_int, C.c_int, _P, C.c_size_t]),
    "sh_mix_events_loop": (C.c_int, [C.POINTER(_P), C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, C.c_int, C.c_int, _P, C.c_size_t]),
    "sh_mix_events_rev": (C.c_int, [C.POINTER(_P), C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, C.c_int, C.c_int, _P, C.c_size_t]),
    "sh_mix_events_chan": (C.c_int, [C.POINTER(_P), C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, C.c_int, C.c_int, _P, C.c_size_t]),
    "sh_seq_create": (C.c_int, [C.POINTER(_P), C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, C.c_int, C.c_int, C.c_size_t, C.POINTER(_P)]),
    "sh_seq_render": (C.c_int, [_P, C.c_size_t, C.c_size_t, _P, C.c_size_t]),
    "sh_seq_get_info": (C.c_int, [_P, C.POINTER(SeqInfo)]),
    "sh_seq_destroy": (C.c_int, [_P]),
    "sh_seq_create_tracks": (C.c_int, [C.POINTER(_P), C.c_uint32, _P, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, _P, C.c_uint32, C.c_int, C.c_int,
                                       C.c_size_t, C.POINTER(_P)]),
    "sh_seq_render_gains": (C.c_int, [_P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_double), C.c_uint32]),
    "sh_seq_get_tracks": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "sh_seq_render_meters": (C.c_int, [_P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_double), C.c_uint32, C.POINTER(SeqMeter), C.c_uint32]),
    "sh_seq_render_desk": (C.c_int, [_P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_double), C.c_uint32,
                                     C.c_double, C.POINTER(SeqMeter), C.c_uint32]),
    "sh_seq_auto_create": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(_P)]),
    "sh_seq_auto_create_buses": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "sh_seq_auto_create_pans": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, _P, C.c_uint32, C.POINTER(C.c_uint32),
                                          C.POINTER(_P)]),
    "sh_seq_auto_destroy": (C.c_int, [_P]),
    "sh_seq_render_auto": (C.c_int, [_P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_double), C.c_uint32,
                                     C.c_double, C.POINTER(SeqMeter), C.c_uint32, _P]),
    "sh_seq_render_groups": (C.c_int, [_P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_double), C.c_uint32,
                                       C.c_double, C.POINTER(SeqMeter), C.c_uint32, _P, C.POINTER(SeqGroup), C.c_uint32]),
    "sh_seq_render_history": (C.c_int, [_P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_double), C.c_uint32,
                                        C.c_double, C.POINTER(SeqMeter), C.c_uint32, C.c_uint32, _P, C.POINTER(SeqGroup), C.c_uint32]),
    "sh_seq_render_clips": (C.c_int, [_P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_double), C.c_uint32,
                                      C.c_double, C.POINTER(SeqMeterClips), C.c_uint32, C.c_uint32, _P, C.POINTER(SeqGroup), C.c_uint32]),
    "sh_seq_render_stems": (C.c_int, [_P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_uint32, C.POINTER(C.c_double), C.c_uint32,
                                      C.POINTER(C.c_double), C.c_uint32, C.c_double, _P, C.POINTER(SeqGroup), C.c_uint32]),
    "sh_rt_create": (C.c_int, [C.c_size_t, C.c_uint32, C.POINTER(_P)]),
    "sh_rt_destroy": (C.c_int, [_P]),
    "sh_rt_acquire": (C.c_int, [_P, _P]),
    "sh_rt_mix_turn": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]),
    "sh_quantize_f32": (C.c_int, [_P, C.c_size_t, C.c_size_t, C.c_double, C.c_int, _P, C.c_size_t]),
    "sh_quantize_f64": (C.c_int, [_P, C.c_size_t, C.c_size_t, C.c_double, C.c_int, _P, C.c_size_t]),
    "sh_quantize_clip_f32": (C.c_int, [_P, C.c_size_t, C.c_double, _P]),
    "sh_pcm_add": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_int, _P, C.c_size_t]),
    "sh_pcm_add_host": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P]),
    "sh_pcm_mul": (C.c_int, [_P, C.c_size_t, C.c_size_t, C.c_int, C.c_double, _P, C.c_size_t]),
    "sh_pcm_fade": (C.c_int, [_P, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_double, C.c_double, _P, C.c_size_t]),
    "sh_pcm_modulate": (C.c_int, [_P, C.c_size_t, C.c_int, _P, C.c_size_t, _P]),
    "sh_pcm_to_f64": (C.c_int, [_P, C.c_size_t, C.c_int, C.c_double, _P]),
    "sh_pcm_pan_lfo": (C.c_int, [_P, C.c_size_t, C.c_int, C.c_int, _P, _P]),
    "sh_pcm_bias": (C.c_int, [_P, C.c_size_t, C.c_int, C.c_int, _P]),
    "sh_pcm_reverse": (C.c_int, [_P, C.c_size_t, C.c_int, _P]),
    "sh_pcm_tomono": (C.c_int, [_P, C.c_size_t, C.c_int, C.c_double, C.c_double, _P]),
    "sh_pcm_tostereo": (C.c_int, [_P, C.c_size_t, C.c_int, C.c_double, C.c_double, _P]),
    "sh_pcm_lin2lin": (C.c_int, [_P, C.c_size_t, C.c_int, C.c_int, _P]),
    "sh_pcm_stats": (C.c_int, [_P, C.c_size_t, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]),
    "sh_pcm_stats_stereo": (C.c_int, [_P, C.c_size_t, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]),
    "sh_pcm_level_blocks": (C.c_int, [_P, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(SeqMeter),
                                      C.c_size_t]),
    "sh_pcm_extent_blocks": (C.c_int, [_P, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(PcmExtent),
                                       C.c_size_t]),
    "sh_pcm_convolve": (C.c_int, [_P, C.c_size_t, C.c_uint64, C.c_int, C.c_int, _P, C.c_size_t, C.c_uint32, C.c_int, C.c_double, C.c_uint64, C.c_uint64,
                                  _P, C.c_size_t]),
    "sh_pcm_resample_fir": (C.c_int, [_P, C.c_size_t, C.c_uint64, C.c_int, C.c_int, _P, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double,
                                      C.c_uint64, C.c_uint64, _P, C.c_size_t]),
    "sh_pcm_resample_fir_frames": (C.c_uint64, [C.c_uint64, C.c_uint32, C.c_uint32]),
    "sh_pcm_limit": (C.c_int, [_P, C.c_size_t, C.c_uint64, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, _P, C.c_size_t, _P,
                               C.c_size_t]),
    "sh_resample_out_frames": (C.c_size_t, [C.c_size_t, C.c_int, C.c_int]),
    "sh_resample": (C.c_int, [_P, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.POINTER(C.c_size_t)]),
    "sh_resample_span": (C.c_int, [C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "sh_resample_range": (C.c_int, [_P, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, _P]),
    "sh_resample_host": (C.c_int, [_P, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.POINTER(C.c_size_t)]),
    "sh_dist_unique_id": (C.c_int, [_P]),
    "sh_dist_init": (C.c_int, [C.c_int, C.c_int, _P]),
    "sh_dist_shutdown": (C.c_int, []),
    "sh_dist_rank": (C.c_int, []),
    "sh_dist_world": (C.c_int, []),
    "sh_dist_comm_info": (C.c_int, [C.POINTER(C.c_int32), C.c_int]),
    "sh_dist_reduce_bus": (C.c_int, [_P, C.c_size_t, C.c_int]),
    "sh_dist_allreduce_bus": (C.c_int, [_P, C.c_size_t]),
    "sh_dist_barrier": (C.c_int, []),
    "sh_dist_slots": (C.c_int, []),
    "sh_dist_reduce_bus_async": (C.c_int, [_P, C.c_size_t, C.c_int, _P, C.c_int]),
    "sh_dist_wait_slot": (C.c_int, [C.c_int]),
    "sh_dist_mark_slot": (C.c_int, [C.c_int]),
    "sh_dist_reduce_bus_lagged": (C.c_int, [_P, C.c_size_t, C.c_int, _P, C.c_int]),
    "sh_dist_wait_slot_keep": (C.c_int, [C.c_int]),
    "sh_dist_gather_parts": (C.c_int, [_P, C.c_size_t, C.c_int, _P]),
    "sh_bus_finalize": (C.c_int, [_P, C.c_size_t, _P]),
}

_lib: Optional[C.CDLL] = None


SH_ABI_VERSION = 6           # include/synthhip.h; bumped with every change of a struct layout or of an entry point's meaning


class NativeLibraryStale(ImportError):
    pass


def _abi_expected() -> list:
    return [SH_ABI_VERSION, SEGMENT_DTYPE.itemsize, PARTIAL_DTYPE.itemsize, ENVELOPE_DTYPE.itemsize, VOICE_DTYPE.itemsize,
            C.sizeof(DevInfo), C.sizeof(Counters)]


def _check_abi(handle: C.CDLL, path) -> None:
    """Refuse a library whose view of the structs differs from this binding's: Python would pack records it misreads."""
    if not hasattr(handle, "sh_abi"):
        raise NativeLibraryStale("%s exports no sh_abi: it predates this binding (ABI %d); rebuild it with "
                                 "`python -m synthesizer_amd.build`" % (path, SH_ABI_VERSION))
    handle.sh_abi.restype = C.c_int
    handle.sh_abi.argtypes = [C.POINTER(C.c_uint32), C.c_int]
    got = (C.c_uint32 * 7)()
    n = handle.sh_abi(got, 7)
    want = _abi_expected()
    if n != 7 or list(got) != want:
        raise NativeLibraryStale("%s was built for another binary interface: (ABI, sizeof sh_segment, sh_partial, sh_envelope, sh_voice, "
                                 "sh_devinfo, sh_counters) = %s, this binding packs %s; rebuild it with `python -m synthesizer_amd.build`"
                                 % (path, list(got), want))


def lib() -> C.CDLL:
    """Load libsynthhip.so (CDLL: the GIL is released around every call).

    The in-tree library is rebuilt when its embedded source hash differs from the tree's.  A stale library is only ever loaded
    when the COMPILER is absent (a shipped .so on a box without hipcc) or SYNTHHIP_ALLOW_STALE=1 says so -- a tree that no longer
    compiles is an error, not a reason to run old code -- and in every case the library's binary interface (sh_abi: version and
    struct sizes) must be this binding's."""
    global _lib
    if _lib is None:
        if "SYNTHHIP_LIB" not in os.environ:
            from . import build as _build
            try:                                    # in-tree build when missing or stale (embedded source hash != the tree's)
                _build.build(verbose=False)
            except Exception as exc:
                if not LIB_PATH.exists():
                    raise NativeLibraryMissing(
                        "%s not found and building it failed (%s): run `python -m synthesizer_amd.build` "
                        "(hipcc, gfx950).  There is no CPU fallback." % (LIB_PATH, exc))
                no_compiler = isinstance(exc, FileNotFoundError) and not Path(_build.HIPCC).exists()
                if not (no_compiler or os.environ.get("SYNTHHIP_ALLOW_STALE") == "1"):
                    raise NativeLibraryStale(
                        "%s is stale (built from sources %s, the tree is %s) and rebuilding it FAILED (%s).  Fix the build, or set "
                        "SYNTHHIP_ALLOW_STALE=1 to load the old library knowingly." % (LIB_PATH, _build.built_hash() or "?", _build.source_hash(), exc))
                # a shipped library on a box without the compiler: use it, but say that it is not what the tree describes
                import warnings
                warnings.warn("%s is stale (built from sources %s, the tree is %s) and cannot be rebuilt here (%s): loading it as it is"
                              % (LIB_PATH, _build.built_hash() or "?", _build.source_hash(), exc), RuntimeWarning)
        if not LIB_PATH.exists():
            raise NativeLibraryMissing(
                "%s not found: build it with `python -m synthesizer_amd.build` (hipcc, gfx950). "
                "There is no CPU fallback." % LIB_PATH)
        handle = C.CDLL(str(LIB_PATH))
        _check_abi(handle, LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            if "SYNTHHIP_LIB" in os.environ and not hasattr(handle, name):
                continue                    # an older build named for an A/B timing (tools/): what it lacks cannot be called
            fn = getattr(handle, name)      # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def exported_symbols() -> list:
    return sorted(_SIGNATURES)


def check(rc: int) -> None:
    if rc != SH_OK:
        msg = lib().sh_last_error().decode("utf-8", "replace")
        if rc == SH_ERR_OVERFLOW:
            raise OverflowError(msg)
        if rc == SH_ERR_LENGTH:
            raise ValueError("Lengths should be the same (" + msg + ")")
        if rc == SH_ERR_INVALID:
            raise ValueError(msg)
        if rc == SH_ERR_NOMEM:
            raise MemoryError(msg)
        raise SynthHipError(rc, msg)


def set_quantise_round(on: bool) -> None:
    """params.variants["quantise"]: "round" -> the library's quantisers round half to even (sh_set_option); "trunc" -> int()'s rule."""
    check(lib().sh_set_option(SH_OPT_QUANTISE_ROUND, 1 if on else 0))


_initialized = False


def ensure_init(device: Optional[int] = None) -> None:
    """sh_init on first use.  Device: explicit argument, else SYNTHHIP_DEVICE, else LOCAL_RANK, else 0."""
    global _initialized
    if _initialized:
        return
    if device is None:
        device = int(os.environ.get("SYNTHHIP_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    L = lib()
    if L.sh_device_count() <= 0:
        raise SynthHipError(SH_ERR_NOTINIT, "no HIP device visible; this package has no CPU fallback")
    check(L.sh_init(device))
    _initialized = True


def shutdown() -> None:
    """sh_shutdown (which tears the RCCL state down first) and forget the initialisation, so that the next call
    re-initialises instead of failing with SH_ERR_NOTINIT."""
    global _initialized
    if _lib is not None:
        check(_lib.sh_shutdown())
    _initialized = False


def device_info() -> dict:
    ensure_init()
    info = DevInfo()
    check(lib().sh_device_info(C.byref(info)))
    return {"name": info.name.decode(), "arch": info.arch.decode(), "compute_units": info.compute_units,
            "clock_mhz": info.clock_mhz, "hbm_bytes": info.hbm_bytes, "wavefront": info.wavefront,
            "device": info.device}


def device_pci() -> str:
    """PCI bus id of the GPU this process renders on (distinct per rank of a multi-GPU job: bench.py prints it per rank)."""
    ensure_init()
    buf = C.create_string_buffer(64)
    check(lib().sh_device_pci(buf, 64))
    return buf.value.decode()


class RtLane:
    """A real-time lane (sh_rt_*; include/synthhip.h): a stream, a lock and buffers of its own for a mixer that another thread drains
    while the library's one stream pair is busy.  ``mix_turn`` returns the chunk as bytes and takes the lane's lock only."""

    def __init__(self, max_chunk_bytes: int, max_sources: int = 1024) -> None:
        ensure_init()
        self._h = _P()
        self.max_chunk_bytes = int(max_chunk_bytes)
        check(lib().sh_rt_create(self.max_chunk_bytes, int(max_sources), C.byref(self._h)))
        self._out = (C.c_char * self.max_chunk_bytes)()

    def acquire(self, buf: "DeviceBuffer") -> None:
        """The lane's next turn waits (on the device) for everything the library has been given so far: what made ``buf``."""
        check(lib().sh_rt_acquire(self._h, buf.handle))

    def mix_turn(self, sources, nsamples: int, width: int) -> bytes:
        n = len(sources)
        bufs = (C.c_void_p * max(n, 1))(*[b.handle for b, _o, _n in sources])
        offs = (C.c_size_t * max(n, 1))(*[o for _b, o, _n in sources])
        lens = (C.c_uint32 * max(n, 1))(*[min(k, 0xFFFFFFFF) for _b, _o, k in sources])
        check(lib().sh_rt_mix_turn(self._h, bufs, offs, lens, n, nsamples, width, C.cast(self._out, C.c_void_p)))
        return self._out.raw[:nsamples * width]

    def close(self) -> None:
        if self._h:
            try:
                lib().sh_rt_destroy(self._h)
            finally:
                self._h = _P()

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:
            pass


def _doubles(v):
    """None, or a C array of doubles (of one element at least)"""
    return None if v is None else (C.c_double * max(1, len(v)))(*v)


def _count(v) -> int:
    return 0 if v is None else len(v)


def _group_table(groups) -> tuple:
    """(the sh_seq_group table of a desk's groups, their number): (None, 0) where there are none"""
    if not groups:
        return None, 0
    return (SeqGroup * len(groups))(*[SeqGroup(*g) for g in groups]), len(groups)


class Sequence:
    """RAII wrapper over sh_seq: a list of placed samples compiled once (records and per-tile index resident on the device), rendered
    window by window.  ``sources`` are the DeviceBuffers the records point into: the handle keeps them alive.  ``track_first`` (one offset
    into ``table`` per track and the table's length behind them): a song of tracks, sh_seq_create_tracks, rendered with a gain per track."""

    def __init__(self, sources, table: np.ndarray, segments: Optional[np.ndarray], width: int, nchannels: int, track_samples: int,
                 track_first=None) -> None:
        ensure_init()
        assert table.dtype == MIX_EVENT_CHAN_DTYPE and (segments is None or segments.dtype == ENV_SEGMENT_DTYPE)
        self._sources = list(sources)
        self._width = width
        self._h = _P()
        srcs = (C.c_void_p * max(1, len(self._sources)))(*[b.handle for b in self._sources])
        nseg = 0 if segments is None else len(segments)
        if track_first is None:
            check(lib().sh_seq_create(srcs, len(self._sources), _ptr(table), len(table), _ptr(segments), nseg, width, nchannels,
                                      track_samples, C.byref(self._h)))
        else:
            first = (C.c_uint32 * len(track_first))(*track_first)
            check(lib().sh_seq_create_tracks(srcs, len(self._sources), _ptr(table), len(table), first, len(track_first) - 1, _ptr(segments), nseg,
                                             width, nchannels, track_samples, C.byref(self._h)))

    @property
    def handle(self):
        return self._h

    def info(self) -> dict:
        i = SeqInfo()
        check(lib().sh_seq_get_info(self._h, C.byref(i)))
        return {name: getattr(i, name) for name, _ in SeqInfo._fields_}

    def tracks(self) -> tuple:
        """(tracks, runs): sh_seq_get_tracks; (0, 0) for a song without tracks"""
        nt, nr = C.c_uint32(), C.c_uint32()
        check(lib().sh_seq_get_tracks(self._h, C.byref(nt), C.byref(nr)))
        return nt.value, nr.value

    def render(self, first_sample: int, nsamples: int, out: "DeviceBuffer", out_sample: int = 0, gains=None, meters: bool = False, pans=None,
               master=None, automation: Optional["SeqAutomation"] = None, groups=None, clips: bool = False):
        """``meters=True`` (a song of tracks): sh_seq_render_meters -- the same bytes and, from the same launch, one row per track and one for
        the master, each ``(peak, sum_squares)`` of per-channel pairs, the sums exact Python ints.  Otherwise None.
        ``pans`` (2 * ntracks factors, left then right per track) or ``master`` (a gain) given: sh_seq_render_desk, with or without meters.
        ``automation`` (a ``SeqAutomation`` of this song) given: sh_seq_render_auto, with or without any of the others.
        ``groups`` (a non-empty list of ``(first_track, end_track, gain, left, right)``) given: sh_seq_render_groups, with or without any
        of the others; the rows of the groups follow the master's.  An ``automation`` with lanes of the buses (``SeqAutomation(...,
        ngroups)``) goes the same two ways: a master ride alone needs no ``groups``, a ride on group ``g`` more than ``g`` of them.
        ``meters="history"`` (a song of tracks): sh_seq_render_history -- the same bytes and, from the same launch, the rows per BLOCK of the
        window, a block being one tile of the song's grid (``SEQ_TILE_SAMPLES[width]`` samples) cut to the window: a numpy array of shape
        ``(nblocks, nrows)`` and dtype ``SEQ_METER_DTYPE`` (sh_seq_meter's fields; a sum is ``(sq_hi << 32) + sq_lo``), rows in the order
        ``meters=True`` has them.  With or without any of the others, ``groups`` empty or None included.
        ``clips=True`` with ``meters="history"``: sh_seq_render_clips -- the same, the array's dtype ``SEQ_METER_CLIPS_DTYPE``: a field
        ``clipped`` behind the levels, per channel the block's samples at which the row's own arithmetic was clamped."""
        if not isinstance(meters, bool) and not (isinstance(meters, str) and meters == "history"):
            raise ValueError("Sequence.render: meters is True, False or \"history\", not %r" % (meters,))
        if clips and meters != "history":
            raise ValueError("Sequence.render: clips=True counts per block of a history: it needs meters=\"history\"")
        desk = pans is not None or master is not None
        rows, nrows = None, 0
        if meters == "history":
            tile = SEQ_TILE_SAMPLES[self._width]
            nblocks = (first_sample + nsamples - 1) // tile - first_sample // tile + 1 if nsamples > 0 else 0
            nrows = self.tracks()[0] + 1 + (len(groups) if groups else 0)
            blocks = np.zeros((nblocks, nrows), dtype=SEQ_METER_CLIPS_DTYPE if clips else SEQ_METER_DTYPE)
            rows = blocks.ctypes.data_as(C.POINTER(SeqMeterClips if clips else SeqMeter)) if nblocks else None
            table, ngroups = _group_table(groups)
            entry = lib().sh_seq_render_clips if clips else lib().sh_seq_render_history
            check(entry(self._h, first_sample, nsamples, out.handle, out_sample, _doubles(gains), _count(gains), _doubles(pans),
                                              _count(pans), 1.0 if master is None else master, rows, nrows, nblocks,
                                              None if automation is None else automation.handle, table, ngroups))
            return blocks
        if meters:
            nrows = self.tracks()[0] + 1 + (len(groups) if groups else 0)
            rows = (SeqMeter * nrows)()
        if groups:
            table, ngroups = _group_table(groups)
            check(lib().sh_seq_render_groups(self._h, first_sample, nsamples, out.handle, out_sample, _doubles(gains), _count(gains), _doubles(pans),
                                             _count(pans), 1.0 if master is None else master, rows, nrows,
                                             None if automation is None else automation.handle, table, ngroups))
        elif automation is not None:
            check(lib().sh_seq_render_auto(self._h, first_sample, nsamples, out.handle, out_sample, _doubles(gains), _count(gains), _doubles(pans), _count(pans),
                                           1.0 if master is None else master, rows, nrows, automation.handle))
        elif desk:
            check(lib().sh_seq_render_desk(self._h, first_sample, nsamples, out.handle, out_sample, _doubles(gains), _count(gains), _doubles(pans), _count(pans),
                                           1.0 if master is None else master, rows, nrows))
        elif meters:
            check(lib().sh_seq_render_meters(self._h, first_sample, nsamples, out.handle, out_sample, _doubles(gains), _count(gains), rows, nrows))
        elif gains is None:
            check(lib().sh_seq_render(self._h, first_sample, nsamples, out.handle, out_sample))
        else:
            check(lib().sh_seq_render_gains(self._h, first_sample, nsamples, out.handle, out_sample, _doubles(gains), len(gains)))
        if meters:
            return [((r.peak[0], r.peak[1]), ((r.sq_hi[0] << 32) + r.sq_lo[0], (r.sq_hi[1] << 32) + r.sq_lo[1])) for r in rows]

    def stems(self, first_sample: int, nsamples: int, out: "DeviceBuffer", out_sample: int, plane_samples: int, gains=None, pans=None, master=None,
              automation: Optional["SeqAutomation"] = None, groups=None) -> None:
        """sh_seq_render_stems (a song of tracks): the desk of ``render`` with the same keywords, and instead of the master alone
        ``ntracks + 1 + len(groups)`` planes of ``nsamples`` samples, ``plane_samples`` apart from ``out_sample`` on, in the meter rows'
        order -- the tracks as their bus takes them, the master, the groups as the master takes them.  One launch, asynchronous."""
        table, ngroups = _group_table(groups)
        check(lib().sh_seq_render_stems(self._h, first_sample, nsamples, out.handle, out_sample, plane_samples, self.tracks()[0] + 1 + ngroups,
                                        _doubles(gains), _count(gains), _doubles(pans), _count(pans), 1.0 if master is None else master,
                                        None if automation is None else automation.handle, table, ngroups))

    def free(self) -> None:
        if self._h:
            try:
                lib().sh_seq_destroy(self._h)
            finally:
                self._h = _P()
                self._sources = []

    def __del__(self) -> None:
        try:
            self.free()
        except Exception:
            pass


class SeqAutomation:
    """RAII wrapper over sh_seq_auto: the fader moves of a song of tracks -- ``segments`` (ENV_SEGMENT_DTYPE rows in SONG samples, the tracks'
    one behind the other) and ``seg_first`` (one offset per track and the table's length behind them) -- uploaded once into a device table
    of its own; ``Sequence.render(automation=)`` applies it.  With ``ngroups`` the table also holds the lanes of the BUSES, in the meter
    table's row order: the master's behind the last track's, then the groups' (sh_seq_auto_create_buses); a render with such a handle
    names every group it rides."""

    def __init__(self, seq: Sequence, segments: np.ndarray, seg_first, ngroups: Optional[int] = None, pan_segments: Optional[np.ndarray] = None,
                 pan_first=None) -> None:
        """``ngroups`` None: one lane per track (sh_seq_auto_create).  A number 0 .. SEQ_MAX_GROUPS: the lanes of the buses behind the
        tracks', in the meter table's row order -- the master's, then ``ngroups`` groups' (sh_seq_auto_create_buses).  ``pan_segments``
        (ENV_SEGMENT_DTYPE rows, moves of kind ENV_PAN) and ``pan_first`` given, with ``ngroups``: the PAN lanes as well, the tracks'
        and then ``ngroups`` groups', ``ntracks + ngroups + 1`` offsets (sh_seq_auto_create_pans)."""
        ensure_init()
        assert segments.dtype == ENV_SEGMENT_DTYPE and len(seg_first) >= 2 and seg_first[-1] == len(segments)
        self._h = _P()
        first = (C.c_uint32 * len(seg_first))(*seg_first)
        if pan_segments is not None:
            assert ngroups is not None and 0 <= ngroups and len(seg_first) >= ngroups + 3 and pan_segments.dtype == ENV_SEGMENT_DTYPE
            ntracks = len(seg_first) - 2 - ngroups
            assert len(pan_first) == ntracks + ngroups + 1 and pan_first[-1] == len(pan_segments)
            pfirst = (C.c_uint32 * len(pan_first))(*pan_first)
            check(lib().sh_seq_auto_create_pans(seq.handle, _ptr(segments), len(segments), first, ntracks, ngroups, _ptr(pan_segments),
                                                len(pan_segments), pfirst, C.byref(self._h)))
        elif ngroups is None:
            check(lib().sh_seq_auto_create(seq.handle, _ptr(segments), len(segments), first, len(seg_first) - 1,
                                           C.byref(self._h)))
        else:
            assert 0 <= ngroups and len(seg_first) >= ngroups + 3
            check(lib().sh_seq_auto_create_buses(seq.handle, _ptr(segments), len(segments), first, len(seg_first) - 2 - ngroups, ngroups,
                                                 C.byref(self._h)))

    @property
    def handle(self):
        return self._h

    def free(self) -> None:
        if self._h:
            try:
                lib().sh_seq_auto_destroy(self._h)
            finally:
                self._h = _P()

    def __del__(self) -> None:
        try:
            self.free()
        except Exception:
            pass


def pcm_level_blocks(buf: "DeviceBuffer", sample_offset: int, nframes: int, nch: int, width: int, plane_samples: int, nplanes: int,
                     origin_frame: int, block_frames: int) -> np.ndarray:
    """sh_pcm_level_blocks: the levels per block of ``nplanes`` planes of PCM in ``buf`` -- ``nframes`` frames of ``nch`` channels from
    sample ``sample_offset`` on, the planes ``plane_samples`` samples apart -- on the frame grid of ``block_frames`` on which the first
    frame stands at ``origin_frame``: a numpy array of shape ``(nblocks, nplanes)`` and dtype ``SEQ_METER_DTYPE``, as
    ``Sequence.render(meters="history")`` returns it.  One launch, synchronous; an empty window launches nothing."""
    nblocks = (origin_frame + nframes - 1) // block_frames - origin_frame // block_frames + 1 if nframes > 0 else 0
    blocks = np.zeros((nblocks, nplanes), dtype=SEQ_METER_DTYPE)
    rows = blocks.ctypes.data_as(C.POINTER(SeqMeter)) if blocks.size else None
    check(lib().sh_pcm_level_blocks(buf.handle, sample_offset, nframes, nch, width, plane_samples, nplanes, origin_frame, block_frames, rows, nblocks))
    return blocks


def pcm_extent_blocks(buf: "DeviceBuffer", sample_offset: int, nframes: int, nch: int, width: int, plane_samples: int, nplanes: int,
                      origin_frame: int, block_frames: int) -> np.ndarray:
    """sh_pcm_extent_blocks: the waveform extremes per block of the planes ``pcm_level_blocks`` describes, on its grid: a numpy array of
    shape ``(nblocks, nplanes)`` and dtype ``PCM_EXTENT_DTYPE`` -- per channel ``lo`` and ``hi``, the smallest and the largest sample
    (``audioop.minmax``), a mono input's channel 1 reading 0.  One launch, synchronous; an empty window launches nothing."""
    nblocks = (origin_frame + nframes - 1) // block_frames - origin_frame // block_frames + 1 if nframes > 0 else 0
    blocks = np.zeros((nblocks, nplanes), dtype=PCM_EXTENT_DTYPE)
    rows = blocks.ctypes.data_as(C.POINTER(PcmExtent)) if blocks.size else None
    check(lib().sh_pcm_extent_blocks(buf.handle, sample_offset, nframes, nch, width, plane_samples, nplanes, origin_frame, block_frames, rows, nblocks))
    return blocks


def debug_counters() -> dict:
    """Driver allocations / frees / self-inserted stream synchronisations / pool hits since sh_init (sh_debug_counters)."""
    c = Counters()
    check(lib().sh_debug_counters(C.byref(c)))
    return {name: getattr(c, name) for name, _ in Counters._fields_}


def sync() -> None:
    ensure_init()
    check(lib().sh_sync())


class DeviceBuffer:
    """RAII wrapper over sh_buf (HBM allocation owned by the library)."""

    def __init__(self, nbytes: int) -> None:
        ensure_init()
        self._h = _P()
        self.nbytes = int(nbytes)
        check(lib().sh_buf_alloc(self.nbytes, C.byref(self._h)))

    @property
    def handle(self):
        return self._h

    def view(self, offset: int, nbytes: int) -> "DeviceBuffer":
        """A non-owning window of this buffer (keeps the parent alive)."""
        v = DeviceBuffer.__new__(DeviceBuffer)
        v._h = _P()
        v.nbytes = int(nbytes)
        v._parent = self
        check(lib().sh_buf_view(self._h, offset, nbytes, C.byref(v._h)))
        return v

    @classmethod
    def from_array(cls, arr: np.ndarray) -> "DeviceBuffer":
        arr = np.ascontiguousarray(arr)
        buf = cls(arr.nbytes)
        buf.upload(arr)
        return buf

    @classmethod
    def from_bytes(cls, data: bytes) -> "DeviceBuffer":
        buf = cls(len(data))
        if data:
            tmp = (C.c_char * len(data)).from_buffer_copy(data)
            check(lib().sh_buf_upload(buf._h, 0, C.addressof(tmp), len(data)))
        return buf

    def upload(self, arr: np.ndarray, offset: int = 0) -> None:
        arr = np.ascontiguousarray(arr)
        if arr.nbytes:
            check(lib().sh_buf_upload(self._h, offset, arr.ctypes.data, arr.nbytes))

    def download(self, dtype, count: int, offset: int = 0) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        if out.nbytes:
            check(lib().sh_buf_download(self._h, offset, out.ctypes.data, out.nbytes))
        return out

    def download_bytes(self, nbytes: int, offset: int = 0) -> bytes:
        return self.download(np.uint8, nbytes, offset).tobytes()

    def zero(self, offset: int = 0, nbytes: Optional[int] = None) -> None:
        check(lib().sh_buf_fill_zero(self._h, offset, self.nbytes - offset if nbytes is None else nbytes))

    def free(self) -> None:
        if self._h:
            try:
                lib().sh_buf_free(self._h)
            finally:
                self._h = _P()

    def __del__(self) -> None:
        try:
            self.free()
        except Exception:
            pass


def _ptr(arr: Optional[np.ndarray]):
    return None if arr is None or arr.size == 0 else arr.ctypes.data


class Bank:
    """RAII wrapper over sh_bank."""

    def __init__(self, voices: np.ndarray, segs: np.ndarray, coefs: np.ndarray, partials: np.ndarray) -> None:
        ensure_init()
        assert voices.dtype == VOICE_DTYPE and segs.dtype == SEGMENT_DTYPE
        assert coefs.dtype == np.float64 and partials.dtype == PARTIAL_DTYPE
        self._keep = (np.ascontiguousarray(voices), np.ascontiguousarray(segs),
                      np.ascontiguousarray(coefs), np.ascontiguousarray(partials))
        v, s, c, p = self._keep
        self._h = _P()
        self.nvoices = len(v)
        check(lib().sh_bank_create(_ptr(v), len(v), _ptr(s), len(s), _ptr(c), len(c), _ptr(p), len(p), C.byref(self._h)))

    @property
    def handle(self):
        return self._h

    def free(self) -> None:
        if self._h:
            try:
                lib().sh_bank_destroy(self._h)
            finally:
                self._h = _P()

    def __del__(self) -> None:
        try:
            self.free()
        except Exception:
            pass


def timer_start() -> None:
    check(lib().sh_timer_start())


def timer_stop() -> float:
    ms = C.c_float()
    check(lib().sh_timer_stop(C.byref(ms)))
    return float(ms.value)
