/*
 * synthhip.h -- C ABI of libsynthhip.so: the MI355X (gfx950) implementation of
 * synthplayer's oscillator-bank + sample-mixing hot path.
 *
 * The reference (irmen/synthesizer, package `synthplayer`) is pure Python and has
 * NO native/FFI boundary of its own; its "plugin interface" for this path is the
 * public Python class API.  The tree mounted at /root/reference holds only a
 * relocation notice (/root/reference/README.md:1-2), so the upstream symbols are
 * named here without line numbers:
 *
 *   synthplayer/oscillators.py  Oscillator.blocks(), Sine, Sawtooth, Square, Pulse,
 *                               Harmonics, fm_lfo= / pwm_lfo=, EnvelopeFilter
 *   synthplayer/sample.py       Sample.from_osc_block (quantise), Sample.mix,
 *                               Sample.mix_at, Sample.resample
 *   synthplayer/playback.py     mixer loop: repeated audioop.add over voice chunks
 *   CPython 3.10 Modules/audioop.c  audioop.add, audioop.ratecv (the arithmetic
 *                               Sample.mix / Sample.resample delegate to)
 *
 * Each entry point below says which of those it replaces.  INTEGRATION.md shows the
 * ctypes binding a synthplayer maintainer would add.
 *
 * Conventions
 *   - every function returns SH_OK (0) or a negative sh_status; nothing throws across
 *     the ABI; sh_last_error() returns a thread-local message for the last failure.
 *   - the caller owns all host memory; the library owns device memory behind sh_buf /
 *     sh_bank handles.  No callbacks.  Plain pointers and sizes only.
 *   - one HIP stream per process (created by sh_init).  Calls may come from any thread:
 *     each entry point runs under one process-wide lock (the real-time mixer is fed from
 *     one thread and drained from another), so calls serialise -- in the order the lock is
 *     won, which is also their order on the stream.  Kernel launches are asynchronous;
 *     functions that copy to host memory, and sh_sync(), synchronise (holding the lock).
 *   - "frame" = one sample period (all channels); PCM is interleaved, little endian.
 */
#ifndef SYNTHHIP_H
#define SYNTHHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum sh_status {
    SH_OK = 0,
    SH_ERR_INVALID = -1,   /* bad argument */
    SH_ERR_HIP = -2,       /* HIP runtime error (message has the hipError string) */
    SH_ERR_NOMEM = -3,
    SH_ERR_NOTINIT = -4,   /* sh_init not called / no GPU */
    SH_ERR_OVERFLOW = -5,  /* quantise: a sample does not fit the PCM width (OverflowError upstream) */
    SH_ERR_RCCL = -6,
    SH_ERR_LENGTH = -7     /* audioop.add: "Lengths should be the same" */
} sh_status;

typedef enum sh_kind {     /* oscillators.py class names */
    SH_SINE = 0, SH_SAWTOOTH = 1, SH_SQUARE = 2, SH_PULSE = 3, SH_HARMONICS = 4, SH_TRIANGLE = 5,
    SH_LINEAR = 6,         /* Linear: the sample IS the accumulated value of the phase table (level += increment until
                            * it leaves (min, max); the host ends the table with a constant piece there) */
    SH_NOISE = 7,          /* WhiteNoise: sample-and-hold uniform noise from a counter-based generator, below */
    SH_BUFFER = 8          /* a voice whose float64 samples were rendered elsewhere (MixingFilter, EchoFilter, nested envelopes ...):
                            * row fm_row[voice] of sh_bank_render_rows' matrix; the fused envelope and the bus gains still apply */
} sh_kind;

typedef enum sh_fm_mode {
    SH_FM_NONE = 0,        /* non-FM branch of blocks(): t accumulates f/sr, phase table below */
    SH_FM_SINE = 1,        /* fm_lfo is a plain (non-FM) Sine: closed-form running sum of the LFO */
    SH_FM_BUFFER = 2       /* any fm_lfo: running sum supplied as a device buffer (sh_osc_render only) */
} sh_fm_mode;

/* One piece of an accumulated-phase table: for n0 <= n < next.n0 the reference's
 * running `t` (t += inc in float64) equals fma(n - n0, dt, t0) exactly. */
typedef struct sh_segment {
    uint64_t n0;
    double   t0;
    double   dt;
} sh_segment;

/* One (k, amp) pair of Harmonics(harmonics=[...]) -- used when the list is not dense. */
typedef struct sh_partial {
    double k;
    double amp;
} sh_partial;

/* EnvelopeFilter, reduced on the host to integer sample boundaries (the host replays the
 * reference's accumulated `time` exactly) and per-phase slopes. */
typedef struct sh_envelope {
    uint64_t n_attack_end;     /* [0, n_attack_end): gain = n*attack_slope */
    uint64_t n_decay_end;      /* [.., n_decay_end): gain = 1 + (n-n_attack_end)*decay_slope */
    uint64_t n_sustain_end;    /* [.., n_sustain_end): gain = sustain_level */
    uint64_t n_release_end;    /* [.., n_release_end): gain = sustain_level + (n-n_sustain_end)*release_slope */
    double   attack_slope, decay_slope, sustain_level, release_slope;
    double   tail_amp;         /* gain of the one extra sample at n_release_end when has_tail */
    int32_t  enabled;
    int32_t  has_tail;
} sh_envelope;

typedef struct sh_voice {
    int32_t  kind;             /* sh_kind */
    int32_t  fm_mode;          /* sh_fm_mode */
    double   amplitude, bias, pulsewidth;
    /* SH_FM_NONE: carrier phase table (t in radians for Sine/Harmonics, in turns otherwise).
     * SH_FM_SINE with a Sine LFO that moves (lfo_K != 0): the table of the LFO's running sum, TWO records per piece of the LFO's own
     * accumulated phase -- (n0, t0, dt) and (n0, K_p, C_p): on samples n0_p <= n < n0_{p+1},
     * L(n) = K_p * (C_p - cos(t0_p + (n - n0_p - 1/2) * dt_p)) + lfo_bias * n  (oscillators.LfoTable: the prefix sums of the pieces in
     * front are folded into C_p); seg_count = 0: a constant LFO, lfo_a .. lfo_C0 below are all there is. */
    uint32_t seg_offset, seg_count;
    /* Harmonics, by harm_dense:
     *   0 sparse  -> harm_count sh_partial at partial[harm_offset], summed term by term
     *   1 dense   -> harm_count Clenshaw coefficients (doubles, k = harm_count..1, count a multiple of 8)
     *                at coef[harm_offset]
     *   2 poly    -> 16 doubles at coef[harm_offset], highest power first: sum_k a_k sin(k t) =
     *                sin(t) * P(cos t), P of degree 15 (all k <= 16; converted exactly on the host) */
    uint32_t harm_offset, harm_count;
    int32_t  harm_dense;
    int32_t  flip;             /* SawtoothH: the sample is mirrored around the bias, value = bias*2.0 - value */
    /* FM: theta_n = fm_phase0 + frequency*T_n + frequency*fm_inc*L(n), T = shared time table
     * (t += fm_inc from 0), L(n) = sum_{j<n} lfo_j */
    double   frequency, fm_phase0, fm_inc;
    uint32_t time_seg_offset, time_seg_count;
    /* SH_FM_SINE: lfo_j = lfo_amp*sin(phase_j) + lfo_bias, phase_j the LFO's accumulated phase (lfo_a, += lfo_d per sample in float64:
     * piecewise exactly linear -- the table at seg_offset); on the ideal line phase_j = lfo_a + j*lfo_d (the first piece, and all
     * there is for a library older than ABI 5):
     * L(n) = lfo_K*(lfo_C0 - cos(lfo_a + (n-0.5)*lfo_d)) + lfo_bias*n,
     * lfo_K = lfo_amp/(2 sin(lfo_d/2)), lfo_C0 = cos(lfo_a - lfo_d/2).  ABI 5: lfo_bias must be 0 -- the bias rides in `frequency`
     * (f * (1 + bias)) -- and lfo_K != 0 needs the table; sh_bank_create rejects anything else. */
    double   lfo_a, lfo_d, lfo_amp, lfo_bias, lfo_K, lfo_C0;
    sh_envelope env;
    float    gain_l, gain_r;   /* stereo bus gains (bank only) */
    /* SH_NOISE: sample n holds value number h = n / noise_hold; u = (splitmix64(noise_seed + h * 0x9E3779B97F4A7C15) >> 11)
     * * 2^-53 in [0, 1); value = (-amplitude + (2*amplitude)*u) + bias   (random.uniform(-a, a) + bias) */
    uint64_t noise_seed;
    uint32_t noise_hold;       /* samples per held value, >= 1: int(samplerate / frequency) */
    uint32_t reserved0;
    /* Onset: the voice is silent in frames n < start_frame and plays its sample n - start_frame from there (phase tables,
     * envelope boundaries, FM sums and noise counters all count from the onset): upstream's DelayFilter(voice, seconds) with
     * seconds >= 0, start_frame = int(samplerate * seconds), fused into the voice.  0 for voices that read rows. */
    uint64_t start_frame;
    /* ABI 6 -- the int16 boundary guard of a Harmonics voice in the polynomial or Clenshaw form (harm_dense 2 / 1).  Those forms sum
     * a_k sin(k t) of the EXACT products k t where the reference rounds every `t * k` before its sine: the float64 samples part
     * ways by up to guard_t * |t| + guard_c (t: the accumulated phase), far inside the float contract -- but where int(scale * v)
     * of such a sample lies that close to an integer, the int16 routes (sh_bank_generate_i16, sh_bank_mixdown_i16) recompute it
     * term by term from the voice's own list, guard_count sh_partial at partial[guard_offset] in the order of the reference's
     * loop: equal integers whatever the time into the note.  guard_count = 0: no guard (the sample is quantised as it is).  Any
     * tolerance is honoured (from 1/8 on, every sample is summed term by term), and a list of any length: a polynomial voice whose list
     * is longer than 255 entries takes the general code instead of the lean kernels on every route. */
    double   guard_t, guard_c;
    uint32_t guard_offset, guard_count;
} sh_voice;

typedef struct sh_devinfo {
    char     name[128];
    char     arch[32];
    int32_t  compute_units;
    int32_t  clock_mhz;
    uint64_t hbm_bytes;
    int32_t  wavefront;
    int32_t  device;
} sh_devinfo;

typedef struct sh_buf  sh_buf;   /* device buffer */
typedef struct sh_bank sh_bank;  /* voice table resident in HBM */

/* ---- lifecycle -------------------------------------------------------------------- */
int  sh_init(int device);                 /* select GPU, create the stream; idempotent */
int  sh_shutdown(void);
int  sh_is_initialized(void);
int  sh_device_count(void);               /* 0 when no GPU is visible; never fails */
int  sh_device_info(sh_devinfo* out);
int  sh_device_pci(char* out, int n);     /* PCI bus id ("0000:c1:00.0") of the device sh_init selected, NUL-terminated */
const char* sh_last_error(void);
const char* sh_version(void);
/* The binary interface this library was compiled with, so that a binding can refuse a library whose structs it would mis-pack
 * (a stale .so loaded by path: same symbols, other layouts): out[0] = SH_ABI_VERSION, then sizeof of sh_segment, sh_partial,
 * sh_envelope, sh_voice, sh_devinfo, sh_counters.  Writes min(n, 7) words, returns 7.  Callable before sh_init, without a GPU. */
#define SH_ABI_VERSION 6
int  sh_abi(uint32_t* out, int n);
int  sh_sync(void);                       /* wait for the stream */

/* What the library did behind the caller's back since sh_init: driver allocations (hipMalloc: pool misses, growing blocks),
 * driver frees, host-side stream synchronisations it inserted on its own (NOT the caller's sh_sync / downloads / timers), and
 * buffers served from the pool.  A streaming caller in its steady state -- blocks of lengths it has rendered before, buffers
 * of sizes it has used before -- must leave the first three unchanged (tests/test_gpu_pipeline.py asserts it).  Then which shape
 * the bank renders took: launches cut into segments at shared envelope corners (RENDER_*_SEG), launches classified per (voice,
 * tile) (RENDER_*_TILES: banks whose notes do not move in lock-step), and of those the ones whose tile set had been resolved
 * two launches ahead -- so that a test can tell that the path it means to exercise is the one that ran. */
typedef struct sh_counters {
    uint64_t device_allocs, device_frees, stream_syncs, pool_hits;
    uint64_t segmented_launches, tiled_launches, tiled_predicted;
} sh_counters;
int  sh_debug_counters(sh_counters* out);

/* Measurement knobs: environment variables read ONCE, by sh_init.  None changes a result -- they choose between schedules of the same
 * arithmetic, so that A/B timings can be taken with one library (tests/test_gpu_pipeline.py::test_knobs_change_no_result).  The
 * fifteen others that rounds 1-3 accumulated selected paths that had lost their A/B and were removed with those paths in
 * round 4 (CHANGELOG.md keeps what each measured):
 *   SYNTHHIP_NO_OVERLAP=1         consecutive renders of a bank stay on one stream
 *   SYNTHHIP_NO_SPECULATION=1     launch records by a prepare kernel in front of every render (no records two launches ahead)
 *   SYNTHHIP_NO_SMALL_PIPELINE=1  single-group (small) banks render on one stream; several-group banks still alternate
 *   SYNTHHIP_NO_SPLIT=1           lean and general code in one render kernel (k_render_combined) instead of k_render_lean + k_render_general
 *   SYNTHHIP_NO_SEG=1             transition launches / the heads of materialised rows are not cut into segments
 *   SYNTHHIP_NO_TILES=1           banks whose notes do not move in lock-step (onsets, envelopes of their own) are not classified tile
 *                                 by tile: every voice that holds an onset or a corner in the launch takes the general code
 *   SYNTHHIP_VARIANT=WFM          render kernel shape: waves per workgroup, frames per lane, min waves per SIMD -- one of 4163, 484, 444,
 *                                 844, 821, 421, 211 (the shapes the library chooses between by itself; 4163 -- sixteen frames per lane --
 *                                 exists for split launches of polynomial-Harmonics banks and of FM Sine banks only)
 *   SYNTHHIP_GROUPS=n             voice groups of a render launch
 *   SYNTHHIP_POOL_FILL=0..255     device blocks that grow are filled with this byte first (diagnostics: a kernel that reads what it
 *                                 should have written shows)
 *   (round 6)
 *   SYNTHHIP_SELF=1|2|3           a render that stands alone resolves its records (1, 3) / folds its partial buses (1, 2) inside its one kernel
 *                                 (off: measured slower, profiles/r06_run_lengths.txt)
 *   SYNTHHIP_NO_LADDER=1          a render launch that nothing runs beside keeps its wavefronts at one priority (default: the priority falls as a
 *                                 wavefront gets on with its voice lists, profiles/r06_prio_ladder.txt)
 *   SYNTHHIP_RT_CUS=n             the last n compute units are kept for real-time lanes (sh_rt_*); 0 = off (profiles/r06_rt_lane.txt)
 *   SYNTHHIP_NO_PERIOD=1          16-bit mono resampling between rates with a short period (reduced outrate <= 2048: 44.1 / 48 / 96 kHz ...)
 *                                 goes through k_resample_small like any other pair of rates, not through k_resample_period_i16
 *   SYNTHHIP_PERIOD_CHUNKS=n      consecutive chunks per workgroup of k_resample_period_i16 (default: 1, 2 or 4 by the rates' ratio;
 *                                 profiles/r06_resample_period.txt)
 *   SYNTHHIP_SEQ_ALIGN=1          the 16-bit sequence kernels read an event's misaligned samples through a vector type of alignment 2 instead of
 *                                 two aligned 16-byte loads and a funnel shift (profiles/sequence_ab.txt)
 * (SYNTHHIP_LIB, read by the Python binding, names another build of this library to load; SYNTHHIP_ALLOW_STALE=1 lets it load a
 * library whose sources have changed when rebuilding fails.) */

/* Readings of the recalled reference arithmetic that the DEVICE has to know about (the others are host-side choices of
 * synthesizer_amd/params.py `variants`: increments, Square as a Pulse record, pulse widths, envelope boundaries -- they change the records,
 * not the kernels).  SH_OPT_QUANTISE_ROUND: 0 (default) Sample.from_osc_block quantises int(scale * v), truncation toward zero;
 * 1: round(scale * v), half to even (Python 3's round) -- sh_quantize_f32 / sh_quantize_f64 follow it (the saturating [SPEC] forms,
 * sh_quantize_clip_f32 and sh_bank_render_pcm, and the fused sh_bank_generate_i16 do not: under 1 the latter refuses and the caller
 * quantises float64 rows).  Process-wide, like the stream.  Returns SH_ERR_INVALID for an unknown option. */
typedef enum sh_option { SH_OPT_QUANTISE_ROUND = 1,
                         SH_INFO_LAST_MIXDOWN_FUSED = 2   /* read-only (sh_get_option): how many stretches of the last sh_bank_mixdown_i16
                                                           * call were folded where the samples are made (0: all through int16 rows) */
} sh_option;
int  sh_set_option(int option, int value);
int  sh_get_option(int option);

/* ---- device buffers ---------------------------------------------------------------- */
int    sh_buf_alloc(size_t bytes, sh_buf** out);
int    sh_buf_free(sh_buf* b);
/* a non-owning window [offset, offset+bytes) of `parent` (must be freed before the parent) */
int    sh_buf_view(sh_buf* parent, size_t offset, size_t bytes, sh_buf** out);
size_t sh_buf_size(const sh_buf* b);
void*  sh_buf_devptr(sh_buf* b);
int    sh_buf_upload(sh_buf* b, size_t offset, const void* host, size_t bytes);
int    sh_buf_download(const sh_buf* b, size_t offset, void* host, size_t bytes);
int    sh_buf_fill_zero(sh_buf* b, size_t offset, size_t bytes);
int    sh_buf_copy(sh_buf* dst, size_t dst_off, const sh_buf* src, size_t src_off, size_t bytes);

/* ---- timing (HIP events on the library's stream) ------------------------------------ */
int  sh_timer_start(void);
int  sh_timer_stop(float* elapsed_ms);    /* records, synchronises, returns elapsed */

/* ---- voice bank: the voice table (oscillator parameters + phase tables) resident in HBM.
 *      A bank of ONE voice backs a Python Oscillator object; a bank of N voices backs the
 *      mixer sum bus over oscillator voices. ------------------------------------------- */
int sh_bank_create(const sh_voice* voices, uint32_t nvoices,
                   const sh_segment* segs, uint32_t nsegs,
                   const double* coefs, uint32_t ncoefs,
                   const sh_partial* partials, uint32_t npartials,
                   sh_bank** out);
int sh_bank_destroy(sh_bank* b);
uint32_t sh_bank_nvoices(const sh_bank* b);
/* How the last sh_bank_render launch classified the voices: *nfast took the lean loop (polynomial Harmonics, no FM,
 * constant envelope over the launch, one phase-table piece), *ngeneral the general code; voices released before the
 * launch are in neither count.  Synchronises the stream.  (A tile-classified launch -- a table of notes -- classifies per (voice, tile),
 * not per voice: both counts are 0; sh_debug_counters tells which shape a launch took.) */
int sh_bank_launch_stats(sh_bank* bank, uint32_t* nfast, uint32_t* ngeneral);

/* ---- oscillators: replaces Oscillator.blocks() of Sine/Sawtooth/Square/Pulse/Harmonics
 *      (+fm_lfo, +pwm_lfo) and EnvelopeFilter.blocks() ---------------------------------
 * Renders samples [start, start+n) of voice `voice` of the bank.  The call is stateless: the
 * reference's generator state is (sample index, accumulated t), and the phase tables
 * reproduce the accumulated t from the index.
 *   fm_cumsum    SH_FM_BUFFER voices: device buffer of >= n doubles, L(start) .. L(start+n-1)
 *                (L(m) = sum_{j<m} lfo_j, see sh_scan_f64); else NULL
 *   pwm          Pulse with pwm_lfo: device buffer of n doubles (pulse width per sample); else NULL
 *   out_host     host destination, n floats, or NULL
 *   out_f32/off  device destination (float index `off`), or NULL
 *   out_f64      device destination receiving the samples as float64 (modulators), or NULL
 */
int sh_osc_render(sh_bank* bank, uint32_t voice,
                  const sh_buf* fm_cumsum, const sh_buf* pwm,
                  uint64_t start, uint32_t n,
                  float* out_host, sh_buf* out_f32, size_t out_off, sh_buf* out_f64);

/* ---- filters over rendered oscillator blocks: MixingFilter (a+b),
 *      AmpModulationFilter (a*b), ClipFilter (max(min(a, p1), p0)), AbsFilter (|a|), copy / constant fill.
 *      CLIP follows Python's min and max, which keep their FIRST argument on a tie and when a NaN makes the comparison false:
 *      t = p1 < a ? p1 : a, then p0 > t ? p0 : t -- clip(-0.0, 0.0, 1.0) is -0.0 and a NaN sample stays NaN.
 *      a, b, out_f64: float64 device buffers; out_f32 (+ element offset) / out_host: optional float32 copies */
typedef enum sh_ew_op { SH_EW_ADD = 0, SH_EW_MUL = 1, SH_EW_CLIP = 2, SH_EW_ABS = 3, SH_EW_COPY = 4, SH_EW_FILL = 5,
                        SH_EW_AXPY = 6 /* a + b*p0 (product rounded first): EchoFilter */,
                        SH_EW_NEXTUP = 7 /* the float64 successor of a: pulse widths under the `<=` reading (below) */ } sh_ew_op;
int sh_ew_f64(int op, const sh_buf* a, size_t a_off, const sh_buf* b, size_t b_off, size_t n, double p0, double p1,
              sh_buf* out_f64, size_t out64_off, sh_buf* out_f32, size_t out32_off, float* out_host);

/* exclusive running sum of n float64 values on the device (FM with an arbitrary fm_lfo):
 * out[i] = carry_in + x[0] + .. + x[i-1], i = 0..n-1 (n values).
 * carry_out (host, may be NULL) receives carry_in + x[0] + .. + x[n-1].
 * Error bound (sh_scan_rows_f64 alike): |out[i] - exact| <= K 2^-53 (|carry_in| + |x[0]| + .. + |x[i-1]|), K = 31 + ceil(ceil(n / 2048) / 256),
 * the rounded additions on the longest path from an input to an output; out[i] holds no part of x[i] or of anything behind it.
 * carry_out: the same with K = 23 + ceil(ceil(n / 2048) / 256) over all n values. */
int sh_scan_f64(const sh_buf* x, uint32_t n, double carry_in, sh_buf* out, double* carry_out);

/* ---- voice bank rendering: N voices -> stereo bus (the "Mixer sum bus" over oscillator voices) */
/* materialise: voices_out[v*stride + i] = voice v at frame start+i (float32, voice-major); nframes <= 2^32 - 65536 */
int sh_bank_generate(sh_bank* b, uint64_t start, uint32_t nframes, sh_buf* voices_out, size_t stride);
/* fused generate-and-mix: bus_f32[i] = (sum_v gl_v x_v[i], sum_v gr_v x_v[i]), float32 x2 interleaved.
 * bus_f64 (optional) receives the float64 partial bus (frames x 2) used for the multi-GPU reduce.
 * Work is enqueued like every other call.  One detail matters to code that reads the bus buffers with its OWN
 * kernels through sh_buf_devptr: consecutive renders of a bank (same block length, the next block each time) form a
 * run that is pipelined (every bank has its own: banks rendering turn by turn do not end each other's runs) -- they
 * alternate between two HIP streams so that one launch fills the tail of the other, and
 * with several voice groups the last step of a render (folding the groups' partial buses into the bus) is done inside
 * the render kernel two launches later.  Any other call into the library (sh_sync, sh_buf_download, sh_buf_free, ...;
 * not sh_buf_alloc) ends the run first: it joins the streams and folds what is outstanding -- so such code must call
 * sh_sync() (or any other entry point) before touching the buffers.  Everything inside the library sees completed
 * buses.  To keep a run going while consuming its output, render into a ring of bus buffers and read a buffer only
 * after the run has been ended.
 * Any nframes is accepted: renders beyond 2^22 frames are carried out as a run of launches of 2^22 frames each into
 * consecutive parts of the buffers (a launch's grid holds fewer than 2^32 work-items per dimension, and the partial
 * buses of the voice groups are sized per launch). */
int sh_bank_render(sh_bank* b, uint64_t start, uint32_t nframes, sh_buf* bus_f32, sh_buf* bus_f64);
/* The same render delivered as saturated int16 stereo PCM (frames x 2, interleaved): sample = trunc(scale * bus) of the
 * float32 bus, clamped to the int16 range -- exactly what sh_quantize_clip_f32 makes of sh_bank_render's bus_f32 -- but
 * produced by the fold of the partial buses itself, so a stream of PCM blocks (what a player consumes: upstream's
 * synth -> Sample.from_osc_block -> mixer route) stays on the two-stream pipeline described above instead of ending
 * the run with a quantise kernel after every block.  The same rule about reading the buffer applies. */
int sh_bank_render_pcm(sh_bank* b, uint64_t start, uint32_t nframes, double scale, sh_buf* pcm_i16);

/* A run of blocks per call: blocks k = 0 .. nblocks - 1 of nframes frames each, block k = frames [start + k nframes, +nframes),
 * into bus_f32[k % nring] (float32 stereo) and / or pcm_i16[k % nring] (saturated int16 stereo, as sh_bank_render_pcm) -- what a
 * caller streaming blocks through a ring of buffers does with one sh_bank_render per block, with ONE crossing of the ABI, one
 * acquisition of the library's lock, and ONE LAUNCH for every stretch of blocks whose ring buffers lie back to back in memory
 * (windows of one allocation, sh_buf_view): a launch costs the host 2-4 us whatever it renders, and a small bank's one-second block
 * costs the device less (BASELINE config 2: 64 voices).  Blocks of a merged stretch are one render of the whole stretch: the same
 * samples as block-by-block renders up to the float64 summation order of the voice groups (a longer launch may use fewer groups).
 * Either ring may be NULL (not both).  The rule about reading the buffers is sh_bank_render's. */
int sh_bank_render_run(sh_bank* b, uint64_t start, uint32_t nframes, uint32_t nblocks, sh_buf* const* bus_f32, sh_buf* const* pcm_i16,
                       uint32_t nring, double pcm_scale);

/* ---- banks whose voices are modulated by arbitrary oscillators (fm_lfo= / pwm_lfo= any Oscillator, upstream oscillators.py)
 *      or ARE arbitrary oscillator graphs (filters): the modulators / sources are rendered as float64 rows of one matrix
 *      [row][row_stride] (launch-relative: element i = frame start + i) and the bank's general code reads them.
 * sh_bank_set_rows: per voice, the row holding L(start + i) = running sum of its fm_lfo (SH_FM_BUFFER voices) or its samples
 *   (SH_BUFFER voices) in fm_row, the row holding its pulse width per sample in pwm_row (Pulse with a pwm_lfo); -1 = none.
 * sh_bank_generate_f64: every voice of a bank of closed-form oscillators as float64 rows row0 .. row0 + nvoices - 1 (one launch
 *   for all the modulators of a bank).
 * sh_scan_rows_f64: rows row0 .. row0 + nrows - 1 replaced by their exclusive running sums, row r continuing from carry[r]
 *   (device buffer of nrows doubles, updated to the carry-out: consecutive blocks chain without a host round trip).
 * sh_bank_render_rows: sh_bank_render with that matrix. */
int sh_bank_set_rows(sh_bank* b, const int32_t* fm_row, const int32_t* pwm_row);
int sh_bank_generate_f64(sh_bank* b, uint64_t start, uint32_t nframes, sh_buf* rows_out, size_t row0, size_t row_stride);
int sh_scan_rows_f64(sh_buf* rows, size_t row0, uint32_t nrows, uint32_t n, size_t row_stride, sh_buf* carry);
int sh_bank_render_rows(sh_bank* b, uint64_t start, uint32_t nframes, const sh_buf* rows_f64, size_t row_stride,
                        sh_buf* bus_f32, sh_buf* bus_f64);
/* sh_bank_generate (the reference-shaped two-step route: every voice as a float32 row) for such a bank */
int sh_bank_generate_rows(sh_bank* b, uint64_t start, uint32_t nframes, const sh_buf* rows_f64, size_t row_stride,
                          sh_buf* voices_out, size_t stride);

/* The reference-shaped INTEGER route (upstream synthplayer/sample.py Sample.from_osc_block, [RECALL]: one oscillator block ->
 * int(amplitude_scale * v) per sample through array('h'), OverflowError where a value does not fit): every voice of the bank as a
 * row of int16 PCM, voices_out[v*stride + i] = int(scale * x_v[start + i]) -- the float64 sample, the float64 product, truncation
 * toward zero -- made where the sample is made: 2 bytes per voice-sample reach HBM instead of a float row (4 written) that a
 * quantise pass re-reads (4) and re-writes (2).  The rows are what sh_mix_chain_i16 / sh_mix_chain_pan_i16 fold (the mixer's
 * audioop.add chain).  stride must be even (rows are written as 32-bit pairs).  SH_ERR_OVERFLOW when a sample of ANY voice does not
 * fit (the rows are unspecified then); the call synchronises to learn it, like the quantisers.  _rows_: the same for a bank with
 * modulation rows (sh_bank_set_rows). */
int sh_bank_generate_i16(sh_bank* b, uint64_t start, uint32_t nframes, double scale, sh_buf* voices_out, size_t stride);
/* The streaming form: enqueues the same work and returns; a sample that does not fit raises a flag on the device that stays up until
 * sh_overflow_check() -- which waits for the stream, returns SH_ERR_OVERFLOW if any sh_bank_generate_i16_async since the last
 * check met one, and lowers the flag -- is called: once per batch of blocks instead of a host round trip per block.  The flag is
 * ONE word per process: the synchronous forms (sh_bank_generate_i16, sh_bank_mixdown_i16) read and lower it too, so a synchronous
 * call consumes -- and reports as its own -- an overflow still pending from an _async call of any bank; a synchronous call that
 * fails with another error lowers it as well, so that nothing it raised is left for the next call. */
int sh_bank_generate_i16_async(sh_bank* b, uint64_t start, uint32_t nframes, double scale, sh_buf* voices_out, size_t stride);
int sh_overflow_check(void);
/* The MONO mixdown the reference's mixer makes of the bank -- every voice quantised like sh_bank_generate_i16, then mixed =
 * audioop.add(mixed, voice, 2) down the voices in order -- without the rows: out[i], nframes int16 samples, equal byte for byte to
 * sh_mix_chain_i16 of sh_bank_generate_i16's rows.  Where every voice of a 65 536-frame stretch takes the lean polynomial-Harmonics loop
 * the samples enter the chain where they are made (a saturating chain over a range of voices is the map x -> clamp(x + a, L, U); such
 * maps compose in voice order: the kernel leaves one per frame and (64-voice chunk, half), a second small kernel applies them); the
 * other stretches go through int16 rows in a temporary and the chain kernel.  SH_ERR_OVERFLOW / _async / sh_overflow_check: as above. */
int sh_bank_mixdown_i16(sh_bank* b, uint64_t start, uint32_t nframes, double scale, sh_buf* out_i16);
int sh_bank_mixdown_i16_async(sh_bank* b, uint64_t start, uint32_t nframes, double scale, sh_buf* out_i16);
int sh_bank_generate_rows_i16(sh_bank* b, uint64_t start, uint32_t nframes, const sh_buf* rows_f64, size_t row_stride,
                              double scale, sh_buf* voices_out, size_t stride);

/* ---- chain maps: the mixer's saturating chain over a RANGE of voices, as a value ------------------------------------------
 * mixed = audioop.add(mixed, voice, 2) down a range of voices is, per int16 value, the map x -> clamp(x + add, lo, hi).  One map
 * per value, 8 bytes (int32 add; int16 lo; int16 hi -- as a pair of int32: .x = add, .y = lo | hi << 16, little-endian).  A mono
 * block has nframes maps, a stereo block 2 * nframes, interleaved L / R like the samples.  Identity: (0, -32768, 32767); the
 * map of one voice sample s: (s, -32768, 32767).  f then g: (a1 + a2, clamp(lo1 + a2, lo2, hi2), clamp(hi1 + a2, lo2, hi2)).
 * Applied in voice order to silence the maps of a table's consecutive ranges give the chain over the whole table; applied to x0
 * they give audioop.add(x0, voice0), then voice1, ... -- the chain continued from an existing sample.
 * add saturates at +-2^17 (SH_CHAIN_ADD_MAX) everywhere the library makes or reads a map: for |add| >= 65535 every int16 x
 * already lands on lo or hi, so the map on int16 inputs is the same, and any count of voices or parts stays inside int32. */
typedef struct sh_chain_map {
    int32_t add;
    int16_t lo;
    int16_t hi;
} sh_chain_map;
#define SH_CHAIN_ADD_MAX 131072
/* sh_bank_mixdown_i16 (same voices, quantiser, boundary guard and choice of route per 65 536-frame stretch, same 32 768-voice
 * limit) ending in the composed map of the bank's voices per frame: parts_out holds nframes sh_chain_map.  _async / overflow
 * semantics as sh_bank_mixdown_i16. */
int sh_bank_mixdown_i16_parts(sh_bank* b, uint64_t start, uint32_t nframes, double scale, sh_buf* parts_out);
int sh_bank_mixdown_i16_parts_async(sh_bank* b, uint64_t start, uint32_t nframes, double scale, sh_buf* parts_out);
/* sh_mix_chain_i16 / sh_mix_chain_pan_i16 ending in the composed map per sample (parts_out: nsamples, resp. 2 * nframes, maps). */
int sh_mix_chain_i16_parts(const sh_buf* chunks, uint32_t nvoices, size_t stride, uint32_t nsamples, sh_buf* parts_out);
int sh_mix_chain_pan_i16_parts(const sh_buf* chunks, uint32_t nvoices, size_t stride, uint32_t nframes, const sh_buf* factors_lr,
                               sh_buf* parts_out);
/* nparts planes of nvalues maps each, plane k at parts[k * part_stride ..] (in maps), in order: composed into one map per value
 * (out_parts may be plane 0 itself), or applied to x0 (nvalues int16; NULL: silence) into out_i16.  nparts == 0: the identity. */
int sh_chain_parts_compose(const sh_buf* parts, uint32_t nparts, size_t part_stride, uint32_t nvalues, sh_buf* out_parts);
int sh_chain_parts_apply(const sh_buf* parts, uint32_t nparts, size_t part_stride, uint32_t nvalues, const sh_buf* x0_i16,
                         sh_buf* out_i16);

/* ---- mixer sum bus over materialised voices ------------------------------------------ */
/* float32: bus[i] = sum_v gains[v] * voices[v*stride+i]; gains = device buffer of nvoices x (l, r) floats; one fmaf per term,
 * the order of the sum is the launch plan's (csrc/mixbus_plan.hpp).  Reads (nvoices - 1) * stride + nframes floats of `voices` (the
 * floats between frame nframes of a row and the next row are never read), writes the first nframes * 8 bytes of bus_f32 and nothing
 * else.  Pointers (buffers and sh_buf_view windows alike): voices and bus_f32 need their natural alignment only (4 and 8 bytes) -- a
 * call with both on the 16-byte grid and stride % 4 == 0 takes the vector kernels, any other call gives the same sums without a
 * 16-byte access; gains_lr must be 8-byte aligned (read as float2).  SH_ERR_INVALID, before any launch: a NULL argument,
 * nvoices == 0, stride < nframes, voices shorter than the floats read, bus_f32 shorter than nframes * 8 bytes, gains_lr shorter than
 * nvoices * 8 bytes or off the 8-byte grid.  nframes == 0: SH_OK, nothing written. */
int sh_mix_bus_f32(const sh_buf* voices, uint32_t nvoices, size_t stride, uint32_t nframes,
                   const sh_buf* gains_lr, sh_buf* bus_f32);
/* integer: the reference mixer's fold, mixed = add(add(c0, c1), c2) ... in voice order,
 * saturating at every step (playback.py mixer loop -> audioop.add).  chunks[v*stride + i] int16. */
int sh_mix_chain_i16(const sh_buf* chunks, uint32_t nvoices, size_t stride, uint32_t nsamples, sh_buf* out);
/* The same fold over MONO voice rows that enter it as Sample.stereo(left_factor, right_factor) of themselves (upstream
 * synthplayer/sample.py Sample.stereo -> audioop.tostereo(frames, 2, lf, rf), [RECALL]): out frame i = (L, R) with
 * L = add(add(tostereo_l(c0), tostereo_l(c1)), ...) -- per voice and channel fbound(sample * factor) (clamp, then floor), then the
 * saturating chain in voice order.  The stereo rows are never materialised: 2 bytes are read per voice-sample, 4 written per frame.
 * factors_lr: device buffer of nvoices x (left, right) doubles, 8-byte aligned (a view 2 or 4 bytes off that grid: SH_ERR_INVALID,
 * here and in the _parts form).  chunks[v*stride + i] int16 mono; out: nframes x 2 int16. */
int sh_mix_chain_pan_i16(const sh_buf* chunks, uint32_t nvoices, size_t stride, uint32_t nframes, const sh_buf* factors_lr, sh_buf* out);
/* The same fold with every chunk read where its sample lives (no staging copy): source v contributes
 * srcs[v][sample_offsets[v] .. +nsamples_each[v]) and silence after that, up to nsamples; the result goes to
 * out[out_sample_off ..).  This is one turn of the real-time mixer's chunk loop (upstream synthplayer/playback.py
 * RealTimeMixer.chunks, [RECALL]: next(chunk) of every active sample, short chunks padded with silence, then
 * mixed = audioop.add(mixed, chunk, 2) in the order the samples were added).  An in-place source (out among srcs)
 * is not allowed. */
int sh_mix_chain_gather_i16(const sh_buf* const* srcs, const size_t* sample_offsets, const uint32_t* nsamples_each, uint32_t nsrc,
                            uint32_t nsamples, sh_buf* out, size_t out_sample_off);

/* The same two folds for every sample width audioop.add takes (1, 2, 3, 4 bytes; offsets, strides and counts in SAMPLES;
 * width 2 = the two functions above): upstream's mixer calls audioop.add(mixed, chunk, samplewidth) with the width of its
 * output format, which need not be 16 bits. */
int sh_mix_chain(const sh_buf* chunks, uint32_t nvoices, size_t stride, uint32_t nsamples, int width, sh_buf* out);
int sh_mix_chain_gather(const sh_buf* const* srcs, const size_t* sample_offsets, const uint32_t* nsamples_each, uint32_t nsrc,
                        uint32_t nsamples, int width, sh_buf* out, size_t out_sample_off);

/* ---- a list of placed samples mixed into a track ---------------------------------------------------------------------------------
 * Replaces: a loop of Sample.mix_at(seconds, other.at_volume(volume), other_seconds) calls (upstream synthplayer/sample.py, [RECALL];
 * what its track-mixer example and Sample.echo do) -- one launch over one short region per call, plus a copy of the whole track
 * whenever it grows.  Per event audioop.mul(frames, width, factor) (fbound: clamp, then floor) of srcs[src][src_sample .. +nsamples),
 * then audioop.add into track[dst_sample ..) with saturation AT EVERY EVENT, IN LIST ORDER: the same bytes as the loop.  One launch;
 * tiles of the track that no event touches are neither read nor written. */
typedef struct sh_mix_event {      /* one placed sample; all positions in SAMPLES (not frames, not bytes) */
    uint64_t dst_sample;           /* where in the track its first sample lands */
    uint64_t src_sample;           /* first sample taken from the source buffer */
    uint64_t nsamples;             /* may be 0 */
    double   factor;               /* audioop.mul factor; exactly 1.0 = none */
    uint32_t src;                  /* index into srcs */
    uint32_t reserved;             /* 0 */
} sh_mix_event;                    /* 40 bytes */
/* track[0 .. track_samples) = the events applied in order, in place.  No src may be `track`.  SH_ERR_INVALID, and nothing launched,
 * for: a source index >= nsrc, a range outside its source or the track, a non-finite factor, reserved != 0, a width other than
 * 1 - 4, a source that is (or overlaps) the track, more than 2^32 - 65536 track samples.  "The track" is the bytes of its first
 * track_samples samples: a source that is a view of the same allocation in front of them or behind them does not overlap it. */
int sh_mix_events(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event* events, uint32_t nevents,
                  int width, sh_buf* track, size_t track_samples);

/* The same with a playback speed per event: a sampler -- one recorded note at many pitches -- in one launch.
 * Replaces: per note, Sample.copy().speed(s) (upstream synthplayer/sample.py, [RECALL]: audioop.ratecv(frames, width, nchannels,
 * int(rate * s), rate, None)), .at_volume(v) and mix_at(...): four to six launches and three allocations for a few thousand frames.
 * An event with inrate != outrate contributes audioop.ratecv(srcs[src][src_sample .. + src_frames * nchannels), width, nchannels,
 * inrate, outrate) from its output frame 0 on -- its first nsamples samples, THEN audioop.mul by factor, then the saturating add, in
 * that order (mul and ratecv do not commute).  The resampled source is never materialised: the lane that owns a track sample forms
 * the output frame that lands there from two input frames.  inrate == outrate is a plain event of sh_mix_events (src_frames ignored);
 * a list may hold both kinds. */
typedef struct sh_mix_event_rate { /* all positions in SAMPLES unless named frames */
    uint64_t dst_sample;           /* where in the track its first sample lands */
    uint64_t src_sample;           /* first sample of the source buffer the event may read (resampled: input frame 0) */
    uint64_t nsamples;             /* samples landing in the track -- RESAMPLED samples for a resampled event; may be 0 */
    uint64_t src_frames;           /* resampled: input frames the event may read from src_sample on */
    double   factor;               /* audioop.mul factor, applied after the resample; exactly 1.0 = none */
    uint32_t src;                  /* index into srcs */
    uint32_t inrate, outrate;      /* audioop.ratecv's; equal: a plain event */
    uint32_t reserved;             /* 0 */
} sh_mix_event_rate;               /* 56 bytes */
/* SH_ERR_INVALID, and nothing launched, for everything sh_mix_events refuses, and: a rate of 0 or >= 2^31, nchannels < 1; for a
 * resampled event src_sample or nsamples not a multiple of nchannels, src_frames beyond the source, nsamples beyond the
 * sh_resample_out_frames(src_frames, inrate, outrate) * nchannels samples that src_frames yield. */
int sh_mix_events_rate(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event_rate* events, uint32_t nevents,
                       int width, int nchannels, sh_buf* track, size_t track_samples);

/* The same into a STEREO track, with a place in the stereo field per event: mono one-shots and mono recorded notes panned into a stereo
 * master -- a drum machine, a tracker -- in one launch.
 * Replaces: per note, Sample.copy().speed(s).pan(p) or .stereo(left, right) (upstream synthplayer/sample.py, [RECALL]:
 * audioop.tostereo(frames, width, left, right) of the mono frames), .at_volume(v) and mix_at(...): six to eight launches and four
 * allocations; or a stereo copy of the instrument per (instrument, speed, pan), which reads twice the source bytes per event.
 * An event with src_channels == 1 contributes, in this order (none of the steps commute): audioop.ratecv of the MONO frames
 * srcs[src][src_sample .. + src_frames) when inrate != outrate, audioop.tostereo of the result -- frame f becomes
 * (fbound(s * left), fbound(s * right)), fbound: clamp, then floor -- its first nsamples STEREO samples, audioop.mul by factor, the
 * saturating add.  Neither the resampled nor the stereo source is materialised: the lane that owns a track frame forms it from one
 * (plain) or two (resampled) mono input frames.  An event with src_channels == 2 is an event of sh_mix_events_rate with nchannels == 2,
 * left and right ignored; a list may hold both kinds, plain and resampled. */
typedef struct sh_mix_event_pan {  /* all positions in SAMPLES unless named frames; a mono source's samples are its frames */
    uint64_t dst_sample;           /* where in the track its first sample lands; mono source: even (a left sample) */
    uint64_t src_sample;           /* first sample of the source buffer the event may read (resampled: input frame 0) */
    uint64_t nsamples;             /* samples landing in the TRACK (mono source: two per source or resampled frame, so even); may be 0 */
    uint64_t src_frames;           /* resampled: input frames the event may read from src_sample on */
    double   factor;               /* audioop.mul factor, applied after tostereo; exactly 1.0 = none */
    double   left, right;          /* mono source: audioop.tostereo's factors */
    uint32_t src;                  /* index into srcs */
    uint32_t inrate, outrate;      /* audioop.ratecv's; equal: a plain event */
    uint32_t src_channels;         /* 1: a mono source through tostereo; 2: a stereo source, as sh_mix_events_rate has it */
    uint32_t reserved;             /* 0 */
} sh_mix_event_pan;                /* 80 bytes */
/* The track is stereo.  SH_ERR_INVALID, and nothing launched, for everything sh_mix_events_rate refuses (nchannels = src_channels), and:
 * src_channels other than 1 or 2; for a mono source a non-finite left or right, an odd dst_sample or nsamples, nsamples / 2 beyond the
 * source's samples from src_sample on (plain) or beyond the sh_resample_out_frames(src_frames, inrate, outrate) frames that src_frames
 * yield (resampled). */
int sh_mix_events_pan(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event_pan* events, uint32_t nevents,
                      int width, sh_buf* track, size_t track_samples);

/* The same with an ADSR envelope per event: a recorded or looped instrument played at a chosen length gets an attack and a release --
 * shaped notes, one launch per track.
 * Replaces: per note, Sample.copy().speed(s), .clip(0, length), .envelope(attack, decay, sustainlevel, release) (upstream
 * synthplayer/sample.py, [RECALL]: split, audioop.mul of the sustain and release parts, fadein / fadeout -- int(x * f) per sample
 * through array -- and join), .stereo(left, right), .at_volume(v) and mix_at(...): some fifteen launches and ten allocations.
 * An event with seg_count > 0 is shaped after the ratecv and the cut and BEFORE tostereo and the mul: source sample p of the event (the
 * p-th sample it takes of its plain or resampled source; a mono source of a stereo track: its p-th frame) lies in the first of its
 * segments segments[seg_first .. + seg_count) whose end is > p and becomes
 *     x = fbound(x * mul)                                        unless mul == 1.0       (audioop.mul: clamp, then floor)
 *     x = trunc(x * (1.0 - (p - origin) * slope / numsamples))   kind 2, a fade-out      (float64, in this order, each step rounded)
 *     x = trunc(x * ((p - origin) * slope / numsamples + offset)) kind 1, a fade-in
 * and stays as it is past the last end.  The caller replays Sample.envelope's boundaries; nothing is materialised.  src_channels is the
 * source's channel count: nchannels, the track's -- an event of sh_mix_events_rate -- or 1 with nchannels == 2 -- a mono source through
 * tostereo, as sh_mix_events_pan has it.  An event with seg_count == 0 has no envelope; a list may hold every kind. */
typedef struct sh_env_segment {    /* positions in the event's source samples */
    uint64_t end;                  /* the segment is [the end of the one before it (0 for the first), end) */
    uint64_t origin;               /* where a ramp's k == 0 */
    double   mul;                  /* audioop.mul factor before the ramp; exactly 1.0 = none */
    double   slope;                /* a ramp's: fade-in 1 - start volume, fade-out 1 - target volume */
    double   numsamples;           /* a ramp's: samples of the whole faded stretch, > 0 */
    double   offset;               /* a fade-in's start volume */
    uint32_t kind;                 /* 0: no ramp, 1: fade-in, 2: fade-out */
    uint32_t reserved;             /* 0 */
} sh_env_segment;                  /* 56 bytes */
typedef struct sh_mix_event_env {  /* sh_mix_event_pan's fields, then the segments */
    uint64_t dst_sample;
    uint64_t src_sample;
    uint64_t nsamples;
    uint64_t src_frames;
    double   factor;
    double   left, right;
    uint32_t src;
    uint32_t inrate, outrate;
    uint32_t src_channels;         /* nchannels, or 1 into a stereo track: through tostereo */
    uint32_t seg_first;            /* index into segments */
    uint32_t seg_count;            /* 0: no envelope; at most 7 */
    uint32_t reserved;             /* 0 */
} sh_mix_event_env;                /* 88 bytes */
/* SH_ERR_INVALID, the event named and nothing launched, for everything sh_mix_events_pan refuses (sh_mix_events_rate for src_channels ==
 * nchannels), and: a width other than 1, 2 or 4 (upstream's fades have no 24-bit form), src_channels that is neither nchannels nor 1
 * into a stereo track, more than 7 segments, segments outside the table, ends that descend or lie beyond the event's source samples
 * (nsamples; a mono source of a stereo track: nsamples / 2), an origin beyond them, a kind other than 0 - 2, a non-finite mul, slope,
 * numsamples or offset, a ramp with numsamples <= 0, reserved != 0 in an event or a segment it names. */
int sh_mix_events_env(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event_env* events, uint32_t nevents,
                      const sh_env_segment* segments, uint32_t nsegments, int width, int nchannels, sh_buf* track, size_t track_samples);

/* The same with a sustain loop per event: a note longer than its recording -- a recorded instrument held until its release -- still in
 * one launch and without an unrolled copy per (instrument, length).
 * Replaces: per note, o = other.copy().clip(0, loop_end); body = other.copy().clip(loop_start, loop_end); while o.duration < length:
 * o.join(body); o.clip(0, length) in front of the loop body that sh_mix_events_env replaces.
 * An event with loop_frames > 0 plays src_frames VIRTUAL frames: virtual frame v is frame v of the source (counted from src_sample) while
 * v < loop_start + loop_frames, and frame loop_start + (v - loop_start - loop_frames) % loop_frames behind that.  The loop comes FIRST:
 * audioop.ratecv runs over the virtual frames (it interpolates across the seam, from the loop's last frame to its first; its output
 * count is that of src_frames input frames), then the cut, the envelope, tostereo, the mul and the saturating add as above.  A note with
 * src_frames <= loop_start + loop_frames is a plain cut.  An event with loop_frames == 0 is an event of sh_mix_events_env, loop_start
 * ignored; a list may hold every kind.  24-bit samples may loop (every step but the envelope has a 24-bit form). */
typedef struct sh_mix_event_loop { /* sh_mix_event_env's fields, then the loop */
    uint64_t dst_sample;
    uint64_t src_sample;
    uint64_t nsamples;
    uint64_t src_frames;           /* looped: the note's VIRTUAL frames, which may exceed the source's */
    double   factor;
    double   left, right;
    uint32_t src;
    uint32_t inrate, outrate;
    uint32_t src_channels;
    uint32_t seg_first;
    uint32_t seg_count;
    uint32_t reserved;             /* 0 */
    uint64_t loop_start;           /* first frame of the loop region, in frames from src_sample */
    uint64_t loop_frames;          /* frames of the loop region; 0: no loop */
} sh_mix_event_loop;               /* 104 bytes */
/* SH_ERR_INVALID, the event named and nothing launched, for everything sh_mix_events_env refuses -- its src_frames-beyond-the-source rule
 * holds for events without a loop; width 3 is refused only for an event with segments -- and for a looped event: loop_start +
 * loop_frames beyond the source's frames from src_sample on, src_sample or nsamples off whole frames, more samples than src_frames hold
 * (plain) or resample to (resampled), src_frames * src_channels above 2^32 - 65536. */
int sh_mix_events_loop(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event_loop* events, uint32_t nevents,
                       const sh_env_segment* segments, uint32_t nsegments, int width, int nchannels, sh_buf* track, size_t track_samples);

/* The same with a reversed event: a reversed cymbal at 300 places, or at several pitches, without a materialised reversed copy.  (A
 * REGION of a recording -- one hit out of a drum break, a recording whose attack is skipped -- needs nothing new: src_sample and
 * src_frames say it in every struct above.)
 * Replaces: o = other.copy().clip(start, end).reverse() (upstream synthplayer/sample.py, [RECALL]: audioop.reverse) in front of the loop
 * body that sh_mix_events_loop replaces.
 * An event with SH_MIX_EVENT_REVERSED set plays a region of its source backwards, FIRST in the chain: the region as stored, forwards, is
 * the R frames from src_sample on -- R = src_frames, or loop_start + loop_frames for a looped event (nothing behind the loop's end is
 * played, and its src_frames counts virtual frames) -- and played sample i is stored sample R * src_channels - 1 - i: audioop.reverse
 * turns the order of the SAMPLES round, so the frames come backwards and, in a stereo source, left and right change places.  Everything
 * sh_mix_event_loop says of frames (loop_start, loop_frames, src_frames, the input frames of audioop.ratecv, whose prev is 0 at the
 * first PLAYED frame) it says of the played ones.  An event without the flag is an event of sh_mix_events_loop; a list may hold every
 * kind. */
#define SH_MIX_EVENT_REVERSED 1u
typedef struct sh_mix_event_rev {  /* sh_mix_event_loop's fields, then the flags */
    uint64_t dst_sample;
    uint64_t src_sample;           /* reversed: the first STORED sample of the region, on a whole frame */
    uint64_t nsamples;
    uint64_t src_frames;           /* reversed and not looped: the region's frames, honoured for a plain event as well */
    double   factor;
    double   left, right;
    uint32_t src;
    uint32_t inrate, outrate;
    uint32_t src_channels;
    uint32_t seg_first;
    uint32_t seg_count;
    uint32_t reserved;             /* 0 */
    uint64_t loop_start;           /* in PLAYED frames */
    uint64_t loop_frames;
    uint32_t flags;                /* SH_MIX_EVENT_REVERSED; every other bit 0 */
} sh_mix_event_rev;                /* 112 bytes */
/* SH_ERR_INVALID, the event named and nothing launched, for everything sh_mix_events_loop refuses, and: a flag bit other than
 * SH_MIX_EVENT_REVERSED; for a reversed event a src_sample off whole frames, a region that reaches beyond its source, more samples than
 * the region holds (plain). */
int sh_mix_events_rev(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event_rev* events, uint32_t nevents,
                      const sh_env_segment* segments, uint32_t nsegments, int width, int nchannels, sh_buf* track, size_t track_samples);

/* The same with a STEREO source's two channels weighed per event: a stereo drum break in a mono track, a stereo pad set to one side of a
 * stereo track, without a converted copy per pair of factors.  This closes the channel matrix (mono into stereo: left / right of
 * sh_mix_events_pan).
 * Replaces: o = o.copy().mono(lf, rf) / o = o.copy().stereo(lf, rf) of a stereo o (upstream synthplayer/sample.py, [RECALL]:
 * audioop.tomono; left().amplify(lf) mixed with right().amplify(rf)) where sh_mix_events_pan's tostereo stands in the loop body: behind
 * the envelope, in front of audioop.mul.
 * The mode is a flag bit, said per event and never derived from the channel counts (a stereo row in a stereo track is a plain event
 * unless it says otherwise, and a row's meaning does not change with the call's nchannels):
 *   SH_MIX_EVENT_DOWNMIX  src_channels == 2, nchannels == 1.  dst_sample and nsamples count TRACK (mono) samples; track sample
 *                         dst_sample + f is floor(fbound(l * left + r * right)) of frame f of what the fields describe over the stereo
 *                         source -- src_sample, src_frames, the loop and a reversed region in stereo frames / samples as for any stereo
 *                         source, audioop.ratecv with two channels, the segments' ends and origins in stereo SAMPLES (2 per track sample).
 *                         A reversed source has left and right swapped BEFORE the factors.  Two products and a sum, three roundings.
 *   SH_MIX_EVENT_BALANCE  src_channels == 2, nchannels == 2.  An event of sh_mix_events_rev whose even samples then go through
 *                         fbound(x * left) and its odd ones through fbound(x * right); a factor of exactly 1.0 does nothing.
 * An event with neither bit is an event of sh_mix_events_rev (left / right are tostereo's for a mono source there); a list may hold every
 * kind. */
#define SH_MIX_EVENT_DOWNMIX 2u
#define SH_MIX_EVENT_BALANCE 4u
typedef struct sh_mix_event_chan { /* sh_mix_event_rev's layout */
    uint64_t dst_sample;
    uint64_t src_sample;
    uint64_t nsamples;             /* TRACK samples: a downmix takes 2 * nsamples of its (resampled) source */
    uint64_t src_frames;
    double   factor;
    double   left, right;          /* tostereo's, tomono's or the balance's factors */
    uint32_t src;
    uint32_t inrate, outrate;
    uint32_t src_channels;
    uint32_t seg_first;
    uint32_t seg_count;
    uint32_t reserved;             /* 0 */
    uint64_t loop_start;
    uint64_t loop_frames;
    uint32_t flags;                /* SH_MIX_EVENT_REVERSED | one of SH_MIX_EVENT_DOWNMIX, SH_MIX_EVENT_BALANCE; every other bit 0 */
} sh_mix_event_chan;               /* 112 bytes */
/* SH_ERR_INVALID, the event named and nothing launched, for everything sh_mix_events_rev refuses (a downmix's src_channels of 2 in a
 * mono track is none of it), and: a flag bit other than the three; both modes on one event; a mode on a source that is not stereo; a
 * downmix into a track that is not mono, a balance into one that is not stereo; a left or right that is not finite; a balance whose
 * dst_sample is odd; a downmix with dst_sample + nsamples > 2^31 - 32768 -- the kernels form its source-sample coordinates, twice the
 * track's, in 32 bits (the limit of the track itself stays 2^32 - 65536 samples). */
int sh_mix_events_chan(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event_chan* events, uint32_t nevents,
                       const sh_env_segment* segments, uint32_t nsegments, int width, int nchannels, sh_buf* track, size_t track_samples);

/* A song of placed samples compiled once and rendered window by window: the host work of sh_mix_events_chan -- checking the events,
 * filling the records, planning the tiles, copying the tables -- is paid by sh_seq_create, and sh_seq_render is one launch that copies
 * nothing.  Every track sample is a fold over the events that cover it, in list order, and every step of an event's chain is evaluated
 * from the sample's position inside the event, so a window rendered alone holds exactly the bytes of that slice of the whole song.
 * Replaces: nothing upstream renders part of a track; this is what lets a sequenced song be streamed chunk by chunk to a player, or its
 * middle be rendered again.
 * sh_seq_create takes sh_mix_events_chan's arguments without the track -- the rows are sh_mix_event_chan's, a row without a mode, flag,
 * loop or rate being the lower level's event -- and refuses what sh_mix_events_chan refuses, in the same words under its own name.  The
 * song is track_samples long and starts as silence.  The records are written for the LOWEST feature level that covers every row
 * (sh_seq_info.level), so a plain list is rendered by the plain kernels.  The tables go into a device block the handle owns.
 * LIFETIME: the handle keeps POINTERS into the sources and their byte ranges, not their data: the caller keeps every source buffer
 * alive, and unchanged, until sh_seq_destroy.
 * sh_seq_render writes song samples [first_sample, first_sample + nsamples) to samples out_sample .. of `out`, from silence: it never
 * reads `out` and writes every sample of the range, zeros where nothing plays.  Any sample offset is legal on either side; the steps that
 * count parity (tostereo, balance, downmix) count the SONG's samples.  nsamples == 0: SH_OK, nothing launched.  SH_ERR_INVALID, nothing
 * launched: a NULL argument, a range outside the song, a range outside `out`, an `out` range that overlaps a source of the song. */
typedef struct sh_seq sh_seq;
#define SH_SEQ_LEVEL_PLAIN 0u      /* placed, scaled, added */
#define SH_SEQ_LEVEL_RATE  1u      /* + audioop.ratecv */
#define SH_SEQ_LEVEL_PAN   2u      /* + a mono source into a stereo song */
#define SH_SEQ_LEVEL_ENV   3u      /* + envelopes */
#define SH_SEQ_LEVEL_LOOP  4u      /* + sustain loops */
#define SH_SEQ_LEVEL_REV   5u      /* + reversed playback */
#define SH_SEQ_LEVEL_CHAN  6u      /* + downmix and balance */
typedef struct sh_seq_info {
    uint64_t track_samples;        /* the song's length */
    uint64_t pairs;                /* (event, tile) overlaps: the entries of the per-tile index */
    uint64_t device_bytes;         /* records, segments and index on the device */
    uint32_t nevents;
    uint32_t ntiles;               /* tiles of the song (2048 samples at 16 bits, 1024 otherwise), idle ones included */
    uint32_t active_tiles;         /* those that some event touches */
    uint32_t level;                /* SH_SEQ_LEVEL_* */
} sh_seq_info;                     /* 40 bytes */
int sh_seq_create(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event_chan* events, uint32_t nevents,
                  const sh_env_segment* segments, uint32_t nsegments, int width, int nchannels, size_t track_samples, sh_seq** out);
int sh_seq_render(const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample);
int sh_seq_get_info(const sh_seq* seq, sh_seq_info* out);
int sh_seq_destroy(sh_seq* seq);

/* A song made of TRACKS, each with a gain given when it is RENDERED: mute, solo and faders without compiling again.  The bytes are those
 * of this chain, which is NOT the flat list -- a track saturates on its own before its gain applies, and the master at every track:
 *     master = silence; for t in tracks, in order:
 *         sub = the track's events folded from silence, in list order, saturating at every event (what sh_seq_create's song holds)
 *         if gains[t] != 1.0: sub = audioop.mul(sub, gains[t])        (clamp, then floor)
 *         master = audioop.add(master, sub)                            (saturating; a shorter track is padded with silence)
 * A gain of exactly 1.0 takes no multiply and one of exactly 0.0 skips the track's events (neither changes a byte).
 * sh_seq_create_tracks takes sh_seq_create's arguments and, behind the events, track_first: ntracks + 1 offsets into `events`, track t
 * holding rows [track_first[t], track_first[t + 1]) -- the tracks' lists one behind the other; a track may be empty.  It refuses what
 * sh_seq_create refuses, in its words and its order, and: ntracks == 0, ntracks > SH_SEQ_MAX_TRACKS, a track_first that is NULL, does
 * not start at 0, does not end at nevents or decreases.  The handle is sh_seq_create's (sh_seq_get_info, sh_seq_destroy), with a table
 * of per-tile runs -- one per track with events in the tile -- behind its index.
 * sh_seq_render_gains is sh_seq_render with ngains == the handle's track count gains, passed to the kernel BY VALUE in its arguments:
 * one launch, nothing uploaded, copied or materialised.  SH_ERR_INVALID, nothing launched: what sh_seq_render refuses, a handle without
 * tracks, another ngains than the handle has tracks, a gain that is not finite.  sh_seq_render of a handle with tracks renders with every
 * gain 1.0 -- the chain above, still grouped by track.  sh_seq_get_tracks: the track count (0: a handle of sh_seq_create) and the runs. */
#define SH_SEQ_MAX_TRACKS 32u
int sh_seq_create_tracks(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event_chan* events, uint32_t nevents,
                         const uint32_t* track_first, uint32_t ntracks, const sh_env_segment* segments, uint32_t nsegments, int width,
                         int nchannels, size_t track_samples, sh_seq** out);
int sh_seq_render_gains(const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample, const double* gains,
                        uint32_t ngains);
int sh_seq_get_tracks(const sh_seq* seq, uint32_t* ntracks, uint32_t* nruns);

/* The desk's METERS: sh_seq_render_gains, and from the SAME launch one row of levels per track, post-fader, and one for the master --
 * what Sample.level_db_peak / level_db_rms read off a finished sample, taken from the values the kernel holds anyway.  For the window
 * [first_sample, first_sample + nsamples): row t < ntracks is over audioop.mul(sub_t, gains[t]) (none at exactly 1.0; sub_t as above,
 * padded with silence) cut to the window, row ntracks over the window's output bytes.  Per channel -- song sample s is channel s & 1 of a
 * stereo song and channel 0 of any other, whose second channel reads 0 -- a row holds peak = max |x| (audioop.max; |-2^31| is 2^31) and
 * the exact integer sum of x * x as sq_hi * 2^32 + sq_lo: sq_lo = sum (x * x & 0xffffffff) and sq_hi = sum (x * x >> 32) at widths 3 and
 * 4, one sum in sq_lo and sq_hi == 0 at widths 1 and 2.  Width 3 is metered on the raw 24-bit values, as sh_pcm_stats.  A muted track
 * (gain exactly 0.0) and a track without events in the window have all-zero rows.  Integer max and add: the rows are the same on every
 * run and for every alignment of the window.
 * gains == NULL with ngains == 0: every gain 1.0.  nmeters must be the handle's track count + 1.  The call is SYNCHRONOUS, as sh_pcm_stats:
 * the handle's row table zeroed on the stream, the one launch, one copy of the rows to `meters`, one stream synchronise.  The table
 * belongs to the handle: a handle serves ONE metered render at a time (the library's lock sees to that for its own callers).
 * SH_ERR_INVALID, nothing launched, `out` and `meters` untouched: what sh_seq_render_gains refuses, a handle without tracks (a flat
 * song's only row is the peak of its output), meters == NULL, another nmeters.  nsamples == 0 zeroes the rows and returns SH_OK.
 * NOT here: pre-fader meters (they would read a muted track's events), meters of a song without tracks, clip counters. */
typedef struct sh_seq_meter {
    uint32_t peak[2];
    uint64_t sq_hi[2];
    uint64_t sq_lo[2];
} sh_seq_meter;                    /* 40 bytes */
int sh_seq_render_meters(const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample, const double* gains,
                         uint32_t ngains, sh_seq_meter* meters, uint32_t nmeters);

/* The desk's PAN POTS and MASTER FADER: sh_seq_render_gains (with meters != NULL: sh_seq_render_meters) of a STEREO song of tracks with
 * two more steps, both given when a window is rendered and passed to the kernel BY VALUE -- still one launch, nothing uploaded:
 *     master = silence; for t in tracks, in order:
 *         sub = the track's events folded from silence
 *         if gains[t] != 1.0: sub = audioop.mul(sub, gains[t])                                  (clamp, then floor)
 *         sub = (fbound(L * pans[2 t]), fbound(R * pans[2 t + 1])) per frame (L, R)             (Sample.stereo of a stereo sample)
 *         master = audioop.add(master, sub)
 *     if master_gain != 1.0: master = audioop.mul(master, master_gain)                          (once, behind the last track)
 * Two roundings per track, the gain first: not one product, and the master's gain on the saturated master.  A factor of exactly 1.0
 * takes no multiply; a track whose two factors are both exactly 0.0 is skipped like a muted one (all-zero row).  Song sample s takes
 * the left factor where s is even, whatever sample the window starts on.
 * pans: 2 * ntracks doubles, left then right per track; NULL with npans == 0: no pan.  gains: NULL with ngains == 0: every gain 1.0.
 * meters: NULL with nmeters == 0: unmetered, asynchronous as sh_seq_render_gains; otherwise ntracks + 1 rows as sh_seq_render_meters
 * gives them, a track's row over what the master takes of it (post-fader and post-pan), the master's over the stored bytes.
 * SH_ERR_INVALID, nothing launched, `out` and `meters` untouched: what sh_seq_render_gains refuses, a handle without tracks, pans on a
 * song whose nchannels != 2, another ngains, npans or nmeters than the handle's tracks ask for, a factor that is not finite. */
int sh_seq_render_desk(const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample, const double* gains,
                       uint32_t ngains, const double* pans, uint32_t npans, double master_gain, sh_seq_meter* meters, uint32_t nmeters);

/* The desk's FADER AUTOMATION: fader moves per track in SONG samples, uploaded once (sh_seq_auto_create) and applied by
 * sh_seq_render_auto -- sh_seq_render_desk with one more step per track, behind its gain and in front of its pan; still one launch,
 * nothing uploaded by a render (the table's two pointers travel by value):
 *     master = silence; for t in tracks, in order:
 *         sub = the track's events folded from silence
 *         if gains[t] != 1.0: sub = audioop.mul(sub, gains[t])                                  (clamp, then floor)
 *         for each segment of track t with kind 1, song samples s in [the end of the one before it, end):
 *             sub[s] = trunc(sub[s] * ((s - origin) * slope / numsamples + offset))              (float64, in this order; toward zero)
 *         sub = (fbound(L * pans[2 t]), fbound(R * pans[2 t + 1])) per frame (L, R)
 *         master = audioop.add(master, sub)
 *     if master_gain != 1.0: master = audioop.mul(master, master_gain)
 * -- Sample.fadein's expression (sh_mix_events_env's kind 1) with s counting interleaved SAMPLES of the song, whatever window is rendered.
 * A move from volume v0 to v1 over frames [a, b) of a song of nch channels is {end = b nch, origin = a nch, mul = 1.0, slope = v1 - v0,
 * numsamples = (b - a) nch, offset = v0, kind = 1}; a hold (v0 == v1) is trunc(x * v), NOT audioop.mul's floor.  Segments of kind 0 fill
 * the gaps; past a track's last segment nothing is shaped.  A track's row of levels is read behind its moves, as the master takes it; a
 * muted track is still skipped.  A kernel finds a tile's first segment by binary search, so a long list of moves costs log2 of its length.
 * sh_seq_auto_create: segments[seg_first[t] .. seg_first[t + 1]) are track t's, ntracks + 1 offsets.  SH_ERR_INVALID: a NULL argument, a
 * handle without tracks, width 3 (the fades have no 24-bit form), another ntracks than the handle's, a seg_first that does not start at
 * 0, does not end at nsegments or decreases; a segment whose reserved is not 0, whose end does not lie past the one before or lies past
 * the song, whose kind is not 0 or 1 or whose mul is not exactly 1.0; a move whose origin is not its first sample, whose numsamples is
 * smaller than its length, or whose volumes (offset, offset + slope) are not finite or leave 0 .. 1 -- so the factor never exceeds 1 and
 * the result never leaves the width's range.  The handle keeps nothing of `seq` but its track count, width, channels and length.
 * sh_seq_render_auto takes sh_seq_render_desk's arguments and the automation's handle; pans == NULL with npans == 0 and master_gain == 1.0
 * mean no desk step.  SH_ERR_INVALID, nothing launched, `out` and `meters` untouched: what sh_seq_render_desk refuses, automation ==
 * NULL, a handle made for another song (other track count, width, channels or length), width 3. */
typedef struct sh_seq_auto sh_seq_auto;
int sh_seq_auto_create(const sh_seq* seq, const sh_env_segment* segments, uint32_t nsegments, const uint32_t* seg_first, uint32_t ntracks,
                       sh_seq_auto** out);
int sh_seq_auto_destroy(sh_seq_auto* automation);
int sh_seq_render_auto(const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample, const double* gains,
                       uint32_t ngains, const double* pans, uint32_t npans, double master_gain, sh_seq_meter* meters, uint32_t nmeters,
                       const sh_seq_auto* automation);

/* The desk's GROUP BUSES: at most SH_SEQ_MAX_GROUPS runs of consecutive tracks [first, end), ascending and not overlapping, given when a
 * window is rendered; the tracks of a group are mixed into a bus of their own, which saturates ON ITS OWN, takes one gain and one pan and
 * enters the master where the group's LAST track stands.  sh_seq_render_groups is sh_seq_render_auto with that level between the tracks
 * and the master; still one launch, nothing uploaded by a render (the group table travels by value):
 *     master = silence; for t in tracks, in order:
 *         sub = the track's events folded from silence; its gain, its fader moves, its pan    (as sh_seq_render_auto)
 *         if t lies in group g:
 *             if t == first_g: bus = silence
 *             bus = audioop.add(bus, sub)
 *             if t == end_g - 1:
 *                 if gain_g != 1.0: bus = audioop.mul(bus, gain_g)                            (clamp, then floor: ONE rounding over the sum)
 *                 bus = (fbound(L * left_g), fbound(R * right_g)) per frame (L, R)              (a factor of exactly 1.0: none)
 *                 master = audioop.add(master, bus)
 *         else: master = audioop.add(master, sub)
 *     if master_gain != 1.0: master = audioop.mul(master, master_gain)
 * -- not a gain on each track (floor(g (a + b)) != floor(g a) + floor(g b)) and not the flat list (the group clips before the master
 * sees it).  A group whose gain is exactly 0.0, or whose factors are both exactly 0.0, skips its tracks' events as a muted track does;
 * its row and its tracks' rows read zero.  automation may be NULL (no fader moves); gains, pans and master_gain as sh_seq_render_desk's.
 * meters: NULL, or ntracks + 1 + ngroups rows -- the tracks and the master where sh_seq_render_desk has them, group g in row
 * ntracks + 1 + g, over what the master takes of it (behind its gain and pan); a track's row is what its bus takes of it.
 * SH_ERR_INVALID, nothing launched, `out` and `meters` untouched: what sh_seq_render_desk refuses and, with a handle, what
 * sh_seq_render_auto refuses (an automation handle at width 3 among it); ngroups == 0 or > SH_SEQ_MAX_GROUPS; groups == NULL; an entry
 * with first >= end, with end > ntracks, or that starts in front of the previous entry's end; a gain or factor that is not finite;
 * factors other than (1.0, 1.0) on a song that is not stereo; nmeters other than ntracks + 1 + ngroups where meters is given.  The
 * error text names the entry; an automation handle that rides a group this call does not name (below).  Not built: groups inside
 * groups. */
typedef struct sh_seq_group { uint32_t first, end; double gain; double left, right; } sh_seq_group;   /* 32 bytes */
#define SH_SEQ_MAX_GROUPS 8u
int sh_seq_render_groups(const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample, const double* gains,
                         uint32_t ngains, const double* pans, uint32_t npans, double master_gain, sh_seq_meter* meters, uint32_t nmeters,
                         const sh_seq_auto* automation /* may be NULL */, const sh_seq_group* groups, uint32_t ngroups);

/* The desk's BUS RIDES: fader moves on a group's bus and on the master, in the same table and the same launch.  sh_seq_auto_create_buses is
 * sh_seq_auto_create with ntracks + 1 + ngroups lanes in the meter table's row order -- tracks 0 .. ntracks - 1, the master at ntracks,
 * group g at ntracks + 1 + g -- so seg_first holds ntracks + 1 + ngroups + 1 offsets; ngroups is 0 .. SH_SEQ_MAX_GROUPS.  The chain:
 *     ... if t == end_g - 1:
 *             if gain_g != 1.0: bus = audioop.mul(bus, gain_g)
 *             bus[s] = trunc(bus[s] * ((s - origin) * slope / numsamples + offset)) over the segments of group g's lane    (NEW)
 *             bus = (fbound(L * left_g), fbound(R * right_g)) per frame;  master = audioop.add(master, bus)
 *     if master_gain != 1.0: master = audioop.mul(master, master_gain)
 *     master[s] = trunc(master[s] * (...)) over the segments of the master's lane                                           (NEW)
 * -- the group's ride behind its gain and in front of its pan, over the saturated bus (not a ride of each of its tracks); the master's
 * behind its gain, over the saturated master: Sample.fadein / fadeout of the mix.  Positions are song samples whatever the window.  A
 * group's row of levels is read behind its ride and pan, the master's over the stored bytes.  Every segment is held to sh_seq_auto_create's
 * rules, the error text naming `master` or `group g` where that says `track t`.  sh_seq_render_auto and sh_seq_render_groups take a
 * handle from either function: one without a segment on a bus lane renders exactly as one from sh_seq_auto_create; a master ride needs
 * no groups (sh_seq_render_auto); SH_ERR_INVALID, nothing launched: a handle with a segment on group g's lane given to
 * sh_seq_render_auto, or to sh_seq_render_groups with ngroups <= g. */
int sh_seq_auto_create_buses(const sh_seq* seq, const sh_env_segment* segments, uint32_t nsegments, const uint32_t* seg_first, uint32_t ntracks,
                             uint32_t ngroups, sh_seq_auto** out);

/* The desk's PAN RIDES, of a STEREO song: pan moves of a track and of a group's bus, in the same table and the same launch.
 * sh_seq_auto_create_pans is sh_seq_auto_create_buses (segments, seg_first, ntracks, ngroups: as there) plus a second array of segments,
 * the PAN LANES: ntracks + ngroups of them, the tracks' and then the groups', pan_segments[pan_first[l] .. pan_first[l + 1]) lane l's,
 * ntracks + ngroups + 1 offsets.  A pan move over frames [a, b) from pan p0 to p1 (-1.0 .. 1.0) is {kind = 3, origin = 2 a, end = 2 b
 * (song SAMPLES, both even), numsamples = b - a (FRAMES), offset = p0, slope = p1 - p0, mul = 1.0}; segments of kind 0 fill the gaps.
 * The chain is sh_seq_render_groups' with the two static pan steps replaced where a move covers a frame:
 *     sub = the track folded from silence; audioop.mul(gains[t]); the track's fader moves                      (unchanged)
 *     for each frame f of the song, (L, R) = sub's frame f:
 *         if f lies in a move [a, b) of track t's pan lane, with k = f - a:
 *             p = k * slope / numsamples + offset                                   (float64, in this order; k counts FRAMES, in 64 bits)
 *             (L, R) = (trunc(L * (1.0 - p) / 2.0), trunc(R * (1.0 + p) / 2.0))     (toward zero: Sample.pan(lfo=...)'s expression)
 *         else:
 *             (L, R) = (fbound(L * pans[2 t]), fbound(R * pans[2 t + 1]))           (the static pan, unchanged)
 *     ... into the group's bus or the master as before; and a group's bus the same way: behind its gain and its fader ride, group g's
 *     pan lane stands where its static factors (left_g, right_g) stand.
 * The move REPLACES the static pan inside its frames, it is not applied on top of it.  A hold (slope 0) is trunc(x * (1 -+ p) / 2), NOT
 * Sample.stereo's floor: a hold at 0.0 differs from static factors (0.5, 0.5) on every negative odd sample.  A track or group whose STATIC
 * factors are both exactly 0.0, or whose gain is 0.0, is still skipped entirely, moves or not.  A track's row of levels is read behind its
 * pan lane, a group's behind its ride and its pan lane, the master's over the stored bytes.  Positions are song samples whatever the
 * window.  |p| <= 1 up to one rounding, so no result leaves the width's range and nothing is clamped (csrc/seqpan.hpp has the proof).
 * SH_ERR_INVALID: what sh_seq_auto_create_buses refuses; a song whose nchannels != 2; pan_first NULL, or pan_segments NULL with
 * npan_segments != 0; a pan_first that does not start at 0, does not end at npan_segments or decreases; a pan segment whose reserved is
 * not 0, whose end does not lie past the one before or lies past the song, whose end is odd, whose kind is not 0 or 3 or whose mul is
 * not exactly 1.0; a move whose origin is not its first sample, whose numsamples is smaller than its frames, or whose pans (offset,
 * offset + slope) are not finite or leave -1 .. 1.  The error text names `track t pan` or `group g pan` and the segment.
 * sh_seq_render_auto and sh_seq_render_groups take the handle: one without a pan segment renders exactly as one from
 * sh_seq_auto_create_buses; tracks' pan moves need no groups (sh_seq_render_auto); SH_ERR_INVALID, nothing launched: a handle with a
 * segment on group g's pan lane given to sh_seq_render_auto, or to sh_seq_render_groups with ngroups <= g.  Not built: groups inside
 * groups, a stem of a group, automation at width 3. */
#define SH_ENV_PAN 3u
int sh_seq_auto_create_pans(const sh_seq* seq, const sh_env_segment* segments, uint32_t nsegments, const uint32_t* seg_first, uint32_t ntracks,
                            uint32_t ngroups, const sh_env_segment* pan_segments, uint32_t npan_segments, const uint32_t* pan_first,
                            sh_seq_auto** out);

/* The desk's LEVEL HISTORY: the rows of the meters per BLOCK of the window, from the launch that renders it.  A block is one tile of the
 * SONG's tile grid -- TILE = 2048 samples at width 2, 1024 at widths 1, 3 and 4 -- cut to the window: a render of song samples [lo, hi) has
 *     nblocks = (hi - 1) / TILE - lo / TILE + 1                                                   (0 for an empty window)
 * blocks, block j counting song samples [max(lo, (lo / TILE + j) * TILE), min(hi, (lo / TILE + j + 1) * TILE)): the first and the last
 * may be partial, and a song block that lies whole inside two windows reads the same from both.  sh_seq_render_history is
 * sh_seq_render_groups -- the same chain, the same bytes -- with three changes: ngroups may be 0 (groups NULL), automation may be NULL, and
 * instead of meters / nmeters it takes `rows`, a host array of nblocks * nrows rows, block-major: row r of block j at rows[j * nrows + r],
 * nrows == ntracks + 1 + ngroups in the meter table's order (tracks, master, groups).  Each row is what the meters of a render of that
 * block's own samples return: post-fader, post-moves and post-pan for a track, over the bus as the master takes it for a group, over the
 * stored bytes for the master; a muted or skipped track or group and an idle tile read zero; a mono song fills channel 0.  Folding all
 * blocks (max of the peaks, integer sums of sq_hi and of sq_lo) gives exactly the rows of the metered render of the window.  Every block
 * is written by the one workgroup that folds its tile: no atomics, no zeroing, the same table on every run.  The device table is the
 * library's scratch, sized for the call; one launch, one copy of nblocks * nrows rows, one wait.  An empty window writes nothing and
 * succeeds (nblocks 0).  SH_ERR_INVALID, nothing launched, `out` and `rows` untouched: what sh_seq_render_groups refuses apart from
 * ngroups == 0; nrows other than ntracks + 1 + ngroups; nblocks other than the window's; rows NULL with a window that is not empty; an
 * automation handle with a segment on a bus lane or on a pan lane (rides of buses and pans have no history yet).  SH_ERR_NOMEM: the
 * table cannot be allocated.  Not built: a history with bus rides or pan rides, a history without rendering the bytes. */
int sh_seq_render_history(const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample, const double* gains,
                          uint32_t ngains, const double* pans, uint32_t npans, double master_gain, sh_seq_meter* rows, uint32_t nrows,
                          uint32_t nblocks, const sh_seq_auto* automation /* may be NULL */, const sh_seq_group* groups /* NULL: none */,
                          uint32_t ngroups);

/* The history's OVERS: sh_seq_render_history -- the same arguments, the same chain, the same bytes, the same levels per block, the same
 * checks and refusals -- whose rows carry, behind the levels, `clipped`: per channel the number of the block's samples at which AT LEAST
 * ONE of the row's OWN steps was clamped (csrc/seqclip.hpp states the contract).  A step is clamped where the value it would have produced
 * without the clamp lies outside the width's range [LO, HI]; a sample counts ONCE per row, however many steps clamped at it.  Track t's
 * steps: every saturating add of an event's samples into the track's sub-mix, the track's amplify(gain), its static pan factors.  Group
 * g's: every saturating add of a track into the group's bus, the group's amplify(gain), its pan factors.  The master's: every saturating
 * add of a track or a group into the master, the master's amplify(master_gain).  An add clamps where the exact integer sum of the
 * saturated accumulator and the addend is > HI or < LO; a multiply by a factor f != 1.0 clamps where floor(p) > HI or floor(p) < LO, p
 * the float64 product audioop.mul forms (a product in (HI, HI + 1) floors to HI and is no over).  A row counts its OWN stage only: a track
 * that clipped does not make its group or the master count.  Not counted: what an event does to its own samples in front of the add (its
 * volume, pan, channel factors, envelope), and the tracks' fader moves, which cannot leave the range.  A muted or skipped track or group
 * and an idle tile count 0; a mono song fills channel 0.  Counts add over blocks.  SH_ERR_INVALID, nothing launched: what
 * sh_seq_render_history refuses, a bus ride or pan ride with a message of its own.  Not built: overs of an event's own chain, overs with
 * bus or pan rides. */
typedef struct sh_seq_meter_clips {
    uint32_t peak[2];
    uint64_t sq_hi[2];
    uint64_t sq_lo[2];
    uint32_t clipped[2];
} sh_seq_meter_clips;              /* 48 bytes: sh_seq_meter, then the counts */
int sh_seq_render_clips(const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample, const double* gains,
                        uint32_t ngains, const double* pans, uint32_t npans, double master_gain, sh_seq_meter_clips* rows, uint32_t nrows,
                        uint32_t nblocks, const sh_seq_auto* automation /* may be NULL */, const sh_seq_group* groups /* NULL: none */,
                        uint32_t ngroups);

/* The desk's STEMS: the samples of every bus, from ONE launch that walks every event once (csrc/seqstem.hpp states the contract).
 * sh_seq_render_stems is sh_seq_render_groups without meters -- the same chain, the same arguments with the same meaning, ngroups may be 0
 * (groups NULL) and automation may be NULL or any handle of the song: track lanes, bus rides, pan rides -- that writes, instead of the
 * master alone, nplanes == ntracks + 1 + ngroups PLANES of nsamples samples each into `out`, in the meter table's row order: track t in
 * plane t, the master in plane ntracks, group g in plane ntracks + 1 + g.  Plane r is samples [out_sample + r * plane_samples,
 * out_sample + r * plane_samples + nsamples) of `out`, and holds exactly the samples over which sh_seq_render_groups' meters of the same
 * call read row r: a track as its bus takes it (its gain, its fader moves, its pan or pan ride), a group's bus as the master takes it
 * (saturated at every track, its gain, its ride, its pan or pan ride), the master's plane the bytes sh_seq_render_groups stores.  A
 * muted or skipped track or group is all zeros.  EVERY byte of every plane is written whatever `out` held, idle tiles and muted rows
 * included, and no byte of `out` outside the planes' windows: none in front, none behind, none in the gaps where plane_samples >
 * nsamples.  At width 2 the store is one 16-byte vector per lane where plane 0's first sample lies (first_sample mod 8) samples behind
 * a 16-byte boundary and plane_samples is a multiple of 8; any other geometry is stored sample by sample and is the same bytes.
 * Asynchronous on the library's stream, as sh_seq_render_groups without meters; nothing is zeroed or copied in front of the launch.
 * nsamples == 0 writes nothing and succeeds.  SH_ERR_INVALID, nothing launched, `out` untouched: what sh_seq_render_groups refuses apart
 * from ngroups == 0; a song without tracks; nplanes other than ntracks + 1 + ngroups; plane_samples < nsamples; a last plane that ends
 * outside `out`; a span of all planes, gaps included, that overlaps a source of the song -- each by a message of its own.  Not built:
 * stems together with meters, a history or overs in the same launch; pre-fader stems; the raw group bus in front of its gain. */
int sh_seq_render_stems(const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample, size_t plane_samples,
                        uint32_t nplanes, const double* gains, uint32_t ngains, const double* pans, uint32_t npans, double master_gain,
                        const sh_seq_auto* automation /* may be NULL */, const sh_seq_group* groups /* NULL: none */, uint32_t ngroups);

/* ---- the real-time lane -------------------------------------------------------------------------------------------------------
 * Replaces: the thread upstream's playback.py runs its mixer on (the output thread pulls RealTimeMixer.chunks() while other threads
 * make sound).  Every entry point above holds the library's one lock and enqueues on its one stream pair: a mixer turn from another
 * thread queues behind whatever the others have enqueued, and its download holds the lock while the stream drains.  A LANE is a
 * stream (high priority), a lock, a source-table buffer and a chunk buffer of its own: sh_rt_mix_turn -- the ordered saturating fold
 * of sh_mix_chain_gather over the sources' current chunks (bit-identical: the same kernels) + the chunk copied to out_host --
 * takes the lane's lock only and waits for the lane's stream only; it returns when out_host holds the chunk.  Order against the
 * library's streams is established once per source: sh_rt_acquire(lane, src) makes the lane's next turn wait (on the device) for
 * everything the library has been given so far -- the upload / resample / render that made `src` -- and folds first what a render
 * still owes into it.  After that the caller must not write `src` while the lane can read it, and must not free it before the last
 * turn that names it has returned (turns are synchronous: once sh_rt_mix_turn is back nothing of the lane is in flight).
 * One lane per mixer; distinct lanes are independent; sh_rt_create / sh_rt_destroy / sh_rt_acquire take the library's lock. */
typedef struct sh_rt sh_rt;
int sh_rt_create(size_t max_chunk_bytes, uint32_t max_sources, sh_rt** out);
int sh_rt_destroy(sh_rt* lane);
int sh_rt_acquire(sh_rt* lane, const sh_buf* src);
int sh_rt_mix_turn(sh_rt* lane, const sh_buf* const* srcs, const size_t* sample_offsets, const uint32_t* nsamples_each, uint32_t nsrc,
                   uint32_t nsamples, int width, void* out_host);

/* ---- Sample.from_osc_block: int(scale*v), truncation toward zero; SH_ERR_OVERFLOW if out of range */
int sh_quantize_f32(const sh_buf* in_f32, size_t in_off, size_t n, double scale, int width,
                    sh_buf* out_pcm, size_t out_off);
/* same for float64 input (blocks produced by a float64 generator, e.g. upstream's own oscillators) */
int sh_quantize_f64(const sh_buf* in_f64, size_t in_off, size_t n, double scale, int width,
                    sh_buf* out_pcm, size_t out_off);
/* float stereo bus -> int16 with saturation instead of OverflowError (bus epilogue, [SPEC]) */
int sh_quantize_clip_f32(const sh_buf* in_f32, size_t n, double scale, sh_buf* out_i16);

/* ---- Sample.mix -> audioop.add(frag1, frag2, width): saturating pairwise add, width 1/2/4 */
int sh_pcm_add(const sh_buf* a, size_t a_off, const sh_buf* b, size_t b_off, size_t nbytes, int width,
               sh_buf* out, size_t out_off);
int sh_pcm_add_host(const void* a, const void* b, size_t nbytes, int width, void* out);

/* ---- the other elementwise Sample operations that delegate to audioop ----
 * Sample.amplify / invert -> audioop.mul: fbound(sample * factor) (clamp, then floor) */
int sh_pcm_mul(const sh_buf* in, size_t in_off, size_t nbytes, int width, double factor, sh_buf* out, size_t out_off);
/* Sample.fadeout (fadeout != 0): int(sample_i * (1 - i*slope/numsamples)); Sample.fadein: int(sample_i *
 * (i*slope/numsamples + offset)); i = sample index in the range, numsamples = nbytes/width, truncation */
int sh_pcm_fade(const sh_buf* in, size_t in_off, size_t nbytes, int width, int fadeout, double slope, double offset,
                sh_buf* out, size_t out_off);
/* Sample.modulate_amp: out[i] = int(in[i] * mod[i mod nmod]) (float64 product, truncation toward zero); mod_f64 is
 * a device buffer of nmod float64 factors, cycled.  A product outside the sample range is SH_ERR_OVERFLOW
 * (upstream: OverflowError from the array store). */
int sh_pcm_modulate(const sh_buf* in, size_t nbytes, int width, const sh_buf* mod_f64, size_t nmod, sh_buf* out);
/* samples as float64: out[i] = in[i] / divisor (Sample.get_frames_as_floats uses 2^(bits-1); modulate_amp with a
 * waveform modulator uses its largest absolute value) */
int sh_pcm_to_f64(const sh_buf* in, size_t nsamples, int width, double divisor, sh_buf* out_f64);
/* Sample.pan(lfo=...) (upstream synthplayer/sample.py, [RECALL]): out frame i = (int(l*(1-p)/2), int(r*(1+p)/2)),
 * p = pan_f64[i] (one float64 per frame, device resident: an oscillator rendered in place, or uploaded values);
 * nchannels 1 (l = r = the mono sample) or 2; out is stereo.  SH_ERR_OVERFLOW where Python would raise. */
int sh_pcm_pan_lfo(const sh_buf* in, size_t nframes, int width, int nchannels, const sh_buf* pan_f64, sh_buf* out);
/* Sample.bias -> audioop.bias: wrapping add */
int sh_pcm_bias(const sh_buf* in, size_t nbytes, int width, int bias, sh_buf* out);
/* Sample.reverse -> audioop.reverse: sample order reversed (out must not alias in) */
int sh_pcm_reverse(const sh_buf* in, size_t nbytes, int width, sh_buf* out);
/* Sample.mono / left / right -> audioop.tomono; Sample.stereo (mono source) -> audioop.tostereo */
int sh_pcm_tomono(const sh_buf* in, size_t nframes, int width, double lfactor, double rfactor, sh_buf* out);
int sh_pcm_tostereo(const sh_buf* in, size_t nframes, int width, double lfactor, double rfactor, sh_buf* out);
/* Sample.normalize / make_16bit / make_32bit -> audioop.lin2lin */
int sh_pcm_lin2lin(const sh_buf* in, size_t nsamples, int width, int new_width, sh_buf* out);
/* audioop.max (maximum absolute sample) and the sum of squares audioop.rms takes the root of
 * (exact for widths 1 and 2; width 4 is summed in float64 in a fixed tree order) */
int sh_pcm_stats(const sh_buf* in, size_t nbytes, int width, uint32_t* max_abs, double* sum_squares);
/* The same for interleaved stereo, per channel in one pass: [0] = left, [1] = right.  Replaces the
 * audioop.tomono(frames, w, 1, 0) / (.., 0, 1) + audioop.max / audioop.rms sequence of Sample.level_db_peak /
 * level_db_rms and LevelMeter.update (upstream synthplayer/sample.py, [RECALL], tree not mounted). */
int sh_pcm_stats_stereo(const sh_buf* in, size_t nframes, int width, uint32_t max_abs[2], double sum_squares[2]);
/* The levels PER BLOCK of PCM that lies in device memory, exact in integers, for one plane or many, in one launch (csrc/pcmblocks.hpp
 * has the geometry).  The input: nframes frames of nch (1 or 2) interleaved channels of `width` bytes (1, 2, 4, or 3: the raw 24-bit
 * values, as sh_pcm_stats), from sample `sample_offset` of `in` on; nplanes such planes, plane r beginning r * plane_samples samples
 * behind plane 0 (any whole number of samples, at least nframes * nch where there is more than one plane; the stems of
 * sh_seq_render_stems are such planes).  Nothing outside the planes is read, and the rows do not depend on their alignment.
 * Positions are FRAMES in 64 bits: frame i of the input stands at grid frame origin_frame + i, and block j of the call is grid block
 * origin_frame / block_frames + j, cut to [origin_frame, origin_frame + nframes) -- sh_seq_render_history's rule with frames in place
 * of tiles and any block size: nblocks = (origin_frame + nframes - 1) / block_frames - origin_frame / block_frames + 1 (0 for an empty
 * window), the first and the last block may be partial, and a block that lies whole inside two calls reads the same from both.
 * rows: a HOST array of nblocks * nplanes sh_seq_meter, block-major, row r of block j at j * nplanes + r: per channel the peak
 * (audioop.max) and the exact integer sum of squares sq_hi * 2^32 + sq_lo -- one sum (sq_hi == 0) at widths 1 and 2, two at widths 3
 * and 4; a mono input fills channel 0 and leaves channel 1 at 0.  Integer max and integer add only: the same table on every run.
 * SYNCHRONOUS, as sh_seq_render_history: one launch (two where a block is longer than 8192 samples: its parts are folded by a second,
 * small kernel; at width 3 an unpacking launch per plane in front), the table copied back, one wait.  SH_ERR_INVALID, each with a
 * message of its own and before anything is launched or written: nch not 1 or 2, a bad width, block_frames == 0, nplanes == 0,
 * plane_samples < nframes * nch with more than one plane, a last plane that ends outside in, nblocks other than the count above,
 * rows == NULL with a non-empty window.  nframes == 0 with nblocks == 0 succeeds and launches nothing. */
int sh_pcm_level_blocks(const sh_buf* in, size_t sample_offset, size_t nframes, int nch, int width, size_t plane_samples, uint32_t nplanes,
                        uint64_t origin_frame, uint64_t block_frames, sh_seq_meter* rows /* host, nblocks * nplanes */, size_t nblocks);
/* The waveform EXTREMES per block of the same PCM, for drawing: per block and channel the smallest and the largest sample as signed
 * values of the width (audioop.minmax of that channel's samples; width 1 signed, width 3 the sign-extended 24-bit value).  A mono
 * input fills channel 0 and stores lo[1] = hi[1] = 0.  Every block of a call counts at least one frame, so the identity of the fold
 * (lo = INT32_MAX, hi = INT32_MIN) never reaches the table.  csrc/pcmextent.hpp has the row, csrc/pcmblocks.hpp the geometry. */
typedef struct sh_pcm_extent {
    int32_t lo[2];
    int32_t hi[2];
} sh_pcm_extent;                   /* 16 bytes */
/* sh_pcm_level_blocks' arguments, planes, grid, block-major table and refusals (each message under this function's name), with rows a
 * HOST array of nblocks * nplanes sh_pcm_extent.  Integer min and max only: the same table on every run and for every split.
 * SYNCHRONOUS: one launch, one wave per block and plane (two launches where a block is longer than 8192 samples; at width 3 an
 * unpacking launch per plane in front), the table copied back, one wait.  nframes == 0 with nblocks == 0 succeeds and launches nothing. */
int sh_pcm_extent_blocks(const sh_buf* in, size_t sample_offset, size_t nframes, int nch, int width, size_t plane_samples, uint32_t nplanes,
                         uint64_t origin_frame, uint64_t block_frames, sh_pcm_extent* rows /* host, nblocks * nplanes */, size_t nblocks);

/* ---- Sample.convolve: a finite impulse response (a room, a plate, a cabinet, a filter) over PCM in device memory, in the direct
 * form and EXACT (csrc/pcmfir.hpp has the contract).  The input: in_frames frames of nch (1 or 2) interleaved channels of `width` (1
 * or 2) bytes from byte in_off of `in` on; the response: ir_frames frames (1 .. 2^22) of ir_nch channels of the same width from byte
 * ir_off of `ir` on -- ir_nch == 1: the one response over every channel; ir_nch == 2 == nch: left over left, right over right.  The
 * result has in_frames + ir_frames - 1 frames (0 where in_frames == 0) of nch channels: per channel and frame the exact integer sum of
 * response[k] * input[i - k], input outside its frames counting as 0, then ONE rounding, audioop.mul's: fbound(sum * factor) --
 * clamped to the width's limits, then floor.  With at most 2^22 taps every partial sum stays below 2^53, so the float64 FMA chain of
 * the kernel is integer arithmetic and the bytes do not depend on how the work is divided.  The call writes frames [first, first +
 * nframes) of the result to byte out_off of `out` on, and those bytes are that slice of the whole result's bytes.  All offsets are
 * BYTES, and any byte will do: the kernels read and write sample by sample and ask for no alignment.  Asynchronous on the
 * library's stream, as sh_pcm_mul: two launches (the response to float64 in the library's scratch, then one workgroup per tile of
 * 2048 frames and channel).
 * SH_ERR_INVALID, each with a message of its own and before anything is launched or written: a width other than 1 or 2, nch not 1
 * or 2, ir_nch not 1 and not nch, ir_frames == 0 or above 2^22, a factor that is not finite, a window past the result, an operand that
 * reaches past its buffer, out overlapping in or ir.  An empty window succeeds and launches nothing. */
int sh_pcm_convolve(const sh_buf* in, size_t in_off, uint64_t in_frames, int nch, int width, const sh_buf* ir, size_t ir_off, uint32_t ir_frames,
                    int ir_nch, double factor, uint64_t first, uint64_t nframes, sh_buf* out, size_t out_off);

/* ---- Sample.resample_fir: a rational, band-limited sample-rate conversion of PCM in device memory -- zero-stuff by `up`, filter with
 * integer taps, keep every `down`-th frame -- in polyphase form and EXACT (csrc/pcmresample.hpp has the contract).  The input:
 * in_frames frames of nch (1 or 2) interleaved channels of `width` (1 or 2) bytes from byte in_off of `in` on; the taps: ntaps
 * (1 .. 2^22) int16 values from byte taps_off of `taps` on, ONE bank for every channel, 16 bits whatever `width` is.  The result has
 * sh_pcm_resample_fir_frames(in_frames, up, down) = ceil(in_frames * up / down) frames of nch channels: per channel and frame j the
 * exact integer sum over k of taps[k] * u[j * down + delay - k], u being the input with up - 1 zeros behind every frame and zeros
 * outside it, then ONE rounding, audioop.mul's: fbound(sum * factor).  up and down need not be coprime.  The bytes depend on the input,
 * the taps, up, down, delay and factor alone.  The call writes frames [first, first + nframes) of the result to byte out_off of `out`
 * on: that slice of the whole result's bytes.  All offsets are BYTES, and any byte will do.  Asynchronous on the library's stream, as
 * sh_pcm_convolve: two launches (the taps of every phase to float64 rows in the library's scratch, then the arithmetic).
 * SH_ERR_INVALID, each with a message of its own and before anything is launched or written: a width other than 1 or 2, nch not 1
 * or 2, ntaps == 0 or above 2^22, up or down 0, up above 4096, a ratio whose stride (down, times ceil(8 / up) where up < 8) times 63
 * plus 1024 exceeds 32768 frames (convert in two steps), delay >= ntaps, a factor that is not finite, a window past the result, an
 * operand that reaches past its buffer, out overlapping in or taps, a NULL buffer.  An empty window succeeds and launches nothing. */
int sh_pcm_resample_fir(const sh_buf* in, size_t in_off, uint64_t in_frames, int nch, int width, const sh_buf* taps, size_t taps_off, uint32_t ntaps,
                        uint32_t up, uint32_t down, uint32_t delay, double factor, uint64_t first, uint64_t nframes, sh_buf* out, size_t out_off);
uint64_t sh_pcm_resample_fir_frames(uint64_t in_frames, uint32_t up, uint32_t down);   /* pure, works without a device */

/* ---- Sample.limit: a look-ahead peak limiter (a brick wall) over PCM in device memory, EXACT in integers (csrc/pcmlimit.hpp has the
 * contract).  The input: in_frames frames of nch (1 or 2) interleaved channels of `width` (1, 2 or 4) bytes from byte in_off of `in`
 * on.  With ONE = 2^30 and HI = 2^(8 width - 1) - 1, per frame i: p = the largest magnitude of the frame's channels (one gain per
 * frame: the channels are linked); g[i] = ONE where p <= ceiling, else floor(ceiling * ONE / p);
 *     G[i] = min(ONE, min over j >= i of g[j] + (j - i) * s_a, min over j < i of g[j] + (i - j) * s_r),
 * s_a = slope(attack_frames), s_r = slope(release_frames), slope(f) = ONE where f <= 1, else ceil(ONE / f) -- a linear ramp down in
 * front of a peak and a linear ramp up behind it; and the sample is (x * G[i]) >> 30, the floor of the signed 64-bit product.  No
 * float anywhere.  G[i] <= g[i], so no sample of the result exceeds the ceiling in magnitude; where G[i] == ONE the frame is
 * untouched.  The bytes depend on the input, ceiling, attack_frames and release_frames alone.  The call writes frames [first, first +
 * nframes) of the result (which has in_frames frames) to byte out_off of `out` on and their gains G as uint32 to byte gain_off of
 * `gain` on: that slice of the whole result's bytes -- peaks outside the window still shape the gain inside it.  `out` or `gain` may
 * be NULL, not both.  IN PLACE: `out` may be exactly the window's own bytes of the input (out's address == in's + first frames).
 * All offsets are BYTES, and any byte will do.  Asynchronous on the library's stream, as sh_pcm_convolve: two launches (two
 * summaries per tile of 2048 frames into the library's scratch, then one workgroup per tile of the window).
 * SH_ERR_INVALID, each with a message of its own and before anything is launched or written: a width other than 1, 2 or 4, nch not
 * 1 or 2, a ceiling of 0 or above HI, attack_frames or release_frames above 2^20, a window past in_frames, an operand that reaches
 * past its buffer, out overlapping in in any way but exactly the window's own bytes, gain overlapping in or out, both destinations
 * NULL, a NULL input.  An empty window succeeds and launches nothing. */
int sh_pcm_limit(const sh_buf* in, size_t in_off, uint64_t in_frames, int nch, int width, uint32_t ceiling, uint32_t attack_frames,
                 uint32_t release_frames, uint64_t first, uint64_t nframes, sh_buf* out, size_t out_off, sh_buf* gain, size_t gain_off);

/* ---- Sample.resample -> audioop.ratecv(frames, width, nchannels, inrate, outrate, None) */
size_t sh_resample_out_frames(size_t in_frames, int inrate, int outrate);
/* width 1/2/4 integer PCM (bit-exact audioop arithmetic); is_float!=0: float32 PCM (width must be 4) */
int sh_resample(const sh_buf* in, size_t in_frames, int nchannels, int width, int is_float,
                int inrate, int outrate, sh_buf* out, size_t* out_frames);
int sh_resample_host(const void* in, size_t in_frames, int nchannels, int width, int is_float,
                     int inrate, int outrate, void* out, size_t* out_frames);
/* Sharding Sample.resample by output-frame range (no collective, a halo of one input frame).
 * sh_resample_span: the input frames [*in_first, *in_first + *in_count) that output frames [out_first, out_first +
 * out_n) of a stream of in_total_frames read (*in_first rounded down to a multiple of 16).  Host-only arithmetic.
 * sh_resample_range: resample that output range from a buffer holding input frames [in_first, in_first + in_held)
 * into out[0 .. out_n); out_first and in_first must be multiples of 16 frames.  Concatenating the ranges of a
 * partition gives sh_resample's result bit for bit. */
int sh_resample_span(size_t in_total_frames, int inrate, int outrate, size_t out_first, size_t out_n,
                     size_t* in_first, size_t* in_count);
int sh_resample_range(const sh_buf* in, size_t in_first, size_t in_held, int nchannels, int width, int is_float,
                      int inrate, int outrate, size_t out_first, size_t out_n, sh_buf* out);

/* ---- multi-GPU: voice-sharded banks, partial buses summed by RCCL over xGMI ------------ */
#define SH_DIST_ID_BYTES 128
int sh_dist_unique_id(void* id128);                       /* rank 0: ncclGetUniqueId */
int sh_dist_init(int rank, int world, const void* id128); /* ncclCommInitRank on the library stream */
int sh_dist_shutdown(void);
int sh_dist_rank(void);
int sh_dist_world(void);
/* What RCCL itself says about the communicator (not what the caller passed to sh_dist_init): out[0] = 1 when a communicator exists,
 * out[1] = ncclCommCount, out[2] = ncclCommUserRank (-1 without a communicator), out[3] = ncclGetVersion (0 while librccl.so has not
 * been loaded), out[4] = 1 when librccl.so is loaded.  Writes min(n, 5) words, returns 5; never loads the library by itself. */
int sh_dist_comm_info(int32_t* out, int n);
/* sum the ranks' float64 partial buses into root's buffer (ncclReduce, ncclDouble, in place) */
int sh_dist_reduce_bus(sh_buf* bus_f64, size_t nvalues, int root);
int sh_dist_allreduce_bus(sh_buf* bus_f64, size_t nvalues);
int sh_dist_barrier(void);
/* pipelined form: the collective (and, on root, the float64 -> float32 rounding into bus_f32) is enqueued on
 * the library's communication stream behind everything already enqueued on the main stream, so block s is
 * reduced while block s+1 renders.  `slot` (0 .. sh_dist_slots()-1) names the buffer pair; call
 * sh_dist_wait_slot(slot) before the main stream overwrites that slot's buffers again.  sh_sync() waits
 * for both streams. */
int sh_dist_slots(void);
int sh_dist_reduce_bus_async(sh_buf* bus_f64, size_t nvalues, int root, sh_buf* bus_f32, int slot);
int sh_dist_wait_slot(int slot);
/* The two calls above end the run of pipelined renders they are made in (like every entry point that can touch a bus buffer): a
 * pipeline drain per batch.  These three do not.  sh_dist_mark_slot(slot): call once the slot's last render lies at least two
 * launches back in its bank's run -- every partial bus of the slot has been folded by then -- it records where both render streams
 * stand.  sh_dist_reduce_bus_lagged: call a few launches after the mark; the collective waits for the two marks only, and the run
 * goes on (without a mark, or if a fold into the buffers is still owed, it behaves like sh_dist_reduce_bus_async).
 * sh_dist_wait_slot_keep makes both render streams wait for the slot's collective. */
int sh_dist_mark_slot(int slot);
int sh_dist_reduce_bus_lagged(sh_buf* bus_f64, size_t nvalues, int root, sh_buf* bus_f32, int slot);
int sh_dist_wait_slot_keep(int slot);
/* This rank's nvalues chain maps (sh_chain_map) to root's gathered[rank * nvalues ..] on the library stream (ncclGather where
 * librccl has it, else grouped ncclSend / ncclRecv); gathered is only read on root.  Without a communicator, or in a world of
 * one: a copy. */
int sh_dist_gather_parts(const sh_buf* parts, size_t nvalues, int root, sh_buf* gathered);
/* float64 bus -> float32 bus after the reduce: IEEE round to nearest, ties to even (overflow to +-inf, gradual underflow) */
int sh_bus_finalize(const sh_buf* bus_f64, size_t nvalues, sh_buf* bus_f32);

#ifdef __cplusplus
}
#endif
#endif /* SYNTHHIP_H */
