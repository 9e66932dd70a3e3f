// sequence.hip -- a list of placed samples mixed into a track in one launch (sh_mix_events, sh_mix_events_rate, sh_mix_events_pan,
// sh_mix_events_env: Sample.mix_at_many, mixer.sequence).
//
// Per event audioop.mul (fbound: clamp, then floor) and audioop.add with saturation AT EVERY EVENT, IN LIST ORDER -- the loop of
// Sample.mix_at calls it replaces, byte for byte.  The track is cut into tiles (seqplan.hpp); one workgroup per tile that some event
// touches walks that tile's events in order, every lane keeping its own few track samples in registers from the one load of the base
// to the one store of the result.  Lanes own disjoint samples and read the track only there, so the fold is in place; a source may
// not be the track.  sh_mix_events_rate: an event may play its source at another speed -- audioop.ratecv in front of the mul, output
// frame m of the resampled source formed by whichever lane owns the track sample it lands on (ratecv.hpp: the position in closed form,
// the sample arithmetic), never materialised.  sh_mix_events_pan: a mono source into a stereo track -- audioop.tostereo between the
// ratecv and the mul, in the same lane.  sh_mix_events_env: an ADSR envelope per event -- Sample.envelope's
// gain (seqenv.hpp) on the (resampled, cut) source samples, between the ratecv and the tostereo.  Built with -ffp-contract=off (the float64 product of audioop.mul stays one rounding,
// ratecv's prev*d + cur*(outr-d) two).
#include "common.hpp"
#include "chain.hpp"
#include "pcmdev.hpp"
#include "ratecv.hpp"
#include "seqenv.hpp"
#include "seqplan.hpp"
#include <math.h>
#include <string.h>
#include <type_traits>
#include <vector>

namespace {

typedef int int4v __attribute__((ext_vector_type(4)));
typedef short short8u __attribute__((ext_vector_type(8), aligned(2)));      // eight samples at any sample offset
// A source pointer comes out of a record in memory, so the compiler cannot know its address space and would read through it with flat
// loads: the sources are device buffers, say so (global_load).
#define SH_SEQ_GLOBAL __attribute__((address_space(1)))
typedef const SH_SEQ_GLOBAL short* gshort_p;

// One event as the kernels read it: wave-uniform, so a record is fetched by scalar loads.
struct SeqEv {
    const void* src;          // the first sample taken from the source
    double      factor;       // audioop.mul's; exactly 1.0: none
    uint32_t    dst;          // where in the track its first sample lands (samples)
    uint32_t    n;            // samples, > 0 for every event a tile lists
    uint32_t    pad[2];
};
static_assert(sizeof(SeqEv) == 32, "SeqEv is read as one 32-byte scalar load");

// How a lane gets the eight samples of an event that start at sample `rel` of its source, when they sit at any 2-byte offset against
// the lane's aligned sixteen.  All lanes of a workgroup start on multiples of eight track samples, so that offset -- (src - 2 dst)
// mod 16 -- is the same for every lane: wave-uniform per event.
//   FUNNEL  two aligned 16-byte loads and a funnel shift by that byte count (v_alignbyte_b32); an aligned event takes one load.
//   VEC2    one load through a vector type of alignment 2: the compiler emits ONE global_load_dwordx4 at the odd address (read
//           in the ISA: no global_load_ushort), the memory pipeline splits what crosses a line.
// FUNNEL is the default and SYNTHHIP_SEQ_ALIGN=1 selects VEC2.  Measured (profiles/sequence_ab.txt; one call of Sample.mix_at_many on the
// 120-s song with 4096 / 32 768 events, 75 % of the starts misaligned): 3.36 / 30.6 ms against 3.48 / 31.5 ms -- within 4 %, and that call is
// still bound by the host's table packing, so the choice is not settled by it: FUNNEL stays because it asks nothing of how the memory
// pipeline treats a vector load that straddles a line.  Staging an event's span through LDS was not built.
// Lanes on the edges of an event (not all eight samples inside it; FUNNEL: not both aligned vectors inside the source) assemble
// their samples one by one, zeros outside: x + 0 is the identity of the saturating add and fbound(0 * factor) == 0.
enum Scheme { FUNNEL = 0, VEC2 = 1 };

__device__ __forceinline__ short8v seq_edge8(gshort_p src, long long rel, uint32_t n) {
    short8v x = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (rel + j >= 0 && rel + j < (long long)n) x[j] = src[rel + j];
    return x;
}

template <int SCHEME>
__device__ __forceinline__ short8v seq_load8(const SeqEv& c, uint32_t s0) {
    gshort_p src = (gshort_p)c.src;
    const long long rel = (long long)s0 - (long long)c.dst;
    if (rel + 8 <= 0 || rel >= (long long)c.n) return (short8v){0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (SCHEME == VEC2) {
        if (rel >= 0 && rel + 8 <= (long long)c.n) return *(const SH_SEQ_GLOBAL short8u*)(src + rel);
    } else {
        const uint32_t sh = (uint32_t)(((uintptr_t)c.src - 2 * (uintptr_t)c.dst) & 15);      // (uniform) 0, 2 .. 14
        if (sh == 0) {
            if (rel >= 0 && rel + 8 <= (long long)c.n) return *(const SH_SEQ_GLOBAL short8v*)(src + rel);
        } else if (rel >= 8 && rel + 16 <= (long long)c.n) {
            const SH_SEQ_GLOBAL int4v* q = (const SH_SEQ_GLOBAL int4v*)((uintptr_t)(src + rel) - sh);
            const int4v lo = q[0], hi = q[1];
            const uint32_t r = sh & 3;
            union { int4v v; short8v s; } o;
#define SH_FUNNEL(A_, B_, C_, D_, E_) o.v = (int4v){(int)__builtin_amdgcn_alignbyte(B_, A_, r), (int)__builtin_amdgcn_alignbyte(C_, B_, r), \
                                                    (int)__builtin_amdgcn_alignbyte(D_, C_, r), (int)__builtin_amdgcn_alignbyte(E_, D_, r)}
            switch (sh >> 2) {                              // (uniform)
            case 0: SH_FUNNEL(lo[0], lo[1], lo[2], lo[3], hi[0]); break;
            case 1: SH_FUNNEL(lo[1], lo[2], lo[3], hi[0], hi[1]); break;
            case 2: SH_FUNNEL(lo[2], lo[3], hi[0], hi[1], hi[2]); break;
            default: SH_FUNNEL(lo[3], hi[0], hi[1], hi[2], hi[3]); break;
            }
#undef SH_FUNNEL
            return o.s;
        }
    }
    return seq_edge8(src, rel, c.n);
}

__device__ __forceinline__ short8v seq_mul8(const short8v x, const double factor) {
    short8v r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (short)fbound((double)x[j] * factor, Lim<short>::lo, Lim<short>::hi);
    return r;
}

// The 16-bit kernel: workgroup k folds active tile tiles[k]; a lane owns LANE_SAMPLES_I16 = 8 consecutive track samples (one aligned
// 16-byte load of the base, one aligned 16-byte store).  INFLIGHT events' records (scalar loads, one batch ahead) and source vectors
// are in flight before their adds.  `aligned`: the track starts on a 16-byte boundary (a view that does not: sample by sample).
template <int SCHEME, int INFLIGHT>
__global__ __launch_bounds__(shq::TILE_THREADS) void k_mix_events_i16(const SeqEv* __restrict__ ev, const uint32_t* __restrict__ tiles,
                                                                      const uint32_t* __restrict__ first, const uint32_t* __restrict__ idx,
                                                                      uint32_t ntiles, short* track, uint32_t track_samples, int aligned) {
    const uint32_t k = (uint32_t)sh::block_id();
    if (k >= ntiles) return;
    const uint32_t s0 = tiles[k] * shq::TILE_I16 + threadIdx.x * shq::LANE_SAMPLES_I16;
    if (s0 >= track_samples) return;
    const bool whole = aligned && s0 + 8 <= track_samples;
    short8v acc = {0, 0, 0, 0, 0, 0, 0, 0};
    if (whole) acc = *reinterpret_cast<const short8v*>(track + s0);
    else
        for (uint32_t j = 0; j < 8 && s0 + j < track_samples; ++j) acc[j] = track[s0 + j];
    uint32_t e = first[k];
    const uint32_t e1 = first[k + 1];
    auto fold = [&](const SeqEv& c, short8v x) {
        if (c.factor != 1.0) x = seq_mul8(x, c.factor);       // (uniform)
        acc = __builtin_elementwise_add_sat(acc, x);
    };
    if (e1 - e >= INFLIGHT) {
        SeqEv c[INFLIGHT], nx[INFLIGHT];
#pragma unroll
        for (int u = 0; u < INFLIGHT; ++u) c[u] = ev[idx[e + u]];
        for (; e + INFLIGHT <= e1; e += INFLIGHT) {
            const bool more = e + 2 * INFLIGHT <= e1;
            if (more) {
#pragma unroll
                for (int u = 0; u < INFLIGHT; ++u) nx[u] = ev[idx[e + INFLIGHT + u]];
            }
            short8v x[INFLIGHT];
#pragma unroll
            for (int u = 0; u < INFLIGHT; ++u) x[u] = seq_load8<SCHEME>(c[u], s0);
#pragma unroll
            for (int u = 0; u < INFLIGHT; ++u) fold(c[u], x[u]);
            if (more) {
#pragma unroll
                for (int u = 0; u < INFLIGHT; ++u) c[u] = nx[u];
            }
        }
    }
    for (; e < e1; ++e) {
        const SeqEv c = ev[idx[e]];
        fold(c, seq_load8<SCHEME>(c, s0));
    }
    if (whole) *reinterpret_cast<short8v*>(track + s0) = acc;
    else
        for (uint32_t j = 0; j < 8 && s0 + j < track_samples; ++j) track[s0 + j] = acc[j];
}

// Widths 1, 3 and 4: the reference's loop as it stands, LANE_SAMPLES_W = 4 consecutive samples per thread, bytes assembled for 24-bit
// samples, 64-bit sums for 32-bit ones -- the shape of k_mix_chain_gather_w (pcm.hip), which says why these widths get the plain kernel.
template <int WIDTH>
__global__ __launch_bounds__(shq::TILE_THREADS) void k_mix_events_w(const SeqEv* __restrict__ ev, const uint32_t* __restrict__ tiles,
                                                                    const uint32_t* __restrict__ first, const uint32_t* __restrict__ idx,
                                                                    uint32_t ntiles, unsigned char* track, uint32_t track_samples) {
    const uint32_t k = (uint32_t)sh::block_id();
    if (k >= ntiles) return;
    const uint32_t s0 = tiles[k] * shq::TILE_W + threadIdx.x * shq::LANE_SAMPLES_W;
    if (s0 >= track_samples) return;
    constexpr long long HI = WIDTH == 1 ? 127LL : (WIDTH == 3 ? 8388607LL : 2147483647LL), LO = -HI - 1;
    long long acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (s0 + j < track_samples) acc[j] = chain_get<WIDTH>(track, s0 + j);
    const uint32_t e1 = first[k + 1];
    for (uint32_t e = first[k]; e < e1; ++e) {
        const SeqEv c = ev[idx[e]];
        const unsigned char* src = (const unsigned char*)c.src;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long rel = (long long)s0 + j - (long long)c.dst;
            if (rel >= 0 && rel < (long long)c.n) {
                long long x = chain_get<WIDTH>(src, (size_t)rel);
                if (c.factor != 1.0) x = fbound((double)x * c.factor, (double)LO, (double)HI);
                const long long t = acc[j] + x;
                acc[j] = t > HI ? HI : (t < LO ? LO : t);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (s0 + j < track_samples) chain_put<WIDTH>(track, s0 + j, acc[j]);
}

// ---- events with a playback speed (sh_mix_events_rate) ----------------------------------------------------------------------------------
// One event as these kernels read it: wave-uniform again (scalar loads), 64 bytes.  inr == outr: a plain event, src its first sample.
// Otherwise src is input frame 0, and track sample dst + i is channel i % nch of output frame i / nch of audioop.ratecv(src, width,
// nch, inr, outr): the host has checked that the n samples exist (n <= out_frames(source frames) * nch), so every input frame a lane
// computes lies inside the source and the kernels test nothing but [0, n).
struct SeqEvR {
    const void* src;
    double      factor;       // audioop.mul's, after the resample; exactly 1.0: none
    double      inv_outr;     // 1.0 / outr
    uint32_t    dst, n;       // as SeqEv's, n counting RESAMPLED samples
    uint32_t    inr, outr;    // reduced rates
    uint32_t    step_q, step_r;   // inr / outr, inr % outr (shr::step)
    uint32_t    nch;
    uint32_t    small;        // 1: shr::small_int (8/16-bit samples, outr < 65536), 0: the float64 expression (shr::shifted_int)
    uint32_t    pad[2];
};
static_assert(sizeof(SeqEvR) == 64, "SeqEvR is read as one 64-byte scalar load");

// A lane's N consecutive track samples from s0 on, as a resampled event gives them: zeros outside the event (the identity of the fold,
// as seq_edge8), inside it frame m = rel / nch and channel rel % nch -- the position of the lane's first frame once (shr::position),
// then shr::step per frame -- prev = frame j - 1 (zero when j == 0 or d == 0, as k_resample), cur = frame j, both straight from global
// memory: an instrument is a few tens of KB that every note re-reads (L2 / TCP hits), and a lane's samples span about
// N / nch * speed + 2 input frames.  get(i): sample i of the source, sign-extended.
template <int WIDTH, int N, typename Get>
__device__ __forceinline__ void seq_rate(const SeqEvR& c, uint32_t s0, Get get, int (&x)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) x[k] = 0;
    const long long rel = (long long)s0 - (long long)c.dst;
    if (rel + N <= 0 || rel >= (long long)c.n) return;
    const uint32_t r0 = rel > 0 ? (uint32_t)rel : 0u;                  // the first sample of the event that this lane owns
    uint32_t m, ch;                                                     // (nch is uniform)
    if (c.nch == 1) { m = r0; ch = 0; }
    else if (c.nch == 2) { m = r0 >> 1; ch = r0 & 1u; }
    else { m = r0 / c.nch; ch = r0 - m * c.nch; }
    shr::Pos p = shr::position(m, c.inr, c.outr, c.inv_outr);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const long long r = rel + k;
        if (r < 0 || r >= (long long)c.n) continue;
        uint64_t j;
        uint32_t d;
        shr::index(p, c.outr, j, d);
        const size_t at = (size_t)j * c.nch + ch;
        const int cur = get(at);
        const int prev = (j && d) ? get(at - c.nch) : 0;
        if constexpr (WIDTH <= 2) {
            typedef typename std::conditional<WIDTH == 1, signed char, short>::type T;
            x[k] = c.small ? (int)shr::small_int<T>((T)prev, (T)cur, d, c.outr, c.inv_outr)
                           : shr::shifted_int(prev, cur, d, c.outr, c.inv_outr, 32 - 8 * WIDTH);
        } else {
            x[k] = shr::shifted_int(prev, cur, d, c.outr, c.inv_outr, 32 - 8 * WIDTH);
        }
        if (++ch == c.nch) {
            ch = 0;
            shr::step<uint64_t>(p.q, p.r, (uint64_t)c.step_q, c.step_r, c.outr);
        }
    }
}

// k_mix_events_i16 with a speed per event: the same tile, lane and fold; a plain event of a mixed list takes seq_load8's vector
// loads (a uniform branch on the record), a resampled one seq_rate.  One record ahead instead of INFLIGHT: a resampled event is sixteen
// dependent-address loads and some forty instructions per sample, which is what there is to hide behind.
template <int SCHEME>
__global__ __launch_bounds__(shq::TILE_THREADS) void k_mix_events_rate_i16(const SeqEvR* __restrict__ ev, const uint32_t* __restrict__ tiles,
                                                                           const uint32_t* __restrict__ first, const uint32_t* __restrict__ idx,
                                                                           uint32_t ntiles, short* track, uint32_t track_samples, int aligned) {
    const uint32_t k = (uint32_t)sh::block_id();
    if (k >= ntiles) return;
    const uint32_t s0 = tiles[k] * shq::TILE_I16 + threadIdx.x * shq::LANE_SAMPLES_I16;
    if (s0 >= track_samples) return;
    const bool whole = aligned && s0 + 8 <= track_samples;
    short8v acc = {0, 0, 0, 0, 0, 0, 0, 0};
    if (whole) acc = *reinterpret_cast<const short8v*>(track + s0);
    else
        for (uint32_t j = 0; j < 8 && s0 + j < track_samples; ++j) acc[j] = track[s0 + j];
    uint32_t e = first[k];
    const uint32_t e1 = first[k + 1];
    SeqEvR nx = ev[idx[e]];                                   // (an active tile lists at least one event)
    while (e < e1) {
        const SeqEvR c = nx;
        if (++e < e1) nx = ev[idx[e]];
        short8v x;
        if (c.inr == c.outr) {                                // (uniform)
            x = seq_load8<SCHEME>(SeqEv{c.src, c.factor, c.dst, c.n, {0, 0}}, s0);
        } else {
            gshort_p src = (gshort_p)c.src;
            int v[8];
            seq_rate<2, 8>(c, s0, [&](size_t i) { return (int)src[i]; }, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = (short)v[j];
        }
        if (c.factor != 1.0) x = seq_mul8(x, c.factor);       // (uniform)
        acc = __builtin_elementwise_add_sat(acc, x);
    }
    if (whole) *reinterpret_cast<short8v*>(track + s0) = acc;
    else
        for (uint32_t j = 0; j < 8 && s0 + j < track_samples; ++j) track[s0 + j] = acc[j];
}

// chain_get (pcmdev.hpp) through a pointer that says where a source lives: a pointer out of a record is read with flat loads otherwise
// (SH_SEQ_GLOBAL above).
typedef const SH_SEQ_GLOBAL unsigned char* gbyte_p;
typedef int int_u1 __attribute__((aligned(1)));
template <int WIDTH>
__device__ __forceinline__ int seq_get(gbyte_p p, size_t i) {
    if (WIDTH == 1) return (int)(signed char)p[i];
    if (WIDTH == 3) {
        gbyte_p q = p + 3 * i;
        return (int)q[0] | ((int)q[1] << 8) | ((int)(signed char)q[2] << 16);
    }
    return *(const SH_SEQ_GLOBAL int_u1*)(p + 4 * i);
}

// k_mix_events_w with a speed per event (widths 1, 3, 4): the same loop, a resampled event's four samples from seq_rate.
template <int WIDTH>
__global__ __launch_bounds__(shq::TILE_THREADS) void k_mix_events_rate_w(const SeqEvR* __restrict__ ev, const uint32_t* __restrict__ tiles,
                                                                         const uint32_t* __restrict__ first, const uint32_t* __restrict__ idx,
                                                                         uint32_t ntiles, unsigned char* track, uint32_t track_samples) {
    const uint32_t k = (uint32_t)sh::block_id();
    if (k >= ntiles) return;
    const uint32_t s0 = tiles[k] * shq::TILE_W + threadIdx.x * shq::LANE_SAMPLES_W;
    if (s0 >= track_samples) return;
    constexpr long long HI = WIDTH == 1 ? 127LL : (WIDTH == 3 ? 8388607LL : 2147483647LL), LO = -HI - 1;
    long long acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (s0 + j < track_samples) acc[j] = chain_get<WIDTH>(track, s0 + j);
    const uint32_t e1 = first[k + 1];
    for (uint32_t e = first[k]; e < e1; ++e) {
        const SeqEvR c = ev[idx[e]];
        gbyte_p src = (gbyte_p)c.src;
        int v[4] = {0, 0, 0, 0};
        bool in[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long rel = (long long)s0 + j - (long long)c.dst;
            in[j] = rel >= 0 && rel < (long long)c.n;
        }
        if (c.inr == c.outr) {                                // (uniform)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (in[j]) v[j] = seq_get<WIDTH>(src, (size_t)((long long)s0 + j - (long long)c.dst));
        } else {
            seq_rate<WIDTH, 4>(c, s0, [&](size_t i) { return seq_get<WIDTH>(src, i); }, v);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (in[j]) {
                long long x = v[j];
                if (c.factor != 1.0) x = fbound((double)x * c.factor, (double)LO, (double)HI);
                const long long t = acc[j] + x;
                acc[j] = t > HI ? HI : (t < LO ? LO : t);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (s0 + j < track_samples) chain_put<WIDTH>(track, s0 + j, acc[j]);
}

// ---- mono sources panned into a stereo track (sh_mix_events_pan) ------------------------------------------------------------------------
// One event as these kernels read it: SeqEvR and audioop.tostereo's two factors, wave-uniform (scalar loads), 96 bytes.  r.nch is the
// SOURCE's channel count.  2: an event of the kernels above, left and right unused.  1: r.dst and r.n count TRACK samples, both even --
// track frame r.dst / 2 + f is frame f of the mono source (plain) or of audioop.ratecv(src, width, 1, inr, outr) (resampled) through
// tostereo, (fbound(s * left), fbound(s * right)), then the mul and the add of every event: ratecv, tostereo, mul, add, in that order.
struct SeqEvP {
    SeqEvR   r;
    double   left, right;
    uint32_t pad[4];
};
static_assert(sizeof(SeqEvP) == 96, "SeqEvP is read as a 64-byte and a 32-byte scalar load");

typedef short short4v __attribute__((ext_vector_type(4)));
typedef short short4u __attribute__((ext_vector_type(4), aligned(2)));      // four samples at any sample offset
typedef int int2v __attribute__((ext_vector_type(2)));

// seq_load8 for a mono source: a lane's eight track samples are four stereo frames, so four source samples -- eight bytes, at
// (src - 2 dstf) mod 8 against the lane's aligned eight (all lanes start on multiples of four track frames: uniform per event).
// FUNNEL: one aligned 8-byte load, or two and the funnel shift; VEC2: one load at the odd address; the edges sample by sample.
template <int SCHEME>
__device__ __forceinline__ short4v seq_load4(gshort_p src, uint32_t dstf, uint32_t nf, uint32_t f0) {
    const long long rel = (long long)f0 - (long long)dstf;
    short4v x = {0, 0, 0, 0};
    if (rel + 4 <= 0 || rel >= (long long)nf) return x;
    if constexpr (SCHEME == VEC2) {
        if (rel >= 0 && rel + 4 <= (long long)nf) return *(const SH_SEQ_GLOBAL short4u*)(src + rel);
    } else {
        const uint32_t sh = (uint32_t)(((uintptr_t)src - 2 * (uintptr_t)dstf) & 7);          // (uniform) 0, 2, 4, 6
        if (sh == 0) {
            if (rel >= 0 && rel + 4 <= (long long)nf) return *(const SH_SEQ_GLOBAL short4v*)(src + rel);
        } else if (rel >= 4 && rel + 8 <= (long long)nf) {
            const SH_SEQ_GLOBAL int2v* q = (const SH_SEQ_GLOBAL int2v*)((uintptr_t)(src + rel) - sh);
            const int2v lo = q[0], hi = q[1];
            const uint32_t r = sh & 3;
            union { int2v v; short4v s; } o;
            if (sh < 4) o.v = (int2v){(int)__builtin_amdgcn_alignbyte(lo[1], lo[0], r), (int)__builtin_amdgcn_alignbyte(hi[0], lo[1], r)};
            else o.v = (int2v){(int)__builtin_amdgcn_alignbyte(hi[0], lo[1], r), (int)__builtin_amdgcn_alignbyte(hi[1], hi[0], r)};
            return o.s;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (rel + j >= 0 && rel + j < (long long)nf) x[j] = src[rel + j];
    return x;
}

// a resampled mono event in frames: seq_rate's record counts what it resamples
__device__ __forceinline__ SeqEvR seq_mono_frames(const SeqEvR& r) {
    SeqEvR f = r;
    f.dst = r.dst >> 1;
    f.n = r.n >> 1;
    return f;
}

// k_mix_events_rate_i16 with mono sources beside stereo ones: the same tile, lane and fold, one record ahead.  A stereo event exactly
// as there; a mono one fetches four frames -- seq_load4's vector loads (plain) or seq_rate with nch == 1 (resampled), half the source
// bytes of a stereo event -- and makes them stereo in registers.  Zeros outside the event stay zeros: fbound(0 * factor) == 0.
template <int SCHEME>
__global__ __launch_bounds__(shq::TILE_THREADS) void k_mix_events_pan_i16(const SeqEvP* __restrict__ ev, const uint32_t* __restrict__ tiles,
                                                                          const uint32_t* __restrict__ first, const uint32_t* __restrict__ idx,
                                                                          uint32_t ntiles, short* track, uint32_t track_samples, int aligned) {
    const uint32_t k = (uint32_t)sh::block_id();
    if (k >= ntiles) return;
    const uint32_t s0 = tiles[k] * shq::TILE_I16 + threadIdx.x * shq::LANE_SAMPLES_I16;
    if (s0 >= track_samples) return;
    const bool whole = aligned && s0 + 8 <= track_samples;
    short8v acc = {0, 0, 0, 0, 0, 0, 0, 0};
    if (whole) acc = *reinterpret_cast<const short8v*>(track + s0);
    else
        for (uint32_t j = 0; j < 8 && s0 + j < track_samples; ++j) acc[j] = track[s0 + j];
    uint32_t e = first[k];
    const uint32_t e1 = first[k + 1];
    SeqEvP nx = ev[idx[e]];                                   // (an active tile lists at least one event)
    while (e < e1) {
        const SeqEvP c = nx;
        if (++e < e1) nx = ev[idx[e]];
        gshort_p src = (gshort_p)c.r.src;
        short8v x;
        if (c.r.nch == 2) {                                   // (uniform, as every branch on the record)
            if (c.r.inr == c.r.outr) {
                x = seq_load8<SCHEME>(SeqEv{c.r.src, c.r.factor, c.r.dst, c.r.n, {0, 0}}, s0);
            } else {
                int v[8];
                seq_rate<2, 8>(c.r, s0, [&](size_t i) { return (int)src[i]; }, v);
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = (short)v[j];
            }
        } else {
            short4v m;
            if (c.r.inr == c.r.outr) {
                m = seq_load4<SCHEME>(src, c.r.dst >> 1, c.r.n >> 1, s0 >> 1);
            } else {
                int v[4];
                seq_rate<2, 4>(seq_mono_frames(c.r), s0 >> 1, [&](size_t i) { return (int)src[i]; }, v);
#pragma unroll
                for (int j = 0; j < 4; ++j) m[j] = (short)v[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double s = (double)m[j];
                x[2 * j] = (short)fbound(s * c.left, Lim<short>::lo, Lim<short>::hi);
                x[2 * j + 1] = (short)fbound(s * c.right, Lim<short>::lo, Lim<short>::hi);
            }
        }
        if (c.r.factor != 1.0) x = seq_mul8(x, c.r.factor);
        acc = __builtin_elementwise_add_sat(acc, x);
    }
    if (whole) *reinterpret_cast<short8v*>(track + s0) = acc;
    else
        for (uint32_t j = 0; j < 8 && s0 + j < track_samples; ++j) track[s0 + j] = acc[j];
}

// k_mix_events_rate_w with mono sources beside stereo ones (widths 1, 3, 4): a thread's four track samples are two stereo frames.
template <int WIDTH>
__global__ __launch_bounds__(shq::TILE_THREADS) void k_mix_events_pan_w(const SeqEvP* __restrict__ ev, const uint32_t* __restrict__ tiles,
                                                                        const uint32_t* __restrict__ first, const uint32_t* __restrict__ idx,
                                                                        uint32_t ntiles, unsigned char* track, uint32_t track_samples) {
    const uint32_t k = (uint32_t)sh::block_id();
    if (k >= ntiles) return;
    const uint32_t s0 = tiles[k] * shq::TILE_W + threadIdx.x * shq::LANE_SAMPLES_W;
    if (s0 >= track_samples) return;
    constexpr long long HI = WIDTH == 1 ? 127LL : (WIDTH == 3 ? 8388607LL : 2147483647LL), LO = -HI - 1;
    long long acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (s0 + j < track_samples) acc[j] = chain_get<WIDTH>(track, s0 + j);
    const uint32_t e1 = first[k + 1];
    for (uint32_t e = first[k]; e < e1; ++e) {
        const SeqEvP c = ev[idx[e]];
        gbyte_p src = (gbyte_p)c.r.src;
        int v[4] = {0, 0, 0, 0};
        bool in[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long rel = (long long)s0 + j - (long long)c.r.dst;
            in[j] = rel >= 0 && rel < (long long)c.r.n;
        }
        if (c.r.nch == 2) {                                   // (uniform, as every branch on the record)
            if (c.r.inr == c.r.outr) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (in[j]) v[j] = seq_get<WIDTH>(src, (size_t)((long long)s0 + j - (long long)c.r.dst));
            } else {
                seq_rate<WIDTH, 4>(c.r, s0, [&](size_t i) { return seq_get<WIDTH>(src, i); }, v);
            }
        } else {
            int m[2] = {0, 0};
            if (c.r.inr == c.r.outr) {
#pragma unroll
                for (int f = 0; f < 2; ++f)                   // (dst, n and s0 are even: a frame is inside the event or outside it)
                    if (in[2 * f]) m[f] = seq_get<WIDTH>(src, (size_t)((long long)(s0 >> 1) + f - (long long)(c.r.dst >> 1)));
            } else {
                seq_rate<WIDTH, 2>(seq_mono_frames(c.r), s0 >> 1, [&](size_t i) { return seq_get<WIDTH>(src, i); }, m);
            }
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                const double s = (double)m[f];
                v[2 * f] = fbound(s * c.left, (double)LO, (double)HI);
                v[2 * f + 1] = fbound(s * c.right, (double)LO, (double)HI);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (in[j]) {
                long long x = v[j];
                if (c.r.factor != 1.0) x = fbound((double)x * c.r.factor, (double)LO, (double)HI);
                const long long t = acc[j] + x;
                acc[j] = t > HI ? HI : (t < LO ? LO : t);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (s0 + j < track_samples) chain_put<WIDTH>(track, s0 + j, acc[j]);
}

// ---- an ADSR envelope per event (sh_mix_events_env) -------------------------------------------------------------------------------------
// One event as these kernels read it: SeqEvP with its padding put to use, wave-uniform (scalar loads), 96 bytes.  r.nch is the SOURCE's
// channel count.  tostereo == 0: an event of the rate kernels (any channel count, the track's).  tostereo == 1: a mono source into a
// stereo track, as SeqEvP's.  nseg > 0: segs[seg0 .. seg0 + nseg) (she::Seg, seqenv.hpp) shape the event's source samples -- the samples
// of the mono frames for a tostereo event -- after the load or the ratecv and before tostereo and the mul: ratecv, the cut, the
// envelope, tostereo, mul, add, in that order.
struct SeqEvE {
    SeqEvR   r;
    double   left, right;
    uint32_t seg0, nseg;
    uint32_t tostereo;
    uint32_t pad;
};
static_assert(sizeof(SeqEvE) == 96, "SeqEvE is read as a 64-byte and a 32-byte scalar load");

// What the tile [t0, t0 + tile) of the track takes of an event, in the event's source samples (sh = 1: a tostereo event, whose source
// samples are track frames; dst, n, t0 and tile are even then): [tlo, thi), uniform.  The tile lists the event, so they overlap.
__device__ __forceinline__ void seq_env_span(const SeqEvE& c, uint32_t t0, uint32_t tile, uint32_t& tlo, uint32_t& thi) {
    const uint32_t sh = c.tostereo, d = c.r.dst >> sh, n = c.r.n >> sh, a = t0 >> sh, b = a + (tile >> sh);       // (no wrap: MAX_TRACK_SAMPLES)
    tlo = a > d ? a - d : 0u;
    thi = (b < d + n ? b : d + n) - d;
}

// k_mix_events_pan_i16 with an envelope per event: the same tile, lane ownership, accumulator in registers and one record ahead.  An
// event without an envelope takes the paths of that kernel behind a uniform branch (nseg == 0); an enveloped one shapes the lane's eight
// source samples (four mono frames for a tostereo event) with she::shape_lane -- float64 per sample only inside a ramp, one fbound
// multiply inside the sustain, nothing inside a plain stretch, a per-sample select only in a tile that straddles a boundary.
template <int SCHEME>
__global__ __launch_bounds__(shq::TILE_THREADS) void k_mix_events_env_i16(const SeqEvE* __restrict__ ev, const she::Seg* __restrict__ segs,
                                                                          const uint32_t* __restrict__ tiles, const uint32_t* __restrict__ first,
                                                                          const uint32_t* __restrict__ idx, uint32_t ntiles, short* track,
                                                                          uint32_t track_samples, int aligned) {
    const uint32_t k = (uint32_t)sh::block_id();
    if (k >= ntiles) return;
    const uint32_t t0 = tiles[k] * shq::TILE_I16;
    const uint32_t s0 = t0 + threadIdx.x * shq::LANE_SAMPLES_I16;
    if (s0 >= track_samples) return;
    const bool whole = aligned && s0 + 8 <= track_samples;
    short8v acc = {0, 0, 0, 0, 0, 0, 0, 0};
    if (whole) acc = *reinterpret_cast<const short8v*>(track + s0);
    else
        for (uint32_t j = 0; j < 8 && s0 + j < track_samples; ++j) acc[j] = track[s0 + j];
    uint32_t e = first[k];
    const uint32_t e1 = first[k + 1];
    SeqEvE nx = ev[idx[e]];                                   // (an active tile lists at least one event)
    while (e < e1) {
        const SeqEvE c = nx;
        if (++e < e1) nx = ev[idx[e]];
        gshort_p src = (gshort_p)c.r.src;
        uint32_t tlo = 0, thi = 0;
        if (c.nseg) seq_env_span(c, t0, shq::TILE_I16, tlo, thi);      // (uniform, as every branch on the record)
        short8v x;
        if (!c.tostereo) {
            if (c.r.inr == c.r.outr) {
                x = seq_load8<SCHEME>(SeqEv{c.r.src, c.r.factor, c.r.dst, c.r.n, {0, 0}}, s0);
                if (c.nseg) {
                    int v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = (int)x[j];
                    she::shape_lane<8>(segs + c.seg0, c.nseg, tlo, thi, (long long)s0 - (long long)c.r.dst, v, Lim<short>::lo, Lim<short>::hi);
#pragma unroll
                    for (int j = 0; j < 8; ++j) x[j] = (short)v[j];
                }
            } else {
                int v[8];
                seq_rate<2, 8>(c.r, s0, [&](size_t i) { return (int)src[i]; }, v);
                if (c.nseg) she::shape_lane<8>(segs + c.seg0, c.nseg, tlo, thi, (long long)s0 - (long long)c.r.dst, v, Lim<short>::lo, Lim<short>::hi);
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = (short)v[j];
            }
        } else {
            int v[4];
            if (c.r.inr == c.r.outr) {
                const short4v m = seq_load4<SCHEME>(src, c.r.dst >> 1, c.r.n >> 1, s0 >> 1);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (int)m[j];
            } else {
                seq_rate<2, 4>(seq_mono_frames(c.r), s0 >> 1, [&](size_t i) { return (int)src[i]; }, v);
            }
            if (c.nseg) she::shape_lane<4>(segs + c.seg0, c.nseg, tlo, thi, (long long)(s0 >> 1) - (long long)(c.r.dst >> 1), v, Lim<short>::lo, Lim<short>::hi);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double s = (double)v[j];
                x[2 * j] = (short)fbound(s * c.left, Lim<short>::lo, Lim<short>::hi);
                x[2 * j + 1] = (short)fbound(s * c.right, Lim<short>::lo, Lim<short>::hi);
            }
        }
        if (c.r.factor != 1.0) x = seq_mul8(x, c.r.factor);
        acc = __builtin_elementwise_add_sat(acc, x);
    }
    if (whole) *reinterpret_cast<short8v*>(track + s0) = acc;
    else
        for (uint32_t j = 0; j < 8 && s0 + j < track_samples; ++j) track[s0 + j] = acc[j];
}

// k_mix_events_pan_w with an envelope per event (widths 1 and 4: upstream's fades have no 24-bit form): a thread's four track samples
// are four source samples, or two mono frames of a tostereo event.
template <int WIDTH>
__global__ __launch_bounds__(shq::TILE_THREADS) void k_mix_events_env_w(const SeqEvE* __restrict__ ev, const she::Seg* __restrict__ segs,
                                                                        const uint32_t* __restrict__ tiles, const uint32_t* __restrict__ first,
                                                                        const uint32_t* __restrict__ idx, uint32_t ntiles, unsigned char* track,
                                                                        uint32_t track_samples) {
    static_assert(WIDTH == 1 || WIDTH == 4, "an envelope has widths 1, 2 and 4");
    const uint32_t k = (uint32_t)sh::block_id();
    if (k >= ntiles) return;
    const uint32_t t0 = tiles[k] * shq::TILE_W;
    const uint32_t s0 = t0 + threadIdx.x * shq::LANE_SAMPLES_W;
    if (s0 >= track_samples) return;
    constexpr long long HI = WIDTH == 1 ? 127LL : 2147483647LL, LO = -HI - 1;
    long long acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (s0 + j < track_samples) acc[j] = chain_get<WIDTH>(track, s0 + j);
    const uint32_t e1 = first[k + 1];
    for (uint32_t e = first[k]; e < e1; ++e) {
        const SeqEvE c = ev[idx[e]];
        gbyte_p src = (gbyte_p)c.r.src;
        uint32_t tlo = 0, thi = 0;
        if (c.nseg) seq_env_span(c, t0, shq::TILE_W, tlo, thi);        // (uniform, as every branch on the record)
        int v[4] = {0, 0, 0, 0};
        bool in[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long rel = (long long)s0 + j - (long long)c.r.dst;
            in[j] = rel >= 0 && rel < (long long)c.r.n;
        }
        if (!c.tostereo) {
            if (c.r.inr == c.r.outr) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (in[j]) v[j] = seq_get<WIDTH>(src, (size_t)((long long)s0 + j - (long long)c.r.dst));
            } else {
                seq_rate<WIDTH, 4>(c.r, s0, [&](size_t i) { return seq_get<WIDTH>(src, i); }, v);
            }
            if (c.nseg) she::shape_lane<4>(segs + c.seg0, c.nseg, tlo, thi, (long long)s0 - (long long)c.r.dst, v, (double)LO, (double)HI);
        } else {
            int m[2] = {0, 0};
            if (c.r.inr == c.r.outr) {
#pragma unroll
                for (int f = 0; f < 2; ++f)                   // (dst, n and s0 are even: a frame is inside the event or outside it)
                    if (in[2 * f]) m[f] = seq_get<WIDTH>(src, (size_t)((long long)(s0 >> 1) + f - (long long)(c.r.dst >> 1)));
            } else {
                seq_rate<WIDTH, 2>(seq_mono_frames(c.r), s0 >> 1, [&](size_t i) { return seq_get<WIDTH>(src, i); }, m);
            }
            if (c.nseg) she::shape_lane<2>(segs + c.seg0, c.nseg, tlo, thi, (long long)(s0 >> 1) - (long long)(c.r.dst >> 1), m, (double)LO, (double)HI);
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                const double s = (double)m[f];
                v[2 * f] = fbound(s * c.left, (double)LO, (double)HI);
                v[2 * f + 1] = fbound(s * c.right, (double)LO, (double)HI);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (in[j]) {
                long long x = v[j];
                if (c.r.factor != 1.0) x = fbound((double)x * c.r.factor, (double)LO, (double)HI);
                const long long t = acc[j] + x;
                acc[j] = t > HI ? HI : (t < LO ? LO : t);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (s0 + j < track_samples) chain_put<WIDTH>(track, s0 + j, acc[j]);
}

}  // namespace

// ---- host: what the entry points share ----------------------------------------------------------------------------------------------
namespace {

// the arguments in front of the events: width, pointers, the track's range, no source that is (or overlaps) the track
int seq_check_args(const char* fn, const sh_buf* const* srcs, uint32_t nsrc, const void* events, uint32_t nevents, int width,
                   const sh_buf* track, size_t track_samples) {
    if (width < 1 || width > 4) return sh::set_error(SH_ERR_INVALID, "%s: width %d not in {1, 2, 3, 4}", fn, width);
    if (!track || (nevents && !events) || (nsrc && !srcs)) return sh::set_error(SH_ERR_INVALID, "%s: NULL argument", fn);
    const size_t w = (size_t)width;
    if (track_samples > track->bytes / w) return sh::set_error(SH_ERR_INVALID, "%s: track range outside buffer", fn);
    const char* t0 = (const char*)track->ptr;
    const char* t1 = t0 + track_samples * w;
    for (uint32_t v = 0; v < nsrc; ++v) {
        if (!srcs[v]) continue;
        const char* p = (const char*)srcs[v]->ptr;
        if (srcs[v] == track || (p < t1 && t0 < p + srcs[v]->bytes)) return sh::set_error(SH_ERR_INVALID, "%s: source %u is the track", fn, v);
    }
    return SH_OK;
}

// what every event is asked, whatever its kind
template <typename Ev>
int seq_check_event(const char* fn, const Ev& m, uint32_t e, const sh_buf* const* srcs, uint32_t nsrc) {
    if (m.reserved != 0) return sh::set_error(SH_ERR_INVALID, "%s: event %u: reserved must be 0", fn, e);
    if (!isfinite(m.factor)) return sh::set_error(SH_ERR_INVALID, "%s: event %u: factor is not finite", fn, e);
    if (m.src >= nsrc || !srcs[m.src]) return sh::set_error(SH_ERR_INVALID, "%s: event %u: no source %u", fn, e, m.src);
    return SH_OK;
}

// The plan of the checked events (dst, n), then records | tiles | first | idx as one block on the library's grow-only scratch, one copy,
// one launch: fill(rec) writes the nevents records, launch(records, tiles, first, idx, ntiles, grid, block, stream) names the kernel.
// after_records: bytes of a second table (a multiple of 16) that fill writes behind the records and the kernel finds there.
template <typename Rec, typename Fill, typename Launch>
int seq_run(const char* fn, const std::vector<shq::Event>& pe, int width, size_t track_samples, Fill fill, Launch launch, size_t after_records = 0) {
    const uint32_t nevents = (uint32_t)pe.size();
    const uint32_t tile = shq::tile_samples(width);
    const shq::Plan P = shq::plan(pe.data(), nevents, track_samples, tile);
    if (P.refused == shq::EVENT_BEYOND_TRACK) return sh::set_error(SH_ERR_INVALID, "%s: event %u: range outside the track", fn, P.bad_event);
    if (P.refused == shq::TRACK_TOO_LONG) return sh::set_error(SH_ERR_INVALID, "%s: at most 2^32 - 65536 track samples per call", fn);
    if (P.refused) return sh::set_error(SH_ERR_INVALID, "%s: more than 2^28 (event, tile) overlaps in one call", fn);
    if (P.tiles.empty()) return SH_OK;
    const uint32_t nt = (uint32_t)P.tiles.size();
    const size_t b_ev = (size_t)nevents * sizeof(Rec) + after_records, b_tiles = (size_t)nt * 4, b_first = ((size_t)nt + 1) * 4, b_idx = P.idx.size() * 4;
    std::vector<char> host(b_ev + b_tiles + b_first + b_idx);
    fill(reinterpret_cast<Rec*>(host.data()));
    memcpy(host.data() + b_ev, P.tiles.data(), b_tiles);
    memcpy(host.data() + b_ev + b_tiles, P.first.data(), b_first);
    memcpy(host.data() + b_ev + b_tiles + b_first, P.idx.data(), b_idx);
    int rc = sh::ensure_scratch(host.size());
    if (rc) return rc;
    hipStream_t st = sh::state().stream;
    char* dev = (char*)sh::state().scratch;
    // (pageable source: staged before the call returns, ordered after earlier kernels)
    SH_HIP(hipMemcpyAsync(dev, host.data(), host.size(), hipMemcpyHostToDevice, st));
    launch((const Rec*)dev, (const uint32_t*)(dev + b_ev), (const uint32_t*)(dev + b_ev + b_tiles), (const uint32_t*)(dev + b_ev + b_tiles + b_first),
           nt, sh::grid1d(nt, 1), dim3(shq::TILE_THREADS), st);
    SH_CHECK_LAUNCH(fn);
    return SH_OK;
}

}  // namespace

extern "C" {

int sh_mix_events(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event* events, uint32_t nevents, int width, sh_buf* track,
                  size_t track_samples) {
    SH_REQUIRE_INIT();
    static const char fn[] = "sh_mix_events";
    int rc = seq_check_args(fn, srcs, nsrc, events, nevents, width, track, track_samples);
    if (rc) return rc;
    const size_t w = (size_t)width;
    std::vector<shq::Event> pe(nevents);
    for (uint32_t e = 0; e < nevents; ++e) {
        const sh_mix_event& m = events[e];
        if ((rc = seq_check_event(fn, m, e, srcs, nsrc))) return rc;
        const size_t have = srcs[m.src]->bytes / w;
        if (m.src_sample > have || m.nsamples > have - m.src_sample)
            return sh::set_error(SH_ERR_INVALID, "%s: event %u: range outside its source", fn, e);
        pe[e] = shq::Event{m.dst_sample, m.nsamples};
    }
    const uint32_t ns = (uint32_t)track_samples;
    return seq_run<SeqEv>(fn, pe, width, track_samples,
        [&](SeqEv* rec) {
            for (uint32_t e = 0; e < nevents; ++e) {
                const sh_mix_event& m = events[e];
                rec[e] = SeqEv{(const char*)srcs[m.src]->ptr + m.src_sample * w, m.factor, (uint32_t)m.dst_sample, (uint32_t)m.nsamples, {0, 0}};
            }
        },
        [&](const SeqEv* d_ev, const uint32_t* d_tiles, const uint32_t* d_first, const uint32_t* d_idx, uint32_t nt, dim3 grid, dim3 block, hipStream_t st) {
            if (width == 2) {
                const int aligned = ((uintptr_t)track->ptr & 15) == 0;
                if (sh::knobs().seq_align == VEC2) hipLaunchKernelGGL((k_mix_events_i16<VEC2, 4>), grid, block, 0, st, d_ev, d_tiles, d_first, d_idx, nt, (short*)track->ptr, ns, aligned);
                else hipLaunchKernelGGL((k_mix_events_i16<FUNNEL, 4>), grid, block, 0, st, d_ev, d_tiles, d_first, d_idx, nt, (short*)track->ptr, ns, aligned);
            }
            else if (width == 1) hipLaunchKernelGGL(k_mix_events_w<1>, grid, block, 0, st, d_ev, d_tiles, d_first, d_idx, nt, (unsigned char*)track->ptr, ns);
            else if (width == 3) hipLaunchKernelGGL(k_mix_events_w<3>, grid, block, 0, st, d_ev, d_tiles, d_first, d_idx, nt, (unsigned char*)track->ptr, ns);
            else hipLaunchKernelGGL(k_mix_events_w<4>, grid, block, 0, st, d_ev, d_tiles, d_first, d_idx, nt, (unsigned char*)track->ptr, ns);
        });
}

int sh_mix_events_rate(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event_rate* events, uint32_t nevents, int width, int nchannels,
                       sh_buf* track, size_t track_samples) {
    SH_REQUIRE_INIT();
    static const char fn[] = "sh_mix_events_rate";
    int rc = seq_check_args(fn, srcs, nsrc, events, nevents, width, track, track_samples);
    if (rc) return rc;
    if (nchannels < 1) return sh::set_error(SH_ERR_INVALID, "%s: # of channels should be >= 1", fn);
    const size_t w = (size_t)width;
    const uint64_t nch = (uint64_t)nchannels;
    std::vector<shq::Event> pe(nevents);
    for (uint32_t e = 0; e < nevents; ++e) {
        const sh_mix_event_rate& m = events[e];
        if ((rc = seq_check_event(fn, m, e, srcs, nsrc))) return rc;
        if (!m.inrate || !m.outrate || m.inrate >= (1u << 31) || m.outrate >= (1u << 31))
            return sh::set_error(SH_ERR_INVALID, "%s: event %u: sampling rate not in [1, 2^31)", fn, e);
        const uint64_t have = srcs[m.src]->bytes / w;
        if (m.src_sample > have) return sh::set_error(SH_ERR_INVALID, "%s: event %u: range outside its source", fn, e);
        if (m.inrate == m.outrate) {
            if (m.nsamples > have - m.src_sample) return sh::set_error(SH_ERR_INVALID, "%s: event %u: range outside its source", fn, e);
        } else {
            if (m.src_sample % nch || m.nsamples % nch)
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: a resampled event starts and ends on whole frames", fn, e);
            if (m.src_frames > (have - m.src_sample) / nch) return sh::set_error(SH_ERR_INVALID, "%s: event %u: src_frames outside its source", fn, e);
            if (m.nsamples / nch > shr::out_frames(m.src_frames, shr::reduce(m.inrate, m.outrate)))
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: more samples than src_frames resample to", fn, e);
        }
        pe[e] = shq::Event{m.dst_sample, m.nsamples};
    }
    const uint32_t ns = (uint32_t)track_samples;
    return seq_run<SeqEvR>(fn, pe, width, track_samples,
        [&](SeqEvR* rec) {
            for (uint32_t e = 0; e < nevents; ++e) {
                const sh_mix_event_rate& m = events[e];
                const shr::Rates R = shr::reduce(m.inrate, m.outrate);
                rec[e] = SeqEvR{(const char*)srcs[m.src]->ptr + m.src_sample * w, m.factor, 1.0 / (double)R.outr, (uint32_t)m.dst_sample,
                                (uint32_t)m.nsamples, R.inr, R.outr, R.inr / R.outr, R.inr % R.outr, (uint32_t)nchannels,
                                width <= 2 && R.outr < 65536u ? 1u : 0u, {0, 0}};
            }
        },
        [&](const SeqEvR* d_ev, const uint32_t* d_tiles, const uint32_t* d_first, const uint32_t* d_idx, uint32_t nt, dim3 grid, dim3 block, hipStream_t st) {
            if (width == 2) {
                const int aligned = ((uintptr_t)track->ptr & 15) == 0;
                if (sh::knobs().seq_align == VEC2) hipLaunchKernelGGL(k_mix_events_rate_i16<VEC2>, grid, block, 0, st, d_ev, d_tiles, d_first, d_idx, nt, (short*)track->ptr, ns, aligned);
                else hipLaunchKernelGGL(k_mix_events_rate_i16<FUNNEL>, grid, block, 0, st, d_ev, d_tiles, d_first, d_idx, nt, (short*)track->ptr, ns, aligned);
            }
            else if (width == 1) hipLaunchKernelGGL(k_mix_events_rate_w<1>, grid, block, 0, st, d_ev, d_tiles, d_first, d_idx, nt, (unsigned char*)track->ptr, ns);
            else if (width == 3) hipLaunchKernelGGL(k_mix_events_rate_w<3>, grid, block, 0, st, d_ev, d_tiles, d_first, d_idx, nt, (unsigned char*)track->ptr, ns);
            else hipLaunchKernelGGL(k_mix_events_rate_w<4>, grid, block, 0, st, d_ev, d_tiles, d_first, d_idx, nt, (unsigned char*)track->ptr, ns);
        });
}

int sh_mix_events_pan(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event_pan* events, uint32_t nevents, int width, sh_buf* track,
                      size_t track_samples) {
    SH_REQUIRE_INIT();
    static const char fn[] = "sh_mix_events_pan";
    int rc = seq_check_args(fn, srcs, nsrc, events, nevents, width, track, track_samples);
    if (rc) return rc;
    const size_t w = (size_t)width;
    std::vector<shq::Event> pe(nevents);
    for (uint32_t e = 0; e < nevents; ++e) {
        const sh_mix_event_pan& m = events[e];
        if ((rc = seq_check_event(fn, m, e, srcs, nsrc))) return rc;
        if (m.src_channels != 1 && m.src_channels != 2) return sh::set_error(SH_ERR_INVALID, "%s: event %u: src_channels %u not 1 or 2", fn, e, m.src_channels);
        if (!m.inrate || !m.outrate || m.inrate >= (1u << 31) || m.outrate >= (1u << 31))
            return sh::set_error(SH_ERR_INVALID, "%s: event %u: sampling rate not in [1, 2^31)", fn, e);
        const uint64_t nch = m.src_channels, have = srcs[m.src]->bytes / w;
        uint64_t nsrc_samples = m.nsamples;                   // what the event takes of its (resampled) source
        if (nch == 1) {
            if (!isfinite(m.left) || !isfinite(m.right)) return sh::set_error(SH_ERR_INVALID, "%s: event %u: left / right is not finite", fn, e);
            if (m.dst_sample % 2 || m.nsamples % 2)
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: a mono source starts and ends on whole stereo frames", fn, e);
            nsrc_samples = m.nsamples / 2;
        }
        if (m.src_sample > have) return sh::set_error(SH_ERR_INVALID, "%s: event %u: range outside its source", fn, e);
        if (m.inrate == m.outrate) {
            if (nsrc_samples > have - m.src_sample) return sh::set_error(SH_ERR_INVALID, "%s: event %u: range outside its source", fn, e);
        } else {
            if (m.src_sample % nch || nsrc_samples % nch)
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: a resampled event starts and ends on whole frames", fn, e);
            if (m.src_frames > (have - m.src_sample) / nch) return sh::set_error(SH_ERR_INVALID, "%s: event %u: src_frames outside its source", fn, e);
            if (nsrc_samples / nch > shr::out_frames(m.src_frames, shr::reduce(m.inrate, m.outrate)))
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: more samples than src_frames resample to", fn, e);
        }
        pe[e] = shq::Event{m.dst_sample, m.nsamples};
    }
    const uint32_t ns = (uint32_t)track_samples;
    return seq_run<SeqEvP>(fn, pe, width, track_samples,
        [&](SeqEvP* rec) {
            for (uint32_t e = 0; e < nevents; ++e) {
                const sh_mix_event_pan& m = events[e];
                const shr::Rates R = shr::reduce(m.inrate, m.outrate);
                rec[e] = SeqEvP{SeqEvR{(const char*)srcs[m.src]->ptr + m.src_sample * w, m.factor, 1.0 / (double)R.outr, (uint32_t)m.dst_sample,
                                       (uint32_t)m.nsamples, R.inr, R.outr, R.inr / R.outr, R.inr % R.outr, m.src_channels,
                                       width <= 2 && R.outr < 65536u ? 1u : 0u, {0, 0}},
                                m.left, m.right, {0, 0, 0, 0}};
            }
        },
        [&](const SeqEvP* d_ev, const uint32_t* d_tiles, const uint32_t* d_first, const uint32_t* d_idx, uint32_t nt, dim3 grid, dim3 block, hipStream_t st) {
            if (width == 2) {
                const int aligned = ((uintptr_t)track->ptr & 15) == 0;
                if (sh::knobs().seq_align == VEC2) hipLaunchKernelGGL(k_mix_events_pan_i16<VEC2>, grid, block, 0, st, d_ev, d_tiles, d_first, d_idx, nt, (short*)track->ptr, ns, aligned);
                else hipLaunchKernelGGL(k_mix_events_pan_i16<FUNNEL>, grid, block, 0, st, d_ev, d_tiles, d_first, d_idx, nt, (short*)track->ptr, ns, aligned);
            }
            else if (width == 1) hipLaunchKernelGGL(k_mix_events_pan_w<1>, grid, block, 0, st, d_ev, d_tiles, d_first, d_idx, nt, (unsigned char*)track->ptr, ns);
            else if (width == 3) hipLaunchKernelGGL(k_mix_events_pan_w<3>, grid, block, 0, st, d_ev, d_tiles, d_first, d_idx, nt, (unsigned char*)track->ptr, ns);
            else hipLaunchKernelGGL(k_mix_events_pan_w<4>, grid, block, 0, st, d_ev, d_tiles, d_first, d_idx, nt, (unsigned char*)track->ptr, ns);
        });
}

int sh_mix_events_env(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event_env* events, uint32_t nevents,
                      const sh_env_segment* segments, uint32_t nsegments, int width, int nchannels, sh_buf* track, size_t track_samples) {
    SH_REQUIRE_INIT();
    static const char fn[] = "sh_mix_events_env";
    if (width == 3) return sh::set_error(SH_ERR_INVALID, "%s: width 3: an envelope's fades have no 24-bit form", fn);
    int rc = seq_check_args(fn, srcs, nsrc, events, nevents, width, track, track_samples);
    if (rc) return rc;
    if (nchannels < 1) return sh::set_error(SH_ERR_INVALID, "%s: # of channels should be >= 1", fn);
    if (nsegments && !segments) return sh::set_error(SH_ERR_INVALID, "%s: NULL argument", fn);
    const size_t w = (size_t)width;
    std::vector<shq::Event> pe(nevents);
    for (uint32_t e = 0; e < nevents; ++e) {
        const sh_mix_event_env& m = events[e];
        if ((rc = seq_check_event(fn, m, e, srcs, nsrc))) return rc;
        const bool tostereo = m.src_channels == 1 && nchannels == 2;
        if (!tostereo && m.src_channels != (uint32_t)nchannels)
            return sh::set_error(SH_ERR_INVALID, "%s: event %u: src_channels %u is neither the track's %d nor a mono source of a stereo track", fn, e, m.src_channels, nchannels);
        if (!m.inrate || !m.outrate || m.inrate >= (1u << 31) || m.outrate >= (1u << 31))
            return sh::set_error(SH_ERR_INVALID, "%s: event %u: sampling rate not in [1, 2^31)", fn, e);
        const uint64_t nch = m.src_channels, have = srcs[m.src]->bytes / w;
        uint64_t nsrc_samples = m.nsamples;                   // what the event takes of its (resampled) source
        if (tostereo) {
            if (!isfinite(m.left) || !isfinite(m.right)) return sh::set_error(SH_ERR_INVALID, "%s: event %u: left / right is not finite", fn, e);
            if (m.dst_sample % 2 || m.nsamples % 2)
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: a mono source starts and ends on whole stereo frames", fn, e);
            nsrc_samples = m.nsamples / 2;
        }
        if (m.src_sample > have) return sh::set_error(SH_ERR_INVALID, "%s: event %u: range outside its source", fn, e);
        if (m.inrate == m.outrate) {
            if (nsrc_samples > have - m.src_sample) return sh::set_error(SH_ERR_INVALID, "%s: event %u: range outside its source", fn, e);
        } else {
            if (m.src_sample % nch || nsrc_samples % nch)
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: a resampled event starts and ends on whole frames", fn, e);
            if (m.src_frames > (have - m.src_sample) / nch) return sh::set_error(SH_ERR_INVALID, "%s: event %u: src_frames outside its source", fn, e);
            if (nsrc_samples / nch > shr::out_frames(m.src_frames, shr::reduce(m.inrate, m.outrate)))
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: more samples than src_frames resample to", fn, e);
        }
        if (m.seg_count > she::MAX_SEGMENTS) return sh::set_error(SH_ERR_INVALID, "%s: event %u: more than %u segments", fn, e, she::MAX_SEGMENTS);
        if (m.seg_count && (m.seg_first > nsegments || m.seg_count > nsegments - m.seg_first))
            return sh::set_error(SH_ERR_INVALID, "%s: event %u: segments outside the table", fn, e);
        uint64_t prev = 0;
        for (uint32_t s = 0; s < m.seg_count; ++s) {
            const sh_env_segment& g = segments[m.seg_first + s];
            if (g.reserved != 0) return sh::set_error(SH_ERR_INVALID, "%s: event %u: segment %u: reserved must be 0", fn, e, s);
            if (g.end < prev || g.end > nsrc_samples)
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: segment %u: ends not ascending or beyond the event's source samples", fn, e, s);
            if (g.kind > she::FADE_OUT) return sh::set_error(SH_ERR_INVALID, "%s: event %u: segment %u: kind %u not 0, 1 or 2", fn, e, s, g.kind);
            if (!isfinite(g.mul) || !isfinite(g.slope) || !isfinite(g.numsamples) || !isfinite(g.offset))
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: segment %u: a factor is not finite", fn, e, s);
            if (g.kind != she::NONE && !(g.numsamples > 0.0)) return sh::set_error(SH_ERR_INVALID, "%s: event %u: segment %u: a ramp needs numsamples > 0", fn, e, s);
            if (g.origin > nsrc_samples) return sh::set_error(SH_ERR_INVALID, "%s: event %u: segment %u: origin beyond the event's source samples", fn, e, s);
            prev = g.end;
        }
        pe[e] = shq::Event{m.dst_sample, m.nsamples};
    }
    const uint32_t ns = (uint32_t)track_samples;
    return seq_run<SeqEvE>(fn, pe, width, track_samples,
        [&](SeqEvE* rec) {
            she::Seg* seg = reinterpret_cast<she::Seg*>(rec + nevents);
            for (uint32_t s = 0; s < nsegments; ++s) {
                const sh_env_segment& g = segments[s];        // (a segment that no event names was not checked, and no kernel reads it)
                seg[s] = she::Seg{g.mul, g.slope, g.numsamples, g.offset, (uint32_t)g.end, (uint32_t)g.origin, g.kind, 0};
            }
            for (uint32_t e = 0; e < nevents; ++e) {
                const sh_mix_event_env& m = events[e];
                const shr::Rates R = shr::reduce(m.inrate, m.outrate);
                rec[e] = SeqEvE{SeqEvR{(const char*)srcs[m.src]->ptr + m.src_sample * w, m.factor, 1.0 / (double)R.outr, (uint32_t)m.dst_sample,
                                       (uint32_t)m.nsamples, R.inr, R.outr, R.inr / R.outr, R.inr % R.outr, m.src_channels,
                                       width <= 2 && R.outr < 65536u ? 1u : 0u, {0, 0}},
                                m.left, m.right, m.seg_count ? m.seg_first : 0u, m.seg_count, m.src_channels == 1 && nchannels == 2 ? 1u : 0u, 0};
            }
        },
        [&](const SeqEvE* d_ev, const uint32_t* d_tiles, const uint32_t* d_first, const uint32_t* d_idx, uint32_t nt, dim3 grid, dim3 block, hipStream_t st) {
            const she::Seg* d_seg = reinterpret_cast<const she::Seg*>(d_ev + nevents);
            if (width == 2) {
                const int aligned = ((uintptr_t)track->ptr & 15) == 0;
                if (sh::knobs().seq_align == VEC2) hipLaunchKernelGGL(k_mix_events_env_i16<VEC2>, grid, block, 0, st, d_ev, d_seg, d_tiles, d_first, d_idx, nt, (short*)track->ptr, ns, aligned);
                else hipLaunchKernelGGL(k_mix_events_env_i16<FUNNEL>, grid, block, 0, st, d_ev, d_seg, d_tiles, d_first, d_idx, nt, (short*)track->ptr, ns, aligned);
            }
            else if (width == 1) hipLaunchKernelGGL(k_mix_events_env_w<1>, grid, block, 0, st, d_ev, d_seg, d_tiles, d_first, d_idx, nt, (unsigned char*)track->ptr, ns);
            else hipLaunchKernelGGL(k_mix_events_env_w<4>, grid, block, 0, st, d_ev, d_seg, d_tiles, d_first, d_idx, nt, (unsigned char*)track->ptr, ns);
        },
        (size_t)nsegments * sizeof(she::Seg));
}

}  // extern "C"
