// pcm_ops.hip -- the remaining elementwise / reduction operations that synthplayer's Sample delegates to
// CPython's audioop (Modules/audioop.c, 3.10): mul (amplify, invert), bias, reverse, tomono, tostereo,
// lin2lin, max, rms -- plus the per-sample fade ramps of Sample.fadein / fadeout.  SURVEY.md section 8(f)
// item 2.  HBM-bound byte/integer work: 16-byte vectors per thread where alignment allows, wavefront
// shuffle (DPP) reductions + one integer atomic per workgroup for max / sum of squares.
// Built with -ffp-contract=off: audioop forms val1*lfactor + val2*rfactor with separate roundings.
#include "common.hpp"
#include "pcmdev.hpp"
#include "pcmhost.hpp"
#include "pcmblocks.hpp"
#include "pcmextent.hpp"
#include <stdlib.h>
#include <limits>
#include <type_traits>

namespace {

// out[i] = fbound(in[i] * factor)            (audioop.mul)
template <typename T, int VEC, bool NT = false>
__global__ __launch_bounds__(256) void k_mul(const T* in, T* out, size_t nvec, double factor) {
    typedef T vec_t __attribute__((ext_vector_type(VEC)));
    const size_t i = sh::block_id() * 256 + threadIdx.x;
    if (i >= nvec) return;
    vec_t v = sh::load_vec<NT, vec_t>(reinterpret_cast<const vec_t*>(in) + i), r;       // NT (streaming sizes): +1 % (tomono: -1 %, left as it was)
#pragma unroll
    for (int c = 0; c < VEC; ++c) r[c] = (T)fbound((double)v[c] * factor, Lim<T>::lo, Lim<T>::hi);
    reinterpret_cast<vec_t*>(out)[i] = r;
}

// per-sample linear ramp: out[i] = int(in[i] * (i*slope/numsamples + offset)), truncation toward zero
// (Sample.fadeout: offset 1, slope -decrease; Sample.fadein: offset start_volume, slope increase)
template <typename T>
__global__ __launch_bounds__(256) void k_fade(const T* in, T* out, size_t n, double slope, double numsamples, double offset, int fadeout) {
    const size_t i = sh::block_id() * 256 + threadIdx.x;
    if (i >= n) return;
    const double ramp = (double)i * slope / numsamples;
    const double f = fadeout ? (1.0 - ramp) : (ramp + offset);
    out[i] = (T)(long long)trunc((double)in[i] * f);
}

// out[i] = int(in[i] * mod[i mod nmod])          (Sample.modulate_amp: Python float product, int() truncation;
// a product outside the sample range raises upstream -> flag)
template <typename T>
__global__ __launch_bounds__(256) void k_modulate(const T* __restrict__ in, T* __restrict__ out, size_t n,
                                                  const double* __restrict__ mod, size_t nmod, int* flag) {
    const size_t i = sh::block_id() * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t k = i < nmod ? i : (i < 0xFFFFFFFFull && nmod < 0xFFFFFFFFull ? (size_t)((uint32_t)i % (uint32_t)nmod) : i % nmod);
    constexpr double HI = (double)((1ll << (8 * sizeof(T) - 1)) - 1), LO = -(double)(1ll << (8 * sizeof(T) - 1));
    double t = trunc((double)in[i] * mod[k]);
    if (!(t >= LO && t <= HI)) {
        *flag = 1;
        t = t > HI ? HI : LO;
    }
    out[i] = (T)(long long)t;
}

// Sample.pan(lfo=...): frame i becomes (int(l * (1 - p) / 2), int(r * (1 + p) / 2)) with p = pan[i]; a mono source
// feeds both sides.  float64 like the Python expression (the halving is exact); a value outside the sample range
// raises upstream (array assignment) -> flag.  PAIR: the frame is stored as one two-sample vector (out aligned to 2 * sizeof(T),
// the host's decision); otherwise as two samples.
template <typename T, int NCH, bool PAIR = true>
__global__ __launch_bounds__(256) void k_pan_lfo(const T* __restrict__ in, T* __restrict__ out, size_t nframes,
                                                 const double* __restrict__ pan, int* flag) {
    const size_t i = sh::block_id() * 256 + threadIdx.x;
    if (i >= nframes) return;
    constexpr double HI = (double)((1ll << (8 * sizeof(T) - 1)) - 1), LO = -(double)(1ll << (8 * sizeof(T) - 1));
    const double p = pan[i];
    const double l = (double)in[i * NCH], r = (double)in[i * NCH + NCH - 1];
    double tl = trunc(l * (1.0 - p) / 2.0), tr = trunc(r * (1.0 + p) / 2.0);
    if (!(tl >= LO && tl <= HI)) { *flag = 1; tl = tl > HI ? HI : LO; }
    if (!(tr >= LO && tr <= HI)) { *flag = 1; tr = tr > HI ? HI : LO; }
    typedef T pair_t __attribute__((ext_vector_type(2)));
    pair_t o = {(T)(long long)tl, (T)(long long)tr};
    if constexpr (PAIR) reinterpret_cast<pair_t*>(out)[i] = o;
    else { out[2 * i] = o[0]; out[2 * i + 1] = o[1]; }
}

// out[i] = in[i] / divisor in float64              (Sample.get_frames_as_floats; waveform modulators)
template <typename T>
__global__ __launch_bounds__(256) void k_to_f64(const T* __restrict__ in, double* __restrict__ out, size_t n, double divisor) {
    const size_t i = sh::block_id() * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = (double)in[i] / divisor;
}

// out[i] = in[i] + bias, wrapping                (audioop.bias)
template <typename T>
__global__ __launch_bounds__(256) void k_bias(const T* in, T* out, size_t n, int bias) {
    const size_t i = sh::block_id() * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = (T)((unsigned)(int)in[i] + (unsigned)bias);
}

// out[i] = in[n-1-i]                             (audioop.reverse: samples, not frames)
template <typename T>
__global__ __launch_bounds__(256) void k_reverse(const T* __restrict__ in, T* __restrict__ out, size_t n) {
    const size_t i = sh::block_id() * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = in[n - 1 - i];
}

// stereo -> mono: fbound(l*lfactor + r*rfactor)  (audioop.tomono); F frames per thread (16-byte loads).  The host launches F > 1 only
// with in aligned to 16 and out to 8 bytes; PAIR (F == 1): the frame is loaded as one two-sample vector (in aligned to 2 * sizeof(T)),
// otherwise as two samples.
template <typename T, int F, bool PAIR = true>
__global__ __launch_bounds__(256) void k_tomono(const T* __restrict__ in, T* __restrict__ out, size_t nunits, double lf, double rf) {
    typedef T vin __attribute__((ext_vector_type(2 * F)));
    typedef T vout __attribute__((ext_vector_type(F)));
    const size_t i = sh::block_id() * 256 + threadIdx.x;
    if (i >= nunits) return;
    vin v;
    if constexpr (F == 1 && !PAIR) { v[0] = in[2 * i]; v[1] = in[2 * i + 1]; }
    else v = reinterpret_cast<const vin*>(in)[i];
    vout r;
#pragma unroll
    for (int f = 0; f < F; ++f) r[f] = (T)fbound((double)v[2 * f] * lf + (double)v[2 * f + 1] * rf, Lim<T>::lo, Lim<T>::hi);
    if (F == 1) out[i] = r[0]; else reinterpret_cast<vout*>(out)[i] = r;
}

// mono -> stereo: (fbound(v*lfactor), fbound(v*rfactor))   (audioop.tostereo).  The host launches F > 1 only with in aligned to 8
// and out to 16 bytes; PAIR (F == 1): the frame is stored as one two-sample vector (out aligned to 2 * sizeof(T)), otherwise as two samples.
template <typename T, int F, bool PAIR = true>
__global__ __launch_bounds__(256) void k_tostereo(const T* __restrict__ in, T* __restrict__ out, size_t nunits, double lf, double rf) {
    typedef T vin __attribute__((ext_vector_type(F)));
    typedef T vout __attribute__((ext_vector_type(2 * F)));
    const size_t i = sh::block_id() * 256 + threadIdx.x;
    if (i >= nunits) return;
    vin v;
    if (F == 1) v[0] = in[i]; else v = reinterpret_cast<const vin*>(in)[i];
    vout r;
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const double x = (double)v[f];
        r[2 * f] = (T)fbound(x * lf, Lim<T>::lo, Lim<T>::hi);
        r[2 * f + 1] = (T)fbound(x * rf, Lim<T>::lo, Lim<T>::hi);
    }
    if constexpr (F == 1 && !PAIR) { out[2 * i] = r[0]; out[2 * i + 1] = r[1]; }
    else reinterpret_cast<vout*>(out)[i] = r;
}

// width conversion through the 32-bit form (GETSAMPLE32 / SETSAMPLE32)   (audioop.lin2lin)
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void k_lin2lin(const TI* __restrict__ in, TO* __restrict__ out, size_t n) {
    const size_t i = sh::block_id() * 256 + threadIdx.x;
    if (i >= n) return;
    const int v32 = (int)((unsigned)(int)in[i] << (32 - 8 * (int)sizeof(TI)));
    out[i] = (TO)(v32 >> (32 - 8 * (int)sizeof(TO)));
}

// reductions over a wavefront, lane 0 holds the result
template <typename A>
__device__ __forceinline__ A wave_sum(A v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        unsigned w = __shfl_down(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// lane 0 of each of the four waves has left its channel's maximum and sum in LDS: thread c < NCH folds channel c's four, the waves in
// order, into out[c] = max, out[NCH + c] = sum (A = double: as its bit pattern)
template <typename A, int NCH>
__device__ __forceinline__ void stats_record(unsigned (&mx)[NCH], A (&sq)[NCH], unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s_sum[4][NCH];
    __shared__ unsigned s_max[4][NCH];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        mx[c] = wave_max_u32(mx[c]);
        sq[c] = wave_sum(sq[c]);
        if (lane == 0) { s_sum[wave][c] = __builtin_bit_cast(unsigned long long, sq[c]); s_max[wave][c] = mx[c]; }
    }
    __syncthreads();
    if (threadIdx.x < NCH) {
        const unsigned c = threadIdx.x;
        unsigned m = s_max[0][c];
        for (int w = 1; w < 4; ++w) m = s_max[w][c] > m ? s_max[w][c] : m;
        A t = __builtin_bit_cast(A, s_sum[0][c]);
        for (int w = 1; w < 4; ++w) t += __builtin_bit_cast(A, s_sum[w][c]);
        out[c] = (unsigned long long)m;
        out[NCH + c] = __builtin_bit_cast(unsigned long long, t);
    }
}

// audioop.max and the sum of squares of audioop.rms, per channel of NCH interleaved ones, in one read.  (Stereo: Sample.level_db_peak /
// level_db_rms -- upstream takes audioop.tomono(frames, w, 1, 0) and (.., 0, 1), two copies, and runs audioop.max / rms over each: four
// passes and two temporaries.)  A 16-byte vector holds whole frames, so element c belongs to channel c mod NCH.
// part[2 NCH b ..] = the workgroup's max |x| per channel, then its sums: u64, exact, for widths 1 and 2; for width 4, where squares
// do not fit u64 sums exactly, float64 bit patterns -- the squares added per thread, then a fixed tree: close to, but not
// bit-identical with, audioop's sequential float64 sum (documented).
template <typename T, int NCH>
__global__ __launch_bounds__(256) void k_pcm_stats(const T* __restrict__ in, size_t nframes, unsigned long long* __restrict__ part) {
    typedef typename std::conditional<sizeof(T) == 4, double, unsigned long long>::type acc_t;
    unsigned mx[NCH] = {};
    acc_t sq[NCH] = {};
    auto take = [&](int c, long long v) {
        const unsigned a = (unsigned)(v < 0 ? -v : v);
        mx[c] = a > mx[c] ? a : mx[c];
        if constexpr (sizeof(T) == 4) sq[c] += (double)v * (double)v;
        else sq[c] += (unsigned long long)(v * v);
    };
    constexpr int V = 16 / sizeof(T);
    typedef T vec_t __attribute__((ext_vector_type(V)));
    const vec_t* vin = reinterpret_cast<const vec_t*>(in);
    const size_t nvec = ((reinterpret_cast<uintptr_t>(in) & 15) == 0) ? nframes * NCH / V : 0;
    const size_t step = (size_t)gridDim.x * 256;
    if constexpr (sizeof(T) == 2) {
        // 16-bit: packed arithmetic, two samples per instruction.  |x| = max(x, 0 - x) as int16 pairs, read as
        // uint16 (so |-32768| = 32768 comes out right); running maximum as uint16 pairs; mono: a pair's squares summed
        // by the dot-product instruction (<= 2^31, fits uint32) and added to the 64-bit total; stereo: a pair is a frame, one
        // 24-bit multiply per channel.
        typedef short s2 __attribute__((ext_vector_type(2)));
        typedef unsigned short u2 __attribute__((ext_vector_type(2)));
        u2 mx2 = {0, 0};
        auto pair = [&](const s2 v) {
            const s2 neg = (s2){0, 0} - v;
            const u2 au = __builtin_bit_cast(u2, __builtin_elementwise_max(v, neg));
            mx2 = __builtin_elementwise_max(mx2, au);
            if constexpr (NCH == 1) sq[0] += (unsigned long long)__builtin_amdgcn_udot2(au, au, 0u, false);
            else { sq[0] += (unsigned long long)__umul24(au[0], au[0]); sq[1] += (unsigned long long)__umul24(au[1], au[1]); }
        };
        auto pairs = [&](const vec_t x) {
            pair(__builtin_shufflevector(x, x, 0, 1)); pair(__builtin_shufflevector(x, x, 2, 3));
            pair(__builtin_shufflevector(x, x, 4, 5)); pair(__builtin_shufflevector(x, x, 6, 7));
        };
        // a workgroup reads INFLIGHT * 4 KB contiguous per turn (the loads in flight are neighbours, not a grid apart:
        // the whole chip then sweeps one window of memory at a time, which the DRAM pages like)
        constexpr int INFLIGHT = 4;
        size_t i = (size_t)blockIdx.x * 256 * INFLIGHT + threadIdx.x;
        for (; i + (INFLIGHT - 1) * 256 < nvec; i += step * INFLIGHT) {
            vec_t x[INFLIGHT];
#pragma unroll
            for (int k = 0; k < INFLIGHT; ++k) x[k] = __builtin_nontemporal_load(vin + i + k * 256);
#pragma unroll
            for (int k = 0; k < INFLIGHT; ++k) pairs(x[k]);
        }
        if (i < nvec) {                                            // the last, partial turn of this workgroup
#pragma unroll
            for (int k = 0; k < INFLIGHT; ++k)
                if (i + k * 256 < nvec) pairs(vin[i + k * 256]);
        }
        if constexpr (NCH == 1) mx[0] = mx2[0] > mx2[1] ? mx2[0] : mx2[1];
        else { mx[0] = mx2[0]; mx[1] = mx2[1]; }
    } else {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += step) {
            const vec_t x = vin[i];
#pragma unroll
            for (int c = 0; c < V; ++c) take(c % NCH, (long long)x[c]);
        }
    }
    for (size_t f = nvec * V / NCH + (size_t)blockIdx.x * 256 + threadIdx.x; f < nframes; f += step) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) take(c, (long long)in[NCH * f + c]);
    }
    // per-workgroup records, folded by k_pcm_stats_fold: thousands of atomics on two addresses serialise (10 ns each,
    // 40 % of this kernel's time at 4096 workgroups)
    stats_record<acc_t, NCH>(mx, sq, part + 2 * NCH * (size_t)blockIdx.x);
}

// one workgroup: out = the records of nblocks workgroups folded into one (integer sums: exact, order-independent; F64: the sums are
// float64, added in a fixed order: thread t takes workgroups t, t+256, ...; then the 64-lane tree; then the four waves)
template <int NCH, bool F64>
__global__ __launch_bounds__(256) void k_pcm_stats_fold(const unsigned long long* __restrict__ part, unsigned nblocks,
                                                        unsigned long long* __restrict__ out) {
    typedef typename std::conditional<F64, double, unsigned long long>::type acc_t;
    unsigned mx[NCH] = {};
    acc_t sq[NCH] = {};
    for (unsigned b = threadIdx.x; b < nblocks; b += 256) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const unsigned m = (unsigned)part[2 * NCH * b + c];
            mx[c] = m > mx[c] ? m : mx[c];
            sq[c] += __builtin_bit_cast(acc_t, part[2 * NCH * b + NCH + c]);
        }
    }
    stats_record<acc_t, NCH>(mx, sq, out);
}

// ---- the levels per block of PCM in device memory (sh_pcm_level_blocks; pcmblocks.hpp has the geometry and the arithmetic) ----------------
// what the two kernels are handed: frames in 64 bits, as the header counts them
struct LevelBlocks {
    const void* in;             // the first sample of plane 0
    uint64_t plane_samples;     // plane r begins r * plane_samples samples behind it
    uint64_t n, origin, B;      // the call's frames, the grid frame of the first, the block
    uint64_t first;             // origin / B
    uint32_t shift;             // a block has 2^shift part slots: shpb::slot_shift(the longest block)
    uint64_t nwg;               // nblocks << shift: the workgroups of one plane
    uint32_t nplanes, r0;       // the rows of a block; the plane of blockIdx.z == 0 in this launch
    shmt::Row* out;             // row (w * nplanes + r) of workgroup w of plane r: the table where shift == 0, the partial rows otherwise
};

// a wave's rows into lane 0's: shmt::fold over the six shuffle steps (fields a width or a channel count never fills stay the constant 0)
template <int NCH, bool WIDE>
__device__ __forceinline__ shmt::Row wave_fold_row(shmt::Row r) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        shmt::Row q = shmt::zero();
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            q.peak[c] = __shfl_down(r.peak[c], o, 64);
            q.sq_lo[c] = __shfl_down((unsigned long long)r.sq_lo[c], o, 64);
            if constexpr (WIDE) q.sq_hi[c] = __shfl_down((unsigned long long)r.sq_hi[c], o, 64);
        }
        shmt::fold(r, q);
    }
    return r;
}

// One workgroup per (part slot, plane): the samples [s0, s1) of its block's cut range in its plane, and nothing else -- a scalar head up
// to the 16-byte boundary, 16-byte vectors, a scalar tail; a plane that starts off the sample grid (a view cut at an odd byte) has no
// such boundary and is all head.  Scalar samples are assembled from bytes (memcpy), so they need no alignment.  In a stereo plane a part
// starts on a frame (s0 is even), so a scalar sample's channel is its index's parity; a vector holds whole frames, element e of every
// vector belongs to channel (head + e) & 1, and the vectors' row changes sides once, behind the loop, where the head is odd.
// At 16 bits the packed forms of k_pcm_stats: |x| as uint16 pairs, mono a pair's squares by the dot product, stereo a 24-bit
// multiply per channel.  The lanes' rows fold by wave shuffle, the four waves' through LDS behind the one barrier, and thread
// 2 * 0 + channel stores its channel of the row: one writer per row, zeros too, no atomics, nothing zeroed first.
template <typename T, int NCH>
__global__ __launch_bounds__(256) void k_pcm_level_blocks(const LevelBlocks g) {
    constexpr bool WIDE = sizeof(T) == 4;
    constexpr uint32_t V = 16 / sizeof(T);
    typedef T vec_t __attribute__((ext_vector_type(V)));
    const uint64_t w = sh::block_id();
    if (w >= g.nwg) return;                                    // (a launch folded into two dimensions rounds up)
    const uint32_t r = g.r0 + blockIdx.z;
    const uint64_t j = w >> g.shift, p = w - (j << g.shift);
    uint64_t a, b, s0, s1;
    shpb::range(g.first, j, g.origin, g.n, g.B, a, b);
    shpb::part((b - a) * NCH, p, s0, s1);
    const unsigned char* x = (const unsigned char*)g.in + ((uint64_t)r * g.plane_samples + (a - g.origin) * NCH + s0) * sizeof(T);
    const uint32_t cnt = (uint32_t)(s1 - s0);                  // at most shpb::PART_SAMPLES
    const uintptr_t at = (uintptr_t)x;
    uint32_t head = cnt;
    if (at % sizeof(T) == 0) {
        head = (uint32_t)((16 - (at & 15)) & 15) / (uint32_t)sizeof(T);
        if (head > cnt) head = cnt;
    }
    const uint32_t nvec = (cnt - head) / V, tail = head + nvec * V;
    auto sample = [&](uint32_t i) {
        T v;
        __builtin_memcpy(&v, x + (size_t)i * sizeof(T), sizeof(T));
        return (long long)v;
    };
    shmt::Row row = shmt::zero();
    auto one = [&](uint32_t i) {                               // shpb::take with both channels' adds spelled out: the other side adds 0
        const long long q = sample(i);
        const bool right = NCH == 2 && (i & 1);
        shmt::add<WIDE>(row, 0, right ? 0 : q);
        if constexpr (NCH == 2) shmt::add<WIDE>(row, 1, right ? q : 0);
    };
    for (uint32_t i = threadIdx.x; i < head; i += 256) one(i);
    for (uint32_t i = tail + threadIdx.x; i < cnt; i += 256) one(i);

    const vec_t* vin = reinterpret_cast<const vec_t*>(x + (size_t)head * sizeof(T));
    shmt::Row vrow = shmt::zero();                             // by element parity
    constexpr uint32_t INFLIGHT = 4;
    uint32_t v = threadIdx.x;
    if constexpr (sizeof(T) == 2) {
        typedef short s2 __attribute__((ext_vector_type(2)));
        typedef unsigned short u2 __attribute__((ext_vector_type(2)));
        u2 mx2 = {0, 0};
        unsigned long long sq[NCH] = {};
        auto pair = [&](const s2 q) {
            const s2 neg = (s2){0, 0} - q;
            const u2 au = __builtin_bit_cast(u2, __builtin_elementwise_max(q, neg));       // read as uint16: |-32768| = 32768
            mx2 = __builtin_elementwise_max(mx2, au);
            if constexpr (NCH == 1) sq[0] += (unsigned long long)__builtin_amdgcn_udot2(au, au, 0u, false);
            else { sq[0] += (unsigned long long)__umul24(au[0], au[0]); sq[1] += (unsigned long long)__umul24(au[1], au[1]); }
        };
        auto pairs = [&](const vec_t q) {
            pair(__builtin_shufflevector(q, q, 0, 1)); pair(__builtin_shufflevector(q, q, 2, 3));
            pair(__builtin_shufflevector(q, q, 4, 5)); pair(__builtin_shufflevector(q, q, 6, 7));
        };
        for (; v + (INFLIGHT - 1) * 256 < nvec; v += INFLIGHT * 256) {
            vec_t q[INFLIGHT];
#pragma unroll
            for (uint32_t k = 0; k < INFLIGHT; ++k) q[k] = vin[v + k * 256];
#pragma unroll
            for (uint32_t k = 0; k < INFLIGHT; ++k) pairs(q[k]);
        }
        for (; v < nvec; v += 256) pairs(vin[v]);
        if constexpr (NCH == 1) { vrow.peak[0] = mx2[0] > mx2[1] ? mx2[0] : mx2[1]; vrow.sq_lo[0] = sq[0]; }
        else { vrow.peak[0] = mx2[0]; vrow.peak[1] = mx2[1]; vrow.sq_lo[0] = sq[0]; vrow.sq_lo[1] = sq[1]; }
    } else {
        auto all = [&](const vec_t q) {
#pragma unroll
            for (uint32_t e = 0; e < V; ++e) shmt::add<WIDE>(vrow, (int)(e % NCH), (long long)q[e]);
        };
        for (; v + (INFLIGHT - 1) * 256 < nvec; v += INFLIGHT * 256) {
            vec_t q[INFLIGHT];
#pragma unroll
            for (uint32_t k = 0; k < INFLIGHT; ++k) q[k] = vin[v + k * 256];
#pragma unroll
            for (uint32_t k = 0; k < INFLIGHT; ++k) all(q[k]);
        }
        for (; v < nvec; v += 256) all(vin[v]);
    }
    if constexpr (NCH == 2) {                                  // the vectors began on a right sample: the two sides change places (by
        const uint64_t m = (head & 1) ? ~0ull : 0ull;          // mask, so that no field of a row in registers is picked by a variable)
        const uint32_t tp = (vrow.peak[0] ^ vrow.peak[1]) & (uint32_t)m;
        const uint64_t th = (vrow.sq_hi[0] ^ vrow.sq_hi[1]) & m, tl = (vrow.sq_lo[0] ^ vrow.sq_lo[1]) & m;
        vrow.peak[0] ^= tp, vrow.peak[1] ^= tp, vrow.sq_hi[0] ^= th, vrow.sq_hi[1] ^= th, vrow.sq_lo[0] ^= tl, vrow.sq_lo[1] ^= tl;
    }
    shmt::fold(row, vrow);

    __shared__ shmt::Row s_rows[4];
    row = wave_fold_row<NCH, WIDE>(row);
    if ((threadIdx.x & 63) == 0) {
        shmt::Row& mine = s_rows[threadIdx.x >> 6];
#pragma unroll
        for (int c = 0; c < 2; ++c) mine.peak[c] = row.peak[c], mine.sq_hi[c] = row.sq_hi[c], mine.sq_lo[c] = row.sq_lo[c];
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const uint32_t c = threadIdx.x;
        uint32_t peak = s_rows[0].peak[c];
        uint64_t hi = s_rows[0].sq_hi[c], lo = s_rows[0].sq_lo[c];
        for (int k = 1; k < 4; ++k) {
            peak = s_rows[k].peak[c] > peak ? s_rows[k].peak[c] : peak;
            hi += s_rows[k].sq_hi[c];
            lo += s_rows[k].sq_lo[c];
        }
        shmt::Row* out = g.out + ((size_t)w * g.nplanes + r);
        out->peak[c] = peak;
        out->sq_hi[c] = hi;
        out->sq_lo[c] = lo;
    }
}

// the partial rows of a call whose blocks have 2^shift part slots into the table: one wave per row of the table -- the four waves of a
// workgroup take four consecutive blocks of plane r0 + blockIdx.z -- its lanes over the slots, shmt::fold all the way, lane 0 stores the row
__global__ __launch_bounds__(256) void k_pcm_level_fold(const shmt::Row* __restrict__ parts, uint32_t shift, uint64_t nblocks, uint32_t nplanes, uint32_t r0,
                                                        shmt::Row* __restrict__ table) {
    const uint64_t j = sh::block_id() * 4 + (threadIdx.x >> 6);
    if (j >= nblocks) return;
    const uint32_t r = r0 + blockIdx.z;
    shmt::Row sum = shmt::zero();
    for (uint64_t p = threadIdx.x & 63; p >> shift == 0; p += 64) shmt::fold(sum, parts[((j << shift) + p) * nplanes + r]);
    sum = wave_fold_row<2, true>(sum);
    if ((threadIdx.x & 63) == 0) table[j * nplanes + r] = sum;
}

// ---- the waveform extremes per block of PCM in device memory (sh_pcm_extent_blocks; pcmextent.hpp has the row, pcmblocks.hpp the geometry) --
// a wave's rows into lane 0's: shpe::fold over the six shuffle steps (a mono input's channel 1 stays the constant identity)
template <int NCH>
__device__ __forceinline__ shpe::Row wave_fold_extent(shpe::Row r) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        shpe::Row q = shpe::identity();
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            q.lo[c] = __shfl_down(r.lo[c], o, 64);
            q.hi[c] = __shfl_down(r.hi[c], o, 64);
        }
        shpe::fold(r, q);
    }
    return r;
}

// One WAVE per (part slot, plane), four to a workgroup: wave 4 * block_id + (threadIdx.x >> 6) of plane r0 + blockIdx.z finds its block
// and slot by the shift (g.nwg counts waves here, g.out holds shpe::Row), so the waves of a workgroup take consecutive slots of one
// plane and share nothing.  The wave's number is read into a scalar register, so the geometry is scalar arithmetic.  A wave reads the
// samples [s0, s1) of its block's cut range in its plane and nothing else, as k_pcm_level_blocks divides them: a scalar head up to the
// 16-byte boundary, 16-byte vectors (up to four in flight per lane), a scalar tail; scalar samples are assembled from bytes, so a view
// cut at an odd byte is all head.  The vectors fold into two accumulators of their own type by elementwise min and max -- one statement
// for every width, packed at 16 bits -- whose element e goes to channel e % NCH behind the loop; where a stereo plane's head is odd the
// two sides change places once, there.  A lane that loaded no vector leaves its accumulators out, so an empty slot yields the identity.
// The lanes fold by wave shuffle and lane 0 stores the row, with the mono rule where it is a row of the table: no LDS, no barrier, no
// atomics, one writer per row, nothing zeroed first.
template <typename T, int NCH>
__global__ __launch_bounds__(256) void k_pcm_extent_blocks(const LevelBlocks g) {
    constexpr uint32_t V = 16 / sizeof(T);
    typedef T vec_t __attribute__((ext_vector_type(V)));
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t w = sh::block_id() * 4 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= g.nwg) return;                                    // (the last workgroup's waves past the end; a launch folded into two dimensions rounds up)
    const uint32_t r = g.r0 + blockIdx.z;
    const uint64_t j = w >> g.shift, p = w - (j << g.shift);
    uint64_t a, b, s0, s1;
    shpb::range(g.first, j, g.origin, g.n, g.B, a, b);
    shpb::part((b - a) * NCH, p, s0, s1);
    const unsigned char* x = (const unsigned char*)g.in + ((uint64_t)r * g.plane_samples + (a - g.origin) * NCH + s0) * sizeof(T);
    const uint32_t cnt = (uint32_t)(s1 - s0);                  // at most shpb::PART_SAMPLES
    const uintptr_t at = (uintptr_t)x;
    uint32_t head = cnt;
    if (at % sizeof(T) == 0) {
        head = (uint32_t)((16 - (at & 15)) & 15) / (uint32_t)sizeof(T);
        if (head > cnt) head = cnt;
    }
    const uint32_t nvec = (cnt - head) / V, tail = head + nvec * V;
    shpe::Row row = shpe::identity();
    auto one = [&](uint32_t i) {                               // shpe::take with both channels spelled out: the other side takes its identity
        T v;
        __builtin_memcpy(&v, x + (size_t)i * sizeof(T), sizeof(T));
        const int32_t q = (int32_t)v;
        const bool right = NCH == 2 && (i & 1);
        const int32_t l0 = right ? INT32_MAX : q, h0 = right ? INT32_MIN : q;
        row.lo[0] = l0 < row.lo[0] ? l0 : row.lo[0];
        row.hi[0] = h0 > row.hi[0] ? h0 : row.hi[0];
        if constexpr (NCH == 2) {
            const int32_t l1 = right ? q : INT32_MAX, h1 = right ? q : INT32_MIN;
            row.lo[1] = l1 < row.lo[1] ? l1 : row.lo[1];
            row.hi[1] = h1 > row.hi[1] ? h1 : row.hi[1];
        }
    };
    for (uint32_t i = lane; i < head; i += 64) one(i);
    for (uint32_t i = tail + lane; i < cnt; i += 64) one(i);

    const vec_t* vin = reinterpret_cast<const vec_t*>(x + (size_t)head * sizeof(T));
    vec_t mn = (vec_t)(std::numeric_limits<T>::max()), mx = (vec_t)(std::numeric_limits<T>::min());
    constexpr uint32_t INFLIGHT = 4;
    uint32_t v = lane;
    for (; v + (INFLIGHT - 1) * 64 < nvec; v += INFLIGHT * 64) {
        vec_t q[INFLIGHT];
#pragma unroll
        for (uint32_t k = 0; k < INFLIGHT; ++k) q[k] = vin[v + k * 64];
#pragma unroll
        for (uint32_t k = 0; k < INFLIGHT; ++k) mn = __builtin_elementwise_min(mn, q[k]), mx = __builtin_elementwise_max(mx, q[k]);
    }
    for (; v < nvec; v += 64) {
        const vec_t q = vin[v];
        mn = __builtin_elementwise_min(mn, q), mx = __builtin_elementwise_max(mx, q);
    }
    shpe::Row vrow = shpe::identity();                         // by element parity
    if (lane < nvec) {
#pragma unroll
        for (uint32_t e = 0; e < V; ++e) {
            const int32_t l = (int32_t)mn[e], h = (int32_t)mx[e];
            vrow.lo[e % NCH] = l < vrow.lo[e % NCH] ? l : vrow.lo[e % NCH];
            vrow.hi[e % NCH] = h > vrow.hi[e % NCH] ? h : vrow.hi[e % NCH];
        }
    }
    if (NCH == 2 && (head & 1)) {                              // the vectors began on a right sample: the two sides change places
        const int32_t l = vrow.lo[0], h = vrow.hi[0];
        vrow.lo[0] = vrow.lo[1], vrow.hi[0] = vrow.hi[1], vrow.lo[1] = l, vrow.hi[1] = h;
    }
    shpe::fold(row, vrow);
    row = wave_fold_extent<NCH>(row);
    if (lane == 0) {
        if (!g.shift) row = shpe::stored(row, NCH);            // a row of the table: the mono rule (a partial row keeps the identity)
        typedef int32_t row_t __attribute__((ext_vector_type(4)));
        const row_t q = {row.lo[0], row.lo[1], row.hi[0], row.hi[1]};
        reinterpret_cast<row_t*>(g.out)[(size_t)w * g.nplanes + r] = q;       // (the library's scratch: rows stand on 16 bytes)
    }
}

// the partial rows of a call whose blocks have 2^shift part slots into the table: one wave per table row, as k_pcm_level_fold -- the four
// waves of a workgroup take four consecutive blocks of plane r0 + blockIdx.z -- its lanes over the slots, shpe::fold all the way, lane 0
// stores the row with the mono rule
__global__ __launch_bounds__(256) void k_pcm_extent_fold(const shpe::Row* __restrict__ parts, uint32_t shift, uint64_t nblocks, uint32_t nplanes, uint32_t r0,
                                                         uint32_t nch, shpe::Row* __restrict__ table) {
    const uint64_t j = sh::block_id() * 4 + (threadIdx.x >> 6);
    if (j >= nblocks) return;
    const uint32_t r = r0 + blockIdx.z;
    shpe::Row all = shpe::identity();
    for (uint64_t p = threadIdx.x & 63; p >> shift == 0; p += 64) shpe::fold(all, parts[((j << shift) + p) * nplanes + r]);
    all = wave_fold_extent<2>(all);
    if ((threadIdx.x & 63) == 0) table[j * nplanes + r] = shpe::stored(all, nch);
}

// 24-bit <-> 32-bit: a thread converts four samples (12 bytes <-> 16 bytes); the 12 bytes are read / written as three
// dwords when the 3-byte stream starts on a dword boundary, byte by byte otherwise (the tail always is).
__global__ __launch_bounds__(256) void k_unpack24(const unsigned char* __restrict__ in, size_t n, int shift, int* __restrict__ out, int dwords) {
    const size_t q = sh::block_id() * 256 + threadIdx.x;              // group of four samples
    if (q * 4 >= n) return;
    if (dwords && q * 4 + 4 <= n) {
        const unsigned* w = reinterpret_cast<const unsigned*>(in) + q * 3;
        const unsigned a = w[0], b = w[1], c = w[2];
        int4 r;
        r.x = ((int)(a << 8)) >> 8;
        r.y = ((int)(((a >> 24) | (b << 8)) << 8)) >> 8;
        r.z = ((int)(((b >> 16) | (c << 16)) << 8)) >> 8;
        r.w = ((int)c) >> 8;
        r.x <<= shift; r.y <<= shift; r.z <<= shift; r.w <<= shift;
        if ((reinterpret_cast<uintptr_t>(out) & 15) == 0) reinterpret_cast<int4*>(out)[q] = r;
        else { out[q * 4] = r.x; out[q * 4 + 1] = r.y; out[q * 4 + 2] = r.z; out[q * 4 + 3] = r.w; }
        return;
    }
    for (size_t i = q * 4; i < q * 4 + 4 && i < n; ++i) {
        const unsigned v = (unsigned)in[3 * i] | ((unsigned)in[3 * i + 1] << 8) | ((unsigned)in[3 * i + 2] << 16);
        out[i] = (((int)(v << 8)) >> 8) << shift;
    }
}

__global__ __launch_bounds__(256) void k_pack24(const int* __restrict__ in, size_t n, int shift, unsigned char* __restrict__ out, int dwords) {
    const size_t q = sh::block_id() * 256 + threadIdx.x;
    if (q * 4 >= n) return;
    if (dwords && q * 4 + 4 <= n) {
        const unsigned a = (unsigned)(in[q * 4] >> shift) & 0xFFFFFFu, b = (unsigned)(in[q * 4 + 1] >> shift) & 0xFFFFFFu;
        const unsigned c = (unsigned)(in[q * 4 + 2] >> shift) & 0xFFFFFFu, d = (unsigned)(in[q * 4 + 3] >> shift) & 0xFFFFFFu;
        unsigned* w = reinterpret_cast<unsigned*>(out) + q * 3;
        w[0] = a | (b << 24);
        w[1] = (b >> 8) | (c << 16);
        w[2] = (c >> 16) | (d << 8);
        return;
    }
    for (size_t i = q * 4; i < q * 4 + 4 && i < n; ++i) {
        const unsigned v = (unsigned)(in[i] >> shift);
        out[3 * i] = (unsigned char)v;
        out[3 * i + 1] = (unsigned char)(v >> 8);
        out[3 * i + 2] = (unsigned char)(v >> 16);
    }
}

}  // namespace

namespace sh {
int unpack24(const void* in, size_t nsamples, int shift, int32_t* out) {
    if (!nsamples) return SH_OK;
    hipLaunchKernelGGL(k_unpack24, sh::grid1d((nsamples + 3) / 4, 256), dim3(256), 0, state().stream, (const unsigned char*)in, nsamples, shift,
                       (int*)out, ((uintptr_t)in & 3) == 0 ? 1 : 0);
    SH_CHECK_LAUNCH("k_unpack24");
    return SH_OK;
}
int pack24(const int32_t* in, size_t nsamples, int shift, void* out) {
    if (!nsamples) return SH_OK;
    hipLaunchKernelGGL(k_pack24, sh::grid1d((nsamples + 3) / 4, 256), dim3(256), 0, state().stream, (const int*)in, nsamples, shift,
                       (unsigned char*)out, ((uintptr_t)out & 3) == 0 ? 1 : 0);
    SH_CHECK_LAUNCH("k_pack24");
    return SH_OK;
}
}  // namespace sh

namespace {
// width 3 through the 32-bit kernels: `nin` samples unpacked (<< shift_in), op32(temporary in, temporary out), `nout` samples
// packed (>> shift_out) to out + out_off.  inplace: the 32-bit operation may write where it reads.
template <typename F>
int via32(const sh_buf* in, size_t in_off, size_t nin, int shift_in, sh_buf* out, size_t out_off, size_t nout, int shift_out,
          bool inplace, const char* who, F&& op32) {
    int rc = check_io(in, in_off, nin * 3, out, out_off, nout * 3, who);
    if (rc) return rc;
    sh::Temp tin, tout;
    rc = tin.alloc(nin * 4);
    if (rc) return rc;
    if (!inplace) { rc = tout.alloc(nout * 4); if (rc) return rc; }
    rc = sh::unpack24((const char*)in->ptr + in_off, nin, shift_in, (int32_t*)tin.buf.ptr);
    if (rc) return rc;
    sh_buf* o32 = inplace ? &tin.buf : &tout.buf;
    rc = op32(&tin.buf, o32);
    if (rc) return rc;
    return sh::pack24((const int32_t*)o32->ptr, nout, shift_out, (char*)out->ptr + out_off);
}

// sh_pcm_stats (NCH 1) and sh_pcm_stats_stereo (NCH 2): max |x| and the sum of squares per channel over nframes frames of a width the
// caller has checked, into max_abs[NCH] / sum_squares[NCH] (either may be NULL).  A refusal leaves them alone.
template <int NCH>
int pcm_stats(const char* who, const sh_buf* in, size_t nframes, int width, uint32_t* max_abs, double* sum_squares) {
    if (!in || nframes > in->bytes / (NCH * (size_t)width)) return sh::set_error(SH_ERR_INVALID, "%s: range outside buffer", who);
    const size_t n = nframes * NCH;
    if (width == 3) {                           // the raw 24-bit values as int32
        sh::Temp t32;
        int rc3 = t32.alloc(n * 4);
        if (rc3) return rc3;
        rc3 = sh::unpack24(in->ptr, n, 0, (int32_t*)t32.buf.ptr);
        if (rc3) return rc3;
        return pcm_stats<NCH>(who, &t32.buf, nframes, 4, max_abs, sum_squares);
    }
    for (int c = 0; c < NCH; ++c) {
        if (max_abs) max_abs[c] = 0;
        if (sum_squares) sum_squares[c] = 0.0;
    }
    if (!n) return SH_OK;
    // 512 workgroups x 4 neighbouring 16-byte loads in flight per lane: 6.0 TB/s on 900 MB; 4096 workgroups with the four
    // loads a grid apart read the same data at 4.2-4.8
    const unsigned blocks = n / 8192 < 512 ? (unsigned)(n / 8192 + 1) : 512u;
    constexpr size_t R = 2 * NCH;                                                // words of a record: a maximum and a sum per channel
    int rc = sh::ensure_scratch((1 + (size_t)blocks) * R * 8);
    if (rc) return rc;
    hipStream_t st = sh::state().stream;
    unsigned long long* acc = (unsigned long long*)sh::state().scratch;          // the result's record; then one per workgroup
    rc = dispatch_width(width, [&](auto tag) {
        typedef decltype(tag) T;
        hipLaunchKernelGGL((k_pcm_stats<T, NCH>), dim3(blocks), dim3(256), 0, st, (const T*)in->ptr, nframes, acc + R);
        return launch_result("k_pcm_stats");
    });
    if (rc) return rc;
    if (width == 4) hipLaunchKernelGGL((k_pcm_stats_fold<NCH, true>), dim3(1), dim3(256), 0, st, (const unsigned long long*)(acc + R), blocks, acc);
    else hipLaunchKernelGGL((k_pcm_stats_fold<NCH, false>), dim3(1), dim3(256), 0, st, (const unsigned long long*)(acc + R), blocks, acc);
    SH_CHECK_LAUNCH("k_pcm_stats_fold");
    unsigned long long host_acc[R];
    SH_HIP(hipMemcpyAsync(host_acc, acc, sizeof host_acc, hipMemcpyDeviceToHost, st));
    SH_HIP(hipStreamSynchronize(st));
    for (int c = 0; c < NCH; ++c) {
        if (max_abs) max_abs[c] = (uint32_t)host_acc[c];
        if (sum_squares) sum_squares[c] = width == 4 ? __builtin_bit_cast(double, host_acc[NCH + c]) : (double)host_acc[NCH + c];
    }
    return SH_OK;
}

// sh_pcm_level_blocks behind its checks: nblocks > 0 blocks of the planes at `base` (samples of T, `stride` apart) into rows, synchronously
template <typename T>
int level_blocks_run(const void* base, size_t stride, size_t nframes, int nch, uint32_t nplanes, uint64_t origin, uint64_t B,
                     sh_seq_meter* rows, size_t nblocks) {
    static_assert(sizeof(sh_seq_meter) == sizeof(shmt::Row), "sh_seq_meter is shmt::Row");
    const char* fn = "sh_pcm_level_blocks";
    LevelBlocks g{};
    g.in = base, g.plane_samples = stride, g.n = nframes, g.origin = origin, g.B = B, g.first = origin / B;
    g.shift = shpb::slot_shift(shpb::longest(origin, nframes, B) * (uint64_t)nch);
    g.nwg = (uint64_t)nblocks << g.shift;
    g.nplanes = nplanes;
    if (g.nwg > (uint64_t)sh::GRID_X_MAX * 65535u) return sh::set_error(SH_ERR_INVALID, "%s: %llu parts of blocks are more than one launch takes", fn, (unsigned long long)g.nwg);
    // the library's scratch, sized for the call: the table, and behind it the partial rows of a call whose blocks have more than one part
    const size_t b_table = nblocks * (size_t)nplanes * sizeof(shmt::Row);
    const size_t b_parts = g.shift ? (size_t)g.nwg * nplanes * sizeof(shmt::Row) : 0;
    int rc = sh::ensure_scratch(b_table + b_parts);
    if (rc) return rc;
    shmt::Row* table = (shmt::Row*)sh::state().scratch;
    g.out = g.shift ? table + nblocks * (size_t)nplanes : table;
    hipStream_t st = sh::state().stream;
    dim3 grid = sh::grid1d(g.nwg, 1);
    for (g.r0 = 0; g.r0 < nplanes; g.r0 += 65535u) {          // (a grid's third dimension holds 65535 planes)
        grid.z = nplanes - g.r0 < 65535u ? nplanes - g.r0 : 65535u;
        if (nch == 1) hipLaunchKernelGGL((k_pcm_level_blocks<T, 1>), grid, dim3(256), 0, st, g);
        else hipLaunchKernelGGL((k_pcm_level_blocks<T, 2>), grid, dim3(256), 0, st, g);
        SH_CHECK_LAUNCH("k_pcm_level_blocks");
    }
    if (g.shift) {
        grid = sh::grid1d(nblocks, 4);
        for (uint32_t r0 = 0; r0 < nplanes; r0 += 65535u) {
            grid.z = nplanes - r0 < 65535u ? nplanes - r0 : 65535u;
            hipLaunchKernelGGL(k_pcm_level_fold, grid, dim3(256), 0, st, (const shmt::Row*)g.out, g.shift, (uint64_t)nblocks, nplanes, r0, table);
            SH_CHECK_LAUNCH("k_pcm_level_fold");
        }
    }
    SH_HIP(hipMemcpyAsync(rows, table, b_table, hipMemcpyDeviceToHost, st));
    SH_HIP(hipStreamSynchronize(st));
    return SH_OK;
}

// sh_pcm_extent_blocks behind its checks, as level_blocks_run: one wave per part slot, four to a workgroup; the partial rows of a call
// whose blocks have more than one part folded by k_pcm_extent_fold; the table through the library's scratch, one copy, one wait
template <typename T>
int extent_blocks_run(const void* base, size_t stride, size_t nframes, int nch, uint32_t nplanes, uint64_t origin, uint64_t B,
                      sh_pcm_extent* rows, size_t nblocks) {
    static_assert(sizeof(sh_pcm_extent) == sizeof(shpe::Row), "sh_pcm_extent is shpe::Row");
    const char* fn = "sh_pcm_extent_blocks";
    LevelBlocks g{};
    g.in = base, g.plane_samples = stride, g.n = nframes, g.origin = origin, g.B = B, g.first = origin / B;
    g.shift = shpb::slot_shift(shpb::longest(origin, nframes, B) * (uint64_t)nch);
    g.nwg = (uint64_t)nblocks << g.shift;                     // waves here
    g.nplanes = nplanes;
    if ((g.nwg + 3) / 4 > (uint64_t)sh::GRID_X_MAX * 65535u) return sh::set_error(SH_ERR_INVALID, "%s: %llu parts of blocks are more than one launch takes", fn, (unsigned long long)g.nwg);
    const size_t b_table = nblocks * (size_t)nplanes * sizeof(shpe::Row);
    const size_t b_parts = g.shift ? (size_t)g.nwg * nplanes * sizeof(shpe::Row) : 0;
    int rc = sh::ensure_scratch(b_table + b_parts);
    if (rc) return rc;
    shpe::Row* table = (shpe::Row*)sh::state().scratch;
    shpe::Row* parts = g.shift ? table + nblocks * (size_t)nplanes : table;
    g.out = reinterpret_cast<shmt::Row*>(parts);              // (the kernel stores shpe::Row there)
    hipStream_t st = sh::state().stream;
    dim3 grid = sh::grid1d(g.nwg, 4);
    for (g.r0 = 0; g.r0 < nplanes; g.r0 += 65535u) {          // (a grid's third dimension holds 65535 planes)
        grid.z = nplanes - g.r0 < 65535u ? nplanes - g.r0 : 65535u;
        if (nch == 1) hipLaunchKernelGGL((k_pcm_extent_blocks<T, 1>), grid, dim3(256), 0, st, g);
        else hipLaunchKernelGGL((k_pcm_extent_blocks<T, 2>), grid, dim3(256), 0, st, g);
        SH_CHECK_LAUNCH("k_pcm_extent_blocks");
    }
    if (g.shift) {
        grid = sh::grid1d(nblocks, 4);
        for (uint32_t r0 = 0; r0 < nplanes; r0 += 65535u) {
            grid.z = nplanes - r0 < 65535u ? nplanes - r0 : 65535u;
            hipLaunchKernelGGL(k_pcm_extent_fold, grid, dim3(256), 0, st, (const shpe::Row*)parts, g.shift, (uint64_t)nblocks, nplanes, r0, (uint32_t)nch, table);
            SH_CHECK_LAUNCH("k_pcm_extent_fold");
        }
    }
    SH_HIP(hipMemcpyAsync(rows, table, b_table, hipMemcpyDeviceToHost, st));
    SH_HIP(hipStreamSynchronize(st));
    return SH_OK;
}

// what sh_pcm_level_blocks and sh_pcm_extent_blocks refuse, in this order, each under the caller's name `fn`, before anything is
// launched or written
int blocks_check(const char* fn, const sh_buf* in, size_t sample_offset, size_t nframes, int nch, int width, size_t plane_samples, uint32_t nplanes,
                 uint64_t origin_frame, uint64_t block_frames, const void* rows, size_t nblocks) {
    if (!in) return sh::set_error(SH_ERR_INVALID, "%s: NULL buffer", fn);
    if (nch != 1 && nch != 2) return sh::set_error(SH_ERR_INVALID, "%s: %d channels (1 or 2)", fn, nch);
    if (!valid_width3(width)) return sh::set_error(SH_ERR_INVALID, "%s: sample width %d not in {1,2,3,4}", fn, width);
    if (!block_frames) return sh::set_error(SH_ERR_INVALID, "%s: blocks of 0 frames", fn);
    if (!nplanes) return sh::set_error(SH_ERR_INVALID, "%s: 0 planes", fn);
    const size_t have = in->bytes / (size_t)width, n = nframes * (size_t)nch;
    if (nplanes > 1 && (nframes > SIZE_MAX / (size_t)nch || plane_samples < n))
        return sh::set_error(SH_ERR_INVALID, "%s: planes %llu samples apart for a window of %llu: they would overlap", fn,
                             (unsigned long long)plane_samples, (unsigned long long)n);
    bool inside = nframes <= SIZE_MAX / (size_t)nch && sample_offset <= have && n <= have - sample_offset;
    if (inside && nplanes > 1) inside = plane_samples <= (have - sample_offset - n) / (nplanes - 1);
    if (!inside)
        return sh::set_error(SH_ERR_INVALID, "%s: the last of %u planes ends outside in (%llu samples from sample %llu on, planes %llu apart)", fn, nplanes,
                             (unsigned long long)have, (unsigned long long)sample_offset, (unsigned long long)plane_samples);
    if (origin_frame + nframes < origin_frame) return sh::set_error(SH_ERR_INVALID, "%s: the window ends past 2^64 frames", fn);
    const uint64_t want = shpb::nblocks(origin_frame, nframes, block_frames);
    if ((uint64_t)nblocks != want)
        return sh::set_error(SH_ERR_INVALID, "%s: %llu blocks for a window of %llu (blocks of %llu frames)", fn, (unsigned long long)nblocks,
                             (unsigned long long)want, (unsigned long long)block_frames);
    if (!rows && nblocks) return sh::set_error(SH_ERR_INVALID, "%s: NULL rows", fn);
    return SH_OK;
}

// the planes of a checked call of at least one frame as the kernels read them: run(tag, base, stride) with tag a sample of the kernels'
// type and the planes `stride` samples apart from `base` on -- at width 3 the raw 24-bit values as int32, unpacked plane by plane
// into planes nframes * nch samples apart
template <typename Run>
int blocks_planes(const sh_buf* in, size_t sample_offset, size_t nframes, int nch, int width, size_t plane_samples, uint32_t nplanes, Run&& run) {
    const size_t n = nframes * (size_t)nch;
    const char* base = (const char*)in->ptr + sample_offset * (size_t)width;
    if (width == 3) {
        sh::Temp t32;
        int rc = t32.alloc((size_t)nplanes * n * 4);
        if (rc) return rc;
        for (uint32_t r = 0; r < nplanes; ++r) {
            rc = sh::unpack24(base + (size_t)r * plane_samples * 3, n, 0, (int32_t*)t32.buf.ptr + (size_t)r * n);
            if (rc) return rc;
        }
        return run((int)0, (const void*)t32.buf.ptr, n);
    }
    return dispatch_width(width, [&](auto tag) { return run(tag, (const void*)base, plane_samples); });
}
}  // namespace

extern "C" {

int sh_pcm_level_blocks(const sh_buf* in, size_t sample_offset, size_t nframes, int nch, int width, size_t plane_samples, uint32_t nplanes,
                        uint64_t origin_frame, uint64_t block_frames, sh_seq_meter* rows, size_t nblocks) {
    SH_REQUIRE_INIT();
    int rc = blocks_check("sh_pcm_level_blocks", in, sample_offset, nframes, nch, width, plane_samples, nplanes, origin_frame, block_frames, rows, nblocks);
    if (rc || !nframes) return rc;                            // an empty window: no block, nothing launched
    return blocks_planes(in, sample_offset, nframes, nch, width, plane_samples, nplanes, [&](auto tag, const void* base, size_t stride) {
        return level_blocks_run<decltype(tag)>(base, stride, nframes, nch, nplanes, origin_frame, block_frames, rows, nblocks);
    });
}

int sh_pcm_extent_blocks(const sh_buf* in, size_t sample_offset, size_t nframes, int nch, int width, size_t plane_samples, uint32_t nplanes,
                         uint64_t origin_frame, uint64_t block_frames, sh_pcm_extent* rows, size_t nblocks) {
    SH_REQUIRE_INIT();
    int rc = blocks_check("sh_pcm_extent_blocks", in, sample_offset, nframes, nch, width, plane_samples, nplanes, origin_frame, block_frames, rows, nblocks);
    if (rc || !nframes) return rc;
    return blocks_planes(in, sample_offset, nframes, nch, width, plane_samples, nplanes, [&](auto tag, const void* base, size_t stride) {
        return extent_blocks_run<decltype(tag)>(base, stride, nframes, nch, nplanes, origin_frame, block_frames, rows, nblocks);
    });
}

int sh_pcm_mul(const sh_buf* in, size_t in_off, size_t nbytes, int width, double factor, sh_buf* out, size_t out_off) {
    SH_REQUIRE_INIT();
    if (width == 3) {
        if (nbytes % 3 || in_off % 3 || out_off % 3) return sh::set_error(SH_ERR_INVALID, "sh_pcm_mul: not a whole number of frames");      // (each offset: 3 | 6 is no multiple of 3)
        const size_t n = nbytes / 3;
        return via32(in, in_off, n, 8, out, out_off, n, 8, true, "sh_pcm_mul",
                     [&](sh_buf* a, sh_buf* o) { return sh_pcm_mul(a, 0, n * 4, 4, factor, o, 0); });
    }
    if (!valid_width(width)) return bad_width("sh_pcm_mul", width);
    int rc = check_io(in, in_off, nbytes, out, out_off, nbytes, "sh_pcm_mul");
    if (rc) return rc;
    if (nbytes % width || (in_off | out_off) % width) return sh::set_error(SH_ERR_INVALID, "sh_pcm_mul: not a whole number of frames");
    if (!nbytes) return SH_OK;
    hipStream_t st = sh::state().stream;
    return dispatch_width(width, [&](auto tag) {
        typedef decltype(tag) T;
        constexpr int V = 16 / sizeof(T);
        const T* ip = (const T*)((const char*)in->ptr + in_off);
        T* op = (T*)((char*)out->ptr + out_off);
        const VecSplit s = vec_split((((uintptr_t)ip | (uintptr_t)op) & 15) == 0, nbytes / sizeof(T), V);
        if (s.nvec && nbytes > sh::STREAM_BYTES) hipLaunchKernelGGL((k_mul<T, V, true>), sh::grid1d(s.nvec, 256), dim3(256), 0, st, ip, op, s.nvec, factor);
        else if (s.nvec) hipLaunchKernelGGL((k_mul<T, V, false>), sh::grid1d(s.nvec, 256), dim3(256), 0, st, ip, op, s.nvec, factor);
        if (s.rest) hipLaunchKernelGGL((k_mul<T, 1>), sh::grid1d(s.rest, 256), dim3(256), 0, st, ip + s.done, op + s.done, s.rest, factor);
        return launch_result("k_mul");
    });
}

int sh_pcm_fade(const sh_buf* in, size_t in_off, size_t nbytes, int width, int fadeout, double slope, double offset,
                sh_buf* out, size_t out_off) {
    SH_REQUIRE_INIT();
    if (!valid_width(width)) return bad_width("sh_pcm_fade", width);
    int rc = check_io(in, in_off, nbytes, out, out_off, nbytes, "sh_pcm_fade");
    if (rc) return rc;
    if (nbytes % width) return sh::set_error(SH_ERR_INVALID, "sh_pcm_fade: not a whole number of samples");
    if (!nbytes) return SH_OK;
    const size_t n = nbytes / width;
    hipStream_t st = sh::state().stream;
    return dispatch_width(width, [&](auto tag) {
        typedef decltype(tag) T;
        hipLaunchKernelGGL(k_fade<T>, sh::grid1d(n, 256), dim3(256), 0, st, (const T*)((const char*)in->ptr + in_off),
                           (T*)((char*)out->ptr + out_off), n, slope, (double)nbytes / (double)width, offset, fadeout);
        return launch_result("k_fade");
    });
}

int sh_pcm_modulate(const sh_buf* in, size_t nbytes, int width, const sh_buf* mod_f64, size_t nmod, sh_buf* out) {
    SH_REQUIRE_INIT();
    if (!valid_width(width)) return bad_width("sh_pcm_modulate", width);
    int rc = check_io(in, 0, nbytes, out, 0, nbytes, "sh_pcm_modulate");
    if (rc) return rc;
    if (nbytes % width) return sh::set_error(SH_ERR_INVALID, "sh_pcm_modulate: not a whole number of samples");
    if (!nbytes) return SH_OK;
    if (!mod_f64 || !nmod || mod_f64->bytes / 8 < nmod) return sh::set_error(SH_ERR_INVALID, "sh_pcm_modulate: modulator buffer empty or smaller than nmod");
    const size_t n = nbytes / width;
    sh::State& S = sh::state();
    rc = dispatch_width(width, [&](auto tag) {
        typedef decltype(tag) T;
        hipLaunchKernelGGL(k_modulate<T>, sh::grid1d(n, 256), dim3(256), 0, S.stream, (const T*)in->ptr, (T*)out->ptr, n,
                           (const double*)mod_f64->ptr, nmod, S.flag);
        return launch_result("k_modulate");
    });
    return rc ? rc : take_overflow(width);
}

int sh_pcm_pan_lfo(const sh_buf* in, size_t nframes, int width, int nchannels, const sh_buf* pan_f64, sh_buf* out) {
    SH_REQUIRE_INIT();
    if (!valid_width(width)) return bad_width("sh_pcm_pan_lfo", width);
    if (nchannels != 1 && nchannels != 2) return sh::set_error(SH_ERR_INVALID, "sh_pcm_pan_lfo: %d channels (1 or 2)", nchannels);
    int rc = check_io(in, 0, nframes * width * nchannels, out, 0, nframes * width * 2, "sh_pcm_pan_lfo");
    if (rc) return rc;
    if (!nframes) return SH_OK;
    if (!pan_f64 || pan_f64->bytes / 8 < nframes) return sh::set_error(SH_ERR_INVALID, "sh_pcm_pan_lfo: fewer pan values than frames");
    sh::State& S = sh::state();
    rc = dispatch_width(width, [&](auto tag) {
        typedef decltype(tag) T;
        const bool pair = ((uintptr_t)out->ptr & (2 * sizeof(T) - 1)) == 0;       // a view may start on any sample: then two stores per frame
#define SH_PAN(NCH_, PAIR_) hipLaunchKernelGGL((k_pan_lfo<T, NCH_, PAIR_>), sh::grid1d(nframes, 256), dim3(256), 0, S.stream, (const T*)in->ptr, \
                                               (T*)out->ptr, nframes, (const double*)pan_f64->ptr, S.flag)
        if (nchannels == 1) { if (pair) SH_PAN(1, true); else SH_PAN(1, false); }
        else { if (pair) SH_PAN(2, true); else SH_PAN(2, false); }
#undef SH_PAN
        return launch_result("k_pan_lfo");
    });
    return rc ? rc : take_overflow(width);
}

int sh_pcm_to_f64(const sh_buf* in, size_t nsamples, int width, double divisor, sh_buf* out_f64) {
    SH_REQUIRE_INIT();
    if (!valid_width(width)) return bad_width("sh_pcm_to_f64", width);
    int rc = check_io(in, 0, nsamples * width, out_f64, 0, nsamples * 8, "sh_pcm_to_f64");
    if (rc) return rc;
    if (!(divisor != 0.0)) return sh::set_error(SH_ERR_INVALID, "sh_pcm_to_f64: divisor is zero");
    if (!nsamples) return SH_OK;
    hipStream_t st = sh::state().stream;
    return dispatch_width(width, [&](auto tag) {
        typedef decltype(tag) T;
        hipLaunchKernelGGL(k_to_f64<T>, sh::grid1d(nsamples, 256), dim3(256), 0, st, (const T*)in->ptr, (double*)out_f64->ptr, nsamples, divisor);
        return launch_result("k_to_f64");
    });
}

int sh_pcm_bias(const sh_buf* in, size_t nbytes, int width, int bias, sh_buf* out) {
    SH_REQUIRE_INIT();
    if (width == 3) {
        if (nbytes % 3) return sh::set_error(SH_ERR_INVALID, "sh_pcm_bias: not a whole number of frames");
        const size_t n = nbytes / 3;
        const int bias32 = (int)(((unsigned)bias & 0xFFFFFFu) << 8);           // (v + bias) mod 2^24 == ((v << 8) + (bias << 8) mod 2^32) >> 8
        return via32(in, 0, n, 8, out, 0, n, 8, true, "sh_pcm_bias", [&](sh_buf* a, sh_buf* o) { return sh_pcm_bias(a, n * 4, 4, bias32, o); });
    }
    if (!valid_width(width)) return bad_width("sh_pcm_bias", width);
    int rc = check_io(in, 0, nbytes, out, 0, nbytes, "sh_pcm_bias");
    if (rc) return rc;
    if (nbytes % width) return sh::set_error(SH_ERR_INVALID, "sh_pcm_bias: not a whole number of frames");
    if (!nbytes) return SH_OK;
    const size_t n = nbytes / width;
    hipStream_t st = sh::state().stream;
    return dispatch_width(width, [&](auto tag) {
        typedef decltype(tag) T;
        hipLaunchKernelGGL(k_bias<T>, sh::grid1d(n, 256), dim3(256), 0, st, (const T*)in->ptr, (T*)out->ptr, n, bias);
        return launch_result("k_bias");
    });
}

int sh_pcm_reverse(const sh_buf* in, size_t nbytes, int width, sh_buf* out) {
    SH_REQUIRE_INIT();
    if (width == 3) {
        if (nbytes % 3) return sh::set_error(SH_ERR_INVALID, "sh_pcm_reverse: not a whole number of frames");
        const size_t n = nbytes / 3;
        return via32(in, 0, n, 0, out, 0, n, 0, false, "sh_pcm_reverse", [&](sh_buf* a, sh_buf* o) { return sh_pcm_reverse(a, n * 4, 4, o); });
    }
    if (!valid_width(width)) return bad_width("sh_pcm_reverse", width);
    int rc = check_io(in, 0, nbytes, out, 0, nbytes, "sh_pcm_reverse");
    if (rc) return rc;
    if (nbytes % width) return sh::set_error(SH_ERR_INVALID, "sh_pcm_reverse: not a whole number of frames");
    if (!nbytes) return SH_OK;
    if (in == out || in->ptr == out->ptr) return sh::set_error(SH_ERR_INVALID, "sh_pcm_reverse: cannot reverse in place");
    const size_t n = nbytes / width;
    hipStream_t st = sh::state().stream;
    return dispatch_width(width, [&](auto tag) {
        typedef decltype(tag) T;
        hipLaunchKernelGGL(k_reverse<T>, sh::grid1d(n, 256), dim3(256), 0, st, (const T*)in->ptr, (T*)out->ptr, n);
        return launch_result("k_reverse");
    });
}

int sh_pcm_tomono(const sh_buf* in, size_t nframes, int width, double lfactor, double rfactor, sh_buf* out) {
    SH_REQUIRE_INIT();
    if (width == 3)
        return via32(in, 0, nframes * 2, 8, out, 0, nframes, 8, false, "sh_pcm_tomono",
                     [&](sh_buf* a, sh_buf* o) { return sh_pcm_tomono(a, nframes, 4, lfactor, rfactor, o); });
    if (!valid_width(width)) return bad_width("sh_pcm_tomono", width);
    int rc = check_io(in, 0, nframes * 2 * width, out, 0, nframes * width, "sh_pcm_tomono");
    if (rc) return rc;
    if (!nframes) return SH_OK;
    hipStream_t st = sh::state().stream;
    return dispatch_width(width, [&](auto tag) {
        typedef decltype(tag) T;
        constexpr int F = 8 / sizeof(T);                       // frames per 16-byte load
        // (a view may start on any sample: the vector kernel only where its 16-byte loads and 8-byte stores are aligned, the
        // one-frame kernel's two-sample load only where a frame is)
        const bool aligned = ((uintptr_t)in->ptr & 15) == 0 && ((uintptr_t)out->ptr & 7) == 0;
        const bool pair = ((uintptr_t)in->ptr & (2 * sizeof(T) - 1)) == 0;
        const VecSplit s = vec_split(aligned, nframes, F);
        if (s.nvec) hipLaunchKernelGGL((k_tomono<T, F>), sh::grid1d(s.nvec, 256), dim3(256), 0, st, (const T*)in->ptr, (T*)out->ptr, s.nvec, lfactor, rfactor);
        if (s.rest && pair) hipLaunchKernelGGL((k_tomono<T, 1>), sh::grid1d(s.rest, 256), dim3(256), 0, st,
                                               (const T*)in->ptr + 2 * s.done, (T*)out->ptr + s.done, s.rest, lfactor, rfactor);
        else if (s.rest) hipLaunchKernelGGL((k_tomono<T, 1, false>), sh::grid1d(s.rest, 256), dim3(256), 0, st,
                                            (const T*)in->ptr + 2 * s.done, (T*)out->ptr + s.done, s.rest, lfactor, rfactor);
        return launch_result("k_tomono");
    });
}

int sh_pcm_tostereo(const sh_buf* in, size_t nframes, int width, double lfactor, double rfactor, sh_buf* out) {
    SH_REQUIRE_INIT();
    if (width == 3)
        return via32(in, 0, nframes, 8, out, 0, nframes * 2, 8, false, "sh_pcm_tostereo",
                     [&](sh_buf* a, sh_buf* o) { return sh_pcm_tostereo(a, nframes, 4, lfactor, rfactor, o); });
    if (!valid_width(width)) return bad_width("sh_pcm_tostereo", width);
    int rc = check_io(in, 0, nframes * width, out, 0, nframes * 2 * width, "sh_pcm_tostereo");
    if (rc) return rc;
    if (!nframes) return SH_OK;
    hipStream_t st = sh::state().stream;
    return dispatch_width(width, [&](auto tag) {
        typedef decltype(tag) T;
        constexpr int F = 8 / sizeof(T);                       // frames per 16-byte store
        // (as sh_pcm_tomono: 8-byte loads and 16-byte stores only where aligned, the one-frame kernel's two-sample store only where a frame is)
        const bool aligned = ((uintptr_t)in->ptr & 7) == 0 && ((uintptr_t)out->ptr & 15) == 0;
        const bool pair = ((uintptr_t)out->ptr & (2 * sizeof(T) - 1)) == 0;
        const VecSplit s = vec_split(aligned, nframes, F);
        if (s.nvec) hipLaunchKernelGGL((k_tostereo<T, F>), sh::grid1d(s.nvec, 256), dim3(256), 0, st, (const T*)in->ptr, (T*)out->ptr, s.nvec, lfactor, rfactor);
        if (s.rest && pair) hipLaunchKernelGGL((k_tostereo<T, 1>), sh::grid1d(s.rest, 256), dim3(256), 0, st,
                                               (const T*)in->ptr + s.done, (T*)out->ptr + 2 * s.done, s.rest, lfactor, rfactor);
        else if (s.rest) hipLaunchKernelGGL((k_tostereo<T, 1, false>), sh::grid1d(s.rest, 256), dim3(256), 0, st,
                                            (const T*)in->ptr + s.done, (T*)out->ptr + 2 * s.done, s.rest, lfactor, rfactor);
        return launch_result("k_tostereo");
    });
}

int sh_pcm_lin2lin(const sh_buf* in, size_t nsamples, int width, int new_width, sh_buf* out) {
    SH_REQUIRE_INIT();
    if (width == 3 || new_width == 3) {
        if (!in || !out) return sh::set_error(SH_ERR_INVALID, "sh_pcm_lin2lin: NULL buffer");
        if (!valid_width3(width) || !valid_width3(new_width))
            return sh::set_error(SH_ERR_INVALID, "sh_pcm_lin2lin: widths %d -> %d not in {1,2,3,4}", width, new_width);
        if (nsamples * (size_t)width > in->bytes || nsamples * (size_t)new_width > out->bytes)
            return sh::set_error(SH_ERR_INVALID, "sh_pcm_lin2lin: range outside buffer");
        if (!nsamples) return SH_OK;
        // GETSAMPLE32 of a 24-bit sample is value << 8; SETSAMPLE32 to 24 bits keeps value >> 8
        sh::Temp t32;
        int rc3 = t32.alloc(nsamples * 4);
        if (rc3) return rc3;
        rc3 = width == 3 ? sh::unpack24(in->ptr, nsamples, 8, (int32_t*)t32.buf.ptr) : sh_pcm_lin2lin(in, nsamples, width, 4, &t32.buf);
        if (rc3) return rc3;
        return new_width == 3 ? sh::pack24((const int32_t*)t32.buf.ptr, nsamples, 8, out->ptr) : sh_pcm_lin2lin(&t32.buf, nsamples, 4, new_width, out);
    }
    int rc = check_io(in, 0, nsamples * width, out, 0, nsamples * new_width, "sh_pcm_lin2lin");
    if (rc) return rc;
    if (!nsamples) return SH_OK;
    hipStream_t st = sh::state().stream;
    return dispatch_width(width, [&](auto tin) {
        return dispatch_width(new_width, [&](auto tout) {
            typedef decltype(tin) TI;
            typedef decltype(tout) TO;
            hipLaunchKernelGGL((k_lin2lin<TI, TO>), sh::grid1d(nsamples, 256), dim3(256), 0, st, (const TI*)in->ptr, (TO*)out->ptr, nsamples);
            return launch_result("k_lin2lin");
        });
    });
}

int sh_pcm_stats(const sh_buf* in, size_t nbytes, int width, uint32_t* max_abs, double* sum_squares) {
    SH_REQUIRE_INIT();
    if (!valid_width3(width)) return bad_width("sh_pcm_stats", width);           // (width 3: raw 24-bit values, audioop.max / rms read GETRAWSAMPLE)
    if (nbytes % width) return sh::set_error(SH_ERR_INVALID, "sh_pcm_stats: not a whole number of frames");
    return pcm_stats<1>("sh_pcm_stats", in, nbytes / width, width, max_abs, sum_squares);
}

int sh_pcm_stats_stereo(const sh_buf* in, size_t nframes, int width, uint32_t max_abs[2], double sum_squares[2]) {
    SH_REQUIRE_INIT();
    if (!valid_width3(width)) return bad_width("sh_pcm_stats_stereo", width);
    return pcm_stats<2>("sh_pcm_stats_stereo", in, nframes, width, max_abs, sum_squares);
}

}  // extern "C"
