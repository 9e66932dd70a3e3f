// pcm.hip -- integer/float PCM kernels: quantise, saturating add (Sample.mix) and the mixer's
// saturating chain.  (Linear-interpolation resampling, Sample.resample: resample.hip.)
//
// These restate CPython 3.10 Modules/audioop.c (audioop_add_impl), the arithmetic synthplayer's
// sample.py delegates to.  All of them are HBM-bound byte/integer work: coalesced loads, one output
// element (or a small vector) per thread, no LDS except for the cross-wave combine of the mixer
// chain.  Built with -ffp-contract=off (float64 products stay two roundings).
#include "common.hpp"
#include "chain.hpp"
#include "pcmdev.hpp"
#include "pcmhost.hpp"
#include <mutex>
#include <string.h>
#include <new>
#include <type_traits>

#define SH_PCM_CONST __attribute__((address_space(4)))

namespace {

typedef int   int4v   __attribute__((ext_vector_type(4)));
typedef char  char16v __attribute__((ext_vector_type(16)));

// ---- quantise: int(scale*v), truncation toward zero (sample.py Sample.from_osc_block) -------
// rnd (sh_set_option(SH_OPT_QUANTISE_ROUND)): the other reading of the reference's rule, round(scale*v) -- half to even, rint -- in
// place of int()'s truncation toward zero; never with clip (the saturating forms are this build's own: [SPEC]).
template <typename OutT, typename InT = float>
__global__ __launch_bounds__(256) void k_quantize(const InT* __restrict__ in, size_t n, double scale,
                                                  double lo, double hi, OutT* __restrict__ out,
                                                  int* __restrict__ flag, int clip, int rnd = 0) {
    size_t i = sh::block_id() * 256 + threadIdx.x;
    if (i >= n) return;
    double v = scale * (double)in[i];          // float64 product, like the Python expression
    double t = rnd ? rint(v) : trunc(v);
    if (!(t >= lo && t <= hi)) {               // also catches NaN
        if (clip) {
            t = (t > hi) ? hi : lo;
            if (v != v) t = 0.0;
        } else {
            *flag = 1;
            t = 0.0;
        }
    }
    out[i] = (OutT)(long long)t;
}

// The vector forms: a workgroup covers 512 vectors of 16 bytes, each thread two of them 256 apart -- every load instruction
// of a wave reads one contiguous kilobyte (streaming: nothing is read twice) and every store instruction writes a contiguous
// 256 / 512 bytes.  round 3 microbenchmark (profiles/r03_summary.md): float64 6.3 TB/s this way, 5.8 with eight consecutive samples per thread and a
// 16-byte store, 4.4 with those loads marked non-temporal, 4.9 one sample per thread.
template <bool CLIP>
__device__ __forceinline__ short quantize16(double p, bool& bad, bool rnd = false) {
    double t = rnd ? rint(p) : trunc(p);
    if (!(t >= -32768.0 && t <= 32767.0)) {                  // also catches NaN
        if (CLIP) { t = (t > 32767.0) ? 32767.0 : -32768.0; if (p != p) t = 0.0; }
        else { bad = true; t = 0.0; }
    }
    return (short)(int)t;
}

// float32 -> int16, four samples per 16-byte vector
typedef float float4v __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_quantize_f32_i16_vec(const float4v* __restrict__ in, size_t nvec, double scale,
                                                              short4v* __restrict__ out, int* __restrict__ flag, int clip, int rnd = 0) {
    const size_t base = sh::block_id() * 512 + threadIdx.x;
    float4v v[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) if (base + u * 256 < nvec) v[u] = __builtin_nontemporal_load(in + base + u * 256);
    bool bad = false;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        if (base + u * 256 >= nvec) break;
        short4v r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = clip ? quantize16<true>(scale * (double)v[u][j], bad) : quantize16<false>(scale * (double)v[u][j], bad, rnd != 0);
        __builtin_nontemporal_store(r, out + base + u * 256);       // streaming store: +3.5 %
    }
    if (bad) *flag = 1;
}

// float64 -> int16, two samples per 16-byte vector; the route WaveSynth.to_sample takes
typedef double double2v __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(256) void k_quantize_f64_i16_vec(const double2v* __restrict__ in, size_t nvec, double scale,
                                                              short2v* __restrict__ out, int* __restrict__ flag, int rnd = 0) {
    const size_t base = sh::block_id() * 512 + threadIdx.x;
    double2v v[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) if (base + u * 256 < nvec) v[u] = __builtin_nontemporal_load(in + base + u * 256);
    bool bad = false;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        if (base + u * 256 >= nvec) break;
        short2v r;
        r[0] = quantize16<false>(scale * v[u][0], bad, rnd != 0);
        r[1] = quantize16<false>(scale * v[u][1], bad, rnd != 0);
        __builtin_nontemporal_store(r, out + base + u * 256);       // streaming store: +3.5 %
    }
    if (bad) *flag = 1;
}

// ---- audioop.add (no __restrict__: Sample.mix_at adds in place) ---------------------------------
template <typename V, bool NT>
__global__ __launch_bounds__(256) void k_add_vec(const V* a, const V* b, V* o, size_t nvec) {
    size_t i = sh::block_id() * 256 + threadIdx.x;
    if (i >= nvec) return;
    const V r = __builtin_elementwise_add_sat(sh::load_vec<NT, V>(a + i), sh::load_vec<NT, V>(b + i));
    if (NT) __builtin_nontemporal_store(r, o + i); else o[i] = r;        // streaming sizes: loads +3 %, store +4 %
}

template <typename T>
__global__ __launch_bounds__(256) void k_add_scalar(const T* a, const T* b,
                                                    T* o, size_t n) {
    size_t i = sh::block_id() * 256 + threadIdx.x;
    if (i >= n) return;
    o[i] = __builtin_elementwise_add_sat(a[i], b[i]);
}


// ---- mixer chain: mixed = add(...add(add(c0, c1), c2)..., c_{N-1}), saturating at every step ----
// The chain over a range of voices is one map x -> clamp(x + a, L, U) per value (chain.hpp), so each wave folds a contiguous range of
// voices into its map and the first waves apply the W maps in voice order to x = 0.  Bit-exact with the sequential fold.

// sh_chain_parts_compose / _apply: nparts stored planes of maps, plane k at parts[k * plane], folded in order per value -- composed
// into one map (APPLY false) or applied to x0 (or 0).
template <bool APPLY>
__global__ __launch_bounds__(256) void k_chain_parts(const int2v* parts, uint32_t nparts, size_t plane, uint32_t n,
                                                     const short* __restrict__ x0, int2v* out_maps, short* __restrict__ out) {
    const uint32_t f = (uint32_t)(sh::block_id() * 256 + threadIdx.x);
    if (f >= n) return;
    if constexpr (APPLY) out[f] = (short)shc::apply_planes<shc::STORED, false>(parts + f, nparts, plane, x0 ? (int)x0[f] : 0);
    else out_maps[f] = shc::store(shc::compose_planes<shc::STORED, false>(parts + f, nparts, plane));
}

// Where a split kernel's voice v gives its 8 samples from s0.  whole(): (uniform) every voice's 8 samples are one aligned vector --
// decided once, outside the voice loop; tail(): the ragged form, zeros past the end.  vec: every row starts on the vector's grid --
// decided on the host (rows_vec) from the row pointer AND the stride: 16 bytes for the eight mono samples, 8 for the four PAN frames.
// Strided rows (PAN forms, sh_mix_chain_pan_i16: the rows are MONO voices and each enters the fold as Sample.stereo(lf, rf) of itself,
// shc::stereo on the four mono frames of eight stereo samples; the factors of a voice are wave-uniform: scalar loads).
template <bool NT>
struct RowSrc {
    const short* __restrict__ chunks;
    size_t stride;
    const double2* __restrict__ pan;
    uint32_t vec;
    __device__ __forceinline__ bool whole(uint32_t s0, uint32_t nsamples) const { return s0 + 7 < nsamples && vec != 0; }
    __device__ __forceinline__ short8v load(uint32_t v, uint32_t s0) const {
        if (pan) {                                       // (uniform) s0 = the first of eight STEREO samples: four mono frames from s0 / 2
            const double2 f = pan[v];
            return shc::stereo<4>(sh::load_vec<NT, short4v>(chunks + v * stride + (s0 >> 1)), f.x, f.y);
        }
        return sh::load_vec<NT, short8v>(chunks + v * stride + s0);
    }
    __device__ __forceinline__ short8v tail(uint32_t v, uint32_t s0, uint32_t nsamples) const {
        if (pan) {
            const short* row = chunks + (size_t)v * stride + (s0 >> 1);
            short4v m;
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = (s0 + 2 * j < nsamples) ? row[j] : (short)0;
            const double2 fac = pan[v];
            return shc::stereo<4>(m, fac.x, fac.y);
        }
        const short* row = chunks + (size_t)v * stride + s0;
        short8v x;
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = (s0 + j < nsamples) ? row[j] : (short)0;
        return x;
    }
};

// Chunks that live where their samples live: a table of (pointer, samples available) per source instead of one padded array -- the
// real-time mixer's loop without the staging copy (every active sample is read in place at its play position; past its end it counts
// as silence, which the fold skips: x + 0 saturates to x).  Each load decides for itself between the vector and the ragged form.
struct ChainSrc {
    const short* p;
    uint32_t n;
    uint32_t pad;
};
__device__ __forceinline__ short8v chain_load8(const short* p, uint32_t n, uint32_t s0) {
    short8v x = {0, 0, 0, 0, 0, 0, 0, 0};
    if (s0 + 8 <= n && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        x = *reinterpret_cast<const short8v*>(p + s0);
    } else if (s0 < n) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (s0 + j < n) x[j] = p[s0 + j];
    }
    return x;
}
struct TableSrc {
    const ChainSrc* __restrict__ tab;
    __device__ __forceinline__ bool whole(uint32_t, uint32_t) const { return true; }
    __device__ __forceinline__ short8v load(uint32_t v, uint32_t s0) const { const ChainSrc c = tab[v]; return chain_load8(c.p, c.n, s0); }
    __device__ __forceinline__ short8v tail(uint32_t v, uint32_t s0, uint32_t) const { return load(v, s0); }
};

// The split fold: WAVES waves = (WAVES / COLS) voice ranges x COLS adjacent 1 KB columns (a workgroup visits COLS KB of a row at a
// time), eight samples per lane; PARTS (sh_mix_chain_i16_parts, sh_mix_chain_pan_i16_parts): the map of all the voices is stored
// (sh_chain_map, 8 bytes per sample, in maps) instead of its result.
template <int WAVES, int COLS, bool PARTS, typename Src>
__device__ __forceinline__ void mix_chain_split(const Src src, uint32_t nvoices, uint32_t nsamples, short* __restrict__ out,
                                                int2v* __restrict__ maps) {
    constexpr int VG = WAVES / COLS;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t col = wave % COLS, vg = wave / COLS;
    const uint32_t s0 = (((uint32_t)sh::block_id() * COLS + col) * 64 + lane) * 8;        // (grid1d folds beyond 2^21 workgroups)
    const uint32_t per = (nvoices + VG - 1) / VG;
    const uint32_t v0 = vg * per;
    uint32_t v1 = v0 + per;
    if (v1 > nvoices) v1 = nvoices;
    shc::ChainFold f;
    f.init();
    if (s0 < nsamples && v0 < v1) {
        if (src.whole(s0, nsamples)) {
            uint32_t v = v0;
            f.first(src.load(v, s0));                     // (a table source past its end contributes zeros: still a voice of the fold)
            ++v;
            for (; v + 3 < v1; v += 4) {                  // four voices in flight
                const short8v x0 = src.load(v, s0);
                const short8v x1 = src.load(v + 1, s0);
                const short8v x2 = src.load(v + 2, s0);
                const short8v x3 = src.load(v + 3, s0);
                f.add(x0); f.add(x1); f.add(x2); f.add(x3);
            }
            for (; v < v1; ++v) f.add(src.load(v, s0));
        } else {
            for (uint32_t v = v0; v < v1; ++v) {
                const short8v x = src.tail(v, s0, nsamples);
                if (v == v0) f.first(x); else f.add(x);
            }
        }
    }
    shc::split_store<WAVES, COLS, PARTS>(f, wave, lane, s0, nsamples, out, maps);
}

template <int WAVES, int COLS, bool NT, bool PARTS = false>
__global__ __launch_bounds__(WAVES * 64) void k_mix_chain_i16(const short* __restrict__ chunks, uint32_t nvoices,
                                                              size_t stride, uint32_t nsamples,
                                                              short* __restrict__ out, uint32_t vec, const double2* __restrict__ pan = nullptr,
                                                              int2v* __restrict__ maps = nullptr) {
    mix_chain_split<WAVES, COLS, PARTS>(RowSrc<NT>{chunks, stride, pan, vec}, nvoices, nsamples, out, maps);
}

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_mix_chain_gather(const ChainSrc* __restrict__ tab, uint32_t nsrc, uint32_t nsamples,
                                                                 short* __restrict__ out) {
    mix_chain_split<WAVES, 1, false>(TableSrc{tab}, nsrc, nsamples, out, nullptr);
}

// The same with the source table IN the kernel arguments (up to 64 sources: one real-time mixer turn): no table upload in front of
// the launch -- the copy of a pageable kilobyte costs more than the kernel.
struct ChainTab { ChainSrc e[64]; };
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_mix_chain_gather_args(const ChainTab tab, uint32_t nsrc, uint32_t nsamples,
                                                                      short* __restrict__ out) {
    mix_chain_split<WAVES, 1, false>(TableSrc{tab.e}, nsrc, nsamples, out, nullptr);
}

// Long buffers: enough columns to fill the chip without splitting the voices, so a lane simply runs the reference's loop --
// mixed = add_sat(mixed, row) down all the rows, packed int16 -- with S samples (F frames) per lane, INFLIGHT independent row loads, no
// fold state, no LDS.  From 1536 1 KB columns eight samples per lane (NTS false: a plain store).  For rows of MIDDLING length (a few
// hundred thousand samples: too few 1 KB columns to fill the chip with eight samples per lane, more than the split kernels like) four
// samples per lane -- 8-byte loads, twice the wavefronts, eight row loads in flight -- run the mono chain at 0.87 of the HBM peak where
// the split kernel reaches 0.74 (1024 rows x 480 000 samples: 166 -> 142 us).  The PAN chain -- mono rows that enter as
// Sample.stereo(lf, rf) of themselves, see shc::stereo -- is bound by its float64 arithmetic (ten operations per frame), not by HBM:
// four frames per lane at every length from ~300 000 frames (480 000: 290 -> 202 us, 0.61 of HBM; 960 000: 392 -> 358 us, 0.69);
// eight frames per lane were slower at both.
template <int S, int WAVES, int INFLIGHT, bool NT, bool NTS = true>
__global__ __launch_bounds__(WAVES * 64) void k_mix_chain_direct_s(const short* __restrict__ chunks, uint32_t nvoices, size_t stride,
                                                                   uint32_t nsamples, short* __restrict__ out) {
    typedef typename ShortVec<S>::type vec;
    const uint32_t s0 = (uint32_t)(sh::block_id() * (WAVES * 64) + threadIdx.x) * S;
    if (s0 >= nsamples) return;
    const short* col = chunks + s0;
    if (s0 + S <= nsamples) {
        vec acc = *reinterpret_cast<const vec*>(col);
        uint32_t v = 1;
        for (; v + INFLIGHT <= nvoices; v += INFLIGHT) {
            vec x[INFLIGHT];
#pragma unroll
            for (int k = 0; k < INFLIGHT; ++k) x[k] = sh::load_vec<NT, vec>(col + (size_t)(v + k) * stride);     // NT: 0.81 -> 0.90 of the HBM peak on 2 GB
#pragma unroll
            for (int k = 0; k < INFLIGHT; ++k) acc = __builtin_elementwise_add_sat(acc, x[k]);
        }
        for (; v < nvoices; ++v) acc = __builtin_elementwise_add_sat(acc, *reinterpret_cast<const vec*>(col + (size_t)v * stride));
        if (NTS) __builtin_nontemporal_store(acc, reinterpret_cast<vec*>(out + s0));
        else *reinterpret_cast<vec*>(out + s0) = acc;
    } else {
        for (uint32_t j = 0; s0 + j < nsamples; ++j) {
            short acc = col[j];
            for (uint32_t v = 1; v < nvoices; ++v) acc = __builtin_elementwise_add_sat(acc, col[(size_t)v * stride + j]);
            out[s0 + j] = acc;
        }
    }
}

template <int F, int WAVES, int INFLIGHT, bool NT>
__global__ __launch_bounds__(WAVES * 64) void k_mix_chain_pan_direct_s(const short* __restrict__ chunks, uint32_t nvoices, size_t stride,
                                                                       uint32_t nframes, const double2* __restrict__ pan, short* __restrict__ out) {
    typedef typename ShortVec<F>::type vin;                       // F mono frames in, 2 F stereo samples out
    typedef typename ShortVec<2 * F>::type vout;
    const uint32_t f0 = (uint32_t)(sh::block_id() * (WAVES * 64) + threadIdx.x) * F;
    if (f0 >= nframes) return;
    const short* col = chunks + f0;
    const double SH_PCM_CONST* fac = (const double SH_PCM_CONST*)pan;
    if (f0 + F <= nframes) {
        vout acc = shc::stereo<F>(*reinterpret_cast<const vin*>(col), fac[0], fac[1]);
        uint32_t v = 1;
        for (; v + INFLIGHT <= nvoices; v += INFLIGHT) {
            vin x[INFLIGHT];
#pragma unroll
            for (int k = 0; k < INFLIGHT; ++k) x[k] = sh::load_vec<NT, vin>(col + (size_t)(v + k) * stride);
#pragma unroll
            for (int k = 0; k < INFLIGHT; ++k) acc = __builtin_elementwise_add_sat(acc, shc::stereo<F>(x[k], fac[2 * (v + k)], fac[2 * (v + k) + 1]));
        }
        for (; v < nvoices; ++v) acc = __builtin_elementwise_add_sat(acc, shc::stereo<F>(*reinterpret_cast<const vin*>(col + (size_t)v * stride), fac[2 * v], fac[2 * v + 1]));
        __builtin_nontemporal_store(acc, reinterpret_cast<vout*>(out + 2 * (size_t)f0));
    } else {
        for (uint32_t j = 0; f0 + j < nframes; ++j) {
            short2v acc = {0, 0};
            for (uint32_t v = 0; v < nvoices; ++v) {
                const short2v p = shc::stereo1(col[(size_t)v * stride + j], fac[2 * v], fac[2 * v + 1]);
                acc = v == 0 ? p : __builtin_elementwise_add_sat(acc, p);
            }
            out[2 * (size_t)(f0 + j)] = acc[0];
            out[2 * (size_t)(f0 + j) + 1] = acc[1];
        }
    }
}

// the direct loop over the pointer table (long samples: mix_samples of whole tracks)
template <int WAVES, int INFLIGHT, bool NT>
__global__ __launch_bounds__(WAVES * 64) void k_mix_chain_gather_direct(const ChainSrc* __restrict__ tab, uint32_t nsrc, uint32_t nsamples,
                                                                        short* __restrict__ out) {
    const uint32_t s0 = (blockIdx.x * (WAVES * 64) + threadIdx.x) * 8;
    const uint32_t wave_s0 = __builtin_amdgcn_readfirstlane(s0 - (threadIdx.x & 63) * 8);
    if (s0 >= nsamples) return;
    short8v acc = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t v = 0;
    if (nsrc >= INFLIGHT) {
        ChainSrc c[INFLIGHT], nx[INFLIGHT];               // table entries one batch ahead: their scalar loads overlap the row loads
#pragma unroll
        for (int k = 0; k < INFLIGHT; ++k) c[k] = tab[k];
        for (; v + INFLIGHT <= nsrc; v += INFLIGHT) {
            const bool more = v + 2 * INFLIGHT <= nsrc;
            if (more) {
#pragma unroll
                for (int k = 0; k < INFLIGHT; ++k) nx[k] = tab[v + INFLIGHT + k];
            }
            short8v x[INFLIGHT];
            bool whole = true;                            // wave-uniform: every source of the batch covers this wave's 1 KB, aligned
#pragma unroll
            for (int k = 0; k < INFLIGHT; ++k) whole = whole && wave_s0 + 512 <= c[k].n && (reinterpret_cast<uintptr_t>(c[k].p) & 15) == 0;
            if (whole) {
#pragma unroll
                for (int k = 0; k < INFLIGHT; ++k) x[k] = sh::load_vec<NT, short8v>(c[k].p + s0);
            } else {
#pragma unroll
                for (int k = 0; k < INFLIGHT; ++k) x[k] = chain_load8(c[k].p, c[k].n, s0);
            }
#pragma unroll
            for (int k = 0; k < INFLIGHT; ++k) acc = __builtin_elementwise_add_sat(acc, x[k]);
            if (more) {
#pragma unroll
                for (int k = 0; k < INFLIGHT; ++k) c[k] = nx[k];
            }
        }
    }
    for (; v < nsrc; ++v) {
        const ChainSrc c = tab[v];
        acc = __builtin_elementwise_add_sat(acc, chain_load8(c.p, c.n, s0));
    }
    if (s0 + 8 <= nsamples && ((reinterpret_cast<uintptr_t>(out + s0) & 15) == 0)) {
        *reinterpret_cast<short8v*>(out + s0) = acc;
    } else {
        for (uint32_t j = 0; j < 8 && s0 + j < nsamples; ++j) out[s0 + j] = acc[j];
    }
}

// ---- the mixer fold for the other sample widths audioop.add takes (8, 24 and 32 bits) -------------------------------------
// The reference's loop as it stands -- mixed = clamp(mixed + sample) down the sources, in their order, per output sample --
// with four consecutive samples per thread and the source table read by scalar loads (uniform).  8-bit and 24-bit samples are
// assembled from bytes (a 24-bit sample: GETINT24, sign-extended; stored back as its three low bytes), 32-bit sums are taken in
// 64 bits.  Sources past their end count as silence.  These widths are the mixer's side door -- WAV files that were not
// converted to 16 bits first -- so the kernel is the plain one; the 16-bit shapes above are the tuned ones.
struct ChainSrcB {
    const unsigned char* p;
    uint32_t n;               // samples available
    uint32_t pad;
};

template <int WIDTH>
__global__ __launch_bounds__(256) void k_mix_chain_gather_w(const ChainSrcB* __restrict__ tab, uint32_t nsrc, uint32_t nsamples,
                                                            unsigned char* __restrict__ out) {
    const size_t s0 = (sh::block_id() * 256 + threadIdx.x) * 4;
    if (s0 >= nsamples) return;
    constexpr long long HI = WIDTH == 1 ? 127LL : (WIDTH == 3 ? 8388607LL : 2147483647LL), LO = -HI - 1;
    long long acc[4] = {0, 0, 0, 0};
    for (uint32_t v = 0; v < nsrc; ++v) {
        const unsigned char* p = tab[v].p;
        const uint32_t n = tab[v].n;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t i = s0 + j;
            if (i < n) {
                const long long t = acc[j] + chain_get<WIDTH>(p, i);
                acc[j] = t > HI ? HI : (t < LO ? LO : t);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (s0 + j < nsamples) chain_put<WIDTH>(out, s0 + j, acc[j]);
}

}  // namespace

extern "C" {

int sh_quantize_f32(const sh_buf* in_f32, size_t in_off, size_t n, double scale, int width,
                    sh_buf* out_pcm, size_t out_off) {
    SH_REQUIRE_INIT();
    if (!in_f32 || !out_pcm) return sh::set_error(SH_ERR_INVALID, "sh_quantize_f32: NULL argument");
    if (!valid_width(width)) return bad_width("sh_quantize_f32", width);
    if (in_off > in_f32->bytes / 4 || n > in_f32->bytes / 4 - in_off) return sh::set_error(SH_ERR_INVALID, "sh_quantize_f32: input range outside buffer");
    if (out_off > out_pcm->bytes / width || n > out_pcm->bytes / width - out_off) return sh::set_error(SH_ERR_INVALID, "sh_quantize_f32: output range outside buffer");
    if (!n) return SH_OK;
    const double lo = -ldexp(1.0, 8 * width - 1), hi = ldexp(1.0, 8 * width - 1) - 1.0;
    const float* in = (const float*)in_f32->ptr + in_off;
    hipStream_t st = sh::state().stream;
    int* flag = sh::state().flag;
    const int rnd = sh::state().quantise_round;
    const int rc = dispatch_width(width, [&](auto tag) {
        typedef decltype(tag) T;
        T* o = (T*)out_pcm->ptr + out_off;
        const VecSplit s = vec_split(sizeof(T) == 2 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)o & 7) == 0, n, 4);      // the vector kernel is the 16-bit one
        if (s.nvec) hipLaunchKernelGGL(k_quantize_f32_i16_vec, sh::grid1d(s.nvec, 512), dim3(256), 0, st, (const float4v*)in, s.nvec, scale, (short4v*)o, flag, 0, rnd);
        if (s.rest) hipLaunchKernelGGL(k_quantize<T>, sh::grid1d(s.rest, 256), dim3(256), 0, st, in + s.done, s.rest, scale, lo, hi, o + s.done, flag, 0, rnd);
        return launch_result("k_quantize");
    });
    return rc ? rc : take_overflow(width);
}

int sh_quantize_f64(const sh_buf* in_f64, size_t in_off, size_t n, double scale, int width,
                    sh_buf* out_pcm, size_t out_off) {
    SH_REQUIRE_INIT();
    if (!in_f64 || !out_pcm) return sh::set_error(SH_ERR_INVALID, "sh_quantize_f64: NULL argument");
    if (!valid_width(width)) return bad_width("sh_quantize_f64", width);
    if (in_off > in_f64->bytes / 8 || n > in_f64->bytes / 8 - in_off) return sh::set_error(SH_ERR_INVALID, "sh_quantize_f64: input range outside buffer");
    if (out_off > out_pcm->bytes / width || n > out_pcm->bytes / width - out_off) return sh::set_error(SH_ERR_INVALID, "sh_quantize_f64: output range outside buffer");
    if (!n) return SH_OK;
    const double lo = -ldexp(1.0, 8 * width - 1), hi = ldexp(1.0, 8 * width - 1) - 1.0;
    const double* in = (const double*)in_f64->ptr + in_off;
    hipStream_t st = sh::state().stream;
    int* flag = sh::state().flag;
    const int rnd = sh::state().quantise_round;
    const int rc = dispatch_width(width, [&](auto tag) {
        typedef decltype(tag) T;
        T* o = (T*)out_pcm->ptr + out_off;
        const VecSplit s = vec_split(sizeof(T) == 2 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)o & 3) == 0, n, 2);      // the vector kernel is the 16-bit one
        if (s.nvec) hipLaunchKernelGGL(k_quantize_f64_i16_vec, sh::grid1d(s.nvec, 512), dim3(256), 0, st, (const double2v*)in, s.nvec, scale, (short2v*)o, flag, rnd);
        if (s.rest) hipLaunchKernelGGL((k_quantize<T, double>), sh::grid1d(s.rest, 256), dim3(256), 0, st, in + s.done, s.rest, scale, lo, hi, o + s.done, flag, 0, rnd);
        return launch_result("k_quantize");
    });
    return rc ? rc : take_overflow(width);
}

int sh_quantize_clip_f32(const sh_buf* in_f32, size_t n, double scale, sh_buf* out_i16) {
    SH_REQUIRE_INIT();
    if (!in_f32 || !out_i16) return sh::set_error(SH_ERR_INVALID, "sh_quantize_clip_f32: NULL argument");
    if (in_f32->bytes / 4 < n || out_i16->bytes / 2 < n) return sh::set_error(SH_ERR_INVALID, "sh_quantize_clip_f32: buffer too small");
    if (!n) return SH_OK;
    {
        hipStream_t st = sh::state().stream;
        const bool aligned = ((uintptr_t)in_f32->ptr & 15) == 0 && ((uintptr_t)out_i16->ptr & 7) == 0;      // (a ring slot of odd length is not)
        const VecSplit s = vec_split(aligned, n, 4);
        if (s.nvec) hipLaunchKernelGGL(k_quantize_f32_i16_vec, sh::grid1d(s.nvec, 512), dim3(256), 0, st, (const float4v*)in_f32->ptr, s.nvec, scale, (short4v*)out_i16->ptr, sh::state().flag, 1);
        if (s.rest) hipLaunchKernelGGL(k_quantize<short>, sh::grid1d(s.rest, 256), dim3(256), 0, st,
                                       (const float*)in_f32->ptr + s.done, s.rest, scale, -32768.0, 32767.0, (short*)out_i16->ptr + s.done, sh::state().flag, 1);
    }
    SH_CHECK_LAUNCH("k_quantize(clip)");
    return SH_OK;
}

static int pcm_add_dev(const char* a, const char* b, char* o, size_t nbytes, int width) {
    hipStream_t st = sh::state().stream;
    return dispatch_width(width, [&](auto tag) {
        typedef decltype(tag) T;
        typedef typename std::conditional<sizeof(T) == 1, char16v, typename std::conditional<sizeof(T) == 2, short8v, int4v>::type>::type V;
        const T *pa = (const T*)a, *pb = (const T*)b;
        T* po = (T*)o;
        const VecSplit s = vec_split((((uintptr_t)a | (uintptr_t)b | (uintptr_t)o) & 15) == 0, nbytes / sizeof(T), 16 / sizeof(T));
        if (s.nvec && 2 * nbytes > sh::STREAM_BYTES) hipLaunchKernelGGL((k_add_vec<V, true>), sh::grid1d(s.nvec, 256), dim3(256), 0, st, (const V*)pa, (const V*)pb, (V*)po, s.nvec);
        else if (s.nvec) hipLaunchKernelGGL((k_add_vec<V, false>), sh::grid1d(s.nvec, 256), dim3(256), 0, st, (const V*)pa, (const V*)pb, (V*)po, s.nvec);
        if (s.rest) hipLaunchKernelGGL(k_add_scalar<T>, sh::grid1d(s.rest, 256), dim3(256), 0, st, pa + s.done, pb + s.done, po + s.done, s.rest);
        return launch_result("k_add");
    });
}

int sh_pcm_add(const sh_buf* a, size_t a_off, const sh_buf* b, size_t b_off, size_t nbytes, int width,
               sh_buf* out, size_t out_off) {
    SH_REQUIRE_INIT();
    if (!a || !b || !out) return sh::set_error(SH_ERR_INVALID, "sh_pcm_add: NULL argument");
    if (width == 3) {
        // audioop.add at width 3: int sum clamped to [-2^23, 2^23 - 1] == the 32-bit saturating add of the samples << 8, >> 8
        if (nbytes % 3 || a_off % 3 || b_off % 3 || out_off % 3) return sh::set_error(SH_ERR_INVALID, "sh_pcm_add: not a whole number of frames");   // (each offset: 3 | 6 is no multiple of 3)
        if (a_off > a->bytes || nbytes > a->bytes - a_off || b_off > b->bytes || nbytes > b->bytes - b_off ||
            out_off > out->bytes || nbytes > out->bytes - out_off)
            return sh::set_error(SH_ERR_LENGTH, "sh_pcm_add: range outside buffer (Lengths should be the same)");
        const size_t n = nbytes / 3;
        if (!n) return SH_OK;
        sh::Temp ta, tb;
        int rc = ta.alloc(n * 4);
        if (!rc) rc = tb.alloc(n * 4);
        if (!rc) rc = sh::unpack24((const char*)a->ptr + a_off, n, 8, (int32_t*)ta.buf.ptr);
        if (!rc) rc = sh::unpack24((const char*)b->ptr + b_off, n, 8, (int32_t*)tb.buf.ptr);
        if (!rc) rc = pcm_add_dev((const char*)ta.buf.ptr, (const char*)tb.buf.ptr, (char*)ta.buf.ptr, n * 4, 4);
        if (!rc) rc = sh::pack24((const int32_t*)ta.buf.ptr, n, 8, (char*)out->ptr + out_off);
        return rc;
    }
    if (!valid_width(width)) return bad_width("sh_pcm_add", width);
    if (nbytes % width) return sh::set_error(SH_ERR_INVALID, "sh_pcm_add: not a whole number of frames");
    if (a_off > a->bytes || nbytes > a->bytes - a_off || b_off > b->bytes || nbytes > b->bytes - b_off ||
        out_off > out->bytes || nbytes > out->bytes - out_off)
        return sh::set_error(SH_ERR_LENGTH, "sh_pcm_add: range outside buffer (Lengths should be the same)");
    if ((a_off | b_off | out_off) % width) return sh::set_error(SH_ERR_INVALID, "sh_pcm_add: offsets not sample-aligned");
    if (!nbytes) return SH_OK;
    return pcm_add_dev((const char*)a->ptr + a_off, (const char*)b->ptr + b_off, (char*)out->ptr + out_off, nbytes, width);
}

int sh_pcm_add_host(const void* a, const void* b, size_t nbytes, int width, void* out) {
    SH_REQUIRE_INIT();
    if (width == 3) {                                       // staged in device temporaries, then the device form (24-bit via 32-bit)
        if (nbytes % 3) return sh::set_error(SH_ERR_INVALID, "sh_pcm_add_host: not a whole number of frames");
        if (!nbytes) return SH_OK;
        if (!a || !b || !out) return sh::set_error(SH_ERR_INVALID, "sh_pcm_add_host: NULL argument");
        sh::Temp da, db;
        int rc3 = da.alloc(nbytes);
        if (!rc3) rc3 = db.alloc(nbytes);
        if (rc3) return rc3;
        hipStream_t st3 = sh::state().stream;
        SH_HIP(hipMemcpyAsync(da.buf.ptr, a, nbytes, hipMemcpyHostToDevice, st3));
        SH_HIP(hipMemcpyAsync(db.buf.ptr, b, nbytes, hipMemcpyHostToDevice, st3));
        rc3 = sh_pcm_add(&da.buf, 0, &db.buf, 0, nbytes, 3, &da.buf, 0);
        if (rc3) return rc3;
        SH_HIP(hipMemcpyAsync(out, da.buf.ptr, nbytes, hipMemcpyDeviceToHost, st3));
        SH_HIP(hipStreamSynchronize(st3));
        return SH_OK;
    }
    if (!valid_width(width)) return bad_width("sh_pcm_add_host", width);
    if (nbytes % width) return sh::set_error(SH_ERR_INVALID, "sh_pcm_add_host: not a whole number of frames");
    if (!nbytes) return SH_OK;
    if (!a || !b || !out) return sh::set_error(SH_ERR_INVALID, "sh_pcm_add_host: NULL argument");
    size_t pad = (nbytes + 255) & ~size_t(255);
    int rc = sh::ensure_scratch(3 * pad);
    if (rc) return rc;
    char* s = (char*)sh::state().scratch;
    hipStream_t st = sh::state().stream;
    SH_HIP(hipMemcpyAsync(s, a, nbytes, hipMemcpyHostToDevice, st));
    SH_HIP(hipMemcpyAsync(s + pad, b, nbytes, hipMemcpyHostToDevice, st));
    rc = pcm_add_dev(s, s + pad, s + 2 * pad, nbytes, width);
    if (rc) return rc;
    SH_HIP(hipMemcpyAsync(out, s + 2 * pad, nbytes, hipMemcpyDeviceToHost, st));
    SH_HIP(hipStreamSynchronize(st));
    return SH_OK;
}

// (uniform, host) RowSrc::vec: whether every row of a strided chunk array starts on the grid of the split kernels' vector load.
static uint32_t rows_vec(const void* chunks, size_t stride, bool pan) {
    return (stride & (pan ? 3 : 7)) == 0 && ((uintptr_t)chunks & (pan ? 7 : 15)) == 0;
}

// The checks of the four strided chain entry points: nvoices rows of nframes samples (pan: mono frames, two output values each) at
// stride; out holds an int16 result (unit 2) or a map (unit 8, parts_out) per output value.  1: an empty call, nothing to launch.
static int chain_rows_check(const char* who, const sh_buf* chunks, uint32_t nvoices, size_t stride, uint32_t nframes,
                            const sh_buf* factors_lr, bool pan, const sh_buf* out, size_t unit) {
    if (!chunks || !out || (pan && !factors_lr) || nvoices == 0) return sh::set_error(SH_ERR_INVALID, "%s: NULL argument", who);
    if (nvoices > 32768) return sh::set_error(SH_ERR_INVALID, "%s: at most 32768 voices", who);
    if (!pan && nframes > 0xFFFF0000u) return sh::set_error(SH_ERR_INVALID, "%s: at most 2^32 - 65536 samples per call", who);
    if (pan && nframes > 0x7FFF0000u) return sh::set_error(SH_ERR_INVALID, "%s: at most 2^31 - 65536 frames per call", who);
    if (!nframes) return 1;
    if (stride < nframes || chunks->bytes / 2 < (size_t)(nvoices - 1) * stride + nframes)
        return sh::set_error(SH_ERR_INVALID, "%s: chunk buffer too small", who);
    if (pan && factors_lr->bytes / 16 < nvoices) return sh::set_error(SH_ERR_INVALID, "%s: one (left, right) pair of doubles per voice", who);
    if (pan && ((uintptr_t)factors_lr->ptr & 7)) return sh::set_error(SH_ERR_INVALID, "%s: factors_lr not 8-byte aligned", who);
    const size_t nvalues = (size_t)nframes * (pan ? 2 : 1);
    if (unit == 8 && (out->bytes / 8 < nvalues || ((uintptr_t)out->ptr & 7)))
        return sh::set_error(SH_ERR_INVALID, "%s: parts_out too small or not 8-byte aligned", who);
    if (unit == 2 && out->bytes / 2 < nvalues) return sh::set_error(SH_ERR_INVALID, "%s: output too small", who);
    return SH_OK;
}

int sh_mix_chain_i16(const sh_buf* chunks, uint32_t nvoices, size_t stride, uint32_t nsamples, sh_buf* out) {
    SH_REQUIRE_INIT();
    if (int rc = chain_rows_check("sh_mix_chain_i16", chunks, nvoices, stride, nsamples, nullptr, false, out, 2)) return rc < 0 ? rc : SH_OK;
    hipStream_t st = sh::state().stream;
    // shape by the number of 1 KB columns (= waves when the voices are not split): plenty -> the direct loop
    // (6.4-6.5 TB/s at 1875 columns, where the split kernel's waves of one workgroup fetch the same column of eight
    // distant rows: 5.8); fewer -> split the voices over the waves of a workgroup for parallelism
    const uint32_t columns = (uint32_t)sh::div_up(nsamples, 512);
    const bool aligned = (stride & 7) == 0 && ((uintptr_t)chunks->ptr & 15) == 0 && ((uintptr_t)out->ptr & 15) == 0;
    const bool stream = (size_t)nvoices * nsamples * 2 > sh::STREAM_BYTES;           // rows beyond the Infinity Cache: streaming loads
    // (the split kernel keeps plain loads: 1024 x 96 000 samples = 197 MB ran 13 % slower with streaming ones)
#define SH_CHAIN(W_, C_) hipLaunchKernelGGL((k_mix_chain_i16<W_, C_, false>), sh::grid1d(nsamples, 512 * C_), dim3(W_ * 64), 0, st, \
                                            (const short*)chunks->ptr, nvoices, stride, nsamples, (short*)out->ptr, rows_vec(chunks->ptr, stride, false))
#define SH_DIRECT_S(S_, W_, INF_, NTS_) do { \
        if (stream) hipLaunchKernelGGL((k_mix_chain_direct_s<S_, W_, INF_, true, NTS_>), sh::grid1d(nsamples, W_ * 64 * S_), dim3(W_ * 64), 0, st, (const short*)chunks->ptr, nvoices, stride, nsamples, (short*)out->ptr); \
        else hipLaunchKernelGGL((k_mix_chain_direct_s<S_, W_, INF_, false, NTS_>), sh::grid1d(nsamples, W_ * 64 * S_), dim3(W_ * 64), 0, st, (const short*)chunks->ptr, nvoices, stride, nsamples, (short*)out->ptr); } while (0)
    if (columns >= 640 && columns < 1536 && aligned) SH_DIRECT_S(4, 4, 8, true);      // (measured at 937 columns; 187 columns: the split kernel, 31 against 86 us)
    else if (columns >= 1536 && aligned) SH_DIRECT_S(8, 8, 4, false);
#undef SH_DIRECT_S
    else if (nvoices < 64) SH_CHAIN(2, 1);
    else if (columns >= 512) SH_CHAIN(8, 2);
    else SH_CHAIN(8, 1);
#undef SH_CHAIN
    SH_CHECK_LAUNCH("k_mix_chain_i16");
    return SH_OK;
}

int sh_mix_chain_pan_i16(const sh_buf* chunks, uint32_t nvoices, size_t stride, uint32_t nframes, const sh_buf* factors_lr, sh_buf* out) {
    SH_REQUIRE_INIT();
    if (int rc = chain_rows_check("sh_mix_chain_pan_i16", chunks, nvoices, stride, nframes, factors_lr, true, out, 2)) return rc < 0 ? rc : SH_OK;
    hipStream_t st = sh::state().stream;
    const short* in = (const short*)chunks->ptr;
    const double2* fac = (const double2*)factors_lr->ptr;
    const uint32_t nsamples = 2 * nframes;
    const uint32_t columns = (uint32_t)sh::div_up(nframes, 512);                      // 1 KB of a mono row
    const bool aligned = (stride & 7) == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out->ptr & 15) == 0 && ((uintptr_t)fac & 15) == 0;
    const bool stream = (size_t)nvoices * nframes * 2 > sh::STREAM_BYTES;
    if (columns >= 640 && aligned) {
        if (stream) hipLaunchKernelGGL((k_mix_chain_pan_direct_s<4, 4, 8, true>), sh::grid1d(nframes, 256 * 4), dim3(256), 0, st, in, nvoices, stride, nframes, fac, (short*)out->ptr);
        else hipLaunchKernelGGL((k_mix_chain_pan_direct_s<4, 4, 8, false>), sh::grid1d(nframes, 256 * 4), dim3(256), 0, st, in, nvoices, stride, nframes, fac, (short*)out->ptr);
    } else if (nvoices < 64) {
        hipLaunchKernelGGL((k_mix_chain_i16<2, 1, false>), sh::grid1d(nsamples, 512), dim3(128), 0, st, in, nvoices, stride, nsamples, (short*)out->ptr, rows_vec(in, stride, true), fac);
    } else {
        hipLaunchKernelGGL((k_mix_chain_i16<8, 1, false>), sh::grid1d(nsamples, 512), dim3(512), 0, st, in, nvoices, stride, nsamples, (short*)out->ptr, rows_vec(in, stride, true), fac);
    }
    SH_CHECK_LAUNCH("k_mix_chain_pan");
    return SH_OK;
}

// ---- chain maps (include/synthhip.h, sh_chain_map) ---------------------------------------------------------------------------
int sh_mix_chain_i16_parts(const sh_buf* chunks, uint32_t nvoices, size_t stride, uint32_t nsamples, sh_buf* parts_out) {
    SH_REQUIRE_INIT();
    if (int rc = chain_rows_check("sh_mix_chain_i16_parts", chunks, nvoices, stride, nsamples, nullptr, false, parts_out, 8)) return rc < 0 ? rc : SH_OK;
    hipStream_t st = sh::state().stream;
    const short* in = (const short*)chunks->ptr;
    int2v* maps = (int2v*)parts_out->ptr;
    // the split kernel throughout (the direct loops keep no map); long rows: one voice range per wave, eight columns per workgroup
    const uint32_t columns = (uint32_t)sh::div_up(nsamples, 512);
#define SH_CHAIN_PARTS(W_, C_) hipLaunchKernelGGL((k_mix_chain_i16<W_, C_, false, true>), sh::grid1d(nsamples, 512 * C_), dim3(W_ * 64), 0, st, \
                                                  in, nvoices, stride, nsamples, (short*)nullptr, rows_vec(in, stride, false), (const double2*)nullptr, maps)
    if (nvoices < 64) SH_CHAIN_PARTS(2, 1);
    else if (columns >= 1536) SH_CHAIN_PARTS(8, 8);
    else if (columns >= 512) SH_CHAIN_PARTS(8, 2);
    else SH_CHAIN_PARTS(8, 1);
#undef SH_CHAIN_PARTS
    SH_CHECK_LAUNCH("k_mix_chain_i16(parts)");
    return SH_OK;
}

int sh_mix_chain_pan_i16_parts(const sh_buf* chunks, uint32_t nvoices, size_t stride, uint32_t nframes, const sh_buf* factors_lr,
                               sh_buf* parts_out) {
    SH_REQUIRE_INIT();
    if (int rc = chain_rows_check("sh_mix_chain_pan_i16_parts", chunks, nvoices, stride, nframes, factors_lr, true, parts_out, 8)) return rc < 0 ? rc : SH_OK;
    hipStream_t st = sh::state().stream;
    const short* in = (const short*)chunks->ptr;
    const double2* fac = (const double2*)factors_lr->ptr;
    const uint32_t nsamples = 2 * nframes;
    int2v* maps = (int2v*)parts_out->ptr;
    if (nvoices < 64) hipLaunchKernelGGL((k_mix_chain_i16<2, 1, false, true>), sh::grid1d(nsamples, 512), dim3(128), 0, st, in, nvoices, stride, nsamples, (short*)nullptr, rows_vec(in, stride, true), fac, maps);
    else hipLaunchKernelGGL((k_mix_chain_i16<8, 1, false, true>), sh::grid1d(nsamples, 512), dim3(512), 0, st, in, nvoices, stride, nsamples, (short*)nullptr, rows_vec(in, stride, true), fac, maps);
    SH_CHECK_LAUNCH("k_mix_chain_pan(parts)");
    return SH_OK;
}

static int chain_parts_check(const char* who, const sh_buf* parts, uint32_t nparts, size_t part_stride, uint32_t nvalues) {
    if (nparts == 0) return SH_OK;
    if (!parts) return sh::set_error(SH_ERR_INVALID, "%s: NULL parts", who);
    if (nparts > 1 && (part_stride < nvalues || part_stride == 0)) return sh::set_error(SH_ERR_INVALID, "%s: part_stride < nvalues", who);
    const size_t cap = parts->bytes / 8;
    if (cap < nvalues || (nparts > 1 && (size_t)(nparts - 1) > (cap - nvalues) / part_stride))
        return sh::set_error(SH_ERR_INVALID, "%s: parts buffer too small", who);
    if ((uintptr_t)parts->ptr & 7) return sh::set_error(SH_ERR_INVALID, "%s: parts not 8-byte aligned", who);
    return SH_OK;
}

int sh_chain_parts_compose(const sh_buf* parts, uint32_t nparts, size_t part_stride, uint32_t nvalues, sh_buf* out_parts) {
    SH_REQUIRE_INIT();
    if (!out_parts) return sh::set_error(SH_ERR_INVALID, "sh_chain_parts_compose: NULL argument");
    if (nvalues > 0xFFFF0000u) return sh::set_error(SH_ERR_INVALID, "sh_chain_parts_compose: at most 2^32 - 65536 values per call");
    int rc = chain_parts_check("sh_chain_parts_compose", parts, nparts, part_stride, nvalues);
    if (rc) return rc;
    if (out_parts->bytes / 8 < nvalues || ((uintptr_t)out_parts->ptr & 7))
        return sh::set_error(SH_ERR_INVALID, "sh_chain_parts_compose: out_parts too small or not 8-byte aligned");
    if (!nvalues) return SH_OK;
    hipLaunchKernelGGL(k_chain_parts<false>, sh::grid1d(nvalues, 256), dim3(256), 0, sh::state().stream,
                       nparts ? (const int2v*)parts->ptr : (const int2v*)nullptr, nparts, part_stride, nvalues, (const short*)nullptr,
                       (int2v*)out_parts->ptr, (short*)nullptr);
    SH_CHECK_LAUNCH("k_chain_parts(compose)");
    return SH_OK;
}

int sh_chain_parts_apply(const sh_buf* parts, uint32_t nparts, size_t part_stride, uint32_t nvalues, const sh_buf* x0_i16,
                         sh_buf* out_i16) {
    SH_REQUIRE_INIT();
    if (!out_i16) return sh::set_error(SH_ERR_INVALID, "sh_chain_parts_apply: NULL argument");
    if (nvalues > 0xFFFF0000u) return sh::set_error(SH_ERR_INVALID, "sh_chain_parts_apply: at most 2^32 - 65536 values per call");
    int rc = chain_parts_check("sh_chain_parts_apply", parts, nparts, part_stride, nvalues);
    if (rc) return rc;
    if (x0_i16 && x0_i16->bytes / 2 < nvalues) return sh::set_error(SH_ERR_INVALID, "sh_chain_parts_apply: x0 too small");
    if (out_i16->bytes / 2 < nvalues) return sh::set_error(SH_ERR_INVALID, "sh_chain_parts_apply: output too small");
    if (!nvalues) return SH_OK;
    hipLaunchKernelGGL(k_chain_parts<true>, sh::grid1d(nvalues, 256), dim3(256), 0, sh::state().stream,
                       nparts ? (const int2v*)parts->ptr : (const int2v*)nullptr, nparts, part_stride, nvalues,
                       x0_i16 ? (const short*)x0_i16->ptr : (const short*)nullptr, (int2v*)nullptr, (short*)out_i16->ptr);
    SH_CHECK_LAUNCH("k_chain_parts(apply)");
    return SH_OK;
}

}  // extern "C"

namespace {
// Where a gather fold runs: the library's stream with its grow-only scratch (the table of a turn with more than 64 sources), or a
// real-time lane's stream with the lane's own table buffer (sh_rt: below).
struct GatherLane {
    hipStream_t st;
    void*       tab_dev;          // NULL: the library's scratch (sh::ensure_scratch)
    size_t      tab_cap;
};
int lane_table(const GatherLane& L, const void* host, size_t bytes, const void** dev) {
    if (!L.tab_dev) {
        int rc = sh::ensure_scratch(bytes);
        if (rc) return rc;
        *dev = sh::state().scratch;
    } else {
        if (bytes > L.tab_cap) return sh::set_error(SH_ERR_INVALID, "real-time lane: %zu sources, the lane was created for %zu", bytes / 16, L.tab_cap / 16);
        *dev = L.tab_dev;
    }
    // the table goes through the stream (pageable source: staged before the call returns, ordered after earlier kernels)
    SH_HIP(hipMemcpyAsync(const_cast<void*>(*dev), host, bytes, hipMemcpyHostToDevice, L.st));
    return SH_OK;
}

int gather_i16_on(const GatherLane& L, const sh_buf* const* srcs, const size_t* sample_offsets, const uint32_t* nsamples_each, uint32_t nsrc,
                  uint32_t nsamples, short* op) {
    std::vector<ChainSrc> tab;
    tab.reserve(nsrc);
    for (uint32_t v = 0; v < nsrc; ++v) {
        if (!nsamples_each[v]) continue;                  // silence: the fold's identity
        if (!srcs[v] || sample_offsets[v] > srcs[v]->bytes / 2 || nsamples_each[v] > srcs[v]->bytes / 2 - sample_offsets[v])
            return sh::set_error(SH_ERR_INVALID, "sh_mix_chain_gather_i16: source %u range outside its buffer", v);
        ChainSrc c;
        c.p = (const short*)srcs[v]->ptr + sample_offsets[v];
        c.n = nsamples_each[v] < nsamples ? nsamples_each[v] : nsamples;
        c.pad = 0;
        tab.push_back(c);
    }
    hipStream_t st = L.st;
    if (tab.empty()) {
        SH_HIP(hipMemsetAsync(op, 0, (size_t)nsamples * 2, st));
        return SH_OK;
    }
    if (tab.size() <= 64 && sh::div_up(nsamples, 512) < 1536) {          // a mixer turn: the table travels in the kernel arguments
        ChainTab args;
        for (size_t k = 0; k < 64; ++k) args.e[k] = k < tab.size() ? tab[k] : ChainSrc{nullptr, 0, 0};
        const uint32_t n = (uint32_t)tab.size();
        dim3 grid(sh::div_up(nsamples, 512));
        if (n >= 64) hipLaunchKernelGGL(k_mix_chain_gather_args<8>, grid, dim3(8 * 64), 0, st, args, n, nsamples, op);
        else hipLaunchKernelGGL(k_mix_chain_gather_args<2>, grid, dim3(2 * 64), 0, st, args, n, nsamples, op);
        SH_CHECK_LAUNCH("k_mix_chain_gather_args");
        return SH_OK;
    }
    const void* dtab = nullptr;
    int rc = lane_table(L, tab.data(), tab.size() * sizeof(ChainSrc), &dtab);
    if (rc) return rc;
    const uint32_t n = (uint32_t)tab.size();
    dim3 grid(sh::div_up(nsamples, 512));
    size_t read_bytes = 0;
    for (const ChainSrc& c : tab) read_bytes += (size_t)c.n * 2;
    if (sh::div_up(nsamples, 512) >= 1536 && read_bytes > sh::STREAM_BYTES)
        hipLaunchKernelGGL((k_mix_chain_gather_direct<8, 4, true>), sh::grid1d(nsamples, 512 * 8), dim3(8 * 64), 0, st, (const ChainSrc*)dtab, n, nsamples, op);
    else if (sh::div_up(nsamples, 512) >= 1536)
        hipLaunchKernelGGL((k_mix_chain_gather_direct<8, 4, false>), sh::grid1d(nsamples, 512 * 8), dim3(8 * 64), 0, st, (const ChainSrc*)dtab, n, nsamples, op);
    else if (n >= 64) hipLaunchKernelGGL(k_mix_chain_gather<8>, grid, dim3(8 * 64), 0, st, (const ChainSrc*)dtab, n, nsamples, op);
    else hipLaunchKernelGGL(k_mix_chain_gather<2>, grid, dim3(2 * 64), 0, st, (const ChainSrc*)dtab, n, nsamples, op);
    SH_CHECK_LAUNCH("k_mix_chain_gather");
    return SH_OK;
}

// widths 1, 3, 4
int gather_w_on(const GatherLane& L, const sh_buf* const* srcs, const size_t* sample_offsets, const uint32_t* nsamples_each, uint32_t nsrc,
                uint32_t nsamples, int width, unsigned char* op) {
    const size_t w = (size_t)width;
    std::vector<ChainSrcB> tab;
    tab.reserve(nsrc);
    for (uint32_t v = 0; v < nsrc; ++v) {
        if (!nsamples_each[v]) continue;                  // silence: the fold's identity
        if (!srcs[v] || sample_offsets[v] > srcs[v]->bytes / w || nsamples_each[v] > srcs[v]->bytes / w - sample_offsets[v])
            return sh::set_error(SH_ERR_INVALID, "sh_mix_chain_gather: source %u range outside its buffer", v);
        ChainSrcB c;
        c.p = (const unsigned char*)srcs[v]->ptr + sample_offsets[v] * w;
        c.n = nsamples_each[v] < nsamples ? nsamples_each[v] : nsamples;
        c.pad = 0;
        tab.push_back(c);
    }
    hipStream_t st = L.st;
    if (tab.empty()) {
        SH_HIP(hipMemsetAsync(op, 0, (size_t)nsamples * w, st));
        return SH_OK;
    }
    const void* dtab = nullptr;
    int rc = lane_table(L, tab.data(), tab.size() * sizeof(ChainSrcB), &dtab);
    if (rc) return rc;
    const uint32_t n = (uint32_t)tab.size();
    const dim3 grid = sh::grid1d(nsamples, 1024);
    const ChainSrcB* dt = (const ChainSrcB*)dtab;
    if (width == 1) hipLaunchKernelGGL(k_mix_chain_gather_w<1>, grid, dim3(256), 0, st, dt, n, nsamples, op);
    else if (width == 3) hipLaunchKernelGGL(k_mix_chain_gather_w<3>, grid, dim3(256), 0, st, dt, n, nsamples, op);
    else hipLaunchKernelGGL(k_mix_chain_gather_w<4>, grid, dim3(256), 0, st, dt, n, nsamples, op);
    SH_CHECK_LAUNCH("k_mix_chain_gather_w");
    return SH_OK;
}
}  // namespace

// ---- the real-time lane (include/synthhip.h: sh_rt_*) -----------------------------------------------------------------------------
// The reference drives its mixer from a thread of its own (playback.py: the output thread pulls chunks) while other threads make
// sound.  Through the library's one lock and one stream pair that thread's turn queues behind whatever the others have enqueued and
// its download holds the lock while the stream drains.  A lane is a stream (high priority), a lock, a table buffer and a chunk
// buffer of its own: a turn -- the gather fold + the chunk back to the host -- takes the LANE's lock only and waits for the lane's
// stream only.  Order against the library's streams is established once per source, by sh_rt_acquire.
struct sh_rt {
    hipStream_t stream = nullptr;
    hipEvent_t  ev1 = nullptr, ev2 = nullptr;
    std::mutex  mu;
    void*       tab_dev = nullptr;
    size_t      tab_cap = 0;
    void*       out_dev = nullptr;
    void*       out_pinned = nullptr;
    size_t      out_cap = 0;
};

extern "C" {

int sh_rt_create(size_t max_chunk_bytes, uint32_t max_sources, sh_rt** out) {
    SH_REQUIRE_INIT();
    if (!out || max_chunk_bytes == 0) return sh::set_error(SH_ERR_INVALID, "sh_rt_create: NULL / empty argument");
    sh_rt* r = new (std::nothrow) sh_rt;
    if (!r) return sh::set_error(SH_ERR_NOMEM, "host allocation failed");
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);                      // (hi: the numerically lowest = most urgent)
    hipError_t e;
    const int rt_cus = sh::knobs().rt_cus;
    if (rt_cus > 0) {                                                     // the compute units the library's streams leave out (SYNTHHIP_RT_CUS)
        hipDeviceProp_t prop;
        e = hipGetDeviceProperties(&prop, sh::state().device);
        const int ncu = e == hipSuccess ? prop.multiProcessorCount : 0;
        std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
        for (int c = ncu - rt_cus; c >= 0 && c < ncu; ++c) mask[(size_t)c / 32] |= 1u << (c % 32);
        if (e == hipSuccess) e = hipExtStreamCreateWithCUMask(&r->stream, (uint32_t)mask.size(), mask.data());
    } else {
        e = hipStreamCreateWithPriority(&r->stream, hipStreamNonBlocking, hi);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->ev1, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->ev2, hipEventDisableTiming);
    r->tab_cap = (size_t)(max_sources < 64 ? 64 : max_sources) * 16;
    r->out_cap = (max_chunk_bytes + 255) & ~(size_t)255;
    if (e == hipSuccess) e = hipMalloc(&r->tab_dev, r->tab_cap);
    if (e == hipSuccess) e = hipMalloc(&r->out_dev, r->out_cap);
    if (e == hipSuccess) e = hipHostMalloc(&r->out_pinned, r->out_cap, hipHostMallocDefault);
    if (e != hipSuccess) {
        sh_rt_destroy(r);
        return sh::hip_error(e, "sh_rt_create");
    }
    *out = r;
    return SH_OK;
}

int sh_rt_destroy(sh_rt* r) {
    if (!r) return SH_OK;
    if (r->stream) (void)hipStreamSynchronize(r->stream);
    if (r->out_pinned) (void)hipHostFree(r->out_pinned);
    if (r->out_dev) (void)hipFree(r->out_dev);
    if (r->tab_dev) (void)hipFree(r->tab_dev);
    if (r->ev1) (void)hipEventDestroy(r->ev1);
    if (r->ev2) (void)hipEventDestroy(r->ev2);
    if (r->stream) (void)hipStreamDestroy(r->stream);
    delete r;
    return SH_OK;
}

int sh_rt_acquire(sh_rt* r, const sh_buf* src) {
    SH_API_LOCK();                                            // (the library's lock: this call looks at the library's streams)
    if (!sh::state().initialized) return sh::set_error(SH_ERR_NOTINIT, "sh_init() has not been called");
    if (!r || !src) return sh::set_error(SH_ERR_INVALID, "sh_rt_acquire: NULL argument");
    int rc = sh::bind_thread_to_device();
    if (rc) return rc;
    if (sh::fold_owed_into(src->ptr, src->bytes)) {           // a render still owes a fold into this memory: done now
        rc = sh::flush_pending();
        if (rc) return rc;
    }
    // whatever either of the library's streams has been given so far precedes the lane's next turn (events: nobody waits on the host)
    sh::State& S = sh::state();
    SH_HIP(hipEventRecord(r->ev1, S.stream));
    SH_HIP(hipStreamWaitEvent(r->stream, r->ev1, 0));
    if (S.stream2) {
        SH_HIP(hipEventRecord(r->ev2, S.stream2));
        SH_HIP(hipStreamWaitEvent(r->stream, r->ev2, 0));
    }
    return SH_OK;
}

int sh_rt_mix_turn(sh_rt* r, const sh_buf* const* srcs, const size_t* sample_offsets, const uint32_t* nsamples_each, uint32_t nsrc,
                   uint32_t nsamples, int width, void* out_host) {
    if (!r || !out_host || (nsrc && (!srcs || !sample_offsets || !nsamples_each))) return sh::set_error(SH_ERR_INVALID, "sh_rt_mix_turn: NULL argument");
    if (width < 1 || width > 4) return sh::set_error(SH_ERR_INVALID, "sh_rt_mix_turn: width %d not in {1, 2, 3, 4}", width);
    if (nsrc > 32768) return sh::set_error(SH_ERR_INVALID, "sh_rt_mix_turn: at most 32768 sources");
    const size_t nbytes = (size_t)nsamples * (size_t)width;
    if (nbytes > r->out_cap) return sh::set_error(SH_ERR_INVALID, "sh_rt_mix_turn: %zu bytes, the lane was created for chunks of %zu", nbytes, r->out_cap);
    if (!nsamples) return SH_OK;
    std::lock_guard<std::mutex> lane_lock(r->mu);             // the LANE's lock: the library's is not taken
    if (!sh::state().initialized) return sh::set_error(SH_ERR_NOTINIT, "sh_init() has not been called");
    int rc = sh::bind_thread_to_device();
    if (rc) return rc;
    const GatherLane L{r->stream, r->tab_dev, r->tab_cap};
    rc = width == 2 ? gather_i16_on(L, srcs, sample_offsets, nsamples_each, nsrc, nsamples, (short*)r->out_dev)
                    : gather_w_on(L, srcs, sample_offsets, nsamples_each, nsrc, nsamples, width, (unsigned char*)r->out_dev);
    if (rc) return rc;
    SH_HIP(hipMemcpyAsync(r->out_pinned, r->out_dev, nbytes, hipMemcpyDeviceToHost, r->stream));
    SH_HIP(hipStreamSynchronize(r->stream));
    memcpy(out_host, r->out_pinned, nbytes);
    return SH_OK;
}

int sh_mix_chain_gather_i16(const sh_buf* const* srcs, const size_t* sample_offsets, const uint32_t* nsamples_each, uint32_t nsrc,
                            uint32_t nsamples, sh_buf* out, size_t out_sample_off) {
    SH_REQUIRE_INIT();
    if (!out || (nsrc && (!srcs || !sample_offsets || !nsamples_each))) return sh::set_error(SH_ERR_INVALID, "sh_mix_chain_gather_i16: NULL argument");
    if (nsrc > 32768) return sh::set_error(SH_ERR_INVALID, "sh_mix_chain_gather_i16: at most 32768 sources");
    if (nsamples > 0xFFFF0000u) return sh::set_error(SH_ERR_INVALID, "sh_mix_chain_gather_i16: at most 2^32 - 65536 samples per call");
    if (out_sample_off > out->bytes / 2 || nsamples > out->bytes / 2 - out_sample_off)
        return sh::set_error(SH_ERR_INVALID, "sh_mix_chain_gather_i16: output range outside buffer");
    if (!nsamples) return SH_OK;
    return gather_i16_on(GatherLane{sh::state().stream, nullptr, 0}, srcs, sample_offsets, nsamples_each, nsrc, nsamples, (short*)out->ptr + out_sample_off);
}

int sh_mix_chain_gather(const sh_buf* const* srcs, const size_t* sample_offsets, const uint32_t* nsamples_each, uint32_t nsrc,
                        uint32_t nsamples, int width, sh_buf* out, size_t out_sample_off) {
    if (width == 2) return sh_mix_chain_gather_i16(srcs, sample_offsets, nsamples_each, nsrc, nsamples, out, out_sample_off);
    SH_REQUIRE_INIT();
    if (width != 1 && width != 3 && width != 4) return sh::set_error(SH_ERR_INVALID, "sh_mix_chain_gather: width %d not in {1, 2, 3, 4}", width);
    if (!out || (nsrc && (!srcs || !sample_offsets || !nsamples_each))) return sh::set_error(SH_ERR_INVALID, "sh_mix_chain_gather: NULL argument");
    if (nsrc > 32768) return sh::set_error(SH_ERR_INVALID, "sh_mix_chain_gather: at most 32768 sources");
    if (nsamples > 0xFFFF0000u) return sh::set_error(SH_ERR_INVALID, "sh_mix_chain_gather: at most 2^32 - 65536 samples per call");
    const size_t w = (size_t)width;
    if (out_sample_off > out->bytes / w || nsamples > out->bytes / w - out_sample_off)
        return sh::set_error(SH_ERR_INVALID, "sh_mix_chain_gather: output range outside buffer");
    if (!nsamples) return SH_OK;
    return gather_w_on(GatherLane{sh::state().stream, nullptr, 0}, srcs, sample_offsets, nsamples_each, nsrc, nsamples, width,
                       (unsigned char*)out->ptr + out_sample_off * w);
}

int sh_mix_chain(const sh_buf* chunks, uint32_t nvoices, size_t stride, uint32_t nsamples, int width, sh_buf* out) {
    if (width == 2) return sh_mix_chain_i16(chunks, nvoices, stride, nsamples, out);
    if (!chunks || !out || nvoices == 0) return sh::set_error(SH_ERR_INVALID, "sh_mix_chain: NULL argument");
    if (nvoices > 32768) return sh::set_error(SH_ERR_INVALID, "sh_mix_chain: at most 32768 voices");
    if (width != 1 && width != 3 && width != 4) return sh::set_error(SH_ERR_INVALID, "sh_mix_chain: width %d not in {1, 2, 3, 4}", width);
    if (stride < nsamples || chunks->bytes / (size_t)width < (size_t)(nvoices - 1) * stride + nsamples)
        return sh::set_error(SH_ERR_INVALID, "sh_mix_chain: chunk buffer too small");
    std::vector<const sh_buf*> srcs(nvoices, chunks);
    std::vector<size_t> offs(nvoices);
    std::vector<uint32_t> lens(nvoices, nsamples);
    for (uint32_t v = 0; v < nvoices; ++v) offs[v] = (size_t)v * stride;
    return sh_mix_chain_gather(srcs.data(), offs.data(), lens.data(), nvoices, nsamples, width, out, 0);
}

}  // extern "C"
