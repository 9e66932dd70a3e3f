// chain.hpp -- the int16 mixer chain as maps: the one statement of its arithmetic.
//
// Upstream mixes int16 voices with mixed = audioop.add(mixed, voice, 2), in voice order.  For one int16 value the chain over a range
// of voices is the map x -> clamp(x + add, lo, hi); maps of consecutive ranges compose in order, and the chain over a table is its
// ranges' maps composed and applied to 0.  Stored form (include/synthhip.h, sh_chain_map): .x = add, .y = lo | hi << 16.
//
// Two rules make and read maps, and they stay two operations:
//   RANGE   makes maps from int16 samples (ChainFold, the split kernels' cross-wave combine, the planes of the fused fold,
//           k_mixdown_compose): add is the exact int32 sum (at most 32 768 voices of |s| <= 32 768), saturated at +-SH_CHAIN_ADD_MAX
//           once, when the map is stored;
//   STORED  reads maps that are already stored (k_chain_parts, synthesizer_amd/chainmaps.py): add saturates on the way in and at
//           every step.
// On int16 inputs both give the same function, but not the same add bytes: add 200 000 then -100 000 stores 100 000 by the range
// rule, 31 072 by the stored-map rule.
//
// The scalar part is __host__ __device__ (tests/test_chain_maps.py builds it with g++); the rest is device code.
#pragma once
#include <stdint.h>
#include "../../include/synthhip.h"

#ifndef SH_HD
#if defined(__HIPCC__)
#define SH_HD __host__ __device__ __forceinline__
#else
#define SH_HD static inline
#endif
#endif

namespace shc {

struct Map { int add, lo, hi; };
enum Rule { RANGE, STORED };

SH_HD int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }
SH_HD int add_sat(int a) { return clampi(a, -SH_CHAIN_ADD_MAX, SH_CHAIN_ADD_MAX); }

// the map of no voices (on int16 inputs)
SH_HD Map identity() { return Map{0, -32768, 32767}; }

// the stored form: add saturated (for |add| >= 65535 every int16 input already lands on a bound, so the map is unchanged on int16
// inputs and sums of two stored adds fit int32), and the bounds as two int16
SH_HD int packed_add(Map m) { return add_sat(m.add); }
SH_HD uint32_t packed_bounds(Map m) { return (uint32_t)(uint16_t)m.lo | ((uint32_t)(uint16_t)m.hi << 16); }
template <Rule R>
SH_HD Map unpack(int add, uint32_t bounds) {
    return Map{R == STORED ? add_sat(add) : add, (int)(int16_t)(uint16_t)(bounds & 0xFFFFu), (int)(int16_t)(uint16_t)(bounds >> 16)};
}

// f, then g -- (f.add + g.add, clamp(f.lo + g.add, g.lo, g.hi), clamp(f.hi + g.add, g.lo, g.hi)); f and g unpacked by the same rule
template <Rule R>
SH_HD Map compose(Map f, Map g) {
    const int a = f.add + g.add;
    return Map{R == STORED ? add_sat(a) : a, clampi(f.lo + g.add, g.lo, g.hi), clampi(f.hi + g.add, g.lo, g.hi)};
}

SH_HD int apply(Map m, int x) { return clampi(x + m.add, m.lo, m.hi); }

}  // namespace shc

#if defined(__HIPCC__)
typedef short short2v __attribute__((ext_vector_type(2)));
typedef short short4v __attribute__((ext_vector_type(4)));
typedef short short8v __attribute__((ext_vector_type(8)));
typedef int   int2v   __attribute__((ext_vector_type(2)));

template <int S> struct ShortVec;
template <> struct ShortVec<8> { typedef short8v type; };
template <> struct ShortVec<4> { typedef short4v type; };
template <> struct ShortVec<2> { typedef short2v type; };

namespace shc {

__device__ __forceinline__ int2v store(Map m) { return (int2v){packed_add(m), (int)packed_bounds(m)}; }
template <Rule R>
__device__ __forceinline__ Map load(int2v v) { return unpack<R>(v.x, (uint32_t)v.y); }

// Planes of maps, plane k at p[k * plane], folded in order per value: composed into one map, or applied to x.  Four planes in flight,
// 8-byte loads (NT: streaming), one value per lane.
template <Rule R, bool NT, typename Step>
__device__ __forceinline__ void for_planes(const int2v* p, uint32_t nplanes, size_t plane, Step step) {
    uint32_t k = 0;
    for (; k + 4 <= nplanes; k += 4) {
        int2v v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = NT ? __builtin_nontemporal_load(p + (size_t)(k + u) * plane) : p[(size_t)(k + u) * plane];
#pragma unroll
        for (int u = 0; u < 4; ++u) step(load<R>(v[u]));
    }
    for (; k < nplanes; ++k) step(load<R>(p[(size_t)k * plane]));
}
template <Rule R, bool NT>
__device__ __forceinline__ Map compose_planes(const int2v* p, uint32_t nplanes, size_t plane) {
    Map m = identity();
    for_planes<R, NT>(p, nplanes, plane, [&](const Map g) { m = compose<R>(m, g); });
    return m;
}
template <Rule R, bool NT>
__device__ __forceinline__ int apply_planes(const int2v* p, uint32_t nplanes, size_t plane, int x) {
    for_planes<R, NT>(p, nplanes, plane, [&](const Map g) { x = apply(g, x); });
    return x;
}

// audioop.tostereo of F mono frames -> 2 F interleaved samples: (fbound(v * lf), fbound(v * rf)) per frame, fbound = clamp to the
// sample range, then floor.  For every finite product fbound(p) == clamp(floor(p), -32768, 32767) (the "val < minval + 1 -> minval"
// branch selects values whose floor is minval anyway), so a frame costs one int -> float64 conversion, two products, two floors, two
// conversions (saturating at the int32 range) and ONE v_cvt_pk_i16_i32, whose saturation is the clamp and whose packed result is the
// (L, R) pair.
__device__ __forceinline__ short2v stereo1(const short m, const double lf, const double rf) {
    const double x = (double)m;
    return __builtin_amdgcn_cvt_pk_i16((int)floor(x * lf), (int)floor(x * rf));
}
template <int F>
__device__ __forceinline__ typename ShortVec<2 * F>::type stereo(const typename ShortVec<F>::type m, const double lf, const double rf) {
    union { typename ShortVec<2 * F>::type v; short2v p[F]; } r;
#pragma unroll
    for (int j = 0; j < F; ++j) r.p[j] = stereo1(m[j], lf, rf);
    return r.v;
}

// The range rule over a range of voices for 8 samples per lane: the sums in int32, the two bounds as packed int16 pairs.  Bounds start
// at the int16 range (the identity), and bound' = clamp(bound + s, -32768, 32767) is exactly the packed saturating add: one instruction
// per two samples; the sum takes one dot-product instruction per sample ((s_lo, s_hi) . (1, 0) + a), no unpacking.
struct ChainFold {
    int a[8];
    short2v L[4], U[4];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { L[q] = (short2v){-32768, -32768}; U[q] = (short2v){32767, 32767}; }
    }
    // first voice of the range: x -> clamp(x + s, -32768, 32767), the bounds as init set them
    __device__ __forceinline__ void first(const short8v x) {
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = x[j];
    }
    __device__ __forceinline__ void add(const short8v x) {
#define SH_PAIR(Q_)                                                                              \
        {                                                                                        \
            const short2v s2 = __builtin_shufflevector(x, x, 2 * Q_, 2 * Q_ + 1);                \
            L[Q_] = __builtin_elementwise_add_sat(L[Q_], s2);                                    \
            U[Q_] = __builtin_elementwise_add_sat(U[Q_], s2);                                    \
            a[2 * Q_] = __builtin_amdgcn_sdot2(s2, (short2v){1, 0}, a[2 * Q_], false);           \
            a[2 * Q_ + 1] = __builtin_amdgcn_sdot2(s2, (short2v){0, 1}, a[2 * Q_ + 1], false);   \
        }
        SH_PAIR(0) SH_PAIR(1) SH_PAIR(2) SH_PAIR(3)
#undef SH_PAIR
    }
};

// The end of a split kernel: WAVES waves = (WAVES / COLS) voice ranges x COLS columns, each wave's ChainFold of its range for the lane's
// 8 samples from s0.  The first range's waves combine the ranges' maps in voice order (LDS) and store the chain's result, or (PARTS)
// its map.
template <int WAVES, int COLS, bool PARTS>
__device__ __forceinline__ void split_store(const ChainFold& f, uint32_t wave, uint32_t lane, uint32_t s0, uint32_t nsamples,
                                            short* __restrict__ out, int2v* __restrict__ maps) {
    constexpr int S = 8, VG = WAVES / COLS;
    __shared__ int red[WAVES][3][S][64];
#pragma unroll
    for (int j = 0; j < S; ++j) {
        red[wave][0][j][lane] = f.a[j];
        red[wave][1][j][lane] = (int)f.L[j >> 1][j & 1];
        red[wave][2][j][lane] = (int)f.U[j >> 1][j & 1];
    }
    __syncthreads();
    const uint32_t col = wave % COLS;
    if (wave / COLS != 0 || s0 >= nsamples) return;
    auto range = [&](int g, int j) { const int w = g * COLS + col; return Map{red[w][0][j][lane], red[w][1][j][lane], red[w][2][j][lane]}; };
    if constexpr (PARTS) {
#pragma unroll
        for (int j = 0; j < S; ++j) {
            Map m = identity();
#pragma unroll
            for (int g = 0; g < VG; ++g) m = compose<RANGE>(m, range(g, j));
            if (s0 + j < nsamples) maps[s0 + j] = store(m);
        }
    } else {
        short8v r;
#pragma unroll
        for (int j = 0; j < S; ++j) {
            int x = 0;
#pragma unroll
            for (int g = 0; g < VG; ++g) x = apply(range(g, j), x);
            r[j] = (short)x;
        }
        if (s0 + S - 1 < nsamples && ((reinterpret_cast<uintptr_t>(out + s0) & 15) == 0)) {
            *reinterpret_cast<short8v*>(out + s0) = r;
        } else {
            for (uint32_t j = 0; j < S && s0 + j < nsamples; ++j) out[s0 + j] = r[j];
        }
    }
}

}  // namespace shc
#endif
