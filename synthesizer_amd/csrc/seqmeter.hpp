// seqmeter.hpp -- the level meters of a song of tracks (sh_seq_render_meters, sequence.hip): per track, post-fader, and for the master, what
// Sample.level_db_peak / level_db_rms read off a finished Sample, taken from the samples a lane of the window kernels already holds.
// A ROW is, per channel, peak = max |x| (audioop.max) and the exact integer sum of x * x, carried as two 64-bit sums
//     sq_lo = sum (x * x & 0xffffffff),  sq_hi = sum (x * x >> 32),  the value sq_hi * 2^32 + sq_lo
// at widths 3 and 4, where x * x reaches 2^46 and 2^62 and a window 2^32 samples: each sum stays below 2^64.  At widths 1 and 2 one sum
// holds it (2^30 * 2^32 < 2^64): sq_lo is the sum and sq_hi stays 0, the value is formed the same way.  Song sample s belongs to channel
// s & 1 of a stereo song and to channel 0 of a mono one, whose second channel reads 0.  |x| is taken in 64 bits: |-2^31| is 2^31.
// Integer max and integer add are associative and commutative, so partial rows fold in any order to the same row: lanes into a wave,
// waves into a workgroup, workgroups into the handle's table, however they arrive.
// Plain C++17 integers, no intrinsics, SH_HD (tests/cpu_seqmeter.cpp builds it with g++).
#pragma once
#include <cstdint>

#ifndef SH_HD
#if defined(__HIPCC__)
#define SH_HD __host__ __device__ __forceinline__
#else
#define SH_HD static inline
#endif
#endif

namespace shmt {

struct Row {                    // sh_seq_meter's layout (synthhip.h), 40 bytes
    uint32_t peak[2];
    uint64_t sq_hi[2];
    uint64_t sq_lo[2];
};
static_assert(sizeof(Row) == 40, "a row is sh_seq_meter");

SH_HD Row zero() { return Row{{0u, 0u}, {0u, 0u}, {0u, 0u}}; }

// |x| of a sample of any width (-2^31 <= x < 2^31), in 64 bits
SH_HD uint32_t magnitude(long long x) { return (uint32_t)(x < 0 ? 0ull - (unsigned long long)x : (unsigned long long)x); }

// x * x (at most 2^62) as the two addends of a row; WIDE: widths 3 and 4
template <bool WIDE>
SH_HD void square(uint32_t mag, uint64_t& hi, uint64_t& lo) {
    const uint64_t sq = (uint64_t)mag * (uint64_t)mag;
    if (WIDE) {
        hi = sq >> 32;
        lo = sq & 0xffffffffull;
    } else {
        hi = 0;
        lo = sq;
    }
}

// one sample into channel c of a row
template <bool WIDE>
SH_HD void add(Row& r, int c, long long x) {
    const uint32_t m = magnitude(x);
    uint64_t hi, lo;
    square<WIDE>(m, hi, lo);
    if (m > r.peak[c]) r.peak[c] = m;
    r.sq_hi[c] += hi;
    r.sq_lo[c] += lo;
}

// A lane's partial row: its N samples x[0 .. N) sit at song samples s0 .. s0 + N, s0 EVEN (a lane starts on a multiple of N), and only
// those inside [lo, hi) count -- a lane on the window's edge holds samples outside it.  The channel of x[j] is j & 1 in a stereo song
// (nch == 2) and 0 otherwise: known where the loop is unrolled, so a row in registers is never indexed by a variable.
template <bool WIDE, int N, typename X>
SH_HD Row lane(const X& x, uint32_t s0, uint32_t lo, uint32_t hi, uint32_t nch) {
    Row r = zero();
    const bool stereo = nch == 2;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < N; ++j) {
        const uint64_t s = (uint64_t)s0 + (uint32_t)j;
        if (s < lo || s >= hi) continue;
        if ((j & 1) && stereo) add<WIDE>(r, 1, (long long)x[j]);
        else add<WIDE>(r, 0, (long long)x[j]);
    }
    return r;
}

// two partial rows into one
SH_HD void fold(Row& a, const Row& b) {
    if (b.peak[0] > a.peak[0]) a.peak[0] = b.peak[0];
    if (b.peak[1] > a.peak[1]) a.peak[1] = b.peak[1];
    a.sq_hi[0] += b.sq_hi[0];
    a.sq_hi[1] += b.sq_hi[1];
    a.sq_lo[0] += b.sq_lo[0];
    a.sq_lo[1] += b.sq_lo[1];
}

}  // namespace shmt
