// ratecv.hpp -- audioop.ratecv's index arithmetic, its per-sample arithmetic and the resampler's route plan: the one statement of each.
//
// Rates are gcd-reduced (inr, outr).  Output frame m sits at input position q + r/outr (q = floor(m inr / outr), r = m inr mod outr) and
// interpolates input frames j - 1 and j with weights d and outr - d: j = ceil(m inr / outr) = q + (r != 0), d = (outr - r) mod outr --
// the reference's state machine evaluated in closed form.  Frame m + 1 lies (step_q, step_r) = (inr / outr, inr % outr) further on.
//
// The scalar part is SH_HD (tests/test_ratecv_plan.py builds it with g++); the 128-bit counts and the plan are host code.
#pragma once
#include <stdint.h>
#include <math.h>

#ifndef SH_HD
#if defined(__HIPCC__)
#define SH_HD __host__ __device__ __forceinline__
#else
#define SH_HD static inline
#endif
#endif

namespace shr {

SH_HD uint64_t gcd(uint64_t a, uint64_t b) {
    while (b) {
        const uint64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

struct Rates { uint32_t inr, outr; };
SH_HD Rates reduce(uint64_t inrate, uint64_t outrate) {         // (rates > 0, below 2^31)
    const uint64_t g = gcd(inrate, outrate);
    return Rates{(uint32_t)(inrate / g), (uint32_t)(outrate / g)};
}

// The position q + r/outr of output frame m (inv_outr = 1.0 / outr): below 2^52 one float64 product and a correction step, beyond it
// the 64-bit division.
struct Pos { uint64_t q; uint32_t r; };
SH_HD Pos position(uint64_t m, uint32_t inr, uint32_t outr, double inv_outr) {
    const uint64_t M = m * (uint64_t)inr;
    if (M < (1ull << 52)) {
        uint64_t q = (uint64_t)floor((double)M * inv_outr);
        int64_t r = (int64_t)(M - q * (uint64_t)outr);
        if (r < 0) { q -= 1; r += outr; }
        else if (r >= (int64_t)outr) { q += 1; r -= outr; }
        return Pos{q, (uint32_t)r};
    }
    return Pos{M / outr, (uint32_t)(M % outr)};
}

// (j, d) of a position: output frame m interpolates input frames j - 1 (weight d) and j (weight outr - d)
SH_HD void index(Pos p, uint32_t outr, uint64_t& j, uint32_t& d) {
    j = p.q + (p.r != 0);
    d = p.r ? outr - p.r : 0u;
}

// One output frame on: r += step_r, q += step_q and the carry.  q may count LDS elements instead of frames (unit = elements per frame).
template <typename Q>
SH_HD void step(Q& q, uint32_t& r, Q step_q, uint32_t step_r, uint32_t outr, Q unit = 1) {
    r += step_r;
    const bool wrap = r >= outr;
    r -= wrap ? outr : 0u;
    q += step_q + (wrap ? unit : (Q)0);
}

// floor(u / outr) for 0 <= u < 2^32 and outr < 65536, as trunc(fma(u, 1/outr, 1/(2 outr))) in float64: (u + 1/2)/outr is at least
// 1/(2 outr) > 2^-17 away from every integer, and the evaluation is off by less than 2^-20 (a quotient below 2^32, 1/outr rounded to
// 53 bits, one rounding of the fma), so the truncation is the floor -- 3 instructions, no correction step.
SH_HD uint32_t floor_by_outr(uint32_t u, double inv_outr) { return (uint32_t)fma((double)u, inv_outr, 0.5 * inv_outr); }

// ---- one output sample (resample.hip's kernels and sequence.hip's resampled events; built with -ffp-contract=off) ---------------------

// (prev*d + cur*(outrate-d)) / outrate in float64, exactly as audioop forms it: two products, one sum, one
// correctly rounded division.  The division is Markstein's sequence q = a*y, r = fma(-q, b, a),
// q' = fma(r, y, q) with y = RN(1/b): it returns the correctly rounded quotient (checked against IEEE
// division on 3e8 operands in tests/ and by every bit-exact parity test), at 3 instructions instead of
// the ~12 of the generic lowering -- k_resample must stay HBM-bound.
SH_HD double value(double prev, double cur, double dd, double od, double outr, double inv_outr) {
    const double a = prev * dd + cur * od;
    const double q = a * inv_outr;
    const double r = fma(-q, outr, a);
    return fma(r, inv_outr, q);
}

// 8/16-bit PCM, reduced outrate < 65536.  audioop computes trunc(fl(N / outr)) >> s with N = (prev*d + cur*(outr-d)) << s
// (s = 32 - bits): N is an exact float64 integer (< 2^48), a non-integer N/outr is at least 1/outr > 2^-16 away
// from an integer while its float64 rounding error is below 2^-21, so the truncation equals integer division, and
// trunc(.) >> s == floor(M / outr) with M = prev*d + cur*(outr-d) (|M| <= 2^(bits-1)*outr < 2^31; for M < 0 the
// inner truncation loses less than 2^-s < 1/outr, which the floor of the arithmetic shift restores).  floor(M/outr)
// is formed as an unsigned division of u = M + 2^(bits-1)*outr (0 <= u < 2^32): floor_by_outr.  Bit-exactness against
// audioop is what tests/test_gpu_pcm.py (both paths) and tests/test_seqrate.py assert.
template <typename T>
SH_HD T small_int(T prev, T cur, uint32_t d, uint32_t outr, double inv_outr) {
    constexpr int HALF = 1 << (8 * (int)sizeof(T) - 1);
    const int M = (int)prev * (int)d + (int)cur * (int)(outr - d);
    const uint32_t u = (uint32_t)M + (uint32_t)HALF * outr;
    return (T)((int)floor_by_outr(u, inv_outr) - HALF);
}

// Integer PCM of any width through the float64 expression: GETSAMPLE32 (the sample in the high bits of 32: shift = 32 - 8 width), the
// value, SETSAMPLE32 (truncation toward zero, then the arithmetic shift back).
SH_HD int shifted_int(int prev, int cur, uint32_t d, uint32_t outr, double inv_outr, int shift) {
    const int ci = (int)((unsigned)cur << shift);
    const int pi = (int)((unsigned)prev << shift);
    return (int)value((double)pi, (double)ci, (double)d, (double)(outr - d), (double)outr, inv_outr) >> shift;
}

// frames per thread of the few-channel kernels: 16-byte stores, at most 8 frames
SH_HD constexpr int frames_per_thread(int frame_bytes) { return 16 / frame_bytes > 8 ? 8 : 16 / frame_bytes; }

// ---- host: counts in 128-bit arithmetic, and the route plan --------------------------------------------------------------------------

// output frames of in_frames input frames: output m exists iff ceil(m inr / outr) <= in_frames - 1
inline uint64_t out_frames(uint64_t in_frames, Rates R) {
    return in_frames ? (uint64_t)((unsigned __int128)(in_frames - 1) * R.outr / R.inr) + 1 : 0;
}

// the input frames [lo, hi] that output frames [m0, m0 + n) read (n >= 1): j(m0) - 1 (clipped at 0) to j(m0 + n - 1)
struct Span { uint64_t lo, hi; };
inline Span reads(uint64_t m0, uint64_t n, Rates R) {
    const auto j = [&](uint64_t m) { return (uint64_t)(((unsigned __int128)m * R.inr + R.outr - 1) / R.outr); };
    const uint64_t lo = j(m0);
    return Span{lo ? lo - 1 : 0, j(m0 + n - 1)};
}

// how a kernel forms one output sample
enum { RS_INT_F64 = 0,          // integer PCM through the float64 expression (any width, any rate)
       RS_FLOAT = 1,            // float32 PCM through the float64 expression
       RS_INT_SMALL = 2 };      // 8/16-bit PCM with reduced outrate < 65536: exact 32-bit integer arithmetic

constexpr uint32_t RS_LDS_BYTES = 48 * 1024;     // LDS budget of the kernels that stage a workgroup's input span

// k_resample_period_i16's launch (resample.hip)
struct PeriodArgs {
    uint64_t c0, c1;             // chunks [c0, c1), absolute: chunk C = output frames [C L, (C + 1) L) = input frames from C kinr on.  The plan
                                 // passes INTERIOR chunks only -- span wholly inside the held input, frames wholly inside the launch's range --
                                 // so the kernel tests nothing; what lies in front of and behind them goes through k_resample_small
    uint32_t L, kinr;            // output / input frames per chunk (K periods); L is a multiple of 8: 16-byte stores
    uint32_t inr, outr;
    uint32_t span_vecs;          // 16-byte vectors staged per chunk
    uint32_t per_wg;             // consecutive chunks per workgroup
    double   inv_outr;
};

enum Route {
    RT_NONE,                     // nothing to write
    RT_GENERIC,                  // k_resample: one thread per output frame x channel vector
    RT_FRAMES,                   // k_resample_frames<..., false>: FR frames per thread, samples gathered from global memory
    RT_LDS,                      // k_resample_frames<..., true>: the same from the workgroup's input span staged in LDS
    RT_SMALL,                    // k_resample_small: 8/16-bit integer arithmetic from the staged span
    RT_PERIOD,                   // k_resample_period_i16 over the interior chunks; head and tail planned again without it
};

// One launch over output frames [m_base, m_end).  T follows from (width, is_float).
struct Plan {
    int route = RT_NONE;
    int vec = 1, fr = 1, groups = 1, mode = RS_INT_F64, nv = 0;     // template arguments (nv: RT_PERIOD)
    uint32_t grid = 0, lds_bytes = 0, span_vecs = 0;
    uint64_t m_base = 0, m_end = 0, n_out = 0;                      // n_out: work units (RatecvArgs::n_out_samples)
    PeriodArgs P{};                                                 // RT_PERIOD
    uint64_t head_end = 0, tail_begin = 0;                          // RT_PERIOD: [m_base, head_end) and [tail_begin, m_end) are left over
};

// The route of a launch: width 1/2/4 (is_float: float32), nch channels, reduced rates, both pointers 16-byte aligned or not, the knobs
// SYNTHHIP_NO_PERIOD / SYNTHHIP_PERIOD_CHUNKS, output frames [m_base, m_end), held input frames [in_lo, in_frames).
inline Plan plan(int width, bool is_float, uint32_t nch, Rates R, bool aligned, bool no_period, int period_chunks,
                 uint64_t m_base, uint64_t m_end, uint64_t in_lo, uint64_t in_frames) {
    Plan p;
    p.m_base = m_base;
    p.m_end = m_end;
    if (m_end <= m_base) return p;
    const uint64_t n = m_end - m_base;
    const bool small = !is_float && width <= 2 && R.outr < 65536u;
    p.mode = is_float ? RS_FLOAT : small ? RS_INT_SMALL : RS_INT_F64;
    const auto blocks = [](uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); };
    if (!aligned || nch * width > 8 || (nch != 1 && nch != 2 && nch != 4)) {
        // one thread per output frame x channel vector: the widest vector that divides nch, stays <= 16 bytes and keeps every access aligned
        if (aligned)
            for (int v = 16 / width; v > 1; v >>= 1)
                if (nch % v == 0) { p.vec = v; break; }
        p.route = RT_GENERIC;
        p.n_out = n * (nch / p.vec);
        p.grid = blocks(p.n_out, 256);
        return p;
    }
    // mono / stereo (and other narrow layouts that fit one vector): several frames per thread, nch == VEC
    p.vec = (int)nch;
    if (small && width == 2 && nch <= 2 && R.inr < 65536u && R.outr <= 2048u && !no_period) {
        // 16-bit mono / stereo between rates with a short period: chunks of whole periods, the weights loop-invariant per thread
        const uint32_t V = nch, fpr = 8u / V, lmax = 512u * fpr;          // a run = 16 bytes; two runs per thread
        const uint32_t s_out = fpr / (uint32_t)gcd(R.outr, fpr);          // L = K outr must be a multiple of a run (16-byte stores)
        uint32_t K = lmax / R.outr;
        const uint32_t k_span = (14336u / V) / R.inr;                     // ... and the chunk's input span at most 28 KB
        if (K > k_span) K = k_span;
        K -= K % s_out;
        const uint32_t L = K * R.outr;
        if (L >= lmax / 4u * 3u) {                                        // (three quarters of the threads' frames in use, at least)
            PeriodArgs& P = p.P;
            P.L = L; P.kinr = K * R.inr; P.inr = R.inr; P.outr = R.outr; P.inv_outr = 1.0 / (double)R.outr;
            const uint32_t off_max = (uint32_t)(((uint64_t)(L - 1) * R.inr) / R.outr);
            P.span_vecs = (7u + (off_max + 2u) * V + 7u) / 8u;
            // the interior chunks: frames wholly inside [m_base, m_end), span wholly inside the held input [in_lo, in_frames)
            uint64_t cA = (m_base + L - 1) / L, cB = m_end / L;
            while (cA < cB && ((cA * P.kinr * V) & ~(uint64_t)7) < in_lo * V) ++cA;
            while (cB > cA && (((cB - 1) * P.kinr * V) & ~(uint64_t)7) + 8ull * P.span_vecs > in_frames * V) --cB;
            if (cB > cA + 1) {
                P.c0 = cA; P.c1 = cB;
                // consecutive chunks per workgroup (profiles/r06_resample_period.txt; SYNTHHIP_PERIOD_CHUNKS overrides).  Mono: two -- one where
                // the input is the larger side (nothing to amortise the set-up against but reads), four where the output is (upsampling by
                // two or more).  Stereo: one (a thread's set-up is eight entries, and the longer a workgroup stays the more of them march in step).
                P.per_wg = period_chunks > 0 ? (uint32_t)period_chunks : nch == 2 || R.inr >= 2 * R.outr ? 1u : R.outr >= 2 * R.inr ? 4u : 2u;
                p.route = RT_PERIOD;
                p.nv = P.span_vecs <= 512u ? 2 : P.span_vecs <= 1024u ? 4 : 8;
                p.grid = blocks(cB - cA, P.per_wg);
                p.span_vecs = P.span_vecs;
                p.lds_bytes = P.span_vecs * 16u;
                p.head_end = cA * L;
                p.tail_begin = cB * L;
                return p;
            }
        }
    }
    const int fr = frames_per_thread((int)nch * width);
    const auto span_frames = [&](int f) { return ((uint64_t)256 * f * R.inr + R.outr - 1) / R.outr + 3; };   // input frames a workgroup reads
    p.n_out = n;
    if (small && R.inr < 65536u) {
        // span: frames q0 .. q0 + floor((r0 + (256*fr-1)*inr)/outr) + 1, the alignment slack of the first vector, and one more vector for
        // the dword-pair reads
        const uint64_t epv = 16 / width;
        const auto svecs = [&](int f) { return (span_frames(f) * nch + epv + epv - 1) / epv + 1; };
        // 16-bit mono: 16 frames per thread as two runs of 8 (GROUPS = 2) when the doubled span still fits -- the per-thread set-up is a
        // fifth of the instructions at 8 frames (+4 %), and a wave's store instruction writes 1 KB of consecutive bytes: +0.4 / +2.2 / +4 %
        // on 44.1 -> 48, 96 -> 44.1, 48 -> 44.1 kHz against one run of 16
        const int f = width == 2 && nch == 1 && svecs(2 * fr) * 16 <= RS_LDS_BYTES ? 2 * fr : fr;
        if (svecs(f) * 16 <= RS_LDS_BYTES) {
            p.route = RT_SMALL;
            p.fr = f;
            p.groups = f / fr;
            p.grid = blocks(blocks(n, f), 256);
            p.span_vecs = (uint32_t)svecs(f);
            p.lds_bytes = p.span_vecs * 16;
            return p;
        }
    }
    p.fr = fr;
    p.grid = blocks(blocks(n, fr), 256);
    const uint64_t span_bytes = span_frames(fr) * nch * width + 32;
    if (nch <= 2 && span_bytes <= RS_LDS_BYTES) {           // stage the span when it fits
        p.route = RT_LDS;
        p.lds_bytes = (uint32_t)((span_bytes + 15) & ~15ull);
    } else {
        p.route = RT_FRAMES;
    }
    return p;
}

}  // namespace shr
