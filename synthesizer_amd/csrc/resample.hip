// resample.hip -- linear-interpolation resampling (Sample.resample): audioop.ratecv on 8/16/24/32-bit PCM and its float32 form, and the
// sh_resample* entry points.
//
// CPython 3.10 Modules/audioop.c, audioop_ratecv_impl, in closed form: ratecv.hpp states the index arithmetic and the route plan, this
// file the kernels and their launch.  HBM-bound byte/integer work; the few-channel kernels stage a workgroup's input span in LDS.  Built
// with -ffp-contract=off: audioop forms prev*d + cur*(outrate-d) with two roundings and a division, and so does k_resample.
#include "common.hpp"
#include "ratecv.hpp"
#include <type_traits>

namespace {

using shr::PeriodArgs;
using shr::RS_INT_F64;
using shr::RS_FLOAT;
using shr::RS_INT_SMALL;

typedef short short8v __attribute__((ext_vector_type(8)));

struct RatecvArgs {
    uint64_t n_out_samples;     // work units of the launch (shr::Plan::n_out)
    uint64_t m_base;            // output frame index of the launch's first frame (range launches; else 0)
    uint32_t nch;
    uint32_t inr, outr;
    uint32_t step_q, step_r;    // inr / outr and inr % outr: output frame m+1 starts (step_q, step_r) after frame m
    double   inv_outr;
    int      shift;             // 32 - 8*width (integer PCM)
};

__device__ __forceinline__ shr::Pos ratecv_pos(const RatecvArgs& A, uint64_t m) { return shr::position(m, A.inr, A.outr, A.inv_outr); }

// One output sample in the launch's mode; the arithmetic itself is ratecv.hpp's (shr::value, shr::small_int, shr::shifted_int).
template <typename T, int MODE>
__device__ __forceinline__ T ratecv_sample(T prev, T cur, uint32_t d, const RatecvArgs& A) {
    if (MODE == RS_INT_SMALL) {
        if constexpr (sizeof(T) <= 2) return shr::small_int<T>(prev, cur, d, A.outr, A.inv_outr);
        else return (T)0;
    }
    if (MODE == RS_FLOAT) return (T)shr::value((double)prev, (double)cur, (double)d, (double)(A.outr - d), (double)A.outr, A.inv_outr);
    return (T)shr::shifted_int((int)prev, (int)cur, d, A.outr, A.inv_outr, A.shift);
}

// One thread = one output frame x VEC channels, moved as one vector (VEC*sizeof(T) bytes).
template <typename T, int VEC, int MODE>
__global__ __launch_bounds__(256) void k_resample(const T* __restrict__ in, T* __restrict__ out, RatecvArgs A) {
    typedef T vec_t __attribute__((ext_vector_type(VEC)));
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= A.n_out_samples) return;                     // here: number of (frame, channel group) units
    const uint32_t groups = A.nch / VEC;
    uint64_t m;
    uint32_t cg;
    if (groups == 1) { m = u; cg = 0; }
    else if (u < 0xFFFFFFFFull) { uint32_t u32 = (uint32_t)u; uint32_t m32 = u32 / groups; m = m32; cg = u32 - m32 * groups; }
    else { m = u / groups; cg = (uint32_t)(u - m * groups); }
    m += A.m_base;
    uint64_t j;
    uint32_t d;
    shr::index(ratecv_pos(A, m), A.outr, j, d);
    const size_t cur_at = (size_t)j * A.nch + (size_t)cg * VEC;
    vec_t cur, prev, res;
    if (VEC == 1) cur[0] = in[cur_at]; else cur = *reinterpret_cast<const vec_t*>(in + cur_at);
    if (j && d) {
        if (VEC == 1) prev[0] = in[cur_at - A.nch]; else prev = *reinterpret_cast<const vec_t*>(in + cur_at - A.nch);
    } else {
#pragma unroll
        for (int c = 0; c < VEC; ++c) prev[c] = (T)0;
    }
#pragma unroll
    for (int c = 0; c < VEC; ++c) res[c] = ratecv_sample<T, MODE>(prev[c], cur[c], d, A);
    const size_t out_at = (size_t)m * A.nch + (size_t)cg * VEC;
    // (streaming store: +4 % on the 8-channel rows; the frames-per-thread kernels below lose with it -- stereo float32 -14 %)
    if (VEC == 1) out[out_at] = res[0]; else __builtin_nontemporal_store(res, reinterpret_cast<vec_t*>(out + out_at));
}

// The workgroup's input span -- nvec 16-byte vectors from input element lo_elem (16-byte aligned) on -- into LDS with aligned 16-byte loads
// (coalesced, every input byte fetched once), zeros beyond total_elems.  NT: streaming loads.
template <bool NT, typename T>
__device__ __forceinline__ void stage_span(unsigned char* smem, const T* __restrict__ in, uint64_t lo_elem, uint32_t nvec, uint64_t total_elems) {
    typedef T ld_t __attribute__((ext_vector_type(16 / sizeof(T))));
    constexpr uint32_t EPV = 16 / sizeof(T);                      // elements per 16-byte vector
    T* lds = reinterpret_cast<T*>(smem);
    for (uint32_t v = threadIdx.x; v < nvec; v += 256) {
        const uint64_t e = lo_elem + (uint64_t)v * EPV;
        if (e + EPV <= total_elems) {
            const ld_t* src = reinterpret_cast<const ld_t*>(in + e);
            if constexpr (NT) reinterpret_cast<ld_t*>(lds)[v] = __builtin_nontemporal_load(src);
            else reinterpret_cast<ld_t*>(lds)[v] = *src;
        } else {
            for (uint32_t k = 0; k < EPV; ++k) lds[v * EPV + k] = (e + k < total_elems) ? in[e + k] : (T)0;
        }
    }
}

// A thread's FR frames x VEC channels from output frame m0 on: one vector store, or sample by sample at the end of the output.  NT: a
// streaming store.
template <bool NT, int VEC, int FR, typename T, typename V>
__device__ __forceinline__ void store_frames(T* __restrict__ out, uint64_t m0, uint64_t out_frames, const V& res) {
    if (m0 + FR <= out_frames) {
        if constexpr (NT) __builtin_nontemporal_store(res, reinterpret_cast<V*>(out + m0 * VEC));
        else *reinterpret_cast<V*>(out + m0 * VEC) = res;
    } else {
        for (int f = 0; f < FR && m0 + f < out_frames; ++f)
            for (int c = 0; c < VEC; ++c) out[(m0 + f) * VEC + c] = res[f * VEC + c];
    }
}

// Few channels (nch == VEC): one thread = FR consecutive output frames x all channels, so that the store is one 8..16-byte vector even for
// mono 16-bit PCM (a 2-byte store per lane reaches ~1/4 of the bandwidth).  The samples come from global memory, or (LDS) from the
// workgroup's input span staged first -- instead of 2*FR narrow gathers per thread; the plan stages it when it fits the LDS budget (ratios
// up to ~10:1).  (Plain stores: the streaming store loses here -- stereo float32 -14 %.)
template <typename T, int VEC, int FR, int MODE, bool LDS>
__global__ __launch_bounds__(256) void k_resample_frames(const T* __restrict__ in, T* __restrict__ out, RatecvArgs A,
                                                         uint64_t in_frames, uint64_t out_frames) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const T* lds = reinterpret_cast<const T*>(smem);
    typedef T vec_t __attribute__((ext_vector_type(VEC * FR)));
    const uint64_t m_first = A.m_base + (uint64_t)blockIdx.x * (256 * FR);
    uint64_t lo_elem = 0;                                         // LDS element 0 = input element lo_elem
    if constexpr (LDS) {
        constexpr uint32_t EPV = 16 / sizeof(T);
        if (m_first >= out_frames) return;
        const uint64_t m_last = m_first + 256 * FR - 1 < out_frames ? m_first + 256 * FR - 1 : out_frames - 1;
        // input frames this workgroup reads: [j(m_first) - 1, j(m_last)]   (uniform)
        uint64_t jf, jl;
        uint32_t d;
        shr::index(ratecv_pos(A, m_first), A.outr, jf, d);
        shr::index(ratecv_pos(A, m_last), A.outr, jl, d);
        lo_elem = ((jf ? jf - 1 : 0) * VEC) & ~(uint64_t)(EPV - 1);
        stage_span<false>(smem, in, lo_elem, (uint32_t)(((jl + 1) * VEC - lo_elem + EPV - 1) / EPV), in_frames * VEC);
        __syncthreads();
    }
    const auto x = [&](uint64_t j, int c) { return LDS ? lds[(uint32_t)(j * VEC - lo_elem) + c] : in[j * VEC + c]; };   // sample c of frame j
    const uint64_t m0 = m_first + (uint64_t)threadIdx.x * FR;
    if (m0 >= out_frames) return;
    shr::Pos p = ratecv_pos(A, m0);
    const uint64_t frames_after = out_frames - 1 - m0;            // frames after m0 that exist
    vec_t res;
#pragma unroll
    for (int f = 0; f < FR; ++f) {
        uint64_t j;
        uint32_t d;
        shr::index(p, A.outr, j, d);
        if ((uint64_t)f < frames_after) shr::step<uint64_t>(p.q, p.r, A.step_q, A.step_r, A.outr);   // never past the last output frame
#pragma unroll
        for (int c = 0; c < VEC; ++c) res[f * VEC + c] = ratecv_sample<T, MODE>((j && d) ? x(j - 1, c) : (T)0, x(j, c), d, A);
    }
    store_frames<false, VEC, FR>(out, m0, out_frames, res);
}

// One thread's FR output frames of k_resample_small, from the staged span (LDS element 0 = input element lo_elem).  GROUPS == 2:
// the thread's frames are two runs of FR/2, 256*FR/2 frames apart, so that each of its stores is one 16-byte vector NEXT to its
// neighbour lanes' (a wave's store instruction then writes 1 KB of consecutive bytes; with one run of 16 16-bit frames a lane's two
// 16-byte stores interleave with its neighbours' at a 32-byte stride).
template <typename T, int VEC, int FR, int GROUPS = 1>
__device__ __forceinline__ void resample_small_frames(const unsigned char* smem, T* __restrict__ out, const RatecvArgs& A, uint64_t m_first,
                                                      uint64_t q0, uint32_t r0, uint64_t lo_elem, uint64_t out_frames) {
    const T* lds = reinterpret_cast<const T*>(smem);
    constexpr int FRG = FR / GROUPS;
    typedef T vec_t __attribute__((ext_vector_type(VEC * FRG)));
    constexpr int HALF = 1 << (8 * (int)sizeof(T) - 1);
    uint64_t m0 = m_first + (uint64_t)threadIdx.x * FRG;
    if (m0 >= out_frames) return;
    // this thread's first frame: (q0, r0) advanced by threadIdx.x*FR output frames (host guarantees < 2^31)
    uint32_t r, qe_elem;
    {
        const uint32_t tot = r0 + __umul24(threadIdx.x * FRG, A.inr);
        const uint32_t dq = shr::floor_by_outr(tot, A.inv_outr);
        r = tot - dq * A.outr;
        qe_elem = (uint32_t)(q0 * VEC - lo_elem) + dq * VEC;                     // LDS element index of frame q
    }
    const uint32_t step_elem = A.step_q * VEC;
    constexpr bool PAIR_IN_DWORD = 2 * VEC * sizeof(T) <= 4;
    constexpr uint32_t MASK = (1u << (8 * sizeof(T))) - 1u;
    constexpr uint32_t FLIP = sizeof(T) == 2 ? 0x80008000u : 0x80808080u;
#pragma unroll
    for (int g = 0; g < GROUPS; ++g) {
    vec_t res;
#pragma unroll
    for (int f = 0; f < FRG; ++f) {
        uint32_t pair = 0;
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            // ua = a + HALF, ub = b + HALF as unsigned bit patterns (x + HALF == x ^ HALF on the sample width)
            uint32_t ua, ub;
            if (PAIR_IN_DWORD) {
                // frames q and q+1 together are <= 4 bytes at a 1- or 2-byte aligned address: two aligned dwords and a
                // funnel shift (a misaligned ds_read_b32 is several times slower than the extra three instructions)
                if (c == 0) {
                    const uint32_t byte_off = qe_elem * (uint32_t)sizeof(T);
                    const uint32_t* l32 = reinterpret_cast<const uint32_t*>(smem) + (byte_off >> 2);
                    pair = __builtin_amdgcn_alignbit(l32[1], l32[0], (byte_off & 3u) * 8u) ^ FLIP;
                }
                ua = (pair >> (8 * sizeof(T) * c)) & MASK;
                ub = (pair >> (8 * sizeof(T) * (VEC + c))) & MASK;
            } else {
                ua = ((uint32_t)lds[qe_elem + c] & MASK) ^ (uint32_t)HALF;
                ub = ((uint32_t)lds[qe_elem + VEC + c] & MASK) ^ (uint32_t)HALF;
            }
            const uint32_t u = (uint32_t)__mul24((int)ub - (int)ua, (int)r) + __umul24(ua, A.outr);
            res[f * VEC + c] = (T)(shr::floor_by_outr(u, A.inv_outr) ^ (uint32_t)HALF);
        }
        shr::step<uint32_t>(qe_elem, r, step_elem, A.step_r, A.outr, (uint32_t)VEC);
    }
    if (m0 + FRG <= out_frames) {
        __builtin_nontemporal_store(res, reinterpret_cast<vec_t*>(out + m0 * VEC));
    } else {
        for (int f = 0; f < FRG && m0 + f < out_frames; ++f)
            for (int c = 0; c < VEC; ++c) out[(m0 + f) * VEC + c] = res[f * VEC + c];
    }
    if (g + 1 < GROUPS) {
        // on to the thread's next run: 255 * FRG frames further (the loop above has moved FRG already)
        m0 += 256 * FRG;
        if (m0 >= out_frames) return;
        const uint32_t tot = r + (uint32_t)(255 * FRG) * A.inr;
        const uint32_t dq = shr::floor_by_outr(tot, A.inv_outr);
        r = tot - dq * A.outr;
        qe_elem += dq * VEC;
    }
    }
}

// 8/16-bit PCM, few channels, reduced rates below 65536 (the common Sample.resample case: 16-bit mono/stereo
// between 44.1k/48k/96k).  The generic kernels above are VALU-issue-bound there (~55 instructions per output
// sample at 2-4 bytes of traffic each), so this one strips the arithmetic to ~20 full-rate instructions:
//  * the workgroup's input span goes through LDS (aligned 16-byte loads), positions are 32-bit LDS-relative;
//  * output m sits at input position q + r/outr; with a = x[q], b = x[q+1] the reference's expression is
//    M = a*(outr-r) + b*r for every r (r == 0 gives cur = x[q], weight outr), so there is no prev/cur select;
//  * u = M + HALF*outr = (b-a)*r + (a+HALF)*outr in 24-bit multiplies (mod 2^32; 0 <= u < 2^32);
//  * floor(u/outr) by shr::floor_by_outr.  See shr::small_int for why the floor equals audioop's float64 expression.
// (Measured and dropped, bit-identical both: the interpolation as ONE v_dot2_u32_u16 on packed weights -- 0.395 vs 0.391 ms on 900 MB;
// the output frames dealt to the lanes, no LDS bank conflicts and 16 instead of 20 instructions per sample -- not faster either:
// CHANGELOG items 39 and 22; profiles/r03_summary.md.)
template <typename T, int VEC, int FR, int GROUPS = 1>
__global__ __launch_bounds__(256) void k_resample_small(const T* __restrict__ in, T* __restrict__ out, RatecvArgs A,
                                                        uint64_t in_frames, uint64_t out_frames, uint32_t span_vecs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr uint32_t EPV = 16 / sizeof(T);
    const uint64_t m_first = A.m_base + (uint64_t)blockIdx.x * (256 * FR);
    if (m_first >= out_frames) return;
    const shr::Pos p0 = ratecv_pos(A, m_first);                                  // the workgroup's first output frame (uniform)
    const uint64_t lo_elem = (p0.q * VEC) & ~(uint64_t)(EPV - 1);                // 16-byte aligned start of the span
    // streaming on both sides (input read once per workgroup, output never re-read): +1..3 % on the 16-bit rows
    stage_span<true>(smem, in, lo_elem, span_vecs, in_frames * VEC);
    __syncthreads();
    resample_small_frames<T, VEC, FR, GROUPS>(smem, out, A, m_first, p0.q, p0.r, lo_elem, out_frames);
}

// ---- 16-bit mono between rates with a SHORT period (44.1k <-> 48k <-> 96k ...: reduced outrate <= 2048) --------------------------------
// k_resample_small needs ~23 VALU instructions per output sample (the position's remainder stepped and wrapped, the frame pair cut out of
// two dwords, the weights), and with its 78 % of the VALU slots taken it sits between its two roofs: 0.68 of HBM whatever one of those
// instructions is replaced by (five variants: profiles/r06_resample_ab.txt).  But output frame m and m + outr lie at the same fraction
// r / outr, inr input frames apart: with CHUNKS of K whole periods (L = K outr output frames, K inr input frames, starting at remainder 0)
// thread t's sixteen frames of EVERY chunk have the same weights (outr - r, r) and the same offsets into the chunk's input span.  The
// workgroups stay (chunk C, C + grid, ...), a thread works its sixteen (weights, offset) pairs out ONCE, and a sample is
//      an address (offset + where the span starts in its first 16-byte vector), two sign-extending 16-bit LDS reads,
//      u = a (outr - r) + b r + 65536 outr in two 24-bit multiply-adds, floor(u / outr) by shr::floor_by_outr (3 instructions) --
// whose low sixteen bits ARE the sample (floor(M / outr) + 65536: no bias to take off again) -- 6.5 instructions instead of 23.
// The same integers as k_resample_small's, i.e. audioop.ratecv's (tests/test_gpu_pcm.py against the live module).  PeriodArgs: ratecv.hpp.

template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// NV: 16-byte vectors of the span per thread (span_vecs <= 256 NV).  A workgroup works through per_wg CONSECUTIVE chunks and ends; the
// span of the next chunk is loaded into registers while this one is worked on.  What the shape of the loop is for
// (profiles/r06_resample_period.txt):
//  * this chip counts loads and stores in ONE in-order counter (vmcnt): "wait for my loads" also waits for every store issued before
//    them.  The next span's loads are therefore issued BEFORE the chunk's stores and waited for at the END of the turn, where the wait
//    the compiler inserts is vmcnt(stores of this turn): the stores stay in flight across the barrier.  That needs a turn without a
//    branch around a memory instruction (a path with fewer stores, and the count drops to zero): lanes beyond the span load its last
//    vector again, lanes beyond the chunk's last run do that run again (same frames, same values, same address), and L is a multiple
//    of 8, so a run is whole or absent;
//  * workgroups that STAY for the whole call (chunks C, C + grid, ...) march in step -- all load, all compute, all store -- and reach 0.63-0.70
//    of HBM on the 44.1 -> 48 kHz row where workgroups of ONE chunk each (dispatched as others end, their phases mixed) reach 0.72;
//    but one chunk per workgroup pays the sixteen (weights, offset) set-ups for sixteen samples (upsampling 44.1 -> 96 kHz: 0.60
//    against 0.70).  A few chunks per workgroup keep both.
// VEC: channels (1: mono, a run = 8 frames; 2: stereo, a run = 4 frames -- 16 bytes either way).  All positions below are in FRAMES; a frame
// is VEC shorts.
template <int VEC, int NV>
__global__ __launch_bounds__(256) void k_resample_period_i16(const short* __restrict__ in, short* __restrict__ out, PeriodArgs P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int FPR = 8 / VEC;                      // frames per run
    constexpr uint32_t RUN2 = 256u * FPR;             // the second run lies this many frames behind the first: a wave's store instruction writes 1 KB of consecutive bytes
    const uint32_t t = threadIdx.x;
    // the thread's frames of a chunk: two runs (the last run of each half that lies inside the chunk: L >= RUN2 + FPR, a multiple of FPR)
    uint32_t w0[2 * FPR], w1[2 * FPR], ob[2 * FPR];
    const uint32_t last0 = P.L / FPR - 1u, last1 = (P.L - RUN2) / FPR - 1u;
    const uint32_t run0[2] = {(uint32_t)FPR * (t < last0 ? t : last0), RUN2 + (uint32_t)FPR * (t < last1 ? t : last1)};
#pragma unroll
    for (int k = 0; k < 2 * FPR; ++k) {
        const uint32_t e = __umul24(run0[k / FPR] + (uint32_t)(k % FPR), P.inr);  // < 2^12 * 2^16
        const uint32_t dq = shr::floor_by_outr(e, P.inv_outr);                     // floor(e / outr)
        const uint32_t r = e - dq * P.outr;
        w0[k] = P.outr - r;
        w1[k] = r;
        ob[k] = dq * (uint32_t)(2 * VEC);              // bytes
    }
    const int acc = (int)(65536u * P.outr);
    // (the LDS address of the staged span for the hand-written reads below: 0 in this kernel -- it has no other shared memory -- but asked for, not assumed)
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    uint64_t C = P.c0 + (uint64_t)blockIdx.x * P.per_wg;
    if (C >= P.c1) return;
    const uint64_t c_end = C + P.per_wg < P.c1 ? C + P.per_wg : P.c1;
    short8v pre[NV];
    uint32_t vi[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) vi[i] = t + 256u * i < P.span_vecs ? t + 256u * i : P.span_vecs - 1u;
    {
        const short8v* __restrict__ src = reinterpret_cast<const short8v*>(in + ((C * (uint64_t)P.kinr * VEC) & ~(uint64_t)7));
#pragma unroll
        for (int i = 0; i < NV; ++i) pre[i] = __builtin_nontemporal_load(src + vi[i]);
#pragma unroll
        for (int i = 0; i < NV; ++i) reinterpret_cast<short8v*>(smem)[vi[i]] = pre[i];
    }
    for (;;) {
        __syncthreads();                                   // the chunk's span is in LDS
        const bool more = C + 1 < c_end;                   // (uniform)
        if (more) {
            const short8v* __restrict__ src = reinterpret_cast<const short8v*>(in + (((C + 1) * (uint64_t)P.kinr * VEC) & ~(uint64_t)7));
            static_for<0, NV>([&](auto i_) { constexpr int i = decltype(i_)::value; pre[i] = __builtin_nontemporal_load(src + vi[i]); });
        }
        const uint32_t rel0b = (uint32_t)((C * (uint64_t)P.kinr * VEC) & 7) * 2u;
        short* __restrict__ outC = out + C * (uint64_t)P.L * VEC;
        auto run = [&](auto g_) __attribute__((always_inline)) {
            constexpr int g = decltype(g_)::value;
            // The run's frame pairs (a, b) out of LDS, by hand.  Mono: two sign-extending 16-bit reads per frame -- written as plain loads the
            // compiler fuses each pair into ONE ds_read_b32 at a 2-byte-aligned address, which the LDS serves at a fraction of the rate
            // (0.87 ms for the 900 MB row against 0.44 for k_resample_small); `volatile` loads become FLAT loads; and the D16 forms that
            // would fill the halves of one register for a v_dot2 clear the other half on this chip (SRAM ECC).  Stereo: frames are dwords,
            // one ds_read2_b32 per pair.  The reads are waited for inside the statement (the compiler's counters do not see them).
            uint32_t at[FPR];
#pragma unroll
            for (int f = 0; f < FPR; ++f) at[f] = ob[FPR * g + f] + rel0b + lds0;
            short8v res;
            if constexpr (VEC == 1) {
                int a[8], b[8];
                asm volatile(
                    "ds_read_i16 %0, %16\n\tds_read_i16 %8, %16 offset:2\n\t"
                    "ds_read_i16 %1, %17\n\tds_read_i16 %9, %17 offset:2\n\t"
                    "ds_read_i16 %2, %18\n\tds_read_i16 %10, %18 offset:2\n\t"
                    "ds_read_i16 %3, %19\n\tds_read_i16 %11, %19 offset:2\n\t"
                    "ds_read_i16 %4, %20\n\tds_read_i16 %12, %20 offset:2\n\t"
                    "ds_read_i16 %5, %21\n\tds_read_i16 %13, %21 offset:2\n\t"
                    "ds_read_i16 %6, %22\n\tds_read_i16 %14, %22 offset:2\n\t"
                    "ds_read_i16 %7, %23\n\tds_read_i16 %15, %23 offset:2\n\t"
                    "s_waitcnt lgkmcnt(0)"
                    : "=&v"(a[0]), "=&v"(a[1]), "=&v"(a[2]), "=&v"(a[3]), "=&v"(a[4]), "=&v"(a[5]), "=&v"(a[6]), "=&v"(a[7]),
                      "=&v"(b[0]), "=&v"(b[1]), "=&v"(b[2]), "=&v"(b[3]), "=&v"(b[4]), "=&v"(b[5]), "=&v"(b[6]), "=&v"(b[7])
                    : "v"(at[0]), "v"(at[1]), "v"(at[2]), "v"(at[3]), "v"(at[4]), "v"(at[5]), "v"(at[6]), "v"(at[7])
                    : "memory");
#pragma unroll
                for (int f = 0; f < 8; ++f) {
                    const uint32_t u = (uint32_t)__mul24(a[f], (int)w0[8 * g + f]) + (uint32_t)(__mul24(b[f], (int)w1[8 * g + f]) + acc);
                    res[f] = (short)shr::floor_by_outr(u, P.inv_outr);
                }
            } else {
                uint64_t ab[4];                            // low dword: frame q (L | R << 16), high dword: frame q + 1
                asm volatile(
                    "ds_read2_b32 %0, %4 offset1:1\n\tds_read2_b32 %1, %5 offset1:1\n\t"
                    "ds_read2_b32 %2, %6 offset1:1\n\tds_read2_b32 %3, %7 offset1:1\n\t"
                    "s_waitcnt lgkmcnt(0)"
                    : "=&v"(ab[0]), "=&v"(ab[1]), "=&v"(ab[2]), "=&v"(ab[3])
                    : "v"(at[0]), "v"(at[1]), "v"(at[2]), "v"(at[3])
                    : "memory");
#pragma unroll
                for (int f = 0; f < 4; ++f) {
                    const int fa = (int)(uint32_t)ab[f], fb = (int)(uint32_t)(ab[f] >> 32);
                    const int la = (int)(short)fa, ra = fa >> 16, lb = (int)(short)fb, rb = fb >> 16;
                    const int k0 = (int)w0[4 * g + f], k1 = (int)w1[4 * g + f];
                    const uint32_t ul = (uint32_t)__mul24(la, k0) + (uint32_t)(__mul24(lb, k1) + acc);
                    const uint32_t ur = (uint32_t)__mul24(ra, k0) + (uint32_t)(__mul24(rb, k1) + acc);
                    res[2 * f] = (short)shr::floor_by_outr(ul, P.inv_outr);
                    res[2 * f + 1] = (short)shr::floor_by_outr(ur, P.inv_outr);
                }
            }
            __builtin_nontemporal_store(res, reinterpret_cast<short8v*>(outC + (size_t)run0[g] * VEC));
        };
        run(std::integral_constant<int, 0>{});
        run(std::integral_constant<int, 1>{});
        __syncthreads();                                   // everybody has read the span
        if (!more) break;
        // (waits for the loads; this turn's stores stay in flight)
        static_for<0, NV>([&](auto i_) { constexpr int i = decltype(i_)::value; reinterpret_cast<short8v*>(smem)[vi[i]] = pre[i]; });
        C += 1;
    }
}

// ---- launch: the plan, then the kernel it names ----------------------------------------------------------------------------------------

// The plan's kernel for element type T and mode MODE at channel vector VEC -- only the instances a plan can name; false for any other.
template <typename T, int MODE, int VEC>
bool launch_vec(const shr::Plan& p, const T* in, T* out, const RatecvArgs& A, uint64_t in_frames, hipStream_t st) {
    const dim3 g(p.grid), b(256);
    if (p.route == shr::RT_GENERIC) {
        hipLaunchKernelGGL((k_resample<T, VEC, MODE>), g, b, 0, st, in, out, A);
        return true;
    }
    constexpr int FR = shr::frames_per_thread(VEC * (int)sizeof(T));
    if constexpr (VEC <= 4 && VEC * sizeof(T) <= 8) {
        if (p.fr == FR && p.route == shr::RT_FRAMES) {
            hipLaunchKernelGGL((k_resample_frames<T, VEC, FR, MODE, false>), g, b, 0, st, in, out, A, in_frames, p.m_end);
            return true;
        }
        if constexpr (VEC <= 2)
            if (p.fr == FR && p.route == shr::RT_LDS) {
                hipLaunchKernelGGL((k_resample_frames<T, VEC, FR, MODE, true>), g, b, p.lds_bytes, st, in, out, A, in_frames, p.m_end);
                return true;
            }
        if constexpr (MODE == RS_INT_SMALL) {
            if (p.fr == FR && p.groups == 1 && p.route == shr::RT_SMALL) {
                hipLaunchKernelGGL((k_resample_small<T, VEC, FR>), g, b, p.lds_bytes, st, in, out, A, in_frames, p.m_end, p.span_vecs);
                return true;
            }
            if constexpr (sizeof(T) == 2 && VEC == 1)       // 16-bit mono: two runs of 8 frames per thread
                if (p.fr == 2 * FR && p.groups == 2 && p.route == shr::RT_SMALL) {
                    hipLaunchKernelGGL((k_resample_small<T, 1, 2 * FR, 2>), g, b, p.lds_bytes, st, in, out, A, in_frames, p.m_end, p.span_vecs);
                    return true;
                }
        }
    }
    return false;
}

template <typename T, int MODE>
bool launch_mode(const shr::Plan& p, const void* in, void* out, const RatecvArgs& A, uint64_t in_frames, hipStream_t st) {
    const T* x = (const T*)in;
    T* y = (T*)out;
    switch (p.vec) {
    case 1: return launch_vec<T, MODE, 1>(p, x, y, A, in_frames, st);
    case 2: return launch_vec<T, MODE, 2>(p, x, y, A, in_frames, st);
    case 4: return launch_vec<T, MODE, 4>(p, x, y, A, in_frames, st);
    case 8: if constexpr (sizeof(T) <= 2) return launch_vec<T, MODE, 8>(p, x, y, A, in_frames, st); break;
    case 16: if constexpr (sizeof(T) == 1) return launch_vec<T, MODE, 16>(p, x, y, A, in_frames, st); break;
    }
    return false;
}

template <typename T>
bool launch_type(const shr::Plan& p, const void* in, void* out, const RatecvArgs& A, uint64_t in_frames, hipStream_t st) {
    if constexpr (std::is_same<T, float>::value) return p.mode == RS_FLOAT && launch_mode<T, RS_FLOAT>(p, in, out, A, in_frames, st);
    else if constexpr (sizeof(T) == 4) return p.mode == RS_INT_F64 && launch_mode<T, RS_INT_F64>(p, in, out, A, in_frames, st);
    else return p.mode == RS_INT_SMALL ? launch_mode<T, RS_INT_SMALL>(p, in, out, A, in_frames, st)
                                       : p.mode == RS_INT_F64 && launch_mode<T, RS_INT_F64>(p, in, out, A, in_frames, st);
}

template <int VEC>
bool launch_period(const shr::Plan& p, const void* in, void* out, hipStream_t st) {
    const dim3 g(p.grid), b(256);
    const short* x = (const short*)in;
    short* y = (short*)out;
    switch (p.nv) {
    case 2: hipLaunchKernelGGL((k_resample_period_i16<VEC, 2>), g, b, p.lds_bytes, st, x, y, p.P); return true;
    case 4: hipLaunchKernelGGL((k_resample_period_i16<VEC, 4>), g, b, p.lds_bytes, st, x, y, p.P); return true;
    case 8: hipLaunchKernelGGL((k_resample_period_i16<VEC, 8>), g, b, p.lds_bytes, st, x, y, p.P); return true;
    }
    return false;
}

// One planned launch.  in / out are the addresses input frame 0 / output frame 0 would have (range launches pass pointers shifted back by the
// frames they do not hold: never dereferenced outside the held input and [m_base, m_end)); in_frames = end of the held input.
int launch(const shr::Plan& p, const void* in, void* out, int width, int is_float, uint32_t nch, shr::Rates R, uint64_t in_frames) {
    static const char* const name[] = {"", "k_resample", "k_resample_frames", "k_resample_frames", "k_resample_small", "k_resample_period_i16"};
    if (p.route == shr::RT_NONE) return SH_OK;
    hipStream_t st = sh::state().stream;
    RatecvArgs A;
    A.n_out_samples = p.n_out;
    A.m_base = p.m_base;
    A.nch = nch;
    A.inr = R.inr;
    A.outr = R.outr;
    A.inv_outr = 1.0 / (double)R.outr;
    A.step_q = R.inr / R.outr;
    A.step_r = R.inr % R.outr;
    A.shift = 32 - 8 * width;
    const bool ok = p.route == shr::RT_PERIOD ? (p.vec == 1 ? launch_period<1>(p, in, out, st) : p.vec == 2 && launch_period<2>(p, in, out, st))
                  : is_float ? launch_type<float>(p, in, out, A, in_frames, st)
                  : width == 1 ? launch_type<signed char>(p, in, out, A, in_frames, st)
                  : width == 2 ? launch_type<short>(p, in, out, A, in_frames, st)
                               : launch_type<int>(p, in, out, A, in_frames, st);
    if (!ok) return sh::set_error(SH_ERR_INVALID, "resample: no kernel for route %d (width %d, VEC %d, FR %d)", p.route, width, p.vec, p.fr);
    SH_CHECK_LAUNCH(name[p.route]);
    return SH_OK;
}

// Output frames [m_base, m_end) from held input frames [in_lo, in_frames): the plan's launch, and around the period kernel's interior
// chunks the head and tail it leaves, planned without it.
int resample_launch(const void* in, size_t in_frames, int nch, int width, int is_float, int inrate, int outrate,
                    void* out, size_t m_base, size_t m_end, size_t in_lo) {
    const shr::Rates R = shr::reduce((uint64_t)inrate, (uint64_t)outrate);
    const bool aligned = (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
    const sh::Knobs& k = sh::knobs();
    const auto plan = [&](bool no_period, uint64_t a, uint64_t b) {
        return shr::plan(width, is_float != 0, (uint32_t)nch, R, aligned, no_period, k.period_chunks, a, b, in_lo, in_frames);
    };
    const auto run = [&](const shr::Plan& p) { return launch(p, in, out, width, is_float, (uint32_t)nch, R, in_frames); };
    const shr::Plan p = plan(k.no_period, m_base, m_end);
    int rc = run(p);
    if (!rc && p.route == shr::RT_PERIOD) rc = run(plan(true, m_base, p.head_end));
    if (!rc && p.route == shr::RT_PERIOD) rc = run(plan(true, p.tail_begin, m_end));
    return rc;
}

// Output ranges of any length: one launch per 2^30 output samples at most (a dispatch holds fewer than 2^32 work-items per grid
// dimension; the kernels work from absolute output positions, so a range cut at multiples of 4096 frames is the same range)
int resample_dev(const void* in, size_t in_frames, int nch, int width, int is_float, int inrate, int outrate,
                 void* out, size_t m_base, size_t m_end, size_t in_lo) {
    size_t chunk = (((size_t)1 << 30) / (size_t)nch) & ~(size_t)4095;
    if (chunk < 4096) chunk = 4096;
    for (size_t m = m_base; m < m_end; m += chunk) {
        const int rc = resample_launch(in, in_frames, nch, width, is_float, inrate, outrate, out, m, m_end - m < chunk ? m_end : m + chunk, in_lo);
        if (rc) return rc;
    }
    return SH_OK;
}

// Output frames [out_first, out_first + out_n) from input frames [in_first, in_first + in_held), held at in / out.  audioop.ratecv at
// width 3 works on GETSAMPLE32 = value << 8 and stores SETSAMPLE32 = result >> 8: the 32-bit path on unpacked samples, packed again.
int resample_at(const void* in, size_t in_first, size_t in_held, int nch, int width, int is_float, int inrate, int outrate,
                void* out, size_t out_first, size_t out_n) {
    if (!out_n) return SH_OK;
    const size_t fb = (size_t)width * nch;
    if (width != 3)
        return resample_dev((const char*)in - in_first * fb, in_first + in_held, nch, width, is_float, inrate, outrate,
                            (char*)out - out_first * fb, out_first, out_first + out_n, in_first);
    sh::Temp tin, tout;
    int rc = tin.alloc(in_held * nch * 4);
    if (!rc) rc = tout.alloc(out_n * nch * 4);
    if (!rc) rc = sh::unpack24(in, in_held * nch, 8, (int32_t*)tin.buf.ptr);
    if (!rc) rc = resample_at(tin.buf.ptr, in_first, in_held, nch, 4, 0, inrate, outrate, tout.buf.ptr, out_first, out_n);
    if (!rc) rc = sh::pack24((const int32_t*)tout.buf.ptr, out_n * nch, 8, out);
    return rc;
}

int resample_check(int nch, int width, int is_float, int inrate, int outrate) {
    if (nch < 1) return sh::set_error(SH_ERR_INVALID, "resample: # of channels should be >= 1");
    if (width != 1 && width != 2 && width != 3 && width != 4) return sh::set_error(SH_ERR_INVALID, "resample: width %d not in {1,2,3,4}", width);
    if (is_float && width != 4) return sh::set_error(SH_ERR_INVALID, "resample: float PCM must have width 4");
    if (inrate <= 0 || outrate <= 0) return sh::set_error(SH_ERR_INVALID, "resample: sampling rate not > 0");
    return SH_OK;
}

}  // namespace

extern "C" {

size_t sh_resample_out_frames(size_t in_frames, int inrate, int outrate) {
    if (inrate <= 0 || outrate <= 0) return 0;
    return (size_t)shr::out_frames(in_frames, shr::reduce((uint64_t)inrate, (uint64_t)outrate));
}

int sh_resample(const sh_buf* in, size_t in_frames, int nchannels, int width, int is_float,
                int inrate, int outrate, sh_buf* out, size_t* out_frames) {
    SH_REQUIRE_INIT();
    if (!in || !out) return sh::set_error(SH_ERR_INVALID, "sh_resample: NULL argument");
    int rc = resample_check(nchannels, width, is_float, inrate, outrate);
    if (rc) return rc;
    size_t nout = sh_resample_out_frames(in_frames, inrate, outrate);
    if (in->bytes / ((size_t)width * nchannels) < in_frames) return sh::set_error(SH_ERR_INVALID, "sh_resample: input buffer smaller than in_frames");
    if (out->bytes / ((size_t)width * nchannels) < nout) return sh::set_error(SH_ERR_INVALID, "sh_resample: output buffer too small (%zu frames needed)", nout);
    if (out_frames) *out_frames = nout;
    return resample_at(in->ptr, 0, in_frames, nchannels, width, is_float, inrate, outrate, out->ptr, 0, nout);
}

int sh_resample_span(size_t in_total_frames, int inrate, int outrate, size_t out_first, size_t out_n,
                     size_t* in_first, size_t* in_count) {
    if (!in_first || !in_count) return sh::set_error(SH_ERR_INVALID, "sh_resample_span: NULL argument");
    if (inrate <= 0 || outrate <= 0) return sh::set_error(SH_ERR_INVALID, "resample: sampling rate not > 0");
    const size_t nout = sh_resample_out_frames(in_total_frames, inrate, outrate);
    if (out_first > nout || out_n > nout - out_first) return sh::set_error(SH_ERR_INVALID, "sh_resample_span: output range outside the %zu output frames", nout);
    *in_first = 0;
    *in_count = 0;
    if (!out_n) return SH_OK;
    const shr::Span s = shr::reads(out_first, out_n, shr::reduce((uint64_t)inrate, (uint64_t)outrate));
    const uint64_t first = s.lo & ~(uint64_t)15;      // 16 frames of any layout are a multiple of 16 bytes: vector loads stay aligned
    *in_first = (size_t)first;
    *in_count = (size_t)(s.hi - first + 1);
    return SH_OK;
}

int sh_resample_range(const sh_buf* in, size_t in_first, size_t in_held, int nchannels, int width, int is_float,
                      int inrate, int outrate, size_t out_first, size_t out_n, sh_buf* out) {
    SH_REQUIRE_INIT();
    if (!in || !out) return sh::set_error(SH_ERR_INVALID, "sh_resample_range: NULL argument");
    int rc = resample_check(nchannels, width, is_float, inrate, outrate);
    if (rc) return rc;
    if ((out_first | in_first) & 15) return sh::set_error(SH_ERR_INVALID, "sh_resample_range: ranges must start at a multiple of 16 frames");
    const size_t fb = (size_t)width * nchannels;
    if (in->bytes / fb < in_held) return sh::set_error(SH_ERR_INVALID, "sh_resample_range: input buffer smaller than in_held frames");
    if (out->bytes / fb < out_n) return sh::set_error(SH_ERR_INVALID, "sh_resample_range: output buffer too small (%zu frames needed)", out_n);
    if (!out_n) return SH_OK;
    const shr::Span s = shr::reads(out_first, out_n, shr::reduce((uint64_t)inrate, (uint64_t)outrate));
    if (in_first > s.lo || s.hi >= (uint64_t)in_first + in_held)
        return sh::set_error(SH_ERR_INVALID, "sh_resample_range: output frames [%zu,+%zu) read input frames [%llu,%llu], buffer holds [%zu,+%zu)",
                             out_first, out_n, (unsigned long long)s.lo, (unsigned long long)s.hi, in_first, in_held);
    return resample_at(in->ptr, in_first, in_held, nchannels, width, is_float, inrate, outrate, out->ptr, out_first, out_n);
}

int sh_resample_host(const void* in, size_t in_frames, int nchannels, int width, int is_float,
                     int inrate, int outrate, void* out, size_t* out_frames) {
    SH_REQUIRE_INIT();
    int rc = resample_check(nchannels, width, is_float, inrate, outrate);
    if (rc) return rc;
    size_t nout = sh_resample_out_frames(in_frames, inrate, outrate);
    if (out_frames) *out_frames = nout;
    if (!nout) return SH_OK;
    if (!in || !out) return sh::set_error(SH_ERR_INVALID, "sh_resample_host: NULL argument");
    size_t fb = (size_t)width * nchannels;
    size_t in_bytes = in_frames * fb, out_bytes = nout * fb;
    size_t in_pad = (in_bytes + 255) & ~size_t(255);
    rc = sh::ensure_scratch(in_pad + out_bytes);
    if (rc) return rc;
    char* s = (char*)sh::state().scratch;
    hipStream_t st = sh::state().stream;
    SH_HIP(hipMemcpyAsync(s, in, in_bytes, hipMemcpyHostToDevice, st));
    rc = resample_at(s, 0, in_frames, nchannels, width, is_float, inrate, outrate, s + in_pad, 0, nout);
    if (rc) return rc;
    SH_HIP(hipMemcpyAsync(out, s + in_pad, out_bytes, hipMemcpyDeviceToHost, st));
    SH_HIP(hipStreamSynchronize(st));
    return SH_OK;
}

}  // extern "C"
