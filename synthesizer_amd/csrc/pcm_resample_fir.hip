// pcm_resample_fir.hip -- sh_pcm_resample_fir: a rational sample-rate conversion of PCM in device memory as a polyphase FIR with
// integer taps, exact to the last bit (pcmresample.hpp has the contract: the refusals, the result's length, the index arithmetic,
// the plan by which a call is divided; pcmfir.hpp the bound that makes a float64 FMA chain the exact integer sum).  Two kernels:
// k_firp_rows builds the row bank -- the taps of every residue, shifted by the residue's offset inside its chunk, as float64
// [chunk][step][r] -- and the table of E_q in the library's scratch; k_firp<T, NCH> does the arithmetic, one workgroup per `blocks`
// blocks of 64 groups of one channel.  No atomics, no scratch memory; every sample of x, of the taps and of the result is read and
// written as one sample through a type of alignment 1, so an operand may begin at any byte.
// Built with -ffp-contract=off like the rest: fma() where it is written and nowhere else.
#include "common.hpp"
#include "pcmdev.hpp"
#include "pcmhost.hpp"
#include "pcmresample.hpp"

namespace {

// a sample that may lie at any byte
template <typename T> struct Unaligned { typedef T type __attribute__((aligned(1))); };

#ifdef SH_FIRP_STAGE_F32
template <typename T> struct Staged { typedef float type; };
#else
template <typename T> struct Staged { typedef T type; };
#endif

struct Rows {
    const void* taps;          // m int16 values, at any byte
    double*     rows;          // [chunks][steps][R]
    uint32_t*   E;             // [chunks]
    uint32_t    m, L, M, delay, P, chunks, steps;
};

// element (q, t, r) of the row bank is tap row_tap(q, R q + r, t) or 0.0; the thread of a chunk's first element writes E_q
__global__ __launch_bounds__(256) void k_firp_rows(const Rows g) {
    constexpr uint32_t R = shpr::LANE_OUTPUTS;
    const size_t i = sh::block_id() * 256 + threadIdx.x;
    if (i >= (size_t)g.chunks * g.steps * R) return;
    const uint32_t r = (uint32_t)(i % R), t = (uint32_t)(i / R % g.steps), q = (uint32_t)(i / R / g.steps);
    const int64_t k = shpr::row_tap(q, q * R + r, t, g.P, g.L, g.M, g.delay, g.m);
    g.rows[i] = k < 0 ? 0.0 : (double)((const Unaligned<short>::type*)g.taps)[k];
    if (r == 0 && t == 0) g.E[q] = (uint32_t)shpr::E_of(q, g.P, g.L, g.M, g.delay);
}

// a tap of the row bank, read through the constant address space: the bank was written by the launch before, and with a wave-uniform
// address that makes the loads scalar whatever the kernel stores elsewhere
typedef double __attribute__((address_space(4))) Tap;

struct Firp {
    const void*     in;        // x: n frames of NCH channels
    const double*   rows;      // k_firp_rows' bank
    const uint32_t* E;         // and its E_q
    void*           out;       // frame `first` of the result
    uint64_t        n, first, count, g_first, g_last, nwg;
    shpr::Plan      pl;
    double          factor;
};

// One workgroup: workgroup blockIdx.(x, y) of channel blockIdx.z, `blocks` blocks of 64 consecutive groups from group g_first +
// wg * 64 * blocks on.  Per round wave w owns residue chunk q = round * q_waves + w % q_waves of block w / q_waves; its lane l is
// group l of that block and keeps the R sums of outputs P g + R q + r.  Per chunk of steps the span of x under ALL the workgroup's
// groups and chunks is staged once (coalesced; a frame outside [0, n) is a zero and no address outside x is formed); per step a lane
// reads ONE staged sample, converts it and feeds R fma() whose taps are wave-uniform (q comes through readfirstlane: scalar loads,
// 64 bytes a step).  The staged address is the lane's row base plus a wave-uniform offset that steps over the padding (staged_at).
template <typename T, int NCH>
__global__ __launch_bounds__(256) void k_firp(const Firp g) {
    constexpr uint32_t R = shpr::LANE_OUTPUTS, U = shpr::STEP_UNROLL;
    typedef typename Staged<T>::type S;
    extern __shared__ __align__(16) unsigned char firp_lds[];
    S* staged = (S*)firp_lds;
    const uint64_t wg = sh::block_id();
    if (wg >= g.nwg) return;
    const shpr::Plan& pl = g.pl;
    const uint32_t c = blockIdx.z;
    typedef typename Unaligned<T>::type X;
    const X* __restrict__ x = (const X*)g.in + c;
    const int64_t n = (int64_t)g.n;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint32_t groups = pl.blocks * shpr::BLOCK_GROUPS, blk = wave / pl.q_waves, gl = blk * shpr::BLOCK_GROUPS + lane;
    const uint64_t g0 = g.g_first + wg * groups;
    const S* at = staged + gl * (pl.Mp + pl.pad);
    for (uint32_t round = 0; round < pl.rounds; ++round) {
        const uint32_t q = round * pl.q_waves + wave % pl.q_waves;
        const bool live = blk < pl.blocks && q < pl.chunks;         // (wave-uniform)
        const uint32_t Eq = live ? g.E[q] : pl.e_lo;
        double acc[R];
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) acc[r] = 0.0;
        for (uint32_t t0 = 0; t0 < pl.steps; t0 += pl.step_chunk) {
            const uint32_t sc = pl.steps - t0 < pl.step_chunk ? pl.steps - t0 : pl.step_chunk, span = (groups - 1) * pl.Mp + pl.e_span + sc;
            const int64_t base = (int64_t)(g0 * pl.Mp) + pl.e_lo - (int64_t)(t0 + sc - 1);
            if (base >= n || base + (int64_t)span <= 0) continue;   // (the same for the whole workgroup) nothing of x under this chunk
            if (round == 0 || pl.steps > pl.step_chunk) {           // one chunk of steps: what round 0 staged serves every round
                __syncthreads();                                    // the span before has been read
                for (uint32_t j = threadIdx.x; j < span; j += 256) {
                    const int64_t f = base + (int64_t)j;
                    staged[shpr::staged_at(j, pl.Mp, pl.pad)] = f >= 0 && f < n ? (S)x[(size_t)f * NCH] : (S)0;
                }
                __syncthreads();
            }
            if (!live) continue;
            // step t0 + t reads o = o_hi - t frames into the lane's own: row o / M', column o % M' of the padded layout
            const uint32_t o_hi = Eq - pl.e_lo + sc - 1;
            uint32_t col = o_hi % pl.Mp, off = o_hi + o_hi / pl.Mp * pl.pad;
            const Tap* h = (const Tap*)(g.rows + ((size_t)q * pl.steps + t0) * R);
            for (uint32_t t = 0; t < sc; t += U, h += U * R) {
#pragma unroll
                for (uint32_t u = 0; u < U; ++u) {
                    const double xv = (double)at[off];
#pragma unroll
                    for (uint32_t r = 0; r < R; ++r) acc[r] = fma(h[u * R + r], xv, acc[r]);
                    off -= col ? 1 : 1 + pl.pad;                    // (never below 0 before the last step is done: unsigned wrap is unused)
                    col = col ? col - 1 : pl.Mp - 1;
                }
            }
        }
        if (!live || g0 + gl > g.g_last) continue;
        typename Unaligned<T>::type* out = (typename Unaligned<T>::type*)g.out + c;
        const uint64_t j0 = (g0 + gl) * pl.P + q * R;
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) {
            const uint64_t j = j0 + r;
            if (q * R + r < pl.P && j >= g.first && j - g.first < g.count)
                out[(size_t)(j - g.first) * NCH] = (T)fbound(acc[r] * g.factor, Lim<T>::lo, Lim<T>::hi);
        }
    }
}

int refuse(shpr::Refusal why, int nch, int width, uint64_t in_frames, uint32_t ntaps, uint32_t up, uint32_t down, uint32_t delay, double factor, uint64_t first,
           uint64_t nframes) {
    const char* fn = "sh_pcm_resample_fir";
    switch (why) {
    case shpr::OK: return SH_OK;
    case shpr::BAD_WIDTH: return sh::set_error(SH_ERR_INVALID, "%s: sample width %d not in {1,2} (widths 3 and 4 are not built)", fn, width);
    case shpr::BAD_CHANNELS: return sh::set_error(SH_ERR_INVALID, "%s: %d channels (1 or 2)", fn, nch);
    case shpr::NO_TAPS: return sh::set_error(SH_ERR_INVALID, "%s: no taps", fn);
    case shpr::TOO_MANY_TAPS: return sh::set_error(SH_ERR_INVALID, "%s: %u taps are more than %u: the sum would not be exact", fn, ntaps, shpr::MAX_TAPS);
    case shpr::BAD_RATIO: return sh::set_error(SH_ERR_INVALID, "%s: up %u and down %u are both at least 1", fn, up, down);
    case shpr::BAD_UP: return sh::set_error(SH_ERR_INVALID, "%s: up %u is more than %u", fn, up, shpr::MAX_UP);
    case shpr::BAD_STRIDE:
        return sh::set_error(SH_ERR_INVALID, "%s: %u/%u puts the lanes of a wave %llu frames apart, too far for a staged span of %u: convert in two steps", fn, up, down,
                             (unsigned long long)shpr::copies(up) * down, shpr::STAGED_SAMPLES);
    case shpr::BAD_DELAY: return sh::set_error(SH_ERR_INVALID, "%s: a delay of %u with %u taps (below the taps' count)", fn, delay, ntaps);
    case shpr::BAD_FACTOR: return sh::set_error(SH_ERR_INVALID, "%s: the factor %g is not finite", fn, factor);
    case shpr::BAD_WINDOW:
        return sh::set_error(SH_ERR_INVALID, "%s: frames [%llu, +%llu) reach past the result's %llu", fn, (unsigned long long)first, (unsigned long long)nframes,
                             (unsigned long long)shpr::result_frames(in_frames, up, down));
    case shpr::IN_RANGE: return sh::set_error(SH_ERR_INVALID, "%s: input range outside buffer", fn);
    case shpr::TAPS_RANGE: return sh::set_error(SH_ERR_INVALID, "%s: taps range outside buffer", fn);
    case shpr::OUT_RANGE: return sh::set_error(SH_ERR_INVALID, "%s: output range outside buffer", fn);
    case shpr::OVERLAP: return sh::set_error(SH_ERR_INVALID, "%s: out overlaps an input", fn);
    }
    return sh::set_error(SH_ERR_INVALID, "%s: refused", fn);
}

template <typename T, int NCH>
int firp_launch(const Firp& g, dim3 grid, size_t lds, hipStream_t st) {
#ifdef SH_FIRP_STAGE_F32
    if (lds > 65536) {                                          // (the diagnostic build alone stages more than 64 KB)
        hipError_t e = hipFuncSetAttribute((const void*)k_firp<T, NCH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return sh::hip_error(e, "k_firp");
    }
#endif
    hipLaunchKernelGGL((k_firp<T, NCH>), grid, dim3(256), lds, st, g);
    return launch_result("k_firp");
}

template <typename T>
int resample_run(const sh_buf* in, size_t in_off, uint64_t in_frames, int nch, const sh_buf* taps, size_t taps_off, uint32_t ntaps, uint32_t up, uint32_t down,
                 uint32_t delay, double factor, uint64_t first, uint64_t nframes, sh_buf* out, size_t out_off) {
    const shpr::Plan pl = shpr::plan(ntaps, up, down, delay, (uint32_t)sizeof(typename Staged<T>::type));
    const size_t row_bytes = (size_t)pl.chunks * pl.steps * shpr::LANE_OUTPUTS * sizeof(double);
    int rc = sh::ensure_scratch(row_bytes + (size_t)pl.chunks * sizeof(uint32_t));
    if (rc) return rc;
    hipStream_t st = sh::state().stream;
    Rows r{};
    r.taps = (const char*)taps->ptr + taps_off, r.rows = (double*)sh::state().scratch, r.E = (uint32_t*)((char*)sh::state().scratch + row_bytes);
    r.m = ntaps, r.L = up, r.M = down, r.delay = delay, r.P = pl.P, r.chunks = pl.chunks, r.steps = pl.steps;
    hipLaunchKernelGGL(k_firp_rows, sh::grid1d(row_bytes / sizeof(double), 256), dim3(256), 0, st, r);
    SH_CHECK_LAUNCH("k_firp_rows");
    Firp g{};
    g.in = (const char*)in->ptr + in_off, g.rows = r.rows, g.E = r.E, g.out = (char*)out->ptr + out_off;
    g.n = in_frames, g.first = first, g.count = nframes, g.g_first = shpr::first_group(first, pl), g.g_last = (first + nframes - 1) / pl.P;
    g.nwg = shpr::workgroups_of(first, nframes, pl), g.pl = pl, g.factor = factor;
    dim3 grid = sh::grid1d(g.nwg, 1);
    grid.z = nch;
    const size_t lds = (size_t)pl.staged * sizeof(typename Staged<T>::type);
    return nch == 1 ? firp_launch<T, 1>(g, grid, lds, st) : firp_launch<T, 2>(g, grid, lds, st);
}
}  // namespace

extern "C" {

uint64_t sh_pcm_resample_fir_frames(uint64_t in_frames, uint32_t up, uint32_t down) { return shpr::result_frames(in_frames, up, down); }

int sh_pcm_resample_fir(const sh_buf* in, size_t in_off, uint64_t in_frames, int nch, int width, const sh_buf* taps, size_t taps_off, uint32_t ntaps, uint32_t up,
                        uint32_t down, uint32_t delay, double factor, uint64_t first, uint64_t nframes, sh_buf* out, size_t out_off) {
    SH_REQUIRE_INIT();
    if (!in || !taps || !out) return sh::set_error(SH_ERR_INVALID, "sh_pcm_resample_fir: NULL buffer");
    const shpr::Operand a{(uint64_t)(uintptr_t)in->ptr, in->bytes, in_off}, h{(uint64_t)(uintptr_t)taps->ptr, taps->bytes, taps_off},
        o{(uint64_t)(uintptr_t)out->ptr, out->bytes, out_off};
    int rc = refuse(shpr::check(width, nch, in_frames, ntaps, up, down, delay, factor, first, nframes, a, h, o), nch, width, in_frames, ntaps, up, down, delay,
                    factor, first, nframes);
    if (rc || !nframes) return rc;                            // an empty window: nothing launched
    if (width == 1) return resample_run<signed char>(in, in_off, in_frames, nch, taps, taps_off, ntaps, up, down, delay, factor, first, nframes, out, out_off);
    return resample_run<short>(in, in_off, in_frames, nch, taps, taps_off, ntaps, up, down, delay, factor, first, nframes, out, out_off);
}

}  // extern "C"
