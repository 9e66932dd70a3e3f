// pcm_fir.hip -- sh_pcm_convolve: a finite impulse response over PCM in device memory, in the direct form, exact to the last bit
// (pcmfir.hpp has the contract: the refusals, the result's length, the bound that makes a float64 FMA chain the exact integer sum, the
// one rounding, and how a call is divided into tiles and chunks).  Two kernels: k_fir_taps turns the response into float64 planes in
// the library's scratch, k_fir<T, NCH> computes one tile of output frames of one channel per workgroup.  No atomics; every sample of
// x, of the response and of the result is read and written as one sample through a type of alignment 1 (Unaligned<T>), so an operand
// may begin at any byte -- a DeviceBuffer.view at an odd one included -- and there is no vector body with a scalar head and tail.
// Built with -ffp-contract=off like the rest: fma() where it is written and nowhere else.
#include "common.hpp"
#include "pcmdev.hpp"
#include "pcmhost.hpp"
#include "pcmfir.hpp"

namespace {

// a sample that may lie at any byte
template <typename T> struct Unaligned { typedef T type __attribute__((aligned(1))); };

// the response as float64: plane c holds channel c's m taps and zeros behind them up to m8 (a zero tap adds exactly nothing)
template <typename T>
__global__ __launch_bounds__(256) void k_fir_taps(const typename Unaligned<T>::type* __restrict__ ir, uint32_t m, uint32_t m8, uint32_t hch, double* __restrict__ taps) {
    const size_t i = sh::block_id() * 256 + threadIdx.x;
    if (i >= (size_t)m8 * hch) return;
    const uint32_t c = (uint32_t)(i / m8), k = (uint32_t)(i % m8);
    taps[i] = k < m ? (double)ir[(size_t)k * hch + c] : 0.0;
}

struct Fir {
    const void*   in;          // x: n frames of NCH channels
    const double* taps;        // k_fir_taps' planes
    void*         out;         // frame `first` of the result
    uint64_t      n, first, count, ntiles;
    uint32_t      m8;          // taps per plane (padded)
    uint32_t      plane;       // channel c reads plane c: m8 apart, or 0 apart where one response serves both channels
    double        factor;
};

// One workgroup: tile blockIdx.(x, y) of channel blockIdx.z.  Lane l owns frames [R l, R l + R) of the tile (R = LANE_FRAMES = 8) and
// keeps their R sums and a window of x in registers.  Per group of R taps k .. k + R - 1 the sums need x at 2 R - 1 consecutive
// frames; the upper R - 1 are the lower R - 1 of the group before, so a group reads R new values from the staged span -- one LDS read
// per tap and lane for R FMAs -- and with the group loop unrolled by two the window turns by renaming, not by moves.  The taps are
// wave-uniform operands (scalar loads, sixteen taps to a batch).
template <typename T, int NCH>
__global__ __launch_bounds__(256) void k_fir(const Fir g) {
    constexpr int R = (int)shpf::LANE_FRAMES;
    static_assert(R == (int)shpf::TAP_UNROLL, "a group of taps is as long as a lane's run of frames");
    __shared__ double staged[shpf::STAGED_DOUBLES];
    const uint64_t tile = sh::block_id();
    if (tile >= g.ntiles) return;
    const uint32_t c = blockIdx.z;
    typedef typename Unaligned<T>::type U;
    const U* __restrict__ x = (const U*)g.in + c;
    const double* __restrict__ taps = g.taps + (size_t)c * g.plane;
    const int64_t tile_first = (int64_t)(g.first + tile * shpf::TILE_FRAMES);
    const int64_t n = (int64_t)g.n;
    const uint32_t lane = threadIdx.x;
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0;
    for (uint32_t k0 = 0; k0 < g.m8; k0 += shpf::TAP_CHUNK) {
        const uint32_t kc = g.m8 - k0 < shpf::TAP_CHUNK ? g.m8 - k0 : shpf::TAP_CHUNK, span = shpf::TILE_FRAMES + kc - 1;
        const int64_t base = tile_first - (int64_t)k0 - (int64_t)kc + 1;
        if (base >= n || base + (int64_t)span <= 0) continue;   // (the same for the whole workgroup) nothing of x under this chunk
        __syncthreads();                                        // the chunk before has been read
        for (uint32_t j = lane; j < span; j += 256) {
            const int64_t f = base + (int64_t)j;
            staged[shpf::staged_at(j)] = f >= 0 && f < n ? (double)x[(size_t)f * NCH] : 0.0;      // no address outside [0, n) is formed
        }
        __syncthreads();
        // v[q] = staged frame q0 + q, q = 0 .. 2 R - 2, of the group of taps kk .. kk + R - 1; frame r under tap kk + u reads
        // v[r - u + R - 1].  q0 is a multiple of R: the R low values lie side by side (staged_at)
        const double* lo_at = staged + shpf::staged_at(lane * R + kc - R);
        double lo[R], hi[R - 1];
#pragma unroll
        for (int q = 0; q < R - 1; ++q) hi[q] = lo_at[R + 1 + q];
        const double* h = taps + k0;
#pragma unroll 2
        for (uint32_t kk = 0; kk < kc; kk += R, lo_at -= R + 1, h += R) {
#pragma unroll
            for (int q = 0; q < R; ++q) lo[q] = lo_at[q];
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const double hu = h[u];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int q = r - u + R - 1;
                    acc[r] = fma(hu, q < R ? lo[q] : hi[q - R], acc[r]);
                }
            }
#pragma unroll
            for (int q = 0; q < R - 1; ++q) hi[q] = lo[q];
        }
    }
    U* out = (U*)g.out + c;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint64_t i = (uint64_t)tile * shpf::TILE_FRAMES + lane * R + r;      // from `first` on
        if (i < g.count) out[(size_t)i * NCH] = (T)fbound(acc[r] * g.factor, Lim<T>::lo, Lim<T>::hi);
    }
}

int refuse(shpf::Refusal why, int nch, int width, int ir_nch, uint64_t in_frames, uint32_t ir_frames, double factor, uint64_t first, uint64_t nframes) {
    const char* fn = "sh_pcm_convolve";
    switch (why) {
    case shpf::OK: return SH_OK;
    case shpf::BAD_WIDTH: return sh::set_error(SH_ERR_INVALID, "%s: sample width %d not in {1,2} (widths 3 and 4 are not built)", fn, width);
    case shpf::BAD_CHANNELS: return sh::set_error(SH_ERR_INVALID, "%s: %d channels (1 or 2)", fn, nch);
    case shpf::BAD_IR_CHANNELS: return sh::set_error(SH_ERR_INVALID, "%s: a response of %d channels over %d (1, or as many)", fn, ir_nch, nch);
    case shpf::NO_TAPS: return sh::set_error(SH_ERR_INVALID, "%s: an empty response", fn);
    case shpf::TOO_MANY_TAPS: return sh::set_error(SH_ERR_INVALID, "%s: %u taps are more than %u: the sum would not be exact", fn, ir_frames, shpf::MAX_TAPS);
    case shpf::BAD_FACTOR: return sh::set_error(SH_ERR_INVALID, "%s: the factor %g is not finite", fn, factor);
    case shpf::BAD_WINDOW:
        return sh::set_error(SH_ERR_INVALID, "%s: frames [%llu, +%llu) reach past the result's %llu", fn, (unsigned long long)first, (unsigned long long)nframes,
                             (unsigned long long)shpf::result_frames(in_frames, ir_frames));
    case shpf::IN_RANGE: return sh::set_error(SH_ERR_INVALID, "%s: input range outside buffer", fn);
    case shpf::IR_RANGE: return sh::set_error(SH_ERR_INVALID, "%s: response range outside buffer", fn);
    case shpf::OUT_RANGE: return sh::set_error(SH_ERR_INVALID, "%s: output range outside buffer", fn);
    case shpf::OVERLAP: return sh::set_error(SH_ERR_INVALID, "%s: out overlaps an input", fn);
    }
    return sh::set_error(SH_ERR_INVALID, "%s: refused", fn);
}

template <typename T>
int convolve_run(const sh_buf* in, size_t in_off, uint64_t in_frames, int nch, const sh_buf* ir, size_t ir_off, uint32_t ir_frames, int ir_nch,
                 double factor, uint64_t first, uint64_t nframes, sh_buf* out, size_t out_off) {
    const uint32_t m8 = shpf::padded_taps(ir_frames);
    int rc = sh::ensure_scratch((size_t)m8 * ir_nch * sizeof(double));
    if (rc) return rc;
    hipStream_t st = sh::state().stream;
    double* taps = (double*)sh::state().scratch;
    hipLaunchKernelGGL(k_fir_taps<T>, sh::grid1d((size_t)m8 * ir_nch, 256), dim3(256), 0, st, (const typename Unaligned<T>::type*)((const char*)ir->ptr + ir_off), ir_frames, m8,
                       (uint32_t)ir_nch, taps);
    SH_CHECK_LAUNCH("k_fir_taps");
    Fir g{};
    g.in = (const char*)in->ptr + in_off, g.taps = taps, g.out = (char*)out->ptr + out_off;
    g.n = in_frames, g.first = first, g.count = nframes, g.ntiles = shpf::tiles_of(nframes);
    g.m8 = m8, g.plane = ir_nch == 2 ? m8 : 0, g.factor = factor;
    dim3 grid = sh::grid1d(g.ntiles, 1);
    grid.z = nch;
    if (nch == 1) hipLaunchKernelGGL((k_fir<T, 1>), grid, dim3(256), 0, st, g);
    else hipLaunchKernelGGL((k_fir<T, 2>), grid, dim3(256), 0, st, g);
    return launch_result("k_fir");
}
}  // namespace

extern "C" {

int sh_pcm_convolve(const sh_buf* in, size_t in_off, uint64_t in_frames, int nch, int width, const sh_buf* ir, size_t ir_off, uint32_t ir_frames,
                    int ir_nch, double factor, uint64_t first, uint64_t nframes, sh_buf* out, size_t out_off) {
    SH_REQUIRE_INIT();
    if (!in || !ir || !out) return sh::set_error(SH_ERR_INVALID, "sh_pcm_convolve: NULL buffer");
    const shpf::Operand a{(uint64_t)(uintptr_t)in->ptr, in->bytes, in_off}, h{(uint64_t)(uintptr_t)ir->ptr, ir->bytes, ir_off},
        o{(uint64_t)(uintptr_t)out->ptr, out->bytes, out_off};
    int rc = refuse(shpf::check(width, nch, ir_nch, in_frames, ir_frames, factor, first, nframes, a, h, o), nch, width, ir_nch, in_frames, ir_frames, factor,
                    first, nframes);
    if (rc || !nframes) return rc;                            // an empty window: nothing launched
    if (width == 1) return convolve_run<signed char>(in, in_off, in_frames, nch, ir, ir_off, ir_frames, ir_nch, factor, first, nframes, out, out_off);
    return convolve_run<short>(in, in_off, in_frames, nch, ir, ir_off, ir_frames, ir_nch, factor, first, nframes, out, out_off);
}

}  // extern "C"
