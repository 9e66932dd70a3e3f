// pcm_limit.hip -- sh_pcm_limit: a look-ahead peak limiter over PCM in device memory, exact in integers (pcmlimit.hpp has the contract:
// the gain curve, the wall, the reach, the refusals, and how a call is divided into tiles, tile summaries and carries).  Two launches
// and no grid-wide sync: k_limit_tiles<T, NCH> writes two summaries per tile into the library's scratch, each with one writer;
// k_limit_apply<T, NCH, GAIN> folds the carries of the tiles around its own, scans its own tile and writes it.  No atomics, no
// memset, no float.  A lane owns eight consecutive frames.  Where an operand's base allows it, a lane whose run lies whole inside the
// tile and the sample moves it as one aligned vector; every other sample goes singly through a type of alignment 1, so an operand may
// begin at any byte.  Neither kernel reads outside [0, n) or writes outside the window, and k_limit_apply reads no frame of x outside
// its own tile and every lane reads its run before it writes it: out may be exactly the window's own bytes of x.
#include "common.hpp"
#include "pcmhost.hpp"
#include "pcmlimit.hpp"

namespace {

constexpr int R = (int)shpl::LANE_FRAMES;
constexpr uint32_t T_FRAMES = shpl::TILE_FRAMES;
constexpr uint32_t WAVE_FRAMES = 64 * shpl::LANE_FRAMES;
static_assert(R == 8 && T_FRAMES == 2048, "256 lanes of eight frames");

// a value that may lie at any byte
template <typename T> struct Unaligned { typedef T type __attribute__((aligned(1))); };
// a lane's run of eight frames where it may move as a whole: 8, 16, 32 or 64 bytes
template <typename T, int NCH> constexpr size_t run_align() { return sizeof(T) * NCH * R < 16 ? 8 : 16; }
template <typename T, int NCH> struct alignas(run_align<T, NCH>()) Run { T v[R * NCH]; };

struct Limit {
    const void* in;            // frame 0 of x: n frames of NCH channels
    void*       out;           // frame `first` of the result, or NULL
    void*       gain;          // G[first] of the gain plane (GAIN)
    uint32_t*   fs;            // FS and BS of tiles [plan.sum_first, +plan.sum_count), indexed from plan.sum_first
    uint32_t*   bs;
    uint64_t    n, first, count;
    shpl::Plan  plan;
    uint32_t    ceiling;
    uint32_t    in_vec, out_vec;   // whole runs of x / of the result lie at multiples of run_align
};

__device__ __forceinline__ uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = umin32(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}

// The lane's run: frames [i0, i0 + R) of x, `valid` of them inside [0, n) (the others read as 0), and their required gains (ONE there).
template <typename T, int NCH>
__device__ __forceinline__ void load_run(const Limit& g, uint64_t i0, uint32_t valid, int32_t (&x)[R * NCH], uint32_t (&need)[R]) {
    typedef typename Unaligned<T>::type U;
    if (g.in_vec && valid == (uint32_t)R) {
        const Run<T, NCH> run = *reinterpret_cast<const Run<T, NCH>*>((const T*)g.in + i0 * NCH);
#pragma unroll
        for (int k = 0; k < R * NCH; ++k) x[k] = (int32_t)run.v[k];
    } else {
        const U* p = (const U*)g.in + i0 * NCH;
#pragma unroll
        for (int k = 0; k < R * NCH; ++k) x[k] = (uint32_t)(k / NCH) < valid ? (int32_t)p[k] : 0;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        uint32_t peak = shpl::magnitude(x[r * NCH]);
        if (NCH == 2) peak = peak > shpl::magnitude(x[r * NCH + 1]) ? peak : shpl::magnitude(x[r * NCH + 1]);
        need[r] = shpl::required_gain(peak, g.ceiling);          // (the division only where peak > ceiling)
    }
}

__device__ __forceinline__ uint32_t valid_frames(uint64_t i0, uint64_t n) { return i0 >= n ? 0u : n - i0 < (uint64_t)R ? (uint32_t)(n - i0) : (uint32_t)R; }

// One workgroup: the two summaries of tile plan.sum_first + block_id (pcmlimit.hpp).  A frame at unity adds nothing to either.
template <typename T, int NCH>
__global__ __launch_bounds__(256) void k_limit_tiles(const Limit g) {
    __shared__ uint32_t part[2][4];
    const uint64_t idx = sh::block_id();
    if (idx >= g.plan.sum_count) return;
    const uint32_t lane = threadIdx.x, q0 = lane * R;
    const uint64_t i0 = (g.plan.sum_first + idx) * T_FRAMES + q0;
    int32_t x[R * NCH];
    uint32_t need[R];
    load_run<T, NCH>(g, i0, valid_frames(i0, g.n), x, need);
    uint32_t fs = shpl::ONE, bs = shpl::ONE;
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (need[r] < shpl::ONE) {
            fs = umin32(fs, shpl::ramp(need[r], T_FRAMES - 1 - q0 - r, g.plan.s_r));
            bs = umin32(bs, shpl::ramp(need[r], q0 + r, g.plan.s_a));
        }
    fs = wave_min(fs), bs = wave_min(bs);
    if ((lane & 63) == 0) part[0][lane >> 6] = fs, part[1][lane >> 6] = bs;
    __syncthreads();
    if (lane == 0) {
        g.fs[idx] = umin32(umin32(part[0][0], part[0][1]), umin32(part[0][2], part[0][3]));
        g.bs[idx] = umin32(umin32(part[1][0], part[1][1]), umin32(part[1][2], part[1][3]));
    }
}

// One workgroup: tile u = plan.apply_first + block_id of the window.  The carries CF (at the tile's first frame) and CB (at its last)
// are folded from up to 512 summaries a side, two a lane.  The tile's own curves are prefix minima in three levels, as osc_scan.hip's
// sums are: a lane's run in registers, the wave's lanes by shuffles (a distance of d lanes is 8 d frames for every lane, so the ramp
// between two partial results is one wave-uniform number, capped), the four waves through LDS behind the one barrier, which the
// carries' partial minima share.  Every value is capped at ONE at every step and so stays in 32 bits; only distances times slopes
// are formed in 64.
template <typename T, int NCH, bool GAIN>
__global__ __launch_bounds__(256) void k_limit_apply(const Limit g) {
    __shared__ uint32_t part[4][4];                             // per wave: CF's and CB's partial minimum, the wave's own F at its last frame, its B at its first
    const uint64_t idx = sh::block_id();
    if (idx >= g.plan.apply_count) return;
    const uint64_t u = g.plan.apply_first + idx;
    const uint32_t lane = threadIdx.x, wave = lane >> 6, wl = lane & 63, q0 = lane * R;
    const uint32_t s_a = g.plan.s_a, s_r = g.plan.s_r;
    const uint64_t behind = u - g.plan.sum_first, ahead = g.plan.sum_first + g.plan.sum_count - 1 - u;      // summaries held on either side
    uint32_t cf = shpl::ONE, cb = shpl::ONE;
    for (uint64_t k = lane + 1; k <= g.plan.carry_r && k <= behind; k += 256) cf = umin32(cf, shpl::ramp(g.fs[behind - k], shpl::carry_distance(k), s_r));
    for (uint64_t k = lane + 1; k <= g.plan.carry_a && k <= ahead; k += 256) cb = umin32(cb, shpl::ramp(g.bs[behind + k], shpl::carry_distance(k), s_a));
    cf = wave_min(cf), cb = wave_min(cb);

    const uint64_t i0 = u * T_FRAMES + q0;
    int32_t x[R * NCH];
    uint32_t G[R];
    load_run<T, NCH>(g, i0, valid_frames(i0, g.n), x, G);       // (G holds g for now)

    // the lane's own run: its release curve at its last frame, its attack curve at its first
    uint32_t xf = G[0], xb = G[R - 1];
#pragma unroll
    for (int r = 1; r < R; ++r) xf = umin32(G[r], shpl::step(xf, s_r)), xb = umin32(G[R - 1 - r], shpl::step(xb, s_a));
    // the wave: after the step of d lanes, xf holds the curve of the 2 d lanes up to this one, xb of the 2 d lanes from this one on
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t far_r = shpl::ramp(0, (uint64_t)d * R, s_r), far_a = shpl::ramp(0, (uint64_t)d * R, s_a);
        const uint32_t yf = (uint32_t)__shfl_up((int)xf, d, 64), yb = (uint32_t)__shfl_down((int)xb, d, 64);
        if (wl >= (uint32_t)d) xf = umin32(xf, shpl::cap((uint64_t)yf + far_r));
        if (wl + d < 64) xb = umin32(xb, shpl::cap((uint64_t)yb + far_a));
    }
    const uint32_t prev_f = (uint32_t)__shfl_up((int)xf, 1, 64), next_b = (uint32_t)__shfl_down((int)xb, 1, 64);
    if (wl == 0) part[wave][0] = cf, part[wave][1] = cb, part[wave][3] = xb;
    if (wl == 63) part[wave][2] = xf;
    __syncthreads();
    cf = umin32(umin32(part[0][0], part[1][0]), umin32(part[2][0], part[3][0]));
    cb = umin32(umin32(part[0][1], part[1][1]), umin32(part[2][1], part[3][1]));
    // everything in front of this wave, at the wave's first frame; everything behind it, at its last
    uint32_t wf = shpl::ramp(cf, (uint64_t)wave * WAVE_FRAMES, s_r), wb = shpl::ramp(cb, (uint64_t)(3 - wave) * WAVE_FRAMES, s_a);
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
        if (w < wave) wf = umin32(wf, shpl::ramp(part[w][2], (uint64_t)(wave - w - 1) * WAVE_FRAMES + 1, s_r));
        if (w > wave) wb = umin32(wb, shpl::ramp(part[w][3], (uint64_t)(w - wave - 1) * WAVE_FRAMES + 1, s_a));
    }
    // everything in front of this lane, at its first frame; everything behind it, at its last
    uint32_t f = shpl::ramp(wf, (uint64_t)wl * R, s_r), b = shpl::ramp(wb, (uint64_t)(63 - wl) * R, s_a);
    if (wl > 0) f = umin32(f, shpl::step(prev_f, s_r));
    if (wl < 63) b = umin32(b, shpl::step(next_b, s_a));
    uint32_t F[R];
#pragma unroll
    for (int r = 0; r < R; ++r) f = umin32(G[r], f), F[r] = f, f = shpl::step(f, s_r);
#pragma unroll
    for (int r = R - 1; r >= 0; --r) b = umin32(G[r], b), G[r] = umin32(F[r], b), b = shpl::step(b, s_a);

    // the window's frames of the run: [lo, hi) of its eight
    const uint64_t w_end = g.first + g.count;
    const uint32_t lo = i0 >= g.first ? 0u : g.first - i0 < (uint64_t)R ? (uint32_t)(g.first - i0) : (uint32_t)R;
    const uint32_t hi = i0 >= w_end ? 0u : w_end - i0 < (uint64_t)R ? (uint32_t)(w_end - i0) : (uint32_t)R;
    if (lo >= hi) return;
    if (g.out) {
        typedef typename Unaligned<T>::type U;
        if (g.out_vec && lo == 0 && hi == (uint32_t)R) {
            Run<T, NCH> run;
#pragma unroll
            for (int k = 0; k < R * NCH; ++k) run.v[k] = (T)shpl::apply_gain(x[k], G[k / NCH]);
            *reinterpret_cast<Run<T, NCH>*>((T*)g.out + (i0 - g.first) * NCH) = run;
        } else {
            U* p = (U*)g.out + (int64_t)(i0 - g.first) * NCH;   // (not dereferenced below lo)
#pragma unroll
            for (int k = 0; k < R * NCH; ++k)
                if ((uint32_t)(k / NCH) >= lo && (uint32_t)(k / NCH) < hi) p[k] = (T)shpl::apply_gain(x[k], G[k / NCH]);
        }
    }
    if (GAIN) {
        Unaligned<uint32_t>::type* p = (Unaligned<uint32_t>::type*)g.gain + (int64_t)(i0 - g.first);
#pragma unroll
        for (int r = 0; r < R; ++r)
            if ((uint32_t)r >= lo && (uint32_t)r < hi) p[r] = G[r];
    }
}

int refuse(shpl::Refusal why, int nch, int width, uint64_t in_frames, uint32_t ceiling, uint32_t attack, uint32_t release, uint64_t first, uint64_t nframes) {
    const char* fn = "sh_pcm_limit";
    switch (why) {
    case shpl::OK: return SH_OK;
    case shpl::BAD_WIDTH: return sh::set_error(SH_ERR_INVALID, "%s: sample width %d not in {1,2,4} (width 3 is not built)", fn, width);
    case shpl::BAD_CHANNELS: return sh::set_error(SH_ERR_INVALID, "%s: %d channels (1 or 2)", fn, nch);
    case shpl::BAD_CEILING: return sh::set_error(SH_ERR_INVALID, "%s: a ceiling of %u is not in [1, %u]", fn, ceiling, shpl::hi_of(width));
    case shpl::BAD_ATTACK: return sh::set_error(SH_ERR_INVALID, "%s: an attack of %u frames is more than %u", fn, attack, shpl::MAX_FRAMES);
    case shpl::BAD_RELEASE: return sh::set_error(SH_ERR_INVALID, "%s: a release of %u frames is more than %u", fn, release, shpl::MAX_FRAMES);
    case shpl::BAD_WINDOW:
        return sh::set_error(SH_ERR_INVALID, "%s: frames [%llu, +%llu) reach past the sample's %llu", fn, (unsigned long long)first, (unsigned long long)nframes,
                             (unsigned long long)in_frames);
    case shpl::IN_RANGE: return sh::set_error(SH_ERR_INVALID, "%s: input range outside buffer", fn);
    case shpl::OUT_RANGE: return sh::set_error(SH_ERR_INVALID, "%s: output range outside buffer", fn);
    case shpl::GAIN_RANGE: return sh::set_error(SH_ERR_INVALID, "%s: gain range outside buffer", fn);
    case shpl::OUT_OVERLAP: return sh::set_error(SH_ERR_INVALID, "%s: out overlaps the input and is not the window's own bytes", fn);
    case shpl::GAIN_OVERLAP: return sh::set_error(SH_ERR_INVALID, "%s: gain overlaps the input or out", fn);
    case shpl::NO_DESTINATION: return sh::set_error(SH_ERR_INVALID, "%s: neither out nor gain", fn);
    }
    return sh::set_error(SH_ERR_INVALID, "%s: refused", fn);
}

template <typename T, int NCH>
int limit_run(Limit g) {
    // whole runs begin at multiples of eight frames of x; of the result they begin `first` frames earlier
    const uint64_t align = run_align<T, NCH>(), fb = sizeof(T) * NCH;
    g.in_vec = (uint64_t)(uintptr_t)g.in % align == 0;
    g.out_vec = g.out && ((uint64_t)(uintptr_t)g.out % align + align - g.first * fb % align) % align == 0;
    int rc = sh::ensure_scratch((size_t)g.plan.sum_count * 2 * sizeof(uint32_t));
    if (rc) return rc;
    g.fs = (uint32_t*)sh::state().scratch, g.bs = g.fs + g.plan.sum_count;
    hipStream_t st = sh::state().stream;
    hipLaunchKernelGGL((k_limit_tiles<T, NCH>), sh::grid1d(g.plan.sum_count, 1), dim3(256), 0, st, g);
    SH_CHECK_LAUNCH("k_limit_tiles");
    if (g.gain) hipLaunchKernelGGL((k_limit_apply<T, NCH, true>), sh::grid1d(g.plan.apply_count, 1), dim3(256), 0, st, g);
    else hipLaunchKernelGGL((k_limit_apply<T, NCH, false>), sh::grid1d(g.plan.apply_count, 1), dim3(256), 0, st, g);
    return launch_result("k_limit_apply");
}
}  // namespace

extern "C" {

int sh_pcm_limit(const sh_buf* in, size_t in_off, uint64_t in_frames, int nch, int width, uint32_t ceiling, uint32_t attack_frames, uint32_t release_frames,
                 uint64_t first, uint64_t nframes, sh_buf* out, size_t out_off, sh_buf* gain, size_t gain_off) {
    SH_REQUIRE_INIT();
    if (!in) return sh::set_error(SH_ERR_INVALID, "sh_pcm_limit: NULL buffer");
    const shpl::Operand a{(uint64_t)(uintptr_t)in->ptr, in->bytes, in_off, true};
    const shpl::Operand o{out ? (uint64_t)(uintptr_t)out->ptr : 0, out ? out->bytes : 0, out_off, out != nullptr};
    const shpl::Operand p{gain ? (uint64_t)(uintptr_t)gain->ptr : 0, gain ? gain->bytes : 0, gain_off, gain != nullptr};
    int rc = refuse(shpl::check(width, nch, in_frames, ceiling, attack_frames, release_frames, first, nframes, a, o, p), nch, width, in_frames, ceiling,
                    attack_frames, release_frames, first, nframes);
    if (rc || !nframes) return rc;                            // an empty window: nothing launched
    Limit g{};
    g.in = (const char*)in->ptr + in_off;
    g.out = out ? (char*)out->ptr + out_off : nullptr, g.gain = gain ? (char*)gain->ptr + gain_off : nullptr;
    g.n = in_frames, g.first = first, g.count = nframes, g.ceiling = ceiling;
    g.plan = shpl::plan(in_frames, attack_frames, release_frames, first, nframes);
    return dispatch_width(width, [&](auto t) {
        typedef decltype(t) T;
        return nch == 1 ? limit_run<T, 1>(g) : limit_run<T, 2>(g);
    });
}

}  // extern "C"
