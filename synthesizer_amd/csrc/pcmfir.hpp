// pcmfir.hpp -- a finite impulse response over PCM that already lies in device memory (sh_pcm_convolve, pcm_fir.hip): the contract of
// the call, stated once -- what is refused, how long the result is, the one rounding, how the kernel divides the work -- and the whole
// call as a host loop that divides it the same way.
// The input x: n frames of nch (1 or 2) interleaved channels of w (1 or 2) bytes.  The response h: m frames of hch channels of the
// same width; hch == 1 applies the one response to every channel of x, hch == 2 needs nch == 2 and applies the left response to the
// left channel and the right one to the right.  The result: result_frames(n, m) = n + m - 1 frames (0 when n == 0) of nch channels,
// for channel c and frame i
//     acc = sum over k in [0, m) of h_c[k] * x_c[i - k],     samples of x outside [0, n) counting as 0,
// the EXACT integer, and then ONE rounding: the sample is scale(acc, factor, w) = fbound((double)acc * factor) -- one float64 multiply
// of a value that converts exactly, above HI gives HI, below LO + 1.0 gives LO, otherwise floor: audioop.mul's last step, applied to
// the exact sum (the kernel takes pcmdev.hpp's fbound for it; this header states it for the host).
// A call computes frames [first, first + count) of the result, and those bytes are that slice of the whole result's bytes.
// Plain C++17, no intrinsics, SH_HD (tests/cpu_pcmfir.cpp builds it with g++).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifndef SH_HD
#if defined(__HIPCC__)
#define SH_HD __host__ __device__ __forceinline__
#else
#define SH_HD static inline
#endif
#endif

namespace shpf {

// Why float64 is exact here.  A sample of 1 or 2 bytes has a magnitude of at most 2^15, a product of two of at most 2^30.  With
// m <= MAX_TAPS = 2^22 terms, |acc| <= m * 2^30 <= 2^52 -- and so is every partial sum over ANY subset of the terms taken in ANY
// order: an integer of a magnitude below 2^53.  Every such integer is a float64, a product of two samples is one, and an FMA rounds
// once, the exact value h * x + partial, which is such an integer again: nothing is ever rounded.  Hence an FMA chain in float64 IS the
// integer sum, and the bytes of the result are the same for every tile, chunk, window, order of the taps and run.
constexpr uint32_t MAX_TAPS = 1u << 22;

// How the kernel divides a call (exported as N.PCM_FIR_TILE_FRAMES and N.PCM_FIR_TAP_CHUNK: the tests are sized from them).  A
// workgroup of 256 lanes computes one TILE of output frames of one channel, tile t of a call being frames [first + t * TILE_FRAMES,
// ...) cut to the window; a lane owns LANE_FRAMES consecutive frames of it.  The taps -- padded with zeros to a multiple of
// TAP_UNROLL, a zero tap adding exactly nothing -- are walked in chunks of TAP_CHUNK; per chunk of kc taps from tap k0 on the tile
// needs the span of x from frame tile_first - k0 - kc + 1 on, TILE_FRAMES + kc - 1 frames, which is staged once as float64.
// LANE_FRAMES = 8 and TAP_CHUNK = 1024 are the shape the arithmetic suggests (one LDS read per eight FMAs; 27 KB of LDS, five
// workgroups a CU); profiles/convolve_ab.txt holds what has been measured of it and of the others.  A diagnostic build may name
// others (SYNTHHIP_BUILD_FLAGS=-DSH_FIR_LANE_FRAMES=4 -DSH_FIR_TAP_CHUNK=2048), never the shipped library.
#ifndef SH_FIR_LANE_FRAMES
#define SH_FIR_LANE_FRAMES 8
#endif
#ifndef SH_FIR_TAP_CHUNK
#define SH_FIR_TAP_CHUNK 1024
#endif
constexpr uint32_t LANE_FRAMES = SH_FIR_LANE_FRAMES;
constexpr uint32_t TILE_FRAMES = 256 * LANE_FRAMES;
constexpr uint32_t TAP_UNROLL = LANE_FRAMES;                    // a lane's window of x turns once per group of taps
constexpr uint32_t TAP_CHUNK = SH_FIR_TAP_CHUNK;
static_assert(TAP_CHUNK % TAP_UNROLL == 0 && (LANE_FRAMES == 4 || LANE_FRAMES == 8), "groups of four or eight taps, whole groups per chunk");

SH_HD uint32_t padded_taps(uint32_t m) { return (m + TAP_UNROLL - 1) / TAP_UNROLL * TAP_UNROLL; }

// where frame j of a staged span lies: one float64 of padding behind every LANE_FRAMES, so that the lanes of a wave, which read
// LANE_FRAMES frames apart, read 18 dwords apart (10 with four frames to a lane) and by that arithmetic meet no bank twice (not measured)
SH_HD uint32_t staged_at(uint32_t j) { return j + j / LANE_FRAMES; }
constexpr uint32_t STAGED_DOUBLES = (TILE_FRAMES + TAP_CHUNK - 2) + (TILE_FRAMES + TAP_CHUNK - 2) / LANE_FRAMES + 1;

SH_HD uint64_t result_frames(uint64_t n, uint64_t m) { return n ? n + m - 1 : 0; }

// the limits of a width's samples
SH_HD double rail_lo(int w) { return w == 1 ? -128.0 : -32768.0; }
SH_HD double rail_hi(int w) { return w == 1 ? 127.0 : 32767.0; }

// the one rounding: audioop's fbound of the exact sum times the factor
SH_HD int32_t scale(int64_t acc, double factor, int w) {
    double p = (double)acc * factor;
    const double lo = rail_lo(w), hi = rail_hi(w);
    if (p > hi) p = hi;
    else if (p < lo + 1.0) p = lo;
    return (int32_t)std::floor(p);
}

// Every refusal of a call, in the order in which it is looked for.  The operands are byte ranges: a buffer of `bytes` bytes at
// address `addr`, the operand from byte `off` of it on -- any byte: the kernels read and write sample by sample and ask for no alignment.
enum Refusal {
    OK = 0,
    BAD_WIDTH,          // a width other than 1 or 2
    BAD_CHANNELS,       // nch not 1 or 2
    BAD_IR_CHANNELS,    // ir_nch not 1 and not nch
    NO_TAPS,            // m == 0
    TOO_MANY_TAPS,      // m > MAX_TAPS
    BAD_FACTOR,         // a factor that is not finite
    BAD_WINDOW,         // [first, first + count) reaches past result_frames(n, m)
    IN_RANGE,           // x reaches past its buffer
    IR_RANGE,           // h reaches past its buffer
    OUT_RANGE,          // the window reaches past the destination
    OVERLAP,            // the destination's bytes overlap x's or h's
};

struct Operand {
    uint64_t addr, bytes, off;
};

SH_HD bool inside(const Operand& o, uint64_t frames, uint64_t frame_bytes) {
    return o.off <= o.bytes && frames <= (o.bytes - o.off) / frame_bytes;
}

SH_HD bool overlap(const Operand& a, uint64_t a_bytes, const Operand& b, uint64_t b_bytes) {
    const uint64_t a0 = a.addr + a.off, b0 = b.addr + b.off;
    return a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

SH_HD Refusal check(int width, int nch, int ir_nch, uint64_t n, uint64_t m, double factor, uint64_t first, uint64_t count, const Operand& in,
                    const Operand& ir, const Operand& out) {
    if (width != 1 && width != 2) return BAD_WIDTH;
    if (nch != 1 && nch != 2) return BAD_CHANNELS;
    if (ir_nch != 1 && ir_nch != nch) return BAD_IR_CHANNELS;
    if (m == 0) return NO_TAPS;
    if (m > MAX_TAPS) return TOO_MANY_TAPS;
    if (!(factor - factor == 0.0)) return BAD_FACTOR;            // (an infinity or a NaN less itself is a NaN)
    if (n > UINT64_MAX - m) return BAD_WINDOW;
    const uint64_t total = result_frames(n, m);
    if (count > total || first > total - count) return BAD_WINDOW;
    const uint64_t w = (uint64_t)width;
    if (!inside(in, n, w * (uint64_t)nch)) return IN_RANGE;
    if (!inside(ir, m, w * (uint64_t)ir_nch)) return IR_RANGE;
    if (!inside(out, count, w * (uint64_t)nch)) return OUT_RANGE;
    const uint64_t out_bytes = count * w * (uint64_t)nch;
    if (overlap(out, out_bytes, in, n * w * (uint64_t)nch) || overlap(out, out_bytes, ir, m * w * (uint64_t)ir_nch)) return OVERLAP;
    return OK;
}

SH_HD uint64_t tiles_of(uint64_t count) { return (count + TILE_FRAMES - 1) / TILE_FRAMES; }

// One tile of one channel on the host, as a workgroup of the kernel computes it: per chunk of the padded taps the staged span (a frame
// outside [0, n) is 0.0 and is never asked for), per lane LANE_FRAMES sums, every term one fma in float64, the taps in rising order.
// get_x(c, i): sample of frame i, channel c, of x; get_h(c, k): tap k of the response's channel c.  put(c, i, sample): frame i of
// the RESULT, channel c; only frames of the window are put.
template <typename GetX, typename GetH, typename Put>
static inline void host_tile(GetX&& get_x, GetH&& get_h, Put&& put, uint64_t n, uint32_t m, int c, int hc, int w, double factor, uint64_t first,
                             uint64_t count, uint64_t tile) {
    const uint32_t m8 = padded_taps(m);
    const int64_t tile_first = (int64_t)(first + tile * TILE_FRAMES);
    double* staged = new double[STAGED_DOUBLES];
    double* acc = new double[TILE_FRAMES]();
    for (uint32_t k0 = 0; k0 < m8; k0 += TAP_CHUNK) {
        const uint32_t kc = m8 - k0 < TAP_CHUNK ? m8 - k0 : TAP_CHUNK, span = TILE_FRAMES + kc - 1;
        const int64_t base = tile_first - (int64_t)k0 - (int64_t)kc + 1;
        if (base >= (int64_t)n || base + (int64_t)span <= 0) continue;          // nothing of x under this chunk: it adds nothing
        for (uint32_t j = 0; j < span; ++j) {
            const int64_t g = base + (int64_t)j;
            staged[staged_at(j)] = g >= 0 && g < (int64_t)n ? (double)get_x(c, (uint64_t)g) : 0.0;
        }
        for (uint32_t lane = 0; lane < 256; ++lane)
            for (uint32_t kk = 0; kk < kc; ++kk) {
                const double h = k0 + kk < m ? (double)get_h(hc, k0 + kk) : 0.0;
                for (uint32_t r = 0; r < LANE_FRAMES; ++r) {
                    const uint32_t f = lane * LANE_FRAMES + r;
                    acc[f] = std::fma(h, staged[staged_at(f + kc - 1 - kk)], acc[f]);
                }
            }
    }
    for (uint32_t f = 0; f < TILE_FRAMES; ++f) {
        const uint64_t i = (uint64_t)tile_first + f;
        if (i - first < count) put(c, i, scale((int64_t)acc[f], factor, w));
    }
    delete[] acc;
    delete[] staged;
}

// The whole call on the host, tile by tile and chunk by chunk as the kernel divides it: every tile of every channel, in rising order.
template <typename GetX, typename GetH, typename Put>
static inline void host_convolve(GetX&& get_x, GetH&& get_h, Put&& put, uint64_t n, uint32_t m, int nch, int ir_nch, int w, double factor,
                                 uint64_t first, uint64_t count) {
    for (uint64_t tile = 0; tile < tiles_of(count); ++tile)
        for (int c = 0; c < nch; ++c) host_tile(get_x, get_h, put, n, m, c, ir_nch == 2 ? c : 0, w, factor, first, count, tile);
}

}  // namespace shpf
