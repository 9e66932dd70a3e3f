// pcmlimit.hpp -- a look-ahead peak limiter over PCM that already lies in device memory (sh_pcm_limit, pcm_limit.hip): the contract of
// the call, stated once -- the gain curve in integers, what is refused, how the kernels divide the work into tiles, tile summaries and
// carries -- and the whole call as a host loop that divides it the same way.
// The input x: n frames of nch (1 or 2) interleaved channels of w (1, 2 or 4) bytes.  With ONE = 2^30, HI = 2^(8w-1) - 1, the ceiling
// C in [1, HI], a attack frames and r release frames, each at most MAX_FRAMES, per frame i:
//     p[i] = max over the frame's channels of |x[i][c]|                      (|-2^31| is 2^31; the channels are linked: one gain a frame)
//     g[i] = ONE where p[i] <= C, else floor(C * ONE / p[i])                  (the required gain; frames outside [0, n) count as ONE)
//     G[i] = min(ONE, min over j >= i of g[j] + (j - i) * s_a, min over j < i of g[j] + (i - j) * s_r)
//     y[i][c] = (x[i][c] * G[i]) >> 30                                        (the arithmetic shift of the signed 64-bit product: floor)
// s_a = slope(a) and s_r = slope(r), slope(f) = ONE where f <= 1, else ceil(ONE / f): a linear ramp down in front of a peak, a linear
// ramp up behind it.  Integers throughout and no float anywhere; every term of G is below 2^51 (a distance below 2^21 times a slope of
// at most 2^30).  A minimum is associative and commutative, so the bytes depend on x, C, a and r alone: not on tiles, windows, order or run.
//   The wall.  j = i is among the terms, so G[i] <= g[i].  Where p <= C, |x| G / ONE <= |x| <= C.  Where p > C, G <= floor(C ONE / p)
// gives p G <= C ONE: on the positive side floor(x G / ONE) <= x G / ONE <= p G / ONE <= C; on the negative side x >= -p gives
// x G / ONE >= -p G / ONE >= -C, and -C is an integer, so floor(x G / ONE) >= -C as well.  Hence |y| <= C on every sample.
//   Unity.  Where G[i] = ONE, y = (x * 2^30) >> 30 = x: the frame is untouched.
//   The slopes.  Every term of G[i + 1] plus s_a is a term of G[i] or at least ONE (for j >= i + 1 the distance grows by one; for
// j <= i the term g[j] + (i + 1 - j) s_r + s_a is at least g[j] + (i - j) s_r, a term of G[i] -- or g[i] itself for j = i), so
// G[i] - G[i + 1] <= s_a; the mirror image gives G[i + 1] - G[i] <= s_r.
//   The reach.  g >= 0, so a frame at distance d adds a term of at least d * s, and only a term below ONE can lower G: d * s < ONE, which
// is d <= reach(f) - 1 with reach(f) = ceil(ONE / slope(f)) <= max(f, 1) (slope(f) >= ONE / f).  A frame reach(f) or more away changes
// nothing, whatever it holds.
// A call computes frames [first, first + count) of the result, and those bytes are that slice of the whole result's bytes: peaks that
// lie outside the window shape the gain inside it.  The result has n frames.
// Plain C++17, no intrinsics, SH_HD (tests/cpu_pcmlimit.cpp builds it with g++).
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef SH_HD
#if defined(__HIPCC__)
#define SH_HD __host__ __device__ __forceinline__
#else
#define SH_HD static inline
#endif
#endif

namespace shpl {

constexpr uint32_t ONE = 1u << 30;
constexpr uint32_t MAX_FRAMES = 1u << 20;                       // of attack and of release: 21.8 s at 48 kHz

// How the kernels divide a call (exported as N.PCM_LIMIT_TILE_FRAMES: the tests are sized from it).  Tile t is frames [t T, (t + 1) T)
// of the SAMPLE's own grid (not the window's), cut to [0, n); a workgroup of 256 lanes owns one tile, a lane LANE_FRAMES consecutive frames.
constexpr uint32_t LANE_FRAMES = 8;
constexpr uint32_t TILE_FRAMES = 256 * LANE_FRAMES;

SH_HD uint32_t hi_of(int w) { return (uint32_t)((1ull << (8 * w - 1)) - 1); }
SH_HD uint32_t slope(uint32_t f) { return f <= 1 ? ONE : (ONE + f - 1) / f; }
SH_HD uint32_t reach(uint32_t f) { return (ONE + slope(f) - 1) / slope(f); }

// min(ONE, v): the cap.  It commutes with min and with adding a non-negative number -- min(ONE, min(ONE, a) + b) = min(ONE, a + b) for
// b >= 0 -- so a value may be capped at every step, and a capped value plus a capped distance fits 32 bits (at most 2^31).
SH_HD uint32_t cap(uint64_t v) { return v < ONE ? (uint32_t)v : ONE; }
// a gain of at most ONE, d frames further along a ramp of slope s: d < 2^22 and s <= 2^30, so the sum is below 2^53 and wants 64 bits
SH_HD uint32_t ramp(uint32_t gain, uint64_t d, uint32_t s) { return cap((uint64_t)gain + d * (uint64_t)s); }
// one frame further: 32 bits do
SH_HD uint32_t step(uint32_t gain, uint32_t s) { return gain + s < ONE ? gain + s : ONE; }

SH_HD uint32_t magnitude(int32_t x) { return x < 0 ? 0u - (uint32_t)x : (uint32_t)x; }

// g: floor(C * ONE / p) where p > C -- then the quotient is below ONE and has 30 digits, taken one at a time: the remainder stays below
// p <= 2^31, so twice it fits 32 bits.  (The long division and not the operator: on the device a 64-bit `/` is carried out with
// float reciprocals, and the kernels hold no float instruction.  tests/cpu_pcmlimit.cpp holds it to the operator.)
SH_HD uint32_t required_gain(uint32_t p, uint32_t ceiling) {
    if (p <= ceiling) return ONE;
    uint32_t rem = ceiling, q = 0;
    for (int k = 0; k < 30; ++k) {
        rem <<= 1, q <<= 1;
        if (rem >= p) rem -= p, q |= 1;
    }
    return q;
}

SH_HD int32_t apply_gain(int32_t x, uint32_t gain) { return (int32_t)(((int64_t)x * (int64_t)gain) >> 30); }

// The tile summaries.  For a frame i of a later tile u > t, the release terms of tile t's frames are
//     min over j in t of g[j] + (i - j) s_r = FS[t] + (i - ((t + 1) T - 1)) s_r,   FS[t] = min over j in t of g[j] + ((t + 1) T - 1 - j) s_r
// -- tile t's own release curve where it leaves the tile, at its last frame -- and for an earlier tile u < t the attack terms are
// BS[t] + (t T - i) s_a with BS[t] = min over j in t of g[j] + (j - t T) s_a, the attack curve at the tile's first frame.  Both are kept
// capped at ONE (cap commutes, above).  The carries into tile u: the release curve of everything in front of u at u's FIRST frame,
//     CF[u] = min over t < u of FS[t] + ((u - t - 1) T + 1) s_r,
// and the attack curve of everything behind u at u's LAST frame (u + 1) T - 1, CB[u] = min over t > u of BS[t] + ((t - u - 1) T + 1) s_a.
// A tile k = u - t tiles away lies (k - 1) T + 1 frames away at the least, and past reach - 1 frames nothing matters:
// k <= (reach - 2) / T + 1 = carry_tiles (none where reach <= 1: a slope of ONE puts every other frame at ONE or above).
SH_HD uint32_t carry_tiles(uint32_t f) { return reach(f) <= 1 ? 0 : (reach(f) - 2) / TILE_FRAMES + 1; }
SH_HD uint64_t carry_distance(uint64_t k) { return (k - 1) * TILE_FRAMES + 1; }      // between the nearest frames of two tiles k apart

// What a call computes: tiles [apply_first, apply_first + apply_count) hold the window, and they need the summaries of tiles
// [sum_first, sum_first + sum_count): the window's own and carry_tiles(r) in front and carry_tiles(a) behind, cut to the sample.
struct Plan {
    uint32_t s_a, s_r, carry_a, carry_r;
    uint64_t apply_first, apply_count, sum_first, sum_count;
};

SH_HD Plan plan(uint64_t n, uint32_t attack, uint32_t release, uint64_t first, uint64_t count) {      // count >= 1, the window inside [0, n)
    Plan p{};
    p.s_a = slope(attack), p.s_r = slope(release), p.carry_a = carry_tiles(attack), p.carry_r = carry_tiles(release);
    const uint64_t ntiles = (n + TILE_FRAMES - 1) / TILE_FRAMES, apply_last = (first + count - 1) / TILE_FRAMES;
    p.apply_first = first / TILE_FRAMES, p.apply_count = apply_last - p.apply_first + 1;
    p.sum_first = p.apply_first > p.carry_r ? p.apply_first - p.carry_r : 0;
    const uint64_t sum_last = ntiles - 1 - apply_last > p.carry_a ? apply_last + p.carry_a : ntiles - 1;
    p.sum_count = sum_last - p.sum_first + 1;
    return p;
}

// Every refusal of a call, in the order in which it is looked for.  The operands are byte ranges: a buffer of `bytes` bytes at
// address `addr`, the operand from byte `off` of it on -- any byte: no alignment is asked for.  A destination may be absent.
enum Refusal {
    OK = 0,
    BAD_WIDTH,          // a width other than 1, 2 or 4
    BAD_CHANNELS,       // nch not 1 or 2
    BAD_CEILING,        // 0, or above HI
    BAD_ATTACK,         // above MAX_FRAMES
    BAD_RELEASE,        // above MAX_FRAMES
    BAD_WINDOW,         // [first, first + count) reaches past n
    IN_RANGE,           // x reaches past its buffer
    OUT_RANGE,          // the window reaches past the destination
    GAIN_RANGE,         // the window's gains reach past the gain plane
    OUT_OVERLAP,        // out overlaps x in any way but one: being exactly the window's own bytes of x (the call in place)
    GAIN_OVERLAP,       // the gain plane overlaps x or out
    NO_DESTINATION,     // neither out nor gain
};

struct Operand {
    uint64_t addr, bytes, off;
    bool     present;
};

SH_HD bool inside(const Operand& o, uint64_t items, uint64_t item_bytes) { return o.off <= o.bytes && items <= (o.bytes - o.off) / item_bytes; }

SH_HD bool overlap(uint64_t a0, uint64_t a_bytes, uint64_t b0, uint64_t b_bytes) { return a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes; }

SH_HD Refusal check(int width, int nch, uint64_t n, uint64_t ceiling, uint64_t attack, uint64_t release, uint64_t first, uint64_t count, const Operand& in,
                    const Operand& out, const Operand& gain) {
    if (width != 1 && width != 2 && width != 4) return BAD_WIDTH;
    if (nch != 1 && nch != 2) return BAD_CHANNELS;
    if (ceiling == 0 || ceiling > hi_of(width)) return BAD_CEILING;
    if (attack > MAX_FRAMES) return BAD_ATTACK;
    if (release > MAX_FRAMES) return BAD_RELEASE;
    if (count > n || first > n - count) return BAD_WINDOW;
    const uint64_t fb = (uint64_t)width * (uint64_t)nch;
    if (!inside(in, n, fb)) return IN_RANGE;
    if (out.present && !inside(out, count, fb)) return OUT_RANGE;
    if (gain.present && !inside(gain, count, sizeof(uint32_t))) return GAIN_RANGE;
    const uint64_t a0 = in.addr + in.off, o0 = out.addr + out.off, g0 = gain.addr + gain.off;
    if (out.present && o0 != a0 + first * fb && overlap(o0, count * fb, a0, n * fb)) return OUT_OVERLAP;
    if (gain.present && (overlap(g0, count * sizeof(uint32_t), a0, n * fb) || (out.present && overlap(g0, count * sizeof(uint32_t), o0, count * fb))))
        return GAIN_OVERLAP;
    if (!out.present && !gain.present) return NO_DESTINATION;
    return OK;
}

// The summaries of tile t on the host, as a workgroup of k_limit_tiles computes them.  get_g(i): g[i], 0 <= i < n.
template <typename GetG>
static inline void host_summary(GetG&& get_g, uint64_t n, uint64_t t, uint32_t s_a, uint32_t s_r, uint32_t* fs, uint32_t* bs) {
    const uint64_t base = t * TILE_FRAMES;
    uint32_t f = ONE, b = ONE;
    for (uint32_t q = 0; q < TILE_FRAMES && base + q < n; ++q) {
        const uint32_t g = get_g(base + q);
        const uint32_t to_end = ramp(g, TILE_FRAMES - 1 - q, s_r), to_start = ramp(g, q, s_a);
        f = to_end < f ? to_end : f, b = to_start < b ? to_start : b;
    }
    *fs = f, *bs = b;
}

// The carries into tile u from the summaries of tiles [p.sum_first, p.sum_first + p.sum_count): fs and bs are indexed from p.sum_first.
static inline void host_carries(const Plan& p, const uint32_t* fs, const uint32_t* bs, uint64_t u, uint32_t* cf, uint32_t* cb) {
    uint32_t f = ONE, b = ONE;
    for (uint64_t k = 1; k <= p.carry_r && k <= u - p.sum_first; ++k) {
        const uint32_t v = ramp(fs[u - k - p.sum_first], carry_distance(k), p.s_r);
        f = v < f ? v : f;
    }
    for (uint64_t k = 1; k <= p.carry_a && u + k < p.sum_first + p.sum_count; ++k) {
        const uint32_t v = ramp(bs[u + k - p.sum_first], carry_distance(k), p.s_a);
        b = v < b ? v : b;
    }
    *cf = f, *cb = b;
}

// Tile u applied on the host: the carries, then the release curve swept forwards and the attack curve swept backwards through the
// tile's own frames -- F[i] = min(g[i], F[i - 1] + s_r) from CF at the first frame, the mirror image from CB at the last -- and
// G = min(F, B).  put_gain(i, G) for every frame of the window in the tile; no frame outside the tile is looked at.
template <typename GetG, typename PutGain>
static inline void host_apply(GetG&& get_g, PutGain&& put_gain, uint64_t n, const Plan& p, const uint32_t* fs, const uint32_t* bs, uint64_t first,
                              uint64_t count, uint64_t u) {
    uint32_t cf, cb;
    host_carries(p, fs, bs, u, &cf, &cb);
    uint32_t* F = new uint32_t[TILE_FRAMES];
    const uint64_t base = u * TILE_FRAMES;
    uint32_t f = cf;
    for (uint32_t q = 0; q < TILE_FRAMES; ++q) {
        const uint32_t g = base + q < n ? get_g(base + q) : ONE;
        f = g < f ? g : f, F[q] = f, f = step(f, p.s_r);
    }
    uint32_t b = cb;
    for (uint32_t q = TILE_FRAMES; q-- > 0;) {
        const uint32_t g = base + q < n ? get_g(base + q) : ONE;
        b = g < b ? g : b;
        if (base + q >= first && base + q - first < count) put_gain(base + q, b < F[q] ? b : F[q]);
        b = step(b, p.s_a);
    }
    delete[] F;
}

// The whole call on the host, divided as the kernels divide it: the summaries, then per tile of the window the carries and the tile.
// get_x(c, i): sample of frame i, channel c; put(c, i, sample) and put_gain(i, G) for the frames of the window (either may do nothing).
template <typename GetX, typename Put, typename PutGain>
static inline void host_limit(GetX&& get_x, Put&& put, PutGain&& put_gain, uint64_t n, int nch, uint32_t ceiling, uint32_t attack, uint32_t release,
                              uint64_t first, uint64_t count) {
    if (!count) return;
    const Plan p = plan(n, attack, release, first, count);
    auto get_g = [&](uint64_t i) {
        uint32_t peak = magnitude(get_x(0, i));
        if (nch == 2 && magnitude(get_x(1, i)) > peak) peak = magnitude(get_x(1, i));
        return required_gain(peak, ceiling);
    };
    uint32_t* fs = new uint32_t[2 * p.sum_count];
    uint32_t* bs = fs + p.sum_count;
    for (uint64_t k = 0; k < p.sum_count; ++k) host_summary(get_g, n, p.sum_first + k, p.s_a, p.s_r, fs + k, bs + k);
    auto gained = [&](uint64_t i, uint32_t G) {
        put_gain(i, G);
        for (int c = 0; c < nch; ++c) put(c, i, apply_gain(get_x(c, i), G));
    };
    for (uint64_t k = 0; k < p.apply_count; ++k) host_apply(get_g, gained, n, p, fs, bs, first, count, p.apply_first + k);
    delete[] fs;
}

}  // namespace shpl
