// pcmresample.hpp -- a rational, band-limited sample-rate conversion of PCM that already lies in device memory (sh_pcm_resample_fir,
// pcm_resample_fir.hip): the contract of the call, stated once -- what is refused, how long the result is, the index arithmetic of the
// polyphase form, how the kernel divides the work (plan) -- and the whole call as a host loop that divides it the same way.
// The input x: n frames of nch (1 or 2) interleaved channels of w (1 or 2) bytes.  The taps h: m int16 values (1 <= m <= 2^22), ONE
// mono bank for every channel, 16 bits whatever w is.  up = L >= 1, down = M >= 1 (they need not be coprime), 0 <= delay < m, a finite
// factor.  The result: result_frames(n, L, M) = ceil(n L / M) frames (0 when n == 0) of nch channels of w bytes; for channel c and
// frame j, with u[i] = x_c[i / L] where L divides i and 0 <= i < n L, and 0 elsewhere,
//     acc[j] = sum over k in [0, m) of h[k] * u[j M + delay - k],          y[j] = fbound((double)acc[j] * factor):
// zero-stuff by L, filter, keep every M-th -- the EXACT integer sum and then ONE rounding, pcmdev.hpp's fbound (audioop.mul's last
// step; shpf::scale states it for the host).  In polyphase form, with p = (j M + delay) mod L and b = (j M + delay) div L,
//     acc[j] = sum over t of h[p + t L] * x_c[b - t],                      frames of x outside [0, n) counting as 0:
// at most ceil(m / L) <= 2^22 terms of a magnitude of at most 2^30 each, so pcmfir.hpp's proof ("Why float64 is exact here") applies
// word for word: a float64 FMA chain IS the integer sum, and the bytes depend on x, h, L, M, delay and factor alone -- not on blocks,
// chunks, windows or runs.  A call computes frames [first, first + count) of the result: that slice of the whole result's bytes.
// Plain C++17, no intrinsics, SH_HD (tests/cpu_pcmresample.cpp builds it with g++).
#pragma once
#include "pcmfir.hpp"

namespace shpr {

using shpf::Operand;
using shpf::inside;
using shpf::overlap;

constexpr uint32_t MAX_TAPS = shpf::MAX_TAPS;       // 2^22: up to here every partial sum is a float64 (pcmfir.hpp)
constexpr uint32_t MAX_UP = 4096;                   // the residues of one group of outputs: P = c L row sets of the bank
constexpr uint32_t LANE_OUTPUTS = 8;                // R: the outputs (accumulators) of one lane, fed by ONE read of x per step
constexpr uint32_t BLOCK_GROUPS = 64;               // a wave's lanes are 64 consecutive groups
constexpr uint32_t WAVES = 4;                       // of a workgroup
constexpr uint32_t STEP_CHUNK = 1024;               // steps t'' under one staged span of x
constexpr uint32_t STEP_UNROLL = 2;                 // the rows are padded with zeros to a multiple of it (a zero tap adds exactly nothing)
constexpr uint32_t STAGED_SAMPLES = 32768;          // the staged span's bound, padding included

// A diagnostic build may stage x as float32 instead of as the sample type (SYNTHHIP_BUILD_FLAGS=-DSH_FIRP_STAGE_F32): the alternative
// profiles/resample_fir_ab.txt measures, never the shipped library.
#ifdef SH_FIRP_STAGE_F32
SH_HD uint32_t stage_bytes(int) { return 4; }
#else
SH_HD uint32_t stage_bytes(int width) { return (uint32_t)width; }
#endif

// ceil(n L / M) without a 128-bit product: n = q M + r gives q L + ceil(r L / M), and r L < 2^64.  A length that no uint64 holds
// comes back as UINT64_MAX (no buffer is that long: check() then refuses the window or the destination).
SH_HD uint64_t result_frames(uint64_t n, uint32_t L, uint32_t M) {
    if (n == 0 || L == 0 || M == 0) return 0;
    const uint64_t q = n / M, r = n % M, tail = (r * L + M - 1) / M;
    if (q > (UINT64_MAX - tail) / L) return UINT64_MAX;
    return q * L + tail;
}

// ---- the mapping.  R = LANE_OUTPUTS outputs per lane; c = 1 if L >= R else ceil(R / L); P = c L; M' = c M.  Output j = P g + rho
// (g the group, 0 <= rho < P the residue) has b = g M' + e(rho) and p = p(rho): neither table depends on g.  The residues are cut
// into chunks of R (a last short chunk has rows of zeros, which are never stored); chunk q takes E_q = max e over it -- e rises
// with rho, so that is its last residue's -- and folds each residue's offset into its taps:
//     row[rho][t''] = h[p(rho) + (t'' - (E_q - e(rho))) L]     (0 where that index is outside [0, m)),
//     acc[P g + rho] = sum over t'' in [0, TT) of row[rho][t''] * x_c[g M' + E_q - t''].
// So lane g reads ONE value of x per step t'', which feeds R FMAs whose R taps are wave-uniform; successive lanes are M' frames apart.
SH_HD uint32_t copies(uint32_t L) { return L >= LANE_OUTPUTS ? 1u : (LANE_OUTPUTS + L - 1) / L; }
SH_HD uint64_t e_of(uint32_t rho, uint32_t L, uint32_t M, uint32_t delay) { return ((uint64_t)rho * M + delay) / L; }
SH_HD uint32_t p_of(uint32_t rho, uint32_t L, uint32_t M, uint32_t delay) { return (uint32_t)(((uint64_t)rho * M + delay) % L); }
SH_HD uint32_t chunk_last(uint32_t q, uint32_t P) { return q * LANE_OUTPUTS + LANE_OUTPUTS - 1 < P ? q * LANE_OUTPUTS + LANE_OUTPUTS - 1 : P - 1; }
SH_HD uint64_t E_of(uint32_t q, uint32_t P, uint32_t L, uint32_t M, uint32_t delay) { return e_of(chunk_last(q, P), L, M, delay); }
// tap k of row rho at step t of chunk q, or -1: no tap (a zero)
SH_HD int64_t row_tap(uint32_t q, uint32_t rho, uint32_t t, uint32_t P, uint32_t L, uint32_t M, uint32_t delay, uint32_t m) {
    if (rho >= P) return -1;
    const uint64_t d = E_of(q, P, L, M, delay) - e_of(rho, L, M, delay);
    if (t < d) return -1;
    const uint64_t k = p_of(rho, L, M, delay) + (t - d) * (uint64_t)L;
    return k < m ? (int64_t)k : -1;
}

// Where frame j of a staged span lies.  Lane l of a wave reads l M' frames further on than lane 0, so an M' that is a multiple of 4
// (of 2 with four bytes a sample, of 8 with one) puts the 32 lanes of an LDS access on few banks -- M' = 160 (48 -> 44.1 kHz) as
// int16 on 2 of 32.  The span is therefore laid out in rows of M' frames with `pad` unused ones behind each: lane l, o frames into its
// own, reads at l (M' + pad) + o + (o / M') pad, and o is wave-uniform.
SH_HD uint32_t staged_at(uint32_t j, uint32_t Mp, uint32_t pad) { return pad ? j + j / Mp * pad : j; }

// the most distinct dwords that lanes 0..31, `stride` samples of `bytes` bytes apart, put on one of the 32 banks of a 4-byte LDS
// read, over every phase inside a dword (lanes on the same dword share one read).  ARITHMETIC on the bank formula (byte address / 4)
// mod 32, not a counter reading.
static inline uint32_t bank_ways(uint32_t stride, uint32_t bytes) {
    uint32_t worst = 0;
    for (uint32_t o = 0; o < 4 / bytes; ++o) {
        uint32_t dw[32];
        for (uint32_t l = 0; l < 32; ++l) dw[l] = (uint32_t)(((uint64_t)l * stride + o) * bytes / 4);
        for (uint32_t b = 0; b < 32; ++b) {
            uint32_t ways = 0;
            for (uint32_t l = 0; l < 32; ++l) {
                if (dw[l] % 32 != b) continue;
                bool seen = false;
                for (uint32_t k = 0; k < l; ++k) seen = seen || dw[k] == dw[l];
                ways += !seen;
            }
            worst = ways > worst ? ways : worst;
        }
    }
    return worst;
}
// the smallest pad in [0, 4) with the fewest ways
static inline uint32_t pick_pad(uint32_t Mp, uint32_t bytes) {
    uint32_t best = 0, ways = bank_ways(Mp, bytes);
    for (uint32_t pad = 1; pad < 4 && ways > 1; ++pad)
        if (bank_ways(Mp + pad, bytes) < ways) best = pad, ways = bank_ways(Mp + pad, bytes);
    return best;
}

// ---- every refusal of a call, in the order in which it is looked for (operands as in pcmfir.hpp: byte ranges, any byte)
enum Refusal {
    OK = 0,
    BAD_WIDTH,          // a width other than 1 or 2
    BAD_CHANNELS,       // nch not 1 or 2
    NO_TAPS,            // m == 0
    TOO_MANY_TAPS,      // m > MAX_TAPS
    BAD_RATIO,          // up == 0 or down == 0
    BAD_UP,             // up > MAX_UP
    BAD_STRIDE,         // (BLOCK_GROUPS - 1) M' + STEP_CHUNK > STAGED_SAMPLES: the lanes of a wave lie too far apart for one staged span
    BAD_DELAY,          // delay >= m
    BAD_FACTOR,         // a factor that is not finite
    BAD_WINDOW,         // [first, first + count) reaches past result_frames(n, up, down)
    IN_RANGE,           // x reaches past its buffer
    TAPS_RANGE,         // h reaches past its buffer
    OUT_RANGE,          // the window reaches past the destination
    OVERLAP,            // the destination's bytes overlap x's or h's
};

SH_HD bool stride_fits(uint32_t up, uint32_t down) {
    return (uint64_t)(BLOCK_GROUPS - 1) * copies(up) * down + STEP_CHUNK <= STAGED_SAMPLES;
}

SH_HD Refusal check(int width, int nch, uint64_t n, uint64_t m, uint32_t up, uint32_t down, uint32_t delay, double factor, uint64_t first, uint64_t count,
                    const Operand& in, const Operand& taps, const Operand& out) {
    if (width != 1 && width != 2) return BAD_WIDTH;
    if (nch != 1 && nch != 2) return BAD_CHANNELS;
    if (m == 0) return NO_TAPS;
    if (m > MAX_TAPS) return TOO_MANY_TAPS;
    if (up == 0 || down == 0) return BAD_RATIO;
    if (up > MAX_UP) return BAD_UP;
    if (!stride_fits(up, down)) return BAD_STRIDE;
    if (delay >= m) return BAD_DELAY;
    if (!(factor - factor == 0.0)) return BAD_FACTOR;            // (an infinity or a NaN less itself is a NaN)
    const uint64_t total = result_frames(n, up, down);
    if (count > total || first > total - count) return BAD_WINDOW;
    const uint64_t fb = (uint64_t)width * (uint64_t)nch;
    if (!inside(in, n, fb)) return IN_RANGE;
    if (!inside(taps, m, 2)) return TAPS_RANGE;
    if (!inside(out, count, fb)) return OUT_RANGE;
    if (overlap(out, count * fb, in, n * fb) || overlap(out, count * fb, taps, m * 2)) return OVERLAP;
    return OK;
}

// ---- how the kernel divides a call that check() has passed: ONE pure function, its constants exported as N.PCM_RESAMPLE_*.
// A workgroup of WAVES waves owns `blocks` blocks of BLOCK_GROUPS consecutive groups of one channel and stages their span of x once
// per chunk of `step_chunk` steps; `q_waves` = min(chunks, WAVES) waves share out the residue chunks of a block in `rounds` rounds
// (wave w: block w / q_waves of the workgroup, chunk round * q_waves + w % q_waves), and with fewer than WAVES chunks (L <= 24) the
// waves left over take further blocks -- as many as the staged span holds.
struct Plan {
    uint32_t c, P, Mp;          // copies, residues, lane stride in frames of x
    uint32_t chunks;            // residue chunks: ceil(P / R)
    uint32_t e_lo, e_span;      // e(0), and e(P - 1) - e(0): the staged span covers every chunk's E_q
    uint32_t spread;            // the largest E_q - e over a chunk
    uint32_t steps;             // TT: ceil(m / L) + spread, up to STEP_UNROLL
    uint32_t pad;               // staged_at's
    uint32_t q_waves, rounds, blocks;
    uint32_t step_chunk;        // steps per staged span: STEP_CHUNK where it fits, at most `steps`
    uint32_t staged;            // samples of LDS, padding included (<= STAGED_SAMPLES)
};

SH_HD uint32_t staged_need(uint32_t groups, uint32_t Mp, uint32_t pad, uint32_t e_span, uint32_t steps) {
    return staged_at((groups - 1) * Mp + e_span + steps - 1, Mp, pad) + 1;
}

static inline Plan plan(uint32_t m, uint32_t L, uint32_t M, uint32_t delay, uint32_t bytes) {
    Plan pl{};
    pl.c = copies(L), pl.P = pl.c * L, pl.Mp = pl.c * M;
    pl.chunks = (pl.P + LANE_OUTPUTS - 1) / LANE_OUTPUTS;
    pl.e_lo = (uint32_t)e_of(0, L, M, delay), pl.e_span = (uint32_t)e_of(pl.P - 1, L, M, delay) - pl.e_lo;
    for (uint32_t q = 0; q < pl.chunks; ++q) {
        const uint32_t s = (uint32_t)(E_of(q, pl.P, L, M, delay) - e_of(q * LANE_OUTPUTS, L, M, delay));
        pl.spread = s > pl.spread ? s : pl.spread;
    }
    pl.steps = ((m + L - 1) / L + pl.spread + STEP_UNROLL - 1) / STEP_UNROLL * STEP_UNROLL;
    pl.pad = pick_pad(pl.Mp, bytes);
    pl.q_waves = pl.chunks < WAVES ? pl.chunks : WAVES;
    pl.rounds = (pl.chunks + pl.q_waves - 1) / pl.q_waves;
    pl.step_chunk = pl.steps < STEP_CHUNK ? pl.steps : STEP_CHUNK;
    pl.blocks = WAVES / pl.q_waves;
    while (pl.blocks > 1 && staged_need(pl.blocks * BLOCK_GROUPS, pl.Mp, pl.pad, pl.e_span, pl.step_chunk) > STAGED_SAMPLES) --pl.blocks;
    // (e_span <= M' + 1 and the padding at most 3 * 64: behind stride_fits there is room for some hundred steps at the least)
    while (pl.step_chunk > STEP_UNROLL && staged_need(pl.blocks * BLOCK_GROUPS, pl.Mp, pl.pad, pl.e_span, pl.step_chunk) > STAGED_SAMPLES)
        pl.step_chunk -= STEP_UNROLL;
    pl.staged = staged_need(pl.blocks * BLOCK_GROUPS, pl.Mp, pl.pad, pl.e_span, pl.step_chunk);
    return pl;
}

// the groups a window touches and the workgroups over them
SH_HD uint64_t first_group(uint64_t first, const Plan& pl) { return first / pl.P; }
SH_HD uint64_t workgroups_of(uint64_t first, uint64_t count, const Plan& pl) {
    if (!count) return 0;
    const uint64_t groups = (first + count - 1) / pl.P - first / pl.P + 1, per = (uint64_t)pl.blocks * BLOCK_GROUPS;
    return (groups + per - 1) / per;
}

// the row bank as k_firp_rows builds it: float64, [chunk][step][r], so that one step's R taps lie side by side; new[]'d
template <typename GetH>
static inline double* host_rows(GetH&& get_h, uint32_t m, uint32_t L, uint32_t M, uint32_t delay, const Plan& pl) {
    double* rows = new double[(size_t)pl.chunks * pl.steps * LANE_OUTPUTS];
    for (uint32_t q = 0; q < pl.chunks; ++q)
        for (uint32_t t = 0; t < pl.steps; ++t)
            for (uint32_t r = 0; r < LANE_OUTPUTS; ++r) {
                const int64_t k = row_tap(q, q * LANE_OUTPUTS + r, t, pl.P, L, M, delay, m);
                rows[((size_t)q * pl.steps + t) * LANE_OUTPUTS + r] = k < 0 ? 0.0 : (double)get_h((uint32_t)k);
            }
    return rows;
}

// One workgroup of one channel on the host, as the kernel computes it: per round and per chunk of steps the staged span laid out by
// staged_at (a frame outside [0, n) is 0 and is never asked for), per wave and lane R sums, every term one fma in float64, the steps
// in rising order.  get_x(c, i): sample of frame i, channel c; rows: host_rows'; put(c, j, sample): frame j of the RESULT -- only
// frames of the window are put.
template <typename GetX, typename Put>
static inline void host_workgroup(GetX&& get_x, const double* rows, Put&& put, uint64_t n, uint32_t L, uint32_t M, uint32_t delay, int c, int w,
                                  double factor, uint64_t first, uint64_t count, const Plan& pl, uint64_t wg) {
    const uint32_t groups = pl.blocks * BLOCK_GROUPS, R = LANE_OUTPUTS;
    const uint64_t g0 = first_group(first, pl) + wg * groups, g_last = (first + count - 1) / pl.P;
    double* staged = new double[pl.staged];
    double* acc = new double[(size_t)WAVES * BLOCK_GROUPS * R];          // a lane's R sums, wave by wave
    for (uint32_t round = 0; round < pl.rounds; ++round) {
        for (size_t i = 0; i < (size_t)WAVES * BLOCK_GROUPS * R; ++i) acc[i] = 0.0;
        for (uint32_t t0 = 0; t0 < pl.steps; t0 += pl.step_chunk) {
            const uint32_t sc = pl.steps - t0 < pl.step_chunk ? pl.steps - t0 : pl.step_chunk, span = (groups - 1) * pl.Mp + pl.e_span + sc;
            const int64_t base = (int64_t)(g0 * pl.Mp) + pl.e_lo - (int64_t)(t0 + sc - 1);
            if (base >= (int64_t)n || base + (int64_t)span <= 0) continue;      // nothing of x under this chunk: it adds nothing
            for (uint32_t j = 0; j < span; ++j) {
                const int64_t f = base + (int64_t)j;
                staged[staged_at(j, pl.Mp, pl.pad)] = f >= 0 && f < (int64_t)n ? (double)get_x(c, (uint64_t)f) : 0.0;
            }
            for (uint32_t wave = 0; wave < WAVES; ++wave) {
                const uint32_t blk = wave / pl.q_waves, q = round * pl.q_waves + wave % pl.q_waves;
                if (blk >= pl.blocks || q >= pl.chunks) continue;
                const uint32_t o_hi = (uint32_t)(E_of(q, pl.P, L, M, delay) - pl.e_lo) + sc - 1;
                for (uint32_t lane = 0; lane < BLOCK_GROUPS; ++lane) {
                    const uint32_t gl = blk * BLOCK_GROUPS + lane;
                    for (uint32_t t = 0; t < sc; ++t) {
                        const uint32_t o = o_hi - t;
                        const double xv = staged[gl * (pl.Mp + pl.pad) + o + o / pl.Mp * pl.pad];
                        const double* h = rows + ((size_t)q * pl.steps + t0 + t) * R;
                        double* a = acc + ((size_t)wave * BLOCK_GROUPS + lane) * R;
                        for (uint32_t r = 0; r < R; ++r) a[r] = std::fma(h[r], xv, a[r]);
                    }
                }
            }
        }
        for (uint32_t wave = 0; wave < WAVES; ++wave) {
            const uint32_t blk = wave / pl.q_waves, q = round * pl.q_waves + wave % pl.q_waves;
            if (blk >= pl.blocks || q >= pl.chunks) continue;
            for (uint32_t lane = 0; lane < BLOCK_GROUPS; ++lane) {
                const uint32_t gl = blk * BLOCK_GROUPS + lane;
                if (g0 + gl > g_last) continue;
                for (uint32_t r = 0; r < R && q * R + r < pl.P; ++r) {
                    const uint64_t j = (g0 + gl) * pl.P + q * R + r;
                    if (j >= first && j - first < count) put(c, j, shpf::scale((int64_t)acc[((size_t)wave * BLOCK_GROUPS + lane) * R + r], factor, w));
                }
            }
        }
    }
    delete[] acc;
    delete[] staged;
}

// The whole call on the host, workgroup by workgroup as the kernel divides it: every workgroup of every channel, in rising order.
template <typename GetX, typename GetH, typename Put>
static inline void host_resample(GetX&& get_x, GetH&& get_h, Put&& put, uint64_t n, uint32_t m, uint32_t L, uint32_t M, uint32_t delay, int nch, int w,
                                 double factor, uint64_t first, uint64_t count) {
    const Plan pl = plan(m, L, M, delay, stage_bytes(w));
    double* rows = host_rows(get_h, m, L, M, delay, pl);
    for (uint64_t wg = 0; wg < workgroups_of(first, count, pl); ++wg)
        for (int c = 0; c < nch; ++c) host_workgroup(get_x, rows, put, n, L, M, delay, c, w, factor, first, count, pl, wg);
    delete[] rows;
}

}  // namespace shpr
