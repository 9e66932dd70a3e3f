// csrc/pcmresample.hpp built for the host behind a few C functions (tests/test_pcmresample.py drives them through ctypes): the
// constants, the result's length, every refusal of check, the plan with its tables, and the whole call of sh_pcm_resample_fir as a
// host loop over raw PCM -- workgroup by workgroup as the kernel divides it, forwards or from the last workgroup to the first.  With
// PCMRESAMPLE_MAIN it is a program of its own (its own main: generated PCM against the zero-stuffed definition in 64-bit integers,
// frame by frame).
#include "../synthesizer_amd/csrc/pcmresample.hpp"

namespace {
// sample s of raw little-endian PCM of `width` (1 or 2) bytes a sample
int32_t raw_sample(const unsigned char* p, int width, uint64_t s) {
    p += s * (uint64_t)width;
    if (width == 1) return (int32_t)(signed char)p[0];
    return (int32_t)(int16_t)((unsigned)p[0] | ((unsigned)p[1] << 8));
}

void raw_put(unsigned char* p, int width, uint64_t s, int32_t v) {
    p += s * (uint64_t)width;
    p[0] = (unsigned char)(v & 0xFF);
    if (width == 2) p[1] = (unsigned char)((v >> 8) & 0xFF);
}
}  // namespace

extern "C" {

void pr_constants(uint32_t* out) {
    out[0] = shpr::MAX_TAPS, out[1] = shpr::MAX_UP, out[2] = shpr::LANE_OUTPUTS, out[3] = shpr::BLOCK_GROUPS, out[4] = shpr::WAVES;
    out[5] = shpr::STEP_CHUNK, out[6] = shpr::STEP_UNROLL, out[7] = shpr::STAGED_SAMPLES;
}
uint64_t pr_result_frames(uint64_t n, uint32_t L, uint32_t M) { return shpr::result_frames(n, L, M); }
int pr_stride_fits(uint32_t L, uint32_t M) { return shpr::stride_fits(L, M) ? 1 : 0; }
uint32_t pr_bank_ways(uint32_t stride, uint32_t bytes) { return shpr::bank_ways(stride, bytes); }
uint32_t pr_staged_at(uint32_t j, uint32_t Mp, uint32_t pad) { return shpr::staged_at(j, Mp, pad); }

// operands as (addr, bytes, off) triples
int pr_check(int width, int nch, uint64_t n, uint64_t m, uint32_t up, uint32_t down, uint32_t delay, double factor, uint64_t first, uint64_t count,
             const uint64_t* in, const uint64_t* taps, const uint64_t* out) {
    return (int)shpr::check(width, nch, n, m, up, down, delay, factor, first, count, shpr::Operand{in[0], in[1], in[2]},
                            shpr::Operand{taps[0], taps[1], taps[2]}, shpr::Operand{out[0], out[1], out[2]});
}

// the plan as 14 words: c, P, Mp, chunks, e_lo, e_span, spread, steps, pad, q_waves, rounds, blocks, step_chunk, staged
void pr_plan(uint32_t m, uint32_t L, uint32_t M, uint32_t delay, uint32_t bytes, uint32_t* out) {
    const shpr::Plan p = shpr::plan(m, L, M, delay, bytes);
    const uint32_t v[14] = {p.c, p.P, p.Mp, p.chunks, p.e_lo, p.e_span, p.spread, p.steps, p.pad, p.q_waves, p.rounds, p.blocks, p.step_chunk, p.staged};
    for (int k = 0; k < 14; ++k) out[k] = v[k];
}
// the tables of the P residues, and the E_q of the chunks
void pr_tables(uint32_t L, uint32_t M, uint32_t delay, uint32_t P, uint64_t* e, uint32_t* p, uint64_t* E) {
    for (uint32_t rho = 0; rho < P; ++rho) e[rho] = shpr::e_of(rho, L, M, delay), p[rho] = shpr::p_of(rho, L, M, delay);
    for (uint32_t q = 0; q < (P + shpr::LANE_OUTPUTS - 1) / shpr::LANE_OUTPUTS; ++q) E[q] = shpr::E_of(q, P, L, M, delay);
}
int64_t pr_row_tap(uint32_t q, uint32_t rho, uint32_t t, uint32_t P, uint32_t L, uint32_t M, uint32_t delay, uint32_t m) {
    return shpr::row_tap(q, rho, t, P, L, M, delay, m);
}
uint64_t pr_workgroups(uint64_t first, uint64_t count, uint32_t m, uint32_t L, uint32_t M, uint32_t delay, uint32_t bytes) {
    return shpr::workgroups_of(first, count, shpr::plan(m, L, M, delay, bytes));
}

// the whole call: frames [first, first + count) of x (n frames, nch channels) under the m int16 taps h into out, which holds count
// frames; backwards != 0: the workgroups from the last to the first and the channels from the last to the first; owners (or NULL)
// counts, per frame of the window and channel, how often it was put
void pr_host_resample(const unsigned char* x, const int16_t* h, int width, uint64_t n, uint32_t m, uint32_t L, uint32_t M, uint32_t delay, int nch, double factor,
                      uint64_t first, uint64_t count, unsigned char* out, int backwards, uint32_t* owners) {
    auto get_x = [&](int c, uint64_t i) { return raw_sample(x, width, i * (uint64_t)nch + c); };
    auto get_h = [&](uint32_t k) { return (int32_t)h[k]; };
    auto put = [&](int c, uint64_t j, int32_t v) {
        raw_put(out, width, (j - first) * (uint64_t)nch + c, v);
        if (owners) ++owners[(j - first) * (uint64_t)nch + c];
    };
    if (!backwards) {
        shpr::host_resample(get_x, get_h, put, n, m, L, M, delay, nch, width, factor, first, count);
        return;
    }
    const shpr::Plan pl = shpr::plan(m, L, M, delay, shpr::stage_bytes(width));
    double* rows = shpr::host_rows(get_h, m, L, M, delay, pl);
    for (uint64_t wg = shpr::workgroups_of(first, count, pl); wg-- > 0;)
        for (int c = nch; c-- > 0;) shpr::host_workgroup(get_x, rows, put, n, L, M, delay, c, width, factor, first, count, pl, wg);
    delete[] rows;
}

}  // extern "C"

#ifdef PCMRESAMPLE_MAIN
#include <cstdio>
#include <vector>
// generated PCM of both widths, mono and stereo, ratios on both sides of one, windows that begin and end anywhere, forwards and
// backwards, against the definition: the zero-stuffed sum in 64-bit integers and the rounding written out
int main() {
    uint64_t state = 88172645463325252ull;
    auto rnd = [&](uint64_t m) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state % m; };
    const uint32_t ratios[][2] = {{1, 1}, {2, 1}, {1, 2}, {3, 2}, {2, 3}, {7, 8}, {8, 1}, {1, 8}, {5, 3}, {4, 6}, {160, 147}, {147, 160}, {80, 441}};
    unsigned calls = 0;
    for (int k = 0; k < 78; ++k) {
        const uint32_t L = ratios[k % 13][0], M = ratios[k % 13][1];
        const int width = 1 + (int)rnd(2), nch = 1 + (int)rnd(2);
        const uint32_t m = k < 52 ? 1 + (uint32_t)rnd(5 * L + 3) : (shpr::STEP_CHUNK + (uint32_t)rnd(6)) * L - 3 + (uint32_t)rnd(6);
        const uint32_t delay = (uint32_t)rnd(m);
        const uint64_t n = k < 52 ? 1 + rnd(40 * (uint64_t)shpr::copies(L) * M + 5) : 3 * (uint64_t)shpr::copies(L) * M + rnd(9);
        const double factor = k % 4 == 0 ? 1.0 : 1.0 / (double)(1u << (15 - rnd(3)));
        std::vector<unsigned char> x((size_t)(n * nch * width));
        std::vector<int16_t> h(m);
        for (auto& c : x) c = (unsigned char)(rnd(5) == 0 ? (rnd(2) ? 0x80 : 0x7f) : rnd(256));
        for (auto& t : h) t = (int16_t)(rnd(5) == 0 ? (rnd(2) ? -32768 : 32767) : (int)rnd(65536) - 32768);
        const uint64_t total = shpr::result_frames(n, L, M), first = rnd(total), count = 1 + rnd(total - first);
        std::vector<unsigned char> got((size_t)(count * nch * width)), back(got.size());
        pr_host_resample(x.data(), h.data(), width, n, m, L, M, delay, nch, factor, first, count, got.data(), 0, nullptr);
        pr_host_resample(x.data(), h.data(), width, n, m, L, M, delay, nch, factor, first, count, back.data(), 1, nullptr);
        const double lo = width == 1 ? -128.0 : -32768.0, hi = width == 1 ? 127.0 : 32767.0;
        for (uint64_t j = first; j < first + count; ++j)
            for (int c = 0; c < nch; ++c) {
                int64_t acc = 0;
                for (uint32_t t = 0; t < m; ++t) {
                    const int64_t i = (int64_t)(j * M + delay) - (int64_t)t;         // u[i] = x[i / L] where L divides i
                    if (i >= 0 && i % L == 0 && (uint64_t)i / L < n) acc += (int64_t)h[t] * raw_sample(x.data(), width, ((uint64_t)i / L) * nch + c);
                }
                double p = (double)acc * factor;
                if (p > hi) p = hi;
                else if (p < lo + 1.0) p = lo;
                const int32_t want = (int32_t)std::floor(p);
                const uint64_t s = (j - first) * nch + c;
                if (raw_sample(got.data(), width, s) != want || raw_sample(back.data(), width, s) != want) {
                    printf("case %d: %u/%u, %u taps, delay %u, width %d, %d channels, frame %llu, channel %d\n", k, L, M, m, delay, width, nch, (unsigned long long)j, c);
                    return 1;
                }
            }
        ++calls;
    }
    printf("pcmresample: %u calls ok\n", calls);
    return 0;
}
#endif
