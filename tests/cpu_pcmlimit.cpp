// csrc/pcmlimit.hpp built for the host behind a few C functions (tests/test_pcmlimit.py drives them through ctypes): the constants,
// slope, reach and carry_tiles, the required gain, every refusal of check, the carries folded from given summaries, and the whole call
// of sh_pcm_limit as a host loop over raw PCM -- summaries, carries, tiles, as the kernels divide it, and with the tiles taken from
// the last to the first.  With PCMLIMIT_MAIN it is a program of its own (its own main, generated PCM against the definition written
// out over every pair of frames).
#include "../synthesizer_amd/csrc/pcmlimit.hpp"

namespace {
// sample s of raw little-endian PCM of `width` (1, 2 or 4) bytes a sample
int32_t raw_sample(const unsigned char* p, int width, uint64_t s) {
    p += s * (uint64_t)width;
    if (width == 1) return (int32_t)(signed char)p[0];
    if (width == 2) return (int32_t)(int16_t)((unsigned)p[0] | ((unsigned)p[1] << 8));
    return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
}

void raw_put(unsigned char* p, int width, uint64_t s, int32_t v) {
    p += s * (uint64_t)width;
    for (int k = 0; k < width; ++k) p[k] = (unsigned char)(((uint32_t)v >> (8 * k)) & 0xFF);
}
}  // namespace

extern "C" {

void pl_constants(uint32_t* out) { out[0] = shpl::ONE, out[1] = shpl::MAX_FRAMES, out[2] = shpl::TILE_FRAMES, out[3] = shpl::LANE_FRAMES; }
uint32_t pl_hi(int w) { return shpl::hi_of(w); }
uint32_t pl_slope(uint32_t f) { return shpl::slope(f); }
uint32_t pl_reach(uint32_t f) { return shpl::reach(f); }
uint32_t pl_carry_tiles(uint32_t f) { return shpl::carry_tiles(f); }
uint32_t pl_required_gain(uint32_t p, uint32_t ceiling) { return shpl::required_gain(p, ceiling); }
int32_t pl_apply_gain(int32_t x, uint32_t gain) { return shpl::apply_gain(x, gain); }

// out: s_a, s_r, carry_a, carry_r, apply_first, apply_count, sum_first, sum_count
void pl_plan(uint64_t n, uint32_t attack, uint32_t release, uint64_t first, uint64_t count, uint64_t* out) {
    const shpl::Plan p = shpl::plan(n, attack, release, first, count);
    out[0] = p.s_a, out[1] = p.s_r, out[2] = p.carry_a, out[3] = p.carry_r, out[4] = p.apply_first, out[5] = p.apply_count, out[6] = p.sum_first,
    out[7] = p.sum_count;
}

// operands as (addr, bytes, off, present) quadruples
int pl_check(int width, int nch, uint64_t n, uint64_t ceiling, uint64_t attack, uint64_t release, uint64_t first, uint64_t count, const uint64_t* in,
             const uint64_t* out, const uint64_t* gain) {
    return (int)shpl::check(width, nch, n, ceiling, attack, release, first, count, shpl::Operand{in[0], in[1], in[2], in[3] != 0},
                            shpl::Operand{out[0], out[1], out[2], out[3] != 0}, shpl::Operand{gain[0], gain[1], gain[2], gain[3] != 0});
}

// the carries into tile u of a sample of n frames whose summaries (of the tiles the plan of the one-frame window at u's first frame
// asks for) are given: out[0] = CF, out[1] = CB
void pl_carries(uint64_t n, uint32_t attack, uint32_t release, uint64_t u, const uint32_t* fs, const uint32_t* bs, uint32_t* out) {
    const shpl::Plan p = shpl::plan(n, attack, release, u * shpl::TILE_FRAMES, 1);
    shpl::host_carries(p, fs, bs, u, out, out + 1);
}

// the whole call: frames [first, first + count) of x (n frames, nch channels) into out (count frames) and gain (count values); either
// may be NULL.  backwards != 0: the summaries from the last tile to the first, then the tiles of the window from the last to the first.
void pl_host_limit(const unsigned char* x, int width, uint64_t n, int nch, uint32_t ceiling, uint32_t attack, uint32_t release, uint64_t first, uint64_t count,
                   unsigned char* out, uint32_t* gain, int backwards) {
    auto get_x = [&](int c, uint64_t i) { return raw_sample(x, width, i * (uint64_t)nch + c); };
    auto put = [&](int c, uint64_t i, int32_t v) { if (out) raw_put(out, width, (i - first) * (uint64_t)nch + c, v); };
    auto put_gain = [&](uint64_t i, uint32_t G) { if (gain) gain[i - first] = G; };
    if (!backwards) {
        shpl::host_limit(get_x, put, put_gain, n, nch, ceiling, attack, release, first, count);
        return;
    }
    if (!count) return;
    const shpl::Plan p = shpl::plan(n, attack, release, first, count);
    auto get_g = [&](uint64_t i) {
        uint32_t peak = shpl::magnitude(get_x(0, i));
        if (nch == 2 && shpl::magnitude(get_x(1, i)) > peak) peak = shpl::magnitude(get_x(1, i));
        return shpl::required_gain(peak, ceiling);
    };
    uint32_t* fs = new uint32_t[2 * p.sum_count];
    uint32_t* bs = fs + p.sum_count;
    for (uint64_t k = p.sum_count; k-- > 0;) shpl::host_summary(get_g, n, p.sum_first + k, p.s_a, p.s_r, fs + k, bs + k);
    auto gained = [&](uint64_t i, uint32_t G) {
        put_gain(i, G);
        for (int c = nch; c-- > 0;) put(c, i, shpl::apply_gain(get_x(c, i), G));
    };
    for (uint64_t k = p.apply_count; k-- > 0;) shpl::host_apply(get_g, gained, n, p, fs, bs, first, count, p.apply_first + k);
    delete[] fs;
}

}  // extern "C"

#ifdef PCMLIMIT_MAIN
#include <cstdio>
#include <vector>
// generated PCM of the three widths, mono and stereo, windows that begin and end anywhere, forwards and backwards, against the
// definition over every pair of frames in 64-bit integers, the division by the operator
int main() {
    uint64_t state = 88172645463325252ull;
    auto rnd = [&](uint64_t m) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state % m; };
    const uint32_t T = shpl::TILE_FRAMES;
    const uint32_t spans[] = {0, 1, 2, 3, 7, 100, T - 1, T, T + 1, 2 * T + 3};
    unsigned calls = 0;
    for (int k = 0; k < 48; ++k) {
        const int width = 1 << (int)rnd(3), nch = 1 + (int)rnd(2);
        const uint64_t n = k < 40 ? 1 + rnd(400) : 2 * T - 3 + rnd(T + 6);
        const uint32_t hi = shpl::hi_of(width), ceiling = 1 + (uint32_t)rnd(hi), attack = spans[rnd(10)], release = spans[rnd(10)];
        std::vector<unsigned char> x((size_t)(n * nch * width));
        for (uint64_t s = 0; s < n * nch; ++s) {
            int64_t v = (int64_t)rnd(ceiling / 2 + 1) - (int64_t)(ceiling / 4);
            if (rnd(97) == 0) v = rnd(2) ? (int64_t)hi - (int64_t)rnd(hi / 2 + 1) : -(int64_t)hi - 1 + (int64_t)rnd(hi / 2 + 1);
            raw_put(x.data(), width, s, (int32_t)v);
        }
        const uint64_t first = rnd(n), count = 1 + rnd(n - first);
        std::vector<unsigned char> got((size_t)(count * nch * width)), back(got.size());
        std::vector<uint32_t> gain(count), gain_back(count);
        pl_host_limit(x.data(), width, n, nch, ceiling, attack, release, first, count, got.data(), gain.data(), 0);
        pl_host_limit(x.data(), width, n, nch, ceiling, attack, release, first, count, back.data(), gain_back.data(), 1);
        std::vector<uint64_t> need(n);
        for (uint64_t i = 0; i < n; ++i) {
            uint64_t p = 0;
            for (int c = 0; c < nch; ++c) {
                const int64_t v = raw_sample(x.data(), width, i * nch + c);
                p = (uint64_t)(v < 0 ? -v : v) > p ? (uint64_t)(v < 0 ? -v : v) : p;
            }
            need[i] = p <= ceiling ? shpl::ONE : (uint64_t)ceiling * shpl::ONE / p;
        }
        const uint64_t s_a = attack <= 1 ? shpl::ONE : (shpl::ONE + attack - 1) / attack, s_r = release <= 1 ? shpl::ONE : (shpl::ONE + release - 1) / release;
        for (uint64_t i = first; i < first + count; ++i) {
            uint64_t G = shpl::ONE;
            for (uint64_t j = 0; j < n; ++j) {
                const uint64_t term = j >= i ? need[j] + (j - i) * s_a : need[j] + (i - j) * s_r;
                G = term < G ? term : G;
            }
            bool ok = gain[i - first] == G && gain_back[i - first] == G;
            for (int c = 0; c < nch && ok; ++c) {
                const int64_t xv = raw_sample(x.data(), width, i * nch + c), prod = xv * (int64_t)G;
                const int64_t want = prod >= 0 ? prod / (int64_t)shpl::ONE : -((-prod + (int64_t)shpl::ONE - 1) / (int64_t)shpl::ONE);      // floor
                const uint64_t s = (i - first) * nch + c;
                ok = raw_sample(got.data(), width, s) == want && raw_sample(back.data(), width, s) == want && want <= (int64_t)ceiling && -want <= (int64_t)ceiling;
            }
            if (!ok) {
                printf("case %d: width %d, %d channels, attack %u, release %u, frame %llu\n", k, width, nch, attack, release, (unsigned long long)i);
                return 1;
            }
        }
        ++calls;
    }
    printf("pcmlimit: %u calls ok\n", calls);
    return 0;
}
#endif
