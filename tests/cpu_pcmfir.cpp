// csrc/pcmfir.hpp built for the host behind a few C functions (tests/test_pcmfir.py drives them through ctypes): the constants, the
// result's length, the one rounding, every refusal of check, and the whole call of sh_pcm_convolve as a host loop over raw PCM -- tile
// by tile as the kernel divides it, and with the tiles taken from the last to the first.  With PCMFIR_MAIN it is a program of its own
// (its own main, generated PCM against a restatement in 64-bit integers, frame by frame).
#include "../synthesizer_amd/csrc/pcmfir.hpp"

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

void pf_constants(uint32_t* out) {
    out[0] = shpf::MAX_TAPS, out[1] = shpf::TILE_FRAMES, out[2] = shpf::TAP_CHUNK, out[3] = shpf::LANE_FRAMES, out[4] = shpf::TAP_UNROLL;
}
uint64_t pf_result_frames(uint64_t n, uint64_t m) { return shpf::result_frames(n, m); }
int32_t pf_scale(int64_t acc, double factor, int w) { return shpf::scale(acc, factor, w); }
uint32_t pf_padded_taps(uint32_t m) { return shpf::padded_taps(m); }

// operands as (addr, bytes, off) triples
int pf_check(int width, int nch, int ir_nch, uint64_t n, uint64_t m, double factor, uint64_t first, uint64_t count, const uint64_t* in, const uint64_t* ir,
             const uint64_t* out) {
    return (int)shpf::check(width, nch, ir_nch, n, m, factor, first, count, shpf::Operand{in[0], in[1], in[2]}, shpf::Operand{ir[0], ir[1], ir[2]},
                            shpf::Operand{out[0], out[1], out[2]});
}

// the whole call: frames [first, first + count) of x (n frames, nch channels) under h (m frames, ir_nch channels) into out, which
// holds count frames; backwards != 0: the tiles from the last to the first and the channels from the last to the first
void pf_host_convolve(const unsigned char* x, const unsigned char* h, int width, uint64_t n, uint32_t m, int nch, int ir_nch, double factor, uint64_t first,
                      uint64_t count, unsigned char* out, int backwards) {
    auto get_x = [&](int c, uint64_t i) { return raw_sample(x, width, i * (uint64_t)nch + c); };
    auto get_h = [&](int c, uint32_t k) { return raw_sample(h, width, (uint64_t)k * ir_nch + c); };
    auto put = [&](int c, uint64_t i, int32_t v) { raw_put(out, width, (i - first) * (uint64_t)nch + c, v); };
    if (!backwards) {
        shpf::host_convolve(get_x, get_h, put, n, m, nch, ir_nch, width, factor, first, count);
        return;
    }
    for (uint64_t tile = shpf::tiles_of(count); tile-- > 0;)
        for (int c = nch; c-- > 0;) shpf::host_tile(get_x, get_h, put, n, m, c, ir_nch == 2 ? c : 0, width, factor, first, count, tile);
}

}  // extern "C"

#ifdef PCMFIR_MAIN
#include <cstdio>
#include <vector>
// generated PCM of both widths, the three channel layouts, windows that begin and end anywhere, forwards and backwards, against the
// sum in 64-bit integers and the rounding written out
int main() {
    uint64_t state = 88172645463325252ull;
    auto rnd = [&](uint64_t m) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state % m; };
    unsigned calls = 0;
    for (int k = 0; k < 60; ++k) {
        const int width = 1 + (int)rnd(2), nch = 1 + (int)rnd(2), ir_nch = nch == 2 && rnd(2) ? 2 : 1;
        const uint64_t n = k < 50 ? 1 + rnd(300) : shpf::TILE_FRAMES - 2 + rnd(6);
        const uint32_t m = k < 50 ? 1 + (uint32_t)rnd(40) : shpf::TAP_CHUNK - 2 + (uint32_t)rnd(6);
        const double factor = k % 4 == 0 ? 1.0 : 1.0 / (double)(1u << (8 * width - 1 - rnd(3)));
        std::vector<unsigned char> x((size_t)(n * nch * width)), h((size_t)((uint64_t)m * ir_nch * width));
        for (auto& c : x) c = (unsigned char)(rnd(5) == 0 ? (rnd(2) ? 0x80 : 0x7f) : rnd(256));
        for (auto& c : h) c = (unsigned char)(rnd(5) == 0 ? (rnd(2) ? 0x80 : 0x7f) : rnd(256));
        const uint64_t total = shpf::result_frames(n, m), first = rnd(total), count = 1 + rnd(total - first);
        std::vector<unsigned char> got((size_t)(count * nch * width)), back(got.size());
        pf_host_convolve(x.data(), h.data(), width, n, m, nch, ir_nch, factor, first, count, got.data(), 0);
        pf_host_convolve(x.data(), h.data(), width, n, m, nch, ir_nch, factor, first, count, back.data(), 1);
        const double lo = width == 1 ? -128.0 : -32768.0, hi = width == 1 ? 127.0 : 32767.0;
        for (uint64_t i = first; i < first + count; ++i)
            for (int c = 0; c < nch; ++c) {
                int64_t acc = 0;
                for (uint32_t t = 0; t < m; ++t)
                    if (i >= t && i - t < n) acc += (int64_t)raw_sample(h.data(), width, (uint64_t)t * ir_nch + (ir_nch == 2 ? c : 0)) * raw_sample(x.data(), width, (i - t) * nch + c);
                double p = (double)acc * factor;
                if (p > hi) p = hi;
                else if (p < lo + 1.0) p = lo;
                const int32_t want = (int32_t)std::floor(p);
                const uint64_t s = (i - first) * nch + c;
                if (raw_sample(got.data(), width, s) != want || raw_sample(back.data(), width, s) != want) {
                    printf("case %d: width %d, %d channels under %d, frame %llu, channel %d\n", k, width, nch, ir_nch, (unsigned long long)i, c);
                    return 1;
                }
            }
        ++calls;
    }
    printf("pcmfir: %u calls ok\n", calls);
    return 0;
}
#endif
