// Host build of synthesizer_amd/csrc/seqauto.hpp for tests/test_seqauto.py (g++ -ffp-contract=off, no GPU): the search for a tile's first
// segment, and a track shaped the way the automation kernels of sequence.hip shape a sub-mix -- the track cut into tiles of `tile` samples,
// per tile sha::find from the tile's first sample, every lane taking `lane` consecutive samples at SONG positions through sha::shape_from.
// sa_selfcheck holds both against brute force (a linear scan for the segment, she::gain sample by sample); with -DSEQAUTO_MAIN the file is
// a program that runs it, for a stand-alone build under -fsanitize=address,undefined.
#include "../synthesizer_amd/csrc/seqauto.hpp"
#include <stdio.h>
#include <string.h>
#include <vector>

namespace {

int get(const unsigned char* p, int width, uint64_t i) {
    if (width == 1) return (int)(signed char)p[i];
    if (width == 2) { int16_t v; memcpy(&v, p + 2 * i, 2); return v; }
    int32_t v;
    memcpy(&v, p + 4 * i, 4);
    return v;
}

void put(unsigned char* p, int width, uint64_t i, int x) {
    for (int b = 0; b < width; ++b) p[(uint64_t)width * i + b] = (unsigned char)(((unsigned)x >> (8 * b)) & 0xFF);
}

template <int N>
void run(const unsigned char* in, int width, uint32_t n, const she::Seg* segs, uint32_t nseg, uint32_t tile, unsigned char* out) {
    const double hi = width == 1 ? 127.0 : (width == 2 ? 32767.0 : 2147483647.0), lo = -hi - 1.0;
    for (uint32_t t0 = 0; t0 < n; t0 += tile) {
        const uint32_t i = sha::find(segs, nseg, t0);           // once per tile, as once per run in the kernels
        for (uint32_t s0 = t0; s0 < t0 + tile; s0 += N) {
            int x[N];
            for (int k = 0; k < N; ++k) x[k] = s0 + k < n ? get(in, width, s0 + k) : 0;
            sha::shape_from<N>(segs, nseg, i, t0, t0 + tile, (long long)s0, x, lo, hi);
            for (int k = 0; k < N; ++k)
                if (s0 + k < n) put(out, width, s0 + k, x[k]);
        }
    }
}

// brute force: the segment of sample s by a scan from the first, she::gain on it
int brute(const she::Seg* segs, uint32_t nseg, uint32_t s, int x, double lo, double hi) {
    for (uint32_t g = 0; g < nseg; ++g)
        if (segs[g].end > s) return she::gain(segs[g], (long long)s, x, lo, hi);
    return x;
}

// a table of moves: npieces pieces of `len` samples with `gap` samples between them from `start` on, plain segments in the gaps
std::vector<she::Seg> table(uint32_t start, uint32_t npieces, uint32_t len, uint32_t gap) {
    std::vector<she::Seg> t;
    uint32_t at = 0, a = start;
    for (uint32_t p = 0; p < npieces; ++p, a += len + gap) {
        if (a > at) t.push_back(she::Seg{1.0, 0.0, 0.0, 0.0, a, 0, she::NONE, 0});
        const double v0 = (p % 5) * 0.25, v1 = ((3 * p + 1) % 5) * 0.25;
        t.push_back(she::Seg{1.0, v1 - v0, (double)len, v0, a + len, a, she::FADE_IN, 0});
        at = a + len;
    }
    return t;
}

template <int N>
int check_lanes(const std::vector<she::Seg>& t, uint32_t n, uint32_t tile) {
    int bad = 0;
    const double hi = 32767.0, lo = -32768.0;
    const uint32_t nseg = (uint32_t)t.size();
    for (uint32_t t0 = 0; t0 < n; t0 += tile) {
        const uint32_t i = sha::find(t.data(), nseg, t0);
        for (uint32_t s0 = t0; s0 < t0 + tile; s0 += N) {
            int x[N], want[N];
            for (int k = 0; k < N; ++k) {
                x[k] = (int)((s0 + k) * 2654435761u % 65536u) - 32768;
                want[k] = brute(t.data(), nseg, s0 + k, x[k], lo, hi);
            }
            sha::shape_from<N>(t.data(), nseg, i, t0, t0 + tile, (long long)s0, x, lo, hi);
            for (int k = 0; k < N; ++k) bad += x[k] != want[k];
        }
    }
    return bad;
}

}  // namespace

extern "C" {

unsigned sa_find(const void* segs, uint32_t n, uint32_t s) { return sha::find((const she::Seg*)segs, n, s); }

// out[0 .. n) = the n samples of `in` shaped by segs (song positions from 0).  lane: 4 or 8; tile: a multiple of lane.  0, or -1.
int sa_shape(const unsigned char* in, int width, uint32_t n, const void* segs, uint32_t nseg, uint32_t tile, int lane, unsigned char* out) {
    const she::Seg* g = (const she::Seg*)segs;
    if (tile % (uint32_t)lane) return -1;
    if (lane == 8) run<8>(in, width, n, g, nseg, tile, out);
    else if (lane == 4) run<4>(in, width, n, g, nseg, tile, out);
    else return -1;
    return 0;
}

// the search on tables of 0, 1, 2 and 1000 segments for every s around every boundary, the lane function at N = 4 and 8 on tiles inside
// one segment, tiles that straddle one boundary and tiles that hold several one-frame pieces: the number of mismatches
int sa_selfcheck() {
    int bad = 0;
    const uint32_t counts[] = {0, 1, 2, 1000};
    for (uint32_t n : counts) {
        std::vector<she::Seg> t(n);
        for (uint32_t g = 0; g < n; ++g) t[g] = she::Seg{1.0, 0.0, 0.0, 0.0, 7 + 13 * g + (g % 3), 0, she::NONE, 0};
        auto want = [&](uint32_t s) {
            uint32_t g = 0;
            while (g < n && t[g].end <= s) ++g;
            return g;
        };
        bad += sha::find(t.data(), n, 0) != want(0);
        bad += sha::find(t.data(), n, 0xFFFFFFFFu) != n;
        for (uint32_t g = 0; g < n; ++g)
            for (int d = -3; d <= 3; ++d) {
                const uint32_t s = (uint32_t)((long long)t[g].end + d);
                bad += sha::find(t.data(), n, s) != want(s);
            }
    }
    // (start, pieces, length, gap, samples, tile): long pieces (tiles inside one segment, tiles across one boundary), one-sample and
    // two-sample pieces (several to a tile and to a lane), no table at all, a tile past the last segment
    const uint32_t shapes[][6] = {{5, 3, 700, 90, 4096, 256}, {0, 2, 2048, 0, 4096, 1024}, {3, 600, 1, 1, 2048, 64}, {0, 500, 2, 1, 2048, 32},
                                  {0, 0, 1, 1, 512, 64},     {1, 513, 3, 1, 4096, 2048},  {100, 1, 50, 0, 1024, 128}};
    for (const auto& s : shapes) {
        const std::vector<she::Seg> t = table(s[0], s[1], s[2], s[3]);
        bad += check_lanes<4>(t, s[4], s[5]);
        bad += check_lanes<8>(t, s[4], s[5]);
    }
    return bad;
}

}

#ifdef SEQAUTO_MAIN
int main() {
    const int bad = sa_selfcheck();
    printf("cpu_seqauto: %d mismatches\n", bad);
    return bad ? 1 : 0;
}
#endif
