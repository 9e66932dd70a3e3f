// csrc/pcmblocks.hpp built for the host behind a few C functions (tests/test_pcmblocks.py drives them through ctypes): the blocks of a
// call of sh_pcm_level_blocks -- how many, which frames each counts, the parts of a block, the part slots of a call -- and the whole
// call as a host loop over raw PCM of every width.  With PCMBLOCKS_MAIN it is a program of its own (its own main, generated windows and
// PCM against a restatement sample by sample in 128-bit integers), which a sanitizer build can run as it stands.
#include "../synthesizer_amd/csrc/pcmblocks.hpp"

namespace {
// sample s of raw little-endian PCM of `width` bytes a sample (width 3: the raw 24-bit value, sign-extended)
long long raw_sample(const unsigned char* p, int width, uint64_t s) {
    p += s * (uint64_t)width;
    if (width == 1) return (long long)(signed char)p[0];
    if (width == 2) return (long long)(int16_t)((unsigned)p[0] | ((unsigned)p[1] << 8));
    if (width == 3) return (long long)(((int32_t)(((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16)) << 8)) >> 8);
    return (long long)(int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
}
}  // namespace

extern "C" {

uint32_t pb_part_samples() { return shpb::PART_SAMPLES; }
uint64_t pb_nblocks(uint64_t origin, uint64_t n, uint64_t B) { return shpb::nblocks(origin, n, B); }
void pb_range(uint64_t j, uint64_t origin, uint64_t n, uint64_t B, uint64_t* a, uint64_t* b) { shpb::range(origin / B, j, origin, n, B, *a, *b); }
uint64_t pb_longest(uint64_t origin, uint64_t n, uint64_t B) { return shpb::longest(origin, n, B); }
uint64_t pb_parts_of(uint64_t samples) { return shpb::parts_of(samples); }
void pb_part(uint64_t samples, uint64_t p, uint64_t* s0, uint64_t* s1) { shpb::part(samples, p, *s0, *s1); }
uint32_t pb_slot_shift(uint64_t samples) { return shpb::slot_shift(samples); }
uint64_t pb_row_at(uint64_t j, uint32_t nplanes, uint32_t r) { return (uint64_t)shpb::row_at(j, nplanes, r); }

// the whole call: nplanes planes of n frames of nch channels, plane_samples samples apart from `pcm` on, into table
void pb_host_rows(const unsigned char* pcm, int width, uint64_t n, uint32_t nch, uint32_t nplanes, uint64_t plane_samples, uint64_t origin, uint64_t B,
                  shmt::Row* table) {
    auto get = [&](uint32_t r, uint64_t s) { return raw_sample(pcm, width, (uint64_t)r * plane_samples + s); };
    if (width >= 3) shpb::host_rows<true>(get, n, nch, nplanes, origin, B, table);
    else shpb::host_rows<false>(get, n, nch, nplanes, origin, B, table);
}

}  // extern "C"

#ifdef PCMBLOCKS_MAIN
#include <cstdio>
#include <vector>
// windows at every alignment against the definition frame by frame, the parts of ranges around the part size, and generated PCM of every
// width, mono and stereo, one plane and three, against sums in 128 bits
int main() {
    typedef unsigned __int128 u128;
    uint64_t state = 88172645463325252ull;
    auto rnd = [&](uint64_t m) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state % m; };
    unsigned windows = 0, ranges = 0, calls = 0;
    for (uint64_t B : {1ull, 4ull, 7ull})
        for (uint64_t origin = 0; origin <= 2 * B + 1; ++origin)
            for (uint64_t n = 0; n <= 3 * B + 2; ++n) {
                const uint64_t nb = shpb::nblocks(origin, n, B);
                std::vector<uint64_t> count(nb, 0);
                for (uint64_t f = origin; f < origin + n; ++f) {
                    const uint64_t j = f / B - origin / B;
                    if (j >= nb) { printf("origin %llu n %llu B %llu: frame in block %llu of %llu\n", (unsigned long long)origin, (unsigned long long)n, (unsigned long long)B, (unsigned long long)j, (unsigned long long)nb); return 1; }
                    uint64_t a, b;
                    shpb::range(origin / B, j, origin, n, B, a, b);
                    if (f < a || f >= b) { printf("origin %llu n %llu B %llu: a frame outside its block\n", (unsigned long long)origin, (unsigned long long)n, (unsigned long long)B); return 1; }
                    ++count[j];
                }
                uint64_t longest = 0;
                for (uint64_t j = 0; j < nb; ++j) {
                    uint64_t a, b;
                    shpb::range(origin / B, j, origin, n, B, a, b);
                    if (b - a != count[j] || !count[j]) { printf("origin %llu n %llu B %llu: block %llu counts wrongly\n", (unsigned long long)origin, (unsigned long long)n, (unsigned long long)B, (unsigned long long)j); return 1; }
                    if (count[j] > longest) longest = count[j];
                }
                if (nb && shpb::longest(origin, n, B) != longest) { printf("origin %llu n %llu B %llu: the longest block\n", (unsigned long long)origin, (unsigned long long)n, (unsigned long long)B); return 1; }
                ++windows;
            }
    {   // far positions: a block of 2^33 frames behind 2^32, and the end of the 64-bit range
        uint64_t a, b;
        const uint64_t B = 1ull << 33, origin = (1ull << 32) + 3;
        if (shpb::nblocks(origin, 3 * B - 2, B) != 4) { printf("far: the count\n"); return 1; }
        shpb::range(origin / B, 3, origin, 3 * B - 2, B, a, b);
        if (a != 3 * B || b != origin + 3 * B - 2) { printf("far: the last block\n"); return 1; }
        shpb::range((~0ull - 9) >> 63, 0, ~0ull - 9, 9, 1ull << 63, a, b);
        if (a != ~0ull - 9 || b != ~0ull || shpb::nblocks(~0ull - 9, 9, 1ull << 63) != 1) { printf("far: the end of the range\n"); return 1; }
    }
    const uint64_t P = shpb::PART_SAMPLES;
    for (uint64_t samples : {(uint64_t)1, (uint64_t)2, P - 1, P, P + 1, 2 * P, 3 * P + 5, 5 * P - 2}) {
        const uint64_t np = shpb::parts_of(samples), slots = 1ull << shpb::slot_shift(samples);
        if (np != (samples + P - 1) / P || slots < np || (slots > 1 && slots / 2 >= np)) { printf("%llu samples: parts and slots\n", (unsigned long long)samples); return 1; }
        uint64_t at = 0;
        for (uint64_t p = 0; p < slots + 2; ++p) {
            uint64_t s0, s1;
            shpb::part(samples, p, s0, s1);
            if (p < np ? (s0 != at || s1 <= s0 || s1 - s0 > P || (s0 & 1)) : (s0 != samples || s1 != samples)) { printf("%llu samples: part %llu\n", (unsigned long long)samples, (unsigned long long)p); return 1; }
            at = s1;
        }
        if (at != samples) { printf("%llu samples: the parts do not end at the range's end\n", (unsigned long long)samples); return 1; }
        ++ranges;
    }
    for (int k = 0; k < 160; ++k) {
        const int width = 1 + (int)rnd(4);
        const uint32_t nch = 1 + (uint32_t)rnd(2), nplanes = rnd(2) ? 1u : 3u;
        const uint64_t n = k < 150 ? rnd(300) : P + rnd(2 * P), B = k < 150 ? 1 + rnd(120) : P / 2 + rnd(3 * P), origin = rnd(1000);
        const uint64_t plane = n * nch + rnd(5);
        std::vector<unsigned char> pcm((size_t)(nplanes * plane * width + 1));
        for (auto& c : pcm) c = (unsigned char)(rnd(5) == 0 ? (rnd(2) ? 0x80 : 0x7f) : rnd(256));      // (a top byte 0x80 over zeros: the rail)
        const uint64_t nb = shpb::nblocks(origin, n, B);
        std::vector<shmt::Row> table((size_t)(nb * nplanes + 1));
        pb_host_rows(pcm.data(), width, n, nch, nplanes, plane, origin, B, table.data());
        for (uint64_t j = 0; j < nb; ++j)
            for (uint32_t r = 0; r < nplanes; ++r) {
                u128 sum[2] = {0, 0};
                uint64_t peak[2] = {0, 0};
                for (uint64_t f = 0; f < n; ++f) {
                    if ((origin + f) / B - origin / B != j) continue;
                    for (uint32_t c = 0; c < nch; ++c) {
                        const long long x = raw_sample(pcm.data(), width, r * plane + f * nch + c);
                        const uint64_t m = (uint64_t)(x < 0 ? -x : x);
                        sum[c] += (u128)m * m;
                        if (m > peak[c]) peak[c] = m;
                    }
                }
                const shmt::Row& got = table[shpb::row_at(j, nplanes, r)];
                for (int c = 0; c < 2; ++c)
                    if (got.peak[c] != peak[c] || (((u128)got.sq_hi[c] << 32) + got.sq_lo[c]) != sum[c] || (width < 3 && got.sq_hi[c])) {
                        printf("case %d: width %d, %u channels, block %llu, plane %u, channel %d\n", k, width, nch, (unsigned long long)j, r, c);
                        return 1;
                    }
            }
        ++calls;
    }
    printf("pcmblocks: %u windows, %u ranges, %u calls ok\n", windows, ranges, calls);
    return 0;
}
#endif
