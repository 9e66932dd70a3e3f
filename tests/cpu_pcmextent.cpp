// csrc/pcmextent.hpp built for the host behind a few C functions (tests/test_pcmextent.py drives them through ctypes): a row, the
// identity, take and fold, the mono rule, and the whole call of sh_pcm_extent_blocks as a host loop over raw PCM of every width --
// forwards as the kernels divide it, and with every block's parts taken backwards.  With PCMEXTENT_MAIN it is a program of its own
// (its own main, generated PCM against a restatement frame by frame), which a sanitizer build can run as it stands.
#include "../synthesizer_amd/csrc/pcmextent.hpp"

namespace {
// sample s of raw little-endian PCM of `width` bytes a sample (width 1 signed; width 3: the raw 24-bit value, sign-extended)
int32_t raw_sample(const unsigned char* p, int width, uint64_t s) {
    p += s * (uint64_t)width;
    if (width == 1) return (int32_t)(signed char)p[0];
    if (width == 2) return (int32_t)(int16_t)((unsigned)p[0] | ((unsigned)p[1] << 8));
    if (width == 3) return ((int32_t)(((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16)) << 8)) >> 8;
    return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
}
}  // namespace

extern "C" {

uint32_t pe_row_bytes() { return (uint32_t)sizeof(shpe::Row); }
void pe_identity(shpe::Row* row) { *row = shpe::identity(); }
void pe_take(shpe::Row* row, uint64_t s, uint32_t nch, int32_t x) { shpe::take(*row, s, nch, x); }
void pe_fold(shpe::Row* a, const shpe::Row* b) { shpe::fold(*a, *b); }
void pe_stored(shpe::Row* row, uint32_t nch) { *row = shpe::stored(*row, nch); }

// the whole call: nplanes planes of n frames of nch channels, plane_samples samples apart from `pcm` on, into table
void pe_host_rows(const unsigned char* pcm, int width, uint64_t n, uint32_t nch, uint32_t nplanes, uint64_t plane_samples, uint64_t origin, uint64_t B,
                  shpe::Row* table) {
    auto get = [&](uint32_t r, uint64_t s) { return raw_sample(pcm, width, (uint64_t)r * plane_samples + s); };
    shpe::host_rows(get, n, nch, nplanes, origin, B, table);
}

// the same call with every block's part slots taken from the last to the first and every part's samples from the last to the first,
// the partial row folded INTO the part's (fold(one, all)) instead of the other way round: any order gives the same table
void pe_host_rows_backwards(const unsigned char* pcm, int width, uint64_t n, uint32_t nch, uint32_t nplanes, uint64_t plane_samples, uint64_t origin,
                            uint64_t B, shpe::Row* table) {
    const uint64_t nb = shpb::nblocks(origin, n, B), first = origin / B;
    const uint64_t slots = nb ? (uint64_t)1 << shpb::slot_shift(shpb::longest(origin, n, B) * nch) : 0;
    for (uint64_t j = nb; j-- > 0;) {
        uint64_t a, b;
        shpb::range(first, j, origin, n, B, a, b);
        for (uint32_t r = nplanes; r-- > 0;) {
            shpe::Row all = shpe::identity();
            for (uint64_t p = slots; p-- > 0;) {
                uint64_t s0, s1;
                shpb::part((b - a) * nch, p, s0, s1);
                shpe::Row one = shpe::identity();
                for (uint64_t s = s1; s-- > s0;) shpe::take(one, s, nch, raw_sample(pcm, width, (uint64_t)r * plane_samples + (a - origin) * nch + s));
                shpe::fold(one, all);
                all = one;
            }
            table[shpb::row_at(j, nplanes, r)] = shpe::stored(all, nch);
        }
    }
}

}  // extern "C"

#ifdef PCMEXTENT_MAIN
#include <cstdio>
#include <vector>
// the identity and the mono rule, then generated PCM of every width, mono and stereo, one plane and three, blocks of one part and of
// several, forwards and backwards against a restatement frame by frame
int main() {
    static_assert(sizeof(shpe::Row) == 16, "16-byte rows");
    uint64_t state = 88172645463325252ull;
    auto rnd = [&](uint64_t m) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state % m; };
    {
        shpe::Row id = shpe::identity(), row = {{-5, 7}, {9, 11}}, kept = row;
        shpe::fold(row, id);
        if (row.lo[0] != kept.lo[0] || row.lo[1] != kept.lo[1] || row.hi[0] != kept.hi[0] || row.hi[1] != kept.hi[1]) { printf("the identity changes a row\n"); return 1; }
        shpe::fold(id, kept);
        if (id.lo[0] != -5 || id.lo[1] != 7 || id.hi[0] != 9 || id.hi[1] != 11) { printf("the identity does not take a row\n"); return 1; }
        shpe::Row one = shpe::identity();
        shpe::take(one, 0, 1, INT32_MIN);
        shpe::take(one, 1, 1, INT32_MAX);
        if (one.lo[0] != INT32_MIN || one.hi[0] != INT32_MAX || one.lo[1] != INT32_MAX || one.hi[1] != INT32_MIN) { printf("a mono take\n"); return 1; }
        one = shpe::stored(one, 1);
        if (one.lo[1] != 0 || one.hi[1] != 0 || one.lo[0] != INT32_MIN || one.hi[0] != INT32_MAX) { printf("the mono rule\n"); return 1; }
    }
    const uint64_t P = shpb::PART_SAMPLES;
    unsigned calls = 0;
    for (int k = 0; k < 160; ++k) {
        const int width = 1 + (int)rnd(4);
        const uint32_t nch = 1 + (uint32_t)rnd(2), nplanes = rnd(2) ? 1u : 3u;
        const uint64_t n = k < 150 ? rnd(300) : P + rnd(2 * P), B = k < 150 ? 1 + rnd(120) : P / 2 + rnd(3 * P), origin = rnd(1000);
        const uint64_t plane = n * nch + rnd(5);
        std::vector<unsigned char> pcm((size_t)(nplanes * plane * width + 1));
        for (auto& c : pcm) c = (unsigned char)(rnd(5) == 0 ? (rnd(2) ? 0x80 : 0x7f) : rnd(256));
        if (k % 3 == 0) for (auto& c : pcm) c |= 0x80;           // every sample negative: hi < 0, which an accumulator that starts at 0 misses
        const uint64_t nb = shpb::nblocks(origin, n, B);
        std::vector<shpe::Row> table((size_t)(nb * nplanes + 1)), back((size_t)(nb * nplanes + 1));
        pe_host_rows(pcm.data(), width, n, nch, nplanes, plane, origin, B, table.data());
        pe_host_rows_backwards(pcm.data(), width, n, nch, nplanes, plane, origin, B, back.data());
        for (uint64_t j = 0; j < nb; ++j)
            for (uint32_t r = 0; r < nplanes; ++r) {
                int64_t lo[2] = {INT32_MAX, INT32_MAX}, hi[2] = {INT32_MIN, INT32_MIN};
                for (uint64_t f = 0; f < n; ++f) {
                    if ((origin + f) / B - origin / B != j) continue;
                    for (uint32_t c = 0; c < nch; ++c) {
                        const int64_t x = raw_sample(pcm.data(), width, r * plane + f * nch + c);
                        if (x < lo[c]) lo[c] = x;
                        if (x > hi[c]) hi[c] = x;
                    }
                }
                if (nch == 1) lo[1] = hi[1] = 0;
                const shpe::Row& got = table[shpb::row_at(j, nplanes, r)];
                const shpe::Row& rev = back[shpb::row_at(j, nplanes, r)];
                for (int c = 0; c < 2; ++c)
                    if (got.lo[c] != lo[c] || got.hi[c] != hi[c] || rev.lo[c] != lo[c] || rev.hi[c] != hi[c]) {
                        printf("case %d: width %d, %u channels, block %llu, plane %u, channel %d\n", k, width, nch, (unsigned long long)j, r, c);
                        return 1;
                    }
            }
        ++calls;
    }
    printf("pcmextent: %u calls ok\n", calls);
    return 0;
}
#endif
