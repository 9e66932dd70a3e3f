// csrc/seqclip.hpp built for the host behind a few C functions (tests/test_seqclip.py drives them through ctypes): the two predicates of an
// over -- a saturating add that clamps, a multiply whose floor leaves the range --, the 16-bit form the kernels evaluate on packed samples,
// a lane's count cut to a window, and the fold.  With SEQCLIP_MAIN it is a program of its own (its own main: the 16-bit equivalence over a
// stated set of pairs that includes both rails, the add at width 1 over every pair, generated lanes and folds against restatements in
// place), which a sanitizer build can run as it stands.
#include "../synthesizer_amd/csrc/seqclip.hpp"

extern "C" {

int sc_add_clamps(int width, long long acc, long long x) {
    switch (width) {
    case 1: return shcl::add_clamps<1>(acc, x);
    case 2: return shcl::add_clamps<2>(acc, x);
    case 3: return shcl::add_clamps<3>(acc, x);
    default: return shcl::add_clamps<4>(acc, x);
    }
}
int sc_mul_clamps(int width, double p) {
    switch (width) {
    case 1: return shcl::mul_clamps<1>(p);
    case 2: return shcl::mul_clamps<2>(p);
    case 3: return shcl::mul_clamps<3>(p);
    default: return shcl::mul_clamps<4>(p);
    }
}
int sc_add_clamps16(int a, int x) { return shcl::add_clamps16((int16_t)a, (int16_t)x); }
int sc_sat16(int a, int x) { return shcl::sat16((int16_t)a, (int16_t)x); }
int sc_wrap16(int a, int x) { return shcl::wrap16((int16_t)a, (int16_t)x); }
// every pair (a, x) of 16-bit values with x in {x0, x0 + stride, ...}: the number of pairs at which add_clamps16 and the exact sum disagree
uint64_t sc_disagree16(int x0, int stride) {
    uint64_t bad = 0;
    for (int a = -32768; a <= 32767; ++a)
        for (int x = x0; x <= 32767; x += stride) {
            const int t = a + x;
            if (shcl::add_clamps16((int16_t)a, (int16_t)x) != (t > 32767 || t < -32768)) ++bad;
        }
    return bad;
}
// a lane of eight (flags: eight shorts, 0 or not) and a lane of four (bits of a word)
void sc_lane8(const short* flags, uint32_t s0, uint32_t lo, uint32_t hi, uint32_t nch, uint32_t* out) {
    const shcl::Count c = shcl::lane<8>(flags, s0, lo, hi, nch);
    out[0] = c.c[0];
    out[1] = c.c[1];
}
void sc_lane4(uint32_t bits, uint32_t s0, uint32_t lo, uint32_t hi, uint32_t nch, uint32_t* out) {
    const shcl::Count c = shcl::lane<4>(shcl::Bits{bits}, s0, lo, hi, nch);
    out[0] = c.c[0];
    out[1] = c.c[1];
}
void sc_fold_counts(uint32_t* a, const uint32_t* b) {
    shcl::Count x{{a[0], a[1]}};
    shcl::fold(x, shcl::Count{{b[0], b[1]}});
    a[0] = x.c[0];
    a[1] = x.c[1];
}
void sc_fold_rows(shcl::Row* a, const shcl::Row* b) { shcl::fold(*a, *b); }
uint32_t sc_row_size() { return (uint32_t)sizeof(shcl::Row); }
uint32_t sc_clipped_offset() {
    shcl::Row r{};
    return (uint32_t)((const char*)&r.clipped[0] - (const char*)&r);
}

}  // extern "C"

#ifdef SEQCLIP_MAIN
#include <cstdio>
int main() {
    // the 16-bit equivalence: every a against x on a stride of 61 from the lower rail on (1075 values of x) and the 64 values at each
    // rail, 2^16 * 1203 pairs
    uint64_t bad = sc_disagree16(-32768, 61);
    for (int x = -32768; x < -32768 + 64; ++x) bad += sc_disagree16(x, 1 << 20);
    for (int x = 32767 - 63; x <= 32767; ++x) bad += sc_disagree16(x, 1 << 20);
    if (bad) { printf("16 bits: %llu pairs where saturating != wrapping disagrees with the exact sum\n", (unsigned long long)bad); return 1; }
    // the add at width 1, every pair of saturated values
    for (int a = -128; a <= 127; ++a)
        for (int x = -128; x <= 127; ++x)
            if (shcl::add_clamps<1>(a, x) != (a + x > 127 || a + x < -128)) { printf("width 1: %d + %d\n", a, x); return 1; }
    // products around the rails
    if (shcl::mul_clamps<2>(32767.0) || shcl::mul_clamps<2>(32767.5) || !shcl::mul_clamps<2>(32768.0) || shcl::mul_clamps<2>(-32768.0) ||
        !shcl::mul_clamps<2>(-32768.25) || !shcl::mul_clamps<2>(-32769.0)) { printf("the multiply at the rails of width 2\n"); return 1; }
    // generated lanes against a count sample by sample, and folds in both orders
    uint64_t state = 88172645463325252ull;
    auto rnd = [&](uint64_t m) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state % m; };
    unsigned lanes = 0;
    for (int k = 0; k < 20000; ++k) {
        short f[8];
        uint32_t bits = 0;
        for (int j = 0; j < 8; ++j) f[j] = rnd(3) ? 0 : (short)-1;
        for (int j = 0; j < 4; ++j) bits |= (f[j] ? 1u : 0u) << j;
        const uint32_t s0 = 8 * (uint32_t)rnd(64), lo = (uint32_t)rnd(560), hi = lo + (uint32_t)rnd(40), nch = 1 + (uint32_t)rnd(2);
        uint32_t want8[2] = {0, 0}, want4[2] = {0, 0};
        for (uint32_t j = 0; j < 8; ++j)
            if (s0 + j >= lo && s0 + j < hi && f[j]) {
                ++want8[nch == 2 ? j & 1 : 0];
                if (j < 4) ++want4[nch == 2 ? j & 1 : 0];
            }
        const shcl::Count c8 = shcl::lane<8>(f, s0, lo, hi, nch), c4 = shcl::lane<4>(shcl::Bits{bits}, s0, lo, hi, nch);
        if (c8.c[0] != want8[0] || c8.c[1] != want8[1] || c4.c[0] != want4[0] || c4.c[1] != want4[1]) { printf("lane %d counts wrongly\n", k); return 1; }
        shcl::Count ab = c8, ba = c4;
        shcl::fold(ab, c4);
        shcl::fold(ba, c8);
        if (ab.c[0] != ba.c[0] || ab.c[1] != ba.c[1] || ab.c[0] != c8.c[0] + c4.c[0]) { printf("fold %d\n", k); return 1; }
        ++lanes;
    }
    printf("seqclip: %u pairs at 16 bits, %u lanes: ok\n", 65536u * 1203u, lanes);
    return 0;
}
#endif
