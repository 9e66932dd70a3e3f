// csrc/seqmeter.hpp built for the host behind a few C functions (tests/test_seqmeter.py drives them through ctypes): a lane's partial row of
// levels from its 4 or 8 samples cut to a window, two partial rows into one, and x * x as the two addends of a row.  With SEQMETER_MAIN it
// is a program of its own (its own main, generated lanes against a restatement in 128-bit integers in place), which a sanitizer build
// can run as it stands.
#include "../synthesizer_amd/csrc/seqmeter.hpp"

extern "C" {

uint32_t sm_row_bytes(void) { return (uint32_t)sizeof(shmt::Row); }
uint32_t sm_magnitude(int64_t x) { return shmt::magnitude((long long)x); }
void sm_square(int wide, uint32_t mag, uint64_t* hi, uint64_t* lo) {
    if (wide) shmt::square<true>(mag, *hi, *lo);
    else shmt::square<false>(mag, *hi, *lo);
}
// n: 4 or 8 samples x[0 .. n) at song samples s0 .., cut to [lo, hi)
void sm_lane(int wide, int n, const int64_t* x, uint32_t s0, uint32_t lo, uint32_t hi, uint32_t nch, shmt::Row* out) {
    long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < n; ++j) v[j] = (long long)x[j];
    if (n == 8) *out = wide ? shmt::lane<true, 8>(v, s0, lo, hi, nch) : shmt::lane<false, 8>(v, s0, lo, hi, nch);
    else *out = wide ? shmt::lane<true, 4>(v, s0, lo, hi, nch) : shmt::lane<false, 4>(v, s0, lo, hi, nch);
}
void sm_fold(shmt::Row* a, const shmt::Row* b) { shmt::fold(*a, *b); }

}  // extern "C"

#ifdef SEQMETER_MAIN
#include <cstdio>
#include <vector>
namespace {
typedef unsigned __int128 u128;
struct Ref { uint32_t peak[2]; u128 sq[2]; };
bool same(const shmt::Row& r, const Ref& w) {
    for (int c = 0; c < 2; ++c)
        if (r.peak[c] != w.peak[c] || ((u128)r.sq_hi[c] << 32) + r.sq_lo[c] != w.sq[c]) return false;
    return true;
}
}  // namespace
// lanes of 4 and 8 samples at every width's range and extremes, every cut, mono and stereo, against 128-bit integers; then 2^k partial
// rows folded forwards, backwards and pairwise
int main() {
    uint64_t state = 88172645463325252ull;
    auto rnd = [&](uint64_t m) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state % m; };
    const long long extremes[] = {-2147483648LL, 2147483647LL, -8388608LL, -128LL, 0LL, 1LL, -1LL, 32767LL, -32768LL};
    unsigned lanes = 0, folds = 0;
    for (int k = 0; k < 4000; ++k) {
        const int width = 1 + k % 4, n = width == 2 ? 8 : 4;
        const bool wide = width >= 3;
        const long long top = 1LL << (8 * width - 1);
        const uint32_t nch = 1 + (uint32_t)rnd(2), s0 = (uint32_t)rnd(1000) * (uint32_t)n;
        long long x[8];
        for (int j = 0; j < n; ++j) {
            x[j] = rnd(3) ? (long long)rnd(2 * (uint64_t)top) - top : extremes[rnd(9)];
            if (x[j] < -top) x[j] = -top;
            if (x[j] > top - 1) x[j] = top - 1;
        }
        for (int a = 0; a <= n; ++a)
            for (int b = a; b <= n; ++b) {                     // every cut [s0 + a, s0 + b), the empty ones too
                const uint32_t lo = s0 + (uint32_t)a, hi = s0 + (uint32_t)b;
                shmt::Row r;
                if (n == 8) r = wide ? shmt::lane<true, 8>(x, s0, lo, hi, nch) : shmt::lane<false, 8>(x, s0, lo, hi, nch);
                else r = wide ? shmt::lane<true, 4>(x, s0, lo, hi, nch) : shmt::lane<false, 4>(x, s0, lo, hi, nch);
                Ref w{{0, 0}, {0, 0}};
                for (int j = a; j < b; ++j) {
                    const int c = nch == 2 ? j & 1 : 0;
                    const u128 m = (u128)(x[j] < 0 ? -(__int128)x[j] : (__int128)x[j]);
                    if ((uint32_t)m > w.peak[c]) w.peak[c] = (uint32_t)m;
                    w.sq[c] += m * m;
                }
                if (!same(r, w)) { printf("lane %d cut [%d, %d): differs\n", k, a, b); return 1; }
                if (!wide && (r.sq_hi[0] | r.sq_hi[1])) { printf("lane %d: a narrow width has a high sum\n", k); return 1; }
                ++lanes;
            }
    }
    for (int k = 0; k < 200; ++k) {                           // 2^p rows of full-scale 32-bit lanes: three orders, one row
        const int p = 1 + k % 8, count = 1 << p;
        std::vector<shmt::Row> rows((size_t)count);
        for (auto& r : rows) {
            long long x[4];
            for (int j = 0; j < 4; ++j) x[j] = rnd(2) ? -2147483648LL : (long long)rnd(1ull << 32) - 2147483648LL;
            r = shmt::lane<true, 4>(x, 0, 0, 4, 2);
        }
        shmt::Row f = shmt::zero(), b = shmt::zero();
        for (int i = 0; i < count; ++i) shmt::fold(f, rows[(size_t)i]);
        for (int i = count - 1; i >= 0; --i) shmt::fold(b, rows[(size_t)i]);
        std::vector<shmt::Row> t = rows;
        for (int m = 1; m < count; m <<= 1)                   // the butterfly of a wave reduction
            for (int i = 0; i + m < count; i += 2 * m) shmt::fold(t[(size_t)i], t[(size_t)(i + m)]);
        for (int c = 0; c < 2; ++c)
            if (f.peak[c] != b.peak[c] || f.sq_hi[c] != b.sq_hi[c] || f.sq_lo[c] != b.sq_lo[c] || f.peak[c] != t[0].peak[c] ||
                f.sq_hi[c] != t[0].sq_hi[c] || f.sq_lo[c] != t[0].sq_lo[c]) { printf("fold %d: the order matters\n", k); return 1; }
        ++folds;
    }
    uint64_t hi, lo;
    shmt::square<true>(shmt::magnitude(-2147483648LL), hi, lo);
    if (hi != (1ull << 30) || lo != 0) { printf("2^62 splits wrongly\n"); return 1; }
    printf("seqmeter: %u lanes, %u folds: ok\n", lanes, folds);
    return 0;
}
#endif
