// csrc/seqhist.hpp built for the host behind a few C functions (tests/test_seqhist.py drives them through ctypes): the blocks of a window
// of a song -- how many, which samples each counts, the block of a tile, where a row stands in the table -- and the fold of consecutive
// blocks into one.  With SEQHIST_MAIN it is a program of its own (its own main, generated windows and tables against a restatement in
// 128-bit integers in place), which a sanitizer build can run as it stands.
#include "../synthesizer_amd/csrc/seqhist.hpp"

extern "C" {

uint32_t sq_nblocks(uint64_t lo, uint64_t hi, uint32_t tile) { return shhs::nblocks(lo, hi, tile); }
uint32_t sq_tile_of(uint64_t s, uint32_t tile) { return shhs::tile_of(s, tile); }
uint32_t sq_block_of(uint32_t t, uint64_t lo, uint32_t tile) { return shhs::block_of(t, lo, tile); }
void sq_range(uint32_t j, uint64_t lo, uint64_t hi, uint32_t tile, uint64_t* a, uint64_t* b) { shhs::range(j, lo, hi, tile, *a, *b); }
uint64_t sq_row_at(uint32_t j, uint32_t nrows, uint32_t r) { return (uint64_t)shhs::row_at(j, nrows, r); }
void sq_fold(const shmt::Row* table, uint32_t j, uint32_t n, uint32_t nrows, shmt::Row* out) { shhs::fold(table, j, n, nrows, out); }

}  // extern "C"

#ifdef SEQHIST_MAIN
#include <cstdio>
#include <vector>
// windows at every alignment against the definition sample by sample (small tiles), the far end of the longest song, and folds of
// generated tables against 128-bit sums
int main() {
    typedef unsigned __int128 u128;
    uint64_t state = 88172645463325252ull;
    auto rnd = [&](uint64_t m) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state % m; };
    unsigned windows = 0, folds = 0;
    for (uint32_t tile : {4u, 8u}) {
        const uint64_t total = 5 * tile + 3;
        for (uint64_t lo = 0; lo <= total; ++lo)
            for (uint64_t hi = lo; hi <= total; ++hi) {
                const uint32_t nb = shhs::nblocks(lo, hi, tile);
                std::vector<uint32_t> count(nb, 0u);
                for (uint64_t s = lo; s < hi; ++s) {             // every sample of the window lies in exactly the block of its tile
                    const uint32_t j = shhs::block_of(shhs::tile_of(s, tile), lo, tile);
                    if (j >= nb) { printf("[%llu, %llu): sample %llu in block %u of %u\n", (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)s, j, nb); return 1; }
                    uint64_t a, b;
                    shhs::range(j, lo, hi, tile, a, b);
                    if (s < a || s >= b) { printf("[%llu, %llu): sample %llu outside its block\n", (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)s); return 1; }
                    ++count[j];
                }
                for (uint32_t j = 0; j < nb; ++j) {
                    uint64_t a, b;
                    shhs::range(j, lo, hi, tile, a, b);
                    if (b - a != count[j] || count[j] == 0) { printf("[%llu, %llu): block %u counts wrongly\n", (unsigned long long)lo, (unsigned long long)hi, j); return 1; }
                }
                ++windows;
            }
    }
    const uint64_t MAX = (1ull << 32) - 65536;
    for (uint32_t tile : {1024u, 2048u}) {
        if (shhs::nblocks(0, MAX, tile) != MAX / tile) { printf("the longest song has another block count\n"); return 1; }
        uint64_t a, b;
        shhs::range((uint32_t)(MAX / tile) - 1, 0, MAX, tile, a, b);
        if (a != MAX - tile || b != MAX) { printf("the last block of the longest song\n"); return 1; }
        shhs::range(0, MAX - 1, MAX, tile, a, b);
        if (a != MAX - 1 || b != MAX || shhs::nblocks(MAX - 1, MAX, tile) != 1) { printf("the last sample of the longest song\n"); return 1; }
    }
    if (shhs::row_at(4194239u, 41u, 40u) != (size_t)4194239ull * 41 + 40) { printf("a row offset wraps\n"); return 1; }
    for (int k = 0; k < 300; ++k) {
        const uint32_t nrows = 1 + (uint32_t)rnd(41), nb = 1 + (uint32_t)rnd(40);
        std::vector<shmt::Row> table((size_t)nrows * nb);
        for (auto& r : table)
            for (int c = 0; c < 2; ++c) {
                r.peak[c] = (uint32_t)rnd(1ull << 32);
                r.sq_hi[c] = rnd(1ull << 50);
                r.sq_lo[c] = rnd(1ull << 50);
            }
        const uint32_t j = (uint32_t)rnd(nb), n = (uint32_t)rnd(nb - j + 1);      // (n may be 0: the empty fold is the zero row)
        std::vector<shmt::Row> out(nrows);
        shhs::fold(table.data(), j, n, nrows, out.data());
        for (uint32_t r = 0; r < nrows; ++r)
            for (int c = 0; c < 2; ++c) {
                uint32_t peak = 0;
                u128 hi = 0, lo = 0;
                for (uint32_t b = j; b < j + n; ++b) {
                    const shmt::Row& x = table[(size_t)b * nrows + r];
                    if (x.peak[c] > peak) peak = x.peak[c];
                    hi += x.sq_hi[c];
                    lo += x.sq_lo[c];
                }
                if (out[r].peak[c] != peak || (u128)out[r].sq_hi[c] != hi || (u128)out[r].sq_lo[c] != lo) { printf("fold %d: row %u differs\n", k, r); return 1; }
            }
        ++folds;
    }
    printf("seqhist: %u windows, %u folds: ok\n", windows, folds);
    return 0;
}
#endif
