// seqhist.hpp -- the level HISTORY of a song of tracks (sh_seq_render_history, sequence.hip): the rows of seqmeter.hpp kept per BLOCK of the
// window instead of merged into one row set.  A block is one tile of the SONG's tile grid (shq::tile_samples(width) samples: the tile a
// window workgroup folds anyway), cut to the window: a render of song samples [lo, hi) has
//     nblocks = (hi - 1) / TILE - lo / TILE + 1                                  (0 for an empty window)
// blocks, block j being song tile lo / TILE + j and counting the samples
//     [max(lo, (lo / TILE + j) * TILE), min(hi, (lo / TILE + j + 1) * TILE)),
// so the first and the last block of a window may be partial, and a song block that lies whole inside two windows reads the same from
// both.  The table is block-major: block j holds its nrows rows (tracks, master, groups -- the meter table's order) one behind the other,
// row r of block j at j * nrows + r, formed in size_t (a song of 2^32 - 65536 samples at width 1 has 4 194 240 blocks of up to 41 rows).
// Every block is written by exactly ONE workgroup, the one that folds its tile, so plain stores fill the table, nothing zeroes it first
// and the result does not depend on the order the workgroups run in.  Coarser blocks are folds of consecutive ones: max of the peaks,
// integer sums -- shmt::fold, in any order.
// Plain C++17 integers, no intrinsics, SH_HD (tests/cpu_seqhist.cpp builds it with g++).
#pragma once
#include <cstddef>
#include <cstdint>

#include "seqmeter.hpp"

namespace shhs {

// the song tile that holds song sample s
SH_HD uint32_t tile_of(uint64_t s, uint32_t tile) { return (uint32_t)(s / tile); }

// the blocks of the window [lo, hi)
SH_HD uint32_t nblocks(uint64_t lo, uint64_t hi, uint32_t tile) { return hi > lo ? tile_of(hi - 1, tile) - tile_of(lo, tile) + 1u : 0u; }

// the block of song tile t in a window that starts at sample lo (t >= lo / tile: the window's workgroups fold no tile in front of it)
SH_HD uint32_t block_of(uint32_t t, uint64_t lo, uint32_t tile) { return t - tile_of(lo, tile); }

// the song samples [a, b) that block j of the window [lo, hi) counts, in 64 bits: (t + 1) * tile passes 2^32 in the last tile of the
// longest song
SH_HD void range(uint32_t j, uint64_t lo, uint64_t hi, uint32_t tile, uint64_t& a, uint64_t& b) {
    const uint64_t t = (uint64_t)tile_of(lo, tile) + j;
    a = t * tile;
    b = a + tile;
    if (a < lo) a = lo;
    if (b > hi) b = hi;
}

// where row r of block j stands in a table of nrows rows per block, in rows
SH_HD size_t row_at(uint32_t j, uint32_t nrows, uint32_t r) { return (size_t)j * nrows + r; }

// n consecutive blocks, from block j on, into one: out[0 .. nrows)
SH_HD void fold(const shmt::Row* table, uint32_t j, uint32_t n, uint32_t nrows, shmt::Row* out) {
    for (uint32_t r = 0; r < nrows; ++r) {
        shmt::Row sum = shmt::zero();
        for (uint32_t k = 0; k < n; ++k) shmt::fold(sum, table[row_at(j + k, nrows, r)]);
        out[r] = sum;
    }
}

}  // namespace shhs
