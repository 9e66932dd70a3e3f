// pcmblocks.hpp -- the levels PER BLOCK of PCM that already lies in device memory (sh_pcm_level_blocks, pcm_ops.hip): the rows of
// seqmeter.hpp -- per channel the peak (audioop.max) and the exact integer sum of squares, sq_hi * 2^32 + sq_lo, one sum at widths 1
// and 2, two at widths 3 and 4, a mono input filling channel 0 and leaving channel 1 at 0 -- kept per block of a frame grid, for one
// plane or many.  shmt::add and shmt::fold are the only arithmetic.
// Positions are FRAMES in 64 bits.  Frame i of the input stands at grid frame origin + i; block j of a call is grid block
// origin / B + j, cut to [origin, origin + n): a call has
//     nblocks = (origin + n - 1) / B - origin / B + 1                           (0 for n == 0)
// blocks -- seqhist.hpp's rule with frames in place of tiles -- so the first and the last block may be partial, and a block that lies
// whole inside two calls reads the same from both.  The table is block-major: row r of block j at j * nplanes + r (shhs::row_at's
// order, formed in size_t here because a call may have more than 2^32 blocks).
// A block's cut range is divided into consecutive PARTS of at most PART_SAMPLES samples (samples: frames times channels; the constant
// is even, so a part of a stereo input starts on a frame), the last one shorter.  PART_SAMPLES is at least 4096, so a song tile (2048
// samples at 16 bits, 1024 otherwise) is always one part.  One workgroup reads one part of one plane; a call whose longest block is one
// part stores its rows straight into the table, any other call stores partial rows that a second kernel folds -- integer max and
// integer add, so the table is the same for every split.  Every block of a call owns the same number of part slots, the parts of the
// longest block rounded up to a power of two, and a slot behind a block's last part is an empty range whose row is zero: folding it
// changes nothing.
// Plain C++17 integers, no intrinsics, SH_HD (tests/cpu_pcmblocks.cpp builds it with g++).
#pragma once
#include <cstddef>
#include <cstdint>

#include "seqmeter.hpp"

namespace shpb {

constexpr uint32_t PART_SAMPLES = 8192;         // the samples one workgroup reads at most: 16 KB at 16 bits, four 16-byte vectors a lane
static_assert(PART_SAMPLES >= 4096 && PART_SAMPLES % 2 == 0, "a song tile is one part, and a stereo part starts on a frame");

// the blocks of n frames from grid frame origin on, in blocks of B frames (B > 0, origin + n does not pass 2^64)
SH_HD uint64_t nblocks(uint64_t origin, uint64_t n, uint64_t B) { return n ? (origin + n - 1) / B - origin / B + 1 : 0; }

// the grid frames [a, b) that block j of the call counts; first = origin / B, the grid block of block 0 (the kernel is handed it: one
// division on the host, none per workgroup).  first + j is a block of the call, so (first + j) * B <= origin + n - 1 does not overflow,
// and the block's end is formed from the frames left, never as a + B (B may be 2^63)
SH_HD void range(uint64_t first, uint64_t j, uint64_t origin, uint64_t n, uint64_t B, uint64_t& a, uint64_t& b) {
    const uint64_t end = origin + n;
    a = (first + j) * B;
    b = end - a > B ? a + B : end;
    if (a < origin) a = origin;
}

// the frames of the longest block of a call of nb = nblocks(origin, n, B) > 0 blocks: a whole one where there are three, else the
// longer of the two ends
SH_HD uint64_t longest(uint64_t origin, uint64_t n, uint64_t B) {
    const uint64_t nb = nblocks(origin, n, B);
    if (nb <= 1) return n;
    if (nb > 2) return B;
    const uint64_t head = (origin / B + 1) * B - origin;
    return head > n - head ? head : n - head;
}

// the parts of a range of `samples` samples
SH_HD uint64_t parts_of(uint64_t samples) { return samples / PART_SAMPLES + (samples % PART_SAMPLES ? 1 : 0); }

// the samples [s0, s1) of part p of a range of `samples` samples, counted from the range's first; empty (s0 == s1 == samples) for a
// slot behind the last part
SH_HD void part(uint64_t samples, uint64_t p, uint64_t& s0, uint64_t& s1) {
    s0 = p < parts_of(samples) ? p * PART_SAMPLES : samples;
    s1 = samples - s0 > PART_SAMPLES ? s0 + PART_SAMPLES : samples;
}

// the part slots every block of a call owns, as a shift: the parts of the longest block's `samples` samples rounded up to a power of two,
// so that workgroup w of a plane finds its block and slot (w >> shift, w & (2^shift - 1)) without a division
SH_HD uint32_t slot_shift(uint64_t samples) {
    uint32_t shift = 0;
    while (((uint64_t)1 << shift) < parts_of(samples)) ++shift;
    return shift;
}

// where row r of block j stands in a table of nplanes rows per block, in rows
SH_HD size_t row_at(uint64_t j, uint32_t nplanes, uint32_t r) { return (size_t)j * nplanes + r; }

// one sample of a plane into its row: sample s of the plane (counted from the plane's first) belongs to channel s & 1 of a stereo
// input and to channel 0 of a mono one
template <bool WIDE>
SH_HD void take(shmt::Row& row, uint64_t s, uint32_t nch, long long x) {
    if (nch == 2 && (s & 1)) shmt::add<WIDE>(row, 1, x);
    else shmt::add<WIDE>(row, 0, x);
}

// The whole call on the host, as the two kernels divide it: per block and plane, the part slots of the call one by one, each into a
// partial row, the partial rows folded.  get(r, s): sample s of plane r.  table: nblocks * nplanes rows.
template <bool WIDE, typename Get>
static inline void host_rows(Get&& get, uint64_t n, uint32_t nch, uint32_t nplanes, uint64_t origin, uint64_t B, shmt::Row* table) {
    const uint64_t nb = nblocks(origin, n, B), first = origin / B;
    const uint64_t slots = nb ? (uint64_t)1 << slot_shift(longest(origin, n, B) * nch) : 0;
    for (uint64_t j = 0; j < nb; ++j) {
        uint64_t a, b;
        range(first, j, origin, n, B, a, b);
        for (uint32_t r = 0; r < nplanes; ++r) {
            shmt::Row sum = shmt::zero();
            for (uint64_t p = 0; p < slots; ++p) {
                uint64_t s0, s1;
                part((b - a) * nch, p, s0, s1);
                shmt::Row one = shmt::zero();
                for (uint64_t s = s0; s < s1; ++s) take<WIDE>(one, s, nch, get(r, (a - origin) * nch + s));
                shmt::fold(sum, one);
            }
            table[row_at(j, nplanes, r)] = sum;
        }
    }
}

}  // namespace shpb
