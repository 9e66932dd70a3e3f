// pcmextent.hpp -- the waveform EXTREMES per block of PCM that already lies in device memory (sh_pcm_extent_blocks, pcm_ops.hip): per
// block and channel the smallest and the largest sample, lo and hi, as signed values of the width (audioop.minmax of that channel's
// samples; width 1 signed, width 3 the sign-extended 24-bit value), for one plane or many -- what a waveform overview draws per pixel
// column, and what a peak row cannot say: a DC offset, a half-wave, which way a transient points.
// The geometry is pcmblocks.hpp's and is stated there alone: the blocks of a frame grid cut to a window (nblocks, range, longest), the
// parts of a block and the part slots of a call (parts_of, part, slot_shift), the block-major table (row_at).  This header adds the
// second reduction over it: a row, its identity, take and fold.
// The identity of the fold is lo = INT32_MAX, hi = INT32_MIN -- what audioop.minmax returns for an empty fragment.  An empty part slot
// yields it, and folding it changes nothing; every block of a call counts at least one frame, so no identity reaches the table.  A mono
// input fills channel 0; where a row of the TABLE is written (stored), its channel 1 reads lo = hi = 0, the rule of the level rows.
// take and fold are min and max and nothing else, so any split and any order give the same table.
// Plain C++17 integers, no intrinsics, SH_HD (tests/cpu_pcmextent.cpp builds it with g++).
#pragma once
#include <cstddef>
#include <cstdint>

#include "pcmblocks.hpp"

namespace shpe {

struct Row {                    // sh_pcm_extent's layout (synthhip.h), 16 bytes
    int32_t lo[2];
    int32_t hi[2];
};
static_assert(sizeof(Row) == 16, "a row is sh_pcm_extent");

SH_HD Row identity() { return Row{{INT32_MAX, INT32_MAX}, {INT32_MIN, INT32_MIN}}; }

// one sample of a plane into its row: sample s of the plane (counted from the plane's first) belongs to channel s & 1 of a stereo
// input and to channel 0 of a mono one (shpb::take's rule)
SH_HD void take(Row& row, uint64_t s, uint32_t nch, int32_t x) {
    const int c = nch == 2 && (s & 1) ? 1 : 0;
    row.lo[c] = x < row.lo[c] ? x : row.lo[c];
    row.hi[c] = x > row.hi[c] ? x : row.hi[c];
}

SH_HD void fold(Row& a, const Row& b) {
    for (int c = 0; c < 2; ++c) {
        a.lo[c] = b.lo[c] < a.lo[c] ? b.lo[c] : a.lo[c];
        a.hi[c] = b.hi[c] > a.hi[c] ? b.hi[c] : a.hi[c];
    }
}

// a folded row as the table holds it: the mono rule for channel 1
SH_HD Row stored(Row row, uint32_t nch) {
    if (nch != 2) row.lo[1] = row.hi[1] = 0;
    return row;
}

// The whole call on the host, as the two kernels divide it (the twin of shpb::host_rows): per block and plane, the part slots of the
// call one by one, each into a partial row from the identity, the partial rows folded, the mono rule where the row is stored.
// get(r, s): sample s of plane r.  table: nblocks * nplanes rows.
template <typename Get>
static inline void host_rows(Get&& get, uint64_t n, uint32_t nch, uint32_t nplanes, uint64_t origin, uint64_t B, Row* table) {
    const uint64_t nb = shpb::nblocks(origin, n, B), first = origin / B;
    const uint64_t slots = nb ? (uint64_t)1 << shpb::slot_shift(shpb::longest(origin, n, B) * nch) : 0;
    for (uint64_t j = 0; j < nb; ++j) {
        uint64_t a, b;
        shpb::range(first, j, origin, n, B, a, b);
        for (uint32_t r = 0; r < nplanes; ++r) {
            Row all = identity();
            for (uint64_t p = 0; p < slots; ++p) {
                uint64_t s0, s1;
                shpb::part((b - a) * nch, p, s0, s1);
                Row one = identity();
                for (uint64_t s = s0; s < s1; ++s) take(one, s, nch, (int32_t)get(r, (a - origin) * nch + s));
                fold(all, one);
            }
            table[shpb::row_at(j, nplanes, r)] = stored(all, nch);
        }
    }
}

}  // namespace shpe
