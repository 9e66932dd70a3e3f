// seqauto.hpp -- fader automation of a track of a kept song (sh_seq_auto_create, sh_seq_render_auto; sequence.hip): a track's sub-mix,
// behind its gain and in front of its pan, is covered by a table of consecutive segments (she::Seg, seqenv.hpp) in SONG samples -- a
// fader move is a FADE_IN segment, x -> int(x * (k * slope / numsamples + offset)) with k counting samples from the move's first, and
// plain segments fill the gaps; past the last segment's end nothing is shaped.  A song is long and a move list may be too (a ride per
// bar), so a tile does not walk its track's table from the start as she::shape_lane walks an event's seven segments: find() is a binary
// search over the segments' ends for the first one that ends past the tile's first sample -- wave-uniform, scalar loads, log2(n) steps --
// and shape_from() shapes a lane's samples from that segment on with she::shape_lane's two paths and she::gain's arithmetic, which stay
// stated once.  Positions are song samples, never window-relative; she::gain forms k in 64 bits.  Build with -ffp-contract=off.
// Plain C++17, SH_HD (tests/cpu_seqauto.cpp builds it with g++).
#pragma once
#include "seqenv.hpp"

namespace sha {

// the first of segs[0 .. n) whose end lies past sample s, n where there is none; the ends ascend
SH_HD uint32_t find(const she::Seg* segs, uint32_t n, uint32_t s) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (segs[mid].end > s) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// A lane's N consecutive samples x[0 .. N) at song positions p0 .., all of them inside the tile [tlo, thi), shaped by the segments from
// i == find(segs, n, tlo) on.  Segment i starts at or before tlo (the one before it ends there or earlier) and no position lies in front
// of tlo, so she::shape_lane, which takes its first segment to start at 0, sees from segs + i what a walk from segment 0 would see: a
// tile inside one segment applies that segment's gain without looking at positions, a plain segment costs nothing, and only a tile that
// straddles a boundary selects sample by sample.
template <int N>
SH_HD void shape_from(const she::Seg* segs, uint32_t n, uint32_t i, uint32_t tlo, uint32_t thi, long long p0, int (&x)[N], double lo, double hi) {
    if (i < n) she::shape_lane<N>(segs + i, n - i, tlo, thi, p0, x, lo, hi);
}

}  // namespace sha
