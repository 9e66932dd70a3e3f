// seqauto.hpp -- fader automation of a track of a kept song (sh_seq_auto_create, sh_seq_render_auto; sequence.hip): a track's sub-mix,
// behind its gain and in front of its pan, is covered by a table of consecutive segments (she::Seg, seqenv.hpp) in SONG samples -- a
// fader move is a FADE_IN segment, x -> int(x * (k * slope / numsamples + offset)) with k counting samples from the move's first, and
// plain segments fill the gaps; past the last segment's end nothing is shaped.  A song is long and a move list may be too (a ride per
// bar), so a tile does not walk its track's table from the start as she::shape_lane walks an event's seven segments: find() is a binary
// search over the segments' ends for the first one that ends past the tile's first sample -- wave-uniform, scalar loads, log2(n) steps --
// and shape_from() shapes a lane's samples from that segment on with she::shape_lane's two paths and she::gain's arithmetic, which stay
// stated once.  Positions are song samples, never window-relative; she::gain forms k in 64 bits.  Build with -ffp-contract=off.
// The same table carries the lanes of the BUSES (sh_seq_auto_create_buses): the master's and the groups' behind the tracks', numbered
// below; and check() is every rule a table is held to, for both create functions.
// Plain C++17, SH_HD (tests/cpu_seqauto.cpp and tests/cpu_seqbus.cpp build it with g++).
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

// ---- the lanes of the BUSES (sh_seq_auto_create_buses): the table's lanes stand in the meter table's row order -- tracks 0 .. ntracks - 1,
// the master at ntracks, group g at ntracks + 1 + g.  A kernel knows row0 = ntracks + 1, the meter row of group 0 (shg::Table).
constexpr uint32_t MAX_GROUP_LANES = 8;                      // shg::MAX_GROUPS (sequence.hip asserts it)
SH_HD uint32_t master_lane(uint32_t row0) { return row0 - 1u; }
SH_HD uint32_t group_lane(uint32_t row0, uint32_t g) { return row0 + g; }
SH_HD uint32_t lanes(uint32_t ntracks, uint32_t ngroups) { return ntracks + 1u + ngroups; }

enum Refusal { OK = 0, FIRST_ENDS, FIRST_DECREASES, RESERVED, ENDS, KIND, MUL, ORIGIN, NUMSAMPLES, VOLUME };
struct Verdict {
    Refusal  why;
    uint32_t lane;                                           // the first lane at fault (FIRST_ENDS: 0; FIRST_DECREASES: the lane whose offset lies below the one before)
    uint32_t segment;                                        // its segment, counted from the lane's first
};

// Every refusal of an automation table of nlanes lanes, lane by lane and segment by segment, in this order per segment: a reserved word
// that is not 0, an end that does not lie past the one before or lies past the song, a kind other than NONE and FADE_IN, a mul other than
// 1.0 (a lane's static gain is the render's); and of a move: an origin that is not its first sample, numsamples shorter than the move, a
// volume that is not finite or outside 0 .. 1 -- k runs over [0, end - origin) and numsamples covers it, so the factor stays between
// the two volumes and the kernels need no clamp.  S: sh_env_segment, or whatever has its fields.
template <typename S>
inline Verdict check(const S* segments, uint32_t nsegments, const uint32_t* seg_first, uint32_t nlanes, uint64_t track_samples) {
    if (seg_first[0] != 0 || seg_first[nlanes] != nsegments) return Verdict{FIRST_ENDS, 0, 0};
    for (uint32_t t = 0; t < nlanes; ++t)
        if (seg_first[t] > seg_first[t + 1]) return Verdict{FIRST_DECREASES, t + 1, 0};
    for (uint32_t t = 0; t < nlanes; ++t) {
        uint64_t prev = 0;
        for (uint32_t s = seg_first[t]; s < seg_first[t + 1]; ++s) {
            const S& g = segments[s];
            const uint32_t k = s - seg_first[t];
            if (g.reserved != 0) return Verdict{RESERVED, t, k};
            if (g.end <= prev || g.end > track_samples) return Verdict{ENDS, t, k};
            if (g.kind > she::FADE_IN) return Verdict{KIND, t, k};
            if (g.mul != 1.0) return Verdict{MUL, t, k};
            if (g.kind == she::FADE_IN) {
                if (g.origin != prev) return Verdict{ORIGIN, t, k};
                if (!(g.numsamples >= (double)(g.end - g.origin))) return Verdict{NUMSAMPLES, t, k};
                if (!std::isfinite(g.numsamples) || !(g.offset >= 0.0 && g.offset <= 1.0) || !(g.slope >= -g.offset && g.slope <= 1.0 - g.offset))
                    return Verdict{VOLUME, t, k};
            }
            prev = g.end;
        }
    }
    return Verdict{OK, 0, 0};
}

}  // namespace sha
