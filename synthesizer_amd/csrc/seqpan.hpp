// seqpan.hpp -- pan automation of a kept STEREO song of tracks (sh_seq_auto_create_pans; sequence.hip): a track's sub-mix, behind its gain
// and its fader moves, and a group's bus, behind its gain and its fader ride, pass a PAN LANE where they passed their static pan -- a table
// of consecutive segments (she::Seg, seqenv.hpp) in SONG samples, as a fader lane is (seqauto.hpp), with a kind of its own: a pan move over
// frames [a, b) from p0 to p1 is {kind PAN, origin 2 a, end 2 b, numsamples b - a (FRAMES), offset p0, slope p1 - p0, mul 1.0}, and frame
// f of it, k = f - a, becomes
//     p = k * slope / numsamples + offset;   (L, R) = (int(L * (1.0 - p) / 2.0), int(R * (1.0 + p) / 2.0))
// -- Sample.pan(lfo=...)'s expression (k_pan_lfo, pcm_ops.hip): Python floats in this order, truncated toward zero.  Plain segments fill the
// gaps; in a gap, and past the lane's last segment, the STATIC factors apply as they always did: fbound(L * left), fbound(R * right),
// a factor of exactly 1.0 none.  The move REPLACES the static pan, it does not stand on top of it.  Here, stated once: every rule a pan
// table is held to (check), where the pan lanes stand in the automation's table (track_lane, group_lane), the pan of a frame and what it
// does to the frame (pan_of, ride), and "shape this lane's N samples through pan lane L, else the static factors" (shape_from), with the
// three wave-uniform paths a tile takes.  Lanes start on even song samples and segments on even ones too, so sample j of a lane is a left
// one where j is even and a frame never straddles a boundary.  Build with -ffp-contract=off.
// Plain C++17, SH_HD (tests/cpu_seqpan.cpp builds it with g++).
#pragma once
#include "seqauto.hpp"

namespace shp {

constexpr uint32_t PAN = 3;                                  // sh_env_segment.kind of a pan move (she::Kind ends at 2)

// ---- where the pan lanes stand: a handle with pan lanes keeps, behind the row0 + MAX_GROUP_LANES + 1 offsets of its fader lanes (tracks,
// master, all MAX_GROUP_LANES groups: seqauto.hpp), the offsets of ntracks + MAX_GROUP_LANES pan lanes -- the tracks', then the groups' --
// and one more for the end.  A kernel knows row0 = ntracks + 1 (shg::Table), nothing else.
SH_HD uint32_t lane0(uint32_t row0) { return row0 + sha::MAX_GROUP_LANES + 1u; }
SH_HD uint32_t track_lane(uint32_t row0, uint32_t t) { return lane0(row0) + t; }
SH_HD uint32_t group_lane(uint32_t row0, uint32_t g) { return lane0(row0) + (row0 - 1u) + g; }
SH_HD uint32_t lanes(uint32_t ntracks, uint32_t ngroups) { return ntracks + ngroups; }

enum Refusal { OK = 0, FIRST_ENDS, FIRST_DECREASES, RESERVED, ENDS, ODD, KIND, MUL, ORIGIN, NUMSAMPLES, RANGE };
struct Verdict {
    Refusal  why;
    uint32_t lane;                                           // the first lane at fault (FIRST_ENDS: 0; FIRST_DECREASES: the lane whose offset lies below the one before)
    uint32_t segment;                                        // its segment, counted from the lane's first
};

// Every refusal of a pan table of nlanes lanes, lane by lane and segment by segment, in this order per segment: a reserved word that is not
// 0, an end that does not lie past the one before or lies past the song, an end that is odd (a segment holds whole frames), a kind other
// than NONE and PAN, a mul other than 1.0; and of a move: an origin that is not its first sample, numsamples smaller than its FRAMES, a
// pan (offset, offset + slope) that is not finite or outside -1 .. 1.  S: sh_env_segment, or whatever has its fields.
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
            if (g.end & 1u) return Verdict{ODD, t, k};
            if (g.kind != she::NONE && g.kind != PAN) return Verdict{KIND, t, k};
            if (g.mul != 1.0) return Verdict{MUL, t, k};
            if (g.kind == PAN) {
                if (g.origin != prev) return Verdict{ORIGIN, t, k};
                if (!(g.numsamples >= (double)((g.end - g.origin) >> 1))) return Verdict{NUMSAMPLES, t, k};
                if (!std::isfinite(g.numsamples) || !(g.offset >= -1.0 && g.offset <= 1.0) || !(g.slope >= -1.0 - g.offset && g.slope <= 1.0 - g.offset))
                    return Verdict{RANGE, t, k};
            }
            prev = g.end;
        }
    }
    return Verdict{OK, 0, 0};
}

// the pan of the frame that holds song sample s of move g: k counts FRAMES from the move's first, formed in 64 bits
SH_HD double pan_of(const she::Seg& g, long long s) {
    return (double)((s - (long long)g.origin) >> 1) * g.slope / g.numsamples + g.offset;
}

// The frame (l, r) at pan p, truncated toward zero.  No clamp, as the oracle has none, and none is needed: for a CHECKED move |result| <=
// |sample|.  0 <= k < frames <= numsamples and frames < 2^31, so k / numsamples <= 1 - 2^-31, which two roundings of 2^-53 each do not
// lift to 1: t = fl(fl(k * slope) / numsamples) has slope's sign and |t| <= |slope|.  The check holds slope to fl(-1 - p0) .. fl(1 - p0)
// with p0 in -1 .. 1 (the host's fl(p1 - p0) lies inside by monotonicity), each within 2^-53 of the real bound, so t + p0 lies inside
// [-1 - 2^-53, 1 + 2^-53] and p, rounded once more, inside [-1 - 2^-52, 1 + 2^-52]: |p| <= 1 up to one rounding.  Then -2^-52 <= 1 -+ p
// <= 2 + 2^-51, and for |x| <= 2^31 the product |x * (1 -+ p) / 2| <= |x| * (1 + 2^-52) * (1 + 2^-53) < |x| + 2^-20, whose truncation
// toward zero is at most |x|; at the other end |x * 2^-52 / 2| < 1 truncates to 0.
SH_HD void ride(const double p, int& l, int& r) {
    l = (int)trunc((double)l * (1.0 - p) / 2.0);
    r = (int)trunc((double)r * (1.0 + p) / 2.0);
}

// the static pan step of a lane's N samples: Sample.stereo's, audioop.mul per side; a factor of exactly 1.0 takes no multiply
template <int N>
SH_HD void statics(int (&x)[N], const double left, const double right, const double lo, const double hi) {
    if (left != 1.0) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int k = 0; k < N; k += 2) x[k] = she::fbound((double)x[k] * left, lo, hi);
    }
    if (right != 1.0) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int k = 1; k < N; k += 2) x[k] = she::fbound((double)x[k] * right, lo, hi);
    }
}

// No move reaches into the tile that ends at thi: i == sha::find(segs, n, tlo) names no segment, or a plain one that covers the tile.
// Then the static factors apply to every sample, by whatever code the caller has for them.
SH_HD bool plain(const she::Seg* segs, uint32_t n, uint32_t i, uint32_t thi) {
    if (i >= n) return true;
    return segs[i].kind != PAN && segs[i].end >= thi;
}

// A lane's N consecutive samples x[0 .. N) at song positions p0 .. (p0 even), all of them inside the tile [tlo, thi), through the pan lane
// segs[0 .. n) from i == sha::find(segs, n, tlo) on; left, right: the static factors.  Segment i starts at or before tlo and no position
// lies in front of tlo.  Everything but x and p0 is wave-uniform, and one of three uniform paths is taken: no move in reach -- the static
// factors; the tile inside ONE move -- the ride on every frame, without looking at segment bounds; a tile that straddles a boundary --
// frame by frame the move that holds it, else the static factors.
template <int N>
SH_HD void shape_from(const she::Seg* segs, uint32_t n, uint32_t i, uint32_t tlo, uint32_t thi, long long p0, int (&x)[N], double left, double right,
                      double lo, double hi) {
    static_assert(N % 2 == 0, "a lane holds whole frames");
    if (plain(segs, n, i, thi)) {
        statics<N>(x, left, right, lo, hi);
        return;
    }
    if (segs[i].kind == PAN && segs[i].end >= thi) {
        const she::Seg g = segs[i];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int k = 0; k < N; k += 2) ride(pan_of(g, p0 + k), x[k], x[k + 1]);
        return;
    }
    int y[N];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < N; ++k) y[k] = x[k];
    statics<N>(y, left, right, lo, hi);
    uint32_t prev = tlo;
    for (uint32_t s = i; s < n && prev < thi; ++s) {
        const uint32_t end = segs[s].end;
        if (segs[s].kind == PAN) {
            const she::Seg g = segs[s];
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int k = 0; k < N; k += 2) {
                if (p0 + k >= (long long)prev && p0 + k < (long long)end) {
                    y[k] = x[k];
                    y[k + 1] = x[k + 1];
                    ride(pan_of(g, p0 + k), y[k], y[k + 1]);
                }
            }
        }
        prev = end;
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < N; ++k) x[k] = y[k];
}

}  // namespace shp
