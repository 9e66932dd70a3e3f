// seqclip.hpp -- the OVERS of a song of tracks (sh_seq_render_clips, sequence.hip): beside the levels of seqmeter.hpp and per block as
// seqhist.hpp keeps them, how many samples a bus's OWN arithmetic clamped.  The contract, stated once:
//   For a row (a track, a group, the master), a channel and a set of song samples, `clipped` is the number of samples of that channel in
//   the set at which AT LEAST ONE of the row's own steps was clamped.  A step is clamped where the value it would have produced without
//   the clamp lies outside the width's range [LO, HI].  A sample counts ONCE per row, however many steps clamped at it.
//   Track t's steps: every saturating add of an event's samples into the track's sub-mix (mix_at's audioop.add), the track's
//   amplify(gain), its static pan factors.  Group g's: every saturating add of a track into the group's bus, the group's amplify(gain),
//   its pan factors.  The master's: every saturating add of a track or a group into the master, the master's amplify(master_gain).
//   An ADD clamps where the exact integer sum of the saturated accumulator and the addend is > HI or < LO.  A MULTIPLY by a factor
//   f != 1.0 clamps where floor(p) > HI or floor(p) < LO, p being the float64 product audioop.mul forms: a product in (HI, HI + 1) floors
//   to HI and is no over.  A row counts its own stage only: a track that clipped does not make its group or the master count.
//   NOT counted: what an event does to its own samples in front of the add (its volume, pan, channel factors, envelope -- the sample as
//   placed), and the tracks' fader moves (volumes are at most 1.0 and int() truncates toward zero: nothing leaves the range).
//   A muted or skipped track or group and an idle tile count 0; a mono song fills channel 0.
// A lane keeps one sticky flag per sample and bus; its partial count is the flags of its samples inside [lo, hi), the channel by j & 1 as
// shmt::lane has it.  Counts add, so partial counts fold in any order.
// Plain C++17, no intrinsics, SH_HD (tests/cpu_seqclip.cpp builds it with g++).
#pragma once
#include <cmath>
#include <cstdint>

#include "seqmeter.hpp"

namespace shcl {

template <int WIDTH> constexpr long long HI = WIDTH == 1 ? 127LL : (WIDTH == 2 ? 32767LL : (WIDTH == 3 ? 8388607LL : 2147483647LL));
template <int WIDTH> constexpr long long LO = -HI<WIDTH> - 1;

// a saturating add of x into acc (both inside [LO, HI]) clamps: the exact sum lies outside the range
template <int WIDTH>
SH_HD bool add_clamps(long long acc, long long x) {
    const long long t = acc + x;
    return t > HI<WIDTH> || t < LO<WIDTH>;
}

// The same at 16 bits as the kernels evaluate it on PACKED samples, without the exact sum: the add clamped exactly where the saturating
// and the WRAPPING 16-bit sums differ -- they differ for every out-of-range sum (the wrapped one lies 65536 away from the exact one, the
// saturated one on the rail) and for none in range (both are the exact sum).  The wrapping sum is formed unsigned.
SH_HD int16_t sat16(int16_t a, int16_t x) {
    const int t = (int)a + (int)x;
    return (int16_t)(t > 32767 ? 32767 : (t < -32768 ? -32768 : t));
}
SH_HD int16_t wrap16(int16_t a, int16_t x) { return (int16_t)(uint16_t)((uint16_t)a + (uint16_t)x); }
SH_HD bool add_clamps16(int16_t a, int16_t x) { return sat16(a, x) != wrap16(a, x); }

// audioop.mul's float64 product p clamps: its floor lies outside the range (p in (HI, HI + 1) floors to HI: no over)
template <int WIDTH>
SH_HD bool mul_clamps(double p) {
    const double f = floor(p);
    return f > (double)HI<WIDTH> || f < (double)LO<WIDTH>;
}

struct Row : shmt::Row {        // sh_seq_meter_clips' layout (synthhip.h), 48 bytes: the levels, then the overs per channel
    uint32_t clipped[2];
};
static_assert(sizeof(Row) == 48, "a row is sh_seq_meter_clips");

struct Count { uint32_t c[2]; };

// a lane's sticky flags: an array (or a vector) of N values, 0 or not -- or, Bits, the bits of a word
struct Bits { uint32_t m; };
template <typename F>
SH_HD bool flag(const F& flags, int j) { return flags[j] != 0; }
SH_HD bool flag(const Bits& flags, int j) { return (flags.m >> j) & 1u; }

// A lane's partial count: flag(flags, j) says sample j of its N, at song sample s0 + j (s0 even), was clamped; only samples inside
// [lo, hi) count, the channel of sample j is j & 1 in a stereo song and 0 otherwise (shmt::lane's cut and channel rule)
template <int N, typename F>
SH_HD Count lane(const F& flags, uint32_t s0, uint32_t lo, uint32_t hi, uint32_t nch) {
    Count r{{0u, 0u}};
    const bool stereo = nch == 2;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < N; ++j) {
        const uint64_t s = (uint64_t)s0 + (uint32_t)j;
        if (s < lo || s >= hi) continue;
        const uint32_t one = flag(flags, j) ? 1u : 0u;
        if ((j & 1) && stereo) r.c[1] += one;
        else r.c[0] += one;
    }
    return r;
}

// two partial counts into one
SH_HD void fold(Count& a, const Count& b) {
    a.c[0] += b.c[0];
    a.c[1] += b.c[1];
}

// two rows into one: shmt::fold of the levels, the counts add
SH_HD void fold(Row& a, const Row& b) {
    shmt::fold(a, b);
    a.clipped[0] += b.clipped[0];
    a.clipped[1] += b.clipped[1];
}

}  // namespace shcl
