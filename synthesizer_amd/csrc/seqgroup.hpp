// seqgroup.hpp -- group buses of a kept song of tracks (sh_seq_render_groups; sequence.hip): a render names at most MAX_GROUPS runs of
// consecutive tracks [first, end), ascending and not overlapping; the tracks of a group are mixed, saturating, into a bus of their own,
// the bus takes ONE gain (audioop.mul over the saturated sum) and one pan, and enters the master where the group's last track stands.
// Here: the checks of a group list (check) and its packing (pack) into the table the kernels take BY VALUE in their arguments -- a byte
// per track naming its group (NONE: the track goes straight to the master), four to a 32-bit word so that a wave-uniform track number
// reads it by one scalar load and a shift (group_of), the groups' gains, their pan factors, their count and their first meter row.
// Plain C++17, SH_HD (tests/cpu_seqgroup.cpp builds it with g++).
#pragma once
#include <cmath>
#include <cstdint>

#ifndef SH_HD
#ifdef __HIPCC__
#define SH_HD __host__ __device__ __forceinline__
#else
#define SH_HD static inline
#endif
#endif

namespace shg {

constexpr uint32_t MAX_GROUPS = 8;
constexpr uint32_t MAX_TRACKS = 32;                          // shq::MAX_TRACKS (sequence.hip asserts it)
constexpr uint32_t NONE = 0xFFu;

struct Group {                                               // sh_seq_group (sequence.hip asserts it)
    uint32_t first, end;                                     // tracks [first, end)
    double   gain;                                           // audioop.mul's over the bus; exactly 1.0: none
    double   left, right;                                    // Sample.stereo's over the bus, behind the gain; exactly 1.0: none
};

struct Table {
    uint32_t of[MAX_TRACKS / 4];                             // byte t: the group of track t, or NONE
    double   gain[MAX_GROUPS];
    double   pan[2 * MAX_GROUPS];                            // left, right per group
    uint32_t n;                                              // groups
    uint32_t row0;                                           // the meter row of group 0: ntracks + 1
};
static_assert(sizeof(Group) == 32 && sizeof(Table) == 232, "the group table: 232 bytes of kernel arguments");

enum Refusal { OK = 0, COUNT, RANGE_EMPTY, RANGE_BEYOND, RANGE_ORDER, GAIN_NOT_FINITE, PAN_NOT_FINITE, PAN_NOT_STEREO };
struct Verdict {
    Refusal  why;
    uint32_t entry;                                          // the first entry at fault (COUNT: 0)
};

// the group of track t < MAX_TRACKS, or NONE
SH_HD uint32_t group_of(const Table& g, uint32_t t) { return (g.of[t >> 2] >> (8u * (t & 3u))) & 0xFFu; }

// Every refusal of a group list, entry by entry, in this order per entry: an empty range, one past the song's tracks, one that starts
// in front of the previous entry's end, a gain that is not finite, a factor that is not finite, factors other than (1.0, 1.0) on a
// song that is not stereo.
inline Verdict check(const Group* groups, uint32_t n, uint32_t ntracks, int nchannels) {
    if (n == 0 || n > MAX_GROUPS || !groups) return Verdict{COUNT, 0};
    uint32_t prev = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const Group& g = groups[i];
        if (g.first >= g.end) return Verdict{RANGE_EMPTY, i};
        if (g.end > ntracks || g.end > MAX_TRACKS) return Verdict{RANGE_BEYOND, i};
        if (g.first < prev) return Verdict{RANGE_ORDER, i};
        if (!std::isfinite(g.gain)) return Verdict{GAIN_NOT_FINITE, i};
        if (!std::isfinite(g.left) || !std::isfinite(g.right)) return Verdict{PAN_NOT_FINITE, i};
        if (nchannels != 2 && (g.left != 1.0 || g.right != 1.0)) return Verdict{PAN_NOT_STEREO, i};
        prev = g.end;
    }
    return Verdict{OK, 0};
}

// the table of a CHECKED list
inline void pack(const Group* groups, uint32_t n, uint32_t ntracks, Table& out) {
    for (uint32_t w = 0; w < MAX_TRACKS / 4; ++w) out.of[w] = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < MAX_GROUPS; ++i) {
        out.gain[i] = 1.0;
        out.pan[2 * i] = out.pan[2 * i + 1] = 1.0;
    }
    for (uint32_t i = 0; i < n; ++i) {
        for (uint32_t t = groups[i].first; t < groups[i].end; ++t) {
            const uint32_t sh = 8u * (t & 3u);
            out.of[t >> 2] = (out.of[t >> 2] & ~(0xFFu << sh)) | (i << sh);
        }
        out.gain[i] = groups[i].gain;
        out.pan[2 * i] = groups[i].left;
        out.pan[2 * i + 1] = groups[i].right;
    }
    out.n = n;
    out.row0 = ntracks + 1;
}

}  // namespace shg
