// seqbus.hpp -- which BUS a render of a compiled song gets (sequence.hip: SeqBusOf<F>, seq_render).  A bus is described once, as a set of
// FEATURES; the window kernels exist for the 22 sets in ROUTES and for no other, and route() is the one place that says which of them a
// call takes.  Three kinds of bits:
//   payload   METERS, DESK, AUTO, GROUPS, STEMS: the bus carries that part in its kernel arguments (SeqMeters, SeqDesk, SeqAuto,
//             SeqGroups, SeqStems of sequence.hip, in this order behind the plain bus), and the kernels do that part's work;
//   lanes     RIDES, PANS: no argument of their own -- the kernel READS bus lanes (RIDES) and pan lanes (PANS) of the automation's table,
//             so only a call whose automation handle holds those lanes may be routed there;
//   rows      HISTORY, CLIPS: no argument either -- what becomes of the meter rows (kept per tile; with a count of overs).
// The width rule (valid_at): automation has no 24-bit form, and a group bus carries the WHOLE desk so that the kernel count does not
// double -- at widths 1, 2 and 4 the automation's two pointers as well, NULL meaning no moves; at width 3 without them.
// Plain C++17 constant expressions, which hipcc takes for host and device alike (tests/cpu_seqroute.cpp builds them with g++).
#pragma once
#include <cstdint>

namespace shb {

enum : uint32_t { METERS = 1, DESK = 2, AUTO = 4, GROUPS = 8, RIDES = 16, PANS = 32, HISTORY = 64, CLIPS = 128, STEMS = 256 };
constexpr uint32_t PLAIN = 0;                                // a song of tracks, a gain per track: no feature
constexpr uint32_t NO_BUS = ~0u;                             // a flat song: the kernels without a bus
constexpr uint32_t PARTS = METERS | DESK | AUTO | GROUPS | STEMS;      // every payload part

constexpr uint32_t G = DESK | AUTO | GROUPS, G3 = DESK | GROUPS;       // the group bus at widths 1, 2, 4 and at width 3
constexpr uint32_t ROUTES[] = {
    PLAIN,                                                   // SeqBus
    METERS,                                                  // SeqBusM
    DESK,                                                    // SeqBusD
    METERS | DESK,                                           // SeqBusDM
    DESK | AUTO,                                             // SeqBusA
    METERS | DESK | AUTO,                                    // SeqBusAM
    G,                                                       // SeqBusG
    G3,                                                      // SeqBusG3
    G | RIDES,                                               // SeqBusR
    G | RIDES | PANS,                                        // SeqBusP
    G | STEMS,                                               // SeqBusGS
    G | RIDES | STEMS,                                       // SeqBusRS
    G | RIDES | PANS | STEMS,                                // SeqBusPS
    G3 | STEMS,                                              // SeqBusGS3
    METERS | G,                                              // SeqBusGM
    METERS | G3,                                             // SeqBusGM3
    METERS | G | RIDES,                                      // SeqBusRM
    METERS | G | RIDES | PANS,                               // SeqBusPM
    METERS | G | HISTORY,                                    // SeqBusGH
    METERS | G3 | HISTORY,                                   // SeqBusGH3
    METERS | G | HISTORY | CLIPS,                            // SeqBusGC
    METERS | G3 | HISTORY | CLIPS,                           // SeqBusGC3
};
constexpr uint32_t NROUTES = sizeof(ROUTES) / sizeof(ROUTES[0]);

constexpr bool known(uint32_t mask) {
    for (uint32_t i = 0; i < NROUTES; ++i)
        if (ROUTES[i] == mask) return true;
    return false;
}

// whether the kernels of `mask` exist at this width: automation serves widths 1, 2 and 4; a group bus without it width 3 alone; the four
// buses with neither every width
constexpr bool valid_at(uint32_t mask, int width) {
    if (!known(mask) || width < 1 || width > 4) return false;
    if (mask & AUTO) return width != 3;
    if (mask & GROUPS) return width == 3;
    return true;
}

// what seq_render is told: the handle (tracks or flat, its width), which tables the call gave, and what the entry point found in the
// automation's handle (rides: it holds bus lanes; pans: pan lanes as well) and asked of the rows
struct Call {
    bool tracks, meters, desk, automation, groups, rides, pans, history, clips, stems;
    int  width;
};

// The bus of a call.  Without a desk only the meters count; a desk without groups takes what it was given; with a desk AND groups the whole
// desk rides on a group bus whether or not automation was given (AUTO at widths 1, 2 and 4: NULL pointers mean no moves).  Stems come in
// front of the rows, overs in front of a history, either in front of plain meters; a history and overs have no riding kernels, and width 3
// has none at all.
constexpr uint32_t route(const Call& c) {
    if (!c.tracks) return NO_BUS;
    if (!c.desk) return c.meters ? METERS : PLAIN;
    if (!c.groups) return DESK | (c.automation ? AUTO : 0u) | (c.meters ? METERS : 0u);
    const uint32_t bus = c.width == 3 ? G3 : G;
    const uint32_t lanes = c.width == 3 ? 0u : c.pans ? RIDES | PANS : c.rides ? RIDES : 0u;
    if (c.stems) return bus | lanes | STEMS;
    if (c.clips) return bus | METERS | HISTORY | CLIPS;
    if (c.history) return bus | METERS | HISTORY;
    return bus | lanes | (c.meters ? METERS : 0u);
}

}  // namespace shb
