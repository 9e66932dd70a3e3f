// seqloop.hpp -- the sustain loop of an event of sh_mix_events_loop (sequence.hip): a note longer than its recording.  The note is a
// run of VIRTUAL frames 0 .. V; virtual frame v is frame v of the source while v < E (the head: everything up to the loop's end), and
// frame S + (v - E) % L after it (L = E - S frames of loop, passed again and again) -- the bytes of
//     o = other.clip(0, loop_end); while o.duration < length: o.join(other.clip(loop_start, loop_end)); o.clip(0, length)
// without the copy.  Everything behind it in the chain (ratecv, the envelope, ...) sees virtual frames.
//
// A cursor is (v, f): a virtual frame and the loop frame f = S + (v - E) mod L in [S, E) that belongs to it -- the mathematical residue,
// so f is defined in the head as well, a stepping lane never has to know where the seam is, and S itself is needed nowhere: one 32-bit
// division where a lane starts (at), compare and subtract from there on (step1, step).
// Plain C++17, SH_HD (tests/cpu_seqloop.cpp builds it with g++).
#pragma once
#include <cstdint>

#ifndef SH_HD
#if defined(__HIPCC__)
#define SH_HD __host__ __device__ __forceinline__
#else
#define SH_HD static inline
#endif
#endif

namespace shl {

struct Cur { uint32_t v, f; };          // a virtual frame and its loop frame, E - L <= f < E

// from scratch: the cursor of virtual frame v (0 < L <= E)
SH_HD Cur at(uint32_t v, uint32_t E, uint32_t L) {
    if (v >= E) return Cur{v, E - L + (v - E) % L};
    const uint32_t back = (E - v) % L;                     // (v - E) mod L of a negative v - E is L - back, or 0
    return Cur{v, back ? E - back : E - L};
}

// the source frame of a cursor
SH_HD uint32_t frame(Cur c, uint32_t E) { return c.v < E ? c.v : c.f; }

// from scratch, in one: the source frame of virtual frame v
SH_HD uint32_t map(uint32_t v, uint32_t E, uint32_t L) { return frame(at(v, E, L), E); }

// one virtual frame on (a plain event; the carry of a resampled one)
SH_HD void step1(Cur& c, uint32_t E, uint32_t L) {
    ++c.v;
    ++c.f;
    if (c.f >= E) c.f -= L;
}

// `inc` virtual frames on, inc_mod = inc % L (uniform per event: the host divides once) -- a step may be longer than the loop
SH_HD void step(Cur& c, uint32_t inc, uint32_t inc_mod, uint32_t E, uint32_t L) {
    c.v += inc;
    c.f += inc_mod;
    if (c.f >= E) c.f -= L;
}

}  // namespace shl
