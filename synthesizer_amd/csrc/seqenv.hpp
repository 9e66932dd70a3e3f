// seqenv.hpp -- the ADSR envelope of an event of sh_mix_events_env (sequence.hip), as Sample.envelope leaves it: the samples an event
// takes of its (resampled, cut) source are covered by up to MAX_SEGMENTS consecutive segments -- the faded attack, its unfaded tail,
// the unfaded head of the decay, the faded decay, the sustain, the unfaded head of the release, the faded release (the host replays
// upstream's float arithmetic for their boundaries, drops the empty ones and joins neighbours that do the same) -- and a sample's gain
// is its segment's: audioop.mul by the sustain level first (fbound: clamp, then floor), then the fade, int(x * f) (a Python float
// product, truncated toward zero) with f = 1.0 - k * slope / numsamples (fade-out) or k * slope / numsamples + offset (fade-in), k
// counting SAMPLES from the segment's origin.  The expression order is k_fade's (pcm_ops.hip); build with -ffp-contract=off.
// Plain C++17, SH_HD (tests/cpu_seqenv.cpp builds it with g++).
#pragma once
#include <cmath>
#include <cstdint>

#ifndef SH_HD
#if defined(__HIPCC__)
#define SH_HD __host__ __device__ __forceinline__
#else
#define SH_HD static inline
#endif
#endif

namespace she {

constexpr uint32_t MAX_SEGMENTS = 7;
enum Kind : uint32_t { NONE = 0, FADE_IN = 1, FADE_OUT = 2 };

// One segment as the kernels read it: wave-uniform, 48 bytes (scalar loads).  Positions count the event's source samples from its first.
struct Seg {
    double   mul;             // audioop.mul's, before the fade; exactly 1.0: none
    double   slope;           // fade-in: 1 - start volume; fade-out: 1 - target volume
    double   numsamples;      // samples of the whole faded stretch (> 0 where kind != NONE), also where the event is cut inside it
    double   offset;          // fade-in: the start volume
    uint32_t end;             // the segment is [the segment before's end, end)
    uint32_t origin;          // where k == 0
    uint32_t kind;
    uint32_t pad;
};
static_assert(sizeof(Seg) == 48, "Seg is read as a 32-byte and a 16-byte scalar load");

// audioop's fbound(): clamp, then round toward minus infinity (pcmdev.hpp has the device-only one)
SH_HD int fbound(double val, double minval, double maxval) {
    if (val > maxval) val = maxval;
    else if (val < minval + 1.0) val = minval;
    return (int)floor(val);
}

// sample x at position pos of a segment; [lo, hi] is the sample range of the width.  Zero stays zero (g's numbers are finite).
SH_HD int gain(const Seg& g, long long pos, int x, double lo, double hi) {
    if (g.mul != 1.0) x = fbound((double)x * g.mul, lo, hi);
    if (g.kind != NONE) {
        const double ramp = (double)(pos - (long long)g.origin) * g.slope / g.numsamples;
        const double f = g.kind == FADE_OUT ? 1.0 - ramp : ramp + g.offset;
        x = (int)trunc((double)x * f);
    }
    return x;
}

// A lane's N consecutive source samples x[0 .. N) at positions p0 .. (zeros where a position lies outside the event), shaped.
// [tlo, thi) is what the lane's whole TILE takes of the event, so everything but x and p0 is wave-uniform: the walk over the segments is
// scalar, a tile inside ONE segment (nearly all of them: the sustain, or the inside of a ramp) applies that segment's gain to all N
// without looking at positions, a plain segment costs nothing, and only a tile that straddles a boundary selects sample by sample.
// Past the last segment's end nothing is shaped.
template <int N>
SH_HD void shape_lane(const Seg* segs, uint32_t nseg, uint32_t tlo, uint32_t thi, long long p0, int (&x)[N], double lo, double hi) {
    uint32_t prev = 0;
    for (uint32_t s = 0; s < nseg && prev < thi; ++s) {
        const uint32_t end = segs[s].end;
        if (end > tlo) {
            const Seg g = segs[s];
            if (g.kind != NONE || g.mul != 1.0) {
                if (prev <= tlo && thi <= end) {
#if defined(__HIPCC__)
#pragma unroll
#endif
                    for (int k = 0; k < N; ++k) x[k] = gain(g, p0 + k, x[k], lo, hi);
                } else {
#if defined(__HIPCC__)
#pragma unroll
#endif
                    for (int k = 0; k < N; ++k)
                        if (p0 + k >= (long long)prev && p0 + k < (long long)end) x[k] = gain(g, p0 + k, x[k], lo, hi);
                }
            }
        }
        prev = end;
    }
}

}  // namespace she
