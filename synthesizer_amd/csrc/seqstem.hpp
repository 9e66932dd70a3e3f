// seqstem.hpp -- the STEMS of a song of tracks (sh_seq_render_stems, sequence.hip): the samples of every bus of the desk, from the render's
// one launch.  A stems render of song samples [lo, hi) writes
//     nrows = ntracks + 1 + ngroups
// PLANES of hi - lo samples each, in the meter table's row order: track t in plane t, the master in plane ntracks, group g in plane
// ntracks + 1 + g.  Plane r holds exactly the samples over which the metered render of the same window with the same arguments reads
// row r (seqmeter.hpp):
//   track t   as its bus takes it: the track's events folded from silence, amplify(gain), its fader moves, its static pan or -- where a pan
//             piece holds the frame -- its pan ride.  All zeros where the track is skipped: gain 0.0, both static factors 0.0, or a group
//             that is silent.
//   group g   as the master takes it: the bus saturating at every one of its tracks, amplify(gain), its fader ride, its pan or pan ride.
//             All zeros for a group at gain 0.0 or pan (0.0, 0.0).
//   master    the bytes the render without stems stores for the same arguments.
// EVERY byte of every plane is written, whatever the buffer held -- idle tiles, tiles where a sounding track has no run, the planes of
// muted rows -- and NO byte outside the planes' windows: none in front, none behind, none in the gap between two planes where the stride
// is larger than the window.  Every sample of a plane has one writer, the lane that folds its song sample, so nothing zeroes the planes
// in front of the launch.
// Geometry.  Plane r of song sample s stands at
//     biased + r * stride + s * width                                         (bytes; 64-bit, wrapping)
// `biased` being the caller's buffer biased by (out_sample - first_sample) samples as the render's is, and `stride` ONE 64-bit count of
// BYTES, plane_samples * width: plane r is samples [out_sample + r * plane_samples, ... + nsamples) of the buffer.  A song of
// 2^32 - 65536 samples at width 4 in 41 planes spans 2^39.4 bytes, so none of this is formed in 32 bits.
// Here: the row order, the address, the refusals of a call's geometry (check), whether the 16-bit store's aligned fast path holds for
// EVERY plane (aligned), the span of all planes (span) and the stride that keeps the fast path for a window (plane_samples_for).
// Plain C++17 integers, no intrinsics, SH_HD (tests/cpu_seqstem.cpp builds it with g++).
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef SH_HD
#ifdef __HIPCC__
#define SH_HD __host__ __device__ __forceinline__
#else
#define SH_HD static inline
#endif
#endif

namespace shst {

constexpr uint32_t MAX_ROWS = 32 + 1 + 8;                    // shq::MAX_TRACKS + 1 + shg::MAX_GROUPS (sequence.hip asserts it): bits of one 64-bit mask
constexpr uint64_t VECTOR_BYTES = 16;                        // the 16-bit store's vector: eight samples

// the planes of a call, and where each bus stands among them
SH_HD uint32_t nrows(uint32_t ntracks, uint32_t ngroups) { return ntracks + 1u + ngroups; }
SH_HD uint32_t track_row(uint32_t t) { return t; }
SH_HD uint32_t master_row(uint32_t ntracks) { return ntracks; }
SH_HD uint32_t group_row(uint32_t ntracks, uint32_t g) { return ntracks + 1u + g; }

// the stride of a call, in bytes
SH_HD uint64_t stride_bytes(uint64_t plane_samples, uint32_t width) { return plane_samples * (uint64_t)width; }

// the byte offset of plane r against plane 0, and the address of song sample s of plane r: unsigned 64-bit arithmetic, which wraps as
// the biased base may have wrapped
SH_HD uint64_t plane_offset(uint32_t r, uint64_t stride) { return (uint64_t)r * stride; }
SH_HD uint64_t address(uint64_t biased, uint32_t r, uint64_t stride, uint64_t s, uint32_t width) {
    return biased + plane_offset(r, stride) + s * (uint64_t)width;
}

// the refusals of a call's geometry, in this order
enum Refusal { OK = 0, PLANES, STRIDE, EXTENT };

// nplanes planes of nsamples samples, plane_samples apart, from sample out_sample of a buffer of `have` samples, for a song of ntracks
// tracks rendered with ngroups groups: PLANES -- nplanes is not ntracks + 1 + ngroups; STRIDE -- the planes would overlap
// (plane_samples < nsamples); EXTENT -- the last plane ends past the buffer (or the first one starts past it).  No product is formed that
// can pass 2^64: the room behind out_sample is divided instead.
SH_HD Refusal check(uint32_t nplanes, uint32_t ntracks, uint32_t ngroups, uint64_t plane_samples, uint64_t nsamples, uint64_t out_sample, uint64_t have) {
    if (nplanes != nrows(ntracks, ngroups)) return PLANES;
    if (plane_samples < nsamples) return STRIDE;
    if (out_sample > have || nsamples > have - out_sample) return EXTENT;
    const uint64_t room = have - out_sample - nsamples;      // samples behind the FIRST plane's window
    if (nplanes > 1u && plane_samples > room / (uint64_t)(nplanes - 1u)) return EXTENT;
    return OK;
}

// the samples from the first sample of plane 0 to the last of the last plane: what the call may write into, gaps included (a CHECKED
// call: no overflow, the span lies inside the buffer)
SH_HD uint64_t span(uint32_t nplanes, uint64_t plane_samples, uint64_t nsamples) {
    return nplanes && nsamples ? (uint64_t)(nplanes - 1u) * plane_samples + nsamples : 0u;
}

// whether [a0, a1) and [b0, b1) (addresses) share a byte
SH_HD bool overlaps(uint64_t a0, uint64_t a1, uint64_t b0, uint64_t b1) { return a0 < b1 && b0 < a1; }

// The 16-bit store writes a lane's eight samples as one 16-byte vector where the lane's address is a multiple of 16.  Lanes start on
// multiples of eight SONG samples, so plane 0's are aligned where the biased base is, and plane r's where r * stride is a multiple of 16
// as well: for every r exactly where the stride is.  Any other stride takes the careful path, sample by sample, and is still right.
SH_HD bool aligned(uint64_t biased, uint64_t stride) { return biased % VECTOR_BYTES == 0 && stride % VECTOR_BYTES == 0; }

// the smallest plane_samples >= nsamples whose stride is a multiple of 16 bytes at this width: what a caller picks to keep the fast path
// in every plane (width 3: a multiple of 16 samples)
SH_HD uint64_t plane_samples_for(uint64_t nsamples, uint32_t width) {
    const uint64_t unit = width == 1u ? 16u : width == 2u ? 8u : width == 3u ? 16u : 4u;
    return (nsamples + unit - 1u) / unit * unit;
}

}  // namespace shst
