// seqrev.hpp -- where an event of sh_mix_events_rev (sequence.hip) finds its samples in memory: region, reverse, loop -> source sample.
// An event plays a REGION of its source, R = F * nch samples stored forwards.  A reversed event plays them in the order of
// audioop.reverse -- the order of the SAMPLES, so played sample i is stored sample R - 1 - i: played frame f is stored frame F - 1 - f
// with its channels in reverse order (left and right change places).  Its record's pointer stands one sample BEHIND the region, so
// played sample i is ptr[-1 - i], and the channel swap falls out of the index; a forward event's pointer stands on the region's first
// sample and played sample i is ptr[i].  The sustain loop (seqloop.hpp) counts PLAYED frames: virtual frame v -> played frame
// (shl::map from scratch, shl::at / step1 / step / frame stepped) -> played sample frame * nch + ch -> memory, the reversal applied last
// by shv::offset: every fetch of sequence.hip that may belong to a reversed event goes through it.
// Plain C++17, SH_HD (tests/cpu_seqrev.cpp builds it with g++ and composes it with seqloop.hpp's map the way the kernels do).
#pragma once
#include "seqloop.hpp"

namespace shv {

// played sample i against the record's pointer, in samples
SH_HD int64_t offset(uint32_t reversed, uint64_t i) { return reversed ? -1 - (int64_t)i : (int64_t)i; }

// where the record's pointer stands against the region's first stored sample, in samples
SH_HD uint64_t origin(uint32_t reversed, uint64_t region_samples) { return reversed ? region_samples : 0; }

}  // namespace shv
