// Host build of synthesizer_amd/csrc/seqrev.hpp for tests/test_seqrev.py (g++, no GPU): where the kernels of sequence.hip find channel ch
// of virtual frame v of an event -- region, reverse, loop -> stored sample -- as an offset against the record's pointer, which stands
// shv::origin behind the region's first stored sample.
#include "../synthesizer_amd/csrc/seqrev.hpp"

extern "C" {

// out[v * nch + ch] = the stored sample, counted from the region's first, of channel ch of virtual frame v, each from scratch as a
// resampled lane starts (shl::map, then shv::offset on frame * nch + ch, as seq_rate and seq_at have it): a region of F frames, a loop
// of L frames that ends at played frame E (L == 0: none), V virtual frames.  A reversed looped event's region is the E frames it plays.
void sv_map(uint32_t reversed, uint32_t F, uint32_t E, uint32_t L, uint32_t V, uint32_t nch, int64_t* out) {
    const int64_t origin = (int64_t)shv::origin(reversed, (uint64_t)F * nch);
    for (uint32_t v = 0; v < V; ++v) {
        const uint32_t frame = L ? shl::map(v, E, L) : v;   // (an unlooped record: the kernels skip the map)
        for (uint32_t ch = 0; ch < nch; ++ch) out[(uint64_t)v * nch + ch] = origin + shv::offset(reversed, (uint64_t)frame * nch + ch);
    }
}

// the same stepped as a plain looped event steps it: the cursor once (shl::at), then shl::step1 per frame, the reversal applied last
void sv_walk(uint32_t reversed, uint32_t F, uint32_t E, uint32_t L, uint32_t V, uint32_t nch, int64_t* out) {
    const int64_t origin = (int64_t)shv::origin(reversed, (uint64_t)F * nch);
    shl::Cur c = shl::at(0, E, L);
    for (uint32_t v = 0; v < V; ++v) {
        for (uint32_t ch = 0; ch < nch; ++ch) out[(uint64_t)v * nch + ch] = origin + shv::offset(reversed, (uint64_t)shl::frame(c, E) * nch + ch);
        shl::step1(c, E, L);
    }
}

}
