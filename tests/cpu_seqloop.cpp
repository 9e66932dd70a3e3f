// Host build of synthesizer_amd/csrc/seqloop.hpp for tests/test_seqloop.py (g++, no GPU): the source frame of a run of virtual frames,
// from scratch (shl::map) and stepped the way the kernels of sequence.hip step it -- one frame on per frame for a plain event, a ratecv
// step of `inc` frames (inc % L divided once, as the host does for the record) with a carry of one more frame now and then for a
// resampled one.
#include "../synthesizer_amd/csrc/seqloop.hpp"

extern "C" {

// out[i] = the source frame of virtual frame v0 + i, each from scratch
void sl_map(uint32_t v0, uint32_t count, uint32_t E, uint32_t L, uint32_t* out) {
    for (uint32_t i = 0; i < count; ++i) out[i] = shl::map(v0 + i, E, L);
}

// The cursor from scratch at v0, then `count` steps: step i goes inc frames on, and one more when carry[i] != 0 (inc == 1 and no carry:
// shl::step1 alone, the plain event).  vout[i], fout[i]: the virtual frame and the source frame BEFORE step i.
void sl_walk(uint32_t v0, uint32_t count, uint32_t E, uint32_t L, uint32_t inc, const unsigned char* carry, uint32_t* vout, uint32_t* fout) {
    shl::Cur c = shl::at(v0, E, L);
    const uint32_t inc_mod = inc % L;
    for (uint32_t i = 0; i < count; ++i) {
        vout[i] = c.v;
        fout[i] = shl::frame(c, E);
        if (inc == 1 && !carry[i]) shl::step1(c, E, L);
        else {
            shl::step(c, inc, inc_mod, E, L);
            if (carry[i]) shl::step1(c, E, L);
        }
    }
}

}
