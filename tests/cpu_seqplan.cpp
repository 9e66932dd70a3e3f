// csrc/seqplan.hpp built for the host behind a few C functions (tests/test_seqplan.py drives them through ctypes).
#include "../synthesizer_amd/csrc/seqplan.hpp"

extern "C" {

uint32_t sq_tile(int width) { return shq::tile_samples(width); }
uint64_t sq_max_track(void) { return shq::MAX_TRACK_SAMPLES; }
uint64_t sq_max_pairs(void) { return shq::MAX_PAIRS; }

// dst[e], n[e]: the events.  Returns the refusal (0: none; bad_event then holds nothing) and a plan to read with the calls below.
void* sq_plan(const uint64_t* dst, const uint64_t* n, uint32_t nev, uint64_t track_samples, uint32_t tile, uint64_t max_pairs, int* refused,
              uint32_t* bad_event) {
    std::vector<shq::Event> ev(nev);
    for (uint32_t e = 0; e < nev; ++e) ev[e] = shq::Event{dst[e], n[e]};
    shq::Plan* P = new shq::Plan(shq::plan(ev.data(), nev, track_samples, tile, max_pairs));
    *refused = (int)P->refused;
    *bad_event = P->bad_event;
    return P;
}
void sq_free(void* p) { delete (shq::Plan*)p; }
uint32_t sq_ntiles(const void* p) { return (uint32_t)((const shq::Plan*)p)->tiles.size(); }
uint64_t sq_npairs(const void* p) { return ((const shq::Plan*)p)->idx.size(); }
uint32_t sq_nfirst(const void* p) { return (uint32_t)((const shq::Plan*)p)->first.size(); }
const uint32_t* sq_tiles(const void* p) { return ((const shq::Plan*)p)->tiles.data(); }
const uint32_t* sq_first(const void* p) { return ((const shq::Plan*)p)->first.data(); }
const uint32_t* sq_idx(const void* p) { return ((const shq::Plan*)p)->idx.data(); }

}  // extern "C"
