// csrc/seqplan.hpp's two planners built for the host behind a few C functions (tests/test_seqtiles.py drives them through ctypes):
// plan_by_tile, the per-tile index in song order of a kept song, and plan, the heaviest-first one it is compared with.
#include "../synthesizer_amd/csrc/seqplan.hpp"

namespace {
struct Both {
    shq::TilePlan by_tile;
    shq::Plan plan;
};
}  // namespace

extern "C" {

uint32_t st_tile(int width) { return shq::tile_samples(width); }
uint64_t st_max_track(void) { return shq::MAX_TRACK_SAMPLES; }
uint64_t st_max_pairs(void) { return shq::MAX_PAIRS; }

// dst[e], n[e]: the events.  Both planners over the same list; the refusals of each.
void* st_plan(const uint64_t* dst, const uint64_t* n, uint32_t nev, uint64_t track_samples, uint32_t tile, uint64_t max_pairs, int* refused,
              uint32_t* bad_event, int* plan_refused) {
    std::vector<shq::Event> ev(nev);
    for (uint32_t e = 0; e < nev; ++e) ev[e] = shq::Event{dst[e], n[e]};
    Both* B = new Both{shq::plan_by_tile(ev.data(), nev, track_samples, tile, max_pairs), shq::plan(ev.data(), nev, track_samples, tile, max_pairs)};
    *refused = (int)B->by_tile.refused;
    *bad_event = B->by_tile.bad_event;
    *plan_refused = (int)B->plan.refused;
    return B;
}
void st_free(void* p) { delete (Both*)p; }
uint32_t st_ntiles(const void* p) { return ((const Both*)p)->by_tile.ntiles; }
uint32_t st_active(const void* p) { return ((const Both*)p)->by_tile.active; }
uint64_t st_npairs(const void* p) { return ((const Both*)p)->by_tile.idx.size(); }
uint64_t st_nfirst(const void* p) { return ((const Both*)p)->by_tile.first.size(); }
const uint32_t* st_first(const void* p) { return ((const Both*)p)->by_tile.first.data(); }
const uint32_t* st_idx(const void* p) { return ((const Both*)p)->by_tile.idx.data(); }
uint32_t st_plan_ntiles(const void* p) { return (uint32_t)((const Both*)p)->plan.tiles.size(); }
uint64_t st_plan_npairs(const void* p) { return ((const Both*)p)->plan.idx.size(); }
const uint32_t* st_plan_tiles(const void* p) { return ((const Both*)p)->plan.tiles.data(); }
const uint32_t* st_plan_first(const void* p) { return ((const Both*)p)->plan.first.data(); }
const uint32_t* st_plan_idx(const void* p) { return ((const Both*)p)->plan.idx.data(); }

}  // extern "C"
