// csrc/seqplan.hpp's two planners built for the host behind a few C functions (tests/test_seqtiles.py drives them through ctypes):
// plan_by_tile, the per-tile index in song order of a kept song, and plan, the heaviest-first one it is compared with.  With SEQTILES_MAIN it
// is a program of its own (its own main: the far-out lists of cpu_seqfar.hpp as songs of up to 2^22 - 64 tiles), which a sanitizer build
// (-fsanitize=address,undefined) can run as it stands.
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

#ifdef SEQTILES_MAIN
#include "cpu_seqfar.hpp"
#include <cstdio>
// shq::plan_by_tile of every near list moved to every base: nothing in front of the song, the near index behind it where the base is a
// multiple of the tile, and the brute-force overlap count at the far coordinates either way
int main() {
    unsigned songs = 0;
    uint32_t longest = 0;
    for (uint32_t tile : {shq::TILE_I16, shq::TILE_W}) {
        for (const far::List& l : far::near_lists(tile)) {
            const shq::TilePlan N = shq::plan_by_tile(l.ev.data(), (uint32_t)l.ev.size(), l.track, tile);
            if (N.refused) { printf("tile %u: the near list is refused\n", tile); return 1; }
            for (const far::Base& b : far::bases(tile, l)) {
                const far::List f = far::shifted(l, b.B);
                const shq::TilePlan P = shq::plan_by_tile(f.ev.data(), (uint32_t)f.ev.size(), f.track, tile);
                if (P.refused) { printf("tile %u base %s: refused\n", tile, b.name); return 1; }
                if (P.ntiles != (f.track + tile - 1) / tile || P.first.size() != (size_t)P.ntiles + 1 || P.first.back() != P.idx.size()) { printf("tile %u base %s: the tile count\n", tile, b.name); return 1; }
                if (b.aligned) {
                    const uint32_t k = (uint32_t)(b.B / tile);
                    bool same = P.ntiles == k + N.ntiles && P.active == N.active && P.idx == N.idx;
                    for (uint32_t t = 0; same && t < k; ++t) same = P.first[t] == 0;
                    for (uint32_t t = 0; same && t <= N.ntiles; ++t) same = P.first[k + t] == N.first[t];
                    if (!same) { printf("tile %u base %s: not the near index raised by B / tile\n", tile, b.name); return 1; }
                }
                const auto want = far::brute(f, tile);
                uint32_t active = 0;
                for (uint32_t t = 0; t < P.ntiles; ++t) {
                    if (P.first[t + 1] < P.first[t]) { printf("tile %u base %s: first decreases\n", tile, b.name); return 1; }
                    if (P.first[t + 1] == P.first[t]) continue;
                    ++active;
                    const auto it = want.find(t);
                    if (it == want.end() || std::vector<uint32_t>(P.idx.begin() + P.first[t], P.idx.begin() + P.first[t + 1]) != it->second) { printf("tile %u base %s: tile %u\n", tile, b.name, t); return 1; }
                }
                if (active != want.size() || P.active != active) { printf("tile %u base %s: %u active tiles\n", tile, b.name, active); return 1; }
                longest = std::max(longest, P.ntiles);
                ++songs;
            }
        }
    }
    if (longest != far::MAX / shq::TILE_W) { printf("no song of the greatest length\n"); return 1; }
    printf("seqtiles: %u far songs, the longest of %u tiles: ok\n", songs, longest);
    return 0;
}
#endif
