// csrc/seqplan.hpp built for the host behind a few C functions (tests/test_seqplan.py drives them through ctypes).  With SEQPLAN_MAIN it is a
// program of its own (its own main: the far-out lists of cpu_seqfar.hpp, planned past 2^31 samples and up to the last tile of a track),
// which a sanitizer build (-fsanitize=address,undefined) can run as it stands.
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

#ifdef SEQPLAN_MAIN
#include "cpu_seqfar.hpp"
#include <cstdio>
// shq::plan of every near list moved to every base: the near plan with its tile numbers raised where the base is a multiple of the tile,
// and the brute-force overlap count at the far coordinates either way
int main() {
    unsigned plans = 0, crossed = 0;
    for (uint32_t tile : {shq::TILE_I16, shq::TILE_W}) {
        for (const far::List& l : far::near_lists(tile)) {
            const shq::Plan N = shq::plan(l.ev.data(), (uint32_t)l.ev.size(), l.track, tile);
            if (N.refused || N.tiles.empty()) { printf("tile %u: the near list is refused or silent\n", tile); return 1; }
            for (const far::Base& b : far::bases(tile, l)) {
                const far::List f = far::shifted(l, b.B);
                if (f.track > far::MAX) { printf("tile %u base %s: beyond the greatest track\n", tile, b.name); return 1; }
                const shq::Plan P = shq::plan(f.ev.data(), (uint32_t)f.ev.size(), f.track, tile);
                if (P.refused) { printf("tile %u base %s: refused\n", tile, b.name); return 1; }
                if (b.aligned) {
                    bool same = P.tiles.size() == N.tiles.size() && P.first == N.first && P.idx == N.idx;
                    for (size_t k = 0; same && k < N.tiles.size(); ++k) same = P.tiles[k] == N.tiles[k] + (uint32_t)(b.B / tile);
                    if (!same) { printf("tile %u base %s: not the near plan raised by B / tile\n", tile, b.name); return 1; }
                }
                const auto want = far::brute(f, tile);
                if (P.tiles.size() != want.size() || P.first.size() != P.tiles.size() + 1 || P.first.back() != P.idx.size()) { printf("tile %u base %s: the active tiles\n", tile, b.name); return 1; }
                for (size_t k = 0; k < P.tiles.size(); ++k) {
                    const auto it = want.find(P.tiles[k]);
                    if (it == want.end() || std::vector<uint32_t>(P.idx.begin() + P.first[k], P.idx.begin() + P.first[k + 1]) != it->second) { printf("tile %u base %s: tile %u\n", tile, b.name, P.tiles[k]); return 1; }
                    if (k && P.first[k + 1] - P.first[k] > P.first[k] - P.first[k - 1]) { printf("tile %u base %s: not heaviest first\n", tile, b.name); return 1; }
                }
                for (const shq::Event& e : f.ev) crossed += e.dst < (1ull << 31) && e.dst + e.n > (1ull << 31);
                std::vector<shq::Event> over = f.ev;           // one sample more than the track holds is still refused up there
                over.push_back(shq::Event{f.track, 1});
                const shq::Plan R = shq::plan(over.data(), (uint32_t)over.size(), f.track, tile);
                if (R.refused != shq::EVENT_BEYOND_TRACK || R.bad_event != f.ev.size()) { printf("tile %u base %s: an event beyond the track is taken\n", tile, b.name); return 1; }
                ++plans;
            }
        }
    }
    if (!crossed) { printf("no event crosses sample 2^31\n"); return 1; }
    printf("seqplan: %u far plans, %u events across 2^31: ok\n", plans, crossed);
    return 0;
}
#endif
