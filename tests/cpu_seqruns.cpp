// csrc/seqplan.hpp's plan_runs built for the host behind a few C functions (tests/test_seqruns.py drives them through ctypes): the per-tile
// runs of a song made of tracks, over plan_by_tile's index of the tracks' events laid one track behind the other.  With SEQRUNS_MAIN it is a
// program of its own (its own main, a fixed list of songs against a restatement in place, and the far-out lists of cpu_seqfar.hpp as songs
// of tracks past 2^31 samples), which a sanitizer build (-fsanitize=address,undefined) can run as it stands.
#include "../synthesizer_amd/csrc/seqplan.hpp"

namespace {
struct Runs {
    shq::TilePlan by_tile;
    shq::RunPlan runs;
};
}  // namespace

extern "C" {

uint32_t sr_max_tracks(void) { return shq::MAX_TRACKS; }

// dst[e], n[e], track_of[e]: the events, track-major (track_of does not decrease)
void* sr_plan(const uint64_t* dst, const uint64_t* n, const uint32_t* track_of, uint32_t nev, uint64_t track_samples, uint32_t tile, int* refused) {
    std::vector<shq::Event> ev(nev);
    for (uint32_t e = 0; e < nev; ++e) ev[e] = shq::Event{dst[e], n[e]};
    Runs* R = new Runs;
    R->by_tile = shq::plan_by_tile(ev.data(), nev, track_samples, tile);
    *refused = (int)R->by_tile.refused;
    if (!R->by_tile.refused) R->runs = shq::plan_runs(R->by_tile.first.data(), R->by_tile.idx.data(), R->by_tile.ntiles, track_of);
    return R;
}
void sr_free(void* p) { delete (Runs*)p; }
uint32_t sr_ntiles(const void* p) { return ((const Runs*)p)->by_tile.ntiles; }
uint64_t sr_npairs(const void* p) { return ((const Runs*)p)->by_tile.idx.size(); }
uint64_t sr_nruns(const void* p) { return ((const Runs*)p)->runs.runs.size(); }
uint64_t sr_nrfirst(const void* p) { return ((const Runs*)p)->runs.rfirst.size(); }
const uint32_t* sr_first(const void* p) { return ((const Runs*)p)->by_tile.first.data(); }
const uint32_t* sr_idx(const void* p) { return ((const Runs*)p)->by_tile.idx.data(); }
const uint32_t* sr_rfirst(const void* p) { return ((const Runs*)p)->runs.rfirst.data(); }
const uint32_t* sr_runs(const void* p) { return (const uint32_t*)((const Runs*)p)->runs.runs.data(); }      // (end, track) pairs
uint32_t sr_run_bytes(void) { return (uint32_t)sizeof(shq::Run); }

}  // extern "C"

#ifdef SEQRUNS_MAIN
#include "cpu_seqfar.hpp"
#include <cstdio>
// the runs of a near list dealt over ntracks tracks and moved to base b: nothing in front of the song and the near runs behind it where the
// base is a multiple of the tile; the restatement below at the far coordinates either way
static bool far_runs(uint32_t tile, const far::List& l, uint32_t ntracks, const far::Base& b) {
    far::List near_l{l.track, {}};                             // track-major: track k holds events k, k + ntracks, ... in list order
    std::vector<uint32_t> track_of;
    for (uint32_t k = 0; k < ntracks; ++k)
        for (size_t e = k; e < l.ev.size(); e += ntracks) { near_l.ev.push_back(l.ev[e]); track_of.push_back(k); }
    const far::List f = far::shifted(near_l, b.B);
    const shq::TilePlan N = shq::plan_by_tile(near_l.ev.data(), (uint32_t)near_l.ev.size(), near_l.track, tile);
    const shq::TilePlan P = shq::plan_by_tile(f.ev.data(), (uint32_t)f.ev.size(), f.track, tile);
    if (N.refused || P.refused) return false;
    const shq::RunPlan RN = shq::plan_runs(N.first.data(), N.idx.data(), N.ntiles, track_of.data());
    const shq::RunPlan R = shq::plan_runs(P.first.data(), P.idx.data(), P.ntiles, track_of.data());
    if (R.rfirst.size() != (size_t)P.ntiles + 1 || R.rfirst[0] != 0 || R.rfirst.back() != R.runs.size()) return false;
    if (b.aligned) {
        const uint32_t k = (uint32_t)(b.B / tile);
        if (P.ntiles != k + N.ntiles || R.runs.size() != RN.runs.size()) return false;
        for (uint32_t t = 0; t < k; ++t) if (R.rfirst[t] != 0) return false;
        for (uint32_t t = 0; t <= N.ntiles; ++t) if (R.rfirst[k + t] != RN.rfirst[t]) return false;
        for (size_t r = 0; r < R.runs.size(); ++r) if (R.runs[r].end != RN.runs[r].end || R.runs[r].track != RN.runs[r].track) return false;
    }
    for (uint32_t t = 0; t < P.ntiles; ++t) {                  // every tile's slice cut where the track changes
        uint32_t e = P.first[t], r = R.rfirst[t];
        while (e < P.first[t + 1]) {
            uint32_t end = e;
            while (end < P.first[t + 1] && track_of[P.idx[end]] == track_of[P.idx[e]]) ++end;
            if (r >= R.rfirst[t + 1] || R.runs[r].end != end || R.runs[r].track != track_of[P.idx[e]]) return false;
            e = end;
            ++r;
        }
        if (r != R.rfirst[t + 1]) return false;
    }
    return true;
}
// every tile's runs against the tile's slice of idx cut where the track changes, over a few hundred generated songs
int main() {
    uint64_t state = 88172645463325252ull;
    auto rnd = [&](uint64_t m) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state % m; };
    unsigned songs = 0, nruns = 0;
    for (int k = 0; k < 400; ++k) {
        const uint32_t tile = k % 3 ? 1024 : 8, ntiles = 1 + (uint32_t)rnd(40), ntracks = 1 + (uint32_t)rnd(shq::MAX_TRACKS);
        const uint64_t track_samples = (uint64_t)ntiles * tile - rnd(tile);
        std::vector<shq::Event> ev;
        std::vector<uint32_t> track_of;
        for (uint32_t t = 0; t < ntracks; ++t)
            for (uint64_t e = rnd(12); e > 0; --e) {
                const uint64_t n = rnd(3 * tile) % (track_samples + 1), dst = rnd(track_samples - n + 1);
                ev.push_back(shq::Event{dst, n});
                track_of.push_back(t);
            }
        const shq::TilePlan P = shq::plan_by_tile(ev.data(), (uint32_t)ev.size(), track_samples, tile);
        if (P.refused) { printf("song %d refused\n", k); return 1; }
        const shq::RunPlan R = shq::plan_runs(P.first.data(), P.idx.data(), P.ntiles, track_of.data());
        if (R.rfirst.size() != (size_t)P.ntiles + 1 || R.rfirst[0] != 0 || R.rfirst.back() != R.runs.size()) { printf("song %d: rfirst\n", k); return 1; }
        for (uint32_t t = 0; t < P.ntiles; ++t) {
            uint32_t e = P.first[t], r = R.rfirst[t];
            while (e < P.first[t + 1]) {                       // the slice cut where the track changes
                uint32_t end = e;
                while (end < P.first[t + 1] && track_of[P.idx[end]] == track_of[P.idx[e]]) ++end;
                if (r >= R.rfirst[t + 1] || R.runs[r].end != end || R.runs[r].track != track_of[P.idx[e]]) { printf("song %d tile %u: run %u\n", k, t, r); return 1; }
                e = end;
                ++r;
            }
            if (r != R.rfirst[t + 1]) { printf("song %d tile %u: %u runs too many\n", k, t, R.rfirst[t + 1] - r); return 1; }
        }
        ++songs;
        nruns += (unsigned)R.runs.size();
    }
    unsigned far_songs = 0;
    for (uint32_t tile : {shq::TILE_I16, shq::TILE_W})
        for (const far::List& l : far::near_lists(tile))
            for (uint32_t ntracks : {1u, 3u})
                for (const far::Base& b : far::bases(tile, l)) {
                    if (!far_runs(tile, l, ntracks, b)) { printf("tile %u, %u tracks, base %s: the far runs\n", tile, ntracks, b.name); return 1; }
                    ++far_songs;
                }
    printf("seqruns: %u songs, %u runs, %u far songs: ok\n", songs, nruns, far_songs);
    return 0;
}
#endif
