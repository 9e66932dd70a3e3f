// The far-out cases that the stand-alone programs of cpu_seqplan.cpp, cpu_seqtiles.cpp and cpu_seqruns.cpp share: a handful of near
// lists (tests/test_seqplan.py's near_lists, restated), the bases that carry them past 2^31 samples and up to the last tile a track can
// have, and the brute-force overlap count they are compared with where the base is no multiple of the tile.
#pragma once
#include "../synthesizer_amd/csrc/seqplan.hpp"
#include <map>

namespace far {

constexpr uint64_t MAX = shq::MAX_TRACK_SAMPLES;
constexpr uint64_t DM_LIMIT = (1ull << 31) - 32768;          // where a downmix ends at the latest: sequence.hip forms 2 (dst + n) in 32 bits

struct List {
    uint64_t track;
    std::vector<shq::Event> ev;
};

inline std::vector<List> near_lists(uint32_t tile) {
    const uint64_t T = tile, L = tile / 256, w0 = T + 3 * L;
    std::vector<List> out;
    // the four-tile song of the GPU tests: a note across the first tile edge, a pile-up in tile 1, tile 2 idle, the end mid-lane in tile 3
    out.push_back(List{3 * T + 37 * L + 3, {{0, 300}, {T - T / 4, T / 2}, {w0 - L, 3 * L}, {w0 + 10, T / 8}, {w0 + 13, T / 8}, {w0 + 17, T / 8}, {3 * T, 37 * L + 3}}});
    // on and around every tile edge, empty events between; a whole number of tiles
    out.push_back(List{4 * T, {{0, 0}, {T - 1, 1}, {T - 1, 2}, {T, T}, {2 * T, 0}, {3 * T - 1, T + 1}, {5, 4 * T - 5}, {4 * T - 1, 1}}});
    out.push_back(List{7 * T, {{0, 7 * T}, {3 * T + 1, 2}, {7 * T - 2, 2}}});
    uint64_t state = 88172645463325252ull + tile;
    auto rnd = [&](uint64_t m) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state % m; };
    for (uint64_t ntiles : {3ull, 17ull}) {
        List l{ntiles * T - 1 - rnd(T - 1), {}};
        for (int k = 0; k < 60; ++k) {
            const uint64_t pick[6] = {0, 1, T - 1, T, T + 1, rnd(3 * T)};
            const uint64_t n = std::min(pick[rnd(6)], l.track);
            l.ev.push_back(shq::Event{rnd(l.track - n + 1), n});
        }
        out.push_back(l);
    }
    return out;
}

struct Base {
    const char* name;
    uint64_t B;
    bool aligned;
};

// mid: the list's second tile starts on sample 2^31; top: its last tile is the last one a track can have; dm: its first sounding event ends
// on the downmix limit, no multiple of the tile
inline std::vector<Base> bases(uint32_t tile, const List& l) {
    const uint64_t ntiles = (l.track + tile - 1) / tile;
    uint64_t dm = DM_LIMIT;
    for (const shq::Event& e : l.ev)
        if (e.n) { dm -= e.dst + e.n; break; }
    if (dm % tile == 0) dm -= 3;
    return {{"mid", (1ull << 31) - tile, true}, {"top", MAX - ntiles * tile, true}, {"dm", dm, false}};
}

inline List shifted(const List& l, uint64_t B) {
    List s{l.track + B, l.ev};
    for (shq::Event& e : s.ev) e.dst += B;
    return s;
}

// tile -> the events that overlap it, in list order: an event covers [dst, dst + n)
inline std::map<uint32_t, std::vector<uint32_t>> brute(const List& l, uint32_t tile) {
    std::map<uint32_t, std::vector<uint32_t>> per;
    for (uint32_t e = 0; e < l.ev.size(); ++e)
        if (l.ev[e].n)
            for (uint64_t t = l.ev[e].dst / tile; t <= (l.ev[e].dst + l.ev[e].n - 1) / tile; ++t) per[(uint32_t)t].push_back(e);
    return per;
}

}  // namespace far
