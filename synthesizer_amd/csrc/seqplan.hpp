// seqplan.hpp -- which tiles of a track a list of placed samples touches, and which events each of them folds, in which order
// (sh_mix_events, sequence.hip): the active tiles, heaviest first, and per tile the indices of its events in list order, as one
// CSR array.  plan_by_tile is the same index for a list that is kept (sh_seq_create): EVERY tile of the song in song order, so that a
// window of the song finds its tiles by their number.  Plain C++17, no HIP include (tests/cpu_seqplan.cpp and tests/cpu_seqtiles.cpp
// build it with g++): nothing here launches or allocates on the device.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace shq {

// The two lane shapes of the kernels of sequence.hip (their template arguments and launch bounds are these, nothing else states them): a workgroup of
// TILE_THREADS lanes per active tile, LANE_SAMPLES consecutive track samples per lane.
constexpr uint32_t TILE_THREADS = 256;
constexpr uint32_t LANE_SAMPLES_I16 = 8;                                   // 16-bit samples (k_seq_plain16, k_seq_16): one aligned 16-byte vector
constexpr uint32_t LANE_SAMPLES_W = 4;                                     // widths 1, 3, 4 (k_seq_w)
constexpr uint32_t TILE_I16 = TILE_THREADS * LANE_SAMPLES_I16;             // 2048 samples
constexpr uint32_t TILE_W = TILE_THREADS * LANE_SAMPLES_W;                 // 1024 samples
constexpr uint32_t tile_samples(int width) { return width == 2 ? TILE_I16 : TILE_W; }

// Index types: a sample position inside the track and an offset into the CSR array are 32 bits on the device.
constexpr uint64_t MAX_TRACK_SAMPLES = 0xFFFF0000ull;
constexpr uint64_t MAX_PAIRS = 1ull << 28;                                 // (event, tile) overlaps: 1 GB of indices

struct Event { uint64_t dst, n; };                                         // first track sample, samples (may be 0)

enum Refusal { OK = 0, EVENT_BEYOND_TRACK, TRACK_TOO_LONG, TOO_MANY_PAIRS };

struct Plan {
    Refusal refused = OK;
    uint32_t bad_event = 0;               // EVENT_BEYOND_TRACK: the first such event
    std::vector<uint32_t> tiles;          // the active tiles (track samples [t * tile, (t + 1) * tile)), non-increasing event count
    std::vector<uint32_t> first;          // tiles.size() + 1 offsets into idx: active tile k folds idx[first[k] .. first[k + 1])
    std::vector<uint32_t> idx;            // event indices, ascending inside a tile (= list order)
};

// A tile is active when at least one non-empty event overlaps it; the others are neither launched nor touched.  Heaviest first: one
// workgroup per tile, and a pile-up of hits on one bar must not be the last workgroup to start.  Counting pass, prefix sum over
// the sorted tiles, fill: O(pairs) besides the sort of the active tiles.
inline Plan plan(const Event* ev, uint32_t nev, uint64_t track_samples, uint32_t tile, uint64_t max_pairs = MAX_PAIRS) {
    Plan P;
    if (track_samples > MAX_TRACK_SAMPLES) { P.refused = TRACK_TOO_LONG; return P; }
    for (uint32_t e = 0; e < nev; ++e)
        if (ev[e].dst > track_samples || ev[e].n > track_samples - ev[e].dst) { P.refused = EVENT_BEYOND_TRACK; P.bad_event = e; return P; }
    const uint32_t ntiles = (uint32_t)((track_samples + tile - 1) / tile);
    std::vector<uint32_t> count(ntiles, 0);
    uint64_t pairs = 0;
    for (uint32_t e = 0; e < nev; ++e) {
        if (!ev[e].n) continue;
        const uint32_t t0 = (uint32_t)(ev[e].dst / tile), t1 = (uint32_t)((ev[e].dst + ev[e].n - 1) / tile);
        pairs += (uint64_t)(t1 - t0) + 1;
        if (pairs > max_pairs) { P.refused = TOO_MANY_PAIRS; return P; }
        for (uint32_t t = t0; t <= t1; ++t) ++count[t];
    }
    for (uint32_t t = 0; t < ntiles; ++t)
        if (count[t]) P.tiles.push_back(t);
    std::stable_sort(P.tiles.begin(), P.tiles.end(), [&](uint32_t a, uint32_t b) { return count[a] > count[b]; });
    P.first.assign(P.tiles.size() + 1, 0);
    std::vector<uint32_t>& cursor = count;                                  // from here on: where tile t's next index goes
    for (size_t k = 0; k < P.tiles.size(); ++k) {
        const uint32_t t = P.tiles[k];
        P.first[k + 1] = P.first[k] + count[t];
        cursor[t] = P.first[k];
    }
    P.idx.resize((size_t)pairs);
    for (uint32_t e = 0; e < nev; ++e) {
        if (!ev[e].n) continue;
        const uint32_t t0 = (uint32_t)(ev[e].dst / tile), t1 = (uint32_t)((ev[e].dst + ev[e].n - 1) / tile);
        for (uint32_t t = t0; t <= t1; ++t) P.idx[cursor[t]++] = e;
    }
    return P;
}

// The same index for a song that is kept and rendered window by window (sh_seq_create, sh_seq_render): every tile of the song in SONG
// order, tile t folding idx[first[t] .. first[t + 1]) -- an empty range where no event plays, which a window kernel renders as silence.
// A window's workgroups find their tiles by number, so nothing is sorted and nothing names the tiles.  plan's refusals, in plan's order.
struct TilePlan {
    Refusal refused = OK;
    uint32_t bad_event = 0;               // EVENT_BEYOND_TRACK: the first such event
    uint32_t ntiles = 0;                  // ceil(track_samples / tile)
    uint32_t active = 0;                  // tiles with at least one event
    std::vector<uint32_t> first;          // ntiles + 1 offsets into idx
    std::vector<uint32_t> idx;            // event indices, ascending inside a tile (= list order)
};

inline TilePlan plan_by_tile(const Event* ev, uint32_t nev, uint64_t track_samples, uint32_t tile, uint64_t max_pairs = MAX_PAIRS) {
    TilePlan P;
    if (track_samples > MAX_TRACK_SAMPLES) { P.refused = TRACK_TOO_LONG; return P; }
    for (uint32_t e = 0; e < nev; ++e)
        if (ev[e].dst > track_samples || ev[e].n > track_samples - ev[e].dst) { P.refused = EVENT_BEYOND_TRACK; P.bad_event = e; return P; }
    const uint32_t ntiles = (uint32_t)((track_samples + tile - 1) / tile);
    std::vector<uint32_t> count(ntiles, 0);
    uint64_t pairs = 0;
    for (uint32_t e = 0; e < nev; ++e) {
        if (!ev[e].n) continue;
        const uint32_t t0 = (uint32_t)(ev[e].dst / tile), t1 = (uint32_t)((ev[e].dst + ev[e].n - 1) / tile);
        pairs += (uint64_t)(t1 - t0) + 1;
        if (pairs > max_pairs) { P.refused = TOO_MANY_PAIRS; return P; }
        for (uint32_t t = t0; t <= t1; ++t) ++count[t];
    }
    P.ntiles = ntiles;
    P.first.assign((size_t)ntiles + 1, 0);
    std::vector<uint32_t>& cursor = count;                                  // from here on: where tile t's next index goes
    for (uint32_t t = 0; t < ntiles; ++t) {
        if (count[t]) ++P.active;
        P.first[t + 1] = P.first[t] + count[t];
        cursor[t] = P.first[t];
    }
    P.idx.resize((size_t)pairs);
    for (uint32_t e = 0; e < nev; ++e) {
        if (!ev[e].n) continue;
        const uint32_t t0 = (uint32_t)(ev[e].dst / tile), t1 = (uint32_t)((ev[e].dst + ev[e].n - 1) / tile);
        for (uint32_t t = t0; t <= t1; ++t) P.idx[cursor[t]++] = e;
    }
    return P;
}

// A kept song made of TRACKS (sh_seq_create_tracks): the events of the tracks are concatenated track-major, so track_of -- one track per
// event -- does not decrease along the list, every tile's slice of plan_by_tile's idx (ascending event indices) is already in (track, list)
// order, and idx stays as it is.  What a window kernel needs besides is where, inside a tile's slice, one track's events end and the next
// one's begin: per tile its RUNS, one per track that has events there, in track order -- runs[rfirst[t] .. rfirst[t + 1]), run r covering
// idx[(r == rfirst[t] ? first[t] : runs[r - 1].end) .. runs[r].end).  An idle tile has none; a tile's last run ends at first[t + 1].
constexpr uint32_t MAX_TRACKS = 32;

struct Run { uint32_t end, track; };                                       // end: exclusive, an offset into idx

struct RunPlan {
    std::vector<uint32_t> rfirst;         // ntiles + 1 offsets into runs
    std::vector<Run> runs;
};

inline RunPlan plan_runs(const uint32_t* first, const uint32_t* idx, uint32_t ntiles, const uint32_t* track_of) {
    RunPlan R;
    R.rfirst.assign((size_t)ntiles + 1, 0);
    for (uint32_t t = 0; t < ntiles; ++t) {
        for (uint32_t e = first[t]; e < first[t + 1]; ++e) {
            const uint32_t track = track_of[idx[e]];
            if (e == first[t] || R.runs.back().track != track) R.runs.push_back(Run{e + 1, track});
            else R.runs.back().end = e + 1;
        }
        R.rfirst[t + 1] = (uint32_t)R.runs.size();
    }
    return R;
}

}  // namespace shq
