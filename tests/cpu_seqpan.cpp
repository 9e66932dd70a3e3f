// Host build of synthesizer_amd/csrc/seqpan.hpp for tests/test_seqpan.py (g++, no GPU): the pan lane's statements as sequence.hip takes
// them -- shp::check (a verdict with a reason, the lane and the segment), the numbering of the pan lanes, and shp::shape_from, "shape this
// lane's N samples through pan lane L, else the static factors", run tile by tile and lane by lane as the kernels run it (a binary search
// at the tile's first sample, then one of the three uniform paths) and held to a straight loop over the frames that knows nothing of
// tiles.  sp_selfcheck holds random lanes at both lane widths, the three paths at tile positions on segment boundaries, origins past 2^31
// samples, the endpoints (-1, 1) and (1, -1) at extreme sample values, and every refusal in the order the check reports them; with
// -DSEQPAN_MAIN the file is a program that runs it, for a stand-alone build under -fsanitize=address,undefined.
#include "../synthesizer_amd/csrc/seqpan.hpp"
#include <stdio.h>
#include <initializer_list>
#include <limits>
#include <vector>

namespace {

struct Segment {                                             // sh_env_segment's fields (include/synthhip.h)
    uint64_t end, origin;
    double   mul, slope, numsamples, offset;
    uint32_t kind, reserved;
};

Segment move(uint64_t a, uint64_t b, double p0, double p1) { return Segment{2 * b, 2 * a, 1.0, p1 - p0, (double)(b - a), p0, shp::PAN, 0}; }   // frames [a, b)
Segment gap(uint64_t b) { return Segment{2 * b, 0, 1.0, 0.0, 0.0, 0.0, she::NONE, 0}; }

she::Seg seg(const Segment& g) { return she::Seg{g.mul, g.slope, g.numsamples, g.offset, (uint32_t)g.end, (uint32_t)g.origin, g.kind, 0}; }

// a sample of the width's range at song position s: a hash, with the range's ends and zero and minus one among the values
int sample(uint64_t s, int width, uint64_t seed) {
    uint64_t h = (s + seed) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    const long long lo = -(1ll << (8 * width - 1)), hi = (1ll << (8 * width - 1)) - 1;
    switch (h & 15u) {
    case 0: return (int)lo;
    case 1: return (int)hi;
    case 2: return 0;
    case 3: return -1;
    case 4: return (int)(lo + 1);
    default: return (int)(lo + (long long)((h >> 8) % (uint64_t)(hi - lo + 1)));
    }
}

// the straight loop: sample s of the lane through the FRAME that holds it -- the move that covers the frame (Sample.pan(lfo=...)'s
// expression, k counting frames from the move's first), else the static factors (audioop.mul per side)
int straight(const std::vector<she::Seg>& segs, uint64_t s, int x, double left, double right, double lo, double hi) {
    uint64_t prev = 0;
    for (const she::Seg& g : segs) {
        if (s >= prev && s < g.end) {
            if (g.kind != shp::PAN) break;
            const uint64_t k = (s - g.origin) / 2;
            const double p = (double)k * g.slope / g.numsamples + g.offset;
            const double v = s % 2 ? (double)x * (1.0 + p) / 2.0 : (double)x * (1.0 - p) / 2.0;
            return (int)(v < 0 ? std::ceil(v) : std::floor(v));
        }
        prev = g.end;
    }
    const double f = s % 2 ? right : left;
    if (f == 1.0) return x;
    double v = (double)x * f;
    if (v > hi) v = hi;
    else if (v < lo + 1.0) v = lo;
    return (int)std::floor(v);
}

// tiles [tile0, tile1) of TILE = 256 N samples as the kernels take them; the mismatches against the straight loop, and whether a result
// left the width's range.  paths[0 .. 3): how many tiles took the static path, the one-move path and the straddling one.
template <int N>
int run_tiles(const std::vector<she::Seg>& segs, uint64_t tile0, uint64_t tile1, int width, double left, double right, uint64_t seed, int* paths) {
    const uint32_t TILE = 256u * N, n = (uint32_t)segs.size();
    const double lo = -(double)(1ll << (8 * width - 1)), hi = (double)((1ll << (8 * width - 1)) - 1);
    int bad = 0;
    for (uint64_t k = tile0; k < tile1; ++k) {
        const uint32_t t0 = (uint32_t)(k * TILE), t1 = t0 + TILE;
        const uint32_t i = sha::find(segs.data(), n, t0);
        if (paths) {
            if (shp::plain(segs.data(), n, i, t1)) ++paths[0];
            else if (segs[i].kind == shp::PAN && segs[i].end >= t1) ++paths[1];
            else ++paths[2];
        }
        for (uint32_t lane = 0; lane < 256; ++lane) {
            const long long p0 = (long long)t0 + lane * N;
            int x[N], want[N];
            for (int j = 0; j < N; ++j) {
                x[j] = sample((uint64_t)p0 + j, width, seed);
                want[j] = straight(segs, (uint64_t)p0 + j, x[j], left, right, lo, hi);
            }
            shp::shape_from<N>(segs.data(), n, i, t0, t1, p0, x, left, right, lo, hi);
            for (int j = 0; j < N; ++j) bad += x[j] != want[j] || (double)x[j] < lo || (double)x[j] > hi;
        }
    }
    return bad;
}

uint64_t rnd(uint64_t& state) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return state >> 33;
}

// a random lane over `frames` frames from frame `from` on: gaps, moves, holds, adjacent moves, one-frame moves
std::vector<she::Seg> random_lane(uint64_t from, uint64_t frames, uint64_t& state) {
    std::vector<she::Seg> segs;
    uint64_t at = 0, f = from;                               // at: where the segment before ends
    for (;;) {
        if (rnd(state) & 1u) f += 1 + rnd(state) % 900;      // a gap, or a move adjacent to the one before
        if (f >= from + frames) break;
        if (f > at) segs.push_back(seg(gap(f)));             // a move starts where the segment before it ends
        uint64_t len = 1 + rnd(state) % ((rnd(state) & 3u) ? 700 : 3);
        if (f + len > from + frames) len = from + frames - f;
        const double p0 = (double)(rnd(state) % 2001) / 1000.0 - 1.0;
        const double p1 = (rnd(state) & 3u) ? (double)(rnd(state) % 2001) / 1000.0 - 1.0 : p0;
        segs.push_back(seg(move(f, f + len, p0, p1)));
        at = f = f + len;
    }
    return segs;
}

// a pan table of nlanes lanes, every lane a gap to frame 50 and a move over frames [50, 100), with `bad` in place of one segment
int verdict(uint32_t nlanes, uint32_t lane, uint32_t segment, const Segment& bad, shp::Refusal why, uint64_t song = 1000) {
    std::vector<Segment> segs;
    std::vector<uint32_t> first(1, 0);
    for (uint32_t t = 0; t < nlanes; ++t) {
        segs.push_back(gap(50));
        segs.push_back(move(50, 100, -0.25, 1.0));
        if (t == lane) segs[segs.size() - 2 + segment] = bad;
        first.push_back((uint32_t)segs.size());
    }
    const shp::Verdict v = shp::check(segs.data(), (uint32_t)segs.size(), first.data(), nlanes, song);
    return v.why != why || (why != shp::OK && (v.lane != lane || v.segment != segment));
}

}  // namespace

extern "C" {

// 0 (the table passes) or the refusal's number; *lane and *segment: where.  rows: n x (end, origin, mul, slope, numsamples, offset, kind,
// reserved) as doubles
int sp_check(const double* rows, uint32_t n, const uint32_t* seg_first, uint32_t nlanes, double track_samples, uint32_t* lane, uint32_t* segment) {
    std::vector<Segment> s(n);
    for (uint32_t i = 0; i < n; ++i) {
        const double* r = rows + 8 * i;
        s[i] = Segment{(uint64_t)r[0], (uint64_t)r[1], r[2], r[3], r[4], r[5], (uint32_t)r[6], (uint32_t)r[7]};
    }
    const shp::Verdict v = shp::check(s.data(), n, seg_first, nlanes, (uint64_t)track_samples);
    *lane = v.lane;
    *segment = v.segment;
    return (int)v.why;
}

uint32_t sp_track_lane(uint32_t row0, uint32_t t) { return shp::track_lane(row0, t); }
uint32_t sp_group_lane(uint32_t row0, uint32_t g) { return shp::group_lane(row0, g); }
uint32_t sp_lanes(uint32_t ntracks, uint32_t ngroups) { return shp::lanes(ntracks, ngroups); }
uint32_t sp_kind() { return shp::PAN; }

// samples[0 .. nsamples) (nsamples a multiple of 256 * lane_width, the song from sample 0 on) through the lane rows (as sp_check's), tile by
// tile as the kernels go; lane_width 4 or 8
int sp_shape(const double* rows, uint32_t n, int* samples, uint32_t nsamples, int lane_width, int width, double left, double right) {
    std::vector<she::Seg> segs(n);
    for (uint32_t i = 0; i < n; ++i) {
        const double* r = rows + 8 * i;
        segs[i] = she::Seg{r[2], r[3], r[4], r[5], (uint32_t)r[0], (uint32_t)r[1], (uint32_t)r[6], 0};
    }
    const uint32_t TILE = 256u * lane_width;
    if ((lane_width != 4 && lane_width != 8) || nsamples % TILE) return -1;
    const double lo = -(double)(1ll << (8 * width - 1)), hi = (double)((1ll << (8 * width - 1)) - 1);
    for (uint32_t t0 = 0; t0 < nsamples; t0 += TILE) {
        const uint32_t i = sha::find(segs.data(), n, t0);
        for (uint32_t p0 = t0; p0 < t0 + TILE; p0 += lane_width) {
            if (lane_width == 4) shp::shape_from<4>(segs.data(), n, i, t0, t0 + TILE, p0, *reinterpret_cast<int(*)[4]>(samples + p0), left, right, lo, hi);
            else shp::shape_from<8>(segs.data(), n, i, t0, t0 + TILE, p0, *reinterpret_cast<int(*)[8]>(samples + p0), left, right, lo, hi);
        }
    }
    return 0;
}

// the number of mismatches
int sp_selfcheck() {
    int bad = 0;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // the pan lanes stand behind the fader lanes' row0 + 8 + 1 offsets: the tracks', then the groups'
    for (uint32_t ntracks = 1; ntracks <= 32; ++ntracks) {
        const uint32_t row0 = ntracks + 1;
        for (uint32_t t = 0; t < ntracks; ++t) bad += shp::track_lane(row0, t) != sha::lanes(ntracks, 8) + 1 + t;
        for (uint32_t g = 0; g < 8; ++g) bad += shp::group_lane(row0, g) != sha::lanes(ntracks, 8) + 1 + ntracks + g;
        bad += shp::lanes(ntracks, 8) != ntracks + 8;
    }
    // random lanes against the straight loop, lane widths 4 and 8, widths 1, 2 and 4, static factors of every sort
    const double factors[][2] = {{1.0, 1.0}, {0.5, 0.5}, {0.25, 1.0}, {1.0, 0.0}, {1.5, 0.75}, {0.0, 0.0}};
    uint64_t state = 12345;
    int paths[3] = {0, 0, 0};
    for (int round = 0; round < 12; ++round) {
        const std::vector<she::Seg> segs = random_lane(0, 9000, state);
        const double* f = factors[round % 6];
        for (int width : {1, 2, 4}) {
            bad += run_tiles<4>(segs, 0, 20, width, f[0], f[1], (uint64_t)round, paths);      // 20 tiles of 1024: past the lane's end
            bad += run_tiles<8>(segs, 0, 10, width, f[0], f[1], (uint64_t)round, paths);
        }
    }
    bad += !(paths[0] && paths[1] && paths[2]);
    // the three paths at tile positions on segment boundaries (N = 8: tiles of 2048 samples, 1024 frames)
    {
        std::vector<she::Seg> segs;
        segs.push_back(seg(gap(1024)));                      // tile 0: no move (a plain segment that ends ON the tile's end)
        segs.push_back(seg(move(1024, 3072, -1.0, 1.0)));    // tiles 1 and 2: inside one move, which starts and ends on tile edges
        segs.push_back(seg(move(3072, 3073, 0.5, 0.5)));     // tile 3: a one-frame move at the tile's first frame, adjacent to the one before
        segs.push_back(seg(gap(4095)));
        segs.push_back(seg(move(4095, 4097, 1.0, -1.0)));    // across the edge of tiles 3 and 4
        segs.push_back(seg(gap(6143)));
        segs.push_back(seg(move(6143, 6144, -1.0, -1.0)));   // tile 5: its last frame alone; tiles 6 ..: behind the lane's last segment
        int p[3] = {0, 0, 0};
        for (int width : {1, 2, 4}) bad += run_tiles<8>(segs, 0, 8, width, 0.75, 0.25, 7, p);
        bad += !(p[0] == 3 * 3 && p[1] == 3 * 2 && p[2] == 3 * 3);      // tiles 0, 6, 7 | 1, 2 | 3, 4, 5
        int q[3] = {0, 0, 0};
        for (int width : {1, 2, 4}) bad += run_tiles<4>(segs, 0, 16, width, 0.75, 0.25, 7, q);
        bad += !(q[0] && q[1] && q[2]);
    }
    // origins past 2^31 samples: a move over frames [2^30 + 100, 2^30 + 5000) and a later one, the tiles around them
    {
        const uint64_t f0 = (1ull << 30) + 100;
        std::vector<she::Seg> segs;
        segs.push_back(seg(gap(f0)));
        segs.push_back(seg(move(f0, f0 + 4900, -0.9, 0.8)));
        segs.push_back(seg(move(f0 + 4900, f0 + 4901, 1.0, 1.0)));
        segs.push_back(seg(gap((1ull << 30) + (1ull << 29))));
        segs.push_back(seg(move((1ull << 30) + (1ull << 29), (1ull << 30) + (1ull << 29) + 3000, 0.3, -1.0)));
        bad += segs[1].origin <= 0x80000000u;
        for (int width : {1, 2, 4}) {
            bad += run_tiles<8>(segs, (1ull << 31) / 2048 - 1, (1ull << 31) / 2048 + 7, width, 0.5, 1.0, 3, nullptr);
            bad += run_tiles<4>(segs, (1ull << 31) / 1024 - 1, (1ull << 31) / 1024 + 12, width, 0.5, 1.0, 3, nullptr);
            bad += run_tiles<8>(segs, (3ull << 30) / 2048 - 1, (3ull << 30) / 2048 + 4, width, 0.5, 1.0, 3, nullptr);
        }
    }
    // the endpoints (-1, 1) and (1, -1) at extreme samples: every result inside the width's range and no larger than the sample; a full
    // side passes the sample through, the other side gives 0
    for (int width : {1, 2, 4}) {
        const long long lo = -(1ll << (8 * width - 1)), hi = (1ll << (8 * width - 1)) - 1;
        for (const uint64_t frames : std::initializer_list<uint64_t>{1, 2, 3, 7, 1000, 65537, (1ull << 31) - 1}) {
            for (int dir = 0; dir < 2; ++dir) {
                const she::Seg g = seg(move(0, frames, dir ? 1.0 : -1.0, dir ? -1.0 : 1.0));
                for (const uint64_t k : std::initializer_list<uint64_t>{0, 1, frames / 3, frames / 2, frames - 2, frames - 1}) {
                    if (k >= frames) continue;
                    const double p = shp::pan_of(g, (long long)(2 * k));
                    bad += !(p >= -1.0 - 0x1p-52 && p <= 1.0 + 0x1p-52);
                    for (const long long x : std::initializer_list<long long>{lo, lo + 1, -1, 0, 1, hi - 1, hi}) {
                        int l = (int)x, r = (int)x;
                        shp::ride(p, l, r);
                        bad += l < lo || l > hi || r < lo || r > hi;
                        bad += (x >= 0 ? (l < 0 || l > x || r < 0 || r > x) : (l > 0 || l < x || r > 0 || r < x));
                        if (k == 0) bad += dir ? (l != 0 || r != x) : (l != x || r != 0);
                    }
                }
            }
        }
    }
    // accepted: tables of 3 tracks with 0 and with 8 group lanes; an empty table
    const Segment good = move(50, 100, -0.25, 1.0);
    bad += verdict(shp::lanes(3, 0), 0, 1, good, shp::OK);
    bad += verdict(shp::lanes(3, 8), 0, 1, good, shp::OK);
    {
        const uint32_t first[12] = {0};
        bad += shp::check((const Segment*)nullptr, 0, first, 11, 1000).why != shp::OK;
    }
    // every refusal in its order, on a track's lane (1) and on the last group's (10) of 3 tracks and 8 groups
    const uint32_t n = shp::lanes(3, 8);
    for (uint32_t lane : {1u, 10u}) {
        Segment s = good;
        s.reserved = 1;
        s.end = 50;                                          // (and an end that does not ascend: the reserved word is reported)
        bad += verdict(n, lane, 1, s, shp::RESERVED);
        s = good;
        s.end = 100;                                         // not past the one before
        s.kind = 1;
        bad += verdict(n, lane, 1, s, shp::ENDS);
        s = good;
        s.end = 1002;                                        // past the song
        bad += verdict(n, lane, 1, s, shp::ENDS);
        s = move(50, 500, -0.25, 1.0);                       // the song's last frame: passes
        bad += verdict(n, lane, 1, s, shp::OK);
        s = gap(0);                                          // a first segment that ends at 0
        bad += verdict(n, lane, 0, s, shp::ENDS);
        s = good;
        s.end = 199;                                         // half a frame
        s.kind = 1;
        bad += verdict(n, lane, 1, s, shp::ODD);
        for (uint32_t kind : {1u, 2u, 4u}) {                 // a fade is no pan move
            s = good;
            s.kind = kind;
            s.mul = 0.5;
            bad += verdict(n, lane, 1, s, shp::KIND);
        }
        s = good;
        s.mul = 0.5;
        s.origin = 4;
        bad += verdict(n, lane, 1, s, shp::MUL);
        s = gap(50);
        s.mul = 0.999;                                       // a plain segment has no mul either
        bad += verdict(n, lane, 0, s, shp::MUL);
        s = good;
        s.origin = 98;
        s.numsamples = 1.0;
        bad += verdict(n, lane, 1, s, shp::ORIGIN);
        s = move(0, 50, 0.5, 0.5);                           // a first move starts at 0
        bad += verdict(n, lane, 0, s, shp::OK);
        s.origin = 2;
        bad += verdict(n, lane, 0, s, shp::ORIGIN);
        s = good;
        s.numsamples = 49.0;                                 // its FRAMES are 50 (100 samples would pass a count in samples)
        s.offset = 2.0;
        bad += verdict(n, lane, 1, s, shp::NUMSAMPLES);
        s.numsamples = nan;
        bad += verdict(n, lane, 1, s, shp::NUMSAMPLES);
        s = good;
        s.numsamples = inf;
        bad += verdict(n, lane, 1, s, shp::RANGE);
        for (const double offset : {-1.001, 1.001, nan, inf}) {
            s = good;
            s.offset = offset;
            s.slope = 0.0;
            bad += verdict(n, lane, 1, s, shp::RANGE);
        }
        for (const double slope : {1.251, -0.751, nan, -inf}) {     // offset -0.25: the end pan leaves -1 .. 1
            s = good;
            s.slope = slope;
            bad += verdict(n, lane, 1, s, shp::RANGE);
        }
        s = good;
        s.slope = -0.75;                                     // to exactly -1.0
        bad += verdict(n, lane, 1, s, shp::OK);
        bad += verdict(n, lane, 1, move(50, 100, -1.0, 1.0), shp::OK);
        bad += verdict(n, lane, 1, move(50, 100, 1.0, -1.0), shp::OK);
    }
    // the offsets: in front of every segment
    {
        std::vector<Segment> segs(2, move(0, 50, 0.5, 1.0));
        segs[0].reserved = 1;
        const uint32_t starts_late[3] = {1, 2, 2}, ends_early[3] = {0, 1, 1}, decreases[4] = {0, 2, 1, 2};
        shp::Verdict v = shp::check(segs.data(), 2, starts_late, 2, 1000);
        bad += v.why != shp::FIRST_ENDS;
        v = shp::check(segs.data(), 2, ends_early, 2, 1000);
        bad += v.why != shp::FIRST_ENDS;
        v = shp::check(segs.data(), 2, decreases, 3, 1000);
        bad += v.why != shp::FIRST_DECREASES || v.lane != 2;
    }
    return bad;
}

}

#ifdef SEQPAN_MAIN
int main() {
    const int bad = sp_selfcheck();
    printf("cpu_seqpan: %d mismatches\n", bad);
    return bad ? 1 : 0;
}
#endif
