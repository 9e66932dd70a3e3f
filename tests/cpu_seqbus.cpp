// Host build of synthesizer_amd/csrc/seqauto.hpp for tests/test_seqbus.py (g++, no GPU): the pure check of an automation table
// (sha::check: a verdict with a reason, the lane and the segment) and the numbering of the lanes of the buses (sha::master_lane,
// sha::group_lane, sha::lanes).  sb_selfcheck holds every refusal, in the order the check reports them, and accepted tables with 0 and 8
// group lanes; with -DSEQBUS_MAIN the file is a program that runs it, for a stand-alone build under -fsanitize=address,undefined.
#include "../synthesizer_amd/csrc/seqauto.hpp"
#include <stdio.h>
#include <limits>
#include <vector>

namespace {

struct Segment {                                             // sh_env_segment's fields (include/synthhip.h)
    uint64_t end, origin;
    double   mul, slope, numsamples, offset;
    uint32_t kind, reserved;
};

const uint64_t SONG = 1000;

Segment move(uint64_t a, uint64_t b, double v0, double v1) { return Segment{b, a, 1.0, v1 - v0, (double)(b - a), v0, she::FADE_IN, 0}; }
Segment gap(uint64_t b) { return Segment{b, 0, 1.0, 0.0, 0.0, 0.0, she::NONE, 0}; }

// a table of nlanes lanes, every lane a gap to 100 and a move over [100, 200), with `bad` in place of segment `segment` of lane `lane`
int verdict(uint32_t nlanes, uint32_t lane, uint32_t segment, const Segment& bad, sha::Refusal why) {
    std::vector<Segment> segs;
    std::vector<uint32_t> first(1, 0);
    for (uint32_t t = 0; t < nlanes; ++t) {
        segs.push_back(gap(100));
        segs.push_back(move(100, 200, 0.25, 1.0));
        if (t == lane) segs[segs.size() - 2 + segment] = bad;
        first.push_back((uint32_t)segs.size());
    }
    const sha::Verdict v = sha::check(segs.data(), (uint32_t)segs.size(), first.data(), nlanes, SONG);
    return v.why != why || (why != sha::OK && (v.lane != lane || v.segment != segment));
}

}  // namespace

extern "C" {

// 0 (the table passes) or the refusal's number; *lane and *segment: where.  rows: n x (end, origin, mul, slope, numsamples, offset, kind,
// reserved) as doubles
int sb_check(const double* rows, uint32_t n, const uint32_t* seg_first, uint32_t nlanes, double track_samples, uint32_t* lane, uint32_t* segment) {
    std::vector<Segment> s(n);
    for (uint32_t i = 0; i < n; ++i) {
        const double* r = rows + 8 * i;
        s[i] = Segment{(uint64_t)r[0], (uint64_t)r[1], r[2], r[3], r[4], r[5], (uint32_t)r[6], (uint32_t)r[7]};
    }
    const sha::Verdict v = sha::check(s.data(), n, seg_first, nlanes, (uint64_t)track_samples);
    *lane = v.lane;
    *segment = v.segment;
    return (int)v.why;
}

uint32_t sb_master_lane(uint32_t row0) { return sha::master_lane(row0); }
uint32_t sb_group_lane(uint32_t row0, uint32_t g) { return sha::group_lane(row0, g); }
uint32_t sb_lanes(uint32_t ntracks, uint32_t ngroups) { return sha::lanes(ntracks, ngroups); }
uint32_t sb_max_group_lanes() { return sha::MAX_GROUP_LANES; }

// the number of mismatches
int sb_selfcheck() {
    int bad = 0;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // the lanes stand in the meter table's row order: the master behind the last track, the groups behind the master
    for (uint32_t ntracks = 1; ntracks <= 32; ++ntracks) {
        const uint32_t row0 = ntracks + 1;                   // shg::Table::row0
        bad += sha::master_lane(row0) != ntracks;
        for (uint32_t g = 0; g < sha::MAX_GROUP_LANES; ++g) bad += sha::group_lane(row0, g) != ntracks + 1 + g;
        bad += sha::lanes(ntracks, 0) != ntracks + 1 || sha::lanes(ntracks, 8) != ntracks + 9;
    }
    // accepted: 3 tracks and the master with 0 and with 8 group lanes; a track table alone; an empty table
    const Segment good = move(100, 200, 0.25, 1.0);
    bad += verdict(sha::lanes(3, 0), 0, 1, good, sha::OK);
    bad += verdict(sha::lanes(3, 8), 0, 1, good, sha::OK);
    bad += verdict(3, 0, 1, good, sha::OK);
    {
        const uint32_t first[13] = {0};
        bad += sha::check((const Segment*)nullptr, 0, first, 12, SONG).why != sha::OK;
    }
    // every refusal in its order, on a track's lane (1), the master's (3) and the last group's (11) of 3 tracks and 8 groups
    const uint32_t n = sha::lanes(3, 8);
    for (uint32_t lane : {1u, 3u, 11u}) {
        Segment s = good;
        s.reserved = 1;
        s.end = 50;                                          // (and an end that does not ascend: the reserved word is reported)
        bad += verdict(n, lane, 1, s, sha::RESERVED);
        s = good;
        s.end = 100;                                         // not past the one before
        s.kind = 2;
        bad += verdict(n, lane, 1, s, sha::ENDS);
        s = good;
        s.end = SONG + 1;                                    // past the song
        bad += verdict(n, lane, 1, s, sha::ENDS);
        s = good;
        s.end = SONG;                                        // the song's last sample: passes
        s.numsamples = (double)(SONG - 100);
        bad += verdict(n, lane, 1, s, sha::OK);
        s = gap(0);                                          // a first segment that ends at 0
        bad += verdict(n, lane, 0, s, sha::ENDS);
        s = good;
        s.kind = she::FADE_OUT;
        s.mul = 0.5;
        bad += verdict(n, lane, 1, s, sha::KIND);
        s = good;
        s.mul = 0.5;
        s.origin = 4;
        bad += verdict(n, lane, 1, s, sha::MUL);
        s = gap(100);
        s.mul = 0.999;                                       // a plain segment has no mul either
        bad += verdict(n, lane, 0, s, sha::MUL);
        s = good;
        s.origin = 99;
        s.numsamples = 1.0;
        bad += verdict(n, lane, 1, s, sha::ORIGIN);
        s = move(0, 100, 0.5, 0.5);                          // a first move starts at 0
        bad += verdict(n, lane, 0, s, sha::OK);
        s.origin = 1;
        bad += verdict(n, lane, 0, s, sha::ORIGIN);
        s = good;
        s.numsamples = 99.0;
        s.offset = 2.0;
        bad += verdict(n, lane, 1, s, sha::NUMSAMPLES);
        s.numsamples = nan;
        bad += verdict(n, lane, 1, s, sha::NUMSAMPLES);
        s = good;
        s.numsamples = 100.5;                                // longer than the move: a cut move, legal
        bad += verdict(n, lane, 1, s, sha::OK);
        s.numsamples = inf;
        bad += verdict(n, lane, 1, s, sha::VOLUME);
        for (const double offset : {-0.001, 1.001, nan, inf}) {
            s = good;
            s.offset = offset;
            s.slope = 0.0;
            bad += verdict(n, lane, 1, s, sha::VOLUME);
        }
        for (const double slope : {0.751, -0.251, nan, -inf}) {    // offset 0.25: the end volume leaves 0 .. 1
            s = good;
            s.slope = slope;
            bad += verdict(n, lane, 1, s, sha::VOLUME);
        }
        s = good;
        s.slope = -0.25;                                     // to exactly 0.0
        bad += verdict(n, lane, 1, s, sha::OK);
    }
    // the offsets: in front of every segment
    {
        std::vector<Segment> segs(2, good);
        segs[0].reserved = 1;
        const uint32_t starts_late[3] = {1, 2, 2}, ends_early[3] = {0, 1, 1}, decreases[4] = {0, 2, 1, 2};
        sha::Verdict v = sha::check(segs.data(), 2, starts_late, 2, SONG);
        bad += v.why != sha::FIRST_ENDS;
        v = sha::check(segs.data(), 2, ends_early, 2, SONG);
        bad += v.why != sha::FIRST_ENDS;
        v = sha::check(segs.data(), 2, decreases, 3, SONG);
        bad += v.why != sha::FIRST_DECREASES || v.lane != 2;
    }
    return bad;
}

}

#ifdef SEQBUS_MAIN
int main() {
    const int bad = sb_selfcheck();
    printf("cpu_seqbus: %d mismatches\n", bad);
    return bad ? 1 : 0;
}
#endif
