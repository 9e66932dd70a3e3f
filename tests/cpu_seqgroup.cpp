// Host build of synthesizer_amd/csrc/seqgroup.hpp for tests/test_seqgroup.py (g++, no GPU): the checks of a group list and its packing
// into the byte-per-track table the kernels of sequence.hip take by value.  sg_selfcheck holds both against a plain restatement -- the
// group of every track by a scan over the entries -- for 0, 1 and 8 groups and every refusal at its boundary; with -DSEQGROUP_MAIN the
// file is a program that runs it, for a stand-alone build under -fsanitize=address,undefined.
#include "../synthesizer_amd/csrc/seqgroup.hpp"
#include <stdio.h>
#include <string.h>
#include <limits>
#include <vector>

namespace {

uint32_t scan(const std::vector<shg::Group>& g, uint32_t t) {
    for (uint32_t i = 0; i < g.size(); ++i)
        if (t >= g[i].first && t < g[i].end) return i;
    return shg::NONE;
}

int packed_right(const std::vector<shg::Group>& g, uint32_t ntracks) {
    shg::Table T;
    memset(&T, 0x5A, sizeof T);
    shg::pack(g.data(), (uint32_t)g.size(), ntracks, T);
    int bad = T.n != g.size() || T.row0 != ntracks + 1;
    for (uint32_t t = 0; t < shg::MAX_TRACKS; ++t) bad += shg::group_of(T, t) != scan(g, t);
    for (uint32_t i = 0; i < shg::MAX_GROUPS; ++i) {
        const bool in = i < g.size();
        bad += T.gain[i] != (in ? g[i].gain : 1.0) || T.pan[2 * i] != (in ? g[i].left : 1.0) || T.pan[2 * i + 1] != (in ? g[i].right : 1.0);
    }
    return bad;
}

int verdict(const std::vector<shg::Group>& g, uint32_t ntracks, int nch, shg::Refusal why, uint32_t entry) {
    const shg::Verdict v = shg::check(g.data(), (uint32_t)g.size(), ntracks, nch);
    return v.why != why || (why != shg::OK && v.entry != entry);
}

}  // namespace

extern "C" {

// 0 (the list passes) or the refusal's number; *entry: the entry at fault.  rows: n x (first, end, gain, left, right) as doubles.
int sg_check(const double* rows, uint32_t n, uint32_t ntracks, int nchannels, uint32_t* entry) {
    std::vector<shg::Group> g(n);
    for (uint32_t i = 0; i < n; ++i) g[i] = shg::Group{(uint32_t)rows[5 * i], (uint32_t)rows[5 * i + 1], rows[5 * i + 2], rows[5 * i + 3], rows[5 * i + 4]};
    const shg::Verdict v = shg::check(n ? g.data() : nullptr, n, ntracks, nchannels);
    *entry = v.entry;
    return (int)v.why;
}

// the table of a checked list: of[32] the group of every track (255: none), gains[8], pans[16]; returns row0
uint32_t sg_pack(const double* rows, uint32_t n, uint32_t ntracks, unsigned char* of, double* gains, double* pans, uint32_t* count) {
    std::vector<shg::Group> g(n);
    for (uint32_t i = 0; i < n; ++i) g[i] = shg::Group{(uint32_t)rows[5 * i], (uint32_t)rows[5 * i + 1], rows[5 * i + 2], rows[5 * i + 3], rows[5 * i + 4]};
    shg::Table T;
    shg::pack(g.data(), n, ntracks, T);
    for (uint32_t t = 0; t < shg::MAX_TRACKS; ++t) of[t] = (unsigned char)shg::group_of(T, t);
    memcpy(gains, T.gain, sizeof T.gain);
    memcpy(pans, T.pan, sizeof T.pan);
    *count = T.n;
    return T.row0;
}

unsigned sg_table_bytes() { return (unsigned)sizeof(shg::Table); }

// the number of mismatches
int sg_selfcheck() {
    using shg::Group;
    int bad = 0;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // packing: 0, 1 and 8 groups; a group over all 32 tracks; groups that touch; groups across the words of the table
    bad += packed_right({}, 6);
    bad += packed_right({Group{2, 5, 0.5, 1.0, 1.0}}, 6);
    bad += packed_right({Group{0, 32, -1.5, 0.25, 2.0}}, 32);
    bad += packed_right({Group{3, 4, 0.0, 0.0, 0.0}, Group{4, 9, 2.0, 1.0, 0.5}}, 9);
    std::vector<Group> eight;
    for (uint32_t i = 0; i < 8; ++i) eight.push_back(Group{4 * i, 4 * i + 4, 0.5 + 0.1 * i, 1.0 - 0.1 * i, 0.3 + 0.05 * i});
    bad += packed_right(eight, 32);
    std::vector<Group> odd;
    for (uint32_t i = 0; i < 8; ++i) odd.push_back(Group{3 * i + 1, 3 * i + 3, 1.0 + i, 1.0, 1.0});      // one loose track between any two
    bad += packed_right(odd, 25);
    // every refusal at its boundary
    bad += verdict({}, 6, 2, shg::COUNT, 0);
    bad += verdict(std::vector<Group>(9, Group{0, 1, 1.0, 1.0, 1.0}), 6, 2, shg::COUNT, 0);
    bad += verdict(eight, 32, 2, shg::OK, 0);
    bad += verdict({Group{0, 6, 1.0, 1.0, 1.0}}, 6, 2, shg::OK, 0);                                     // end == ntracks
    bad += verdict({Group{0, 7, 1.0, 1.0, 1.0}}, 6, 2, shg::RANGE_BEYOND, 0);                           // end == ntracks + 1
    bad += verdict({Group{0, 2, 1.0, 1.0, 1.0}, Group{5, 7, 1.0, 1.0, 1.0}}, 6, 2, shg::RANGE_BEYOND, 1);
    bad += verdict({Group{3, 3, 1.0, 1.0, 1.0}}, 6, 2, shg::RANGE_EMPTY, 0);
    bad += verdict({Group{4, 3, 1.0, 1.0, 1.0}}, 6, 2, shg::RANGE_EMPTY, 0);
    bad += verdict({Group{0, 3, 1.0, 1.0, 1.0}, Group{3, 6, 1.0, 1.0, 1.0}}, 6, 2, shg::OK, 0);        // touching
    bad += verdict({Group{0, 3, 1.0, 1.0, 1.0}, Group{2, 6, 1.0, 1.0, 1.0}}, 6, 2, shg::RANGE_ORDER, 1);     // overlapping by one
    bad += verdict({Group{3, 6, 1.0, 1.0, 1.0}, Group{0, 3, 1.0, 1.0, 1.0}}, 6, 2, shg::RANGE_ORDER, 1);
    bad += verdict({Group{0, 3, nan, 1.0, 1.0}}, 6, 2, shg::GAIN_NOT_FINITE, 0);
    bad += verdict({Group{0, 3, 1.0, 1.0, 1.0}, Group{3, 4, -inf, 1.0, 1.0}}, 6, 2, shg::GAIN_NOT_FINITE, 1);
    bad += verdict({Group{0, 3, 1.0, inf, 1.0}}, 6, 2, shg::PAN_NOT_FINITE, 0);
    bad += verdict({Group{0, 3, 1.0, 1.0, nan}}, 6, 1, shg::PAN_NOT_FINITE, 0);
    bad += verdict({Group{0, 3, 2.0, 1.0, 1.0}}, 6, 1, shg::OK, 0);
    bad += verdict({Group{0, 3, 2.0, 1.0, 0.5}}, 6, 1, shg::PAN_NOT_STEREO, 0);
    bad += verdict({Group{0, 3, 2.0, 1.0, 0.5}}, 6, 2, shg::OK, 0);
    bad += verdict({Group{0, 33, 1.0, 1.0, 1.0}}, 40, 2, shg::RANGE_BEYOND, 0);                         // never past the table
    return bad;
}

}

#ifdef SEQGROUP_MAIN
int main() {
    const int bad = sg_selfcheck();
    printf("cpu_seqgroup: %d mismatches\n", bad);
    return bad ? 1 : 0;
}
#endif
