// genplan.hpp -- which kernels, grids and record sets materialise a bank's rows or fold its int16 mixdown: the static facts of a
// bank that the choice may depend on (BankFacts), the two pure functions over them that the render path shares
// (no_general_voice, plan_segments), and plan(): a whole call as a flat list of steps that osc_generate.hip walks.
// Plain C++17, no HIP include (tests/cpu_genplan.cpp builds it with g++): nothing here launches or allocates on the device.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace shosc {
constexpr int SEG_MAX = 24;            // segments of a transition launch
// Unequal segments of a materialised row's head (n = 0: none): entry k holds the frames [first[k], first[k] + len[k]) and reads
// record set set[k] (the lists launch skips the segments the host can prove free of general voices)
struct SegTab { uint32_t n; uint32_t first[SEG_MAX]; uint32_t len[SEG_MAX]; uint32_t set[SEG_MAX]; };
}  // namespace shosc

namespace shg {
using shosc::SEG_MAX;
using shosc::SegTab;

constexpr uint32_t SEG = 65536;        // frames per equal segment / record set (a multiple of the 1024-frame tile)
constexpr uint32_t MIXDOWN_MAX_VOICES = 32768;

// What route choice may depend on, filled once by sh_bank_create (sh_bank derives from it).
struct BankFacts {
    uint32_t    nvoices = 0;
    uint32_t    lean_candidates = 0;      // voices that can take the lean loop in some launch (static properties)
    uint32_t    lean_fm_candidates = 0;   // ... of them other than polynomial Harmonics (FM Sine, plain waveforms)
    bool        all_lean = false;         // every voice is a lean candidate (of any lean kind)
    bool        has_guard = false;        // some voice carries a guard list (sh_voice::guard_count): the int16 kernels with the boundary check
    uint64_t    env_flat_from = 0, env_flat_until = ~0ull;      // last decay end / onset, first sustain end
    std::vector<uint64_t> env_corners;    // the distinct attack / decay / sustain / release ends of the voices, sorted (empty when there are many)
    uint64_t    short_piece_end[34] = {}; // [k]: the largest end of any phase-table piece shorter than 2^k samples
    // When can a launch hold NO general voice (so that a split launch needs no general-lists kernel)?  Conservative, from
    // static properties: every voice is a lean candidate, every envelope is on its sustain piece for the
    // whole launch, and no phase-table piece shorter than the launch ends after its start (a launch then crosses at most one
    // piece end per voice).
    bool        no_general_voice(uint64_t start, uint32_t nframes) const {
        if (!all_lean || start < env_flat_from || start + nframes > env_flat_until) return false;
        int k = 0;
        while ((1ull << k) < (uint64_t)nframes) ++k;
        return short_piece_end[k] <= start;
    }
};

// The cuts of a transition launch / of the head of a materialised row (see RENDER_LEAN_HARM_SEG): with `corners`, the envelope
// corners the voices share (sloped records: a line of any slope is lean, a corner is not) -- without, or when the voices have
// envelopes of their own, the frame from which all of them are flat and the first sustain end -- and, between those, doubling
// positions (at most one piece end of the phase sum per voice in [pos, 2 pos)); no segment longer than max_len.
// seg_first[0 .. n] = launch-relative segment starts; returns n; the segments cover seg_first[n] <= nframes frames (fewer than
// nframes only when SEG_MAX segments do not reach the end).
inline uint32_t plan_segments(const BankFacts& F, uint64_t start, uint32_t nframes, uint64_t T, uint64_t max_len, bool corners, uint32_t* seg_first) {
    const uint64_t end = start + nframes;
    uint64_t cuts[SEG_MAX + 2];
    uint32_t nc = 0;
    uint64_t pos = start;
    cuts[nc++] = pos;
    const uint64_t flat = F.env_flat_from, rel = F.env_flat_until;
    const bool shared = corners && !F.env_corners.empty();
    if (!shared && pos < flat && flat < end && flat - pos <= max_len) { pos = flat; cuts[nc++] = pos; }
    while (pos < end && nc <= SEG_MAX) {
        uint64_t next = pos < T ? T : 2 * pos;
        if (shared) {
            for (uint64_t c : F.env_corners)
                if (c > pos && c < next) { next = c; break; }
        } else if (pos < rel && rel < next) {
            next = rel;
        }
        if (next - pos > max_len) next = pos + max_len;
        if (next >= end || (end - next <= next / 64 && !shared && end - pos <= max_len)) next = end;   // (a very short rest joins the last segment)
        pos = next;
        cuts[nc++] = pos;
    }
    for (uint32_t k = 0; k < nc; ++k) seg_first[k] = (uint32_t)(cuts[k] - start);
    return nc - 1;
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------------
enum Form { ROWS_F32, ROWS_I16, ROWS_F64, MIXDOWN, MIXDOWN_MAPS };
// (reads_rows: sh_bank_generate_rows[_i16] -- sh_bank::launch_rows is set for the one call, so it is a fact of the call, not of the bank)
struct Call { uint64_t start; uint32_t nframes; Form form; bool reads_rows; };

enum Records {
    ONE_SET,        // acquire_records: the bank's ring of sets, resolved for [start, start + n) unless one already is
    EQUAL_SETS,     // nseg sets of SEG frames each, resolved by one launch_prepare_segments
    TABLE_SETS,     // nseg sets for the unequal segments seg_first[0 .. nseg], resolved by one launch_prepare_segments_var
};
enum Kernel { GENERATE, LISTS, LEAN_HARM, COMBINE, COMPOSE };
struct Launch {                    // (filled by the four *_launch functions below, one per kind)
    Kernel   kernel = GENERATE;
    int      fpl = 4;              // k_generate<FPL>, k_generate_lean_harm<LF = fpl, ..>; k_generate_lists: 4
    bool     lean = false, fold = false, guard = true;      // k_generate_lists<4, LEAN, ..>; k_generate_lean_harm<.., FOLD, GUARD>
    uint32_t gx = 1, gy = 1;       // the grid (256 threads a workgroup everywhere)
    uint32_t first = 0, n = 0;     // its frames, relative to the step
    uint32_t set = 0;              // LISTS over equal segments: the segment whose record set it reads
    uint32_t seg_frames = 0;       // LEAN_HARM: frames per record set
    uint32_t split = 1;            // LEAN_HARM: rec_split; LISTS: vsplit; GENERATE: voices_per_group; COMBINE / COMPOSE: planes
    SegTab   tab = {};             // LEAN_HARM / LISTS over a head's unequal segments
};
enum Mix { ROWS, FUSED, TWO_STEP };
// One set of records and the launches that read it.  A stretch of a mixdown is one FUSED step or a run of TWO_STEP steps (the head
// of a row and its rest) that share one temporary: `opens` allocates temp_bytes (planes / int16 rows of stride
// round_up(stretch_n, 64)), `closes` runs the chain over [stretch_first, stretch_first + stretch_n) when the stretch is TWO_STEP.
struct Step {
    uint32_t first = 0, n = 0;     // frames of the call
    Records  records = ONE_SET;
    uint32_t nseg = 1;
    uint32_t seg_first[SEG_MAX + 1] = {};
    Mix      mix = ROWS;
    uint32_t stretch_first = 0, stretch_n = 0;
    size_t   temp_bytes = 0;
    bool     opens = false, closes = false;
    std::vector<Launch> launches;
};
struct Plan {
    bool     refused = false;      // a mixdown of more than MIXDOWN_MAX_VOICES voices (the planes are numbered in 16 bits of grid.y)
    uint32_t fused = 0;            // fused stretches (sh::state().last_mixdown_fused)
    std::vector<Step> steps;
};

inline uint32_t div_up(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }
inline uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }

// The ONE statement of "this bank's lean voices go through k_generate_lean_harm": not when the call reads rows (every voice through
// the general kernel, which reads them), only long rows (four frames per lane: one lookup + three rotations per voice), some lean
// candidate, and all of them polynomial Harmonics.  The rows route asks it of the frames it is about to materialise (the rest behind
// a head, a two-step stretch); the mixdown asks it ONCE, of the whole call -- so the short last stretch of a long call still folds
// (a fused stretch needs no_general_voice besides, which implies all_lean: the `all_lean` the mixdown's copy used to spell out was
// redundant).  That difference came with the fused mixdown (CHANGELOG item 67) and is kept as found.
inline bool lean_bank(const BankFacts& F, bool reads_rows, uint32_t nframes) {
    return !reads_rows && nframes >= 8192 && F.lean_candidates != 0 && F.lean_fm_candidates == 0;
}
// frames per lane of k_generate / k_generate_lists: 4 for long rows, else 2 / 1
inline int frames_per_lane(uint32_t n) { return n >= 8192 ? 4 : (n >= 2048 ? 2 : 1); }
// frames per lane of the lean kernel: sixteen on long rows (1024 x 480 000: 496 us, eight: 508), fewer when that leaves
// the chip short of workgroups (1024 x 48 000 at sixteen: 12 x 16 = 192 workgroups of four 1024-frame tiles)
inline int lean_frames_per_lane(uint32_t n, uint32_t nchunks) {
    int lf = 16;
    while (lf > 4 && (uint64_t)div_up(n, 256 * lf) * nchunks < 512) lf /= 2;
    return lf;
}
// voices per workgroup of k_generate: as many as keeps >= ~4096 blocks in flight (and gridDim.y <= 65535)
inline uint32_t voices_per_group(uint32_t tile_groups, uint32_t nvoices) {
    uint32_t vpg = 1;
    while (vpg < 64 && (uint64_t)tile_groups * ((nvoices + 2 * vpg - 1) / (2 * vpg)) >= 4096) vpg *= 2;
    while ((nvoices + vpg - 1) / vpg > 65535) vpg *= 2;
    return vpg;
}
constexpr uint32_t REC_SPLIT = 2;      // workgroups per chunk of lean records: enough waves for several rounds of the chip's wave slots (1, 4, 8 measured: CHANGELOG item 38)
constexpr uint32_t VSPLIT = 8;         // workgroups the general voices of a chunk are dealt to in the head's lists launch

inline Launch generate_launch(uint32_t n, uint32_t nvoices) {
    Launch l;
    l.kernel = GENERATE; l.n = n;
    l.fpl = frames_per_lane(n);
    l.gx = div_up(n, 256 * l.fpl);
    l.split = voices_per_group(l.gx, nvoices);
    l.gy = (nvoices + l.split - 1) / l.split;
    return l;
}
inline Launch lists_launch(bool lean, uint32_t gx, uint32_t gy, uint32_t first, uint32_t n, uint32_t set, uint32_t vsplit = 1, const SegTab& tab = SegTab{}) {
    Launch l;
    l.kernel = LISTS; l.lean = lean; l.gx = gx; l.gy = gy; l.first = first; l.n = n; l.set = set; l.split = vsplit; l.tab = tab;
    return l;
}
// (guard: the int16 kernels in two forms -- with the boundary guard's check, and, a bank none of whose voices carries a guard list, without)
inline Launch lean_launch(const BankFacts& F, int lf, bool i16, bool fold, uint32_t gx, uint32_t n, uint32_t seg_frames, const SegTab& tab = SegTab{}) {
    Launch l;
    l.kernel = LEAN_HARM; l.fpl = lf; l.fold = fold; l.guard = !i16 || F.has_guard;
    l.gx = gx; l.gy = div_up(F.nvoices, 64) * REC_SPLIT; l.n = n; l.seg_frames = seg_frames; l.split = REC_SPLIT; l.tab = tab;
    return l;
}
inline Launch planes_launch(Kernel k, uint32_t n, uint32_t nplanes) {
    Launch l;
    l.kernel = k; l.fpl = 0; l.gx = div_up(n, 256); l.n = n; l.split = nplanes;
    return l;
}

// `nseg` equal record sets (one: the bank's own) under one lean launch over n frames; FOLD: into planes instead of rows
inline Step lean_step(const BankFacts& F, uint32_t first, uint32_t n, bool i16, bool fold) {
    Step s;
    s.first = first; s.n = n;
    s.nseg = div_up(n, SEG);
    s.records = s.nseg == 1 ? ONE_SET : EQUAL_SETS;
    const int lf = lean_frames_per_lane(n, div_up(F.nvoices, 64));
    s.launches.push_back(lean_launch(F, lf, i16, fold, div_up(n, 256 * lf), n, s.nseg == 1 ? (n + 1023u) / 1024u * 1024u : SEG));
    return s;
}

// Frames [first, end) of the call as rows of float32 / int16 (i16): appended to `steps`.
inline void plan_rows(const BankFacts& F, const Call& c, bool i16, bool no_seg, uint32_t first, uint32_t end, std::vector<Step>& steps) {
    const uint32_t nchunks = div_up(F.nvoices, 64);
    while (first < end) {
        const uint32_t n = end - first;
        const uint64_t start = c.start + first;
        if (!lean_bank(F, c.reads_rows, n)) {
            // every voice through k_generate -- or, long rows of a bank with lean candidates of other kinds: one workgroup column per
            // 64-voice chunk, walking the launch's lists
            Step s;
            s.first = first; s.n = n;
            if (!c.reads_rows && frames_per_lane(n) == 4 && F.lean_candidates != 0) s.launches.push_back(lists_launch(true, div_up(n, 1024), nchunks, 0, n, 0));
            else s.launches.push_back(generate_launch(n, F.nvoices));
            steps.push_back(s);
            return;
        }
        // Rows that start with the notes (attack, decay, a dozen binades of the phase sum in the first 65 536 frames): the head
        // is cut like a transition launch of the render path (plan_segments: where the envelopes are flat, then doubling
        // positions) so that its voices stay lean -- one prepare launch, one lean launch, ONE lists launch over all segments with
        // the general voices of a chunk dealt to eight workgroups; the rest of the row follows as a step of its own.
        if (start < SEG && F.all_lean && !no_seg && !F.no_general_voice(start, min_u32(n, SEG))) {
            const int lf = lean_frames_per_lane(n, nchunks);
            Step s;
            s.nseg = plan_segments(F, start, n, 64 * lf, SEG, false, s.seg_first);
            if (s.nseg >= 2) {
                s.first = first; s.n = s.seg_first[s.nseg];       // (all of the row, or what SEG_MAX cuts reach)
                s.records = TABLE_SETS;
                SegTab tab{}, ltab{};
                uint32_t tiles = 0, list_groups = 0;
                for (uint32_t k = 0; k < s.nseg; ++k) {
                    const uint32_t f = s.seg_first[k], len = s.seg_first[k + 1] - f;
                    tab.first[k] = f; tab.len[k] = len; tab.set[k] = k;
                    tiles += div_up(len, 64 * lf);
                    if (!F.no_general_voice(start + f, len)) {         // (the lists launch: where general or silent voices can be)
                        ltab.first[ltab.n] = f; ltab.len[ltab.n] = len; ltab.set[ltab.n] = k;
                        ++ltab.n;
                        list_groups += div_up(len, 4 * 64 * 4);
                    }
                }
                tab.n = s.nseg;
                s.launches.push_back(lean_launch(F, lf, i16, false, div_up(tiles, 4), s.n, SEG, tab));
                if (ltab.n) s.launches.push_back(lists_launch(false, list_groups, nchunks * VSPLIT, 0, s.n, 0, VSPLIT, ltab));
                first += s.n;
                steps.push_back(s);
                continue;
            }
        }
        // the lean records by the recurrence kernel, then the general and silent lists segment by segment -- unless the segment
        // provably has none.  Rows longer than a segment get one record set per segment, all resolved by ONE prepare launch.
        Step s = lean_step(F, first, n, i16, false);
        for (uint32_t sg = 0; sg < s.nseg; ++sg) {
            const uint32_t f = sg * SEG, len = min_u32(n - f, SEG);
            if (F.no_general_voice(start + f, len)) continue;
            s.launches.push_back(lists_launch(false, div_up(len, 1024), nchunks, f, len, sg));
        }
        steps.push_back(s);
        return;
    }
}

// The whole call.  (nframes = 0: no step.)
inline Plan plan(const BankFacts& F, const Call& c, bool no_seg) {
    Plan p;
    if (c.form == ROWS_F32 || c.form == ROWS_I16) {
        plan_rows(F, c, c.form == ROWS_I16, no_seg, 0, c.nframes, p.steps);
    } else if (c.form == ROWS_F64) {
        if (c.nframes) {               // float64 rows (modulators, the round() quantise variant): every voice through k_generate
            Step s;
            s.n = c.nframes;
            s.launches.push_back(generate_launch(c.nframes, F.nvoices));
            p.steps.push_back(s);
        }
    } else {
        if (F.nvoices > MIXDOWN_MAX_VOICES) { p.refused = true; return p; }
        // Stretches of whole 65 536-frame segments in which every voice takes the lean polynomial-Harmonics loop (its records then hold the
        // bank in voice order, silent voices -- which add nothing to a chain -- left out) are folded where the samples are made; the others
        // (the notes' attack and decay, banks with other kinds of voice, short calls) go through int16 rows and the chain kernel.
        const bool lean = lean_bank(F, c.reads_rows, c.nframes);
        const uint32_t nplanes = div_up(F.nvoices, 64) * REC_SPLIT;
        uint32_t f0 = 0;
        while (f0 < c.nframes) {
            const uint32_t n0 = min_u32(c.nframes - f0, SEG);
            const bool fused = lean && F.no_general_voice(c.start + f0, n0);
            uint32_t f1 = f0 + n0;
            while (f1 < c.nframes) {                              // extend the stretch while the next segment is of the same sort
                const uint32_t n1 = min_u32(c.nframes - f1, SEG);
                if ((lean && F.no_general_voice(c.start + f1, n1)) != fused) break;
                if (!fused && f1 - f0 >= 4 * SEG) break;          // (two-step stretches: a temporary of nvoices x 2 B per frame each)
                if (fused && f1 - f0 >= 16 * SEG) break;          // (fused stretches: planes of 16 B per frame each -- 1024 voices: 0.5 GB per 2^20 frames; the chain is per frame, so cutting changes nothing)
                f1 += n1;
            }
            const uint32_t len = f1 - f0;
            const size_t at = p.steps.size();
            if (fused) {
                Step s = lean_step(F, f0, len, true, true);
                s.launches.push_back(planes_launch(c.form == MIXDOWN_MAPS ? COMPOSE : COMBINE, len, nplanes));
                s.temp_bytes = (size_t)nplanes * len * 8;
                p.steps.push_back(s);
                p.fused += 1;
            } else {
                plan_rows(F, c, true, no_seg, f0, f1, p.steps);
                p.steps[at].temp_bytes = (size_t)F.nvoices * (((size_t)len + 63) & ~(size_t)63) * 2;
            }
            for (size_t k = at; k < p.steps.size(); ++k) {
                p.steps[k].mix = fused ? FUSED : TWO_STEP;
                p.steps[k].stretch_first = f0; p.steps[k].stretch_n = len;
            }
            p.steps[at].opens = true;
            p.steps.back().closes = true;
            f0 = f1;
        }
    }
    return p;
}

}  // namespace shg
