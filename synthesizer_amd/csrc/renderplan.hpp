// renderplan.hpp -- which shape a bank render's launch takes: the static facts of a bank the choice reads (Facts, on top of
// genplan.hpp's BankFacts), the constants the choice shares with the kernels, shape(): kernel variant, frames per lane, voice groups,
// split or combined, tile-classified / segmented / plain, as a pure function of (facts, call, knobs) -- the grids of every kernel the
// three launch functions of osc_render.hip enqueue, and the decisions of the two-stream run that touch no HIP object.
// Plain C++17, no HIP include (tests/cpu_renderplan.cpp builds it with g++).  A plan is a POD on the caller's stack: nothing here
// allocates -- it runs on every render call, and the blocks of a small bank are host-bound.
#pragma once
#include "genplan.hpp"

namespace shosc {
// ---- what the plan shares with the kernels (osc_device.hpp, osc_render_kernels.hpp take them from here) -------------------------------
enum { COMBINED_DIRECT = 0, COMBINED_LEAN_HARM = 1, COMBINED_LEAN_ALL = 2 };     // k_render_combined<.., MODE>: which lean kinds the bank can hold
enum { LEAN_K_HARM = 0, LEAN_K_ALL = 1, LEAN_K_FM = 2, LEAN_K_REST = 3 };     // which kinds of lean record a bank can hold (static); _REST: a run of a list
constexpr uint32_t TILE_FRAMES = 512;         // = the lean render kernel's tile (four waves, eight frames per lane)
constexpr uint32_t TILE_REC_BYTES = 128;      // sizeof(TileRec) (osc_device.hpp asserts it)
constexpr uint32_t GEN_SPLIT = 2;      // general workgroups per tile of a tile-classified launch (each writes a plane of general parts; <= groups)
#ifndef SH_TPW
#define SH_TPW 3
#endif
constexpr uint32_t TILES_PER_WAVE = SH_TPW;   // tiles a wavefront of the tile-set prepare classifies in a row (prepare_tiles)
constexpr uint32_t SELF_TILES = 16384;        // arrival counters of a self-folding launch: one per tile (sh_bank::d_self)
constexpr int      NSETS = 4;                 // launch-record sets of a bank (sh_bank::NSETS)
}  // namespace shosc

namespace shr {
using namespace shosc;
using shg::div_up;

// What shape choice may depend on besides BankFacts, filled once by sh_bank_create (sh_bank derives from it).
struct Facts : shg::BankFacts {
    uint32_t    lean_fmsine_candidates = 0;   // the lean candidates that are FM Sine voices (all of the lean candidates: the FM-only lean kernel)
    bool        has_onsets = false;        // some voice starts late (sh_voice::start_frame)
    bool        own_envelopes = false;     // the voices' envelope corners are too many to cut launches at (more than 16 distinct ones)
    // (nearly: nine in ten) every voice can be a lean pair of a tile-classified launch: polynomial Harmonics or a plain Sine / Sawtooth / Square /
    // Triangle / Pulse, no FM, no bias, not mirrored; tile_waveforms: some of them are no Harmonics / Sine (the tiles kernel with the
    // waveform branch)
    bool        tile_all = false, tile_waveforms = false;
    long long   first_row_voice = -1;  // the first voice that reads a modulation / sample row (SH_FM_BUFFER, SH_BUFFER); -1: none
    std::vector<uint64_t> chunk_span;      // [chunk][2]: first onset, last frame of sound + 1 of the chunk's voices (host copy of d_chunk_span)
};
// (reads_rows: sh_bank::needs_rows -- sh_bank_set_rows changes it after creation, so it is a fact of the call, as in genplan.hpp)
struct Call { uint64_t start; uint32_t nframes; bool reads_rows; };
// The measurement knobs the plan reads (sh::Knobs lives behind HIP includes)
struct Knobs {
    int  variant = 0, groups = 0, self = 0;
    bool no_split = false, no_seg = false, no_tiles = false, no_speculation = false, no_overlap = false, no_small_pipeline = false, no_ladder = false;
};

enum Kind { PLAIN, SEGMENTED, TILED };
struct Shape {
    int      mode, var;           // mode: COMBINED_* (which lean kinds the bank can hold); var: waves * 100 + frames per lane * 10 + min waves per SIMD
    int      W, F;                // waves per workgroup, frames per lane
    bool     tile_candidate;
    uint32_t tiles, groups, vpg, nchunks;      // tiles of 64 F frames, voice groups of vpg voices, chunks of 64 voices
    bool     split;               // a lean and a general kernel (k_render_lean + k_render_general), not the combined one
    Kind     kind;
    uint32_t c_lo, c_hi;          // TILED: the chunks that can sound in the block, [c_lo, c_hi)
    uint32_t nseg;                // SEGMENTED: segments, at the launch-relative frames seg_first[0 .. nseg]
    uint32_t seg_first[SEG_MAX + 1];
    bool     with_general;        // the general-lists kernel behind the lean one
    int      lean_kind, lean_var; // split, not TILED: LEAN_K_* and the shape of the lean kernel (a segmented launch: 484 whatever var says)
    bool     combined;            // the combined kernel (PLAIN and not split)
    size_t   parts_bytes;         // what a ring slot of partial buses has to hold (0: one voice group, the kernel writes the caller's buses)
    // the run: a single-group launch writes the caller's buffers itself (direct); may_pipeline: two streams; pipelined: the launch can
    // be part of a run (the executor drops that when a direct launch would write where its predecessor wrote)
    bool     direct, may_pipeline, pipelined;
};

// A table of notes: a bank whose notes do not move in lock-step (onsets, envelope corners of their own), nearly all of them
// voices the tiles kernel can take, not rendered from rows.  Such a bank is a candidate for tile-classified launches, and is
// rendered in launches of at most 2^17 frames (max_launch_frames).
inline bool table_of_notes(const Facts& F, bool reads_rows, const Knobs& K) {
    return F.tile_all && F.nvoices >= 128 && (F.has_onsets || F.own_envelopes) && !reads_rows && F.first_row_voice < 0 && !K.no_tiles;
}
// Renders of any length: the launch's x dimension is a tile count (tiles x threads per workgroup must stay below 2^32 work-items,
// which the shapes of small banks reach first: sixteen waves on 128 frames), and a bank with several voice groups keeps
// 32 bytes of partial buses per frame and group.  Long renders are therefore a run of launches of at most this many frames (87 s
// at 48 kHz; consecutive blocks of one shape: the two-stream pipeline applies) into views of the caller's buffers.
// A table of notes (tile-classified launches) is rendered in launches of at most 2^17 frames: a tile set holds a record per
// (tile, sounding voice), and a launch of minutes of audio would not get one (it would fall back to the general code for
// every voice of the table); everything else in launches of at most 2^22 (the 32-bit work-item count of a dispatch).
inline uint32_t max_launch_frames(bool notes) { return notes ? (1u << 17) : (1u << 22); }

// The chunks that can sound in [s0, s0 + nframes): [lo, hi) -- hi = 0: none (lo = the chunk count then)
struct ChunkRange { uint32_t lo, hi; };
inline ChunkRange sounding_chunks(const Facts& F, uint64_t s0, uint32_t nframes) {
    const uint32_t nchunks = div_up(F.nvoices, 64);
    ChunkRange r{nchunks, 0};
    const uint64_t s1 = s0 + (uint64_t)nframes;
    for (uint32_t c = 0; c < nchunks; ++c)
        if (!(s1 <= F.chunk_span[2 * c] || s0 >= F.chunk_span[2 * c + 1])) { r.lo = c < r.lo ? c : r.lo; r.hi = c + 1; }
    return r;
}

inline Shape shape(const Facts& B, const Call& c, const Knobs& K) {
    Shape S{};
    const uint64_t start = c.start;
    const uint32_t nframes = c.nframes;
    // (asked only where the parent's launch code asked: behind the cheaper conditions, so a small bank's call never walks to it)
    int quiet_known = -1;
    auto quiet = [&] { if (quiet_known < 0) quiet_known = B.no_general_voice(start, nframes) ? 1 : 0; return quiet_known == 1; };
    // variant = WAVES*100 + FPL*10 + MINW (SYNTHHIP_VARIANT overrides the tuned default)
    int var = K.variant;
    const int mode = B.lean_candidates == 0 ? COMBINED_DIRECT : (B.lean_fm_candidates ? COMBINED_LEAN_ALL : COMBINED_LEAN_HARM);
    // Shapes <waves, frames per lane, min waves per SIMD>: 484 / 444 banks of >= 128 mostly lean voices (long / short
    // blocks), 844 other large banks, 821 / 421 / 211 small ones (64 .. 127, 8 .. 63, < 8 voices).
    // mostly-lean banks take eight frames per lane on long blocks: the recurrences make every frame after the second cost one or
    // two FMAs of trigonometry (one table lookup per eight frames)
    if (var == 0) var = B.nvoices >= 128 ? (2 * B.lean_candidates >= B.nvoices ? (nframes >= 16384 ? 484 : 444) : 844)
                                         : (B.nvoices >= 64 ? 821 : (B.nvoices >= 8 ? 421 : 211));
    // a LONG launch of a small, mostly lean bank (a run of blocks in one launch: sh_bank_render_run; a whole piece rendered at once) is
    // throughput work, not a latency problem: 64 voices x 480 000 frames at two frames per lane are 3750 workgroups of eight waves that
    // each pay a table lookup per two frames -- at eight frames per lane the recurrences carry six of them (46.7 -> us per run of ten
    // one-second blocks of BASELINE config 2)
    if (K.variant == 0 && B.nvoices < 128 && B.nvoices >= 16 && nframes >= (1u << 18) && 2 * B.lean_candidates >= B.nvoices) var = 484;
    // A bank whose notes do not move in lock-step takes the tile-classified launch (below) at EVERY block length: in real-time
    // chunks (256 .. 4096 frames) the general code walked the whole table for every tile -- a table of 22 528 notes, ~780 of them
    // sounding: 60 .. 85 us per chunk where the arithmetic is 2 us.  The lean tiles kernel has one shape (four waves, 512-frame
    // tiles); a short launch is a few tiles of it, with more voice groups (but not hundreds: their partial buses are folded
    // frame by frame).
    const bool tile_candidate = K.variant == 0 && table_of_notes(B, c.reads_rows, K) && mode != COMBINED_DIRECT && !quiet();
    if (tile_candidate) var = 484;
    // SIXTEEN frames per lane (var 4163; round 4): what a (wave, voice) pair pays once -- the record's scalar loads, the table lookup,
    // the rotation: ~40 of the ~190 VALU instructions of eight frames -- is paid once per sixteen, ~10 % fewer instructions per
    // voice-sample.  The 32 float64 accumulator pairs do not fit 128 registers beside the loop (at 128 the compiler spills inside the
    // Horner chains: 63 us per block), so the shape runs at THREE waves per SIMD (167 registers): 41.6 instead of 46 us for a launch
    // alone, 35.4-35.7 instead of 35.8-35.9 us in a stream of launches (fewer instructions, but a CU holds three workgroups, not four:
    // less of the neighbouring launch beside it).  TWELVE frames per lane fit 128 registers without a spill in the loop -- 7 % fewer
    // instructions at four waves per SIMD -- and ran 36.5-36.7 us: slower than eight (36.0).  Fewer instructions do not buy time in
    // the stream of launches; the clock the chip holds falls as the pipe fills (2.38 GHz with one wavefront per SIMD, 2.12-2.18 with
    // two launches in flight: profiles/r04_headline_phases.md).  Tiles of 1024 frames need twice the voice groups to fill the chip (47 tiles x 16
    // groups of 64 voices for the headline: the same 752 workgroups), so: polynomial-Harmonics banks and FM Sine banks (the lean kernels
    // of these kinds are the ones instantiated at this shape; config 3: 1.8 % faster than at eight frames, 72 B of scratch), a split
    // launch, and enough 64-voice chunks for the groups.
    const bool fm_only = B.lean_fmsine_candidates == B.lean_candidates;     // every lean candidate an FM Sine voice (BASELINE config 3)
    const bool fm_bank = mode == COMBINED_LEAN_ALL && B.lean_candidates > 0 && fm_only;
    if (K.variant == 0 && var == 484 && (mode == COMBINED_LEAN_HARM || fm_bank) && !tile_candidate && !K.no_split && K.groups == 0) {
        const uint32_t tiles16 = div_up(nframes, 1024u);
        uint32_t g16 = 1;
        while (tiles16 * g16 * 2 <= 1024u && B.nvoices / (g16 * 2) >= 64u) g16 *= 2;         // (whole chunks per group)
        // a LONG launch (a run of blocks in one: sh_bank_render_run) has tiles enough for the chip with ONE voice group -- which would
        // make it a combined-kernel launch at eight frames per lane, general code and all (37.9 us per block where the stream of
        // one-block launches needs 36.4): two groups keep it a split launch of the sixteen-frame lean kernel
        if (g16 == 1 && tiles16 >= 640u && B.nvoices >= 128u) g16 = 2;
        if (g16 >= 2 && tiles16 * g16 >= 640u) var = 4163;
    }
    const int W = var >= 1000 ? var / 1000 : var / 100, F = var >= 1000 ? (var / 10) % 100 : (var / 10) % 10;
    // Voice groups: split the voices when the frame range alone gives too few tiles for 256 CUs -- up to ONE round of
    // resident workgroups (1024 slots of four waves), not beyond: 752 workgroups that all start at once beat 1504 whose
    // second round runs half empty (MI355X, 1024 voices x 48 000 frames: 4 groups of 188 tiles 46.7 us, 8 groups 47.2, 16
    // groups 50.1; eight frames per lane: 8 groups of 94 tiles 36.9, 16 groups 38.9, 4 groups 40.3).  SYNTHHIP_GROUPS overrides.
    const uint32_t tiles = div_up(nframes, 64 * F);
    const uint32_t slots = 4096u / (uint32_t)W;
    uint32_t groups = 1;
    if (W == 4) {
        while (tiles * groups * 2 <= slots && B.nvoices / (groups * 2) >= (uint32_t)(4 * W)) groups *= 2;
    } else {                                                 // the eight-wave shapes of small / non-lean banks: cover the chip several times over
        while (tiles * groups < 1024 && B.nvoices / (groups * 2) >= (uint32_t)(4 * W)) groups *= 2;
    }
    if (tile_candidate && groups > 32) groups = 32;
    if (var == 4163 && K.variant == 0 && groups < 2) groups = 2;      // (the long launch above)
    // ... and the long launch of any other bank of >= 128 voices with lean candidates (mixed kinds; eight frames per lane): two groups, so
    // that it is a split launch -- lean lists in the lean kernel, the general lists beside it -- like its one-block launches
    if (K.variant == 0 && W == 4 && groups == 1 && mode != COMBINED_DIRECT && B.nvoices >= 128 && tiles >= 640 && !tile_candidate) groups = 2;
    if (K.groups > 0) groups = (uint32_t)K.groups;
    uint32_t vpg = (B.nvoices + groups - 1) / groups;
    if (groups > 1) vpg = (vpg + 63) & ~63u;                // groups are made of whole 64-voice chunks (the lists' unit)
    groups = (B.nvoices + vpg - 1) / vpg;                  // no empty trailing groups
    // a bank with lean candidates + several voice groups: the launch is split into a lean and a general kernel
    // (k_render_lean + k_render_general); SYNTHHIP_NO_SPLIT=1 keeps the combined kernel
    // (the shapes of banks of fewer than 64 voices -- 421, 211 -- have no lean kernel: such banks never have two voice groups by
    //  themselves; forced on a larger bank by SYNTHHIP_VARIANT they render through the combined kernel)
    const bool split = mode != COMBINED_DIRECT && groups > 1 && !K.no_split && var != 421 && var != 211;
    S.mode = mode; S.var = var; S.W = W; S.F = F;
    S.tile_candidate = tile_candidate;
    S.tiles = tiles; S.groups = groups; S.vpg = vpg; S.nchunks = div_up(B.nvoices, 64);
    S.split = split;
    // A transition launch (segmented): cut where the envelopes become flat (every voice past its decay) and from there on
    // into segments no longer than their own distance from the note's start -- piece ends of the phase sum lie an octave apart,
    // so such a segment crosses at most one per voice; a cut, too, where the first voice leaves its sustain.  Tile-aligned cuts.
    // A TILE-CLASSIFIED launch: banks whose notes do not move in lock-step -- onsets, envelope corners of their
    // own -- have no corners to cut a launch at, and nearly every voice holds a corner somewhere in a one-second block; but nearly
    // every (voice, 512-frame tile) pair lies on one envelope line and one piece of the phase table.  Those pairs take the lean
    // loop, the others the general code for that tile only (see TileRec).
    S.kind = PLAIN;
    if (split && tile_candidate && var == 484) {
        // (a tile set holds records for the RANGE of chunks that can sound in the block; a block in which more than 2 GB worth of them
        // do -- a million notes at once -- goes through the general code)
        const ChunkRange r = sounding_chunks(B, start, nframes);
        S.c_lo = r.lo; S.c_hi = r.hi;
        const uint64_t range = r.hi > r.lo ? (uint64_t)(r.hi - r.lo) + 2 * groups : 0;
        if ((uint64_t)div_up(nframes, TILE_FRAMES) * range * 64 * TILE_REC_BYTES <= ((uint64_t)1 << 31)) S.kind = TILED;
    }
    // (a 4163 launch that is segmented renders through the 484 lean kernel, with cuts planned at its own tile of 64 F = 1024 frames)
    if (S.kind != TILED && split && (var == 484 || var == 4163) && B.all_lean && !K.no_seg && !c.reads_rows && !quiet()) {
        S.nseg = shg::plan_segments(B, start, nframes, (uint64_t)(64 * F), ~0ull, true, S.seg_first);
        if (S.nseg < 2 || S.seg_first[S.nseg] != nframes) S.nseg = 0;        // nothing to cut, or more cuts than a launch carries
        if (S.nseg) S.kind = SEGMENTED;
    }
    // ... and the general-lists kernel is only launched when the launch CAN hold a general voice
    S.with_general = split && !quiet();
    S.lean_kind = mode == COMBINED_LEAN_HARM ? LEAN_K_HARM : (S.kind == PLAIN && fm_only ? LEAN_K_FM : LEAN_K_ALL);
    S.lean_var = S.kind == SEGMENTED ? 484 : var;
    S.combined = S.kind == PLAIN && !split;
    // partial buses of a split launch: the general kernel's parts follow the lean kernel's, then one flag per group
    S.parts_bytes = groups <= 1 ? 0 : split ? 2 * (size_t)groups * nframes * 16 + (size_t)groups * sizeof(uint32_t) : (size_t)groups * nframes * 16;
    // A RUN: consecutive renders of a bank (same shape, the next block each time) alternate between two HIP streams so that the
    // tail of one launch -- its launch latency, for a small bank: nearly all of it -- is filled by the next; with several voice
    // groups a launch also folds the partial buses of the launch before its predecessor.  A single-group launch writes the
    // caller's buffers itself, so it may only run beside its predecessor when the two do not write the same memory (a ring of
    // bus buffers; a caller that renders every block into ONE buffer stays on one stream, as in round 2).
    S.may_pipeline = !K.no_speculation && !K.no_overlap;
    S.direct = groups == 1;
    S.pipelined = groups > 1 || (S.may_pipeline && !K.no_small_pipeline);
    return S;
}

// ---- the run -------------------------------------------------------------------------------------------------------------------------------
struct RunView { bool active; uint32_t nframes, groups, tile; uint64_t next_start; };     // sh_bank::run_*
// does this launch continue the bank's run: same shape, the next block
inline bool continues_run(const RunView& R, const Shape& S, const Call& c) {
    return S.pipelined && R.active && R.nframes == c.nframes && R.groups == S.groups && R.tile == (uint32_t)(64 * S.F) && R.next_start == c.start;
}
// what each record set holds (or will); sparse: resolved for a tile-classified launch -- the chunks whose voices are all silent in
// the block were skipped (nobody reads them there), so only such a launch may take the set
struct SetSpec { bool valid = false; uint64_t start = 0; uint32_t nframes = 0; bool sparse = false; };
// the records of the block two launches on go to a set that is neither this launch's, nor its predecessor's (perhaps
// still executing), nor the one holding the block in between; -1: none (no speculation)
inline int next_record_set(const SetSpec (&spec)[NSETS], int cur, int prev_cur, int last_target, bool cont, const Call& c, const Knobs& K) {
    if (K.no_speculation) return -1;
    for (int s = 0; s < NSETS; ++s) {
        const bool holds_between = spec[s].valid && spec[s].start == c.start + c.nframes && spec[s].nframes == c.nframes;
        if (s != cur && !(cont && (s == prev_cur || s == last_target)) && !holds_between) return s;
    }
    return -1;
}
// the tile set of a tile-classified launch is resolved for one block and one number of voice groups (sh_bank::tile_spec)
struct TileSetSpec { bool valid = false; uint64_t start = 0; uint32_t nframes = 0, groups = 0; };
inline bool holds(const TileSetSpec& sp, const Call& c, uint32_t groups) { return sp.valid && sp.start == c.start && sp.nframes == c.nframes && sp.groups == groups; }
// A plain split launch whose records nothing has resolved (a render that stands alone, the first of a run, a jump) CAN resolve them in
// the lean kernel itself (LaunchArgs::self_prepare: every workgroup its own voice group's records) and fold its partial buses itself
// (FoldIn::self).  Both are OFF (SYNTHHIP_SELF = 1 both, 2 the fold, 3 the records): round 6 built them for VERDICT r05 item 3 (the
// lone call, 56 -> <= 45 us) and measured 61 us with both, 63 with the fold (planes stored and loaded at agent scope; with fences at
// agent scope instead: 123 us -- every workgroup writes back and invalidates its XCD's L2), 57 with the records (and +7 us per
// launch of two or more blocks: hundreds of workgroups resolving the same sixteen chunks) against 57 for the prepare kernel +
// k_bus_combine: profiles/r06_run_lengths.txt.
inline bool plain_split(const Shape& S, const Knobs& K) { return S.split && S.kind == PLAIN && K.self != 0; }
inline bool may_self_prepare(const Shape& S, const Knobs& K) { return plain_split(S, K) && K.self != 2; }
// A launch that does not continue a run and has nothing to take over folds ITSELF (FoldIn::self): the last workgroup of a tile to
// store its plane folds the tile -- a render that stands alone is complete when its one kernel ends (no k_bus_combine behind it),
// and the first launch of a run owes nobody a fold.  Only where the lean kernel writes every plane (no general-lists kernel behind it).
inline bool self_fold(const Shape& S, const Knobs& K, bool cont, int npending) {
    return plain_split(S, K) && K.self != 3 && S.groups > 1 && !cont && npending == 0 && !S.with_general && S.tiles <= SELF_TILES;
}
// nothing renders beside a launch that does not continue a run (LaunchArgs::alone: its wavefronts' priority ladder)
inline bool stands_alone(bool cont, const Knobs& K) { return !cont && !K.no_ladder; }
// the workgroups that resolve the next-but-one block's records: one wavefront per chunk of 64 voices, in rows of the grid behind the voice groups'
inline uint32_t prepare_workgroups(const Shape& S, int target) { return target >= 0 ? S.nchunks : 0u; }

// ---- grids ---------------------------------------------------------------------------------------------------------------------------------
struct Grid { uint32_t x, y; };
inline Grid behind_groups(const Shape& S, uint32_t tiles, uint32_t behind) { return Grid{tiles, S.groups + div_up(behind, tiles)}; }

// A TILE-CLASSIFIED launch: the lean tiles kernel (which also resolves, in rows behind its voice groups, the tile set -- and the launch
// records that will be needed -- of the block two launches on) and the general pairs' kernel behind it, or the merged kernel for a
// short launch.
struct TiledGrids {
    uint32_t ntiles;              // tiles of TILE_FRAMES
    uint32_t k0, k1;              // this block's sounding chunks as mask slots k (chunk c = group + k groups): [k0, k1)
    uint32_t nk0, nk1;            // ... and those of the block two launches on (has_next)
    uint32_t next_tile_wgs;       // workgroups that resolve that block's tile set
    bool     merged;
    uint32_t behind;              // workgroups in rows behind the voice groups
    bool     next_in_kernel;      // the kernel gets the next record set (NextArgs)
    Grid     tiles, general;      // k_render_tiles; k_render_general<GEN_TILES> (x only; not merged)
};
inline void mask_slots(ChunkRange r, uint32_t groups, uint32_t& k0, uint32_t& k1) {
    k0 = r.hi ? r.lo / groups : 0u;
    k1 = r.hi ? div_up(r.hi, groups) : 0u;
}
inline TiledGrids tiled_grids(const Facts& B, const Shape& S, const Call& c, bool has_next) {
    TiledGrids G{};
    G.ntiles = div_up(c.nframes, TILE_FRAMES);
    mask_slots(ChunkRange{S.c_lo, S.c_hi}, S.groups, G.k0, G.k1);
    if (has_next) {
        mask_slots(sounding_chunks(B, c.start + 2 * (uint64_t)c.nframes, c.nframes), S.groups, G.nk0, G.nk1);
        uint32_t in_range = (G.nk1 - G.nk0) * S.groups;                 // chunks of the range (the last slot's may not all exist)
        if (G.nk1 * S.groups > S.nchunks) in_range -= G.nk1 * S.groups - S.nchunks;
        G.next_tile_wgs = in_range * div_up(div_up(G.ntiles, TILES_PER_WAVE), 4);
    }
    // A short launch (real-time chunks: a handful of tiles) is ONE kernel -- the lean tiles' workgroups and, in rows behind them, the
    // general pairs' and the ones that resolve the next-but-one tile set: the chip has room for all of them at once, the launch is
    // latency-bound, and a second kernel costs the host and the stream more than its work; the general code in the same kernel costs
    // the lean loop registers, which a long launch cannot afford and a short one does not notice.
    // (Measured in round 4: the merged kernel for LONG launches too -- no general kernel between two lean kernels of a stream -- 50.7
    // against 48.4 us per block of the staggered row; with the general workgroups' code behind a function call, so that it would not
    // cost the lean pairs' loop registers, 530 us: the call's stack frame makes every wavefront of the dispatch a scratch user.)
    G.merged = S.tiles <= 16;
    // (merged: general workgroups, then the tile-set prepare workgroups)
    // (where the next-but-one tile set is resolved was moved three times in round 3 -- between the lean workgroups, a kernel of its
    // own on a third stream, the general kernel -- before it ended in rows behind the lean kernel's voice groups: CHANGELOG item 34)
    G.behind = G.merged ? S.tiles * GEN_SPLIT + G.next_tile_wgs : G.next_tile_wgs;
    G.next_in_kernel = has_next && (G.merged || G.behind);
    G.tiles = behind_groups(S, S.tiles, G.behind);
    // the general pairs: GEN_SPLIT workgroups per 256-frame tile, each all voice groups' pairs of it
    G.general = Grid{div_up(c.nframes, 256) * GEN_SPLIT, 1};
    return G;
}

// A transition launch cut into SEGMENTS: one batched prepare, the lean kernel over all segments, the general kernel (the first
// segment's groups split SUB ways) and the combine of its slices.
struct SegmentedGrids {
    uint32_t tiles_lean, tiles_gen;        // tiles of 512 / 256 frames over all segments
    uint32_t SUB, n0;                      // the first segment's n0 frames: its groups are split SUB ways (BankPtrs::gen_sub)
    size_t   scratch_bytes, valid_bytes;   // the slices of the first segment's general parts; the groups' flags
    Grid     lean, general, combine;
};
inline SegmentedGrids segmented_grids(const Shape& S, uint32_t prep_wgs) {
    SegmentedGrids G{};
    for (uint32_t k = 0; k < S.nseg; ++k) {
        G.tiles_lean += div_up(S.seg_first[k + 1] - S.seg_first[k], 64 * 8);
        G.tiles_gen += div_up(S.seg_first[k + 1] - S.seg_first[k], 64 * 4);
    }
    // the first segment's groups are split SUB ways (BankPtrs::gen_sub): with sixteen waves per workgroup a wave walks two
    // or three of the 128 voices of its group
    G.SUB = 4;
    G.n0 = S.seg_first[1];
    G.scratch_bytes = (size_t)S.groups * G.SUB * G.n0 * 16;
    G.valid_bytes = (size_t)S.groups * sizeof(uint32_t);
    G.lean = behind_groups(S, G.tiles_lean, prep_wgs);
    G.general = Grid{G.tiles_gen + (G.SUB - 1) * div_up(G.n0, 64 * 4), S.groups};
    G.combine = Grid{div_up(G.n0, 256), S.groups};
    return G;
}

// A plain launch: the lean kernel of a split launch (+ the general lists' kernel where the launch can hold a general voice), or the
// combined kernel.
struct PlainGrids { Grid render, lists; };
inline PlainGrids plain_grids(const Shape& S, const Call& c, uint32_t prep_wgs) {
    // the general lists of the same launch: four waves x four frames per lane whatever the lean kernel's shape (the parts
    // are indexed by frame), same voice groups, behind the lean kernel on the same stream
    return PlainGrids{behind_groups(S, S.tiles, prep_wgs), Grid{div_up(c.nframes, 256), S.groups}};
}

}  // namespace shr
