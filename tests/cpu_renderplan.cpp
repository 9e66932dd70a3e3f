// csrc/renderplan.hpp built for the host behind a few C functions (tests/test_renderplan.py drives them through ctypes).
#include "../synthesizer_amd/csrc/renderplan.hpp"
#include <cstdio>
#include <string>

using namespace shr;

namespace {
int copy_out(const std::string& s, char* buf, size_t cap) {
    if (s.size() + 1 > cap) return -1;
    std::snprintf(buf, cap, "%s", s.c_str());
    return (int)s.size();
}
std::string cuts_text(const Shape& S) {
    std::string s;
    for (uint32_t k = 0; S.nseg && k <= S.nseg; ++k) s += (k ? "," : "") + std::to_string(S.seg_first[k]);
    return S.nseg ? s : "-";
}
const char* kind_name(Kind k) { return k == TILED ? "tiled" : k == SEGMENTED ? "segmented" : "plain"; }
// knobs as the table's KNOBS line lists them: variant groups self no_split no_seg no_tiles no_speculation no_overlap no_small_pipeline no_ladder
Knobs knobs_of(const int* k) {
    Knobs K;
    K.variant = k[0]; K.groups = k[1]; K.self = k[2];
    K.no_split = k[3]; K.no_seg = k[4]; K.no_tiles = k[5]; K.no_speculation = k[6]; K.no_overlap = k[7]; K.no_small_pipeline = k[8]; K.no_ladder = k[9];
    return K;
}
}  // namespace

extern "C" {

void* rp_facts(uint32_t nvoices, uint32_t lean, uint32_t lean_fm, uint32_t lean_fmsine, int all_lean, int has_guard, uint64_t flat_from, uint64_t flat_until,
               const uint64_t* short_piece_end, const uint64_t* corners, uint32_t ncorners, int tile_all, int tile_waveforms, int has_onsets,
               int own_envelopes, long long first_row_voice, const uint64_t* chunk_span, uint32_t nspan) {
    Facts* F = new Facts;
    F->nvoices = nvoices; F->lean_candidates = lean; F->lean_fm_candidates = lean_fm; F->lean_fmsine_candidates = lean_fmsine;
    F->all_lean = all_lean != 0; F->has_guard = has_guard != 0;
    F->env_flat_from = flat_from; F->env_flat_until = flat_until;
    for (int k = 0; k < 34; ++k) F->short_piece_end[k] = short_piece_end[k];
    F->env_corners.assign(corners, corners + ncorners);
    F->tile_all = tile_all != 0; F->tile_waveforms = tile_waveforms != 0; F->has_onsets = has_onsets != 0; F->own_envelopes = own_envelopes != 0;
    F->first_row_voice = first_row_voice;
    F->chunk_span.assign(chunk_span, chunk_span + nspan);
    return F;
}
void rp_free(void* f) { delete (Facts*)f; }
// the constants the plan shares with the kernels: TILE_FRAMES TILE_REC_BYTES GEN_SPLIT TILES_PER_WAVE SELF_TILES NSETS SEG_MAX
void rp_constants(uint32_t* out) {
    const uint32_t v[7] = {TILE_FRAMES, TILE_REC_BYTES, GEN_SPLIT, TILES_PER_WAVE, SELF_TILES, (uint32_t)NSETS, (uint32_t)SEG_MAX};
    for (int k = 0; k < 7; ++k) out[k] = v[k];
}
int rp_table_of_notes(const void* f, int reads_rows, const int* knobs) { return table_of_notes(*(const Facts*)f, reads_rows != 0, knobs_of(knobs)); }
uint32_t rp_max_launch_frames(const void* f, int reads_rows, const int* knobs) {
    return max_launch_frames(table_of_notes(*(const Facts*)f, reads_rows != 0, knobs_of(knobs)));
}
void rp_sounding_chunks(const void* f, uint64_t start, uint32_t nframes, uint32_t* lo_hi) {
    const ChunkRange r = sounding_chunks(*(const Facts*)f, start, nframes);
    lo_hi[0] = r.lo; lo_hi[1] = r.hi;
}

// Every field of shape(), as "name=value" words
int rp_shape(const void* f, uint64_t start, uint32_t nframes, int reads_rows, const int* knobs, char* buf, size_t cap) {
    const Shape S = shape(*(const Facts*)f, Call{start, nframes, reads_rows != 0}, knobs_of(knobs));
    char line[1024];
    std::snprintf(line, sizeof line, "mode=%d var=%d W=%d F=%d tile_candidate=%d tiles=%u groups=%u vpg=%u nchunks=%u split=%d kind=%s c_lo=%u c_hi=%u nseg=%u with_general=%d "
                  "lean_kind=%d lean_var=%d combined=%d parts_bytes=%zu direct=%d may_pipeline=%d pipelined=%d cuts=",
                  S.mode, S.var, S.W, S.F, (int)S.tile_candidate, S.tiles, S.groups, S.vpg, S.nchunks, (int)S.split, kind_name(S.kind), S.c_lo, S.c_hi, S.nseg,
                  (int)S.with_general, S.lean_kind, S.lean_var, (int)S.combined, S.parts_bytes, (int)S.direct, (int)S.may_pipeline, (int)S.pipelined);
    return copy_out(line + cuts_text(S), buf, cap);
}

// The grids of the launch a call takes, as "name=value" words: what tiled_grids / segmented_grids / plain_grids give for its shape
// (has_next: a record set was found for the block two launches on)
int rp_grids(const void* f, uint64_t start, uint32_t nframes, int reads_rows, const int* knobs, int has_next, char* buf, size_t cap) {
    const Facts& B = *(const Facts*)f;
    const Call c{start, nframes, reads_rows != 0};
    const Shape S = shape(B, c, knobs_of(knobs));
    const uint32_t prep_wgs = prepare_workgroups(S, has_next ? 0 : -1);
    char line[1024];
    if (S.kind == TILED) {
        const TiledGrids G = tiled_grids(B, S, c, has_next != 0);
        std::snprintf(line, sizeof line, "ntiles=%u k0=%u k1=%u nk0=%u nk1=%u next_tile_wgs=%u merged=%d behind=%u next_in_kernel=%d x=%u y=%u general=%u", G.ntiles, G.k0, G.k1,
                      G.nk0, G.nk1, G.next_tile_wgs, (int)G.merged, G.behind, (int)G.next_in_kernel, G.tiles.x, G.tiles.y, G.general.x);
    } else if (S.kind == SEGMENTED) {
        const SegmentedGrids G = segmented_grids(S, prep_wgs);
        std::snprintf(line, sizeof line, "tiles_lean=%u tiles_gen=%u sub=%u n0=%u scratch=%zu valid=%zu x=%u y=%u gx=%u gy=%u cx=%u cy=%u", G.tiles_lean, G.tiles_gen, G.SUB, G.n0,
                      G.scratch_bytes, G.valid_bytes, G.lean.x, G.lean.y, G.general.x, G.general.y, G.combine.x, G.combine.y);
    } else {
        const PlainGrids G = plain_grids(S, c, prep_wgs);
        std::snprintf(line, sizeof line, "x=%u y=%u lx=%u ly=%u", G.render.x, G.render.y, G.lists.x, G.lists.y);
    }
    return copy_out(line, buf, cap);
}
// does a tile set resolved for (start, nframes, groups) hold the call's block; does a launch stand alone
int rp_holds(int valid, uint64_t sp_start, uint32_t sp_nframes, uint32_t sp_groups, uint64_t start, uint32_t nframes, uint32_t groups) {
    return holds(TileSetSpec{valid != 0, sp_start, sp_nframes, sp_groups}, Call{start, nframes, false}, groups);
}
int rp_stands_alone(int cont, const int* knobs) { return stands_alone(cont != 0, knobs_of(knobs)); }

// One call in the notation of the recorded table: the decisions of a C line (its third part) and the L lines of its launches.
// What the executor adds from the bank's state comes in as the table's second part gives it:
// run = {active, nframes, groups, tile, next_start}; sets = {cur, prev_cur, last_target}; spec = 4 x {valid, start, nframes};
// state = {npending, pipelined, cont, unresolved, predicted}: the launch's place in the run after the buffer checks, whether
// acquire_records found no resolved set, and (a tile-classified launch; -1: no P line) whether its tile set had been resolved ahead.
int rp_call(const void* f, uint64_t start, uint32_t nframes, int reads_rows, const int* knobs, const uint64_t* run, const int* sets, const uint64_t* spec,
            const int* state, char* buf, size_t cap) {
    const Facts& B = *(const Facts*)f;
    const Knobs K = knobs_of(knobs);
    const Call c{start, nframes, reads_rows != 0};
    const Shape S = shape(B, c, K);
    const RunView R{run[0] != 0, (uint32_t)run[1], (uint32_t)run[2], (uint32_t)run[3], run[4]};
    SetSpec sp[NSETS];
    for (int k = 0; k < NSETS; ++k) { sp[k].valid = spec[3 * k] != 0; sp[k].start = spec[3 * k + 1]; sp[k].nframes = (uint32_t)spec[3 * k + 2]; }
    const int npending = state[0];
    const bool cont = state[2] != 0, unresolved = state[3] != 0;
    const int target = next_record_set(sp, sets[0], sets[1], sets[2], cont, c, K);
    const uint32_t prep_wgs = prepare_workgroups(S, target);
    const bool self_prepare = S.kind == PLAIN && may_self_prepare(S, K) && unresolved;
    char line[2048];
    std::snprintf(line, sizeof line, "%d %d %d %d %d %u %u %u %d %s %u,%u %u %s %d %d %d %d %d %u %u %zu\n",
                  S.mode, S.var, S.W, S.F, (int)S.tile_candidate, S.tiles, S.groups, S.vpg, (int)S.split, kind_name(S.kind), S.c_lo, S.c_hi, S.nseg, cuts_text(S).c_str(),
                  (int)S.with_general, (int)self_prepare, (int)self_fold(S, K, cont, npending), (int)continues_run(R, S, c), target, S.nchunks, prep_wgs, S.parts_bytes);
    std::string s = line;
    if (S.kind == TILED) {
        const TiledGrids G = tiled_grids(B, S, c, target >= 0);
        if (state[4] >= 0) { std::snprintf(line, sizeof line, "P %d %u,%u\n", state[4], G.k0, G.k1); s += line; }
        std::snprintf(line, sizeof line, "L tiles<4,8,%d,%d,%d> %ux%u behind=%u next=%u,%u,%u,%d\n", (G.merged || B.tile_waveforms) ? 3 : 4,
                      (int)B.tile_waveforms, (int)G.merged, G.tiles.x, G.tiles.y, G.behind, G.next_tile_wgs, G.nk0, G.nk1, (int)G.next_in_kernel);
        s += line;
        if (!G.merged) { std::snprintf(line, sizeof line, "L general<tiles> %u\n", G.general.x); s += line; }
    } else if (S.kind == SEGMENTED) {
        const SegmentedGrids G = segmented_grids(S, prep_wgs);
        std::snprintf(line, sizeof line, "L lean var=%d kinds=%d seg=1 %ux%u\nL memset %zu scratch=%zu\nL general<seg> %ux%u\nL seg_combine %ux%u sub=%u n0=%u\n",
                      S.lean_var, S.lean_kind, G.lean.x, G.lean.y, G.valid_bytes, G.scratch_bytes, G.general.x, G.general.y, G.combine.x, G.combine.y, G.SUB, G.n0);
        s += line;
    } else {
        const PlainGrids G = plain_grids(S, c, prep_wgs);
        if (S.combined) std::snprintf(line, sizeof line, "L combined var=%d mode=%d %ux%u\n", S.var, S.mode, G.render.x, G.render.y);
        else std::snprintf(line, sizeof line, "L lean var=%d kinds=%d seg=0 %ux%u\n", S.lean_var, S.lean_kind, G.render.x, G.render.y);
        s += line;
        if (S.with_general) { std::snprintf(line, sizeof line, "L general<lists> %ux%u\n", G.lists.x, G.lists.y); s += line; }
    }
    return copy_out(s, buf, cap);
}

uint32_t rp_plan_segments(const void* f, uint64_t start, uint32_t n, uint64_t T, uint32_t* seg_first) {
    return shg::plan_segments(*(const Facts*)f, start, n, T, ~0ull, true, seg_first);
}

}  // extern "C"
