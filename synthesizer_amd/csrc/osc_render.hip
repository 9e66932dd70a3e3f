// osc_render.hip -- fused generate-and-mix of a voice bank into the stereo bus: the host side of a render call (which shape a launch
// takes, the two-stream pipeline, who folds whose partial buses) and the launches.  The kernels: osc_render_kernels.hpp.
#include "osc_host.hpp"
#include "osc_render_kernels.hpp"
#include "renderplan.hpp"
#include <stdlib.h>


namespace {

// Memory that render launches write (directly, or through a fold they owe / carry out) while some bank's run is open.  The two
// render streams are ordered against each other only where a run starts (ev_join) and where one ends (ev_aux): a launch on
// stream2 is NOT behind what the main stream was given after its run began.  So every launch checks what it is about to
// write against this list -- another bank's entry: every run ends first (sh::flush_pending: the order of the two writes must
// be the callers'); an entry of its own bank written on the OTHER stream (single-group launches write the caller's buffers
// themselves): its own run ends first.  The list is emptied whenever the streams are fully joined.
struct WriteRec { const char* lo; const char* hi; const sh_bank* owner; uint8_t streams; };     // streams: bit 0 `stream`, bit 1 stream2
std::vector<WriteRec>& bank_writes() {
    static std::vector<WriteRec> v;
    return v;
}
bool overlaps_writes(const sh_bank* b, bool own, uint8_t streams, const void* p, size_t bytes) {
    if (!p) return false;
    const char* lo = (const char*)p;
    for (const WriteRec& r : bank_writes())
        if ((r.owner == b) == own && (!own || (r.streams & streams)) && lo < r.hi && r.lo < lo + bytes) return true;
    return false;
}
void note_write(const sh_bank* b, const void* p, size_t bytes, uint8_t stream_bit) {
    if (!p) return;
    const char* lo = (const char*)p;
    for (WriteRec& r : bank_writes())
        if (r.owner == b && r.lo == lo) { if (lo + bytes > r.hi) r.hi = lo + bytes; r.streams |= stream_bit; return; }
    bank_writes().push_back(WriteRec{lo, lo + bytes, b, stream_bit});
}

}  // namespace

namespace shosc {

// Fold what one bank still owes (oldest first: a bus used for two blocks ends up holding the later one) on the main stream and
// end its run.  The caller has joined stream2 into the main stream.
int fold_bank(sh_bank* b) {
    sh::State& S = sh::state();
    if (b->run_active) S.open_runs -= 1;
    b->run_active = false;
    b->run_count = 0;
    // (the caller has made the main stream wait for stream2, and this bank's next stream2 launch will wait for the main stream:
    // its own earlier writes are ordered from here on; with no run open anywhere, everybody's are)
    for (WriteRec& r : bank_writes()) if (r.owner == b) r.streams = 0;
    if (S.open_runs == 0) bank_writes().clear();
    const int n = b->npending;
    b->npending = 0;
    S.pending_total -= n;
    for (int k = 0; k < n; ++k) {
        const sh::PendingCombine& pc = b->pending[k];
        hipLaunchKernelGGL(k_bus_combine, sh::grid1d(pc.nframes, 256), dim3(256), 0, S.stream,
                           (const double2*)pc.parts, pc.groups, pc.nframes, (float2*)pc.o32, (double2*)pc.o64,
                           (uint32_t*)pc.o16, pc.scale, (const uint32_t*)pc.gen_valid);
        SH_CHECK_LAUNCH("k_bus_combine");
    }
    return SH_OK;
}

int join_aux() {
    sh::State& S = sh::state();
    if (S.aux_busy) {
        // recorded here, not behind every launch on stream2: an event recorded now stands for everything stream2 has been given
        // so far (0.7 us of host time per block saved for a small bank, whose blocks are host-bound)
        S.aux_busy = false;
        SH_HIP(hipEventRecord(S.ev_aux, S.stream2));
        SH_HIP(hipStreamWaitEvent(S.stream, S.ev_aux, 0));
    }
    return SH_OK;
}

}  // namespace shosc

namespace sh {
int flush_pending() {
    int rc = join_aux();
    if (rc) return rc;
    for (sh_bank* b : live_banks()) {                     // every bank's run ends here: the next one starts on `stream`
        rc = fold_bank(b);
        if (rc) return rc;
    }
    bank_writes().clear();
    return SH_OK;
}

bool fold_owed_into(const void* p, size_t bytes) {
    const char* lo = (const char*)p;
    for (sh_bank* b : live_banks())
        for (int k = 0; k < b->npending; ++k) {
            const PendingCombine& pc = b->pending[k];
            const struct { const void* q; size_t n; } outs[3] = {{pc.o32, (size_t)pc.nframes * 8}, {pc.o64, (size_t)pc.nframes * 16}, {pc.o16, (size_t)pc.nframes * 4}};
            for (const auto& o : outs)
                if (o.q && lo < (const char*)o.q + o.n && (const char*)o.q < lo + bytes) return true;
        }
    return false;
}

// Both render streams wait for each other (events only): whatever either has been given so far precedes whatever either is
// given from here on.  Used when a device block the launches of both streams use changes hands (grow_pooled).
int join_streams() {
    State& S = state();
    int rc = join_aux();
    if (rc) return rc;
    SH_HIP(hipEventRecord(S.ev_sync, S.stream));
    SH_HIP(hipStreamWaitEvent(S.stream2, S.ev_sync, 0));
    return SH_OK;
}

void free_render_buffers() {
    for (sh_bank* b : live_banks()) {
        for (int k = 0; k < 4; ++k) release_pooled(b->parts[k]);
        for (int k = 0; k < 2; ++k) {
            release_pooled(b->seg_block[k]);
            release_pooled(b->seg_scratch[k]);
            b->seg_cap[k] = 0;
        }
        release_pooled(b->gen_block);
        b->gen_segs = 0;
        for (int k = 0; k < sh_bank::NTILESETS; ++k) {
            release_pooled(b->tile_block[k]);
            b->tile_carved[k] = 0;
            b->tile_spec[k].valid = false;
        }
    }
}
}  // namespace sh

// What the launches of one bank render have in common (bank_render works it out, phase by phase; the three shapes of a launch --
// tile-classified, segmented, plain -- enqueue their kernels from it).  Every count and grid comes from the plan (renderplan.hpp).
struct RenderLaunch {
    sh_bank* b;
    hipStream_t st;
    shr::Call call;
    const shr::Shape& S;
    uint64_t next_start;
    uint32_t prep_wgs;
    bool use_aux;
    bool records_deferred;            // (a tile-classified launch without a resolved record set: its classification resolves what it needs)
    bool self_prepare;                // nothing resolved the launch's records: the lean kernel's workgroups do (LaunchArgs::self_prepare)
    bool alone;                       // the launch does not continue a run: nothing renders beside it (LaunchArgs::alone)
    LaunchSet cur, next;
    BusOut out;                       // the caller's buses
    double2* parts;                   // this launch's partial buses (NULL: one voice group, the kernel writes `out` itself)
    FoldIn fold;                      // the fold this launch takes over
    uint32_t* gen_valid;
    LaunchArgs args(const BankPtrs& P, const LaunchSet& set) const {
        return LaunchArgs{P, trig_table(), b->nvoices, S.vpg, set, call.start, call.nframes, self_prepare ? 1u : 0u, alone ? 1u : 0u};
    }
    NextArgs next_args(const LaunchSet& nx, uint32_t wgs) const { return NextArgs{nx, next_start, wgs}; }
};
static dim3 dim(shr::Grid g) { return dim3(g.x, g.y); }

// A TILE-CLASSIFIED launch (shr::tiled_grids).
static int launch_tiled(const RenderLaunch& L) {
    sh_bank* b = L.b;
    hipStream_t st = L.st;
    const shr::Shape& S = L.S;
    const shr::TiledGrids G = shr::tiled_grids(*b, S, L.call, L.next.launch != nullptr);
    int rc = SH_OK;
    const int ks = (int)(b->tile_count % sh_bank::NTILESETS);
    TileSet& T = b->tile_set[ks];
    sh_bank::TileSpec& sp = b->tile_spec[ks];
    BankPtrs P = ptrs(b);
    sh::counters().tiled_launches += 1;
    const bool predicted = shr::holds(sp, L.call, S.groups);
    if (predicted) sh::counters().tiled_predicted += 1;
    if (!predicted) {
        // not predicted (the first launches of a run, a jump): resolve it in front of the render
        rc = grow_tile_set(b->tile_block[ks], T, b->tile_carved[ks], G.ntiles, b->nvoices, S.groups, (G.k1 - G.k0) * S.groups, st);
        if (rc) return rc;
        T.k0 = G.k0; T.k1 = G.k1;
        P.tiles = T;
        const LaunchSet own = launch_set(b, b->cur);
        rc = launch_prepare_tiles(st, P, T, b->nvoices, L.call.start, L.call.nframes, L.records_deferred ? &own : nullptr);
        if (rc) return rc;
    } else if (L.records_deferred) {
        rc = prepare_chunks_now(b, L.call.start, L.call.nframes, st);      // (a predicted tile set without its records: not a state the pipeline produces)
        if (rc) return rc;
    }
    sp.valid = false;
    // the tile set of the block expected two launches on: set (n + 2) % 4 -- read last by launch n - 2, the launch before on
    // this stream -- resolved by workgroups of this launch's lean kernel
    if (L.next.launch) {
        const int k2 = (int)((b->tile_count + 2) % sh_bank::NTILESETS);
        TileSet& T2 = b->tile_set[k2];
        rc = grow_tile_set(b->tile_block[k2], T2, b->tile_carved[k2], G.ntiles, b->nvoices, S.groups, (G.nk1 - G.nk0) * S.groups, st);
        if (rc) return rc;
        T2.k0 = G.nk0; T2.k1 = G.nk1;
        P.next_tiles = T2;
        P.next_ntiles = G.ntiles;
        P.next_tile_wgs = G.next_tile_wgs;
        b->tile_spec[k2] = sh_bank::TileSpec{true, L.next_start, L.call.nframes, S.groups};
    }
    P.tiles = T;
    const LaunchArgs A = L.args(P, L.cur);
    LaunchSet nx = L.next;
    if (!G.next_in_kernel) nx.launch = nullptr;
    const NextArgs N = L.next_args(nx, G.behind);
    // Waves per SIMD the kernels are compiled for (round 4, same-box A/Bs): the merged kernel 3 (168 registers: 116 B of scratch instead of
    // 328; a 4096-frame chunk 10.9 -> 10.6 us; at 2 -- no scratch at all -- 10.8), the long-launch kernel with the waveform branch 3 (a
    // staggered table of FM Sine notes 64.9 -> 63.0 us), the long-launch Harmonics kernel 4 (at 3: 45.5 instead of 41.0 us per block).
    if (G.merged) {
        if (b->tile_waveforms) hipLaunchKernelGGL((k_render_tiles<4, 8, 3, true, true>), dim(G.tiles), dim3(256), 0, st, A, N, L.fold, L.parts, L.gen_valid);
        else hipLaunchKernelGGL((k_render_tiles<4, 8, 3, false, true>), dim(G.tiles), dim3(256), 0, st, A, N, L.fold, L.parts, L.gen_valid);
    } else {
        if (b->tile_waveforms) hipLaunchKernelGGL((k_render_tiles<4, 8, 3, true, false>), dim(G.tiles), dim3(256), 0, st, A, N, L.fold, L.parts, L.gen_valid);
        else hipLaunchKernelGGL((k_render_tiles<4, 8, 4, false, false>), dim(G.tiles), dim3(256), 0, st, A, N, L.fold, L.parts, L.gen_valid);
    }
    SH_CHECK_LAUNCH("k_render_tiles");
    if (!G.merged) {
        // (on a stream of its own beside the lean kernel it was slower, 95 against 75 us per block: five streams share four
        // hardware queues, and a kernel that waits for an event holds up whatever shares its queue)
        hipLaunchKernelGGL((k_render_general<4, 4, 4, GEN_TILES>), dim3(G.general.x), dim3(256), 0, st, A, L.parts, L.gen_valid);
        SH_CHECK_LAUNCH("k_render_general(tiles)");
    }
    b->tile_count += 1;
    return SH_OK;
}

// A transition launch cut into SEGMENTS (shr::segmented_grids).
static int launch_segmented(const RenderLaunch& L) {
    sh_bank* b = L.b;
    hipStream_t st = L.st;
    const shr::Shape& S = L.S;
    const shr::SegmentedGrids G = shr::segmented_grids(S, L.prep_wgs);
    sh::counters().segmented_launches += 1;
    const int ks = L.use_aux ? 1 : 0;
    LaunchSet& g = b->seg_set[ks];
    int rc = grow_segment_sets(b->seg_block[ks], g, b->seg_cap[ks], S.nseg, b->nvoices);
    if (rc) return rc;
    BankPtrs P = ptrs(b);
    P.nseg = S.nseg;
    for (uint32_t k = 0; k <= S.nseg; ++k) P.seg_first[k] = S.seg_first[k];
    rc = launch_prepare_segments_var(st, true, P, g, b->nvoices, S.nseg, L.call.start);
    if (rc) return rc;
    rc = sh::grow_pooled(b->seg_scratch[ks], G.scratch_bytes);
    if (rc) return rc;
    P.gen_sub = G.SUB;
    P.gen_scratch = (double2*)b->seg_scratch[ks].ptr;
    const LaunchArgs A = L.args(P, g);
    const NextArgs N = L.next_args(L.next, L.prep_wgs);
    rc = launch_render_lean(S.lean_var, S.lean_kind, true, dim(G.lean), st, A, N, L.fold, L.parts);
    if (rc) return rc;
    SH_HIP(hipMemsetAsync(L.gen_valid, 1, G.valid_bytes, st));         // every group's general parts are written
    hipLaunchKernelGGL((k_render_general<16, 4, 1, GEN_SEG>), dim(G.general), dim3(1024), 0, st, A, L.parts, L.gen_valid);
    SH_CHECK_LAUNCH("k_render_general(segments)");
    hipLaunchKernelGGL(k_seg_combine, dim(G.combine), dim3(256), 0, st, (const double2*)b->seg_scratch[ks].ptr, G.SUB, G.n0,
                       L.parts + (size_t)S.groups * L.call.nframes, L.call.nframes);
    SH_CHECK_LAUNCH("k_seg_combine");
    return SH_OK;
}

// A plain launch (shr::plain_grids).
static int launch_plain(const RenderLaunch& L) {
    const shr::Shape& S = L.S;
    const shr::PlainGrids G = shr::plain_grids(S, L.call, L.prep_wgs);
    const LaunchArgs A = L.args(ptrs(L.b), L.cur);
    const NextArgs N = L.next_args(L.next, L.prep_wgs);
    // every k_render_lean lives in osc_render_lean.hip, every k_render_combined in osc_render_combined.hip
    const int rc = S.combined ? launch_render_combined(S.var, S.mode, dim(G.render), L.st, A, N, L.fold, L.parts, L.out)
                              : launch_render_lean(S.lean_var, S.lean_kind, false, dim(G.render), L.st, A, N, L.fold, L.parts);
    if (rc) return rc;
    if (S.with_general) {
        hipLaunchKernelGGL((k_render_general<4, 4, 4, GEN_LISTS>), dim(G.lists), dim3(256), 0, L.st, A, L.parts, L.gen_valid);
        SH_CHECK_LAUNCH("k_render_general(lists)");
    }
    return SH_OK;
}

// ---- the phases of bank_render -----------------------------------------------------------------------------------------------------------

// The caller's buses: float32 / float64 / int16 PCM, and the bytes a launch of nframes writes of each (NULL: not asked for)
struct OutBuses {
    void* p[3];
    size_t n[3];
    OutBuses(uint32_t nframes, sh_buf* f32, sh_buf* f64, sh_buf* i16)
        : p{f32 ? f32->ptr : nullptr, f64 ? f64->ptr : nullptr, i16 ? i16->ptr : nullptr}, n{(size_t)nframes * 8, (size_t)nframes * 16, (size_t)nframes * 4} {}
    template <class Fn> bool any(Fn f) const { return (p[0] && f(p[0], n[0])) || (p[1] && f(p[1], n[1])) || (p[2] && f(p[2], n[2])); }
};
static int check_buses(uint32_t nframes, const sh_buf* bus_f32, const sh_buf* bus_f64, const sh_buf* pcm_i16) {
    if (bus_f32 && bus_f32->bytes < (size_t)nframes * 8) return sh::set_error(SH_ERR_INVALID, "sh_bank_render: bus_f32 too small");
    if (bus_f64 && bus_f64->bytes < (size_t)nframes * 16) return sh::set_error(SH_ERR_INVALID, "sh_bank_render: bus_f64 too small");
    if (pcm_i16 && pcm_i16->bytes < (size_t)nframes * 4) return sh::set_error(SH_ERR_INVALID, "sh_bank_render_pcm: PCM buffer too small");
    return SH_OK;
}
static shr::Knobs plan_knobs() {
    const sh::Knobs& K = sh::knobs();
    shr::Knobs k;
    k.variant = K.variant; k.groups = K.groups; k.self = K.self;
    k.no_split = K.no_split; k.no_seg = K.no_seg; k.no_tiles = K.no_tiles; k.no_speculation = K.no_speculation; k.no_overlap = K.no_overlap;
    k.no_small_pipeline = K.no_small_pipeline; k.no_ladder = K.no_ladder;
    return k;
}

// Where a launch goes: whether it continues the bank's run, and on which stream
struct Placement { bool pipelined, cont, use_aux; uint32_t n; hipStream_t st; };
// Place the launch in a run: the flushes and folds that have to come first, the run's start, the stream.
static int place_in_run(sh_bank* b, const shr::Shape& S, const shr::Call& c, const OutBuses& O, Placement& pl) {
    sh::State& St = sh::state();
    int rc = SH_OK;
    bool pipelined = S.pipelined;
    bool cont = shr::continues_run(shr::RunView{b->run_active, b->run_nframes, b->run_groups, b->run_tile, b->run_next_start}, S, c);
    if (S.direct && pipelined) {
        // memory the previous launch of this bank wrote directly: beside it (other stream) this launch must not write there
        if (O.any([&](const void* p, size_t n) { return b->overlaps_last_direct(p, n); })) { pipelined = false; cont = false; }
        // ... and memory an older launch of the run wrote on the OTHER stream (a ring with an odd number of buffers): new run
        else if (cont) {
            const uint8_t other = (b->run_count & 1) ? 1u : 2u;      // this launch goes to stream2 when run_count is odd: the other is `stream`
            if (O.any([&](const void* p, size_t n) { return overlaps_writes(b, true, other, p, n); })) cont = false;
        }
    }
    // an output buffer another bank's launches may still write (a fold it owes, a fold one of its launches is doing right now on
    // the other stream, a direct write): the order of the writes must be the callers' -- end every run
    if (O.any([&](const void* p, size_t n) { return overlaps_writes(b, false, 3, p, n); }) || bank_writes().size() > 256) {
        rc = sh::flush_pending();
        if (rc) return rc;
        cont = false;
    }
    if (!cont) {
        // this bank's own leftovers are folded now; the other banks' runs go on
        if (b->npending || b->run_active) {
            rc = join_aux();
            if (!rc) rc = fold_bank(b);
            if (rc) return rc;
        }
        if (pipelined) {
            b->run_active = true;
            St.open_runs += 1;
            b->run_nframes = c.nframes;
            b->run_groups = S.groups;
            b->run_tile = (uint32_t)(64 * S.F);
            b->run_count = 0;
            SH_HIP(hipEventRecord(St.ev_join, St.stream));    // everything enqueued so far: stream2's first launch of the run waits for it
        }
    }
    pl.pipelined = pipelined;
    pl.cont = cont;
    pl.n = pipelined ? b->run_count : 0;
    pl.use_aux = pipelined && S.may_pipeline && (pl.n & 1);
    pl.st = pl.use_aux ? St.stream2 : St.stream;
    if (pl.use_aux && pl.n == 1) SH_HIP(hipStreamWaitEvent(St.stream2, St.ev_join, 0));
    return SH_OK;
}

// Commit: what the launch leaves behind -- the fold it took over, the fold it owes, the writes on record, the run's counters
static void commit(sh_bank* b, const shr::Shape& S, const shr::Call& c, const OutBuses& O, const Placement& pl, bool take_over, const sh::PendingCombine& prev,
                   bool self_fold, const sh::PendingCombine& owed, int target) {
    sh::State& St = sh::state();
    if (pl.use_aux) St.aux_busy = true;                     // (join_aux records the event the main stream waits for)
    const uint8_t stream_bit = pl.use_aux ? 2u : 1u;
    if (take_over) {                                        // folded by this launch -- which may be running for a while yet: the
        note_write(b, prev.o32, (size_t)prev.nframes * 8, stream_bit);           // buses it folds into stay on record (they are: from
        note_write(b, prev.o64, (size_t)prev.nframes * 16, stream_bit);          // the launch that rendered them; now with this stream)
        note_write(b, prev.o16, (size_t)prev.nframes * 4, stream_bit);
        b->pending[0] = b->pending[1];
        b->npending = 1;
        St.pending_total -= 1;
    }
    const bool writes_itself = S.direct || self_fold;      // the launch writes the caller's buses on its own stream
    if (owed.parts && !self_fold) {                         // this launch's partial buses: folded two launches on, or by the next other API call
        b->pending[b->npending++] = owed;
        St.pending_total += 1;
    }
    if (St.open_runs > 0) {
        // on record while any run is open (this bank's or another's): direct writes with their stream; the buses a pending fold
        // will write from now (another bank must not slip a write in between), the stream follows when a launch takes the fold over
        for (int k = 0; k < 3; ++k) note_write(b, O.p[k], O.n[k], writes_itself ? stream_bit : 0);
    }
    if (pl.pipelined) {
        b->run_count = pl.n + 1;
        b->run_next_start = c.start + c.nframes;
    }
    for (int k = 0; k < 3; ++k)
        b->last_direct[k] = S.direct && O.p[k] ? sh_bank::Range{(const char*)O.p[k], (const char*)O.p[k] + O.n[k]} : sh_bank::Range{nullptr, nullptr};
    b->last_target = target;
    if (target >= 0) b->spec[target] = sh_bank::Spec{true, c.start + 2 * (uint64_t)c.nframes, c.nframes, S.kind == shr::TILED};
}

// the render behind sh_bank_render (float32 / float64 bus) and sh_bank_render_pcm (int16 PCM straight from the fold)
static int bank_render(sh_bank* b, uint64_t start, uint32_t nframes, sh_buf* bus_f32, sh_buf* bus_f64, sh_buf* pcm_i16, double pcm_scale, const shr::Knobs& K) {
    // ---- argument checks
    SH_REQUIRE_INIT_KEEP_PENDING();          // a pending fold of the previous render is taken over by this launch (below)
    const bool no_out = !bus_f32 && !bus_f64 && !pcm_i16;
    if (!b || nframes == 0 || no_out) {
        int rcp = sh::flush_pending();
        if (rcp) return rcp;
    }
    if (!b || no_out) return sh::set_error(SH_ERR_INVALID, "sh_bank_render: NULL argument");
    if (nframes == 0) return SH_OK;
    int rc = check_buses(nframes, bus_f32, bus_f64, pcm_i16);
    if (!rc) rc = bank_check_plain(b, "sh_bank_render");
    if (rc) return rc;
    const OutBuses O(nframes, bus_f32, bus_f64, pcm_i16);
    const BusOut out{(float2*)O.p[0], (double2*)O.p[1], (uint32_t*)O.p[2], pcm_scale};
    // ---- the shape (renderplan.hpp)
    const shr::Call call{start, nframes, b->needs_rows};
    const shr::Shape S = shr::shape(*b, call, K);
    // ---- the launch's place in a run
    Placement pl;
    rc = place_in_run(b, S, call, O, pl);
    if (rc) return rc;
    // ---- records, partial buses, and the fold the launch takes over
    const int prev_cur = b->cur;
    const bool tiled = S.kind == shr::TILED;
    bool records_deferred = false, self_prepare = false;
    if (S.kind != shr::SEGMENTED) {
        rc = acquire_records(b, start, nframes, pl.st, pl.cont, tiled, tiled ? &records_deferred : shr::may_self_prepare(S, K) ? &self_prepare : nullptr);
        if (rc) return rc;
    }
    // partial buses: ring slot n % 4 (last read by the fold in launch n - 2, which is this stream's previous launch)
    double2* parts = nullptr;
    if (S.parts_bytes) {
        sh::Pooled& slot = b->parts[pl.n & 3];
        rc = sh::grow_pooled(slot, S.parts_bytes);
        if (rc) return rc;
        parts = (double2*)slot.ptr;
    }
    uint32_t* gen_valid = S.with_general ? (uint32_t*)(parts + 2 * (size_t)S.groups * nframes) : nullptr;
    // the fold this launch takes over: the older of two outstanding ones (launch n - 2's) -- or its own (shr::self_fold)
    const bool take_over = b->npending == 2;
    const bool self_fold = shr::self_fold(S, K, pl.cont, b->npending);
    const sh::PendingCombine prev = take_over ? b->pending[0] : sh::PendingCombine();
    const FoldIn fold = self_fold ? FoldIn{parts, nullptr, out, b->d_self()}
                                  : FoldIn{(const double2*)prev.parts, (const uint32_t*)prev.gen_valid, BusOut{(float2*)prev.o32, (double2*)prev.o64, (uint32_t*)prev.o16, prev.scale}, nullptr};
    b->last_groups = S.groups;
    b->last_tiled = tiled;
    // the record set of the block two launches on, and the workgroups that resolve it
    const int target = shr::next_record_set(b->spec, b->cur, prev_cur, b->last_target, pl.cont, call, K);
    LaunchSet next = launch_set(b, target < 0 ? 0 : target);
    if (target < 0) next.launch = nullptr;
    // ---- launch
    const RenderLaunch L{b, pl.st, call, S, start + 2 * (uint64_t)nframes, shr::prepare_workgroups(S, target), pl.use_aux, records_deferred, self_prepare,
                         shr::stands_alone(pl.cont, K), launch_set(b, b->cur), next, out, parts, fold, gen_valid};
    rc = tiled ? launch_tiled(L) : S.kind == shr::SEGMENTED ? launch_segmented(L) : launch_plain(L);
    if (rc) return rc;
    // ---- commit
    sh::PendingCombine owed;
    owed.parts = parts; owed.groups = S.groups; owed.nframes = nframes;
    owed.o32 = O.p[0]; owed.o64 = O.p[1]; owed.o16 = O.p[2];
    owed.scale = pcm_scale; owed.gen_valid = gen_valid;
    commit(b, S, call, O, pl, take_over, prev, self_fold, owed, target);
    return SH_OK;
}

// Renders of any length: a run of launches of at most shr::max_launch_frames into views of the caller's buffers.
static int bank_render_any(sh_bank* b, uint64_t start, uint32_t nframes, sh_buf* bus_f32, sh_buf* bus_f64, sh_buf* pcm_i16, double pcm_scale) {
    SH_API_LOCK();     // (recursive) taken BEFORE the bank is looked at -- sh_bank_set_rows on another thread changes needs_rows /
                       // first_row_voice -- and held across the launches of one call: nothing else gets between them
    const shr::Knobs K = plan_knobs();
    const uint32_t RENDER_MAX_FRAMES = shr::max_launch_frames(b && shr::table_of_notes(*b, b->needs_rows, K));
    if (nframes <= RENDER_MAX_FRAMES) return bank_render(b, start, nframes, bus_f32, bus_f64, pcm_i16, pcm_scale, K);
    int rc = check_buses(nframes, bus_f32, bus_f64, pcm_i16);
    if (rc) return rc;
    const double* rows = b ? b->launch_rows : nullptr;
    for (uint64_t off = 0; off < nframes && !rc; off += RENDER_MAX_FRAMES) {
        const uint32_t n = nframes - off < RENDER_MAX_FRAMES ? (uint32_t)(nframes - off) : RENDER_MAX_FRAMES;
        sh_buf v32{nullptr, 0, false, 0}, v64{nullptr, 0, false, 0}, v16{nullptr, 0, false, 0};
        if (bus_f32) { v32.ptr = (char*)bus_f32->ptr + off * 8; v32.bytes = bus_f32->bytes - off * 8; }
        if (bus_f64) { v64.ptr = (char*)bus_f64->ptr + off * 16; v64.bytes = bus_f64->bytes - off * 16; }
        if (pcm_i16) { v16.ptr = (char*)pcm_i16->ptr + off * 4; v16.bytes = pcm_i16->bytes - off * 4; }
        if (rows) b->launch_rows = rows + off;               // launch-relative rows (sh_bank_render_rows)
        rc = bank_render(b, start + off, n, bus_f32 ? &v32 : nullptr, bus_f64 ? &v64 : nullptr, pcm_i16 ? &v16 : nullptr, pcm_scale, K);
    }
    if (rows) b->launch_rows = rows;
    return rc;
}

extern "C" {

int sh_bank_render(sh_bank* b, uint64_t start, uint32_t nframes, sh_buf* bus_f32, sh_buf* bus_f64) {
    return bank_render_any(b, start, nframes, bus_f32, bus_f64, nullptr, 0.0);
}

int sh_bank_render_pcm(sh_bank* b, uint64_t start, uint32_t nframes, double scale, sh_buf* pcm_i16) {
    if (!pcm_i16) return sh::set_error(SH_ERR_INVALID, "sh_bank_render_pcm: NULL PCM buffer");
    return bank_render_any(b, start, nframes, nullptr, nullptr, pcm_i16, scale);
}

int sh_bank_render_run(sh_bank* b, uint64_t start, uint32_t nframes, uint32_t nblocks, sh_buf* const* bus_f32, sh_buf* const* pcm_i16,
                       uint32_t nring, double pcm_scale) {
    if (!b || (!bus_f32 && !pcm_i16) || nring == 0) return sh::set_error(SH_ERR_INVALID, "sh_bank_render_run: NULL argument");
    if (nframes == 0 || nblocks == 0) return SH_OK;
    for (uint32_t k = 0; k < nring && k < nblocks; ++k) {
        if (bus_f32 && (!bus_f32[k] || bus_f32[k]->bytes < (size_t)nframes * 8)) return sh::set_error(SH_ERR_INVALID, "sh_bank_render_run: bus_f32[%u] missing or too small", k);
        if (pcm_i16 && (!pcm_i16[k] || pcm_i16[k]->bytes < (size_t)nframes * 4)) return sh::set_error(SH_ERR_INVALID, "sh_bank_render_run: pcm_i16[%u] missing or too small", k);
    }
    SH_API_LOCK();                                            // one acquisition for the whole run
    // Blocks whose buffers lie back to back in memory (windows of one allocation: the usual shape of a ring) are ONE launch: a
    // launch costs the host 2-4 us whatever it renders, a small bank's block less than that on the device.  At most
    // RUN_MAX_FRAMES per launch, and never across the ring's wrap (slot nring - 1 is followed by slot 0 somewhere else).
    constexpr uint64_t RUN_MAX_FRAMES = 1u << 20;
    int rc = SH_OK;
    uint32_t k = 0;
    while (k < nblocks && !rc) {
        const uint32_t slot = k % nring;
        uint32_t m = 1;
        while (k + m < nblocks && slot + m < nring && (uint64_t)(m + 1) * nframes <= RUN_MAX_FRAMES) {
            const bool adj32 = !bus_f32 || (char*)bus_f32[slot + m]->ptr == (char*)bus_f32[slot]->ptr + (size_t)m * nframes * 8;
            const bool adj16 = !pcm_i16 || (char*)pcm_i16[slot + m]->ptr == (char*)pcm_i16[slot]->ptr + (size_t)m * nframes * 4;
            if (!adj32 || !adj16) break;
            ++m;
        }
        sh_buf v32{nullptr, 0, false, 0}, v16{nullptr, 0, false, 0};
        if (bus_f32) { v32.ptr = bus_f32[slot]->ptr; v32.bytes = (size_t)m * nframes * 8; }
        if (pcm_i16) { v16.ptr = pcm_i16[slot]->ptr; v16.bytes = (size_t)m * nframes * 4; }
        rc = bank_render_any(b, start + (uint64_t)k * nframes, m * nframes, bus_f32 ? &v32 : nullptr, nullptr, pcm_i16 ? &v16 : nullptr, pcm_scale);
        k += m;
    }
    return rc;
}

int sh_bank_render_rows(sh_bank* b, uint64_t start, uint32_t nframes, const sh_buf* rows_f64, size_t row_stride,
                        sh_buf* bus_f32, sh_buf* bus_f64) {
    if (!b || !rows_f64) return sh::set_error(SH_ERR_INVALID, "sh_bank_render_rows: NULL argument");
    SH_API_LOCK();                                           // held across bank_render (recursive): the rows belong to this call
    {
        if (!b->d_fm_row) return sh::set_error(SH_ERR_INVALID, "sh_bank_render_rows: sh_bank_set_rows has not been called");
        if (row_stride < nframes) return sh::set_error(SH_ERR_INVALID, "sh_bank_render_rows: row_stride < nframes");
        if (b->fm_row_max >= 0 && rows_f64->bytes / 8 < (size_t)b->fm_row_max * row_stride + nframes)
            return sh::set_error(SH_ERR_INVALID, "sh_bank_render_rows: rows buffer too small for row %d", b->fm_row_max);
        b->launch_rows = (const double*)rows_f64->ptr;
        b->launch_row_stride = row_stride;
    }
    int rc = bank_render_any(b, start, nframes, bus_f32, bus_f64, nullptr, 0.0);
    b->launch_rows = nullptr;
    b->launch_row_stride = 0;
    return rc;
}

#ifdef SH_DIAG
int sh_debug_diag2(void* host, size_t bytes) {
    if (hipDeviceSynchronize() != hipSuccess) return SH_ERR_HIP;
    const size_t n = bytes < sizeof(g_diag2) ? bytes : sizeof(g_diag2);
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_diag2), n, 0, hipMemcpyDeviceToHost) == hipSuccess ? SH_OK : SH_ERR_HIP;
}
// (diagnostic builds only) the wavefronts' timestamps of the last launches: 4 banks x DIAG_WAVES x DIAG_SLOTS uint64
int sh_debug_diag(void* host, size_t bytes) {
    if (hipDeviceSynchronize() != hipSuccess) return SH_ERR_HIP;
    const size_t n = bytes < sizeof(g_diag) ? bytes : sizeof(g_diag);
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_diag), n, 0, hipMemcpyDeviceToHost) == hipSuccess ? SH_OK : SH_ERR_HIP;
}
#endif

}  // extern "C"
