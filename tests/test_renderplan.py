"""The bank render's launch plan (synthesizer_amd/csrc/renderplan.hpp) built for the host with g++: shape() against a restatement
written from the header's comments, invariants of the shape and the run decisions over random banks and calls, and the RECORDED SHAPE
TABLE.

The table (tests/golden/renderplan_shapes.txt) was recorded from the launch code of commit ca5472c -- the last one whose
osc_render.hip chose a launch's shape inside the code that launches -- not from the plan: a scratch copy of that commit with one
fprintf after sh_bank_create that dumps the bank's facts, one in bank_render just before the dispatch to launch_tiled /
launch_segmented / launch_plain, and one beside every hipLaunchKernelGGL / launch_render_lean / launch_render_combined / hipMemsetAsync
of those three functions, run once on an MI355X: one process per knob set, one after the other.  The same patch on this
tree's executor, run by the same driver, gives the same bytes.  The notation is terse, for the table's size.  Lines:
    PROCESS name                 a process: one knob set
    K ten numbers                the knobs sh_init read, in the order of KNOB_NAMES
    BANK name                    the driver's label of the bank created next
    F id nvoices=.. ...          what sh_bank_create found (id: the bank's ordinal in its process; lean = candidates, of them not Harmonics,
                                 of them FM Sine; flat = env_flat_from, _until; pieces = short_piece_end, span = chunk_span in run lengths:
                                 a value, or a lo:hi pair, `*k` when it repeats k times; tile = tile_all, tile_waveforms)
    C id start nframes rows | <state> | <decisions>
                                 one bank_render.  <state>: what the executor adds from the bank's run -- STATE_NAMES: the run's fields
                                 (active, nframes, groups, tile, count, next_start) and the folds owed before the call, the record sets
                                 (valid:start:nframes, or 0) at the dispatch, the launch's place in the run after the buffer checks
                                 (pipelined, cont), whether acquire_records found no resolved set, whether a fold was taken over.
                                 <decisions>: the plan's, DECISION_NAMES -- rebuilt here from F, K, the call and <state>, compared as text
    P predicted k0,k1            (a tile-classified launch) whether the tile set had been resolved by the launch two before; its mask slots
                                 (rebuilt too: the ring of four tile sets is followed call by call)
    L kernel ... gxXgy           a launch of the three launch functions, rebuilt and compared as text like the decisions (tiles: the
                                 workgroups behind the voice groups; next = tile-set workgroups, the next set's mask slots, NextArgs given)
Every shape can only be told from another by this table: they all return the same samples."""
import ctypes as C
import random
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
TABLE = ROOT / "tests" / "golden" / "renderplan_shapes.txt"
SEG_MAX = 24
DIRECT, LEAN_HARM, LEAN_ALL = range(3)                   # COMBINED_*
K_HARM, K_ALL, K_FM = range(3)                           # LEAN_K_*
KNOB_NAMES = ["variant", "groups", "self", "no_split", "no_seg", "no_tiles", "no_speculation", "no_overlap", "no_small_pipeline", "no_ladder"]
U64 = 2 ** 64 - 1
STATE_NAMES = ["run", "pend", "cur", "prev_cur", "last_target", "spec", "pipelined", "cont", "unresolved", "taken"]
DECISION_NAMES = ["mode", "var", "W", "F", "tile_candidate", "tiles", "groups", "vpg", "split", "kind", "c", "nseg", "cuts", "with_general", "self_prepare",
                  "self_fold", "cont0", "target", "nchunks", "prep_wgs", "parts_bytes"]


@pytest.fixture(scope="module")
def rp(tmp_path_factory):
    out = tmp_path_factory.mktemp("renderplan") / "librenderplan.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", str(ROOT / "tests" / "cpu_renderplan.cpp"), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    P64, PI, P32 = C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_uint32)
    lib.rp_facts.restype = C.c_void_p
    lib.rp_facts.argtypes = [C.c_uint32] * 4 + [C.c_int] * 2 + [C.c_uint64] * 2 + [P64, P64, C.c_uint32] + [C.c_int] * 4 + [C.c_longlong, P64, C.c_uint32]
    lib.rp_free.argtypes = [C.c_void_p]
    lib.rp_constants.argtypes = [P32]
    lib.rp_table_of_notes.argtypes = [C.c_void_p, C.c_int, PI]
    lib.rp_max_launch_frames.restype = C.c_uint32
    lib.rp_max_launch_frames.argtypes = [C.c_void_p, C.c_int, PI]
    lib.rp_sounding_chunks.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, P32]
    lib.rp_shape.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, PI, C.c_char_p, C.c_size_t]
    lib.rp_call.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, PI, P64, PI, P64, PI, C.c_char_p, C.c_size_t]
    lib.rp_grids.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, PI, C.c_int, C.c_char_p, C.c_size_t]
    lib.rp_holds.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32]
    lib.rp_stands_alone.argtypes = [C.c_int, PI]
    lib.rp_plan_segments.restype = C.c_uint32
    lib.rp_plan_segments.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, P32]
    k = (C.c_uint32 * 7)()
    lib.rp_constants(k)
    assert list(k) == [512, 128, 2, 3, 16384, 4, SEG_MAX]
    return lib


def knob_array(K):
    return (C.c_int * 10)(*[int(K.get(n, 0)) for n in KNOB_NAMES])


class Facts:
    def __init__(self, lib, **kv):
        self.__dict__.update(kv)
        self.lib = lib
        self.nchunks = (self.nvoices + 63) // 64
        assert len(self.chunk_span) == 2 * self.nchunks and len(self.spe) == 34
        self.h = lib.rp_facts(self.nvoices, self.lean, self.lean_fm, self.lean_fmsine, int(self.all_lean), int(self.has_guard), self.flat_from, self.flat_until,
                              (C.c_uint64 * 34)(*self.spe), (C.c_uint64 * max(1, len(self.corners)))(*self.corners), len(self.corners),
                              int(self.tile_all), int(self.tile_waveforms), int(self.has_onsets), int(self.own_envelopes), self.first_row_voice,
                              (C.c_uint64 * len(self.chunk_span))(*self.chunk_span), len(self.chunk_span))

    def __del__(self):
        self.lib.rp_free(self.h)

    def what(self):
        return {k: v for k, v in self.__dict__.items() if k not in ("lib", "h")}

    # -- restatements, from the comments of genplan.hpp and renderplan.hpp ------------------------------------------------------------
    def no_general_voice(self, start, n):
        if not self.all_lean or start < self.flat_from or start + n > self.flat_until:
            return False
        return self.spe[max(0, (n - 1).bit_length())] <= start

    def table_of_notes(self, rows, K):
        """notes that do not move in lock-step, nearly all of them voices the tiles kernel takes, at least 128, no rows"""
        return bool(self.tile_all and self.nvoices >= 128 and (self.has_onsets or self.own_envelopes) and not rows and self.first_row_voice < 0
                    and not K.get("no_tiles"))

    def sounding_chunks(self, start, n):
        on = [c for c in range(self.nchunks) if start + n > self.chunk_span[2 * c] and start < self.chunk_span[2 * c + 1]]
        return (min(on), max(on) + 1) if on else (self.nchunks, 0)

    def shape(self, start, n, rows, K):
        """shape() as its comments tell it"""
        nv, lean = self.nvoices, self.lean
        variant, kgroups = K.get("variant", 0), K.get("groups", 0)
        tuned = variant == 0
        quiet = self.no_general_voice(start, n)
        mode = DIRECT if lean == 0 else (LEAN_ALL if self.lean_fm else LEAN_HARM)
        mostly_lean = 2 * lean >= nv
        if not tuned:
            var = variant
        elif nv >= 128:                                      # 484 / 444: mostly lean banks, long / short blocks; 844: other large banks
            var = (484 if n >= 16384 else 444) if mostly_lean else 844
        else:                                                # small banks: 64 .. 127, 8 .. 63, < 8 voices
            var = 821 if nv >= 64 else 421 if nv >= 8 else 211
        if tuned and 16 <= nv < 128 and n >= 2 ** 18 and mostly_lean:
            var = 484                                        # a long launch of a small, mostly lean bank is throughput work
        candidate = tuned and self.table_of_notes(rows, K) and mode != DIRECT and not quiet
        if candidate:
            var = 484                                        # the tiles kernel has one shape
        fm_only = self.lean_fmsine == lean
        if tuned and var == 484 and (mode == LEAN_HARM or (mode == LEAN_ALL and fm_only)) and not candidate and not K.get("no_split") and kgroups == 0:
            tiles16, g16 = -(-n // 1024), 1                  # sixteen frames per lane: tiles of 1024 frames, groups of whole chunks
            while tiles16 * g16 * 2 <= 1024 and nv // (g16 * 2) >= 64:
                g16 *= 2
            if g16 == 1 and tiles16 >= 640 and nv >= 128:
                g16 = 2                                      # the long launch: two groups keep it split
            if g16 >= 2 and tiles16 * g16 >= 640:
                var = 4163
        W, F = (var // 1000, var // 10 % 100) if var >= 1000 else (var // 100, var // 10 % 10)
        tiles, groups = -(-n // (64 * F)), 1
        if W == 4:                                           # up to ONE round of resident workgroups: 1024 slots of four waves
            while tiles * groups * 2 <= 4096 // W and nv // (groups * 2) >= 4 * W:
                groups *= 2
        else:                                                # the eight-wave shapes: cover the chip several times over
            while tiles * groups < 1024 and nv // (groups * 2) >= 4 * W:
                groups *= 2
        if candidate:
            groups = min(groups, 32)
        if var == 4163 and tuned:
            groups = max(groups, 2)
        if tuned and W == 4 and groups == 1 and mode != DIRECT and nv >= 128 and tiles >= 640 and not candidate:
            groups = 2                                       # the long launch of a bank of mixed kinds
        if kgroups > 0:
            groups = kgroups                                 # SYNTHHIP_GROUPS overrides -- before the groups are rounded to whole chunks
        vpg = -(-nv // groups)
        if groups > 1:
            vpg = -(-vpg // 64) * 64
        groups = -(-nv // vpg)
        split = mode != DIRECT and groups > 1 and not K.get("no_split") and var not in (421, 211)
        kind, c_lo, c_hi, nseg, cuts = "plain", 0, 0, 0, []
        if split and candidate and var == 484:
            c_lo, c_hi = self.sounding_chunks(start, n)
            span = c_hi - c_lo + 2 * groups if c_hi > c_lo else 0
            if -(-n // 512) * span * 64 * 128 <= 2 ** 31:    # at most 2 GB of tile records
                kind = "tiled"
        if kind != "tiled" and split and var in (484, 4163) and self.all_lean and not K.get("no_seg") and not rows and not quiet:
            seg = (C.c_uint32 * (SEG_MAX + 2))()
            ns = self.lib.rp_plan_segments(self.h, start, n, 64 * F, seg)
            if ns >= 2 and seg[ns] == n:                     # fewer than 2 segments, or not reaching nframes: none
                kind, nseg, cuts = "segmented", ns, list(seg[:ns + 1])
        lean_kind = K_HARM if mode == LEAN_HARM else K_FM if kind == "plain" and fm_only else K_ALL
        parts = 0 if groups <= 1 else 2 * groups * n * 16 + 4 * groups if split else groups * n * 16
        may = not K.get("no_speculation") and not K.get("no_overlap")
        return dict(mode=mode, var=var, W=W, F=F, tile_candidate=int(candidate), tiles=tiles, groups=groups, vpg=vpg, nchunks=self.nchunks, split=int(split),
                    kind=kind, c_lo=c_lo, c_hi=c_hi, nseg=nseg, with_general=int(split and not quiet), lean_kind=lean_kind,
                    lean_var=484 if kind == "segmented" else var, combined=int(kind == "plain" and not split), parts_bytes=parts, direct=int(groups == 1),
                    may_pipeline=int(may), pipelined=int(groups > 1 or (may and not K.get("no_small_pipeline"))), cuts=cuts)


    def grids(self, S, start, n, has_next):
        """tiled_grids / segmented_grids / plain_grids as their comments tell them, for a shape S"""
        up = lambda a, b: -(-a // b)
        g, prep = S["groups"], self.nchunks if has_next else 0         # one wavefront per chunk resolves the next-but-one block's records
        behind = lambda tiles, wgs: (tiles, g + up(wgs, tiles))         # rows of workgroups behind the voice groups'
        if S["kind"] == "tiled":
            slots = lambda lo, hi: (lo // g, up(hi, g)) if hi else (0, 0)          # chunk c = group + k groups
            ntiles, (k0, k1), nk0, nk1, wgs = up(n, 512), slots(S["c_lo"], S["c_hi"]), 0, 0, 0
            if has_next:
                nk0, nk1 = slots(*self.sounding_chunks(start + 2 * n, n))
                wgs = (min(nk1 * g, self.nchunks) - nk0 * g) * up(up(ntiles, 3), 4)    # the last slot's chunks may not all exist; 3 tiles a wave, 4 waves
            merged = S["tiles"] <= 16                        # a short launch is ONE kernel: two general workgroups per tile ride behind too
            rows_behind = (2 * S["tiles"] if merged else 0) + wgs
            x, y = behind(S["tiles"], rows_behind)
            return dict(ntiles=ntiles, k0=k0, k1=k1, nk0=nk0, nk1=nk1, next_tile_wgs=wgs, merged=int(merged), behind=rows_behind,
                        next_in_kernel=int(bool(has_next and (merged or rows_behind))), x=x, y=y, general=2 * up(n, 256))
        if S["kind"] == "segmented":
            lens, n0 = [b - a for a, b in zip(S["cuts"], S["cuts"][1:])], S["cuts"][1]
            tiles_lean, tiles_gen = sum(up(x, 512) for x in lens), sum(up(x, 256) for x in lens)
            x, y = behind(tiles_lean, prep)
            return dict(tiles_lean=tiles_lean, tiles_gen=tiles_gen, sub=4, n0=n0, scratch=g * 4 * n0 * 16, valid=4 * g, x=x, y=y,
                        gx=tiles_gen + 3 * up(n0, 256), gy=g, cx=up(n0, 256), cy=g)       # the first segment's groups split four ways
        x, y = behind(S["tiles"], prep)
        return dict(x=x, y=y, lx=up(n, 256), ly=g)


def plan_shape(lib, F, start, n, rows, K):
    buf = C.create_string_buffer(4096)
    assert lib.rp_shape(F.h, start, n, int(rows), knob_array(K), buf, len(buf)) >= 0
    d = dict(x.split("=") for x in buf.value.decode().split())
    cuts = [int(x) for x in d.pop("cuts").split(",") if x != "-"]
    return dict({k: (v if k == "kind" else int(v)) for k, v in d.items()}, cuts=cuts)


def random_facts(lib, rng):
    nv = rng.choice([1, 7, 8, 16, 63, 64, 127, 128, 130, 192, 1024, 5000, 8192])
    kind = rng.random()
    lean = nv if kind < 0.6 else (0 if kind < 0.7 else rng.randrange(1, nv + 1))
    lean_fm = 0 if rng.random() < 0.6 else rng.randrange(1, lean + 1) if lean else 0
    lean_fmsine = lean_fm if rng.random() < 0.5 else rng.randrange(0, lean_fm + 1)
    all_lean = lean == nv
    flat_from = rng.choice([0, 0, 2880, 48000]) if all_lean else 0
    flat_until = rng.choice([U64, 26880, 146880, 14402880]) if all_lean else U64
    spe, top = [0] * 34, rng.choice([0, 0, 5000, 300000, 3000000])
    for k in range(1, 34):
        spe[k] = min(top, 2 ** k) if all_lean else 0
    corners = sorted({flat_from, flat_until, 480, 156480} - {0, U64}) if all_lean and rng.random() < 0.5 else []
    notes = rng.random() < 0.4
    nchunks = (nv + 63) // 64
    span = []
    for c in range(nchunks):
        lo = rng.choice([0, 3000 * c, 48000 * c]) if notes else 0
        span += [lo, rng.choice([U64, lo + 36481, lo + 500000])]
    return Facts(lib, nvoices=nv, lean=lean, lean_fm=lean_fm, lean_fmsine=lean_fmsine, all_lean=all_lean, has_guard=rng.random() < 0.5, flat_from=flat_from,
                 flat_until=flat_until, spe=spe, corners=corners, tile_all=rng.random() < (0.9 if notes else 0.3), tile_waveforms=rng.random() < 0.3,
                 has_onsets=notes and rng.random() < 0.7, own_envelopes=not corners and rng.random() < 0.5,
                 first_row_voice=-1 if rng.random() < 0.9 else rng.randrange(nv), chunk_span=span)


def random_call(rng):
    # (36 481 .. 548 000: ends of the random chunk spans -- a block that starts where a chunk's sound ends does not hold it)
    start = rng.choice([0, 0, 100, 48000, 65536, 480000, 14400000, 36481, 39481, 500000, 548000, rng.randrange(0, 200000)])
    n = rng.choice([1, 256, 4096, 8192, 8704, 16383, 16384, 40960, 40961, 48000, 2 ** 17, 2 ** 17 + 512, 2 ** 18, 327680, 327681, 655360, 2 ** 22,
                    rng.randrange(1, 400000)])
    return start, n, rng.random() < 0.1


def random_knobs(rng):
    K = {}
    r = rng.random()
    if r < 0.25:
        K["variant"] = rng.choice([484, 444, 844, 821, 421, 211])
    elif r < 0.4:
        K["groups"] = rng.choice([1, 2, 3, 8, 64])
    for name in KNOB_NAMES[3:]:
        if rng.random() < 0.1:
            K[name] = 1
    if rng.random() < 0.15:
        K["self"] = rng.choice([1, 2, 3])
    return K


def plain_facts(lib, nv, **kv):
    """nv polynomial-Harmonics voices that sound throughout"""
    base = dict(nvoices=nv, lean=nv, lean_fm=0, lean_fmsine=0, all_lean=True, has_guard=False, flat_from=0, flat_until=U64, spe=[0] * 34, corners=[],
                tile_all=True, tile_waveforms=False, has_onsets=False, own_envelopes=False, first_row_voice=-1, chunk_span=[0, U64] * ((nv + 63) // 64))
    return Facts(lib, **dict(base, **kv))


def edge_cases(lib):
    """sizes at which a bound of the plan turns, that random banks do not reach"""
    # 1138 chunks that all sound, 229 tiles, 4 groups: 229 x (1138 + 2 x 4) x 64 records of 128 bytes are just over 2 GB -- not tile-classified
    yield plain_facts(lib, 72832, has_onsets=True, flat_from=10 ** 9), 100000, 117000, False, {}
    yield plain_facts(lib, 72832 - 4 * 64, has_onsets=True, flat_from=10 ** 9), 100000, 117000, False, {}        # ... and just under
    # 32 768 tiles of 128 frames, two groups, no general voice: more tiles than a self-folding launch has arrival counters for
    yield plain_facts(lib, 1024), 14400000, 2 ** 22, False, {"variant": 821, "groups": 2, "self": 1}
    yield plain_facts(lib, 1024), 14400000, 2 ** 21, False, {"variant": 821, "groups": 2, "self": 1}


def cases(lib, seed, nfacts, ncalls):
    rng = random.Random(seed)
    yield from edge_cases(lib)
    for _ in range(nfacts):
        F = random_facts(lib, rng)
        for _ in range(ncalls):
            start, n, rows = random_call(rng)
            K = random_knobs(rng)
            yield F, start, n, rows, K


def test_shape_follows_its_comments(rp):
    seen = set()
    for F, start, n, rows, K in cases(rp, 11, 400, 10):
        got, want = plan_shape(rp, F, start, n, rows, K), F.shape(start, n, rows, K)
        assert got == want, (F.what(), start, n, rows, K, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
        seen.add((got["kind"], got["var"]))
        lo_hi = (C.c_uint32 * 2)()
        rp.rp_sounding_chunks(F.h, start, n, lo_hi)
        assert tuple(lo_hi) == F.sounding_chunks(start, n)
        notes = F.table_of_notes(rows, K)
        assert bool(rp.rp_table_of_notes(F.h, int(rows), knob_array(K))) == notes
        assert rp.rp_max_launch_frames(F.h, int(rows), knob_array(K)) == (2 ** 17 if notes else 2 ** 22)
    assert {("tiled", 484), ("segmented", 484), ("segmented", 4163), ("plain", 4163), ("plain", 484), ("plain", 444), ("plain", 844), ("plain", 821),
            ("plain", 421), ("plain", 211)} <= seen, seen
    kinds = [plan_shape(rp, *c)["kind"] for c in edge_cases(rp)]
    assert kinds == ["segmented", "tiled", "plain", "plain"], kinds       # (over the cap: cut into segments like any all-lean bank)


def test_the_grids_follow_their_comments(rp):
    rng = random.Random(14)
    buf = C.create_string_buffer(4096)
    trimmed = odd_general = 0
    for F, start, n, rows, K in cases(rp, 14, 400, 10):
        S, has_next = plan_shape(rp, F, start, n, rows, K), rng.random() < 0.7
        assert rp.rp_grids(F.h, start, n, int(rows), knob_array(K), int(has_next), buf, len(buf)) >= 0
        got, want = {k: int(v) for k, v in (x.split("=") for x in buf.value.decode().split())}, F.grids(S, start, n, has_next)
        assert got == want, (F.what(), start, n, rows, K, has_next, S, {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]})
        if S["kind"] == "tiled":
            trimmed += want["nk1"] * S["groups"] > F.nchunks           # a last mask slot with chunks that do not exist
            odd_general += 0 < n % 512 <= 256 and not want["merged"]
    assert trimmed >= 10 and odd_general >= 10, (trimmed, odd_general)        # (both cases occur, more than once or twice)


def test_shape_invariants(rp):
    kinds = {"plain": 0, "segmented": 0, "tiled": 0}
    for F, start, n, rows, K in cases(rp, 12, 400, 10):
        S = plan_shape(rp, F, start, n, rows, K)
        what = (F.what(), start, n, rows, K, S)
        kinds[S["kind"]] += 1
        assert S["groups"] * S["vpg"] >= F.nvoices > (S["groups"] - 1) * S["vpg"], what       # the groups cover the voices, no empty trailing group
        if S["groups"] > 1:
            assert S["vpg"] % 64 == 0, what
        assert S["tiles"] * 64 * S["F"] >= n > (S["tiles"] - 1) * 64 * S["F"], what
        if S["kind"] == "tiled":
            assert S["var"] == 484 and S["tile_candidate"] and S["nseg"] == 0, what
        else:
            assert S["c_lo"] == 0 and S["c_hi"] == 0 or S["tile_candidate"], what
        if S["kind"] == "segmented":
            cuts = S["cuts"]
            assert 2 <= S["nseg"] <= SEG_MAX and len(cuts) == S["nseg"] + 1 and cuts[0] == 0 and cuts[-1] == n, what
            assert all(a < b for a, b in zip(cuts, cuts[1:])), what
            # a cut lies at the first tile's end, at twice the cut before it, or at a corner of the envelopes: a launch that starts
            # with the notes is cut at tiles' ends until the first corner that is none
            T, edges = 64 * S["F"], {F.flat_from, F.flat_until} | set(F.corners)
            for a, b in zip(cuts, cuts[1:-1]):
                assert start + b in edges or start + b == (T if start + a < T else 2 * (start + a)), what
            assert S["lean_var"] == 484 and S["var"] in (484, 4163), what
        else:
            assert S["nseg"] == 0 and not S["cuts"] and S["lean_var"] == S["var"], what
        if S["split"]:
            assert F.lean > 0 and S["groups"] > 1, what
        if S["with_general"]:
            assert S["split"], what
        assert S["combined"] == int(S["kind"] == "plain" and not S["split"]), what            # the launch kinds are exclusive
        assert (S["parts_bytes"] > 0) == (S["groups"] > 1) and S["direct"] == int(S["groups"] == 1), what
    assert min(kinds.values()) > 50, kinds


def test_the_run_decisions_follow_their_comments(rp):
    """continues_run, next_record_set and self_fold over random states of a bank's run"""
    rng = random.Random(13)
    buf = C.create_string_buffer(1 << 16)
    targets = set()
    for F, start, n, rows, K in cases(rp, 13, 100, 10):
        S = plan_shape(rp, F, start, n, rows, K)
        run = [rng.random() < 0.8, rng.choice([n, n, 4096]), rng.choice([S["groups"], S["groups"], 3]), rng.choice([64 * S["F"], 64 * S["F"], 128]),
               rng.choice([start, start, start + n])]
        cur, prev_cur, last_target = rng.randrange(4), rng.randrange(4), rng.randrange(-1, 4)
        spec = [(rng.random() < 0.5, rng.choice([start + n, start + 2 * n]), rng.choice([n, n, 256])) for _ in range(4)]
        cont, pend, unresolved = rng.random() < 0.5, rng.randrange(3), rng.random() < 0.5
        assert rp.rp_call(F.h, start, n, int(rows), knob_array(K), (C.c_uint64 * 5)(*[int(x) for x in run]), (C.c_int * 3)(cur, prev_cur, last_target),
                          (C.c_uint64 * 12)(*[int(y) for x in spec for y in x]), (C.c_int * 5)(pend, 1, int(cont), int(unresolved), -1), buf, len(buf)) >= 0
        d = dict(zip(DECISION_NAMES, buf.value.decode().splitlines()[0].split()))
        what = (F.what(), start, n, rows, K, run, cur, prev_cur, last_target, spec, cont, pend, unresolved, d)
        # the same shape, the next block
        assert int(d["cont0"]) == int(bool(S["pipelined"] and run[0] and run[1] == n and run[2] == S["groups"] and run[3] == 64 * S["F"] and run[4] == start)), what
        # a set that is neither this launch's, nor -- in a run -- its predecessor's or the one that is filling, nor the one holding the block in between
        free = [c for c in range(4) if c != cur and not (cont and c in (prev_cur, last_target)) and not (spec[c][0] and spec[c][1] == start + n and spec[c][2] == n)]
        want = -1 if K.get("no_speculation") or not free else free[0]
        assert int(d["target"]) == want and int(d["prep_wgs"]) == (F.nchunks if want >= 0 else 0), what
        targets.add(want)
        # SYNTHHIP_SELF: 1 both, 2 the fold, 3 the records; a plain split launch only, and a fold only where nothing is owed or continued
        plain_split = S["split"] and S["kind"] == "plain" and K.get("self", 0) != 0
        assert int(d["self_prepare"]) == int(bool(plain_split and K["self"] != 2 and unresolved)), what
        assert int(d["self_fold"]) == int(bool(plain_split and K["self"] != 3 and not cont and pend == 0 and not S["with_general"] and S["tiles"] <= 16384)), what
        assert bool(rp.rp_stands_alone(int(cont), knob_array(K))) == (not cont and not K.get("no_ladder")), what
        # a tile set holds a block when it is valid and was resolved for that start, length and number of groups
        sp = (rng.random() < 0.8, rng.choice([start, start, start + n]), rng.choice([n, n, 512]), rng.choice([S["groups"], S["groups"], 5]))
        assert bool(rp.rp_holds(int(sp[0]), sp[1], sp[2], sp[3], start, n, S["groups"])) == bool(sp[0] and sp[1:] == (start, n, S["groups"])), (what, sp)
    assert targets == {-1, 0, 1, 2, 3}
    # a launch of more tiles than there are arrival counters does not fold itself; one of half the length does
    folds = []
    for F, start, n, rows, K in list(edge_cases(rp))[2:]:
        assert rp.rp_call(F.h, start, n, 0, knob_array(K), (C.c_uint64 * 5)(), (C.c_int * 3)(0, 0, -1), (C.c_uint64 * 12)(), (C.c_int * 5)(0, 1, 0, 1, -1), buf, len(buf)) >= 0
        folds.append(int(dict(zip(DECISION_NAMES, buf.value.decode().splitlines()[0].split()))["self_fold"]))
    assert folds == [0, 1]


def unpack(text, width):
    """run lengths back to a list: `a*k`, `lo:hi*k`"""
    out = []
    for item in ([] if text == "-" else text.split(",")):
        value, _, k = item.partition("*")
        v = [int(x) for x in value.split(":")]
        assert len(v) == width
        out += v * int(k or 1)
    return out


def launch_head(line):
    """an L line without its grid and counts: the kernel and its template arguments"""
    w = line.split()
    return " ".join(w[:next(i for i, x in enumerate(w) if x[0].isdigit())])


def recorded():
    """[(process, knobs, {id: facts kv}, [(call line, [its P / L lines])])]"""
    procs = []
    for line in TABLE.read_text().splitlines():
        w = line.split()
        if not w or w[0] in ("#", "BANK", "END"):
            continue
        if w[0] == "PROCESS":
            procs.append([w[1], {}, {}, []])
        elif w[0] == "K":
            procs[-1][1] = dict(zip(KNOB_NAMES, (int(x) for x in w[1:])))
        elif w[0] == "F":
            procs[-1][2][int(w[1])] = dict(x.split("=") for x in w[2:])
        elif w[0] == "C":
            procs[-1][3].append((line, []))
        else:
            procs[-1][3][-1][1].append(line)
    return procs


def test_the_recorded_shape_table(rp):
    """The plan's decisions and launches, call by call, against what the parent's launch code did: zero differing lines."""
    buf = C.create_string_buffer(1 << 16)
    differing, seen, ncalls, knob_sets, npredicted = [], set(), 0, set(), 0
    for name, K, banks, calls in recorded():
        knob_sets.add(name)
        facts = {}
        for i, kv in banks.items():
            lean, flat, tile = ([int(x) for x in kv[k].split(",")] for k in ("lean", "flat", "tile"))
            facts[i] = Facts(rp, nvoices=int(kv["nvoices"]), lean=lean[0], lean_fm=lean[1], lean_fmsine=lean[2], all_lean=int(kv["all_lean"]),
                             has_guard=int(kv["guard"]), flat_from=flat[0], flat_until=flat[1], spe=unpack(kv["pieces"], 1), corners=unpack(kv["corners"], 1),
                             tile_all=tile[0], tile_waveforms=tile[1], has_onsets=int(kv["onsets"]), own_envelopes=int(kv["own_env"]),
                             first_row_voice=int(kv["row_voice"]), chunk_span=unpack(kv["span"], 2))
        ring = {}                                            # per bank: tile-classified launches so far, what its four tile sets were resolved for
        for line, events in calls:
            head, state, decisions = [x.strip() for x in line.split("|")]
            bank, start, n, rows = (int(x) for x in head.split()[1:])
            s = dict(zip(STATE_NAMES, state.split()))
            spec = [int(y) for x in s["spec"].split(",") for y in (x.split(":") if x != "0" else (0, 0, 0))]
            run = [int(x) for x in s["run"].split(",")]      # active, nframes, groups, tile, count, next_start
            pend = int(s["pend"]) if int(s["cont"]) else 0    # (folds owed before the call: a launch that starts a run has had them folded)
            d = dict(zip(DECISION_NAMES, decisions.split()))
            assert len(d) == len(DECISION_NAMES), line
            predicted = -1
            if d["kind"] == "tiled":
                # launch k reads tile set k % 4 -- resolved ahead if launch k - 2 expected this block -- and has set (k + 2) % 4
                # resolved for the block two launches on when it has a record set for that block
                count, sets = ring.setdefault(bank, [0, [(0, 0, 0, 0)] * 4])
                predicted = rp.rp_holds(*sets[count % 4], start, n, int(d["groups"]))
                sets[count % 4] = (0, 0, 0, 0)
                if int(d["target"]) >= 0:
                    sets[(count + 2) % 4] = (1, start + 2 * n, n, int(d["groups"]))
                ring[bank][0] += 1
            got_n = rp.rp_call(facts[bank].h, start, n, rows, knob_array(K),
                               (C.c_uint64 * 5)(run[0], run[1], run[2], run[3], run[5]), (C.c_int * 3)(int(s["cur"]), int(s["prev_cur"]), int(s["last_target"])),
                               (C.c_uint64 * 12)(*spec), (C.c_int * 5)(pend, int(s["pipelined"]), int(s["cont"]), int(s["unresolved"]), predicted), buf, len(buf))
            assert got_n >= 0, line
            got = buf.value.decode().splitlines()
            want = [decisions] + events
            ncalls += 1
            npredicted += predicted == 1
            seen.add((d["kind"], int(d["var"])))
            seen.update(launch_head(e) for e in events if e.startswith("L "))
            # the executor's part of `cont`: the plan's answer, unless a buffer check said otherwise
            assert int(s["cont"]) <= int(d["cont0"]) and int(s["pipelined"]) >= int(s["cont"]), line
            if got != want:
                differing.append((name, line, [(a, b) for a, b in zip(want + [None] * len(got), got + [None] * len(want)) if a != b][:3]))
    assert not differing, differing[:5]
    assert npredicted >= 10
    assert ncalls >= 400 and len(knob_sets) == 17, (ncalls, sorted(knob_sets))
    assert len(TABLE.read_text().splitlines()) < 2000
    # every kind of launch at every shape it takes, and every instantiation osc_render.hip has of the tiles kernel
    want = {("tiled", 484), ("segmented", 484), ("segmented", 4163), ("plain", 4163), ("plain", 484), ("plain", 444), ("plain", 844), ("plain", 821),
            ("plain", 421), ("plain", 211)}
    want |= {"L tiles<4,8,3,1,1>", "L tiles<4,8,3,0,1>", "L tiles<4,8,3,1,0>", "L tiles<4,8,4,0,0>", "L general<tiles>", "L general<seg>",
             "L general<lists>", "L seg_combine", "L memset"}
    want |= {"L lean var=%d kinds=%d seg=0" % (v, k) for v, k in ((4163, 0), (4163, 2), (484, 0), (484, 1), (444, 0), (444, 1), (444, 2), (844, 0), (821, 0))}
    want |= {"L lean var=484 kinds=0 seg=1", "L combined var=821 mode=1", "L combined var=421 mode=1", "L combined var=211 mode=1", "L combined var=844 mode=0", "L combined var=821 mode=2"}
    assert want <= seen, sorted(str(x) for x in want - seen)
