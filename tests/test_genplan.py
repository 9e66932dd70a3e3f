"""The bank's route plan (synthesizer_amd/csrc/genplan.hpp) built for the host with g++: no_general_voice and plan_segments against
restatements written from their comments, invariants of plan() over random banks and calls, and the RECORDED ROUTE TABLE.

The table (tests/golden/genplan_routes.txt) was recorded from the launch code of commit 8e50923 -- the last one whose
osc_generate.hip chose its routes inside the code that launches -- not from the plan: a scratch copy of that commit with one fprintf
beside every hipLaunchKernelGGL, acquire_records, launch_prepare_segments[_var], temporary and mixdown_fused / mixdown_two_step call
of the host half of osc_generate.hip, and one after sh_bank_create that dumps the bank's facts, run once on an MI355X (four
processes: segmented heads on, SYNTHHIP_NO_SEG=1, one for the 1024-voice bank without guard lists, one for rows of 1.26 - 1.4 M
frames whose head SEG_MAX segments do not carry to the end).  Lines:
    BANK name / FACTS ...        a bank and what sh_bank_create found
    CALL bank form start nframes seg|noseg [rows]
    R one|eq|var ...             record sets: acquire_records(start, n) / nseg equal sets / nseg sets at the cuts listed
    L kernel<template args> grid=.. ..   a launch       T bytes: a temporary       M fused|two start len: a mixdown stretch
    C chain[_parts] ..           the chain kernel over a two-step stretch's rows
(the bank that reads rows fills them through a one-voice modulator bank's sh_bank_generate_f64: those calls are listed as calls
of `rows40.mod`).  Every route can only be told from another by this table: they all return the same samples."""
import ctypes as C
import random
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SEG, SEG_MAX = 65536, 24
FORM = {"f32": 0, "i16": 1, "f64": 2, "mix": 3, "maps": 4}
GENERATE, LISTS, LEAN_HARM, COMBINE, COMPOSE = range(5)
ONE_SET, EQUAL_SETS, TABLE_SETS = range(3)
ROWS, FUSED, TWO_STEP = range(3)


@pytest.fixture(scope="module")
def gp(tmp_path_factory):
    out = tmp_path_factory.mktemp("genplan") / "libgenplan.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", str(ROOT / "tests" / "cpu_genplan.cpp"), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.gp_facts.restype = C.c_void_p
    lib.gp_facts.argtypes = [C.c_uint32] * 3 + [C.c_int] * 2 + [C.c_uint64] * 2 + [C.POINTER(C.c_uint64)] * 2 + [C.c_uint32]
    lib.gp_free.argtypes = [C.c_void_p]
    lib.gp_no_general_voice.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32]
    lib.gp_lean_bank.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
    lib.gp_plan_segments.restype = C.c_uint32
    lib.gp_plan_segments.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint32)]
    for fn in (lib.gp_plan_routes, lib.gp_plan_fields):
        fn.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    assert lib.gp_seg_max() == SEG_MAX
    return lib


class Facts:
    def __init__(self, lib, nvoices, lean, lean_fm, all_lean, has_guard, flat_from, flat_until, spe, corners):
        self.__dict__.update(nvoices=nvoices, lean=lean, lean_fm=lean_fm, all_lean=all_lean, has_guard=has_guard, flat_from=flat_from,
                             flat_until=flat_until, spe=list(spe), corners=list(corners), lib=lib)
        self.h = lib.gp_facts(nvoices, lean, lean_fm, int(all_lean), int(has_guard), flat_from, flat_until, (C.c_uint64 * 34)(*spe),
                              (C.c_uint64 * max(1, len(corners)))(*corners), len(corners))

    def __del__(self):
        self.lib.gp_free(self.h)

    # -- restatements, from the comments of genplan.hpp ---------------------------------------------------------------------------
    def no_general_voice(self, start, n):
        """every voice lean, all envelopes flat over [start, start + n), no piece shorter than the launch ends after its start"""
        if not self.all_lean or start < self.flat_from or start + n > self.flat_until:
            return False
        k = max(0, (n - 1).bit_length())                     # the smallest k with 2^k >= n
        return self.spe[k] <= start

    def lean_bank(self, reads_rows, n):
        return not reads_rows and n >= 8192 and self.lean != 0 and self.lean_fm == 0


def random_facts(lib, rng):
    nv = rng.choice([1, 16, 33, 64, 80, 130, 192, 1024, 5000, 40000])
    kind = rng.random()
    lean = nv if kind < 0.6 else (0 if kind < 0.7 else rng.randrange(1, nv + 1))
    lean_fm = 0 if rng.random() < 0.75 else rng.randrange(1, lean + 1) if lean else 0
    all_lean = lean == nv
    flat_from = rng.choice([0, 0, 2880, 48000]) if all_lean else 0
    flat_until = rng.choice([2 ** 64 - 1, 26880, 146880, 14402880]) if all_lean else 2 ** 64 - 1
    spe, top = [0] * 34, rng.choice([0, 0, 5000, 300000, 3000000])
    for k in range(1, 34):
        spe[k] = min(top, 2 ** k) if all_lean else 0
    corners = sorted({flat_from, flat_until, 480, 156480} - {0, 2 ** 64 - 1}) if all_lean and rng.random() < 0.5 else []
    return Facts(lib, nv, lean, lean_fm, all_lean, rng.random() < 0.7, flat_from, flat_until, spe, corners)


def random_call(rng):
    start = rng.choice([0, 0, 100, 40000, 65000, 65536, 480000, 14400000, rng.randrange(0, 200000)])
    # (beyond 1.3 M frames a head's SEG_MAX segments no longer reach the end of a row: head + rest)
    n = rng.choice([1, 2047, 2048, 8191, 8192, 65536, 65537, 300000, 480000, 17 * SEG + 5, 1_262_500, 1_266_000, 1_300_000, 1_400_000, 2_000_000,
                    rng.randrange(1, 400000)])
    return start, n


def test_no_general_voice_and_the_lean_bank_predicate(gp):
    rng = random.Random(1)
    for _ in range(300):
        F = random_facts(gp, rng)
        for _ in range(20):
            start, n = random_call(rng)
            assert bool(gp.gp_no_general_voice(F.h, start, n)) == F.no_general_voice(start, n), (F.__dict__, start, n)
            assert bool(gp.gp_lean_bank(F.h, 0, n)) == F.lean_bank(False, n) and not gp.gp_lean_bank(F.h, 1, n)


def test_plan_segments_follows_its_comment(gp):
    rng = random.Random(2)
    cut = (C.c_uint32 * (SEG_MAX + 2))()
    for _ in range(300):
        F = random_facts(gp, rng)
        for _ in range(10):
            start, n = random_call(rng)
            T = rng.choice([256, 512, 1024])
            max_len, corners = rng.choice([(SEG, False), (2 ** 64 - 1, True), (2 ** 64 - 1, False)])
            ns = gp.gp_plan_segments(F.h, start, n, T, max_len, int(corners), cut)
            c = [start + cut[k] for k in range(ns + 1)]
            what = (F.__dict__, start, n, T, max_len, corners, c)
            assert 1 <= ns <= SEG_MAX and c[0] == start and c[-1] <= start + n, what
            assert all(a < b and b - a <= max_len for a, b in zip(c, c[1:])), what
            assert c[-1] == start + n or ns == SEG_MAX, what            # short of the end only when the segments run out
            shared = corners and F.corners
            if not shared and start < F.flat_from < start + n and F.flat_from - start <= max_len:
                assert c[1] == F.flat_from, what                          # a cut where the envelopes turn flat
            for a, b in zip(c, c[1:]):
                # never across a shared corner / the first sustain end; otherwise T, then doubling positions -- or less: max_len,
                # the end, or a very short rest (at most 1/64 of the position) joining the last segment
                if shared:
                    assert not any(a < x < b for x in F.corners), what
                elif a >= F.flat_from or a > start:
                    assert not a < F.flat_until < b or b == start + n, what
                nxt = T if a < T else 2 * a
                if a != start or shared or not start < F.flat_from < start + n:
                    assert b <= nxt or (b == start + n and b - nxt <= nxt // 64), what


def fields(gp, F, start, n, form, rows=False, no_seg=False):
    buf = C.create_string_buffer(1 << 22)
    rc = gp.gp_plan_fields(F.h, start, n, FORM[form], int(rows), int(no_seg), buf, len(buf))
    if rc == -2:
        return None, 0
    assert rc >= 0
    steps = []
    for line in buf.value.decode().splitlines():
        p = line.split()
        if p[0] == "S":
            v = [int(x) for x in p[1:11]]
            steps.append(dict(first=v[0], n=v[1], records=v[2], nseg=v[3], mix=v[4], sfirst=v[5], sn=v[6], temp=v[7], opens=v[8], closes=v[9],
                              cuts=[int(x) for x in p[11].split(",")], launches=[]))
        elif p[0] == "X":
            v = [int(x) for x in p[1:13]]
            tab = [tuple(int(y) for y in x.replace("+", " ").replace("@", " ").split()) for x in p[13][p[13].index("[") + 1:-1].split(",") if x]
            steps[-1]["launches"].append(dict(kernel=v[0], fpl=v[1], lean=v[2], fold=v[3], guard=v[4], gx=v[5], gy=v[6], first=v[7], n=v[8], set=v[9],
                                              segf=v[10], split=v[11], tab=tab))
        else:
            fused = int(p[1])
    return steps, fused


def test_plan_invariants(gp):
    rng = random.Random(3)
    ncalls = 0
    for _ in range(400):
        F = random_facts(gp, rng)
        nchunks = (F.nvoices + 63) // 64
        for _ in range(8):
            start, n = random_call(rng)
            form = rng.choice(list(FORM))
            rows = form in ("f32", "i16") and rng.random() < 0.15
            steps, fused = fields(gp, F, start, n, form, rows, rng.random() < 0.2)
            what = (F.__dict__, start, n, form, rows)
            if form in ("mix", "maps") and F.nvoices > 32768:
                assert steps is None, what                  # refused before planning
                continue
            ncalls += 1
            pos = 0
            for s in steps:                                  # the steps tile [0, n) once, in order
                assert s["first"] == pos and s["n"] > 0, what
                pos += s["n"]
            assert pos == n, what
            assert fused == sum(1 for s in steps if s["mix"] == FUSED), what
            for s in steps:
                i16 = form in ("i16", "mix", "maps")
                assert (s["mix"] == ROWS) == (form in ("f32", "i16", "f64")), what
                if s["records"] == TABLE_SETS:
                    assert 2 <= s["nseg"] <= SEG_MAX and s["cuts"][0] == 0 and s["cuts"][-1] == s["n"] and start + s["first"] < SEG, what
                elif s["records"] == EQUAL_SETS:
                    assert s["nseg"] == -(-s["n"] // SEG) > 1, what
                else:
                    assert s["nseg"] == 1, what
                if s["mix"] != ROWS:                         # stretches: whole segments, capped, one temporary each
                    assert s["sfirst"] % SEG == 0 and s["sfirst"] <= s["first"] and s["first"] + s["n"] <= s["sfirst"] + s["sn"], what
                    assert s["sn"] <= (16 if s["mix"] == FUSED else 4) * SEG, what
                    if s["opens"]:
                        assert s["first"] == s["sfirst"], what
                        assert s["temp"] == (2 * nchunks * s["sn"] * 8 if s["mix"] == FUSED else F.nvoices * ((s["sn"] + 63) // 64 * 64) * 2), what
                    if s["closes"]:
                        assert s["first"] + s["n"] == s["sfirst"] + s["sn"], what
                if s["mix"] == FUSED:
                    assert s["opens"] and s["closes"] and F.lean_bank(False, n), what
                    for f in range(0, s["n"], SEG):          # a fused stretch: no general voice in any of its segments
                        assert F.no_general_voice(start + s["first"] + f, min(SEG, s["n"] - f)), what
                    assert [l["kernel"] for l in s["launches"]] == [LEAN_HARM, COMPOSE if form == "maps" else COMBINE], what
                    assert s["launches"][1]["gx"] * 256 >= s["n"] and s["launches"][1]["split"] == 2 * nchunks, what
                if s["mix"] == TWO_STEP and s["opens"] and F.lean_bank(False, n):
                    assert not F.no_general_voice(start + s["sfirst"], min(SEG, s["sn"])), what
                for l in s["launches"]:
                    assert l["first"] + l["n"] <= s["n"] and l["gx"] >= 1 and 1 <= l["gy"] <= 65535, what
                    if l["kernel"] == LEAN_HARM:
                        assert F.lean_bank(rows, n if s["mix"] == FUSED else s["n"]) or s["records"] == TABLE_SETS, what
                        assert l["fpl"] in (4, 8, 16) and l["segf"] % 1024 == 0 and l["gy"] == 2 * nchunks and l["split"] == 2, what
                        assert l["guard"] == (F.has_guard if i16 else 1) and l["fold"] == (s["mix"] == FUSED), what
                        if l["tab"]:
                            assert sum(t[1] for t in l["tab"]) == s["n"] and l["segf"] == SEG, what
                            assert l["gx"] * 4 >= sum(-(-t[1] // (64 * l["fpl"])) for t in l["tab"]), what
                        else:
                            assert l["gx"] * 256 * l["fpl"] >= s["n"] and l["segf"] * s["nseg"] >= s["n"], what
                    elif l["kernel"] == LISTS:
                        if l["tab"]:
                            assert all(not F.no_general_voice(start + s["first"] + t[0], t[1]) for t in l["tab"]) and l["gy"] == 8 * nchunks, what
                        else:
                            assert l["gx"] * 1024 >= l["n"] and l["gy"] == nchunks and l["set"] * SEG == l["first"], what
                            assert l["lean"] or not F.no_general_voice(start + s["first"] + l["first"], l["n"]), what
                    elif l["kernel"] == GENERATE:
                        assert l["fpl"] == (4 if s["n"] >= 8192 else 2 if s["n"] >= 2048 else 1), what
                        assert l["gx"] * 256 * l["fpl"] >= s["n"] and l["gy"] * l["split"] >= F.nvoices, what
    assert ncalls > 2500


def recorded():
    banks, calls, cur = {}, [], None
    for line in (ROOT / "tests" / "golden" / "genplan_routes.txt").read_text().splitlines():
        if line.startswith("BANK"):
            cur = line.split()[1]
        elif line.startswith("FACTS"):
            banks[cur] = dict(x.split("=") for x in line.split()[1:])
        elif line.startswith("CALL"):
            calls.append((line, []))
        else:
            calls[-1][1].append(line)
    return banks, calls


def test_the_recorded_route_table(gp):
    """plan()'s output, call by call, against what the parent's launch code did: zero differing lines."""
    banks, calls = recorded()
    facts = {}
    for name, kv in banks.items():
        ints = lambda s: [int(x) for x in s.split(",")] if s else []
        facts[name] = Facts(gp, int(kv["nvoices"]), int(kv["lean"]), int(kv["lean_fm"]), int(kv["all_lean"]), int(kv["has_guard"]),
                            int(kv["flat_from"]), int(kv["flat_until"]), ints(kv["short_piece_end"]), ints(kv["corners"]))
    assert len(calls) >= 660
    # the segmented head followed by the rest of the row (the parent's recursion): a rest of >= 8192 frames, one set and equal sets, and a shorter one
    rests = set()
    for line, ev in calls:
        rs = [k for k, e in enumerate(ev) if e.startswith("R ")]
        if line.split()[2] in ("f32", "i16") and len(rs) == 2 and ev[rs[0]].startswith("R var"):
            kernel = ev[rs[1] + 1].split()[1]
            rests.add((ev[rs[1]].split()[1], kernel if kernel.startswith("gen") else kernel.split("<")[0]))
    assert {("one", "lean"), ("eq", "lean"), ("one", "gen<2>"), ("one", "gen<1>")} <= rests, rests
    buf = C.create_string_buffer(1 << 20)
    differing, seen = [], set()
    for line, events in calls:
        p = line.split()
        rc = gp.gp_plan_routes(facts[p[1]].h, int(p[3]), int(p[4]), FORM[p[2]], int(len(p) > 6), int(p[5] == "noseg"), buf, len(buf))
        assert rc >= 0, line
        got = buf.value.decode().splitlines()
        seen.update(e.split(" grid")[0] for e in events if e.startswith("L "))
        if got != events:
            differing.append((line, [(a, b) for a, b in zip(events + [None] * len(got), got + [None] * len(events)) if a != b][:3]))
    assert not differing, differing[:5]
    # the table takes every instantiation the unit has: 3 + 4 + 3 + 12 + 2
    want = {"L gen<%d> %s" % (f, t) for f in (1, 2, 4) for t in ("f32",)} | {"L lists<%d,%s>" % (l, t) for l in (0, 1) for t in ("f32", "i16")}
    want |= {"L lean<%d,f32,0,1>" % f for f in (4, 8, 16)} | {"L lean<%d,i16,%d,%d>" % (f, fo, g) for f in (4, 8, 16) for fo in (0, 1) for g in (0, 1)}
    want |= {"L combine", "L compose"}
    assert want <= seen, sorted(want - seen)
