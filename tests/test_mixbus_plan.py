"""The launch plan of sh_mix_bus_f32 (synthesizer_amd/csrc/mixbus_plan.hpp) built for the host with g++: the plan of every case of
tests/test_gpu_mixbus.py (a case named for a kernel route reaches that route), every threshold of the plan from both sides, the
chunks of a long call and what a pointer off the 16-byte grid changes.  No GPU."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
U32, U64 = ctypes.c_uint32, ctypes.c_uint64
FIELDS = ("tiles", "groups", "voices_per_group", "direct", "stream", "vec", "part_stride", "part_bytes")
MAX_FRAMES = 1 << 24


@pytest.fixture(scope="module")
def mb(tmp_path_factory):
    out = tmp_path_factory.mktemp("mixbus") / "libmixbus.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", str(ROOT / "tests" / "cpu_mixbus.cpp"), "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    lib.mb_chunks.argtypes = [U32]
    lib.mb_chunks.restype = U32
    lib.mb_chunk.argtypes = [U32, U32, ctypes.c_void_p]
    lib.mb_plan.argtypes = [U32, U64, U32, U64, U64, ctypes.c_void_p]
    return lib


def plan(mb, nvoices, nframes, stride, voices=0, bus=0):
    """the plan of ONE launch (nframes <= 2^24) as a dict of FIELDS; voices / bus: device addresses (their residues mod 16 decide)"""
    assert 0 < nframes <= MAX_FRAMES
    v = np.zeros(8, np.uint64)
    mb.mb_plan(nvoices, stride, nframes, voices, bus, v.ctypes.data)
    return dict(zip(FIELDS, (int(x) for x in v)))


def launches(mb, nvoices, nframes, stride, voices=0, bus=0):
    """[(first frame, frames, plan)] of a call: one entry per chunk, each with the addresses its launch sees"""
    out = []
    v = np.zeros(2, np.uint64)
    for c in range(mb.mb_chunks(nframes)):
        mb.mb_chunk(nframes, c, v.ctypes.data)
        off, n = int(v[0]), int(v[1])
        out.append((off, n, plan(mb, nvoices, n, stride, voices + 4 * off, bus + 8 * off)))
    return out


def route(p):
    return "direct-nt" if p["direct"] and p["stream"] else "direct" if p["direct"] else "split"


def group_sizes(p, nvoices):
    g, per = p["groups"], p["voices_per_group"]
    return [min(per, nvoices - k * per) for k in range(g)]


def test_every_gpu_case_reaches_its_route(mb):
    from tests import test_gpu_mixbus as M
    assert {c.route for c in M.CASES} == {"split", "direct", "direct-nt", "chunked"}
    for c in M.CASES:
        ls = launches(mb, c.nv, c.nf, c.stride)
        if c.route == "chunked":
            assert [(off, n, route(p)) for off, n, p in ls] == [(0, MAX_FRAMES, "direct"), (MAX_FRAMES, c.nf - MAX_FRAMES, "split")], c.id
            continue
        assert len(ls) == 1 and ls[0][:2] == (0, c.nf), c.id
        p = ls[0][2]
        assert route(p) == c.route, (c.id, p)
        assert p["vec"] == 1 and p["tiles"] == -(-c.nf // 256), c.id
        if c.route == "split":
            assert group_sizes(p, c.nv) == list(c.groups), (c.id, p)
            assert p["part_stride"] % 2 == 0 and p["part_stride"] - c.nf in (0, 1)
            assert p["part_bytes"] == (p["groups"] * p["part_stride"] * 8 if p["groups"] > 1 else 0)
        else:
            assert p["groups"] == 1 and p["part_bytes"] == 0, c.id


def test_the_loops_and_lane_branches_the_cases_are_named_for(mb):
    """What each split case promises about the kernel's loops, restated from k_mix_bus_f32: a wave w of a group of n voices walks
    v = w, w + 8, ...: the 8-in-flight loop runs while v + 56 < n, the 4-loop while v + 24 < n, then one row at a time."""
    from tests import test_gpu_mixbus as M

    def loops(n):
        got = set()
        for w in range(8):
            v = w
            while v + 56 < n:
                got.add(8)
                v += 64
            while v + 24 < n:
                got.add(4)
                v += 32
            if v < n:
                got.add(1)
        return got
    by_id = {c.id: c for c in M.CASES}
    for cid in ("split-loop8-1group", "split-loop8-2groups", "split-loop8-4groups"):
        assert all(8 in loops(n) for n in by_id[cid].groups), cid
    assert max(by_id["split-loop8-1group"].groups) == 63 and loops(56) == {4, 1} and 8 in loops(57)       # 57 voices: the first that enter it
    assert loops(33) == {4, 1} and loops(26) == {4, 1} and by_id["split-loop41-8groups"].groups == (33,) * 7 + (26,)
    assert len(by_id["split-32groups"].groups) == 32
    # lane branches: a vector launch (stride % 4 == 0) whose last lane is ragged needs stride > nframes
    assert sorted(c.nf % 4 for c in M.CASES if c.id.startswith("split-ragged")) == [1, 2, 3]
    assert all(c.stride % 4 == 0 and c.stride > c.nf for c in M.CASES if c.id.startswith("split-ragged"))
    assert by_id["split-scalar-stride"].stride % 4 != 0 and by_id["split-scalar-stride"].nf % 2 == 1 and len(by_id["split-scalar-stride"].groups) == 2
    assert {c.nf for c in M.CASES if c.id.startswith("split-edge")} == {1, 255, 256, 257}
    assert sorted(c.nf % 4 for c in M.CASES if c.id.startswith("direct-ragged")) == [1, 3]
    assert all(c.stride % 4 == 0 for c in M.CASES if c.route in ("direct", "direct-nt", "chunked"))
    assert by_id["direct-remainder-only"].nv < 4 <= by_id["direct-no-remainder"].nv and by_id["direct-no-remainder"].nv % 4 == 0 and by_id["direct"].nv % 4 != 0
    # every route has a windowed case, and the direct ones come off the grid
    assert {by_id[cid].route for cid in M.WINDOW_IDS} == {"split", "direct", "direct-nt", "chunked"}


def test_thresholds_from_both_sides(mb):
    # 1535 tiles against 1536: the direct kernel
    assert route(plan(mb, 9, 1535 * 256, 1535 * 256)) == "split" and route(plan(mb, 9, 1535 * 256 + 1, 1535 * 256 + 4)) == "direct"
    assert plan(mb, 9, 1535 * 256, 1535 * 256)["tiles"] == 1535 and plan(mb, 9, 1535 * 256 + 1, 1535 * 256 + 4)["tiles"] == 1536
    # tiles x groups 1023 against 1024: the next doubling of the groups
    assert plan(mb, 64, 1023 * 256, 1023 * 256)["groups"] == 2 and plan(mb, 64, 1023 * 256 + 1, 1023 * 256 + 4)["groups"] == 1
    assert plan(mb, 128, 511 * 256, 511 * 256)["groups"] == 4 and plan(mb, 128, 511 * 256 + 1, 511 * 256 + 4)["groups"] == 2
    # nvoices / (2 groups) 31 against 32
    assert plan(mb, 63, 1000, 1000)["groups"] == 1 and plan(mb, 64, 1000, 1000)["groups"] == 2
    assert plan(mb, 127, 1000, 1000)["groups"] == 2 and plan(mb, 128, 1000, 1000)["groups"] == 4
    assert plan(mb, 2047, 256, 256)["groups"] == 32 and plan(mb, 2048, 256, 256)["groups"] == 64
    # 128 MiB of rows, and one row more (393216 frames: 1536 tiles; 393216 * 4 * 85 < 2^27 < 393216 * 4 * 86; 2^27 itself: 32 x 2^20)
    assert route(plan(mb, 85, 393216, 393216)) == "direct" and route(plan(mb, 86, 393216, 393216)) == "direct-nt"
    assert route(plan(mb, 32, 1 << 20, 1 << 20)) == "direct" and route(plan(mb, 33, 1 << 20, 1 << 20)) == "direct-nt"
    # 2^24 frames, and one more
    assert [(o, n) for o, n, _p in launches(mb, 2, MAX_FRAMES, MAX_FRAMES)] == [(0, MAX_FRAMES)]
    assert [(o, n) for o, n, _p in launches(mb, 2, MAX_FRAMES + 1, MAX_FRAMES + 4)] == [(0, MAX_FRAMES), (MAX_FRAMES, 1)]
    assert [(o, n) for o, n, _p in launches(mb, 1, 0xFFFFFFFF, 0xFFFFFFFF)][-1] == (255 * MAX_FRAMES, MAX_FRAMES - 1) and mb.mb_chunks(0) == 0


def test_pointers_off_the_grid_take_no_16_byte_access(mb):
    for nv, nf, stride in ((9, 392961, 392964), (86, 392964, 392964), (33, 1003, 1004), (120, 1001, 1004), (64, 4099, 4099)):
        on = plan(mb, nv, nf, stride)
        for av in (0, 4, 8, 12):
            for ab in (0, 8):
                p = plan(mb, nv, nf, stride, 0x7F0000000000 + av, 0x7F0100000000 + ab)
                if av == 0 and ab == 0:
                    assert p == on and p["vec"] == 1
                    continue
                assert p["direct"] == 0 and p["stream"] == 0
                # partial buses sit in the library's scratch: with groups the bus itself is written 8 bytes at a time by k_bus_sum
                assert p["vec"] == (1 if av == 0 and p["groups"] > 1 else 0), (nv, nf, av, ab)
                assert (p["groups"], p["voices_per_group"], p["part_stride"]) == (on["groups"], on["voices_per_group"], on["part_stride"]) or on["direct"]
    # a chunk keeps the residues of its call: 2^24 frames are a multiple of 16 bytes in the rows and in the bus
    for off, n, p in launches(mb, 2, MAX_FRAMES + 261, MAX_FRAMES + 264, 4, 0):
        assert p["direct"] == 0 and p["vec"] == 0
