"""The per-tile index of a compiled song (shq::plan_by_tile, synthesizer_amd/csrc/seqplan.hpp) built for the host with g++: every tile of
the song in song order, against a brute-force restatement and against shq::plan, the heaviest-first index of sh_mix_events -- each
active tile lists the same events in the same order -- with idle tiles, empty events, a partial last tile and the three refusals."""
import ctypes as C
import random
import subprocess
from pathlib import Path

import pytest

from tests.test_seqplan import brute, random_list

ROOT = Path(__file__).resolve().parents[1]
OK, EVENT_BEYOND_TRACK, TRACK_TOO_LONG, TOO_MANY_PAIRS = range(4)


@pytest.fixture(scope="module")
def st(tmp_path_factory):
    out = tmp_path_factory.mktemp("seqtiles") / "libseqtiles.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", str(ROOT / "tests" / "cpu_seqtiles.cpp"), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.st_tile.restype = C.c_uint32
    lib.st_max_track.restype = lib.st_max_pairs.restype = C.c_uint64
    lib.st_plan.restype = C.c_void_p
    lib.st_plan.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.POINTER(C.c_int),
                            C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
    for name in ("st_free", "st_ntiles", "st_active", "st_npairs", "st_nfirst", "st_first", "st_idx", "st_plan_ntiles", "st_plan_npairs",
                 "st_plan_tiles", "st_plan_first", "st_plan_idx"):
        getattr(lib, name).argtypes = [C.c_void_p]
    lib.st_free.restype = None
    lib.st_ntiles.restype = lib.st_active.restype = lib.st_plan_ntiles.restype = C.c_uint32
    lib.st_npairs.restype = lib.st_nfirst.restype = lib.st_plan_npairs.restype = C.c_uint64
    for name in ("st_first", "st_idx", "st_plan_tiles", "st_plan_first", "st_plan_idx"):
        getattr(lib, name).restype = C.POINTER(C.c_uint32)
    return lib


def run(st, events, track, tile, max_pairs=None):
    """{refused, bad, ntiles, active, first, idx; plan_refused, tiles, pfirst, pidx}"""
    n = len(events)
    dst = (C.c_uint64 * max(n, 1))(*[e[0] for e in events])
    cnt = (C.c_uint64 * max(n, 1))(*[e[1] for e in events])
    refused, bad, plan_refused = C.c_int(), C.c_uint32(), C.c_int()
    p = st.st_plan(dst, cnt, n, track, tile, st.st_max_pairs() if max_pairs is None else max_pairs, C.byref(refused), C.byref(bad),
                   C.byref(plan_refused))
    try:
        nt = st.st_plan_ntiles(p)
        return dict(refused=refused.value, bad=bad.value, ntiles=st.st_ntiles(p), active=st.st_active(p),
                    first=st.st_first(p)[:st.st_nfirst(p)], idx=st.st_idx(p)[:st.st_npairs(p)], plan_refused=plan_refused.value,
                    tiles=st.st_plan_tiles(p)[:nt], pfirst=st.st_plan_first(p)[:nt + 1] if nt else [0], pidx=st.st_plan_idx(p)[:st.st_plan_npairs(p)])
    finally:
        st.st_free(p)


def holds(r, events, track, tile, what):
    """everything plan_by_tile promises of an accepted list"""
    want = brute(events, tile)
    ntiles = (track + tile - 1) // tile
    assert r["refused"] == OK and r["ntiles"] == ntiles, what
    first, idx = r["first"], r["idx"]
    assert len(first) == ntiles + 1 and first[0] == 0 and first[-1] == len(idx), what
    assert all(a <= b for a, b in zip(first, first[1:])), what
    for t in range(ntiles):                                             # EVERY tile, in song order; an idle one has an empty range
        got = idx[first[t]:first[t + 1]]
        assert got == want.get(t, []), (what, t)
        assert all(a < b for a, b in zip(got, got[1:])), (what, t)      # ascending = list order
    assert r["active"] == len(want) == sum(first[t + 1] > first[t] for t in range(ntiles)), what
    assert len(idx) == sum((d + n - 1) // tile - d // tile + 1 for d, n in events if n), what
    # against shq::plan: the same active tiles, each with the same list in the same order
    assert r["plan_refused"] == OK and sorted(r["tiles"]) == sorted(want), what
    for k, t in enumerate(r["tiles"]):
        assert r["pidx"][r["pfirst"][k]:r["pfirst"][k + 1]] == idx[first[t]:first[t + 1]], (what, t)
    assert len(r["pidx"]) == len(idx), what


def test_every_tile_in_song_order_against_brute_force_and_against_plan(st):
    assert st.st_tile(2) == 2048 and st.st_tile(1) == st.st_tile(3) == st.st_tile(4) == 1024
    rng = random.Random(12)
    idle = partial = big = 0
    for k in range(320):
        tile = rng.choice([st.st_tile(2), st.st_tile(1), 8])
        track, events = random_list(rng, tile)
        r = run(st, events, track, tile)
        holds(r, events, track, tile, (k, tile, track, len(events)))
        idle += r["active"] < r["ntiles"]
        partial += track % tile != 0
        big += len(events) >= 1000
    assert idle >= 30 and partial >= 30 and big >= 30


def test_idle_tiles_empty_events_and_a_partial_last_tile(st):
    tile = st.st_tile(2)
    track = 4 * tile - 1000                                             # four tiles, the last one partial
    events = [(5, tile - 5), (100, 0), (tile - 1, 2), (3 * tile + 7, tile - 1007), (2 * tile, 0), (3 * tile, 1)]
    r = run(st, events, track, tile)
    holds(r, events, track, tile, "four tiles")
    assert r["ntiles"] == 4 and r["active"] == 3
    assert r["first"] == [0, 2, 3, 3, 5] and r["idx"] == [0, 2, 2, 3, 5]              # tile 2 is idle; the empty events are nowhere
    # an idle LAST tile: its range is empty and ends the index
    r = run(st, [(0, 10)], 3 * tile, tile)
    assert r["first"] == [0, 1, 1, 1] and r["idx"] == [0] and r["active"] == 1
    # nothing at all
    for events, track in (([], 0), ([(0, 0)], 0)):
        r = run(st, events, track, tile)
        assert r["refused"] == OK and r["ntiles"] == 0 and r["first"] == [0] and r["idx"] == [] and r["active"] == 0
    for events in ([], [(7, 0), (5000, 0)]):                            # a song of silence: three idle tiles
        r = run(st, events, 5000, tile)
        assert r["refused"] == OK and r["ntiles"] == 3 and r["first"] == [0, 0, 0, 0] and r["idx"] == [] and r["active"] == 0


def test_each_refusal_fires_and_only_then(st):
    tile = st.st_tile(2)
    track = 10 * tile
    assert run(st, [(0, track), (track, 0), (track - 1, 1)], track, tile)["refused"] == OK
    for events, bad in (([(0, 5), (track - 1, 2), (track + 1, 0)], 1), ([(track + 1, 0)], 0), ([(2 ** 64 - 1, 2)], 0), ([(3, 2 ** 64 - 1)], 0)):
        r = run(st, events, track, tile)
        assert (r["refused"], r["bad"]) == (EVENT_BEYOND_TRACK, bad) and r["plan_refused"] == EVENT_BEYOND_TRACK
    big = st.st_max_track()
    assert big == 2 ** 32 - 65536
    assert run(st, [], big + 1, tile)["refused"] == TRACK_TOO_LONG
    events = [(0, 4 * tile), (1, 4 * tile - 1), (tile, 3 * tile + 1)]      # three events over four tiles each = 12 pairs
    assert len(run(st, events, track, tile, max_pairs=12)["idx"]) == 12
    r = run(st, events, track, tile, max_pairs=11)
    assert r["refused"] == TOO_MANY_PAIRS == r["plan_refused"]


# ---- the same index far out: a song of up to 2^22 tiles, its events in the last few ------------------------------------------------------------
def run_far(st, events, track, tile):
    """run() for a song of millions of tiles: first and idx as numpy arrays, nothing of plan's but its active tiles"""
    import numpy as np
    n = len(events)
    dst = (C.c_uint64 * max(n, 1))(*[e[0] for e in events])
    cnt = (C.c_uint64 * max(n, 1))(*[e[1] for e in events])
    refused, bad, plan_refused = C.c_int(), C.c_uint32(), C.c_int()
    p = st.st_plan(dst, cnt, n, track, tile, st.st_max_pairs(), C.byref(refused), C.byref(bad), C.byref(plan_refused))
    try:
        assert refused.value == OK == plan_refused.value
        first = np.ctypeslib.as_array(st.st_first(p), shape=(st.st_nfirst(p),)).copy()
        npairs = st.st_npairs(p)
        idx = np.ctypeslib.as_array(st.st_idx(p), shape=(npairs,)).copy() if npairs else np.zeros(0, dtype=np.uint32)
        return dict(ntiles=st.st_ntiles(p), active=st.st_active(p), first=first, idx=idx, tiles=st.st_plan_tiles(p)[:st.st_plan_ntiles(p)])
    finally:
        st.st_free(p)


def test_a_song_placed_far_out_indexes_as_the_near_one_with_its_tiles_raised(st):
    import numpy as np
    from tests.test_seqplan import MAX, far_bases, near_lists, shifted
    assert st.st_max_track() == MAX
    longest = 0
    for tile in (st.st_tile(2), st.st_tile(1)):
        for track, events in near_lists(tile):
            near = run(st, events, track, tile)
            holds(near, events, track, tile, (tile, track))
            for name, (B, aligned) in far_bases(tile, track, events).items():
                what = (tile, track, len(events), name)
                far = shifted(events, B)
                r = run_far(st, far, B + track, tile)
                first, idx = r["first"], r["idx"]
                assert r["ntiles"] == -(-(B + track) // tile) == len(first) - 1 and first[0] == 0 and first[-1] == len(idx), what
                if aligned:                                 # tile t of the near song is tile t + B / tile: nothing in front, the same index behind
                    k = B // tile
                    assert r["ntiles"] == k + near["ntiles"] and r["active"] == near["active"], what
                    assert not first[:k].any() and first[k:].tolist() == near["first"] and idx.tolist() == near["idx"], what
                want = brute(far, tile)                     # and, aligned or not, the brute-force overlap count at the far coordinates
                counts = np.diff(first.astype(np.int64))
                assert (counts >= 0).all() and np.flatnonzero(counts).tolist() == sorted(want) == sorted(r["tiles"]), what
                assert r["active"] == len(want), what
                for t, evs in want.items():
                    assert idx[first[t]:first[t + 1]].tolist() == evs, (what, t)
                longest = max(longest, r["ntiles"])
    assert longest == MAX // st.st_tile(1) == 2 ** 22 - 64 > 2 ** 21     # a song of the greatest length: more tiles than one grid row takes


def test_the_program_of_its_own(tmp_path):
    """cpu_seqtiles.cpp with its own main: the form a sanitizer build runs (here built plainly)"""
    exe = tmp_path / "seqtiles"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-DSEQTILES_MAIN", str(ROOT / "tests" / "cpu_seqtiles.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert out.startswith("seqtiles: ") and out.rstrip().endswith("ok")
