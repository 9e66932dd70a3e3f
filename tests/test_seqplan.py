"""The plan of sh_mix_events (synthesizer_amd/csrc/seqplan.hpp) built for the host with g++, against a brute-force restatement:
which tiles of the track a list of placed samples touches, which events each tile folds and in which order, and the refusals."""
import ctypes as C
import random
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
OK, EVENT_BEYOND_TRACK, TRACK_TOO_LONG, TOO_MANY_PAIRS = range(4)


@pytest.fixture(scope="module")
def sq(tmp_path_factory):
    out = tmp_path_factory.mktemp("seqplan") / "libseqplan.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", str(ROOT / "tests" / "cpu_seqplan.cpp"), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.sq_tile.restype = C.c_uint32
    lib.sq_max_track.restype = lib.sq_max_pairs.restype = lib.sq_npairs.restype = C.c_uint64
    lib.sq_plan.restype = C.c_void_p
    lib.sq_plan.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.POINTER(C.c_int),
                            C.POINTER(C.c_uint32)]
    for fn in (lib.sq_free, lib.sq_ntiles, lib.sq_npairs, lib.sq_nfirst, lib.sq_tiles, lib.sq_first, lib.sq_idx):
        fn.argtypes = [C.c_void_p]
    lib.sq_ntiles.restype = lib.sq_nfirst.restype = C.c_uint32
    for fn in (lib.sq_tiles, lib.sq_first, lib.sq_idx):
        fn.restype = C.POINTER(C.c_uint32)
    return lib


def run_plan(sq, events, track, tile, max_pairs=None):
    """(refusal, bad_event, tiles, first, idx)"""
    n = len(events)
    dst = (C.c_uint64 * max(n, 1))(*[e[0] for e in events])
    cnt = (C.c_uint64 * max(n, 1))(*[e[1] for e in events])
    refused, bad = C.c_int(), C.c_uint32()
    p = sq.sq_plan(dst, cnt, n, track, tile, sq.sq_max_pairs() if max_pairs is None else max_pairs, C.byref(refused), C.byref(bad))
    try:
        nt, npairs, nf = sq.sq_ntiles(p), sq.sq_npairs(p), sq.sq_nfirst(p)
        return refused.value, bad.value, sq.sq_tiles(p)[:nt], sq.sq_first(p)[:nf], sq.sq_idx(p)[:npairs]
    finally:
        sq.sq_free(p)


def brute(events, tile):
    """tile -> the events that overlap it, in list order; sample by sample in meaning: an event covers [dst, dst + n)"""
    per = {}
    for e, (dst, n) in enumerate(events):
        if n:
            for t in range(dst // tile, (dst + n - 1) // tile + 1):
                per.setdefault(t, []).append(e)
    return per


def random_list(rng, tile):
    ntiles = rng.choice([1, 2, 3, 17, 200])
    track = ntiles * tile - rng.choice([0, 0, 1, tile // 2, tile - 1])
    nev = rng.choice([0, 1, 2, 3, 10, 50, 300, 1000, 5000])
    lengths = [0, 1, tile - 1, tile, tile + 1, 5 * tile + 3, 40 * tile]
    pile = rng.randrange(track)
    events = []
    for _ in range(nev):
        n = min(rng.choice(lengths + [rng.randrange(0, 3 * tile)]), track)
        kind = rng.random()
        if kind < 0.25:
            dst = rng.randrange(0, ntiles) * tile                     # on a tile edge
        elif kind < 0.4:
            dst = max(0, rng.randrange(0, ntiles) * tile + rng.choice([-1, 1, -n, -n + 1, -n - 1]))
        elif kind < 0.55:
            dst = pile                                                  # a pile-up on one sample
        else:
            dst = rng.randrange(0, track)
        dst = min(dst, track - n)                                       # every event ends inside the track
        events.append((dst, n))
    return track, events


def test_plan_against_brute_force(sq):
    assert sq.sq_tile(2) == 2048 and sq.sq_tile(1) == sq.sq_tile(3) == sq.sq_tile(4) == 1024
    rng = random.Random(11)
    nlists = sizes = 0
    for k in range(320):
        tile = rng.choice([sq.sq_tile(2), sq.sq_tile(1), 8])
        track, events = random_list(rng, tile)
        refused, _bad, tiles, first, idx = run_plan(sq, events, track, tile)
        assert refused == OK
        want = brute(events, tile)
        what = (k, tile, track, len(events))
        assert sorted(tiles) == sorted(want), what                       # the active tiles: exactly those some non-empty event overlaps
        assert len(set(tiles)) == len(tiles), what
        assert len(first) == len(tiles) + 1 and first[0] == 0 and first[-1] == len(idx), what
        counts = [first[j + 1] - first[j] for j in range(len(tiles))]
        assert all(c > 0 for c in counts), what                           # no tile without events
        assert all(a >= b for a, b in zip(counts, counts[1:])), what      # heaviest first
        for j, t in enumerate(tiles):
            got = idx[first[j]:first[j + 1]]
            assert got == want[t], (what, t)                              # every overlap once, ascending = list order
            assert all(a < b for a, b in zip(got, got[1:])), (what, t)
        assert len(idx) == sum((d + n - 1) // tile - d // tile + 1 for d, n in events if n), what      # pairs = sum of tiles spanned
        nlists += 1
        sizes += len(events) >= 1000
    assert nlists >= 300 and sizes >= 30


def test_each_refusal_fires_and_only_then(sq):
    tile = sq.sq_tile(2)
    track = 10 * tile
    # an event that ends beyond the track: the first such is named; one that ends exactly at the end is taken
    assert run_plan(sq, [(0, track), (track, 0), (track - 1, 1)], track, tile)[0] == OK
    assert run_plan(sq, [(0, 5), (track - 1, 2), (track + 1, 0)], track, tile)[:2] == (EVENT_BEYOND_TRACK, 1)
    assert run_plan(sq, [(track + 1, 0)], track, tile)[:2] == (EVENT_BEYOND_TRACK, 0)
    assert run_plan(sq, [(2 ** 64 - 1, 2)], track, tile)[:2] == (EVENT_BEYOND_TRACK, 0)          # (no wrap-around)
    assert run_plan(sq, [(3, 2 ** 64 - 1)], track, tile)[:2] == (EVENT_BEYOND_TRACK, 0)
    # the track's length against the 32-bit sample index
    big = sq.sq_max_track()
    assert big == 2 ** 32 - 65536
    assert run_plan(sq, [(big - 1, 1)], big, tile)[0] == OK
    assert run_plan(sq, [], big + 1, tile)[0] == TRACK_TOO_LONG
    # the pair count against the CSR offsets: three events over four tiles each = 12 pairs
    events = [(0, 4 * tile), (1, 4 * tile - 1), (tile, 3 * tile + 1)]
    assert len(run_plan(sq, events, track, tile, max_pairs=12)[4]) == 12
    assert run_plan(sq, events, track, tile, max_pairs=11)[0] == TOO_MANY_PAIRS
    assert sq.sq_max_pairs() < 2 ** 32


def test_empty_inputs(sq):
    tile = sq.sq_tile(2)
    for events, track in (([], 0), ([], 5000), ([(0, 0)], 0), ([(7, 0), (5000, 0)], 5000)):
        refused, _bad, tiles, first, idx = run_plan(sq, events, track, tile)
        assert refused == OK and tiles == [] and first == [0] and idx == []


# ---- the same plans far out: past 2^31 samples and up to the last tile a track can have ---------------------------------------------------------
MAX = 2 ** 32 - 65536
DM_LIMIT = 2 ** 31 - 32768                                  # where a downmix ends at the latest (sequence.hip forms 2 * (dst + n) in 32 bits)


def near_lists(tile):
    """[(track samples, events)]: the four-tile song of the GPU tests (a note across the first tile edge, a pile-up in tile 1, tile 2
    idle, the song ending mid-lane in tile 3), events on and around every tile edge with empty ones between, a whole number of tiles
    under one long note, and two generated lists"""
    lane = tile // 256 or 1
    w0 = tile + 3 * lane
    song = [(0, 300 % tile), (tile - tile // 4, tile // 2), (w0 - lane, 3 * lane), (w0 + 10, tile // 8), (w0 + 13, tile // 8), (w0 + 17, tile // 8),
            (3 * tile, 37 * lane + 3)]
    edges = [(0, 0), (tile - 1, 1), (tile - 1, 2), (tile, tile), (2 * tile, 0), (3 * tile - 1, tile + 1), (5, 4 * tile - 5), (4 * tile - 1, 1)]
    lists = [(3 * tile + 37 * lane + 3, song), (4 * tile, edges), (7 * tile, [(0, 7 * tile), (3 * tile + 1, 2), (7 * tile - 2, 2)])]
    rng = random.Random(1000 + tile)
    for ntiles in (3, 17):
        track = ntiles * tile - rng.randrange(1, tile)
        events = []
        for _ in range(60):
            n = rng.choice([0, 1, tile - 1, tile, tile + 1, rng.randrange(0, 3 * tile)])
            n = min(n, track)
            events.append((rng.randrange(0, track - n + 1), n))
        lists.append((track, events))
    return lists


def far_bases(tile, track, events):
    """{name: (B, tile-aligned)}: `mid` puts the list's second tile on sample 2^31, `top` its last tile on the last tile a track can have (a
    list of whole tiles then ends at MAX), `dm` the end of its first sounding event on the downmix limit, which is no multiple of the tile"""
    ntiles = -(-track // tile)
    d, n = next(e for e in events if e[1])
    dm = DM_LIMIT - (d + n)
    if dm % tile == 0:
        dm -= 3
    return {"mid": (2 ** 31 - tile, True), "top": (MAX - ntiles * tile, True), "dm": (dm, False)}


def shifted(events, B):
    return [(d + B, n) for d, n in events]


def test_a_list_placed_far_out_plans_as_the_near_one_with_its_tiles_raised(sq):
    assert sq.sq_max_track() == MAX
    crossed = ended = 0
    for tile in (sq.sq_tile(2), sq.sq_tile(1)):
        for track, events in near_lists(tile):
            refused, _bad, tiles, first, idx = run_plan(sq, events, track, tile)
            assert refused == OK and tiles
            for name, (B, aligned) in far_bases(tile, track, events).items():
                what = (tile, track, len(events), name)
                far = shifted(events, B)
                assert B + track <= MAX and B > 2 ** 30
                r2, _b2, tiles2, first2, idx2 = run_plan(sq, far, B + track, tile)
                assert r2 == OK, what
                if aligned:                                 # the near plan, every tile number raised by B / tile
                    assert B % tile == 0 and tiles2 == [t + B // tile for t in tiles] and first2 == first and idx2 == idx, what
                    assert max(tiles2) == (B + max(d + n for d, n in events if n) - 1) // tile < 2 ** 22, what
                want = brute(far, tile)                     # and, aligned or not, the brute-force overlap count at the far coordinates
                assert sorted(tiles2) == sorted(want) and len(first2) == len(tiles2) + 1 and first2[-1] == len(idx2), what
                counts = [first2[j + 1] - first2[j] for j in range(len(tiles2))]
                assert all(a >= b for a, b in zip(counts, counts[1:])), what
                for j, t in enumerate(tiles2):
                    assert idx2[first2[j]:first2[j + 1]] == want[t], (what, t)
                crossed += any(d < 2 ** 31 < d + n for d, n in far)
                ended += B + track == MAX
                # one sample more than the track holds is still refused up there
                assert run_plan(sq, far + [(B + track, 1)], B + track, tile)[:2] == (EVENT_BEYOND_TRACK, len(far)), what
    assert crossed >= 4 and ended >= 2


def test_the_program_of_its_own(tmp_path):
    """cpu_seqplan.cpp with its own main: the form a sanitizer build runs (here built plainly)"""
    exe = tmp_path / "seqplan"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-DSEQPLAN_MAIN", str(ROOT / "tests" / "cpu_seqplan.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert out.startswith("seqplan: ") and out.rstrip().endswith("ok")
