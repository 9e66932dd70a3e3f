"""shq::plan_runs (synthesizer_amd/csrc/seqplan.hpp) built for the host with g++, against a brute-force restatement: the per-tile runs of
a song made of tracks -- one run per (tile, track) that has events there, in track order, each ending where the next track's events begin
in the tile's slice of plan_by_tile's index, which itself does not change."""
import ctypes as C
import random
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
TILE = 1024


@pytest.fixture(scope="module")
def sr(tmp_path_factory):
    out = tmp_path_factory.mktemp("seqruns") / "libseqruns.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", str(ROOT / "tests" / "cpu_seqruns.cpp"), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.sr_plan.restype = C.c_void_p
    lib.sr_plan.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_int)]
    for fn in (lib.sr_free, lib.sr_ntiles, lib.sr_npairs, lib.sr_nruns, lib.sr_nrfirst, lib.sr_first, lib.sr_idx, lib.sr_rfirst, lib.sr_runs):
        fn.argtypes = [C.c_void_p]
    lib.sr_ntiles.restype = lib.sr_max_tracks.restype = lib.sr_run_bytes.restype = C.c_uint32
    lib.sr_npairs.restype = lib.sr_nruns.restype = lib.sr_nrfirst.restype = C.c_uint64
    for fn in (lib.sr_first, lib.sr_idx, lib.sr_rfirst, lib.sr_runs):
        fn.restype = C.POINTER(C.c_uint32)
    return lib


def run_plan(sr, tracks, track_samples, tile=TILE):
    """tracks: per track a list of (dst, n).  (first, idx, rfirst, runs as (end, track)) of the concatenation"""
    events = [e for t in tracks for e in t]
    track_of = [k for k, t in enumerate(tracks) for _e in t]
    n = len(events)
    dst = (C.c_uint64 * max(n, 1))(*[e[0] for e in events])
    cnt = (C.c_uint64 * max(n, 1))(*[e[1] for e in events])
    tof = (C.c_uint32 * max(n, 1))(*track_of)
    refused = C.c_int()
    p = sr.sr_plan(dst, cnt, tof, n, track_samples, tile, C.byref(refused))
    try:
        assert refused.value == 0
        nt, npairs, nruns = sr.sr_ntiles(p), sr.sr_npairs(p), sr.sr_nruns(p)
        assert sr.sr_nrfirst(p) == nt + 1
        flat = sr.sr_runs(p)[:2 * nruns]
        return sr.sr_first(p)[:nt + 1], sr.sr_idx(p)[:npairs], sr.sr_rfirst(p)[:nt + 1], list(zip(flat[0::2], flat[1::2]))
    finally:
        sr.sr_free(p)


def brute(tracks, ntiles, tile=TILE):
    """tile -> [(track, [event indices in list order])] for the tracks that have events there, in track order; an event covers
    [dst, dst + n), sample by sample in meaning"""
    per = [[] for _ in range(ntiles)]
    e = 0
    for k, t in enumerate(tracks):
        for dst, n in t:
            if n:
                for tl in range(dst // tile, (dst + n - 1) // tile + 1):
                    if not per[tl] or per[tl][-1][0] != k:
                        per[tl].append((k, []))
                    per[tl][-1][1].append(e)
            e += 1
    return per


def check(sr, tracks, track_samples, tile=TILE):
    first, idx, rfirst, runs = run_plan(sr, tracks, track_samples, tile)
    ntiles = len(first) - 1
    want = brute(tracks, ntiles, tile)
    assert rfirst[0] == 0 and rfirst[-1] == len(runs)
    for t in range(ntiles):
        mine = runs[rfirst[t]:rfirst[t + 1]]
        assert [trk for _end, trk in mine] == [trk for trk, _ev in want[t]], t          # one run per track with events here, in track order
        e = first[t]
        for (end, trk), (_trk, evs) in zip(mine, want[t]):
            assert e < end <= first[t + 1] and idx[e:end] == evs, (t, trk)              # the run IS that track's events of the tile, list order
            e = end
        assert e == first[t + 1], t                                                     # the runs cover the tile's slice; an idle tile has none
    assert idx == [e for t in want for _trk, evs in t for e in evs]                     # idx is plan_by_tile's, unchanged: (tile, track, list) order
    return first, idx, rfirst, runs


def test_the_run_row_is_eight_bytes_and_the_limit_is_32(sr):
    assert sr.sr_run_bytes() == 8 and sr.sr_max_tracks() == 32


def test_one_track(sr):
    first, idx, rfirst, runs = check(sr, [[(0, 100), (1000, 100), (5 * TILE, 1)]], 6 * TILE)
    assert rfirst == [0, 1, 2, 2, 2, 2, 3] and runs == [(2, 0), (3, 0), (4, 0)]           # tiles 2 .. 4 idle: no run


def test_a_track_with_no_events(sr):
    first, idx, rfirst, runs = check(sr, [[(0, 10)], [], [(5, 10)], []], TILE)
    assert runs == [(1, 0), (2, 2)]
    first, idx, rfirst, runs = check(sr, [[], [], []], 3 * TILE)
    assert runs == [] and rfirst == [0, 0, 0, 0]
    first, idx, rfirst, runs = check(sr, [[(3, 0)], [(7, 0)]], TILE)                     # empty events are in no tile
    assert runs == [] and idx == []


def test_a_track_that_touches_only_some_tiles(sr):
    tracks = [[(0, 4 * TILE)], [(TILE + 5, 10), (3 * TILE, 1)], [(2 * TILE - 1, 2)]]
    first, idx, rfirst, runs = check(sr, tracks, 4 * TILE)
    assert [[trk for _e, trk in runs[rfirst[t]:rfirst[t + 1]]] for t in range(4)] == [[0], [0, 1, 2], [0, 2], [0, 1]]


def test_every_event_of_a_tile_in_one_track(sr):
    tracks = [[(0, 10)], [(TILE, 5), (TILE + 1, 5), (TILE + 2, 5), (2 * TILE - 1, 1)], [(2 * TILE, 3)]]
    first, idx, rfirst, runs = check(sr, tracks, 3 * TILE)
    assert runs[rfirst[1]:rfirst[2]] == [(first[2], 1)] and first[2] - first[1] == 4
    last = [[], [], [(0, 7), (3, 7), (9, 7)]]                                            # and all of them in the LAST track
    first, idx, rfirst, runs = check(sr, last, TILE)
    assert runs == [(3, 2)]


def test_alternating_tracks_in_adjacent_tiles(sr):
    tracks = [[(t * TILE + 3, 10) for t in range(0, 8, 2)], [(t * TILE + 3, 10) for t in range(1, 8, 2)]]
    first, idx, rfirst, runs = check(sr, tracks, 8 * TILE)
    assert [trk for _e, trk in runs] == [0, 1] * 4 and rfirst == list(range(9))


def test_the_run_totals_on_random_songs(sr):
    rng = random.Random(5)
    for k in range(200):
        tile = rng.choice([TILE, 2048, 8])
        ntiles = rng.choice([1, 2, 5, 40])
        total = ntiles * tile - rng.choice([0, 1, tile // 2])
        tracks = []
        for _t in range(rng.choice([1, 2, 3, 8, 32])):
            evs = []
            for _e in range(rng.choice([0, 1, 3, 20])):
                n = min(rng.choice([0, 1, tile - 1, tile, tile + 1, 3 * tile + 3, rng.randrange(0, 2 * tile)]), total)
                evs.append((min(rng.choice([rng.randrange(0, total), rng.randrange(0, ntiles) * tile]), total - n), n))
            tracks.append(evs)
        first, idx, rfirst, runs = check(sr, tracks, total, tile)
        want = brute(tracks, ntiles, tile)
        assert len(runs) == sum(len(t) for t in want)                                     # runs = (tile, track) pairs with events
        assert len(runs) <= len(idx) and len(runs) <= ntiles * len(tracks)
        assert sum(end - (first[t] if r == rfirst[t] else runs[r - 1][0]) for t in range(ntiles) for r, (end, _trk) in
                   enumerate(runs[rfirst[t]:rfirst[t + 1]], rfirst[t])) == len(idx)      # the runs' lengths add up to the pairs


def test_the_program_of_its_own(tmp_path):
    """cpu_seqruns.cpp with its own main: the form a sanitizer build runs (here built plainly)"""
    exe = tmp_path / "seqruns"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-DSEQRUNS_MAIN", str(ROOT / "tests" / "cpu_seqruns.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert out.startswith("seqruns: 400 songs") and out.rstrip().endswith("ok")


# ---- the runs of a song of tracks far out ------------------------------------------------------------------------------------------------------
def run_far(sr, tracks, track_samples, tile):
    """run_plan for a song of millions of tiles: (first, idx, rfirst) as numpy arrays, runs as (end, track)"""
    import numpy as np
    events = [e for t in tracks for e in t]
    track_of = [k for k, t in enumerate(tracks) for _e in t]
    n = len(events)
    dst = (C.c_uint64 * max(n, 1))(*[e[0] for e in events])
    cnt = (C.c_uint64 * max(n, 1))(*[e[1] for e in events])
    tof = (C.c_uint32 * max(n, 1))(*track_of)
    refused = C.c_int()
    p = sr.sr_plan(dst, cnt, tof, n, track_samples, tile, C.byref(refused))
    try:
        assert refused.value == 0
        nt, npairs, nruns = sr.sr_ntiles(p), sr.sr_npairs(p), sr.sr_nruns(p)
        assert sr.sr_nrfirst(p) == nt + 1
        arr = lambda ptr, count: np.ctypeslib.as_array(ptr, shape=(count,)).copy() if count else np.zeros(0, dtype=np.uint32)      # noqa: E731
        flat = sr.sr_runs(p)[:2 * nruns]
        return arr(sr.sr_first(p), nt + 1), arr(sr.sr_idx(p), npairs), arr(sr.sr_rfirst(p), nt + 1), list(zip(flat[0::2], flat[1::2]))
    finally:
        sr.sr_free(p)


def test_a_song_of_tracks_placed_far_out_has_the_near_runs_with_its_tiles_raised(sr):
    import numpy as np
    from tests.test_seqplan import MAX, far_bases, near_lists
    for tile in (2048, TILE):
        for track, events in near_lists(tile):
            for ntracks in (1, 3):
                dealt = [events[k::ntracks] for k in range(ntracks)]                   # the list dealt over the tracks, each in list order
                near_first, near_idx, near_rfirst, near_runs = check(sr, dealt, track, tile)
                for name, (B, aligned) in far_bases(tile, track, events).items():
                    what = (tile, track, ntracks, name)
                    far = [[(d + B, n) for d, n in t] for t in dealt]
                    first, idx, rfirst, runs = run_far(sr, far, B + track, tile)
                    ntiles = len(first) - 1
                    assert ntiles == -(-(B + track) // tile) and rfirst[0] == 0 and rfirst[-1] == len(runs), what
                    if aligned:                             # tile t of the near song is tile t + B / tile
                        k = B // tile
                        assert not rfirst[:k].any() and rfirst[k:].tolist() == near_rfirst and runs == near_runs, what
                        assert not first[:k].any() and first[k:].tolist() == near_first and idx.tolist() == near_idx, what
                    want = {}                               # brute()'s restatement, kept per tile that has events: tile -> [(track, [events])]
                    e = 0
                    for trk, t in enumerate(far):
                        for d, n in t:
                            if n:
                                for tl in range(d // tile, (d + n - 1) // tile + 1):
                                    if tl not in want or want[tl][-1][0] != trk:
                                        want.setdefault(tl, []).append((trk, []))
                                    want[tl][-1][1].append(e)
                            e += 1
                    assert np.flatnonzero(np.diff(rfirst.astype(np.int64))).tolist() == sorted(want), what
                    for tl, mine in want.items():
                        got = runs[rfirst[tl]:rfirst[tl + 1]]
                        assert [trk for _end, trk in got] == [trk for trk, _ev in mine], (what, tl)
                        at = int(first[tl])
                        for (end, _trk), (_t, evs) in zip(got, mine):
                            assert idx[at:end].tolist() == evs, (what, tl)
                            at = end
                        assert at == first[tl + 1], (what, tl)
    assert MAX // TILE > 2 ** 21
