"""csrc/seqhist.hpp -- the block geometry of a level history of a compiled song and the fold of consecutive blocks -- built for the host
with g++, against Python integers: the number of blocks of a window and the samples each counts for windows at every alignment (one
sample, exactly one tile, the far end of a song of 2^32 - 65536 samples), the block of a tile, the row offsets in 64 bits, and the fold.
tests/cpu_seqhist.cpp also builds as a program of its own (-DSEQHIST_MAIN), which is built and run once here without a sanitizer.  No GPU."""
import ctypes as C
import random
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
MAX = 2 ** 32 - 65536                                       # shq::MAX_TRACK_SAMPLES
TILES = [1024, 2048]                                        # shq::tile_samples: widths 1, 3, 4 and width 2


class Row(C.Structure):
    _fields_ = [("peak", C.c_uint32 * 2), ("sq_hi", C.c_uint64 * 2), ("sq_lo", C.c_uint64 * 2)]


@pytest.fixture(scope="module")
def sq(tmp_path_factory):
    out = tmp_path_factory.mktemp("seqhist") / "libseqhist.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", str(ROOT / "tests" / "cpu_seqhist.cpp"), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.sq_nblocks.restype = lib.sq_tile_of.restype = lib.sq_block_of.restype = C.c_uint32
    lib.sq_nblocks.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
    lib.sq_tile_of.argtypes = [C.c_uint64, C.c_uint32]
    lib.sq_block_of.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32]
    lib.sq_range.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.sq_range.restype = None
    lib.sq_row_at.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    lib.sq_row_at.restype = C.c_uint64
    lib.sq_fold.argtypes = [C.POINTER(Row), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Row)]
    lib.sq_fold.restype = None
    return lib


def want_blocks(lo, hi, tile):
    """the issue's statement, in Python ints: [(a, b)] per block"""
    if hi <= lo:
        return []
    n = (hi - 1) // tile - lo // tile + 1
    return [(max(lo, (lo // tile + j) * tile), min(hi, (lo // tile + j + 1) * tile)) for j in range(n)]


def got_blocks(sq, lo, hi, tile):
    out = []
    for j in range(sq.sq_nblocks(lo, hi, tile)):
        a, b = C.c_uint64(), C.c_uint64()
        sq.sq_range(j, lo, hi, tile, C.byref(a), C.byref(b))
        out.append((a.value, b.value))
    return out


def windows(tile, total):
    """every alignment: starts and ends on, one off and mid-way between the tile edges; one sample; exactly one tile; empty ones"""
    marks = sorted({0, 1, tile // 2, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1, 3 * tile, total - 1, total})
    return [(a, b) for a in marks for b in marks if a <= b <= total]


@pytest.mark.parametrize("tile", TILES)
def test_the_blocks_of_windows_at_every_alignment(sq, tile):
    total = 3 * tile + 37 * 8 + 3                           # the tests' songs: four tiles, ending mid-lane
    seen = set()
    for lo, hi in windows(tile, total):
        want = want_blocks(lo, hi, tile)
        assert got_blocks(sq, lo, hi, tile) == want, (lo, hi)
        assert sum(b - a for a, b in want) == hi - lo and all(a < b for a, b in want)      # the blocks tile the window, none is empty
        assert all((a // tile) == ((b - 1) // tile) for a, b in want)                      # and none crosses a tile's edge
        for j, (a, _b) in enumerate(want):
            assert sq.sq_block_of(sq.sq_tile_of(a, tile), lo, tile) == j
        seen.add(len(want))
    assert seen >= {0, 1, 2, 3, 4}
    assert got_blocks(sq, 5, 6, tile) == [(5, 6)] and got_blocks(sq, tile, 2 * tile, tile) == [(tile, 2 * tile)]       # one sample; exactly one tile
    assert got_blocks(sq, tile - 1, tile + 1, tile) == [(tile - 1, tile), (tile, tile + 1)] and got_blocks(sq, 7, 7, tile) == []


@pytest.mark.parametrize("tile", TILES)
def test_the_blocks_at_the_far_end_of_the_longest_song(sq, tile):
    assert MAX % tile == 0 and sq.sq_nblocks(0, MAX, tile) == MAX // tile
    for lo, hi in ((MAX - 1, MAX), (MAX - tile, MAX), (MAX - tile - 1, MAX), (2 ** 31 - 1, 2 ** 31 + 1), (2 ** 31 - tile, 2 ** 31 + 3 * tile + 5),
                   (MAX - 3 * tile - 7, MAX - 9), (0, MAX)):
        n = sq.sq_nblocks(lo, hi, tile)
        assert n == (hi - 1) // tile - lo // tile + 1
        want = want_blocks(lo, hi, tile) if n <= 8 else None
        if want is not None:
            assert got_blocks(sq, lo, hi, tile) == want, (lo, hi)
        for j in {0, 1, n // 2, n - 1} & set(range(n)):     # (t + 1) * tile passes 2^32 in the last tile: the range is formed in 64 bits
            a, b = C.c_uint64(), C.c_uint64()
            sq.sq_range(j, lo, hi, tile, C.byref(a), C.byref(b))
            assert (a.value, b.value) == (max(lo, (lo // tile + j) * tile), min(hi, (lo // tile + j + 1) * tile))
            assert sq.sq_block_of((lo // tile + j), lo, tile) == j and sq.sq_tile_of(a.value, tile) == lo // tile + j


def test_a_row_offset_is_formed_in_64_bits(sq):
    blocks = MAX // 1024                                    # 4 194 240 blocks at width 1
    for j, nrows, r in ((0, 4, 3), (1, 4, 0), (blocks - 1, 41, 40), (blocks - 1, 33, 0), (2 ** 27, 41, 7), (2 ** 32 - 1, 41, 40)):
        assert sq.sq_row_at(j, nrows, r) == j * nrows + r
    assert (blocks - 1) * 41 + 40 < 2 ** 32 < ((blocks - 1) * 41 + 40) * 40     # rows fit 32 bits, BYTES do not: the pointer arithmetic is size_t's
    assert sq.sq_row_at(2 ** 32 - 1, 41, 40) > 2 ** 32


def value(r):
    return (r.peak[0], r.peak[1]), ((r.sq_hi[0] << 32) + r.sq_lo[0], (r.sq_hi[1] << 32) + r.sq_lo[1])


def test_the_fold_of_consecutive_blocks(sq):
    rng = random.Random(7)
    for case in range(60):
        nrows, nblocks = rng.randrange(1, 42), rng.randrange(1, 30)
        table = (Row * (nrows * nblocks))()
        for r in table:
            for c in range(2):
                r.peak[c] = rng.choice([0, 1, 2 ** 31, rng.randrange(2 ** 32)])
                r.sq_hi[c] = rng.choice([0, rng.randrange(2 ** 41)])       # 2048 samples of 2^62 >> 32 at the most
                r.sq_lo[c] = rng.choice([0, rng.randrange(2 ** 43)])
        j = rng.randrange(nblocks)
        n = rng.randrange(0, nblocks - j + 1)
        out = (Row * nrows)()
        C.memset(out, 0xAB, C.sizeof(out))
        sq.sq_fold(table, j, n, nrows, out)
        for r in range(nrows):
            rows = [table[b * nrows + r] for b in range(j, j + n)]
            for c in range(2):
                assert out[r].peak[c] == max([x.peak[c] for x in rows] + [0])
                assert out[r].sq_hi[c] == sum(x.sq_hi[c] for x in rows) and out[r].sq_lo[c] == sum(x.sq_lo[c] for x in rows)
            # the value of the fold is the sum of the values: integer sums, whatever the order
            assert value(out[r])[1] == tuple(sum(value(x)[1][c] for x in rows) for c in range(2))
    # folding a fold: blocks [0, 6) as three pairs, then the pairs, against all six at once
    nrows = 3
    table = (Row * (nrows * 6))()
    for r in table:
        for c in range(2):
            r.peak[c], r.sq_hi[c], r.sq_lo[c] = rng.randrange(2 ** 32), rng.randrange(2 ** 40), rng.randrange(2 ** 43)
    pairs = (Row * (nrows * 3))()
    for k in range(3):
        part = (Row * nrows)()
        sq.sq_fold(table, 2 * k, 2, nrows, part)
        for r in range(nrows):
            pairs[k * nrows + r] = part[r]
    once, twice = (Row * nrows)(), (Row * nrows)()
    sq.sq_fold(table, 0, 6, nrows, once)
    sq.sq_fold(pairs, 0, 3, nrows, twice)
    assert bytes(once) == bytes(twice)


def test_the_file_is_a_program_of_its_own_as_well(tmp_path):
    exe = tmp_path / "cpu_seqhist"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DSEQHIST_MAIN", str(ROOT / "tests" / "cpu_seqhist.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("seqhist: ") and p.stdout.strip().endswith("ok"), p.stdout + p.stderr
