"""The lookup and the lane function of fader automation as synthesizer_amd/csrc/seqauto.hpp states them for sequence.hip (sha::find,
sha::shape_from), built for the host with g++ -ffp-contract=off: the binary search against a scan, for every sample around every
boundary of tables of 0, 1, 2 and 1000 segments; a track shaped tile by tile and lane by lane against the per-sample expression
``int(x * (k * (v1 - v0) / n + v0))`` in Python floats, for tiles inside one segment, tiles that straddle a boundary and tiles that hold
several one-frame pieces, lanes of 4 and 8.  The same cases run inside the C++ file against its own brute force (sa_selfcheck), which a
stand-alone build of it with a ``main`` runs as a program.  Equality, no tolerance.  No GPU."""
import bisect
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
U32 = ctypes.c_uint32
SEG = np.dtype([("mul", "<f8"), ("slope", "<f8"), ("numsamples", "<f8"), ("offset", "<f8"), ("end", "<u4"), ("origin", "<u4"),
                ("kind", "<u4"), ("pad", "<u4")])               # she::Seg
FLAGS = ["-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-fast-math"]


@pytest.fixture(scope="module")
def sa(tmp_path_factory):
    out = tmp_path_factory.mktemp("seqauto") / "libseqauto.so"
    subprocess.run(["g++"] + FLAGS + ["-shared", "-fPIC", str(ROOT / "tests" / "cpu_seqauto.cpp"), "-o", str(out)], check=True)
    lib = ctypes.CDLL(str(out))
    lib.sa_find.argtypes = [ctypes.c_void_p, U32, U32]
    lib.sa_find.restype = ctypes.c_uint
    lib.sa_shape.argtypes = [ctypes.c_char_p, ctypes.c_int, U32, ctypes.c_void_p, U32, U32, ctypes.c_int, ctypes.c_char_p]
    return lib


def table(pieces):
    """pieces: (first sample, end, v0, v1), ascending: fade-in segments, plain ones in the gaps -- as the mixer packs a lane"""
    rows, at = [], 0
    for a, b, v0, v1 in pieces:
        if a > at:
            rows.append((1.0, 0.0, 0.0, 0.0, a, 0, 0, 0))
        rows.append((1.0, v1 - v0, float(b - a), v0, b, a, 1, 0))
        at = b
    t = np.zeros(len(rows), dtype=SEG)
    for i, r in enumerate(rows):
        t[i] = r
    return t


def expected(v, pieces):
    out = list(v)
    for a, b, v0, v1 in pieces:
        n = float(b - a)
        for k in range(min(b, len(out)) - a):
            out[a + k] = int(out[a + k] * (k * (v1 - v0) / n + v0))
    return out


def test_the_cases_inside_the_cpp_file_hold(sa):
    assert sa.sa_selfcheck() == 0


@pytest.mark.parametrize("n", [0, 1, 2, 1000])
def test_the_search_finds_the_first_segment_that_ends_past_a_sample(sa, n):
    rng = np.random.default_rng(n)
    ends = np.cumsum(rng.integers(1, 40, n)).astype(np.uint32)
    t = np.zeros(n, dtype=SEG)
    t["end"] = ends
    ptr = t.ctypes.data if n else None
    around = {0, 1, 2 ** 32 - 1} | {int(e) + d for e in ends for d in (-2, -1, 0, 1, 2) if int(e) + d >= 0}
    for s in sorted(around):
        assert sa.sa_find(ptr, n, s) == bisect.bisect_right(ends.tolist(), s), (n, s)
    assert sa.sa_find(ptr, n, 2 ** 32 - 1) == n


@pytest.mark.parametrize("width", [1, 2, 4])
def test_a_track_shaped_lane_by_lane_is_the_per_sample_expression(sa, width):
    rng = np.random.default_rng(40 + width)
    bits = 8 * width
    dtype = {1: np.int8, 2: "<i2", 4: "<i4"}[width]
    vols = [0.0, 0.25, 1.0, 0.37, 0.9, 0.5]
    n = 4099
    v = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), n, dtype=np.int64)
    v[100:110], v[2000:2010], v[3000:3004] = -(1 << (bits - 1)), (1 << (bits - 1)) - 1, -1
    data = v.astype(dtype).tobytes()
    cases = {
        "none": [],
        "whole": [(0, n, 0.9, 0.15)],
        "inside and across": [(5, 700, 0.2, 0.9), (700, 1301, 0.9, 0.1), (1400, 3000, 1.0, 0.3), (3001, n, 0.3, 1.0)],
        "on tile edges": [(1024, 2048, 0.0, 1.0), (2048, 3072, 0.5, 0.5)],
        "one-sample pieces": [(2 * i + 1, 2 * i + 2, vols[i % 6], vols[(i + 1) % 6]) for i in range(1500)],
        "three samples, one apart": [(4 * i, 4 * i + 3, vols[i % 6], vols[(2 * i + 1) % 6]) for i in range(513)],
        "past the track's end is never read": [(4000, 4200, 1.0, 0.0)],
    }
    for name, pieces in cases.items():
        t = table(pieces)
        want = np.asarray(expected(v.tolist(), pieces), dtype=np.int64).astype(dtype).tobytes()
        for tile, lane in ((2048, 8), (1024, 4), (64, 8), (16, 4), (8, 8), (4, 4)):
            out = ctypes.create_string_buffer(len(data))
            assert sa.sa_shape(data, width, n, t.ctypes.data if len(t) else None, len(t), tile, lane, out) == 0
            assert out.raw == want, (name, width, tile, lane)
        if pieces:
            assert want != data, name


def test_a_program_of_its_own_runs_the_same_cases(tmp_path):
    """the file with its ``main``, as a stand-alone build takes it (with sanitizers, where they are wanted: host code alone)"""
    exe = tmp_path / "cpu_seqauto"
    subprocess.run(["g++"] + FLAGS + ["-DSEQAUTO_MAIN", str(ROOT / "tests" / "cpu_seqauto.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "0 mismatches" in p.stdout, p.stdout + p.stderr
