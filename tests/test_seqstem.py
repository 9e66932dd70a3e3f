"""csrc/seqstem.hpp -- the geometry of the stems of a compiled song: the planes' row order, the 64-bit address of a plane's sample, the
three refusals of a call's geometry at their boundaries, the all-planes-aligned predicate, the span of all planes and the stride that
keeps the store's fast path -- built for the host with g++, against Python integers.  tests/cpu_seqstem.cpp also builds as a program of
its own (-DSEQSTEM_MAIN), which is built and run once here without a sanitizer.  No GPU."""
import ctypes as C
import random
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
OK, PLANES, STRIDE, EXTENT = 0, 1, 2, 3
M64 = (1 << 64) - 1
LONGEST = 2 ** 32 - 65536                                   # samples of the longest song


@pytest.fixture(scope="module")
def st(tmp_path_factory):
    out = tmp_path_factory.mktemp("seqstem") / "libseqstem.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", str(ROOT / "tests" / "cpu_seqstem.cpp"), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    u32, u64 = C.c_uint32, C.c_uint64
    for name, args, res in (("st_nrows", [u32, u32], u32), ("st_track_row", [u32], u32), ("st_master_row", [u32], u32), ("st_group_row", [u32, u32], u32),
                            ("st_max_rows", [], u32), ("st_stride_bytes", [u64, u32], u64), ("st_plane_offset", [u32, u64], u64),
                            ("st_address", [u64, u32, u64, u64, u32], u64), ("st_check", [u32, u32, u32, u64, u64, u64, u64], C.c_int),
                            ("st_span", [u32, u64, u64], u64), ("st_overlaps", [u64, u64, u64, u64], C.c_int), ("st_aligned", [u64, u64], C.c_int),
                            ("st_plane_samples_for", [u64, u32], u64)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, res
    return lib


def test_the_planes_stand_in_the_meter_rows_order(st):
    assert st.st_max_rows() == 41 == st.st_nrows(32, 8)
    for ntracks in (1, 3, 6, 32):
        for ngroups in (0, 1, 8):
            rows = [st.st_track_row(t) for t in range(ntracks)] + [st.st_master_row(ntracks)] + [st.st_group_row(ntracks, g) for g in range(ngroups)]
            assert rows == list(range(ntracks + 1 + ngroups)) and len(rows) == st.st_nrows(ntracks, ngroups)


def test_the_address_is_formed_in_64_bits(st):
    rng = random.Random(17)
    for _ in range(2000):
        width = rng.choice([1, 2, 3, 4])
        biased, r, plane, s = rng.randrange(1 << 64), rng.randrange(41), rng.randrange(1 << 33), rng.randrange(1 << 32)
        stride = st.st_stride_bytes(plane, width)
        assert stride == plane * width and st.st_plane_offset(r, stride) == r * stride
        assert st.st_address(biased, r, stride, s, width) == (biased + r * stride + s * width) & M64
    # 41 planes of the longest song at width 4: plane_samples * nplanes * width is past 2^32 bytes (2^39.4), and so is one plane
    stride = st.st_stride_bytes(LONGEST, 4)
    assert stride == 4 * LONGEST > 1 << 32 and st.st_plane_offset(40, stride) == 40 * 4 * LONGEST > 1 << 39
    assert st.st_address(1 << 20, 40, stride, LONGEST - 1, 4) == (1 << 20) + 40 * 4 * LONGEST + 4 * (LONGEST - 1)
    # song samples past 2^31: the base is biased by first_sample and may have wrapped below zero; the sum comes back into the buffer
    buffer, first = 0x7F0000001000, 3_000_000_000
    for width in (1, 2, 3, 4):
        biased = (buffer - first * width) & M64
        stride = st.st_stride_bytes(1 << 31, width)
        for r in (0, 1, 40):
            assert st.st_address(biased, r, stride, first + 5, width) == buffer + r * stride + 5 * width
    assert st.st_address((16 - 4 * 4_000_000_000) & M64, 2, 64, 4_000_000_000, 4) == 16 + 128      # a base that wrapped


def test_the_three_refusals_at_their_boundaries(st):
    # PLANES: the count is ntracks + 1 + ngroups, nothing else
    for nplanes, want in ((9, OK), (8, PLANES), (10, PLANES), (6, PLANES), (0, PLANES)):
        assert st.st_check(nplanes, 6, 2, 100, 100, 0, 900) == want
    # STRIDE: planes at least a window apart
    assert st.st_check(9, 6, 2, 100, 100, 0, 900) == OK and st.st_check(9, 6, 2, 99, 100, 0, 900) == STRIDE
    assert st.st_check(9, 6, 2, 0, 0, 0, 0) == OK and st.st_check(9, 6, 2, 0, 1, 0, 900) == STRIDE
    # EXTENT: the last plane's last sample is the buffer's last, or one past it
    for out_sample, plane, n, have, want in ((0, 100, 100, 900, OK), (0, 100, 100, 899, EXTENT), (1, 100, 100, 900, EXTENT), (1, 100, 100, 901, OK),
                                             (0, 124, 100, 8 * 124 + 100, OK), (0, 124, 100, 8 * 124 + 99, EXTENT), (7, 124, 100, 8 * 124 + 107, OK),
                                             (901, 0, 0, 900, EXTENT), (900, 0, 0, 900, OK), (0, 113, 0, 8 * 113, OK), (0, 113, 0, 8 * 113 - 1, EXTENT)):
        assert st.st_check(9, 6, 2, plane, n, out_sample, have) == want, (out_sample, plane, n, have)
    # the order: PLANES in front of STRIDE in front of EXTENT
    assert st.st_check(8, 6, 2, 99, 100, 0, 10) == PLANES and st.st_check(9, 6, 2, 99, 100, 0, 10) == STRIDE
    # past 2^32 bytes and past 2^64: 41 planes of the longest song at width 4 fit a buffer of exactly that many samples and no smaller one;
    # a stride whose product with the plane count passes 2^64 is refused, not wrapped
    need = 40 * LONGEST + LONGEST
    assert need * 4 > 1 << 39
    assert st.st_check(41, 32, 8, LONGEST, LONGEST, 0, need) == OK and st.st_check(41, 32, 8, LONGEST, LONGEST, 0, need - 1) == EXTENT
    assert st.st_check(41, 32, 8, LONGEST, LONGEST, 5, need + 4) == EXTENT and st.st_check(41, 32, 8, LONGEST, LONGEST, 5, need + 5) == OK
    assert st.st_check(41, 32, 8, 1 << 60, 10, 0, M64) == EXTENT              # 40 * 2^60 wraps to a small number
    assert st.st_check(41, 32, 8, (1 << 64) // 40 + 1, 10, 0, M64) == EXTENT
    rng = random.Random(23)
    for _ in range(4000):
        ntracks, ngroups = rng.randrange(1, 33), rng.randrange(0, 9)
        nplanes = ntracks + 1 + ngroups if rng.random() < 0.8 else rng.randrange(0, 50)
        n = rng.choice([rng.randrange(0, 3000), rng.randrange(0, 1 << 33)])
        plane = n + rng.randrange(0, 30) if rng.random() < 0.8 else rng.randrange(0, n + 1)
        out_sample = rng.randrange(0, 50)
        need = out_sample + max(nplanes - 1, 0) * plane + n
        have = max(0, need + rng.choice([-1, 0, 0, 1, 1000, -1000]))
        want = PLANES if nplanes != ntracks + 1 + ngroups else STRIDE if plane < n else EXTENT if need > have else OK
        assert st.st_check(nplanes, ntracks, ngroups, plane, n, out_sample, have) == want, (nplanes, ntracks, ngroups, plane, n, out_sample, have)


def test_every_plane_is_aligned_exactly_where_the_base_and_the_stride_are(st):
    rng = random.Random(29)
    for _ in range(3000):
        width = rng.choice([1, 2, 3, 4])
        base = rng.randrange(1 << 48) & ~15 if rng.random() < 0.7 else rng.randrange(1 << 48)
        plane = rng.randrange(1, 5000) * rng.choice([1, 2, 4, 8, 16])
        stride = st.st_stride_bytes(plane, width)
        every = all((base + r * stride) % 16 == 0 for r in range(41))
        assert bool(st.st_aligned(base, stride)) == every, (base, stride)
    assert st.st_aligned(32, 16) and st.st_aligned(0, 0) and not st.st_aligned(32, 8) and not st.st_aligned(2, 16) and not st.st_aligned(32, 2 * 100 + 2 * 24 + 2)
    # the stride a caller picks: the smallest one past the window that keeps every plane aligned
    for width in (1, 2, 3, 4):
        for n in list(range(0, 70)) + [LONGEST - 3, (1 << 31) + 1]:
            p = st.st_plane_samples_for(n, width)
            assert p >= n and (p * width) % 16 == 0 and st.st_aligned(4096, st.st_stride_bytes(p, width))
            assert all((q * width) % 16 for q in range(n, p)), (width, n, p)


def test_the_span_of_all_planes_and_what_it_overlaps(st):
    assert st.st_span(9, 124, 100) == 8 * 124 + 100 and st.st_span(9, 100, 100) == 900 and st.st_span(1, 7, 5) == 5
    assert st.st_span(9, 124, 0) == 0 and st.st_span(0, 124, 100) == 0
    assert st.st_span(41, LONGEST, LONGEST) == 41 * LONGEST > 1 << 37
    # a source in the gap between two planes is inside the span; one that ends where the span starts, or starts where it ends, is not
    a0 = 1 << 33
    a1 = a0 + 2 * st.st_span(9, 124, 100)
    gap = a0 + 2 * 100
    assert st.st_overlaps(a0, a1, gap, gap + 2 * 24) and st.st_overlaps(a0, a1, a1 - 1, a1 + 50) and st.st_overlaps(a0, a1, a0 - 50, a0 + 1)
    assert not st.st_overlaps(a0, a1, a1, a1 + 50) and not st.st_overlaps(a0, a1, a0 - 50, a0) and st.st_overlaps(a0, a1, a0 - 50, a1 + 50)


def test_the_file_is_a_program_of_its_own_as_well(tmp_path):
    exe = tmp_path / "cpu_seqstem"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DSEQSTEM_MAIN", str(ROOT / "tests" / "cpu_seqstem.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("seqstem: ") and p.stdout.strip().endswith("ok"), p.stdout + p.stderr
