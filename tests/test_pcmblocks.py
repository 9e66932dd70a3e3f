"""csrc/pcmblocks.hpp -- the block geometry of sh_pcm_level_blocks, the split of a block into parts and the arithmetic of a call -- built
for the host with g++, against Python integers: the number of blocks of a call and the frames each counts against a brute-force count
(blocks of 1, 7, 1000 and 2^33 frames, origins up to 2^32 + 3), the parts of a block without gap or overlap, a host loop built from the
header's functions against ``audioop.max`` and integer sums at all four widths, and the binding's mirror of PART_SAMPLES.
tests/cpu_pcmblocks.cpp also builds as a program of its own (-DPCMBLOCKS_MAIN), which is built and run once here without a sanitizer.
No GPU."""
import audioop
import ctypes as C
import random
import subprocess
from pathlib import Path

import pytest

from synthesizer_amd import _native as N

ROOT = Path(__file__).resolve().parents[1]


class Row(C.Structure):
    _fields_ = [("peak", C.c_uint32 * 2), ("sq_hi", C.c_uint64 * 2), ("sq_lo", C.c_uint64 * 2)]


@pytest.fixture(scope="module")
def pb(tmp_path_factory):
    out = tmp_path_factory.mktemp("pcmblocks") / "libpcmblocks.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", str(ROOT / "tests" / "cpu_pcmblocks.cpp"), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    u64, u32 = C.c_uint64, C.c_uint32
    lib.pb_part_samples.restype = lib.pb_slot_shift.restype = u32
    lib.pb_nblocks.restype = lib.pb_longest.restype = lib.pb_parts_of.restype = lib.pb_row_at.restype = u64
    lib.pb_part_samples.argtypes = []
    lib.pb_nblocks.argtypes = lib.pb_longest.argtypes = [u64, u64, u64]
    lib.pb_range.argtypes = [u64, u64, u64, u64, C.POINTER(u64), C.POINTER(u64)]
    lib.pb_parts_of.argtypes = lib.pb_slot_shift.argtypes = [u64]
    lib.pb_part.argtypes = [u64, u64, C.POINTER(u64), C.POINTER(u64)]
    lib.pb_row_at.argtypes = [u64, u32, u32]
    lib.pb_host_rows.argtypes = [C.c_char_p, C.c_int, u64, u32, u32, u64, u64, u64, C.POINTER(Row)]
    lib.pb_range.restype = lib.pb_part.restype = lib.pb_host_rows.restype = None
    return lib


def brute_blocks(origin, n, B):
    """the frames [a, b) of every grid block that holds a frame of [origin, origin + n), found block by block: no formula of the header's"""
    out, k = [], origin // B
    while n and k * B < origin + n:
        a, b = max(k * B, origin), min((k + 1) * B, origin + n)
        if a < b:
            out.append((a, b))
        k += 1
    return out


def got_blocks(pb, origin, n, B):
    out = []
    for j in range(pb.pb_nblocks(origin, n, B)):
        a, b = C.c_uint64(), C.c_uint64()
        pb.pb_range(j, origin, n, B, C.byref(a), C.byref(b))
        out.append((a.value, b.value))
    return out


@pytest.mark.parametrize("B", [1, 7, 1000, 2 ** 33])
def test_the_blocks_of_a_call_against_a_brute_force_count(pb, B):
    for origin in (0, 5, B - 1, 2 ** 32 + 3):
        for n in (0, 1, B, B + 1, 3 * B - 2):
            want = brute_blocks(origin, n, B)
            assert pb.pb_nblocks(origin, n, B) == len(want) == ((origin + n - 1) // B - origin // B + 1 if n else 0), (origin, n)
            assert got_blocks(pb, origin, n, B) == want, (origin, n)
            assert sum(b - a for a, b in want) == n and all(a // B == (b - 1) // B for a, b in want)      # they tile the call, none crosses an edge
            if B <= 7 and n:                                # frame by frame as well
                assert sorted({(origin + i) // B for i in range(n)}) == [a // B for a, _b in want]
            if want:
                assert pb.pb_longest(origin, n, B) == max(b - a for a, b in want), (origin, n)


def test_a_block_that_lies_whole_inside_two_calls_reads_the_same_range(pb):
    B = 1000
    assert (3000, 4000) in got_blocks(pb, 2500, 2000, B) and (3000, 4000) in got_blocks(pb, 7, 9000, B) and (3000, 4000) in got_blocks(pb, 3000, 1000, B)
    assert pb.pb_row_at(2 ** 33, 41, 40) == 2 ** 33 * 41 + 40


def test_the_parts_tile_a_blocks_range_without_gap_or_overlap(pb):
    P = pb.pb_part_samples()
    assert P == N.PCM_PART_SAMPLES and P >= 4096 and P % 2 == 0 and P >= max(N.SEQ_TILE_SAMPLES.values())      # a song tile is one part
    for samples in (1, 2, 2047, 2048, P - 1, P, P + 1, 2 * P, 3 * P + 5, 6 * P + 10, 17 * P - 1):
        nparts, shift = pb.pb_parts_of(samples), pb.pb_slot_shift(samples)
        assert nparts == -(-samples // P) and 2 ** shift >= nparts and (shift == 0 or 2 ** (shift - 1) < nparts)
        at = 0
        for p in range(2 ** shift + 1):
            s0, s1 = C.c_uint64(), C.c_uint64()
            pb.pb_part(samples, p, C.byref(s0), C.byref(s1))
            if p < nparts:
                assert s0.value == at and at < s1.value <= at + P and s0.value % 2 == 0, (samples, p)
                at = s1.value
            else:
                assert s0.value == s1.value == samples, (samples, p)      # a slot behind the last part: empty
        assert at == samples


def pcm(rng, n, width):
    """n samples with both rails among them, as raw bytes and as ints"""
    lo, hi = -(1 << (8 * width - 1)), (1 << (8 * width - 1)) - 1
    values = [rng.choice([lo, hi, 0, rng.randrange(lo, hi + 1), rng.randrange(lo, hi + 1)]) for _ in range(n)]
    return b"".join(v.to_bytes(width, "little", signed=True) for v in values), values


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_a_host_loop_of_the_headers_functions_equals_the_brute_force_rows(pb, width):
    rng = random.Random(100 + width)
    P = pb.pb_part_samples()
    for nch, nplanes, n, B, origin, gap in ((1, 1, 257, 64, 5, 0), (2, 1, 257, 64, 5, 0), (2, 3, 100, 7, 999, 3), (1, 3, 33, 1, 0, 1), (2, 1, 50, 1000, 990, 0),
                                            (1, 1, 3 * P + 5, 2 * P + 1, 11, 0), (2, 2, P + 3, P, 1, 5)):
        plane = n * nch + gap
        raw, values = pcm(rng, nplanes * plane, width)
        blocks = brute_blocks(origin, n, B)
        table = (Row * max(1, len(blocks) * nplanes))()
        pb.pb_host_rows(raw, width, n, nch, nplanes, plane, origin, B, table)
        for j, (a, b) in enumerate(blocks):
            for r in range(nplanes):
                got = table[j * nplanes + r]
                for c in range(2):
                    xs = values[r * plane + (a - origin) * nch + c:r * plane + (b - origin) * nch:nch] if c < nch else []
                    chan = b"".join(x.to_bytes(width, "little", signed=True) for x in xs)
                    assert got.peak[c] == (audioop.max(chan, width) if xs else 0), (nch, nplanes, j, r, c)
                    assert (got.sq_hi[c] << 32) + got.sq_lo[c] == sum(int(x) ** 2 for x in xs), (nch, nplanes, j, r, c)
                    assert width >= 3 or got.sq_hi[c] == 0     # one sum at widths 1 and 2


def test_the_file_is_a_program_of_its_own_as_well(tmp_path):
    exe = tmp_path / "cpu_pcmblocks"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DPCMBLOCKS_MAIN", str(ROOT / "tests" / "cpu_pcmblocks.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("pcmblocks: ") and p.stdout.strip().endswith("ok"), p.stdout + p.stderr
