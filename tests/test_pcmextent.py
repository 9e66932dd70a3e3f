"""csrc/pcmextent.hpp -- the row of sh_pcm_extent_blocks, its identity, take, fold and the mono rule, and the whole call as a host loop
over pcmblocks.hpp's geometry -- built for the host with g++, against the live ``audioop.minmax`` on each channel's samples,
de-interleaved in Python, at widths 1 to 4: every block of windows that are no multiple of the block, blocks of one frame and blocks
of several parts, one plane and three with a gap between them; the same table from parts taken backwards; planes of one sign, which an
accumulator that starts at 0 misses.  tests/cpu_pcmextent.cpp also builds as a program of its own (-DPCMEXTENT_MAIN), which is built
and run once here without a sanitizer.  No GPU."""
import audioop
import ctypes as C
import random
import subprocess
from pathlib import Path

import pytest

from synthesizer_amd import _native as N

ROOT = Path(__file__).resolve().parents[1]
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


class Row(C.Structure):
    _fields_ = [("lo", C.c_int32 * 2), ("hi", C.c_int32 * 2)]


@pytest.fixture(scope="module")
def pe(tmp_path_factory):
    out = tmp_path_factory.mktemp("pcmextent") / "libpcmextent.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", str(ROOT / "tests" / "cpu_pcmextent.cpp"), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    u64, u32 = C.c_uint64, C.c_uint32
    lib.pe_row_bytes.restype, lib.pe_row_bytes.argtypes = u32, []
    lib.pe_identity.argtypes = [C.POINTER(Row)]
    lib.pe_take.argtypes = [C.POINTER(Row), u64, u32, C.c_int32]
    lib.pe_fold.argtypes = [C.POINTER(Row), C.POINTER(Row)]
    lib.pe_stored.argtypes = [C.POINTER(Row), u32]
    lib.pe_host_rows.argtypes = lib.pe_host_rows_backwards.argtypes = [C.c_char_p, C.c_int, u64, u32, u32, u64, u64, u64, C.POINTER(Row)]
    for f in (lib.pe_identity, lib.pe_take, lib.pe_fold, lib.pe_stored, lib.pe_host_rows, lib.pe_host_rows_backwards):
        f.restype = None
    return lib


def fields(row):
    return (row.lo[0], row.lo[1]), (row.hi[0], row.hi[1])


def blocks_of(origin, n, B):
    return [(max(k * B, origin), min((k + 1) * B, origin + n)) for k in range(origin // B, (origin + n - 1) // B + 1)] if n else []


def pack(values, width):
    return b"".join(int(v).to_bytes(width, "little", signed=True) for v in values)


def want_row(values, width, nch):
    """audioop.minmax per channel of one block's interleaved samples; a mono input's channel 1 reads (0, 0)"""
    lo, hi = [0, 0], [0, 0]
    for c in range(nch):
        lo[c], hi[c] = audioop.minmax(pack(values[c::nch], width), width)
    return tuple(lo), tuple(hi)


def test_rows_are_16_bytes_and_the_bindings_mirror_them(pe):
    assert pe.pe_row_bytes() == 16 == C.sizeof(Row) == C.sizeof(N.PcmExtent) == N.PCM_EXTENT_DTYPE.itemsize
    assert N.PCM_EXTENT_DTYPE.names == ("lo", "hi") and [N.PCM_EXTENT_DTYPE.fields[k][1] for k in ("lo", "hi")] == [0, 8]
    assert [(name, C.sizeof(kind)) for name, kind in N.PcmExtent._fields_] == [("lo", 8), ("hi", 8)]


def test_the_identity_is_what_audioop_gives_for_no_sample_and_folds_away(pe):
    ident = Row()
    pe.pe_identity(C.byref(ident))
    assert fields(ident) == ((INT32_MAX, INT32_MAX), (INT32_MIN, INT32_MIN))
    for width in (1, 2, 3, 4):
        assert audioop.minmax(b"", width) == (INT32_MAX, INT32_MIN)
    row = Row((-5, 7), (-3, 11))
    pe.pe_fold(C.byref(row), C.byref(ident))
    assert fields(row) == ((-5, 7), (-3, 11))                   # folding the identity changes nothing ...
    pe.pe_fold(C.byref(ident), C.byref(row))
    assert fields(ident) == ((-5, 7), (-3, 11))                 # ... and the identity takes whatever is folded into it
    a, b = Row((-5, 7), (-3, 11)), Row((2, -9), (-4, 12))
    ab, ba = Row((-5, 7), (-3, 11)), Row((2, -9), (-4, 12))
    pe.pe_fold(C.byref(ab), C.byref(b))
    pe.pe_fold(C.byref(ba), C.byref(a))
    assert fields(ab) == fields(ba) == ((-5, -9), (-3, 12))     # min of lo, max of hi, either way round


def test_take_sends_a_sample_to_its_channel_and_the_mono_rule_is_applied_where_a_row_is_stored(pe):
    stereo = Row()
    pe.pe_identity(C.byref(stereo))
    for s, x in enumerate([-7, 100, -2, 50, INT32_MIN, INT32_MAX]):
        pe.pe_take(C.byref(stereo), s, 2, x)
    assert fields(stereo) == ((INT32_MIN, 50), (-2, INT32_MAX))
    pe.pe_stored(C.byref(stereo), 2)
    assert fields(stereo) == ((INT32_MIN, 50), (-2, INT32_MAX))   # a stereo row is stored as it is
    mono = Row()
    pe.pe_identity(C.byref(mono))
    for s, x in enumerate([-7, -100, -2]):                      # odd positions too: all of them channel 0
        pe.pe_take(C.byref(mono), s, 1, x)
    assert fields(mono) == ((-100, INT32_MAX), (-2, INT32_MIN))  # the fold leaves channel 1 at the identity
    pe.pe_stored(C.byref(mono), 1)
    assert fields(mono) == ((-100, 0), (-2, 0))                  # the table reads lo[1] = hi[1] = 0


def pcm(rng, n, width, sign=0):
    """n samples with both rails among them (sign 0), or strictly negative (-1) or strictly positive (+1) ones"""
    lo, hi = -(1 << (8 * width - 1)), (1 << (8 * width - 1)) - 1
    if sign < 0:
        return [rng.choice([lo, -1, rng.randrange(lo, 0)]) for _ in range(n)]
    if sign > 0:
        return [rng.choice([hi, 1, rng.randrange(1, hi + 1)]) for _ in range(n)]
    return [rng.choice([lo, hi, 0, rng.randrange(lo, hi + 1), rng.randrange(lo, hi + 1)]) for _ in range(n)]


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_the_host_loop_equals_audioop_minmax_per_block_and_channel_forwards_and_backwards(pe, width):
    rng = random.Random(200 + width)
    P = N.PCM_PART_SAMPLES
    # the GPU tests' shapes that fit a host loop: the grid, the alignment window, three planes with a gap, blocks of three parts and a
    # few samples, one frame, a block longer than the window
    cases = [(nch, 1, 4097, B, origin, 0) for nch in (1, 2) for B in (1, 7, 64, 1000, 5000) for origin in (0, 5, 999)]
    cases += [(nch, 1, 203, 48, 7, 0) for nch in (1, 2)] + [(nch, 3, 333, 100, 250, 3) for nch in (1, 2)]
    cases += [(1, 1, 2 * (3 * P + 5) + 1000, 3 * P + 5, 0, 0), (1, 3, 2 * (3 * P + 6) + 1000, 3 * P + 6, 0, 3), (2, 1, 2 * ((3 * P + 8) // 2) + 1000, (3 * P + 8) // 2, 0, 0)]
    cases += [(nch, 1, 1, 64, 2 ** 40 + 1, 0) for nch in (1, 2)] + [(nch, 1, 500, 10 ** 9, 10 ** 9 - 100, 0) for nch in (1, 2)]
    for k, (nch, nplanes, n, B, origin, gap) in enumerate(cases):
        if width in (1, 3) and n > 3 * P:                       # (blocks of several parts: the widths of the GPU case, and fewer Python loops)
            continue
        plane = n * nch + gap
        values = pcm(rng, nplanes * plane, width, sign=(0, -1, 1)[k % 3])
        raw = pack(values, width)
        blocks = blocks_of(origin, n, B)
        table, back = (Row * (len(blocks) * nplanes))(), (Row * (len(blocks) * nplanes))()
        pe.pe_host_rows(raw, width, n, nch, nplanes, plane, origin, B, table)
        pe.pe_host_rows_backwards(raw, width, n, nch, nplanes, plane, origin, B, back)
        for j, (a, b) in enumerate(blocks):
            for r in range(nplanes):
                want = want_row(values[r * plane + (a - origin) * nch:r * plane + (b - origin) * nch], width, nch)
                assert fields(table[j * nplanes + r]) == want, (nch, nplanes, n, B, origin, j, r)
                assert fields(back[j * nplanes + r]) == want, (nch, nplanes, n, B, origin, j, r)
        if k % 3 == 1:
            assert all(table[i].hi[0] < 0 for i in range(len(table)))       # strictly negative planes: hi < 0
        if k % 3 == 2:
            assert all(table[i].lo[0] > 0 for i in range(len(table)))       # strictly positive planes: lo > 0


def test_the_file_is_a_program_of_its_own_as_well(tmp_path):
    exe = tmp_path / "cpu_pcmextent"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DPCMEXTENT_MAIN", str(ROOT / "tests" / "cpu_pcmextent.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("pcmextent: ") and p.stdout.strip().endswith("ok"), p.stdout + p.stderr
