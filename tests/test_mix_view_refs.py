"""The references and case tables of tests/test_gpu_mix_views.py, tests/test_gpu_resample_views.py and
tests/test_gpu_quantize_views.py on their own (no GPU): the tables reach what those files promise, so that a pass on the device is the
kernels' doing and not a gap in the inputs."""
import numpy as np
import pytest

from tests import test_gpu_mix_views as M
from tests import test_gpu_quantize_views as Q
from tests import test_gpu_resample_views as R
from tests.seqcases import ROOT, lists, named, rows_of
from tests.seqref import discriminates
from tests.test_gpu_pcm_views import residues
from tests.test_ratecv_plan import rc  # noqa: F401  (the fixture: tests/cpu_ratecv.cpp built with g++)

LANE = {1: 4, 2: 8, 3: 4, 4: 4}


def test_the_route_table_names_every_route_and_the_host_plan_agrees(rc):  # noqa: F811
    assert {c[0] for c in R.CASES} == set(R.ROUTES) - {"NONE"}
    src = ROOT / "synthesizer_amd" / "csrc" / "ratecv.hpp"
    text = src.read_text()
    enum = text[text.index("enum Route {"):]
    enum = enum[:enum.index("};")]
    names = [line.split(",")[0].strip() for line in enum.splitlines()[1:] if line.strip().startswith("RT_")]
    assert names == ["RT_" + k for k, _v in sorted(R.ROUTES.items(), key=lambda kv: kv[1])]           # the numbers are the enum's
    for case in R.CASES:
        route, width, is_float, nch, inrate, outrate = case
        counts = R.frame_counts(rc, case)
        if case is R.BELOW_PERIOD:
            assert counts == [12345] and any(c[0] == "PERIOD" and c[1:] == case[1:] for c in R.CASES)      # the same layout and rates reach PERIOD
        elif route == "PERIOD":
            assert len(counts) == 2 and 40001 in counts
        else:
            assert {1, 2, 9, 20011} <= set(counts) and len(counts) == 6
        for frames in counts:
            if R.expected_route(case, frames):
                assert R.host_plan(rc, width, is_float, nch, inrate, outrate, True, frames)[0] == R.ROUTES[R.expected_route(case, frames)], (R.case_id(case), frames)
            assert R.host_plan(rc, width, is_float, nch, inrate, outrate, False, frames)[0] == R.ROUTES["GENERIC"], (R.case_id(case), frames)
        if route == "PERIOD":                               # at least three interior chunks and a tail (a whole sample's head is empty: c0 = 0)
            for frames in counts:
                p = R.host_plan(rc, width, is_float, nch, inrate, outrate, True, frames)
                m_base, m_end, c0, c1, head_end, tail_begin = p[9], p[10], p[12], p[13], p[17], p[18]
                assert c1 - c0 >= 3 and m_base <= head_end < tail_begin < m_end, (R.case_id(case), frames, p)


def test_the_gather_batches_have_the_composition_claimed():
    case = M.direct_case()
    n = M.DIRECT_N
    assert len(case) == 9 and -(-n // 512) >= 1536 and n % 8 == 3
    on_grid = lambda c: (c[2] + 2 * c[1]) % 16 == 0
    whole = lambda c: c[0] >= n
    first, second, rest = case[:4], case[4:8], case[8:]
    assert sum(1 for c in first if not on_grid(c)) == 1
    inside = [c for c in first if on_grid(c) and not whole(c)]
    assert len(inside) == 1 and inside[0][0] % 512 and 0 < inside[0][0] < n          # it ends inside a wave's 1 KB
    assert sum(1 for c in first if on_grid(c) and whole(c)) == 2
    assert all(on_grid(c) and whole(c) for c in second)
    assert len(rest) == 1 and not on_grid(rest[0])
    for nsrc in (5, 64, 70):
        small = M.small_case(nsrc, 1024 + M.TAIL)
        assert len(small) == nsrc and {c[1] for c in small} == set(M.SRC_OFFS)
        assert any(c[0] == 0 for c in small) and any(c[0] == 1024 + M.TAIL for c in small)
        assert sum(1 for c in small if c[0]) <= 64 or nsrc == 70                     # 64: the table still travels in the arguments
    assert {(a % 16 == 0, o % 16 == 0) for a, o in M.CHAIN_PAIRS} == {(True, True), (True, False), (False, True), (False, False)}
    assert {(a % 16 == 0, o % 16 == 0) for a, o in M.CHAIN_PAIRS_LONG} == {(True, True), (True, False), (False, True), (False, False)}
    for pairs in (M.CHAIN_PAIRS, M.CHAIN_PAIRS_LONG):
        assert {a for a, _o in pairs} == {o for _a, o in pairs} == set(M.CHAIN_RESIDUES)
        assert all(a != o for a, o in pairs if a and o)
    shapes = {(nv < 64, -(-n // 512)) for _id, nv, n, _long in M.CHAIN_SHAPES}
    assert {(True, 641), (True, 1537), (False, 513)} <= shapes and all(n % 8 == 3 for _id, _nv, n, _long in M.CHAIN_SHAPES)


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_every_track_list_ends_on_the_last_sample_and_has_an_event_shorter_than_a_lane(width):
    sources, base, A, B, C_ = lists(width)[:5]
    ns = len(base) // width
    assert ns % 8 and (ns + M.SURPLUS) * width + 2 * M.PCM_GUARD < 1 << 20
    for lst in (A, B, C_):
        rows = rows_of(lst, sources, width)
        assert any(d + n == ns for d, n, *_ in rows) and any(0 < n < LANE[width] for _d, n, *_ in rows)
    for kind in ("loop", "rev"):
        instruments, base2, events, want, spans = M.shaped(kind, width)
        assert base2 == base and len(want) == len(base)
        assert any(d + n == ns for d, n in spans) and any(0 < n < LANE[width] for _d, n in spans)
        tile = 2048 if width == 2 else 1024
        assert any(d < tile < d + n for d, n in spans)                                   # across a tile edge
        full = named(instruments, [e + (None, False) if len(e) == 8 else e for e in events])
        assert any(e[7] is not None and e[4] is not None for e in full)                # looped and resampled
        assert any(e[6] is not None for e in full) or width == 3                       # an envelope
        if kind == "rev":
            assert any(e[9] and e[8] is not None for e in full)                        # reversed from a region
            discriminates(want, full, width, M.RATE, 2, "rev", base)
    assert {r % 16 for r in residues(width)} >= {0, width, 8, 16 - width}


def test_the_quantise_reference_and_its_inputs():
    for ftype in (np.float32, np.float64):
        for width in Q.WIDTHS:
            for n in Q.LENGTHS:
                v = Q.values(ftype, width, n)
                p = Q.scale_of(width) * v.astype(np.float64)
                lo, hi = -(1 << (8 * width - 1)), (1 << (8 * width - 1)) - 1
                assert v.dtype == ftype and len(v) == n and np.all((np.trunc(p) >= lo) & (np.trunc(p) <= hi))        # nothing overflows
                assert Q.reference(v, width) == np.array([int(Q.scale_of(width) * float(x)) for x in v], dtype=Q.INT[width]).tobytes()
    assert not -(1 << 31) <= Q.scale_of(1) * Q.BAD <= (1 << 31) - 1
    assert np.float32(Q.BAD) == np.float32(1e30) and np.isfinite(np.float32(Q.BAD))
    v = np.array([Q.BAD, -Q.BAD, np.nan, np.inf, 0.5], dtype=np.float32)
    assert np.frombuffer(Q.reference_clip(v, 40000.0), dtype="<i2").tolist() == [32767, -32768, 0, 32767, 20000]
    assert {0, 1, 3, 4, 5, 1023, 1024, 1025, 2048 + 3} == set(Q.LENGTHS)
