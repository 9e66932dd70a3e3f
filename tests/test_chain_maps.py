"""Chain maps on the host (synthesizer_amd.chainmaps, the statement of sh_chain_map): the reference mixer's saturating chain
``mixed = audioop.add(mixed, voice, 2)`` over a range of voices is one map per value, maps of consecutive ranges compose in order,
and applied to silence (or to an existing sample) they give the live ``audioop`` chain byte for byte.  No GPU."""
import audioop

import numpy as np
import pytest

from synthesizer_amd import chainmaps as CM


def audioop_chain(rows, x0=None):
    mixed = x0 if x0 is not None else rows[0]
    for r in (rows if x0 is not None else rows[1:]):
        mixed = audioop.add(mixed, r, 2)
    return mixed


def loud_rows(rng, nvoices, n):
    """int16 voices loud enough for the running sum to hit the rails mid-chain and come back (order matters)."""
    t = np.arange(n)
    rows = []
    for v in range(nvoices):
        amp = rng.uniform(4000, 32767)
        f = rng.uniform(0.001, 0.05)
        bias = rng.uniform(-8000, 8000) if v % 3 == 0 else 0.0
        x = amp * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.3)) + bias + rng.normal(0, 300, n)
        rows.append(np.clip(x, -32768, 32767).astype(np.int16))
    return rows


def test_every_split_composes_to_the_sequential_chain():
    rng = np.random.default_rng(11)
    n, nv = 257, 23
    rows = loud_rows(rng, nv, n)
    want = audioop_chain([r.tobytes() for r in rows])
    exact = np.clip(np.sum(np.stack(rows).astype(np.int64), axis=0), -32768, 32767).astype(np.int16).tobytes()
    assert want != exact                                         # the chain saturated on the way
    maps = [CM.voice_maps(r) for r in rows]
    assert CM.apply(maps).tobytes() == want
    assert CM.apply([CM.compose_all(maps)]).tobytes() == want
    for k in range(nv + 1):                                      # two ranges, split at every position (empty ranges included)
        head = CM.compose_all(maps[:k], n)
        tail = CM.compose_all(maps[k:], n)
        assert CM.apply([head, tail]).tobytes() == want, k
        assert CM.apply([CM.compose(head, tail)]).tobytes() == want, k
    # three uneven ranges, as shards of a table over three ranks
    for a, b in ((1, 2), (5, 17), (11, 22), (0, 23)):
        parts = [CM.compose_all(maps[:a], n), CM.compose_all(maps[a:b], n), CM.compose_all(maps[b:], n)]
        assert CM.apply(parts).tobytes() == want, (a, b)


def test_maps_equal_the_chain_on_every_int16_input():
    """A composed map, applied to each of the 65 536 int16 values, equals audioop's chain continued from that value."""
    rng = np.random.default_rng(3)
    x0 = np.arange(-32768, 32768, dtype=np.int16)
    n = len(x0)
    rows = []
    for v in range(9):
        s = rng.integers(-32768, 32768, size=n, dtype=np.int64)
        s[rng.random(n) < 0.5] //= 64                            # quiet and loud samples mixed
        rows.append(s.astype(np.int16))
    want = audioop_chain([r.tobytes() for r in rows], x0=x0.tobytes())
    maps = [CM.voice_maps(r) for r in rows]
    for k in range(len(rows) + 1):
        parts = [CM.compose_all(maps[:k], n), CM.compose_all(maps[k:], n)]
        assert CM.apply(parts, x0=x0).tobytes() == want, k
    # a constant voice sample against every input: the map of one voice is the saturating add itself
    for s in (-32768, -1, 0, 1, 12345, 32767):
        m = CM.voice_maps(np.full(n, s, dtype=np.int16))
        assert CM.apply([m], x0=x0).tobytes() == audioop.add(x0.tobytes(), np.full(n, s, dtype=np.int16).tobytes(), 2)


def test_composition_is_associative_with_an_identity():
    rng = np.random.default_rng(7)
    n = 4096
    rows = loud_rows(rng, 12, n)
    maps = [CM.voice_maps(r) for r in rows]
    f, g, h = CM.compose_all(maps[:3]), CM.compose_all(maps[3:8]), CM.compose_all(maps[8:])
    left = CM.compose(CM.compose(f, g), h)
    right = CM.compose(f, CM.compose(g, h))
    assert left.tobytes() == right.tobytes()
    # the identity: the same map (a map has more than one spelling -- bounds the sum never reaches -- so compare values)
    e = CM.identity(n)
    probes = [np.full(n, x, dtype=np.int16) for x in (-32768, -32767, -1, 0, 1, 32766, 32767)]
    probes.append(rng.integers(-32768, 32768, size=n).astype(np.int16))
    for x0 in probes:
        want = CM.apply([f], x0=x0)
        assert np.array_equal(CM.apply([CM.compose(e, f)], x0=x0), want)
        assert np.array_equal(CM.apply([CM.compose(f, e)], x0=x0), want)
        assert np.array_equal(CM.apply([left], x0=x0), CM.apply([f, g, h], x0=x0))
    assert CM.apply([e]).tobytes() == bytes(2 * n)
    # the wire format: 8 bytes, (int32 add, int16 lo, int16 hi), little-endian
    assert CM.CHAIN_MAP_DTYPE.itemsize == 8
    m = CM.voice_maps(np.array([-5], dtype=np.int16))
    assert m.tobytes() == np.int32(-5).tobytes() + np.int16(-32768).tobytes() + np.int16(32767).tobytes()


def test_add_saturates_and_the_map_is_unchanged():
    """add saturates at +-2^17: 70 000 voices at full scale would carry 2.3e9 in int32; the saturated map gives the same int16 values."""
    n = 8
    x0 = np.array([-32768, -20000, -1, 0, 1, 999, 20000, 32767], dtype=np.int16)
    loud = CM.voice_maps(np.full(n, 32767, dtype=np.int16))
    quiet = CM.voice_maps(np.full(n, -3, dtype=np.int16))
    acc = CM.identity(n)
    for _ in range(70000):                                       # (composed one by one: the sum never leaves its bound)
        acc = CM.compose(acc, loud)
    assert (acc["add"] == CM.ADD_MAX).all() and (acc["lo"] == 32767).all() and (acc["hi"] == 32767).all()
    assert (CM.apply([acc], x0=x0) == 32767).all()
    tail = CM.compose(acc, quiet)
    assert (CM.apply([tail], x0=x0) == 32764).all()
    # a saturated add is the same map as the exact one on every int16 input
    big = CM.voice_maps(np.zeros(n, dtype=np.int16))
    for a in (65535, 65536, 200000, 2 ** 31 - 1, -65535, -2 ** 31):
        exact = np.clip(x0.astype(np.int64) + a, -32768, 32767)
        m = big.copy()
        m["add"] = a
        assert (CM.apply([m], x0=x0) == exact).all(), a
        sat = CM.compose(CM.identity(n), m)
        assert abs(int(sat["add"][0])) == min(abs(a), CM.ADD_MAX) and (CM.apply([sat], x0=x0) == exact).all(), a


@pytest.mark.parametrize("split", [1, 2, 3])
def test_chunked_chain_of_stereo_interleaved_values(split):
    """A stereo block is 2 * nframes maps interleaved L / R: the chain is per value, so interleaving changes nothing."""
    rng = np.random.default_rng(20 + split)
    nframes = 300
    monos = loud_rows(rng, 10 + split, nframes)
    gains = [(rng.uniform(0.2, 1.5), rng.uniform(0.2, 1.5)) for _ in monos]
    st = [audioop.tostereo(m.tobytes(), 2, gl, gr) for m, (gl, gr) in zip(monos, gains)]
    want = audioop_chain(st)
    maps = [CM.voice_maps(np.frombuffer(s, dtype=np.int16)) for s in st]
    k = len(maps) // (split + 1)
    assert CM.apply([CM.compose_all(maps[:k]), CM.compose_all(maps[k:])]).tobytes() == want


# ---- chain.hpp (the kernels' statement of the same algebra) built for the host -------------------------------------------------
@pytest.fixture(scope="module")
def ch(tmp_path_factory):
    import ctypes
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    out = tmp_path_factory.mktemp("chain") / "libchain.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", str(root / "tests" / "cpu_chain.cpp"), "-o", str(out)], check=True)
    return ctypes.CDLL(str(out))


def _ptr(a):
    import ctypes
    return a.ctypes.data_as(ctypes.c_void_p)


def _split(m):
    lo, hi = m["lo"].astype(np.uint16).astype(np.uint32), m["hi"].astype(np.uint16).astype(np.uint32)
    return np.ascontiguousarray(m["add"]), lo | (hi << 16)


def _join(add, bounds):
    out = np.empty(len(add), dtype=CM.CHAIN_MAP_DTYPE)
    out["add"] = add
    lohi = bounds.view(np.int16).reshape(-1, 2)
    out["lo"], out["hi"] = lohi[:, 0], lohi[:, 1]
    return out


def _random_maps(rng, n):
    """Maps as stored: any int32 add (the ends, +-2^17 and the int16 edges among them), lo <= hi anywhere in int16."""
    edges = np.array([-2 ** 31, 2 ** 31 - 1, -CM.ADD_MAX - 1, -CM.ADD_MAX, CM.ADD_MAX, CM.ADD_MAX + 1, -65536, -65535, 65535, 65536,
                      -32768, 32767, -1, 0, 1], dtype=np.int64)
    add = np.where(rng.random(n) < 0.3, rng.choice(edges, n), rng.integers(-2 ** 31, 2 ** 31, n))
    add = np.where(rng.random(n) < 0.3, rng.integers(-70000, 70000, n), add)
    b = np.sort(rng.integers(-32768, 32768, size=(n, 2)), axis=1)
    b[rng.random(n) < 0.1] = [-32768, 32767]
    b[rng.random(n) < 0.05, 1] = 32767
    m = np.empty(n, dtype=CM.CHAIN_MAP_DTYPE)
    m["add"], m["lo"], m["hi"] = add.astype(np.int32), b[:, 0], b[:, 1]
    return m


def test_host_build_stored_rule_equals_chainmaps(ch):
    rng = np.random.default_rng(5)
    n = 200000
    f, g = _random_maps(rng, n), _random_maps(rng, n)
    fa, fb = _split(f)
    ga, gb = _split(g)
    oa, ob = np.empty(n, np.int32), np.empty(n, np.uint32)
    ch.ch_compose_stored(_ptr(fa), _ptr(fb), _ptr(ga), _ptr(gb), ctypes_long(n), _ptr(oa), _ptr(ob))
    assert _join(oa, ob).tobytes() == CM.compose(f, g).tobytes()
    x = rng.integers(-32768, 32768, n).astype(np.int16)
    x[:4] = [-32768, 32767, 0, -1]
    out = np.empty(n, np.int16)
    ch.ch_apply_stored(_ptr(fa), _ptr(fb), _ptr(x), ctypes_long(n), _ptr(out))
    assert out.tobytes() == CM.apply([f], x0=x).tobytes()


def test_host_build_range_rule_equals_its_numpy_statement(ch):
    """The range rule saturates add once, at the end: it differs from the stored-map rule's bytes, not from its function on int16."""
    from tests.helpers import range_rule_maps
    rng = np.random.default_rng(6)
    n = 20000
    for nv in (1, 2, 9, 40):
        rows = rng.integers(-32768, 32768, size=(nv, n)).astype(np.int16)
        rows[:, : n // 4] = np.where(rng.random((nv, 1)) < 0.5, 32767, -32768)      # partial sums beyond 2^17 and back
        rows[:, n // 4: n // 2] = 32767 if nv % 2 else -32768
        rows[:, -3:] = 0
        oa, ob = np.empty(n, np.int32), np.empty(n, np.uint32)
        ch.ch_range_rows(_ptr(np.ascontiguousarray(rows)), ctypes_long(nv), ctypes_long(n), _ptr(oa), _ptr(ob))
        got = _join(oa, ob)
        assert got.tobytes() == range_rule_maps(rows, n).tobytes(), nv
        assert CM.apply([got]).tobytes() == CM.apply([CM.voice_maps(r) for r in rows]).tobytes(), nv
    # add 200 000 then -100 000: the range rule stores 100 000, the stored-map rule 31 072
    rows = np.array([[32767]] * 6 + [[3398]] + [[-32768]] * 3 + [[-1696]], dtype=np.int16)
    oa, ob = np.empty(1, np.int32), np.empty(1, np.uint32)
    ch.ch_range_rows(_ptr(rows), ctypes_long(len(rows)), ctypes_long(1), _ptr(oa), _ptr(ob))
    assert int(oa[0]) == 100000
    two = np.array([200000, -100000], dtype=np.int32)
    b = _split(CM.identity(2))[1]
    ch.ch_compose_stored(_ptr(two[:1].copy()), _ptr(b[:1].copy()), _ptr(two[1:].copy()), _ptr(b[1:].copy()), ctypes_long(1), _ptr(oa), _ptr(ob))
    assert int(oa[0]) == 31072


def ctypes_long(v):
    import ctypes
    return ctypes.c_long(v)
