"""Chain maps on the GPU: a voice table split into contiguous shards, each a VoiceBank of its own, each leaving the chain's map per
value (``mixdown_i16_parts_device``: sh_bank_mixdown_i16_parts, sh_mix_chain_i16_parts, sh_mix_chain_pan_i16_parts), the maps
applied in order (sh_chain_parts_apply) -- byte for byte the whole bank's ``mixdown_i16_device`` / ``mixdown_stereo_i16_device`` and
the live ``audioop`` chain over the int16 rows.  Fused and rows stretches, filter graphs, saturating stretches, odd and long blocks,
late windows, a chain continued from an existing Sample, tables beyond one bank's 32 768 voices, and the 1-rank RCCL gather."""
import audioop

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 48000


def audioop_chain(rows_bytes, x0=None):
    mixed = rows_bytes[0] if x0 is None else x0
    for r in (rows_bytes[1:] if x0 is None else rows_bytes):
        mixed = audioop.add(mixed, r, 2)
    return mixed


def _fused(N):
    return N.lib().sh_get_option(N.SH_INFO_LAST_MIXDOWN_FUSED)


def _split(voices, gains, sizes):
    from synthesizer_amd.mixer import VoiceBank
    assert sum(sizes) == len(voices)
    out, lo = [], 0
    for s in sizes:
        out.append(VoiceBank(voices[lo:lo + s], gains=gains[lo:lo + s]))
        lo += s
    return out


def _sharded(shards, n, start, stereo=False, x0=None):
    """Apply the shards' maps in order (list form: one buffer per shard) -> bytes."""
    from synthesizer_amd.mixer import apply_chain_parts
    nvalues = n * (2 if stereo else 1)
    parts = [b.mixdown_i16_parts_device(n, start, stereo=stereo) for b in shards]
    got = apply_chain_parts(parts, nvalues, x0=x0).download_bytes(nvalues * 2)
    for p in parts:
        p.free()
    return got


def _rows(bank, n, start):
    rows, stride = bank.generate_i16_device(n, start)
    got = rows.download(np.int16, bank.nvoices * stride).reshape(bank.nvoices, stride)[:, :n].copy()
    rows.free()
    return got


def test_config2_additive_shards_fused(gpu):
    """The bench's 1024-voice additive table on its plateau: every shard folds fused (the one-voice shard too), and the maps applied
    in order are the whole bank's fused mixdown; odd length over three 65 536-frame segments; 300 s into the notes; stereo."""
    N = gpu
    from synthesizer_amd import oscillators as G
    from synthesizer_amd.mixer import VoiceBank, mixdown_i16_banks
    from synthesizer_amd.workloads import additive_voices
    gv, gains = additive_voices(G, 1024, SR, seed=0, partials=16, adsr={"sustain": 1.0e6})
    whole = VoiceBank(gv, gains=gains)
    shards = _split(gv, gains, [1, 300, 723])
    for start, n in ((3 * SR + 11, 150001), (300 * SR, 48000), (3 * SR, 48000)):
        want = whole.mixdown_i16_device(n, start).download_bytes(n * 2)
        assert _fused(N) >= 1
        parts = []
        for b in shards:
            parts.append(b.mixdown_i16_parts_device(n, start))
            assert _fused(N) >= 1, (start, n, b.nvoices)           # every shard took the fused fold
        from synthesizer_amd.mixer import apply_chain_parts, compose_chain_parts
        assert apply_chain_parts(parts, n).download_bytes(n * 2) == want, (start, n)
        one = compose_chain_parts(parts, n)                         # composed first, then applied: the same bytes
        assert apply_chain_parts([one], n).download_bytes(n * 2) == want, (start, n)
        assert bytes(mixdown_i16_banks(shards, n, start).view_frame_data()) == want
        for p in parts + [one]:
            p.free()
    # the whole bank's own maps equal the shards' maps composed, and applied to silence they are its mixdown
    n, start = 20001, 3 * SR
    assert _sharded([whole], n, start) == whole.mixdown_i16_device(n, start).download_bytes(n * 2)
    # stereo: Sample.stereo(l, r) per voice, the chain over the interleaved samples
    n = 30001
    want_st = whole.mixdown_stereo_i16_device(n, start).download_bytes(n * 4)
    assert _sharded(shards, n, start, stereo=True) == want_st
    assert bytes(mixdown_i16_banks(shards, n, start, stereo=True).view_frame_data()) == want_st


def test_config3_fm_shards_rows_and_the_oracle(gpu):
    """FM voices go through int16 rows and the parts form of the chain kernel; against the whole bank and audioop over its rows."""
    from synthesizer_amd import oscillators as G
    from synthesizer_amd.mixer import VoiceBank
    from synthesizer_amd.workloads import fm_voices
    gv, gains = fm_voices(G, 1024, SR, seed=0)
    whole = VoiceBank(gv, gains=gains)
    for sizes in ([512, 512], [1, 100, 923], [1023, 1]):
        shards = _split(gv, gains, sizes)
        for start, n in ((1000, 20001), (0, 4097)):
            want = whole.mixdown_i16_device(n, start).download_bytes(n * 2)
            assert _sharded(shards, n, start) == want, (sizes, start, n)
    n, start = 6001, 333
    rows = _rows(whole, n, start)
    assert _sharded(_split(gv, gains, [7, 1017]), n, start) == audioop_chain([r.tobytes() for r in rows])
    want_st = audioop_chain([audioop.tostereo(r.tobytes(), 2, gl, gr) for r, (gl, gr) in zip(rows, gains)])
    assert whole.mixdown_stereo_i16_device(n, start).download_bytes(n * 4) == want_st
    assert _sharded(_split(gv, gains, [300, 1, 723]), n, start, stereo=True) == want_st


def test_additive_shards_against_the_oracle(gpu):
    """A small additive table against the C oracle's quantised rows folded by the live audioop (strict: the additive banks' boundary
    guard makes every int16 sample the oracle's)."""
    from oracle import c_oracle as CO
    from oracle import synth_oracle as O
    from synthesizer_amd import oscillators as G
    from synthesizer_amd.workloads import additive_voices
    gv, gains = additive_voices(G, 40, SR, seed=3, partials=16)
    ov, _ = additive_voices(O, 40, SR, seed=3, partials=16)
    n = 9001
    want_rows = [CO.quantise(CO.render(v, n)).astype(np.int16) for v in ov]
    want = audioop_chain([r.tobytes() for r in want_rows])
    assert _sharded(_split(gv, gains, [13, 27]), n, 0) == want
    want_st = audioop_chain([audioop.tostereo(r.tobytes(), 2, gl, gr) for r, (gl, gr) in zip(want_rows, gains)])
    assert _sharded(_split(gv, gains, [1, 39]), n, 0, stereo=True) == want_st


def test_fused_shard_beside_a_rows_shard_and_filter_graphs(gpu):
    """One shard folds fused, its neighbour (filter graphs, a modulated carrier) goes through rows; the whole table -- which has rows
    -- goes through rows in one piece: the same bytes, and audioop's chain over the whole bank's rows."""
    N = gpu
    from synthesizer_amd import oscillators as G
    from synthesizer_amd.mixer import VoiceBank
    from synthesizer_amd.workloads import additive_voices
    lean, lg = additive_voices(G, 128, SR, seed=1, partials=16, adsr={"sustain": 1.0e6})
    harm = [(1, 1.0), (3, 0.2)]
    other = [G.ClipFilter(G.Harmonics(300.0, harm, amplitude=0.9, samplerate=SR), -0.5, 0.6),
             G.AbsFilter(G.Sine(220.0, 0.7, samplerate=SR)),
             G.AmpModulationFilter(G.Sine(440.0, 0.8, samplerate=SR), G.Sine(3.0, 1.0, samplerate=SR)),
             G.Sine(500.0, 0.4, fm_lfo=G.Sine(3.0, 0.2, samplerate=SR), samplerate=SR),
             G.EnvelopeFilter(G.Triangle(120.0, 0.6, samplerate=SR), 0.01, 0.02, 30.0, 0.5, 0.1)]
    og = [(0.3 + 0.1 * i, 0.9 - 0.1 * i) for i in range(len(other))]
    voices, gains = lean + other, lg + og
    whole = VoiceBank(voices, gains=gains)
    a, b = VoiceBank(lean, gains=lg), VoiceBank(other, gains=og)
    for start, n in ((3 * SR, 70001), (3 * SR + 3, 12345)):
        pa = a.mixdown_i16_parts_device(n, start)
        assert _fused(N) >= 1                                        # the lean shard folded where the samples are made
        pb = b.mixdown_i16_parts_device(n, start)
        from synthesizer_amd.mixer import apply_chain_parts
        got = apply_chain_parts([pa, pb], n).download_bytes(n * 2)
        assert got == whole.mixdown_i16_device(n, start).download_bytes(n * 2), (start, n)
        assert got == audioop_chain([r.tobytes() for r in _rows(whole, n, start)]), (start, n)
        # the other order of the same shards is another chain: the maps apply in the order they are given
        assert _sharded([b, a], n, start) == audioop_chain([r.tobytes() for r in _rows(VoiceBank(other + lean, gains=og + lg), n, start)])
        pa.free()
        pb.free()
    n, start = 7001, SR
    assert _sharded([a, b], n, start, stereo=True) == whole.mixdown_stereo_i16_device(n, start).download_bytes(n * 4)


def test_shard_edge_inside_a_saturating_stretch_and_a_chain_continued_from_a_sample(gpu):
    """Loud voices: the chain hits the rails mid-table and comes back; shard edges fall inside that stretch.  Then x0: the maps applied
    to an existing Sample's frames equal audioop.add chained onto it."""
    from synthesizer_amd import _native as N
    from synthesizer_amd import oscillators as G
    from synthesizer_amd.mixer import VoiceBank, apply_chain_parts
    from synthesizer_amd.sample import Sample
    rng = np.random.default_rng(8)
    nv, start, n = 70, SR, 70001
    f, ph = rng.uniform(150.0, 1200.0, nv), rng.uniform(0.0, 1.0, nv)
    harm = [(1, 1.0), (2, 0.3), (5, 0.1)]
    voices = [G.EnvelopeFilter(G.Harmonics(float(f[i]), harm, amplitude=0.6, phase=float(ph[i]), samplerate=SR), 0.01, 0.05, 30.0, 0.8, 0.1)
              for i in range(nv)]
    gains = [(0.5, 0.5)] * nv
    whole = VoiceBank(voices, gains=gains)
    rows = _rows(whole, n, start)
    want = audioop_chain([r.tobytes() for r in rows])
    assert want != np.clip(rows.astype(np.int64).sum(axis=0), -32768, 32767).astype(np.int16).tobytes()
    # the running chain of the first k voices saturates somewhere for the edges used below
    run = np.zeros(n, dtype=np.int64)
    railed = []
    for k in range(nv):
        run = np.clip(run + rows[k], -32768, 32767)
        railed.append(bool(np.any(np.abs(run) >= 32767)))
    edges = [k for k in (20, 35, 50) if railed[k - 1]]
    assert edges
    for e in edges:
        assert _sharded(_split(voices, gains, [e, nv - e]), n, start) == want, e
    assert _sharded(_split(voices, gains, [1, 34, 1, 34]), n, start) == want
    # x0: an existing (loud) Sample, the table's voices chained onto it
    x0 = (rng.integers(-32768, 32768, size=n)).astype(np.int16)
    x0[::3] = 32767
    smp = Sample.from_raw_frames(x0.tobytes(), 2, SR, 1)
    want_x0 = audioop_chain([r.tobytes() for r in rows], x0=x0.tobytes())
    assert _sharded(_split(voices, gains, [35, 35]), n, start, x0=smp) == want_x0
    xb = N.DeviceBuffer.from_array(x0)
    parts = whole.mixdown_i16_parts_device(n, start)
    assert apply_chain_parts(parts, n, x0=xb).download_bytes(n * 2) == want_x0
    assert apply_chain_parts([], n, x0=xb).download_bytes(n * 2) == x0.tobytes()        # no parts: x0 itself
    assert apply_chain_parts([], n).download_bytes(n * 2) == bytes(2 * n)               # ... or silence


def test_device_compose_and_apply_match_the_host_algebra(gpu):
    """sh_chain_parts_compose / _apply on arbitrary maps (extreme adds included: they saturate at +-2^17) equal chainmaps, byte for
    byte; several planes in one buffer, an odd plane count, and compose in place."""
    from synthesizer_amd import _native as N
    from synthesizer_amd import chainmaps as CM
    from synthesizer_amd.mixer import apply_chain_parts, compose_chain_parts
    rng = np.random.default_rng(2)
    nvalues, nparts = 10007, 7
    planes = []
    for k in range(nparts):
        s = rng.integers(-32768, 32768, size=nvalues).astype(np.int16)
        m = CM.compose_all([CM.voice_maps(s), CM.voice_maps(rng.integers(-32768, 32768, size=nvalues).astype(np.int16))])
        if k == 3:
            m["add"][::5] = 2 ** 31 - 1                              # a map from outside the library: saturated on the way in
            m["add"][1::5] = -2 ** 31
        planes.append(m)
    buf = N.DeviceBuffer.from_array(np.concatenate(planes))
    want = CM.compose_all(planes)
    got = compose_chain_parts(buf, nvalues).download(np.uint8, nvalues * 8).tobytes()
    assert got == want.tobytes()
    x0 = rng.integers(-32768, 32768, size=nvalues).astype(np.int16)
    assert apply_chain_parts(buf, nvalues, x0=N.DeviceBuffer.from_array(x0)).download(np.int16, nvalues).tobytes() == CM.apply(planes, x0=x0).tobytes()
    assert apply_chain_parts(buf, nvalues).download(np.int16, nvalues).tobytes() == CM.apply(planes).tobytes()
    # in place: the result over plane 0
    N.check(N.lib().sh_chain_parts_compose(buf.handle, nparts, nvalues, nvalues, buf.handle))
    assert buf.download(np.uint8, nvalues * 8).tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        N.check(N.lib().sh_chain_parts_apply(buf.handle, nparts + 1, nvalues, nvalues, None, N.DeviceBuffer(nvalues * 2).handle))


def test_parts_bytes_follow_the_range_rule(gpu):
    """The maps the library MAKES, byte for byte: add = the exact sum of the voices saturated at +-2^17 once, lo / hi = the chain
    applied to -32768 / 32767 (tests/helpers.range_rule_maps) -- not the stored-map rule, which saturates add at every step.  Loud
    voices whose partial sums pass 2^17 and come back; sh_mix_chain_i16_parts, _pan_i16_parts, and sh_bank_mixdown_i16_parts on
    its fused and its two-step stretches, against the rows generate_i16 returns."""
    from synthesizer_amd import _native as N
    from synthesizer_amd import chainmaps as CM
    from synthesizer_amd import oscillators as G
    from synthesizer_amd.mixer import VoiceBank
    from tests.helpers import range_rule_maps
    L = N.lib()
    rng = np.random.default_rng(21)
    for nv, n in ((23, 40001), (90, 20003)):
        rows = rng.integers(-32768, 32768, size=(nv, n)).astype(np.int16)
        rows[: nv // 2, : n // 3] = 32000                       # the running sum passes +2^17 ...
        rows[nv // 2:, : n // 3] = -30000                       # ... and comes back below it
        rows[:, n // 3: n // 2] = -32768
        stride = n + 1
        chunks = N.DeviceBuffer(nv * stride * 2)
        for v in range(nv):
            chunks.upload(rows[v], v * stride * 2)
        maps = N.DeviceBuffer(n * 16)
        N.check(L.sh_mix_chain_i16_parts(chunks.handle, nv, stride, n, maps.handle))
        want = range_rule_maps(rows, n)
        assert rows[: nv // 2, 0].astype(np.int64).sum() > CM.ADD_MAX and abs(int(want["add"][0])) < CM.ADD_MAX
        assert want["add"][n // 3] == -CM.ADD_MAX
        assert maps.download_bytes(n * 8) == want.tobytes(), nv
        fac = N.DeviceBuffer.from_array(np.tile([1.5, 0.75], nv))
        st = [np.frombuffer(audioop.tostereo(r.tobytes(), 2, 1.5, 0.75), dtype=np.int16) for r in rows]
        N.check(L.sh_mix_chain_pan_i16_parts(chunks.handle, nv, stride, n, fac.handle, maps.handle))
        assert maps.download_bytes(n * 16) == range_rule_maps(st, 2 * n).tobytes(), nv
        for b in (chunks, maps, fac):
            b.free()
    # a bank in phase: 70 voices of amplitude 0.9 sum far beyond 2^17; from frame 0 the notes' attack and decay go through the rows
    # (two-step), the plateau through the fused fold
    nv = 70
    f = rng.uniform(200.0, 210.0, nv)
    voices = [G.EnvelopeFilter(G.Harmonics(float(f[i]), [(1, 1.0), (3, 0.2)], amplitude=0.9, phase=0.0, samplerate=SR), 0.01, 0.05, 30.0, 0.8, 0.1)
              for i in range(nv)]
    bank = VoiceBank(voices, gains=[(0.5, 0.5)] * nv)
    for start, n in ((0, 70001), (SR, 30001)):
        rows = _rows(bank, n, start)
        want = range_rule_maps(rows, n)
        assert np.max(np.abs(want["add"])) == CM.ADD_MAX
        parts = bank.mixdown_i16_parts_device(n, start)
        assert _fused(N) >= 1, start
        assert parts.download_bytes(n * 8) == want.tobytes(), start
        parts.free()


def test_table_beyond_one_bank_through_mixdown_i16_banks(gpu):
    """40 000 voices: no single bank's integer route takes them (sh_bank_mixdown_i16 still refuses), two banks' maps do; short blocks."""
    from synthesizer_amd import oscillators as G
    from synthesizer_amd.mixer import VoiceBank, mixdown_i16_banks
    rng = np.random.default_rng(12)
    nv = 40000
    f = rng.uniform(50.0, 4000.0, nv)
    a = rng.uniform(0.01, 0.2, nv)
    voices = [G.Sine(float(f[i]), float(a[i]), phase=float(i % 7) / 7.0, samplerate=SR) for i in range(nv)]
    gains = [(float(x), float(1.0 - x)) for x in rng.uniform(0.0, 1.0, nv)]
    whole = VoiceBank(voices, gains=gains)
    banks = _split(voices, gains, [20000, 17000, 3000])
    for start, n in ((0, 1000), (5 * SR + 1, 777)):
        rows = _rows(whole, n, start)
        want = audioop_chain([r.tobytes() for r in rows])
        assert want != np.clip(rows.astype(np.int64).sum(axis=0), -32768, 32767).astype(np.int16).tobytes()
        got = mixdown_i16_banks(banks, n, start)
        assert got.nchannels == 1 and len(got) == n and bytes(got.view_frame_data()) == want, (start, n)
        with pytest.raises(ValueError):
            whole.mixdown_i16_device(n, start)
    n, start = 500, 1234
    rows = _rows(whole, n, start)
    want_st = audioop_chain([audioop.tostereo(r.tobytes(), 2, gl, gr) for r, (gl, gr) in zip(rows, gains)])
    got = mixdown_i16_banks(banks, n, start, stereo=True)
    assert got.nchannels == 2 and bytes(got.view_frame_data()) == want_st


def test_one_rank_rccl_gather_and_dist_mixdown(gpu):
    """sh_dist_gather_parts without a communicator and on a 1-rank RCCL communicator (a copy either way), and DistVoiceBank.mixdown_i16
    of a world of one: the bank's own mixdown."""
    from synthesizer_amd import _native as N
    from synthesizer_amd import dist
    from synthesizer_amd import oscillators as G
    from synthesizer_amd.workloads import additive_voices
    L = N.lib()
    voices, gains = additive_voices(G, 64, SR, seed=2, adsr={"sustain": 1.0e6})
    n, start = 24001, SR
    local = dist.DistVoiceBank(voices, gains, 0, 1)
    want = local.local.mixdown_i16_device(n, start).download_bytes(n * 2)
    want_st = local.local.mixdown_stereo_i16_device(n, start).download_bytes(n * 4)
    parts = local.local.mixdown_i16_parts_device(n, start)
    g = N.DeviceBuffer(n * 8)
    N.check(L.sh_dist_gather_parts(parts.handle, n, 0, g.handle))          # (no communicator yet)
    assert g.download_bytes(n * 8) == parts.download_bytes(n * 8)
    assert local.mixdown_i16(n, start) == want
    dist.init(0, 1, broadcast=lambda payload, rank, world, nb: payload)
    try:
        g.zero()
        N.check(L.sh_dist_gather_parts(parts.handle, n, 0, g.handle))
        assert g.download_bytes(n * 8) == parts.download_bytes(n * 8)
        with pytest.raises(ValueError):
            N.check(L.sh_dist_gather_parts(parts.handle, n, 1, g.handle))
        with pytest.raises(ValueError):
            N.check(L.sh_dist_gather_parts(parts.handle, n + 1, 0, g.handle))
        bank = dist.DistVoiceBank(voices, gains, 0, 1)
        assert bank.mixdown_i16(n, start) == want
        assert bank.mixdown_i16(n, start, stereo=True) == want_st
        # the float ring and the integer route on the same bank, interleaved
        ref = bank.local.render(n, start)
        assert np.array_equal(bank.render(n, start), ref)
        assert bank.mixdown_i16(n, start) == want
        assert np.array_equal(bank.render(n, start), ref)
    finally:
        dist.shutdown()
