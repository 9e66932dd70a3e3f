"""dist.DistVoiceBank.mixdown_i16 on CPU (gloo, worlds 2 and 3): every rank renders its contiguous shard with the oracle, quantises
every voice (from_osc_block), leaves the chain maps of its shard (synthesizer_amd.chainmaps), the maps are gathered to root by gloo,
and root applies them in rank order.  Root's bytes must equal the live ``audioop`` chain over ALL the voices -- the reference's
int16 mixdown, which the float64 reduce cannot give -- and the other ranks get None.  (RCCL: tests/test_gpu_dist_int_mixdown.py.)"""
import audioop
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SR = 48000


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _voices(O, nvoices):
    """Loud enveloped Harmonics: the running sum hits the rails mid-chain and later voices pull it back (order matters)."""
    rng = np.random.default_rng(9)
    f, ph = rng.uniform(150.0, 1200.0, nvoices), rng.uniform(0.0, 1.0, nvoices)
    harm = [(1, 1.0), (2, 0.3), (5, 0.1)]
    voices = [O.EnvelopeFilter(O.Harmonics(float(f[i]), harm, amplitude=0.6, phase=float(ph[i]), samplerate=SR), 0.002, 0.003, 30.0, 0.8, 0.1)
              for i in range(nvoices)]
    gains = [((1.0 + 0.05 * i) / 2.0, (1.0 - 0.04 * i) / 2.0) for i in range(nvoices)]
    return voices, gains


def _rows(O, voices, start, n):
    return [np.array(O.quantise(v.take(start + n)[start:]), dtype=np.int16) for v in voices]


class _OracleGlooIntBackend:
    """DistVoiceBank's integer route on CPU: the oracle renders and quantises the shard, chainmaps folds it, gloo gathers."""

    def __init__(self, voices, gains, td, torch, rank, world):
        self.voices, self.gains = voices, gains
        self.td, self.torch, self.rank, self.world = td, torch, rank, world
        self.log = []

    def sync(self):
        self.log.append(("sync",))

    def mixdown_parts(self, nframes, start, scale, stereo):
        from oracle import synth_oracle as O
        from synthesizer_amd import chainmaps as CM
        self.log.append(("parts", nframes, start, stereo))
        rows = _rows(O, self.voices, start, nframes)
        if stereo:
            rows = [np.frombuffer(audioop.tostereo(r.tobytes(), 2, gl, gr), dtype=np.int16) for r, (gl, gr) in zip(rows, self.gains)]
        return CM.compose_all([CM.voice_maps(r) for r in rows])

    def gather_parts(self, parts, nvalues, root, rank, world):
        self.log.append(("gather", nvalues, root))
        t = self.torch.from_numpy(parts.view(np.int64).copy())
        bucket = [self.torch.empty_like(t) for _ in range(world)] if rank == root else None
        self.td.gather(t, gather_list=bucket, dst=root)
        if rank != root:
            return None
        return np.concatenate([b.numpy() for b in bucket])

    def apply_parts(self, gathered, nparts, nvalues):
        from synthesizer_amd import chainmaps as CM
        self.log.append(("apply", nparts, nvalues))
        planes = gathered.view(CM.CHAIN_MAP_DTYPE).reshape(nparts, nvalues)
        return CM.apply(list(planes)).tobytes()


def _worker(rank, world, port, nvoices, cases, q):
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as td
    from oracle import synth_oracle as O
    from synthesizer_amd import dist
    td.init_process_group("gloo", rank=rank, world_size=world)
    try:
        voices, gains = _voices(O, nvoices)
        lo, hi = dist.shard_range(nvoices, rank, world)
        backend = _OracleGlooIntBackend(voices[lo:hi], gains[lo:hi], td, torch, rank, world)
        bank = dist.DistVoiceBank(voices, gains, rank, world, backend=backend)
        out = [bank.mixdown_i16(n, start, root=root, stereo=stereo) for n, start, root, stereo in cases]
        td.barrier()
        q.put((rank, out, backend.log))
    finally:
        td.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_dist_int_mixdown_equals_audioop_chain_over_all_voices(world):
    import torch.multiprocessing as mp
    from oracle import synth_oracle as O
    nvoices = 11
    cases = [(601, 0, 0, False), (333, 700, world - 1, False), (257, 100, 0, True), (0, 0, 0, False)]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, nvoices, cases, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = sorted((q.get(timeout=240) for _ in procs), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    voices, gains = _voices(O, nvoices)
    saturated = False
    for k, (n, start, root, stereo) in enumerate(cases):
        if n == 0:
            assert results[root][1][k] == b""
            continue
        rows = _rows(O, _voices(O, nvoices)[0], start, n)
        if stereo:
            rows = [np.frombuffer(audioop.tostereo(r.tobytes(), 2, gl, gr), dtype=np.int16) for r, (gl, gr) in zip(rows, gains)]
        want = rows[0].tobytes()
        for r in rows[1:]:
            want = audioop.add(want, r.tobytes(), 2)
        exact = np.clip(np.sum(np.stack(rows).astype(np.int64), axis=0), -32768, 32767).astype(np.int16).tobytes()
        saturated |= want != exact
        for rank, out, _log in results:
            if rank == root:
                assert out[k] == want, (world, k)
            else:
                assert out[k] is None, (world, k, rank)
    assert saturated                                           # the chain hit the rails somewhere: the sum of truncations would differ
    for rank, _out, log in results:
        gathers = [e for e in log if e[0] == "gather"]
        assert gathers == [("gather", n * (2 if st else 1), root) for n, _s, root, st in cases if n]
        applies = [e for e in log if e[0] == "apply"]
        assert applies == ([("apply", world, n * (2 if st else 1)) for n, _s, root, st in cases if n and root == rank])
