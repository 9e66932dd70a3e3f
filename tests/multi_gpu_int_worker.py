"""One rank of the integer mixdown across GPUs (tests/test_gpu_multi_int_mixdown.py): RANK / WORLD_SIZE / LOCAL_RANK / MASTER_* from
the launcher (dist.rank_env), one process per GPU.  The rank renders its contiguous shard of the table, leaves the chain maps of it,
RCCL gathers them to root, root applies them in rank order.  Root writes the int16 bytes to <out>/mono.bin and <out>/stereo.bin;
every rank writes <out>/done_<rank> with what it got (bytes on root, None elsewhere)."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

SR = 48000
NVOICES = 512
MONO = (96000, 3 * SR + 5)          # (frames, start): one fused stretch past the attack, one of rows inside it
STEREO = (4001, 700)


def workload():
    from synthesizer_amd import oscillators as G
    from synthesizer_amd.workloads import additive_voices
    return additive_voices(G, NVOICES, SR, seed=4, partials=16, adsr={"sustain": 1.0e6})


def main(out: Path) -> None:
    from synthesizer_amd import dist
    rank, world = dist.init_from_env()
    try:
        voices, gains = workload()
        bank = dist.DistVoiceBank(voices, gains, rank, world)
        mono = bank.mixdown_i16(MONO[0], MONO[1], root=0)
        stereo = bank.mixdown_i16(STEREO[0], STEREO[1], root=world - 1, stereo=True)
        if mono is not None:
            (out / "mono.bin").write_bytes(mono)
        if stereo is not None:
            (out / "stereo.bin").write_bytes(stereo)
        (out / ("done_%d" % rank)).write_text(json.dumps({"rank": rank, "world": world, "mono": mono is not None,
                                                          "stereo": stereo is not None, "rccl": dist.comm_info()}))
    finally:
        if world > 1:
            dist.shutdown()


if __name__ == "__main__":
    main(Path(sys.argv[1]))
