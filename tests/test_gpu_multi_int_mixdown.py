"""The reference's int16 mixdown across GPUs: RCCL with MORE THAN ONE rank (worlds 2, 4 and 8 as the box allows, one process per
GPU, tests/multi_gpu_int_worker.py).  Root's bytes must equal the single-GPU mixdown of the whole table, byte for byte, and the
other ranks get None.  Skips, saying why, on a box with fewer than two GPUs (1-rank RCCL: tests/test_gpu_chain_parts.py; the
same code over gloo on CPU: tests/test_dist_int_mixdown_gloo.py)."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
WORKER = ROOT / "tests" / "multi_gpu_int_worker.py"


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_worker_dry_run_on_one_gpu(gpu, tmp_path):
    """The worker with WORLD_SIZE=1 (no communicator: the gather is a copy), against the whole table's own mixdown."""
    sys.path.insert(0, str(ROOT / "tests"))
    import multi_gpu_int_worker as W
    from synthesizer_amd.mixer import VoiceBank
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, str(WORKER), str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=660)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    voices, gains = W.workload()
    alone = VoiceBank(voices, gains=gains)
    assert (tmp_path / "mono.bin").read_bytes() == alone.mixdown_i16_device(W.MONO[0], W.MONO[1]).download_bytes(W.MONO[0] * 2)
    assert (tmp_path / "stereo.bin").read_bytes() == alone.mixdown_stereo_i16_device(W.STEREO[0], W.STEREO[1]).download_bytes(W.STEREO[0] * 4)


def test_int_mixdown_gathered_by_rccl_across_gpus(gpu, tmp_path):
    ngpus = gpu.lib().sh_device_count()
    if ngpus < 2:
        pytest.skip("needs >= 2 GPUs for a multi-rank RCCL communicator; this box shows %d (1-rank RCCL: "
                    "tests/test_gpu_chain_parts.py, worlds 2 and 3 over gloo: tests/test_dist_int_mixdown_gloo.py)" % ngpus)
    sys.path.insert(0, str(ROOT / "tests"))
    import multi_gpu_int_worker as W
    from synthesizer_amd import dist
    from synthesizer_amd.mixer import VoiceBank
    voices, gains = W.workload()
    alone = VoiceBank(voices, gains=gains)
    want_mono = alone.mixdown_i16_device(W.MONO[0], W.MONO[1]).download_bytes(W.MONO[0] * 2)
    want_st = alone.mixdown_stereo_i16_device(W.STEREO[0], W.STEREO[1]).download_bytes(W.STEREO[0] * 4)
    for world in [w for w in (2, 4, 8) if w <= ngpus]:
        out = tmp_path / ("w%d" % world)
        out.mkdir()
        port = _free_port()
        procs = []
        for r in range(world):
            env = dist.rank_env(r, world, port)
            procs.append(subprocess.Popen(["timeout", "-k", "10", "600", sys.executable, str(WORKER), str(out)], env=env,
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        logs = []
        for p in procs:
            try:
                o, _ = p.communicate(timeout=660)
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                raise
            logs.append(o)
        assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
        done = [json.loads((out / ("done_%d" % r)).read_text()) for r in range(world)]
        assert [d["mono"] for d in done] == [r == 0 for r in range(world)], done
        assert [d["stereo"] for d in done] == [r == world - 1 for r in range(world)], done
        assert all(d["rccl"]["communicator"] and d["rccl"]["world"] == world for d in done), done
        assert (out / "mono.bin").read_bytes() == want_mono, world
        assert (out / "stereo.bin").read_bytes() == want_st, world
