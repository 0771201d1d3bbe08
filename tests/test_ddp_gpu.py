"""Multi-rank data parallelism on the GPU path (2 ranks sharing cuda:0, gloo collectives).

RCCL cannot put two ranks on one device, and gpurun boxes have one GPU, so this
exercises everything of the multi-GPU path except RCCL itself: native kernels,
in-place gradient sinks, the side-stream weight gradients the reducer must join
before each bucket's collective, bucket ordering and the fused optimizer.  The
RCCL communicator + C++ reducer path itself is executed on one GPU by
test_rccl_gpu.py (forced world-1 communicator: bitwise gradients, bf16 wire,
timing, launch order, strict duplicate-mark checking).
"""
import json
import os
import subprocess
import sys

import pytest
from conftest import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_ddp_two_ranks_one_gpu(tmp_path, gpu):
    out = str(tmp_path / "res")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["OMP_NUM_THREADS"] = "2"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tests", "ddp_gpu_worker.py"), "--out", out]
    r = subprocess.run(cmd, cwd=ROOT, env=env, timeout=110, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = [json.load(open(f"{out}.rank{i}.json")) for i in range(2)]
    for x in res:
        assert x["finite"]
        assert x["grad_rel_err"] < 2e-2, x["worst_params"]
        assert x["launch_order"] == list(range(x["bucket_info"]["num_buckets"]))
    cs = res[0]["checksums"]
    assert cs[0] == cs[1], cs


def test_bench_two_ranks_share_device_ranks_identical(tmp_path, gpu):
    """bench.py at N>1 proves its ranks ended bit-identical (all-gathered
    parameter checksum in the JSON) -- rehearsed with 2 gloo ranks sharing cuda:0 on the native
    kernels, the same bench path the driver's 8-GPU run takes."""
    out = tmp_path / "b.json"
    env = dict(os.environ, MASTER_PORT=str(free_port()), OMP_NUM_THREADS="2")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-device",
                        "--backend", "gloo", "--arch", "resnet18", "--image-size", "64", "--batch", "16",
                        "--steps", "2", "--warmup", "1", "--full", "--json-out", str(out)],
                       cwd=ROOT, env=env, timeout=110, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = json.loads(out.read_text())
    assert d["n_gpus"] == 2 and d["config"]["shared_device"]
    assert d["config"]["ranks_identical"] is True, d["config"]



@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "default"])
def test_bench_dump_outputs_same_every_run(tmp_path, gpu, det):
    """``bench.py --dump-outputs`` writes the last timed step's logits, loss and updated parameters
    as float32 ``.npy``, computed by the kernels the arguments select, from the seeded initial
    weights (put back before that step).  So a run of 1 + 3 steps dumps what a run of one single
    step -- an independent first forward / backward / update from the same seed -- dumps: bit for
    bit with ``--deterministic``; with the default kernels (fp32-atomic reductions, whose order
    varies) to a relative L2 error of 2^-8 per array, one bf16 rounding: every activation and
    activation gradient of the step is stored in bf16, so a reduction that lands on the other
    side of a rounding boundary moves a value by at most that much."""
    import numpy as np
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    dumps = []
    for run, steps, warmup in (("a", 3, 1), ("b", 1, 0)):
        d = tmp_path / run
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--arch", "resnet18", "--image-size", "64",
                            "--batch", "16", "--steps", str(steps), "--warmup", str(warmup),
                            "--dump-outputs", str(d)] + (["--deterministic"] if det else []),
                           cwd=ROOT, env=env, timeout=110, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
        assert res["steps"] == steps and res["config"]["deterministic"] is det and res["full"] is False
        dumps.append({n: np.load(d / f"{n}.npy") for n in ("logits", "loss", "params")})
        assert abs(float(dumps[-1]["loss"][0]) - res["config"]["final_loss"]) < 1e-3
    a, b = dumps
    assert a["logits"].shape == (16, 1000) and a["loss"].shape == (1,)
    assert a["params"].shape == (8 * 2**20,)  # ResNet-18 has 11.7 M parameters: the seeded sample
    for n in a:
        assert a[n].dtype == np.float32 and np.isfinite(a[n]).all()
        err = float(np.linalg.norm(a[n].astype(np.float64) - b[n]) / np.linalg.norm(b[n].astype(np.float64)))
        print(f"{n}: relative L2 difference {err:.3e}")
        if det:
            assert np.array_equal(a[n], b[n]), n
        else:
            assert err <= 2.0 ** -8, (n, err)
