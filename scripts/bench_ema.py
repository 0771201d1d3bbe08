#!/usr/bin/env python3
"""Time the weight-EMA update (``_C_ema.ema_update``, ``optim.ModelEma``) on the GPU: alone against the
fused SGD step it is modelled on and the torch ``AveragedModel`` it replaces, and inside the training
step.

    python scripts/bench_ema.py [--arch resnet50] [--batch 256] [--iters 50] [--rounds 7]
                                [--step-iters 64] [--step-rounds 7] [--skip-step] [--out FILE]

Isolated, on the model's real flat parameter space plus its flat buffers:

* ``ema_update``      one launch with the bf16 mirror side output: 2 fp32 reads, 1 fp32 write and 1
                      bf16 write per parameter = 14 B (the float buffers 12 B, the counters 16 B);
* ``sgd_step``        ``_C.sgd_step`` with momentum and the mirror on a space of the same size: 3 reads,
                      2 writes and the bf16 write = 22 B per parameter.  The yardstick: the same launch
                      shape and streaming pattern;
* ``averaged_model``  ``AveragedModel(use_buffers=True, get_ema_multi_avg_fn).update_parameters`` on the
                      stock module: what the kernel replaces (12 B per element, no bf16 image).

In the step (``--skip-step`` leaves it out): the ``bench.py`` training step (native model behind the DDP
wrapper, batch x 3 x size x size synthetic input, SGD momentum 0.9 / wd 1e-5, per-bucket update) with
the EMA off, updated every step and every 32nd step.  ms per step over ``--step-iters`` back-to-back
steps.

(The A/B of a non-temporal variant of the kernel, isolated and in the step, was made with an earlier
version of this script and is kept in ``profiles/ema_nt_ab.json``; the variant lost and was removed.)

Method of ``scripts/bench_optim.py`` / ``bench_mix.py``: one process, device events, a warm-up, the
candidates alternating round by round, the figure per candidate the median round with min-max.  Bytes
are counted from the shapes, so the rates are counted bytes per second of the call, launch included.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arch", default="resnet50")
    ap.add_argument("--num-classes", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--decay", type=float, default=0.9998)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step-iters", type=int, default=64, help="a multiple of 32, for the every-32 configuration")
    ap.add_argument("--step-rounds", type=int, default=7)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.json"))
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema needs a GPU")
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    from pytorch_distributed_tutorials_amd import ops
    from pytorch_distributed_tutorials_amd.models import build_model
    from pytorch_distributed_tutorials_amd.ops._ext import native, native_ema
    from pytorch_distributed_tutorials_amd.optim import SGD, ModelEma
    from pytorch_distributed_tutorials_amd.parallel import DistributedDataParallel

    C, E = native(), native_ema()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = build_model(a.arch, num_classes=a.num_classes, impl="native").to(dev)
    model.set_impl("native")
    ddp = DistributedDataParallel(model)
    opt = SGD(ddp.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-5)
    ema = ModelEma(ddp, a.decay)
    assert ema._flat is not None
    tsp, sp, mirror, (fe, fm), (ie, im) = ema._flat
    n, nf, ni = sp.numel, fe.numel(), ie.numel()
    w = 1.0 - a.decay

    # the yardstick runs on buffers of its own (same size), so the model is not stepped by it
    p2, g2, b2 = sp.param_flat.clone(), torch.zeros_like(sp.param_flat), torch.zeros_like(sp.param_flat)
    k2 = torch.empty(n, dtype=torch.bfloat16, device=dev)
    stock = build_model(a.arch, num_classes=a.num_classes, impl="torch").to(dev)
    avg = AveragedModel(stock, use_buffers=True, multi_avg_fn=get_ema_multi_avg_fn(a.decay))
    avg.update_parameters(stock)  # the copy of n_averaged == 0

    cands = {
        "ema_update": lambda: E.ema_update(tsp.param_flat, sp.param_flat, w, mirror.krsc, fe, fm, ie, im),
        "sgd_step": lambda: C.sgd_step(p2, g2, b2, 0.01, 0.9, 0.0, 1e-5, False, False, 1.0, k2),
        "averaged_model": lambda: avg.update_parameters(stock),
    }
    ema_bytes = 14 * n + 12 * nf + 16 * ni
    n_stock = sum(t.numel() * t.element_size() for t in list(stock.parameters()) + list(stock.buffers()))
    nbytes = {"ema_update": ema_bytes, "sgd_step": 22 * n, "averaged_model": 3 * n_stock}

    def timed(fn, iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) * 1e3 / iters  # us per call

    for fn in cands.values():  # warm-up: code objects, allocator pools, clocks
        timed(fn, 10)
    rounds = {k: [] for k in cands}
    for _ in range(a.rounds):
        for k, fn in cands.items():  # alternate the candidates
            rounds[k].append(timed(fn, a.iters))
    us = {k: statistics.median(v) for k, v in rounds.items()}
    gbps = {k: nbytes[k] / us[k] * 1e-3 for k in us}
    res = {
        "bench": "ema", "arch": a.arch, "params": n, "float_buffer_elems": nf, "int_buffer_elems": ni,
        "decay": a.decay, "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
        "us": {k: round(v, 2) for k, v in us.items()},
        "us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in rounds.items()},
        "counted_bytes": nbytes,
        "GBps": {k: round(v, 1) for k, v in gbps.items()},
        "ema_over_sgd_GBps": round(gbps["ema_update"] / gbps["sgd_step"], 3),
        "averaged_model_over_ema_us": round(us["averaged_model"] / us["ema_update"], 1),
    }

    if not a.skip_step:
        del p2, g2, b2, k2, avg, stock
        torch.cuda.empty_cache()
        g = torch.Generator(device="cpu").manual_seed(1234)
        images = torch.randn((a.batch, 3, a.size, a.size), generator=g).to(dev)
        labels = torch.randint(0, a.num_classes, (a.batch,), generator=g).to(dev)
        criterion = ops.CrossEntropyLoss()
        ema.reset()

        def step():
            opt.zero_grad()
            loss = criterion(ddp(images), labels)
            loss.backward()
            opt.step()

        def config(every):
            def run():
                step()
                if every:
                    ema.update()

            def arm():
                ema.every, ema._calls = max(every, 1), 0
            return arm, run

        cfgs = {"off": config(0), "every1": config(1), "every32": config(32)}
        for arm, run in cfgs.values():
            arm()
            timed(run, 8)
        srounds = {k: [] for k in cfgs}
        for _ in range(a.step_rounds):
            for k, (arm, run) in cfgs.items():
                arm()
                srounds[k].append(timed(run, a.step_iters) * 1e-3)  # ms per step
        ms = {k: statistics.median(v) for k, v in srounds.items()}
        res["step"] = {
            "batch": a.batch, "size": a.size, "iters": a.step_iters, "rounds": a.step_rounds,
            "ms": {k: round(v, 3) for k, v in ms.items()},
            "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in srounds.items()},
            "every1_share_of_step": round((ms["every1"] - ms["off"]) / ms["off"], 4),
        }

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
