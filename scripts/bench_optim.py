#!/usr/bin/env python3
"""Time the fused flat-space optimizer steps on the GPU: SGD against LARS and its three passes.

    python scripts/bench_optim.py [--arch resnet50] [--iters 200] [--rounds 5] [--out FILE]

The flat space is a real model's (default ResNet-50: 25.6 M elements, 161 tensors) with the bf16
weight mirror as a side output, as in training.  Everything is timed with device events after a
warm-up, in one process, the candidates alternating round by round; the figure per candidate is
the median round (each round = ``iters`` back-to-back calls).  Bytes are counted from the layout
(SGD: 3 reads + 2 writes of fp32 plus the bf16 mirror write; LARS adds one read of p and g for the
adapted segments), so the rates are achieved bytes per second of the call, launches included.
The target the LARS step is held to: ``t_lars <= 1.25 * t_sgd * 7 / 5``.
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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim needs a GPU")
    from pytorch_distributed_tutorials_amd.models import build_model
    from pytorch_distributed_tutorials_amd.ops._ext import native
    from pytorch_distributed_tutorials_amd.optim.lars import LarsTable
    from pytorch_distributed_tutorials_amd.parallel import DistributedDataParallel

    C = native()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = build_model(a.arch, num_classes=1000, impl="native").to(dev)
    model.set_impl("native")
    sp = DistributedDataParallel(model).space
    n = sp.numel
    segs = [(o, p.numel(), p.ndim <= 1) for p, o in zip(sp.params, sp.offsets)]
    tb = LarsTable(segs, dev)
    p0 = sp.param_flat.clone()
    p = p0.clone()
    g = torch.randn(n, device=dev) * 1e-3
    buf = torch.zeros(n, device=dev)
    pb = torch.empty(n, dtype=torch.bfloat16, device=dev)
    adapted = sum(s for _, s, e in segs if not e)
    hp = dict(lr=1e-3, mom=0.9, damp=0.0, wd=1e-4, eta=1e-3, eps=1e-8)
    full = (0, tb.nseg)

    cands = {
        "sgd_step": lambda: C.sgd_step(p, g, buf, hp["lr"], hp["mom"], hp["damp"], hp["wd"], False, False, 1.0, pb),
        "lars_step": lambda: C.lars_step(p, g, buf, tb.table, tb.partials, tb.trust, *full, hp["lr"], hp["mom"],
                                         hp["damp"], hp["wd"], False, False, hp["eta"], hp["eps"], pb),
        "lars_norms": lambda: C.lars_norms(p, g, tb.table, tb.partials, tb.trust, *full),
        "lars_trust": lambda: C.lars_trust_only(tb.table, tb.partials, tb.trust, *full, hp["wd"], hp["eta"],
                                                hp["eps"]),
        "lars_update": lambda: C.lars_update(p, g, buf, tb.table, tb.partials, tb.trust, *full, hp["lr"],
                                             hp["mom"], hp["damp"], hp["wd"], False, False, pb),
    }
    update_bytes = n * (3 * 4 + 2 * 4 + 2)
    nbytes = {"sgd_step": update_bytes, "lars_update": update_bytes, "lars_norms": adapted * 8,
              "lars_trust": tb.nchunks * 16, "lars_step": update_bytes + adapted * 8}

    def timed(fn, iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) * 1e3 / iters  # us per call

    for fn in cands.values():  # warm-up: code objects, clocks
        timed(fn, 20)
    rounds = {k: [] for k in cands}
    for _ in range(a.rounds):
        for k, fn in cands.items():  # alternate the candidates
            p.copy_(p0)
            rounds[k].append(timed(fn, a.iters))
    us = {k: statistics.median(v) for k, v in rounds.items()}
    target = 1.25 * us["sgd_step"] * 7 / 5
    res = {
        "bench": "optim_flat_step", "arch": a.arch, "numel": n, "tensors": len(segs), "chunks": tb.nchunks,
        "adapted_numel": adapted, "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
        "us": {k: round(v, 2) for k, v in us.items()},
        "us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in rounds.items()},
        "GBps": {k: round(nbytes[k] / us[k] * 1e-3, 1) for k in us},
        "lars_over_sgd": round(us["lars_step"] / us["sgd_step"], 3),
        "target_us": round(target, 2), "meets_target": bool(us["lars_step"] <= target),
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
