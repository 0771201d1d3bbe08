#!/usr/bin/env python3
"""Time the batch-mixing kernels (MixUp / CutMix) on the GPU against the passes they fold into.

    python scripts/bench_mix.py [--batch 256] [--size 224] [--iters 100] [--rounds 5] [--out FILE]

At batch x 3 x size x size from a uint8 source (the ImageNet-shaped step input):

* ``augment``          ``_C.augment``, unchanged: the yardstick;
* ``mix_mixup``        ``_C_mix.augment_mix`` with every sample blended (reads the source twice);
* ``mix_cutmix``       ``augment_mix`` with every sample in CutMix mode (boxes from ``draw_mix``);
* ``mix_none``         ``augment_mix`` with no sample mixed (must sit close to the yardstick);
* ``augment_torch_mix`` ``_C.augment`` followed by the torch ``mix_batch``: what the fusion replaces.

At 256 x 1000 logits: ``_C.softmax_xent`` against ``_C_mix.softmax_xent_mix``.

Method of ``scripts/bench_optim.py``: one process, device events, a warm-up, the candidates
alternating round by round, the figure per candidate the median round (a round = ``iters``
back-to-back calls).  Bytes are counted from the shapes -- source bytes read once per gather that
needs them (twice for MixUp; once for CutMix, where a pixel comes from the sample or its partner)
plus the fp32 batch written once; the torch chain adds the least it can move, two reads and one
write of the fp32 batch -- so the rates are counted bytes per second of the call, launches included.
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
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--source", type=int, default=1024, help="images in the device-resident source set")
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_bench.json"))
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mix needs a GPU")
    from pytorch_distributed_tutorials_amd.data import draw_mix, mix_batch
    from pytorch_distributed_tutorials_amd.data.datasets import IMAGENET_MEAN, IMAGENET_STD
    from pytorch_distributed_tutorials_amd.ops._ext import native, native_mix

    C, M = native(), native_mix()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    B, S = a.batch, a.size
    src = torch.randint(0, 256, (a.source, 3, S, S), device=dev, dtype=torch.uint8, generator=g)
    idx = torch.randperm(a.source, device=dev, generator=g)[:B].contiguous()
    oy = torch.randint(0, 9, (B,), device=dev, generator=g)
    ox = torch.randint(0, 9, (B,), device=dev, generator=g)
    flip = torch.rand((B,), device=dev, generator=g) < 0.5
    mean, std = list(IMAGENET_MEAN), list(IMAGENET_STD)
    aug_args = (src, idx, oy, ox, flip, 4, True, mean, std)

    partner = (torch.arange(B, device=dev) - 1) % B
    ones = torch.ones(B, device=dev)
    nobox = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    w_mixup = torch.rand((B,), device=dev, generator=g) * 0.98 + 0.01
    cut = draw_mix(B, S, S, 0.0, 1.0, 1.0, 0.5, dev, g)
    box_share = float(1.0 - cut.lam.mean().item())

    V = a.classes
    logits = 3 * torch.randn((B, V), device=dev, generator=g)
    la = torch.randint(0, V, (B,), device=dev, generator=g)
    lb = la.roll(1)
    lam = torch.rand((B,), device=dev, generator=g)

    cands = {
        "augment": lambda: C.augment(*aug_args),
        "mix_mixup": lambda: M.augment_mix(*aug_args, partner, w_mixup, nobox),
        "mix_cutmix": lambda: M.augment_mix(*aug_args, partner, cut.w, cut.box),
        "mix_none": lambda: M.augment_mix(*aug_args, partner, ones, nobox),
        "augment_torch_mix": lambda: mix_batch(C.augment(*aug_args), partner, w_mixup, nobox),
        "softmax_xent": lambda: C.softmax_xent(logits, la, 0.1),
        "softmax_xent_mix": lambda: M.softmax_xent_mix(logits, la, lb, lam, 0.1),
    }
    px = B * 3 * S * S
    head = 2 * B * V * 4  # logits read (the three passes hit the cache after the first), dlogits written
    nbytes = {"augment": px + 4 * px, "mix_mixup": 2 * px + 4 * px, "mix_cutmix": px + 4 * px,
              "mix_none": px + 4 * px, "augment_torch_mix": (px + 4 * px) + 3 * 4 * px,
              "softmax_xent": head, "softmax_xent_mix": head}

    # the candidates compute what they should before they are timed
    base = C.augment(*aug_args)
    assert torch.equal(M.augment_mix(*aug_args, partner, ones, nobox), base)
    assert torch.equal(M.augment_mix(*aug_args, partner, w_mixup, nobox), mix_batch(base, partner, w_mixup, nobox))
    assert torch.equal(M.augment_mix(*aug_args, partner, cut.w, cut.box), mix_batch(base, partner, cut.w, cut.box))
    l0, d0 = C.softmax_xent(logits, la, 0.1)
    l1, d1 = M.softmax_xent_mix(logits, la, lb, torch.ones_like(lam), 0.1)
    assert torch.equal(l0, l1) and torch.equal(d0, d1)
    del base, d0, d1

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
    res = {
        "bench": "mix", "batch": B, "size": S, "source_images": a.source, "classes": V, "iters": a.iters,
        "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "cutmix_mean_box_share": round(box_share, 4),
        "us": {k: round(v, 2) for k, v in us.items()},
        "us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in rounds.items()},
        "counted_bytes": nbytes,
        "GBps": {k: round(nbytes[k] / us[k] * 1e-3, 1) for k in us},
        "over_augment": {k: round(us[k] / us["augment"], 3) for k in
                         ("mix_mixup", "mix_cutmix", "mix_none", "augment_torch_mix")},
        "xent_mix_over_xent": round(us["softmax_xent_mix"] / us["softmax_xent"], 3),
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
