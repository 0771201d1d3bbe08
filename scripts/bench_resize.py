#!/usr/bin/env python3
"""Time the resampling input transform (RandomResizedCrop) on the GPU against the pass it stands in for.

    python scripts/bench_resize.py [--batch 256] [--size 224] [--source-size 256] [--iters 100] [--rounds 5] [--out FILE]

At batch x 3 x size x size output from a uint8 source of source-size pixels (the ImageNet-shaped
step input from a down-sized resident set):

* ``augment``           ``_C.augment`` (pad-crop + flip) on a size-pixel source: the yardstick, it
                        writes the same bytes;
* ``resized_crop_rrc``  ``_C_img.resized_crop`` with ``draw_rrc`` boxes (scale 0.08-1, ratio 3/4-4/3) and flips;
* ``resized_crop_eval`` ``_C_img.resized_crop`` with the centred ``crop_pct`` 0.875 box (at most 2 x 2 taps
                        when source-size x 0.875 <= size: the branch-free body in every wave);
* ``torch_rrc``         the torch-path chain of the loader on the same boxes: index_select, float, /255,
                        ``data.resize.resized_crop`` (two batched matmuls), flip, normalize.

Method of ``scripts/bench_mix.py``: one process, device events, a warm-up, the candidates alternating
round by round, the figure per candidate the median round (a round = ``iters`` back-to-back calls).
Bytes are counted from the shapes -- the source bytes inside the boxes read once, the fp32 batch
written once; the torch chain is given the same count, the least any implementation moves -- so the
rates are counted bytes per second of the call, launches included.
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
    ap.add_argument("--size", type=int, default=224, help="output side")
    ap.add_argument("--source-size", type=int, default=256, help="side of the stored images")
    ap.add_argument("--source", type=int, default=1024, help="images in the device-resident source set")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_bench.json"))
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize needs a GPU")
    from pytorch_distributed_tutorials_amd.data import center_box, draw_rrc, resized_crop
    from pytorch_distributed_tutorials_amd.data.datasets import IMAGENET_MEAN, IMAGENET_STD
    from pytorch_distributed_tutorials_amd.ops._ext import native, native_img

    C, I = native(), native_img()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    B, S, SS = a.batch, a.size, a.source_size
    src = torch.randint(0, 256, (a.source, 3, SS, SS), device=dev, dtype=torch.uint8, generator=g)
    src_s = torch.randint(0, 256, (a.source, 3, S, S), device=dev, dtype=torch.uint8, generator=g)
    idx = torch.randperm(a.source, device=dev, generator=g)[:B].contiguous()
    oy = torch.randint(0, 9, (B,), device=dev, generator=g)
    ox = torch.randint(0, 9, (B,), device=dev, generator=g)
    box = draw_rrc(B, SS, SS, device=dev, gen=g)
    flip = torch.rand((B,), device=dev, generator=g) < 0.5
    ebox = center_box(B, SS, SS, 0.875, dev)
    mean, std = list(IMAGENET_MEAN), list(IMAGENET_STD)
    m = torch.tensor(mean, device=dev).view(1, 3, 1, 1)
    s = torch.tensor(std, device=dev).view(1, 3, 1, 1)

    def torch_rrc():
        x = src.index_select(0, idx).float().div_(255.0)
        return (resized_crop(x, box, (S, S), flip) - m) / s

    cands = {
        "augment": lambda: C.augment(src_s, idx, oy, ox, flip, 4, True, mean, std),
        "resized_crop_rrc": lambda: I.resized_crop(src, idx, box, flip, S, S, True, mean, std),
        "resized_crop_eval": lambda: I.resized_crop(src, idx, ebox, None, S, S, True, mean, std),
        "torch_rrc": torch_rrc,
    }
    out_bytes = 4 * B * 3 * S * S
    rrc_src = 3 * int((box[:, 2].long() * box[:, 3].long()).sum().item())
    eval_src = 3 * int((ebox[:, 2].long() * ebox[:, 3].long()).sum().item())
    nbytes = {"augment": B * 3 * S * S + out_bytes, "resized_crop_rrc": rrc_src + out_bytes,
              "resized_crop_eval": eval_src + out_bytes, "torch_rrc": rrc_src + out_bytes}

    # the candidates compute what they should before they are timed
    # (against the chain in fp64: in fp32 its tap centres near pixel 250 carry 1e-5 of rounding)
    x64 = src.index_select(0, idx).double().div_(255.0)
    chain = (resized_crop(x64, box, (S, S), flip) - m.double()) / s.double()
    dev_rrc = float((cands["resized_crop_rrc"]().double() - chain).abs().max().item())
    assert dev_rrc <= 2e-6 / min(std), dev_rrc
    del x64, chain

    def timed(fn, iters):
        st, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        for _ in range(iters):
            fn()
        e.record()
        e.synchronize()
        return st.elapsed_time(e) * 1e3 / iters  # us per call

    for fn in cands.values():  # warm-up: code objects, allocator pools, clocks
        timed(fn, 10)
    rounds = {k: [] for k in cands}
    for _ in range(a.rounds):
        for k, fn in cands.items():  # alternate the candidates
            rounds[k].append(timed(fn, a.iters))
    us = {k: statistics.median(v) for k, v in rounds.items()}
    bh, bw = box[:, 2].float(), box[:, 3].float()
    res = {
        "bench": "resize", "batch": B, "size": S, "source_size": SS, "source_images": a.source, "iters": a.iters,
        "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
        "rrc_mean_box_share": round(float((bh * bw).mean().item()) / (SS * SS), 4),
        "rrc_downscaled_samples": int(((bh > S) | (bw > S)).sum().item()),
        "rrc_max_abs_diff_to_fp64_chain": dev_rrc,
        "us": {k: round(v, 2) for k, v in us.items()},
        "us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in rounds.items()},
        "counted_bytes": nbytes,
        "GBps": {k: round(nbytes[k] / us[k] * 1e-3, 1) for k in us},
        "over_augment": {k: round(us[k] / us["augment"], 3) for k in ("resized_crop_rrc", "resized_crop_eval", "torch_rrc")},
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
