#!/usr/bin/env python3
"""Record the launch policy of the implicit-GEMM convolutions from the introspection ops of `_C`.

    python scripts/dump_nt_plan.py [--write]

Two tables, both computed on the host (needs no GPU):

* ``resnet``: every convolution of torchvision's ResNet-18 and ResNet-50 at (batch, resolution) =
  (256, 224), (32, 112) and (128, 32).  Per convolution: the forward GEMM's ``conv_nt_tile`` and
  ``conv_nt_group_rows`` at bf16 and at fp8 operand bytes, the same for every non-empty parity class
  of its input gradient, ``conv_wgrad_plan`` (atomic and deterministic) and, where ``C % 16 == 0 and
  K % 64 == 0``, ``conv_wgrad_fp8_plan``.  The stem is recorded as the super-pixel GEMM the forward
  runs (8-channel pixels, 7 x 4 taps); it has no input gradient, and its weight gradient has a
  launcher of its own (stem.hip), so only its forward GEMM is listed.
* ``grid``: ``conv_nt_tile`` / ``conv_nt_group_rows`` over the product of M, Nout and B-row bytes
  that straddle every constant of the tile policy, under no override, ``conv_nt_force(-1, 0, -1)``
  (no 128x256 tile) and ``conv_nt_force(-1, -1, 0)`` (no 256x256 tile).

`--write` refreshes tests/golden/nt_plan.json (tests/test_nt_plan_cpu.py compares against it);
without it the JSON goes to stdout.
"""
from __future__ import annotations

import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "nt_plan.json")

CONFIGS = [(256, 224), (32, 112), (128, 32)]  # (batch, resolution)
GRID_M = [64, 8192, 8193, 50175, 50176, 50177, 786431, 786432]
GRID_NOUT = [8, 64, 72, 128, 248, 256, 264, 512, 2048]
GRID_KG_BYTES = [64, 128, 255, 256, 257, 1024, 1025, 1152, 4608]
GRID_FORCE = {"policy": (-1, -1, -1), "mid_off": (-1, 0, -1), "wide_off": (-1, -1, 0)}


def _out(n: int, k: int, stride: int, pad: int) -> int:
    return (n + 2 * pad - k) // stride + 1


def resnet_convs(model: str, res: int) -> list:
    """(name, H, W, C, K, R, S, stride, pad) of every convolution after the stem, in module order."""
    block, layers = {"resnet18": ("basic", [2, 2, 2, 2]), "resnet50": ("bottleneck", [3, 4, 6, 3])}[model]
    exp = 1 if block == "basic" else 4
    h = _out(_out(res, 7, 2, 3), 3, 2, 1)  # stem conv, then the 3x3/s2/p1 max pool
    convs, cin = [], 64
    for li, (planes, nblocks) in enumerate(zip([64, 128, 256, 512], layers), start=1):
        for bi in range(nblocks):
            stride = 2 if (li > 1 and bi == 0) else 1
            name = f"layer{li}.{bi}"
            ho = _out(h, 3, stride, 1)
            if block == "basic":
                convs.append((f"{name}.conv1", h, h, cin, planes, 3, 3, stride, 1))
                convs.append((f"{name}.conv2", ho, ho, planes, planes, 3, 3, 1, 1))
            else:
                convs.append((f"{name}.conv1", h, h, cin, planes, 1, 1, 1, 0))
                convs.append((f"{name}.conv2", h, h, planes, planes, 3, 3, stride, 1))
                convs.append((f"{name}.conv3", ho, ho, planes, planes * exp, 1, 1, 1, 0))
            if stride != 1 or cin != planes * exp:
                convs.append((f"{name}.downsample", h, h, cin, planes * exp, 1, 1, stride, 0))
            cin, h = planes * exp, ho
    return convs


def _nt(C, M: int, nout: int, kg: int) -> dict:
    """The NT launch of a GEMM with kg reduction elements per B row, at bf16 and at fp8 bytes."""
    return {"M": M,
            "bf16": {"tile": list(C.conv_nt_tile(M, nout, kg * 2)), "rows": C.conv_nt_group_rows(M, nout, kg * 2)},
            "fp8": {"tile": list(C.conv_nt_tile(M, nout, kg)), "rows": C.conv_nt_group_rows(M, nout, kg)}}


def _conv_entry(C, model: str, batch: int, res: int, conv: tuple) -> dict:
    name, h, w, c, k, r, s, stride, pad = conv
    ho, wo = _out(h, r, stride, pad), _out(w, s, stride, pad)
    e = {"model": model, "batch": batch, "res": res, "name": name,
         "shape": [batch, h, w, c, k, r, s, stride, pad],
         "fwd": _nt(C, batch * ho * wo, k, r * s * c), "dgrad": []}
    for ph, pw in itertools.product(range(stride), repeat=2):
        mi, mj = (h - ph + stride - 1) // stride, (w - pw + stride - 1) // stride
        if mi > 0 and mj > 0:
            e["dgrad"].append(dict(_nt(C, batch * mi * mj, c, r * s * k), parity=[ph, pw]))
    xs, ws = [batch, h, w, c], [k, c, r, s]
    e["wgrad"] = dict(C.conv_wgrad_plan(xs, ws, stride, pad, False))
    e["wgrad_det"] = dict(C.conv_wgrad_plan(xs, ws, stride, pad, True))
    e["wgrad_fp8"] = dict(C.conv_wgrad_fp8_plan(xs, ws, stride, pad)) if c % 16 == 0 and k % 64 == 0 else None
    return e


def collect(C) -> dict:
    C.conv_nt_force(-1, -1, -1)
    resnet = []
    for model in ("resnet18", "resnet50"):
        for batch, res in CONFIGS:
            ho = _out(res, 7, 2, 3)
            resnet.append({"model": model, "batch": batch, "res": res, "name": "conv1 (super-pixel)",
                           "shape": [batch, res + 6, ho + 3, 8, 64, 7, 4, 2, 0],
                           "fwd": _nt(C, batch * ho * ho, 64, 7 * 4 * 8)})
            resnet += [_conv_entry(C, model, batch, res, conv) for conv in resnet_convs(model, res)]
    grid = {}
    try:
        for key, force in GRID_FORCE.items():
            C.conv_nt_force(*force)
            grid[key] = [[m, n, kb, *C.conv_nt_tile(m, n, kb), C.conv_nt_group_rows(m, n, kb)]
                         for m, n, kb in itertools.product(GRID_M, GRID_NOUT, GRID_KG_BYTES)]
    finally:
        C.conv_nt_force(-1, -1, -1)
    return {"resnet": resnet, "grid_columns": ["M", "Nout", "kg_bytes", "bm", "bn", "rows"], "grid": grid}


def dumps(plan: dict) -> str:
    """One line per convolution and per grid point."""
    row = lambda v: json.dumps(v, sort_keys=True)
    out = ['{\n "resnet": [\n' + ",\n".join("  " + row(e) for e in plan["resnet"]) + "\n ],",
           ' "grid_columns": ' + row(plan["grid_columns"]) + ",", ' "grid": {']
    keys = list(plan["grid"])
    for i, key in enumerate(keys):
        out.append(f'  "{key}": [\n' + ",\n".join("   " + row(r) for r in plan["grid"][key]) + "\n  ]"
                   + ("," if i + 1 < len(keys) else ""))
    return "\n".join(out) + "\n }\n}\n"


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else argv
    sys.path.insert(0, ROOT)
    from pytorch_distributed_tutorials_amd.ops import _ext
    text = dumps(json.loads(json.dumps(collect(_ext.native()))))
    if "--write" in argv:
        os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
        with open(GOLDEN, "w") as f:
            f.write(text)
        print(GOLDEN)
    else:
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
