"""Checkpoint save / resume.

Reference (``resnet/main.py:83-85,109-112``): rank 0 ``torch.save(ddp_model.state_dict(),
model_dir/model_filename)``; resume with ``torch.load(path, map_location={"cuda:0":
"cuda:r"})`` + strict ``ddp_model.load_state_dict``.  The file written here is
byte-compatible in schema: zip pickle, ``module.``-prefixed
torchvision keys, OIHW contiguous fp32 conv weights (our channels_last / flat
storage is converted on the way out), int64 ``num_batches_tracked``.

Reference defect D10 (resume restores weights only) is fixed without touching
that schema: optimizer state and the next epoch go to a SEPARATE sidecar file
``<checkpoint>.train_state.pt``.

A weight EMA (``optim.ModelEma``) goes to a file of its own next to the checkpoint,
``<name>.ema<ext>`` -- the same schema, so the reference's loader reads it -- and its update count and
settings to the sidecar's ``"ema"`` entry.  The main file is the same with and without an EMA.
"""
from __future__ import annotations

import os
from typing import Optional

import torch


def portable_state_dict(module: torch.nn.Module) -> dict:
    """state_dict with every tensor detached, contiguous (OIHW) and on the CPU."""
    out = {}
    for k, v in module.state_dict().items():
        out[k] = v.detach().contiguous().cpu() if isinstance(v, torch.Tensor) else v
    return out


def sidecar_path(path: str) -> str:
    return path + ".train_state.pt"


def ema_path(path: str) -> str:
    """``dir/name.pth`` -> ``dir/name.ema.pth``."""
    root, ext = os.path.splitext(path)
    return root + ".ema" + ext


def save_checkpoint(module: torch.nn.Module, path: str, optimizer: Optional[torch.optim.Optimizer] = None,
                    epoch: Optional[int] = None, ema=None) -> None:
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    tmp = path + ".tmp"
    torch.save(portable_state_dict(module), tmp)
    os.replace(tmp, path)
    if ema is not None:
        tmp = ema_path(path) + ".tmp"
        torch.save({k: v.detach().contiguous().cpu() if isinstance(v, torch.Tensor) else v
                    for k, v in ema.state_dict().items()}, tmp)
        os.replace(tmp, ema_path(path))
    if optimizer is not None or epoch is not None or ema is not None:
        side = {"epoch": epoch}
        if optimizer is not None:
            side["optimizer"] = optimizer.state_dict()
        if ema is not None:
            side["ema"] = ema.extra_state()
        torch.save(side, sidecar_path(path) + ".tmp")
        os.replace(sidecar_path(path) + ".tmp", sidecar_path(path))


def load_checkpoint(module: torch.nn.Module, path: str, device: torch.device,
                    optimizer: Optional[torch.optim.Optimizer] = None, strict: bool = True,
                    ema=None) -> Optional[int]:
    """Load weights (strict); returns the epoch to resume from if the sidecar exists.  ``ema``: also
    restored from its own file; without that file it starts over from the loaded weights."""
    sd = torch.load(path, map_location=device, weights_only=True)
    module.load_state_dict(sd, strict=strict)
    side = sidecar_path(path)
    st = torch.load(side, map_location=device, weights_only=True) if os.path.exists(side) else None
    if ema is not None:
        if os.path.exists(ema_path(path)):
            ema.load_state_dict(torch.load(ema_path(path), map_location=device, weights_only=True))
            if st is not None and st.get("ema") is not None:
                ema.load_extra_state(st["ema"])
        else:
            ema.reset()
            print("No EMA checkpoint at {}: the EMA starts from the loaded weights".format(ema_path(path)),
                  flush=True)
    if st is not None:
        if optimizer is not None and st.get("optimizer") is not None:
            optimizer.load_state_dict(st["optimizer"])
        return st.get("epoch")
    return None
