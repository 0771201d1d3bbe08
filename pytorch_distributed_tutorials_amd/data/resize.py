"""The ImageNet input transforms, crop-then-resize: the semantics in plain PyTorch.

Training uses torchvision's ``RandomResizedCrop(size, scale, ratio)`` + ``RandomHorizontalFlip``,
evaluation a centre crop by ``crop_pct`` resized to the output size (timm's ``crop_pct`` form of
``Resize(256) + CenterCrop(224)``).  Both are one parameterisation -- a box ``(y0, x0, h, w)`` per
sample, resized to a fixed ``OH x OW`` -- so one kernel serves both (``csrc/img/resample.hip``).

The resize is ATen's antialiased bilinear filter
(``F.interpolate(mode="bilinear", antialias=True, align_corners=False)``) over the box alone: taps
are clipped to the box, as in torchvision's ``resized_crop`` (crop first, then resize).  Resampling
runs in floating point on the ``[0, 1]`` image with no rounding back to uint8 in between, so a
result differs from the PIL chain (which stores the resized image as uint8 before ``ToTensor``) by
at most 0.5/255 per pixel.

This module is the oracle of the fused HIP kernel and the CPU / torch path of the loader; both
loader paths draw through ``draw_rrc`` and so see the same boxes.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import torch

Size = Union[int, Tuple[int, int]]


def _hw(size: Size) -> Tuple[int, int]:
    h, w = (size, size) if isinstance(size, int) else size
    if int(h) != h or int(w) != w or h < 1 or w < 1:
        raise ValueError(f"output size must be a positive int or (h, w) pair, got {size!r}")
    return int(h), int(w)


@dataclass(frozen=True)
class RandomResizedCrop:
    """Training transform: a random box of ``scale`` x the image area and aspect (w / h) in ``ratio``
    (log-uniform), resized to ``size``, then a horizontal flip with probability 0.5."""
    size: Size
    scale: Tuple[float, float] = (0.08, 1.0)
    ratio: Tuple[float, float] = (3.0 / 4.0, 4.0 / 3.0)

    def validate(self) -> "RandomResizedCrop":
        _hw(self.size)
        s0, s1 = self.scale
        r0, r1 = self.ratio
        if not 0.0 < s0 <= s1 <= 1.0:
            raise ValueError(f"RandomResizedCrop scale must be 0 < lo <= hi <= 1, got {tuple(self.scale)}")
        if not 0.0 < r0 <= r1 or not math.isfinite(r1):
            raise ValueError(f"RandomResizedCrop ratio must be 0 < lo <= hi, got {tuple(self.ratio)}")
        return self

    @property
    def out_hw(self) -> Tuple[int, int]:
        return _hw(self.size)


@dataclass(frozen=True)
class CenterCropResize:
    """Evaluation transform: the centred box of ``crop_pct`` x each side, resized to ``size``."""
    size: Size
    crop_pct: float = 0.875

    def validate(self) -> "CenterCropResize":
        _hw(self.size)
        if not 0.0 < self.crop_pct <= 1.0:
            raise ValueError(f"CenterCropResize crop_pct must be in (0, 1], got {self.crop_pct}")
        return self

    @property
    def out_hw(self) -> Tuple[int, int]:
        return _hw(self.size)


def _box_weights(start: torch.Tensor, size: torch.Tensor, n_full: int, n_out: int, dtype) -> torch.Tensor:
    """``[B, n_out, n_full]``: row ``i`` of sample ``b`` holds the weights of output ``i`` over the full
    axis, zero outside the taps of the sample's interval ``[start, start + size)``."""
    dev = size.device
    scale = size.to(dtype) / n_out
    support = scale.clamp(min=1.0)
    inv = (1.0 / support)[:, None, None]
    center = scale[:, None] * (torch.arange(n_out, device=dev, dtype=dtype) + 0.5)   # [B, n_out]
    lo = (center - support[:, None] + 0.5).to(torch.int64).clamp_(min=0)
    hi = torch.minimum((center + support[:, None] + 0.5).to(torch.int64), size.to(torch.int64)[:, None])
    j = (torch.arange(n_full, device=dev) - start.to(torch.int64)[:, None])[:, None, :]  # [B, 1, n_full], box-relative
    w = (1.0 - ((j.to(dtype) - center[:, :, None] + 0.5) * inv).abs()).clamp_(min=0.0)
    w = w * ((j >= lo[:, :, None]) & (j < hi[:, :, None])).to(dtype)
    return w / w.sum(dim=2, keepdim=True)


def resample_weights(n_in: int, n_out: int, dtype=torch.float32) -> torch.Tensor:
    """``[n_out, n_in]`` antialiased-bilinear weights of ATen's separable resize of ``n_in`` pixels
    to ``n_out``: with ``scale = n_in / n_out`` and ``support = max(scale, 1)``, output ``i`` takes
    the taps ``j`` in ``[max(0, int(c - support + 0.5)), min(n_in, int(c + support + 0.5)))`` around
    ``c = scale * (i + 0.5)`` with weights ``max(0, 1 - |j - c + 0.5| / support)``, divided by their
    sum.  At ``n_in == n_out`` it is the identity matrix exactly."""
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resample_weights: sizes must be positive, got {n_in} -> {n_out}")
    return _box_weights(torch.zeros(1, dtype=torch.int64), torch.tensor([n_in]), n_in, n_out, dtype)[0]


def resized_crop(x: torch.Tensor, box: torch.Tensor, out_hw: Size,
                 flip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[b] = Wy(h_b -> OH) @ x[b, :, y0:y0+h, x0:x0+w] @ Wx(w_b -> OW)^T``, flipped along x where
    ``flip[b]``.  ``x``: float ``[B, C, H, W]`` (a uint8 source already divided by 255); ``box``:
    integer ``[B, 4]`` rows ``(y0, x0, h, w)`` inside the image.  Batched (the weight matrices span
    the full axes and are zero outside the box), no host synchronisation."""
    if not x.is_floating_point() or x.dim() != 4:
        raise ValueError("resized_crop: x must be a float [B, C, H, W] tensor")
    B, _, H, W = x.shape
    if box.dim() != 2 or box.shape[0] != B or box.shape[1] != 4 or box.is_floating_point():
        raise ValueError(f"resized_crop: box must be an integer [B, 4] tensor, got {tuple(box.shape)} {box.dtype}")
    oh, ow = _hw(out_hw)
    box = box.to(x.device)
    wy = _box_weights(box[:, 0], box[:, 2], H, oh, x.dtype)   # [B, OH, H]
    wx = _box_weights(box[:, 1], box[:, 3], W, ow, x.dtype)   # [B, OW, W]
    out = torch.matmul(torch.matmul(wy[:, None], x), wx[:, None].transpose(2, 3))
    if flip is not None:
        out = torch.where(flip.to(x.device)[:, None, None, None], out.flip(3), out)
    return out


def draw_rrc(b: int, H: int, W: int, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), device="cpu",
             gen: Optional[torch.Generator] = None) -> torch.Tensor:
    """torchvision's ``RandomResizedCrop.get_params`` for a batch: int32 ``[b, 4]`` boxes
    ``(y0, x0, h, w)``, as device tensors with no host synchronisation.

    Draw order (it depends on ``b`` alone, never on what was drawn): the areas of all ten attempts,
    ``rand [b, 10]``; their log-ratios, ``rand [b, 10]``; the row offsets, ``rand [b]``; the column
    offsets, ``rand [b]``.  The loader draws the flips after this, from the same generator.

    Attempt ``k`` has ``area = H W U(scale)``, ``r = exp(U(log r0, log r1))``, ``w = round(sqrt(area r))``,
    ``h = round(sqrt(area / r))`` and is valid iff ``0 < w <= W and 0 < h <= H``; a sample takes its
    first valid attempt and offsets uniform in ``[0, H - h]``, ``[0, W - w]``.  A sample with no valid
    attempt takes torchvision's centred fallback: ``w = W, h = round(W / r0)`` when ``W / H < r0``,
    ``h = H, w = round(H r1)`` when ``W / H > r1``, the whole image otherwise.  The distribution is
    torchvision's; its Python RNG stream is not reproduced."""
    dev = torch.device(device)
    s0, s1 = float(scale[0]), float(scale[1])
    l0, l1 = math.log(ratio[0]), math.log(ratio[1])
    area = float(H * W) * (s0 + (s1 - s0) * torch.rand((b, 10), device=dev, generator=gen))
    r = torch.exp(l0 + (l1 - l0) * torch.rand((b, 10), device=dev, generator=gen))
    uy = torch.rand((b,), device=dev, generator=gen)
    ux = torch.rand((b,), device=dev, generator=gen)
    w = torch.round(torch.sqrt(area * r)).to(torch.int64)
    h = torch.round(torch.sqrt(area / r)).to(torch.int64)
    ok = (w > 0) & (w <= W) & (h > 0) & (h <= H)
    first = (ok.cumsum(dim=1) == 0).sum(dim=1)           # invalid attempts before the first valid one
    found = first < 10
    first = first.clamp_(max=9)[:, None]
    h, w = h.gather(1, first)[:, 0], w.gather(1, first)[:, 0]
    y0 = (uy * (H - h + 1).to(uy.dtype)).to(torch.int64)
    x0 = (ux * (W - w + 1).to(ux.dtype)).to(torch.int64)
    # the centred fallback, known on the host
    fh, fw = H, W
    if W / H < ratio[0]:
        fh = min(max(int(round(W / ratio[0])), 1), H)
    elif W / H > ratio[1]:
        fw = min(max(int(round(H * ratio[1])), 1), W)
    h = torch.where(found, h, torch.full_like(h, fh))
    w = torch.where(found, w, torch.full_like(w, fw))
    y0 = torch.minimum(torch.where(found, y0, torch.full_like(y0, (H - fh) // 2)), H - h)
    x0 = torch.minimum(torch.where(found, x0, torch.full_like(x0, (W - fw) // 2)), W - w)
    return torch.stack([y0, x0, h, w], dim=1).to(torch.int32)


def center_box(b: int, H: int, W: int, crop_pct: float, device="cpu") -> torch.Tensor:
    """int32 ``[b, 4]``: the centred box of ``round(H crop_pct) x round(W crop_pct)`` for every sample."""
    h = min(max(int(round(H * crop_pct)), 1), H)
    w = min(max(int(round(W * crop_pct)), 1), W)
    row = torch.tensor([(H - h) // 2, (W - w) // 2, h, w], dtype=torch.int32, device=device)
    return row.repeat(b, 1)
