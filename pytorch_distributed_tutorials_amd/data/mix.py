"""MixUp and CutMix on a batch: the semantics in plain PyTorch.

torchvision v2's ``MixUp`` / ``CutMix`` with the draws made per sample, applied to the batch the
loader yields (after crop, flip and normalise).  Sample ``b`` is paired with ``partner[b]``
(``(b - 1) mod B``: torchvision's ``roll(1, 0)``) and, independently of its neighbours,

* with probability ``prob`` it is mixed at all;
* it takes CutMix when ``cutmix_alpha > 0`` and (``mixup_alpha == 0`` or a draw falls below
  ``switch_prob``), MixUp otherwise;
* ``lam0 ~ Beta(alpha, alpha)`` from two gamma draws (0.5 when both underflow to 0);
* CutMix pastes the partner inside torchvision's box (centre uniform over the image, half sides
  ``int(0.5 sqrt(1 - lam0) * H)`` and ``... * W``, clipped) and sets ``lam`` to the share of the
  image the sample keeps; MixUp blends ``a * lam0 + partner * (1 - lam0)``.

This module is the oracle of the fused HIP kernel (``csrc/mix/mix.hip``) and the CPU path; both
loader paths draw through ``draw_mix`` and so agree bit for bit.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch


class MixConfig(NamedTuple):
    mixup_alpha: float = 0.0
    cutmix_alpha: float = 0.0
    prob: float = 1.0
    switch_prob: float = 0.5

    def validate(self) -> "MixConfig":
        if self.mixup_alpha < 0 or self.cutmix_alpha < 0:
            raise ValueError(f"mixup/cutmix alpha must be >= 0, got {self.mixup_alpha}, {self.cutmix_alpha}")
        if not 0.0 <= self.prob <= 1.0 or not 0.0 <= self.switch_prob <= 1.0:
            raise ValueError(f"mix prob / switch_prob must be in [0, 1], got {self.prob}, {self.switch_prob}")
        return self

    @property
    def enabled(self) -> bool:
        return self.mixup_alpha > 0 or self.cutmix_alpha > 0


class MixedTarget(NamedTuple):
    """The target ``lam * onehot(labels_a) + (1 - lam) * onehot(labels_b)``, row by row."""
    labels_a: torch.Tensor  # int64 [B]
    labels_b: torch.Tensor  # int64 [B]
    lam: torch.Tensor       # fp32 [B]

    def to(self, *args, **kwargs) -> "MixedTarget":
        return MixedTarget(*(t.to(*args, **kwargs) for t in self))


class MixDraw(NamedTuple):
    partner: torch.Tensor  # int64 [B] batch positions
    w: torch.Tensor        # fp32 [B] blend weight of the sample itself (1 = no blend)
    box: torch.Tensor      # int32 [B, 4] = (y1, y2, x1, x2), half-open; empty = all zeros
    lam: torch.Tensor      # fp32 [B] weight of labels_a in the target


def draw_mix(b: int, H: int, W: int, mixup_alpha: float, cutmix_alpha: float, prob: float, switch_prob: float,
             device, gen: Optional[torch.Generator]) -> MixDraw:
    """Per-sample mixing decisions as device tensors, with no host synchronisation.  The number
    and order of the draws depend on ``b`` alone, never on what was drawn."""
    dev = torch.device(device)
    partner = (torch.arange(b, device=dev) - 1) % max(b, 1)
    apply = torch.rand((b,), device=dev, generator=gen) < prob
    switch = torch.rand((b,), device=dev, generator=gen) < switch_prob
    if cutmix_alpha > 0 and mixup_alpha > 0:
        cut = switch
    else:
        cut = torch.full((b,), bool(cutmix_alpha > 0), device=dev)
    if not (cutmix_alpha > 0 or mixup_alpha > 0):
        apply = torch.zeros_like(apply)
    # Beta(alpha, alpha) = g1 / (g1 + g2) for two Gamma(alpha, 1) draws; a placeholder alpha of 1
    # keeps the gamma sampler in its domain for a method that is switched off
    alpha = torch.where(cut, torch.full((b,), float(cutmix_alpha) if cutmix_alpha > 0 else 1.0, device=dev),
                        torch.full((b,), float(mixup_alpha) if mixup_alpha > 0 else 1.0, device=dev))
    g1 = torch._standard_gamma(alpha, generator=gen)
    g2 = torch._standard_gamma(alpha, generator=gen)
    s = g1 + g2
    ok = (s > 0) & torch.isfinite(s)
    lam0 = torch.where(ok, g1 / torch.where(ok, s, torch.ones_like(s)), torch.full_like(s, 0.5)).clamp_(0.0, 1.0)
    cy = torch.randint(0, H, (b,), device=dev, generator=gen)
    cx = torch.randint(0, W, (b,), device=dev, generator=gen)
    r = 0.5 * torch.sqrt(1.0 - lam0)
    hh = (r * H).to(torch.int64)
    hw = (r * W).to(torch.int64)
    y1, y2 = (cy - hh).clamp_(min=0), (cy + hh).clamp_(max=H)
    x1, x2 = (cx - hw).clamp_(min=0), (cx + hw).clamp_(max=W)
    use_box = apply & cut
    box = torch.stack([y1, y2, x1, x2], dim=1) * use_box[:, None]
    area = ((x2 - x1) * (y2 - y1)).float()
    one = torch.ones_like(lam0)
    lam_cut = 1.0 - area / float(H * W)
    lam = torch.where(apply, torch.where(cut, lam_cut, lam0), one)
    w = torch.where(apply & ~cut, lam0, one)
    return MixDraw(partner, w, box.to(torch.int32), lam)


def mix_batch(a: torch.Tensor, partner: torch.Tensor, w: torch.Tensor, box: torch.Tensor) -> torch.Tensor:
    """Inside ``box[b]``: the partner's pixel.  Elsewhere ``a[b]`` when ``w[b] == 1``, else
    ``a[b] * w[b] + a[partner[b]] * (1 - w[b])`` with both products rounded on their own (no fused
    multiply-add) and ``1 - w`` computed in fp32."""
    B, _, H, W = a.shape
    p = a.index_select(0, partner)
    ys = torch.arange(H, device=a.device).view(1, H, 1)
    xs = torch.arange(W, device=a.device).view(1, 1, W)
    bx = box.to(torch.int64)
    inside = ((ys >= bx[:, 0].view(B, 1, 1)) & (ys < bx[:, 1].view(B, 1, 1)) &
              (xs >= bx[:, 2].view(B, 1, 1)) & (xs < bx[:, 3].view(B, 1, 1)))[:, None]
    wv = w.to(a.dtype).view(B, 1, 1, 1)
    blend = a * wv + p * (1.0 - wv)
    return torch.where(inside, p, torch.where(wv == 1, a, blend))
