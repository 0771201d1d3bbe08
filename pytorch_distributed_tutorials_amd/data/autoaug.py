"""TrivialAugmentWide and RandomErasing on a batch: the semantics in plain PyTorch.

torchvision's ``TrivialAugmentWide`` (one of 14 operations per sample, one of 31 magnitudes, a random
sign) and ``RandomErasing(value=0)``, with the draws made per sample on the device.  The policy runs
on the batch after crop and flip and before normalisation, erasing after normalisation, batch mixing
last -- torchvision's order.

The policy works on 8-bit levels, as the PIL chain does (it stores the image as uint8): the fp32
batch ``x`` in ``[0, 1]`` is quantised by ``q = clamp(rint(x * 255), 0, 255)`` (an fp32 product,
round-half-even), every sample included, ``Identity`` too; a sample the policy leaves alone thus
differs from the policy-off batch by at most 0.5/255 before normalisation (the figure
``data/resize.py`` quotes for the PIL chain).

Operations (ids follow torchvision's table; "signed" ones negate the magnitude on a sign draw of 1):

====== ======================== ==================================================== ======
id     op                       magnitude of bin k                                   signed
====== ======================== ==================================================== ======
0      Identity
1, 2   ShearX, ShearY           ``linspace(0, 0.99, 31)[k]``                         yes
3, 4   TranslateX, TranslateY   ``int(linspace(0, 32, 31)[k] * sign)`` pixels        yes
5      Rotate                   ``linspace(0, 135, 31)[k]`` degrees                  yes
6 .. 9 Brightness, Color,       ``linspace(0, 0.99, 31)[k]``; ``ratio = 1 + m``      yes
       Contrast, Sharpness
10     Posterize                ``bits = 8 - round(k / 5)``
11     Solarize                 threshold ``255 - 8.5 k``
12     AutoContrast
13     Equalize
====== ======================== ==================================================== ======

Photometric operations, on levels.  Every "fp32" step is one rounded fp32 operation in the written
order, so that the HIP kernel (``csrc/img/autoaug.hip``) reproduces them bit for bit:

* ``blend(a, b) = trunc(clamp(r * a + r1 * b, 0, 255))``: two products and one sum, with
  ``r = fp32(ratio)`` and ``r1 = fp32(1.0 - ratio)`` (the subtraction in float64, as torchvision's
  Python scalars do);
* ``gray = trunc((0.2989 R + 0.587 G) + 0.114 B)`` in fp32;
* Brightness ``blend(q, 0)``; Color ``blend(q, gray)``; Contrast ``blend(q, mean)`` with
  ``mean = fp32(integer sum of gray) / fp32(H W)``; Sharpness ``blend(q, blurred)`` where on interior
  pixels ``blurred = (2 S + 13) // 26``, ``S`` = the 8 neighbours + 5 x the centre (torchvision's
  rounded convolution with ``[[1, 1, 1], [1, 5, 1], [1, 1, 1]] / 13``), border pixels keep ``q``, and
  an image with a side of 2 or less is returned unchanged;
* Posterize ``q & (0xFF << (8 - bits))``; Solarize ``255 - q`` where ``q >= ceil(threshold)``;
* AutoContrast, per channel with minimum ``lo`` and maximum ``hi``: unchanged when ``hi == lo``, else
  ``trunc(clamp((q - lo) * (255 / (hi - lo)), 0, 255))`` (an fp32 divide, then an fp32 multiply);
* Equalize, per channel in integers: histogram ``h``, ``step = (sum of the non-zero bins but the last
  non-zero one) // 255``, unchanged when ``step == 0``, else
  ``lut[v] = min(255, (cumsum(h)[v - 1] + step // 2) // step)`` with ``lut[0] = 0``.

Geometric operations sample the nearest pixel and fill with black, through an inverse matrix
``m[6]`` (fp32, computed in float64): ShearX ``[1, m, m H / 2, 0, 1, 0]``, ShearY
``[1, 0, 0, m, 1, m W / 2]`` (torchvision's shear about the top-left corner), TranslateX
``[1, 0, -t, 0, 1, 0]``, TranslateY ``[1, 0, 0, 0, 1, -t]``, Rotate
``[cos, -sin, 0, sin, cos, 0]``, the identity otherwise.  For output pixel ``(y, x)``, with
``xc = x + 0.5 - W / 2`` and ``yc = y + 0.5 - H / 2``,

    sx = ((m0 xc + m1 yc) + m2) + (W / 2 - 0.5)        sy = ((m3 xc + m4 yc) + m5) + (H / 2 - 0.5)

every operation rounded to fp32 on its own; the source pixel is ``(rint(sy), rint(sx))``
(half-to-even) and a pixel outside the image is 0.

RandomErasing is torchvision's ``get_params``: ten attempts of ``area = H W U(scale)``,
``aspect = exp(U(log r0, log r1))``, ``h = round(sqrt(area aspect))``, ``w = round(sqrt(area / aspect))``,
valid iff ``h < H and w < W``; the first valid attempt is placed at ``y0 = int(U (H - h + 1))``,
``x0`` likewise, and zeroed after normalisation.  A sample that is not erased has ``h = 0``.

This module is the oracle of the fused HIP kernel and the CPU / torch path of the loader; both loader
paths draw through ``draw_policy`` and so see the same operations.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import torch

NUM_OPS = 14
NUM_BINS = 31
OP_NAMES = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color",
            "Contrast", "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")
(IDENTITY, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS,
 POSTERIZE, SOLARIZE, AUTOCONTRAST, EQUALIZE) = range(NUM_OPS)
POLICIES = ("none", "trivial-wide")
# the largest side the integer statistics (gray sum, histogram) of the fused kernel hold in 32 bits
MAX_SIDE = 4096


class AugConfig(NamedTuple):
    policy: str = "none"
    erase_prob: float = 0.0
    erase_scale: Tuple[float, float] = (0.02, 0.33)
    erase_ratio: Tuple[float, float] = (0.3, 3.3)

    def validate(self) -> "AugConfig":
        if self.policy not in POLICIES:
            raise ValueError(f"augmentation policy must be one of {POLICIES}, got {self.policy!r}")
        if not 0.0 <= self.erase_prob <= 1.0:
            raise ValueError(f"random-erase probability must be in [0, 1], got {self.erase_prob}")
        s0, s1 = self.erase_scale
        r0, r1 = self.erase_ratio
        if not 0.0 < s0 <= s1 <= 1.0:
            raise ValueError(f"random-erase scale must be 0 < lo <= hi <= 1, got {tuple(self.erase_scale)}")
        if not 0.0 < r0 <= r1 or not math.isfinite(r1):
            raise ValueError(f"random-erase ratio must be 0 < lo <= hi, got {tuple(self.erase_ratio)}")
        return self

    @property
    def enabled(self) -> bool:
        return self.policy != "none" or self.erase_prob > 0.0


class AugDraw(NamedTuple):
    op: torch.Tensor      # int32 [B] operation id, 0..13
    param: torch.Tensor   # fp32 [B, 2]: blend ops (r, r1); Posterize (bits, 0); Solarize (ceil(threshold), 0)
    matrix: torch.Tensor  # fp32 [B, 6] inverse matrix of the geometric ops, the identity otherwise
    erase: torch.Tensor   # int32 [B, 4] = (y0, x0, h, w); h = 0: not erased


_TABLES = {}  # device -> the magnitude table, built there once


def magnitude_table(device="cpu") -> torch.Tensor:
    """float64 ``[14, 31]`` on ``device``: the unsigned magnitude of bin ``k`` of every operation.  Built
    on the device itself with torch ops and kept, so a draw copies nothing from the host."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    t = _TABLES.get(dev)
    if t is None:
        def lin(end):
            return torch.linspace(0.0, end, NUM_BINS, dtype=torch.float64, device=dev)

        k = torch.arange(NUM_BINS, dtype=torch.float64, device=dev)
        zero, unit = torch.zeros_like(k), lin(0.99)
        rows = {SHEAR_X: unit, SHEAR_Y: unit, TRANSLATE_X: lin(32.0), TRANSLATE_Y: lin(32.0), ROTATE: lin(135.0),
                BRIGHTNESS: unit, COLOR: unit, CONTRAST: unit, SHARPNESS: unit,
                POSTERIZE: 8.0 - torch.round(k / 5.0), SOLARIZE: 255.0 - 8.5 * k}
        t = _TABLES[dev] = torch.stack([rows.get(i, zero) for i in range(NUM_OPS)])
    return t


def policy_params(op: torch.Tensor, bin_: torch.Tensor, sign: torch.Tensor, H: int, W: int):
    """``(param fp32 [B, 2], matrix fp32 [B, 6])`` of operations ``op`` at bins ``bin_`` with sign draws
    ``sign`` (1 negates a signed magnitude), for ``H x W`` images: float64 torch ops on the device of
    ``op``, then one cast."""
    dev = op.device
    op = op.to(torch.int64)
    mag = magnitude_table(dev)[op, bin_.to(torch.int64)]
    signed = (op >= SHEAR_X) & (op <= SHARPNESS)
    m = torch.where(signed & (sign.to(torch.int64) == 1), -mag, mag)
    zero, one = torch.zeros_like(m), torch.ones_like(m)

    def pick(code, val, other):
        return torch.where(op == code, val, other)

    t = torch.trunc(m)  # whole pixels, toward zero
    th = m * (math.pi / 180.0)
    cos, sin = torch.cos(th), torch.sin(th)
    matrix = torch.stack([
        pick(ROTATE, cos, one),
        pick(SHEAR_X, m, pick(ROTATE, -sin, zero)),
        pick(SHEAR_X, m * (H / 2.0), pick(TRANSLATE_X, -t, zero)),
        pick(SHEAR_Y, m, pick(ROTATE, sin, zero)),
        pick(ROTATE, cos, one),
        pick(SHEAR_Y, m * (W / 2.0), pick(TRANSLATE_Y, -t, zero)),
    ], dim=1).to(torch.float32)
    blend = (op >= BRIGHTNESS) & (op <= SHARPNESS)
    ratio = 1.0 + m
    p0 = torch.where(blend, ratio, pick(POSTERIZE, mag, pick(SOLARIZE, torch.ceil(mag), zero)))
    p1 = torch.where(blend, 1.0 - ratio, zero)
    return torch.stack([p0, p1], dim=1).to(torch.float32), matrix


def draw_erase(b: int, H: int, W: int, prob: float, scale, ratio, device, gen) -> torch.Tensor:
    """torchvision's ``RandomErasing.get_params`` for a batch: int32 ``[b, 4]`` boxes ``(y0, x0, h, w)``,
    all zeros for a sample that is not erased.  Draws ``rand [b]`` (erase at all), ``rand [b, 10]``
    (areas), ``rand [b, 10]`` (log-ratios), ``rand [b]``, ``rand [b]`` (offsets)."""
    dev = torch.device(device)
    s0, s1 = float(scale[0]), float(scale[1])
    l0, l1 = math.log(ratio[0]), math.log(ratio[1])
    apply = torch.rand((b,), device=dev, generator=gen) < prob
    area = float(H * W) * (s0 + (s1 - s0) * torch.rand((b, 10), device=dev, generator=gen))
    aspect = torch.exp(l0 + (l1 - l0) * torch.rand((b, 10), device=dev, generator=gen))
    uy = torch.rand((b,), device=dev, generator=gen)
    ux = torch.rand((b,), device=dev, generator=gen)
    h = torch.round(torch.sqrt(area * aspect)).to(torch.int64)
    w = torch.round(torch.sqrt(area / aspect)).to(torch.int64)
    ok = (h < H) & (w < W)
    first = (ok.cumsum(dim=1) == 0).sum(dim=1)           # invalid attempts before the first valid one
    use = apply & (first < 10)
    first = first.clamp_(max=9)[:, None]
    h, w = h.gather(1, first)[:, 0], w.gather(1, first)[:, 0]
    y0 = torch.minimum((uy * (H - h + 1).to(uy.dtype)).to(torch.int64), H - h)
    x0 = torch.minimum((ux * (W - w + 1).to(ux.dtype)).to(torch.int64), W - w)
    use = use & (h > 0) & (w > 0)
    return (torch.stack([y0, x0, h, w], dim=1) * use[:, None]).to(torch.int32)


def draw_policy(b: int, H: int, W: int, cfg: AugConfig, device="cpu",
                gen: Optional[torch.Generator] = None) -> AugDraw:
    """The per-sample decisions of one batch as device tensors, with no host synchronisation.  The
    number and order of the draws depend on ``b`` and ``cfg`` alone: with a policy ``randint(14) [b]``
    (operation), ``randint(31) [b]`` (bin), ``randint(2) [b]`` (sign); with ``erase_prob > 0`` then the
    five draws of ``draw_erase``."""
    dev = torch.device(device)
    if cfg.policy != "none":
        op = torch.randint(0, NUM_OPS, (b,), device=dev, generator=gen)
        bin_ = torch.randint(0, NUM_BINS, (b,), device=dev, generator=gen)
        sign = torch.randint(0, 2, (b,), device=dev, generator=gen)
    else:
        op = bin_ = sign = torch.zeros((b,), dtype=torch.int64, device=dev)
    param, matrix = policy_params(op, bin_, sign, H, W)
    if cfg.erase_prob > 0.0:
        erase = draw_erase(b, H, W, cfg.erase_prob, cfg.erase_scale, cfg.erase_ratio, dev, gen)
    else:
        erase = torch.zeros((b, 4), dtype=torch.int32, device=dev)
    return AugDraw(op.to(torch.int32), param, matrix, erase)


# ---------------------------------------------------------------------------------- the operations
def quantize(x: torch.Tensor) -> torch.Tensor:
    """fp32 levels ``clamp(rint(x * 255), 0, 255)`` of a ``[0, 1]`` batch."""
    return torch.round(x.to(torch.float32) * 255.0).clamp_(0.0, 255.0)


def _warp(q: torch.Tensor, matrix: torch.Tensor) -> torch.Tensor:
    B, C, H, W = q.shape
    m = matrix.to(torch.float32)[:, :, None, None]                                       # [B, 6, 1, 1]
    xc = (torch.arange(W, device=q.device, dtype=torch.float32) + 0.5 - W / 2.0).view(1, 1, W)
    yc = (torch.arange(H, device=q.device, dtype=torch.float32) + 0.5 - H / 2.0).view(1, H, 1)
    sx = ((m[:, 0] * xc + m[:, 1] * yc) + m[:, 2]) + (W / 2.0 - 0.5)
    sy = ((m[:, 3] * xc + m[:, 4] * yc) + m[:, 5]) + (H / 2.0 - 0.5)
    ix, iy = torch.round(sx), torch.round(sy)
    inside = (ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1)                       # NaN: outside
    zero = torch.zeros_like(ix)
    lin = torch.where(inside, iy, zero).to(torch.int64) * W + torch.where(inside, ix, zero).to(torch.int64)
    lin = lin.view(B, 1, H * W).expand(B, C, H * W)
    return q.reshape(B, C, H * W).gather(2, lin).view(B, C, H, W) * inside[:, None].to(q.dtype)


def _gray(q: torch.Tensor) -> torch.Tensor:
    return torch.trunc((0.2989 * q[:, 0] + 0.587 * q[:, 1]) + 0.114 * q[:, 2])[:, None]   # [B, 1, H, W]


def _blurred(q: torch.Tensor) -> torch.Tensor:
    B, C, H, W = q.shape
    if H <= 2 or W <= 2:
        return q
    qi = q.to(torch.int64)
    s = 4 * qi[:, :, 1:-1, 1:-1]
    for dy in range(3):
        for dx in range(3):
            s = s + qi[:, :, dy:H - 2 + dy, dx:W - 2 + dx]
    out = q.clone()
    out[:, :, 1:-1, 1:-1] = ((2 * s + 13) // 26).to(q.dtype)
    return out


def _autocontrast(q: torch.Tensor) -> torch.Tensor:
    lo = q.amin(dim=(2, 3), keepdim=True)
    hi = q.amax(dim=(2, 3), keepdim=True)
    flat = hi == lo
    # the fp32 quotient, correctly rounded: a float64 quotient of fp32 operands rounds to it
    scale = (255.0 / torch.where(flat, torch.ones_like(hi), hi - lo).to(torch.float64)).to(torch.float32)
    out = torch.trunc(((q - lo) * scale).clamp_(0.0, 255.0))
    return torch.where(flat, q, out)


def _equalize(q: torch.Tensor) -> torch.Tensor:
    B, C, H, W = q.shape
    v = q.to(torch.int64).view(B * C, H * W)
    h = torch.zeros((B * C, 256), dtype=torch.int64, device=q.device).scatter_add_(1, v, torch.ones_like(v))
    last = h.gather(1, v.amax(dim=1, keepdim=True))      # the last non-zero bin
    step = (H * W - last) // 255                          # [B*C, 1]
    safe = step.clamp(min=1)
    lut = torch.clamp((h.cumsum(dim=1) - h + step // 2) // safe, max=255)
    lut[:, 0] = 0
    out = lut.gather(1, v).to(q.dtype)
    return torch.where(step == 0, q.view(B * C, H * W), out).view(B, C, H, W)


def apply_policy_levels(x: torch.Tensor, draw: AugDraw) -> torch.Tensor:
    """The policy alone: uint8 ``[B, 3, H, W]`` levels of the ``[0, 1]`` batch ``x`` after each
    sample's operation, before normalisation and erasing.  Batched, no host synchronisation."""
    if not x.is_floating_point() or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"apply_policy: x must be a float [B, 3, H, W] batch, got {x.dtype} {tuple(x.shape)}")
    B, _, H, W = x.shape
    if draw.op.shape != (B,) or draw.param.shape != (B, 2) or draw.matrix.shape != (B, 6) or \
            draw.erase.shape != (B, 4):
        raise ValueError("apply_policy: the draw is not one of this batch "
                         f"(op {tuple(draw.op.shape)}, param {tuple(draw.param.shape)}, matrix "
                         f"{tuple(draw.matrix.shape)}, erase {tuple(draw.erase.shape)} for {B} samples)")
    op = draw.op.to(x.device).view(B, 1, 1, 1)
    op = torch.where((op < 0) | (op >= NUM_OPS), torch.zeros_like(op), op)   # unknown ids: Identity
    p0 = draw.param.to(x.device, torch.float32)[:, 0].view(B, 1, 1, 1)
    p1 = draw.param.to(x.device, torch.float32)[:, 1].view(B, 1, 1, 1)
    q = quantize(x)
    geometric = (op >= SHEAR_X) & (op <= ROTATE)
    out = torch.where(geometric, _warp(q, draw.matrix.to(x.device)), q)
    # the blend operations: one blend against the operation's second image
    gray = _gray(q)
    mean = (gray.to(torch.int64).sum(dim=(1, 2, 3), keepdim=True).to(torch.float32).to(torch.float64)
            / float(H * W)).to(torch.float32)            # the correctly rounded fp32 quotient
    other = torch.where(op == COLOR, gray, torch.where(op == CONTRAST, mean, torch.where(
        op == SHARPNESS, _blurred(q), torch.zeros_like(q))))
    blend = torch.trunc((p0 * q + p1 * other).clamp_(0.0, 255.0))
    is_blend = (op >= BRIGHTNESS) & (op <= SHARPNESS)
    if H <= 2 or W <= 2:
        is_blend = is_blend & (op != SHARPNESS)
    out = torch.where(is_blend, blend, out)
    qi = q.to(torch.int32)
    shift = (8 - p0.to(torch.int32)).clamp_(0, 8)
    post = (qi & torch.bitwise_left_shift(torch.full_like(shift, 0xFF), shift) & 0xFF).to(q.dtype)
    out = torch.where(op == POSTERIZE, post, out)
    out = torch.where((op == SOLARIZE) & (q >= p0), 255.0 - q, out)
    out = torch.where(op == AUTOCONTRAST, _autocontrast(q), out)
    out = torch.where(op == EQUALIZE, _equalize(q), out)
    return out.to(torch.uint8)


def erase_boxes(x: torch.Tensor, erase: torch.Tensor) -> torch.Tensor:
    """``x`` with the box ``(y0, x0, h, w)`` of every sample set to 0; a box is clipped to the image."""
    B, _, H, W = x.shape
    e = erase.to(x.device, torch.int64)
    ys = torch.arange(H, device=x.device).view(1, H, 1)
    xs = torch.arange(W, device=x.device).view(1, 1, W)
    y0, x0 = e[:, 0].clamp(0, H), e[:, 1].clamp(0, W)
    y1 = (y0 + torch.minimum(e[:, 2].clamp(min=0), H - y0)).view(B, 1, 1)
    x1 = (x0 + torch.minimum(e[:, 3].clamp(min=0), W - x0)).view(B, 1, 1)
    inside = (ys >= y0.view(B, 1, 1)) & (ys < y1) & (xs >= x0.view(B, 1, 1)) & (xs < x1)
    return torch.where(inside[:, None], torch.zeros_like(x), x)


def apply_policy(x: torch.Tensor, draw: AugDraw, mean, std, normalize: bool = True) -> torch.Tensor:
    """The reference of ``_C_img.autoaug``: quantise the ``[0, 1]`` batch, apply each sample's
    operation, return to ``[0, 1]`` (``level / 255``), normalise with ``(p - mean) / std`` when
    ``normalize``, and zero the erase boxes.  fp32 ``[B, 3, H, W]``."""
    out = apply_policy_levels(x, draw).to(torch.float32) / 255.0
    if normalize:
        m = torch.tensor(mean, device=x.device, dtype=torch.float32).view(1, -1, 1, 1)
        s = torch.tensor(std, device=x.device, dtype=torch.float32).view(1, -1, 1, 1)
        out = (out - m) / s
    return erase_boxes(out, draw.erase)
