"""PyTorch reference implementations of every native op (NHWC layout).

Used (a) as the CPU execution path, so the whole framework -- models, DDP,
trainer -- runs and is tested on CPU/gloo without a GPU, and (b) as the fp32
numerics oracle the HIP kernels are checked against in ``tests/test_kernels_gpu.py``.

Layout conventions shared with the kernels (``csrc/kernels/*.hip``):
  activations  [N, H, W, C]  contiguous (NHWC), stem input padded to C=8
  conv weight  [K, C, R, S]  logical OIHW, channels_last memory (= KRSC)
  BN stats     per-channel fp32
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

STEM_CPAD = 8  # channel granule of the kernels' 16-byte loads (8 x bf16)


def image_to_nhwc(x: torch.Tensor, dtype: torch.dtype, cpad: int = STEM_CPAD) -> torch.Tensor:
    n, c, h, w = x.shape
    out = torch.zeros((n, h, w, cpad), dtype=dtype, device=x.device)
    out[..., :c] = x.permute(0, 2, 3, 1).to(dtype)
    return out


def conv2d_nhwc(x: torch.Tensor, w: torch.Tensor, stride: int, pad: int) -> torch.Tensor:
    """x [N,H,W,Cx] (Cx >= w.C; extra channels are zero padding), w [K,C,R,S]."""
    c = w.shape[1]
    xin = x[..., :c].permute(0, 3, 1, 2).float()
    y = F.conv2d(xin, w.float(), stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1)


def conv2d_nhwc_dgrad(dy: torch.Tensor, w: torch.Tensor, x_shape, stride: int, pad: int) -> torch.Tensor:
    n, h, wd, cx = x_shape
    c = w.shape[1]
    g = torch.nn.grad.conv2d_input((n, c, h, wd), w.float(), dy.permute(0, 3, 1, 2).float(),
                                   stride=stride, padding=pad)
    g = g.permute(0, 2, 3, 1)
    if cx != c:
        g = F.pad(g, (0, cx - c))
    return g


def conv2d_nhwc_wgrad(dy: torch.Tensor, x: torch.Tensor, w_shape, stride: int, pad: int) -> torch.Tensor:
    k, c, r, s = w_shape
    xin = x[..., :c].permute(0, 3, 1, 2).float()
    return torch.nn.grad.conv2d_weight(xin, (k, c, r, s), dy.permute(0, 3, 1, 2).float(),
                                       stride=stride, padding=pad)


def bn_batch_stats(y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-channel mean and biased variance over N,H,W (fp32)."""
    yf = y.float().reshape(-1, y.shape[-1])
    mean = yf.mean(0)
    var = yf.var(0, unbiased=False)
    return mean, var


def bn_act_fwd(y: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor, gamma: torch.Tensor,
               beta: torch.Tensor, residual: Optional[torch.Tensor], relu: bool,
               out_dtype: torch.dtype) -> torch.Tensor:
    z = (y.float() - mean) * (invstd * gamma.float()) + beta.float()
    if residual is not None:
        z = z + residual.float()
    if relu:
        z = torch.relu(z)
    return z.to(out_dtype)


def bn_act_bwd(dz: torch.Tensor, z: torch.Tensor, y: torch.Tensor, mean: torch.Tensor,
               invstd: torch.Tensor, gamma: torch.Tensor, relu: bool, training: bool,
               want_dres: bool, out_dtype: torch.dtype):
    """Returns dy, dgamma, dbeta, dres (dres = dz*mask, the residual-branch grad)."""
    g = dz.float()
    if relu:
        g = g * (z.float() > 0)
    c = g.shape[-1]
    g2 = g.reshape(-1, c)
    xhat = ((y.float() - mean) * invstd).reshape(-1, c)
    dbeta = g2.sum(0)
    dgamma = (g2 * xhat).sum(0)
    m = g2.shape[0]
    scale = gamma.float() * invstd
    if training:
        dy = scale * (g2 - dbeta / m - xhat * (dgamma / m))
    else:
        dy = scale * g2
    dy = dy.reshape(g.shape).to(out_dtype)
    dres = g.to(out_dtype) if want_dres else None
    return dy, dgamma, dbeta, dres


def maxpool3x3s2_fwd(x: torch.Tensor) -> torch.Tensor:
    y = F.max_pool2d(x.permute(0, 3, 1, 2).float(), 3, 2, 1)
    return y.permute(0, 2, 3, 1).to(x.dtype).contiguous()


def maxpool3x3s2_bwd(dy: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    xn = x.permute(0, 3, 1, 2).float().detach().requires_grad_(True)
    with torch.enable_grad():
        y = F.max_pool2d(xn, 3, 2, 1)
        (g,) = torch.autograd.grad(y, xn, dy.permute(0, 3, 1, 2).float())
    return g.permute(0, 2, 3, 1).to(x.dtype).contiguous()


def global_avgpool(x: torch.Tensor) -> torch.Tensor:
    return x.float().mean(dim=(1, 2))


def softmax_xent(logits: torch.Tensor, labels: torch.Tensor,
                 label_smoothing: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Mean-reduced cross entropy and its gradient w.r.t. logits.  ``label_smoothing`` eps as in
    ``F.cross_entropy``: the target is (1-eps) onehot + eps/V, so the gradient is
    (softmax - (1-eps) onehot - eps/V) / N."""
    lf = logits.float()
    if label_smoothing == 0.0:
        loss = F.cross_entropy(lf, labels)
        p = torch.softmax(lf, dim=1)
        p[torch.arange(lf.shape[0]), labels] -= 1.0
        return loss, p / lf.shape[0]
    loss = F.cross_entropy(lf, labels, label_smoothing=label_smoothing)
    p = torch.softmax(lf, dim=1) - label_smoothing / lf.shape[1]
    p[torch.arange(lf.shape[0]), labels] -= 1.0 - label_smoothing
    return loss, p / lf.shape[0]


def softmax_xent_mix(logits: torch.Tensor, labels_a: torch.Tensor, labels_b: torch.Tensor, lam: torch.Tensor,
                     label_smoothing: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """``softmax_xent`` against the two-label target lam onehot(a) + (1-lam) onehot(b) (MixUp /
    CutMix, ``data/mix.py``), smoothed as there.  Row loss
    hit (lam (lse - x[a]) + (1-lam) (lse - x[b])) + eps (lse - mean x) with hit = 1 - eps, written
    as the loss on ``labels_a`` plus hit (1-lam) (x[a] - x[b]); gradient
    (softmax - hit lam 1[a] - hit (1-lam) 1[b] - eps/V) / N, the two terms adding where a == b.
    With lam == 1 on every row both are ``softmax_xent(logits, labels_a)`` bit for bit."""
    lf = logits.float()
    n, v = lf.shape
    rows = torch.arange(n, device=lf.device)
    lam = lam.float()
    hit = 1.0 - label_smoothing
    xa, xb = lf[rows, labels_a], lf[rows, labels_b]
    if label_smoothing == 0.0:
        loss = F.cross_entropy(lf, labels_a) + ((1.0 - lam) * (xa - xb)).mean()
        p = torch.softmax(lf, dim=1)
        p[rows, labels_a] -= lam
        p[rows, labels_b] -= 1.0 - lam
        return loss, p / n
    loss = F.cross_entropy(lf, labels_a, label_smoothing=label_smoothing) + hit * ((1.0 - lam) * (xa - xb)).mean()
    p = torch.softmax(lf, dim=1) - label_smoothing / v
    p[rows, labels_a] -= hit * lam
    p[rows, labels_b] -= hit * (1.0 - lam)
    return loss, p / n


def bce_with_logits(logits: torch.Tensor, labels_a: torch.Tensor, labels_b: Optional[torch.Tensor] = None,
                    lam: Optional[torch.Tensor] = None, label_smoothing: float = 0.0,
                    target_threshold: float = -1.0, sum_classes: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Binary cross entropy with logits, every class an independent sigmoid, and its gradient
    w.r.t. the logits.  The target is the smoothed label vector T_x(c) = on if c == x else off with
    off = s / C and on = 1 - s + off, blended per row as lam T_a + (1 - lam) T_b when ``labels_b``
    and ``lam`` are given (T_a alone where a == b), formed in fp32, and binarised to (t > thr) when
    ``target_threshold`` is not negative.  Mean over all elements, or with ``sum_classes`` the sum
    over classes and the mean over rows.  With lam == 1 on every row the result is that of the
    hard-label call bit for bit."""
    if (labels_b is None) != (lam is None):
        raise ValueError("labels_b and lam go together")
    z = logits.float()
    n, c = z.shape
    off = label_smoothing / c
    on = 1.0 - label_smoothing + off
    cols = torch.arange(c, device=z.device)

    def smoothed(x):
        return torch.where(cols[None, :] == x[:, None], on, off).to(torch.float32)

    t = smoothed(labels_a)
    if lam is not None:
        l = lam.float()[:, None]
        t = torch.where((labels_a == labels_b)[:, None], t, l * t + (1.0 - l) * smoothed(labels_b))
    if target_threshold >= 0.0:
        t = (t > torch.tensor(target_threshold, dtype=torch.float32, device=z.device)).to(torch.float32)
    scale = 1.0 / n if sum_classes else 1.0 / (n * c)
    e = torch.exp(-z.abs())
    loss = (z.clamp_min(0.0) - z * t + torch.log1p(e)).sum() * scale
    sig = torch.where(z >= 0, torch.ones_like(e), e) / (1.0 + e)
    return loss, (sig - t) * scale


def top1_correct(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    return (logits.argmax(1) == labels).sum()


def sgd_momentum_(params, grads, bufs, lr: float, momentum: float, dampening: float,
                  weight_decay: float, nesterov: bool, first_step: bool, grad_scale: float = 1.0):
    """torch.optim.SGD semantics (torch/optim/sgd.py:343-380) on lists of tensors."""
    for p, g, b in zip(params, grads, bufs):
        d = g if grad_scale == 1.0 else g * grad_scale
        if weight_decay != 0:
            d = d.add(p, alpha=weight_decay)
        if momentum != 0:
            if first_step:
                b.copy_(d)
            else:
                b.mul_(momentum).add_(d, alpha=1 - dampening)
            d = d.add(b, alpha=momentum) if nesterov else b
        p.add_(d, alpha=-lr)


def lars_trust_ratio(p: torch.Tensor, g: torch.Tensor, weight_decay: float, eta: float, eps: float,
                     excluded: bool) -> float:
    """Layer-wise trust ratio: float32(eta |p| / (|g| + wd |p| + eps)) with the norms and the
    expression in float64; 1 for an excluded tensor and for a zero parameter or gradient norm."""
    if excluded:
        return 1.0
    pn = float(p.detach().double().pow(2).sum().sqrt())
    gn = float(g.detach().double().pow(2).sum().sqrt())
    if pn == 0 or gn == 0:
        return 1.0
    return float(torch.tensor(eta * pn / (gn + weight_decay * pn + eps), dtype=torch.float64).float())


def lars_momentum_(params, grads, bufs, lr: float, momentum: float, dampening: float,
                   weight_decay: float, nesterov: bool, first_step: bool, eta: float = 1e-3,
                   eps: float = 1e-8, exclude_1d: bool = True):
    """LARS as "rescale the gradient, then SGD" on lists of tensors: per tensor
    ``d = trust * (g + wd_eff * p)`` and then ``sgd_momentum_``'s momentum / Nesterov / update, so
    ``bufs`` keep torch.optim.SGD's meaning.  ``exclude_1d``: tensors with ``ndim <= 1`` (BatchNorm
    weights and biases, the fc bias) get neither weight decay nor the trust ratio."""
    for p, g, b in zip(params, grads, bufs):
        excluded = bool(exclude_1d and p.ndim <= 1)
        trust = lars_trust_ratio(p, g, weight_decay, eta, eps, excluded)
        d = g
        if weight_decay != 0 and not excluded:
            d = d.add(p, alpha=weight_decay)
        if trust != 1.0:
            d = d * trust
        sgd_momentum_([p], [d], [b], lr, momentum, dampening, 0.0, nesterov, first_step)


def clip_coef(grads, max_norm: float):
    """``(norm, coef)`` of ``torch.nn.utils.clip_grad_norm_`` over a list of tensors, as Python floats
    from float64 sums of squares: ``norm = sqrt(sum g^2)`` and ``coef = min(max_norm / (norm + 1e-6), 1)``.
    A NaN norm gives a NaN coefficient and an infinite one 0, as torch's clamp does."""
    norm = math.sqrt(sum(float(g.detach().double().pow(2).sum()) for g in grads))
    c = max_norm / (norm + 1e-6)
    return norm, (1.0 if c >= 1.0 else c)


def lamb_(params, grads, exp_avgs, exp_avg_sqs, step: int, lr: float, beta1: float = 0.9, beta2: float = 0.999,
          eps: float = 1e-6, weight_decay: float = 0.0, trust: bool = True, exclude_1d: bool = True,
          grad_coef: float = 1.0, trust_clip: bool = False):
    """LAMB (You et al. 2020) on lists of tensors, update number ``step = 1, 2, ...``; returns the
    trust ratio of every tensor.  Per tensor, with ``bc1 = 1 - beta1**step`` and
    ``bc2 = 1 - beta2**step`` in float64 (a float32 tensor rounds them, and ``sqrt(bc2)``, to float32)::

        m = beta1*m + (1-beta1)*g ;  v = beta2*v + (1-beta2)*g*g
        a = (m/bc1) / (sqrt(v)/sqrt(bc2) + eps)                 # torch.optim.Adam's form
        u = a + wd_eff*p                                        # wd_eff = 0 for an excluded tensor
        ratio = float32(|p| / |u|), norms from float64 sums of squares;
                1 if excluded, or trust is off, or |p| == 0, or |u| == 0
        p = p - lr*ratio*u

    ``exclude_1d``: tensors with ``ndim <= 1`` get neither weight decay nor the ratio, as in
    ``lars_momentum_``.  ``trust=False`` is AdamW (with ``exclude_1d=False``, ``torch.optim.AdamW`` in
    exact arithmetic).  ``grad_coef`` (``clip_coef``'s coefficient) multiplies every gradient first,
    rounded to the tensors' dtype; ``trust_clip`` clamps the ratio at 1.  The gradients are not modified."""
    if step < 1:
        raise ValueError(f"lamb_: update numbers start at 1, got {step}")
    bc1 = 1.0 - beta1 ** step
    sbc2 = (1.0 - beta2 ** step) ** 0.5
    ratios = []
    for p, g, m, v in zip(params, grads, exp_avgs, exp_avg_sqs):
        excluded = bool(exclude_1d and p.ndim <= 1)
        if grad_coef != 1.0:
            g = g * grad_coef
        m.mul_(beta1).add_(g, alpha=1 - beta1)
        v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
        u = (m / bc1) / (v.sqrt() / sbc2 + eps)
        if weight_decay != 0 and not excluded:
            u = u.add(p, alpha=weight_decay)
        ratio = 1.0
        if trust and not excluded:
            pn = float(p.detach().double().pow(2).sum().sqrt())
            un = float(u.double().pow(2).sum().sqrt())
            if pn != 0 and un != 0:
                ratio = float(torch.tensor(pn / un, dtype=torch.float64).float())
            if trust_clip and ratio > 1.0:
                ratio = 1.0
        p.add_(u, alpha=-lr * ratio)
        ratios.append(ratio)
    return ratios
