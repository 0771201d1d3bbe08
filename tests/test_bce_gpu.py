"""The fused binary cross-entropy head on the GPU against the same expression in fp64.

Bound of every comparison: the kernel's maximum error may be at most 4x the maximum error of
``ops/reference.py`` run in fp32 on the device, both measured against fp64 on the case itself, with
floors of 4 fp32 ulps of the scale (2^-21 |loss| for the loss, 2^-22 scale for the gradients, which
are bounded by the scale).

Measured on an MI355X, worst over the 40 cases of ``test_kernel_against_fp64``:
  dlogits  kernel error / reference error 1.00 (never above the reference), at most 0.73 of the floor;
  loss     kernel error / reference error 3.2 where the reference happens to land within 0.05 of the
           floor; the kernel's error is at most 0.15 of the floor, the reference's at most 0.26.
``test_training_step_weight_gradient``: both paths 1.757e-04 from fp64 (the bf16 MFMA of the fc
weight gradient), ratio 1.00.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_tutorials_amd import ops
from pytorch_distributed_tutorials_amd.data.mix import MixedTarget
from pytorch_distributed_tutorials_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

# a single row; a partial block of rows; C below one wave with unaligned rows; the 16-byte path; the
# unaligned path with a tail; more than one column tile per lane
SHAPES = [(1, 10), (5, 10), (7, 1000), (6, 1001), (9, 4100)]
S = 0.1
LAMS = (1.0, 0.75, 0.5, 0.25, 0.1, 0.0)


@functools.lru_cache(maxsize=None)
def _case(n, c):
    """Device inputs of one shape: logits randn * 8 with saturated entries (+-100), labels with
    a == b rows, lam cycling through LAMS."""
    g = torch.Generator().manual_seed(1000 * n + c)
    z = torch.randn(n, c, generator=g) * 8
    if n > 2:
        z[0], z[1] = 100.0, -100.0
    else:
        z[0, :3], z[0, 3:6] = 100.0, -100.0
    a = torch.randint(0, c, (n,), generator=g)
    b = torch.randint(0, c, (n,), generator=g)
    b[::3] = a[::3]
    lam = torch.tensor(LAMS)[torch.arange(n) % len(LAMS)]
    return tuple(t.cuda() for t in (z, a, b, lam))


def _fp64(z, a, b, lam, thr, sum_classes):
    """(loss, dlogits) of the stable expression in fp64 on the dense target."""
    n, c = z.shape
    t = F.one_hot(a, c).double() * (1.0 - S) + S / c
    if lam is not None:
        t = lam.double()[:, None] * t + (1.0 - lam.double())[:, None] * (F.one_hot(b, c).double() * (1.0 - S) + S / c)
    assert (t - 0.2).abs().min() >= 1e-3  # no target sits on the threshold
    if thr is not None:
        t = (t > thr).double()
    z = z.double()
    scale = 1.0 / n if sum_classes else 1.0 / (n * c)
    loss = (z.clamp_min(0) - z * t + torch.log1p(torch.exp(-z.abs()))).sum() * scale
    return loss, (torch.sigmoid(z) - t) * scale, scale


def _within(got, fp32_ref, want, floor, what):
    err, err_ref = (got.double() - want).abs().max().item(), (fp32_ref.double() - want).abs().max().item()
    print(f"{what}: kernel error {err:.3e}, fp32 reference error {err_ref:.3e}, floor {floor:.3e}")
    assert err <= max(4.0 * err_ref, floor), (what, err, err_ref, floor)


@pytest.mark.parametrize("thr", [None, 0.2])
@pytest.mark.parametrize("sum_classes", [False, True])
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("n,c", SHAPES)
def test_kernel_against_fp64(gpu, n, c, mixed, sum_classes, thr):
    z, a, b, lam = _case(n, c)
    b, lam = (b, lam) if mixed else (None, None)
    want_loss, want_dz, scale = _fp64(z, a, b, lam, thr, sum_classes)
    args = (b, lam, S, -1.0 if thr is None else thr, sum_classes)
    loss, dz = ops.native_loss().bce_with_logits(z, a, *args)
    ref_loss, ref_dz = ref.bce_with_logits(z, a, *args)
    assert torch.isfinite(loss) and loss.shape == () and dz.shape == z.shape
    _within(loss, ref_loss, want_loss, 2.0 ** -21 * want_loss.abs().item(), "loss")
    _within(dz, ref_dz, want_dz, 2.0 ** -22 * scale, "dlogits")


@pytest.mark.parametrize("n,c", SHAPES)
def test_repeatable_and_lam_one_is_the_hard_label_call(gpu, n, c):
    z, a, b, lam = _case(n, c)
    op = ops.native_loss().bce_with_logits
    for thr in (-1.0, 0.2):
        first, again = op(z, a, b, lam, S, thr), op(z, a, b, lam, S, thr)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
        hard, one = op(z, a, None, None, S, thr, True), op(z, a, b, torch.ones_like(lam), S, thr, True)
        assert torch.equal(hard[0], one[0]) and torch.equal(hard[1], one[1])


def test_training_step_weight_gradient(gpu):
    """fc.weight.grad of one backward through avgpool_linear: the fused loss and the fp32 reference
    loss in its place, both against dlogits^T . pooled in fp64."""
    g = torch.Generator().manual_seed(7)
    n, c, k = 6, 10, 64
    x = torch.randn(n, 2, 2, k, generator=g).to(torch.bfloat16).cuda()
    w0, bias0 = (torch.randn(c, k, generator=g) * 4).cuda(), torch.randn(c, generator=g).cuda()
    a, b = torch.randint(0, c, (n,), generator=g).cuda(), torch.randint(0, c, (n,), generator=g).cuda()
    lam = torch.tensor(LAMS).cuda()
    grads = []
    for fused in (True, False):
        w, bias = w0.clone().requires_grad_(), bias0.clone().requires_grad_()
        logits = ops.avgpool_linear(x, w, bias)
        if fused:
            ops.BCEWithLogitsLoss(S, 0.2)(logits, MixedTarget(a, b, lam)).backward()
        else:
            logits.backward(ref.bce_with_logits(logits.detach(), a, b, lam, S, 0.2)[1])
        grads.append(w.grad)
    _, dz64, scale = _fp64(logits.detach(), a, b, lam, 0.2, False)
    pooled = x.double().mean(dim=(1, 2))
    _within(grads[0], grads[1], dz64.t() @ pooled, 2.0 ** -22 * scale * pooled.abs().sum(0).max().item(),
            "fc.weight.grad")
