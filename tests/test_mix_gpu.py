"""MixUp / CutMix on the MI355X: the fused augment_mix kernel against the torch path (bit for bit),
the two-label loss head against F.cross_entropy with soft targets, and one native training step."""
import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_tutorials_amd.data import (DeviceLoader, MixConfig, MixedTarget, TensorImageDataset,
                                                    mix_batch)
from pytorch_distributed_tutorials_amd.data.datasets import CIFAR_MEAN, CIFAR_STD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mix_ext(native_ext):
    from pytorch_distributed_tutorials_amd.ops import _ext
    return _ext.native_mix()


def _dataset(n, h, w, normalized, seed=21):
    g = torch.Generator().manual_seed(seed)
    if normalized:
        imgs = torch.randn(n, 3, h, w, generator=g)
    else:
        imgs = torch.randint(0, 256, (n, 3, h, w), generator=g, dtype=torch.uint8)
    return TensorImageDataset(imgs, torch.randint(0, 10, (n,), generator=g), normalized=normalized)


@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("normalized", [False, True])
@pytest.mark.parametrize("n,h,w", [(40, 32, 32), (16, 16, 24)])
def test_fused_augment_mix_matches_torch_loader(gpu, mix_ext, n, h, w, normalized, augment):
    ds = _dataset(n, h, w, normalized)
    kw = dict(batch_size=16, shuffle=True, augment=augment, device=gpu, seed=3, mix=MixConfig(0.4, 1.0, prob=0.6))
    fused = list(DeviceLoader(ds, fused=True, **kw))
    plain = list(DeviceLoader(ds, fused=False, **kw))
    assert len(fused) == len(plain) == (n + 15) // 16
    assert fused[-1][0].shape[0] == (8 if n == 40 else 16)  # 40 images leave a partial batch of 8
    kinds = set()
    for (xa, ta), (xb, tb) in zip(fused, plain):
        assert isinstance(ta, MixedTarget) and all(torch.equal(p, q) for p, q in zip(ta, tb))
        assert xa.dtype == torch.float32 and xa.shape == xb.shape
        assert torch.equal(xa, xb)
        kinds.add("unmixed" if bool((ta.lam == 1).any()) else "")
        kinds.add("mixed" if bool((ta.lam != 1).any()) else "")
    assert {"unmixed", "mixed"} <= kinds


def _direct_case(gpu, normalized, seed=7):
    """Hand-made operands over 8 samples of 3x8x12: every box / weight / partner case at once."""
    g = torch.Generator().manual_seed(seed)
    if normalized:
        imgs = torch.randn(20, 3, 8, 12, generator=g)
    else:
        imgs = torch.randint(0, 256, (20, 3, 8, 12), generator=g, dtype=torch.uint8)
    B = 8
    idx = torch.randperm(20, generator=g)[:B]
    oy = torch.randint(0, 5, (B,), generator=g)
    ox = torch.randint(0, 5, (B,), generator=g)
    flip = torch.tensor([False, True, False, True, False, False, True, False])
    partner = torch.tensor([1, 0, 2, 6, 4, 3, 5, 7])  # a permutation with fixed points 2, 4, 7
    assert not flip[0] and flip[partner[0]]               # a flipped partner under an unflipped sample
    w = torch.tensor([1.0, 1.0, 0.25, 0.0, 0.25, 1.0, 1.0, 1.0])
    box = torch.tensor([[1, 7, 1, 5],     # x edges 1 and 5
                        [0, 8, 2, 3],     # x edges 2 and 3: one pixel wide, inside one store
                        [0, 0, 0, 0],     # blended, no box
                        [0, 0, 0, 0],     # w = 0: the partner everywhere
                        [0, 0, 0, 0],     # blended with itself
                        [0, 8, 0, 12],    # the full image
                        [3, 4, 3, 11],    # one row, x edges 3 and 11
                        [0, 0, 0, 0]],    # unmixed
                       dtype=torch.int32)
    dev = lambda t: t.to(gpu)  # noqa: E731
    return dict(imgs=dev(imgs), idx=dev(idx), oy=dev(oy), ox=dev(ox), flip=dev(flip), partner=dev(partner), w=dev(w),
                box=dev(box), normalize=not normalized)


@pytest.mark.parametrize("normalized", [False, True])
def test_augment_mix_direct_matches_mix_batch_of_augment(gpu, native_ext, mix_ext, normalized):
    c = _direct_case(gpu, normalized)
    mean, std = list(CIFAR_MEAN), list(CIFAR_STD)
    for flip in (c["flip"], None):
        base = native_ext.augment(c["imgs"], c["idx"], c["oy"], c["ox"], flip, 2, c["normalize"], mean, std)
        got = mix_ext.augment_mix(c["imgs"], c["idx"], c["oy"], c["ox"], flip, 2, c["normalize"], mean, std,
                                  c["partner"], c["w"], c["box"])
        want = mix_batch(base, c["partner"], c["w"], c["box"])
        assert torch.equal(got, want)
        assert not torch.equal(got, base)
        # nothing mixed: bitwise _C.augment, whatever partner holds
        none = mix_ext.augment_mix(c["imgs"], c["idx"], c["oy"], c["ox"], flip, 2, c["normalize"], mean, std,
                                   c["partner"], torch.ones_like(c["w"]), torch.zeros_like(c["box"]))
        assert torch.equal(none, base)
    # B = 1: the sample is its own partner
    one = {k: (v[:1].contiguous() if k not in ("imgs", "normalize") else v) for k, v in c.items()}
    one["partner"] = torch.zeros(1, dtype=torch.long, device=gpu)
    one["w"] = torch.tensor([0.25], device=gpu)
    base = native_ext.augment(one["imgs"], one["idx"], one["oy"], one["ox"], one["flip"], 2, one["normalize"], mean, std)
    got = mix_ext.augment_mix(one["imgs"], one["idx"], one["oy"], one["ox"], one["flip"], 2, one["normalize"], mean,
                              std, one["partner"], one["w"], one["box"])
    assert torch.equal(got, mix_batch(base, one["partner"], one["w"], one["box"]))


def test_augment_mix_checks_its_operands(gpu, mix_ext):
    c = _direct_case(gpu, False)
    mean, std = list(CIFAR_MEAN), list(CIFAR_STD)
    args = [c["imgs"], c["idx"], c["oy"], c["ox"], c["flip"], 2, True, mean, std]
    with pytest.raises(RuntimeError):
        mix_ext.augment_mix(*args, c["partner"][:4].contiguous(), c["w"], c["box"])
    with pytest.raises(RuntimeError):
        mix_ext.augment_mix(*args, c["partner"], c["w"], c["box"].long())
    with pytest.raises(RuntimeError):
        mix_ext.augment_mix(*args, c["partner"], c["w"].cpu(), c["box"])


def soft_target(a, b, lam, v):
    return lam[:, None] * F.one_hot(a, v).float() + (1 - lam)[:, None] * F.one_hot(b, v).float()


def loss_case(n, v, seed=11):
    """Logits 3 * randn, labels with one a == b row, lam holding 0, 1 and interior values."""
    g = torch.Generator().manual_seed(seed + n + v)
    logits = 3 * torch.randn(n, v, generator=g)
    a = torch.randint(0, v, (n,), generator=g)
    b = torch.randint(0, v, (n,), generator=g)
    b[n - 1] = a[n - 1]
    lam = torch.rand(n, generator=g)
    lam[0] = 0.0
    if n > 1:
        b[0] = (a[0] + 1) % v
        lam[1] = 1.0
    return logits, a, b, lam


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("shape", [(1, 10), (5, 10), (4, 257), (6, 1000), (64, 1000)])
def test_softmax_xent_mix_matches_soft_target_cross_entropy(gpu, native_ext, mix_ext, shape, eps):
    n, v = shape
    logits, a, b, lam = loss_case(n, v)
    x = logits.clone().requires_grad_(True)
    want = F.cross_entropy(x, soft_target(a, b, lam, v), label_smoothing=eps)
    (dwant,) = torch.autograd.grad(want, x)
    lg, ag, bg, lamg = logits.to(gpu), a.to(gpu), b.to(gpu), lam.to(gpu)
    loss, dl = mix_ext.softmax_xent_mix(lg, ag, bg, lamg, eps)
    assert loss.dtype == torch.float32 and dl.dtype == torch.float32 and dl.shape == lg.shape
    print(f"loss err {abs(loss.item() - want.item()):.3e} dlogits err {(dl.cpu() - dwant).abs().max().item():.3e}")
    assert abs(loss.item() - want.item()) < 1e-4
    assert torch.allclose(dl.cpu(), dwant, atol=1e-6)
    # deterministic: two calls are bitwise equal
    loss2, dl2 = mix_ext.softmax_xent_mix(lg, ag, bg, lamg, eps)
    assert torch.equal(loss, loss2) and torch.equal(dl, dl2)
    # lam == 1 everywhere: the hard-label kernel bit for bit, whatever labels_b holds
    l1, d1 = mix_ext.softmax_xent_mix(lg, ag, bg, torch.ones_like(lamg), eps)
    l0, d0 = native_ext.softmax_xent(lg, ag, eps)
    assert torch.equal(l1, l0) and torch.equal(d1, d0)


def test_mix_cross_entropy_backward_on_device(gpu, native_ext, mix_ext):
    from pytorch_distributed_tutorials_amd import ops
    from pytorch_distributed_tutorials_amd.ops import reference as ref
    logits, a, b, lam = loss_case(6, 1000, seed=5)
    x = logits.to(gpu).requires_grad_(True)
    loss = ops.mix_cross_entropy(x, a.to(gpu), b.to(gpu), lam.to(gpu), 0.1)
    (loss * 2.5).backward()
    want_loss, want = ref.softmax_xent_mix(logits, a, b, lam, 0.1)
    assert abs(loss.item() - want_loss.item()) < 1e-4
    assert torch.allclose(x.grad.cpu(), 2.5 * want, atol=2.5e-6)
    # the module front end takes the MixedTarget
    crit = ops.CrossEntropyLoss(label_smoothing=0.1)
    assert torch.equal(crit(x.detach(), MixedTarget(a.to(gpu), b.to(gpu), lam.to(gpu))), loss.detach())


def test_native_training_step_on_a_mixed_batch(gpu, native_ext, mix_ext):
    from pytorch_distributed_tutorials_amd import ops
    from pytorch_distributed_tutorials_amd.models import build_model
    from pytorch_distributed_tutorials_amd.optim import SGD
    from pytorch_distributed_tutorials_amd.parallel import DistributedDataParallel
    torch.manual_seed(0)
    model = build_model("resnet18", num_classes=10, impl="native").to(gpu)
    model.set_impl("native")
    ddp = DistributedDataParallel(model)
    opt = SGD(ddp.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-5)
    loader = DeviceLoader(_dataset(8, 32, 32, False), batch_size=8, augment=True, device=gpu, seed=1,
                          mix=MixConfig(0.2, 1.0))
    assert loader.fused
    crit = ops.CrossEntropyLoss(label_smoothing=0.1)
    (x, target), = list(loader)
    assert isinstance(target, MixedTarget) and bool((target.lam != 1).any())
    opt.zero_grad()
    loss = crit(ddp(x), target)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    lv = float(loss.item())
    gn = float(ddp.space.grad_flat.norm().item())
    assert lv == lv and 0 < lv < 100
    assert gn == gn and gn != float("inf") and gn > 0
