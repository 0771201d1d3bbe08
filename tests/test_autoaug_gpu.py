"""The fused augmentation policy on the GPU: `_C_img.autoaug` (csrc/img/autoaug.hip) against the
reference of data/autoaug.py on a hand-made operation table, erase boxes, sample independence, the
fused loader against the torch path, the binding's refusals and a native training step.

Shapes: 3 x 20 x 36 (H != W, H < 32, a width that is a multiple of 4 but not of 16), 3 x 32 x 32, and
3 x 68 x 64: a block of the statistics pass covers 4096 pixels of a plane, so 68 x 64 = 4352 pixels is
the smallest shape of this kind whose statistics (gray sum, min / max, histogram) are merged from two
workgroups; its apply pass spans five."""
import pytest
import torch

from pytorch_distributed_tutorials_amd.data import (AugConfig, AugDraw, DeviceLoader, MixConfig, MixedTarget,
                                                    RandomResizedCrop, TensorImageDataset, apply_policy,
                                                    apply_policy_levels, draw_policy)
from pytorch_distributed_tutorials_amd.data import autoaug as A
from pytorch_distributed_tutorials_amd.data.datasets import IMAGENET_MEAN, IMAGENET_STD

pytestmark = pytest.mark.gpu

MEAN, STD = list(IMAGENET_MEAN), list(IMAGENET_STD)
SHAPES = [(20, 36), (32, 32), (68, 64)]


@pytest.fixture(scope="module")
def img_ext(native_ext):
    from pytorch_distributed_tutorials_amd.ops import _ext
    return _ext.native_img()


def op_table():
    """(op, bin, sign, image kind): every signed operation at bins 0, 1, 15, 30 with both signs,
    Posterize and Solarize at bins 0, 15, 30, and Identity, AutoContrast and Equalize on a noise, a
    constant and a narrow-range sample."""
    rows = [(op, k, s, "noise") for op in range(A.SHEAR_X, A.SHARPNESS + 1) for k in (0, 1, 15, 30) for s in (0, 1)]
    rows += [(op, k, 0, "noise") for op in (A.POSTERIZE, A.SOLARIZE) for k in (0, 15, 30)]
    rows += [(op, 0, 0, kind) for op in (A.IDENTITY, A.AUTOCONTRAST, A.EQUALIZE)
             for kind in ("noise", "const", "narrow")]
    return rows


def build_case(h, w):
    """CPU operands of the table at one shape: x fp32 [B, 3, h, w] off the 8-bit lattice and its draw."""
    rows = op_table()
    g = torch.Generator().manual_seed(h * 1000 + w)
    x = torch.rand((len(rows), 3, h, w), generator=g)
    for b, (_, _, _, kind) in enumerate(rows):
        if kind == "const":
            x[b] = 0.30173
        elif kind == "narrow":
            x[b] = (100.0 + 39.0 * x[b]) / 255.0
    op = torch.tensor([r[0] for r in rows])
    param, matrix = A.policy_params(op, torch.tensor([r[1] for r in rows]), torch.tensor([r[2] for r in rows]), h, w)
    return x, AugDraw(op.to(torch.int32), param, matrix, torch.zeros((len(rows), 4), dtype=torch.int32))


def run(img_ext, gpu, x, d, normalize, **kw):
    return img_ext.autoaug(x.to(gpu), d.op.to(gpu), d.param.to(gpu), d.matrix.to(gpu), d.erase.to(gpu), normalize,
                           MEAN, STD, **kw)


@pytest.fixture(scope="module")
def cases():
    """shape -> (x, draw, reference levels uint8), computed once on the CPU and left unchanged."""
    out = {}
    for hw in SHAPES:
        x, d = build_case(*hw)
        out[hw] = (x, d, apply_policy_levels(x, d))
    return out


def _names(rows):
    return [f"{A.OP_NAMES[op]}/bin{k}/sign{s}/{kind}" for op, k, s, kind in rows]


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_levels_equal_the_reference(gpu, img_ext, cases, hw):
    x, d, ref = cases[hw]
    out = run(img_ext, gpu, x, d, False).cpu()
    got = torch.round(out * 255.0)
    bad = (got != ref.float()).flatten(1).any(dim=1)
    worst = (got - ref.float()).abs().flatten(1).amax(dim=1)
    print(f"{hw}: samples that differ {[n for n, f in zip(_names(op_table()), bad.tolist()) if f]}, "
          f"max level difference {float(worst.max())}")
    assert not bool(bad.any())
    assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_normalised_output(gpu, img_ext, cases, hw):
    x, d, ref = cases[hw]
    out = run(img_ext, gpu, x, d, True).double().cpu()
    mean = torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    want = (ref.double() / 255.0 - mean) / std
    err = (out - want).abs().amax(dim=(0, 2, 3))
    bound = torch.tensor([2e-6 / s for s in STD], dtype=torch.float64)
    print(f"{hw}: max |kernel - reference| per channel {err.tolist()} bound {bound.tolist()}")
    assert (err <= bound).all()
    # the reference's own fp32 normalisation agrees within the same bound
    err = (out - apply_policy(x, d, MEAN, STD).double()).abs().amax(dim=(0, 2, 3))
    assert (err <= bound).all()


def test_erase_boxes(gpu, img_ext):
    h, w = 20, 36
    ops = [A.IDENTITY, A.ROTATE, A.COLOR, A.EQUALIZE, A.SHARPNESS]
    boxes = [[0, 0, 0, 0], [0, 0, h - 1, w - 1], [1, 1, h - 1, w - 1], [h - 1, w - 1, 1, 1], [3, 5, 7, 9]]
    x = torch.rand((5, 3, h, w), generator=torch.Generator().manual_seed(1))
    op = torch.tensor(ops)
    param, matrix = A.policy_params(op, torch.tensor([0, 15, 30, 0, 15]), torch.tensor([0, 1, 0, 0, 1]), h, w)
    d = AugDraw(op.to(torch.int32), param, matrix, torch.tensor(boxes, dtype=torch.int32))
    inside = torch.zeros((5, 1, h, w), dtype=torch.bool)
    for b, (y0, x0, bh, bw) in enumerate(boxes):
        inside[b, :, y0:y0 + bh, x0:x0 + bw] = True
    for normalize in (False, True):
        free = run(img_ext, gpu, x, d._replace(erase=torch.zeros_like(d.erase)), normalize).cpu()
        out = run(img_ext, gpu, x, d, normalize).cpu()
        m = inside.expand_as(out)
        assert float(out[m].abs().max()) == 0.0 and not bool(torch.signbit(out[m]).any())
        assert torch.equal(out[~m], free[~m])
        if normalize:
            assert float(free[m].abs().min()) > 0.0  # normalised levels are never 0: the boxes did something


def test_a_sample_alone_equals_the_sample_in_its_batch(gpu, img_ext, cases):
    hw = (68, 64)
    x, d, _ = cases[hw]
    rows = op_table()
    batch = run(img_ext, gpu, x, d, True)
    # one sample of every operation, the statistics operations on every image kind
    pick = [b for b, (op, k, s, kind) in enumerate(rows)
            if (k, s) == (15, 1) or (op in (A.POSTERIZE, A.SOLARIZE) and k == 15) or op in (0, 12, 13)]
    assert {rows[b][0] for b in pick} == set(range(14))
    for b in pick:
        one = AugDraw(*(t[b:b + 1].clone() for t in d))
        assert torch.equal(run(img_ext, gpu, x[b:b + 1].clone(), one, True)[0], batch[b]), _names(rows)[b]
    # and a call is reproducible as a whole
    assert torch.equal(run(img_ext, gpu, x, d, True), batch)


def _dataset(n, side=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return TensorImageDataset(torch.randint(0, 256, (n, 3, side, side), generator=g, dtype=torch.uint8),
                              torch.randint(0, 10, (n,), generator=g), IMAGENET_MEAN, IMAGENET_STD)


def _channel_err(got, want):
    return (got.double().cpu() - want.double().cpu()).abs().amax(dim=(0, 2, 3))


BOUND = torch.tensor([2e-6 / s for s in STD], dtype=torch.float64)


def test_fused_pad_crop_loader_matches_torch_loader(gpu, img_ext):
    ds = _dataset(40)
    kw = dict(batch_size=16, shuffle=True, augment=True, device=gpu, seed=3, mix=MixConfig(0.4, 1.0, prob=0.6),
              aug=AugConfig("trivial-wide", 0.5))
    fused_loader = DeviceLoader(ds, fused=True, **kw)
    assert fused_loader.fused
    fused, plain = list(fused_loader), list(DeviceLoader(ds, fused=False, **kw))
    assert [x.shape[0] for x, _ in fused] == [x.shape[0] for x, _ in plain] == [16, 16, 8]
    worst = torch.zeros(3, dtype=torch.float64)
    for (xa, ta), (xb, tb) in zip(fused, plain):
        assert isinstance(ta, MixedTarget) and all(torch.equal(p, q) for p, q in zip(ta, tb))
        assert xa.dtype == torch.float32 and xa.shape == xb.shape
        worst = torch.maximum(worst, _channel_err(xa, xb))
    print(f"pad-crop + policy + erase + mix: max |fused - torch| per channel {worst.tolist()} bound {BOUND.tolist()}")
    assert (worst <= BOUND).all()
    # without the mix the two paths agree level for level
    kw["mix"] = None
    for (xa, ya), (xb, yb) in zip(DeviceLoader(ds, fused=True, **kw), DeviceLoader(ds, fused=False, **kw)):
        assert torch.equal(ya, yb)
        mean, std = torch.tensor(MEAN, device=gpu).view(1, 3, 1, 1), torch.tensor(STD, device=gpu).view(1, 3, 1, 1)
        la, lb = torch.round((xa * std + mean) * 255.0), torch.round((xb * std + mean) * 255.0)
        erased = (xa == 0) & (xb == 0)
        assert torch.equal(la[~erased], lb[~erased]) and torch.equal(xa == 0, xb == 0)


def test_fused_rrc_loader_is_the_policy_on_its_own_resized_crops(gpu, img_ext):
    ds = _dataset(24, side=40)
    cfg = AugConfig("trivial-wide", 0.5)
    loader = DeviceLoader(ds, batch_size=16, device=gpu, seed=4, fused=True, transform=RandomResizedCrop(32), aug=cfg)
    assert loader.fused
    gen = torch.Generator(device=gpu).manual_seed(4 * 1000003)
    agen = torch.Generator(device=gpu).manual_seed((4 * 1000003) ^ 0x417567)
    images = ds.images.to(gpu)
    start = 0
    for x, y in loader:
        b = x.shape[0]
        bi = torch.arange(start, start + b, device=gpu)
        start += b
        box, flip = loader._draw_transform(b, gen)
        crops = img_ext.resized_crop(images, bi, box, flip, 32, 32, False, MEAN, STD)
        d = draw_policy(b, 32, 32, cfg, gpu, agen)
        want_levels = apply_policy_levels(crops, d).float()
        want = apply_policy(crops, d, MEAN, STD)
        assert (_channel_err(x, want) <= BOUND).all()
        mean, std = torch.tensor(MEAN, device=gpu).view(1, 3, 1, 1), torch.tensor(STD, device=gpu).view(1, 3, 1, 1)
        erased = want == 0
        assert torch.equal(x == 0, erased)
        assert torch.equal(torch.round((x * std + mean) * 255.0)[~erased], want_levels[~erased])
        assert torch.equal(y, ds.labels.to(gpu)[bi])
    assert start == 24


def test_binding_refuses_bad_operands(gpu, img_ext, cases):
    x, d, _ = cases[(20, 36)]
    x, d = x[:8].to(gpu), AugDraw(*(t[:8].to(gpu) for t in d))

    def call(x=x, op=d.op, param=d.param, matrix=d.matrix, erase=d.erase, **kw):
        return img_ext.autoaug(x, op, param, matrix, erase, True, MEAN, STD, **kw)

    with pytest.raises(RuntimeError, match="x must be contiguous fp32"):
        call(x=x.half())
    with pytest.raises(RuntimeError, match="x must be contiguous"):
        call(x=x.transpose(2, 3))
    with pytest.raises(RuntimeError, match="x must be a GPU tensor"):
        call(x=x.cpu())
    with pytest.raises(RuntimeError, match=r"fp32 \[B, 3, H, W\]"):
        call(x=x[:, :2].contiguous())
    with pytest.raises(RuntimeError, match="multiple of 4"):
        call(x=x[:, :, :, :34].contiguous())
    with pytest.raises(RuntimeError, match=r"sides must be in \[1, 4096\]"):
        call(x=torch.zeros((8, 3, 4100, 4), device=gpu))
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        call(x=torch.zeros(8 * 3 * 20 * 36 + 1, device=gpu)[1:].view(8, 3, 20, 36))
    with pytest.raises(RuntimeError, match=r"op must be device int32 \[B\]"):
        call(op=d.op.long())
    with pytest.raises(RuntimeError, match=r"op must be device int32 \[B\]"):
        call(op=d.op[:7].contiguous())
    with pytest.raises(RuntimeError, match="op must be a GPU tensor"):
        call(op=d.op.cpu())
    with pytest.raises(RuntimeError, match=r"param must be device fp32 \[B, 2\]"):
        call(param=d.matrix)
    with pytest.raises(RuntimeError, match=r"matrix must be device fp32 \[B, 6\]"):
        call(matrix=d.param)
    with pytest.raises(RuntimeError, match="matrix must be contiguous fp32"):
        call(matrix=d.matrix.double())
    with pytest.raises(RuntimeError, match=r"erase must be device int32 \[B, 4\]"):
        call(erase=d.erase.long())
    with pytest.raises(RuntimeError, match=r"erase must be device int32 \[B, 4\]"):
        call(erase=d.erase[:, :3].contiguous())
    with pytest.raises(RuntimeError, match="passes must be"):
        call(passes=0)
    with pytest.raises(RuntimeError, match="mean/std per channel"):
        img_ext.autoaug(x, d.op, d.param, d.matrix, d.erase, True, MEAN[:2], STD)
    with pytest.raises(RuntimeError, match="mean/std per channel"):
        img_ext.autoaug(x, d.op, d.param, d.matrix, d.erase, True, MEAN, STD[:2])
    n = 65536  # one sample more than the grid's y extent holds; refused before anything is launched
    with pytest.raises(RuntimeError, match="at most 65535 samples"):
        img_ext.autoaug(torch.zeros((n, 3, 1, 4), device=gpu), torch.zeros(n, dtype=torch.int32, device=gpu),
                        torch.zeros((n, 2), device=gpu), torch.zeros((n, 6), device=gpu),
                        torch.zeros((n, 4), dtype=torch.int32, device=gpu), True, MEAN, STD)
    # unknown ids and wild boxes cannot be read without a stall: the kernel takes Identity and clamps ...
    wild_op, tame_op = d.op.clone(), d.op.clone()
    wild_op[0], tame_op[0] = 14, 0
    wild_op[1], tame_op[1] = -1, 0
    wild, tame = d.erase.clone(), d.erase.clone()
    wild[2] = torch.tensor([-3, 30, 100, 100], dtype=torch.int32)
    tame[2] = torch.tensor([0, 30, 20, 6], dtype=torch.int32)
    wild[3] = torch.tensor([25, 0, 4, 4], dtype=torch.int32)       # below the image: nothing
    assert torch.equal(call(op=wild_op, erase=wild), call(op=tame_op, erase=tame))
    # ... and the op's debug mode, which synchronizes anyway, copies both back and checks them
    on = img_ext.sync_check_enabled()
    img_ext.set_sync_check(True)
    try:
        with pytest.raises(RuntimeError, match="op 0 = 14 is not an operation id"):
            call(op=wild_op)
        with pytest.raises(RuntimeError, match="erase box 2 .* reaches outside the 20 x 36 image"):
            call(erase=wild)
        assert torch.equal(call(op=tame_op, erase=tame), call(op=tame_op.clone(), erase=tame.clone()))
    finally:
        img_ext.set_sync_check(on)


def test_draws_make_no_host_synchronisation(gpu):
    """A blocking host-to-device copy or a read-back in ``draw_policy`` would stall the training
    stream once per batch: torch's sync debug mode raises on either."""
    cfg = AugConfig("trivial-wide", 0.5)
    g = torch.Generator(device=gpu).manual_seed(1)
    torch.cuda.set_sync_debug_mode("error")
    try:
        first = draw_policy(32, 32, 48, cfg, gpu, g)   # builds the magnitude table on the device
        again = draw_policy(32, 32, 48, cfg, gpu, g)
        only_erase = draw_policy(32, 32, 48, AugConfig("none", 0.5), gpu, g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(t.device == gpu for d in (first, again, only_erase) for t in d)
    assert not torch.equal(first.op, again.op) and int(only_erase.op.abs().max()) == 0
    # the table built on the device is the host's, to float64 rounding of the two linspace kernels
    assert A.magnitude_table(gpu).device == gpu and A.magnitude_table(gpu) is A.magnitude_table(gpu)
    assert float((A.magnitude_table(gpu).cpu() - A.magnitude_table("cpu")).abs().max()) <= 1e-12


def test_fused_loader_erasing_alone_matches_torch_loader(gpu, img_ext):
    """Erasing alone skips the statistics pass (every operation is Identity)."""
    ds = _dataset(24)
    kw = dict(batch_size=16, augment=True, device=gpu, seed=6, aug=AugConfig("none", 1.0))
    seen = 0
    for (xa, ya), (xb, yb) in zip(DeviceLoader(ds, fused=True, **kw), DeviceLoader(ds, fused=False, **kw)):
        assert torch.equal(ya, yb) and torch.equal(xa == 0, xb == 0)
        assert (_channel_err(xa, xb) <= BOUND).all()
        seen += int((xa == 0).sum())
    assert seen > 0


def test_native_training_step_on_an_augmented_batch(gpu, native_ext, img_ext):
    from pytorch_distributed_tutorials_amd import ops
    from pytorch_distributed_tutorials_amd.models import build_model
    from pytorch_distributed_tutorials_amd.optim import SGD
    from pytorch_distributed_tutorials_amd.parallel import DistributedDataParallel
    torch.manual_seed(0)
    model = build_model("resnet18", num_classes=10, impl="native").to(gpu)
    model.set_impl("native")
    ddp = DistributedDataParallel(model)
    opt = SGD(ddp.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-5)
    loader = DeviceLoader(_dataset(8), batch_size=8, augment=True, device=gpu, seed=1,
                          aug=AugConfig("trivial-wide", 0.5))
    assert loader.fused
    (x, y), = list(loader)
    assert x.shape == (8, 3, 32, 32) and bool(torch.isfinite(x).all())
    opt.zero_grad()
    loss = ops.cross_entropy(ddp(x), y)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    lv = float(loss.item())
    gn = float(ddp.space.grad_flat.norm().item())
    assert lv == lv and 0 < lv < 100
    assert gn == gn and gn != float("inf") and gn > 0
