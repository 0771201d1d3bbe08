"""The resampling input transform on the MI355X: `_C_img.resized_crop` against the fp64 semantics of
data/resize.py, the fused loader against the torch-path loader, the binding's refusals and one
native training step on RandomResizedCrop output.

Tolerances (not tuned to the kernel): the fp32 torch path deviates from fp64 by 1.8e-7 on [0, 1] data,
a convex combination of at most 9 x 9 taps in fp32 is bounded by about 1.2e-6, and the margin up
to 2e-6 covers a different summation order.  Normalisation divides by std_c, so does the bound.  The
randn source reaches |x| ~ 4.5, hence 1e-5 there."""
import pytest
import torch

from pytorch_distributed_tutorials_amd.data import (CenterCropResize, DeviceLoader, MixConfig, MixedTarget,
                                                    RandomResizedCrop, TensorImageDataset, resized_crop)
from pytorch_distributed_tutorials_amd.data.datasets import IMAGENET_MEAN, IMAGENET_STD

pytestmark = pytest.mark.gpu

MEAN, STD = list(IMAGENET_MEAN), list(IMAGENET_STD)
H, W, N, B = 40, 52, 20, 8
OUTS = [(16, 16), (16, 24)]
TOL = {"u8": 2e-6, "fp": 1e-5}


@pytest.fixture(scope="module")
def img_ext(native_ext):
    from pytorch_distributed_tutorials_amd.ops import _ext
    return _ext.native_img()


def hand_boxes(oh, ow):
    """(y0, x0, h, w) over a 40 x 52 source: every tap regime the kernel has."""
    return torch.tensor([[0, 0, H, W],             # the full image: scales 2.5 and 3.25 (2.17 at width 24)
                         [5, 9, oh, ow],           # the output's own size: scale 1
                         [H - 1, W - 1, 1, 1],     # one pixel, the image's last
                         [H - 21, W - 30, 21, 30],  # the bottom-right corner of the allocation's last sample
                         [7, 3, 5, 7],             # up-scale on both axes
                         [0, 0, H, W],             # the full image again, flipped
                         [30, 0, 3, W],            # anisotropic: rows up-scaled, columns down-scaled
                         [0, 44, H, 4]],           # ... and the other way round
                        dtype=torch.int32)


IDX = torch.tensor([3, 17, 0, N - 1, 8, 5, 11, 2])      # position 3 reads the last sample
FLIP = torch.tensor([False, True, False, True, False, True, False, True])


@pytest.fixture(scope="module")
def cases():
    """The two sources and, per output size, the fp64 reference of the hand-made boxes (with the
    flips), computed once on the CPU and left unchanged."""
    g = torch.Generator().manual_seed(7)
    src = {"u8": torch.randint(0, 256, (N, 3, H, W), generator=g, dtype=torch.uint8),
           "fp": torch.randn(N, 3, H, W, generator=g)}
    ref = {}
    for kind, s in src.items():
        x = (s.double() / 255.0 if kind == "u8" else s.double()).index_select(0, IDX)
        for out in OUTS:
            ref[kind, out] = resized_crop(x, hand_boxes(*out), out, FLIP)
    return src, ref


def _normalized(ref):
    m = torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    s = torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    return (ref - m) / s


def _channel_err(got, want):
    return (got.double().cpu() - want).abs().amax(dim=(0, 2, 3))


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("out", OUTS)
@pytest.mark.parametrize("kind", ["u8", "fp"])
def test_resized_crop_matches_the_fp64_semantics(gpu, img_ext, cases, kind, out, normalize):
    src, ref = cases
    images, idx, flip = src[kind].to(gpu), IDX.to(gpu), FLIP.to(gpu)
    box = hand_boxes(*out).to(gpu)
    got = img_ext.resized_crop(images, idx, box, flip, out[0], out[1], normalize, MEAN, STD)
    assert got.shape == (B, 3, *out) and got.dtype == torch.float32 and got.is_contiguous()
    want = _normalized(ref[kind, out]) if normalize else ref[kind, out]
    err = _channel_err(got, want)
    bound = torch.tensor([TOL[kind] / s for s in STD] if normalize else [TOL[kind]] * 3, dtype=torch.float64)
    print(f"{kind} {out} normalize={normalize}: max err per channel {err.tolist()} bound {bound.tolist()}")
    assert (err <= bound).all()
    # no flip operand: the unflipped result, bit for bit (a sample's arithmetic depends on its own operands alone)
    plain = img_ext.resized_crop(images, idx, box, None, out[0], out[1], normalize, MEAN, STD)
    assert torch.equal(plain[~flip], got[~flip]) and torch.equal(plain[flip], got[flip].flip(3))
    assert not torch.equal(plain[flip], got[flip])
    # ... and so is a sample on its own the sample of the batch
    one = img_ext.resized_crop(images, idx[5:6], box[5:6].contiguous(), flip[5:6], out[0], out[1], normalize, MEAN, STD)
    assert torch.equal(one[0], got[5])
    # a host box is checked and uploaded: the same batch
    assert torch.equal(img_ext.resized_crop(images, idx, box.cpu(), flip, out[0], out[1], normalize, MEAN, STD), got)
    # deterministic
    assert torch.equal(img_ext.resized_crop(images, idx, box, flip, out[0], out[1], normalize, MEAN, STD), got)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("out", OUTS)
@pytest.mark.parametrize("kind", ["u8", "fp"])
def test_a_box_of_the_output_size_is_augment_without_augmentation(gpu, native_ext, img_ext, cases, kind, out,
                                                                  normalize):
    images = cases[0][kind].to(gpu)
    idx = IDX.to(gpu)
    oy, ox = 5, 9
    box = torch.tensor([[oy, ox, *out]] * B, dtype=torch.int32, device=gpu)
    got = img_ext.resized_crop(images, idx, box, None, out[0], out[1], normalize, MEAN, STD)
    # _C.augment shifted by (oy, ox) with no padding: its top-left corner is that window
    full = native_ext.augment(images, idx, torch.full((B,), oy, device=gpu), torch.full((B,), ox, device=gpu), None, 0,
                              normalize, MEAN, STD)
    assert torch.equal(got, full[:, :, :out[0], :out[1]])


def test_source_offsets_past_32_bits(gpu, img_ext):
    """A resident set larger than 2^32 bytes: the last sample's offsets need 64 bits."""
    n, side = 22000, 256
    assert n * 3 * side * side > 2 ** 32
    images = torch.empty((n, 3, side, side), dtype=torch.uint8, device=gpu)
    g = torch.Generator().manual_seed(3)
    last = torch.randint(0, 256, (2, 3, side, side), generator=g, dtype=torch.uint8)
    images[n - 1].copy_(last[0])
    images[n // 2 + 1].copy_(last[1])  # past 2^31
    idx = torch.tensor([n - 1, n // 2 + 1], device=gpu)
    # the last 40 x 52 pixels of the allocation (at most 6 x 8 taps), and a window at scale 1
    box = torch.tensor([[side - 40, side - 52, 40, 52], [100, 200, 16, 16]], dtype=torch.int32)
    got = img_ext.resized_crop(images, idx, box.to(gpu), None, 16, 16, False, MEAN, STD)
    want = resized_crop(last.double() / 255.0, box, 16)
    err = (got.double().cpu() - want).abs().max().item()
    print(f"offsets past 2^32: max err {err:.3e}")
    assert err <= 2e-6
    assert torch.equal(got[1].cpu(), last[1, :, 100:116, 200:216].float() * (1.0 / 255.0))


def _dataset(n, normalized, seed=21):
    g = torch.Generator().manual_seed(seed)
    if normalized:
        imgs = torch.randn(n, 3, H, W, generator=g)
    else:
        imgs = torch.randint(0, 256, (n, 3, H, W), generator=g, dtype=torch.uint8)
    return TensorImageDataset(imgs, torch.randint(0, 10, (n,), generator=g), IMAGENET_MEAN, IMAGENET_STD, normalized)


@pytest.mark.parametrize("mix", [None, MixConfig(0.4, 1.0, prob=0.6)])
@pytest.mark.parametrize("normalized", [False, True])
@pytest.mark.parametrize("transform", [RandomResizedCrop(16), CenterCropResize(16)])
def test_fused_loader_matches_torch_loader(gpu, img_ext, transform, normalized, mix):
    ds = _dataset(40, normalized)
    kw = dict(batch_size=16, shuffle=True, device=gpu, seed=3, mix=mix, transform=transform)
    fused_loader = DeviceLoader(ds, fused=True, **kw)
    assert fused_loader.fused
    fused, plain = list(fused_loader), list(DeviceLoader(ds, fused=False, **kw))
    assert [x.shape[0] for x, _ in fused] == [x.shape[0] for x, _ in plain] == [16, 16, 8]  # a partial batch of 8
    # a uint8 source is normalised by the loader, so the bound is divided by std_c; randn is not
    bound = torch.tensor([1e-5] * 3 if normalized else [2e-6 / s for s in STD], dtype=torch.float64)
    worst = torch.zeros(3, dtype=torch.float64)
    for (xa, ta), (xb, tb) in zip(fused, plain):
        if mix is None:
            assert torch.equal(ta, tb)
        else:
            assert isinstance(ta, MixedTarget) and all(torch.equal(p, q) for p, q in zip(ta, tb))
        assert xa.dtype == torch.float32 and xa.shape == xb.shape == (ta[0].numel() if mix else ta.numel(), 3, 16, 16)
        worst = torch.maximum(worst, _channel_err(xa, xb.double().cpu()))
    print(f"{type(transform).__name__} normalized={normalized} mix={mix is not None}: "
          f"max |fused - torch| per channel {worst.tolist()} bound {bound.tolist()}")
    assert (worst <= bound).all()


def test_binding_refuses_bad_operands(gpu, img_ext, cases):
    images, idx, flip = cases[0]["u8"].to(gpu), IDX.to(gpu), FLIP.to(gpu)
    box = hand_boxes(16, 16)

    def call(box=box.to(gpu), out_w=16, idx=idx, flip=flip):
        return img_ext.resized_crop(images, idx, box, flip, 16, out_w, True, MEAN, STD)

    with pytest.raises(RuntimeError, match="int32"):
        call(box=box.to(gpu).long())
    with pytest.raises(RuntimeError, match=r"\[B, 4\]"):
        call(box=box.to(gpu)[:, :3].contiguous())
    with pytest.raises(RuntimeError, match=r"\[B, 4\]"):
        call(box=box.to(gpu)[:7].contiguous())
    with pytest.raises(RuntimeError, match="multiple of 4"):
        call(out_w=18)
    with pytest.raises(RuntimeError, match="idx"):
        call(idx=idx.cpu())
    with pytest.raises(RuntimeError, match="flip"):
        call(flip=flip.cpu())
    # a host box is read row by row before anything is launched
    for row in ([0, 0, H + 1, W], [0, 1, H, W], [-1, 0, 4, 4], [3, 3, 0, 4], [3, 3, 4, -2], [H, 0, 1, 1]):
        bad = box.clone()
        bad[5] = torch.tensor(row, dtype=torch.int32)
        with pytest.raises(RuntimeError, match="box 5 .* is empty or reaches outside"):
            call(box=bad)
    # a device box cannot be read without a stall: the kernel clamps it into the image ...
    wild = box.clone()
    wild[0] = torch.tensor([-3, -5, 100, 100], dtype=torch.int32)   # -> the full image
    wild[4] = torch.tensor([H - 2, W - 3, 9, 9], dtype=torch.int32)  # -> the 2 x 3 corner
    wild[6] = torch.tensor([30, 0, 0, W], dtype=torch.int32)        # -> one row
    tame = box.clone()
    tame[4] = torch.tensor([H - 2, W - 3, 2, 3], dtype=torch.int32)
    tame[6] = torch.tensor([30, 0, 1, W], dtype=torch.int32)
    assert torch.equal(call(box=wild.to(gpu)), call(box=tame.to(gpu)))
    # ... and the op's debug mode, which synchronizes anyway, copies it back and checks it
    on = img_ext.sync_check_enabled()
    img_ext.set_sync_check(True)
    try:
        with pytest.raises(RuntimeError, match="box 0 .* is empty or reaches outside"):
            call(box=wild.to(gpu))
        assert torch.equal(call(box=tame.to(gpu)), call(box=tame))
    finally:
        img_ext.set_sync_check(on)


def test_native_training_step_on_random_resized_crops(gpu, native_ext, img_ext):
    from pytorch_distributed_tutorials_amd import ops
    from pytorch_distributed_tutorials_amd.models import build_model
    from pytorch_distributed_tutorials_amd.optim import SGD
    from pytorch_distributed_tutorials_amd.parallel import DistributedDataParallel
    torch.manual_seed(0)
    model = build_model("resnet18", num_classes=10, impl="native").to(gpu)
    model.set_impl("native")
    ddp = DistributedDataParallel(model)
    opt = SGD(ddp.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-5)
    loader = DeviceLoader(_dataset(8, False), batch_size=8, device=gpu, seed=1, transform=RandomResizedCrop(32))
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
