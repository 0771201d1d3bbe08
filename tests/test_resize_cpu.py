"""The ImageNet input pipeline on the CPU: the resampling semantics (data/resize.py) against ATen's
antialiased interpolate, the box draws, the torch-path loader, the array dataset, the trainer flags
and the build of the `_C_img` extension module."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_tutorials_amd.data import (CenterCropResize, DeviceLoader, MixConfig, MixedTarget,
                                                    RandomResizedCrop, TensorImageDataset, build_dataset, center_box,
                                                    draw_rrc, resample_weights, resized_crop)
from pytorch_distributed_tutorials_amd.data.datasets import IMAGENET_MEAN, IMAGENET_STD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (box h, box w) -> output side
SIZES = [((37, 29), 16), ((9, 50), 16), ((5, 7), 16), ((64, 3), 8), ((1, 1), 8), ((16, 16), 16)]


def aten_resize(crop, out_hw):
    return F.interpolate(crop, size=out_hw, mode="bilinear", antialias=True, align_corners=False)


@pytest.mark.parametrize("dtype,atol", [(torch.float64, 1e-12), (torch.float32, 1e-6)])
@pytest.mark.parametrize("hw,out", SIZES)
def test_resized_crop_matches_aten_antialiased_interpolate(hw, out, dtype, atol):
    h, w = hw
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.rand(3, 3, h + 6, w + 5, generator=g, dtype=dtype)
    box = torch.tensor([[0, 0, h, w], [6, 5, h, w], [3, 2, h, w]], dtype=torch.int32)  # corners and the middle
    flip = torch.tensor([False, True, False])
    got = resized_crop(x, box, out, flip)
    assert got.shape == (3, 3, out, out) and got.dtype == dtype
    for b in range(3):
        y0, x0 = box[b, 0].item(), box[b, 1].item()
        crop = x[b:b + 1, :, y0:y0 + h, x0:x0 + w]
        want = aten_resize(crop, (out, out))[0]
        if flip[b]:
            want = want.flip(2)
        err = (got[b] - want).abs().max().item()
        print(f"{hw}->{out} {dtype} sample {b}: max err {err:.3e}")
        assert err <= atol
        if hw == (out, out) and not flip[b]:
            assert torch.equal(got[b], crop[0])  # scale 1: the window itself, bit for bit
    # a rectangular output takes each axis' own weights
    got = resized_crop(x, box, (out, out + 4))
    assert (got[1] - aten_resize(x[1:2, :, 6:6 + h, 5:5 + w], (out, out + 4))[0]).abs().max().item() <= atol


@pytest.mark.parametrize("dtype,atol", [(torch.float64, 1e-12), (torch.float32, 1e-6)])
@pytest.mark.parametrize("n_in,n_out", [(37, 16), (50, 16), (5, 16), (3, 8), (1, 8), (16, 16), (64, 8)])
def test_resample_weights_are_atens(n_in, n_out, dtype, atol):
    w = resample_weights(n_in, n_out, dtype)
    assert w.shape == (n_out, n_in) and w.dtype == dtype
    assert torch.allclose(w.sum(1), torch.ones(n_out, dtype=dtype), atol=1e-6) and (w >= 0).all()
    # ATen applied to the identity rows gives its weight matrix
    eye = torch.eye(n_in, dtype=dtype).view(1, n_in, 1, n_in)
    want = aten_resize(eye, (1, n_out))[0, :, 0, :].t()
    assert (w - want).abs().max().item() <= atol
    if n_in == n_out:
        assert torch.equal(w, torch.eye(n_in, dtype=dtype))


def test_draw_rrc_boxes_and_determinism():
    H, W, n = 64, 48, 4096
    scale, ratio = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)
    box = draw_rrc(n, H, W, scale, ratio, "cpu", torch.Generator().manual_seed(5))
    assert box.dtype == torch.int32 and box.shape == (n, 4)
    y0, x0, h, w = box.long().unbind(1)
    assert (h >= 1).all() and (w >= 1).all() and (y0 >= 0).all() and (x0 >= 0).all()
    assert (y0 + h <= H).all() and (x0 + w <= W).all()
    again = draw_rrc(n, H, W, scale, ratio, "cpu", torch.Generator().manual_seed(5))
    assert torch.equal(box, again)
    assert not torch.equal(box, draw_rrc(n, H, W, scale, ratio, "cpu", torch.Generator().manual_seed(6)))
    # a box that is not the centred fallback (here: the whole image, 48/64 lies inside the ratio range)
    # comes from w = round(sqrt(area r)), h = round(sqrt(area / r)): both within 0.5 of their real
    # values, whose product is the area and whose quotient the ratio
    drawn = ~((h == H) & (w == W))
    assert drawn.sum() > 0.9 * n
    hf, wf = h[drawn].double(), w[drawn].double()
    assert ((hf + 0.5) * (wf + 0.5) >= scale[0] * H * W).all() and ((hf - 0.5) * (wf - 0.5) <= scale[1] * H * W).all()
    assert ((wf + 0.5) / (hf - 0.5) >= ratio[0]).all() and ((wf - 0.5) / (hf + 0.5) <= ratio[1]).all()
    # the draws cover the ranges and the offsets reach both ends
    frac = (hf * wf) / (H * W)
    assert frac.min() < 0.12 and frac.max() > 0.9 and (wf / hf).min() < 0.8 and (wf / hf).max() > 1.25
    assert ((y0 == 0) & (h < H)).any() and ((y0 + h == H) & (h < H)).any()
    assert ((x0 == 0) & (w < W)).any() and ((x0 + w == W) & (w < W)).any()


def test_draw_rrc_full_box_and_fallback():
    g = torch.Generator().manual_seed(0)
    full = draw_rrc(64, 32, 32, (1.0, 1.0), (1.0, 1.0), "cpu", g)
    assert torch.equal(full, torch.tensor([[0, 0, 32, 32]], dtype=torch.int32).expand(64, 4))
    # every attempt is wider than the image: torchvision's centred fallback, w = W, h = round(W / r0)
    fb = draw_rrc(64, 32, 32, (1.0, 1.0), (3.0, 4.0), "cpu", g)
    hh = round(32 / 3.0)
    assert torch.equal(fb, torch.tensor([[(32 - hh) // 2, 0, hh, 32]], dtype=torch.int32).expand(64, 4))
    # ... and h = H, w = round(H r1) for an image wider than the range
    tall = draw_rrc(8, 32, 32, (1.0, 1.0), (0.25, 1.0 / 3.0), "cpu", g)
    ww = round(32 / 3.0)
    assert torch.equal(tall, torch.tensor([[0, (32 - ww) // 2, 32, ww]], dtype=torch.int32).expand(8, 4))


def test_center_box_values():
    assert center_box(2, 40, 52, 0.875).tolist() == [[2, 3, 35, 46]] * 2
    assert center_box(1, 256, 256, 0.875).tolist() == [[16, 16, 224, 224]]
    assert center_box(1, 24, 24, 1.0).tolist() == [[0, 0, 24, 24]]
    assert center_box(1, 5, 7, 0.01).tolist() == [[2, 3, 1, 1]]
    assert center_box(3, 8, 8, 0.5).dtype == torch.int32


def test_transform_configs_are_validated():
    for bad in (RandomResizedCrop(16, scale=(0.5, 0.2)), RandomResizedCrop(16, scale=(0.0, 1.0)),
                RandomResizedCrop(16, scale=(0.5, 1.5)), RandomResizedCrop(16, ratio=(2.0, 1.0)),
                RandomResizedCrop(16, ratio=(0.0, 1.0)), RandomResizedCrop(0), CenterCropResize(16, crop_pct=0.0),
                CenterCropResize(16, crop_pct=1.2), CenterCropResize((16, -4))):
        with pytest.raises(ValueError):
            bad.validate()
    assert RandomResizedCrop((16, 24)).validate().out_hw == (16, 24) and CenterCropResize(8).validate().out_hw == (8, 8)
    ds = _dataset(4)
    with pytest.raises(ValueError):
        DeviceLoader(ds, batch_size=2, transform=RandomResizedCrop(16, scale=(0.5, 0.2)))
    with pytest.raises(ValueError):
        DeviceLoader(ds, batch_size=2, augment=True, transform=CenterCropResize(16))
    with pytest.raises(ValueError):
        DeviceLoader(ds, batch_size=2, transform="random-resized-crop")


def _dataset(n=40, h=24, w=28, normalized=False, seed=21):
    g = torch.Generator().manual_seed(seed)
    if normalized:
        imgs = torch.randn(n, 3, h, w, generator=g)
    else:
        imgs = torch.randint(0, 256, (n, 3, h, w), generator=g, dtype=torch.uint8)
    return TensorImageDataset(imgs, torch.randint(0, 10, (n,), generator=g), IMAGENET_MEAN, IMAGENET_STD, normalized)


@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("mix", [None, MixConfig(0.2, 1.0)])
def test_loader_without_a_transform_is_unchanged(augment, mix):
    ds = _dataset()
    kw = dict(batch_size=16, shuffle=True, augment=augment, device="cpu", seed=3, mix=mix)
    for (xa, ya), (xb, yb) in zip(DeviceLoader(ds, **kw), DeviceLoader(ds, transform=None, **kw)):
        assert torch.equal(xa, xb)
        assert all(torch.equal(p, q) for p, q in zip(ya, yb)) if mix else torch.equal(ya, yb)


@pytest.mark.parametrize("normalized", [False, True])
def test_rrc_loader_batches_are_resized_crops_of_its_draws(normalized):
    ds = _dataset(normalized=normalized)
    tf = RandomResizedCrop((16, 20))
    loader = DeviceLoader(ds, batch_size=16, shuffle=True, device="cpu", seed=3, transform=tf)
    batches = list(loader)
    assert [x.shape[0] for x, _ in batches] == [16, 16, 8]  # a partial last batch
    order = torch.randperm(40, generator=torch.Generator().manual_seed(3))
    gen = torch.Generator().manual_seed(3 * 1000003)
    mean = torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD).view(1, 3, 1, 1)
    for k, (x, y) in enumerate(batches):
        bi = order[16 * k:16 * k + 16]
        assert x.shape == (bi.numel(), 3, 16, 20) and x.dtype == torch.float32 and x.is_contiguous()
        assert torch.equal(y, ds.labels[bi])
        # the documented draw order: the boxes of the batch, then its flips, from the crop generator
        box = draw_rrc(bi.numel(), 24, 28, tf.scale, tf.ratio, "cpu", gen)
        flip = torch.rand(bi.numel(), generator=gen) < 0.5
        src = ds.images[bi].float()
        want = resized_crop(src, box, (16, 20), flip) if normalized else \
            (resized_crop(src / 255.0, box, (16, 20), flip) - mean) / std
        assert torch.equal(x, want)
    # another epoch draws other boxes; the same epoch repeats them
    again = list(loader)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(batches, again))
    loader.set_epoch(1)
    assert not torch.equal(next(iter(loader))[0], batches[0][0])


def test_rrc_loader_with_mix_keeps_the_rrc_draws():
    ds = _dataset()
    kw = dict(batch_size=16, shuffle=True, device="cpu", seed=3, transform=RandomResizedCrop(16))
    plain = list(DeviceLoader(ds, **kw))
    on = list(DeviceLoader(ds, mix=MixConfig(0.2, 1.0, prob=0.6), **kw))
    assert len(plain) == len(on) == 3 and on[2][0].shape[0] == 8
    mixed = 0
    for (xp, yp), (xm, tm) in zip(plain, on):
        assert isinstance(tm, MixedTarget) and xm.shape == xp.shape == (yp.numel(), 3, 16, 16)
        assert torch.equal(tm.labels_a, yp) and torch.equal(tm.labels_b, yp.roll(1))
        same = tm.lam == 1
        assert torch.equal(xm[same], xp[same])  # an unmixed sample: the plain run's box and flip
        mixed += int((~same).sum())
    assert 10 < mixed < 40


def test_center_crop_loader():
    ds = _dataset(n=20)
    loader = DeviceLoader(ds, batch_size=16, device="cpu", transform=CenterCropResize(16, crop_pct=0.75))
    batches = list(loader)
    assert [x.shape for x, _ in batches] == [(16, 3, 16, 16), (4, 3, 16, 16)]
    x = torch.cat([b[0] for b in batches])
    mean = torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD).view(1, 3, 1, 1)
    crop = ds.images[:, :, 3:21, 3:24].float() / 255.0   # the centred 18 x 21 box of 24 x 28
    want = (aten_resize(crop, (16, 16)) - mean) / std
    assert (x - want).abs().max().item() <= 1e-5
    # crop_pct 1 at the stored size is the untransformed evaluation loader
    ident = list(DeviceLoader(ds, batch_size=16, device="cpu", transform=CenterCropResize((24, 28), crop_pct=1.0)))
    none = list(DeviceLoader(ds, batch_size=16, device="cpu"))
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(ident, none))


def _write_arrays(root, n_train=48, n_val=16, side=24, seed=0):
    rng = np.random.default_rng(seed)
    for split, n in (("train", n_train), ("val", n_val)):
        np.save(os.path.join(root, f"{split}_images.npy"), rng.integers(0, 256, (n, 3, side, side), dtype=np.uint8))
        np.save(os.path.join(root, f"{split}_labels.npy"), rng.integers(0, 10, (n,), dtype=np.int16))


def test_array_dataset_round_trip_and_refusals(tmp_path):
    root = str(tmp_path)
    _write_arrays(root)
    for train, n in ((True, 48), (False, 16)):
        ds = build_dataset("array", train, root)
        split = "train" if train else "val"
        assert len(ds) == n and ds.images.dtype == torch.uint8 and ds.images.shape == (n, 3, 24, 24)
        assert ds.labels.dtype == torch.int64 and not ds.normalized
        assert ds.mean == IMAGENET_MEAN and ds.std == IMAGENET_STD
        assert np.array_equal(ds.images.numpy(), np.load(os.path.join(root, f"{split}_images.npy")))
        assert np.array_equal(ds.labels.numpy(), np.load(os.path.join(root, f"{split}_labels.npy")))
    x, y = next(iter(DeviceLoader(build_dataset("array", True, root), batch_size=8, transform=RandomResizedCrop(16))))
    assert x.shape == (8, 3, 16, 16) and y.shape == (8,)

    def refuses(images=None, labels=None, exc=ValueError, match="array dataset"):
        d = tmp_path / f"bad{len(os.listdir(root))}"
        d.mkdir()
        _write_arrays(str(d))
        if images is not None:
            np.save(str(d / "train_images.npy"), images)
        if labels is not None:
            np.save(str(d / "train_labels.npy"), labels)
        with pytest.raises(exc, match=match):
            build_dataset("array", True, str(d))

    refuses(images=np.zeros((48, 3, 24, 24), dtype=np.float32), match="uint8")
    refuses(images=np.zeros((48, 24, 24, 3), dtype=np.uint8), match=r"\[N, 3, H, W\]")
    refuses(images=np.zeros((48, 3, 24), dtype=np.uint8), match=r"\[N, 3, H, W\]")
    refuses(labels=np.zeros((48,), dtype=np.float32), match="integer")
    refuses(labels=np.zeros((47,), dtype=np.int64), match="labels for the 48")
    refuses(labels=np.full((48,), -1, dtype=np.int64), match="negative")
    with pytest.raises(FileNotFoundError, match="train_images.npy"):
        build_dataset("array", True, str(tmp_path / "nowhere"))


def _trainer(args, tmp_path):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["OMP_NUM_THREADS"] = "2"
    cmd = [sys.executable, "-m", "pytorch_distributed_tutorials_amd.train", "--impl", "torch", "--arch", "resnet18",
           "--batch-size", "16", "--num-classes", "10", "--backend", "gloo", "--model_dir", str(tmp_path / "models"),
           "--eval-every", "1"] + args
    return subprocess.run(cmd, cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)


def test_trainer_two_steps_on_an_array_dataset_with_the_imagenet_transforms(tmp_path):
    _write_arrays(str(tmp_path))
    r = _trainer(["--data", "array", "--data-root", str(tmp_path), "--train-transform", "random-resized-crop",
                  "--train-size", "16", "--eval-transform", "center-crop", "--num_epochs", "1", "--steps", "2",
                  "--log-every", "1"], tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(s.split()[3]) for s in r.stdout.splitlines() if s.strip().startswith("step ")]
    assert len(losses) == 2 and all(l == l and 0 < l < 100 for l in losses)
    assert "Epoch: 0, Accuracy:" in r.stdout  # the centre-crop evaluation ran
    # labels past --num-classes are refused
    r = _trainer(["--data", "array", "--data-root", str(tmp_path), "--num-classes", "5", "--steps", "1"], tmp_path)
    assert r.returncode != 0 and "--num-classes is 5" in r.stderr


def test_trainer_transform_flags():
    from pytorch_distributed_tutorials_amd.train import build_parser, input_transforms, main
    a = build_parser().parse_args([])
    assert (a.train_transform, a.train_size, a.eval_transform, a.eval_crop_pct) == ("pad-crop", None, "none", 0.875)
    assert tuple(a.rrc_scale) == (0.08, 1.0) and tuple(a.rrc_ratio) == (3.0 / 4.0, 4.0 / 3.0)
    assert input_transforms(a, (32, 32)) == (None, None)  # the defaults leave both loaders as they were
    a = build_parser().parse_args(["--train-transform", "random-resized-crop", "--train-size", "224", "--rrc-scale",
                                   "0.35", "1", "--eval-transform", "center-crop"])
    assert input_transforms(a, (256, 256)) == (RandomResizedCrop((224, 224), (0.35, 1.0)),
                                               CenterCropResize((224, 224), 0.875))
    a = build_parser().parse_args(["--train-transform", "random-resized-crop"])
    assert input_transforms(a, (128, 160))[0].out_hw == (128, 160)  # no --train-size: the stored size
    for bad in (["--train-transform", "random-resized-crop", "--rrc-scale", "0.5", "0.2"],
                ["--train-transform", "random-resized-crop", "--rrc-scale", "0", "1"],
                ["--train-transform", "random-resized-crop", "--rrc-ratio", "2", "1"],
                ["--train-transform", "random-resized-crop", "--train-size", "0"],
                ["--eval-transform", "center-crop", "--eval-crop-pct", "1.5"],
                ["--eval-transform", "center-crop", "--eval-crop-pct", "0"]):
        with pytest.raises(SystemExit) as e:
            main(bad)
        assert "must be" in str(e.value)


def test_img_extension_builds_next_to_the_main_one():
    import build_native
    so = build_native.ensure_built()
    assert so == build_native.out_path()
    assert os.path.exists(build_native.img_out_path())
    assert os.path.dirname(build_native.img_out_path()) == os.path.dirname(so)
    # its objects stay out of build/native, whose every object other tools link into _C
    assert not [f for f in os.listdir(build_native.BUILD) if f.startswith("img_")]
    assert sorted(os.listdir(build_native.BUILD_IMG)) == ["img_bind_img.cpp.o", "img_resample.hip.o"]
    from pytorch_distributed_tutorials_amd.ops import _ext
    ci = _ext.native_img()
    assert _ext.native_img_available()
    assert ci.__name__.endswith("._C_img")
    assert {"resized_crop", "set_sync_check", "sync_check_enabled"} <= set(dir(ci))
    # _C and _C_mix gain no name: _C against its pinned surface, _C_mix against what it had
    with open(os.path.join(ROOT, "tests", "golden", "c_api.json")) as f:
        golden = json.load(f)
    assert not hasattr(_ext.native(), "resized_crop") and not hasattr(_ext.native_mix(), "resized_crop")
    assert {n for n in dir(_ext.native_mix()) if not n.startswith("_")} == {"augment_mix", "softmax_xent_mix",
                                                                            "set_sync_check", "sync_check_enabled"}
    assert "resized_crop" not in json.dumps(golden)
    on = ci.sync_check_enabled()
    ci.set_sync_check(not on)
    assert ci.sync_check_enabled() == (not on)
    ci.set_sync_check(on)


def test_img_extension_honours_disable_native():
    code = ("from pytorch_distributed_tutorials_amd.ops import _ext\n"
            "assert not _ext.native_img_available() and not _ext.native_available()\n"
            "try:\n    _ext.native_img()\nexcept RuntimeError as e:\n"
            "    assert 'PDT_DISABLE_NATIVE' in str(e) and '_C_img' in str(e)\n"
            "else:\n    raise SystemExit(1)\n")
    env = dict(os.environ, PDT_DISABLE_NATIVE="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
