"""The augmentation policy on the CPU: the reference semantics (data/autoaug.py) against PIL and
``F.grid_sample``, degenerate inputs, the draws, the torch-path loader and the trainer flags."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_tutorials_amd.data import (AugConfig, AugDraw, DeviceLoader, MixConfig, MixedTarget,
                                                    RandomResizedCrop, CenterCropResize, TensorImageDataset,
                                                    apply_policy, apply_policy_levels, draw_policy)
from pytorch_distributed_tutorials_amd.data import autoaug as A
from pytorch_distributed_tutorials_amd.data.datasets import CIFAR_MEAN, CIFAR_STD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 48, 64


def make_draw(ops, bins, signs, h, w, erase=None) -> AugDraw:
    """A hand-made draw: operation ``ops[b]`` at bin ``bins[b]`` with sign draw ``signs[b]``."""
    op = torch.tensor(ops, dtype=torch.int64)
    param, matrix = A.policy_params(op, torch.tensor(bins), torch.tensor(signs), h, w)
    e = torch.zeros((len(ops), 4), dtype=torch.int32) if erase is None else torch.tensor(erase, dtype=torch.int32)
    return AugDraw(op.to(torch.int32), param, matrix, e)


def images():
    """uint8 [3, 3, 48, 64]: uniform noise, a smooth ramp, a narrow range (levels 100..139)."""
    g = torch.Generator().manual_seed(7)
    noise = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    ramp = torch.stack([(xx * 255) // (W - 1), (yy * 255) // (H - 1), ((xx + yy) * 255) // (H + W - 2)]).to(torch.uint8)
    narrow = torch.randint(100, 140, (3, H, W), generator=g, dtype=torch.uint8)
    return torch.stack([noise, ramp, narrow])


IMAGES = images()
NAMES = ("noise", "ramp", "narrow")


def run_op(img_u8, op, k, sign=0):
    """uint8 [3, h, w]: operation ``op`` at bin ``k`` on one image."""
    x = img_u8[None].float() / 255.0
    return apply_policy_levels(x, make_draw([op], [k], [sign], *img_u8.shape[1:]))[0]


def to_pil(img_u8):
    from PIL import Image
    return Image.fromarray(np.ascontiguousarray(img_u8.permute(1, 2, 0).numpy()), "RGB")


def from_pil(im):
    return torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1)


def max_diff(a, b):
    return int((a.int() - b.int()).abs().max())


# ---------------------------------------------------------------------------- reference against PIL
@pytest.mark.parametrize("which", range(3), ids=NAMES)
def test_exact_photometric_ops_match_pil(which):
    pytest.importorskip("PIL")
    from PIL import ImageOps
    img, pil = IMAGES[which], to_pil(IMAGES[which])
    for k, bits in ((0, 8), (5, 7), (15, 5), (30, 2)):
        assert float(A.magnitude_table()[A.POSTERIZE, k]) == bits
        assert torch.equal(run_op(img, A.POSTERIZE, k), from_pil(ImageOps.posterize(pil, bits))), f"posterize {bits}"
    for k, thr in ((0, 255.0), (7, 195.5), (15, 127.5), (30, 0.0)):
        assert float(A.magnitude_table()[A.SOLARIZE, k]) == thr
        assert torch.equal(run_op(img, A.SOLARIZE, k), from_pil(ImageOps.solarize(pil, thr))), f"solarize {thr}"
    assert torch.equal(run_op(img, A.EQUALIZE, 0), from_pil(ImageOps.equalize(pil)))


@pytest.mark.parametrize("which", range(3), ids=NAMES)
def test_blend_ops_and_autocontrast_match_pil_within_one_level(which):
    pytest.importorskip("PIL")
    from PIL import ImageEnhance, ImageOps
    img, pil = IMAGES[which], to_pil(IMAGES[which])
    enhancers = {A.BRIGHTNESS: ImageEnhance.Brightness, A.COLOR: ImageEnhance.Color,
                 A.CONTRAST: ImageEnhance.Contrast, A.SHARPNESS: ImageEnhance.Sharpness}
    for op, enh in enhancers.items():
        for k in (1, 15, 30):
            for sign in (0, 1):
                m = float(A.magnitude_table()[op, k]) * (-1.0 if sign else 1.0)
                d = max_diff(run_op(img, op, k, sign), from_pil(enh(pil).enhance(1.0 + m)))
                print(f"{A.OP_NAMES[op]} bin {k} sign {sign}: max diff {d}")
                assert d <= 1, (A.OP_NAMES[op], k, sign, d)
    d = max_diff(run_op(img, A.AUTOCONTRAST, 0), from_pil(ImageOps.autocontrast(pil)))
    print(f"AutoContrast: max diff {d}")
    assert d <= 1


def _pil_affine(pil, coeffs):
    from PIL import Image
    return from_pil(pil.transform(pil.size, Image.AFFINE, coeffs, resample=Image.NEAREST, fillcolor=0))


# (op, bin, sign): ShearX/Y at bins 3, 15, 30 with both signs; Translate by 3, -16 and 32; Rotate by
# 4.5, -67.5 and 90 degrees
EXACT_WARPS = [(op, k, s) for op in (A.SHEAR_X, A.SHEAR_Y) for k in (3, 15, 30) for s in (0, 1)] + \
              [(op, k, s) for op in (A.TRANSLATE_X, A.TRANSLATE_Y) for k, s in ((3, 0), (15, 1), (30, 0))] + \
              [(A.ROTATE, 1, 0), (A.ROTATE, 15, 1), (A.ROTATE, 20, 0)]


def _signed(op, k, s):
    return float(A.magnitude_table()[op, k]) * (-1.0 if s else 1.0)


@pytest.mark.parametrize("which", range(3), ids=NAMES)
def test_geometric_ops_match_pil(which):
    pytest.importorskip("PIL")
    from PIL import Image
    img, pil = IMAGES[which], to_pil(IMAGES[which])
    assert [int(_signed(A.TRANSLATE_X, k, s)) for k, s in ((3, 0), (15, 1), (30, 0))] == [3, -16, 32]
    assert [_signed(A.ROTATE, k, s) for k, s in ((1, 0), (15, 1), (20, 0), (30, 0))] == [4.5, -67.5, 90.0, 135.0]
    for op, k, s in EXACT_WARPS:
        m = _signed(op, k, s)
        ours = run_op(img, op, k, s)
        if op == A.ROTATE:
            ref = from_pil(pil.rotate(m, resample=Image.NEAREST))
        else:  # the matrix in corner coordinates: a shear about the top-left corner, a shift by whole pixels
            t = float(int(m))
            coeffs = {A.SHEAR_X: (1, m, 0, 0, 1, 0), A.SHEAR_Y: (1, 0, 0, m, 1, 0),
                      A.TRANSLATE_X: (1, 0, -t, 0, 1, 0), A.TRANSLATE_Y: (1, 0, 0, 0, 1, -t)}[op]
            ref = _pil_affine(pil, coeffs)
        assert torch.equal(ours, ref), (A.OP_NAMES[op], k, s, float((ours != ref).float().mean()))
    ours, ref = run_op(img, A.ROTATE, 30, 0), from_pil(pil.rotate(135.0, resample=Image.NEAREST))
    share = float((ours != ref).any(dim=0).float().mean())
    print(f"Rotate 135: {100 * share:.2f} % of pixels differ")
    assert share <= 0.02


def test_warp_matches_grid_sample_nearest():
    q = IMAGES.float()  # levels
    for op, k, s in EXACT_WARPS:
        d = make_draw([op] * 3, [k] * 3, [s] * 3, H, W)
        ours = apply_policy_levels(q / 255.0, d).float()
        m = d.matrix[0].double()
        # the same source coordinates in grid_sample's normalised form (align_corners=False)
        xc = torch.arange(W, dtype=torch.float64) + 0.5 - W / 2.0
        yc = (torch.arange(H, dtype=torch.float64) + 0.5 - H / 2.0)[:, None]
        sx = m[0] * xc + m[1] * yc + m[2] + (W / 2.0 - 0.5)
        sy = m[3] * xc + m[4] * yc + m[5] + (H / 2.0 - 0.5)
        grid = torch.stack([(2 * sx + 1) / W - 1, (2 * sy + 1) / H - 1], dim=-1)[None].expand(3, H, W, 2)
        ref = F.grid_sample(q.double(), grid, mode="nearest", padding_mode="zeros", align_corners=False).float()
        assert torch.equal(ours, ref), (A.OP_NAMES[op], k, s)


# ------------------------------------------------------------------------------- degenerate inputs
def test_degenerate_inputs():
    const = torch.full((3, 20, 36), 77, dtype=torch.uint8)
    assert torch.equal(run_op(const, A.AUTOCONTRAST, 0), const)
    assert torch.equal(run_op(const, A.EQUALIZE, 0), const)
    g = torch.Generator().manual_seed(3)
    thin = torch.randint(0, 256, (3, 2, 36), generator=g, dtype=torch.uint8)
    for s in (0, 1):
        assert torch.equal(run_op(thin, A.SHARPNESS, 30, s), thin)
    short = torch.randint(0, 256, (3, 20, 36), generator=g, dtype=torch.uint8)
    assert int(run_op(short, A.TRANSLATE_Y, 30, 0).max()) == 0  # 32 rows down a 20-row image
    x = torch.rand((1, 3, 20, 36), generator=g)  # off the 8-bit lattice
    q = A.quantize(x).to(torch.uint8)
    assert torch.equal(q.float(), torch.round(x * 255.0))
    for op in range(A.SHEAR_X, A.SHARPNESS + 1):
        for s in (0, 1):
            assert torch.equal(apply_policy_levels(x, make_draw([op], [0], [s], 20, 36)), q), A.OP_NAMES[op]
    assert torch.equal(apply_policy_levels(x, make_draw([0], [9], [1], 20, 36)), q)
    # unknown operation ids are Identity
    d = make_draw([0], [0], [0], 20, 36)
    assert torch.equal(apply_policy_levels(x, d._replace(op=torch.tensor([99], dtype=torch.int32))), q)


def test_apply_policy_normalises_and_erases():
    g = torch.Generator().manual_seed(5)
    x = torch.rand((2, 3, 20, 36), generator=g)
    d = make_draw([A.SOLARIZE, A.COLOR], [15, 30], [0, 1], 20, 36, erase=[[3, 5, 7, 9], [0, 0, 0, 0]])
    lv = apply_policy_levels(x, d).float()
    out = apply_policy(x, d, CIFAR_MEAN, CIFAR_STD)
    ref = (lv / 255.0 - torch.tensor(CIFAR_MEAN).view(1, 3, 1, 1)) / torch.tensor(CIFAR_STD).view(1, 3, 1, 1)
    inside = torch.zeros((2, 1, 20, 36), dtype=torch.bool)
    inside[0, :, 3:10, 5:14] = True
    assert torch.equal(out, torch.where(inside, torch.zeros_like(ref), ref))
    assert torch.equal(apply_policy(x, d._replace(erase=torch.zeros_like(d.erase)), None, None, normalize=False),
                       lv / 255.0)
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        apply_policy_levels(x[:, :1], d)
    with pytest.raises(ValueError, match="not one of this batch"):
        apply_policy_levels(x[:1], d)


# ------------------------------------------------------------------------------------------- draws
def test_draws_are_deterministic_and_ordered():
    cfg = AugConfig("trivial-wide", 0.25)
    a = draw_policy(64, 32, 48, cfg, "cpu", torch.Generator().manual_seed(11))
    b = draw_policy(64, 32, 48, cfg, "cpu", torch.Generator().manual_seed(11))
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    assert a.op.dtype == torch.int32 and a.param.dtype == torch.float32 and a.matrix.dtype == torch.float32
    assert a.erase.dtype == torch.int32 and a.param.shape == (64, 2) and a.matrix.shape == (64, 6)
    # the documented order: op, bin, sign, then the five erase draws
    g = torch.Generator().manual_seed(11)
    op = torch.randint(0, 14, (64,), generator=g)
    k = torch.randint(0, 31, (64,), generator=g)
    s = torch.randint(0, 2, (64,), generator=g)
    assert torch.equal(a.op, op.to(torch.int32))
    param, matrix = A.policy_params(op, k, s, 32, 48)
    assert torch.equal(a.param, param) and torch.equal(a.matrix, matrix)
    assert torch.equal(a.erase, A.draw_erase(64, 32, 48, 0.25, cfg.erase_scale, cfg.erase_ratio, "cpu", g))
    apply = torch.rand((64,), generator=torch.Generator().manual_seed(11))  # erasing alone: its first draw
    e = draw_policy(64, 32, 48, AugConfig("none", 0.25), "cpu", torch.Generator().manual_seed(11))
    assert torch.equal(e.erase[:, 2] > 0, apply < 0.25) and int(e.op.abs().max()) == 0
    # p = 0 makes no erase draws: the generator stands where the three policy draws left it
    g0, g1 = torch.Generator().manual_seed(4), torch.Generator().manual_seed(4)
    d = draw_policy(16, 32, 48, AugConfig("trivial-wide", 0.0), "cpu", g0)
    for hi in (14, 31, 2):
        torch.randint(0, hi, (16,), generator=g1)
    assert torch.equal(g0.get_state(), g1.get_state()) and int(d.erase.abs().max()) == 0
    g0 = torch.Generator().manual_seed(4)
    state = g0.get_state()
    draw_policy(16, 32, 48, AugConfig("none", 0.0), "cpu", g0)
    assert torch.equal(g0.get_state(), state)


def test_draw_statistics_and_boxes():
    n, p = 20000, 0.1
    d = draw_policy(n, 32, 48, AugConfig("trivial-wide", p), "cpu", torch.Generator().manual_seed(2))
    sd = math.sqrt(n * (1 / 14) * (13 / 14))
    counts = torch.bincount(d.op.long(), minlength=14)
    assert counts.numel() == 14 and float((counts - n / 14).abs().max()) <= 5 * sd, counts
    y0, x0, h, w = d.erase.long().unbind(1)
    erased = h > 0
    assert abs(int(erased.sum()) - n * p) <= 5 * math.sqrt(n * p * (1 - p))
    assert bool(((h < 32) & (w < 48) & (y0 >= 0) & (x0 >= 0) & (y0 + h <= 32) & (x0 + w <= 48)).all())
    assert bool((erased == (w > 0)).all()) and int(d.erase[~erased].abs().max()) == 0
    area = (h * w)[erased].float() / (32 * 48)
    assert 0.01 < float(area.min()) and float(area.max()) < 0.36  # scale (0.02, 0.33), sides rounded


def test_magnitude_table_is_built_once_per_device():
    t = A.magnitude_table("cpu")
    assert t is A.magnitude_table(torch.device("cpu")) and t.shape == (14, 31) and t.dtype == torch.float64
    assert torch.equal(t[A.ROTATE], torch.linspace(0.0, 135.0, 31, dtype=torch.float64))
    assert torch.equal(t[A.COLOR], torch.linspace(0.0, 0.99, 31, dtype=torch.float64))
    assert torch.equal(t[A.TRANSLATE_Y], torch.linspace(0.0, 32.0, 31, dtype=torch.float64))
    assert t[A.POSTERIZE].tolist() == [8.0 - round(k / 5) for k in range(31)]
    assert t[A.SOLARIZE].tolist() == [255.0 - 8.5 * k for k in range(31)]
    assert float(t[[A.IDENTITY, A.AUTOCONTRAST, A.EQUALIZE]].abs().max()) == 0.0


def test_config_is_validated():
    assert not AugConfig().enabled and AugConfig("trivial-wide").enabled and AugConfig("none", 0.1).enabled
    for bad, msg in ((AugConfig("rand"), "policy must be one of"), (AugConfig("none", 1.5), "probability"),
                     (AugConfig("none", -0.1), "probability"), (AugConfig("none", 0.1, (0.5, 0.2)), "scale"),
                     (AugConfig("none", 0.1, (0.0, 0.2)), "scale"), (AugConfig("none", 0.1, (0.02, 0.33), (2.0, 1.0)), "ratio"),
                     (AugConfig("none", 0.1, (0.02, 0.33), (0.0, 1.0)), "ratio")):
        with pytest.raises(ValueError, match=msg):
            bad.validate()


# ------------------------------------------------------------------------------------------ loader
def _dataset(n=40, side=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return TensorImageDataset(torch.randint(0, 256, (n, 3, side, side), generator=g, dtype=torch.uint8),
                              torch.randint(0, 10, (n,), generator=g))


@pytest.mark.parametrize("transform", [None, RandomResizedCrop(16)], ids=["pad-crop", "rrc"])
def test_loader_without_a_policy_is_unchanged(transform):
    kw = dict(batch_size=16, augment=True, seed=3, shuffle=True, transform=transform, mix=MixConfig(0.2, 1.0))
    for aug in (None, AugConfig()):
        for (xa, ya), (xb, yb) in zip(DeviceLoader(_dataset(), **kw), DeviceLoader(_dataset(), aug=aug, **kw)):
            assert torch.equal(xa, xb) and all(torch.equal(s, t) for s, t in zip(ya, yb))


@pytest.mark.parametrize("transform", [None, RandomResizedCrop(16)], ids=["pad-crop", "rrc"])
def test_loader_erasing_alone_keeps_the_crops_and_flips(transform):
    kw = dict(batch_size=16, augment=True, seed=5, transform=transform)
    cfg = AugConfig("none", 1.0)
    side = 32 if transform is None else 16
    gen = torch.Generator().manual_seed((5 * 1000003 + 0) ^ 0x417567)
    tol = (0.5 / 255 + 2e-6) / torch.tensor(CIFAR_STD).view(1, 3, 1, 1)
    seen = 0
    for (xa, ya), (xb, yb) in zip(DeviceLoader(_dataset(), **kw), DeviceLoader(_dataset(), aug=cfg, **kw)):
        d = draw_policy(xa.shape[0], side, side, cfg, "cpu", gen)
        inside = torch.zeros_like(xa[:, :1], dtype=torch.bool)
        for b, (y0, x0, h, w) in enumerate(d.erase.tolist()):
            inside[b, :, y0:y0 + h, x0:x0 + w] = True
        seen += int(inside.sum())
        assert torch.equal(ya, yb)
        assert float(xb[inside.expand_as(xb)].abs().max()) == 0.0
        assert bool((((xa - xb).abs() <= tol) | inside).all())
    assert seen > 0


def test_loader_policy_keeps_labels_and_mix_draws():
    kw = dict(batch_size=16, augment=True, seed=9, shuffle=True, mix=MixConfig(0.2, 1.0))
    cfg = AugConfig("trivial-wide", 0.1)
    changed = False
    for (xa, ya), (xb, yb) in zip(DeviceLoader(_dataset(), **kw), DeviceLoader(_dataset(), aug=cfg, **kw)):
        assert isinstance(yb, MixedTarget) and all(torch.equal(s, t) for s, t in zip(ya, yb))
        assert xb.shape == xa.shape and xb.dtype == torch.float32 and bool(torch.isfinite(xb).all())
        changed |= not torch.equal(xa, xb)
    assert changed
    # the same seed and epoch give the same batches; another epoch gives other draws
    la, lb = DeviceLoader(_dataset(), aug=cfg, **kw), DeviceLoader(_dataset(), aug=cfg, **kw)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(la, lb))
    lb.set_epoch(1)
    la.shuffle = lb.shuffle = False
    assert not all(torch.equal(a[0], b[0]) for a, b in zip(la, lb))


def test_loader_refusals():
    cfg = AugConfig("trivial-wide")
    ds = _dataset()
    with pytest.raises(ValueError, match="needs augment=True or a RandomResizedCrop"):
        DeviceLoader(ds, 8, aug=cfg)
    with pytest.raises(ValueError, match="cannot follow CenterCropResize"):
        DeviceLoader(ds, 8, transform=CenterCropResize(16), aug=cfg)
    normed = TensorImageDataset(torch.randn(8, 3, 32, 32), torch.zeros(8, dtype=torch.int64), normalized=True)
    with pytest.raises(ValueError, match="un-normalised"):
        DeviceLoader(normed, 8, augment=True, aug=cfg)
    mono = TensorImageDataset(torch.zeros((8, 1, 32, 32), dtype=torch.uint8), torch.zeros(8, dtype=torch.int64))
    with pytest.raises(ValueError, match="needs RGB images, got C = 1"):
        DeviceLoader(mono, 8, augment=True, aug=cfg)
    with pytest.raises(ValueError, match="policy must be one of"):
        DeviceLoader(ds, 8, augment=True, aug=AugConfig("auto"))
    with pytest.raises(ValueError, match="probability"):
        DeviceLoader(ds, 8, augment=True, aug=AugConfig("none", 2.0))


# ----------------------------------------------------------------------------------------- trainer
def _write_arrays(root, n_train=48, n_val=16, side=24, seed=0):
    rng = np.random.default_rng(seed)
    for split, n in (("train", n_train), ("val", n_val)):
        np.save(os.path.join(root, f"{split}_images.npy"), rng.integers(0, 256, (n, 3, side, side), dtype=np.uint8))
        np.save(os.path.join(root, f"{split}_labels.npy"), rng.integers(0, 10, (n,), dtype=np.int16))


def test_trainer_two_steps_with_the_policy_and_erasing(tmp_path):
    _write_arrays(str(tmp_path))
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["OMP_NUM_THREADS"] = "2"
    cmd = [sys.executable, "-m", "pytorch_distributed_tutorials_amd.train", "--impl", "torch", "--arch", "resnet18",
           "--batch-size", "16", "--num-classes", "10", "--backend", "gloo", "--model_dir", str(tmp_path / "models"),
           "--eval-every", "1", "--data", "array", "--data-root", str(tmp_path), "--num_epochs", "1", "--steps", "2",
           "--log-every", "1", "--auto-augment", "trivial-wide", "--random-erase-prob", "0.5"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(s.split()[3]) for s in r.stdout.splitlines() if s.strip().startswith("step ")]
    assert len(losses) == 2 and all(l == l and 0 < l < 100 for l in losses)
    assert "Epoch: 0, Accuracy:" in r.stdout  # the evaluation, which never augments, ran


def test_trainer_flags():
    from pytorch_distributed_tutorials_amd.train import build_parser, main
    a = build_parser().parse_args([])
    assert (a.auto_augment, a.random_erase_prob) == ("none", 0.0)
    assert tuple(a.random_erase_scale) == (0.02, 0.33) and tuple(a.random_erase_ratio) == (0.3, 3.3)
    for flags in (["--auto-augment", "trivial-wide"], ["--random-erase-prob", "0.1"]):
        with pytest.raises(SystemExit) as e:
            main(["--data", "synthetic-imagenet"] + flags)
        assert "cannot be combined with --data synthetic-imagenet" in str(e.value)
    for bad in (["--random-erase-prob", "1.5"], ["--random-erase-prob", "-0.1"],
                ["--random-erase-prob", "0.1", "--random-erase-scale", "0.5", "0.2"],
                ["--random-erase-prob", "0.1", "--random-erase-scale", "0", "0.2"],
                ["--random-erase-prob", "0.1", "--random-erase-ratio", "3", "0.3"]):
        with pytest.raises(SystemExit) as e:
            main(["--data", "array"] + bad)
        assert "must be" in str(e.value)
    with pytest.raises(SystemExit):  # argparse refuses an unknown policy
        build_parser().parse_args(["--auto-augment", "rand"])
