"""Binary cross entropy with logits on the CPU: the PyTorch reference against torch's own loss in
fp64, the binding's argument checks, the trainer flags and one short ``--loss bce`` run."""
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_tutorials_amd.ops import reference as ref
from test_trainer_cpu import ROOT, _env


@pytest.mark.parametrize("sum_classes", [False, True])
@pytest.mark.parametrize("thr", [-1.0, 0.2])
@pytest.mark.parametrize("s", [0.0, 0.1])
@pytest.mark.parametrize("mixed", [False, True])
def test_reference_matches_torch_in_fp64(mixed, s, thr, sum_classes):
    g = torch.Generator().manual_seed(3)
    n, c = 6, 10
    z = torch.randn(n, c, generator=g) * 4
    a = torch.randint(0, c, (n,), generator=g)
    b = torch.randint(0, c, (n,), generator=g)
    b[:2] = a[:2]  # a == b rows
    lam = torch.tensor([0.75, 0.1, 1.0, 0.5, 0.25, 0.0])
    # the dense target, built independently: one_hot, smooth, blend, gt
    ta, tb = (F.one_hot(x, c).double() * (1.0 - s) + s / c for x in (a, b))
    t = lam.double()[:, None] * ta + (1.0 - lam.double())[:, None] * tb if mixed else ta
    if thr >= 0:
        assert (t - thr).abs().min() > 1e-3
        t = (t > thr).double()
    z64 = z.double().requires_grad_()
    want = F.binary_cross_entropy_with_logits(z64, t, reduction="sum") / (n if sum_classes else n * c)
    want.backward()
    loss, dz = ref.bce_with_logits(z, a, b if mixed else None, lam if mixed else None, s, thr, sum_classes)
    assert loss.dtype == dz.dtype == torch.float32
    torch.testing.assert_close(loss.double(), want.detach(), rtol=1e-6, atol=0)
    torch.testing.assert_close(dz.double(), z64.grad, rtol=0, atol=2e-7 * (1 / n if sum_classes else 1 / (n * c)))


def test_binding_checks_run_before_any_launch(native_ext):
    from pytorch_distributed_tutorials_amd.ops import _ext
    if not _ext.native_loss_available():
        pytest.skip("the _C_loss extension is not built")
    op = _ext.native_loss().bce_with_logits
    z, a, lam = torch.zeros(4, 10), torch.zeros(4, dtype=torch.long), torch.ones(4)
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):  # everything else is in order
        op(z, a, a, lam, 0.1, 0.2, True)
    for bad, msg in (((z.double(), a), "logits must be fp32"),
                     ((z[:, ::2], a), "logits must be contiguous"),
                     ((z[0], a), r"must be \[N, C\]"),
                     ((z, a.int()), "int64"),
                     ((z, a[:3]), "int64"),
                     ((z, a, a), "go together"),
                     ((z, a, a, lam.double()), "lam must be contiguous fp32"),
                     ((z, a, None, None, 1.5), r"label_smoothing must be in \[0, 1\]"),
                     ((z, a, None, None, 0.0, 1.0), "target_threshold must be below 1")):
        with pytest.raises(RuntimeError, match=msg):
            op(*bad)


def test_trainer_loss_flag_validation():
    from pytorch_distributed_tutorials_amd.train import build_parser, main
    a = build_parser().parse_args([])
    assert (a.loss, a.bce_target_thresh, a.bce_sum_classes) == ("ce", None, False)
    for bad, msg in ((["--loss", "bce", "--bce-target-thresh", "1.5"], "--bce-target-thresh must be in [0, 1)"),
                     (["--loss", "bce", "--bce-target-thresh", "-0.1"], "--bce-target-thresh must be in [0, 1)"),
                     (["--bce-sum-classes"], "need --loss bce"),
                     (["--loss", "bce", "--label-smoothing", "2"], "--label-smoothing must be in [0, 1]")):
        with pytest.raises(SystemExit) as e:
            main(bad)
        assert msg in str(e.value)


def test_trainer_runs_with_bce_and_mixing(tmp_path):
    r = subprocess.run(
        [sys.executable, "-m", "pytorch_distributed_tutorials_amd.train", "--arch", "resnet18", "--data",
         "synthetic-cifar", "--synthetic-samples", "64", "--batch-size", "16", "--num_epochs", "1",
         "--max-steps-per-epoch", "3", "--num-classes", "10", "--backend", "gloo", "--model_dir", str(tmp_path),
         "--loss", "bce", "--bce-target-thresh", "0.2", "--label-smoothing", "0.1", "--mixup-alpha", "0.2",
         "--cutmix-alpha", "1.0", "--log-every", "1"], env=_env(), cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    losses = [float(m) for m in re.findall(r"step \d+ loss (\S+)", r.stdout)]
    assert losses and all(0.0 < v < 10.0 for v in losses), r.stdout
