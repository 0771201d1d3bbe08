"""The large-batch recipe on the CPU: the LARS oracle (``ops.reference.lars_momentum_``) against a
hand-written float64 loop, ``optim.LARS`` on a flat parameter space, the warm-up / polynomial
schedule, label smoothing in the reference cross entropy, and the trainer's flags with resume."""
import copy
import math
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_tutorials_amd.ops import reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f64_lars(ps, gs, bufs, lr, mom, damp, wd, nest, first, eta, eps, exclude_1d):
    """The issue's formula, element by element in float64 (lists of Python floats)."""
    for p, g, b in zip(ps, gs, bufs):
        excluded = exclude_1d and p["ndim"] <= 1
        wd_eff = 0.0 if excluded else wd
        pv, gv = p["v"], g
        pn = math.sqrt(sum(x * x for x in pv))
        gn = math.sqrt(sum(x * x for x in gv))
        trust = 1.0
        if not (excluded or pn == 0 or gn == 0):
            trust = float(torch.tensor(eta * pn / (gn + wd * pn + eps), dtype=torch.float64).float())
        for i in range(len(pv)):
            d = trust * (gv[i] + wd_eff * pv[i])
            if mom != 0:
                b[i] = d if first else mom * b[i] + (1 - damp) * d
                d = d + mom * b[i] if nest else b[i]
            pv[i] -= lr * d


@pytest.mark.parametrize("exclude_1d", [True, False], ids=["exclude1d", "adapt1d"])
@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
def test_lars_reference_matches_float64_loop(nesterov, exclude_1d):
    g = torch.Generator().manual_seed(3)
    shapes = [(5,), (3, 4), (2, 3)]
    params = [torch.randn(s, generator=g) for s in shapes]
    params[2].zero_()                       # an all-zero tensor: trust 1
    lr, mom, damp, wd, eta, eps = 0.1, 0.9, 0.0, 1e-2, 1.0, 1e-8
    bufs = [torch.zeros_like(p) for p in params]
    hp = [{"ndim": p.ndim, "v": p.double().flatten().tolist()} for p in params]
    hb = [[0.0] * p.numel() for p in params]
    for step in range(3):
        grads = [torch.randn(s, generator=g) for s in shapes]
        grads[1].zero_()                    # a zero gradient: trust 1 (weight decay still applies)
        _f64_lars(hp, [x.double().flatten().tolist() for x in grads], hb, lr, mom, damp, wd, nesterov,
                  step == 0, eta, eps, exclude_1d)
        ref.lars_momentum_(params, grads, bufs, lr, mom, damp, wd, nesterov, step == 0, eta, eps, exclude_1d)
        for p, h, b, hbv in zip(params, hp, bufs, hb):
            want = torch.tensor(h["v"], dtype=torch.float64).reshape(p.shape)
            assert torch.allclose(p.double(), want, atol=1e-6), (step, (p.double() - want).abs().max())
            wantb = torch.tensor(hbv, dtype=torch.float64).reshape(p.shape)
            assert torch.allclose(b.double(), wantb, atol=1e-6)
    # the 1-D tensor moved as plain SGD would move it when excluded, and differently when adapted
    assert not torch.equal(params[0], torch.zeros(5))


def test_lars_trust_ratio_degenerate_cases():
    p = torch.tensor([3.0, 4.0])
    g = torch.tensor([0.6, 0.8])
    assert ref.lars_trust_ratio(p, g, 0.0, 1e-3, 0.0, False) == pytest.approx(5e-3, rel=1e-6)
    assert ref.lars_trust_ratio(p, g, 0.0, 1e-3, 0.0, True) == 1.0
    assert ref.lars_trust_ratio(torch.zeros(2), g, 0.0, 1e-3, 1e-8, False) == 1.0
    assert ref.lars_trust_ratio(p, torch.zeros(2), 0.1, 1e-3, 1e-8, False) == 1.0


@pytest.fixture
def gloo_world1(tmp_path):
    import torch.distributed as dist
    store = dist.FileStore(str(tmp_path / "store"), 1)
    dist.init_process_group("gloo", store=store, rank=0, world_size=1)
    try:
        yield
    finally:
        dist.destroy_process_group()


def test_lars_optimizer_on_cpu_ddp(gloo_world1):
    from pytorch_distributed_tutorials_amd.models import build_model
    from pytorch_distributed_tutorials_amd.optim import LARS
    from pytorch_distributed_tutorials_amd.parallel import DistributedDataParallel
    torch.manual_seed(0)
    m1 = build_model("resnet18", num_classes=10).set_impl("native")
    m2 = copy.deepcopy(m1)
    ddp = DistributedDataParallel(m1)
    hyper = dict(lr=0.1, momentum=0.9, weight_decay=1e-4, trust_coefficient=0.02)
    opt = LARS(ddp.parameters(), **hyper)
    assert opt._flat_space_of(opt.param_groups[0]) is ddp.space
    g0 = opt.param_groups[0]
    assert (g0["trust_coefficient"], g0["eps"], g0["exclude_1d"]) == (0.02, 1e-8, True)
    assert opt._hyper(g0)[5:] == (0.02, 1e-8, True)
    p2 = list(m2.parameters())
    b2 = [torch.zeros_like(p) for p in p2]
    x = torch.randn(2, 3, 32, 32)
    y = torch.tensor([1, 2])
    for step in range(2):
        opt.zero_grad()
        F.cross_entropy(ddp(x), y).backward()
        opt.step()
        for p in p2:
            p.grad = None
        F.cross_entropy(m2(x), y).backward()
        with torch.no_grad():
            ref.lars_momentum_(p2, [p.grad for p in p2], b2, 0.1, 0.9, 0.0, 1e-4, False, step == 0,
                               0.02, 1e-8, True)
    for a, b in zip(m1.parameters(), p2):
        assert torch.allclose(a, b, atol=1e-5)
    # torch-format state: one momentum_buffer per parameter, round trip restores it
    sd = opt.state_dict()
    assert len(sd["state"]) == len(p2) and all("momentum_buffer" in v for v in sd["state"].values())
    assert sd["param_groups"][0]["trust_coefficient"] == 0.02
    opt2 = LARS(ddp.parameters(), lr=0.5)
    opt2.load_state_dict(copy.deepcopy(sd))
    assert opt2.param_groups[0]["trust_coefficient"] == 0.02 and opt2.param_groups[0]["lr"] == 0.1
    for p in ddp.parameters():
        assert torch.equal(opt2.state[p]["momentum_buffer"], opt.state[p]["momentum_buffer"])


def test_lars_momentum_buffers_are_views_of_the_flat_buffer():
    """The flat-space bookkeeping ``LARS`` inherits: exercised through ``_flat_momentum`` on the CPU
    (the fused step that fills the buffer needs a GPU)."""
    from pytorch_distributed_tutorials_amd.models import build_model
    from pytorch_distributed_tutorials_amd.optim import LARS
    from pytorch_distributed_tutorials_amd.parallel import DistributedDataParallel
    torch.manual_seed(0)
    ddp = DistributedDataParallel(build_model("resnet18", num_classes=10).set_impl("native"))
    opt = LARS(ddp.parameters(), lr=0.1, momentum=0.9)
    sp = ddp.space
    buf, first = opt._flat_momentum(sp, 0.9)
    assert first and buf.shape == sp.param_flat.shape
    base = buf.untyped_storage().data_ptr()
    for p, o in zip(sp.params, sp.offsets):
        mb = opt.state[p]["momentum_buffer"]
        assert mb.untyped_storage().data_ptr() == base and mb.storage_offset() == o
        assert mb.shape == p.shape and mb.stride() == p.stride()


def test_warmup_poly_schedule():
    from pytorch_distributed_tutorials_amd.optim import WarmupPolyLR
    s = WarmupPolyLR(None, base_lr=2.0, warmup_steps=4, total_steps=14, power=2.0, end_lr=0.2)
    assert s.lr_at(0) == pytest.approx(2.0 / 4)            # step 0
    assert s.lr_at(3) == pytest.approx(2.0)                # last warm-up step
    assert s.lr_at(4) == pytest.approx(2.0)                # first decay step: t = 0
    assert s.lr_at(9) == pytest.approx(0.2 + 1.8 * 0.25)   # half way: (1 - 0.5)^2
    assert s.lr_at(13) == pytest.approx(0.2 + 1.8 * 0.01)  # last step: t = 0.9
    assert s.lr_at(14) == pytest.approx(0.2) and s.lr_at(1000) == pytest.approx(0.2)  # past the end
    assert [s.lr_at(i) for i in range(4)] == sorted(s.lr_at(i) for i in range(4))
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=9.0)
    s2 = WarmupPolyLR(opt, 1.0, 2, 10)
    assert s2.set(0) == 0.5 and opt.param_groups[0]["lr"] == 0.5
    assert "before the forward" in WarmupPolyLR.__doc__.lower()
    with pytest.raises(ValueError):
        WarmupPolyLR(None, 1.0, 5, 3)


@pytest.mark.parametrize("shape", [(5, 10), (33, 1000), (7, 1001)])
def test_reference_label_smoothing_matches_torch(shape):
    g = torch.Generator().manual_seed(11)
    n, v = shape
    logits = (3 * torch.randn(n, v, generator=g)).requires_grad_(True)
    labels = torch.randint(0, v, (n,), generator=g)
    want = F.cross_entropy(logits, labels, label_smoothing=0.1)
    (dwant,) = torch.autograd.grad(want, logits)
    loss, dl = ref.softmax_xent(logits.detach(), labels, label_smoothing=0.1)
    assert abs(loss.item() - want.item()) < 1e-5
    assert torch.allclose(dl, dwant, atol=1e-7)
    # eps = 0 is the unsmoothed function, bit for bit
    l0, d0 = ref.softmax_xent(logits.detach(), labels)
    l1, d1 = ref.softmax_xent(logits.detach(), labels, label_smoothing=0.0)
    assert torch.equal(l0, l1) and torch.equal(d0, d1)


def test_ops_cross_entropy_label_smoothing_cpu():
    from pytorch_distributed_tutorials_amd import ops
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(6, 10, generator=g, requires_grad=True)
    labels = torch.randint(0, 10, (6,), generator=g)
    (ops.cross_entropy(logits, labels, label_smoothing=0.1) * 3.0).backward()
    l2 = logits.detach().clone().requires_grad_(True)
    (F.cross_entropy(l2, labels, label_smoothing=0.1) * 3.0).backward()
    assert torch.allclose(logits.grad, l2.grad, atol=1e-6)
    crit = ops.CrossEntropyLoss(label_smoothing=0.1)
    assert abs(crit(logits, labels).item() - F.cross_entropy(l2, labels, label_smoothing=0.1).item()) < 1e-5


def _trainer(args, tmp_path):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["OMP_NUM_THREADS"] = "2"
    cmd = [sys.executable, "-m", "pytorch_distributed_tutorials_amd.train", "--impl", "torch", "--arch", "resnet18",
           "--data", "synthetic-cifar", "--synthetic-samples", "48", "--batch-size", "16", "--num-classes", "10",
           "--backend", "gloo", "--model_dir", str(tmp_path), "--eval-every", "1"] + args
    return subprocess.run(cmd, cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)


def test_trainer_lars_schedule_and_resume(tmp_path):
    from pytorch_distributed_tutorials_amd.optim import WarmupPolyLR
    recipe = ["--optimizer", "lars", "--label-smoothing", "0.1", "--lr-schedule", "warmup-poly",
              "--warmup-epochs", "1", "--learning_rate", "0.4", "--lr-end", "0.01",
              "--max-steps-per-epoch", "3"]
    r = _trainer(recipe + ["--num_epochs", "2"], tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lrs = {int(s): float(v) for s, v in re.findall(r"step: (\d+), lr: ([0-9.e+-]+)", r.stdout)}
    sched = WarmupPolyLR(None, 0.4, 3, 6, power=2.0, end_lr=0.01)
    assert lrs == {0: pytest.approx(sched.lr_at(0)), 3: pytest.approx(sched.lr_at(3))}
    # the checkpoint of epoch 1 (written before that epoch trained) resumes at global step 3 of a
    # run that is now 4 epochs long: the schedule continues, it does not restart its warm-up
    r = _trainer(recipe + ["--num_epochs", "4", "--resume"], tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lrs = {int(s): float(v) for s, v in re.findall(r"step: (\d+), lr: ([0-9.e+-]+)", r.stdout)}
    sched = WarmupPolyLR(None, 0.4, 3, 12, power=2.0, end_lr=0.01)
    assert min(lrs) == 3 and lrs[3] == pytest.approx(sched.lr_at(3))
    assert "Epoch: 1, Training" in r.stdout and "Epoch: 0, Training" not in r.stdout


def test_trainer_graph_with_schedule_exits(tmp_path):
    r = _trainer(["--graph", "--lr-schedule", "warmup-poly", "--num_epochs", "1"], tmp_path)
    assert r.returncode != 0
    assert "--graph cannot follow --lr-schedule warmup-poly" in r.stderr


def test_trainer_defaults_are_the_plain_sgd_recipe():
    from pytorch_distributed_tutorials_amd.train import build_parser
    a = build_parser().parse_args([])
    assert (a.optimizer, a.momentum, a.weight_decay, a.label_smoothing, a.lr_schedule) == \
        ("sgd", 0.9, 1e-5, 0.0, "constant")
