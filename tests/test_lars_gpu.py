"""Fused LARS (``csrc/kernels/lars.hip``, ``optim.LARS``) and label smoothing in the fused softmax
cross entropy, on the GPU.  The oracle throughout is ``ops.reference.lars_momentum_`` /
``lars_trust_ratio`` (float64 norms) and ``torch.nn.functional.cross_entropy``; tolerances are the
ones ``test_sgd_flat`` and ``test_softmax_xent_and_top1`` use."""
import copy

import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_tutorials_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

GRAD_SCALE = [1, 1e-3, 10, 1, 1e2, 1e-2, 1e3, 1e-3, 1, 30, 0]
EXCLUDED = {0, 3, 5}   # a 1-element, an unaligned 10-element and a 1000-element segment
ZERO_PARAM = 4         # |p| == 0 (adapted, so degenerate)
WD, ETA, EPS = 1e-4, 1.0, 1e-8


def _sizes(C):
    chunk = int(C.lars_chunk_elems())
    return [1, 3, 7, 10, 64, 1000, 4099, chunk, chunk + 1, 70001, 5120]


@pytest.fixture(scope="module")
def flat(gpu, native_ext):
    """Host copies of the flat buffers (never modified): parameters and three steps of gradients."""
    sizes = _sizes(native_ext)
    assert len(sizes) == len(GRAD_SCALE)
    offs = [sum(sizes[:i]) for i in range(len(sizes))]
    g = torch.Generator().manual_seed(123)
    n = sum(sizes)
    p = torch.randn(n, generator=g)
    p[offs[ZERO_PARAM]:offs[ZERO_PARAM] + sizes[ZERO_PARAM]] = 0
    grads = []
    for _ in range(3):
        gr = torch.randn(n, generator=g)
        for o, s, sc in zip(offs, sizes, GRAD_SCALE):
            gr[o:o + s] *= sc
        grads.append(gr)
    assert any(o % 4 for o in offs)
    return {"sizes": sizes, "offs": offs, "p": p, "grads": grads, "n": n}


def _table(flat, gpu):
    from pytorch_distributed_tutorials_amd.optim.lars import LarsTable
    return LarsTable([(o, s, i in EXCLUDED) for i, (o, s) in enumerate(zip(flat["offs"], flat["sizes"]))], gpu)


def _segments(flat, t):
    """Per-segment views shaped so that ``exclude_1d`` marks exactly the EXCLUDED segments."""
    return [t[o:o + s] if i in EXCLUDED else t[o:o + s].view(-1, 1)
            for i, (o, s) in enumerate(zip(flat["offs"], flat["sizes"]))]


def test_trust_ratios_match_float64_oracle(gpu, native_ext, flat):
    C = native_ext
    tb = _table(flat, gpu)
    assert tb.nchunks == sum(-(-s // int(C.lars_chunk_elems())) for s in flat["sizes"])
    p, g = flat["p"].to(gpu), flat["grads"][0].to(gpu)
    tb.trust.fill_(-7.0)
    C.lars_trust(p, g, tb.table, tb.partials, tb.trust, 0, tb.nseg, WD, ETA, EPS)
    got = tb.trust.cpu()
    want = torch.tensor([ref.lars_trust_ratio(ps, gs, WD, ETA, EPS, i in EXCLUDED)
                         for i, (ps, gs) in enumerate(zip(_segments(flat, flat["p"]),
                                                          _segments(flat, flat["grads"][0])))])
    ulps = (got.view(torch.int32) - want.view(torch.int32)).abs()
    print("trust", got.tolist(), "ulps", ulps.tolist())
    adapted = 0
    for i in range(tb.nseg):
        if i in EXCLUDED or i == ZERO_PARAM or GRAD_SCALE[i] == 0:
            assert got[i].item() == 1.0, (i, got[i].item())
        else:
            assert ulps[i].item() <= 2, (i, got[i].item(), want[i].item())
            assert got[i].item() != 1.0
            adapted += 1
    assert adapted == 6


def _run_gpu(C, flat, gpu, mom, nest, parts, mirror=True):
    tb = _table(flat, gpu)
    p = flat["p"].to(gpu)
    buf = torch.zeros_like(p) if mom != 0 else None
    pb = torch.zeros(flat["n"], dtype=torch.bfloat16, device=gpu) if mirror else None
    for step, gr in enumerate(flat["grads"]):
        g = gr.to(gpu)
        for lo, hi in parts:
            C.lars_step(p, g, buf, tb.table, tb.partials, tb.trust, lo, hi, 0.1, mom, 0.0, WD, nest,
                        step == 0, ETA, EPS, pb)
    torch.cuda.synchronize()
    return p, buf, pb, tb.trust.clone()


@pytest.mark.parametrize("mom,nest", [(0.9, False), (0.9, True), (0.0, False)],
                         ids=["momentum", "nesterov", "momentum0"])
def test_update_matches_reference(gpu, native_ext, flat, mom, nest):
    p, buf, pb, _ = _run_gpu(native_ext, flat, gpu, mom, nest, [(0, len(flat["sizes"]))])
    rp = flat["p"].clone()
    rb = torch.zeros_like(rp)
    ps, bs = _segments(flat, rp), _segments(flat, rb)
    for step, gr in enumerate(flat["grads"]):
        ref.lars_momentum_(ps, _segments(flat, gr), bs if mom != 0 else [None] * len(ps), 0.1, mom, 0.0, WD,
                           nest, step == 0, ETA, EPS, True)
    dp = (p.cpu() - rp).abs()
    print("max |p - ref|", dp.max().item(), "max |p|", rp.abs().max().item())
    assert torch.allclose(p.cpu(), rp, atol=1e-6), dp.max().item()
    if mom != 0:
        assert torch.allclose(buf.cpu(), rb, atol=1e-6), (buf.cpu() - rb).abs().max().item()
    # not vacuous: every adapted segment with a gradient moved
    moved = (p.cpu() - flat["p"]).abs()
    for i, (o, s) in enumerate(zip(flat["offs"], flat["sizes"])):
        if i not in EXCLUDED and GRAD_SCALE[i] != 0:
            assert moved[o:o + s].mean().item() > 1e-2, (i, moved[o:o + s].mean().item())
    # the bf16 mirror side output is the rounded new parameter
    assert torch.equal(pb, p.to(torch.bfloat16))


def test_partition_independence_and_determinism(gpu, native_ext, flat):
    nseg = len(flat["sizes"])
    assert flat["offs"][4] % 4 != 0  # the second call starts at an unaligned segment
    whole = _run_gpu(native_ext, flat, gpu, 0.9, True, [(0, nseg)])
    split = _run_gpu(native_ext, flat, gpu, 0.9, True, [(0, 4), (4, 7), (7, nseg)])
    again = _run_gpu(native_ext, flat, gpu, 0.9, True, [(0, 4), (4, 7), (7, nseg)])
    for a, b, c in zip(whole, split, again):
        assert torch.equal(a, b)
        assert torch.equal(b, c)


def test_binding_rejects_bad_tables(gpu, native_ext, flat):
    C = native_ext
    tb = _table(flat, gpu)
    p, g = flat["p"].to(gpu), flat["grads"][0].to(gpu)
    with pytest.raises(RuntimeError, match="segment range"):
        C.lars_trust(p, g, tb.table, tb.partials, tb.trust, 0, tb.nseg + 1, WD, ETA, EPS)
    with pytest.raises(RuntimeError, match="table size"):
        C.lars_trust(p, g, tb.table[:-16], tb.partials, tb.trust, 0, tb.nseg, WD, ETA, EPS)
    with pytest.raises(RuntimeError, match="momentum"):
        C.lars_step(p, g, None, tb.table, tb.partials, tb.trust, 0, tb.nseg, 0.1, 0.9, 0.0, WD, False, True,
                    ETA, EPS)


# ------------------------------------------------------------------ on a model
@pytest.fixture
def det_mode():
    from pytorch_distributed_tutorials_amd.utils import seed
    old = seed._DETERMINISTIC
    yield seed
    seed.set_random_seeds(0, deterministic=old)


HYPER = dict(lr=0.1, momentum=0.9, weight_decay=1e-4, trust_coefficient=0.02)


def _build(gpu, overlap, force=False, comm="auto"):
    from pytorch_distributed_tutorials_amd.models import build_model
    from pytorch_distributed_tutorials_amd.optim import LARS
    from pytorch_distributed_tutorials_amd.parallel import DistributedDataParallel
    torch.manual_seed(0)
    model = build_model("resnet18", num_classes=10, impl="native").to(gpu)
    model.set_impl("native")
    ddp = DistributedDataParallel(model, force_reducer=force, bucket_cap_mb=8, comm=comm)
    return ddp, LARS(ddp.parameters(), overlap=overlap, **HYPER)


def _data(gpu, steps, batch=8, size=32):
    g = torch.Generator().manual_seed(7)
    xs = [torch.randn(batch, 3, size, size, generator=g).to(gpu) for _ in range(steps)]
    ys = [torch.randint(0, 10, (batch,), generator=g).to(gpu) for _ in range(steps)]
    return xs, ys


def test_optimizer_matches_reference_on_resnet18(gpu, det_mode):
    from pytorch_distributed_tutorials_amd import ops
    det_mode.set_random_seeds(0, deterministic=True)
    ddp, opt = _build(gpu, overlap=False)
    params = list(ddp.parameters())
    xs, ys = _data(gpu, 3)
    for step, (x, y) in enumerate(zip(xs, ys)):
        opt.zero_grad()
        ops.cross_entropy(ddp(x), y).backward()
        p0 = [p.detach().cpu().clone() for p in params]
        g0 = [p.grad.detach().cpu().clone() for p in params]
        b0 = [torch.zeros_like(p) if step == 0 else opt.state[q]["momentum_buffer"].detach().cpu().clone()
              for p, q in zip(p0, params)]
        opt.step()
        ref.lars_momentum_(p0, g0, b0, HYPER["lr"], 0.9, 0.0, 1e-4, False, step == 0, 0.02, 1e-8, True)
        worst = 0.0
        for p, want, wb in zip(params, p0, b0):
            worst = max(worst, (p.detach().cpu() - want).abs().max().item())
            assert torch.allclose(p.detach().cpu(), want, atol=1e-6)
            assert torch.allclose(opt.state[p]["momentum_buffer"].cpu(), wb, atol=1e-6)
        print("step", step, "max |p - ref|", worst)
    # momentum_buffer entries are views of the flat buffer, in torch's state_dict format
    buf = opt._flat_bufs[id(ddp.space)]
    for p, o in zip(ddp.space.params, ddp.space.offsets):
        mb = opt.state[p]["momentum_buffer"]
        assert mb.data_ptr() == buf.data_ptr() + 4 * o
    assert len(opt.state_dict()["state"]) == len(params)


def _train(ddp, opt, xs, ys):
    from pytorch_distributed_tutorials_amd import ops
    for x, y in zip(xs, ys):
        opt.zero_grad()
        loss = ops.cross_entropy(ddp(x), y)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    return loss.item()


@pytest.mark.parametrize("mode", ["local", "rccl_world1", "xgmi_world1"])
def test_per_bucket_update_bitwise_equals_post_backward_step(gpu, det_mode, mode):
    det_mode.set_random_seeds(0, deterministic=True)
    kw = {"local": {}, "rccl_world1": {"force": True}, "xgmi_world1": {"comm": "xgmi"}}[mode]
    xs, ys = _data(gpu, 4)
    ddp_a, opt_a = _build(gpu, overlap=False, **kw)
    la = _train(ddp_a, opt_a, xs, ys)
    ddp_b, opt_b = _build(gpu, overlap=None, **kw)
    assert opt_b._overlap_owner is not None, "the per-bucket update did not attach"
    assert ddp_b.reducer is not None and ddp_b.reducer.num_buckets >= 3
    if mode == "local":
        assert ddp_b.reducer.local
    if mode == "xgmi_world1":
        assert ddp_b.xgmi is not None
    lb = _train(ddp_b, opt_b, xs, ys)
    assert la == lb
    pa, pb = ddp_a.space.param_flat, ddp_b.space.param_flat
    assert torch.equal(pa, pb), (pa - pb).abs().max().item()
    assert torch.equal(opt_a._flat_bufs[id(ddp_a.space)], opt_b._flat_bufs[id(ddp_b.space)])
    assert torch.equal(ddp_a.space.mirror().krsc, ddp_b.space.mirror().krsc)
    # both paths left the same trust ratios behind, and they are real ratios
    ta = opt_a._table(ddp_a.space, True).trust
    tb = opt_b._table(ddp_b.space, True).trust
    assert torch.equal(ta, tb)
    assert (ta != 1).sum().item() >= 20


def test_per_bucket_lr_change_still_raises(gpu):
    from pytorch_distributed_tutorials_amd import ops
    xs, ys = _data(gpu, 1)
    ddp, opt = _build(gpu, overlap=None)
    assert opt._overlap_owner is not None
    ops.cross_entropy(ddp(xs[0]), ys[0]).backward()
    opt.param_groups[0]["lr"] = 0.5
    with pytest.raises(RuntimeError, match="hyperparameters changed"):
        opt.step()
    ddp2, opt2 = _build(gpu, overlap=None)
    ops.cross_entropy(ddp2(xs[0]), ys[0]).backward()
    opt2.param_groups[0]["trust_coefficient"] = 0.5
    with pytest.raises(RuntimeError, match="hyperparameters changed"):
        opt2.step()


def test_captured_lars_step_matches_eager(gpu, det_mode):
    from pytorch_distributed_tutorials_amd import ops
    from pytorch_distributed_tutorials_amd.utils.graph import CapturedStep
    det_mode.set_random_seeds(0, deterministic=True)
    x = torch.randn(8, 3, 32, 32, device=gpu)
    y = torch.randint(0, 10, (8,), device=gpu)
    runs = []
    for graphed in (False, True):
        ddp, opt = _build(gpu, overlap=False)

        def step():
            opt.zero_grad()
            loss = ops.cross_entropy(ddp(x), y)
            loss.backward()
            opt.step()
            return loss
        for _ in range(2):
            step()
        run = CapturedStep(step, warmup=0) if graphed else step
        losses = [float(run()) for _ in range(3)]
        runs.append((losses, ddp.space.param_flat.clone(), opt._flat_bufs[id(ddp.space)].clone()))
    (l0, p0, b0), (l1, p1, b1) = runs
    assert l0 == l1, (l0, l1)
    assert torch.equal(p0, p1) and torch.equal(b0, b1)


# ------------------------------------------------------------ label smoothing
@pytest.mark.parametrize("shape", [(5, 10), (33, 1000), (7, 1001)])
def test_label_smoothing_matches_torch(gpu, native_ext, shape):
    from pytorch_distributed_tutorials_amd import ops
    n, v = shape
    g = torch.Generator().manual_seed(17)
    logits = (3 * torch.randn(n, v, generator=g)).to(gpu)
    labels = torch.randint(0, v, (n,), generator=g).to(gpu)
    lt = logits.clone().requires_grad_(True)
    want = F.cross_entropy(lt, labels, label_smoothing=0.1)
    (dwant,) = torch.autograd.grad(want, lt)
    loss, dl = native_ext.softmax_xent(logits, labels, 0.1)
    print("dloss", abs(loss.item() - want.item()), "ddl", (dl - dwant).abs().max().item())
    assert abs(loss.item() - want.item()) < 1e-4
    assert torch.allclose(dl, dwant, atol=1e-6)
    # eps = 0 is the unsmoothed kernel, bit for bit
    l0, d0 = native_ext.softmax_xent(logits, labels)
    l1, d1 = native_ext.softmax_xent(logits, labels, 0.0)
    assert torch.equal(l0, l1) and torch.equal(d0, d1)
    a = ops.cross_entropy(logits, labels)
    b = ops.cross_entropy(logits, labels, label_smoothing=0.0)
    assert torch.equal(a, b)
    # backward through ops.cross_entropy with a non-unit upstream gradient
    lo = logits.clone().requires_grad_(True)
    (ops.cross_entropy(lo, labels, label_smoothing=0.1) * 2.5).backward()
    assert torch.allclose(lo.grad, 2.5 * dwant, atol=2.5e-6)
    assert abs(ops.CrossEntropyLoss(label_smoothing=0.1)(logits, labels).item() - want.item()) < 1e-4
