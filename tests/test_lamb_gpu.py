"""Fused LAMB / AdamW (``csrc/opt/lamb.hip``, ``_C_opt``, ``optim.LAMB``) on the GPU against
``ops.reference.lamb_`` evaluated in float64 on float64 copies of the fp32 inputs.

The flat fixture reaches every branch: unaligned lead and tail, exactly one chunk, a chunk plus one
element, more than 64 chunks (the trust wave's lane stride loops), excluded, all-zero and zero-gradient
segments.  ``test_lamb_cpu.py`` holds the fp32 CPU reference to the bounds below without a GPU.
"""
import functools

import pytest
import torch

from pytorch_distributed_tutorials_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 7, 10, 64, 1000, 4099, 4096, 4097, 5120, 64 * 4096 + 1]
GRAD_SCALE = [1, 1e-3, 30, 1, 1e-3, 30, 1, 1e-3, 30, 0, 1]
EXCLUDED = {0, 3, 5}   # a 1-element, an unaligned 10-element and a 1000-element segment
ZERO_PARAM = 4         # |p| == 0 before the first step: ratio 1
ZERO_GRAD = 9          # g == 0 at every step: u = wd p, so |u| == 0 and ratio 1 when wd == 0
LR, B1, B2, EPS = 0.05, 0.9, 0.999, 1e-6

# Bounds: what ``ref.lamb_`` in fp32 on the CPU differs from its float64 evaluation by on this fixture
# (three steps, every trust / wd combination below): p absolutely, m and v relative to their segment's
# largest magnitude, the ratios in fp32 ulps.  The kernels may contract and order their fmas differently
# from ATen's fp32 and nothing else: the GPU tests allow 4x, test_lamb_cpu.py holds the reference to 1x.
P_ABS = 5.4e-7      # measured 5.35e-07 (|p| reaches 4.7)
M_REL = 1.6e-7      # measured 1.55e-07
V_REL = 1.6e-7      # measured 1.53e-07
RATIO_ULPS = 2      # measured 2 (LARS's bound is 2 as well)
SLACK = 4


@functools.lru_cache(maxsize=None)
def build_flat():
    """Host copies of the flat buffers (never modified): parameters and three steps of gradients."""
    offs = [sum(SIZES[:i]) for i in range(len(SIZES))]
    g = torch.Generator().manual_seed(321)
    n = sum(SIZES)
    p = torch.randn(n, generator=g)
    p[offs[ZERO_PARAM]:offs[ZERO_PARAM] + SIZES[ZERO_PARAM]] = 0
    grads = []
    for _ in range(3):
        gr = torch.randn(n, generator=g)
        for o, s, sc in zip(offs, SIZES, GRAD_SCALE):
            gr[o:o + s] *= sc
        grads.append(gr)
    assert any(o % 4 for o in offs) and offs[4] % 4 != 0
    return {"offs": offs, "p": p, "grads": grads, "n": n}


def segments(flat, t):
    """Per-segment views shaped so that ``exclude_1d`` marks exactly the EXCLUDED segments."""
    return [t[o:o + s] if i in EXCLUDED else t[o:o + s].view(-1, 1)
            for i, (o, s) in enumerate(zip(flat["offs"], SIZES))]


def run_reference(flat, dtype, trust, wd):
    """(p, m, v, ratios) after each of the three steps of ``ref.lamb_`` in ``dtype``."""
    p = flat["p"].to(dtype, copy=True)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    out = []
    for step, gr in enumerate(flat["grads"]):
        r = ref.lamb_(segments(flat, p), segments(flat, gr.to(dtype)), segments(flat, m), segments(flat, v),
                      step + 1, LR, B1, B2, EPS, wd, trust, True)
        out.append((p.clone(), m.clone(), v.clone(), torch.tensor(r, dtype=torch.float32)))
    return out


def seg_rel(flat, got, want):
    """Worst |got - want| relative to the largest |want| of its segment."""
    worst = 0.0
    for o, s in zip(flat["offs"], SIZES):
        top = want[o:o + s].abs().max().item()
        worst = max(worst, (got[o:o + s].double() - want[o:o + s]).abs().max().item() / max(top, 1e-300))
    return worst


def ulps(a, b):
    return (a.view(torch.int32) - b.view(torch.int32)).abs().max().item()


@functools.lru_cache(maxsize=None)
def _oracle(trust, wd):
    return run_reference(build_flat(), torch.float64, trust, wd)


def _run_gpu(flat, gpu, trust, mirror, wd, parts):
    """The three steps through ``_C_opt.lamb_step``; a snapshot after each."""
    from pytorch_distributed_tutorials_amd.ops._ext import native_opt
    from pytorch_distributed_tutorials_amd.optim.lars import LarsTable
    O = native_opt()
    tb = LarsTable([(o, s, i in EXCLUDED) for i, (o, s) in enumerate(zip(flat["offs"], SIZES))], gpu)
    p = flat["p"].to(gpu)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    rec = torch.zeros(int(O.record_elems()), dtype=torch.int64, device=gpu)
    pb = torch.zeros(flat["n"], dtype=torch.bfloat16, device=gpu) if mirror else None
    tb.trust.fill_(-7.0)
    out = []
    for gr in flat["grads"]:
        g = gr.to(gpu)
        for lo, hi in parts:
            O.lamb_step(p, g, m, v, tb.table, tb.partials, tb.trust, rec, lo, hi, LR, B1, B2, EPS, wd, trust,
                        hi == parts[-1][1], pb)
        out.append(tuple(t.clone() for t in (p, m, v, tb.trust, rec[:1])) + (None if pb is None else pb.clone(),))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("mirror", [True, False], ids=["mirror", "nomirror"])
@pytest.mark.parametrize("trust", [True, False], ids=["lamb", "adamw"])
def test_update_matches_float64_reference(gpu, native_ext, trust, mirror, wd):
    flat = build_flat()
    got = _run_gpu(flat, gpu, trust, mirror, wd, [(0, len(SIZES))])
    for step, ((p, m, v, tr, rec, pb), (rp, rm, rv, rr)) in enumerate(zip(got, _oracle(trust, wd))):
        dp = (p.cpu().double() - rp).abs().max().item()
        dm, dv = seg_rel(flat, m.cpu(), rm), seg_rel(flat, v.cpu(), rv)
        print("step", step, "max |p - ref|", dp, "m rel", dm, "v rel", dv)
        assert dp <= SLACK * P_ABS and dm <= SLACK * M_REL and dv <= SLACK * V_REL
        assert rec.item() == step + 1
        if mirror:
            assert torch.equal(pb, p.to(torch.bfloat16))
        if not trust:
            continue
        tr = tr.cpu()
        assert ulps(tr, rr) <= SLACK * RATIO_ULPS
        assert torch.equal(tr == 1, rr == 1) and (tr != 1).sum().item() >= 6
        degenerate = EXCLUDED | ({ZERO_PARAM} if step == 0 else set()) | ({ZERO_GRAD} if wd == 0 else set())
        assert all(tr[i].item() == 1.0 for i in degenerate)
    assert (got[-1][0].cpu() - flat["p"]).abs().mean().item() > 1e-2  # not vacuous: the parameters moved


@pytest.mark.parametrize("trust", [True, False], ids=["lamb", "adamw"])
def test_partition_independence_and_determinism(gpu, native_ext, trust):
    flat, nseg = build_flat(), len(SIZES)
    whole = _run_gpu(flat, gpu, trust, True, 1e-2, [(0, nseg)])
    split = _run_gpu(flat, gpu, trust, True, 1e-2, [(0, 4), (4, 7), (7, nseg)])
    again = _run_gpu(flat, gpu, trust, True, 1e-2, [(0, 4), (4, 7), (7, nseg)])
    for a, b, c in zip(whole[-1], split[-1], again[-1]):
        assert torch.equal(a, b) and torch.equal(b, c)


# ------------------------------------------------------------------ on a model
@pytest.fixture
def det_mode():
    from pytorch_distributed_tutorials_amd.utils import seed
    old = seed._DETERMINISTIC
    seed.set_random_seeds(0, deterministic=True)
    yield seed
    seed.set_random_seeds(0, deterministic=old)


HYPER = dict(lr=0.01, betas=(0.9, 0.99), eps=1e-6, weight_decay=1e-2)


def _build(gpu):
    from pytorch_distributed_tutorials_amd.models import build_model
    from pytorch_distributed_tutorials_amd.optim import LAMB
    from pytorch_distributed_tutorials_amd.parallel import DistributedDataParallel
    torch.manual_seed(0)
    model = build_model("resnet18", num_classes=10, impl="native").to(gpu)
    model.set_impl("native")
    ddp = DistributedDataParallel(model, bucket_cap_mb=8)
    return ddp, LAMB(ddp.parameters(), **HYPER)


def test_captured_step_matches_eager(gpu, det_mode):
    from pytorch_distributed_tutorials_amd import ops
    from pytorch_distributed_tutorials_amd.utils.graph import CapturedStep
    x = torch.randn(8, 3, 32, 32, device=gpu)
    y = torch.randint(0, 10, (8,), device=gpu)
    runs = []
    for graphed in (False, True):
        ddp, opt = _build(gpu)

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
        fs = opt._flat[id(ddp.space)]
        runs.append((losses, ddp.space.param_flat.clone(), fs.m.clone(), fs.v.clone(), fs.rec[:1].clone()))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert torch.equal(a, b)
    assert runs[1][4].item() == 5  # the replays advanced the device record


def test_optimizer_matches_reference_on_resnet18(gpu, det_mode):
    from pytorch_distributed_tutorials_amd import ops
    ddp, opt = _build(gpu)
    params = list(ddp.parameters())
    g = torch.Generator().manual_seed(7)
    for step in range(3):
        x = torch.randn(8, 3, 32, 32, generator=g).to(gpu)
        y = torch.randint(0, 10, (8,), generator=g).to(gpu)
        opt.zero_grad()
        ops.cross_entropy(ddp(x), y).backward()
        p0 = [p.detach().cpu().double() for p in params]
        g0 = [p.grad.detach().cpu().double() for p in params]
        m0 = [opt.state[p]["exp_avg"].cpu().double() for p in params]
        v0 = [opt.state[p]["exp_avg_sq"].cpu().double() for p in params]
        opt.step()
        ref.lamb_(p0, g0, m0, v0, step + 1, HYPER["lr"], 0.9, 0.99, 1e-6, 1e-2, True, True)
        # one step from the optimizer's own fp32 state: the bounds of the three-step fixture hold
        for p, wp, wm, wv in zip(params, p0, m0, v0):
            st = opt.state[p]
            assert (p.detach().cpu() - wp).abs().max().item() <= SLACK * P_ABS
            assert (st["exp_avg"].cpu() - wm).abs().max().item() <= SLACK * M_REL * wm.abs().max().item()
            assert (st["exp_avg_sq"].cpu() - wv).abs().max().item() <= SLACK * V_REL * wv.abs().max().item()
    fs = opt._flat[id(ddp.space)]
    for p, o in zip(ddp.space.params, ddp.space.offsets):
        assert opt.state[p]["exp_avg"].data_ptr() == fs.m.data_ptr() + 4 * o
        assert opt.state[p]["exp_avg_sq"].data_ptr() == fs.v.data_ptr() + 4 * o
    sd = opt.state_dict()
    assert len(sd["state"]) == len(params) and all(int(s["step"]) == 3 for s in sd["state"].values())
    assert (fs.table.trust != 1).sum().item() >= 20
