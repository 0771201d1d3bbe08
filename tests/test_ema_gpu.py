"""Weight EMA on the GPU: the ``_C_ema.ema_update`` kernel against an fp64 reference, its buffer
segments, and ``optim.ModelEma`` on the native ResNet-18 -- against torch's ``AveragedModel``, the
coherence of the twin's bf16 weight mirror with its fp32 weights, the ordering behind the per-bucket
optimizer update, and the eager update beside a replayed HIP graph.

The error bound of one update, per element: ``|got - ref| <= 5 * 2**-24 * max(|e|, |p|)`` with
``ref = e64 + float64(float32(w)) * (p64 - e64)``.  Three roundings at most (the difference, the
product, the sum -- two with a fused multiply-add), each of relative size 2**-24, on magnitudes
``|p - e| <= 2 * max``, ``w * |p - e| <= 2 * max`` and ``|result| <= max`` for w in [0, 1].
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 5.0 * 2.0 ** -24
NS = (0, 1, 3, 4, 5, 255, 256, 257, 1023)
LEADS = (0, 1, 2, 3)
PAD = 8  # canary elements on both sides of every view (keeps the 16-byte phase of the base)


@pytest.fixture(scope="module")
def E(native_ext):
    from pytorch_distributed_tutorials_amd.ops import _ext
    return _ext.native_ema()


@pytest.fixture
def det_mode():
    from pytorch_distributed_tutorials_amd.utils import seed
    old = seed._DETERMINISTIC
    seed.set_random_seeds(0, deterministic=True)
    yield seed
    seed.set_random_seeds(0, deterministic=old)


def _ref64(e, p, w):
    w32 = torch.tensor(w, dtype=torch.float32).double().item()
    return e.double() + w32 * (p.double() - e.double())


def _within(got, e, p, w):
    """The worst ratio of |got - ref| to the bound's unit max(|e|, |p|) * 2**-24 * 5 (<= 1 passes)."""
    err = (got.double() - _ref64(e, p, w)).abs()
    unit = U * torch.maximum(e.abs(), p.abs()).double()
    assert bool((err <= unit).all()), (err / unit.clamp_min(1e-300)).max().item()


def _case(E, gpu, gen, n, lead, w, mirror=True):
    """One update of views that start ``lead`` elements before a 16-byte boundary, canaries around."""
    start = PAD + (4 - lead) % 4
    total = start + n + PAD
    big_e = torch.randn(total, generator=gen).to(gpu)
    big_p = (big_e.cpu() + torch.randn(total, generator=gen)).to(gpu)
    big_k = torch.full((total,), 7.0, dtype=torch.bfloat16, device=gpu)
    assert big_e.data_ptr() % 16 == 0 and big_p.data_ptr() % 16 == 0 and big_k.data_ptr() % 16 == 0
    e0, p0 = big_e.clone(), big_p.clone()
    e, p, k = big_e[start:start + n], big_p[start:start + n], big_k[start:start + n]
    E.ema_update(e, p, w, k if mirror else None)
    torch.cuda.synchronize()
    old = e0[start:start + n]
    _within(e, old, p, w)
    if w == 1.0:
        assert torch.equal(e, p)
    if w == 0.0:
        assert torch.equal(e, old)
    assert torch.equal(big_p, p0)
    assert torch.equal(big_e[:start], e0[:start]) and torch.equal(big_e[start + n:], e0[start + n:])
    want_k = e.to(torch.bfloat16) if mirror else torch.full_like(k, 7.0)
    assert torch.equal(k, want_k)
    assert bool((big_k[:start] == 7.0).all()) and bool((big_k[start + n:] == 7.0).all())


@pytest.mark.parametrize("w", [0.0, 2e-5, 1e-4, 0.5, 1.0])
def test_kernel_matches_fp64_reference(gpu, E, w):
    gen = torch.Generator().manual_seed(11)
    for n in NS:
        for lead in LEADS:
            _case(E, gpu, gen, n, lead, w)
    _case(E, gpu, gen, 257, 3, w, mirror=False)


def test_kernel_large_grid_stride(gpu, E):
    """Just above one sweep of the full grid (4096 blocks x 256 threads x 4 elements): some threads
    take a second trip of the grid-stride loop, and the tail follows."""
    gen = torch.Generator().manual_seed(12)
    _case(E, gpu, gen, 4096 * 256 * 4 + 7, 1, 1e-4)


def test_buffer_segments_in_the_same_launch(gpu, E):
    gen = torch.Generator().manual_seed(13)
    w = 0.1
    e = torch.randn(1000, generator=gen).to(gpu)
    p = (e.cpu() + torch.randn(1000, generator=gen)).to(gpu)
    k = torch.zeros(1000, dtype=torch.bfloat16, device=gpu)
    big_b = torch.randn(PAD + 3 + 333 + PAD, generator=gen).to(gpu)
    big_m = (big_b.cpu() + torch.randn(big_b.numel(), generator=gen)).to(gpu)
    be, bm = big_b[PAD + 3:PAD + 3 + 333], big_m[PAD + 3:PAD + 3 + 333]
    big_i = torch.arange(100, 100 + 53 + 2 * PAD, dtype=torch.int64, device=gpu)
    ie = big_i[PAD:PAD + 53]
    im = torch.randint(0, 1 << 40, (53,), generator=gen).to(gpu)
    e0, b0, i0, im0 = e.clone(), big_b.clone(), big_i.clone(), im.clone()
    E.ema_update(e, p, w, k, be, bm, ie, im)
    torch.cuda.synchronize()
    _within(e, e0, p, w)
    assert torch.equal(k, e.to(torch.bfloat16))
    _within(be, b0[PAD + 3:PAD + 3 + 333], bm, w)
    assert not torch.equal(be, b0[PAD + 3:PAD + 3 + 333])
    assert torch.equal(big_b[:PAD + 3], b0[:PAD + 3]) and torch.equal(big_b[PAD + 3 + 333:], b0[PAD + 3 + 333:])
    assert torch.equal(ie, im) and torch.equal(im, im0)
    assert torch.equal(big_i[:PAD], i0[:PAD]) and torch.equal(big_i[PAD + 53:], i0[PAD + 53:])
    # the parameter segment may be empty while the others are not
    E.ema_update(e[:0], p[:0], 1.0, None, be, bm, ie, im)
    torch.cuda.synchronize()
    assert torch.equal(be, bm)


# ----------------------------------------------------------------------------- ModelEma
def _build(gpu, overlap=None, seed=0):
    from pytorch_distributed_tutorials_amd.models import build_model
    from pytorch_distributed_tutorials_amd.optim import SGD
    from pytorch_distributed_tutorials_amd.parallel import DistributedDataParallel
    torch.manual_seed(seed)
    model = build_model("resnet18", num_classes=10, impl="native").to(gpu)
    model.set_impl("native")
    ddp = DistributedDataParallel(model)
    opt = SGD(ddp.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4, overlap=overlap)
    return ddp, opt


def _data(gpu, steps, batch=8):
    g = torch.Generator().manual_seed(7)
    xs = [torch.randn(batch, 3, 32, 32, generator=g).to(gpu) for _ in range(steps)]
    ys = [torch.randint(0, 10, (batch,), generator=g).to(gpu) for _ in range(steps)]
    return xs, ys


def _step(ddp, opt, x, y):
    from pytorch_distributed_tutorials_amd import ops
    opt.zero_grad()
    ops.cross_entropy(ddp(x), y).backward()
    opt.step()


def _flat_state(ema):
    tsp, _, mirror, (fe, _), (ie, _) = ema._flat
    return [tsp.param_flat, mirror.krsc, fe, ie]


def test_model_ema_matches_averaged_model(gpu, E, det_mode):
    """Three SGD steps with an update after each, against an AveragedModel of CPU fp32 copies fed the
    model's state after each step.  Update 0 is a copy on both sides (exact).  Updates 1 and 2 each
    add at most the one-update bound 5 * 2**-24 * max(|e_before|, |p|) -- an earlier deviation is
    scaled by 1 - w <= 1 on its way through a later update -- so the bound accumulates as their sum.
    Integer buffers are copied by ModelEma (the oracle averages and truncates them): they are
    compared with the model's."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    from pytorch_distributed_tutorials_amd.models import build_model
    from pytorch_distributed_tutorials_amd.optim import ModelEma
    ddp, opt = _build(gpu)
    ema = ModelEma(ddp, 0.9)
    assert ema._flat is not None, "the one-launch path did not engage"
    tsp, sp = ema._flat[0], ema._flat[1]
    assert tsp.grad_flat is None and tsp.offsets == sp.offsets and tsp.param_flat.numel() == sp.param_flat.numel()
    assert not ema._float_pairs and not ema._int_pairs  # parameters, BN statistics and counters: all in the launch
    cpu = build_model("resnet18", num_classes=10, impl="torch")
    cpu.load_state_dict(ddp.module.state_dict())
    oracle = AveragedModel(cpu, use_buffers=True, multi_avg_fn=get_ema_multi_avg_fn(0.9))
    xs, ys = _data(gpu, 3)
    bound = None
    for k, (x, y) in enumerate(zip(xs, ys)):
        _step(ddp, opt, x, y)
        ema.update()
        cpu.load_state_dict(ddp.module.state_dict())
        before = {n: v.clone() for n, v in oracle.module.state_dict().items()}
        oracle.update_parameters(cpu)
        now = cpu.state_dict()
        if k == 0:
            bound = {n: torch.zeros_like(v, dtype=torch.float64) for n, v in before.items()}
        else:
            for n in bound:
                bound[n] += U * torch.maximum(before[n].abs(), now[n].abs()).double()
    torch.cuda.synchronize()
    assert ema.num_updates == 3
    got, want, cur = ema.module.state_dict(), oracle.module.state_dict(), ddp.module.state_dict()
    assert list(got) == list(want)
    for n in got:
        if got[n].is_floating_point():
            err = (got[n].cpu().double() - want[n].double()).abs()
            assert bool((err <= bound[n]).all()), (n, err.max().item())
        else:
            assert torch.equal(got[n], cur[n]) and int(got[n]) == 3, n
    assert not torch.equal(got["conv1.weight"], cur["conv1.weight"])


def test_twin_mirror_is_coherent_with_its_weights(gpu, E, det_mode):
    """The twin's forward reads the bf16 image the update kernel wrote as a side output; a fresh
    model that loads the twin's fp32 state builds its image by the cast path.  Bitwise-equal logits
    mean the side output is current and correct; a stale mirror would repeat the previous logits."""
    from pytorch_distributed_tutorials_amd.optim import ModelEma
    ddp, opt = _build(gpu)
    ema = ModelEma(ddp, 0.9)
    mirror = ema._flat[2]
    refreshes = []
    cast = mirror.refresh
    mirror.refresh = lambda: (refreshes.append(1), cast())[1]
    xs, ys = _data(gpu, 4)
    probe = xs[3]
    for k in range(3):
        _step(ddp, opt, xs[k], ys[k])
        if k == 2:
            with torch.no_grad():
                before = ema.module(probe).clone()
        ema.update()
    with torch.no_grad():
        out = ema.module(probe).clone()
        again = ema.module(probe).clone()
    assert not refreshes, "the twin's forward re-cast its weights: the side output was not trusted"
    assert mirror.valid() and ema._stale is None
    fresh, _ = _build(gpu, seed=1)
    fresh.load_state_dict(ema.state_dict())
    fresh.eval()
    with torch.no_grad():
        want = fresh(probe)
    assert fresh.space.mirror().valid()
    torch.cuda.synchronize()
    assert torch.equal(fresh.space.mirror().krsc, mirror.krsc)
    assert torch.equal(out, want) and torch.equal(again, out)
    assert not torch.equal(out, before)
    assert bool(torch.isfinite(out).all())


def test_update_is_ordered_behind_the_per_bucket_step(gpu, E, det_mode):
    from pytorch_distributed_tutorials_amd.optim import ModelEma
    xs, ys = _data(gpu, 3)
    states = []
    for overlap in (None, False):
        ddp, opt = _build(gpu, overlap=overlap)
        assert (opt._overlap_owner is not None) == (overlap is None)
        ema = ModelEma(ddp, 0.9)
        for x, y in zip(xs, ys):
            _step(ddp, opt, x, y)
            ema.update()
        torch.cuda.synchronize()
        states.append([t.clone() for t in _flat_state(ema)] + [ddp.space.param_flat.clone()])
    for a, b in zip(*states):
        assert torch.equal(a, b)


def test_eager_update_beside_a_replayed_graph(gpu, E, det_mode):
    """Five steps through train._GraphStep (three eager warm-up steps, a capture, replays) with an
    eager update() after each give the same EMA, bit for bit, as five eager steps."""
    from pytorch_distributed_tutorials_amd import ops
    from pytorch_distributed_tutorials_amd.optim import ModelEma
    from pytorch_distributed_tutorials_amd.train import _GraphStep
    xs, ys = _data(gpu, 5, batch=16)
    states = []
    for graph in (False, True):
        ddp, opt = _build(gpu, overlap=False)
        ema = ModelEma(ddp, 0.9)
        gs = _GraphStep(ddp, ops.cross_entropy, opt) if graph else None
        for x, y in zip(xs, ys):
            if gs is not None:
                gs(x, y)
            else:
                _step(ddp, opt, x, y)
            ema.update()
        torch.cuda.synchronize()
        if gs is not None:
            assert gs.captured is not None and gs.captured.calls == 2
        states.append([t.clone() for t in _flat_state(ema)] + [ddp.space.param_flat.clone()])
    assert ema.num_updates == 5
    for a, b in zip(*states):
        assert torch.equal(a, b)
