"""LAMB / AdamW without a GPU: the reference, ``optim.LAMB``'s per-tensor path, schedule, flags, the
``_C_opt`` module and its argument checks, and the error bounds the GPU tests use."""
import copy
import math
import os

import pytest
import torch

import test_lamb_gpu as lg
from pytorch_distributed_tutorials_amd.ops import reference as ref
from pytorch_distributed_tutorials_amd.optim import LAMB, WarmupCosineLR


def _tensors(dtype=torch.float64, seed=3):
    g = torch.Generator().manual_seed(seed)
    shapes = [(5, 4), (7,), (2, 3, 3, 3), (1,)]
    return [torch.randn(s, generator=g).to(dtype) for s in shapes], \
        [[torch.randn(s, generator=g).to(dtype) for s in shapes] for _ in range(3)]


def test_reference_without_trust_is_torch_adamw():
    ps, grads = _tensors()
    want = [torch.nn.Parameter(p.clone()) for p in ps]
    opt = torch.optim.AdamW(want, lr=0.01, betas=(0.9, 0.99), eps=1e-6, weight_decay=0.1)
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    for step, gs in enumerate(grads):
        for w, g in zip(want, gs):
            w.grad = g.clone()
        opt.step()
        assert ref.lamb_(ps, gs, ms, vs, step + 1, 0.01, 0.9, 0.99, 1e-6, 0.1, False, False) == [1.0] * len(ps)
        for p, w in zip(ps, want):
            assert (p - w.detach()).abs().max().item() <= 1e-12


def test_reference_trust_ratio_by_hand_and_degenerate_cases():
    # step 1 with eps = 0: a = sign(g), so u = (1, -1, 1, 1) + 0.5 p and ratio = |p| / |u|
    p = torch.tensor([[3.0, 4.0], [0.0, 0.0]], dtype=torch.float64)
    g = torch.tensor([[2.0, -1.0], [0.5, 8.0]], dtype=torch.float64)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    (r,) = ref.lamb_([p], [g], [m], [v], 1, 0.1, 0.9, 0.999, 0.0, 0.5)
    u = torch.tensor([[2.5, 1.0], [1.0, 1.0]], dtype=torch.float64)
    assert r == pytest.approx(5.0 / math.sqrt(2.5 ** 2 + 3.0), rel=1e-7)
    want = torch.tensor([[3.0, 4.0], [0.0, 0.0]], dtype=torch.float64) - 0.1 * r * u
    assert (p - want).abs().max().item() < 1e-12
    assert torch.allclose(m, 0.1 * g) and torch.allclose(v, 0.001 * g * g)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    assert ref.lamb_([z(2, 2)], [g.clone()], [z(2, 2)], [z(2, 2)], 1, 0.1) == [1.0]                   # |p| == 0
    assert ref.lamb_([p.clone()], [z(2, 2)], [z(2, 2)], [z(2, 2)], 1, 0.1) == [1.0]                   # |u| == 0
    assert ref.lamb_([p.view(-1).clone()], [g.view(-1)], [z(4)], [z(4)], 1, 0.1, weight_decay=0.5) == [1.0]  # 1-D


@pytest.mark.parametrize("trust", [True, False], ids=["lamb", "adamw"])
def test_optimizer_cpu_path_and_state_dict_round_trip(trust):
    ps, grads = _tensors(torch.float32)
    params = [torch.nn.Parameter(p.clone()) for p in ps]
    kw = dict(lr=0.02, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.1, trust=trust)
    opt = LAMB(params, **kw)
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    twin = None
    for step, gs in enumerate(grads):
        for w, g in zip(params, gs):
            w.grad = g.clone()
        opt.step()
        ref.lamb_(ps, gs, ms, vs, step + 1, 0.02, 0.8, 0.95, 1e-6, 0.1, trust, True)
        for p, w, m, v in zip(ps, params, ms, vs):
            assert torch.equal(p, w.detach()) and torch.equal(opt.state[w]["exp_avg"], m)
            assert torch.equal(opt.state[w]["exp_avg_sq"], v) and int(opt.state[w]["step"]) == step + 1
        if twin is not None:  # a twin resumed from the state after step 1 stays bitwise on track
            for w, g in zip(twin_params, gs):
                w.grad = g.clone()
            twin.step()
            assert all(torch.equal(a, b) for a, b in zip(twin_params, params))
        else:
            twin_params = [torch.nn.Parameter(w.detach().clone()) for w in params]
            twin = LAMB(twin_params, **kw)
            twin.load_state_dict(copy.deepcopy(opt.state_dict()))  # (torch shares the tensors otherwise)
    assert set(opt.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}  # torch.optim.Adam's format
    for bad in (dict(lr=-1.0), dict(betas=(1.0, 0.9)), dict(eps=-1.0), dict(weight_decay=-0.1)):
        with pytest.raises(ValueError):
            LAMB(params, **bad)
    assert "never attaches" in LAMB.__doc__


def test_warmup_cosine_schedule():
    s = WarmupCosineLR(None, 2.0, 4, 14, end_lr=0.2)
    assert [s.lr_at(i) for i in range(4)] == [0.5, 1.0, 1.5, 2.0]
    assert s.lr_at(4) == pytest.approx(2.0)                 # first decay step: t = 0
    assert s.lr_at(9) == pytest.approx(1.1)                 # midpoint: half way between 2.0 and 0.2
    assert s.lr_at(14) == pytest.approx(0.2) and s.lr_at(1000) == pytest.approx(0.2)
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=9.0)
    assert WarmupCosineLR(opt, 1.0, 2, 10).set(0) == 0.5 and opt.param_groups[0]["lr"] == 0.5
    with pytest.raises(ValueError):
        WarmupCosineLR(None, 1.0, 5, 3)


def test_trainer_flags():
    from pytorch_distributed_tutorials_amd.train import build_parser, main
    a = build_parser().parse_args([])
    assert (a.optimizer, a.beta1, a.beta2, a.adam_eps, a.lamb_adapt_1d) == ("sgd", 0.9, 0.999, 1e-6, False)
    for name in ("lamb", "adamw"):
        a = build_parser().parse_args(["--optimizer", name, "--lr-schedule", "warmup-cosine", "--lamb-adapt-1d"])
        assert (a.optimizer, a.lr_schedule, a.lamb_adapt_1d) == (name, "warmup-cosine", True)
    for bad, msg in ((["--optimizer", "lamb", "--beta1", "1.0"], "--beta1 / --beta2 must be in [0, 1)"),
                     (["--optimizer", "adamw", "--beta2", "-0.1"], "--beta1 / --beta2 must be in [0, 1)"),
                     (["--optimizer", "lamb", "--adam-eps", "-1"], "--adam-eps must be >= 0"),
                     (["--graph", "--lr-schedule", "warmup-cosine"], "--graph cannot follow --lr-schedule")):
        with pytest.raises(SystemExit) as e:
            main(bad)
        assert msg in str(e.value)


def test_opt_extension_builds_next_to_the_pinned_ones(native_ext, monkeypatch):
    import build_native
    from pytorch_distributed_tutorials_amd.ops import _ext
    assert os.path.dirname(build_native.opt_out_path()) == os.path.dirname(build_native.out_path())
    assert os.path.exists(build_native.opt_out_path())
    assert sorted(os.listdir(build_native.BUILD_OPT)) == ["opt_bind_opt.cpp.o", "opt_lamb.hip.o"]
    for d in (build_native.BUILD, build_native.BUILD_MIX, build_native.BUILD_IMG, build_native.BUILD_EMA):
        assert not [f for f in os.listdir(d) if f.startswith("opt_")]
    O = _ext.native_opt()
    assert _ext.native_opt_available() and O.__name__.endswith("._C_opt")
    assert {"lamb_step", "lamb_trust", "set_sync_check", "sync_check_enabled"} <= set(dir(O))
    assert not [n for n in dir(native_ext) if "lamb" in n or "adamw" in n]
    # both entry points honour PDT_DISABLE_NATIVE (the loader caches outcomes: start from an empty cache)
    monkeypatch.setenv("PDT_DISABLE_NATIVE", "1")
    monkeypatch.setattr(_ext, "_MODULES", {})
    assert not _ext.native_opt_available()
    with pytest.raises(RuntimeError, match=r"_C_opt.*PDT_DISABLE_NATIVE"):
        _ext.native_opt()


def test_binding_checks_run_before_any_launch(native_ext):
    from pytorch_distributed_tutorials_amd.ops import _ext
    O = _ext.native_opt()
    n, nseg, nchunks = 64, 2, 2
    big = torch.zeros(n + 4)
    p, g, m, v = (torch.zeros(n) for _ in range(4))
    assert all(t.data_ptr() % 16 == 0 for t in (big, p, g, m, v))
    table = torch.zeros(nseg * 32 + nchunks * 16, dtype=torch.uint8)
    partials, trust = torch.zeros(2 * nchunks, dtype=torch.float64), torch.ones(nseg)
    rec = torch.zeros(int(O.record_elems()), dtype=torch.int64)
    hyper = (0.1, 0.9, 0.999, 1e-6, 0.0, True, True)

    def call(p=p, g=g, m=m, v=v, table=table, partials=partials, trust=trust, rec=rec, lo=0, hi=nseg, hyper=hyper,
             pb=None):
        O.lamb_step(p, g, m, v, table, partials, trust, rec, lo, hi, *hyper, pb)

    with pytest.raises(RuntimeError, match="must be a GPU tensor"):  # everything else is in order
        call()
    for kw, msg in ((dict(g=g.double()), "must be fp32"), (dict(m=m[:-1]), "length mismatch"),
                    (dict(v=torch.zeros(2 * n)[::2]), "must be contiguous"),
                    (dict(pb=torch.zeros(n - 1, dtype=torch.bfloat16)), "bf16 mirror must match"),
                    (dict(table=table[:-16]), "table size"), (dict(partials=partials.float()), "partials must be"),
                    (dict(rec=rec[:1]), "step record"), (dict(hi=nseg + 1), "segment range"),
                    (dict(lo=1, hi=1), "segment range"), (dict(hyper=(0.1, 1.0) + hyper[2:]), "betas must be"),
                    (dict(p=big[1:n + 1]), "16-byte aligned")):
        with pytest.raises(RuntimeError, match=msg):
            call(**kw)
    assert not p.any() and not m.any() and not v.any() and not rec.any()


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("trust", [True, False], ids=["lamb", "adamw"])
def test_fp32_reference_stays_within_the_gpu_tests_bounds(trust, wd):
    flat = lg.build_flat()
    for (p, m, v, r), (rp, rm, rv, rr) in zip(lg.run_reference(flat, torch.float32, trust, wd),
                                              lg.run_reference(flat, torch.float64, trust, wd)):
        assert (p.double() - rp).abs().max().item() <= lg.P_ABS
        assert lg.seg_rel(flat, m, rm) <= lg.M_REL and lg.seg_rel(flat, v, rv) <= lg.V_REL
        assert lg.ulps(r, rr) <= lg.RATIO_ULPS
