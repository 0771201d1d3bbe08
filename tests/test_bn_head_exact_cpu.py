"""The exact BN / pool / fold / head harness (tests/exact_bn.py) checked without a GPU, and why it exists.

* its fp64 references equal ``torch.nn.functional`` (batch_norm autograd, max_pool2d with indices,
  linear, adaptive_avg_pool2d) in fp64, and the fold's algebra equals apply-then-dgrad / apply-then-wgrad;
* its premise checks raise when an operand breaks the exactness argument;
* the crafted backward apply, evaluated in fp32 in several association orders, equals the fp64 result
  bit for bit; with a row count that is no power of two the fp32 evaluation stays inside the neighbour
  rule and far under its 1 % cap;
* the gaps: the whole-tensor metrics of test_kernels_gpu.py ACCEPT a zeroed 8-channel vector of dy, a
  fold dx whose last row lost its bias, and BN sums that dropped one pooled window -- shown on the
  references alone, on that suite's own Gaussian operands -- while the new comparisons reject each.
"""
import pytest
import torch
import torch.nn.functional as F

import exact_bn as eb
import exact_conv as ec


def _close(a, b):
    return torch.allclose(a, b, rtol=1e-11, atol=1e-11)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


# --------------------------------------------------------------------------- reference agreement
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("nhwk", [(2, 4, 8, 16), (3, 5, 7, 8)])
def test_bn_references_match_batch_norm_autograd_fp64(nhwk, res):
    n, h, w, k = nhwk
    M = n * h * w
    _, yd = ec.int_tensor(nhwk, (-4, 4), 1)
    _, rd = ec.int_tensor(nhwk, (-3, 3), 2)
    _, dzd = ec.int_tensor(nhwk, (-3, 3), 3)
    g = torch.Generator().manual_seed(4)
    gamma = (torch.rand(k, generator=g) + 0.5).double().requires_grad_(True)
    beta = torch.randn(k, generator=g).double().requires_grad_(True)
    x = _nchw(yd).clone().requires_grad_(True)
    r = _nchw(rd).clone().requires_grad_(True)
    eps = 1e-5
    out = F.batch_norm(x, None, None, gamma, beta, training=True, eps=eps)
    out = F.relu(out + r if res else out)
    out.backward(_nchw(dzd))
    mu = yd.reshape(M, k).mean(0)
    invstd = (yd.reshape(M, k).var(0, unbiased=False) + eps).rsqrt()
    scale = gamma.detach() * invstd
    shift = beta.detach() - mu * scale
    z = eb.bn_fwd64(yd, scale, shift, rd if res else None, True)
    assert _close(z, _nhwc(out.detach()))
    on1 = eb.mask_on(1, z, yd, scale, shift)
    sums = eb.bwd_sums(dzd, yd, mu, on1)
    c = eb.pack_coefs(mu, invstd, gamma.detach(), sums[0], sums[1], scale, shift, M, exact=False, fp32=False)
    dy, dres = eb.ref_bwd_apply(c, dzd, yd, on1)
    assert _close(dy, _nhwc(x.grad))
    assert _close(c.s1 * c.invstd, gamma.grad) and _close(c.s0, beta.grad)
    if res:
        assert torch.equal(dres, _nhwc(r.grad))
    else:   # no residual: the mask recomputed from y (mode 2) is the mask of z
        assert torch.equal(yd * scale + shift > 0, on1)
    # evaluation mode: dy = k1 g
    dy_e, _ = eb.ref_bwd_apply(c, dzd, yd, on1, training=False)
    assert torch.equal(dy_e, c.k1 * torch.where(on1, dzd, 0.0))
    # the fold's form of the same apply: dy = k1 g + a y + b
    g1 = torch.where(on1, dzd, 0.0)
    assert _close(dy, c.k1 * g1 + c.a * yd + c.b)


def test_forward_reference_rounds_the_normalised_residual_first():
    """The projection-shortcut form: res * res_scale + res_shift is rounded to bf16 before the add."""
    yd = torch.tensor([[[[1.0] * 8]]], dtype=torch.float64)
    resd = torch.full_like(yd, 129.0)
    one, zero = torch.ones(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64)
    # the residual: 129 * 2 + 1 = 259, a tie between the bf16 values 258 and 260 -> 260 (even)
    z = eb.ref_bn_fwd(3 * yd, one, zero, resd, False, 2 * one, one)
    assert torch.equal(z.double(), torch.full_like(yd, 264.0))          # 3 + 260 = 263, a tie -> 264
    assert eb.to_bf16(3 * yd + 259.0).double().unique().item() == 262.0  # one rounding at the end would give 262


@pytest.mark.parametrize("nhwc", [(2, 17, 16, 8), (1, 1, 1, 8), (3, 2, 9, 8), (2, 7, 8, 8)])
def test_maxpool_reference_matches_max_pool2d_with_indices(nhwc):
    n, h, w, c = nhwc
    _, xd = ec.int_tensor(nhwc, (0, 3), 5)            # ties everywhere
    x = _nchw(xd).clone().requires_grad_(True)
    val, ind = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    best, bi = eb.ref_maxpool(xd)
    ho, wo = eb.pool_hw(h, w)
    assert best.shape == (n, ho, wo, c) and torch.equal(best, _nhwc(val.detach()))
    hh = 2 * torch.arange(ho).view(1, ho, 1, 1) - 1 + (bi // 3).long()
    ww = 2 * torch.arange(wo).view(1, 1, wo, 1) - 1 + (bi % 3).long()
    assert torch.equal(hh * w + ww, _nhwc(ind))        # ATen's first-maximum rule
    _, dyd = ec.int_tensor((n, ho, wo, c), (-3, 3), 6)
    val.backward(_nchw(dyd))
    assert torch.equal(eb.ref_maxpool_bwd(dyd, bi, h, w), _nhwc(x.grad))
    assert torch.equal(eb.ref_pool_gather(xd, bi), best)


def test_fused_pool_reference_is_the_composition():
    nhwk = (2, 9, 7, 16)
    _, yd = ec.int_tensor(nhwk, (-4, 4), 7)
    scale, shift = eb.craft_fwd(16, 8)
    out, bi, u = eb.ref_bn_relu_maxpool(yd, scale, shift)
    z = F.relu(_nchw(yd) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)).float().to(torch.bfloat16).double()
    val, ind = F.max_pool2d(z, 3, 2, 1, return_indices=True)
    assert torch.equal(out.double(), _nhwc(val))
    flat = _nchw(yd).reshape(2, 16, -1).gather(2, ind.reshape(2, 16, -1)).reshape(ind.shape)
    assert torch.equal(u.double(), _nhwc(flat))
    assert int((out == 0).sum()) > 0                    # ReLU zeros take part in the ties


def test_head_references_match_linear_and_avg_pool():
    g = torch.Generator().manual_seed(9)
    _, pd = ec.int_tensor((7, 72), (-2, 2), 10, dtype=torch.float32)
    _, wd = ec.int_tensor((33, 72), (-2, 2), 11, dtype=torch.float32)
    _, bd = ec.int_tensor((33,), (-2, 2), 12, dtype=torch.float32)
    _, dld = ec.int_tensor((7, 33), (-2, 2), 13, dtype=torch.float32)
    p, w, b = (t.clone().requires_grad_(True) for t in (pd, wd, bd))
    F.linear(p, w, b).backward(dld)
    logits, dp, dw, db = eb.ref_linear(pd, wd, bd, dld)
    assert torch.equal(logits, F.linear(pd, wd, bd))
    assert torch.equal(dp, p.grad) and torch.equal(dw, w.grad) and torch.equal(db, b.grad)
    _, xd = ec.int_tensor((3, 3, 5, 16), (-4, 4), 14)
    x = _nchw(xd).clone().requires_grad_(True)
    y = F.adaptive_avg_pool2d(x, 1).flatten(1)
    dyd = torch.randn(3, 16, generator=g).double()
    y.backward(dyd)
    sums, hw = eb.ref_avgpool(xd)
    assert hw == 15 and _close(sums / hw, y.detach())
    s, dx = eb.ref_avgpool_bwd(torch.stack([dyd, 2 * dyd, -dyd]), 3, 5)
    assert _close(s, 2 * dyd) and _close(dx, 2 * _nhwc(x.grad))
    assert eb.fc_split_count(3, 10, 2048) == 8 and eb.fc_split_count(64, 64, 1000) == 2
    assert eb.fc_split_count(7, 72, 33) == 1 and eb.fc_split_count(256, 1000, 2048) == 4


def test_fold_references_match_apply_then_dgrad_and_wgrad():
    """[g | x] [wt k1 | G]^T + bias == (k1 g + a y + b) wt^T with y = x wt, and the fold's dW formula ==
    dy^T x, in exact fp64 arithmetic on crafted operands; wfold is the bf16 rounding of those weights."""
    C_, K, M = 32, 256, 64
    c = eb.craft(K, 1024, seed=15)
    _, wtd = ec.int_tensor((C_, K), (-1, 1), 16)
    _, gd = ec.int_tensor((M, K), (-1, 1), 17)
    _, xd = ec.int_tensor((M, C_), (0, 2), 18)
    wfold, bias, G = eb.ref_fold_weights(wtd, c)
    assert torch.equal(wfold[:, :K].double(), wtd * c.k1) and torch.equal(wfold[:, K:], eb.to_bf16(G))
    assert int((wfold[:, K:].double() != G).sum()) > 0       # G itself is no bf16 tensor
    yd = xd @ wtd
    dy = c.k1 * gd + c.a * yd + c.b
    dx = torch.cat([gd, xd], 1) @ torch.cat([wtd * c.k1, G], 1).t() + bias
    assert torch.equal(dx, dy @ wtd.t())
    on = torch.ones(M, C_, dtype=torch.bool)
    got = eb.ref_fold_dgrad(gd, xd, wfold, bias, on)
    assert got.dtype == torch.bfloat16 and got.shape == (M, C_)
    out0 = torch.zeros(K, C_, dtype=torch.float64)
    dw = eb.ref_fold_wgrad(out0, gd.t() @ xd, xd.t() @ xd, xd.sum(0), wtd, c)
    assert torch.equal(dw, dy.t() @ xd)


# ------------------------------------------------------------------------------- premise checks
def _vec(k, v):
    return torch.full((k,), float(v), dtype=torch.float64)


def test_premise_checks_trip():
    k, M = 8, 64
    ok = dict(mu=_vec(k, 1), invstd=_vec(k, 0.5), gamma=_vec(k, -2), s0=_vec(k, 2 * M), s1=_vec(k, M),
              scale=_vec(k, 1), shift=_vec(k, 0.5))
    pack = lambda **kw: eb.pack_coefs(*({**ok, **kw}[n] for n in ("mu", "invstd", "gamma", "s0", "s1", "scale", "shift")),  # noqa: E731
                                      kw.get("M", M))
    c = pack()
    assert c.k2.unique().item() == 0.25 and c.sgm.unique().item() == 2
    with pytest.raises(ec.PremiseError, match="powers of two"):
        pack(invstd=_vec(k, 0.75))
    with pytest.raises(ec.PremiseError, match="multiple of M"):
        pack(s0=_vec(k, 2 * M + 1))
    with pytest.raises(ec.PremiseError, match="power of two or zero"):
        pack(s1=_vec(k, 3 * M))
    with pytest.raises(ec.PremiseError, match="not a power of two"):
        pack(M=105, s0=_vec(k, 105))
    with pytest.raises(ec.PremiseError, match="not exact in fp32"):
        pack(mu=_vec(k, 1 + 2.0 ** -30))
    # operands too large: |dy| x denominators reaches 2^24
    big = torch.full((1, 1, 1, k), 2.0 ** 23, dtype=torch.float64)
    on = torch.ones_like(big, dtype=torch.bool)
    with pytest.raises(ec.PremiseError, match="denominators"):
        eb.exact_bwd_apply(c, big, torch.zeros_like(big), on)
    with pytest.raises(ec.PremiseError, match="crafted"):
        eb.exact_bwd_apply(eb.generic(k, 105), torch.zeros_like(big), torch.zeros_like(big), on)
    with pytest.raises(ec.PremiseError, match="not exact in fp32"):
        eb.ref_bn_fwd(big + 1, _vec(k, 1), _vec(k, 0.5))                   # 2^23 + 1.5 is no fp32 value
    with pytest.raises(ec.PremiseError):
        eb.ref_bwd_reduce(big.expand(4, 1, 1, k), torch.ones(4, 1, 1, k, dtype=torch.float64), _vec(k, 0),
                          on.expand(4, 1, 1, k))                           # sum |g| = 2^25
    with pytest.raises(ec.PremiseError, match="wt"):
        eb.ref_fold_weights(torch.full((32, 256), 2.0, dtype=torch.float64), eb.craft(256, 1024))
    with pytest.raises(ec.PremiseError):
        eb.ref_linear(torch.full((1, 8), 0.5, dtype=torch.float64), torch.ones(1, 8, dtype=torch.float64),
                      torch.zeros(1, dtype=torch.float64), torch.ones(1, 1, dtype=torch.float64))
    assert eb.lattice_unit(torch.tensor([0.75, -3.0], dtype=torch.float64)) == 0.25
    with pytest.raises(ec.PremiseError):
        eb.lattice_unit(torch.tensor([1 / 3], dtype=torch.float64))


# ------------------------------------------------------------------------------ exact evaluation
@pytest.mark.parametrize("nhwk", [(2, 4, 8, 64), (1, 2, 2, 40), (4, 8, 8, 128)])
def test_crafted_apply_is_association_order_invariant_in_fp32(nhwk):
    n, h, w, k = nhwk
    c = eb.craft(k, n * h * w, seed=20)
    _, gd = ec.int_tensor(nhwk, (-200, 200), 21)
    _, yd = ec.int_tensor(nhwk, (-20, 20), 22)
    on = eb.mask_on(2, None, yd, c.scale, c.shift)
    assert yd.numel() < 1000 or 0 < int((yd * c.scale + c.shift == 0).sum())     # exact zeros: the mask is off there
    want, _ = eb.exact_bwd_apply(c, gd, yd, on)
    g, y = torch.where(on, gd, 0.0).float(), yd.float()
    mu, is_, gm, s0, s1 = c.stats[0], c.stats[1], c.gamma, c.sums[0], c.sums[1]
    invM = torch.tensor(1.0 / c.M, dtype=torch.float32)
    k1, sgm, k2 = gm * is_, s0 * invM, s1 * is_ * is_ * invM
    forms = [k1 * (g - sgm - (y - mu) * k2),                 # the kernel's
             k1 * g - (k1 * sgm + (k1 * k2) * y - (k1 * k2) * mu),
             (g - (sgm + k2 * y - k2 * mu)) * is_ * gm,
             k1 * g + (-k1 * k2) * y + (-k1 * (sgm - mu * k2))]   # the fold's a, b
    for f in forms:
        assert f.dtype == torch.float32 and torch.equal(f.double(), want)
    stored = eb.to_bf16(want)
    assert int((stored.double() != want).sum()) > 0          # the bf16 store does round (ties included)


def test_bf16_neighbours():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -9, -1.0 - 2.0 ** -9, 0.0, 2.0 ** -140, -3.0, 257.0], dtype=torch.float64)
    lo, hi = eb.bf16_down(x).double(), eb.bf16_up(x).double()
    assert torch.equal(lo, torch.tensor([1.0, 1.0, -1.0 - 2.0 ** -7, 0.0, 0.0, -3.0, 256.0], dtype=torch.float64))
    assert torch.equal(hi, torch.tensor([1.0, 1.0 + 2.0 ** -7, -1.0, 0.0, 2.0 ** -133, -3.0, 258.0], dtype=torch.float64))
    ref = torch.tensor([[1.0 + 2.0 ** -9] * 8], dtype=torch.float64)
    zero = torch.zeros_like(ref)
    eb.assert_bf16_neighbour(eb.to_bf16(ref), ref, zero)
    with pytest.raises(AssertionError, match="differ from the rounded reference"):
        eb.assert_bf16_neighbour(eb.bf16_up(ref), ref, zero)            # inside, but every element off
    with pytest.raises(AssertionError, match="outside their bf16 neighbours"):
        eb.assert_bf16_neighbour(eb.to_bf16(ref + 2.0 ** -6), ref, zero)


@pytest.mark.parametrize("nhwk", [(3, 5, 7, 64), (2, 3, 5, 40), (3, 17, 15, 64)])
def test_fp32_apply_stays_within_the_neighbour_rule(nhwk):
    """M = 105, 30, 765: 1 / M is rounded.  A plain fp32 evaluation of the kernel's formula (and of a second
    association) stays inside [bf16_down(ref - slack), bf16_up(ref + slack)], and the share of elements off
    the rounded reference is far below the 1 % cap (about 2^-12 expected: the chance that an fp32-sized
    error straddles a bf16 rounding boundary)."""
    n, h, w, k = nhwk
    c = eb.generic(k, n * h * w, seed=30)
    _, gd = ec.int_tensor(nhwk, (-3, 3), 31)
    _, yd = ec.int_tensor(nhwk, (-4, 4), 32)
    on = eb.mask_on(2, None, yd, c.scale, c.shift)
    want, _ = eb.ref_bwd_apply(c, gd, yd, on)
    slack = eb.bwd_apply_slack(c, gd, yd, on)
    g, y = torch.where(on, gd, 0.0).float(), yd.float()
    mu, is_, gm, s0, s1 = c.stats[0], c.stats[1], c.gamma, c.sums[0], c.sums[1]
    invM = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(c.M), dtype=torch.float32)
    k1, sgm, k2 = gm * is_, s0 * invM, s1 * is_ * is_ * invM
    for f in (k1 * (g - sgm - (y - mu) * k2), k1 * g - k1 * sgm - (k1 * k2) * (y - mu)):
        got = f.to(torch.bfloat16)
        outside, share = eb.neighbour_report(got, want, slack)
        print(f"{nhwk}: outside {outside}, share off the rounded reference {share:.3e}")
        eb.assert_bf16_neighbour(got, want, slack, f"fp32 apply {nhwk}")
        assert share <= 0.1 * eb.NEIGHBOUR_CAP


# ---------------------------------------------------------------------------- gap demonstrations
def _rel_err(a, b):
    """The metric of test_kernels_gpu.py (asserted ``< 1e-2`` there)."""
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def test_gap_zeroed_dy_vector_passes_the_norm_ratio():
    """test_bn_act_fwd_bwd at (8,14,14,512), its own kind of operands: one zeroed 8-channel vector of dy is a
    norm ratio of about sqrt(8 / 802816) = 0.003 < 1e-2; the element-wise comparisons reject it."""
    nhwk = (8, 14, 14, 512)
    n, h, w, k = nhwk
    M = n * h * w
    g = torch.Generator().manual_seed(11)
    y = torch.randn(nhwk, generator=g).to(torch.bfloat16).double()
    dz = torch.randn(nhwk, generator=g).to(torch.bfloat16).double()
    gamma = (torch.rand(k, generator=g) + 0.5).float().double()
    mu = y.reshape(M, k).mean(0).float().double()
    invstd = (y.reshape(M, k).var(0, unbiased=False) + 1e-5).rsqrt().float().double()
    on = torch.ones(nhwk, dtype=torch.bool)
    sums = eb.bwd_sums(dz, y, mu, on).float().double()
    c = eb.pack_coefs(mu, invstd, gamma, sums[0], sums[1], gamma * 0 + 1, gamma * 0, M, exact=False)
    want, _ = eb.ref_bwd_apply(c, dz, y, on)
    slack = eb.bwd_apply_slack(c, dz, y, on)
    good = eb.to_bf16(want)
    bad = good.clone().reshape(-1, 8)
    v = int((want.reshape(-1, 8).abs().min(1).values).argmax())     # a vector with no element near 0
    bad[v] = 0
    bad = bad.reshape(nhwk)
    err = _rel_err(bad, good)
    print(f"norm ratio of one zeroed vector: {err:.2e}")
    assert 0 < err < 1e-2                                            # the old metric accepts it
    eb.assert_bf16_neighbour(good, want, slack, "unchanged")
    with pytest.raises(AssertionError, match="8 of 802816 elements outside"):
        eb.assert_bf16_neighbour(bad, want, slack, "zeroed vector")
    with pytest.raises(AssertionError, match="8 of 802816 elements differ") as e:
        ec.assert_exact(bad, good, None, None, None, "zeroed vector")
    assert "wrong rows: 1, wrong columns: 8" in str(e.value)


def test_gap_fold_dx_row_without_bias_passes_the_norm_ratio():
    """test_folded_bn_backward_dgrad_matches_apply_then_dgrad at (4,14,14,64,256), its kind of operands:
    M = 784 = 12 x 64 + 16 rows end in a ragged tile.  A kernel that added the bias to "rows < M - 1" --
    the last valid row, next to the tile's padding rows, left out -- stays under the 1e-2 norm ratio."""
    n, h, w, c_, k = 4, 14, 14, 64, 256
    M = n * h * w
    g_ = torch.Generator().manual_seed(21)
    x = torch.relu(torch.randn(M, c_, generator=g_)).to(torch.bfloat16).double()
    wt = (torch.randn(c_, k, generator=g_) / c_ ** 0.5).to(torch.bfloat16).double()
    y = eb.to_bf16(x @ wt).double()
    gamma = (1 + 0.2 * torch.randn(k, generator=g_)).float().double()
    mu = y.mean(0).float().double()
    invstd = (y.var(0, unbiased=False) + 1e-5).rsqrt().float().double()
    gd = (torch.randn(M, k, generator=g_) * (torch.rand(M, k, generator=g_) > 0.4)).to(torch.bfloat16).double()
    on_k = torch.ones(M, k, dtype=torch.bool)
    sums = eb.bwd_sums(gd, y, mu, on_k).float().double()
    c = eb.pack_coefs(mu, invstd, gamma, sums[0], sums[1], gamma * 0 + 1, gamma * 0, M, exact=False)
    wfold = torch.cat([eb.to_bf16(wt * c.k1), eb.to_bf16((wt * c.a) @ wt.t())], 1).double()
    bias = wt @ c.b
    dx = torch.cat([gd, x], 1) @ wfold.t() + bias
    bad = dx.clone()
    bad[M - 1] -= bias
    assert M % 64 and float(bias.abs().min()) > 0
    err = _rel_err(eb.to_bf16(bad), dx)
    print(f"norm ratio of a last row without its bias: {err:.2e}")
    assert 0 < err < 1e-2                                            # the old metric accepts it
    with pytest.raises(AssertionError, match="wrong rows: 1,") as e:
        ec.assert_exact(eb.to_bf16(bad), eb.to_bf16(dx), 64, 64, None, "last row without bias")
    assert "by row tile: {12:" in str(e.value)                       # the message names the ragged tile


def test_gap_dropped_pool_window_passes_the_sum_tolerance():
    """test_bn_relu_maxpool_matches_unfused at (4,17,16,64), its kind of operands: pool_bn_bwd_reduce sums
    that drop one pooled window's contribution.  ``allclose(rtol=2e-2, atol=0.5)`` accepts the drop in
    every channel where |dpool| (and |dpool (y - mu)|) is below the tolerance -- about half of the window's
    64 channels, so the demonstration drops the window in those channels (in all 64 the old
    metric would catch it through the larger ones) -- while sums of integers must be equal."""
    nhwk = (4, 17, 16, 64)
    n, h, w, k = nhwk
    g = torch.Generator().manual_seed(21)
    y = torch.randn(nhwk, generator=g).to(torch.bfloat16).double()
    scale = (torch.rand(k, generator=g) + 0.5).float().double()
    shift = (0.2 * torch.randn(k, generator=g)).float().double()
    mu = y.reshape(-1, k).mean(0).float().double()
    z = eb.to_bf16(eb.bn_fwd64(y, scale, shift)).double()
    _, bi = eb.ref_maxpool(z)
    ho, wo = eb.pool_hw(h, w)
    dpool = torch.randn(n, ho, wo, k, generator=g).to(torch.bfloat16).double()
    on = y * scale + shift > 0
    full = eb.bwd_sums(eb.ref_maxpool_bwd(dpool, bi, h, w), y, mu, on)
    win = (1, 3, 4)
    dropped = dpool.clone()
    dropped[win] = 0
    part = eb.bwd_sums(eb.ref_maxpool_bwd(dropped, bi, h, w), y, mu, on)
    diff = (part - full).abs()
    tol = 0.5 + 2e-2 * full.abs()
    ok = ((diff <= tol).all(0)) & (diff[0] > 0)                      # channels where the old metric accepts the drop
    print(f"channels where the dropped window passes allclose: {int(ok.sum())} of {k}; max |diff| {diff.max():.3f}")
    assert int(ok.sum()) >= 8
    assert not torch.allclose(part.float(), full.float(), rtol=2e-2, atol=0.5)   # all 64 channels: caught
    mixed = torch.where(ok, part, full)                              # the nearest corruption that is accepted
    assert torch.allclose(mixed.float(), full.float(), rtol=2e-2, atol=0.5)
    assert not torch.equal(mixed, full)
    # the same drop on integer operands: the exact comparison names the channels
    _, yi = ec.int_tensor(nhwk, (-4, 4), 41)
    _, dpi = ec.int_tensor((n, ho, wo, k), (1, 3), 42)
    sc, sh = eb.craft_fwd(k, 43)
    mui = ec.int_tensor((k,), (-2, 2), 44, dtype=torch.float32)[1]
    _, bii = eb.ref_maxpool(eb.ref_bn_fwd(yi, sc, sh).double())
    oni = eb.mask_on(2, None, yi, sc, sh)
    want = eb.ref_bwd_reduce(eb.ref_maxpool_bwd(dpi, bii, h, w), yi, mui, oni)
    dpi2 = dpi.clone()
    dpi2[win] = 0
    got = eb.ref_bwd_reduce(eb.ref_maxpool_bwd(dpi2, bii, h, w), yi, mui, oni)
    hit = int((got[0] != want[0]).sum())
    assert hit > 0
    with pytest.raises(AssertionError, match="elements differ"):
        ec.assert_exact(got.float(), want.float(), None, None, None, "dropped window")
