"""Crafted coefficients, fp64 references and comparisons for the BatchNorm, pooling, folded-BN and head
kernels (the companion of tests/exact_conv.py, whose integer-operand argument carries over).

The BN backward apply computes, per channel,

    k1 = gamma * invstd,  sgm = s0 * (1 / M),  k2 = s1 * invstd * invstd * (1 / M),
    dy = k1 * (g - sgm - (y - mu) * k2)

and the fold a = -k1 * k2, b = -k1 * (s0 / M - mu * k2).  ``craft`` chooses mu as small integers, invstd
and gamma as powers of two (mixed exponents, gamma of either sign), s0 = M * (small integer), s1 so that
k2 is a power of two or zero, and M a power of two.  Every intermediate is then a small multiple of a
power of two -- exactly representable in fp32 whatever the association or FMA contraction -- and with
integer g and y the result has ONE right answer; its bf16 rounding (ties included) is the same on both
sides.  ``pack_coefs`` asserts those premises.  The forward scale is a power of two and the shift an
integer or half-integer, so y * scale + shift lands on bf16 rounding ties and on exactly 0.

Where M is no power of two, 1 / M is rounded and the result is not exact: ``assert_bf16_neighbour``
then allows every element the bf16 values around ``ref +- slack`` with the DERIVED slack of
``bwd_apply_slack`` (five fp32 roundings), and at most 1 % of elements off the rounded reference.

This module is a helper, not a test file.  Every reference is plain fp64 torch (no fp32 BLAS).
Activations are NHWC; per-channel vectors broadcast over the last axis.
"""
from types import SimpleNamespace

import torch

import exact_conv as ec
from exact_conv import PremiseError, to_bf16

NEIGHBOUR_CAP = 0.01   # share of elements that may differ from to_bf16(ref) under the neighbour rule


# ------------------------------------------------------------------ lattices
def lattice_unit(*tensors):
    """The largest power of two u <= 1 of which every element of every tensor (fp64) is a multiple."""
    for e in range(0, 41):
        u = 2.0 ** -e
        if all(torch.equal((t / u).round(), t / u) for t in tensors):
            return u
    raise PremiseError("values are on no power-of-two lattice down to 2^-40")


def require_lattice_sum(mag, unit, what):
    """Sums of terms that are multiples of ``unit`` are exact in fp32, in any order, while the sum of
    magnitudes stays below 2^24 units."""
    ec.require_below(mag / unit, ec.EXACT_LIMIT, f"{what} (in units of {unit:g})")


def require_fp32(t, what):
    if not torch.equal(t.float().double(), t):
        raise PremiseError(f"{what}: not exact in fp32")


def _is_pow2(t):
    m, _ = torch.frexp(t.abs())
    return bool(((m == 0.5) & (t != 0)).all())


# -------------------------------------------------------------- coefficients
def pack_coefs(mu, invstd, gamma, s0, s1, scale, shift, M, exact=True, fp32=True):
    """Per-channel fp64 vectors -> the kernels' operands (stats [4,K] = mean, invstd, scale, shift; gamma
    [K]; sums [2,K] = s0, s1; all fp32) plus the fp64 coefficients k1, k2, sgm, a, b.  Every operand must
    survive the round trip through fp32 (``fp32=False``: a pure fp64 evaluation, no kernel operands);
    ``exact`` also asserts the crafted-coefficient premises."""
    o = SimpleNamespace(M=int(M), K=mu.numel(), exact=exact, mu=mu, invstd=invstd, gammad=gamma, s0=s0, s1=s1,
                        scale=scale, shift=shift)
    for name in ("mu", "invstd", "gammad", "s0", "s1", "scale", "shift") if fp32 or exact else ():
        require_fp32(getattr(o, name), name)
    o.k1 = gamma * invstd
    o.sgm = s0 / M
    o.k2 = s1 * invstd * invstd / M
    o.a = -o.k1 * o.k2
    o.b = -o.k1 * (o.sgm - mu * o.k2)
    if exact:
        if M & (M - 1):
            raise PremiseError(f"M = {M} is not a power of two")
        if not _is_pow2(invstd) or not _is_pow2(gamma):
            raise PremiseError("invstd and gamma must be powers of two")
        if not torch.equal(mu, mu.round()):
            raise PremiseError("mu must be integers")
        if not torch.equal(o.sgm, o.sgm.round()):
            raise PremiseError("s0 must be a multiple of M")
        if not _is_pow2(torch.where(o.k2 == 0, torch.ones_like(o.k2), o.k2)):
            raise PremiseError("k2 = s1 * invstd^2 / M must be a power of two or zero")
        for name in ("k1", "sgm", "k2", "a", "b"):
            require_fp32(getattr(o, name), name)
    o.stats = torch.stack([mu, invstd, scale, shift]).float().contiguous()
    o.gamma = gamma.float().contiguous()
    o.sums = torch.stack([s0, s1]).float().contiguous()
    return o


def _pick(g, values, k):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), (k,), generator=g)]


def craft_fwd(K, seed=0, device="cpu"):
    """(scale, shift) fp64 of a forward apply.  Scale: powers of two 2^-3 .. 2 of either sign.  Shift:
    integers and half-integers -- in [-2, 2] on about half of the channels, where small integer y reach
    y * scale + shift == 0 exactly, and offset by +96 or -160 on the others, where the sum needs more than
    bf16's 8 bits and the store rounds (ties included; under a ReLU the -160 channels are all ties at 0)."""
    g = torch.Generator().manual_seed(seed)
    scale = _pick(g, [0.125, 0.25, 0.5, 1.0, 2.0, -0.5, -1.0], K)
    shift = torch.randint(-4, 5, (K,), generator=g).double() / 2 + _pick(g, [0.0, 0.0, 96.0, -160.0], K)
    return scale.to(device), shift.to(device)


def craft(K, M, seed=0, device="cpu"):
    """Crafted coefficients of one BatchNorm over M rows (module docstring): exact in every order."""
    g = torch.Generator().manual_seed(seed)
    mu = torch.randint(-2, 3, (K,), generator=g).double()
    invstd = _pick(g, [0.5, 1.0, 2.0], K)
    gamma = _pick(g, [0.5, 1.0, 2.0, -0.5, -1.0, -2.0], K)
    s0 = M * torch.randint(-2, 3, (K,), generator=g).double()
    k2 = _pick(g, [0.0, 0.25, -0.25, 0.5, -0.5], K)    # some a = 0, mixed signs
    s1 = k2 * M / (invstd * invstd)
    scale, shift = craft_fwd(K, seed + 1000)
    return pack_coefs(*(t.to(device) for t in (mu, invstd, gamma, s0, s1, scale, shift)), M)


def generic(K, M, seed=0, device="cpu"):
    """Ordinary real coefficients (as fp32 values) for a row count that is no power of two: the backward
    apply is then judged by the neighbour rule.  Scale and shift stay crafted: the ReLU mask is exact."""
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(K, generator=g)   # noqa: E731
    mu = (0.5 * r()).float().double()
    invstd = (0.5 + 1.5 * torch.rand(K, generator=g)).float().double()
    gamma = ((0.5 + torch.rand(K, generator=g)) * (2 * torch.randint(0, 2, (K,), generator=g) - 1)).float().double()
    s0 = (r() * M ** 0.5).float().double()
    s1 = (r() * M ** 0.5).float().double()
    scale, shift = craft_fwd(K, seed + 1000)
    return pack_coefs(*(t.to(device) for t in (mu, invstd, gamma, s0, s1, scale, shift)), M, exact=False)


# ---------------------------------------------------------------- BN forward
def bitmask(on):
    """The ReLU mask bytes of [..., K] booleans: bit j of byte v = element 8 v + j."""
    bits = on.reshape(-1, 8).to(torch.int32) << torch.arange(8, device=on.device, dtype=torch.int32)
    return bits.sum(1).to(torch.uint8)


def bn_fwd64(yd, scale, shift, resd=None, relu=True, rscale=None, rshift=None, check=False):
    """[relu](y * scale + shift [+ residual]) in fp64, before the store rounds it; with rscale / rshift
    the residual is a raw conv output with its own BatchNorm, rounded to bf16 BEFORE the add as the kernel
    does.  ``check``: every fp32 intermediate must be exact."""
    t = yd * scale + shift
    if check:
        require_fp32(t, "y * scale + shift")
    if resd is not None:
        r = resd
        if rscale is not None:
            r = resd * rscale + rshift
            if check:
                require_fp32(r, "res * res_scale + res_shift")
            r = to_bf16(r).double()
        t = t + r
        if check:
            require_fp32(t, "y * scale + shift + residual")
    return t.clamp_min(0.0) if relu else t


def ref_bn_fwd(yd, scale, shift, resd=None, relu=True, rscale=None, rshift=None):
    """z (bf16) of the forward apply: bn_fwd64 with every fp32 intermediate exact (asserted), so the one
    bf16 rounding of the store decides the result."""
    return to_bf16(bn_fwd64(yd, scale, shift, resd, relu, rscale, rshift, check=True))


def ref_csum(z):
    """Exact per-channel sums of the STORED z (bf16) with the premise of an any-order fp32 sum."""
    zd = z.double().reshape(-1, z.shape[-1])
    require_lattice_sum(zd.abs().sum(0), lattice_unit(zd), "column sums of z")
    return zd.sum(0)


# --------------------------------------------------------------- BN backward
def mask_on(mode, zd, yd, scale, shift):
    """Where the ReLU passes the gradient: 0 everywhere, 1 where the saved z > 0, 2 recomputed from y."""
    if mode == 0:
        return torch.ones_like(yd, dtype=torch.bool)
    if mode == 1:
        return zd > 0
    pre = yd * scale + shift
    require_fp32(pre, "y * scale + shift (mask mode 2)")
    return pre > 0


def bwd_sums(dzd, yd, mu, on):
    """sums [2, K] fp64: s0 = sum g, s1 = sum g * (y - mu) with g = where(on, dz, 0)."""
    k = yd.shape[-1]
    g = torch.where(on, dzd, 0.0).reshape(-1, k)
    return torch.stack([g.sum(0), (g * (yd - mu).reshape(-1, k)).sum(0)])


def ref_bwd_reduce(dzd, yd, mu, on):
    """bwd_sums of integer operands with the premise of the exact fp32 sums asserted."""
    k = yd.shape[-1]
    g = torch.where(on, dzd, 0.0).reshape(-1, k)
    yc = (yd - mu).reshape(-1, k)
    ec.require_integers(g, torch.bfloat16, "dz")
    ec.require_integers(yc, torch.float32, "y - mu")
    ec.require_below(g.abs().sum(0), ec.EXACT_LIMIT, "sum |g|")
    ec.require_below((g.abs() * yc.abs()).sum(0), ec.EXACT_LIMIT, "sum |g||y - mu|")
    return bwd_sums(dzd, yd, mu, on)


def ref_sinks(c, dg0, db0):
    """dgamma / dbeta sinks after a backward pass: sink + s1 * invstd, sink + s0 (premise: exact fp32)."""
    dg, db = dg0 + c.s1 * c.invstd, db0 + c.s0
    require_fp32(dg, "dgamma sink")
    require_fp32(db, "dbeta sink")
    return dg.float(), db.float()


def ref_bwd_apply(c, gd, yd, on, training=True):
    """(dy fp64, dres fp64) of the BN backward apply with coefficients ``c``: g = where(on, dz, 0),
    dy = k1 * (g - sgm - (y - mu) * k2) in training mode, k1 * g in evaluation mode; dres = g."""
    g = torch.where(on, gd, 0.0)
    if not training:
        return c.k1 * g, g
    return c.k1 * (g - c.sgm - (yd - c.mu) * c.k2), g


def bwd_apply_mag(c, gd, yd, on):
    """|k1| (|g| + |sgm| + |y - mu||k2|): the magnitude every rounding of the apply is relative to."""
    g = torch.where(on, gd, 0.0)
    return c.k1.abs() * (g.abs() + c.sgm.abs() + (yd - c.mu).abs() * c.k2.abs())


def exact_bwd_apply(c, gd, yd, on, training=True):
    """ref_bwd_apply with the premises of bit exactness: crafted coefficients, integer operands, and
    |dy| times the coefficient denominators below 2^24."""
    if not c.exact:
        raise PremiseError("exact_bwd_apply needs crafted coefficients (a power-of-two M)")
    ec.require_integers(gd, torch.bfloat16, "dz")
    ec.require_integers(yd, torch.bfloat16, "y")
    k2u = torch.where(c.k2 == 0, torch.ones_like(c.k2), c.k2.abs()).clamp_max(1.0)
    require_lattice_sum(bwd_apply_mag(c, gd, yd, on) / (c.k1.abs() * k2u), 1.0, "|dy| x coefficient denominators")
    return ref_bwd_apply(c, gd, yd, on, training)


def bwd_apply_slack(c, gd, yd, on):
    """2^-21 |k1| (|g| + |sgm| + |y - mu||k2|) in fp64.  Derived, not measured: 1/M, sgm, k2 (two
    products and the 1/M factor), the product with y - mu, and the two differences and the final product
    carry at most five fp32 roundings on any one path, each at most 2^-24 of a magnitude bounded by that
    sum; 2^-21 = 8 x 2^-24 covers them with their second-order terms."""
    return 2.0 ** -21 * bwd_apply_mag(c, gd, yd, on)


# ------------------------------------------------------------ neighbour rule
def _bf16_step(b, up):
    """The next bf16 value above (up) or below a bf16 tensor's values."""
    bits = b.float().view(torch.int32)
    one = torch.full_like(bits, 0x10000)
    pos, neg, zero = b > 0, b < 0, b == 0
    away = (bits + one).view(torch.float32)
    toward = (bits - one).view(torch.float32)
    tiny = torch.full_like(away, 2.0 ** -133)   # the smallest bf16 subnormal
    if up:
        out = torch.where(pos, away, torch.where(neg, toward, tiny))
    else:
        out = torch.where(pos, toward, torch.where(neg, away, -tiny))
    return torch.where(zero | pos | neg, out, b.float()).to(torch.bfloat16)


def bf16_down(x):
    """The largest bf16 value <= x (fp64)."""
    b = to_bf16(x)
    return torch.where(b.double() > x, _bf16_step(b, False), b)


def bf16_up(x):
    """The smallest bf16 value >= x (fp64)."""
    b = to_bf16(x)
    return torch.where(b.double() < x, _bf16_step(b, True), b)


def neighbour_report(got, ref64, slack64):
    """(elements outside [bf16_down(ref - slack), bf16_up(ref + slack)], share differing from to_bf16(ref))."""
    lo, hi = bf16_down(ref64 - slack64).double(), bf16_up(ref64 + slack64).double()
    gd = got.double()
    outside = int(((gd < lo) | (gd > hi) | gd.isnan()).sum())
    share = float((got != to_bf16(ref64)).double().mean()) if got.numel() else 0.0
    return outside, share


def assert_bf16_neighbour(got, ref64, slack64, what=""):
    """Every element of ``got`` (bf16) lies in [bf16_down(ref - slack), bf16_up(ref + slack)], and at most
    NEIGHBOUR_CAP of them differ from to_bf16(ref)."""
    assert got.dtype == torch.bfloat16 and got.shape == ref64.shape, f"{what}: {got.dtype} {tuple(got.shape)}"
    outside, share = neighbour_report(got, ref64, slack64)
    if outside:
        lo, hi = bf16_down(ref64 - slack64).double(), bf16_up(ref64 + slack64).double()
        bad = ((got.double() < lo) | (got.double() > hi) | got.isnan()).reshape(-1, got.shape[-1])
        rows, cols = bad.nonzero(as_tuple=True)
        g2, r2 = got.reshape(bad.shape), ref64.reshape(bad.shape)
        first = [(int(r), int(c_), float(g2[r, c_]), float(r2[r, c_])) for r, c_ in zip(rows[:8], cols[:8])]
        raise AssertionError(f"{what}: {outside} of {bad.numel()} elements outside their bf16 neighbours; "
                             f"first (row, col, got, ref): {first}")
    assert share <= NEIGHBOUR_CAP, f"{what}: {share:.4%} of elements differ from the rounded reference (cap 1 %)"


# ------------------------------------------------------------------ max pool
def pool_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def _taps(xd, fill):
    """The 9 taps of every 3x3 / s2 / p1 window of NHWC xd, row-major: [9, N, Ho, Wo, C]."""
    n, h, w, c = xd.shape
    ho, wo = pool_hw(h, w)
    xp = torch.full((n, h + 2, w + 2, c), fill, dtype=xd.dtype, device=xd.device)
    xp[:, 1:h + 1, 1:w + 1] = xd
    return torch.stack([xp[:, kh:kh + 2 * ho:2, kw:kw + 2 * wo:2] for kh in range(3) for kw in range(3)])


def ref_maxpool(xd):
    """(values fp64, argmax uint8 0..8) of the 3x3 / s2 / p1 max pool with the FIRST maximum in row-major
    window order winning a tie (a later tap replaces the best only when strictly greater)."""
    taps = _taps(xd, float("-inf"))
    best, bi = taps[0], torch.zeros(taps[0].shape, dtype=torch.uint8, device=xd.device)
    for t in range(1, 9):
        upd = taps[t] > best
        best = torch.where(upd, taps[t], best)
        bi = torch.where(upd, torch.full_like(bi, t), bi)
    return best, bi


def ref_pool_gather(vd, bi):
    """The value of vd [N,H,W,C] at each window's argmax: [N,Ho,Wo,C]."""
    taps = _taps(vd, 0.0)
    out = torch.zeros_like(taps[0])
    for t in range(9):
        out = torch.where(bi == t, taps[t], out)
    return out


def ref_maxpool_bwd(dyd, bi, h, w):
    """dx [N,H,W,C] fp64: every window's gradient goes to its argmax pixel, overlaps summed."""
    n, ho, wo, c = dyd.shape
    dxp = torch.zeros(n, h + 2, w + 2, c, dtype=dyd.dtype, device=dyd.device)
    for t in range(9):
        kh, kw = divmod(t, 3)
        dxp[:, kh:kh + 2 * ho:2, kw:kw + 2 * wo:2] += torch.where(bi == t, dyd, 0.0)
    return dxp[:, 1:h + 1, 1:w + 1].contiguous()


def ref_bn_relu_maxpool(yd, scale, shift):
    """The fused stem composition: (out bf16, argmax uint8, u = y at the argmax as bf16)."""
    z = ref_bn_fwd(yd, scale, shift, relu=True).double()
    out, bi = ref_maxpool(z)
    return out.to(torch.bfloat16), bi, ref_pool_gather(yd, bi).to(torch.bfloat16)


# ---------------------------------------------------------------------- fold
def ref_fold_weights(wtd, c):
    """(wfold bf16 [C, K + C] = [bf16(wt k1) | bf16(G)], bias fp64 [C], G fp64) for transposed weights wt
    [C, K]: G = (wt a) wt^T, bias = wt b.  wt k1 and wt a must be bf16 values (integer weights, power-of-two
    coefficients) and the sums exact in fp32: G is then ONE rounding of an exact fp32 sum."""
    ec.require_integers(wtd, torch.bfloat16, "wt", 1)
    wk, wa = wtd * c.k1, wtd * c.a
    for t, name in ((wk, "wt k1"), (wa, "wt a")):
        if not torch.equal(to_bf16(t).double(), t):
            raise PremiseError(f"{name}: not exact in bf16")
    u = lattice_unit(c.a, c.b)
    require_lattice_sum(wa.abs() @ wtd.abs().t(), u, "G: sum |a||w||w'|")
    require_lattice_sum(wtd.abs() @ c.b.abs(), u, "bias: sum |w||b|")
    G = wa @ wtd.t()
    return torch.cat([to_bf16(wk), to_bf16(G)], 1).contiguous(), wtd @ c.b, G


def ref_fold_dgrad(gd, xd, wfold, biasd, on):
    """dx = where(on, [g | x] wfold^T + bias, 0) as bf16 [M, C] from the bf16 wfold the kernel reads; the
    products are multiples of one power of two and their fp32 sum is exact (asserted)."""
    wf = wfold.double()
    cat = torch.cat([gd, xd], 1)
    u = lattice_unit(wf, biasd)
    require_lattice_sum(cat.abs() @ wf.abs().t() + biasd.abs(), u, "fold dgrad: sum |operand||wfold| + |bias|")
    return to_bf16(torch.where(on, cat @ wf.t() + biasd, 0.0))


def ref_bn_sums(gstored, yd, mu):
    """(sum g, sum g (y - mu)) [2, C] of a stored bf16 g [M, C] as a BN-fused dgrad epilogue forms them:
    sum g y and mu sum g separately, each an exact fp32 sum (asserted)."""
    gs = gstored.double()
    u = lattice_unit(gs)
    require_lattice_sum(gs.abs().sum(0) * (1 + mu.abs()), u, "sum |g| (1 + |mu|)")
    require_lattice_sum((gs.abs() * yd.abs()).sum(0), u, "sum |g||y|")
    out = torch.stack([gs.sum(0), (gs * (yd - mu)).sum(0)])
    require_fp32(out, "BN sums")
    return out.float()


def ref_fold_wgrad(out0, t1, gram, colsum, wtd, c):
    """out [K, C] fp64 = out0 + k1 T1 + a (W Gram) + b (x) colsum with W = wt^T; integer operands, the
    whole sum on one power-of-two lattice and below 2^24 units (asserted)."""
    W = wtd.t()
    k1, a, b = c.k1[:, None], c.a[:, None], c.b[:, None]
    u = lattice_unit(c.k1, c.a, c.b)
    mag = out0.abs() + k1.abs() * t1.abs() + a.abs() * (W.abs() @ gram.abs()) + b.abs() * colsum.abs()[None, :]
    require_lattice_sum(mag, u, "fold wgrad: sum of magnitudes")
    require_lattice_sum(W.abs() @ gram.abs(), 1.0, "W Gram")
    return out0 + k1 * t1 + a * (W @ gram) + b * colsum[None, :]


# ---------------------------------------------------------------------- head
def ref_avgpool(xd):
    """(exact sums [N, C], HW) of the global average pool of NHWC xd; the mean is sums / HW."""
    n, h, w, c = xd.shape
    return xd.reshape(n, h * w, c).sum(1), h * w


def ref_avgpool_bwd(dpd, h, w):
    """(sum over splits [N, C], dx fp64 [N,H,W,C] = sum / HW) for dp [N, C] or [splits, N, C]."""
    s = dpd.sum(0) if dpd.dim() == 3 else dpd
    n, c = s.shape
    return s, (s / (h * w))[:, None, None, :].expand(n, h, w, c)


def ref_linear(pd, wd, bd, dld):
    """(logits, dpooled, dW, db) of logits = pooled W^T + b in fp64, integer operands, exact sums asserted."""
    for t, name in ((pd, "pooled"), (wd, "weight"), (dld, "dlogits")):
        ec.require_integers(t, torch.bfloat16, name)
    ec.require_below(pd.abs() @ wd.abs().t() + bd.abs(), ec.EXACT_LIMIT, "logits: sum |p||w| + |b|")
    ec.require_below(dld.abs() @ wd.abs(), ec.EXACT_LIMIT, "dpooled: sum |dl||w|")
    ec.require_below(dld.abs().t() @ pd.abs(), ec.EXACT_LIMIT, "dW: sum |dl||p|")
    return pd @ wd.t() + bd, dld @ wd, dld.t() @ pd, dld.sum(0)


def fc_split_count(m, n, k):
    """The split-K slices the fc launcher takes for an [m, n] output over a k-long reduction: doubled
    while the grid has fewer than 256 workgroups and every slice keeps >= 256 k, then the slices are
    rounded up to 32 k and recounted."""
    tiles = ((m + 63) // 64) * ((n + 63) // 64)
    s = 1
    while tiles * s < 256 and k // (s * 2) >= 256:
        s *= 2
    kper = ((k + s - 1) // s + 31) // 32 * 32
    return (k + kper - 1) // kper
