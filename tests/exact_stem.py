"""fp64 references, premises and case tables for the stem kernels (the companion of tests/exact_conv.py
and tests/exact_bn.py, whose integer-operand and crafted-coefficient arguments carry over).

The stem re-lays the image out as "super-pixels": pairs of horizontally adjacent pixels, channels padded
to 4, form one 8-channel pixel, so an odd S-wide stride-2 filter becomes Sp = (S + 1) / 2 taps of 8
channels at stride (2, 1).  ``ref_stem_image`` / ``ref_stem_pack_weight`` / ``ref_stem_unpack`` are those
layouts, ``ref_stem_fwd`` the convolution (im2col + matmul) and ``ref_stem_fwd_superpixel`` the same
convolution computed from the two layouts; ``ref_row_partials`` the per-output-row BN partials of the halo
kernel with ``row_m2_exact`` / ``require_row_m2_exact`` / ``row_m2_slack`` saying where the M2 has one
right answer and how far it may be off elsewhere; ``ref_stem_dy`` / ``ref_stem_wgrad`` the fused backward.

Images and weights are integers in -1..1 (|y| <= C R S <= 147, a bf16 value); everything is plain fp64
torch (no fp32 BLAS).  Activations are NHWC, weights [K, C, R, S]; the kernels take the image as fp32 NCHW
(``kernel_image``).  The case tables at the end are shared by tests/test_stem_exact_gpu.py (which runs
them) and tests/test_stem_exact_cpu.py (which checks every premise on the references alone).

This module is a helper, not a test file.
"""
from types import SimpleNamespace

import torch

import exact_bn as eb
import exact_conv as ec
from exact_conv import PremiseError, to_bf16

U = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)
STEM_K = 64
ROWS = 4                # output rows per workgroup of the halo forward
BWD_GRID = 512          # workgroups of the fused backward (one (image, row pair) item at a time)


def conv_shape(n, h, w, c=3, k=STEM_K, r=7, pad=3):
    """The exact_conv shape tuple of a square stride-2 stem."""
    return (n, h, w, c, k, r, r, 2, pad)


def kernel_image(xd):
    """NHWC fp64 -> the fp32 NCHW image stem_conv_fwd takes."""
    return xd.permute(0, 3, 1, 2).float().contiguous()


# -------------------------------------------------------------------- layouts
def ref_stem_image(xd, pad, Sp):
    """The super-pixel image [N, Hp, Wsp, 8] of NHWC xd [N, H, W, C <= 4] for an S = 2 Sp - 1 wide filter:
    pixel (hp, ws) holds source columns 2 ws + q - pad - 1, q = 0, 1, of source row hp - pad, channels
    padded to 4 with zeros, zeros outside the image.  Hp = H + 2 pad, Wsp = Wo + Sp - 1."""
    n, h, w, c = xd.shape
    s = 2 * Sp - 1
    wo = (w + 2 * pad - s) // 2 + 1
    hp, wsp = h + 2 * pad, wo + Sp - 1
    wide = torch.zeros(n, hp, 2 * wsp, 4, dtype=xd.dtype, device=xd.device)   # column j = source column j - pad - 1
    j1 = min(w + pad + 1, 2 * wsp)
    wide[:, pad:pad + h, pad + 1:j1, :c] = xd[:, :, :j1 - pad - 1]
    return wide.reshape(n, hp, wsp, 8)


def ref_stem_pack_weight(wd, Sp):
    """The packed weights [K, R, Sp, 8] of wd [K, C <= 4, R, S]: slot (p, q * 4 + c) holds tap s = 2 p + q - 1
    of channel c, zero where s = -1 or c >= C."""
    k, c, r, s = wd.shape
    assert s == 2 * Sp - 1
    wide = torch.zeros(k, r, 2 * Sp, 4, dtype=wd.dtype, device=wd.device)     # column j = tap j - 1
    wide[:, :, 1:, :c] = wd.permute(0, 2, 3, 1)
    return wide.reshape(k, r, Sp, 8)


def ref_stem_unpack(dwsp, C, S):
    """The inverse of ref_stem_pack_weight: [K, R, Sp, 8] -> [K, C, R, S]."""
    k, r, sp, _ = dwsp.shape
    return dwsp.reshape(k, r, 2 * sp, 4)[:, :, 1:S + 1, :C].permute(0, 3, 1, 2).contiguous()


# -------------------------------------------------------------------- forward
def ref_stem_fwd(xd, wd, pad):
    """y [N, Ho, Wo, K] in fp64: the stride-2 convolution by im2col + matmul (exact_conv.ref_fwd)."""
    n, h, w, c = xd.shape
    k, _, r, s = wd.shape
    return ec.ref_fwd(xd, wd, (n, h, w, c, k, r, s, 2, pad))


def ref_stem_fwd_superpixel(xd, wd, pad):
    """The same y from the two layouts alone: the stride-(2, 1) convolution of the super-pixel image with
    the packed weights, one tap at a time (no im2col)."""
    k, _, r, s = wd.shape
    sp = (s + 1) // 2
    xs, ws = ref_stem_image(xd, pad, sp), ref_stem_pack_weight(wd, sp)
    n, hp, wsp, _ = xs.shape
    ho, wo = (hp - r) // 2 + 1, wsp - sp + 1
    y = torch.zeros(n, ho, wo, k, dtype=xd.dtype, device=xd.device)
    for rr in range(r):
        for p in range(sp):
            y += xs[:, rr:rr + 2 * ho:2, p:p + wo] @ ws[:, rr, p].t()
    return y


def exact_stem_fwd(o, pad):
    """ref_stem_fwd of ``ec.int_operands`` output with its premises: exact fp32 accumulation and a bf16 y."""
    ec.require_below(ref_stem_fwd(o.xd.abs(), o.wd.abs(), pad), ec.EXACT_LIMIT, "stem fwd: sum |x||w| per output")
    y = ref_stem_fwd(o.xd, o.wd, pad)
    ec.require_integers(y, torch.bfloat16, "stem y", ec.BF16_EXACT)
    return y


# ------------------------------------------------------------- row statistics
def ref_row_partials(yd):
    """[N * Ho, 2, K] fp64: the exact sum of every output row and its M2 about the row mean."""
    n, ho, wo, k = yd.shape
    rows = yd.reshape(n * ho, wo, k)
    s = rows.sum(1)
    d = rows - (s / wo)[:, None, :]
    return torch.stack([s, (d * d).sum(1)], 1)


def row_m2_exact(yd):
    """[N * Ho, K] booleans: where the kernel's two-pass M2 has ONE right answer.  Wo is a power of two
    (1 / Wo and S / Wo are exact), every d = y - mean is a multiple of 1 / Wo and every d * d a multiple of
    1 / Wo^2 (integer y), and Wo^2 * sum d^2 < 2^24: every fp32 intermediate is then exact in any order.
    All False where Wo is no power of two."""
    n, ho, wo, k = yd.shape
    if not torch.equal(yd, yd.round()):
        raise PremiseError("row M2: y is not integer-valued")
    if wo & (wo - 1):
        return torch.zeros(n * ho, k, dtype=torch.bool, device=yd.device)
    rows = yd.reshape(n * ho, wo, k)
    d = rows - (rows.sum(1) / wo)[:, None, :]
    if not (torch.equal((d * wo).round(), d * wo) and torch.equal((d * d * wo * wo).round(), d * d * wo * wo)):
        raise PremiseError("row M2: deviations off the 1 / Wo lattice")
    return (d * d).sum(1) * (wo * wo) < ec.EXACT_LIMIT


def require_row_m2_exact(yd):
    """The premise of an exact M2 for EVERY (row, channel) of yd; PremiseError otherwise."""
    n, ho, wo, k = yd.shape
    if wo & (wo - 1):
        raise PremiseError(f"row M2: Wo = {wo} is not a power of two")
    row_m2_exact(yd)                                   # integers, lattice
    rows = yd.reshape(n * ho, wo, k)
    d = rows - (rows.sum(1) / wo)[:, None, :]
    eb.require_lattice_sum((d * d).sum(1), 1.0 / (wo * wo), "row M2: sum d^2")


def row_m2_slack(yd):
    """A bound on |M2_kernel - M2_ref| per (row, channel), [N * Ho, K] fp64, in u = 2^-24 and reference
    quantities only.  Derived, not measured:

    The row sum S is exact (integers, asserted exactly by the tests).  The kernel forms the mean
    m' = fl(S * fl(1 / Wo)): two roundings, |m' - m| <= (2u + u^2)|m| <= 3u |m| =: e with m = S / Wo (the
    bound also holds when the compiler contracts the product into the subtraction below, which removes one
    of the two roundings).  With a_i = (y_i - m')^2 the identity

        sum_i a_i = M2 + Wo (m - m')^2                      (the cross term vanishes: sum (y_i - m) = 0)

    gives 0 <= sum a_i - M2 <= Wo e^2.  The kernel computes d_i = fl(y_i - m') (one rounding, so
    d_i^2 = a_i (1 + t)^2, |t| <= u), accumulates fma(d_i, d_i, .) over at most TM = ceil(Wo / 16) terms per
    lane (one rounding per fma) and adds the 16 lanes in four butterfly steps (one rounding each).  All
    terms are non-negative, so every a_i reaches the result times a factor within (1 +- u)^(2 + TM + 4), and
    (1 + u)^(TM + 6) - 1 <= (TM + 7) u while (TM + 6)^2 u < 1 (TM <= 8).  Hence

        |M2_kernel - M2| <= (TM + 7) u (M2 + Wo e^2) + Wo e^2,      e = 3u |S / Wo|.
    """
    n, ho, wo, k = yd.shape
    part = ref_row_partials(yd)
    s, m2 = part[:, 0], part[:, 1]
    tm = (wo + 15) // 16
    e2 = wo * (3 * U * (s / wo).abs()) ** 2
    return (tm + 7) * U * (m2 + e2) + e2


def check_row_partials(part, yd, what=""):
    """part [N * Ho, 2, K] fp32 of the halo forward against the references: sums bit for bit, M2 bit for bit
    where ``row_m2_exact`` holds and within ``row_m2_slack`` elsewhere.  Returns the largest M2 error in
    units of the slack (for the test's report)."""
    n, ho, wo, k = yd.shape
    want = ref_row_partials(yd)
    assert part.shape == (n * ho, 2, k) and part.dtype == torch.float32, f"{what}: {tuple(part.shape)} {part.dtype}"
    eb.require_lattice_sum(yd.reshape(n * ho, wo, k).abs().sum(1), 1.0, f"{what} row sums")
    ec.assert_exact(part[:, 0].double(), want[:, 0], ROWS, None, None, f"{what} row sums")
    exact = row_m2_exact(yd)
    got, ref = part[:, 1].double(), want[:, 1]
    ec.assert_exact(torch.where(exact, got, ref), ref, ROWS, None, None, f"{what} M2 (exact rows)")
    slack = row_m2_slack(yd)
    err = (got - ref).abs()
    bad = (err > slack) | got.isnan()
    if bool(bad.any()):
        rows, cols = bad.nonzero(as_tuple=True)
        first = [(int(r_), int(c_), float(got[r_, c_]), float(ref[r_, c_]), float(slack[r_, c_]))
                 for r_, c_ in zip(rows[:8], cols[:8])]
        raise AssertionError(f"{what} M2: {rows.numel()} of {bad.numel()} partials outside the derived slack; "
                             f"first (row, channel, got, ref, slack): {first}")
    return float((err / slack.clamp_min(1e-300)).max()) if err.numel() else 0.0


# ------------------------------------------------------------ fused backward
def crafted_argmax(n, hq, wq, k, device="cpu"):
    """An argmax map [N, Hq, Wq, K] uint8 in which every selector 0..8 occurs at interior, edge and corner
    windows wherever it points inside the image: window (ph, pw) tap (kh, kw) is pixel (2 ph - 1 + kh,
    2 pw - 1 + kw), outside only for kh = 0 at ph = 0 and kw = 0 at pw = 0 (even Ho, Wo); those are moved
    to kh / kw = 1 or 2 by the channel's low bits."""
    i = torch.arange(n, device=device).view(n, 1, 1, 1)
    ph = torch.arange(hq, device=device).view(1, hq, 1, 1)
    pw = torch.arange(wq, device=device).view(1, 1, wq, 1)
    ch = torch.arange(k, device=device).view(1, 1, 1, k)
    sel = (7 * i + 5 * ph + 2 * pw + ch) % 9
    kh, kw = sel // 3, sel % 3
    kh = torch.where((ph == 0) & (kh == 0), 1 + (ch % 2), kh)
    kw = torch.where((pw == 0) & (kw == 0), 1 + ((ch // 2) % 2), kw)
    return (3 * kh + kw).to(torch.uint8)


def argmax_inside(bi, ho, wo):
    """Every selector of bi [N, Hq, Wq, K] points at a pixel of the [Ho, Wo] image."""
    n, hq, wq, k = bi.shape
    ph = torch.arange(hq, device=bi.device).view(1, hq, 1, 1)
    pw = torch.arange(wq, device=bi.device).view(1, 1, wq, 1)
    hh, ww = 2 * ph - 1 + (bi // 3).long(), 2 * pw - 1 + (bi % 3).long()
    return bool(((bi <= 8) & (hh >= 0) & (hh < ho) & (ww >= 0) & (ww < wo)).all())


def ref_stem_dy(c, dpd, bi, yd, training):
    """dy [N, Ho, Wo, K] bf16 of the stem's BN / pool backward apply as the fused kernel stores it: the
    max-pool gradient gather (``eb.ref_maxpool_bwd``), the ReLU mask recomputed from y (``eb.mask_on(2)``)
    and ``eb.exact_bwd_apply`` with crafted coefficients ``c``, rounded to bf16.

    exact_bwd_apply evaluates k1 (g - sgm - (y - mu) k2); the fused kernel evaluates k1 g + (A y + B) with
    A = -k1 k2 and B = k1 (mu k2 - sgm) formed in fp32 in-kernel from stats, gamma, sums and 1 / M, M taken
    from y's shape.  Both forms are exact for the crafted coefficients: every coefficient product, A, B,
    A y + B and the result are asserted to be fp32 values.  Where y's own M differs from the power-of-two
    count the coefficients were crafted for, 1 / M is rounded and only s0 = s1 = 0 (A = B = 0 whatever 1 / M
    is) leaves one right answer: anything else raises PremiseError."""
    n, ho, wo, k = yd.shape
    if not c.exact:
        raise PremiseError("ref_stem_dy needs crafted coefficients")
    if n * ho * wo != c.M and (bool((c.s0 != 0).any()) or bool((c.s1 != 0).any())):
        raise PremiseError(f"M = {n * ho * wo} of y is not the crafted count {c.M}: 1 / M is rounded, the sums must be 0")
    if not argmax_inside(bi, ho, wo):
        raise PremiseError("argmax map points outside the image")
    g = eb.ref_maxpool_bwd(dpd, bi, ho, wo)
    on = eb.mask_on(2, None, yd, c.scale, c.shift)
    dy, _ = eb.exact_bwd_apply(c, g, yd, on, training)
    gm = torch.where(on, g, 0.0)
    if training:
        a, b = -c.k1 * c.k2, c.k1 * (c.mu * c.k2 - c.sgm)
        for t, name in ((c.s1 * c.invstd, "s1 invstd"), (c.s1 * c.invstd * c.invstd, "s1 invstd^2"),
                        (c.mu * c.k2, "mu k2"), (c.mu * c.k2 - c.sgm, "mu k2 - sgm"), (a, "A"), (b, "B"),
                        (a * yd, "A y"), (a * yd + b, "A y + B"), (c.k1 * gm, "k1 g"), (c.k1 * gm + (a * yd + b), "dy")):
            eb.require_fp32(t, f"stem dy: {name}")
        if not torch.equal(c.k1 * gm + (a * yd + b), dy):
            raise PremiseError("stem dy: the factored and the k1 g + A y + B forms differ in fp64")
    else:
        eb.require_fp32(c.k1 * gm, "stem dy: k1 g")
    return to_bf16(dy)


def ref_stem_wgrad(dy_bf16, xd, pad, w_shape):
    """dW [K, C, R, S] fp64 of the STORED bf16 dy [N, Ho, Wo, K] against the NHWC image xd.  Premise: the
    products lie on one power-of-two lattice and sum |dy||x| per output element stays below 2^24 lattice
    units, so the atomic, slab and split-K orders all have one right answer."""
    k, c, r, s = w_shape
    n, h, w, _ = xd.shape
    shape = (n, h, w, c, k, r, s, 2, pad)
    dyd = dy_bf16.double()
    assert tuple(dyd.shape[1:3]) == ec.out_hw(shape) and dyd.shape[3] == k, "dy does not match the convolution"
    eb.require_lattice_sum(ec.ref_wgrad(dyd.abs(), xd.abs(), shape), eb.lattice_unit(dyd), "stem wgrad: sum |dy||x|")
    return ec.ref_wgrad(dyd, xd, shape)


def fused_coefs(m, seed, device="cpu"):
    """Crafted BN coefficients for a fused-backward case of M = N Ho Wo rows: ``eb.craft`` at M where M is a
    power of two; otherwise crafted for the next power of two with the sums set to zero (ref_stem_dy)."""
    if m & (m - 1) == 0:
        return eb.craft(STEM_K, m, seed, device)
    mc = 1 << m.bit_length()
    c = eb.craft(STEM_K, mc, seed, device)
    zero = torch.zeros_like(c.s0)
    return eb.pack_coefs(c.mu, c.invstd, c.gammad, zero, zero, c.scale, c.shift, mc)


_FUSED = {}


def fused_case(nhw, argmax, device="cpu"):
    """Operands and references of one fused-backward case (built once per (shape, argmax kind, device) and
    never modified): integer image and weights, y = the exact forward, the argmax bytes built here ("pool":
    ``eb.ref_bn_relu_maxpool`` of y; "crafted": ``crafted_argmax``), an integer pooled gradient, and per
    ``training`` the expected dy and dW."""
    key = (tuple(nhw), argmax, str(device))
    if key in _FUSED:
        return _FUSED[key]
    n, h, w = nhw
    shape = conv_shape(n, h, w)
    o = ec.int_operands(shape, (-1, 1), (-1, 1), seed=sum(shape), device=device)
    yd = exact_stem_fwd(o, 3)
    ho, wo = yd.shape[1:3]
    assert ho % 2 == 0 and wo % 16 == 0 and 16 <= wo <= 128, "outside the fused backward's domain"
    c = fused_coefs(n * ho * wo, 70 + n, device)
    if argmax == "pool":
        _, bi, _ = eb.ref_bn_relu_maxpool(yd, c.scale, c.shift)
    else:
        bi = crafted_argmax(n, ho // 2, wo // 2, STEM_K, device)
    dp, dpd = ec.int_tensor((n, ho // 2, wo // 2, STEM_K), (-60, 60), 71 + n, device)
    f = SimpleNamespace(o=o, shape=shape, yd=yd, y=to_bf16(yd), c=c, bi=bi.contiguous(), dp=dp, dpd=dpd,
                        xsp=to_bf16(ref_stem_image(o.xd, 3, 4)), items=n * ho // 2, dy={}, dw={})
    for training in (True, False):
        f.dy[training] = ref_stem_dy(c, dpd, f.bi, yd, training)
        f.dw[training] = ref_stem_wgrad(f.dy[training], o.xd, 3, [STEM_K, 3, 7, 7])
        eb.require_fp32(f.dw[training], "dW")
    _FUSED[key] = f
    return f


# ---------------------------------------------------------------- case tables
# Halo forward, (N, H, W).  H = 9: Ho = 5, two row groups per image, the second with three invalid waves.
TM_WIDTHS = [1, 2, 31, 32, 33, 64, 66, 96, 98, 128, 130, 160, 162, 192, 194, 224, 226, 250, 256]
TM_WOS = [1, 1, 16, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 125, 128]   # every TM 1..8, full and partial
FWD_TM_CASES = [(2, 9, w) for w in TM_WIDTHS]
FWD_HO_CASES = [(2, h, 32) for h in (1, 2, 3, 5, 8, 9, 11, 13, 16)]             # Ho mod 4, Ho = 1, halo clipped at Hp
FWD_PERSISTENT_CASES = [(1600, 8, 32), (700, 9, 32)]                            # more row groups than 4 x the CU count
# Generic fallback through the (2, 1)-stride ConvShape: ((N, H, W), K, R, pad)
FALLBACK_CASES = [
    ((1, 9, 262), 64, 7, 3),        # Wo = 131 > 128
    ((2, 9, 32), 32, 7, 3),
    ((2, 9, 32), 128, 7, 3),
    ((2, 8, 32), 64, 5, 2),
    ((2, 8, 32), 64, 3, 1),
]
# Fused backward, (N, H, W)
BWD_CASES = [
    (1, 4, 32), (4, 8, 32),         # one unit per thread, partly idle (Wq * 8 = 64)
    (2, 4, 160), (1, 4, 256),       # second unit live for some threads / all threads
    (2, 8, 160), (1, 8, 256),       # the same with Hq = 2: the second unit's lower windows (W10, W11) exist
    (2, 7, 32), (2, 3, 64),         # halo clip exactly at Hp (odd H, even Ho)
    (300, 8, 32), (1100, 4, 32),    # items > 512: prefetch, both halo buffers, clamped last prefetch
    (1024, 4, 32),                  # the same with M a power of two: the full A y + B term
]
BWD_SLAB_CASES = [(1, 4, 32), (3, 4, 32), (17, 4, 32), (32, 4, 32)]             # grid 1, 3, 17 (and 32, M a power of two)
BWD_MANY_ITEMS = [(300, 8, 32), (1100, 4, 32), (1024, 4, 32)]
COMPOSITION_CASE = (4, 8, 32)
