"""Crafted operands, fp64 references and case tables for what runs between two forward passes: the flat
optimizer steps (sgd_step, lars_*), the bf16 weight images (cast_to_bf16, pack_weight, pack_weight_t,
pack_t_batched) and the fp8 quantizers with their delayed-scaling state (quant_e4m3, bn_act_fwd_q8,
bn_act_bwd_apply_q8, quant_rows_e4m3, pack_weight_fp8).  The companion of tests/exact_conv.py and
tests/exact_bn.py; a helper, not a test file.  There is no tolerance anywhere in it.

Optimizer element math.  Every operation of ``sgd_kernel`` and ``lars_update_kernel`` is an explicit fmaf
or one multiply, so the order of the roundings is fixed:

    d = fmaf(wd, p, g * scale)                 (LARS: d = trust * fmaf(wd_eff, p, g))
    buf = first ? d : fmaf(m, buf, (1 - damp) * d) ;  d = nesterov ? fmaf(m, buf, d) : buf
    p = fmaf(-lr, d, p)

Parameters, gradients and momentum are small integers; lr, m, 1 - damp, wd, scale and the trust values
are dyadic.  ``ref_update`` transcribes the formula in fp64 and requires EVERY rounding point above to
survive ``.float().double()`` unchanged (``exact_bn.require_fp32``), for both steps of every case: the
fp64 result is then the one right answer and the bf16 mirror is one round-to-nearest-even of it.
``tie_counts`` counts the elements of the new p that sit exactly between two bf16 values, by the
direction RNE takes; the case tables must hold at least ``MIN_TIES`` of each direction wherever a case
has ``TIE_MIN_N`` elements or more, so neither truncation nor round-half-up can pass.  (The sizes below
that exist for the tail loop; a handful of elements cannot hold 32 ties and no minimum is claimed there.)

The bindings reject flat buffers that are not 16-byte aligned (test_param_alignment pins that), so the
``lead`` path of ``sgd_kernel`` cannot be reached from Python and no case here tries to; the same
``lead`` arithmetic of the LARS kernels IS reached, through segment offsets that are 1, 2 and 3 mod 4.

LARS norms and trust.  Integer data makes the float64 partial sums exact integers in any order.  Every
adapted segment is built so that sum p^2 and sum g^2 are perfect squares (four reserved elements take a
four-square decomposition of the gap to the next square): sqrt is then exact, every remaining operation
is one IEEE float64 rounding on both sides, and the expected trust is the formula evaluated operation
by operation in torch float64, cast once to fp32.

fp8.  The codes are the bytes of ``x.float().mul(s).clamp(+-max).to(float8)`` with s a power of two (the
product is exact); ``decode_e4m3`` / ``decode_e5m2`` are hand tables of all 256 codes the CPU file holds
that cast against.  The delayed scale is 2^floor(log2(headroom / amax)) computed on the exact rational
quotient (``scale_for``), clamped to [2^-32, 2^32].  The row-wise quantizers multiply by ``1.f / sc``:
their reference does the same two fp32 operations (``rows_ref``), which is bit-reproducible.
"""
import math
from fractions import Fraction
from types import SimpleNamespace

import torch

import exact_bn as eb
import exact_conv as ec
from exact_conv import PremiseError, to_bf16

CHUNK = 4096            # lars_chunk_elems(), asserted by the GPU file
MIN_TIES = 16           # exact bf16 ties of each direction a case must hold ...
TIE_MIN_N = 1023        # ... when it has at least this many elements
SENT_F32 = 777.0        # sentinel of fp32 buffers that must not be written
SENT_BF16 = -12352.0    # the same for bf16 mirrors (a bf16 value)
SENT_U8 = 0xA5

E4M3_MAX, E5M2_MAX = 448.0, 57344.0
E4M3_HEADROOM, E5M2_HEADROOM = 224.0, 28672.0
AMAX_SHARDS, SHARD_STRIDE = 64, 32
SLOT_FLOATS = AMAX_SHARDS * SHARD_STRIDE


# ===================================================================== optimizer element math
LR, MOM, DAMP, WD = 2.0 ** -3, 0.5, 0.25, 2.0 ** -4

MODES = {"plain": (0.0, False), "momentum": (MOM, False), "nesterov": (MOM, True)}


def variants():
    """{momentum 0, momentum, Nesterov} x {mirror, none} x {dampening 0, 0.25} x {grad_scale 1, 0.5}."""
    out = []
    for mode, (m, nest) in MODES.items():
        for mirror in (True, False):
            for damp in (0.0, DAMP):
                for gs in (1.0, 0.5):
                    out.append(SimpleNamespace(id=f"{mode}-{'mirror' if mirror else 'nomirror'}-d{damp:g}-s{gs:g}",
                                               mode=mode, momentum=m, nesterov=nest, mirror=mirror, dampening=damp,
                                               grad_scale=gs, lr=LR, wd=WD))
    return out


VARIANTS = variants()
SGD_SIZES = [1, 2, 3, 4, 5, 7, 1023, 4099, 4 * 256 * 4096 + 4 * 256 + 3]


def sgd_operands(n, seed=0, device="cpu"):
    """(p, g1, g2) fp64 integers in [-15, 15]: parameters and the gradients of two steps."""
    g = torch.Generator().manual_seed(1000 + seed)
    return tuple(torch.randint(-15, 16, (n,), generator=g).double().to(device) for _ in range(3))


_CHECK = [True]


def _fp32(t, what):
    if _CHECK[0]:
        eb.require_fp32(t, what)
    return t


def ref_update(p, g, buf, v, first, trust=None, wd=None, damp_ignored=False, scale_after_wd=False):
    """One step in fp64 with every fp32 rounding point of the kernels required exact: (p', buf').
    ``trust`` / ``wd`` (per-element fp64 tensors): the LARS form.  ``damp_ignored`` and ``scale_after_wd``
    are the defects of the CPU demonstrations (they change the formula, not the premise)."""
    wd = v.wd if wd is None else wd
    _CHECK[0] = not (damp_ignored or scale_after_wd)         # a defective formula owes no premise
    if trust is None:
        gs = _fp32(g * v.grad_scale, "g * scale")
        d = _fp32(wd * p + gs, "wd * p + g * scale") if not scale_after_wd else (wd * p + g) * v.grad_scale
    else:
        d = _fp32(trust * _fp32(wd * p + g, "wd * p + g"), "trust * (wd * p + g)")
    if v.momentum != 0.0:
        if first:
            buf = d
        else:
            dd = _fp32((1.0 if damp_ignored else 1.0 - v.dampening) * d, "(1 - damp) * d")
            buf = _fp32(v.momentum * buf + dd, "m * buf + (1 - damp) * d")
        d = _fp32(v.momentum * buf + d, "d + m * buf") if v.nesterov else buf
    return _fp32(p - v.lr * d, "p - lr * d"), buf


def ref_two_steps(p, g1, g2, v, **kw):
    """[(p', buf') after step 1 (first=True), (p'', buf'') after step 2]; buf is None at momentum 0."""
    p1, b1 = ref_update(p, g1, None, v, True, **kw)
    p2, b2 = ref_update(p1, g2, b1, v, False, **kw)
    return [(p1, b1), (p2, b2)]


def tie_counts(t):
    """(ties RNE rounds up in magnitude, ties it rounds down) among the fp32 values of fp64 ``t``."""
    bits = t.float().view(torch.int32)
    tie = (bits & 0xFFFF) == 0x8000
    odd = ((bits >> 16) & 1) == 1
    return int((tie & odd).sum()), int((tie & ~odd).sum())


def require_ties(steps, n, what):
    """The stated minimum of ties of each direction over the new p of both steps, and most elements of
    the new p needing more than bf16's 8 significant bits."""
    if n < TIE_MIN_N:
        return
    up = down = 0
    for p_new, _ in steps:
        u, d = tie_counts(p_new)
        up, down = up + u, down + d
        inexact = float((to_bf16(p_new).double() != p_new).double().mean())
        if inexact <= 0.5:
            raise PremiseError(f"{what}: only {inexact:.1%} of the new p need more than 8 significant bits")
    if up < MIN_TIES or down < MIN_TIES:
        raise PremiseError(f"{what}: {up} / {down} bf16 ties (up / down), need {MIN_TIES} of each")


def trunc_bf16(t):
    """The defect: a mirror written by truncation of the fp32 bits."""
    return (t.float().view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)


# ------------------------------------------------------------------------------------- LARS table
def lars_segments():
    """(offset, numel, excluded): starts 1, 2 and 3 mod 4 (lead 3, 2, 1), segments shorter than their lead,
    chunk, chunk + 1, 2 chunk - 1, more than 64 chunks, excluded ones, and gaps no segment covers."""
    c = CHUNK
    segs = [(0, c, False),
            (c + 1, 1, False),                 # start = 1 mod 4, shorter than its lead of 3
            (c + 2, 2, False),                 # start = 2 mod 4, as long as its lead of 2
            (c + 7, c + 1, False),             # start = 3 mod 4
            (2 * c + 9, 2 * c - 1, False),     # start = 1 mod 4
            (4 * c + 10, 7, True),             # start = 2 mod 4, excluded
            (4 * c + 19, 65 * c + 5, False),   # start = 3 mod 4, 66 chunks
            (69 * c + 24, 40, True),           # excluded, aligned
            (69 * c + 65, 5, False)]           # start = 1 mod 4: lead 3, no vector, tail 2
    for (o, n, _), (o2, _, _) in zip(segs, segs[1:]):
        assert o + n <= o2
    return segs, 69 * c + 72                   # total elements (a gap at the end too)


def lars_chunks(segs):
    """(start, n, segment index, excluded) of every chunk, as optim.lars.LarsTable cuts them."""
    out = []
    for si, (off, numel, ex) in enumerate(segs):
        for k in range((numel + CHUNK - 1) // CHUNK):
            start = off + k * CHUNK
            out.append((start, min(CHUNK, off + numel - start), si, ex))
    return out


def seg_index(segs, numel, device="cpu"):
    """Per element: its segment index, -1 in the gaps."""
    idx = torch.full((numel,), -1, dtype=torch.long, device=device)
    for si, (o, n, _) in enumerate(segs):
        idx[o:o + n] = si
    return idx


def lars_trust_values(segs):
    """A different power of two per segment; excluded segments get a non-1 value too (the update must use
    the table value and drop only the weight decay)."""
    exps = [2, 1, 3, -1, -2, -3, -4, 4, 0]         # the long segment gets the smallest: its new p needs the most bits
    tr = torch.tensor([2.0 ** exps[si] for si in range(len(segs))], dtype=torch.float64)
    assert all(float(tr[si]) != 1.0 for si, (_, _, ex) in enumerate(segs) if ex) and tr.unique().numel() == len(segs)
    return tr


def lars_elementwise(segs, numel, trust, wd, device="cpu"):
    """(trust per element, wd_eff per element, covered mask) in fp64."""
    idx = seg_index(segs, numel, device)
    cov = idx >= 0
    safe = idx.clamp_min(0)
    tr = torch.where(cov, trust.to(device)[safe], 1.0)
    ex = torch.tensor([e for _, _, e in segs], device=device)[safe]
    wde = torch.where(cov & ~ex, wd, 0.0).double()
    return tr, wde, cov


def range_mask(segs, numel, lo, hi, device="cpu"):
    idx = seg_index(segs, numel, device)
    return (idx >= lo) & (idx < hi)


# ---------------------------------------------------------------------- LARS norms / trust data
def four_squares(n):
    """(a, b, c, d) >= 0 with a^2 + b^2 + c^2 + d^2 == n (Lagrange), by search."""
    r = math.isqrt(n)
    for a in range(r, -1, -1):
        na = n - a * a
        for b in range(min(a, math.isqrt(na)), -1, -1):
            nb = na - b * b
            for c in range(min(b, math.isqrt(nb)), -1, -1):
                d2 = nb - c * c
                d = math.isqrt(d2)
                if d * d == d2 and d <= c:
                    return a, b, c, d
    raise AssertionError(n)


def _square_fill(t, gen):
    """Fill 1-D fp64 ``t`` (>= 5 elements) with integers in [-3, 3], then set its last four elements so
    that the sum of squares is a perfect square."""
    n = t.numel()
    t[:n - 4] = torch.randint(-3, 4, (n - 4,), generator=gen).double()
    s = int((t[:n - 4] ** 2).sum().item())
    root = math.isqrt(s) + 2
    t[n - 4:] = torch.tensor(four_squares(root * root - s), dtype=torch.float64)
    return t


def lars_norm_operands(segs, numel, seed=0):
    """(p, g) fp64 integers: every adapted segment has perfect-square sum p^2 and sum g^2; segment 2 has
    |g| = 0, the last segment |p| = 0; the gaps hold values no kernel may read into a sum."""
    gen = torch.Generator().manual_seed(2000 + seed)
    p = torch.randint(-3, 4, (numel,), generator=gen).double()
    g = torch.randint(-3, 4, (numel,), generator=gen).double()
    hand = {1: ([3.0], [4.0]), 2: ([3.0, 4.0], [0.0, 0.0])}       # 9 / 16, 25 / 0
    for si, (o, n, ex) in enumerate(segs):
        if ex:
            continue
        if n in hand:
            p[o:o + n] = torch.tensor(hand[n][0], dtype=torch.float64)
            g[o:o + n] = torch.tensor(hand[n][1], dtype=torch.float64)
        else:
            _square_fill(p[o:o + n], gen)
            _square_fill(g[o:o + n], gen)
    o, n, _ = segs[-1]
    p[o:o + n] = 0.0
    return p, g


def ref_partials(p, g, segs, sentinel):
    """[nchunks, 2] fp64: (sum p^2, sum g^2) per chunk; excluded chunks keep the sentinel."""
    ch = lars_chunks(segs)
    out = torch.full((len(ch), 2), sentinel, dtype=torch.float64, device=p.device)
    for ci, (s, n, _, ex) in enumerate(ch):
        if not ex:
            out[ci, 0] = (p[s:s + n] ** 2).sum()
            out[ci, 1] = (g[s:s + n] ** 2).sum()
    ec.require_below(out.abs(), 2.0 ** 53, "chunk sums")
    return out


def require_perfect_squares(p, g, segs):
    for si, (o, n, ex) in enumerate(segs):
        if ex:
            continue
        for t, name in ((p, "p"), (g, "g")):
            s = int((t[o:o + n] ** 2).sum().item())
            if math.isqrt(s) ** 2 != s:
                raise PremiseError(f"segment {si}: sum {name}^2 = {s} is no perfect square")


def ref_trust(p, g, segs, wd, eta, eps):
    """fp32 [nseg]: excluded or |p| == 0 or |g| == 0 ? 1 : float((eta pn) / ((gn + wd pn) + eps)), each
    operation one torch float64 rounding on the CPU."""
    out = []
    for o, n, ex in segs:
        sp, sg = (p[o:o + n].cpu() ** 2).sum(), (g[o:o + n].cpu() ** 2).sum()
        if ex or sp == 0 or sg == 0:
            out.append(torch.tensor(1.0, dtype=torch.float64))
            continue
        pn, gn = sp.sqrt(), sg.sqrt()
        wd_, eta_, eps_ = (torch.tensor(x, dtype=torch.float64) for x in (wd, eta, eps))
        out.append((eta_ * pn) / ((gn + wd_ * pn) + eps_))
    return torch.stack(out).float()


def e2e_trust(segs, g, eta):
    """fp64 [nseg] of the end-to-end case p = 4 g, wd = eps = 0: 4 eta, and 1 where the segment is excluded
    or its gradient is all zero."""
    return torch.tensor([1.0 if ex or float((g[o:o + n] ** 2).sum()) == 0 else 4.0 * eta for o, n, ex in segs],
                        dtype=torch.float64)


TRUST_PARAMS = [(0.0, 2.0 ** -4, 0.0), (1e-4, 1e-3, 1e-8)]      # (wd, eta, eps): both zero, both non-zero


# =========================================================================== casts and weight images
def tie_patterns():
    """fp32 bit patterns (int32): every finite bf16 value followed by 0x8000, 0x7FFF and 0x8001 -- exact ties
    (fp32 subnormals among them) and their neighbours -- plus +-0 and +-inf.  No NaN."""
    hi = torch.arange(0, 1 << 16, dtype=torch.int64)
    hi = hi[((hi >> 7) & 0xFF) != 0xFF]
    pats = torch.cat([(hi << 16) | low for low in (0x8000, 0x7FFF, 0x8001)] +
                     [torch.tensor([0x00000000, 0x80000000, 0x7F800000, 0xFF800000])])
    return torch.where(pats >= 1 << 31, pats - (1 << 32), pats).to(torch.int32)


def cast_data(n, seed=0):
    """fp32 [n]: the tie patterns (cycled from a per-size start), every other element random finite bits."""
    gen = torch.Generator().manual_seed(3000 + seed)
    pats = tie_patterns()
    rnd = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=gen, dtype=torch.int64).to(torch.int32)
    rnd = torch.where(((rnd >> 23) & 0xFF) == 0xFF, rnd & ~(1 << 30), rnd)        # exponent 255 -> finite
    idx = (torch.arange(n) // 2 + 32768 * seed) % pats.numel()
    bits = torch.where(torch.arange(n) % 2 == 0, pats[idx], rnd)
    x = bits.view(torch.float32)
    assert not bool(x.isnan().any())
    return x


CAST_SIZES = [1, 7, 256 * 4096 + 5, 2 * 256 * 4096 + 3]

# (K, C, R, S, cpad, pack_weight_t too)
PACK_SHAPES = [(72, 40, 3, 3, 48, True), (72, 40, 3, 3, 0, True), (8, 3, 7, 7, 8, False), (136, 72, 1, 1, 80, True),
               (8, 8, 1, 1, 0, True)]


def weight_data(k, c, r, s, seed=0):
    """fp32 [K, C, R, S] (contiguous): distinct random values, every fifth one an exact bf16 tie."""
    gen = torch.Generator().manual_seed(4000 + seed)
    w = torch.randn(k, c, r, s, generator=gen)
    flat = w.view(-1)
    ties = ((flat[::5].view(torch.int32) & ~0xFFFF) | 0x8000).view(torch.float32)
    flat[::5] = ties
    return w


def ref_pack_weight(w, cpad):
    """bf16 [K, R, S, max(cpad, C)], zero above C."""
    k, c, r, s = w.shape
    out = torch.zeros(k, r, s, max(cpad, c), dtype=torch.bfloat16, device=w.device)
    out[..., :c] = w.permute(0, 2, 3, 1).to(torch.bfloat16)
    return out


def ref_pack_weight_t(w):
    return w.permute(1, 2, 3, 0).contiguous().to(torch.bfloat16)


# ------------------------------------------------------------------------------ pack_t_batched
def pack_t_layout():
    """[(offset, K, C, RS)] and the flat size: K, C in {8, 64, 72, 136} crossed with RS in {1, 9}, one
    512 x 512 x 9 tensor (576 tiles: the 512-block grid strides), gaps of 8 .. 56 elements between them."""
    ent, off = [], 24
    dims = [(k, c, rs) for rs in (1, 9) for k in (8, 64, 72, 136) for c in (8, 64, 72, 136)]
    dims.insert(5, (512, 512, 9))
    for i, (k, c, rs) in enumerate(dims):
        ent.append((off, k, c, rs))
        off += k * c * rs + 8 * (1 + i % 7)
    return ent, off + 4096      # a long sentinel tail: a store one c row past the last tensor stays inside dst


def pack_t_table_rows(ent):
    """The rows parallel/flat.py builds: (off, K, C, RS, tiles_k, tiles_c, pad) and max_tiles."""
    rows = [(o, k, c, rs, (k + 63) // 64, (c + 63) // 64, 0) for o, k, c, rs in ent]
    return rows, max(r[3] * r[4] * r[5] for r in rows)


def pack_t_src(total, device="cpu"):
    """Distinct 16-bit patterns (int16; view as bf16): any misplaced element is seen."""
    return (torch.arange(total, device=device) & 0xFFFF).to(torch.int16)


def ref_pack_t(src16, ent, sentinel16, skip_last_c_tile=False):
    """int16 [total]: every tensor's [K, RS, C] slice transposed to [C, RS, K], the gaps keeping the
    sentinel.  ``skip_last_c_tile``: the defect of the CPU demonstration."""
    dst = torch.full_like(src16, sentinel16)
    for o, k, c, rs in ent:
        t = src16[o:o + k * c * rs].view(k, rs, c).permute(2, 1, 0).contiguous()
        if skip_last_c_tile and c % 64:
            t[c - c % 64:] = sentinel16
        dst[o:o + k * c * rs] = t.reshape(-1)
    return dst


# ======================================================================================= fp8
def decode_e4m3(code):
    """OCP e4m3fn by hand: bias 7, subnormals m * 2^-9, no infinity, S.1111.111 = NaN."""
    s, e, m = code >> 7, (code >> 3) & 0xF, code & 7
    if e == 0xF and m == 7:
        return math.nan
    v = m * 2.0 ** -9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7)
    return -v if s else v


def decode_e5m2(code):
    """OCP e5m2 by hand: bias 15, subnormals m * 2^-16, exponent 31 = inf / NaN."""
    s, e, m = code >> 7, (code >> 2) & 0x1F, code & 3
    if e == 0x1F:
        return math.nan if m else (-math.inf if s else math.inf)
    v = m * 2.0 ** -16 if e == 0 else (1 + m / 4) * 2.0 ** (e - 15)
    return -v if s else v


def q_e4m3(x, s=1.0):
    """The reference codes (uint8, on the device of x): x (bf16 or fp32) times a power of two, clamped,
    cast.  The cast itself always runs on the CPU, where the CPU file holds it against the hand tables."""
    return x.float().cpu().mul(s).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8).to(x.device)


def q_e5m2(x, s=1.0):
    return x.float().cpu().mul(s).clamp(-E5M2_MAX, E5M2_MAX).to(torch.float8_e5m2).view(torch.uint8).to(x.device)


def scale_for(amax, headroom=E4M3_HEADROOM, late_ulp=False):
    """The delayed scale of a call whose predecessor saw ``amax`` (a float): 1 when amax is 0, else
    2^floor(log2(headroom / amax)) on the exact rational quotient (math.frexp on its numerator and
    denominator, no floating log2), clamped to [2^-32, 2^32].  ``late_ulp``: the defect of the CPU
    demonstration -- a log2 that comes out one ulp low at an exact power of two."""
    if not amax > 0:
        return 1.0
    q = Fraction(headroom) / Fraction(amax)
    e = math.frexp(q.numerator)[1] - math.frexp(q.denominator)[1] if max(q.numerator, q.denominator) < 2 ** 53 \
        else q.numerator.bit_length() - q.denominator.bit_length()
    while Fraction(2) ** e > q:
        e -= 1
    while Fraction(2) ** (e + 1) <= q:
        e += 1
    if late_ulp and Fraction(2) ** e == q:
        e -= 1
    return 2.0 ** max(-32, min(32, e))


def bf16_neighbours(v):
    """(the bf16 value below, v, the one above) of a positive bf16 value, as floats."""
    t = torch.tensor([v], dtype=torch.bfloat16)
    assert float(t) == v
    return float(eb._bf16_step(t, False)), v, float(eb._bf16_step(t, True))


E4M3_BOUNDARIES = [448.0, 224.0, 7.0, 3.5, 0.4375]           # 224 * 2^-k and 448
E5M2_BOUNDARIES = [28672.0, 3584.0, 56.0]                    # 28672 * 2^-k


def boundary_chain(boundaries):
    """amax values of a chain of calls on one state: each boundary with its bf16 neighbour below and above."""
    return [a for b in boundaries for a in bf16_neighbours(b)]


def e4m3_midpoints():
    """Every value exactly between two neighbouring non-negative e4m3 values (subnormals included, 0 and the
    smallest subnormal too): the cast must round each to the even code."""
    vals = [decode_e4m3(c) for c in range(0x7F)]
    return [(a + b) / 2 for a, b in zip(vals, vals[1:])]


def quant_data(nvec, amax, where, seed=0, s_next=1.0):
    """bf16 [1, 1, nvec, 8]: small integers, e4m3 ties and subnormals (divided by ``s_next``, the scale the
    next call applies to it, a power of two), all of magnitude below ``amax``; ``amax`` itself (a bf16
    value, sign from the seed) planted in vector ``where``.  amax == 0: all zeros."""
    n = nvec * 8
    if amax == 0:
        return torch.zeros(1, 1, nvec, 8, dtype=torch.bfloat16)
    gen = torch.Generator().manual_seed(5000 + seed)
    pool = torch.tensor([float(i) for i in range(-40, 41)] + e4m3_midpoints()[:40] +
                        [-m for m in e4m3_midpoints()[:40]] + [17.0, 19.0, 21.0, 23.0, -17.0, -19.0, 208.0, 240.0],
                        dtype=torch.float64) / s_next
    pool = pool[pool.abs() < amax]
    if pool.numel() == 0:
        pool = torch.zeros(1, dtype=torch.float64)
    x = pool[torch.randint(0, pool.numel(), (n,), generator=gen)]
    if not torch.equal(to_bf16(x).double(), x):
        raise PremiseError("quant_data: a pool value is no bf16 value")
    x[where * 8 + seed % 8] = amax if seed % 2 == 0 else -amax
    x = x.to(torch.bfloat16).reshape(1, 1, nvec, 8)
    assert float(x.float().abs().max()) == amax
    return x


QUANT_NVEC = [1, 255, 256 * 64 + 1, 256 * 4096 + 3]


def amax_places(nvec):
    """Vectors that take the amax element in turn: the first, the last, one in a block of index >= 64."""
    return sorted({0, nvec - 1} | ({256 * 64 + min(5, nvec - 1 - 256 * 64)} if nvec > 256 * 64 else set()))


def slot_view(state, slot):
    return state[slot * SLOT_FLOATS:(slot + 1) * SLOT_FLOATS]


def check_state(state, slot, deq_offset, s, amax, what):
    """After a call on ``slot``: deq[slot] == 1 / s exactly, the slot's shards hold the call's amax (their
    max equals it, none exceeds it, nothing else in the slot is written), the next slot is all zero."""
    st = state.cpu()
    assert st[deq_offset + slot].item() == 1.0 / s, f"{what}: deq {st[deq_offset + slot].item()} != 1 / {s}"
    cur = slot_view(st, slot).view(AMAX_SHARDS, SHARD_STRIDE)
    assert cur[:, 0].max().item() == amax, f"{what}: amax {cur[:, 0].max().item()} != {amax}"
    assert bool((cur[:, 0] >= 0).all()) and bool((cur[:, 1:] == 0).all()), f"{what}: shard layout"
    assert bool((slot_view(st, (slot + 1) % 3) == 0).all()), f"{what}: the next slot is not cleared"


# ------------------------------------------------------------------------------ row quantizers
def rows_ref(x, e5m2=False):
    """(scale fp32 [rows], codes uint8 [rows, len]) of fp32 x [rows, len] with the kernels' arithmetic: sc =
    amax / 448 (one fp32 division; 1 for a zero row), inv = 1.f / sc, x * inv (both fp32), clamp, cast."""
    assert x.dtype == torch.float32
    m = x.abs().amax(1)
    sc = torch.where(m > 0, m / torch.tensor(E4M3_MAX), torch.ones_like(m))
    inv = torch.ones_like(sc) / sc
    return sc, q_e4m3(x * inv[:, None])


# (rows, rowlen) of the tensors in one flat buffer; max_rows = 5 exceeds the small ones' row counts
QROWS_TENSORS = [(1, 8), (3, 72), (5, 576), (3, 4608), (5, 8), (1, 4608), (4, 72)]


def qrows_layout():
    """[(off, soff, rows, rowlen)] as WeightMirror._build_fp8 lays them out, with gaps; (total, nscale)."""
    ent, off, soff = [], 16, 0
    for i, (rows, rl) in enumerate(QROWS_TENSORS):
        ent.append((off, soff, rows, rl))
        off += rows * rl + 8 * (1 + i % 3)
        soff += rows
    return ent, off, soff


def qrows_data(ent, total, seed=0):
    """bf16 [total] and the kind of every row: 'zero', 'pow2' (amax 448 * 2^k planted: the division by the
    scale is exact) or 'general'."""
    gen = torch.Generator().manual_seed(6000 + seed)
    src = torch.zeros(total, dtype=torch.bfloat16)
    kinds = []
    for ti, (o, _, rows, rl) in enumerate(ent):
        for r in range(rows):
            kind = ("general", "pow2", "zero")[(ti + 2 * r) % 3] if rows > 1 else ("pow2", "general")[ti % 2]
            row = (torch.randn(rl, generator=gen) * 0.05).to(torch.bfloat16)
            if kind == "zero":
                row.zero_()
            elif kind == "pow2":
                k = (ti + r) % 7 - 9
                row = torch.randint(-447, 448, (rl,), generator=gen).double().mul(2.0 ** k).to(torch.bfloat16)
                row[(7 * r + ti) % rl] = 448.0 * 2.0 ** k * (-1.0 if r % 2 else 1.0)
            src[o + r * rl:o + (r + 1) * rl] = row
            kinds.append((ti, r, kind))
    return src, kinds


def ref_qrows(src, ent, total, nscale):
    """(dst uint8 [total] with the sentinel in the gaps, scale fp32 [nscale])."""
    dst = torch.full((total,), SENT_U8, dtype=torch.uint8)
    scale = torch.zeros(nscale)
    for o, so, rows, rl in ent:
        sc, q = rows_ref(src[o:o + rows * rl].float().view(rows, rl))
        dst[o:o + rows * rl] = q.reshape(-1)
        scale[so:so + rows] = sc
    return dst, scale


# (K, C, R, S, cpad): R*S*Cp of 8 (zero fill from C = 3), 72, and 4 * 256 + 4 (the store loop's second trip)
WFP8_SHAPES = [(5, 3, 1, 1, 8), (9, 8, 3, 3, 0), (6, 1021, 1, 1, 1028), (12, 40, 3, 3, 48)]


def wfp8_data(k, c, r, s, seed=0):
    """fp32 [K, C, R, S]: ordinary values, output channel 1 all zero, channel 0 with amax 448 * 2^-6."""
    gen = torch.Generator().manual_seed(7000 + seed)
    w = torch.randn(k, c, r, s, generator=gen) * 0.1
    w[1] = 0.0
    w[0] = torch.randint(-447, 448, (c, r, s), generator=gen).float() * 2.0 ** -6
    w[0, c // 2, r // 2, s // 2] = -448.0 * 2.0 ** -6
    return w


def ref_wfp8(w, cpad, act_deq):
    """(codes uint8 [K, R, S, Cp], oscale fp32 [K]) of pack_weight_fp8 in its own fp32 arithmetic."""
    k, c, r, s = w.shape
    cp = max(cpad, c)
    x = w.permute(0, 2, 3, 1).reshape(k, -1).contiguous()
    sc, q = rows_ref(x)
    out = torch.zeros(k, r, s, cp, dtype=torch.uint8)
    out[..., :c] = q.view(k, r, s, c)
    osc = sc * (act_deq if act_deq is not None else torch.tensor(1.0))
    return out, osc
