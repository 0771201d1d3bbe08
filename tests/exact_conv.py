"""Integer operands, fp64 references and a bitwise comparison for the implicit-GEMM convolutions.

Small integers are exact in bf16, e4m3 and e5m2; their products, and fp32 sums of them in ANY order,
are exact while the sum of magnitudes stays below 2^24; and the bf16 rounding of an exact fp32 value
is the same on both sides.  So every output element of every kernel path (any K order, split-K order
or atomic order) has exactly one right answer, and a test can use ``torch.equal``.

This module is a helper, not a test file: ``int_operands`` builds the operands as the kernels take
them plus fp64 copies, ``ref_fwd`` / ``ref_dgrad`` / ``ref_wgrad`` are plain fp64 im2col + matmul
references (no fp32 BLAS anywhere: exactness must not rest on a library's choice of precision), the
``require_*`` functions assert the premises on the reference (so a test never passes or fails because
a premise silently broke), and ``assert_exact`` says WHERE a mismatch sits.

Shapes are ``(N, H, W, C, K, R, S, stride, pad)`` throughout; activations are NHWC, weights
``[K, C, R, S]``.
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

EXACT_LIMIT = float(2 ** 24)   # integers below this survive any-order fp32 accumulation
BF16_EXACT = 256.0             # every integer of magnitude <= 256 is a bf16 value
FP8_MAX_INT = 4                # 0..4 are exact in e4m3 (3 mantissa bits) and e5m2 (2 mantissa bits)


class PremiseError(AssertionError):
    """A premise of the exactness argument does not hold for these operands."""


def out_hw(shape):
    n, h, w, c, k, r, s, st, pd = shape
    return (h + 2 * pd - r) // st + 1, (w + 2 * pd - s) // st + 1


def to_bf16(t):
    """Round an fp64 reference the way the kernels store it: through fp32 (exact below 2^24), then RNE."""
    return t.float().to(torch.bfloat16)


def rel_err(a, b):
    """The whole-tensor metric of test_kernels_gpu.py / test_tiles_gpu.py (asserted ``< 1e-2`` there)."""
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


# ------------------------------------------------------------------ premises
def require_integers(t, dtype, what, max_abs=None):
    """``t`` (fp64) holds integers that ``dtype`` represents exactly (and |t| <= max_abs)."""
    if not torch.equal(t, t.round()):
        raise PremiseError(f"{what}: not integer-valued")
    if not torch.equal(t.float().to(dtype).double(), t):
        raise PremiseError(f"{what}: max |v| = {t.abs().max().item():.0f} is not exact in {dtype}")
    if max_abs is not None and t.numel() and t.abs().max().item() > max_abs:
        raise PremiseError(f"{what}: max |v| = {t.abs().max().item():.0f} > {max_abs}")


def require_below(t, limit, what):
    """max(t) < limit for a tensor of non-negative magnitude sums."""
    top = t.max().item() if t.numel() else 0.0
    if not top < limit:
        raise PremiseError(f"{what}: {top:.4g} is not below {limit:.4g}")


def require_stat_sums(y, group_rows, what):
    """Premises of exact fp32 statistics over ``y`` [M, K] (fp64): the stored bf16 value is the exact
    one (max |y| <= 256, so summing before or after the rounding agrees) and sum |y| over every group
    of ``group_rows`` rows is below 2^24 (``group_rows=None``: the whole tensor, one accumulator)."""
    require_integers(y, torch.bfloat16, what, BF16_EXACT)
    mag = y.abs()
    if group_rows is None:
        require_below(mag.sum(0), EXACT_LIMIT, f"{what}: whole-tensor sum |term|")
    else:
        require_below(group_sums(mag, group_rows), EXACT_LIMIT, f"{what}: sum |term| per {group_rows}-row group")


# ------------------------------------------------------------------ operands
def _randint(g, lohi, size):
    lo, hi = lohi
    return torch.randint(lo, hi + 1, size, generator=g).double()


def int_operands(shape, x_range=(-1, 1), w_range=(-2, 2), seed=0, device="cpu", dy_range=None, fp8=False):
    """Integer-valued operands of one convolution as the kernels take them, plus fp64 copies.

    x [N,H,W,C] and dy [N,Ho,Wo,K] are bf16 NHWC; w is fp32 [K,C,R,S] in channels_last; xd / wd /
    dyd are their fp64 copies.  ``fp8=True`` adds the uint8 views of fp8 tensors cast directly from
    the integers (no quantizer, so the bytes are known): x8 e4m3 [N,H,W,C], dy8 e5m2 [N,Ho,Wo,K],
    wq8 e4m3 [K,R,S,C] (forward) and wt8 e4m3 [C,R,S,K] (dgrad), all of magnitude at most 4.
    The premises on the operands are asserted here; ranges a type cannot hold raise PremiseError."""
    n, h, w, c, k, r, s, st, pd = shape
    ho, wo = out_hw(shape)
    g = torch.Generator().manual_seed(seed)
    xd = _randint(g, x_range, (n, h, w, c))
    wd = _randint(g, w_range, (k, c, r, s))
    dyd = _randint(g, dy_range or x_range, (n, ho, wo, k))
    lim = FP8_MAX_INT if fp8 else None
    require_integers(xd, torch.float8_e4m3fn if fp8 else torch.bfloat16, "x", lim)
    require_integers(dyd, torch.float8_e5m2 if fp8 else torch.bfloat16, "dy", lim)
    require_integers(wd, torch.float8_e4m3fn if fp8 else torch.bfloat16, "w", lim)
    o = SimpleNamespace(shape=tuple(shape), xd=xd.to(device), wd=wd.to(device), dyd=dyd.to(device))
    o.x = o.xd.to(torch.bfloat16)
    o.dy = o.dyd.to(torch.bfloat16)
    o.w = o.wd.float().contiguous(memory_format=torch.channels_last)
    if fp8:
        o.x8 = o.xd.float().to(torch.float8_e4m3fn).view(torch.uint8).contiguous()
        o.dy8 = o.dyd.float().to(torch.float8_e5m2).view(torch.uint8).contiguous()
        o.wq8 = o.wd.float().permute(0, 2, 3, 1).contiguous().to(torch.float8_e4m3fn).view(torch.uint8)
        o.wt8 = o.wd.float().permute(1, 2, 3, 0).contiguous().to(torch.float8_e4m3fn).view(torch.uint8)
    return o


def int_tensor(size, lohi, seed, device="cpu", dtype=torch.bfloat16):
    """An integer-valued tensor in [lo, hi] (addends, BN inputs, gradient sinks) and its fp64 copy."""
    d = _randint(torch.Generator().manual_seed(seed), lohi, tuple(size)).to(device)
    require_integers(d, dtype, "int_tensor")
    return d.to(dtype), d


# ---------------------------------------------------------------- references
_CHUNK_BYTES = 128 << 20   # im2col columns held at a time


def _cols(xd, shape, n0, n1):
    """im2col of images n0..n1 of NHWC xd: [n1-n0, C*R*S, Ho*Wo] (channel-major rows, as F.unfold)."""
    n, h, w, c, k, r, s, st, pd = shape
    return F.unfold(xd[n0:n1].permute(0, 3, 1, 2), (r, s), padding=pd, stride=st)


def _chunks(shape):
    n, h, w, c, k, r, s, st, pd = shape
    ho, wo = out_hw(shape)
    per = max(1, _CHUNK_BYTES // max(1, c * r * s * ho * wo * 8))
    return [(i, min(n, i + per)) for i in range(0, n, per)]


def ref_fwd(xd, wd, shape):
    """y [N,Ho,Wo,K] in fp64: im2col by F.unfold, then an fp64 matmul."""
    n, h, w, c, k, r, s, st, pd = shape
    ho, wo = out_hw(shape)
    wm = wd.reshape(k, c * r * s)
    out = [(wm @ _cols(xd, shape, a, b)).permute(0, 2, 1) for a, b in _chunks(shape)]
    return torch.cat(out).reshape(n, ho, wo, k)


def ref_dgrad(dyd, wd, shape):
    """dx [N,H,W,C] in fp64: the transposed matmul, then col2im (F.fold sums the overlapping taps)."""
    n, h, w, c, k, r, s, st, pd = shape
    ho, wo = out_hw(shape)
    wm_t = wd.reshape(k, c * r * s).t()
    out = []
    for a, b in _chunks(shape):
        dcols = wm_t @ dyd[a:b].reshape(b - a, ho * wo, k).permute(0, 2, 1)
        out.append(F.fold(dcols, (h, w), (r, s), padding=pd, stride=st).permute(0, 2, 3, 1))
    return torch.cat(out).contiguous()


def ref_wgrad(dyd, xd, shape, drop_last_rows=0):
    """dw [K,C,R,S] in fp64: dy^T x im2col(x), summed over the N*Ho*Wo reduction rows.
    ``drop_last_rows``: leave the last rows of the reduction out (a corruption for the CPU tests)."""
    n, h, w, c, k, r, s, st, pd = shape
    ho, wo = out_hw(shape)
    dym = dyd.reshape(n * ho * wo, k)
    if drop_last_rows:
        dym = dym.clone()
        dym[n * ho * wo - drop_last_rows:] = 0
    dym = dym.reshape(n, ho * wo, k)
    dw = torch.zeros(k, c * r * s, dtype=torch.float64, device=xd.device)
    for a, b in _chunks(shape):
        dw += (dym[a:b].permute(0, 2, 1) @ _cols(xd, shape, a, b).permute(0, 2, 1)).sum(0)
    return dw.reshape(k, c, r, s)


def exact_fwd(o):
    """Forward reference of ``int_operands`` output with its accumulation premise asserted."""
    require_below(ref_fwd(o.xd.abs(), o.wd.abs(), o.shape), EXACT_LIMIT, "fwd: sum |x||w| per output")
    return ref_fwd(o.xd, o.wd, o.shape)


def exact_dgrad(o):
    require_below(ref_dgrad(o.dyd.abs(), o.wd.abs(), o.shape), EXACT_LIMIT, "dgrad: sum |dy||w| per output")
    return ref_dgrad(o.dyd, o.wd, o.shape)


def exact_wgrad(o, sink=None):
    mag = ref_wgrad(o.dyd.abs(), o.xd.abs(), o.shape)
    if sink is not None:
        mag = mag + sink.abs()
    require_below(mag, EXACT_LIMIT, "wgrad: sum |dy||x| (+ |sink|) per output")
    dw = ref_wgrad(o.dyd, o.xd, o.shape)
    return dw if sink is None else dw + sink


# ---------------------------------------------------------------- statistics
def group_sums(y, rows):
    """Per-group column sums of y [M, K] over consecutive groups of ``rows`` rows, ragged last group
    included: [ceil(M / rows), K]."""
    m, k = y.shape
    g = (m + rows - 1) // rows
    pad = g * rows - m
    if pad:
        y = torch.cat([y, y.new_zeros(pad, k)])
    return y.reshape(g, rows, k).sum(1)


def group_m2(y, rows):
    """Per-group sum of squared deviations from the GROUP mean, in the dtype of y (fp64): [G, K]."""
    m, k = y.shape
    g = (m + rows - 1) // rows
    cnt = torch.full((g, 1), float(rows), dtype=y.dtype, device=y.device)
    cnt[-1, 0] = m - (g - 1) * rows
    s, q = group_sums(y, rows), group_sums(y * y, rows)
    return q - s * s / cnt


# ------------------------------------------------------------------- borders
def fwd_border(shape):
    """border_fn for forward outputs: GEMM row (n, ho, wo) -> True where a filter tap leaves the image."""
    n, h, w, c, k, r, s, st, pd = shape
    ho, wo = out_hw(shape)

    def fn(rows):
        i, j = (rows // wo) % ho, rows % wo
        return (i * st - pd < 0) | (i * st - pd + r > h) | (j * st - pd < 0) | (j * st - pd + s > w)
    return fn


def dgrad_border(shape):
    """border_fn for dgrad outputs: NHWC pixel (n, h, w) -> True where it lies within a filter's reach of
    an image edge (some of the taps that would touch it fall outside dy)."""
    n, h, w, c, k, r, s, st, pd = shape

    def fn(rows):
        i, j = (rows // w) % h, rows % w
        return (i < r - 1) | (i > h - r) | (j < s - 1) | (j > w - s)
    return fn


# ---------------------------------------------------------------- comparison
def _hist(v, top=8):
    vals, cnt = torch.unique(v, return_counts=True)
    order = torch.argsort(cnt, descending=True)[:top]
    return {int(vals[i]): int(cnt[i]) for i in order}


def assert_exact(got, want, row_tile=None, col_tile=None, border_fn=None, what=""):
    """``torch.equal(got, want)`` over [..., columns] tensors read as a GEMM output [rows, columns].
    On a mismatch the message gives the number of wrong elements, the first eight coordinates with both
    values, and counts by ``row % row_tile``, ``col % col_tile``, border / interior pixel
    (``border_fn(rows) -> bool``) and 64-channel block -- where to look in the kernel."""
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype} != {want.dtype}"
    if torch.equal(got, want):
        return
    ncol = got.shape[-1]
    g2, w2 = got.reshape(-1, ncol), want.reshape(-1, ncol)
    bad = (g2 != w2) | (g2.isnan() != w2.isnan())
    rows, cols = bad.nonzero(as_tuple=True)
    first = [(int(r_), int(c_), float(g2[r_, c_]), float(w2[r_, c_])) for r_, c_ in zip(rows[:8], cols[:8])]
    msg = [f"{what}: {rows.numel()} of {bad.numel()} elements differ in a [{g2.shape[0]}, {ncol}] output",
           f"first (row, col, got, want): {first}",
           f"wrong rows: {torch.unique(rows).numel()}, wrong columns: {torch.unique(cols).numel()}"]
    if row_tile:
        msg.append(f"by row % {row_tile}: {_hist(rows % row_tile)}; by row tile: {_hist(rows // row_tile)}")
    if col_tile:
        msg.append(f"by col % {col_tile}: {_hist(cols % col_tile)}; by column tile: {_hist(cols // col_tile)}")
    if border_fn is not None:
        nb = int(border_fn(rows).sum())
        msg.append(f"border pixels: {nb}, interior pixels: {rows.numel() - nb}")
    msg.append(f"by 64-channel block: {_hist(cols // 64)}")
    raise AssertionError("\n".join(msg))
