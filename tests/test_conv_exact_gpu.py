"""Bit-exact tests of the implicit-GEMM convolutions on integer operands (helper: tests/exact_conv.py).

The whole-tensor metric of test_kernels_gpu.py / test_tiles_gpu.py / test_fp8_gpu.py cannot see a
localized error (tests/test_conv_exact_cpu.py shows it accepting a zeroed GEMM row).  Here the operands
are small integers: exact in bf16 / e4m3 / e5m2, with exact products and exact fp32 sums in any order
below 2^24, and one bf16 rounding of an exact value.  Every output element of every path -- any K
order, split-K order or atomic order -- therefore has one right answer, and the tests use
``torch.equal`` against a plain fp64 im2col reference, at small shapes that sit on the places these
kernels go wrong: the last partial row tile, a column tile ``Nout`` does not fill, pixels whose taps
cross an image border, stride-2 parity classes of unequal or zero size, the partial last K-step of
the generic-C loader, the tail of a split-K reduction.

Each case first asserts WHICH path runs (``conv_nt_tile`` / ``conv_wgrad_plan`` /
``conv_wgrad_fp8_plan``); the expected tiles and plans follow ``conv_nt_group_rows`` / ``plan_wg``.
A new tile, loader or epilogue gets a row in the tables below.  Shapes are (N,H,W,C,K,R,S,stride,pad).

The only tolerance in this file is the one on the forward M2 partials (``M2_RTOL``), which are not
integers; everything else is ``torch.equal`` or a one-ulp statement about an exact quotient.
"""
import pytest
import torch

import exact_conv as ec

pytestmark = pytest.mark.gpu

# Forward BN partials part[:, 1, :] (M2 about the group mean, formed per wave as q - s^2 / n and merged
# by Chan's formula): largest error found over every forward case below, relative to the group's sum
# of squares q (the quantity the fp32 roundings of q - s^2 / n scale with; relative to M2 itself a
# constant column would divide by zero).  Asserted at four times the measured value -- headroom for
# run-to-run differences in the wave merge order -- and never looser than the 1e-4 that
# test_tiles_gpu.py::test_fwd_bn_fused_finalize_matches_partials uses for these statistics.
M2_MEASURED = 1.15e-7   # MI355X: 1.149e-07 at (3,9,7,128,136,3,3,1,1); every other case below that
M2_RTOL = min(4 * M2_MEASURED, 1e-4)

_CACHE = {}


def _ops(gpu, shape, fp8=False):
    """Operands of one conv shape on the GPU, built once and shared by the tests of that shape (never
    modified).  bf16: x, dy in {-1, 0, 1}; w in {-2..2}, or {-1, 0, 1} for reductions above 1152 terms
    (at Kg = 2304 the wider range reaches |y| = 264, past the 256 the statistics premise allows).
    fp8: every operand in {-4..4}."""
    key = (shape, fp8)
    if key not in _CACHE:
        n, h, w, c, k, r, s, st, pd = shape
        if fp8:
            o = ec.int_operands(shape, (-4, 4), (-4, 4), seed=sum(shape), device=gpu, fp8=True)
        else:
            wr = (-2, 2) if r * s * max(c, k) <= 1152 else (-1, 1)
            o = ec.int_operands(shape, (-1, 1), wr, seed=sum(shape), device=gpu)
        _CACHE[key] = o
    return _CACHE[key]


def _ints(gpu, size, lohi, seed, dtype=torch.bfloat16):
    """ec.int_tensor on the GPU, built once per (size, range, seed) and shared (never modified)."""
    key = (tuple(size), lohi, seed, dtype)
    if key not in _CACHE:
        _CACHE[key] = ec.int_tensor(size, lohi, seed, gpu, dtype)
    return _CACHE[key]


def _ref(o, kind):
    """The exact fp64 result of ``kind`` (fwd / dgrad / wgrad) for operands ``o``, computed once."""
    if not hasattr(o, kind):
        setattr(o, kind, {"fwd": ec.exact_fwd, "dgrad": ec.exact_dgrad, "wgrad": ec.exact_wgrad}[kind](o))
    return getattr(o, kind)


def _loader(shape):
    """The A-operand loader launch_conv_fwd picks for a bf16 forward shape."""
    n, h, w, c, k, r, s, st, pd = shape
    if c % 64 or r * s > 32:
        return "generic"
    return "halo" if (r, s, st, pd, c) == (3, 3, 1, 1, 64) else "c64"


def _m_class0(shape):
    """GEMM rows of parity class (0, 0) of a dgrad (all of them at stride 1)."""
    n, h, w, c, k, r, s, st, pd = shape
    return n * ((h + st - 1) // st) * ((w + st - 1) // st)


# ------------------------------------------------------------------------------------------ forward
FWD_CASES = [
    # 64x128 tile (M <= 8192, K > 64)
    ((1, 5, 3, 64, 72, 3, 3, 1, 1), (64, 128), "halo"),        # M = 15 < BM, ragged Nout
    ((3, 9, 7, 128, 136, 3, 3, 1, 1), (64, 128), "c64"),       # per-tap loader, Nout = 128 + 8
    ((2, 7, 5, 64, 128, 1, 1, 2, 0), (64, 128), "c64"),        # 1x1 / s2, odd extents
    ((2, 9, 6, 128, 128, 3, 3, 2, 1), (64, 128), "c64"),       # 3x3 / s2, odd and even extents
    ((1, 2, 2, 64, 128, 3, 3, 1, 1), (64, 128), "halo"),       # image smaller than the filter
    ((1, 1, 67, 64, 128, 1, 1, 1, 0), (64, 128), "c64"),       # H = 1, M = BM + 3
    ((2, 6, 10, 24, 72, 3, 3, 1, 1), (64, 128), "generic"),    # Kg = 216: partial last K-step, taps packed across steps
    ((2, 6, 6, 8, 72, 7, 7, 2, 3), (64, 128), "generic"),      # 8 channels, 49 taps
    # 256x64 tile (K <= 64)
    ((3, 11, 9, 64, 64, 3, 3, 1, 1), (256, 64), "halo"),       # M = 256 + 41
    ((2, 13, 10, 128, 40, 1, 1, 1, 0), (256, 64), "c64"),      # ragged Nout = 40
    ((5, 8, 8, 192, 64, 3, 3, 2, 1), (256, 64), "c64"),        # stride 2
    # 128x128 tile (M = 8427 = 65 * 128 + 107)
    ((3, 53, 53, 64, 136, 1, 1, 1, 0), (128, 128), "c64"),     # run_ntq<2,2,2,2>
    ((3, 53, 53, 40, 136, 1, 1, 1, 0), (128, 128), "generic"),  # generic C on run_nt
    ((3, 53, 53, 64, 136, 3, 3, 1, 1), (128, 128), "halo"),
    # 128x256 short-K tile
    ((3, 53, 53, 128, 256, 1, 1, 1, 0), (128, 256), "c64"),
    # 256x256 tile (>= 196 blocks)
    ((9, 53, 53, 128, 264, 1, 1, 1, 0), (256, 256), "c64"),    # M = 98 * 256 + 193; second column tile holds 8 columns
    ((17, 55, 54, 64, 256, 3, 3, 1, 1), (256, 256), "halo"),   # M = 197 * 256 + 58
]
# K32 ring against K64 double buffer: one case per tile, both 256x256 cases, and a stride-2 one
K32_CASES = [FWD_CASES[i] for i in (1, 3, 9, 11, 14, 15, 16)]


def _check_fwd(C, o, tile, y, part, what):
    """y and the per-group integer sums of a forward call against the exact reference."""
    n, h, w, c, k, r, s, st, pd = o.shape
    y64 = _ref(o, "fwd").reshape(-1, k)
    M = y64.shape[0]
    ec.assert_exact(y.reshape(M, k), ec.to_bf16(y64), tile[0], tile[1], ec.fwd_border(o.shape), f"{what} y")
    # part[:, 0, :]: the sum of the STORED y over each group of BM rows, ragged last group included
    ec.require_stat_sums(y64, tile[0], f"{what} y")
    assert part.shape == ((M + tile[0] - 1) // tile[0], 2, k)
    ec.assert_exact(part[:, 0, :].double(), ec.group_sums(y64, tile[0]), None, tile[1], None, f"{what} group sums")
    return y64, M


@pytest.mark.parametrize("shape,tile,loader", FWD_CASES)
def test_fwd_exact_with_stats(gpu, native_ext, shape, tile, loader):
    """conv_fwd: y bit for bit, part[:, 0] the exact per-row-group sums, part[:, 1] (M2) within M2_RTOL
    of the fp64 M2 of the stored y; conv_fwd_bn(acc=): the same y, the accumulator back to zero, the mean
    within one fp32 ulp of exact_sum / M.

    M2: the largest error measured on an MI355X over all 17 cases is 1.149e-07 of the group's sum of
    squares, at (3,9,7,128,136,3,3,1,1); the next two are 1.017e-07 and 9.831e-08.  The bound is four
    times that (M2_RTOL = 4.6e-07)."""
    C = native_ext
    n, h, w, c, k, r, s, st, pd = shape
    o = _ops(gpu, shape)
    ho, wo = ec.out_hw(shape)
    assert tuple(C.conv_nt_tile(n * ho * wo, k, r * s * c * 2)) == tile
    assert _loader(shape) == loader
    wk = C.pack_weight(o.w, c)
    y, part = C.conv_fwd(o.x, wk, st, pd, True)
    y64, M = _check_fwd(C, o, tile, y, part, f"fwd {shape}")
    m2 = ec.group_m2(y64, tile[0])
    q = ec.group_sums(y64 * y64, tile[0])
    err = ((part[:, 1, :].double() - m2).abs() / q.clamp_min(1.0)).max().item()
    print(f"M2 relative error {shape}: {err:.3e}")
    assert err <= M2_RTOL, f"M2 partials off by {err:.3e} of the group's sum of squares"
    # BN finalize fused into the conv: fp64 totals of per-workgroup fp32 sums (exact: same premise)
    acc = torch.zeros(8, 2, k, dtype=torch.float64, device=gpu)
    ones, zeros = torch.ones(k, device=gpu), torch.zeros(k, device=gpu)
    y_b, stats = C.conv_fwd_bn(o.x, wk, st, pd, M, zeros.clone(), ones.clone(), ones, zeros, 0.1, 1e-5, acc)
    assert torch.equal(y_b, y)
    assert torch.count_nonzero(acc) == 0
    mean = (y64.sum(0) / M).float()   # fp64 sums of integers are exact; one rounding to fp32
    lo = torch.nextafter(mean, torch.full_like(mean, -float("inf")))
    hi = torch.nextafter(mean, torch.full_like(mean, float("inf")))
    assert bool(((stats[0] >= lo) & (stats[0] <= hi)).all()), (stats[0] - mean).abs().max().item()


@pytest.mark.parametrize("k32", [1, 0])
@pytest.mark.parametrize("shape,tile,loader", K32_CASES)
def test_fwd_exact_under_forced_k32_and_k64(gpu, native_ext, shape, tile, loader, k32):
    """The same exact answer with the K32 ring (k32 = 1) and the K64 double buffer (k32 = 0) pinned."""
    C = native_ext
    n, h, w, c, k, r, s, st, pd = shape
    assert c % 64 == 0
    o = _ops(gpu, shape)
    C.conv_nt_force(k32, -1, -1)
    try:
        ho, wo = ec.out_hw(shape)
        assert tuple(C.conv_nt_tile(n * ho * wo, k, r * s * c * 2)) == tile
        y, part = C.conv_fwd(o.x, C.pack_weight(o.w, c), st, pd, True)
        torch.cuda.synchronize()
    finally:
        C.conv_nt_force(-1, -1, -1)
    _check_fwd(C, o, tile, y, part, f"fwd k32={k32} {shape}")


def test_one_changed_input_element_is_seen(gpu, native_ext):
    """Negative control on the device: one input element of the last (corner) pixel raised by 1 moves
    only the outputs whose taps read it -- 4 of 189 GEMM rows, a norm ratio of 0.006 --
    and the comparison against the unchanged reference names exactly those elements."""
    C = native_ext
    shape, tile, _ = FWD_CASES[1]
    n, h, w, c, k, r, s, st, pd = shape
    o = _ops(gpu, shape)
    want = ec.to_bf16(_ref(o, "fwd")).reshape(-1, k)
    xd = o.xd.clone()
    xd[-1, -1, -1, -1] += 1
    want_mod = ec.to_bf16(ec.ref_fwd(xd, o.wd, shape)).reshape(-1, k)
    changed = want_mod != want
    rows = changed.any(1).nonzero().flatten().tolist()
    last = n * h * w - 1
    assert rows and set(rows) <= {last - w - 1, last - w, last - 1, last}
    y, _ = C.conv_fwd(xd.to(torch.bfloat16), C.pack_weight(o.w, c), st, pd, False)
    ec.assert_exact(y.reshape(-1, k), want_mod, tile[0], tile[1], ec.fwd_border(shape), "changed input")
    assert ec.rel_err(y.reshape(-1, k), want) < 1e-2   # the old metric accepts it
    with pytest.raises(AssertionError, match=f"{int(changed.sum())} of {changed.numel()} elements differ") as e:
        ec.assert_exact(y.reshape(-1, k), want, tile[0], tile[1], ec.fwd_border(shape), "changed input")
    nb = int(ec.fwd_border(shape)(changed.nonzero()[:, 0]).sum())   # pixel (7, 5) is interior, the other three are not
    assert 0 < nb < int(changed.sum())
    assert f"wrong rows: {len(rows)}," in str(e.value)
    assert f"border pixels: {nb}, interior pixels: {int(changed.sum()) - nb}" in str(e.value)


# -------------------------------------------------------------------------------------------- dgrad
def _swap(shape):
    """The forward shape with the channel roles swapped: its dgrad is the GEMM the forward was (same M,
    Nout and K at stride 1), so the dgrad reaches the tile and loader of that forward row."""
    n, h, w, c, k, r, s, st, pd = shape
    return (n, h, w, k, c, r, s, st, pd)


# (dgrad needs K % 64 == 0; C may be any multiple of 8)
DGRAD_CASES = [(_swap(sh), tile) for sh, tile, _ in FWD_CASES if sh[3] % 64 == 0] + [
    ((2, 7, 5, 72, 64, 1, 1, 2, 0), (64, 128)),     # unequal parity classes, ragged Nout = 72
    ((1, 1, 9, 64, 64, 3, 3, 2, 1), (256, 64)),     # H = 1: the ph = 1 classes are empty
    ((2, 13, 11, 64, 64, 3, 3, 2, 1), (256, 64)),
]
# dgrad on the halo loader: the forward list's own row, which is its own swap
assert ((3, 11, 9, 64, 64, 3, 3, 1, 1), (256, 64)) in DGRAD_CASES
_BN_PER_TILE = [(3, 9, 7, 136, 128, 3, 3, 1, 1), (3, 11, 9, 64, 64, 3, 3, 1, 1), (3, 53, 53, 136, 64, 1, 1, 1, 0),
                (3, 53, 53, 256, 128, 1, 1, 1, 0), (17, 55, 54, 256, 64, 3, 3, 1, 1)]
# one case per tile and every stride-2 case
DGRAD_BN_CASES = [(sh, t) for sh, t in DGRAD_CASES if sh[7] == 2 or sh in _BN_PER_TILE]


def _dgrad_tile_is(C, shape, tile):
    n, h, w, c, k, r, s, st, pd = shape
    assert k % 64 == 0 and c % 8 == 0
    assert tuple(C.conv_nt_tile(_m_class0(shape), c, r * s * k * 2)) == tile


def _addends(gpu, shape):
    """(label, addend as passed, its full-resolution fp64 value): none, a full-resolution integer
    addend, and for stride 2 the compact [N, ceil(H/2), ceil(W/2), C] map of even pixels."""
    n, h, w, c, k, r, s, st, pd = shape
    full, full_d = _ints(gpu, (n, h, w, c), (-3, 3), 101)
    out = [("none", None, None), ("full", full, full_d)]
    if st == 2:
        comp, comp_d = _ints(gpu, (n, (h + 1) // 2, (w + 1) // 2, c), (-3, 3), 102)
        spread = torch.zeros_like(full_d)
        spread[:, ::2, ::2, :] = comp_d
        out.append(("compact", comp, spread))
    return out


def _dx_plus(o, add_d, what):
    """Exact dx (+ addend).  The epilogue stages dx as bf16 before it adds: with |dx| <= 256 that
    staging is exact, so the sum is rounded once on both sides."""
    dx64 = _ref(o, "dgrad")
    if add_d is None:
        return dx64
    ec.require_integers(dx64, torch.bfloat16, what, ec.BF16_EXACT)
    return dx64 + add_d


@pytest.mark.parametrize("shape,tile", DGRAD_CASES)
def test_dgrad_exact(gpu, native_ext, shape, tile):
    C = native_ext
    n, h, w, c, k, r, s, st, pd = shape
    _dgrad_tile_is(C, shape, tile)
    o = _ops(gpu, shape)
    for label, add, add_d in _addends(gpu, shape):
        want = ec.to_bf16(_dx_plus(o, add_d, f"dgrad {shape}"))
        dx = C.conv_dgrad(o.dy, o.w, [n, h, w, c], st, pd, add)
        ec.assert_exact(dx, want, tile[0] if st == 1 else None, tile[1], ec.dgrad_border(shape),
                        f"dgrad {shape} addend={label}")


def _bitmask(z):
    bits = (z.reshape(-1, 8) > 0).to(torch.int32) << torch.arange(8, device=z.device, dtype=torch.int32)
    return bits.sum(1).to(torch.uint8)


@pytest.mark.parametrize("mask", [0, 1, 2, 3])
@pytest.mark.parametrize("shape,tile", DGRAD_BN_CASES)
def test_dgrad_bn_exact(gpu, native_ext, shape, tile, mask):
    """BN-fused dgrad: g = where(mask, dx (+ addend), 0) bit for bit in every mask mode -- y * scale +
    shift is exact in any FMA order and never zero here, so the recomputed mask (2) is bitwise too --
    and sums = (sum g, sum g * (y - mean)) the exact integers, from the partials + reduce path and from
    the fp32-atomic [2, C] accumulator."""
    C = native_ext
    n, h, w, c, k, r, s, st, pd = shape
    _dgrad_tile_is(C, shape, tile)
    o = _ops(gpu, shape)
    dims = (n, h, w, c)
    y, y_d = _ints(gpu, dims, (-2, 2), 201)
    z, z_d = _ints(gpu, dims, (-2, 2), 202)
    z, z_d = torch.relu(z), torch.relu(z_d)                      # an integer ReLU output
    _, mean_d = ec.int_tensor((c,), (-1, 1), 203, gpu, torch.float32)
    _, sgn = ec.int_tensor((c,), (0, 1), 204, gpu, torch.float32)
    _, mag = ec.int_tensor((c,), (1, 2), 205, gpu, torch.float32)
    scale_d = (2 * sgn - 1) * mag                                # +-1, +-2
    shift_d = ec.int_tensor((c,), (-2, 2), 206, gpu, torch.float32)[1] + 0.5
    stats = torch.stack([mean_d, torch.ones_like(mean_d), scale_d, shift_d]).float().contiguous()
    pre = y_d * scale_d + shift_d
    assert bool((pre != 0).all()) and torch.equal(pre.float().double(), pre)
    on = {0: torch.ones_like(pre, dtype=torch.bool), 1: z_d > 0, 2: pre > 0, 3: z_d > 0}[mask]
    zin = {0: None, 1: z, 2: None, 3: _bitmask(z)}[mask]
    for label, add, add_d in _addends(gpu, shape)[:2]:
        what = f"dgrad_bn {shape} mask={mask} addend={label}"
        g_want = ec.to_bf16(torch.where(on, _dx_plus(o, add_d, what), 0.0))
        gs = g_want.double().reshape(-1, c)                     # the sums are of the STORED g
        yc = (y_d - mean_d).reshape(-1, c)
        # the kernel forms sum g*y and mean * sum g separately, each in fp32: both exact below 2^24
        ec.require_below(gs.abs().sum(0) * (1 + mean_d.abs()), ec.EXACT_LIMIT, f"{what}: sum |g| (1 + |mean|)")
        ec.require_below((gs.abs() * y_d.reshape(-1, c).abs()).sum(0), ec.EXACT_LIMIT, f"{what}: sum |g||y|")
        sums_want = torch.stack([gs.sum(0), (gs * yc).sum(0)]).float()
        g1, sums = C.conv_dgrad_bn(o.dy, o.w, list(dims), st, pd, add, y, zin, stats, mask)
        ec.assert_exact(g1, g_want, tile[0] if st == 1 else None, tile[1], ec.dgrad_border(shape), what)
        ec.assert_exact(sums, sums_want, None, tile[1], None, f"{what} sums (partials)")
        acc = torch.zeros(2, c, device=gpu)
        g2, sa = C.conv_dgrad_bn(o.dy, o.w, list(dims), st, pd, add, y, zin, stats, mask, acc=acc)
        assert sa.data_ptr() == acc.data_ptr()
        ec.assert_exact(g2, g_want, tile[0] if st == 1 else None, tile[1], ec.dgrad_border(shape), f"{what} (acc)")
        ec.assert_exact(acc, sums_want, None, tile[1], None, f"{what} sums (acc)")


# ---------------------------------------------------------------------------------- weight gradient
WGRAD_CASES = [
    # (shape, bm, bn, split)      bn = 192: the halo kernel's 3 taps x 64 channels
    ((3, 5, 7, 64, 256, 1, 1, 1, 0), 256, 64, False),       # pointwise loader, reduction 105 = 64 + 41
    ((2, 9, 5, 136, 72, 1, 1, 1, 0), 128, 128, False),      # pointwise, ragged both ways
    ((1, 3, 3, 64, 64, 1, 1, 1, 0), 64, 256, False),        # pointwise, reduction of 9 rows
    ((2, 9, 6, 128, 128, 3, 3, 2, 1), 128, 128, False),     # general loader
    ((4, 14, 13, 72, 40, 3, 3, 2, 1), 64, 256, False),
    ((2, 7, 5, 64, 128, 1, 1, 2, 0), 128, 128, False),
    ((1, 2, 2, 64, 128, 3, 3, 1, 1), 128, 128, False),      # image smaller than the filter
    ((1, 3, 5, 64, 64, 3, 3, 1, 1), 64, 192, False),        # halo kernel
    ((3, 9, 5, 128, 64, 3, 3, 1, 1), 64, 192, False),
    ((2, 14, 13, 192, 64, 3, 3, 1, 1), 64, 192, False),
    ((16, 28, 27, 128, 128, 3, 3, 1, 1), 128, 128, True),   # reduction 12,096 = 189 * 64: uneven splits
    ((15, 28, 27, 64, 256, 1, 1, 1, 0), 256, 64, True),     # 11,340 rows = 177 * 64 + 12: ragged tail in the last split
]


def _krsc(dw):
    """[K, C, R, S] -> the weight-gradient GEMM's [K, R*S*C] output."""
    return dw.permute(0, 2, 3, 1).reshape(dw.shape[0], -1)


@pytest.mark.parametrize("shape,bm,bn,split", WGRAD_CASES)
def test_wgrad_exact(gpu, native_ext, shape, bm, bn, split):
    """conv_wgrad three ways: atomic split-K (twice: both exact), deterministic slabs, and accumulated
    into an integer-valued KRSC sink -- all the one exact integer answer."""
    C = native_ext
    n, h, w, c, k, r, s, st, pd = shape
    o = _ops(gpu, shape)
    ws = [k, c, r, s]
    for det in (False, True):
        plan = C.conv_wgrad_plan([n, h, w, c], ws, st, pd, det)
        assert (plan["bm"], plan["bn"]) == (bm, bn)
        assert (plan["splits"] > 1) if split else True, plan
    want = _ref(o, "wgrad").float()
    for det, rep in ((False, 0), (False, 1), (True, 0)):
        dw = C.conv_wgrad(o.dy, o.x, ws, st, pd, det)
        assert dw.shape == want.shape and dw.is_contiguous(memory_format=torch.channels_last)
        ec.assert_exact(_krsc(dw), _krsc(want), bm, bn, None, f"wgrad {shape} det={det} run {rep}")
    _, sink_d = ec.int_tensor((k, r, s, c), (-50, 50), 301, gpu, torch.float32)
    want_sink = ec.exact_wgrad(o, sink_d.permute(0, 3, 1, 2)).float()
    for det in (False, True):
        sink = sink_d.float().permute(0, 3, 1, 2)   # a KRSC-dense [K, C, R, S] view
        C.conv_wgrad(o.dy, o.x, ws, st, pd, det, sink)
        ec.assert_exact(_krsc(sink), _krsc(want_sink), bm, bn, None, f"wgrad {shape} det={det} into a sink")


# ---------------------------------------------------------------------------------------------- fp8
def _pow2(gpu, n, lo=-1):
    """Per-channel powers of two 2^lo, 2^(lo+1), 2^(lo+2), ... repeating: exact scale factors."""
    return (2.0 ** (torch.arange(n, device=gpu) % 3 + lo)).float()


@pytest.mark.parametrize("shape,tile,loader", [
    ((2, 9, 7, 128, 136, 3, 3, 1, 1), (64, 128), "c128"),
    ((2, 9, 7, 48, 72, 3, 3, 1, 1), (64, 128), "generic"),
    # conv_nt_tile answers for bf16 operands (the 128x256 tile has bf16 kernels only): the fp8 kernel runs
    # 128x128 here, with the same 128-row groups
    ((3, 53, 53, 128, 256, 1, 1, 1, 0), (128, 256), "c128"),
])
def test_fp8_fwd_exact(gpu, native_ext, shape, tile, loader):
    C = native_ext
    n, h, w, c, k, r, s, st, pd = shape
    ho, wo = ec.out_hw(shape)
    assert tuple(C.conv_nt_tile(n * ho * wo, k, r * s * c)) == tile   # fp8: the K bytes are the K elements
    assert ("c128" if c % 128 == 0 and r * s <= 32 else "generic") == loader
    o = _ops(gpu, shape, fp8=True)
    oscale = _pow2(gpu, k)
    ascale = torch.tensor([0.25], device=gpu)
    want = ec.to_bf16(_ref(o, "fwd") * oscale.double() * 0.25)
    bn = 128 if tile == (128, 256) else tile[1]   # the column tile the fp8 kernel runs (diagnostics)
    for stats in (False, True):
        y, _ = C.conv_fwd_fp8(o.x8, o.wq8, oscale, st, pd, stats, ascale)
        ec.assert_exact(y, want, tile[0], bn, ec.fwd_border(shape), f"fp8 fwd {shape} stats={stats}")


@pytest.mark.parametrize("shape,tile", [
    ((2, 9, 6, 72, 128, 3, 3, 2, 1), (64, 128)),
    ((2, 9, 7, 64, 64, 3, 3, 1, 1), (256, 64)),      # the narrow 64-channel dgrad on the generic loader
    ((3, 53, 53, 136, 128, 1, 1, 1, 0), (128, 128)),
])
def test_fp8_dgrad_exact(gpu, native_ext, shape, tile):
    C = native_ext
    n, h, w, c, k, r, s, st, pd = shape
    assert tuple(C.conv_nt_tile(_m_class0(shape), c, r * s * k)) == tile
    o = _ops(gpu, shape, fp8=True)
    wscale = _pow2(gpu, c, -2)
    ascale = torch.tensor([0.5], device=gpu)
    want = ec.to_bf16(_ref(o, "dgrad") * wscale.double() * 0.5)
    dx = C.conv_dgrad_fp8(o.dy8, o.wt8, wscale, ascale, [n, h, w, c], st, pd)
    ec.assert_exact(dx, want, tile[0] if st == 1 else None, tile[1], ec.dgrad_border(shape), f"fp8 dgrad {shape}")


@pytest.mark.parametrize("shape,bm", [
    ((3, 5, 7, 64, 256, 1, 1, 1, 0), 128),
    ((8, 7, 7, 128, 128, 3, 3, 1, 1), 128),          # reduction 392, not a multiple of the 128-pixel step
    ((2, 9, 6, 128, 128, 3, 3, 2, 1), 128),
    ((2, 9, 5, 48, 64, 3, 3, 1, 1), 64),
])
def test_fp8_wgrad_exact(gpu, native_ext, shape, bm):
    C = native_ext
    n, h, w, c, k, r, s, st, pd = shape
    ws = [k, c, r, s]
    assert C.conv_wgrad_fp8_plan([n, h, w, c], ws, st, pd)["bm"] == bm
    o = _ops(gpu, shape, fp8=True)
    dq, xq = torch.tensor([0.25], device=gpu), torch.tensor([0.5], device=gpu)
    want = (_ref(o, "wgrad") * 0.125).float()
    dw = C.conv_wgrad_fp8(0, o.dy8, o.x8, dq, xq, ws, st, pd)
    ec.assert_exact(_krsc(dw), _krsc(want), bm, 128, None, f"fp8 wgrad {shape}")
    _, sink_d = ec.int_tensor((k, r, s, c), (-50, 50), 302, gpu, torch.float32)
    want_sink = (ec.exact_wgrad(o, 8 * sink_d.permute(0, 3, 1, 2)) * 0.125).float()   # premise in units of 1/8
    sink = sink_d.float().permute(0, 3, 1, 2)
    C.conv_wgrad_fp8(0, o.dy8, o.x8, dq, xq, ws, st, pd, sink)
    ec.assert_exact(_krsc(sink), _krsc(want_sink), bm, 128, None, f"fp8 wgrad {shape} into a sink")
