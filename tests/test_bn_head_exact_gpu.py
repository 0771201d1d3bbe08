"""Bit-exact tests of the BatchNorm, pooling, folded-BN and head kernels (helper: tests/exact_bn.py).

The whole-tensor metrics of test_kernels_gpu.py cannot see a localized error in these kernels
(tests/test_bn_head_exact_cpu.py shows them accepting a zeroed 8-channel vector, a row that lost its bias
and a dropped pooled window).  Here the activations are small integers and the per-channel coefficients
are crafted -- powers of two, integers and half-integers -- so that every fp32 intermediate is exact
in any association or FMA contraction and the bf16 store is the one rounding (ties included) of one right
answer: the comparisons are ``torch.equal`` / ``ec.assert_exact`` against plain fp64 references.  Where
the row count M is no power of two, 1 / M is rounded and the backward apply is held to the bf16
neighbours of the reference under a DERIVED slack (``eb.assert_bf16_neighbour``: five fp32 roundings,
at most 1 % of elements off the rounded reference); the average pool at HW = 15 likewise.  No tolerance
in this file is tuned to a kernel's output.

Each case reads: operands -> which path -> one call -> exact compare.  Shapes are (N, H, W, K); they sit
on the places these kernels go wrong: one vector, K / 8 = 5 (a grid rounded to a multiple of 5 blocks),
fewer rows than a block, the channel-chunked reduction grid, rows no multiple of the row-block count,
pool windows clipped on odd extents, ragged GEMM tiles, split-K tails, misaligned operands.  A new BN /
pool / fold / head kernel variant gets a row in the tables below.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import exact_bn as eb
import exact_conv as ec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def _ints(gpu, size, lohi, seed, dtype=torch.bfloat16):
    """ec.int_tensor on the GPU, built once per (size, range, seed, dtype) and shared (never modified)."""
    key = (tuple(size), lohi, seed, dtype)
    if key not in _CACHE:
        _CACHE[key] = ec.int_tensor(size, lohi, seed, gpu, dtype)
    return _CACHE[key]


def _coefs(gpu, k, m, seed=0):
    """Crafted coefficients where M is a power of two, ordinary real ones (neighbour rule) elsewhere."""
    key = ("coefs", k, m, seed)
    if key not in _CACHE:
        _CACHE[key] = eb.craft(k, m, seed, gpu) if (m & (m - 1)) == 0 else eb.generic(k, m, seed, gpu)
    return _CACHE[key]


def _f32(t):
    eb.require_fp32(t, "fp32 operand")
    return t.float().contiguous()


# ------------------------------------------------------------------------------------ BN forward
FWD_SHAPES = [
    (3, 5, 7, 64),
    (2, 3, 5, 40),      # K / 8 = 5: the grid is rounded up to a multiple of 5 blocks
    (1, 1, 1, 8),       # one vector
    (2, 4, 4, 2048),
]
# every instantiation launch_bn_act_fwd reaches: (residual, relu, mask, residual BN)
FWD_FORMS = {
    "plain": (False, False, False, False),
    "relu": (False, True, False, False),
    "res": (True, False, False, False),
    "res_relu": (True, True, False, False),
    "res_mask": (True, True, True, False),
    "mask": (False, True, True, False),
    "resbn": (True, False, False, True),
    "resbn_relu": (True, True, False, True),
    "resbn_mask": (True, True, True, True),
}


@pytest.mark.parametrize("form", list(FWD_FORMS))
@pytest.mark.parametrize("nhwk", FWD_SHAPES)
def test_bn_fwd_exact(gpu, native_ext, nhwk, form):
    """z bit for bit (y * scale + shift lands on bf16 ties and on exactly 0), the residual's own BN
    rounded to bf16 before the add, and bit j of the mask byte = stored z > 0."""
    C = native_ext
    res, relu, mask, resbn = FWD_FORMS[form]
    k = nhwk[3]
    y, yd = _ints(gpu, nhwk, (-20, 20), 1)
    r, rd = _ints(gpu, nhwk, (-20, 20), 2) if res else (None, None)
    scale, shift = eb.craft_fwd(k, 3, gpu)
    rsc, rsh = eb.craft_fwd(k, 4, gpu) if resbn else (None, None)
    want = eb.ref_bn_fwd(yd, scale, shift, rd, relu, rsc, rsh)
    if yd.numel() >= 1000:   # not vacuous: the operands reach an exact 0 before the ReLU and a rounding at the store
        assert int((eb.bn_fwd64(yd, scale, shift, rd, False, rsc, rsh) == 0).sum()) > 0
        assert int((want.double() != eb.bn_fwd64(yd, scale, shift, rd, relu, rsc, rsh)).sum()) > 0
    args = (y, _f32(scale), _f32(shift), r)
    rargs = (_f32(rsc), _f32(rsh)) if resbn else (None, None)
    if mask:
        z, zm = C.bn_act_fwd_mask(*args, *rargs)
        assert torch.equal(zm, eb.bitmask(want > 0)), f"mask bytes {nhwk} {form}"
    else:
        z = C.bn_act_fwd(*args, relu, *rargs)
    ec.assert_exact(z, want, None, None, None, f"bn_act_fwd {nhwk} {form}")


@pytest.mark.parametrize("nhwk", FWD_SHAPES)
def test_bn_fwd_column_sums_exact(gpu, native_ext, nhwk):
    """The column-sum form (legal when 256 % (K / 8) == 0): the same z, the slots summing to the exact
    sum of the STORED z, a second call doubling it; K = 40 raises."""
    C = native_ext
    k = nhwk[3]
    y, yd = _ints(gpu, nhwk, (-20, 20), 1)
    scale, shift = eb.craft_fwd(k, 3, gpu)
    cs = torch.zeros(C.bn_csum_slots(), k, device=gpu)
    if 256 % (k // 8):
        with pytest.raises(RuntimeError, match="column sums"):
            C.bn_act_fwd(y, _f32(scale), _f32(shift), None, True, None, None, cs)
        return
    want = eb.ref_bn_fwd(yd, scale, shift, None, True)
    tot = eb.ref_csum(want)
    eb.require_lattice_sum(2 * want.double().reshape(-1, k).abs().sum(0), eb.lattice_unit(want.double()), "two calls")
    z = C.bn_act_fwd(y, _f32(scale), _f32(shift), None, True, None, None, cs)
    ec.assert_exact(z, want, None, None, None, f"bn_act_fwd csum {nhwk}")
    ec.assert_exact(cs.double().sum(0, keepdim=True), tot[None], None, None, None, f"column sums {nhwk}")
    C.bn_act_fwd(y, _f32(scale), _f32(shift), None, True, None, None, cs)
    ec.assert_exact(cs.double().sum(0, keepdim=True), 2 * tot[None], None, None, None, f"column sums twice {nhwk}")


# ----------------------------------------------------------------------------- BN backward reduce
RED_SHAPES = [
    (3, 5, 7, 64),
    (1, 1, 31, 256),    # fewer rows than one block's 32
    (2, 3, 3, 2048),    # channel-chunked grid, stage-2 CH = 32
    (4, 16, 17, 128),   # 1088 rows: not divisible by the row-block count
]


def _saved_z(gpu, nhwk, seed):
    z, zd = _ints(gpu, nhwk, (-2, 2), seed)
    return torch.relu(z), torch.relu(zd)            # an integer ReLU output


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("nhwk", RED_SHAPES)
def test_bn_bwd_reduce_exact(gpu, native_ext, nhwk, mode):
    """sums = (sum g, sum g (y - mu)): exact integers in every mask mode, and the dgamma / dbeta sinks
    hold sink + s1 * invstd and sink + s0 exactly."""
    C = native_ext
    k = nhwk[3]
    c = _coefs(gpu, k, 1024, seed=10)               # the reduce reads mean, scale, shift and invstd only
    dz, dzd = _ints(gpu, nhwk, (-3, 3), 11)
    y, yd = _ints(gpu, nhwk, (-4, 4), 12)
    z, zd = _saved_z(gpu, nhwk, 13)
    on = eb.mask_on(mode, zd, yd, c.scale, c.shift)
    want = eb.ref_bwd_reduce(dzd, yd, c.mu, on)
    sums = C.bn_act_bwd_reduce(dz, z, y, c.stats, mode)
    ec.assert_exact(sums, want.float(), None, None, None, f"bn_act_bwd_reduce {nhwk} mask={mode}")
    _, dg0 = _ints(gpu, (k,), (-50, 50), 14, torch.float32)
    _, db0 = _ints(gpu, (k,), (-50, 50), 15, torch.float32)
    dg, db = dg0.float(), db0.float()
    sums2 = C.bn_act_bwd_reduce(dz, z, y, c.stats, mode, dg, db)
    assert torch.equal(sums2, sums)
    dg_want, db_want = _f32(dg0 + want[1] * c.invstd), _f32(db0 + want[0])
    ec.assert_exact(dg[None], dg_want[None], None, None, None, f"dgamma sink {nhwk} mask={mode}")
    ec.assert_exact(db[None], db_want[None], None, None, None, f"dbeta sink {nhwk} mask={mode}")


@pytest.mark.parametrize("nhwk", RED_SHAPES[:2])
def test_bn_bwd_reduce_modes_1_and_2_agree_at_exact_zero(gpu, native_ext, nhwk):
    """Where y * scale + shift is exactly 0 the mask is off in both modes: from the saved z (mode 1) and
    recomputed from y (mode 2) -- a `>=` in either would move the sums."""
    C = native_ext
    k = nhwk[3]
    c = _coefs(gpu, k, 1024, seed=10)
    dz, dzd = _ints(gpu, nhwk, (1, 3), 16)          # positive: a wrongly opened mask always shows
    y, yd = _ints(gpu, nhwk, (-4, 4), 12)
    z = eb.ref_bn_fwd(yd, c.scale, c.shift, None, True)
    pre = yd * c.scale + c.shift
    assert int((pre == 0).sum()) > 0
    want = eb.ref_bwd_reduce(dzd, yd, c.mu, pre > 0)
    assert not torch.equal(want, eb.ref_bwd_reduce(dzd, yd, c.mu, pre >= 0))
    s1 = C.bn_act_bwd_reduce(dz, z, y, c.stats, 1)
    s2 = C.bn_act_bwd_reduce(dz, z, y, c.stats, 2)
    ec.assert_exact(s1, want.float(), None, None, None, f"mode 1 {nhwk}")
    ec.assert_exact(s2, want.float(), None, None, None, f"mode 2 {nhwk}")


def test_bn_bwd_reduce_rejects_40_channels(gpu, native_ext):
    C = native_ext
    nhwk = (2, 3, 5, 40)
    c = _coefs(gpu, 40, 1024, seed=10)
    dz, _ = _ints(gpu, nhwk, (-3, 3), 11)
    with pytest.raises(RuntimeError):
        C.bn_act_bwd_reduce(dz, dz, dz, c.stats, 0)


# ------------------------------------------------------------------------------ BN backward apply
APPLY_SHAPES = [
    (2, 4, 8, 64),      # M = 64
    (1, 2, 2, 40),      # M = 4, K / 8 = 5
    (4, 8, 8, 2048),    # M = 256
    (3, 5, 7, 64),      # M = 105: neighbour rule
    (2, 3, 5, 40),      # M = 30: neighbour rule
]


@pytest.mark.parametrize("mask", [0, 1, 2])
@pytest.mark.parametrize("nhwk", APPLY_SHAPES)
def test_bn_bwd_apply_exact(gpu, native_ext, nhwk, mask):
    """dy = k1 (g - sgm - (y - mu) k2) bit for bit on crafted coefficients at a power-of-two M, within
    the bf16 neighbours of the fp64 reference elsewhere; evaluation mode (k1 g) and dres (= g) likewise,
    dres always bit for bit."""
    C = native_ext
    n, h, w, k = nhwk
    c = _coefs(gpu, k, n * h * w, seed=20)
    dz, dzd = _ints(gpu, nhwk, (-200, 200), 21)
    y, yd = _ints(gpu, nhwk, (-20, 20), 22)
    z, zd = _saved_z(gpu, nhwk, 23)
    on = eb.mask_on(mask, zd, yd, c.scale, c.shift)
    slack = eb.bwd_apply_slack(c, dzd, yd, on)
    for training in (True, False):
        ref = eb.exact_bwd_apply if c.exact else eb.ref_bwd_apply
        want, g = ref(c, dzd, yd, on, training)
        for want_dres in (True, False):
            what = f"bn_act_bwd_apply {nhwk} mask={mask} training={training} dres={want_dres}"
            dy, dres = C.bn_act_bwd_apply(dz, z, y, c.stats, c.gamma, c.sums, mask, training, want_dres)
            if c.exact:
                ec.assert_exact(dy, eb.to_bf16(want), None, None, None, what)
            else:
                eb.assert_bf16_neighbour(dy, want, slack, what)
            if want_dres:
                ec.assert_exact(dres, eb.to_bf16(g), None, None, None, what + " dres")
            else:
                assert dres is None
    if c.exact:
        _, dg0 = _ints(gpu, (k,), (-50, 50), 24, torch.float32)
        _, db0 = _ints(gpu, (k,), (-50, 50), 25, torch.float32)
        dg, db = dg0.float(), db0.float()
        dy2, _ = C.bn_act_bwd_apply(dz, z, y, c.stats, c.gamma, c.sums, mask, True, False, dg, db)
        ec.assert_exact(dy2, eb.to_bf16(eb.exact_bwd_apply(c, dzd, yd, on)[0]), None, None, None, "with sinks")
        dg_want, db_want = eb.ref_sinks(c, dg0, db0)
        ec.assert_exact(dg[None], dg_want[None], None, None, None, f"dgamma sink {nhwk}")
        ec.assert_exact(db[None], db_want[None], None, None, None, f"dbeta sink {nhwk}")


def test_crafted_apply_rounds_at_the_store(gpu):
    """The exact cases above are not vacuous: the crafted dy needs more than bf16's 8 bits."""
    nhwk = APPLY_SHAPES[0]
    c = _coefs(gpu, nhwk[3], 64, seed=20)
    _, dzd = _ints(gpu, nhwk, (-200, 200), 21)
    _, yd = _ints(gpu, nhwk, (-20, 20), 22)
    want, _ = eb.exact_bwd_apply(c, dzd, yd, torch.ones_like(yd, dtype=torch.bool))
    assert int((eb.to_bf16(want).double() != want).sum()) > 0


def test_one_changed_gradient_element_is_seen(gpu, native_ext):
    """Negative control on the device: one element of dz replaced moves exactly that element of dy, and the
    comparison against the unchanged reference names it."""
    C = native_ext
    nhwk = APPLY_SHAPES[0]
    n, h, w, k = nhwk
    c = _coefs(gpu, k, n * h * w, seed=20)
    dz, dzd = _ints(gpu, nhwk, (-200, 200), 21)
    y, yd = _ints(gpu, nhwk, (-20, 20), 22)
    on = eb.mask_on(0, None, yd, c.scale, c.shift)
    want = eb.to_bf16(eb.exact_bwd_apply(c, dzd, yd, on)[0])
    dzd2 = dzd.clone()
    dzd2[-1, -1, -1, -1] = 200.0 if dzd[-1, -1, -1, -1] <= 0 else -200.0
    want2 = eb.to_bf16(eb.exact_bwd_apply(c, dzd2, yd, on)[0])
    assert int((want2 != want).sum()) == 1
    dy, _ = C.bn_act_bwd_apply(dzd2.to(torch.bfloat16), dz, y, c.stats, c.gamma, c.sums, 0, True, False)
    ec.assert_exact(dy, want2, None, None, None, "changed dz")
    with pytest.raises(AssertionError, match=f"1 of {dy.numel()} elements differ") as e:
        ec.assert_exact(dy, want, None, None, None, "changed dz")
    assert f"first (row, col, got, want): [({n * h * w - 1}, {k - 1}," in str(e.value)


# -------------------------------------------------------------------- capped grid, a fresh process
_CAP_SCRIPT = r"""
import json, sys, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from pytorch_distributed_tutorials_amd.ops import native
import exact_bn as eb
import exact_conv as ec
C = native()
dev = torch.device("cuda:0")
out = {}
for nhwk in [(4, 64, 64, 40), (8, 64, 65, 64)]:
    n, h, w, k = nhwk
    M = n * h * w
    c = eb.craft(k, M, 50, dev) if (M & (M - 1)) == 0 else eb.generic(k, M, 50, dev)
    y, yd = ec.int_tensor(nhwk, (-20, 20), 51, dev)
    r, rd = ec.int_tensor(nhwk, (-20, 20), 52, dev)
    dz, dzd = ec.int_tensor(nhwk, (-200, 200), 53, dev)
    sc, sh = c.scale.float().contiguous(), c.shift.float().contiguous()
    res = {"exact": bool(c.exact)}
    # forward, residual + mask (cap 32768 by default) against the fp64 reference
    zw = eb.ref_bn_fwd(yd, c.scale, c.shift, rd, True)
    z, zm = C.bn_act_fwd_mask(y, sc, sh, r)
    res["fwd_res_mask_z"] = int((z != zw).sum())
    res["fwd_res_mask_bits"] = int((zm != eb.bitmask(zw > 0)).sum())
    # plain forward
    zp = C.bn_act_fwd(y, sc, sh, None, False)
    res["fwd_plain"] = int((zp != eb.ref_bn_fwd(yd, c.scale, c.shift, None, False)).sum())
    # backward apply, mask from the (reference's) saved z, with dres
    on = zw.double() > 0
    want, g = (eb.exact_bwd_apply if c.exact else eb.ref_bwd_apply)(c, dzd, yd, on)
    dy, dres = C.bn_act_bwd_apply(dz, zw, y, c.stats, c.gamma, c.sums, 1, True, True)
    res["dres"] = int((dres != eb.to_bf16(g)).sum())
    if c.exact:
        res["dy"], res["dy_share"] = int((dy != eb.to_bf16(want)).sum()), 0.0
    else:
        res["dy"], res["dy_share"] = eb.neighbour_report(dy, want, eb.bwd_apply_slack(c, dzd, yd, on))
    out["x".join(map(str, nhwk))] = res
torch.cuda.synchronize()
print(json.dumps(out))
"""


def test_bn_streaming_passes_exact_at_a_capped_grid(gpu):
    """PDT_EW_BLOCKS=256: (4,64,64,40) has 81,920 vectors for a 260-block grid (two grid-stride
    iterations, the second partial) and (8,64,65,64) runs four full iterations and a partial fifth.  The
    forward residual + mask pass, the plain forward and the backward apply (mask 1, dres) against the
    fp64 reference, inside one fresh process that counts the mismatches."""
    env = dict(os.environ)
    env["PDT_EW_BLOCKS"] = "256"
    r = subprocess.run([sys.executable, "-c", _CAP_SCRIPT, ROOT], env=env, capture_output=True, text=True,
                       timeout=110)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(out) == {"4x64x64x40", "8x64x65x64"} and out["4x64x64x40"]["exact"] and not out["8x64x65x64"]["exact"]
    for key, res in out.items():
        for name in ("fwd_res_mask_z", "fwd_res_mask_bits", "fwd_plain", "dres", "dy"):
            assert res[name] == 0, (key, name, res)
        assert res["dy_share"] <= eb.NEIGHBOUR_CAP, (key, res)


# ------------------------------------------------------------------------------------ pool family
POOL_SHAPES = [
    (2, 17, 16, 64),    # odd H: the last window row is clipped
    (1, 1, 1, 64),      # one pixel: every window is clipped to it
    (3, 2, 9, 64),
    (2, 7, 8, 8),       # one vector per pixel
]


@pytest.mark.parametrize("nhwc", POOL_SHAPES)
def test_maxpool_exact(gpu, native_ext, nhwc):
    """Values, argmax bytes under the first-maximum rule (inputs in 0..3: ties everywhere) and dx."""
    C = native_ext
    n, h, w, c = nhwc
    x, xd = _ints(gpu, nhwc, (0, 3), 30)
    val, bi = eb.ref_maxpool(xd)
    y, idx = C.maxpool_fwd(x)
    ec.assert_exact(y, val.to(torch.bfloat16), None, None, None, f"maxpool_fwd {nhwc}")
    ec.assert_exact(idx, bi, None, None, None, f"maxpool_fwd argmax {nhwc}")
    dy, dyd = _ints(gpu, tuple(val.shape), (-3, 3), 31)
    dx = C.maxpool_bwd(dy, bi, h, w)
    ec.assert_exact(dx, eb.to_bf16(eb.ref_maxpool_bwd(dyd, bi, h, w)), None, None, None, f"maxpool_bwd {nhwc}")


@pytest.mark.parametrize("argmax_y", [False, True])
@pytest.mark.parametrize("nhwc", POOL_SHAPES)
def test_bn_relu_maxpool_exact(gpu, native_ext, nhwc, argmax_y):
    """The fused stem pool against the reference composition (not against the unfused kernels)."""
    C = native_ext
    k = nhwc[3]
    y, yd = _ints(gpu, nhwc, (-20, 20), 32)
    scale, shift = eb.craft_fwd(k, 33, gpu)
    out_w, bi, u_w = eb.ref_bn_relu_maxpool(yd, scale, shift)
    got = C.bn_relu_maxpool(y, _f32(scale), _f32(shift), argmax_y)
    assert len(got) == (3 if argmax_y else 2)
    ec.assert_exact(got[0], out_w, None, None, None, f"bn_relu_maxpool {nhwc}")
    ec.assert_exact(got[1], bi, None, None, None, f"bn_relu_maxpool argmax {nhwc}")
    if argmax_y:
        ec.assert_exact(got[2], u_w, None, None, None, f"bn_relu_maxpool u {nhwc}")


@pytest.mark.parametrize("nhwk", [(2, 16, 16, 64), (3, 17, 15, 64)])
def test_pool_bn_bwd_exact(gpu, native_ext, nhwk):
    """The stem's BN backward with the pooled gradient gathered on the fly: sums and sinks exact; dy exact
    at M = 512, within the bf16 neighbours at M = 765 (odd extents: clipped quads)."""
    C = native_ext
    n, h, w, k = nhwk
    M = n * h * w
    y, yd = _ints(gpu, nhwk, (-20, 20), 34)
    cr = _coefs(gpu, k, 1024, seed=35)              # the reduce: integer mean, any M
    _, bi, _ = eb.ref_bn_relu_maxpool(yd, cr.scale, cr.shift)
    dp, dpd = _ints(gpu, tuple(bi.shape), (-60, 60), 36)
    dzd = eb.ref_maxpool_bwd(dpd, bi, h, w)         # never rounded: the kernels gather in fp32
    on = eb.mask_on(2, None, yd, cr.scale, cr.shift)
    want = eb.ref_bwd_reduce(dzd, yd, cr.mu, on)
    sums = C.pool_bn_bwd_reduce(dp, bi, y, cr.stats)
    ec.assert_exact(sums, want.float(), None, None, None, f"pool_bn_bwd_reduce {nhwk}")
    _, dg0 = _ints(gpu, (k,), (-50, 50), 37, torch.float32)
    _, db0 = _ints(gpu, (k,), (-50, 50), 38, torch.float32)
    dg, db = dg0.float(), db0.float()
    assert torch.equal(C.pool_bn_bwd_reduce(dp, bi, y, cr.stats, dg, db), sums)
    ec.assert_exact(dg[None], _f32(dg0 + want[1] * cr.invstd)[None], None, None, None, f"dgamma sink {nhwk}")
    ec.assert_exact(db[None], _f32(db0 + want[0])[None], None, None, None, f"dbeta sink {nhwk}")
    # the apply: coefficients of this M, the same crafted scale / shift (so the same mask and argmax)
    c = _coefs(gpu, k, M, seed=35)
    assert torch.equal(c.scale, cr.scale) and torch.equal(c.shift, cr.shift)
    slack = eb.bwd_apply_slack(c, dzd, yd, on)
    for training in (True, False):
        want_dy, _ = (eb.exact_bwd_apply if c.exact else eb.ref_bwd_apply)(c, dzd, yd, on, training)
        dy = C.pool_bn_bwd_apply(dp, bi, y, c.stats, c.gamma, c.sums, training)
        what = f"pool_bn_bwd_apply {nhwk} training={training}"
        if c.exact:
            ec.assert_exact(dy, eb.to_bf16(want_dy), None, None, None, what)
        else:
            eb.assert_bf16_neighbour(dy, want_dy, slack, what)


# ------------------------------------------------------------------------------------------- fold
FOLD_COUNT = 1024       # the fold ops' `count` is independent of the tensors' row count


def _fold_weights(gpu, c_, k, seed):
    """The fp64 copy of the transposed weights wt [C, K]: integers in -1..1."""
    _, wtd = _ints(gpu, (c_, k), (-1, 1), seed)
    return wtd


@pytest.mark.parametrize("c_,k", [(64, 256), (128, 512), (32, 256)])
def test_bn_fold_weights_exact(gpu, native_ext, c_, k):
    """wfold = [bf16(wt k1) | bf16(G)] and bias = wt b against the fp64 reference: wt k1 exactly, G one
    rounding of an exact fp32 sum, the bias an exact sum; some a = 0 and mixed signs."""
    C = native_ext
    c = _coefs(gpu, k, FOLD_COUNT, seed=40)
    assert int((c.a == 0).sum()) > 0 and int((c.a > 0).sum()) > 0 and int((c.a < 0).sum()) > 0
    wtd = _fold_weights(gpu, c_, k, 41)
    w = wtd.t().float().reshape(k, c_, 1, 1).contiguous(memory_format=torch.channels_last)
    wt = C.pack_weight_t(w).view(c_, k)
    assert torch.equal(wt.double(), wtd)
    wfold_w, bias_w, G = eb.ref_fold_weights(wtd, c)
    wfold, bias = C.bn_fold_weights(wt, c.stats, c.gamma, c.sums, FOLD_COUNT)
    assert wfold.shape == (c_, k + c_) and bias.shape == (c_,)
    ec.assert_exact(wfold[:, :k].contiguous(), eb.to_bf16(wtd * c.k1), None, 64, None, f"wfold[:, :K] {c_, k}")
    ec.assert_exact(wfold[:, k:].contiguous(), eb.to_bf16(G), 32, 32, None, f"wfold[:, K:] {c_, k}")
    ec.assert_exact(bias[None], _f32(bias_w)[None], None, 32, None, f"bias {c_, k}")


def test_bn_fold_weights_rejects_k_not_multiple_of_256(gpu, native_ext):
    C = native_ext
    c = _coefs(gpu, 128, FOLD_COUNT, seed=40)
    wt = _ints(gpu, (64, 128), (-1, 1), 41)[0]
    with pytest.raises(RuntimeError, match="K % 256"):
        C.bn_fold_weights(wt, c.stats, c.gamma, c.sums, FOLD_COUNT)


FOLD_DGRAD_CASES = [
    # (n, h, w, C, K), tile of the [M, C] GEMM over K + C
    ((1, 3, 5, 64, 256), (256, 64)),           # M = 15 < BM
    ((1, 1, 259, 64, 256), (256, 64)),         # M = BM + 3
    ((1, 1, 67, 128, 256), (64, 128)),         # M = BM + 3
    ((3, 53, 53, 128, 256), (128, 128)),       # M = 8427 = 65 * 128 + 107
    ((3, 53, 53, 256, 256), (128, 256)),       # short K: K + C = 512
    ((17, 55, 54, 256, 512), (256, 256)),      # M = 197 * 256 + 58
]


def _fold_prev_unit(gpu, dims, c_):
    """(y_prev bf16, its fp64 copy, scale, shift) of the unit whose BN the epilogue reduces (mask mode 2).
    Up to 1024 rows: integers in -4..4 under a crafted scale / shift (about half the mask on, exact zeros
    included).  Above: the mask is on for 1 element in 128 (y_prev in {1, 2} there, -4 elsewhere, scale 1,
    shift -0.5), so that the whole-column fp32 sums of |dx| up to a few hundred stay below 2^24 units."""
    if dims[0] * dims[1] * dims[2] <= 1024:
        y_prev, ypd = _ints(gpu, dims, (-4, 4), 44)
        return (y_prev, ypd) + eb.craft_fwd(c_, 45, gpu)
    _, pick = _ints(gpu, dims, (0, 127), 44)
    _, val = _ints(gpu, dims, (1, 2), 47)
    ypd = torch.where(pick == 0, val, -4.0)
    one = torch.ones(c_, dtype=torch.float64, device=gpu)
    return ypd.to(torch.bfloat16), ypd, one, -0.5 * one


@pytest.mark.parametrize("shape,tile", FOLD_DGRAD_CASES)
def test_conv_dgrad_bn_fold_exact(gpu, native_ext, shape, tile):
    """dx = mask([g | x] wfold^T + bias) bit for bit from the reference's own wfold and bias -- the bias
    on rows < M only, the loader's switch from g to x at k = K, at ragged tiles.  Mask mode 0 shows every
    element of dx; mask mode 2 on a crafted y_prev the masked dx and the epilogue's BN sums, exact from
    the accumulator and from the partials path."""
    C = native_ext
    n, h, w, c_, k = shape
    M = n * h * w
    assert tuple(C.conv_nt_tile(M, c_, (k + c_) * 2)) == tile
    c = _coefs(gpu, k, FOLD_COUNT, seed=40)
    wfold, bias_d, _ = eb.ref_fold_weights(_fold_weights(gpu, c_, k, 41), c)
    bias = _f32(bias_d)
    g, gd = _ints(gpu, (n, h, w, k), (-1, 1), 42)
    x, xd = _ints(gpu, (n, h, w, c_), (0, 2), 43)
    y_prev, ypd, sc, sh = _fold_prev_unit(gpu, (n, h, w, c_), c_)
    _, mean_d = _ints(gpu, (c_,), (-1, 1), 46, torch.float32)
    st_prev = torch.stack([mean_d, torch.ones_like(mean_d), sc, sh]).float().contiguous()
    want_all = eb.ref_fold_dgrad(gd.reshape(M, k), xd.reshape(M, c_), wfold, bias_d, torch.ones(M, c_, dtype=torch.bool,
                                                                                               device=gpu))
    dx0, _ = C.conv_dgrad_bn_fold(g, x, wfold, bias, y_prev, None, st_prev, 0, torch.zeros(2, c_, device=gpu))
    ec.assert_exact(dx0.reshape(M, c_), want_all, tile[0], tile[1], None, f"conv_dgrad_bn_fold {shape} mask=0")
    on = eb.mask_on(2, None, ypd, sc, sh).reshape(M, c_)
    want = torch.where(on, want_all, torch.zeros_like(want_all))
    sums_want = eb.ref_bn_sums(want, ypd.reshape(M, c_), mean_d)
    acc = torch.zeros(2, c_, device=gpu)
    dx, sa = C.conv_dgrad_bn_fold(g, x, wfold, bias, y_prev, None, st_prev, 2, acc)
    assert sa.data_ptr() == acc.data_ptr()
    ec.assert_exact(dx.reshape(M, c_), want, tile[0], tile[1], None, f"conv_dgrad_bn_fold {shape}")
    ec.assert_exact(acc, sums_want, None, tile[1], None, f"conv_dgrad_bn_fold {shape} sums (acc)")
    dx2, sums = C.conv_dgrad_bn_fold(g, x, wfold, bias, y_prev, None, st_prev, 2)
    ec.assert_exact(dx2.reshape(M, c_), want, tile[0], tile[1], None, f"conv_dgrad_bn_fold {shape} (partials)")
    ec.assert_exact(sums, sums_want, None, tile[1], None, f"conv_dgrad_bn_fold {shape} sums (partials)")


def test_one_changed_bias_channel_is_seen(gpu, native_ext):
    """Negative control on the device: the fold bias of one channel raised by 1 moves that column of dx
    only, and the comparison against the unchanged reference names the column."""
    C = native_ext
    (n, h, w, c_, k), tile = FOLD_DGRAD_CASES[2]
    M = n * h * w
    c = _coefs(gpu, k, FOLD_COUNT, seed=40)
    wfold, bias_d, _ = eb.ref_fold_weights(_fold_weights(gpu, c_, k, 41), c)
    g, gd = _ints(gpu, (n, h, w, k), (-1, 1), 42)
    x, xd = _ints(gpu, (n, h, w, c_), (0, 2), 43)
    y_prev, ypd, sc, sh = _fold_prev_unit(gpu, (n, h, w, c_), c_)
    st_prev = torch.stack([torch.zeros_like(sc), torch.ones_like(sc), sc, sh]).float().contiguous()
    on = torch.ones(M, c_, dtype=torch.bool, device=gpu)
    want = eb.ref_fold_dgrad(gd.reshape(M, k), xd.reshape(M, c_), wfold, bias_d, on)
    bias2 = bias_d.clone()
    bias2[5] += 1.0
    want2 = eb.ref_fold_dgrad(gd.reshape(M, k), xd.reshape(M, c_), wfold, bias2, on)
    changed = want2 != want
    assert int(changed.sum()) > M // 2 and changed.any(0).nonzero().flatten().tolist() == [5]
    dx, _ = C.conv_dgrad_bn_fold(g, x, wfold, _f32(bias2), y_prev, None, st_prev, 0, torch.zeros(2, c_, device=gpu))
    ec.assert_exact(dx.reshape(M, c_), want2, tile[0], tile[1], None, "changed bias")
    with pytest.raises(AssertionError, match=f"{int(changed.sum())} of {M * c_} elements differ") as e:
        ec.assert_exact(dx.reshape(M, c_), want, tile[0], tile[1], None, "changed bias")
    assert "wrong columns: 1" in str(e.value) and f"by col % {tile[1]}: {{5: {int(changed.sum())}}}" in str(e.value)


def _fold_wgrad_operands(gpu, c_, k):
    c = _coefs(gpu, k, FOLD_COUNT, seed=40)
    wt, wtd = _ints(gpu, (c_, k), (-1, 1), 41)
    _, t1 = _ints(gpu, (k, c_), (-8, 8), 47, torch.float32)
    _, gram = _ints(gpu, (c_, c_), (0, 8), 48, torch.float32)
    _, out0 = _ints(gpu, (k, c_), (-50, 50), 49, torch.float32)
    return c, wt, wtd, t1, gram, out0


@pytest.mark.parametrize("c_,k", [(64, 64), (128, 256)])
def test_bn_fold_wgrad_exact(gpu, native_ext, c_, k):
    """out = out0 + k1 T1 + a (W Gram) + b (x) colsum exactly, with one column-sum vector; dgamma / dbeta
    exact; the operands untouched without the completion counter."""
    C = native_ext
    c, wt, wtd, t1d, gramd, out0 = _fold_wgrad_operands(gpu, c_, k)
    _, csd = _ints(gpu, (c_,), (-20, 20), 50, torch.float32)
    want = _f32(eb.ref_fold_wgrad(out0, t1d, gramd, csd, wtd, c))
    _, dg0 = _ints(gpu, (k,), (-50, 50), 51, torch.float32)
    _, db0 = _ints(gpu, (k,), (-50, 50), 52, torch.float32)
    t1, gram, out, dg, db = t1d.float(), gramd.float(), out0.float(), dg0.float(), db0.float()
    C.bn_fold_wgrad(t1, gram, csd.float(), wt, c.stats, c.gamma, c.sums, FOLD_COUNT, out, dg, db)
    ec.assert_exact(out, want, 64, 64, None, f"bn_fold_wgrad {c_, k}")
    dg_want, db_want = eb.ref_sinks(c, dg0, db0)
    ec.assert_exact(dg[None], dg_want[None], None, None, None, "dgamma")
    ec.assert_exact(db[None], db_want[None], None, None, None, "dbeta")
    assert torch.equal(t1.double(), t1d) and torch.equal(gram.double(), gramd)


@pytest.mark.parametrize("c_,k", [(64, 64), (128, 256)])
def test_bn_fold_wgrad_consume_mode_exact_and_rezeroed(gpu, native_ext, c_, k):
    """Consume mode over bn_act_fwd's column-sum slots, twice over the same workspaces: the exact result
    both times, and t1, gram, the slots, sums (zero_sums) and the counters all zero afterwards."""
    C = native_ext
    c, wt, wtd, t1d, gramd, out0 = _fold_wgrad_operands(gpu, c_, k)
    S = C.bn_csum_slots()
    _, slotsd = _ints(gpu, (S, c_), (-2, 2), 53, torch.float32)
    want = _f32(eb.ref_fold_wgrad(out0, t1d, gramd, slotsd.sum(0), wtd, c))
    t1, gram, slots = torch.zeros(k, c_, device=gpu), torch.zeros(c_, c_, device=gpu), torch.zeros(S, c_, device=gpu)
    sums, done = torch.zeros(2, k, device=gpu), torch.zeros(c_ // 64 + 1, dtype=torch.int32, device=gpu)
    outs = []
    for run in range(2):
        t1.copy_(t1d), gram.copy_(gramd), slots.copy_(slotsd), sums.copy_(c.sums)
        out = out0.float()
        C.bn_fold_wgrad(t1, gram, slots, wt, c.stats, c.gamma, sums, FOLD_COUNT, out, None, None, done, True)
        ec.assert_exact(out, want, 64, 64, None, f"bn_fold_wgrad consume {c_, k} run {run}")
        for t, name in ((t1, "t1"), (gram, "gram"), (slots, "slots"), (sums, "sums"), (done, "done")):
            assert int(torch.count_nonzero(t)) == 0, f"{name} not re-zeroed after run {run}"
        outs.append(out)
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------- head
FC_SHAPES = [
    (7, 72, 33),        # row stride 33: dlogits on scalar loads; K = 72 has a partial last step
    (65, 96, 130),      # one row and two columns past a tile
    (3, 2048, 10),      # split-K forward (8 slices), bias added by the reduce
    (64, 64, 1000),     # split-K dgrad over V: 2 slices of 512, the last ragged (488)
]


def _fc_check(C, gpu, n, c_, v, p, pd, w, wd, what):
    b, bd = _ints(gpu, (v,), (-2, 2), 62, torch.float32)
    dl, dld = _ints(gpu, (n, v), (-2, 2), 63, torch.float32)
    logits_w, dp_w, dw_w, db_w = eb.ref_linear(pd, wd, bd, dld)
    logits = C.fc_forward(p, w, b)
    ec.assert_exact(logits, logits_w.float(), 64, 64, None, f"fc_forward {what}")
    dp, dw, db = C.fc_backward(dl, p, w)
    assert dp.shape == (eb.fc_split_count(n, c_, v), n, c_)
    ec.assert_exact(dp.double().sum(0), dp_w, 64, 64, None, f"fc_backward dp {what}")
    ec.assert_exact(dw, dw_w.float(), 64, 64, None, f"fc_backward dw {what}")
    ec.assert_exact(db[None], db_w.float()[None], None, 64, None, f"fc_backward db {what}")
    _, dw0 = _ints(gpu, (v, c_), (-50, 50), 64, torch.float32)
    _, db0 = _ints(gpu, (v,), (-50, 50), 65, torch.float32)
    dw1, db1 = dw0.float(), db0.float()
    C.fc_backward(dl, p, w, dw1, db1)
    ec.assert_exact(dw1, (dw0 + dw_w).float(), 64, 64, None, f"fc_backward dw into a sink {what}")
    ec.assert_exact(db1[None], (db0 + db_w).float()[None], None, 64, None, f"fc_backward db into a sink {what}")
    dw2 = dw0.float()
    _, _, db2 = C.fc_backward(dl, p, w, dw2, None)      # dW accumulated, db fresh: the column-sum kernel
    ec.assert_exact(dw2, (dw0 + dw_w).float(), 64, 64, None, f"fc_backward dw sink only {what}")
    ec.assert_exact(db2[None], db_w.float()[None], None, 64, None, f"fc_backward db fresh {what}")


@pytest.mark.parametrize("n,c_,v", FC_SHAPES)
def test_fc_exact(gpu, native_ext, n, c_, v):
    C = native_ext
    assert (eb.fc_split_count(n, v, c_) > 1) == ((n, c_, v) == (3, 2048, 10))
    assert (eb.fc_split_count(n, c_, v) > 1) == ((n, c_, v) == (64, 64, 1000))
    p, pd = _ints(gpu, (n, c_), (-2, 2), 60, torch.float32)
    w, wd = _ints(gpu, (v, c_), (-2, 2), 61, torch.float32)
    _fc_check(C, gpu, n, c_, v, p, pd, w, wd, f"{n, c_, v}")


def test_fc_exact_on_misaligned_views(gpu, native_ext):
    """pooled and the weights as views one element into a larger buffer: no operand is 16-byte aligned,
    so every load takes the scalar path launch_fc_gemm documents."""
    C = native_ext
    n, c_, v = 7, 72, 33
    _, pd = _ints(gpu, (n, c_), (-2, 2), 60, torch.float32)
    _, wd = _ints(gpu, (v, c_), (-2, 2), 61, torch.float32)
    pbuf, wbuf = torch.zeros(n * c_ + 1, device=gpu), torch.zeros(v * c_ + 1, device=gpu)
    p, w = pbuf[1:].view(n, c_), wbuf[1:].view(v, c_)
    p.copy_(pd), w.copy_(wd)
    assert p.data_ptr() % 16 == 4 and w.data_ptr() % 16 == 4 and p.is_contiguous() and w.is_contiguous()
    _fc_check(C, gpu, n, c_, v, p, pd, w, wd, "misaligned")


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (7, 7), (4, 4)])
def test_avgpool_fwd_exact(gpu, native_ext, hw, aligned):
    """Both kernels -- the 8-channel one, and the scalar one through a view one element into a larger
    buffer: within one fp32 ulp of exact_sum / HW, and equal at HW = 16."""
    C = native_ext
    shape = (3, hw[0], hw[1], 72)
    _, xd = _ints(gpu, shape, (-20, 20), 70)
    numel = xd.numel()
    buf = torch.zeros(numel + 8, dtype=torch.bfloat16, device=gpu)
    off = 0 if aligned else 1
    x = buf[off:off + numel].view(shape)
    x.copy_(xd)
    assert x.is_contiguous() and (x.data_ptr() % 16 == 0) == aligned     # which kernel runs
    sums, n_hw = eb.ref_avgpool(xd)
    got = C.avgpool_fwd(x)
    assert got.shape == (3, 72) and got.dtype == torch.float32
    mean = (sums / n_hw).float()        # fp64 quotient of an exact integer sum, one rounding to fp32
    if n_hw == 16:
        ec.assert_exact(got, mean, None, None, None, f"avgpool_fwd {shape}")
        return
    lo = torch.nextafter(mean, torch.full_like(mean, -float("inf")))
    hi = torch.nextafter(mean, torch.full_like(mean, float("inf")))
    assert bool(((got >= lo) & (got <= hi)).all()), (got - mean).abs().max().item()


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("hw", [(4, 4), (3, 5)])
def test_avgpool_bwd_exact(gpu, native_ext, hw, splits):
    """dx = (sum over splits) / HW: exact at HW = 16; at HW = 15 (1 / 15 and the product are rounded: two
    fp32 roundings, slack 2^-22 |sum|) within the bf16 neighbours."""
    C = native_ext
    h, w = hw
    dp, dpd = _ints(gpu, (splits, 5, 72), (-8, 8), 71, torch.float32)
    s, want = eb.ref_avgpool_bwd(dpd, h, w)
    dx = C.avgpool_bwd(dp, h, w)
    assert dx.shape == (5, h, w, 72) and dx.dtype == torch.bfloat16
    if h * w == 16:
        ec.assert_exact(dx, eb.to_bf16(want), None, None, None, f"avgpool_bwd {hw} splits={splits}")
    else:
        slack = (2.0 ** -22 * s.abs())[:, None, None, :].expand_as(want)
        eb.assert_bf16_neighbour(dx, want.contiguous(), slack.contiguous(), f"avgpool_bwd {hw} splits={splits}")
