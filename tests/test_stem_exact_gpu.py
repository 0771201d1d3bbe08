"""Bit-exact tests of the stem kernels (helper: tests/exact_stem.py): the halo-staged forward with its
per-row BN partials, the fused BN / pool backward + weight gradient with its slab reduce, the three layout
kernels, and the generic implicit GEMMs behind the (2, 1)-stride ``stem_shape``.

The stem tests of test_kernels_gpu.py judge these kernels by whole-tensor norm ratios and, for the fused
backward, mainly against the unfused path that shares its gather and apply arithmetic
(tests/test_stem_exact_cpu.py shows what that accepts).  Here images and weights are integers in -1..1
(|y| <= 147), the pooled gradient small integers, the BN coefficients crafted (exact_bn.craft), the argmax
bytes built in the test -- so every output has one right answer in any accumulation order, and the
comparisons are ``ec.assert_exact`` / ``torch.equal`` against plain fp64 references.  Two exceptions, both
derived and not tuned: the M2 row partials are exact only where ``es.row_m2_exact`` holds (Wo = 1, 16, 32,
some rows of 64) and are held to ``es.row_m2_slack`` elsewhere; and where a fused-backward case's row count
M = N Ho Wo is no power of two (the kernel rounds 1 / M) the crafted sums are zero, so that case pins the
structure -- units, slabs, items, prefetch -- with A = B = 0 and the power-of-two cases pin the A y + B term.

Every path of these kernels depends on Wo, Ho mod 4 and counts of row groups or items, not on image area:
no image is larger than 16 x 256.  Shapes are (N, H, W); the tables live in exact_stem.py so that the CPU
test can check every premise without a GPU.
"""
import pytest
import torch

import exact_bn as eb
import exact_conv as ec
import exact_stem as es

pytestmark = pytest.mark.gpu

W7 = [64, 3, 7, 7]
_CACHE = {}


def _fwd_ops(gpu, nhw, c=3, k=64, r=7, pad=3):
    """Integer operands and the exact y of one forward case on the GPU, built once and never modified."""
    key = (nhw, c, k, r, pad)
    if key not in _CACHE:
        shape = es.conv_shape(*nhw, c, k, r, pad)
        o = ec.int_operands(shape, (-1, 1), (-1, 1), seed=sum(shape), device=gpu)
        o.yd = es.exact_stem_fwd(o, pad)
        o.ximg = es.kernel_image(o.xd)
        _CACHE[key] = o
    return _CACHE[key]


def _check_halo_fwd(C, o, what):
    """stem_conv_fwd on the halo kernel: xsp, y, the row sums and the M2 against the references."""
    n, ho, wo, k = o.yd.shape
    xsp, y, part, grows = C.stem_conv_fwd(o.ximg, o.w, 2, 3, True)
    assert grows == wo and y.shape == (n, ho, wo, k)
    ec.assert_exact(xsp, ec.to_bf16(es.ref_stem_image(o.xd, 3, 4)), None, None, None, f"{what} xsp")
    ec.assert_exact(y, ec.to_bf16(o.yd), wo, 16, None, f"{what} y")
    worst = es.check_row_partials(part, o.yd, what)
    print(f"{what}: M2 exact on {float(es.row_m2_exact(o.yd).double().mean()):.0%} of the partials, "
          f"largest error elsewhere {worst:.3f} of the derived slack")
    return xsp, y, part


# -------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("hw", [(5, 7), (8, 32), (9, 33)])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_stem_image_layout_bitwise(gpu, native_ext, c, hw):
    """stem_image only rounds to bf16 and moves data: random fp32 images against the bf16 rounding of the
    reference layout, bit for bit; and the weight strides do not matter -- contiguous and channels_last
    weights of the same values give the same packed weights, hence the same y and partials."""
    C = native_ext
    g = torch.Generator().manual_seed(100 + c + hw[1])
    x = torch.randn(3, c, hw[0], hw[1], generator=g).to(gpu)
    w = torch.randn(64, c, 7, 7, generator=g).to(gpu)
    w_cl = w.contiguous(memory_format=torch.channels_last)
    assert w.is_contiguous() and (c == 1 or not w_cl.is_contiguous())
    xsp, y, part, grows = C.stem_conv_fwd(x, w, 2, 3, True)
    xsp2, y2, part2, _ = C.stem_conv_fwd(x, w_cl, 2, 3, True)
    want = ec.to_bf16(es.ref_stem_image(x.permute(0, 2, 3, 1).double(), 3, 4))
    ec.assert_exact(xsp, want, None, None, None, f"stem_image C={c} {hw}")
    assert torch.equal(xsp2, xsp) and torch.equal(y2, y) and torch.equal(part2, part)


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_stem_pack_weight_bitwise_through_one_hot_probes(gpu, native_ext, c, channels_last):
    """stem_pack_weight through the forward: image (parity class, channel) is a one-hot probe at pixel
    (6 + ph, 6 + pw) of a 14 x 14 image, so y[n, ho, wo, k] = bf16(w)[k, c, 9 + ph - 2 ho, 9 + pw - 2 wo]
    exactly (one product) -- every tap of every channel is read once, and everything else must be zero."""
    C = native_ext
    g = torch.Generator().manual_seed(200 + c)
    w = torch.randn(64, c, 7, 7, generator=g).to(gpu)
    if channels_last:
        w = w.contiguous(memory_format=torch.channels_last)
    x = torch.zeros(4 * c, c, 14, 14, device=gpu)
    want = torch.zeros(4 * c, 7, 7, 64, dtype=torch.float64, device=gpu)
    wb = w.bfloat16().double()
    seen = torch.zeros(c, 7, 7, dtype=torch.int32)
    for ph in range(2):
        for pw in range(2):
            for ch in range(c):
                n = (ph * 2 + pw) * c + ch
                x[n, ch, 6 + ph, 6 + pw] = 1.0
                for ho in range(7):
                    for wo in range(7):
                        r, s = 9 + ph - 2 * ho, 9 + pw - 2 * wo
                        if 0 <= r < 7 and 0 <= s < 7:
                            want[n, ho, wo] = wb[:, ch, r, s]
                            seen[ch, r, s] += 1
    assert bool((seen == 1).all())
    _, y, _, _ = C.stem_conv_fwd(x, w, 2, 3, False)
    ec.assert_exact(y, ec.to_bf16(want), 49, None, None, f"packed weights C={c} channels_last={channels_last}")


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_stem_wgrad_and_unpack_exact(gpu, native_ext, c, det):
    """stem_wgrad (the generic TN weight gradient on the super-pixel image + stem_wgrad_unpack) on an
    integer dy, odd W: a fresh channels_last result, and ``accumulate`` into a pre-filled integer ``out``
    in contiguous and in channels_last strides."""
    C = native_ext
    o = _fwd_ops(gpu, (2, 9, 33), c=c)
    wsz = [64, c, 7, 7]
    want = es.ref_stem_wgrad(o.dy, o.xd, 3, wsz)
    xsp = ec.to_bf16(es.ref_stem_image(o.xd, 3, 4))
    dw = C.stem_wgrad(o.dy, xsp, wsz, det)
    assert dw.shape == tuple(wsz) and dw.dtype == torch.float32
    ec.assert_exact(dw.permute(0, 2, 3, 1), want.float().permute(0, 2, 3, 1), None, None, None, f"stem_wgrad C={c}")
    _, out0 = ec.int_tensor(wsz, (-50, 50), 300 + c, gpu, torch.float32)
    eb.require_lattice_sum(ec.ref_wgrad(o.dyd.abs(), o.xd.abs(), o.shape) + out0.abs(), 1.0, "sink + sum |dy||x|")
    for fmt in (torch.contiguous_format, torch.channels_last):
        out = out0.float().contiguous(memory_format=fmt)
        ret = C.stem_wgrad(o.dy, xsp, wsz, det, out)
        assert ret.data_ptr() == out.data_ptr() and ret.stride() == out.stride()
        ec.assert_exact(out.permute(0, 2, 3, 1), (out0 + want).float().permute(0, 2, 3, 1), None, None, None,
                        f"stem_wgrad into out C={c} {fmt}")


# --------------------------------------------------------------------------------- halo forward
@pytest.mark.parametrize("nhw", es.FWD_TM_CASES, ids=lambda t: f"W{t[2]}")
def test_stem_halo_fwd_exact_every_tm(gpu, native_ext, nhw):
    """Every TM instantiation 1..8 with a full and with a partial last pixel fragment (the ``lastok`` mask),
    at Ho = 5: two row groups per image, the second with three invalid waves."""
    _check_halo_fwd(native_ext, _fwd_ops(gpu, nhw), f"stem_conv_fwd {nhw}")


@pytest.mark.parametrize("nhw", es.FWD_HO_CASES, ids=lambda t: f"H{t[1]}")
def test_stem_halo_fwd_exact_every_ho_mod_4(gpu, native_ext, nhw):
    """Ho mod 4 = 1, 2, 3, 0 and Ho = 1: invalid trailing waves, halo rows clipped at Hp."""
    _check_halo_fwd(native_ext, _fwd_ops(gpu, nhw), f"stem_conv_fwd {nhw}")


def test_stem_halo_fwd_without_stats_returns_the_same_y(gpu, native_ext):
    C = native_ext
    for nhw in [(2, 9, 250), (2, 11, 32)]:
        o = _fwd_ops(gpu, nhw)
        _, y, part, grows = C.stem_conv_fwd(o.ximg, o.w, 2, 3, False)
        assert part is None and grows == o.yd.shape[2]
        ec.assert_exact(y, ec.to_bf16(o.yd), o.yd.shape[2], 16, None, f"stem_conv_fwd stats=False {nhw}")


@pytest.mark.parametrize("stats", [True, False])
@pytest.mark.parametrize("nhw", es.FWD_PERSISTENT_CASES)
def test_stem_halo_fwd_exact_over_many_persistent_passes(gpu, native_ext, nhw, stats):
    """More row groups than 4 x the CU count, i.e. more than twice the grid of 2 workgroups per CU: every
    workgroup runs its loop two, three or four times, so both halo
    buffers, the counted halo wait, the reuse of a finished halo buffer as the staging tile and the DMA that
    overwrites it two groups later all carry checked data (every image is different)."""
    C = native_ext
    n, h, w = nhw
    groups = n * (((h - 1) // 2 + 1 + es.ROWS - 1) // es.ROWS)
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    assert groups > 4 * cus, f"premise: {groups} row groups are not more than 4 x {cus} CUs"
    o = _fwd_ops(gpu, nhw)
    if stats:
        _check_halo_fwd(C, o, f"stem_conv_fwd {nhw}")
    else:
        _, y, _, _ = C.stem_conv_fwd(o.ximg, o.w, 2, 3, False)
        ec.assert_exact(y, ec.to_bf16(o.yd), o.yd.shape[2], 16, None, f"stem_conv_fwd stats=False {nhw}")


# ----------------------------------------------------------------------------- generic fallback
@pytest.mark.parametrize("nhw,k,r,pad", es.FALLBACK_CASES)
def test_stem_generic_fallback_exact(gpu, native_ext, nhw, k, r, pad):
    """Stems outside the halo kernel's domain (Wo > 128, K != 64, 5x5, 3x3) run the generic NT forward and
    TN weight gradient on ``stem_shape``, the only ConvShape with stride_w != stride: y bit for bit, the
    row-tile partial sums exact, and stem_wgrad (atomic and deterministic) exact on an integer dy."""
    C = native_ext
    o = _fwd_ops(gpu, nhw, 3, k, r, pad)
    n, ho, wo, _ = o.yd.shape
    sp, M = (r + 1) // 2, n * ho * wo
    xsp, y, part, grows = C.stem_conv_fwd(o.ximg, o.w, 2, pad, True)
    assert grows == C.conv_nt_group_rows(M, k, r * sp * 8 * 2) and grows != wo
    ec.assert_exact(xsp, ec.to_bf16(es.ref_stem_image(o.xd, pad, sp)), None, None, None, f"fallback xsp {nhw}")
    y64 = o.yd.reshape(M, k)
    ec.assert_exact(y.reshape(M, k), ec.to_bf16(y64), grows, 64, ec.fwd_border(o.shape), f"fallback y {nhw} K={k} R={r}")
    ec.require_stat_sums(y64, grows, "fallback y")
    assert part.shape == ((M + grows - 1) // grows, 2, k)
    ec.assert_exact(part[:, 0, :].double(), ec.group_sums(y64, grows), None, 64, None, f"fallback group sums {nhw}")
    _, y0, p0, _ = C.stem_conv_fwd(o.ximg, o.w, 2, pad, False)
    assert p0 is None and torch.equal(y0, y)
    wsz = [k, 3, r, r]
    want = es.ref_stem_wgrad(o.dy, o.xd, pad, wsz).float()
    for det in (False, True):
        dw = C.stem_wgrad(o.dy, xsp, wsz, det)
        ec.assert_exact(dw.permute(0, 2, 3, 1), want.permute(0, 2, 3, 1), None, None, None,
                        f"fallback stem_wgrad {nhw} K={k} R={r} det={det}")


# ------------------------------------------------------------------------------- fused backward
def _run_fused(C, f, training, det):
    return C.stem_bwd_fused(f.dp, f.bi, f.y, f.c.stats, f.c.gamma, f.c.sums, training, f.xsp, W7, det)


def _check_fused(C, f, dets, what):
    for training in (True, False):
        want = f.dw[training].float().permute(0, 2, 3, 1)           # [K, R, S, C]: columns = (tap, channel)
        for det in dets:
            dw = _run_fused(C, f, training, det)
            assert dw.shape == tuple(W7) and dw.dtype == torch.float32
            ec.assert_exact(dw.permute(0, 2, 3, 1), want, None, None, None, f"{what} training={training} det={det}")
            if det:
                assert torch.equal(_run_fused(C, f, training, det), dw), f"{what}: deterministic run not repeatable"


@pytest.mark.parametrize("argmax", ["pool", "crafted"])
@pytest.mark.parametrize("nhw", es.BWD_CASES)
def test_stem_bwd_fused_exact(gpu, native_ext, nhw, argmax):
    """stem_bwd_fused against ref_stem_wgrad(ref_stem_dy(...)): the quad gather (all nine terms carry their
    own gradient under the crafted argmax map), the ReLU mask from y, k1 g + (A y + B), the bf16 dy tile and
    the MFMA weight gradient, atomic and slab, training and evaluation mode."""
    f = es.fused_case(nhw, argmax, gpu)
    if nhw in es.BWD_MANY_ITEMS:
        assert f.items > es.BWD_GRID, "premise: more items than workgroups"
    _check_fused(native_ext, f, (False, True), f"stem_bwd_fused {nhw} {argmax}")


@pytest.mark.parametrize("nhw", es.BWD_SLAB_CASES)
def test_stem_bwd_fused_slab_reduce_exact(gpu, native_ext, nhw):
    """Grid 1, 3, 17 and 32 slabs in the fixed-order reduce (fewer slabs than phases, a slab in a phase's
    second round), deterministic."""
    f = es.fused_case(nhw, "crafted", gpu)
    _check_fused(native_ext, f, (True,), f"stem_bwd_fused slabs {nhw}")


def test_stem_bwd_fused_domain(gpu, native_ext):
    """stem_bwd_fused_supported against its documented domain, and the binding raising outside it."""
    C = native_ext
    assert C.stem_bwd_fused_supported(64, 7, 4, 4, 16) and C.stem_bwd_fused_supported(64, 7, 4, 2, 128)
    bad = {"Ho odd": (64, 5, 16), "Wo % 16": (64, 4, 24), "Wo = 144": (64, 4, 144), "K = 32": (32, 4, 16)}
    c = es.fused_coefs(256, 1, gpu)
    for name, (k, ho, wo) in bad.items():
        assert not C.stem_bwd_fused_supported(k, 7, 4, ho, wo), name
        y = torch.zeros(1, ho, wo, k, dtype=torch.bfloat16, device=gpu)
        dp = torch.zeros(1, (ho + 1) // 2, wo // 2, k, dtype=torch.bfloat16, device=gpu)
        idx = torch.full(dp.shape, 4, dtype=torch.uint8, device=gpu)
        xsp = torch.zeros(1, 2 * ho + 5, wo + 3, 8, dtype=torch.bfloat16, device=gpu)
        with pytest.raises(RuntimeError):
            C.stem_bwd_fused(dp, idx, y, c.stats[:, :k].contiguous(), c.gamma[:k].contiguous(),
                             c.sums[:, :k].contiguous(), True, xsp, [k, 3, 7, 7], False)
    assert not C.stem_bwd_fused_supported(64, 5, 3, 4, 16) and not C.stem_bwd_fused_supported(64, 7, 4, 4, 0)


# ---------------------------------------------------------------------------------- composition
def test_stem_fwd_pool_bwd_composition_exact(gpu, native_ext):
    """stem_conv_fwd -> bn_relu_maxpool (crafted scale and shift) -> stem_bwd_fused on the kernels' own
    xsp, y and argmax bytes, against the references chained end to end."""
    C = native_ext
    f = es.fused_case(es.COMPOSITION_CASE, "pool", gpu)
    xsp, y, part, grows = C.stem_conv_fwd(es.kernel_image(f.o.xd), f.o.w, 2, 3, True)
    ec.assert_exact(y, f.y, grows, 16, None, "composition y")
    es.check_row_partials(part, f.yd, "composition")
    pooled, idx = C.bn_relu_maxpool(y, f.c.stats[2].contiguous(), f.c.stats[3].contiguous())
    out_w, bi, _ = eb.ref_bn_relu_maxpool(f.yd, f.c.scale, f.c.shift)
    ec.assert_exact(pooled, out_w, None, None, None, "composition pooled")
    ec.assert_exact(idx, bi, None, None, None, "composition argmax")
    assert torch.equal(bi, f.bi)
    for det in (False, True):
        dw = C.stem_bwd_fused(f.dp, idx, y, f.c.stats, f.c.gamma, f.c.sums, True, xsp, W7, det)
        ec.assert_exact(dw.permute(0, 2, 3, 1), f.dw[True].float().permute(0, 2, 3, 1), None, None, None,
                        f"composition dW det={det}")
