"""The exact stem harness (tests/exact_stem.py) checked without a GPU, and why it exists.

* its fp64 references equal ``torch.nn.functional.conv2d`` and autograd in fp64, and the im2col and the
  super-pixel forms of the convolution equal each other, for C in 1..4, odd and even extents, 7x7 / pad 3,
  5x5 / pad 2 and 3x3 / pad 1;
* every premise of every case table of tests/test_stem_exact_gpu.py holds on the references alone, so a
  table edit that breaks exactness fails here first; the premise checks raise when broken;
* the gaps: what the whole-tensor metrics of the three old stem tests say about five localized defects,
  applied to the reference output of a GPU case, next to what the new comparisons say.  Where the old
  metric does see a defect at these inputs the test says so instead of claiming a gap.
"""
import pytest
import torch
import torch.nn.functional as F

import exact_bn as eb
import exact_conv as ec
import exact_stem as es


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


# --------------------------------------------------------------------------- reference agreement
REF_CASES = [(c, h, w, r, pad) for c in (1, 2, 3, 4) for (h, w) in ((5, 7), (8, 32), (9, 33)) for (r, pad) in ((7, 3),)]
REF_CASES += [(3, 8, 32, 5, 2), (3, 9, 33, 5, 2), (3, 8, 32, 3, 1), (4, 9, 33, 3, 1)]


@pytest.mark.parametrize("c,h,w,r,pad", REF_CASES)
def test_references_match_conv2d_and_each_other(c, h, w, r, pad):
    k, sp = 16, (r + 1) // 2
    shape = es.conv_shape(2, h, w, c, k, r, pad)
    o = ec.int_operands(shape, (-1, 1), (-1, 1), seed=c + h + w + r)
    y = es.ref_stem_fwd(o.xd, o.wd, pad)
    x = _nchw(o.xd).clone()
    wt = o.wd.clone().requires_grad_(True)
    yt = F.conv2d(x, wt, stride=2, padding=pad)
    assert torch.equal(y, _nhwc(yt.detach()))
    assert torch.equal(y, es.ref_stem_fwd_superpixel(o.xd, o.wd, pad))
    # layouts: shapes, the pack / unpack round trip, zeros in the padded channels and in tap s = -1
    xs, ws = es.ref_stem_image(o.xd, pad, sp), es.ref_stem_pack_weight(o.wd, sp)
    ho, wo = ec.out_hw(shape)
    assert xs.shape == (2, h + 2 * pad, wo + sp - 1, 8) and ws.shape == (k, r, sp, 8)
    assert torch.equal(es.ref_stem_unpack(ws, c, r), o.wd)
    assert int(torch.count_nonzero(ws[:, :, 0, :4])) == 0
    assert int(torch.count_nonzero(ws.reshape(k, r, sp, 2, 4)[..., c:])) == 0
    assert int(torch.count_nonzero(xs.reshape(*xs.shape[:3], 2, 4)[..., c:])) == 0
    assert xs.sum() == o.xd[:, :, :2 * (wo + sp - 1) - pad - 1].sum()       # every source pixel once
    # the weight gradient of a stored bf16 dy against autograd
    yt.backward(_nchw(o.dyd))
    assert torch.equal(es.ref_stem_wgrad(o.dy, o.xd, pad, [k, c, r, r]), wt.grad)


def test_row_partials_match_var_and_the_m2_premises_trip():
    o = ec.int_operands(es.conv_shape(2, 9, 32), (-1, 1), (-1, 1), seed=1)
    y = es.exact_stem_fwd(o, 3)
    p = es.ref_row_partials(y)
    rows = y.reshape(-1, 16, 64)
    assert torch.equal(p[:, 0], rows.sum(1))
    assert torch.allclose(p[:, 1], rows.var(1, unbiased=False) * 16, rtol=1e-12, atol=1e-12)
    es.require_row_m2_exact(y)
    assert bool(es.row_m2_exact(y).all())
    with pytest.raises(ec.PremiseError, match="not a power of two"):
        es.require_row_m2_exact(y[:, :, :15])
    with pytest.raises(ec.PremiseError, match="not integer"):
        es.require_row_m2_exact(y + 0.5)
    with pytest.raises(ec.PremiseError, match="sum d"):
        es.require_row_m2_exact(y * 64)
    assert not bool(es.row_m2_exact(y * 64).any()) and not bool(es.row_m2_exact(y[:, :, :15]).any())
    # the slack: zero where the row is constant and the mean exact, a few fp32 ulps of M2 elsewhere
    s = es.row_m2_slack(y)
    assert s.shape == (10, 64) and bool((s >= 8 * es.U * p[:, 1]).all()) and bool((s <= 9 * es.U * p[:, 1] + 1e-9).all())
    # a plain fp32 evaluation of the kernel's two passes at a width that is no power of two stays inside it
    o2 = ec.int_operands(es.conv_shape(2, 9, 250), (-1, 1), (-1, 1), seed=2)
    y2 = es.exact_stem_fwd(o2, 3)
    r2 = y2.reshape(-1, 125, 64).float()
    mean = r2.sum(1) * (torch.tensor(1.0) / torch.tensor(125.0))
    d = r2 - mean[:, None, :]
    m2 = torch.zeros_like(mean)
    for i in range(125):
        m2 = m2 + d[:, i] * d[:, i]
    err = (m2.double() - es.ref_row_partials(y2)[:, 1]).abs()
    assert bool((err <= es.row_m2_slack(y2) * 125 / 14).all())       # 125 sequential roundings instead of 8 + 6
    assert not bool(es.row_m2_exact(y2).any())


def test_stem_dy_premises_trip():
    f = es.fused_case((4, 8, 32), "pool")
    with pytest.raises(ec.PremiseError, match="1 / M is rounded"):
        es.ref_stem_dy(eb.craft(64, 512, 3), f.dpd, f.bi, f.yd, True)
    with pytest.raises(ec.PremiseError, match="crafted"):
        es.ref_stem_dy(eb.generic(64, 256, 3), f.dpd, f.bi, f.yd, True)
    bad = f.bi.clone()
    bad[0, 0, 0, 0] = 0
    with pytest.raises(ec.PremiseError, match="outside the image"):
        es.ref_stem_dy(f.c, f.dpd, bad, f.yd, True)
    with pytest.raises(ec.PremiseError):
        es.ref_stem_wgrad(f.dy[True] * 2.0 ** 12, f.o.xd, 3, [64, 3, 7, 7])
    # the zero-sum coefficients of a row count that is no power of two: training == evaluation == k1 g
    c = es.fused_coefs(320, 5)
    assert c.M == 512 and int(torch.count_nonzero(c.sums)) == 0 and c.exact
    f2 = es.fused_case((2, 4, 160), "crafted")
    assert torch.equal(f2.dy[True], f2.dy[False]) and int(torch.count_nonzero(f2.dy[True])) > 0


# ------------------------------------------------------------------- premises of every GPU case
@pytest.mark.parametrize("nhw", es.FWD_TM_CASES + es.FWD_HO_CASES + es.FWD_PERSISTENT_CASES)
def test_premises_of_the_halo_forward_cases(nhw):
    n, h, w = nhw
    o = ec.int_operands(es.conv_shape(n, h, w), (-1, 1), (-1, 1), seed=sum(nhw))
    y = es.exact_stem_fwd(o, 3)
    ho, wo = y.shape[1:3]
    assert 1 <= wo <= 128
    eb.require_lattice_sum(y.reshape(n * ho, wo, 64).abs().sum(1), 1.0, "row sums")
    if wo in (1, 16, 32):
        es.require_row_m2_exact(y)          # with these operand ranges every row and channel is exact
    else:                                   # no power of two: the slack everywhere; Wo = 64 and 128: on the
        assert wo in (64, 128) or not bool(es.row_m2_exact(y).any())    # rows where 2^24 is reached
        with pytest.raises(ec.PremiseError):
            es.require_row_m2_exact(y)
    s = es.row_m2_slack(y)
    assert bool(torch.isfinite(s).all()) and bool((s <= 2.0 ** -19 * es.ref_row_partials(y)[:, 1] + 1e-9).all())


def test_the_forward_tables_cover_what_they_claim():
    assert [(w - 1) // 2 + 1 for w in es.TM_WIDTHS] == es.TM_WOS
    tms = [(wo + 15) // 16 for wo in es.TM_WOS]
    assert set(tms) == set(range(1, 9))
    for tm in range(1, 9):      # every TM with a full last fragment, every TM with a partial one
        assert any(t == tm and wo % 16 == 0 for t, wo in zip(tms, es.TM_WOS)), tm
        assert any(t == tm and wo % 16 != 0 for t, wo in zip(tms, es.TM_WOS)), tm
    hos = [(h - 1) // 2 + 1 for _, h, _ in es.FWD_HO_CASES]
    assert {ho % 4 for ho in hos} == {0, 1, 2, 3} and 1 in hos
    # a halo clipped at Hp: the last group's 13 rows reach past the padded image
    assert any(2 * ((ho - 1) // 4 * 4) + 13 > h + 6 for ho, (_, h, _) in zip(hos, es.FWD_HO_CASES))
    for n, h, w in es.FWD_PERSISTENT_CASES:     # more row groups than 4 x the CUs of a 256-CU GPU (grid 512)
        assert n * (((h - 1) // 2 + 1 + 3) // 4) > 4 * 256


@pytest.mark.parametrize("nhw,k,r,pad", es.FALLBACK_CASES)
def test_premises_of_the_fallback_cases(nhw, k, r, pad):
    n, h, w = nhw
    shape = es.conv_shape(n, h, w, 3, k, r, pad)
    o = ec.int_operands(shape, (-1, 1), (-1, 1), seed=sum(shape))
    y = es.exact_stem_fwd(o, pad)
    ho, wo = ec.out_hw(shape)
    assert not (k == 64 and r == 7 and wo <= 128)           # not the halo kernel's domain
    ec.require_stat_sums(y.reshape(-1, k), None, "fallback y")
    es.ref_stem_wgrad(o.dy, o.xd, pad, [k, 3, r, r])


@pytest.mark.parametrize("argmax", ["pool", "crafted"])
@pytest.mark.parametrize("nhw", sorted(set(es.BWD_CASES + es.BWD_SLAB_CASES + [es.COMPOSITION_CASE])))
def test_premises_of_the_fused_backward_cases(nhw, argmax):
    f = es.fused_case(nhw, argmax)          # raises PremiseError where a premise breaks
    n, ho, wo, _ = f.yd.shape
    m = n * ho * wo
    assert (f.c.M == m) == (m & (m - 1) == 0)
    assert es.argmax_inside(f.bi, ho, wo)
    for training in (True, False):
        assert f.dy[training].dtype == torch.bfloat16 and int(torch.count_nonzero(f.dw[training])) > 0
    if f.c.M == m:      # not vacuous: A y + B matters, and the bf16 store of dy rounds
        assert not torch.equal(f.dy[True], f.dy[False])
    if f.c.M == m and argmax == "pool":     # (sums of several window gradients need more than 8 bits)
        g = eb.ref_maxpool_bwd(f.dpd, f.bi, ho, wo)
        want, _ = eb.exact_bwd_apply(f.c, g, f.yd, eb.mask_on(2, None, f.yd, f.c.scale, f.c.shift))
        assert int((f.dy[True].double() != want).sum()) > 0
    if nhw in es.BWD_MANY_ITEMS:
        assert f.items > es.BWD_GRID


def test_the_backward_tables_cover_what_they_claim():
    units = {nhw: ((nhw[2] - 1) // 2 + 1) // 2 * 8 for nhw in es.BWD_CASES}
    assert units[(1, 4, 32)] == units[(4, 8, 32)] == 64             # one unit per thread, partly idle
    assert 256 < units[(2, 4, 160)] < 512 and units[(1, 4, 256)] == 512
    assert units[(2, 8, 160)] == units[(2, 4, 160)] and units[(1, 8, 256)] == 512   # ... with two pooled rows
    for n, h, w in [(2, 7, 32), (2, 3, 64)]:                        # the last item's 9 rows end exactly at Hp
        ho = (h - 1) // 2 + 1
        assert h % 2 == 1 and ho % 2 == 0 and 4 * (ho // 2 - 1) + 9 == h + 6
    assert [n * ((h - 1) // 2 + 1) // 2 for n, h, _ in es.BWD_SLAB_CASES] == [1, 3, 17, 32]
    # the crafted argmax map: every legal selector at interior, edge and corner windows
    bi = es.crafted_argmax(4, 2, 8, 64)
    assert es.argmax_inside(bi, 4, 16)
    legal = lambda top, left: {3 * kh + kw for kh in range(3) for kw in range(3)        # noqa: E731
                               if not (top and kh == 0) and not (left and kw == 0)}
    for ph in range(2):
        for pw in range(8):
            assert set(bi[:, ph, pw].flatten().tolist()) == legal(ph == 0, pw == 0), (ph, pw)
    assert set(bi[:, 1, 1:].flatten().tolist()) == set(range(9))


# ---------------------------------------------------------------------------- gap demonstrations
def _fwd_case(nhw):
    o = ec.int_operands(es.conv_shape(*nhw), (-1, 1), (-1, 1), seed=sum(nhw))
    return o, es.exact_stem_fwd(o, 3)


def test_gap_a_zeroed_last_pixel_of_a_row():
    """(a) at Wo = 125, case (2, 9, 250): the last pixel of one output row zeroed.  At this case's 1250
    pixels one pixel is a norm ratio of about sqrt(1 / 1250) = 0.028: the old 1e-2 metric DOES see it here
    (it would not from about 10,000 pixels on, e.g. the old test's (2, 62, 250) is at the limit), so no gap
    is claimed for y at this size; the exact comparison names the pixel."""
    o, y = _fwd_case((2, 9, 250))
    bad = y.clone()
    bad[1, 2, 124] = 0
    err = ec.rel_err(ec.to_bf16(bad), ec.to_bf16(y))
    print(f"(a) norm ratio of one zeroed pixel of 1250: {err:.3e}")
    assert err >= 1e-2                                  # no claim: the old metric sees it at this size
    assert err * (1250 / 12500) ** 0.5 < 1e-2           # ... and would not at ten times the pixels
    with pytest.raises(AssertionError, match="wrong rows: 1,") as e:
        ec.assert_exact(ec.to_bf16(bad), ec.to_bf16(y), 125, None, None, "zeroed pixel")
    assert "by row % 125: {124:" in str(e.value)


def test_gap_b_pixel_missing_from_the_row_statistics():
    """(b) the same pixel missing from its row's sum and M2 (a dropped ``lastok`` lane).  The old test's
    ``rel_err(part[:, 1]) < 1e-2`` accepts the M2 (norm ratio 2.7e-3); the derived slack rejects it.  The
    sums of this case's 10 rows move by a norm ratio of 2.2e-2, which the old ``rel_err(part[:, 0]) < 1e-2``
    DOES see at this size (with the 1400 rows of (700, 9, 32) the same drop is 4.4e-3 and passes), so for
    the sums no gap is claimed here; the exact comparison rejects them at any size."""
    o, y = _fwd_case((2, 9, 250))
    want = es.ref_row_partials(y)
    row = 1 * 5 + 2
    short = y.reshape(10, 125, 64)[row, :124]
    bad = want.clone()
    bad[row, 0] = short.sum(0)
    bad[row, 1] = ((short - short.sum(0) / 125) ** 2).sum(0)     # the kernel's mean still divides by Wo
    e0, e1 = ec.rel_err(bad[:, 0], want[:, 0]), ec.rel_err(bad[:, 1], want[:, 1])
    print(f"(b) norm ratio of the sums {e0:.3e}, of the M2 {e1:.3e}")
    assert 0 < e1 < 1e-2                                # the old metric accepts the M2
    assert e0 >= 1e-2                                   # no claim for the sums at 10 rows
    es.check_row_partials(want.float(), y, "unchanged")
    with pytest.raises(AssertionError, match="row sums"):
        es.check_row_partials(bad.float(), y, "dropped pixel")
    only_m2 = want.clone()
    only_m2[row, 1] = bad[row, 1]
    with pytest.raises(AssertionError, match="outside the derived slack"):
        es.check_row_partials(only_m2.float(), y, "dropped pixel, M2 only")


def test_gap_c_row_group_from_the_previous_images_halo():
    """(c) case (700, 9, 32): the first row group of one image computed from the previous image's halo (a
    halo wait that let the wrong buffer through).  One group of 1400 is a norm ratio of about
    sqrt(2 / 1400) = 0.038: the old metric would see it at this size (the old tests never run a second
    pass, so they cannot meet it at any size); no gap is claimed.  The exact comparison names the rows."""
    o, y = _fwd_case((700, 9, 32))
    bad = y.clone()
    bad[400, 0:4] = y[399, 0:4]
    err = ec.rel_err(ec.to_bf16(bad), ec.to_bf16(y))
    print(f"(c) norm ratio of one row group of 1400 from the wrong image: {err:.3e}")
    assert err >= 1e-2                                  # no claim
    with pytest.raises(AssertionError, match="wrong rows: 64,"):
        ec.assert_exact(ec.to_bf16(bad), ec.to_bf16(y), 16, None, None, "wrong halo")


def _dw_with(f, g_defect):
    """dW of case ``f`` with the gathered pool gradient replaced (training mode)."""
    on = eb.mask_on(2, None, f.yd, f.c.scale, f.c.shift)
    dy, _ = eb.ref_bwd_apply(f.c, g_defect, f.yd, on, True)
    return ec.ref_wgrad(ec.to_bf16(dy).double(), f.o.xd, f.shape)


def test_gap_d_lost_w11_contribution():
    """(d) case (4, 8, 32), crafted argmax: the W11@0 term of the quad gather (the window below and to the
    right, selector 0) missing from dy.  Against a correct reference the norm ratio is far above 1e-3 -- the
    old test accepts this defect for another reason: its reference, the unfused path, gathers with the same
    pool_quad.h and loses the same term.  No gap in the metric is claimed; the fp64 reference here shares
    no code with the kernels."""
    f = es.fused_case((4, 8, 32), "crafted")
    n, ho, wo, k = f.yd.shape
    g = eb.ref_maxpool_bwd(f.dpd, f.bi, ho, wo)
    lost = eb.ref_maxpool_bwd(torch.where(f.bi == 0, 0.0, f.dpd), f.bi, ho, wo)
    assert int((g != lost).sum()) > 0
    bad = _dw_with(f, lost)
    assert torch.equal(_dw_with(f, g), f.dw[True])
    err = ec.rel_err(bad, f.dw[True])
    print(f"(d) norm ratio of dW without the W11@0 term: {err:.3e}")
    assert err >= 1e-3                                  # no claim on the metric
    with pytest.raises(AssertionError, match="elements differ"):
        ec.assert_exact(bad.float(), f.dw[True].float(), None, None, None, "lost W11@0")


def test_gap_e_fourth_fragment_of_wave_1_zeroed():
    """(e) case (4, 8, 32): the packed weight-gradient columns 208..223 (filter row 6, taps s = 3..6: the
    fourth column fragment, owned by wave 1) zeroed.  12 of 147 taps are a norm ratio near sqrt(12 / 147):
    the old metric sees it; no gap is claimed.  The exact comparison names the taps."""
    f = es.fused_case((4, 8, 32), "pool")
    dw = f.dw[True]
    packed = es.ref_stem_pack_weight(dw, 4).reshape(64, 224).clone()
    packed[:, 208:224] = 0
    bad = es.ref_stem_unpack(packed.reshape(64, 7, 4, 8), 3, 7)
    changed = (bad != dw).nonzero()
    assert set(changed[:, 2].tolist()) == {6} and set(changed[:, 3].tolist()) == {3, 4, 5, 6}
    err = ec.rel_err(bad, dw)
    print(f"(e) norm ratio of dW with columns 208..223 zeroed: {err:.3e}")
    assert err >= 1e-3                                  # no claim
    with pytest.raises(AssertionError, match="elements differ"):
        ec.assert_exact(bad.float(), dw.float(), None, None, None, "zeroed fragment")
