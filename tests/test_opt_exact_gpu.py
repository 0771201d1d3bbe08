"""Bit-exact tests of what runs between two forward passes (helper: tests/exact_opt.py): the flat SGD and
LARS steps with their bf16 mirror, cast_to_bf16, pack_weight / pack_weight_t / pack_t_batched, and the fp8
quantizers with their delayed-scaling state.

The loose tests of these kernels (test_kernels_gpu.py::test_sgd_flat*, test_lars_gpu.py, test_fp8_gpu.py)
use one size each, dampening 0, grad_scale 1, two state slots, and whole-tensor tolerances;
tests/test_opt_exact_cpu.py shows what they accept.  Here the operands are crafted so that every fp32
intermediate is exact (small integers, dyadic hyper-parameters, power-of-two trust values and scales):
a plain fp64 transcription of each kernel's formula is the one right answer, the bf16 mirror is one
round-to-nearest-even of it, fp8 codes are compared as bytes, and every comparison is ``torch.equal``.
No tolerance appears in this file.  The premises are asserted by the references themselves
(``PremiseError``), here and -- for every row of the tables -- on the CPU.

Sizes sit where these kernels go wrong: fewer elements than one vector, tails, the capped grid's second
(partial) grid-stride trip, LARS segments starting 1, 2 and 3 elements off a 16-byte boundary, segments
shorter than their lead, partial 64 x 64 transpose tiles, the amax in the first / last vector and in a
block that wraps onto shard 0, all three state slots, the scale's power-of-two boundaries and clamps.
A new optimizer, mirror or quantizer variant gets a row in the tables of tests/exact_opt.py.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import exact_bn as eb
import exact_conv as ec
import exact_opt as eo

pytestmark = pytest.mark.gpu

_CACHE = {}
BF16 = torch.bfloat16


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _f32(t):
    eb.require_fp32(t, "fp32 operand")
    return t.float().contiguous()


def _flat_eq(got, want, what):
    ec.assert_exact(got.reshape(1, -1), want.reshape(1, -1), None, 4, None, what)


def _bits(t):
    return t.view(torch.int16)


# ============================================================================================ SGD
@pytest.mark.parametrize("n", eo.SGD_SIZES)
@pytest.mark.parametrize("v", eo.VARIANTS, ids=lambda v: v.id)
def test_sgd_step_exact(gpu, native_ext, v, n):
    """Two steps (first, then the recurrence): p, buf and the bf16 mirror bit for bit; without a mirror a
    sentinel bf16 buffer on the device stays as it was, and at momentum 0 a momentum buffer passed
    alongside is not written."""
    C = native_ext
    pd, g1d, g2d = _cached(("sgd", n), lambda: eo.sgd_operands(n, n % 97, gpu))
    steps = eo.ref_two_steps(pd, g1d, g2d, v)
    eo.require_ties(steps, n, f"sgd {v.id} n={n}")
    p = pd.float()
    buf = torch.full((n,), eo.SENT_F32, device=gpu)
    mir = torch.full((n,), eo.SENT_BF16, device=gpu, dtype=BF16)
    for i, ((p_want, b_want), gd) in enumerate(zip(steps, (g1d, g2d))):
        C.sgd_step(p, gd.float(), buf, v.lr, v.momentum, v.dampening, v.wd, v.nesterov, i == 0, v.grad_scale,
                   mir if v.mirror else None)
        what = f"sgd_step {v.id} n={n} step {i + 1}"
        _flat_eq(p, p_want.float(), what + " p")
        if v.momentum != 0.0:
            _flat_eq(buf, b_want.float(), what + " buf")
        else:
            assert bool((buf == eo.SENT_F32).all()), what + ": momentum 0 wrote the buffer passed alongside"
        if v.mirror:
            _flat_eq(_bits(mir), _bits(ec.to_bf16(p_want)), what + " mirror")
        else:
            assert bool((mir == eo.SENT_BF16).all()), what + ": a bf16 buffer changed without a mirror argument"


# =========================================================================================== LARS
LARS_VARIANTS = [v for v in eo.VARIANTS if v.grad_scale == 1.0]      # LARS has no grad_scale


def _lars_v(v):
    """The SGD variant with the LARS cases' lr = 2^-1 and wd = 2^-2 (the trust values span 2^-4 .. 2^4)."""
    w = SimpleNamespace(**vars(v))
    w.lr, w.wd = 0.5, 0.25
    return w


def _lars_table(gpu, native_ext):
    def make():
        from pytorch_distributed_tutorials_amd.optim.lars import LarsTable
        assert native_ext.lars_chunk_elems() == eo.CHUNK
        segs, numel = eo.lars_segments()
        tb = LarsTable(segs, gpu)
        assert tb.nchunks == len(eo.lars_chunks(segs))
        return segs, numel, tb
    return _cached("lars_table", make)


def _lars_operands(gpu, numel):
    return _cached(("lars_ops", numel), lambda: eo.sgd_operands(numel, 7, gpu))


def _run_lars_update(C, gpu, tb, v, p0, gs, lo, hi):
    """p, buf, mirror after the two update passes over segments [lo, hi)."""
    n = p0.numel()
    p = p0.float()
    buf = torch.full((n,), eo.SENT_F32, device=gpu)
    mir = torch.full((n,), eo.SENT_BF16, device=gpu, dtype=BF16)
    out = []
    for i, gd in enumerate(gs):
        C.lars_update(p, gd.float(), buf if v.momentum != 0.0 else None, tb.table, tb.partials, tb.trust, lo, hi,
                      v.lr, v.momentum, v.dampening, v.wd, v.nesterov, i == 0, mir if v.mirror else None)
        out.append((p.clone(), buf.clone(), mir.clone()))
    return out


def _check_lars(out, steps, p0, inside, v, what):
    for i, ((p, buf, mir), (p_want, b_want)) in enumerate(zip(out, steps)):
        w = f"{what} step {i + 1}"
        _flat_eq(p, torch.where(inside, p_want, p0).float(), w + " p")
        if v.momentum != 0.0:
            _flat_eq(buf, torch.where(inside, b_want, eo.SENT_F32).float(), w + " buf")
        else:
            assert bool((buf == eo.SENT_F32).all()), w
        if v.mirror:
            want = torch.where(inside, ec.to_bf16(p_want), torch.tensor(eo.SENT_BF16, dtype=BF16, device=p.device))
            _flat_eq(_bits(mir), _bits(want), w + " mirror")
        else:
            assert bool((mir == eo.SENT_BF16).all()), w


@pytest.mark.parametrize("v", LARS_VARIANTS, ids=lambda v: v.id)
def test_lars_update_exact(gpu, native_ext, v):
    """lars_update with a trust tensor written by the test (a different power of two per segment, non-1 on
    the excluded ones, which lose only the weight decay): p, buf and mirror bit for bit over two steps, the
    gaps between segments untouched."""
    C = native_ext
    v = _lars_v(v)
    segs, numel, tb = _lars_table(gpu, native_ext)
    p0, g1, g2 = _lars_operands(gpu, numel)
    trust = eo.lars_trust_values(segs)
    tb.trust.copy_(trust.float())
    tr, wde, cov = eo.lars_elementwise(segs, numel, trust, v.wd, gpu)
    steps = eo.ref_two_steps(p0, g1, g2, v, trust=tr, wd=wde)
    eo.require_ties([(s[0][cov], None) for s in steps], numel, f"lars {v.id}")
    out = _run_lars_update(C, gpu, tb, v, p0, (g1, g2), 0, tb.nseg)
    _check_lars(out, steps, p0, cov, v, f"lars_update {v.id}")


@pytest.mark.parametrize("lo,hi", [(3, 7), (1, 2), (8, 9)])
def test_lars_update_subrange_leaves_the_rest(gpu, native_ext, lo, hi):
    """Segments [lo, hi) only: every element outside is bit-identical in p, buf and the mirror."""
    C = native_ext
    v = _lars_v(next(x for x in LARS_VARIANTS if x.id == "nesterov-mirror-d0.25-s1"))
    segs, numel, tb = _lars_table(gpu, native_ext)
    p0, g1, g2 = _lars_operands(gpu, numel)
    trust = eo.lars_trust_values(segs)
    tb.trust.copy_(trust.float())
    tr, wde, _ = eo.lars_elementwise(segs, numel, trust, v.wd, gpu)
    steps = eo.ref_two_steps(p0, g1, g2, v, trust=tr, wd=wde)
    out = _run_lars_update(C, gpu, tb, v, p0, (g1, g2), lo, hi)
    _check_lars(out, steps, p0, eo.range_mask(segs, numel, lo, hi, gpu), v, f"lars_update [{lo}, {hi})")


def _norm_operands(gpu, segs, numel):
    def make():
        p, g = eo.lars_norm_operands(segs, numel)
        eo.require_perfect_squares(p, g, segs)
        return p.to(gpu), g.to(gpu)
    return _cached("lars_norm_ops", make)


def test_lars_norms_exact(gpu, native_ext):
    """partials = (sum p^2, sum g^2) per chunk: exact integers in float64; excluded chunks keep their
    sentinel."""
    C = native_ext
    segs, numel, tb = _lars_table(gpu, native_ext)
    p, g = _norm_operands(gpu, segs, numel)
    tb.partials.fill_(-7.0)
    C.lars_norms(p.float(), g.float(), tb.table, tb.partials, tb.trust, 0, tb.nseg)
    ec.assert_exact(tb.partials.view(-1, 2), eo.ref_partials(p, g, segs, -7.0), None, None, None, "lars_norms")


@pytest.mark.parametrize("wd,eta,eps", eo.TRUST_PARAMS)
def test_lars_trust_exact(gpu, native_ext, wd, eta, eps):
    """Perfect-square norms: sqrt is exact and every other operation one float64 rounding, so the trust
    ratios equal the formula evaluated in torch float64 and cast once -- from lars_norms + lars_trust_only
    and from lars_trust; |p| = 0, |g| = 0 and excluded segments give exactly 1."""
    C = native_ext
    segs, numel, tb = _lars_table(gpu, native_ext)
    p, g = _norm_operands(gpu, segs, numel)
    want = eo.ref_trust(p, g, segs, wd, eta, eps).to(gpu)
    assert [float(want[i]) for i in (2, 5, 7, 8)] == [1.0] * 4 and float(want[6]) != 1.0
    C.lars_norms(p.float(), g.float(), tb.table, tb.partials, tb.trust, 0, tb.nseg)
    tb.trust.fill_(9.0)
    C.lars_trust_only(tb.table, tb.partials, tb.trust, 0, tb.nseg, wd, eta, eps)
    ec.assert_exact(tb.trust[None], want[None], None, None, None, "lars_trust_only")
    tb.partials.fill_(-7.0)
    tb.trust.fill_(9.0)
    C.lars_trust(p.float(), g.float(), tb.table, tb.partials, tb.trust, 0, tb.nseg, wd, eta, eps)
    ec.assert_exact(tb.trust[None], want[None], None, None, None, "lars_trust")
    tb.trust.fill_(9.0)                                # a sub-range writes its own entries only
    C.lars_trust_only(tb.table, tb.partials, tb.trust, 3, 7, wd, eta, eps)
    sub = torch.full_like(want, 9.0)
    sub[3:7] = want[3:7]
    ec.assert_exact(tb.trust[None], sub[None], None, None, None, "lars_trust_only [3, 7)")


def test_lars_step_end_to_end_exact(gpu, native_ext):
    """p = 4 g, wd = 0, eps = 0, eta = 2^-4: every adapted trust is exactly 4 eta = 2^-2 and the three passes
    chain under the exact premise, Nesterov momentum, dampening and mirror included; the second step's
    gradient is p' / 4 again."""
    C = native_ext
    segs, numel, tb = _lars_table(gpu, native_ext)
    v = _lars_v(next(x for x in LARS_VARIANTS if x.id == "nesterov-mirror-d0.25-s1"))
    v.wd, eta = 0.0, 2.0 ** -4
    _, g1, _ = _lars_operands(gpu, numel)
    p0 = 4.0 * g1
    trust = eo.e2e_trust(segs, g1, eta)
    tr, wde, cov = eo.lars_elementwise(segs, numel, trust, 0.0, gpu)
    p1, b1 = eo.ref_update(p0, g1, None, v, True, trust=tr, wd=wde)
    g2 = p1 / 4.0
    eb.require_fp32(g2, "g2 = p' / 4")
    p2, b2 = eo.ref_update(p1, g2, b1, v, False, trust=tr, wd=wde)
    p = p0.float()
    buf = torch.full((numel,), eo.SENT_F32, device=gpu)
    mir = torch.full((numel,), eo.SENT_BF16, device=gpu, dtype=BF16)
    out = []
    for i, gd in enumerate((g1, g2)):
        tb.trust.fill_(9.0)
        C.lars_step(p, gd.float(), buf, tb.table, tb.partials, tb.trust, 0, tb.nseg, v.lr, v.momentum, v.dampening,
                    0.0, v.nesterov, i == 0, eta, 0.0, mir)
        ec.assert_exact(tb.trust[None], trust.float().to(gpu)[None], None, None, None, f"lars_step trust {i + 1}")
        out.append((p.clone(), buf.clone(), mir.clone()))
    _check_lars(out, [(p1, b1), (p2, b2)], p0, cov, v, "lars_step")


# ======================================================================== casts and weight images
@pytest.mark.parametrize("n", eo.CAST_SIZES)
def test_cast_to_bf16_exact(gpu, native_ext, n):
    """Every bf16 tie pattern with its two neighbours, +-0, fp32 subnormals, +-inf and random bits against
    torch's own round-to-nearest-even cast (made on the CPU)."""
    x = eo.cast_data(n, eo.CAST_SIZES.index(n))
    y = torch.full((n,), eo.SENT_BF16, dtype=BF16, device=gpu)
    native_ext.cast_to_bf16(x.to(gpu), y)
    _flat_eq(_bits(y), _bits(x.to(BF16)).to(gpu), f"cast_to_bf16 n={n}")


@pytest.mark.parametrize("channels_last", [True, False])
@pytest.mark.parametrize("shape", eo.PACK_SHAPES)
def test_pack_weight_exact(gpu, native_ext, shape, channels_last):
    """pack_weight (KRSC, zero fill up to cpad) and pack_weight_t (CRSK) against permute + torch's cast, from
    channels_last and contiguous strides."""
    C = native_ext
    k, c, r, s, cpad, with_t = shape
    w = eo.weight_data(k, c, r, s, k + c)
    wg = w.to(gpu).contiguous(memory_format=torch.channels_last) if channels_last else w.to(gpu).contiguous()
    got = C.pack_weight(wg, cpad)
    ec.assert_exact(_bits(got), _bits(eo.ref_pack_weight(w, cpad)).to(gpu), None, None, None, f"pack_weight {shape}")
    if with_t:
        ec.assert_exact(_bits(C.pack_weight_t(wg)), _bits(eo.ref_pack_weight_t(w)).to(gpu), None, None, None,
                        f"pack_weight_t {shape}")


def test_pack_t_batched_exact(gpu, native_ext):
    """One launch over a flat buffer of 33 tensors (partial k tiles, partial c tiles, both, 576 tiles on a
    512-block grid, max_tiles above the small tensors' counts): dst is view(K, RS, C).permute(2, 1, 0) of
    distinct 16-bit patterns, and the gaps between tensors keep their sentinel."""
    C = native_ext
    ent, total = eo.pack_t_layout()
    rows, max_tiles = eo.pack_t_table_rows(ent)
    assert max_tiles == 576
    dt = np.dtype([("off", "<i8"), ("K", "<i4"), ("C", "<i4"), ("RS", "<i4"), ("tk", "<i4"), ("tc", "<i4"),
                   ("pad", "<i4")])
    assert dt.itemsize == C.pack_t_entry_bytes()
    table = torch.from_numpy(np.array(rows, dtype=dt).view(np.uint8).copy()).to(gpu)
    src = eo.pack_t_src(total, gpu)
    sent = 0x5A5A
    dst = torch.full((total,), sent, dtype=torch.int16, device=gpu)
    C.pack_t_batched(src.view(BF16), dst.view(BF16), table, max_tiles)
    want = eo.ref_pack_t(src, ent, sent)
    if not torch.equal(dst, want):
        for o, k, c, rs in ent:
            n = k * c * rs
            ec.assert_exact(dst[o:o + n].view(c * rs, k), want[o:o + n].view(c * rs, k), rs, 64, None,
                            f"pack_t_batched K={k} C={c} RS={rs} (rows are c * RS + tap)")
        _flat_eq(dst, want, "pack_t_batched gaps")


# ============================================================================================ fp8
def _state(C, gpu):
    return torch.zeros(C.fp8_state_floats(), device=gpu), C.fp8_deq_offset()


def test_fp8_state_layout(native_ext):
    assert native_ext.fp8_deq_offset() == 3 * eo.SLOT_FLOATS
    assert native_ext.fp8_state_floats() == 3 * eo.SLOT_FLOATS + 4


@pytest.mark.parametrize("nvec", eo.QUANT_NVEC)
def test_quant_e4m3_sizes_and_amax_places(gpu, native_ext, nvec):
    """The amax element in the first vector, the last vector and a block of index >= 64 in turn: the codes
    of the call (scale 1) and of the next one (the delayed scale), the slot's amax, deq and the cleared
    next slot."""
    C = native_ext
    for wi, where in enumerate(eo.amax_places(nvec)):
        amax = (100.0, 3.0, 0.75)[wi]
        s1 = eo.scale_for(amax)
        state, D = _state(C, gpu)
        x0 = eo.quant_data(nvec, amax, where, seed=wi)
        x1 = eo.quant_data(nvec, 2.0 * amax, nvec - 1 - where, seed=wi + 3, s_next=s1)
        what = f"quant_e4m3 nvec={nvec} amax at vector {where}"
        q0 = C.quant_e4m3(x0.to(gpu), state, 0)
        _flat_eq(q0, eo.q_e4m3(x0).to(gpu), what + " call 0")
        eo.check_state(state, 0, D, 1.0, amax, what + " call 0")
        q1 = C.quant_e4m3(x1.to(gpu), state, 1)
        _flat_eq(q1, eo.q_e4m3(x1, s1).to(gpu), what + " call 1")
        eo.check_state(state, 1, D, s1, 2.0 * amax, what + " call 1")


def test_quant_e4m3_five_call_rotation(gpu, native_ext):
    """amax 100, 1, 2^-7, 0, 50 on one state: all three slots, the rotation, the cleared next slot, and the
    call after the all-zero one back at scale 1."""
    C = native_ext
    state, D = _state(C, gpu)
    prev = 0.0
    for t, amax in enumerate([100.0, 1.0, 2.0 ** -7, 0.0, 50.0]):
        s = eo.scale_for(prev)
        x = eo.quant_data(255, amax, (37 * t) % 255, seed=t, s_next=s)
        q = C.quant_e4m3(x.to(gpu), state, t % 3)
        _flat_eq(q, eo.q_e4m3(x, s).to(gpu), f"call {t} (amax {amax}, scale {s})")
        eo.check_state(state, t % 3, D, s, amax, f"call {t}")
        prev = amax
    assert eo.scale_for(0.0) == 1.0 and s == 1.0


def test_quant_e4m3_scale_boundaries_and_clamps(gpu, native_ext):
    """A chain of calls whose amax walks 448, 224, 7, 3.5 and 0.4375 with each one's bf16 neighbour below
    and above, then 2^-40 (the scale clamps to 2^32) and 2^127 (clamps to 2^-32; the codes saturate to
    +-448, no NaN byte): the scale of each next call steps exactly at the boundary."""
    C = native_ext
    state, D = _state(C, gpu)
    chain = eo.boundary_chain(eo.E4M3_BOUNDARIES) + [2.0 ** -40, 2.0 ** 127, 1.0]
    scales = [eo.scale_for(a) for a in chain]
    assert scales[chain.index(224.0)] == 1.0 and scales[chain.index(224.0) + 1] == 0.5
    assert scales[chain.index(2.0 ** -40)] == 2.0 ** 32 and scales[chain.index(2.0 ** 127)] == 2.0 ** -32
    prev = 0.0
    for t, amax in enumerate(chain):
        s = eo.scale_for(prev)
        x = eo.quant_data(3, amax, t % 3, seed=t, s_next=s)
        q = C.quant_e4m3(x.to(gpu), state, t % 3)
        want = eo.q_e4m3(x, s)
        assert not bool(((want & 0x7F) == 0x7F).any())
        _flat_eq(q, want.to(gpu), f"call {t}: amax {amax}, previous {prev}, scale {s}")
        eo.check_state(state, t % 3, D, s, amax, f"call {t} (previous amax {prev})")
        if prev == 2.0 ** 127:
            assert int((q & 0x7F).max()) <= 0x7E
        prev = amax
    big = torch.full((1, 1, 1, 8), 2.0 ** 127, dtype=BF16)          # 2^127 * 2^-32 saturates
    big[..., 1::2] *= -1
    state2, _ = _state(C, gpu)
    C.quant_e4m3(big.to(gpu), state2, 0)
    q = C.quant_e4m3(big.to(gpu), state2, 1)
    eo.check_state(state2, 1, D, 2.0 ** -32, 2.0 ** 127, "2^127 twice")
    assert q.flatten().tolist() == [0x7E, 0xFE] * 4


def test_quant_e4m3_ties_and_subnormals(gpu, native_ext):
    """Every midpoint between two neighbouring e4m3 values (subnormals included), of both signs, divided by
    the scale in force: each must round to the even code."""
    C = native_ext
    mids = torch.tensor(eo.e4m3_midpoints(), dtype=torch.float64)
    for amax_prev in (0.0, 14.0, 1792.0):              # scales 1, 16, 2^-3
        s = eo.scale_for(amax_prev)
        vals = torch.cat([mids, -mids]) / s
        vals = vals[(vals.abs() * s < 448.0) & (ec.to_bf16(vals).double() == vals)]
        assert vals.numel() >= 200
        x = torch.zeros(256, dtype=torch.float64)
        x[:vals.numel()] = vals
        x = x.to(BF16).reshape(1, 1, 32, 8)
        state, D = _state(C, gpu)
        C.quant_e4m3(torch.full((1, 1, 1, 8), amax_prev, dtype=BF16, device=gpu), state, 0)
        q = C.quant_e4m3(x.to(gpu), state, 1)
        want = eo.q_e4m3(x, s)
        assert bool((want.flatten()[:vals.numel()] & 1 == 0).all())       # the reference rounds to even
        _flat_eq(q, want.to(gpu), f"ties at scale {s}")


Q8_FWD_SHAPES = [(1, 1, 1, 8), (2, 3, 5, 40), (1, 8, 16385 + 3, 64)]      # the last: 256 * 4096 + 192 vectors
Q8_FWD_FORMS = {"plain": (False, False, False, True), "relu": (False, True, False, True),
                "res": (True, False, False, True), "res_relu_mask": (True, True, True, True),
                "relu_mask_noz": (False, True, True, False), "res_noz": (True, False, False, False)}


@pytest.mark.parametrize("form", list(Q8_FWD_FORMS))
@pytest.mark.parametrize("nhwk", Q8_FWD_SHAPES)
def test_bn_act_fwd_q8_exact(gpu, native_ext, nhwk, form):
    """Two consecutive calls (quartered coefficients first, so the second runs at a non-unit scale): z equals
    bn_act_fwd's and the exact reference, q is the e4m3 of the STORED bf16 z times the delayed scale, the
    mask bits are z > 0, and want_z=False returns no z."""
    C = native_ext
    res, relu, mask, want_z = Q8_FWD_FORMS[form]
    k = nhwk[3]
    y, yd = _cached(("q8y", nhwk), lambda: ec.int_tensor(nhwk, (-20, 20), 1, gpu))
    r, rd = _cached(("q8r", nhwk), lambda: ec.int_tensor(nhwk, (-20, 20), 2, gpu)) if res else (None, None)
    scale, shift = eb.craft_fwd(k, 3, gpu)
    state, D = _state(C, gpu)
    prev = 0.0
    for t, f in enumerate((0.25, 1.0)):
        want = eb.ref_bn_fwd(yd, scale * f, shift * f, rd, relu)
        s = eo.scale_for(prev)
        z, q, zm = C.bn_act_fwd_q8(y, _f32(scale * f), _f32(shift * f), r, relu, state, t, mask, want_z)
        what = f"bn_act_fwd_q8 {nhwk} {form} call {t} scale {s}"
        if want_z:
            ec.assert_exact(z, want, None, None, None, what + " z")
            assert torch.equal(z, C.bn_act_fwd(y, _f32(scale * f), _f32(shift * f), r, relu)), what
        else:
            assert z is None
        ec.assert_exact(q, eo.q_e4m3(want, s), None, None, None, what + " q")
        if mask:
            assert torch.equal(zm, eb.bitmask(want > 0)), what + " mask"
        else:
            assert zm is None
        prev = float(want.float().abs().max())
        eo.check_state(state, t, D, s, prev, what)
    assert s != 1.0 or nhwk == (1, 1, 1, 8)


Q8_BWD_SHAPES = [(2, 4, 8, 64), (4, 8, 8, 2048), (1, 1, 1, 8)]            # M = 64, 256, 1: 1 / M is exact


@pytest.mark.parametrize("mask", [0, 1, 2])
@pytest.mark.parametrize("nhwk", Q8_BWD_SHAPES)
def test_bn_act_bwd_apply_q8_exact(gpu, native_ext, nhwk, mask):
    """The exact BN backward-apply construction through the fp8 variant, two consecutive calls: dy and dres
    bit for bit, dy8 the e5m2 of the STORED bf16 dy times the delayed scale (headroom 28672), want_dy=False,
    and the dgamma / dbeta sinks."""
    C = native_ext
    n, h, w, k = nhwk
    c = _cached(("q8coef", k, n * h * w), lambda: eb.craft(k, n * h * w, 20, gpu))
    dz, dzd = _cached(("q8dz", nhwk), lambda: ec.int_tensor(nhwk, (-200, 200), 21, gpu))
    y, yd = _cached(("q8by", nhwk), lambda: ec.int_tensor(nhwk, (-20, 20), 22, gpu))
    z, zd = (torch.relu(t) for t in _cached(("q8bz", nhwk), lambda: ec.int_tensor(nhwk, (-2, 2), 23, gpu)))
    on = eb.mask_on(mask, zd, yd, c.scale, c.shift)
    want, g = eb.exact_bwd_apply(c, dzd, yd, on, True)
    dyw = ec.to_bf16(want)
    amax = float(dyw.float().abs().max())
    state, D = _state(C, gpu)
    _, dg0 = ec.int_tensor((k,), (-50, 50), 24, gpu, torch.float32)
    _, db0 = ec.int_tensor((k,), (-50, 50), 25, gpu, torch.float32)
    dg_want, db_want = eb.ref_sinks(c, dg0, db0)
    prev = 0.0
    for t, (want_dres, want_dy, sinks) in enumerate([(True, True, False), (False, True, True), (True, False, False)]):
        s = eo.scale_for(prev, eo.E5M2_HEADROOM)
        dg, db = dg0.float(), db0.float()
        dy, dres, dy8 = C.bn_act_bwd_apply_q8(dz, z, y, c.stats, c.gamma, c.sums, mask, want_dres, state, t, want_dy,
                                              dg if sinks else None, db if sinks else None)
        what = f"bn_act_bwd_apply_q8 {nhwk} mask={mask} call {t} scale {s}"
        if want_dy:
            ec.assert_exact(dy, dyw, None, None, None, what + " dy")
        else:
            assert dy is None
        if want_dres:
            ec.assert_exact(dres, ec.to_bf16(g), None, None, None, what + " dres")
        else:
            assert dres is None
        ec.assert_exact(dy8, eo.q_e5m2(dyw, s), None, None, None, what + " dy8")
        if sinks:
            ec.assert_exact(dg[None], dg_want[None], None, None, None, what + " dgamma")
            ec.assert_exact(db[None], db_want[None], None, None, None, what + " dbeta")
        eo.check_state(state, t, D, s, amax, what)
        prev = amax
    assert amax == 0.0 or s != 1.0


def test_bn_act_bwd_apply_q8_scale_boundaries(gpu, native_ext):
    """Identity coefficients (dy = dz): the amax of dy walks 28672 * 2^-k with each one's bf16 neighbours;
    the e5m2 scale of each next call steps exactly at the boundary."""
    C = native_ext
    k = 8
    one, zero = torch.ones(k, dtype=torch.float64, device=gpu), torch.zeros(k, dtype=torch.float64, device=gpu)
    c = eb.pack_coefs(zero, one, one, zero, zero, one, zero, 4)
    chain = eo.boundary_chain(eo.E5M2_BOUNDARIES) + [1.0]
    i = chain.index(28672.0)
    assert (eo.scale_for(chain[i], eo.E5M2_HEADROOM), eo.scale_for(chain[i + 1], eo.E5M2_HEADROOM)) == (1.0, 0.5)
    state, D = _state(C, gpu)
    prev = 0.0
    for t, amax in enumerate(chain):
        s = eo.scale_for(prev, eo.E5M2_HEADROOM)
        dzd = (amax * torch.tensor([1.0, -0.5, 0.25, 0.0, 0.125, -0.5, 0.5, 0.25] * 4, dtype=torch.float64))
        dzd = dzd.reshape(1, 2, 2, k)
        dz = dzd.to(BF16).to(gpu)
        assert torch.equal(dz.double().cpu(), dzd)
        dy, _, dy8 = C.bn_act_bwd_apply_q8(dz, dz, dz, c.stats, c.gamma, c.sums, 0, False, state, t % 3)
        what = f"call {t}: amax {amax}, previous {prev}, scale {s}"
        ec.assert_exact(dy, dz, None, None, None, what + " dy")
        ec.assert_exact(dy8, eo.q_e5m2(dz, s), None, None, None, what + " dy8")
        eo.check_state(state, t % 3, D, s, amax, what)
        prev = amax


def test_quant_rows_e4m3_exact(gpu, native_ext):
    """One launch over a flat bf16 buffer of 7 tensors (row lengths 8, 72, 576, 4608; 1, 3, 4 and 5 rows,
    max_rows above the small ones): the scale is one fp32 division, exactly; rows with amax 448 * 2^k
    divide exactly and their largest element codes to +-448; a zero row has scale 1 and codes 0; general
    rows match the same two fp32 operations (inv = 1 / sc, x * inv) made on the CPU; the bytes between
    tensors and the scale entries past the last row keep their sentinel."""
    C = native_ext
    ent, total, nscale = eo.qrows_layout()
    src, kinds = eo.qrows_data(ent, total)
    assert {kd for _, _, kd in kinds} == {"zero", "pow2", "general"}
    dt = np.dtype([("off", "<i8"), ("soff", "<i8"), ("rows", "<i4"), ("rowlen", "<i4")])
    assert dt.itemsize == C.quant_rows_entry_bytes()
    table = torch.from_numpy(np.array(ent, dtype=dt).view(np.uint8).copy()).to(gpu)
    dst = torch.full((total,), eo.SENT_U8, dtype=torch.uint8, device=gpu)
    scale = torch.full((nscale + 8,), eo.SENT_F32, device=gpu)
    C.quant_rows_e4m3(src.to(gpu), dst, scale, table, max(r for r, _ in eo.QROWS_TENSORS))
    want, wscale = eo.ref_qrows(src, ent, total, nscale)
    _flat_eq(scale[:nscale], wscale.to(gpu), "quant_rows scale")
    assert bool((scale[nscale:] == eo.SENT_F32).all())
    dst = dst.cpu()
    for ti, r, kind in kinds:
        o, so, rows, rl = ent[ti]
        row, code = src[o + r * rl:o + (r + 1) * rl].float(), dst[o + r * rl:o + (r + 1) * rl]
        if kind == "zero":
            assert float(wscale[so + r]) == 1.0 and not bool(code.any())
        if kind == "pow2":
            amax = float(row.abs().max())
            assert float(scale[so + r]) == amax / 448.0
            assert torch.equal(code, eo.q_e4m3(row, 448.0 / amax)), f"tensor {ti} row {r}"
            assert int(code[row.abs().argmax()] & 0x7F) == 0x7E
    _flat_eq(dst, want, "quant_rows codes and gaps")


@pytest.mark.parametrize("act_deq", [None, 0.25, 0.3])
@pytest.mark.parametrize("channels_last", [True, False])
@pytest.mark.parametrize("shape", eo.WFP8_SHAPES)
def test_pack_weight_fp8_exact(gpu, native_ext, shape, channels_last, act_deq):
    """Codes and scales in the kernel's own fp32 arithmetic (scale = amax / 448, inv = 1 / scale, w * inv):
    zero fill above C, an all-zero output channel (scale 1), a channel whose amax is 448 * 2^-6 (exact, its
    largest element -448), oscale = scale * act_deq."""
    C = native_ext
    k, c, r, s, cpad = shape
    w = eo.wfp8_data(k, c, r, s, k)
    wg = w.to(gpu).contiguous(memory_format=torch.channels_last) if channels_last else w.to(gpu).contiguous()
    ad = None if act_deq is None else torch.tensor([act_deq])
    wq, osc = C.pack_weight_fp8(wg, cpad, None if ad is None else ad.to(gpu))
    want, wosc = eo.ref_wfp8(w, cpad, ad)
    _flat_eq(osc, wosc.to(gpu), f"pack_weight_fp8 {shape} oscale")
    ec.assert_exact(wq.view(k, -1), want.view(k, -1).to(gpu), None, None, None, f"pack_weight_fp8 {shape}")
    assert float(wosc[1]) == (1.0 if ad is None else float(ad)) and not bool(want[1].any())
    assert float(wosc[0] / (1.0 if ad is None else ad)) == 2.0 ** -6 and int(want[0].max()) == 0xFE
