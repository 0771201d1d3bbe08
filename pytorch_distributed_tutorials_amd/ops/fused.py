"""Fused ResNet building blocks as autograd Functions.

Each function dispatches on the device of its input:
  * device tensor -> the HIP kernels of the native extension (``_C``); a missing
    extension raises (``_ext.native()``), never silently falls back;
  * CPU tensor    -> ``ops.reference`` (PyTorch), which defines the semantics.

The unit of fusion is ``conv -> BatchNorm(batch stats) -> (+residual) -> ReLU``
(SURVEY.md §3.5 fusion points).  Forward launches: weight pack, implicit-GEMM
conv with per-tile BN partial statistics in its epilogue, a tiny stats
finalize (which also updates the running buffers), one fused
normalize/add/ReLU pass.  Backward: one reduction pass (dgamma, dbeta), one
elementwise pass producing dy (and the residual-branch gradient), then the
dgrad and wgrad implicit GEMMs.
"""
from __future__ import annotations

import os
import weakref
from typing import Optional

import torch
import torch.nn as nn

from . import reference as ref
from . import streams
from ..data.mix import MixedTarget
from ..utils.seed import deterministic
from ._ext import native, native_mix

_CPU_DTYPE = torch.float32  # activation dtype of the CPU reference path
# Module switches: the ones tests, scripts or the README's knob table set.
_NAN_TRACE = os.environ.get("PDT_NAN_TRACE", "0") == "1"  # debug: report NaN in saved tensors
_STEM_POOL = True  # debugging switch (default on): BN + ReLU + max pool of the stem in one pass
_FP8 = False  # forward convolutions on the MX-rate fp8 MFMA (set_fp8)
_FP8_BWD = True  # with fp8: also the input-gradient GEMMs
# with fp8 backward: weight gradients on the MX-rate MFMA from the e5m2 dy and the e4m3 conv input
# the forward already produced (igemm_tn_f8_kernel); deterministic runs keep the bf16 slab path
_FP8_WGRAD = True
# fp8-only storage: activations / input gradients whose every consumer reads the fp8 copy are not
# written in bf16 at all (interior bottleneck outputs, and dy of convs with fp8 dgrad + fp8 wgrad)
_FP8_ONLY = True
_FP8_KMIN = 128  # least GEMM K of an fp8 forward conv (_fp8_conv_ok)
_FP8_DGRAD_NARROW = True  # fp8 input gradients also for k % 16 channels at stride 1 (_fp8_dgrad_ok)
# _BN_ACC (non-deterministic runs only; deterministic runs always take the partial buffers):
# BN-backward sums of a BN-fused dgrad accumulated by its epilogue's fp32 atomics into a per-BN
# [2, C] buffer -- no partial buffer and no reduce launch on the main stream; the consuming apply
# adds the BN parameter gradients, and the buffer is re-zeroed on the weight-gradient side stream
# once the apply is done.  Round 3 measured it neutral (r3t); with round 4's kernels it pays
# (r4ab, interleaved: 18.78 / 18.72 ms on vs 18.86 / 18.85 off), so on.
_BN_ACC = True
# the projection-shortcut BN's backward sums taken in the next block's hand-off dgrad epilogue (the
# same output gradient g feeds both BNs of a downsampling block): no reduction pass over g and y_ds
_DUAL_BN = os.environ.get("PDT_DUAL_BN", "1") == "1"  # (A/B knob)
DUAL_CALLS = 0  # shortcut BNs whose backward sums came from the hand-off epilogue (tests)
# Fold the last unit's BN backward into its 1x1 input gradient (DgradFold) -- ResNet-50 b256 in the
# same calls: 18.15 vs 18.29 and 18.27 vs 18.54 ms/step (r6r / r6s); removing that apply altogether
# bounds the gain at 1.47 ms (r6f), the rest is spent in the fold-weight kernels on the critical
# stream (~20 us per block in-step) and the larger dgrad K.
_FOLD_BN = True
FOLD_CALLS = 0  # folded units so far (tests check that the path engaged)
# test hook (tests/test_blocks_gpu.py, mask-matched reference): when a list, every fused block
# forward appends its units' stored post-activation outputs (z, NHWC bf16), so an fp32 reference
# can take the native path's ReLU decisions and compare gradients without ReLU-flip noise
_CAPTURE = None
# diagnostic hook (bench.py PDT_DIAG_LEAD=1): when a list, every block forward / backward appends
# (tag, host perf_counter, timing event recorded on the current stream at its entry), so the host's
# lead over the device can be read per block after the run
_LEAD = None


def _bacc(p, c):
    """The zeroed [2, C] fp32 BN-backward sum accumulator of BatchNorm weight ``p``."""
    a = getattr(p, "_pdt_bacc", None)
    if a is None or a.numel() != 2 * c or a.device != p.device:
        a = torch.zeros(2, c, dtype=torch.float32, device=p.device)
        p._pdt_bacc = a
    return a


def _facc(p, c):
    """The zeroed fp64 [8, 2, C] forward BN-sum accumulator of BatchNorm weight ``p``: the conv
    producing the BN input adds its per-channel sums into it (one slot per XCD) and the finalize
    that reads them re-zeroes it (kernels.h BnFwdFuse)."""
    a = getattr(p, "_pdt_facc", None)
    if a is None or a.numel() != 16 * c or a.device != p.device:
        a = torch.zeros(8, 2, c, dtype=torch.float64, device=p.device)  # one slot per XCD
        p._pdt_facc = a
    return a


def _lead_mark(tag: str) -> None:
    import time
    ev = torch.cuda.Event(enable_timing=True)
    ev.record()
    _LEAD.append((tag, time.perf_counter(), ev))


def set_fp8(on: bool) -> None:
    """fp8 forward convolutions: activations e4m3 with delayed per-tensor scaling (emitted by the
    producing BatchNorm apply), weights e4m3 with per-output-channel scales, fp32 accumulation on
    v_mfma_f32_16x16x128_f8f6f4, bf16 output; backward GEMMs stay bf16 on the saved bf16 tensors."""
    global _FP8
    _FP8 = bool(on)


def fp8_enabled() -> bool:
    return _FP8


_Q8_STATES: list = []  # weak references to every _Q8State, creation order (fp8_phase_signature)


class _Q8State:
    """Delayed-scaling state of one fp8 activation producer (csrc/kernels/fp8.hip contract)."""

    __slots__ = ("buf", "t", "off", "__weakref__")

    def __init__(self, device):
        C = native()
        self.buf = torch.zeros(C.fp8_state_floats(), dtype=torch.float32, device=device)
        self.off = C.fp8_deq_offset()
        self.t = 0
        _Q8_STATES.append(weakref.ref(self))

    def next_slot(self) -> int:
        slot = self.t % 3
        self.t += 1
        return slot

    def deq(self, slot: int) -> torch.Tensor:
        return self.buf.narrow(0, self.off + slot, 1)


def fp8_ring_state() -> tuple:
    """Step counter of every live delayed-scaling slot ring (creation order): the host state a
    captured fp8 step bakes in (utils.graph.CapturedStep ``ring``)."""
    _Q8_STATES[:] = [r for r in _Q8_STATES if r() is not None]
    return tuple(r().t for r in _Q8_STATES)


def fp8_set_ring_state(ts: tuple) -> None:
    """Set the step counters read by fp8_ring_state (same order)."""
    live = [r() for r in _Q8_STATES if r() is not None]
    for st, t in zip(live, ts):
        st.t = t


FP8_RING = (fp8_ring_state, fp8_set_ring_state)


def _q8_state(owner, device, attr: str = "_pdt_q8") -> _Q8State:
    """Delayed-scaling state kept on ``owner`` (a module for forward activations, the BN gamma
    Parameter for backward gradients)."""
    st = getattr(owner, attr, None)
    if st is None or st.buf.device != device:
        st = _Q8State(device)
        setattr(owner, attr, st)
    return st


def _rows_e4m3(C, src2d: torch.Tensor):
    """Row-wise e4m3 quantization of one bf16 [rows, n] image (fallback when no flat mirror)."""
    import numpy as np
    rows, n = src2d.shape
    dt = np.dtype([("off", "<i8"), ("soff", "<i8"), ("rows", "<i4"), ("rowlen", "<i4")])
    tab = torch.from_numpy(np.array([(0, 0, rows, n)], dtype=dt).view(np.uint8).copy()).to(src2d.device)
    q = torch.empty(src2d.numel(), dtype=torch.uint8, device=src2d.device)
    sc = torch.empty(rows, dtype=torch.float32, device=src2d.device)
    C.quant_rows_e4m3(src2d.reshape(-1), q, sc, tab, rows)
    return q, sc


def _packed_krsc8(C, w, cx):
    """(e4m3 [K,R,S,Cx], per-K scale) forward weights: flat-mirror view or a fresh pack."""
    m = _mirror_of(w)
    v = m.krsc8_view(w) if m is not None and w.shape[1] == cx else None
    if v is not None:
        return v
    return C.pack_weight_fp8(w, cx)


def _packed_crsk8(C, w):
    """(e4m3 [C,R,S,K], per-C scale) dgrad weights: flat-mirror view or a fresh pack."""
    m = _mirror_of(w)
    v = m.crsk8_view(w) if m is not None else None
    if v is not None:
        return v
    k, c, r, s = w.shape
    q, sc = _rows_e4m3(C, C.pack_weight_t(w).view(c, r * s * k))
    return q.view(c, r, s, k), sc


def fp8_attach(x: torch.Tensor, owner: nn.Module) -> torch.Tensor:
    """Attach an e4m3 copy of the NHWC activation ``x`` (for the fp8 convs that consume it)."""
    if _FP8 and x.is_cuda and x.dim() == 4 and x.shape[3] % 16 == 0:
        st = _q8_state(owner, x.device)
        slot = st.next_slot()
        x._pdt_fp8 = (native().quant_e4m3(x, st.buf, slot), st.deq(slot))
    return x


def _nan_trace(tag, **tensors):
    if not _NAN_TRACE:
        return
    torch.cuda.synchronize()
    bad = [k for k, t in tensors.items() if t is not None and t.is_floating_point() and bool(torch.isnan(t).any())]
    if bad:
        print(f"[nan-trace] {tag}: NaN in {bad}", flush=True)


def set_cpu_activation_dtype(dtype: torch.dtype) -> None:
    global _CPU_DTYPE
    _CPU_DTYPE = dtype


def act_dtype(device: torch.device) -> torch.dtype:
    return torch.bfloat16 if device.type == "cuda" else _CPU_DTYPE


# ----------------------------------------------------------------------------
# image -> NHWC
# ----------------------------------------------------------------------------
def image_to_nhwc(x: torch.Tensor) -> torch.Tensor:
    """NCHW float image -> NHWC activation with C padded to 8 (no grad needed)."""
    if x.is_cuda:
        return native().image_to_nhwc(x.contiguous())
    return ref.image_to_nhwc(x, _CPU_DTYPE)


# ----------------------------------------------------------------------------
# conv + BN + (residual) + ReLU
# ----------------------------------------------------------------------------
class _ConvBN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, gamma, beta, residual, running_mean, running_var,
                stride, pad, relu, training, momentum, eps):
        k, c, r, s = weight.shape
        n, h, w, cx = x.shape
        count = n * ((h + 2 * pad - r) // stride + 1) * ((w + 2 * pad - s) // stride + 1)
        if x.is_cuda:
            C = native()
            wk = C.pack_weight(weight, cx)                       # bf16 [K,R,S,Cx]
            if training:
                buffers_ready()
                if running_mean is None:  # track_running_stats=False: updates go to scratch
                    running_mean = torch.zeros(k, device=x.device)
                    running_var = torch.ones(k, device=x.device)
                # the fused block's conv + statistics call (same kernels, same rounding)
                y, stats = C.conv_fwd_bn(x, wk, stride, pad, count, running_mean, running_var, gamma, beta,
                                         float(momentum), float(eps),
                                         None if deterministic() else _facc(gamma, k))
            else:
                y, _ = C.conv_fwd(x, wk, stride, pad, False)
                buffers_ready()
                stats = C.bn_eval_params(running_mean, running_var, gamma, beta, float(eps))
            mean, invstd, scale, shift = stats.unbind(0)
            z = C.bn_act_fwd(y, scale, shift, residual, relu)
        else:
            wk = None
            y = ref.conv2d_nhwc(x, weight, stride, pad).to(x.dtype)
            if training:
                mean, var = ref.bn_batch_stats(y)
                with torch.no_grad():
                    unbiased = var * count / max(count - 1, 1)
                    running_mean.mul_(1 - momentum).add_(mean, alpha=momentum)
                    running_var.mul_(1 - momentum).add_(unbiased, alpha=momentum)
            else:
                mean, var = running_mean.float(), running_var.float()
            invstd = torch.rsqrt(var + eps)
            z = ref.bn_act_fwd(y, mean, invstd, gamma, beta, residual, relu, x.dtype)
            sc = gamma.float() * invstd
            stats = torch.stack([mean, invstd, sc, beta.float() - mean * sc])
        ctx.save_for_backward(x, weight, y, z, stats, gamma)
        ctx.cfg = (stride, pad, relu, training, residual is not None)
        return z

    @staticmethod
    def backward(ctx, dz):
        x, weight, y, z, stats, gamma = ctx.saved_tensors
        mean, invstd = stats[0], stats[1]
        stride, pad, relu, training, has_res = ctx.cfg
        dz = dz.contiguous()
        need_x = ctx.needs_input_grad[0]
        need_w = ctx.needs_input_grad[1]
        if dz.is_cuda:
            C = native()
            # ReLU mask: from z when a residual was added, else recomputed from y (no z read)
            mask = (1 if has_res else 2) if relu else 0
            sums = C.bn_act_bwd_reduce(dz, z, y, stats, mask)    # [sum g, sum g*(y-mean)]
            dbeta, dgamma = sums[0], sums[1] * invstd
            dy, dres = C.bn_act_bwd_apply(dz, z, y, stats, gamma, sums, mask, training, has_res)
            dx = C.conv_dgrad(dy, weight, list(x.shape), stride, pad) if need_x else None
            dw = C.conv_wgrad(dy, x, list(weight.shape), stride, pad, deterministic()) \
                if need_w else None
        else:
            dy, dgamma, dbeta, dres = ref.bn_act_bwd(dz, z, y, mean, invstd, gamma, relu,
                                                     training, has_res, x.dtype)
            dx = ref.conv2d_nhwc_dgrad(dy, weight, x.shape, stride, pad).to(x.dtype) if need_x else None
            dw = ref.conv2d_nhwc_wgrad(dy, x, weight.shape, stride, pad) if need_w else None
            if dw is not None:
                dw = dw.contiguous(memory_format=torch.channels_last) \
                    if weight.is_contiguous(memory_format=torch.channels_last) else dw
        if dw is not None:
            dw = dw.to(weight.dtype)
        return (dx, dw, dgamma.to(gamma.dtype), dbeta.to(gamma.dtype), dres,
                None, None, None, None, None, None, None, None)


def _grad_sink(p):
    """Flat-buffer gradient view to accumulate into, if the parameter lives in a FlatParamSpace."""
    sp = getattr(p, "_pdt_flat", None)
    if sp is None or not p.requires_grad or not p.is_cuda:
        return None
    return sp.grad_sink(p)


def _wgrad_into(p, sunk, fn, *args):
    """Weight gradient ``fn(*args)`` of parameter ``p``: accumulated into its flat-space gradient sink
    (``fn(*args, sink)``; p goes to ``sunk`` for ``mark_ready``) -> None, or without one returned in p's dtype."""
    sink = _grad_sink(p)
    if sink is None:
        return fn(*args).to(p.dtype)
    fn(*args, sink)
    sunk.append(p)
    return None


def _bn_dest(p_gamma, p_beta, atomic):
    """Where a BatchNorm's dgamma / dbeta go.  None: no flat-space sinks, autograd gets them back.  Else
    (acc, sg, sb): into the sinks sg / sb -- by the reducing kernel itself (acc None), or with ``atomic``
    by the BN's apply pass from the [2, C] accumulator ``acc`` that a dgrad epilogue's atomics fill."""
    sg, sb = _grad_sink(p_gamma), _grad_sink(p_beta)
    if sg is None or sb is None:
        return None
    return (_bacc(p_gamma, p_gamma.shape[0]) if atomic else None), sg, sb


def _stem_conv_stats(C, x, weight, gamma, beta, running_mean, running_var, stride, pad, training, momentum, eps):
    """Super-pixel stem conv -> BN statistics (finalize + running-stat update, or the eval
    parameters): (xsp, y, part, stats[4, K])."""
    xsp, y, part, grows = C.stem_conv_fwd(x, weight, stride, pad, training)
    count = y.shape[0] * y.shape[1] * y.shape[2]
    buffers_ready()
    if training:
        if running_mean is None:
            running_mean = torch.zeros(weight.shape[0], device=x.device)
            running_var = torch.ones(weight.shape[0], device=x.device)
        stats = C.bn_finalize(part, count, running_mean, running_var, gamma, beta, float(momentum), float(eps), grows)
    else:
        stats = C.bn_eval_params(running_mean, running_var, gamma, beta, float(eps))
    return xsp, y, part, stats


class _StemConvBN(torch.autograd.Function):
    """Device stem: NCHW fp32 image -> conv 7x7/s2 -> BN -> ReLU as a super-pixel conv.

    The image is re-laid out so pairs of horizontally adjacent pixels form one 8-channel
    "super-pixel" (3 channels + pad each), the seven horizontal taps fold into four tap pairs,
    and the image is pre-padded: the implicit GEMM has K = 7*4*8 = 224 (vs 7*7*8 = 392 with
    channel padding alone) and no bounds checks.  The image itself needs no gradient.
    """

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, running_mean, running_var, stride, pad, training,
                momentum, eps):
        C = native()
        xsp, y, part, stats = _stem_conv_stats(C, x, weight, gamma, beta, running_mean, running_var, stride, pad,
                                               training, momentum, eps)
        z = C.bn_act_fwd(y, stats[2], stats[3], None, True)
        _nan_trace("stem", x=x, xsp=xsp, y=y, part=part, stats=stats, z=z)
        ctx.save_for_backward(xsp, y, stats, gamma)
        ctx.weight = weight
        ctx.training = training
        return z

    @staticmethod
    def backward(ctx, dz):
        C = native()
        xsp, y, stats, gamma = ctx.saved_tensors
        weight = ctx.weight
        dz = dz.contiguous()
        sums = C.bn_act_bwd_reduce(dz, dz, y, stats, 2)
        dgamma, dbeta = sums[1] * stats[1], sums[0]
        dy, _ = C.bn_act_bwd_apply(dz, dz, y, stats, gamma, sums, 2, ctx.training, False)
        dw = None
        if ctx.needs_input_grad[1]:
            sunk = []
            dw = _wgrad_into(weight, sunk, C.stem_wgrad, dy, xsp, list(weight.shape), deterministic())
            if sunk:
                weight._pdt_flat.mark_ready(sunk)
        ctx.weight = None
        return (None, dw, dgamma.to(gamma.dtype), dbeta.to(gamma.dtype), None, None, None, None,
                None, None, None)


def _end_mirror_trust(weight) -> None:
    """The stem's backward is the native model's last backward node: end the bf16 weight mirror's
    per-step trust (parallel/flat.py WeightMirror.end_trust)."""
    sp = getattr(weight, "_pdt_flat", None)
    m = getattr(sp, "_mirror", None) if sp is not None else None
    if m is not None:
        m.end_trust()


class _StemConvBNPool(torch.autograd.Function):
    """_StemConvBN followed by the 3x3/s2/p1 max pool in ONE fused BN-apply/ReLU/pool pass.

    The full-resolution ReLU output (112x112x64 per image) is never written: forward normalises,
    rectifies and pools each window in registers (``bn_relu_maxpool``), backward gathers the
    pooled gradient back through the argmax inside the BN reduction and apply passes
    (``pool_bn_bwd_reduce`` / ``pool_bn_bwd_apply``).  Saves writing z and dz and reading each
    of them back (~1.6 GB of HBM traffic per step at batch 256).
    """

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, running_mean, running_var, stride, pad, training,
                momentum, eps):
        C = native()
        xsp, y, part, stats = _stem_conv_stats(C, x, weight, gamma, beta, running_mean, running_var, stride, pad,
                                               training, momentum, eps)
        if training:  # also u = y at each window's argmax, for the backward reduction
            out, idx, u = C.bn_relu_maxpool(y, stats[2], stats[3], True)
        else:
            (out, idx), u = C.bn_relu_maxpool(y, stats[2], stats[3]), None
        _nan_trace("stem+pool", x=x, xsp=xsp, y=y, part=part, stats=stats, out=out)
        ctx.save_for_backward(xsp, y, stats, gamma, idx, u)
        ctx.weight = weight
        ctx.bn_params = (gamma, beta)
        ctx.training = training
        return out

    @staticmethod
    def backward(ctx, dout):
        C = native()
        xsp, y, stats, gamma, idx, u = ctx.saved_tensors
        weight = ctx.weight
        gp, bp = ctx.bn_params
        ctx.bn_params = None
        dout = dout.contiguous()
        sunk = []
        dest = _bn_dest(gp, bp, False)  # with sinks: dgamma / dbeta straight into the flat buffer
        sinks = dest[1:] if dest is not None else ()
        # BN reduction sum g, sum g*(y - mean): g is nonzero only at window argmaxes, so with u = y at
        # each argmax (saved by the forward pool) it is a plain streaming reduction over the pooled
        # tensors (2 x 103 MB at batch 256) instead of a gather over y (411 MB)
        if u is not None:
            sums = C.bn_act_bwd_reduce(dout, u, u, stats, 2, *sinks)
        else:
            sums = C.pool_bn_bwd_reduce(dout, idx, y, stats, *sinks)
        dgamma = dbeta = None
        if dest is None:
            dgamma, dbeta = (sums[1] * stats[1]).to(gamma.dtype), sums[0].to(gamma.dtype)
        else:
            sunk += [gp, bp]
        dw = None
        shape = list(weight.shape)
        if ctx.needs_input_grad[1] and C.stem_bwd_fused_supported(shape[0], shape[2], (shape[3] + 2) // 2,
                                                                  y.shape[1], y.shape[2]):
            # the image takes no gradient, so dy's only consumer is the weight gradient: the BN/pool
            # backward apply runs inside it and the full-resolution dy is never stored
            dw = _wgrad_into(weight, sunk, C.stem_bwd_fused, dout, idx, y, stats, gamma, sums, ctx.training,
                             xsp, shape, deterministic())
        else:
            dy = C.pool_bn_bwd_apply(dout, idx, y, stats, gamma, sums, ctx.training)
            if ctx.needs_input_grad[1]:
                dw = _wgrad_into(weight, sunk, C.stem_wgrad, dy, xsp, shape, deterministic())
        if sunk:
            sunk[0]._pdt_flat.mark_ready(sunk)
        _end_mirror_trust(weight)
        ctx.weight = None
        return (None, dw, dgamma, dbeta, None, None, None, None, None, None, None)


def _stem_fast(x: torch.Tensor, conv: nn.Conv2d) -> bool:
    return (x.is_cuda and not x.requires_grad and x.dim() == 4 and x.shape[1] <= 4
            and conv.stride == (2, 2) and conv.kernel_size[0] == conv.kernel_size[1]
            and conv.bias is None)


def stem_conv_bn_pool(x: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d,
                      pool: nn.Module) -> torch.Tensor:
    """maxpool3x3s2(relu(BN(conv7x7/s2(image)))) -> NHWC bf16.  One fused BN/ReLU/pool pass on the
    device fast path; otherwise the unfused stem followed by the max pool."""
    std_pool = (isinstance(pool, nn.MaxPool2d) and pool.kernel_size in (3, (3, 3))
                and pool.stride in (2, (2, 2)) and pool.padding in (1, (1, 1))
                and pool.dilation in (1, (1, 1)) and not pool.ceil_mode)
    if _STEM_POOL and std_pool and _stem_fast(x, conv) and conv.out_channels <= 256:
        training, momentum, eps = _bn_prepare(bn)
        return _StemConvBNPool.apply(x.float(), conv.weight, bn.weight, bn.bias, bn.running_mean,
                                     bn.running_var, 2, conv.padding[0], training, momentum, eps)
    return maxpool3x3s2(stem_conv_bn(x, conv, bn))


def stem_conv_bn(x: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d) -> torch.Tensor:
    """z = relu(BN(conv7x7/s2(image))) -> NHWC bf16, device path for <= 4-channel fp32 images.
    Falls back to image_to_nhwc + conv_bn when the image itself needs a gradient."""
    if not _stem_fast(x, conv):
        return conv_bn(image_to_nhwc(x), conv, bn, relu=True)
    training, momentum, eps = _bn_prepare(bn)
    return _StemConvBN.apply(x.float(), conv.weight, bn.weight, bn.bias, bn.running_mean,
                             bn.running_var, 2, conv.padding[0], training, momentum, eps)


def conv_bn(x: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, relu: bool,
            residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """z = act(BN(conv(x)) [+ residual]) on NHWC activations."""
    stride = conv.stride[0]
    pad = conv.padding[0]
    training, momentum, eps = _bn_prepare(bn)
    return _ConvBN.apply(x, conv.weight, bn.weight, bn.bias, residual,
                         bn.running_mean, bn.running_var, stride, pad, relu,
                         training, momentum, eps)


# ----------------------------------------------------------------------------
# max pool 3x3/s2/p1
# ----------------------------------------------------------------------------
class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        if x.is_cuda:
            y, idx = native().maxpool_fwd(x)       # idx: argmax position 0..8 per output (uint8)
            _nan_trace("maxpool", x=x, y=y)
            ctx.save_for_backward(idx)
        else:
            y = ref.maxpool3x3s2_fwd(x)
            ctx.save_for_backward(x)
        ctx.hw = (x.shape[1], x.shape[2])
        return y

    @staticmethod
    def backward(ctx, dy):
        (saved,) = ctx.saved_tensors
        dy = dy.contiguous()
        if dy.is_cuda:
            return native().maxpool_bwd(dy, saved, ctx.hw[0], ctx.hw[1])
        return ref.maxpool3x3s2_bwd(dy, saved)


def maxpool3x3s2(x: torch.Tensor) -> torch.Tensor:
    return _MaxPool.apply(x)


# ----------------------------------------------------------------------------
# global avg pool + fc
# ----------------------------------------------------------------------------
class _AvgPoolLinear(torch.autograd.Function):
    """Global average pool + the classifier Linear (torchvision fc, resnet/main.py:76).

    Device path: avg-pool kernel, then the hand-written fc GEMMs of ``csrc/kernels/fc.hip`` (bf16
    MFMA, fp32 accumulation) -- forward with the bias folded into its split-K reduction; backward
    dW (accumulated straight into the flat gradient buffer under DDP), db, and the input gradient,
    whose split-K partials the avg-pool backward sums while broadcasting over H x W.  No library
    GEMM and no ATen kernel runs for the head."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        if x.is_cuda:
            C = native()
            pooled = C.avgpool_fwd(x)           # fp32 [N, C]
            logits = C.fc_forward(pooled, weight.float().contiguous(), bias.float().contiguous())
        else:
            pooled = ref.global_avgpool(x)
            logits = torch.addmm(bias.float(), pooled, weight.float().t())
        ctx.save_for_backward(pooled, weight)
        ctx.params = (weight, bias)
        ctx.hw = (x.shape[1], x.shape[2], x.dtype)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        pooled, weight = ctx.saved_tensors
        wp, bp = ctx.params
        ctx.params = None
        h, w, dt = ctx.hw
        dlogits = dlogits.float().contiguous()
        if dlogits.is_cuda:
            C = native()
            sw, sb = _grad_sink(wp), _grad_sink(bp)
            if sw is not None and sb is not None and sw.is_contiguous():
                dp, _, _ = C.fc_backward(dlogits, pooled, weight.float().contiguous(), sw, sb)
                wp._pdt_flat.mark_ready([wp, bp])
                dw = db = None
            else:
                dp, dw, db = C.fc_backward(dlogits, pooled, weight.float().contiguous())
                dw, db = dw.to(weight.dtype), db.to(weight.dtype)
            dx = C.avgpool_bwd(dp, h, w)
            return dx, dw, db
        dw = dlogits.t().mm(pooled)
        db = dlogits.sum(0)
        dpooled = dlogits.mm(weight.float())
        dx = (dpooled / (h * w))[:, None, None, :].expand(-1, h, w, -1).to(dt).contiguous()
        return dx, dw.to(weight.dtype), db.to(weight.dtype)


def avgpool_linear(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    return _AvgPoolLinear.apply(x, weight, bias)


# ----------------------------------------------------------------------------
# softmax cross entropy (mean) -- fused fwd+bwd
# ----------------------------------------------------------------------------
class _SoftmaxXent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, label_smoothing=0.0):
        if logits.is_cuda:
            if label_smoothing == 0.0:
                loss, dlogits = native().softmax_xent(logits.contiguous(), labels.contiguous())
            else:
                loss, dlogits = native().softmax_xent(logits.contiguous(), labels.contiguous(),
                                                      float(label_smoothing))
        else:
            loss, dlogits = ref.softmax_xent(logits, labels, label_smoothing)
        ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        (dlogits,) = ctx.saved_tensors
        if dlogits.is_cuda:  # scaled on the device by the (device) loss gradient: no host sync
            return native().scale_by(dlogits, dloss.float().reshape(1)), None, None
        return dlogits * dloss, None, None


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor, label_smoothing: float = 0.0) -> torch.Tensor:
    """Mean cross entropy; ``label_smoothing`` as in ``torch.nn.functional.cross_entropy``."""
    if not 0.0 <= label_smoothing <= 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1], got {label_smoothing}")
    return _SoftmaxXent.apply(logits, labels, label_smoothing)


class _SoftmaxXentMix(torch.autograd.Function):
    """``_SoftmaxXent`` against the two-label target of a mixed batch (``data/mix.py``)."""

    @staticmethod
    def forward(ctx, logits, labels_a, labels_b, lam, label_smoothing=0.0):
        if logits.is_cuda:
            loss, dlogits = native_mix().softmax_xent_mix(logits.contiguous(), labels_a.contiguous(),
                                                          labels_b.contiguous(), lam.float().contiguous(),
                                                          float(label_smoothing))
        else:
            loss, dlogits = ref.softmax_xent_mix(logits, labels_a, labels_b, lam, label_smoothing)
        ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        (dlogits,) = ctx.saved_tensors
        if dlogits.is_cuda:  # scaled on the device by the (device) loss gradient: no host sync
            return native().scale_by(dlogits, dloss.float().reshape(1)), None, None, None, None
        return dlogits * dloss, None, None, None, None


def mix_cross_entropy(logits: torch.Tensor, labels_a: torch.Tensor, labels_b: torch.Tensor, lam: torch.Tensor,
                      label_smoothing: float = 0.0) -> torch.Tensor:
    """Mean cross entropy against lam onehot(labels_a) + (1 - lam) onehot(labels_b), ``lam`` per
    row: ``F.cross_entropy`` with that soft target and ``label_smoothing``."""
    if not 0.0 <= label_smoothing <= 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1], got {label_smoothing}")
    return _SoftmaxXentMix.apply(logits, labels_a, labels_b, lam, label_smoothing)


class CrossEntropyLoss(nn.Module):
    """Drop-in for ``nn.CrossEntropyLoss()`` (mean reduction, ``resnet/main.py:102``); the target
    is a label tensor or the ``MixedTarget`` of a mixed batch."""

    def __init__(self, label_smoothing: float = 0.0):
        super().__init__()
        self.label_smoothing = float(label_smoothing)

    def forward(self, logits: torch.Tensor, labels) -> torch.Tensor:
        if isinstance(labels, MixedTarget):
            return mix_cross_entropy(logits, labels.labels_a, labels.labels_b, labels.lam, self.label_smoothing)
        return cross_entropy(logits, labels, self.label_smoothing)


def top1_correct(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """Number of rows whose argmax equals the label (``resnet/main.py:32-34``)."""
    if logits.is_cuda:
        return native().top1_correct(logits.contiguous(), labels.contiguous())
    return ref.top1_correct(logits, labels)


# ----------------------------------------------------------------------------
# whole residual block (device path): one autograd node per Bottleneck/BasicBlock
# ----------------------------------------------------------------------------
_NBT_BATCHED = 0  # > 0 inside bump_bn_counters(): the counters were already bumped in one launch

# BN buffers arriving from the DDP per-forward broadcast (torch DDP's _sync_buffers,
# torch/nn/parallel/distributed.py:1557): the broadcast runs on the comm stream and only the
# BatchNorm statistics kernels read/write those buffers, so the compute stream waits for it
# at the FIRST BN of the forward (after the stem convolution has been issued), not before the
# forward starts.  The counter bump writes the same (int64) flat buffer, so it is deferred too.
_BUFFER_WAIT = None   # callable: current stream waits for the buffer broadcast
_PENDING_BUMP = None  # num_batches_tracked tensors to bump once the buffers are ours


def defer_buffer_wait(fn) -> None:
    """Register the stream wait for an in-flight buffer broadcast (called by DDP)."""
    global _BUFFER_WAIT
    _BUFFER_WAIT = fn


def buffers_ready() -> None:
    """Make BN buffers safe to use on the current stream: run the deferred broadcast wait and
    the deferred counter bump (no-ops when nothing is pending)."""
    global _BUFFER_WAIT, _PENDING_BUMP
    if _BUFFER_WAIT is not None:
        fn, _BUFFER_WAIT = _BUFFER_WAIT, None
        fn()
    if _PENDING_BUMP is not None:
        counters, _PENDING_BUMP = _PENDING_BUMP, None
        with torch.no_grad():
            flat = _counter_flat(counters)
            if flat is not None:   # every counter is a view of one int64 buffer (DDP): one launch
                native().add_one_i64(flat)
            else:
                torch._foreach_add_(counters, 1)


def _counter_flat(counters):
    """The int64 buffer that exactly holds ``counters`` as consecutive one-element views (what
    ``parallel.flat.flatten_buffers`` builds when every int64 buffer is a BN counter), else None."""
    if not counters or not counters[0].is_cuda:
        return None
    base = counters[0]._base
    if base is None or base.dtype != torch.int64 or base.numel() != len(counters):
        return None
    p0 = base.data_ptr()
    for i, c in enumerate(counters):
        if c._base is not base or c.data_ptr() != p0 + 8 * i:
            return None
    return base


def forget_bn_modules(module: nn.Module) -> None:
    """Drop the BatchNorm list ``bump_bn_counters`` caches on ``module`` (collected at its first
    device forward).  Call after replacing or adding BatchNorm submodules; ``set_impl`` does."""
    module.__dict__.pop("_pdt_bn_list", None)
    module.__dict__.pop("_pdt_bn_counters", None)


class bump_bn_counters:
    """Context for one device forward of a whole model: bumps every training BatchNorm's
    ``num_batches_tracked`` (torch BN semantics) with ONE multi-tensor launch
    instead of one ``add_`` kernel per BN (53 launches per ResNet-50 step); the per-BN
    ``_bn_prepare`` calls inside the context then skip their own bump.  The launch itself is
    issued by the first BN of the forward (``buffers_ready``), behind any buffer broadcast."""

    def __init__(self, module: nn.Module):
        # the counter list is cached on the module: walking every submodule each forward cost
        # ~80 us of host issue per ResNet-18 step (scripts/host_profile.py).  Keyed by what
        # selects the counters (each BN's mode and buffer), so train()/eval() or a replaced
        # buffer rebuilds it.
        bns = getattr(module, "_pdt_bn_list", None)
        if bns is None:
            bns = [m for m in module.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]
            module._pdt_bn_list = bns
        key = tuple((m.training, m.track_running_stats, id(m.num_batches_tracked)) for m in bns)
        cached = getattr(module, "_pdt_bn_counters", None)
        if cached is None or cached[0] != key:
            cached = (key, [m.num_batches_tracked for m in bns if m.training and m.track_running_stats
                            and m.num_batches_tracked is not None])
            module._pdt_bn_counters = cached
        self.counters = cached[1]

    def __enter__(self):
        global _NBT_BATCHED, _PENDING_BUMP
        if self.counters:
            _PENDING_BUMP = self.counters
        _NBT_BATCHED += 1
        return self

    def __exit__(self, *exc):
        global _NBT_BATCHED
        _NBT_BATCHED -= 1
        buffers_ready()  # a forward without BatchNorm still owes the wait and the bump
        return False


def _bn_prepare(bn: nn.BatchNorm2d):
    """(training, momentum, eps) for one BN call; bumps num_batches_tracked like torch."""
    training = bn.training or not bn.track_running_stats
    momentum = bn.momentum
    if training and bn.track_running_stats and not _NBT_BATCHED:
        with torch.no_grad():
            bn.num_batches_tracked.add_(1)
        if momentum is None:
            momentum = 1.0 / float(bn.num_batches_tracked.item())
    return training, (momentum if momentum is not None else 0.0), bn.eps


def _mirror_of(w):
    sp = getattr(w, "_pdt_flat", None)
    return sp._mirror if sp is not None else None


def _packed_krsc(C, w, cx):
    """bf16 [K,R,S,Cx] forward weights: a view of the flat-space mirror when current, else a pack."""
    m = _mirror_of(w)
    v = m.krsc_view(w) if m is not None else None
    if v is not None and v.shape[3] == cx:
        return v
    return C.pack_weight(w, cx)


def _packed_crsk(w):
    """bf16 [C,R,S,K] dgrad weights from the mirror, or None (the binding packs)."""
    m = _mirror_of(w)
    return m.crsk_view(w) if m is not None else None


class _Unit:
    """One conv + BN unit of a residual block (chain unit or projection shortcut): its configuration,
    its tensors as the node got them, the Parameter objects p_* (whose flat-space sinks take the
    gradients), its index ``base`` into ``grads``, and in backward what the forward saved: (z, y,
    stats) -- z None when fp8-only, and for the shortcut -- and the e4m3 copy x8 of its conv input."""

    __slots__ = ("stride", "pad", "training", "momentum", "eps", "w", "gamma", "beta", "rm", "rv",
                 "p_w", "p_gamma", "p_beta", "z", "y", "stats", "x8", "base")


def _block_units(spec, params, saved=None, in8=None):
    """(chain units, shortcut unit or None) of one block.  The one place that knows the flat layouts:
    ``params`` (the node's ``*tensors``, and ``grads``) holds five tensors per unit, chain units
    first, then the shortcut; ``saved`` (backward: ctx.saved_tensors) holds x, (z, y, stats) per
    chain unit, (y, stats) of the shortcut, then the saved ``params``; ``in8`` the e4m3 conv inputs
    of the chain units (the shortcut reads the first one's)."""
    chain, ds_cfg, _ = spec
    nch = len(chain)
    tensors = params if saved is None else saved[len(saved) - len(params):]
    units = []
    for i, cfg in enumerate(chain if ds_cfg is None else (*chain, ds_cfg)):
        u = _Unit()
        u.base = b = 5 * i
        u.stride, u.pad, u.training, u.momentum, u.eps = cfg
        u.w, u.gamma, u.beta, u.rm, u.rv = tensors[b:b + 5]
        u.p_w, u.p_gamma, u.p_beta = params[b:b + 3]
        u.z = u.y = u.stats = u.x8 = None
        if saved is not None and i < nch:
            u.z, u.y, u.stats = saved[1 + 3 * i:4 + 3 * i]
        elif saved is not None:
            u.y, u.stats = saved[1 + 3 * nch:3 + 3 * nch]
        if in8:
            u.x8 = in8[i if i < nch else 0]
        units.append(u)
    return (units, None) if ds_cfg is None else (units[:nch], units[nch])


def _unit_fwd(C, x, u, relu, residual, x8=None, q8=None, want_mask=False, want_z=True, csum=None):
    """conv -> BN -> (+residual) -> (ReLU) of unit ``u`` -> (z, y, stats, z8, zmask).  x8 = (e4m3
    copy of x, its dequant factor): fp8 conv; q8 = _Q8State: also emit the e4m3 copy z8 of the output;
    want_mask (with relu): also the 1-bit ReLU mask zmask a later BN-fused dgrad reads instead of z.
    ``residual`` is an activation, or ``(y_short, stats_short)``: a projection shortcut's raw conv
    output and its BN statistics, normalised inside this unit's apply pass (never materialised).
    csum: fp32 [8, k] slots the apply adds the output's per-channel sums into (DgradFold colsum)."""
    y, stats = _unit_conv_stats(C, x, u, x8)
    k = u.w.shape[0]
    rsc = rsh = None
    if isinstance(residual, tuple):
        residual, rst = residual
        rsc, rsh = rst[2], rst[3]
    if q8 is not None and k % 16 == 0:
        assert rsc is None, "fp8 apply takes a materialised residual"
        slot = q8.next_slot()
        z, zq, zm = C.bn_act_fwd_q8(y, stats[2], stats[3], residual, relu, q8.buf, slot, want_mask, want_z)
        return z, y, stats, (zq, q8.deq(slot)), (zm if want_mask else None)
    if want_mask:
        z, zm = C.bn_act_fwd_mask(y, stats[2], stats[3], residual, rsc, rsh)
        return z, y, stats, None, zm
    z = C.bn_act_fwd(y, stats[2], stats[3], residual, relu, rsc, rsh, csum)
    return z, y, stats, None, None


def _fp8_conv_ok(r, s, cx):
    """fp8 forward conv for a GEMM K of r*s*cx >= _FP8_KMIN (K = 64 half-fills the 128-wide fp8
    K-step).  128 (layer2's 1x1 over 128 channels on fp8, so its input needs no bf16 copy) vs 256:
    fp8 b512 31.23 vs 31.39 ms, b256 17.04 vs 17.01 ms (r3p, one box).  64 (every layer-1 1x1 on
    fp8 too, after the narrow fp8 dgrad) vs 128: b256 16.88 vs 16.77 ms, b512 31.09 vs 30.83 ms
    (r3ap, one box)."""
    return r * s * cx >= _FP8_KMIN


def _fp8_dgrad_ok(k, stride):
    """fp8 input gradient for a dy of k channels: whole 128-byte K-steps per tap (k % 128), or
    (_FP8_DGRAD_NARROW) any k % 16 at stride 1 -- the 64-channel layer-1 convs, whose
    dy then needs no bf16 copy at all when the weight gradient is fp8 too."""
    return k % 128 == 0 or (_FP8_DGRAD_NARROW and stride == 1 and k % 16 == 0)


def _fp8_only_ok(w_next, k, tr):
    """May unit output z (k channels, training) skip its bf16 copy?  Only when every reader takes the
    e4m3 copy: the next conv's forward GEMM and its fp8 weight gradient (backward masks of interior
    units are recomputed from y, so z itself is never read there)."""
    if not (tr and _FP8_BWD and _FP8_WGRAD and _FP8_ONLY) or deterministic():
        return False
    kn, cn, rn, sn = w_next.shape
    return cn == k and k % 16 == 0 and kn % 64 == 0 and _fp8_conv_ok(rn, sn, k)


def _unit_conv_stats(C, x, u, x8=None):
    """conv -> BN statistics (finalize, running-stat update) of unit ``u``: (y, stats[4, K])."""
    w, gamma, beta, rm, rv = u.w, u.gamma, u.beta, u.rm, u.rv
    stride, pad, training, momentum, eps = u.stride, u.pad, u.training, u.momentum, u.eps
    k, _, r, s = w.shape
    n, h, wd, cx = (x if x is not None else x8[0]).shape  # x None: an fp8-only activation
    count = n * ((h + 2 * pad - r) // stride + 1) * ((wd + 2 * pad - s) // stride + 1)
    if x8 is not None and not _fp8_conv_ok(r, s, cx) and x is not None:
        x8 = None  # a GEMM K of 64 (1x1 over 64 channels) half-fills the 128-wide fp8 K-step: bf16 is faster
    if x8 is None and training and not _NAN_TRACE:
        # conv + BN finalize in one host call (the running-stat update waits for the buffers first)
        buffers_ready()
        return C.conv_fwd_bn(x, _packed_krsc(C, w, cx), stride, pad, count, rm, rv, gamma, beta,
                             float(momentum), float(eps), None if deterministic() else _facc(gamma, w.shape[0]))
    if x8 is not None:
        wq, wsc = _packed_krsc8(C, w, cx)
        if training and not _NAN_TRACE and not deterministic():
            # BN finalize inside the conv (conv_fwd_bn's fused path)
            buffers_ready()
            return C.conv_fwd_fp8(x8[0], wq, wsc, stride, pad, True, x8[1],
                                  (count, rm, rv, gamma, beta, float(momentum), float(eps), _facc(gamma, k)))
        y, part = C.conv_fwd_fp8(x8[0], wq, wsc, stride, pad, training, x8[1])
    else:
        wk = _packed_krsc(C, w, cx)
        y, part = C.conv_fwd(x, wk, stride, pad, training)
    if _NAN_TRACE:
        m = _mirror_of(w)
        _nan_trace(f"unit_fwd {tuple(x.shape)}->{tuple(y.shape)} mirror={m is not None and m.krsc_view(w) is wk}",
                   x=x, wk=wk, y=y, part=part)
    buffers_ready()
    if training:
        stats = C.bn_finalize(part, count, rm, rv, gamma, beta, float(momentum), float(eps))
    else:
        stats = C.bn_eval_params(rm, rv, gamma, beta, float(eps))
    return y, stats


class _BnHandoff:
    """What a block leaves on its output tensor so the NEXT block's backward can run this
    block's last BatchNorm backward (relu mask + reduction) inside its own input-gradient
    dgrad epilogue.  The consumer (next block) ``offer``s what that epilogue produced; the
    producer (this block) ``claim``s it, and gets it only if the gradient it receives IS the
    offered one (same storage: no other consumer added to it)."""

    __slots__ = ("y", "stats", "gamma", "beta", "zmask", "deposit", "ds")

    def __init__(self, y, stats, gamma, beta, zmask=None, ds=None):
        self.y, self.stats, self.gamma, self.beta, self.zmask = y, stats, gamma, beta, zmask
        # ds: (y, stats, gamma) of the block's projection-shortcut BN -- fed by the same output
        # gradient g, so the consumer's epilogue reduces it too (kernels.h BnBwdFuse::y2)
        self.ds = ds
        self.deposit = None

    def offer(self, g, sums, dest, acc2):
        """Consumer: the masked gradient g of this BN's output, its backward ``sums`` (already sent to
        ``dest``, the _bn_dest of gamma / beta) and the accumulator ``acc2`` of the shortcut BN's, if taken."""
        self.deposit = (g, sums, dest, acc2)

    def claim(self, dz):
        """Producer, with the output gradient ``dz`` it received: (sums, dest, shortcut sums) of the offer
        when dz is the offered g; else all None, after taking an offer back (another consumer contributed)."""
        if self.deposit is None:
            return None, None, None
        g, sums, dest, acc2 = self.deposit
        self.deposit = None
        if g.data_ptr() == dz.data_ptr() and g.shape == dz.shape:
            return sums, dest, acc2
        if acc2 is not None:
            acc2.zero_()
        acc, sg, sb = dest
        if acc is not None:  # discard the unused sums
            acc.zero_()
        else:  # undo the deposited BN-parameter gradients
            with torch.no_grad():
                sg.sub_(sums[1] * self.stats[1])
                sb.sub_(sums[0])
        return None, None, None


class _BlockBackward:
    """One backward pass of a residual block: its state and its steps.  ``grads``: what autograd gets
    back per forward tensor; ``sunk``: the parameters whose gradient went in place into the flat buffer
    instead (``mark_ready`` at the end); ``deferred``: unit -> (accumulator, dgamma sink, dbeta sink) of
    a BN whose sums sit in an atomic accumulator (its apply adds dgamma / dbeta, its wgrad re-zeroes)."""

    __slots__ = ("C", "det", "side", "grads", "sunk", "deferred", "fp8b", "needs_dx")

    def __init__(self, C, side, ngrads, fp8b, needs_dx):
        self.C, self.side, self.fp8b, self.needs_dx = C, side, fp8b, needs_dx
        self.det = deterministic()
        self.grads = [None] * ngrads
        self.sunk = []
        self.deferred = {}

    def bn_finish(self, u, dest, sums):
        """Unit u's BN backward ``sums`` [sum g, sum g*(y - mean)] are taken and went to ``dest`` (_bn_dest):
        dgamma / dbeta into ``grads`` for autograd, or the parameters into ``sunk`` and, when the sums sit
        in an accumulator, the unit into ``deferred`` (its apply adds dgamma / dbeta)."""
        if dest is None:
            self.grads[u.base + 1], self.grads[u.base + 2] = sums[1] * u.stats[1], sums[0]
            return
        self.sunk += [u.p_gamma, u.p_beta]
        if dest[0] is not None:
            self.deferred[u] = dest

    def bn_reduce(self, u, dz, z, mask):
        """BN backward reduction of unit u as a pass of its own -> sums."""
        dest = _bn_dest(u.p_gamma, u.p_beta, False)
        sums = self.C.bn_act_bwd_reduce(dz, z, u.y, u.stats, mask, *(dest[1:] if dest is not None else ()))
        self.bn_finish(u, dest, sums)
        return sums

    def apply(self, u, dz, z, sums, mask, want_dres, need_dgrad):
        """BN backward apply of unit u -> (dy, dres, d8); d8 = (e5m2 dy, its dequant factor)
        when the dgrad consuming dy runs on fp8 (_fp8_dgrad_ok for the conv's stride), or the
        weight gradient does (K % 64 == 0 and the conv input's e4m3 copy u.x8 exists)"""
        C = self.C
        dfr = self.deferred.get(u)
        pg = dfr[1:] if dfr is not None else (None, None)
        if self.fp8b and u.training:
            k, cin, x8 = dz.shape[3], u.w.shape[1], u.x8
            wgrad8 = x8 is not None and not self.det and k % 64 == 0 and cin % 16 == 0 and x8[0].shape[3] == cin
            dgrad8 = _fp8_dgrad_ok(k, u.stride)
            if (need_dgrad and dgrad8) or wgrad8:
                stq = _q8_state(u.p_gamma, dz.device, "_pdt_q8b")
                slot = stq.next_slot()
                # fp8-only dy: the dgrad (if any) and the weight gradient both read the e5m2 copy
                want_dy = not (_FP8_ONLY and wgrad8 and (not need_dgrad or dgrad8))
                dy, dres, q = C.bn_act_bwd_apply_q8(dz, z, u.y, u.stats, u.gamma, sums, mask, want_dres,
                                                    stq.buf, slot, want_dy, *pg)
                return dy, dres, (q, stq.deq(slot))
        dy, dres = C.bn_act_bwd_apply(dz, z, u.y, u.stats, u.gamma, sums, mask, u.training, want_dres, *pg)
        return dy, dres, None

    def wgrad(self, u, dy, xin, d8):
        """Weight gradient of unit u from dy (bf16) / d8 (e5m2) and its conv input xin / u.x8, and the
        re-zero of the unit's BN-sum accumulator behind it (its apply is queued)."""
        C, side, w, x8 = self.C, self.side, u.w, u.x8
        sink = _grad_sink(u.p_w)
        dfr = self.deferred.pop(u, None)
        zero = dfr[0] if dfr is not None else None
        k, c = w.shape[0], w.shape[1]
        if d8 is not None and x8 is not None and not self.det and c % 16 == 0 and k % 64 == 0 and x8[0].shape[3] == c:
            # e5m2 dy x e4m3 x on the MX-rate MFMA, both already produced for the fp8 GEMMs
            dw = C.conv_wgrad_fp8(side.cuda_stream if sink is not None and side is not None else 0, d8[0], x8[0],
                                  d8[1], x8[1], list(w.shape), u.stride, u.pad, sink, zero)
            if sink is not None:
                self.sunk.append(u.p_w)
            else:
                self.grads[u.base] = dw.to(w.dtype)
            return
        if dy is None or xin is None:
            raise RuntimeError("fp8-only operands reached the bf16 weight gradient")
        if sink is not None and side is not None:
            # into the flat buffer on the side stream, concurrent with the dgrad chain; all-reduce and optimizer
            # wait for that stream (streams.py).  One native call: stream hand-off, launch, record_stream, re-zero
            C.conv_wgrad_side(side.cuda_stream, dy, xin, list(w.shape), u.stride, u.pad, self.det, sink, zero)
            self.sunk.append(u.p_w)
            return
        self.grads[u.base] = _wgrad_into(u.p_w, self.sunk, C.conv_wgrad, dy, xin, list(w.shape), u.stride, u.pad,
                                         self.det)
        if zero is not None:
            zero.zero_()

    def dgrad(self, u, dy, d8, xshape, stride, pad, addend):
        """Input gradient of unit u's conv (``addend`` summed in its epilogue)."""
        C = self.C
        if d8 is not None and _fp8_dgrad_ok(d8[0].shape[3], stride):
            wt8, wsc = _packed_crsk8(C, u.w)
            return C.conv_dgrad_fp8(d8[0], wt8, wsc, d8[1], xshape, stride, pad, addend)
        return C.conv_dgrad(dy, u.w, xshape, stride, pad, addend, _packed_crsk(u.w))

    def dgrad_bn(self, u, dy, d8, xshape, addend, y, z, stats, mask, dest, bn2=None):
        """Input gradient of unit u's conv with, in its epilogue, the backward (ReLU mask ``mask`` from
        ``z``, reduction) of the BN (y, stats) that produced the conv's input -> (g, sums), the sums going
        to ``dest`` (_bn_dest).  bn2 = (y2, stats2, acc2): a second BN of the same gradient (bf16 only)."""
        C = self.C
        acc, sg, sb = dest if dest is not None else (None, None, None)
        if acc is not None:
            sg = sb = None  # the sums stay in acc: the BN's apply adds dgamma / dbeta into the sinks
        if d8 is not None and _fp8_dgrad_ok(d8[0].shape[3], u.stride):
            assert bn2 is None
            wt8, wsc = _packed_crsk8(C, u.w)
            return C.conv_dgrad_bn_fp8(d8[0], wt8, wsc, d8[1], xshape, u.stride, u.pad, addend, y, z, stats, mask,
                                       sg, sb, acc)
        return C.conv_dgrad_bn(dy, u.w, xshape, u.stride, u.pad, addend, y, z, stats, mask, sg, sb,
                               _packed_crsk(u.w), acc, *(bn2 if bn2 is not None else ()))

    def dgrad_handoff(self, u, dy, d8, x, addend, hi):
        """The block's input gradient (first unit u; ``addend`` = the shortcut's gradient).  With a
        hand-off ``hi`` whose BN has gradient sinks, the previous block's last BN backward runs in the
        epilogue (ReLU mask from its output z = x) and is offered to that block."""
        dest = _bn_dest(hi.gamma, hi.beta, _BN_ACC and not self.det) if hi is not None else None
        if dest is None:
            return self.dgrad(u, dy, d8, list(x.shape), u.stride, u.pad, addend)
        zsrc, zmode = (hi.zmask, 3) if hi.zmask is not None else (x, 1)
        bn2 = None
        ds = hi.ds  # the previous block's projection-shortcut BN, reduced in the same epilogue
        if (dest[0] is not None and ds is not None and zmode == 3 and addend is not None
                and (d8 is None or not _fp8_dgrad_ok(d8[0].shape[3], u.stride)) and _grad_sink(ds[2]) is not None):
            bn2 = (ds[0], ds[1], _bacc(ds[2], hi.stats.shape[1]))
        dz, sums = self.dgrad_bn(u, dy, d8, list(x.shape), addend, hi.y, zsrc, hi.stats, zmode, dest, bn2)
        hi.offer(dz, sums, dest, bn2[2] if bn2 is not None else None)
        return dz

    def fold(self, u, g, sums, xin, colsum):
        """BN backward of the last unit u folded into its input gradient (kernels.h DgradFold) -> the
        folded weights: the dgrad reads [g | x] against [w*k1 | W^T diag(a) W] + bias instead of the
        applied dy, and the weight gradient needs no dy either: dW = diag(k1) g^T x + diag(a) W x^T x +
        b sum(x), on the side stream (also the BN parameter gradients and the accumulator re-zero).
        ``colsum``: the forward's sum_m x ([S, C] atomic slots, or deterministic [C] sums) or None."""
        global FOLD_CALLS
        FOLD_CALLS += 1
        C, side, w, stats = self.C, self.side, u.w, u.stats
        wt = _packed_crsk(w)
        if wt is None:
            wt = C.pack_weight_t(w)
        k, c = w.shape[0], w.shape[1]
        count = u.y.numel() // k
        fold = C.bn_fold_weights(wt.view(c, k), stats, u.gamma, sums, count)
        streams.fork(side, g, stats, sums, wt, xin)
        with torch.cuda.stream(side):
            # T1 and Gram accumulate into persistent zeroed workspaces that bn_fold_wgrad
            # clears after reading (with the consumed BN-sum accumulator): no memset / fill
            t1, gram, done = _fold_ws(k, c, xin.device)
            C.conv_wgrad(g, xin, [k, c, 1, 1], 1, 0, self.det, t1)
            C.conv_wgrad(xin, xin, [c, c, 1, 1], 1, 0, self.det, gram)
            if colsum is None:
                colsum = C.bn_act_bwd_reduce(xin, xin, xin, _zero_stats(c, xin.device), 0)[0]
            dfr = self.deferred.pop(u, None)
            _, sg, sb = dfr if dfr is not None else (None, None, None)
            C.bn_fold_wgrad(t1, gram, colsum, wt.view(c, k), stats, u.gamma, sums, count, _grad_sink(u.p_w),
                            sg, sb, done, dfr is not None)
        self.sunk.append(u.p_w)
        return fold

    def dgrad_bn_fold(self, prev, g, xin, fold):
        """The folded input gradient with unit ``prev``'s BN backward in its epilogue -> (g, sums): into the
        atomic accumulator, or (deterministic) fixed-order partials + reduce straight into the sinks."""
        dest = _bn_dest(prev.p_gamma, prev.p_beta, not self.det)
        pre = self.C.conv_dgrad_bn_fold(g, xin, fold[0], fold[1], prev.y, None, prev.stats, 2,
                                        *(dest[:1] if dest[0] is not None else dest))
        self.bn_finish(prev, dest, pre[1])
        return pre

    def shortcut(self, s, g_short, x, sums_dep):
        """Projection shortcut s: BN backward (reduce + apply), weight gradient, and the input
        gradient that the first conv's dgrad epilogue adds (None when x needs none).  ``sums_dep``:
        the BN's backward sums when the next block's hand-off epilogue took them."""
        if sums_dep is not None:
            # the apply adds dgamma / dbeta and the weight gradient re-zeroes the accumulator (as for
            # every acc-mode BN)
            global DUAL_CALLS
            DUAL_CALLS += 1
            sums = sums_dep
            self.bn_finish(s, (sums, _grad_sink(s.p_gamma), _grad_sink(s.p_beta)), sums)
        else:
            sums = self.bn_reduce(s, g_short, g_short, 0)
        dy, _, d8 = self.apply(s, g_short, g_short, sums, 0, False, self.needs_dx)
        self.wgrad(s, dy, x, d8)
        if not self.needs_dx:
            return None
        if s.stride == 2 and s.pad == 0 and s.w.shape[2] == 1 and s.w.shape[3] == 1:
            # 1x1/s2 shortcut: its input gradient is zero at every odd (h, w), so it is
            # computed as a dense 1x1 dgrad on the stride-2 grid and the first conv's
            # dgrad epilogue adds it at even positions only (no full-resolution tensor,
            # no all-zero parity-class launches)
            n, h, w, c = x.shape
            return self.dgrad(s, dy, d8, [n, (h + 1) // 2, (w + 1) // 2, c], 1, 0, None)
        return self.dgrad(s, dy, d8, list(x.shape), s.stride, s.pad, None)


class _ResidualBlock(torch.autograd.Function):
    """z = relu(unit_n(...unit_1(x)) + shortcut(x)) with unit = conv -> BN -> (ReLU).

    One autograd node per block lets backward fuse across units: the shortcut
    gradient is summed into the block-input gradient inside the first conv's
    dgrad epilogue (no separate add kernel); each unit's BatchNorm backward
    (ReLU mask and the per-channel reduction) runs inside the epilogue of the dgrad
    that produces its input gradient (``conv_dgrad_bn``), including -- through a
    ``_BnHandoff`` -- the previous block's last unit; the remaining per-unit pass is
    one elementwise apply.
    tensors = per unit (w, gamma, beta, running_mean, running_var), chain units
    first, then the downsample unit if present (``_block_units``).
    """

    @staticmethod
    def forward(ctx, x, spec, handoff, fp8io, *tensors):
        C = native()
        if _NAN_TRACE:
            _nan_trace(f"block-in {tuple(x.shape)}", x=x)
        if _LEAD is not None:
            _lead_mark(f"fwd {tuple(x.shape)}")
        units, shortcut = _block_units(spec, tensors)
        nch = len(units)
        # fp8io = (x8, per-chain-unit _Q8State list, holder for the output's e4m3 copy) or None
        x8, q8s, holder = fp8io if fp8io is not None else (None, None, None)
        # shortcut first (it only needs x) so its output can be freed into the tail's add
        ds_join = None
        if shortcut is None:
            res = x
        elif q8s is not None:  # fp8: the tail's apply takes a materialised residual
            res, y_ds, st_ds, _, _ = _unit_fwd(C, x, shortcut, False, None, x8)
        else:
            # projection shortcut: conv + statistics only; its BN apply runs inside the block
            # tail's apply pass (bn_act_fwd RESBN), so the normalised shortcut is never stored
            br = streams.branch_stream(x.device) if x.is_cuda and nch > 1 else None
            if br is not None:
                # on the branch stream, concurrent with the chain's first units; the tail unit waits
                buffers_ready()  # a deferred BN-buffer wait lands on this stream, before the fork
                main = streams.fork(br, x)
                with torch.cuda.stream(br):
                    y_ds, st_ds = _unit_conv_stats(C, x, shortcut, x8)
                ds_join = (main, streams.join(br, main, y_ds, st_ds))
            else:
                y_ds, st_ds = _unit_conv_stats(C, x, shortcut, x8)
            res = (y_ds, st_ds)
        h, h8 = x, x8
        outs = []
        ins8 = [x8]  # e4m3 copy (q, dequant factor) of each chain unit's conv input, or None
        zmask = None
        # the last unit's folded weight gradient needs sum_m of its conv input: summed by the apply
        # that writes that input (no reduction pass in backward)
        fold_fwd = not spec[2] and fp8io is None and _fold_colsum_ok(units, x)
        det_fwd = deterministic()
        csum = _csum_slots(units[-1].w, x.device) if fold_fwd and not det_fwd else None
        ctx.colsum = csum
        for i, u in enumerate(units):
            last = i == nch - 1
            if last and ds_join is not None:
                ds_join[0].wait_event(ds_join[1])
            want_z = last or q8s is None or not _fp8_only_ok(units[i + 1].w, u.w.shape[0], u.training)
            # want_mask: the block output's ReLU mask as bits -- the next block's BN-fused dgrad
            # reads it instead of z (1/16 of the bytes)
            z, y, stt, h8, zm = _unit_fwd(C, h, u, True, res if last else None, h8, q8s[i] if q8s else None,
                                          want_mask=last and u.training, want_z=want_z,
                                          csum=csum if i == nch - 2 else None)
            if z is None and h8 is None:
                raise RuntimeError("fp8-only activation without its e4m3 copy")
            if fold_fwd and det_fwd and i == nch - 2:
                # deterministic runs (no atomics): the fixed-order column-sum reduction of the last
                # unit's conv input runs here, on the weight-gradient stream -- idle during the
                # forward -- instead of at the end of backward, where that stream is the tail
                side = streams.wgrad_stream(z.device)
                streams.fork(side, z)
                with torch.cuda.stream(side):
                    ctx.colsum = C.bn_act_bwd_reduce(z, z, z, _zero_stats(z.shape[3], z.device), 0)[0]
            if last:
                zmask = zm
            else:
                ins8.append(h8)
            outs += [z, y, stt]
            h = z
        if holder is not None and h8 is not None:
            holder.append(h8)
        if _CAPTURE is not None:
            _CAPTURE.append(outs[0::3])
        if _NAN_TRACE:
            for ui in range(nch):
                _nan_trace(f"fwd block{id(ctx) % 10007} unit{ui}", z=outs[3 * ui], y=outs[3 * ui + 1],
                           stats=outs[3 * ui + 2])
        if shortcut is not None:
            outs += [y_ds, st_ds]
        ctx.save_for_backward(x, *outs, *tensors)  # the layout _block_units reads back
        ctx.params = tensors  # the Parameter objects: gradients may be written into flat views
        ctx.spec = spec
        ctx.handoff_in = handoff  # the producer of x (previous block), or None
        ctx.fp8b = fp8io is not None and _FP8_BWD  # fp8 dgrads in backward (dy in e5m2)
        ctx.in8 = ins8 if ctx.fp8b and _FP8_WGRAD else None  # fp8 weight-gradient operands
        ctx.handoff_out = _BnHandoff(y, stt, u.gamma, u.beta, zmask,  # y, stt, u: the last unit's
                                     (y_ds, st_ds, shortcut.gamma) if shortcut is not None and _DUAL_BN else None)
        return h

    @staticmethod
    def backward(ctx, dz):
        C = native()
        if _LEAD is not None:
            _lead_mark(f"bwd {tuple(dz.shape)}")
        sv = ctx.saved_tensors
        x = sv[0]
        units, shortcut = _block_units(ctx.spec, ctx.params, sv, ctx.in8)
        ctx.in8 = None
        nch = len(units)
        if _NAN_TRACE:
            for ui, u in enumerate(units):
                _nan_trace(f"bwd-entry block{id(ctx) % 10007} unit{ui} {tuple(u.y.shape)}", z=u.z, y=u.y, stats=u.stats)
            _nan_trace(f"bwd-entry block{id(ctx) % 10007} dz", dz=dz)
        dz = dz.contiguous()
        bw = _BlockBackward(C, streams.begin(x.device), len(ctx.params), ctx.fp8b, ctx.needs_input_grad[0])
        ds_br = streams.branch_stream(x.device) if shortcut is not None and x.is_cuda else None
        ds_join = None

        # does the gradient arrive masked and reduced from the next block's dgrad epilogue?  sums_ds: the
        # shortcut BN's (sum g, sum g*(y_ds - mean)) from the same epilogue
        sums, dest, sums_ds = ctx.handoff_out.claim(dz)
        ctx.handoff_out = None
        pre = None  # (g = dz * relu'(unit), the unit's BN backward sums of g)
        if sums is not None:
            pre = (dz, sums)
            bw.bn_finish(units[-1], dest, sums)

        for i in reversed(range(nch)):
            u = units[i]
            last = i == nch - 1
            xin = x if i == 0 else units[i - 1].z  # None: fp8-only (its e4m3 copy is u.x8)
            need_dx = i > 0 or bw.needs_dx
            fold = None
            if pre is None:
                # reduce, then apply.  Only the last unit of a block nothing was handed to gets here:
                # every other unit's sums come from the epilogue of the dgrad behind it
                assert last
                sums = bw.bn_reduce(u, dz, u.z, 1)
                dy, g_short, d8 = bw.apply(u, dz, u.z, sums, 1, True, need_dx)
            else:
                g, sums = pre  # reduced in the producing epilogue
                if last:
                    g_short = g
                if last and i > 0 and _fold_ok(u, units[i - 1], xin, bw):
                    # the apply -- feeding only the weight gradient -- goes with it to the side stream
                    colsum, ctx.colsum = ctx.colsum, None  # consumed: bn_fold_wgrad re-zeroes the [S, C] slots
                    fold = bw.fold(u, g, sums, xin, colsum)
                else:
                    dy, _, d8 = bw.apply(u, g, g, sums, 0, False, need_dx)
            if fold is None:
                bw.wgrad(u, dy, xin, d8)
            if last and shortcut is not None and nch > 1 and ds_br is not None:
                # projection-shortcut backward on the branch stream, concurrent with the
                # chain's remaining units; the first conv's dgrad waits for its addend
                main = streams.fork(ds_br, g_short, shortcut.y, shortcut.stats, x)
                with torch.cuda.stream(ds_br):
                    addend = bw.shortcut(shortcut, g_short, x, sums_ds)
                ds_join = (main, streams.join(ds_br, main, addend))
            if i > 0:
                prev = units[i - 1]
                if fold is not None:
                    pre = bw.dgrad_bn_fold(prev, g, xin, fold)
                else:
                    dest = _bn_dest(prev.p_gamma, prev.p_beta, _BN_ACC and not bw.det)
                    pre = bw.dgrad_bn(u, dy, d8, list((xin if xin is not None else prev.y).shape), None,
                                      prev.y, None, prev.stats, 2, dest)
                    bw.bn_finish(prev, dest, pre[1])
            else:
                # shortcut gradient: identity -> g_short itself; projection -> its dgrad
                if ds_join is not None:
                    ds_join[0].wait_event(ds_join[1])
                elif shortcut is not None:
                    addend = bw.shortcut(shortcut, g_short, x, sums_ds)
                else:
                    addend = g_short
                dz = bw.dgrad_handoff(u, dy, d8, x, addend, ctx.handoff_in) if bw.needs_dx else None
        ctx.handoff_in = None
        for acc, _, _ in bw.deferred.values():  # (every unit's weight gradient re-zeroes its own)
            acc.zero_()
        if ctx.colsum is not None:  # summed in forward but not folded (no hand-off into this block)
            if ctx.colsum.dim() == 2:  # the atomic slots must be left zeroed
                ctx.colsum.zero_()
            ctx.colsum = None
        if bw.sunk:
            bw.sunk[0]._pdt_flat.mark_ready(bw.sunk)
        return (dz, None, None, None, *bw.grads)


def _fold_shape_ok(u) -> bool:
    """Is unit u's conv one the DgradFold kernels take: training, 1x1 / stride 1, K a multiple of 256
    up to 2048, C a multiple of 64?"""
    k, c, r, s = u.w.shape
    return (u.training and r == 1 and s == 1 and u.stride == 1 and u.pad == 0 and k % 256 == 0 and k <= 2048
            and c % 64 == 0)


def _fold_ok(u, prev, xin, bw) -> bool:
    """May the last unit u of a bottleneck fold its BN backward into its 1x1 input gradient
    (kernels.h DgradFold)?  bf16, training, a weight-gradient side stream, a 1x1 / stride-1 conv over
    a materialised input, and gradient sinks for the BN of the unit before (its sums go to an atomic
    accumulator, or in deterministic runs to fixed-order partials with dgamma / dbeta written by the
    reduce; the fold's weight-gradient GEMMs then take the slab split-K)."""
    if not (_FOLD_BN and _BN_ACC and bw.side is not None and not bw.fp8b and xin is not None
            and _fold_shape_ok(u) and xin.shape[3] == u.w.shape[1]):
        return False
    return (_grad_sink(prev.p_gamma) is not None and _grad_sink(prev.p_beta) is not None
            and _grad_sink(u.p_w) is not None)


def _fold_colsum_ok(units, x) -> bool:
    """Will the last unit's folded weight gradient (DgradFold) want sum_m of its conv input?  The
    static half of _fold_ok: a training bottleneck whose last conv is a foldable 1x1, bf16, with a
    weight-gradient side stream and a flat-space gradient sink."""
    if len(units) < 2 or not x.is_cuda or _FP8 or not (_FOLD_BN and _BN_ACC):
        return False
    u = units[-1]
    if not _fold_shape_ok(u) or 256 % (u.w.shape[1] // 8):
        return False
    return streams.wgrad_stream(x.device) is not None and _grad_sink(u.w) is not None


def _csum_slots(w, dev):
    """The zeroed [S, C] fp32 column-sum slots (S = C.bn_csum_slots()) the apply of the unit before
    the last atomically fills (bn_fold_wgrad re-zeroes them after use), one set per folded conv."""
    c = w.shape[1]
    cs = getattr(w, "_pdt_csum", None)
    if cs is None or cs.shape[1] != c or cs.device != dev:
        cs = torch.zeros(native().bn_csum_slots(), c, dtype=torch.float32, device=dev)
        w._pdt_csum = cs
    return cs


_ZSTATS = {}
_FOLD_WS = {}


def _fold_ws(k, c, dev):
    """Persistent (T1 [k, c, 1, 1], Gram [c, c, 1, 1], completion counter) fp32 workspaces of the
    folded weight gradient, zeroed once; every consumer (bn_fold_wgrad in consume mode) leaves them
    zeroed again.  Units of one shape reuse them in order on the weight-gradient stream."""
    ws = _FOLD_WS.get((k, c, dev))
    if ws is None:
        ws = _FOLD_WS[(k, c, dev)] = (torch.zeros(k, c, 1, 1, device=dev), torch.zeros(c, c, 1, 1, device=dev),
                                      torch.zeros(c // 64 + 1, dtype=torch.int32, device=dev))
    return ws


def _zero_stats(c, dev):
    """Zero [4, c] BN statistics (a column sum through bn_act_bwd_reduce), cached per device."""
    z = _ZSTATS.get((c, dev))
    if z is None:
        z = _ZSTATS[(c, dev)] = torch.zeros(4, c, device=dev)
    return z


def _unit_tensors(conv: nn.Conv2d, bn: nn.BatchNorm2d) -> list:
    """(weight, gamma, beta, running_mean, running_var) of one conv+BN unit, read from the module
    dicts directly: nn.Module.__getattr__'s fallback path for parameters and buffers was ~40 us of
    host issue per ResNet-18 step (scripts/host_profile.py)."""
    bp, bb = bn._parameters, bn._buffers
    return [conv._parameters["weight"], bp["weight"], bp["bias"], bb["running_mean"], bb["running_var"]]


def residual_block(x: torch.Tensor, chain, downsample=None, tail: bool = False) -> torch.Tensor:
    """Device path of a ResNet block: ``chain`` = [(conv, bn), ...] (ReLU after each BN, the
    shortcut added before the last ReLU), ``downsample`` = (conv, bn) or None.  ``tail``: the
    network's last block (no next block hands its last BN backward into this one, so its
    folded weight gradient cannot run and the forward takes no column sums for it)."""
    spec_chain, tensors = [], []
    for conv, bn in chain:
        tr, mo, ep = _bn_prepare(bn)
        spec_chain.append((conv.stride[0], conv.padding[0], tr, mo, ep))
        tensors += _unit_tensors(conv, bn)
    ds_spec = None
    if downsample is not None:
        conv, bn = downsample
        tr, mo, ep = _bn_prepare(bn)
        ds_spec = (conv.stride[0], conv.padding[0], tr, mo, ep)
        tensors += _unit_tensors(conv, bn)
    fp8io = None
    if _FP8:
        q8s = [_q8_state(bn, x.device) for _, bn in chain]
        fp8io = (getattr(x, "_pdt_fp8", None), q8s, [])
    out = _ResidualBlock.apply(x, (tuple(spec_chain), ds_spec, tail), getattr(x, "_pdt_handoff", None),
                               fp8io, *tensors)
    node = out.grad_fn  # the ctx of this block's node (None without autograd)
    if node is not None and getattr(node, "handoff_out", None) is not None:
        out._pdt_handoff = node.handoff_out
    if fp8io is not None and fp8io[2]:
        out._pdt_fp8 = fp8io[2][0]
    return out
