"""Argument checks the binding sources share (csrc/bind_util.h): one test per helper, over every op
that goes through it.  Each call must be rejected before its op launches anything, so the inputs are
the smallest the earlier checks accept and every case takes milliseconds."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
WD, ETA, EPS = 1e-4, 1.0, 1e-8
NSEG, SEG = 8, 16  # the flat optimizer space: 8 segments of 16 elements


@pytest.fixture(scope="module")
def t(gpu, native_ext):
    """Operands (never written: every call is rejected).  Convs: x [1,4,4,8] -> 3x3/s1/p1 -> 16
    channels; the fp8 weight gradient: x8 [1,4,4,16] -> 64 channels."""
    from pytorch_distributed_tutorials_amd.optim.lars import LarsTable

    def z(*shape, dtype=BF16):
        return torch.zeros(*shape, dtype=dtype, device=gpu)

    n = NSEG * SEG
    tb = LarsTable([(i * SEG, SEG, False) for i in range(NSEG)], gpu)
    return SimpleNamespace(
        z=z, n=n, x=z(1, 4, 4, 8), dy=z(1, 4, 4, 16), xs=[1, 4, 4, 8], ws=[16, 8, 3, 3],
        w=z(16, 8, 3, 3, dtype=F32), wt=z(8, 3, 3, 16), stats=z(4, 8, dtype=F32), vec=z(8, dtype=F32),
        sums=z(2, 8, dtype=F32), state=z(native_ext.fp8_state_floats(), dtype=F32),
        dy8=z(1, 4, 4, 16, dtype=U8), wt8=z(8, 3, 3, 16, dtype=U8), one=torch.ones(1, device=gpu),
        x8=z(1, 4, 4, 16, dtype=U8), dy8w=z(1, 4, 4, 64, dtype=U8), ws8=[64, 16, 3, 3],
        p=z(n, dtype=F32), g=z(n, dtype=F32), lars=(tb.table, tb.partials, tb.trust, 0, NSEG))


def _rejects(calls, op, C, t, match):
    with pytest.raises(RuntimeError, match=match):
        calls[op](C, t)
    torch.cuda.synchronize()


SINKS = {  # dgamma (t.vec, or [16] for the fold) without dbeta
    "bn_act_bwd_reduce": lambda C, t: C.bn_act_bwd_reduce(t.x, t.x, t.x, t.stats, 0, t.vec, None),
    "bn_act_bwd_apply": lambda C, t: C.bn_act_bwd_apply(t.x, t.x, t.x, t.stats, t.vec, t.sums, 0, True, False,
                                                        t.vec, None),
    "bn_act_bwd_apply_q8": lambda C, t: C.bn_act_bwd_apply_q8(t.x, t.x, t.x, t.stats, t.vec, t.sums, 0, False,
                                                              t.state, 0, True, t.vec, None),
    "pool_bn_bwd_reduce": lambda C, t: C.pool_bn_bwd_reduce(t.z(1, 2, 2, 8), t.z(1, 2, 2, 8, dtype=U8), t.x,
                                                            t.stats, t.vec, None),
    "conv_dgrad_bn": lambda C, t: C.conv_dgrad_bn(t.dy, t.w, t.xs, 1, 1, None, t.x, None, t.stats, 0, t.vec, None,
                                                  wt=t.wt),
    "bn_fold_wgrad": lambda C, t: C.bn_fold_wgrad(
        t.z(16, 8, dtype=F32), t.z(8, 8, dtype=F32), t.vec, t.z(8, 16), t.z(4, 16, dtype=F32), t.z(16, dtype=F32),
        t.z(2, 16, dtype=F32), 16, t.z(16, 8, 1, 1, dtype=F32), t.z(16, dtype=F32), None),
}


@pytest.mark.parametrize("op", sorted(SINKS))
def test_dgamma_needs_dbeta(gpu, native_ext, t, op):
    _rejects(SINKS, op, native_ext, t, "dgamma and dbeta go together")


ADDEND = {  # [1,3,3,8]: neither dx [1,4,4,8] nor its compact map [1,2,2,8]
    "conv_dgrad": lambda C, t: C.conv_dgrad(t.dy, t.w, t.xs, 1, 1, t.z(1, 3, 3, 8), t.wt),
    "conv_dgrad_bn": lambda C, t: C.conv_dgrad_bn(t.dy, t.w, t.xs, 1, 1, t.z(1, 3, 3, 8), t.x, None, t.stats, 0,
                                                  wt=t.wt),
    "conv_dgrad_fp8": lambda C, t: C.conv_dgrad_fp8(t.dy8, t.wt8, t.vec, t.one, t.xs, 1, 1, t.z(1, 3, 3, 8)),
}


@pytest.mark.parametrize("op", sorted(ADDEND))
def test_addend_shape(gpu, native_ext, t, op):
    _rejects(ADDEND, op, native_ext, t, "dgrad addend must have the shape of dx")


RESIDUAL = {  # 16 channels against y's 8
    "bn_act_fwd": lambda C, t: C.bn_act_fwd(t.x, t.vec, t.vec, t.dy, True),
    "bn_act_fwd_mask": lambda C, t: C.bn_act_fwd_mask(t.x, t.vec, t.vec, t.dy),
    "bn_act_fwd_q8": lambda C, t: C.bn_act_fwd_q8(t.x, t.vec, t.vec, t.dy, True, t.state, 0),
}


@pytest.mark.parametrize("op", sorted(RESIDUAL))
def test_residual_shape(gpu, native_ext, t, op):
    _rejects(RESIDUAL, op, native_ext, t, "residual shape mismatch")


WGRAD_OUT = {  # fp32 [K,C,3,3] of plain contiguous (KCRS) strides
    "conv_wgrad": lambda C, t: C.conv_wgrad(t.dy, t.x, t.ws, 1, 1, False, t.z(*t.ws, dtype=F32)),
    "conv_wgrad_side": lambda C, t: C.conv_wgrad_side(torch.cuda.Stream().cuda_stream, t.dy, t.x, t.ws, 1, 1, False,
                                                      t.z(*t.ws, dtype=F32)),
    "conv_wgrad_fp8": lambda C, t: C.conv_wgrad_fp8(0, t.dy8w, t.x8, t.one, t.one, t.ws8, 1, 1,
                                                    t.z(*t.ws8, dtype=F32)),
}


@pytest.mark.parametrize("op", sorted(WGRAD_OUT))
def test_wgrad_out_must_be_krsc_dense(gpu, native_ext, t, op):
    _rejects(WGRAD_OUT, op, native_ext, t, r"channels_last \(KRSC\) dense")


def _flat_ops(p, g, buf, momentum, mirror):
    return {
        "sgd_step": lambda C, t: C.sgd_step(p(t), g(t), buf, 0.1, momentum, 0.0, WD, False, True, 1.0, mirror(t)),
        "lars_step": lambda C, t: C.lars_step(p(t), g(t), buf, *t.lars, 0.1, momentum, 0.0, WD, False, True, ETA,
                                              EPS, mirror(t)),
        "lars_update": lambda C, t: C.lars_update(p(t), g(t), buf, *t.lars, 0.1, momentum, 0.0, WD, False, True,
                                                  mirror(t)),
    }


NO_BUFFER = _flat_ops(lambda t: t.p, lambda t: t.g, None, 0.9, lambda t: None)
SHORT_MIRROR = _flat_ops(lambda t: t.p, lambda t: t.g, None, 0.0, lambda t: t.z(t.n - 8))
# a parameter view one element into its buffer: 4 bytes off the 16-byte vectors of the kernels
OFFSET_PARAM = _flat_ops(lambda t: t.z(t.n + 4, dtype=F32)[1:t.n + 1], lambda t: t.g, None, 0.0, lambda t: None)


@pytest.mark.parametrize("op", sorted(NO_BUFFER))
def test_momentum_needs_buffer(gpu, native_ext, t, op):
    _rejects(NO_BUFFER, op, native_ext, t, "momentum != 0 needs a momentum buffer")


@pytest.mark.parametrize("op", sorted(SHORT_MIRROR))
def test_mirror_length(gpu, native_ext, t, op):
    _rejects(SHORT_MIRROR, op, native_ext, t, "bf16 mirror must match the parameter buffer")


# lars_update takes its buffers through the same flat_opt_args; it is left out so that a build
# whose lars_update lacks the check cannot launch the kernel on a misaligned buffer from here
@pytest.mark.parametrize("op", ["lars_step", "sgd_step"])
def test_param_alignment(gpu, native_ext, t, op):
    _rejects(OFFSET_PARAM, op, native_ext, t, "16-byte aligned")


HOST_SCALAR = {  # torch.ones(1) on the host where the kernel reads the scalar from device memory
    "scale_by": lambda C, t: C.scale_by(t.vec, torch.ones(1)),
    "pack_weight_fp8": lambda C, t: C.pack_weight_fp8(t.w, 0, act_deq=torch.ones(1)),
    "conv_fwd_fp8": lambda C, t: C.conv_fwd_fp8(t.x8, t.z(16, 3, 3, 16, dtype=U8), t.z(16, dtype=F32), 1, 1, False,
                                                ascale=torch.ones(1)),
}


@pytest.mark.parametrize("op", sorted(HOST_SCALAR))
def test_device_scalar(gpu, native_ext, t, op):
    _rejects(HOST_SCALAR, op, native_ext, t, "must be a device fp32 scalar")
