"""Global gradient-norm clipping -- ``torch.nn.utils.clip_grad_norm_`` semantics, on the device.

On the flat gradient buffer of a GPU ``FlatParamSpace`` the clip is three launches and no host read
(``csrc/opt/clip.hip``): float64 sums of squares over fixed 4096-element chunks, a one-block finalize
that writes the clip record ``(norm, coef)`` with ``coef = min(max_norm / (norm + 1e-6), 1)``, and an
in-place scale that returns at once when ``coef`` is exactly 1.  Everything stays on the stream, so
the clip runs inside a captured step, and the record depends on the gradient's length and values
alone: every rank of a data-parallel job scales its copy of the all-reduced gradient by the same bits.

``optim.LAMB(max_grad_norm=...)`` does not come through here: its first pass reads the record and
multiplies as it loads, which saves the scale pass (``optim/lamb.py``).  This entry point is for the
optimizers that cannot read the record (``optim.SGD``, ``optim.LARS``); construct them with
``overlap=False``, since an update inside backward cannot know the global norm.
"""
from __future__ import annotations

import math
import weakref

import torch

from ..ops._ext import native_opt
from ..parallel.flat import FlatParamSpace

CHUNK = 4096  # elements per float64 partial (csrc/opt/clip.h: kClipChunk)

_BUFS: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()  # flat space -> (gpart, clip)


def clip_buffers(n: int, device):
    """``(gpart, clip)``: the float64 partials of an ``n``-element gradient and the fp32 record."""
    return (torch.zeros((n + CHUNK - 1) // CHUNK, dtype=torch.float64, device=device),
            torch.ones(2, dtype=torch.float32, device=device))


def check_max_norm(max_norm: float) -> float:
    max_norm = float(max_norm)
    if not (math.isfinite(max_norm) and max_norm > 0.0):
        raise ValueError(f"max_norm must be finite and > 0, got {max_norm}")
    return max_norm


@torch.no_grad()
def clip_grad_norm_(space_or_params, max_norm: float) -> torch.Tensor:
    """Scale the gradients so that their global L2 norm is at most ``max_norm``.

    A GPU ``FlatParamSpace``: returns the device record ``[norm, coef]`` (fp32), never read here.
    Anything else (a CPU space, an iterable of parameters): ``torch.nn.utils.clip_grad_norm_``, whose
    total norm is returned."""
    max_norm = check_max_norm(max_norm)
    sp = space_or_params
    if not isinstance(sp, FlatParamSpace):
        return torch.nn.utils.clip_grad_norm_(sp, max_norm)
    if not sp.param_flat.is_cuda:
        return torch.nn.utils.clip_grad_norm_(sp.params, max_norm)
    if not sp.grads_attached():
        sp.gather_grads()
    bufs = _BUFS.get(sp)
    if bufs is None:
        bufs = _BUFS[sp] = clip_buffers(sp.numel, sp.grad_flat.device)
    gpart, clip = bufs
    O = native_opt()
    O.grad_norm(sp.grad_flat, gpart, clip, max_norm)
    O.scale_grads(sp.grad_flat, clip)
    return clip
