"""LAMB (You et al. 2020) and AdamW -- fused over the flat parameter space.

``ops/reference.py::lamb_`` is the exact semantics and the CPU path: Adam's bias-corrected direction
plus decoupled weight decay, ``u = m_hat / (sqrt(v_hat) + eps) + wd * p``, scaled per parameter tensor
by the trust ratio ``|p| / |u|``.  BatchNorm weights and biases and the fc bias (``exclude_1d``: every
tensor with ``ndim <= 1``, exactly as ``LARS``) get neither weight decay nor the ratio.
``trust=False`` is AdamW.

``max_grad_norm > 0`` clips the gradient by its global L2 norm before the moments, with
``torch.nn.utils.clip_grad_norm_``'s coefficient ``min(max_grad_norm / (norm + 1e-6), 1)`` (timm's
``Lamb(max_grad_norm=1.0)`` is the optimizer of the "ResNet strikes back" recipe); ``trust_clip`` clamps
the ratio at 1.  On the flat path the norm is two launches over the flat gradient buffer
(``csrc/opt/clip.hip``: float64 sums over fixed 4096-element chunks, a one-block finalize) that leave
``(norm, coef)`` in a device record; the first LAMB / AdamW pass reads the record and multiplies each
gradient element as it loads it, so a clipped step pays one extra 4 B per parameter read and no scale
pass, and the host never sees the norm.  ``grad_flat`` itself is left unscaled on this path: nothing
reads it after the step.  The norm is taken over the flat space (the per-tensor path: over every
gradient of the optimizer).  Neither setting is part of ``state_dict()``: a resumed run passes them again.

When a param group is exactly the set of parameters of a ``FlatParamSpace`` on the GPU, the step is
three streaming launches over the flat param / grad / moment buffers (``csrc/opt/lamb.hip``; one
launch plus a one-thread one for AdamW) that also write the bf16 KRSC weight mirror.  ``state[p]``
keeps ``torch.optim.Adam``'s format: ``exp_avg`` and ``exp_avg_sq`` are views into two flat buffers,
``step`` is the update count, so a checkpoint of the per-tensor path loads into the fused path and
back.  The update number lives in a device record the kernels read and advance -- never a host
argument -- so a captured step (``utils.graph.CapturedStep``) keeps a live bias correction;
``state_dict()`` reads it back once, at save time.  The norms are float64 sums in a fixed order that
depends on the parameter layout alone: every rank of a data-parallel job computes bitwise-identical
ratios from its copy of the all-reduced gradients.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

from ..ops import reference as ref
from ..ops._ext import native_opt
from .clip import clip_buffers
from .lars import LarsTable
from .sgd import SGD


class LAMB(torch.optim.Optimizer):
    """``trust=True``: LAMB; ``trust=False``: AdamW.  ``exclude_1d``: tensors with ``ndim <= 1`` get
    neither weight decay nor the trust ratio.

    No per-bucket update inside backward: the reducer's per-bucket hook knows SGD and LARS only, so
    ``LAMB`` always takes the post-backward ``step()`` and never attaches to the DDP wrapper.
    """

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6,
                 weight_decay: float = 0.0, trust: bool = True, exclude_1d: bool = True,
                 max_grad_norm: float = 0.0, trust_clip: bool = False):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"Invalid betas: {betas}")
        if eps < 0.0:
            raise ValueError(f"Invalid eps: {eps}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay: {weight_decay}")
        if not (math.isfinite(max_grad_norm) and max_grad_norm >= 0.0):
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        # kept off the param groups: state_dict() stays torch.optim.Adam's
        self.max_grad_norm, self.trust_clip = float(max_grad_norm), bool(trust_clip)
        defaults = dict(lr=lr, betas=(float(betas[0]), float(betas[1])), eps=eps, weight_decay=weight_decay,
                        trust=bool(trust), exclude_1d=bool(exclude_1d))
        super().__init__(params, defaults)
        self._flat = {}  # flat space id -> its table, moment buffers and device record
        # build the device state now (not inside a captured first step)
        for group in self.param_groups:
            sp = self._flat_space_of(group)
            if sp is not None and sp.param_flat.is_cuda:
                self._flat_state(sp, group["exclude_1d"])

    # the flat-space detection and zero_grad of optim.SGD
    _flat_space_of = SGD._flat_space_of
    zero_grad = SGD.zero_grad

    def _flat_state(self, sp, exclude_1d: bool):
        fs = self._flat.get(id(sp))
        if fs is None or fs.exclude_1d != bool(exclude_1d):
            old = fs
            fs = SimpleNamespace(
                exclude_1d=bool(exclude_1d),
                table=LarsTable([(o, p.numel(), bool(exclude_1d and p.ndim <= 1))
                                 for p, o in zip(sp.params, sp.offsets)], sp.param_flat.device),
                m=old.m if old else torch.zeros_like(sp.param_flat),
                v=old.v if old else torch.zeros_like(sp.param_flat),
                # the device record: [0] = finished updates, [1] = the bias corrections in flight
                rec=old.rec if old else torch.zeros(int(native_opt().record_elems()), dtype=torch.int64,
                                                    device=sp.param_flat.device),
                # the clipping's float64 partials and its device record (norm, coef)
                gpart=old.gpart if old else None, clip=old.clip if old else None)
            if fs.clip is None and self.max_grad_norm > 0.0:
                fs.gpart, fs.clip = clip_buffers(sp.numel, sp.param_flat.device)
            self._flat[id(sp)] = fs
            for p, o in zip(sp.params, sp.offsets):
                st = self.state[p]
                st.setdefault("step", torch.tensor(0.0))
                st["exp_avg"] = torch.as_strided(fs.m, p.shape, p.stride(), o)
                st["exp_avg_sq"] = torch.as_strided(fs.v, p.shape, p.stride(), o)
        return fs

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        coef = None  # the per-tensor path's coefficient: one global norm, taken when first needed
        for group in self.param_groups:
            (b1, b2), lr, eps, wd = group["betas"], group["lr"], group["eps"], group["weight_decay"]
            sp = self._flat_space_of(group)
            if sp is not None and sp.param_flat.is_cuda:
                if not sp.grads_attached():
                    sp.gather_grads()
                fs = self._flat_state(sp, group["exclude_1d"])
                mirror = sp.mirror()
                tb = fs.table
                krsc = mirror.krsc if mirror is not None else None
                if fs.clip is None and not self.trust_clip:  # exactly the calls of a step without clipping
                    native_opt().lamb_step(sp.param_flat, sp.grad_flat, fs.m, fs.v, tb.table, tb.partials, tb.trust,
                                           fs.rec, 0, tb.nseg, lr, b1, b2, eps, wd, group["trust"], True, krsc)
                else:
                    if fs.clip is not None:
                        native_opt().grad_norm(sp.grad_flat, fs.gpart, fs.clip, self.max_grad_norm)
                    native_opt().lamb_step(sp.param_flat, sp.grad_flat, fs.m, fs.v, tb.table, tb.partials, tb.trust,
                                           fs.rec, 0, tb.nseg, lr, b1, b2, eps, wd, group["trust"], True, krsc,
                                           clip=fs.clip, trust_clip=self.trust_clip)
                if mirror is not None:
                    mirror.after_optimizer_step()  # bf16 conv weights for the next forward
                continue
            if coef is None:
                coef = ref.clip_coef(self._loose_grads(), self.max_grad_norm)[1] if self.max_grad_norm > 0.0 else 1.0
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if "exp_avg" not in st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                ref.lamb_([p], [p.grad], [st["exp_avg"]], [st["exp_avg_sq"]], int(st["step"]), lr, b1, b2, eps, wd,
                          group["trust"], group["exclude_1d"], coef, self.trust_clip)
        return loss

    def _loose_grads(self):
        """The gradients of every group that takes the per-tensor path."""
        out = []
        for group in self.param_groups:
            sp = self._flat_space_of(group)
            if sp is None or not sp.param_flat.is_cuda:
                out += [p.grad for p in group["params"] if p.grad is not None]
        return out

    def _flat_groups(self):
        for group in self.param_groups:
            sp = self._flat_space_of(group)
            if sp is not None and id(sp) in self._flat:
                yield sp, self._flat[id(sp)]

    def state_dict(self):
        # the one host read of the device record: at save time only
        for sp, fs in self._flat_groups():
            done = float(fs.rec[0].item())
            for p in sp.params:
                self.state[p]["step"] = torch.tensor(done)
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # the moments arrive as standalone tensors: copy them into the flat buffers' views, and the
        # update count into the device record
        for sp, fs in self._flat_groups():
            done = 0
            for p, o in zip(sp.params, sp.offsets):
                st = self.state[p]
                for key, flat in (("exp_avg", fs.m), ("exp_avg_sq", fs.v)):
                    view = torch.as_strided(flat, p.shape, p.stride(), o)
                    if st.get(key) is not None:
                        view.copy_(st[key])
                    else:
                        view.zero_()
                    st[key] = view
                done = max(done, int(st.get("step", 0)))
                st["step"] = torch.tensor(float(done))
            fs.rec.zero_()
            fs.rec[0] = done
