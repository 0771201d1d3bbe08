"""Exponential moving average of a model's weights -- ``torch.optim.swa_utils.AveragedModel`` with
``use_buffers=True`` and ``get_ema_multi_avg_fn(decay)``, on the flat storage.

    ema = ModelEma(ddp_model, decay=0.9998)
    ...
    optimizer.step()
    ema.update()
    ...
    evaluate(ema.module, ...)

``ema.module`` is a twin of the wrapped module (eval mode, nothing requires grad).  Update number k
takes ``e <- e + w * (p - e)`` for every parameter and float buffer, with w = 1 for k = 0 (a copy,
as ``AveragedModel`` does while ``n_averaged == 0``) and ``w = 1 - d_k`` afterwards, ``d_k = decay``
or, with ``warmup=True``, ``min(decay, (1 + k) / (10 + k))`` (timm's rule).  Integer buffers
(``num_batches_tracked``) are copied, not averaged.  ``every=N``: only every N-th ``update()``
call updates.

When the model's parameters live in a GPU ``FlatParamSpace`` (what our ``DistributedDataParallel``
creates, for both ``impl`` values), the twin owns one fp32 flat parameter buffer with the source's
permutation, offsets and strides, its ``WeightMirror`` and flat buffers in the source's order, and
the whole update is ONE launch of ``_C_ema.ema_update`` on the current stream (after ``step()`` has
joined the per-bucket updates that is correctly ordered; no side stream: a fork costs more than the
kernel, profiles/r9f_stream_fork_costs.txt).  The launch also writes bf16(e') into the twin mirror's
``krsc`` image, so an evaluation of the twin needs no cast pass: the raw writes bump no torch
version counter, so the twin is marked stale and its next forward first bumps the space's version
and rebuilds the dgrad layout (``mirror.after_optimizer_step()``: one ``pack_t`` per evaluation, not
per update), after which the model forward's ``ensure()`` finds the mirror valid.

Everything else -- CPU tensors, parameters outside a flat space, ``PDT_DISABLE_NATIVE=1`` -- takes
the reference path: ``torch._foreach_lerp_`` over the float tensors and ``copy_`` for the integer
buffers, bitwise equal to the ``AveragedModel`` above on the CPU.

Distributed: every rank holds the same parameters, so every rank keeps its own identical EMA; there
are no collectives.
"""
from __future__ import annotations

import copy
import os
import warnings
from typing import Dict, List, Optional

import torch

from ..ops import _ext
from ..parallel.flat import FlatParamSpace, flatten_buffers


def _source_space(params: List[torch.nn.Parameter]) -> Optional[FlatParamSpace]:
    """The GPU flat space that holds exactly ``params``, or None."""
    if not params:
        return None
    sp = getattr(params[0], "_pdt_flat", None)
    if sp is None or not sp.param_flat.is_cuda or sp.param_flat.dtype != torch.float32:
        return None
    if len(params) != len(sp.params) or {id(p) for p in params} != {id(p) for p in sp.params}:
        return None
    return sp


class ModelEma:
    def __init__(self, model: torch.nn.Module, decay: float, every: int = 1, warmup: bool = False):
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"decay must be in [0, 1), got {decay}")
        if int(every) != every or every < 1:
            raise ValueError(f"every must be an integer >= 1, got {every}")
        self.decay, self.every, self.warmup = float(decay), int(every), bool(warmup)
        self.num_updates = 0
        self._calls = 0
        wrapped = (hasattr(model, "space") and hasattr(model, "buffer_flats")) \
            or isinstance(model, torch.nn.parallel.DistributedDataParallel)
        src = model.module if wrapped else model
        self.source = src
        self._stale: Optional[str] = None  # "krsc": the kernel wrote krsc; "all": torch wrote the weights
        self._flat = None
        self.module = self._twin(src)
        self._pairs()
        sp = _source_space([p for p in src.parameters()])
        if sp is not None and os.environ.get("PDT_DISABLE_NATIVE", "0") != "1":
            _ext.native_ema()  # a missing kernel is an error, not a reason to fall back
            self._flatten(model, src, sp)

    # ------------------------------------------------------------------ the twin
    @staticmethod
    def _twin(src: torch.nn.Module) -> torch.nn.Module:
        """A copy of ``src`` with fresh, compact parameters and buffers.  The module structure is
        deep-copied, but every parameter and buffer is replaced up front (deepcopy's memo), so a view
        of a flat space is never deep-copied: that would drag the whole space, its gradient buffer
        and every per-parameter attachment along."""
        memo: Dict[int, object] = {}
        with torch.no_grad():
            for p in src.parameters():
                q = torch.empty_strided(p.shape, p.stride(), dtype=p.dtype, device=p.device)
                memo[id(p)] = torch.nn.Parameter(q.copy_(p.detach()), requires_grad=False)
            for b in src.buffers():
                memo[id(b)] = b.detach().clone()
        twin = copy.deepcopy(src, memo)
        from .. import ops
        for m in twin.modules():
            ops.forget_bn_modules(m)  # caches of the source's forward
        twin.eval()
        return twin

    def _pairs(self) -> None:
        """(twin tensor, source tensor) of every parameter and buffer, mapped by name."""
        sp_, sb_ = dict(self.source.named_parameters()), dict(self.source.named_buffers())
        tp_, tb_ = dict(self.module.named_parameters()), dict(self.module.named_buffers())
        assert list(sp_) == list(tp_) and list(sb_) == list(tb_), "the twin's state differs from the model's"
        self._param_pairs = [(tp_[k], sp_[k]) for k in sp_]
        self._buffer_pairs = [(tb_[k], sb_[k]) for k in sb_]
        pairs = self._param_pairs + self._buffer_pairs
        for t, s in pairs:
            assert t.shape == s.shape and t.dtype == s.dtype and t.device == s.device
        self._float_pairs = [(t, s) for t, s in pairs if t.is_floating_point()]
        self._int_pairs = [(t, s) for t, s in pairs if not t.is_floating_point()]

    def _flatten(self, model, src, sp: FlatParamSpace) -> None:
        """Re-home the twin into flat storage of the source's layout and plan the one-launch update."""
        name_of = {id(p): n for n, p in src.named_parameters()}
        twin_params = dict(self.module.named_parameters())
        tsp = FlatParamSpace([twin_params[name_of[id(p)]] for p in sp.params], grads=False)
        assert tsp.numel == sp.numel and tsp.offsets == sp.offsets
        for t, s in zip(tsp.params, sp.params):
            assert t.shape == s.shape and t.stride() == s.stride(), "twin layout differs from the model's"
        mirror = tsp.mirror() if _ext.native_available() else None
        if mirror is not None and not mirror.ntensors:
            mirror = None  # nothing reads a bf16 image (--impl torch): no side output
        # buffers: one flat tensor per dtype, in the source's order
        owner = model if hasattr(model, "buffer_flats") else (sp.owner() if hasattr(sp, "owner") else None)
        src_flats = getattr(owner, "buffer_flats", None) or {}
        twin_flats = flatten_buffers(self.module)
        self._pairs()  # the twin's tensors were re-homed
        fused = {}
        for dt in (torch.float32, torch.int64):
            if dt in twin_flats and dt in src_flats and self._same_layout(twin_flats[dt], src_flats[dt], dt):
                fused[dt] = (twin_flats[dt], src_flats[dt])
        # what the launch does not cover stays on the reference path (the parameters are all covered)
        rest = [(t, s) for t, s in self._buffer_pairs if t.dtype not in fused]
        self._float_pairs = [(t, s) for t, s in rest if t.is_floating_point()]
        self._int_pairs = [(t, s) for t, s in rest if not t.is_floating_point()]
        self._flat = (tsp, sp, mirror, fused.get(torch.float32, (None, None)), fused.get(torch.int64, (None, None)))
        self.module.register_forward_pre_hook(lambda _m, _a: self.sync_mirror())

    def _same_layout(self, twin_flat: torch.Tensor, src_flat: torch.Tensor, dt: torch.dtype) -> bool:
        """Every buffer of ``dt`` sits at the same offset of its flat tensor on both sides."""
        if twin_flat.numel() != src_flat.numel() or twin_flat.device != src_flat.device:
            return False
        sb_, tb_ = dict(self.source.named_buffers()), dict(self.module.named_buffers())
        esz = twin_flat.element_size()
        for k, s in sb_.items():
            if s.dtype != dt:
                continue
            t = tb_[k]
            so, to = s.data_ptr() - src_flat.data_ptr(), t.data_ptr() - twin_flat.data_ptr()
            if so != to or so < 0 or so + s.numel() * esz > src_flat.numel() * esz or not s.is_contiguous():
                return False
        return True

    # ------------------------------------------------------------------ updates
    def weight(self, k: int) -> float:
        """w = 1 - d_k of update number k (Python double)."""
        if k == 0:
            return 1.0
        d = min(self.decay, (1.0 + k) / (10.0 + k)) if self.warmup else self.decay
        return 1.0 - d

    @torch.no_grad()
    def update(self) -> bool:
        """Call after ``optimizer.step()``; True if this call updated the average."""
        self._calls += 1
        if self._calls % self.every:
            return False
        self._apply(self.weight(self.num_updates), first=self.num_updates == 0)
        self.num_updates += 1
        return True

    @torch.no_grad()
    def reset(self) -> None:
        """Start over from the model's current weights: the next update is number 0 again."""
        self._apply(1.0, first=True)
        self.num_updates = 0
        self._calls = 0

    def _apply(self, w: float, first: bool) -> None:
        if self._flat is not None:
            tsp, sp, mirror, (fe, fm), (ie, im) = self._flat
            _ext.native_ema().ema_update(tsp.param_flat, sp.param_flat, w, mirror.krsc if mirror is not None else None,
                                         fe, fm, ie, im)
            if self._stale != "all":
                self._stale = "krsc"
        if self._float_pairs:
            if first:  # a copy, as AveragedModel does while n_averaged == 0
                for t, s in self._float_pairs:
                    t.copy_(s)
            else:
                torch._foreach_lerp_([t for t, _ in self._float_pairs], [s.detach() for _, s in self._float_pairs], w)
        for t, s in self._int_pairs:
            t.copy_(s)

    def sync_mirror(self) -> None:
        """Make the twin's bf16 weight mirror current (runs before every forward of the twin)."""
        if self._flat is None or self._stale is None:
            return
        mirror = self._flat[2]
        if mirror is not None:
            if self._stale == "krsc":
                mirror.after_optimizer_step()  # bumps the space's version, packs the dgrad layout
            else:
                mirror.refresh()
        self._stale = None

    # ------------------------------------------------------------------ state
    def state_dict(self) -> dict:
        """The twin's state, ``module.``-prefixed: the schema of the main checkpoint."""
        return self.module.state_dict(prefix="module.")

    def load_state_dict(self, sd: dict) -> None:
        pre = "module."
        self.module.load_state_dict({(k[len(pre):] if k.startswith(pre) else k): v for k, v in sd.items()},
                                    strict=True)
        self._stale = "all"

    def extra_state(self) -> dict:
        return {"num_updates": self.num_updates, "decay": self.decay, "every": self.every, "warmup": self.warmup}

    def load_extra_state(self, st: dict) -> None:
        """Continue the update count of a checkpoint.  decay / every / warmup stay as constructed (a
        resumed run may change them on purpose); a difference is reported."""
        self.num_updates = int(st["num_updates"])
        self._calls = self.num_updates * self.every
        for k in ("decay", "every", "warmup"):
            if k in st and st[k] != getattr(self, k):
                warnings.warn(f"ModelEma: the checkpoint was written with {k}={st[k]!r}, continuing with "
                              f"{k}={getattr(self, k)!r}")
        if self._flat is not None:
            self._stale = "all"
