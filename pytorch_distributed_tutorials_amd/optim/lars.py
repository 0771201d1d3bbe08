"""LARS -- layer-wise adaptive rate scaling (You, Gitman, Ginsburg 2017) -- fused.

The large-batch ResNet recipe: every parameter tensor's update is scaled by its trust ratio
``eta * |p| / (|g| + wd * |p| + eps)``; BatchNorm weights and biases and the fc bias
(``exclude_1d``: every tensor with ``ndim <= 1``) get neither weight decay nor the ratio.  The
"rescale the gradient, then SGD" form is used (``ops/reference.py::lars_momentum_`` is the exact
semantics and the CPU path), so ``momentum_buffer`` keeps ``torch.optim.SGD``'s format.

``LARS`` subclasses ``optim.SGD`` and keeps everything that class built around the flat parameter
space: one fused pass over the flat param/grad/momentum buffers that also writes the bf16 KRSC
weight mirror (``csrc/kernels/lars.hip``), torch-format ``state_dict()``, and the per-bucket update
inside backward (``overlap``; same contract as ``SGD``).  The norms are float64 sums in a fixed
order that depends on the parameter layout alone, so every rank of a data-parallel job computes
bitwise-identical ratios from its copy of the all-reduced gradients, and the per-bucket update is
bitwise the post-backward step.  No host synchronisation: the ratios never leave the device, so a
captured step (``utils.graph.CapturedStep``) stays valid.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

from ..ops import reference as ref
from ..ops._ext import native
from .sgd import SGD


class LarsTable:
    """Device segment / chunk table of one flat space plus the kernels' work buffers.

    ``segments``: ``(offset, numel, excluded)`` per parameter tensor, in flat order, offsets in
    elements from the start of the flat buffers.  Every segment is cut into chunks of at most
    ``lars_chunk_elems()`` elements; a chunk never crosses a segment.  ``table`` holds the segment
    entries followed by the chunk entries, ``partials`` one float64 ``(sum p^2, sum g^2)`` per
    chunk, ``trust`` one fp32 ratio per segment.
    """

    def __init__(self, segments: Sequence[Tuple[int, int, bool]], device):
        import numpy as np
        C = native()
        chunk = int(C.lars_chunk_elems())
        seg_dt = np.dtype([("off", "<i8"), ("numel", "<i8"), ("chunk0", "<i4"), ("nchunks", "<i4"),
                           ("flags", "<i4"), ("pad", "<i4")])
        chunk_dt = np.dtype([("start", "<i8"), ("n", "<i4"), ("seg", "<u4")])
        assert seg_dt.itemsize == C.lars_entry_bytes(), "LarsSeg layout mismatch"
        assert chunk_dt.itemsize == C.lars_chunk_entry_bytes(), "LarsChunk layout mismatch"
        if not segments:
            raise ValueError("LarsTable needs at least one segment")
        segs, chunks = [], []
        self.chunk0: List[int] = []  # first chunk of every segment, and the total at the end
        for si, (off, numel, excluded) in enumerate(segments):
            n = (numel + chunk - 1) // chunk
            self.chunk0.append(len(chunks))
            segs.append((off, numel, len(chunks), n, 1 if excluded else 0, 0))
            for k in range(n):
                start = off + k * chunk
                # bit 31 of a chunk's segment index repeats the segment's excluded flag
                chunks.append((start, min(chunk, off + numel - start), si | (0x80000000 if excluded else 0)))
        self.chunk0.append(len(chunks))
        self.nseg, self.nchunks = len(segs), len(chunks)
        raw = np.array(segs, dtype=seg_dt).view(np.uint8).tobytes() + \
            np.array(chunks, dtype=chunk_dt).view(np.uint8).tobytes()
        self.table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
        self.partials = torch.zeros(2 * self.nchunks, dtype=torch.float64, device=device)
        self.trust = torch.ones(self.nseg, dtype=torch.float32, device=device)

    def chunks_in(self, seg_lo: int, seg_hi: int) -> int:
        return self.chunk0[seg_hi] - self.chunk0[seg_lo]


class LARS(SGD):
    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.9, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False, trust_coefficient: float = 1e-3,
                 eps: float = 1e-8, exclude_1d: bool = True, overlap=None):
        if trust_coefficient <= 0.0:
            raise ValueError(f"Invalid trust_coefficient: {trust_coefficient}")
        if eps < 0.0:
            raise ValueError(f"Invalid eps: {eps}")
        self._lars_defaults = dict(trust_coefficient=trust_coefficient, eps=eps, exclude_1d=bool(exclude_1d))
        self._lars_tables = {}  # (flat space id, exclude_1d) -> LarsTable
        # the per-bucket update attaches at the end of SGD.__init__, after the groups carry the keys
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                         nesterov=nesterov, overlap=overlap)
        self.defaults.update(self._lars_defaults)
        # build the device table now (not inside a captured first step)
        for group in self.param_groups:
            sp = self._flat_space_of(group)
            if sp is not None and sp.param_flat.is_cuda:
                self._table(sp, group["exclude_1d"])

    def add_param_group(self, param_group):
        for k, v in self._lars_defaults.items():
            param_group.setdefault(k, v)
        super().add_param_group(param_group)

    def _hyper(self, group):
        return super()._hyper(group) + (group["trust_coefficient"], group["eps"], group["exclude_1d"])

    def _table(self, sp, exclude_1d: bool) -> LarsTable:
        key = (id(sp), bool(exclude_1d))
        tb = self._lars_tables.get(key)
        if tb is None:
            tb = LarsTable([(o, p.numel(), bool(exclude_1d and p.ndim <= 1))
                            for p, o in zip(sp.params, sp.offsets)], sp.param_flat.device)
            self._lars_tables[key] = tb
        return tb

    def _bucket_ranges(self, sp, tb: LarsTable):
        """(seg_lo, seg_hi, chunks) per gradient bucket of the space's DDP wrapper: buckets are
        lists of whole parameters in flat order, so each is a contiguous segment range."""
        owner = self._overlap_owner() if self._overlap_owner is not None else None
        if owner is None:
            raise RuntimeError("LARS: the per-bucket update lost its DistributedDataParallel wrapper")
        cached = getattr(tb, "_bucket_ranges", None)
        if cached is not None and cached[0] == owner.bucket_ranges:
            return cached[1]
        seg_at = {o: i for i, o in enumerate(sp.offsets)}
        seg_at[sp.numel] = len(sp.offsets)
        ranges = []
        for start, end in owner.bucket_ranges:
            if start not in seg_at or end not in seg_at:
                raise RuntimeError("LARS: a gradient bucket does not start and end on parameter boundaries")
            lo, hi = seg_at[start], seg_at[end]
            ranges.append((lo, hi, tb.chunks_in(lo, hi)))
        tb._bucket_ranges = (list(owner.bucket_ranges), ranges)
        return ranges

    def _arm_overlap(self, reducer) -> None:
        super()._arm_overlap(reducer)  # contract checks, momentum buffer, mirror: the SGD arguments
        if self._armed is None:
            return
        group = self.param_groups[0]
        sp = self._flat_space_of(group)
        tb = self._table(sp, group["exclude_1d"])
        reducer.arm_lars(tb.table, tb.partials, tb.trust, group["weight_decay"], group["trust_coefficient"],
                         group["eps"], self._bucket_ranges(sp, tb))

    # SGD.step() with these two update rules
    def _flat_update(self, sp, group, buf, first, krsc) -> None:
        tb = self._table(sp, group["exclude_1d"])
        native().lars_step(sp.param_flat, sp.grad_flat, buf, tb.table, tb.partials, tb.trust, 0, tb.nseg,
                           group["lr"], group["momentum"], group["dampening"], group["weight_decay"],
                           group["nesterov"], first, group["trust_coefficient"], group["eps"], krsc)

    def _tensor_update(self, group, p, g, buf, first) -> None:
        ref.lars_momentum_([p], [g], [buf], group["lr"], group["momentum"], group["dampening"],
                           group["weight_decay"], group["nesterov"], first, group["trust_coefficient"],
                           group["eps"], group["exclude_1d"])

