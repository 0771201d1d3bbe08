#!/usr/bin/env python3
"""Record every native call of one training step, per autograd node, and hash the record.

    python scripts/dump_block_calls.py [--write] [--text DIR] [config ...]

``ops/fused.py`` decides which kernel runs, on which stream, with which sink and which accumulator.
This tool pins those decisions: ``fused.native`` is wrapped so it returns a proxy of ``_C``, and
every call through the proxy becomes one line

    op @role(arg, arg, ...) -> result

with the stream role current at call time (``main``, ``side`` = the weight-gradient stream,
``branch`` = the projection-shortcut stream) and a descriptor per argument and result: ``-`` for
None, ``repr`` for bool / int / float (an int equal to the raw handle of the side or branch stream
is that role's name), lists and tuples recursively, and ``dtype[shape]#k`` for a tensor, where k is
the first-seen index of its (data_ptr, dtype, shape).  The recorder keeps every tensor it has seen
alive until the recording ends, so no address is reused and passing ``y`` where ``z`` belongs shows
even at equal shapes.  ``streams.fork`` / ``join`` / ``begin`` and ``torch.cuda.Stream.wait_event``
are recorded too, with the roles of the streams involved.  The lines are split per autograd node
and phase (stem forward, each block forward, head forward, then the backwards in execution order).

Each configuration (CONFIGS) is a whole model on batch 8 of 3x64x64 images, 10 classes, one forward
plus backward from ``torch.manual_seed(0)``.  ``--write`` refreshes tests/golden/block_calls.json
(per configuration and node: the number of lines and the sha256 of their text, plus how far
FOLD_CALLS / DUAL_CALLS advanced); ``--text DIR`` writes the full lines, one file per configuration,
so a mismatch can be diffed against a dump taken from another commit.  Needs a GPU.
tests/test_block_calls_gpu.py compares against the golden.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "block_calls.json")

# name -> (arch, flat space, mode); modes: det, fp8, no_bn_acc, eval
CONFIGS = {
    "resnet50": ("resnet50", True, None),
    "resnet50_det": ("resnet50", True, "det"),
    "resnet50_fp8": ("resnet50", True, "fp8"),
    "resnet50_noflat": ("resnet50", False, None),
    "resnet18": ("resnet18", True, None),
    "resnet18_fp8": ("resnet18", True, "fp8"),
    "resnet50_no_bn_acc": ("resnet50", True, "no_bn_acc"),
    "resnet50_eval": ("resnet50", True, "eval"),
}


class _Proxy:
    """Stands in for ``_C``: callables are recorded, everything else passes through."""

    def __init__(self, rec, C):
        self._rec, self._C = rec, C

    def __getattr__(self, name):
        attr = getattr(self._C, name)
        if not callable(attr):
            return attr
        rec = self._rec

        def call(*args, **kwargs):
            role = rec.role()
            head = f"{name} @{role}({', '.join(rec.describe_args(args, kwargs))})"
            out = attr(*args, **kwargs)
            rec.line(f"{head} -> {rec.describe(out)}")
            return out
        return call


class Recorder:
    """Context manager: while active, native calls and stream hand-offs of ``ops.fused`` are
    recorded into ``sections``, a list of [node/phase name, lines]."""

    def __init__(self, device):
        import pytorch_distributed_tutorials_amd.ops.fused as fused
        from pytorch_distributed_tutorials_amd.ops import streams
        self.fused, self.streams = fused, streams
        self.device = device
        self.sections = []
        self._cur = None       # lines of the node running now (None between nodes)
        self._seen = {}        # (data_ptr, dtype, shape) -> first-seen index
        self._keep = []        # every tensor seen, so no address is reused while recording
        self._handles = {}
        for role, fn in (("side", streams.wgrad_stream), ("branch", streams.branch_stream)):
            s = fn(device)
            if s is not None:
                self._handles[s.cuda_stream] = role
        self._undo = []

    # -- descriptors ---------------------------------------------------------------------------
    def stream_role(self, s) -> str:
        if s is None:
            return "-"
        return self._handles.get(s.cuda_stream, "main" if s == self._main else "other")

    def role(self) -> str:
        return self.stream_role(torch.cuda.current_stream(self.device))

    def describe(self, v) -> str:
        if v is None:
            return "-"
        if isinstance(v, torch.Tensor):
            key = (v.data_ptr(), v.dtype, tuple(v.shape))
            k = self._seen.get(key)
            if k is None:
                k = self._seen[key] = len(self._seen)
                self._keep.append(v)
            return f"{str(v.dtype).replace('torch.', '')}{list(v.shape)}#{k}"
        if isinstance(v, bool):
            return repr(v)
        if isinstance(v, int):
            return self._handles.get(v, repr(v))
        if isinstance(v, float):
            return repr(v)
        if isinstance(v, (list, tuple)):
            inner = ", ".join(self.describe(e) for e in v)
            return f"[{inner}]" if isinstance(v, list) else f"({inner})"
        if isinstance(v, (torch.cuda.Stream, torch.cuda.Event)):
            return self.stream_role(v) if isinstance(v, torch.cuda.Stream) else "event"
        return type(v).__name__

    def describe_args(self, args, kwargs) -> list:
        return [self.describe(a) for a in args] + [f"{k}={self.describe(v)}" for k, v in sorted(kwargs.items())]

    def line(self, text: str) -> None:
        if self._cur is None:  # a call between nodes (the model's own glue)
            self.sections.append([f"{len(self.sections):03d} outside", []])
            self._cur = self.sections[-1][1]
        self._cur.append(text)

    # -- patching ------------------------------------------------------------------------------
    def _patch(self, owner, name, new) -> None:
        self._undo.append((owner, name, vars(owner)[name]))  # the raw entry (a staticmethod stays one)
        setattr(owner, name, new)

    def _node(self, cls, phase):
        orig = getattr(cls, phase)
        tag = f"{cls.__name__.lstrip('_')} {'fwd' if phase == 'forward' else 'bwd'}"

        def run(*args, **kwargs):
            self.sections.append([f"{len(self.sections):03d} {tag}", []])
            self._cur = self.sections[-1][1]
            try:
                return orig(*args, **kwargs)
            finally:
                self._cur = None
        return staticmethod(run)

    def _traced(self, label, fn, show):
        def run(*args, **kwargs):
            out = fn(*args, **kwargs)
            self.line(f"{label} @{self.role()}({show(args, out)})")
            return out
        return run

    def __enter__(self):
        fused, streams = self.fused, self.streams
        self._main = torch.cuda.current_stream(self.device)
        C = fused.native()
        proxy = _Proxy(self, C)
        self._patch(fused, "native", lambda: proxy)
        for cls in (fused._ConvBN, fused._StemConvBN, fused._StemConvBNPool, fused._MaxPool,
                    fused._AvgPoolLinear, fused._SoftmaxXent, fused._ResidualBlock):
            self._patch(cls, "forward", self._node(cls, "forward"))
            self._patch(cls, "backward", self._node(cls, "backward"))
        role = self.stream_role
        self._patch(streams, "fork", self._traced(
            "streams.fork", streams.fork,
            lambda a, out: ", ".join([role(a[0])] + [self.describe(t) for t in a[1:]]) + f" -> {role(out)}"))
        self._patch(streams, "join", self._traced(
            "streams.join", streams.join,
            lambda a, out: ", ".join([role(a[0]), role(a[1])] + [self.describe(t) for t in a[2:]])))
        self._patch(streams, "begin", self._traced("streams.begin", streams.begin, lambda a, out: f"-> {role(out)}"))
        self._patch(torch.cuda.Stream, "wait_event", self._traced(
            "Stream.wait_event", torch.cuda.Stream.wait_event, lambda a, out: role(a[0])))
        return self

    def __exit__(self, *exc):
        for owner, name, old in reversed(self._undo):
            setattr(owner, name, old)
        self._undo.clear()
        self._keep.clear()
        return False


def _accumulators(model, fused) -> dict:
    """Every persistent accumulator the step must leave zeroed: name -> tensor."""
    out = {}
    for pname, p in model.named_parameters():
        for attr in ("_pdt_bacc", "_pdt_facc", "_pdt_csum"):
            a = getattr(p, attr, None)
            if a is not None:
                out[f"{pname}.{attr}"] = a
    for (k, c, _), ws in fused._FOLD_WS.items():
        for name, t in zip(("t1", "gram", "done"), ws):
            out[f"_FOLD_WS[{k},{c}].{name}"] = t
    return out


def run_config(name: str, device) -> dict:
    """Run one configuration: {"sections": [[node, lines], ...], "fold_calls", "dual_calls",
    "nonzero": names of persistent accumulators not left all zero}."""
    import pytorch_distributed_tutorials_amd.ops.fused as fused
    import pytorch_distributed_tutorials_amd.utils.seed as seed
    from pytorch_distributed_tutorials_amd import ops
    from pytorch_distributed_tutorials_amd.models import build_model
    from pytorch_distributed_tutorials_amd.parallel import DistributedDataParallel
    arch, flat, mode = CONFIGS[name]
    torch.manual_seed(0)
    model = build_model(arch, num_classes=10, impl="native").to(device).set_impl("native")
    net = model
    if flat:
        net = DistributedDataParallel(model)  # flat space + bf16 weight mirror, as in bench.py
        net.space.mirror().ensure()
    x = torch.randn(8, 3, 64, 64, device=device)
    labels = torch.randint(0, 10, (8,), device=device)
    det0, acc0 = seed._DETERMINISTIC, fused._BN_ACC
    folds0, duals0 = fused.FOLD_CALLS, fused.DUAL_CALLS
    try:
        seed._DETERMINISTIC = mode == "det"
        fused._BN_ACC = mode != "no_bn_acc"
        ops.set_fp8(mode == "fp8")
        with Recorder(device) as rec:
            if mode == "eval":
                model.eval()
                with torch.no_grad():
                    net(x)
            else:
                model.train()
                if flat:
                    net.space.zero_grad()
                ops.cross_entropy(net(x), labels).backward()
            torch.cuda.synchronize()
    finally:
        seed._DETERMINISTIC, fused._BN_ACC = det0, acc0
        ops.set_fp8(False)
    torch.cuda.synchronize()
    nonzero = sorted(n for n, t in _accumulators(model, fused).items() if bool(t.ne(0).any()))
    return {"sections": rec.sections, "fold_calls": fused.FOLD_CALLS - folds0,
            "dual_calls": fused.DUAL_CALLS - duals0, "nonzero": nonzero}


def digest(result: dict) -> dict:
    """The golden entry of one run_config result."""
    nodes = [[name, len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()]
             for name, lines in result["sections"]]
    return {"nodes": nodes, "fold_calls": result["fold_calls"], "dual_calls": result["dual_calls"]}


def main() -> int:
    args = sys.argv[1:]
    write = "--write" in args
    text_dir = args[args.index("--text") + 1] if "--text" in args else None
    names = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--text")]
    device = torch.device("cuda:0")
    golden, dirty = {}, []
    for name in names or list(CONFIGS):
        res = run_config(name, device)
        golden[name] = digest(res)
        dirty += [f"{name}: {n}" for n in res["nonzero"]]
        nlines = sum(len(lines) for _, lines in res["sections"])
        print(f"{name}: {len(res['sections'])} nodes, {nlines} lines, fold {res['fold_calls']}, "
              f"dual {res['dual_calls']}, non-zero accumulators {res['nonzero']}", flush=True)
        if text_dir:
            os.makedirs(text_dir, exist_ok=True)
            with open(os.path.join(text_dir, f"{name}.txt"), "w") as f:
                for node, lines in res["sections"]:
                    f.write(f"== {node}\n" + "".join(line + "\n" for line in lines))
    text = json.dumps(golden, indent=1, sort_keys=True) + "\n"
    if write:
        with open(GOLDEN, "w") as f:
            f.write(text)
    elif not text_dir:
        sys.stdout.write(text)
    return 1 if dirty else 0


if __name__ == "__main__":
    sys.exit(main())
