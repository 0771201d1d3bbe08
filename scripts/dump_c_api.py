#!/usr/bin/env python3
"""Describe the Python surface of the native extension `_C` from its pybind11 docstrings.

    python scripts/dump_c_api.py [--write]

For every public name of `_C`: the list of [parameter name, default text or null] of each signature
line (type annotations dropped, so the result does not depend on how a pybind11 version spells
types).  For a class: its public members, the callable ones with their parameter lists.  Needs no
GPU.  `--write` refreshes tests/golden/c_api.json (tests/test_bindings_cpu.py compares against it);
without it the JSON goes to stdout.
"""
from __future__ import annotations

import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "c_api.json")


def _split_top(s: str) -> list:
    """Split at commas outside brackets and quotes."""
    out, depth, quote, cur = [], 0, None, ""
    for ch in s:
        if quote:
            quote = None if ch == quote else quote
        elif ch in "'\"":
            quote = ch
        elif ch in "([{<":
            depth += 1
        elif ch in ")]}>":
            depth -= 1
        elif ch == "," and depth == 0:
            out.append(cur)
            cur = ""
            continue
        cur += ch
    if cur.strip():
        out.append(cur)
    return out


def _params(sig: str) -> list:
    """`name(a: T, b: T = 1) -> R`  ->  [["a", None], ["b", "1"]]"""
    depth, end = 0, None
    start = sig.index("(")
    for i in range(start, len(sig)):
        depth += sig[i] in "([{"
        depth -= sig[i] in ")]}"
        if depth == 0:
            end = i
            break
    res = []
    for p in _split_top(sig[start + 1:end]):
        p = p.strip()
        if p in ("/", "*"):
            continue
        name = re.match(r"\*{0,2}\w+", p).group(0)
        rest = p[len(name):]
        default = None
        m = re.search(r"(?<![=!<>])=(?!=)", rest)
        if m:
            default = rest[m.end():].strip()
        res.append([name, default])
    return res


def _signatures(name: str, doc) -> list:
    """Parameter lists of every signature line of a pybind11 docstring (overloads: one each)."""
    lines = [ln.strip() for ln in (doc or "").splitlines()]
    pat = re.compile(r"^(?:\d+\.\s+)?" + re.escape(name) + r"\(")
    return [_params(re.sub(r"^\d+\.\s+", "", ln)) for ln in lines
            if pat.match(ln) and "Overloaded function" not in ln]


def describe(mod) -> dict:
    import inspect
    api = {}
    for name in sorted(n for n in dir(mod) if not n.startswith("_")):
        obj = getattr(mod, name)
        if inspect.isclass(obj):
            members = {"__init__": _signatures("__init__", obj.__init__.__doc__)}
            for mn in sorted(n for n in vars(obj) if not n.startswith("_")):
                raw = vars(obj)[mn]
                if isinstance(raw, property):
                    members[mn] = "property"
                else:
                    members[mn] = _signatures(mn, getattr(obj, mn).__doc__)
            api[name] = {"class": members}
        else:
            api[name] = _signatures(name, obj.__doc__)
    return api


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else argv
    sys.path.insert(0, ROOT)
    from pytorch_distributed_tutorials_amd.ops import _ext
    text = json.dumps(describe(_ext.native()), indent=1, sort_keys=True) + "\n"
    if "--write" in argv:
        os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
        with open(GOLDEN, "w") as f:
            f.write(text)
        print(GOLDEN)
    else:
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
