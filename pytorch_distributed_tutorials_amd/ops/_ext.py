"""Loader for the in-tree native extension (``pytorch_distributed_tutorials_amd/_C*.so``).

The extension is built by ``build_native.py`` (or ``__graft_entry__.build()``)
with hipcc for gfx950 and lives next to this package, so it travels with the
repo snapshot to the GPU box.  On a GPU, every op in ``ops/`` dispatches to it
and FAILS LOUDLY when it is missing -- there is no silent eager fallback for
device tensors.  CPU tensors use the PyTorch reference implementations (tests).

The MixUp / CutMix ops live in a second module of the same build, ``_C_mix*.so``, and the
resampling input transform and the augmentation policy in a third, ``_C_img*.so``, and the weight-EMA update in a fourth,
``_C_ema*.so`` (the public surface of ``_C`` is pinned); ``native_mix()``, ``native_img()`` and
``native_ema()`` load them under the same rules.
"""
from __future__ import annotations

import importlib
import importlib.util as importlib_util
import os
from typing import Any, Dict, Optional, Tuple

# module name ("_C", "_C_mix", "_C_img", "_C_ema") -> (module or None, the reason it failed to load or None)
_MODULES: Dict[str, Tuple[Optional[Any], Optional[BaseException]]] = {}


def _load(mod: str = "_C") -> Tuple[Optional[Any], Optional[BaseException]]:
    """Import one extension module, once; every later call returns the first outcome."""
    if mod in _MODULES:
        return _MODULES[mod]
    if os.environ.get("PDT_DISABLE_NATIVE", "0") == "1":
        _MODULES[mod] = (None, RuntimeError("native extension disabled by PDT_DISABLE_NATIVE=1"))
        return _MODULES[mod]
    name = "pytorch_distributed_tutorials_amd." + mod
    try:
        import torch  # noqa: F401  (libtorch must be loaded before the extension)
        so = os.environ.get("PDT_NATIVE_SO")
        if so:  # an alternative build (build_native.py --sanitize): its modules sit next to its _C
            import sys
            so = os.path.join(os.path.dirname(so), os.path.basename(so).replace("_C", mod, 1))
            spec = importlib_util.spec_from_file_location(name, so)
            m = importlib_util.module_from_spec(spec)
            spec.loader.exec_module(m)
            sys.modules[name] = m
        else:
            m = importlib.import_module(name)
        _MODULES[mod] = (m, None)
    except BaseException as e:  # ImportError, OSError (missing .so deps) ...
        _MODULES[mod] = (None, e)
    return _MODULES[mod]


def _require(mod: str) -> Any:
    m, err = _load(mod)
    if m is None:
        raise RuntimeError(
            f"pytorch_distributed_tutorials_amd native extension ({mod}) is not available: "
            f"{err!r}.  Build it with `python build_native.py` (hipcc, gfx950)."
        )
    return m


def native_available() -> bool:
    return _load("_C")[0] is not None


def native_mix_available() -> bool:
    return _load("_C_mix")[0] is not None


def native_img_available() -> bool:
    return _load("_C_img")[0] is not None


def native_ema_available() -> bool:
    return _load("_C_ema")[0] is not None


def native_mix() -> Any:
    """Return the batch-mixing extension module or raise with the reason it failed to load."""
    return _require("_C_mix")


def native_img() -> Any:
    """Return the input-transform extension module or raise with the reason it failed to load."""
    return _require("_C_img")


def native_ema() -> Any:
    """Return the weight-EMA extension module or raise with the reason it failed to load."""
    return _require("_C_ema")


def native() -> Any:
    """Return the extension module or raise with the reason it failed to load."""
    return _require("_C")
