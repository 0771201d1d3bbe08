"""Loader for the in-tree native extension (``pytorch_distributed_tutorials_amd/_C*.so``).

The extension is built by ``build_native.py`` (or ``__graft_entry__.build()``)
with hipcc for gfx950 and lives next to this package, so it travels with the
repo snapshot to the GPU box.  On a GPU, every op in ``ops/`` dispatches to it
and FAILS LOUDLY when it is missing -- there is no silent eager fallback for
device tensors.  CPU tensors use the PyTorch reference implementations (tests).

The MixUp / CutMix ops live in a second module of the same build, ``_C_mix*.so`` (the public
surface of ``_C`` is pinned); ``native_mix()`` loads it under the same rules.
"""
from __future__ import annotations

import importlib
import importlib.util as importlib_util
import os
from typing import Any, Optional

_C: Optional[Any] = None
_ERR: Optional[BaseException] = None
_LOADED = False


def _load() -> None:
    global _C, _ERR, _LOADED
    if _LOADED:
        return
    _LOADED = True
    if os.environ.get("PDT_DISABLE_NATIVE", "0") == "1":
        _ERR = RuntimeError("native extension disabled by PDT_DISABLE_NATIVE=1")
        return
    try:
        import torch  # noqa: F401  (libtorch must be loaded before _C)
        so = os.environ.get("PDT_NATIVE_SO")
        if so:  # an alternative build of the same module (build_native.py --sanitize)
            import sys
            spec = importlib_util.spec_from_file_location("pytorch_distributed_tutorials_amd._C", so)
            _C = importlib_util.module_from_spec(spec)
            spec.loader.exec_module(_C)
            sys.modules["pytorch_distributed_tutorials_amd._C"] = _C
            return
        _C = importlib.import_module("pytorch_distributed_tutorials_amd._C")
    except BaseException as e:  # ImportError, OSError (missing .so deps) ...
        _C = None
        _ERR = e


_C_MIX: Optional[Any] = None
_ERR_MIX: Optional[BaseException] = None
_LOADED_MIX = False


def _load_mix() -> None:
    """The second extension module, ``_C_mix`` (MixUp / CutMix ops), by the rules of ``_load``."""
    global _C_MIX, _ERR_MIX, _LOADED_MIX
    if _LOADED_MIX:
        return
    _LOADED_MIX = True
    if os.environ.get("PDT_DISABLE_NATIVE", "0") == "1":
        _ERR_MIX = RuntimeError("native extension disabled by PDT_DISABLE_NATIVE=1")
        return
    name = "pytorch_distributed_tutorials_amd._C_mix"
    try:
        import torch  # noqa: F401  (libtorch must be loaded before _C_mix)
        so = os.environ.get("PDT_NATIVE_SO")
        if so:  # the alternative build keeps its _C_mix next to its _C
            import sys
            so = os.path.join(os.path.dirname(so), os.path.basename(so).replace("_C", "_C_mix", 1))
            spec = importlib_util.spec_from_file_location(name, so)
            _C_MIX = importlib_util.module_from_spec(spec)
            spec.loader.exec_module(_C_MIX)
            sys.modules[name] = _C_MIX
            return
        _C_MIX = importlib.import_module(name)
    except BaseException as e:  # ImportError, OSError (missing .so deps) ...
        _C_MIX = None
        _ERR_MIX = e


def native_available() -> bool:
    _load()
    return _C is not None


def native_mix_available() -> bool:
    _load_mix()
    return _C_MIX is not None


def native_mix() -> Any:
    """Return the batch-mixing extension module or raise with the reason it failed to load."""
    _load_mix()
    if _C_MIX is None:
        raise RuntimeError(
            "pytorch_distributed_tutorials_amd native extension (_C_mix) is not available: "
            f"{_ERR_MIX!r}.  Build it with `python build_native.py` (hipcc, gfx950)."
        )
    return _C_MIX


def native() -> Any:
    """Return the extension module or raise with the reason it failed to load."""
    _load()
    if _C is None:
        raise RuntimeError(
            "pytorch_distributed_tutorials_amd native extension (_C) is not available: "
            f"{_ERR!r}.  Build it with `python build_native.py` (hipcc, gfx950)."
        )
    return _C
