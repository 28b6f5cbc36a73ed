"""Loader for the product library `csrc/librt_amd.so` (C-ABI of include/rt_amd.h).

Fails loudly when the library has not been built: there is no fallback renderer of any kind.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

from ._abi import SIGNATURES, declare
from .api import Backend

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "librt_amd.so")

_backend = None


class LibraryMissing(RuntimeError):
    pass


def load() -> Backend:
    """Load librt_amd.so once; every function of include/rt_amd.h is declared, and a build that lacks one is an error here."""
    global _backend
    if _backend is not None:
        return _backend
    _backend = load_path(os.environ.get("RT_AMD_LIB", LIB_PATH))     # RT_AMD_LIB: developer override (tools/)
    return _backend


def load_path(path: str, allow_missing: bool = False) -> Backend:
    """Load a specific build of the library (tools/ab.py compares kernel variants in one process; allow_missing: a build of another
    revision may lack some of today's entry points)."""
    if not os.path.exists(path):
        raise LibraryMissing(
            f"{path} is missing: build it with `make -C raytracinginrust_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no fallback path.")
    # PyTorch first, when this process is going to use it: torch brings its own copy of the HIP runtime, and a process in which this
    # library's copy was loaded before it leaves torch without a device ("No HIP GPUs are available").  dist.py and bench.py need both,
    # so the preload is the default wherever torch is installed; RT_AMD_NO_TORCH_PRELOAD=1 skips it (a host that never imports torch
    # saves the import), and a torch that is present but broken must not make the renderer unloadable.
    if "torch" not in sys.modules and not os.environ.get("RT_AMD_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except Exception:       # ImportError, OSError (a missing .so), RuntimeError (version mismatch): the renderer does not need torch
            pass
    lib = C.CDLL(path)
    be = Backend(lib, "rt_")
    declare(lib, "rt_", SIGNATURES, allow_missing)
    return be
