"""Loader of libmtts_hip.so (C ABI: include/*.h, mirrored in matcha/_abi.py): lib() binds every entry point.

The product path has no fallback: if the library is missing or was built without a symbol, every
op raises.  ``lib()`` loads lazily so that importing the package on a machine without a GPU (CI,
CPU tests) stays cheap; loading itself never touches the GPU.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

import torch

from matcha import _abi
from matcha._abi import (MTTS_MAS_MAX_TX, MTTS_MAS_MAX_TX_ROW_MAJOR, MTTS_MAS_NO_DENSE_PATH,  # noqa: F401
                         MTTS_MAS_VALUE_PREMASKED, MTTS_OK)

_PKG_ROOT = Path(__file__).resolve().parent.parent
LIB_PATH = Path(os.environ.get("MTTS_LIB", _PKG_ROOT / "lib" / "libmtts_hip.so"))

_SIGNATURES = _abi.SIGNATURES  # name -> (restype, argtypes): the whole ABI, bound by lib()
_lib = None


class NativeError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise NativeError(
                f"{LIB_PATH} not found: build it with `python {_PKG_ROOT / 'build_native.py'}` "
                "(hipcc --offload-arch=gfx950). There is no non-HIP fallback.")
        handle = ctypes.CDLL(str(LIB_PATH))
        for name, (restype, argtypes) in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = handle
    return _lib


def check(rc: int, what: str) -> None:
    if rc != MTTS_OK:
        msg = lib().mtts_last_error().decode(errors="replace")
        raise NativeError(f"{what} failed with status {rc}: {msg}")


def ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def stream_handle(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def require_device(*tensors: torch.Tensor) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise NativeError("the MI355X hot path takes device (cuda/hip) tensors only; "
                              f"got a tensor on {t.device}")
