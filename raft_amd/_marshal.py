"""What both ctypes bindings (engine.py, hostio.py) do to every array they hand to a library or take back from one."""
from __future__ import annotations

import ctypes as C

import numpy as np


def carray(x, dtype=None) -> np.ndarray:
    """``x`` as a C-contiguous numpy array of ``dtype`` (None: its own): the object itself when it already is one."""
    return np.ascontiguousarray(np.asarray(x), dtype=dtype)


def count(x) -> int:
    """Elements of a numpy array or a torch tensor."""
    return int(x.size if isinstance(x, np.ndarray) else x.numel())


def ptr(x) -> C.c_void_p:
    """Where a numpy array or a torch tensor begins; NULL for None and for one without elements."""
    if x is None:
        return C.c_void_p(0)
    if isinstance(x, np.ndarray):
        return C.c_void_p(x.ctypes.data if x.size else 0)
    return C.c_void_p(x.data_ptr() if x.numel() else 0)


def address(x) -> int:
    """``ptr`` as a plain integer (a field of a ctypes structure), 0 for NULL."""
    return ptr(x).value or 0


def empty(n: int, dtype, pinned: bool = False) -> np.ndarray:
    """An uninitialised array of ``n`` elements, in page-locked memory when ``pinned`` (torch's allocator)."""
    if not pinned:
        return np.empty(n, dtype)
    import torch
    if dtype == np.uint16:      # (torch has no uint16 everywhere: page-locked bytes, viewed as uint16)
        return torch.empty(2 * int(n), dtype=torch.uint8, pin_memory=True).numpy().view(np.uint16)
    tdt = {np.int64: torch.int64, np.int32: torch.int32, np.uint8: torch.uint8}[dtype]
    return torch.empty(int(n), dtype=tdt, pin_memory=True).numpy()


def fit(have, n: int, dtype, pinned: bool = False) -> np.ndarray:
    """The first ``n`` elements of the caller's buffer when it fits (its dtype, at least n elements, contiguous), else a new
    array -- page-locked only when it has elements."""
    if have is not None and have.dtype == dtype and have.size >= n and have.flags["C_CONTIGUOUS"]:
        return have[:n]
    return empty(n, dtype, pinned and n > 0)
