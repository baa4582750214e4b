"""What the thin ctypes callers of the device stages share (tests/handpaths.py, tests/test_gpu_hbv_handmade.py): host arrays uploaded as
they are, device memory of the context downloaded, and the look at a result struct after a refusal.  Nothing here needs a GPU until it is
called."""
from __future__ import annotations

import ctypes as C

import numpy as np


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype)).to(torch.device("cuda", 0))


def download(engine, ptr, count, dtype):
    host = np.zeros(max(count, 1), dtype)
    if count:
        engine._download(ptr, host.ctypes.data, count * host.itemsize)
    return host[:count].copy()


def _zeroed(out):
    return C.string_at(C.addressof(out), C.sizeof(out)) == bytes(C.sizeof(out))
