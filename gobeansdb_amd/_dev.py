"""What the drivers above the C ABI repeat: host values as device tensors of the ABI's integer
widths, the small read-backs, nullable pointers and the stream convention.

torch has no unsigned 32/64-bit arithmetic worth using, so the ABI's u64 / u32 arrays travel as
int64 / int32 tensors holding the same bits.
"""
from __future__ import annotations

import functools
import inspect

import numpy as np
import torch


def _bits(v, dev, np_dtype, dtype) -> torch.Tensor:
    if isinstance(v, torch.Tensor):
        return v.to(device=dev, dtype=dtype).contiguous()
    if not isinstance(v, np.ndarray):   # Python ints, exactly: up to 2^64 - 1, or negative ones of 32 bits
        v = np.asarray(v, dtype=np.uint64 if np_dtype is np.uint64 else np.int64)
    a = np.ascontiguousarray(v.astype(np_dtype, copy=False))   # astype wraps, as a C cast does
    return torch.from_numpy(a.view(f"i{a.itemsize}")).to(dev)


def u64(v, dev) -> torch.Tensor:
    """A sequence, ndarray or tensor as a contiguous tensor of u64 bits (int64) on `dev`."""
    return _bits(v, dev, np.uint64, torch.int64)


def u32(v, dev) -> torch.Tensor:
    """A sequence, ndarray or tensor as a contiguous tensor of u32 bits (int32) on `dev`."""
    return _bits(v, dev, np.uint32, torch.int32)


def i32(v, dev) -> torch.Tensor:
    """A sequence, ndarray or tensor as a contiguous int32 tensor on `dev` (values from 2^31 to
    2^32 - 1 keep their bits, as in u32)."""
    return _bits(v, dev, np.int32, torch.int32)


def wide(t, lo: int) -> int:
    """The 64-bit total whose halves are t[lo] (low) and t[lo + 1] (high): every lo/hi pair of
    the ABI's totals is adjacent."""
    return int(t[lo]) | int(t[lo + 1]) << 32


def readback(totals: torch.Tensor) -> np.ndarray:
    """A small device tensor of totals on the host, as u32 (one device-to-host copy)."""
    return totals.cpu().numpy().view(np.uint32)


def ptr(t: torch.Tensor | None) -> int | None:
    """The tensor's address for the C ABI; a null pointer for None and for an empty tensor."""
    return None if t is None or t.numel() == 0 else t.data_ptr()


def on_stream(fn):
    """For a function with a `stream=None` parameter: run it with `stream` as torch's current
    stream, so that its allocations, uploads, launches and read-backs are all on that stream.
    The body sees stream=None and launches on the current stream (batch._stream())."""
    at = list(inspect.signature(fn).parameters).index("stream")

    @functools.wraps(fn)
    def call(*args, **kw):
        if len(args) > at:
            stream, args = args[at], args[:at] + (None,) + args[at + 1:]
        else:
            stream = kw.pop("stream", None)
        if stream is None:
            return fn(*args, **kw)
        with torch.cuda.stream(stream):
            return fn(*args, **kw)
    return call
