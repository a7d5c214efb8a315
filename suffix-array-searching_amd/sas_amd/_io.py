"""Which side a call is on, written once ("One host/device call path in the Python
binding"): the C ABI takes host or device pointers by a flag, and every wrapper has to pick the
stream, the flags and the array library to match.

    Side(lead, stream, u32)   built once per call from its leading array: host (numpy) or device
                              (torch CUDA), the stream and the flags to pass, and how to allocate an
                              output of a given kind there (HOST: the one for host-only calls)
    queries(...)              the (qbytes, qoff, qlen) / (qbytes, m) preamble of every query call
    sized(...)                the sized-output protocol of the locate family
    check_out(...)            the out / capacity validation of its device side

torch is imported only when a CUDA tensor comes in.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import errno

import numpy as np

from . import _lib
from ._lib import check

# output kind -> (numpy dtype, torch dtype: torch has no unsigned 16/32/64-bit tensors, so the
# device side carries the same bits in the signed type of that width)
KINDS = {"u64": (np.uint64, "int64"), "u32": (np.uint32, "int32"), "u16": (np.uint16, "int16"),
         "u8": (np.uint8, "uint8")}


_torch = None  # the module, once a CUDA tensor has come in


def is_cuda(x) -> bool:
    return bool(getattr(x, "is_cuda", False))


def ptr(x):
    if x is None:
        return None
    return x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data


def as_u8(x):
    if is_cuda(x):
        return x
    return np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, np.uint8)


class Side:
    """dev: device pointers; device: the tensors' device (None on the host); stream: the caller's,
    else the current stream of that device, else (host) None; u32: positions are 32-bit; keep: the
    arrays the call's pointers point into (set by queries)."""
    __slots__ = ("dev", "device", "stream", "u32", "flags", "keep")

    def __init__(self, lead, stream=None, u32: bool = False):
        global _torch
        self.u32 = u32
        # the flags to OR into the call's: 32-bit positions, device pointers
        self.flags = _lib.SAS_LOCATE_U32 if u32 else 0
        if getattr(lead, "is_cuda", False):
            if _torch is None:
                import torch
                _torch = torch
            self.dev, self.device = True, lead.device
            self.flags |= _lib.SAS_DEVICE_PTRS
            self.stream = stream if stream is not None else _torch.cuda.current_stream(self.device).cuda_stream
        else:
            self.dev, self.device, self.stream = False, None, stream

    def dtype(self, kind: str):
        """The dtype of an output kind on this side; "pos" is a text position (u32 or u64)."""
        if kind == "pos":
            kind = "u32" if self.u32 else "u64"
        np_dt, torch_dt = KINDS[kind]
        return getattr(_torch, torch_dt) if self.dev else np_dt

    def new(self, kind: str | None, shape, fill=None):
        """An output of `shape` (a count, or a tuple whose first entry is the count); kind None: no
        output.  fill None: contents unspecified.  A host array is a [:count] view of max(count, 1)
        zeroed entries: its pointer is never null, and a count of 0 comes back with length 0."""
        if kind is None:
            return None
        shape = tuple(shape) if isinstance(shape, tuple) else (int(shape),)
        if self.dev:
            if fill is None:
                return _torch.empty(shape, dtype=self.dtype(kind), device=self.device)
            return _torch.full(shape, fill, dtype=self.dtype(kind), device=self.device)
        room = (max(shape[0], 1),) + shape[1:]
        a = np.zeros(room, self.dtype(kind)) if not fill else np.full(room, fill, self.dtype(kind))
        return a[:shape[0]]

    def guard(self):
        """A context in which the tensors' device is the current one, for a call that takes no index
        (the library then works on the current device); nothing on the host."""
        return _torch.cuda.device(self.device) if self.dev else contextlib.nullcontext()

    def count(self, x) -> int:
        return int(x.numel() if self.dev else len(x))


HOST = Side(None)  # host-only calls allocate through it too


def queries(qbytes, qoff, qlen, m, stream=None, u32: bool = False, what: str = "search_batch", pairs: bool = False):
    """The preamble of a query call -> (side, nq, lead, suffix): ragged queries (qoff given) or
    fixed-length ones (qoff None; m <= 0 raises ValueError naming the ragged call `what`).  `lead`
    holds the call's leading C arguments, (qbytes, qoff, qlen, count) or (qbytes, m, count), and
    `suffix` ("" or "_fixed") picks the entry point.  pairs: the reads come in interleaved pairs,
    count is the number of pairs, and an odd nq raises ValueError."""
    side = Side(qbytes, stream, u32)
    if not side.dev:
        qbytes = as_u8(qbytes)
    if qoff is None:
        if m <= 0:
            raise ValueError(f"use {what} for empty queries")
        nq = (qbytes.numel() if side.dev else len(qbytes)) // m
    else:
        if not side.dev:
            qoff, qlen = np.ascontiguousarray(qoff, np.uint64), np.ascontiguousarray(qlen, np.uint32)
        nq = int(qoff.numel() if side.dev else len(qoff))
    if pairs and nq % 2:
        raise ValueError(f"paired reads come interleaved, mate 1 then mate 2: {nq} reads is an odd number")
    side.keep = (qbytes, qoff, qlen)
    count = nq // 2 if pairs else nq
    if qoff is None:
        return side, nq, (ptr(qbytes), m, count), "_fixed"
    return side, nq, (ptr(qbytes), ptr(qoff), ptr(qlen), count), ""


def check_out(side: Side, what: str, out, capacity):
    """A device call's position buffer -> (out, capacity): a new one of max(capacity, 1) entries,
    or the caller's `out` (a contiguous CUDA tensor of the position dtype, of at least `capacity`
    entries; capacity None: all of it)."""
    if out is None:
        out = side.new("pos", max(int(capacity), 1))
    elif not is_cuda(out) or out.dtype != side.dtype("pos") or not out.is_contiguous():
        raise ValueError(f"{what}: out must be a contiguous CUDA {side.dtype('pos')} tensor")
    capacity = out.numel() if capacity is None else capacity
    if capacity > out.numel():
        raise ValueError(f"{what}: capacity exceeds out")
    return out, capacity


def sized(side: Side, what: str, call, off, nq: int, kinds=("pos",), out=None, capacity=None, sizing: bool = True):
    """The sized-output protocol -> (bufs, total).  call(bufs, capacity, total) makes the C call that
    fills `off` (nq + 1 entries) and, up to `capacity`, the buffers of `kinds` (the first one the
    positions; a kind None is no buffer); `total` is a byref for the host's count, None on the device.
    Host: a sizing call with capacity 0 (ENOSPC unless nothing occurs), buffers of the total, the
    real call.  Device with out / capacity: one call into buffers of that capacity, returned whole
    (total None), nothing synchronises.  Device without: the sizing call (unless sizing=False: `off`
    is already filled), one off[nq].item(), and the real call, skipped after a sizing call that
    found nothing; the buffers come back cut to the total."""
    none = [None] * len(kinds)
    if not side.dev:
        total = C.c_uint64(0)
        rc = call(none, 0, C.byref(total))
        if rc not in (0, errno.ENOSPC):
            check(rc)
        bufs = [side.new(k, total.value) for k in kinds]
        if total.value:
            check(call(bufs, total.value, C.byref(total)))
        return bufs, total.value
    total = None
    if out is None and capacity is None:
        if sizing:
            check(call(none, 0, None))
        capacity = total = int(off[nq].item())
    out, capacity = check_out(side, what, out, capacity)
    bufs = [out] + [side.new(k, max(int(capacity), 1)) for k in kinds[1:]]
    if not (sizing and total == 0):
        check(call(bufs, capacity, None))
    if total is not None:
        bufs = [b if b is None else b[:total] for b in bufs]
    return bufs, total
