"""The two sides of an entry point that exists in two forms: numpy arrays in and out through a host-pointer entry point, or torch device tensors in and
out through the `_dev` one, queued on torch.cuda.current_stream.  A method picks HOST or device_side(dev) once and writes its body once over the four
operations both sides share: out (allocate an output), ptr (the pointer the library takes), put (a small host table onto the side), call."""
import ctypes as C

import numpy as np

from .. import _lib


def _is_device_tensor(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda") and x.is_cuda


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


_TORCH = None


def _torch():
    global _TORCH
    if _TORCH is None:
        import torch
        _TORCH = torch
    return _TORCH


def device_dtypes(torch):
    """numpy dtype string -> torch dtype.  A torch build without the unsigned 16 and 32-bit types gets the signed type of the same width: the same bits."""
    return {"u1": torch.uint8, "i2": torch.int16, "u2": getattr(torch, "uint16", torch.int16), "i4": torch.int32,
            "u4": getattr(torch, "uint32", torch.int32), "i8": torch.int64, "f4": torch.float32}


class _Host:
    ptr = staticmethod(_vp)

    def out(self, shape, kind, zero=False):
        return np.zeros(shape, kind)                  # calloc: as cheap as np.empty, and the library writes every output in full anyway

    def put(self, a):
        return a

    def call(self, fn_host, fn_dev, *args):
        _lib.check(fn_host(*args))


class _Device:
    _kinds = None

    def __init__(self, dev):
        torch = _torch()
        if _Device._kinds is None:
            # (int8: the obs / occ planes of evict and restore_bricks; float64: the poses and residuals of the pose graph)
            _Device._kinds = dict(device_dtypes(torch), i1=torch.int8, f8=torch.float64)
        self.dev, self._empty, self._zeros, self._stream = dev, torch.empty, torch.zeros, torch.cuda.current_stream

    @staticmethod
    def ptr(a):
        return None if a is None else a.data_ptr()

    def out(self, shape, kind, zero=False):
        return (self._zeros if zero else self._empty)(shape, dtype=self._kinds[kind], device=self.dev)

    def put(self, a):
        return _torch().from_numpy(a).to(self.dev)

    def call(self, fn_host, fn_dev, *args):
        _lib.check(fn_dev(*args, self._stream(self.dev).cuda_stream))


HOST = _Host()


def device_side(dev):
    """The side of a torch device: a torch.device, or the index of a map's device"""
    return _Device(dev if hasattr(dev, "type") else _torch().device(f"cuda:{dev}"))


def record_columns(rec, dtype):
    """An int32 [n, itemsize / 4] block of records as the named fields of the numpy structured dtype that describes one record: on the host copies out of
    the structured view, on the device views of the columns -- a 4-byte integer field is its column, "<f4" the column viewed as float32, "<i8" its two
    columns made contiguous and viewed as int64 [n]."""
    if isinstance(rec, np.ndarray):
        rows = rec.view(dtype).reshape(-1)
        return {k: rows[k].copy() for k in dtype.names}
    torch = _torch()
    out = {}
    for k in dtype.names:
        ft, off = dtype.fields[k][:2]
        c = off // 4
        if ft.itemsize == 8:
            out[k] = rec[:, c:c + 2].reshape(-1).view(torch.int64)        # the copy reshape makes is contiguous: [2 n] int32 -> [n] int64
        else:
            out[k] = rec[:, c].view(torch.float32) if ft.kind == "f" else rec[:, c]
    return out
