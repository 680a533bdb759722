"""ctypes binding of the GPU stream-stream join (include/hstream_join.h)."""
import ctypes as C

import numpy as np

from . import abi
from .engine import load_library

_declared = False


def _lib():
    global _declared
    L = load_library()
    if not _declared:
        vp, P = C.c_void_p, C.POINTER
        L.hsg_join_create.argtypes = [vp, P(abi.hsg_join_config), P(vp)]
        L.hsg_join_create.restype = C.c_int
        L.hsg_join_destroy.argtypes = [vp]
        L.hsg_join_destroy.restype = None
        L.hsg_join_last_error.argtypes = [vp]
        L.hsg_join_last_error.restype = C.c_char_p
        L.hsg_join_push.argtypes = [vp, P(abi.hsg_join_batch)]
        L.hsg_join_push.restype = C.c_int
        L.hsg_join_pending.argtypes = [vp, P(C.c_uint64)]
        L.hsg_join_pending.restype = C.c_int
        L.hsg_join_drain.argtypes = [vp, P(abi.hsg_join_rows), P(C.c_uint64)]
        L.hsg_join_drain.restype = C.c_int
        L.hsg_join_state_rows.argtypes = [vp, P(C.c_uint64)]
        L.hsg_join_state_rows.restype = C.c_int
        _declared = True
    return L


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


# the output columns of hsg_join_rows: (field, numpy dtype, torch dtype name)
ROW_COLUMNS = (("this_handle", np.uint64, "int64"), ("other_handle", np.uint64, "int64"),
               ("join_key", np.uint32, "int32"), ("ts", np.int64, "int64"))
# bytes per element of the five batch arrays (side, key, join key, ts, handle)
_BATCH_ITEMSIZE = (1, 4, 4, 8, 8)


class Join:
    """joinStream over one engine: push poll batches of both streams, drain
    (this handle, other handle, join key, ts) rows."""

    def __init__(self, engine, before_ms, after_ms, batch_capacity=1 << 20):
        self._L = _lib()
        self._device = getattr(engine, "device", 0)
        cfg = abi.hsg_join_config(before_ms=before_ms, after_ms=after_ms, batch_capacity=batch_capacity)
        h = C.c_void_p()
        self._check(self._L.hsg_join_create(engine._h, C.byref(cfg), C.byref(h)), "hsg_join_create", None)
        self._h = h

    def _check(self, rc, what, h="self"):
        if rc != abi.HSG_OK:
            msg = ""
            if h is not None and getattr(self, "_h", None):
                msg = self.last_error()
            raise abi.HStreamGpuError(rc, f"{what}: {msg}")

    def last_error(self):
        return (self._L.hsg_join_last_error(self._h) or b"").decode()

    def push(self, side, key, join_key, ts, handle):
        """One poll batch, both streams interleaved in arrival order.

        Host: five array-likes (converted to uint8 / uint32 / uint32 / int64 /
        uint64). Device: five contiguous 1-d torch CUDA tensors of those widths
        (uint8; int32 holding the uint32 bits; int64; int64 holding the uint64
        bits), read in place (HSG_MEM_DEVICE). hsg_join_batch carries no ready
        event and the join runs on its own non-blocking stream: the caller
        synchronises the stream that produced the tensors before push. Host and
        device arrays in one batch raise ValueError."""
        arrs = (side, key, join_key, ts, handle)
        dev = [_is_torch(a) and a.is_cuda for a in arrs]
        if any(dev):
            if not all(dev):
                raise ValueError("Join.push: every array on the device or every array on the host")
            n = int(ts.shape[0])
            for a, size in zip(arrs, _BATCH_ITEMSIZE):
                if a.dim() != 1 or a.shape[0] != n or not a.is_contiguous() or a.element_size() != size or \
                        a.is_floating_point():
                    raise ValueError(f"Join.push: device arrays are contiguous 1-d integer tensors of {n} elements, "
                                     f"{_BATCH_ITEMSIZE} bytes each")
            mem, ptrs = abi.HSG_MEM_DEVICE, [a.data_ptr() for a in arrs]
        else:
            if any(_is_torch(a) for a in arrs):
                arrs = tuple(a.numpy() if _is_torch(a) else a for a in arrs)
            arrs = (np.ascontiguousarray(arrs[0], np.uint8), np.ascontiguousarray(arrs[1], np.uint32),
                    np.ascontiguousarray(arrs[2], np.uint32), np.ascontiguousarray(arrs[3], np.int64),
                    np.ascontiguousarray(arrs[4], np.uint64))
            n = len(arrs[3])
            if any(len(a) != n for a in arrs):
                raise ValueError("Join.push: arrays of different lengths")
            mem, ptrs = abi.HSG_MEM_HOST, [a.ctypes.data for a in arrs]
        b = abi.hsg_join_batch(n=n, mem=mem, side=ptrs[0], key_id=ptrs[1], join_key=ptrs[2], ts=ptrs[3],
                               handle=ptrs[4])
        self._check(self._L.hsg_join_push(self._h, C.byref(b)), "hsg_join_push")  # (arrs alive until here)

    def pending(self):
        """rows queued for the next drain"""
        n = C.c_uint64()
        self._check(self._L.hsg_join_pending(self._h, C.byref(n)), "hsg_join_pending")
        return n.value

    def drain_into(self, capacity, columns=("this_handle", "other_handle", "join_key", "ts"), device=False):
        """hsg_join_drain as it is: output arrays of `capacity` rows for the
        named columns (the others are passed as null pointers). Returns
        (status, n_out, {column: array}) and raises nothing."""
        out, ptrs = {}, {}
        for name, np_dt, torch_dt in ROW_COLUMNS:
            if name not in columns:
                continue
            if device:
                import torch
                out[name] = torch.empty(capacity, dtype=getattr(torch, torch_dt), device=f"cuda:{self._device}")
                ptrs[name] = out[name].data_ptr()
            else:
                out[name] = np.empty(capacity, np_dt)
                ptrs[name] = out[name].ctypes.data
        r = abi.hsg_join_rows(capacity=capacity, mem=abi.HSG_MEM_DEVICE if device else abi.HSG_MEM_HOST,
                              **{k: (v or None) for k, v in ptrs.items()})
        n = C.c_uint64()
        rc = self._L.hsg_join_drain(self._h, C.byref(r), C.byref(n))
        return rc, n.value, out

    def drain(self, device=False):
        """The queued rows as (this handle, other handle, join key, ts): numpy
        arrays, or with device=True torch CUDA tensors filled through
        HSG_MEM_DEVICE (int64 / int64 / int32 / int64 holding the same bits)."""
        rc, _, out = self.drain_into(self.pending(), device=device)
        self._check(rc, "hsg_join_drain")
        return tuple(out[name] for name, _, _ in ROW_COLUMNS)

    def state_rows(self):
        n = C.c_uint64()
        self._check(self._L.hsg_join_state_rows(self._h, C.byref(n)), "hsg_join_state_rows")
        return n.value

    def close(self):
        if self._h:
            self._L.hsg_join_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
