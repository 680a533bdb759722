"""ctypes binding of the GPU stream-stream join (include/hstream_join.h)."""
import collections
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
        L.hsg_join_create_valued.argtypes = [vp, P(abi.hsg_join_config), P(abi.hsg_join_values), P(vp)]
        L.hsg_join_create_valued.restype = C.c_int
        L.hsg_join_push_valued.argtypes = [vp, P(abi.hsg_join_batch), P(abi.hsg_join_cols)]
        L.hsg_join_push_valued.restype = C.c_int
        L.hsg_join_drain_batch.argtypes = [vp, P(abi.hsg_join_joined), P(C.c_uint64)]
        L.hsg_join_drain_batch.restype = C.c_int
        L.hsg_join_value_rows.argtypes = [vp, P(C.c_uint64), P(C.c_uint64)]
        L.hsg_join_value_rows.restype = C.c_int
        L.hsg_join_value_stride.argtypes = [C.c_int32, C.c_int32]
        L.hsg_join_value_stride.restype = C.c_uint64
        _declared = True
    return L


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


# the output columns of hsg_join_rows: (field, numpy dtype, torch dtype name)
ROW_COLUMNS = (("this_handle", np.uint64, "int64"), ("other_handle", np.uint64, "int64"),
               ("join_key", np.uint32, "int32"), ("ts", np.int64, "int64"))
# bytes per element of the five batch arrays (side, key, join key, ts, handle)
_BATCH_ITEMSIZE = (1, 4, 4, 8, 8)


# one drained batch of joined rows (Join.drain_batch): key_id, ts, cols, valid
# are GpuOp.push's arguments; the optional arrays are None when not asked for
JoinedBatch = collections.namedtuple("JoinedBatch", "key_id ts cols valid this_handle other_handle join_key")
# hsg_join_joined's optional arrays
JOINED_OPTIONAL = ("valid", "this_handle", "other_handle", "join_key")


def value_stride(c0, c1):
    """hsg_join_value_stride, from the library."""
    return int(_lib().hsg_join_value_stride(c0, c1))


class Join:
    """joinStream over one engine: push poll batches of both streams, drain
    (this handle, other handle, join key, ts) rows.

    cols = (types of this side's columns, types of the other side's), each a
    sequence of abi.HSG_I64 / abi.HSG_F64, makes a valued join
    (hsg_join_create_valued): push takes the records' value columns, the join
    keeps them in HBM, and drain_batch returns the joined rows (this side's
    columns, then the other side's) as the arrays of an op's batch."""

    def __init__(self, engine, before_ms, after_ms, batch_capacity=1 << 20, cols=None):
        self._L = _lib()
        self._device = getattr(engine, "device", 0)
        cfg = abi.hsg_join_config(before_ms=before_ms, after_ms=after_ms, batch_capacity=batch_capacity)
        h = C.c_void_p()
        self.col_types = None
        if cols is None:
            self._check(self._L.hsg_join_create(engine._h, C.byref(cfg), C.byref(h)), "hsg_join_create", None)
        else:
            t0, t1 = [int(t) for t in cols[0]], [int(t) for t in cols[1]]
            vals = abi.hsg_join_values()
            vals.n_cols[0], vals.n_cols[1] = len(t0), len(t1)
            for sd, ts_ in enumerate((t0, t1)):
                for c, t in enumerate(ts_[:8]):
                    vals.col_types[sd][c] = t
            self._check(self._L.hsg_join_create_valued(engine._h, C.byref(cfg), C.byref(vals), C.byref(h)),
                        "hsg_join_create_valued", None)
            self.col_types = (t0, t1)
        self._h = h

    def _check(self, rc, what, h="self"):
        if rc != abi.HSG_OK:
            msg = ""
            if h is not None and getattr(self, "_h", None):
                msg = self.last_error()
            raise abi.HStreamGpuError(rc, f"{what}: {msg}")

    def last_error(self):
        return (self._L.hsg_join_last_error(self._h) or b"").decode()

    def push(self, side, key, join_key, ts, handle=None, cols=None, valid=None):
        """One poll batch, both streams interleaved in arrival order.

        A valued join takes cols (max of the two sides' column counts arrays of
        int64 / float64, record i reading the first n_cols[side[i]]) and
        optionally valid (uint8 arrays or None entries: all present) in place
        of handle, which it ignores: a record's handle is its value row, the
        number of records pushed before it. Arrays in the batch's memory.

        Host: five array-likes (converted to uint8 / uint32 / uint32 / int64 /
        uint64). Device: five contiguous 1-d torch CUDA tensors of those widths
        (uint8; int32 holding the uint32 bits; int64; int64 holding the uint64
        bits), read in place (HSG_MEM_DEVICE). hsg_join_batch carries no ready
        event and the join runs on its own non-blocking stream: the caller
        synchronises the stream that produced the tensors before push. Host and
        device arrays in one batch raise ValueError."""
        if self.col_types is not None:
            return self._push_valued(side, key, join_key, ts, cols or (), valid)
        if cols is not None or valid is not None or handle is None:
            raise ValueError("Join.push: a plain join takes handles, not columns")
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

    def _push_valued(self, side, key, join_key, ts, cols, valid):
        vc = max(len(self.col_types[0]), len(self.col_types[1]))
        cols = list(cols)
        valid = [None] * vc if valid is None else list(valid)
        if len(cols) != vc or len(valid) != vc:
            raise ValueError(f"Join.push: a batch of this join carries {vc} columns")
        arrs = (side, key, join_key, ts)
        every = list(arrs) + cols + [v for v in valid if v is not None]
        dev = [_is_torch(a) and a.is_cuda for a in every]
        if any(dev):
            if not all(dev):
                raise ValueError("Join.push: every array on the device or every array on the host")
            n = int(ts.shape[0])
            sizes = list(_BATCH_ITEMSIZE[:4]) + [8] * vc + [1] * (len(every) - 4 - vc)
            for a, size in zip(every, sizes):
                if a.dim() != 1 or a.shape[0] != n or not a.is_contiguous() or a.element_size() != size:
                    raise ValueError(f"Join.push: device arrays are contiguous 1-d tensors of {n} elements")
            mem, ptr = abi.HSG_MEM_DEVICE, (lambda a: a.data_ptr())
        else:
            tonp = lambda a: a.numpy() if _is_torch(a) else a
            arrs = (np.ascontiguousarray(tonp(side), np.uint8), np.ascontiguousarray(tonp(key), np.uint32),
                    np.ascontiguousarray(tonp(join_key), np.uint32), np.ascontiguousarray(tonp(ts), np.int64))
            n = len(arrs[3])
            cols = [np.ascontiguousarray(tonp(c)) for c in cols]
            valid = [None if v is None else np.ascontiguousarray(tonp(v), np.uint8) for v in valid]
            for c in cols:
                if c.dtype.itemsize != 8:
                    raise ValueError("Join.push: value columns are int64 or float64")
            if any(len(a) != n for a in list(arrs) + cols + [v for v in valid if v is not None]):
                raise ValueError("Join.push: arrays of different lengths")
            mem, ptr = abi.HSG_MEM_HOST, (lambda a: a.ctypes.data)
        cp = (C.c_void_p * max(1, vc))(*[ptr(c) for c in cols])
        vp = (C.c_void_p * max(1, vc))(*[None if v is None else ptr(v) for v in valid])
        b = abi.hsg_join_batch(n=n, mem=mem, side=ptr(arrs[0]), key_id=ptr(arrs[1]), join_key=ptr(arrs[2]),
                               ts=ptr(arrs[3]), handle=None)
        jc = abi.hsg_join_cols(cols=C.cast(cp, C.POINTER(C.c_void_p)), valid=C.cast(vp, C.POINTER(C.c_void_p)))
        self._check(self._L.hsg_join_push_valued(self._h, C.byref(b), C.byref(jc)), "hsg_join_push_valued")

    def drain_batch_into(self, capacity, key_col=-1, device=False, optional=JOINED_OPTIONAL):
        """hsg_join_drain_batch as it is: output arrays of `capacity` rows, the
        optional ones (JOINED_OPTIONAL) only when named. Returns (status, n_out,
        JoinedBatch) and raises nothing."""
        t0, t1 = self.col_types if self.col_types is not None else ((), ())
        types = list(t0) + list(t1)
        if device:
            import torch
            dv = f"cuda:{self._device}"
            new = lambda dt: torch.empty(capacity, dtype=getattr(torch, dt), device=dv)
            ptr = lambda a: a.data_ptr()
            names = {"u64": "int64", "u32": "int32", "i64": "int64", "f64": "float64", "u8": "uint8"}
        else:
            new = lambda dt: np.empty(capacity, dt)
            ptr = lambda a: a.ctypes.data
            names = {"u64": np.uint64, "u32": np.uint32, "i64": np.int64, "f64": np.float64, "u8": np.uint8}
        cols = [new(names["f64" if t == abi.HSG_F64 else "i64"]) for t in types]
        valid = [new(names["u8"]) for _ in types] if "valid" in optional else None
        opt = {k: (new(names[dt]) if k in optional else None)
               for k, dt in (("this_handle", "u64"), ("other_handle", "u64"), ("join_key", "u32"))}
        key_id, ts = new(names["u32"]), new(names["i64"])
        cp = (C.c_void_p * max(1, len(types)))(*[ptr(c) for c in cols])
        vp = (C.c_void_p * max(1, len(types)))(*[ptr(v) for v in valid]) if valid is not None else None
        o = abi.hsg_join_joined(capacity=capacity, mem=abi.HSG_MEM_DEVICE if device else abi.HSG_MEM_HOST,
                                key_col=key_col, key_id=ptr(key_id), ts=ptr(ts),
                                cols=C.cast(cp, C.POINTER(C.c_void_p)),
                                valid=C.cast(vp, C.POINTER(C.c_void_p)) if vp is not None else None,
                                **{k: (None if v is None else ptr(v)) for k, v in opt.items()})
        n = C.c_uint64()
        rc = self._L.hsg_join_drain_batch(self._h, C.byref(o), C.byref(n))
        return rc, n.value, JoinedBatch(key_id, ts, cols, valid, opt["this_handle"], opt["other_handle"],
                                        opt["join_key"])

    def drain_batch(self, key_col=-1, device=False, optional=("valid",)):
        """The queued rows joined (hsg_join_drain_batch): a JoinedBatch whose
        key_id, ts, cols, valid go straight into GpuOp.push. cols holds this
        side's columns, then the other side's; key_id is the join key
        (key_col=-1) or joined i64 column key_col as a dictionary id. numpy
        arrays, or with device=True torch CUDA tensors, complete on return."""
        rc, _, out = self.drain_batch_into(self.pending(), key_col, device, optional)
        self._check(rc, "hsg_join_drain_batch")
        return out

    def value_rows(self):
        """(value rows in use, value rows allocated) of a valued join"""
        u, c = C.c_uint64(), C.c_uint64()
        self._check(self._L.hsg_join_value_rows(self._h, C.byref(u), C.byref(c)), "hsg_join_value_rows")
        return u.value, c.value

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
