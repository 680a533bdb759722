"""ctypes binding of libhstream_gpu (the product path).

Loads the in-tree ``hstream_amd/libhstream_gpu.so``; there is no fallback of
any kind: if the library is missing or the GPU is absent, constructing an
Engine raises.
"""
import ctypes as C
import os

import numpy as np

from . import abi
from .columnar import OpHandle, OpSpec, Rows, _is_torch, alloc_rows, declare_op_functions, truncate

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libhstream_gpu.so")
# diagnostics only: HSG_LIB_PATH names another build of the same library
# (e.g. the PHASES=1 phase-clock build, tools/phases.sh)
LIB_PATH = os.environ.get("HSG_LIB_PATH", LIB_PATH)
_lib = None


def load_library(path=LIB_PATH):
    """Load libhstream_gpu.so and declare every exported signature."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(
            f"libhstream_gpu.so not found at {path}: run __graft_entry__.build() "
            "(the GPU path has no fallback)")
    L = C.CDLL(path)
    vp = C.c_void_p
    P = C.POINTER
    L.hsg_comm_unique_id.argtypes = [P(C.c_uint8), C.c_size_t]
    L.hsg_comm_unique_id.restype = C.c_int
    L.hsg_engine_create.argtypes = [P(abi.hsg_engine_config), P(vp)]
    L.hsg_engine_create.restype = C.c_int
    L.hsg_engine_destroy.argtypes = [vp]
    L.hsg_engine_destroy.restype = None
    L.hsg_engine_last_error.argtypes = [vp]
    L.hsg_engine_last_error.restype = C.c_char_p
    L.hsg_op_create.argtypes = [vp, P(abi.hsg_op_config), P(vp)]
    L.hsg_op_create.restype = C.c_int
    L.hsg_where_check.argtypes = [P(abi.hsg_where_ins), C.c_int32, P(C.c_int32), C.c_int32, C.c_char_p, C.c_size_t]
    L.hsg_where_check.restype = C.c_int
    L.hsg_op_create_where.argtypes = [vp, P(abi.hsg_op_config), P(abi.hsg_where_ins), C.c_int32, P(vp)]
    L.hsg_op_create_where.restype = C.c_int
    L.hsg_having_check.argtypes = [P(abi.hsg_where_ins), C.c_int32, P(abi.hsg_op_config), C.c_char_p, C.c_size_t]
    L.hsg_having_check.restype = C.c_int
    L.hsg_op_create_filtered.argtypes = [vp, P(abi.hsg_op_config), P(abi.hsg_where_ins), C.c_int32,
                                         P(abi.hsg_where_ins), C.c_int32, P(vp)]
    L.hsg_op_create_filtered.restype = C.c_int
    L.hsg_map_check.argtypes = [P(abi.hsg_map_expr), C.c_int32, P(C.c_int32), C.c_int32, P(C.c_int32), C.c_char_p,
                                C.c_size_t]
    L.hsg_map_check.restype = C.c_int
    L.hsg_op_create_mapped.argtypes = [vp, P(abi.hsg_op_config), P(abi.hsg_map_expr), C.c_int32,
                                       P(abi.hsg_where_ins), C.c_int32, P(abi.hsg_where_ins), C.c_int32, P(vp)]
    L.hsg_op_create_mapped.restype = C.c_int
    L.hsg_op_map_stats.argtypes = [vp, P(abi.hsg_map_stats)]
    L.hsg_op_map_stats.restype = C.c_int
    L.hsg_map_grid_threads.argtypes = []
    L.hsg_map_grid_threads.restype = C.c_int
    L.hsg_map_grid_threads_fn.argtypes = [C.c_int]
    L.hsg_map_grid_threads_fn.restype = C.c_int
    L.hsg_select_check.argtypes = [P(abi.hsg_where_ins), C.c_int32, P(abi.hsg_map_expr), C.c_int32,
                                   P(abi.hsg_where_ins), C.c_int32, P(C.c_int32), C.c_int32, C.c_char_p, C.c_size_t]
    L.hsg_select_check.restype = C.c_int
    L.hsg_op_create_select.argtypes = [vp, P(abi.hsg_select_config), P(abi.hsg_where_ins), C.c_int32,
                                       P(abi.hsg_map_expr), C.c_int32, P(abi.hsg_where_ins), C.c_int32, P(vp)]
    L.hsg_op_create_select.restype = C.c_int
    L.hsg_op_select_stats.argtypes = [vp, P(abi.hsg_select_stats)]
    L.hsg_op_select_stats.restype = C.c_int
    L.hsg_select_tile_rows.argtypes = []
    L.hsg_select_tile_rows.restype = C.c_int
    L.hsg_select_grid_groups.argtypes = []
    L.hsg_select_grid_groups.restype = C.c_int
    L.hsg_prog_fn_class.argtypes = [P(abi.hsg_where_ins), C.c_int32]
    L.hsg_prog_fn_class.restype = C.c_int
    L.hsg_having_tile_rows.argtypes = []
    L.hsg_having_tile_rows.restype = C.c_int
    L.hsg_op_stats.argtypes = [vp, P(abi.hsg_stats)]
    L.hsg_op_stats.restype = C.c_int
    L.hsg_op_set_changelog.argtypes = [vp, P(abi.hsg_rows)]
    L.hsg_op_set_changelog.restype = C.c_int
    L.hsg_push_batch_async.argtypes = [vp, P(abi.hsg_batch), P(C.c_int64), abi.HSG_DONE_FN, vp]
    L.hsg_push_batch_async.restype = C.c_int
    L.hsg_op_wait.argtypes = [vp]
    L.hsg_op_wait.restype = C.c_int
    L.hsg_view_get.argtypes = [vp, vp, C.c_uint32, P(abi.hsg_rows), P(C.c_uint64)]
    L.hsg_view_get.restype = C.c_int
    L.hsg_table_join.argtypes = [vp, P(abi.hsg_probe), P(abi.hsg_rows), P(C.c_uint64)]
    L.hsg_table_join.restype = C.c_int
    L.hsg_table_join_tile.argtypes = []
    L.hsg_table_join_tile.restype = C.c_int
    L.hsg_testing_set_knob.argtypes = [C.c_int32, C.c_int64]
    L.hsg_testing_set_knob.restype = C.c_int
    declare_op_functions(L, "hsg")
    _lib = L
    return L


class testing_knob:
    """Context manager over hsg_testing_set_knob (tests only): the knob holds
    for ops created inside the block, then returns to its default."""

    DEFAULTS = {abi.HSG_KNOB_XPART_LOG2: -1, abi.HSG_KNOB_SESS_ARENA_MIN: 0, abi.HSG_KNOB_X_CLASSIC: 0}

    def __init__(self, knob, value):
        self.knob, self.value = knob, value

    def __enter__(self):
        rc = load_library().hsg_testing_set_knob(self.knob, self.value)
        if rc != abi.HSG_OK:
            raise abi.HStreamGpuError(rc, "hsg_testing_set_knob")
        return self

    def __exit__(self, *exc):
        load_library().hsg_testing_set_knob(self.knob, self.DEFAULTS[self.knob])
        return False


def where_check(program, col_types):
    """hsg_where_check (host only, no GPU): (status, message) for a WHERE
    program over value columns of the given types."""
    L = load_library()
    prog, n = abi.where_array(program)
    types = (C.c_int32 * max(1, len(col_types)))(*col_types)
    buf = C.create_string_buffer(256)
    rc = L.hsg_where_check(prog, n, types, len(col_types), buf, len(buf))
    return rc, buf.value.decode()


def having_check(program, spec: OpSpec):
    """hsg_having_check (host only, no GPU): (status, message) for a HAVING
    program over the aggregate outputs of the op `spec` describes."""
    L = load_library()
    prog, n = abi.where_array(program)
    cfg, keep = spec.to_config()
    buf = C.create_string_buffer(256)
    rc = L.hsg_having_check(prog, n, C.byref(cfg), buf, len(buf))
    return rc, buf.value.decode()


def map_check(exprs, col_types):
    """hsg_map_check (host only, no GPU): (status, message, out_types) for a
    map -- abi.MapExpr, or bare programs -- over value columns of the given
    types."""
    L = load_library()
    arr, n, keep = abi.map_array(exprs)
    types = (C.c_int32 * max(1, len(col_types)))(*col_types)
    out = (C.c_int32 * max(1, n))()
    buf = C.create_string_buffer(256)
    rc = L.hsg_map_check(arr, n, types, len(col_types), out, buf, len(buf))
    return rc, buf.value.decode(), list(out)[:n] if rc == abi.HSG_OK else None


def select_check(col_types, exprs=(), where=None, having=None):
    """hsg_select_check (host only, no GPU): (status, message) for the three
    programs of a select op over value columns of the given types; where /
    having None = none, exprs may be empty (SELECT *)."""
    L = load_library()
    wprog, wn = abi.where_array(where) if where is not None else (None, 0)
    hprog, hn = abi.where_array(having) if having is not None else (None, 0)
    arr, n, keep = abi.map_array(exprs)
    types = (C.c_int32 * max(1, len(col_types)))(*col_types)
    buf = C.create_string_buffer(256)
    rc = L.hsg_select_check(wprog, wn, arr, n, hprog, hn, types, len(col_types), buf, len(buf))
    return rc, buf.value.decode()


def select_tile_rows() -> int:
    """Records per tile of the select kernel (hsg_select_tile_rows)."""
    return load_library().hsg_select_tile_rows()


def select_grid_groups() -> int:
    """Most workgroups one launch of the select kernel starts (hsg_select_grid_groups)."""
    return load_library().hsg_select_grid_groups()


def map_grid_threads() -> int:
    """Threads of one resident round of the map pass's grid (hsg_map_grid_threads)."""
    return load_library().hsg_map_grid_threads()


def map_grid_threads_fn(fn_class: int) -> int:
    """hsg_map_grid_threads of the map kernel of a function class (hsg_map_grid_threads_fn)."""
    return load_library().hsg_map_grid_threads_fn(fn_class)


def prog_fn_class(program) -> int:
    """hsg_prog_fn_class (host only, no GPU): 0 no function, 1 the exact
    family only, 2 any other function."""
    prog, n = abi.where_array(program)
    return load_library().hsg_prog_fn_class(prog, n)


def having_tile_rows() -> int:
    """Rows of one compaction tile of the HAVING pass (hsg_having_tile_rows)."""
    return load_library().hsg_having_tile_rows()


def table_join_tile() -> int:
    """Records per compaction tile of the stream-table join (hsg_table_join_tile)."""
    return load_library().hsg_table_join_tile()


def make_probe(key_ids, mem=None, ready_event=None):
    """An hsg_probe over a numpy array (host) or a torch tensor (device) of
    key ids in arrival order. Returns (hsg_probe, keepalive)."""
    if _is_torch(key_ids):
        keys = key_ids.contiguous()
        if mem is None:
            mem = abi.HSG_MEM_DEVICE if keys.is_cuda else abi.HSG_MEM_HOST
        n, ptr = int(keys.numel()), keys.data_ptr()
    else:
        keys = np.ascontiguousarray(np.asarray(key_ids, dtype=np.uint32).ravel())
        if mem is None:
            mem = abi.HSG_MEM_HOST
        n, ptr = int(keys.size), keys.ctypes.data
    return abi.hsg_probe(n=n, mem=mem, reserved=0, key_id=ptr if n else None, ready_event=ready_event), keys


def comm_unique_id() -> bytes:
    L = load_library()
    buf = (C.c_uint8 * abi.HSG_COMM_ID_BYTES)()
    rc = L.hsg_comm_unique_id(buf, abi.HSG_COMM_ID_BYTES)
    if rc != abi.HSG_OK:
        raise abi.HStreamGpuError(rc, "hsg_comm_unique_id")
    return bytes(buf)


class Engine:
    """One per process and GPU (hsg_engine_create)."""

    def __init__(self, device=0, rank=0, nranks=1, comm_id=None, batch_capacity=1 << 24,
                 transport=abi.HSG_TRANSPORT_RCCL):
        """comm_id: RCCL id bytes (comm_unique_id() on rank 0) or, with
        transport=HSG_TRANSPORT_HOST, a segment name (str / bytes) shared by
        the ranks of one host."""
        L = load_library()
        self._lib = L
        self._id_buf = None
        cfg = abi.hsg_engine_config(device=device, rank=rank, nranks=nranks, transport=transport,
                                    comm_id=None, batch_capacity=batch_capacity)
        if isinstance(comm_id, str):
            comm_id = comm_id.encode()
        if comm_id is not None and transport == abi.HSG_TRANSPORT_HOST:
            comm_id = comm_id[: abi.HSG_COMM_ID_BYTES - 1].ljust(abi.HSG_COMM_ID_BYTES, b"\0")
        if comm_id is not None:
            self._id_buf = (C.c_uint8 * abi.HSG_COMM_ID_BYTES)(*comm_id[: abi.HSG_COMM_ID_BYTES])
            cfg.comm_id = C.cast(self._id_buf, P_u8)
        h = C.c_void_p()
        rc = L.hsg_engine_create(C.byref(cfg), C.byref(h))
        if rc != abi.HSG_OK:
            raise abi.HStreamGpuError(rc, "hsg_engine_create")
        self._h = h
        self.device, self.rank, self.nranks, self.batch_capacity = device, rank, nranks, batch_capacity

    def op(self, spec: OpSpec) -> "GpuOp":
        return GpuOp(self, spec)

    def select_op(self, col_types, exprs=(), where=None, having=None, out_capacity=0, flags=0) -> "GpuOp":
        """hsg_op_create_select: the op without a group key. exprs are value
        programs (abi.MapExpr or bare programs; none = SELECT *, the rows carry
        src_index only), where / having programs or None. The rows' aggs[j] is
        expression j."""
        spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=list(col_types),
                      aggs=[(abi.HSG_LAST, j) for j in range(len(exprs))], out_capacity=out_capacity, flags=flags,
                      where=where, having=having, map=list(exprs))
        return GpuOp(self, spec, select=True)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.hsg_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


P_u8 = C.POINTER(C.c_uint8)


class GpuOp(OpHandle):
    """One windowed GROUP BY operator on the GPU (hsg_op_create)."""

    def __init__(self, engine: Engine, spec: OpSpec, select=False):
        cfg, keep = spec.to_config()
        h = C.c_void_p()
        what = "hsg_op_create"
        if select:
            what = "hsg_op_create_select"
            scfg = abi.hsg_select_config(n_cols=cfg.n_cols, flags=spec.flags, col_types=cfg.col_types,
                                         out_capacity=spec.out_capacity)
            marr, mn, mkeep = abi.map_array(spec.map or ())
            wprog, wn = abi.where_array(spec.where) if spec.where is not None else (None, 0)
            hprog, hn = abi.where_array(spec.having) if spec.having is not None else (None, 0)
            rc = engine._lib.hsg_op_create_select(engine._h, C.byref(scfg), wprog, wn, marr, mn, hprog, hn, C.byref(h))
        elif spec.map:
            what = "hsg_op_create_mapped"
            marr, mn, mkeep = abi.map_array(spec.map)
            wprog, wn = abi.where_array(spec.where) if spec.where is not None else (None, 0)
            hprog, hn = abi.where_array(spec.having) if spec.having is not None else (None, 0)
            rc = engine._lib.hsg_op_create_mapped(engine._h, C.byref(cfg), marr, mn, wprog, wn, hprog, hn, C.byref(h))
        elif spec.having is not None or spec.where is not None:
            what = "hsg_op_create_filtered"
            wprog, wn = abi.where_array(spec.where) if spec.where is not None else (None, 0)
            hprog, hn = abi.where_array(spec.having) if spec.having is not None else (None, 0)
            rc = engine._lib.hsg_op_create_filtered(engine._h, C.byref(cfg), wprog, wn, hprog, hn, C.byref(h))
        else:
            rc = engine._lib.hsg_op_create(engine._h, C.byref(cfg), C.byref(h))
        if rc != abi.HSG_OK:
            msg = engine._lib.hsg_engine_last_error(engine._h)
            raise abi.HStreamGpuError(rc, f"{what}: {msg.decode() if msg else ''}")
        self.engine = engine  # keep the engine alive while the op lives
        super().__init__(engine._lib, "hsg", h, spec)

    def set_changelog(self, rows):
        """Register caller-owned device columns (an abi.hsg_rows with mem =
        HSG_MEM_DEVICE) as the changelog: pushes write rows there directly and
        drain_count() reports how many (hsg_op_set_changelog). None restores
        the op's own buffer."""
        self._check(self._lib.hsg_op_set_changelog(self._h, C.byref(rows) if rows is not None else None),
                    "op_set_changelog")
        self._sink = rows

    def drain_count(self) -> int:
        """hsg_drain with a registered changelog: the rows are already in place."""
        got = C.c_uint64(0)
        self._check(self._lib.hsg_drain(self._h, None, C.byref(got)), "drain")
        return got.value

    def push_async(self, key_id, ts, cols=(), valid=None, watermark=None, done=None, mem=None, **enc):
        """hsg_push_batch_async: queue the batch and return at once. `watermark`
        is a ctypes.c_int64 shared by consecutive pushes (read when the batch
        starts, written before `done(rc)` runs on the op's completion thread).
        The arrays are kept alive until the completion has run."""
        from .columnar import make_batch
        b, keep = make_batch(key_id, ts, cols, valid, mem, **enc)
        return self.push_batch_async(b, watermark, done, keep)

    def push_batch_async(self, batch, watermark=None, done=None, keep=None):
        """hsg_push_batch_async of a ready hsg_batch (e.g. a GpuDecodedBatch's
        device batch with its ready_event); `keep` is held until the
        completion has run. Otherwise as push_async."""
        wm = watermark if watermark is not None else C.c_int64(-1)
        entry = {}

        def _cb(_ctx, rc):
            try:
                if done is not None:
                    done(rc)
            finally:
                self._inflight.pop(id(entry), None)

        cb = abi.HSG_DONE_FN(_cb)
        entry.update(keep=keep, b=batch, cb=cb, wm=wm)
        if not hasattr(self, "_inflight"):
            self._inflight = {}
        self._inflight[id(entry)] = entry
        rc = self._lib.hsg_push_batch_async(self._h, C.byref(batch), C.byref(wm), cb, None)
        if rc != abi.HSG_OK:
            self._inflight.pop(id(entry), None)
        self._check(rc, "push_batch_async")
        return wm

    def wait(self):
        """hsg_op_wait: block until the queued pushes are done; raises the first failure."""
        self._check(self._lib.hsg_op_wait(self._h), "op_wait")

    def view_get(self, key_ids, capacity=None) -> Rows:
        """hsg_view_get: the state rows of the given key ids (at most
        HSG_VIEW_MAX_KEYS), as dump_state() returns them and in its order. The
        rows land in host columns of `capacity` rows (default: 64 per key); when
        they do not fit, the call is made once more with the count it reported."""
        keys = np.ascontiguousarray(np.asarray(key_ids, dtype=np.uint32).ravel())
        cap = int(capacity) if capacity is not None else 64 * max(1, keys.size)
        for attempt in (0, 1):
            rows, arrs, keep = alloc_rows(cap, self._f64, self._forms)
            got = C.c_uint64(0)
            rc = self._lib.hsg_view_get(self._h, keys.ctypes.data if keys.size else None, keys.size, C.byref(rows),
                                        C.byref(got))
            if rc == abi.HSG_E_CAPACITY and attempt == 0:
                cap = got.value
                continue
            self._check(rc, "view_get")
            return truncate(arrs, got.value)

    def table_join_into(self, key_ids, rows, mem=None, ready_event=None):
        """hsg_table_join into caller-owned columns (an abi.hsg_rows, host or
        device memory): (status, rows written or needed). HSG_E_CAPACITY is
        returned, not raised; any other failure raises."""
        probe, keep = make_probe(key_ids, mem, ready_event)
        got = C.c_uint64(0)
        rc = self._lib.hsg_table_join(self._h, C.byref(probe), C.byref(rows), C.byref(got))
        del keep
        if rc != abi.HSG_E_CAPACITY:
            self._check(rc, "table_join")
        return rc, got.value

    def table_join(self, key_ids, capacity=None, mem=None) -> Rows:
        """hsg_table_join: this unwindowed op as the table of a stream-table
        join. key_ids are the stream records' keys in this op's dictionary, in
        arrival order (numpy, or a torch device tensor as push accepts);
        HSG_KEY_NONE matches nothing. One row per record whose key has a live
        row, in arrival order, src_index = the record's index. The rows land in
        host columns of `capacity` rows (default: one per record); when they do
        not fit, the call is made once more with the count it reported."""
        n = int(key_ids.numel()) if _is_torch(key_ids) else int(np.asarray(key_ids).size)
        cap = int(capacity) if capacity is not None else max(1, n)
        for attempt in (0, 1):
            rows, arrs, keep = alloc_rows(cap, self._f64, self._forms)
            rc, got = self.table_join_into(key_ids, rows, mem)
            if rc == abi.HSG_E_CAPACITY and attempt == 0:
                cap = got
                continue
            self._check(rc, "table_join")
            return truncate(arrs, got)

    def select_stats(self) -> dict:
        """hsg_op_select_stats: a select op's drop and row counts."""
        s = abi.hsg_select_stats()
        self._check(self._lib.hsg_op_select_stats(self._h, C.byref(s)), "op_select_stats")
        return s.as_dict()

    def map_stats(self) -> dict:
        """hsg_op_map_stats: the map's counters (zeros for an op without one)."""
        s = abi.hsg_map_stats()
        self._check(self._lib.hsg_op_map_stats(self._h, C.byref(s)), "op_map_stats")
        return s.as_dict()

    def stats(self) -> dict:
        s = abi.hsg_stats()
        self._check(self._lib.hsg_op_stats(self._h, C.byref(s)), "op_stats")
        return s.as_dict()
