"""Host-side mirror of the reference's Stream DSL for the windowed GROUP BY path.

Names and argument meaning follow hstream-processing (Yu-zh/hstream):

  TimeWindows / mkTumblingWindow / mkHoppingWindow   Stream/TimeWindows.hs:23-43
  TimeWindow / TimeWindowKey                         Stream/TimeWindows.hs:45-63
  SessionWindows / mkSessionWindows                  Stream/SessionWindows.hs:20-30
  GroupedStream.timeWindowedBy / sessionWindowedBy   Stream/GroupedStream.hs:89-117
  GroupedStream / TimeWindowedStream / SessionWindowedStream .aggregate / .count
                                                     GroupedStream.hs:35-69,
                                                     TimeWindowedStream.hs:32-70,
                                                     SessionWindowedStream.hs:33-72
  Materialized                                       Stream/Internal.hs:123-128
  runTask (poll loop + stream time)                  Processor.hs:99-144
  Stream.filter / Stream.map                         Stream.hs:151-194 (the scalar SELECT
                                                     chain, Codegen.hs:542-550)
  joinStream (the SQL JOIN plan's, with genJoiner)   Stream.hs:222-300, Codegen.hs:253-266
  time-window / session key serdes                   TimeWindows.hs:68-93,
                                                     hstream-sql/.../Codegen/Boilerplate.hs:60-88

The reference processes one record at a time through a topology; here an
operator is one libhstream_gpu op and a poll batch is handed over whole.
Records arrive as (key, value-object, timestamp) like SourceRecord
(Type.hs), the group key is dictionary-encoded to a u32 id with the
reference's key equality (Aeson values: 1 and 1.0 are one key), and the
aggregated fields are extracted into typed columns. A record whose
aggregated field has the wrong type makes the reference throw before any
window is updated (Codegen.hs:430-431, Processor.hs:140-143); it is passed as
HSG_KEY_NONE so it still moves stream time, exactly like a record the WHERE
clause filtered.
"""
import struct
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import abi
from .columnar import OpSpec, Rows

GRACE_MS = abi.HSG_DEFAULT_GRACE_MS  # 24 * 3600 * 1000


# ---------------------------------------------------------------------------
# window specs (Stream/TimeWindows.hs, Stream/SessionWindows.hs)
# ---------------------------------------------------------------------------
@dataclass(frozen=True)
class TimeWindows:
    twSizeMs: int
    twAdvanceMs: int
    twGraceMs: int = GRACE_MS


def mkTumblingWindow(windowSize: int) -> TimeWindows:
    return TimeWindows(windowSize, windowSize, GRACE_MS)


def mkHoppingWindow(windowSize: int, stepSize: int) -> TimeWindows:
    return TimeWindows(windowSize, stepSize, GRACE_MS)


@dataclass(frozen=True)
class SessionWindows:
    swInactivityGap: int
    swGraceMs: int = GRACE_MS  # defined by the reference, never read


def mkSessionWindows(inactivityGap: int) -> SessionWindows:
    return SessionWindows(inactivityGap, GRACE_MS)


@dataclass(frozen=True, order=True)
class TimeWindow:
    tWindowStart: int
    tWindowEnd: int


@dataclass(frozen=True)
class TimeWindowKey:
    twkKey: Any
    twkWindow: TimeWindow


# ---------------------------------------------------------------------------
# key and window serdes at the output boundary
# ---------------------------------------------------------------------------
def time_window_bytes(w: TimeWindow) -> bytes:
    """timeWindowSerde: int64BE start ++ int64BE 0 (Boilerplate.hs:60-74)."""
    return struct.pack(">qq", w.tWindowStart, 0)


def session_window_bytes(w: TimeWindow) -> bytes:
    """sessionWindowSerde: int64BE start ++ int64BE end (Boilerplate.hs:76-88)."""
    return struct.pack(">qq", w.tWindowStart, w.tWindowEnd)


def time_window_key_bytes(key_bytes: bytes, w: TimeWindow, session=False) -> bytes:
    """timeWindowKeySerializer: compose (window bytes, key bytes) (TimeWindows.hs:68-73)."""
    return (session_window_bytes(w) if session else time_window_bytes(w)) + key_bytes


def time_window_key_from_bytes(b: bytes, window_size: int, session=False) -> Tuple[bytes, TimeWindow]:
    """timeWindowKeyDeserializer: split at 16, end = start + size (TimeWindows.hs:75-85)."""
    start, second = struct.unpack(">qq", b[:16])
    end = second if session else start + window_size
    return b[16:], TimeWindow(start, end)


# ---------------------------------------------------------------------------
# key dictionary with the reference's key equality
# ---------------------------------------------------------------------------
def _canon(v):
    # Aeson Number is Scientific: 1 == 1.0; bools are not numbers
    if isinstance(v, bool) or v is None:
        return ("b", v)
    if isinstance(v, (int, float, np.integer, np.floating)):
        f = float(v)
        if f.is_integer():
            return ("n", int(f))
        return ("n", f)
    if isinstance(v, dict):
        return ("o", tuple(sorted((k, _canon(x)) for k, x in v.items())))
    if isinstance(v, (list, tuple)):
        return ("a", tuple(_canon(x) for x in v))
    return ("s", v)


class KeyDict:
    """Group key <-> u32 id. HSG_KEY_NONE is never handed out."""

    def __init__(self):
        self._ids: Dict[Any, int] = {}
        self._keys: List[Any] = []

    def encode(self, key) -> int:
        c = _canon(key)
        i = self._ids.get(c)
        if i is None:
            i = len(self._keys)
            if i >= abi.HSG_KEY_NONE:
                raise OverflowError("key dictionary full")
            self._ids[c] = i
            self._keys.append(key)
        return i

    def find(self, key) -> int:
        """The key's id without inserting it (reads): HSG_KEY_NONE when absent."""
        return self._ids.get(_canon(key), abi.HSG_KEY_NONE)

    def decode(self, i: int):
        return self._keys[int(i)]

    def __len__(self):
        return len(self._keys)


# ---------------------------------------------------------------------------
# aggregates: the SQL components the codegen builds (Codegen.hs:399-469)
# ---------------------------------------------------------------------------
@dataclass(frozen=True)
class Expr:
    """A value expression of the SELECT list (hstream_amd.sql RExprBinOp /
    RExprConst / RExprCol tree) in an aggregate's place of a field name, and
    which of the fields it reads carry decimals (f64 columns). The op's map
    pass evaluates it per record on the GPU (hsg_op_create_mapped)."""

    tree: Any
    float_fields: Tuple[str, ...] = ()
    functions: bool = False   # push the tree's numeric unary functions down too (sql.compile_expr)

    def __str__(self):
        return self.tree.name


@dataclass(frozen=True)
class Agg:
    kind: int                 # abi.HSG_COUNT_ALL ...
    field: Any = None         # a field name, or an Expr
    alias: Optional[str] = None
    is_float: bool = False    # the column's type (numbers with decimals -> f64)
    strict: bool = False      # an Expr only: a record whose expression is the error value is dropped (HSG_MAP_STRICT)

    @property
    def name(self):
        if self.alias:
            return self.alias
        n = {abi.HSG_COUNT_ALL: "COUNT(*)", abi.HSG_COUNT: "COUNT", abi.HSG_SUM: "SUM", abi.HSG_MIN: "MIN",
             abi.HSG_MAX: "MAX", abi.HSG_AVG: "AVG", abi.HSG_LAST: ""}[self.kind]
        return n if self.kind == abi.HSG_COUNT_ALL else (f"{n}({self.field})" if n else self.field)


def COUNT_ALL(alias=None):
    return Agg(abi.HSG_COUNT_ALL, None, alias)


def COUNT(f, alias=None):
    return Agg(abi.HSG_COUNT, f, alias)


def SUM(f, alias=None, is_float=False):
    return Agg(abi.HSG_SUM, f, alias, is_float)


def MIN(f, alias=None, is_float=False):
    return Agg(abi.HSG_MIN, f, alias, is_float)


def MAX(f, alias=None, is_float=False):
    return Agg(abi.HSG_MAX, f, alias, is_float)


def AVG(f, alias=None, is_float=False):
    return Agg(abi.HSG_AVG, f, alias, is_float)


def LAST(f, alias=None, is_float=False, strict=False):
    """A non-aggregate SELECT column: the last record's value (Codegen.hs:463-469)."""
    return Agg(abi.HSG_LAST, f, alias, is_float, strict)


@dataclass
class Where:
    """The query's WHERE clause for an aggregate: the refined search condition
    (hstream_amd.sql RCond*) and which of its fields carry decimals (f64
    columns). The op runs it on the GPU ahead of the aggregate, where the
    reference chains genFilterNode in front (Codegen.hs:540)."""

    cond: Any
    float_fields: Sequence[str] = ()
    functions: bool = False   # push the condition's numeric unary functions down too (sql.compile_where)


@dataclass
class Having:
    """The query's HAVING clause for an aggregate: the refined search condition
    (hstream_amd.sql RCond*) over the aggregates' aliases. The op runs it on the
    GPU over the changelog rows it emits and forwards the rows it keeps, where
    the reference chains genFilteRNodeFromHaving behind an unwindowed
    aggregate (Codegen.hs:524-529); the table's state (dump, view reads) is
    that of the aggregate without it."""

    cond: Any
    functions: bool = False   # push the condition's numeric unary functions down too (sql.compile_having)


@dataclass
class Materialized:
    """mKeySerde/mValueSerde/mStateStore (Stream/Internal.hs:123-128): the key
    dictionary plays the key serde, the HBM table the state store."""

    keys: KeyDict = field(default_factory=KeyDict)
    state_capacity: int = 0
    out_capacity: int = 0


# ---------------------------------------------------------------------------
# streams and tables
# ---------------------------------------------------------------------------
class GroupedStream:
    """A re-keyed stream (Stream.groupBy, Stream.hs:196-211)."""

    def __init__(self, engine, key_field: str):
        self.engine = engine
        self.key_field = key_field

    def timeWindowedBy(self, windows: TimeWindows) -> "TimeWindowedStream":
        return TimeWindowedStream(self, windows)

    def sessionWindowedBy(self, windows: SessionWindows) -> "SessionWindowedStream":
        return SessionWindowedStream(self, windows)

    def aggregate(self, aggs: Sequence[Agg], materialized: Materialized, emit=abi.HSG_EMIT_PER_RECORD,
                  where: Optional[Where] = None, having: Optional[Having] = None) -> "Table":
        return Table(self, OpSpec(abi.HSG_UNWINDOWED, emit), aggs, materialized, where, having)

    def count(self, materialized: Materialized, emit=abi.HSG_EMIT_PER_RECORD) -> "Table":
        return self.aggregate([COUNT_ALL("count")], materialized, emit)


def groupBy(engine, key_field: str) -> GroupedStream:
    return GroupedStream(engine, key_field)


class TimeWindowedStream:
    def __init__(self, grouped: GroupedStream, windows: TimeWindows):
        self.grouped = grouped
        self.windows = windows

    def aggregate(self, aggs, materialized, emit=abi.HSG_EMIT_PER_RECORD, where: Optional[Where] = None,
                  having: Optional[Having] = None) -> "Table":
        w = self.windows
        kind = abi.HSG_TUMBLING if w.twAdvanceMs == w.twSizeMs else abi.HSG_HOPPING
        spec = OpSpec(kind, emit, size_ms=w.twSizeMs, advance_ms=w.twAdvanceMs, grace_ms=w.twGraceMs)
        return Table(self.grouped, spec, aggs, materialized, where, having)

    def count(self, materialized, emit=abi.HSG_EMIT_PER_RECORD) -> "Table":
        return self.aggregate([COUNT_ALL("count")], materialized, emit)


class SessionWindowedStream:
    def __init__(self, grouped: GroupedStream, windows: SessionWindows):
        self.grouped = grouped
        self.windows = windows

    def aggregate(self, aggs, materialized, emit=abi.HSG_EMIT_PER_RECORD, where: Optional[Where] = None,
                  having: Optional[Having] = None) -> "Table":
        spec = OpSpec(abi.HSG_SESSION, emit, gap_ms=self.windows.swInactivityGap)
        return Table(self.grouped, spec, aggs, materialized, where, having)

    def count(self, materialized, emit=abi.HSG_EMIT_PER_RECORD) -> "Table":
        return self.aggregate([COUNT_ALL("count")], materialized, emit)


class Table:
    """The aggregate operator's output table (Table.hs), backed by one GPU op.

    process(records) runs one poll batch; it returns the changelog rows as
    (TimeWindowKey | key, {alias: value}) in the order the reference forwards
    them (per-record mode) or one row per touched group (per-batch mode)."""

    def __init__(self, grouped: GroupedStream, spec: OpSpec, aggs: Sequence[Agg], materialized: Materialized,
                 where: Optional[Where] = None, having: Optional[Having] = None):
        self.grouped = grouped
        self.aggs = list(aggs)
        self.mat = materialized
        fields: List[Tuple[str, bool]] = []
        # the aggregates' columns: a field, or a value expression the op's map
        # pass computes (hsg_op_create_mapped); with an expression among them
        # every column is one of the map's, a bare field a one-instruction one
        acols: List[Tuple[Any, bool, bool]] = []
        for a in self.aggs:
            if a.kind == abi.HSG_COUNT_ALL:
                continue
            if (a.field, a.is_float, a.strict) not in acols:
                acols.append((a.field, a.is_float, a.strict))
            if not isinstance(a.field, Expr) and (a.field, a.is_float) not in fields:
                fields.append((a.field, a.is_float))
        mapped = any(isinstance(f, Expr) for f, _, _ in acols)
        if mapped:
            col_of = {a: i for i, a in enumerate(acols)}
        else:
            col_of = {(f, fl, st): i for i, (f, fl) in enumerate(fields) for st in (False, True)}
        # a column read only by COUNT(col) counts any present value (Codegen.hs:412-422);
        # SUM / MIN / MAX / AVG / LAST need a Number (Codegen.hs:423-461)
        self.numeric = [any(a.kind not in (abi.HSG_COUNT_ALL, abi.HSG_COUNT) and (a.field, a.is_float) == fk
                            for a in self.aggs) for fk in fields]
        if mapped:
            # the fields the expressions read follow as columns of the batch;
            # each must hold a Number (a present non-number drops the record at
            # ingest, as for WHERE fields: the program computes numbers only)
            from . import sql
            for f, _, _ in acols:
                if not isinstance(f, Expr):
                    continue
                for name in sql.where_fields(f.tree):
                    names = [x for x, _ in fields]
                    if name in names:
                        self.numeric[names.index(name)] = True
                    else:
                        fields.append((name, name in f.float_fields))
                        self.numeric.append(True)
            names = [x for x, _ in fields]
            spec.map = [abi.MapExpr(sql.compile_expr(f.tree, names, key_field=grouped.key_field, functions=f.functions),
                                    abi.HSG_MAP_STRICT if st else 0) if isinstance(f, Expr)
                        else abi.MapExpr([(abi.HSG_W_COL, fields.index((f, fl)))]) for f, fl, st in acols]
        self.where = where
        if where is not None:
            # the filter runs in the op (hsg_op_create_where): the fields only it
            # reads follow the aggregated ones as columns of their own, and every
            # field it reads must hold a Number (a present non-number drops the
            # record here, at ingest; the program compares numbers only)
            from . import sql
            names = [f for f, _ in fields]
            for f in sql.where_fields(where.cond):
                if f in names:
                    self.numeric[names.index(f)] = True
                else:
                    names.append(f)
                    fields.append((f, f in where.float_fields))
                    self.numeric.append(True)
            spec.where = sql.compile_where(where.cond, names, key_field=grouped.key_field, functions=where.functions)
        self.having = having
        if having is not None:
            # the filter over the emitted rows runs in the op too
            # (hsg_op_create_filtered), over the aggregates by alias
            from . import sql
            spec.having = sql.compile_having(having.cond, self.aggs, functions=having.functions)
        self.fields = fields
        self._decoder = None
        spec.col_types = [abi.HSG_F64 if fl else abi.HSG_I64 for _, fl in fields]
        spec.aggs = [(a.kind, col_of[(a.field, a.is_float, a.strict)] if a.kind != abi.HSG_COUNT_ALL else 0)
                     for a in self.aggs]
        spec.state_capacity = materialized.state_capacity
        spec.out_capacity = materialized.out_capacity
        self.spec = spec
        self.op = grouped.engine.op(spec)
        self.windowed = spec.window_kind != abi.HSG_UNWINDOWED

    # -- columnar extraction ------------------------------------------------
    def columns(self, records):
        n = len(records)
        keys = np.empty(n, dtype=np.uint32)
        ts = np.empty(n, dtype=np.int64)
        cols = [np.zeros(n, dtype=np.float64 if fl else np.int64) for _, fl in self.fields]
        valid = [np.ones(n, dtype=np.uint8) for _ in self.fields]
        kf = self.grouped.key_field
        for i, rec in enumerate(records):
            value = rec["value"]
            ts[i] = rec["timestamp"]
            ok = kf in value
            for c, (f, fl) in enumerate(self.fields):
                if f not in value:
                    valid[c][i] = 0  # HM.lookup ... Nothing -> the component leaves the acc alone
                    continue
                v = value[f]
                if not self.numeric[c]:
                    continue  # COUNT(col): present is enough, whatever the value
                if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                    ok = False  # "Only columns with Int or Number type ..." aborts the record
                    break
                cols[c][i] = float(v) if fl else int(v)
            keys[i] = self.mat.keys.encode(value[kf]) if ok else abi.HSG_KEY_NONE
        return keys, ts, cols, valid

    def _rows(self, rows: Rows):
        out = []
        for i in range(len(rows)):
            key = self.mat.keys.decode(rows.key_id[i])
            vals = {a.name: rows.aggs[j][i].item() for j, a in enumerate(self.aggs)}
            if self.windowed:
                out.append((TimeWindowKey(key, TimeWindow(int(rows.win_start[i]), int(rows.win_end[i]))), vals))
            else:
                out.append((key, vals))
        return out

    def process_json(self, buf: bytes, off, ts, watermark=-1, threads=0, device_decode=False):
        """One poll batch of raw JSON record values (SourceRecord srcValue) and
        their timestamps, decoded by the native ingest (include/hstream_ingest.h)
        straight into the op's columns; needs Materialized(keys=ingest.KeyDict()).
        device_decode: decode on the GPU (ingest.GpuDecoder; the records outside
        its fast subset through the host decoder) and push the device batch."""
        from . import ingest
        if not isinstance(self.mat.keys, ingest.KeyDict):
            raise TypeError("process_json needs Materialized(keys=hstream_amd.ingest.KeyDict())")
        dcols = [(f, abi.HSG_F64 if fl else abi.HSG_I64, num) for (f, fl), num in zip(self.fields, self.numeric)]
        if device_decode:
            self._gpu_decoder = _sized_gpu_decoder(getattr(self, "_gpu_decoder", None), self.grouped.engine,
                                                   self.mat.keys, self.grouped.key_field, dcols, False, off)
            db = self._gpu_decoder.decode(buf, off, ts, threads)
            wm = self.op.push_batch(db.batch, watermark=watermark)
        else:
            if self._decoder is None:
                self._decoder = ingest.Decoder(self.grouped.key_field, dcols)
            keys, ts_out, cols, valid, _, _ = self._decoder.decode(self.mat.keys, buf, off, ts, threads)
            wm = self.op.push(keys, ts_out, cols, valid, watermark=watermark)
        rows = self.op.drain() if self.spec.emit_mode != abi.HSG_EMIT_NONE else None
        return wm, ([] if rows is None else self._rows(rows))

    def process(self, records, watermark=-1):
        keys, ts, cols, valid = self.columns(records)
        wm = self.op.push(keys, ts, cols, valid, watermark=watermark)
        rows = self.op.drain() if self.spec.emit_mode != abi.HSG_EMIT_NONE else None
        return wm, ([] if rows is None else self._rows(rows))

    def dump(self):
        """ksDump / ssDump (views): every live group."""
        return self._rows(self.op.dump_state())

    def get(self, key):
        """The rows of one key (ksGet / findSessions), read from HBM by key
        (hsg_view_get): [] for a key the dictionary has never seen, which is
        looked up without being inserted."""
        kid = self.mat.keys.find(key)
        if kid == abi.HSG_KEY_NONE:
            return []
        return self._rows(self.op.view_get([kid]))

    def select_view(self, key):
        """SELECT ... FROM view WHERE key = x (SelectViewPlan, Handler.hs:277-323)."""
        return select_view_result(self.get(key), self.windowed, self.spec.window_kind == abi.HSG_SESSION,
                                  self.spec.size_ms)

    def close(self):
        self.op.close()


class Stream:
    """A stream without a group key: HS.filter / HS.map (Stream.hs:151-194) as
    the SQL code generator chains them for a SELECT without GROUP BY
    (genFilterNode -> genMapNode -> genFilteRNodeFromHaving, Codegen.hs:542-550),
    backed by one select op (hsg_op_create_select), built on first use.

      Stream(engine, fields).filter(Where).map(exprs).having(Having)

    fields: the numeric fields the query reads, each a name or (name,
    is_float), in the batch's column order. exprs: [(alias, tree)] with tree a
    field name or an hstream_amd.sql value expression; without map() the stream
    is SELECT *: the op returns indices and process() forwards the original
    records. Every field must hold a Number where present (a present
    non-number drops the record at ingest: the programs compute numbers only).

    process(records) runs one poll batch and returns (stream time, the records
    forwarded, in arrival order) as {"value": {alias: number}, "timestamp": ts}."""

    def __init__(self, engine, fields: Sequence, literal_forms: bool = False, out_capacity: int = 0):
        self.engine = engine
        self.fields = [(f, False) if isinstance(f, str) else (f[0], bool(f[1])) for f in fields]
        self.literal_forms = literal_forms
        self.out_capacity = out_capacity
        self.where_prog = None
        self.having_prog = None
        self.exprs: Optional[List[Tuple[str, List[Tuple]]]] = None  # None: SELECT *
        self._having = None
        self._op = None
        self._decoder = None
        self.last_rows: Optional[Rows] = None  # the rows the last process / process_json drained (for the sink)

    def _names(self):
        return [f for f, _ in self.fields]

    def filter(self, where: Where) -> "Stream":
        from . import sql
        self.where_prog = sql.compile_where(where.cond, self._names(), functions=where.functions)
        return self

    def map(self, exprs: Sequence[Tuple[str, Any]], functions: bool = False) -> "Stream":
        from . import sql
        if len(exprs) > abi.HSG_MAP_MAX_EXPRS:
            raise ValueError(f"SELECT list of {len(exprs)} expressions (max {abi.HSG_MAP_MAX_EXPRS})")
        aliases = [a for a, _ in exprs]
        dup = sorted({a for a in aliases if aliases.count(a) > 1})
        if dup:
            raise ValueError(f"SELECT list with duplicate aliases {dup} is not pushed down")
        out = []
        for alias, tree in exprs:
            if isinstance(tree, Expr):
                functions_here, tree = tree.functions or functions, tree.tree
            else:
                functions_here = functions
            if isinstance(tree, str):
                tree = sql.RExprCol(tree, None, tree)
            out.append((alias, sql.compile_expr(tree, self._names(), functions=functions_here)))
        if sum(len(p) for _, p in out) > abi.HSG_MAP_MAX_INS:
            raise ValueError(f"SELECT list needs more than {abi.HSG_MAP_MAX_INS} instructions")
        self.exprs = out
        if self._having is not None:
            self.having(self._having)
        return self

    def having(self, having: Having) -> "Stream":
        from . import sql
        self._having = having
        self.having_prog = sql.compile_having(having.cond, [a for a, _ in (self.exprs or [])],
                                              functions=having.functions)
        return self

    @property
    def aliases(self) -> List[str]:
        return [a for a, _ in (self.exprs or [])]

    @property
    def op(self):
        if self._op is None:
            self._op = self.engine.select_op(
                [abi.HSG_F64 if fl else abi.HSG_I64 for _, fl in self.fields], [p for _, p in (self.exprs or [])],
                where=self.where_prog, having=self.having_prog, out_capacity=self.out_capacity,
                flags=abi.HSG_OPF_LITERAL_FORMS if self.literal_forms else 0)
        return self._op

    def sink(self):
        """The sink encoder of this stream's rows (hstream_amd.sink.Sink): no
        key (every key record is empty), the value object {alias: value}."""
        from .sink import Sink
        return Sink(self.op, None, None, [(a, j) for j, a in enumerate(self.aliases)], windowed=False)

    def columns(self, records):
        n = len(records)
        keys = np.zeros(n, dtype=np.uint32)
        ts = np.empty(n, dtype=np.int64)
        cols = [np.zeros(n, dtype=np.float64 if fl else np.int64) for _, fl in self.fields]
        valid = [np.ones(n, dtype=np.uint8) for _ in self.fields]
        for i, rec in enumerate(records):
            value = rec["value"]
            ts[i] = rec["timestamp"]
            for c, (f, fl) in enumerate(self.fields):
                if f not in value:
                    valid[c][i] = 0
                    continue
                v = value[f]
                if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                    keys[i] = abi.HSG_KEY_NONE  # the programs compute numbers only
                    break
                cols[c][i] = float(v) if fl else int(v)
        return keys, ts, cols, valid

    def _forward(self, rows: Rows, base: int, originals):
        self.last_rows = rows
        out = []
        names = self.aliases
        for i in range(len(rows)):
            if self.exprs is None:
                value = originals(int(rows.src_index[i]) - base)
            else:
                value = {a: rows.aggs[j][i].item() for j, a in enumerate(names)}
            out.append({"value": value, "timestamp": int(rows.win_start[i])})
        return out

    def process(self, records, watermark=-1):
        keys, ts, cols, valid = self.columns(records)
        base = self.op.stats()["records"]
        wm = self.op.push(keys, ts, cols, valid, watermark=watermark)
        return wm, self._forward(self.op.drain(), base, lambda k: records[k]["value"])

    def process_json(self, buf: bytes, off, ts, watermark=-1, threads=0, device_decode=False):
        """One poll batch of raw JSON record values and their timestamps,
        decoded by the native ingest without a key field; a SELECT * stream
        forwards the records' own bytes. device_decode: as Table.process_json."""
        from . import ingest
        dcols = [(f, abi.HSG_F64 if fl else abi.HSG_I64, True) for f, fl in self.fields]
        base = self.op.stats()["records"]
        if device_decode:
            self._gpu_decoder = _sized_gpu_decoder(getattr(self, "_gpu_decoder", None), self.engine, None, None, dcols,
                                                   self.literal_forms, off)
            db = self._gpu_decoder.decode(buf, off, ts, threads)
            wm = self.op.push_batch(db.batch, watermark=watermark)
        else:
            if self._decoder is None:
                self._decoder = ingest.Decoder(None, dcols, literal_forms=self.literal_forms)
            keys, ts_out, cols, valid, _, _ = self._decoder.decode(None, buf, off, ts, threads)
            wm = self.op.push(keys, ts_out, cols, valid, watermark=watermark)
        return wm, self._forward(self.op.drain(), base, lambda k: bytes(buf[int(off[k]):int(off[k + 1])]))

    def close(self):
        if self._op is not None:
            self._op.close()
            self._op = None


def select_view_result(rows, windowed: bool, session: bool, size_ms: int, names: Optional[Sequence[str]] = None):
    """The answer of SELECT ... FROM view WHERE key = x for one key's rows, as
    SelectViewPlan shapes it (hstream/src/HStream/Server/Handler.hs:287-323):

      fixed windows   {"winStart = S ,winEnd = E": values} with E = S + size_ms
                      (:299-312; no row: the empty object)
      sessions        {"winStart = S": values} in start order (:315-323)
      no window       the key's values, or None (ksGet, :313)

    `rows`: Table.get(key)'s pairs, or columnar Rows of one key, whose values
    are then named by `names` (default "0", "1", ...). Pure: no GPU."""
    if isinstance(rows, Rows):
        nm = list(names) if names is not None else [str(j) for j in range(len(rows.aggs))]
        starts = [int(s) for s in rows.win_start]
        vals = [{nm[j]: a[i].item() for j, a in enumerate(rows.aggs)} for i in range(len(rows))]
    else:
        starts = [k.twkWindow.tWindowStart if isinstance(k, TimeWindowKey) else 0 for k, _ in rows]
        vals = [v for _, v in rows]
    if not windowed:
        return vals[0] if vals else None
    order = sorted(range(len(starts)), key=starts.__getitem__)
    if session:
        return {f"winStart = {starts[i]}": vals[i] for i in order}
    return {f"winStart = {starts[i]} ,winEnd = {starts[i] + int(size_ms)}": vals[i] for i in order}


# ---------------------------------------------------------------------------
# tables as join sides (Stream.table, Stream.joinTable)
# ---------------------------------------------------------------------------
def table(engine, key_field: str, fields: Sequence, materialized: Materialized) -> Table:
    """Stream.table / tableStoreProcessor (Stream.hs:79-129): a stream read as a
    table, the latest value per key, kept in HBM to be joined against
    (joinTable). `fields` names the value's fields to keep, each a name or a
    (name, is_float) pair. It is an unwindowed HSG_EMIT_NONE op with one LAST
    per field; feed it with Table.process.

    One difference: the reference replaces the whole stored object per record
    (ksPut keyBytes valueBytes), whereas LAST per field keeps each field's last
    PRESENT value, so a record that lacks a field leaves that field's earlier
    value in place where the reference would drop it. The two are equal when
    every record carries every field."""
    aggs = []
    for f in fields:
        name, is_float = (f, False) if isinstance(f, str) else (f[0], bool(f[1]))
        aggs.append(LAST(name, name, is_float))
    return GroupedStream(engine, key_field).aggregate(aggs, materialized, emit=abi.HSG_EMIT_NONE)


def join_table_result(records, rows: Rows, aliases: Sequence[str], joiner, key_field: str = "key"):
    """The records joinTableProcessor forwards (Stream.hs:334-344) for one poll
    batch `records` of the stream side, given the table's answer `rows`
    (hsg_table_join: one row per matching record, src_index = its index in the
    batch): for each row in src_index order, the stream record with its value
    replaced by joiner(stream value, {alias: table value}); key and timestamp
    are the stream record's. Pure: no GPU."""
    out = []
    for i in np.argsort(np.asarray(rows.src_index), kind="stable"):
        rec = records[int(rows.src_index[i])]
        v2 = {a: rows.aggs[j][i].item() for j, a in enumerate(aliases)}
        out.append({"key": rec["value"][key_field], "value": joiner(rec["value"], v2), "timestamp": rec["timestamp"]})
    return out


def joinTable(table: Table, joiner, records) -> list:
    """Stream.joinTable (Stream.hs:302-344) for one poll batch of the stream
    side: each record whose key has a row in `table` (an unwindowed Table, the
    KV store joinTableProcessor reads) is forwarded with joiner(value, row),
    in arrival order; the others are dropped. The keys are looked up in the
    table's dictionary without being inserted (KeyDict.find): a record without
    the key field, or with a key the table has never seen, probes as
    HSG_KEY_NONE and matches nothing. The lookups run on the GPU
    (GpuOp.table_join)."""
    kf = table.grouped.key_field
    find = table.mat.keys.find
    kids = np.fromiter((find(r["value"][kf]) if kf in r["value"] else abi.HSG_KEY_NONE for r in records),
                       dtype=np.uint32, count=len(records))
    rows = table.op.table_join(kids)
    return join_table_result(records, rows, [a.name for a in table.aggs], joiner, kf)


def _sized_gpu_decoder(dec, engine, keys, key_field, cols, literal_forms, off):
    """The device decoder of a process_json(device_decode=True) caller, made on
    first use and made again, larger, when a poll batch outgrows it."""
    from . import ingest
    n, nbytes = len(off) - 1, int(off[-1]) - int(off[0]) if len(off) else 0
    if dec is not None and n <= dec.max_records and nbytes <= dec.max_bytes:
        return dec
    max_records = max(1 << 16, 2 * n, dec.max_records if dec is not None else 0)
    max_bytes = max(1 << 24, 2 * nbytes, dec.max_bytes if dec is not None else 0)
    if dec is not None:
        dec.close()
    dec = ingest.GpuDecoder(engine, keys, key_field, cols, literal_forms=literal_forms, max_records=max_records,
                            max_bytes=max_bytes)
    return dec


def runTask(poll, table: Table, max_polls=None, sink=None, device_decode=False):
    """Processor.hs:99-144 for one windowed aggregate: poll a batch, advance the
    task's stream time over every polled record, run the operator, forward
    the changelog to `sink`. `poll()` returns a list of records, or the raw
    JSON values of a poll batch as (buf, off, ts) for process_json (decoded on
    the GPU with device_decode), or None.
    `table` is a Table, or a Stream (the scalar SELECT chain)."""
    wm = -1  # tcTimestamp starts at -1 (Processor/Internal.hs:151)
    polls = 0
    while max_polls is None or polls < max_polls:
        batch = poll()
        if batch is None:
            break
        if isinstance(batch, tuple):
            wm, rows = table.process_json(*batch, watermark=wm, device_decode=device_decode)
        else:
            wm, rows = table.process(batch, watermark=wm)
        if sink is not None:
            for r in rows:
                sink(r)
        polls += 1
    return wm


# ---------------------------------------------------------------------------
# stream-stream join (Stream.joinStream)
# ---------------------------------------------------------------------------
def join_stream_rows(before_ms: int, after_ms: int, records, f1: str, f2: str):
    """joinStreamProcessor (Stream.hs:267-300) over both streams' records in
    arrival order, one at a time on the host: what joinStream forwards, as
    (index of this side's record, index of the other side's, timestamp) in
    forwarding order. Each record is {"side": 0 | 1, "key": record key or None,
    "value": object, "timestamp": ts}; the join key is value[f1] (side 0) or
    value[f2] (side 1). A record without a key is dropped before it is stored
    (fromJust, :283); the range over the other store includes its end points
    only when that store holds both end timestamps (tksRange, Store.hs:355-372);
    a missing join field on either side ends the record's scan at that
    candidate (the key selector throws, Codegen.hs:242-244). Pure: no GPU."""
    import bisect
    stores = [dict(), dict()]   # side -> ts -> {canonical key: record index}
    tls = [[], []]              # side -> sorted timestamps held
    fields = (f1, f2)
    out = []
    for i, r in enumerate(records):
        if r.get("key") is None:
            continue
        side, ts, key = int(r["side"]), int(r["timestamp"]), _canon(r["key"])
        st = stores[side]
        if ts not in st:
            st[ts] = {}
            bisect.insort(tls[side], ts)
        st[ts][key] = i
        b, a = (before_ms, after_ms) if side == 0 else (after_ms, before_ms)
        lo, hi = ts - b, ts + a
        ost, tl = stores[1 - side], tls[1 - side]
        if lo in ost and hi > lo and hi in ost:
            i0, i1 = bisect.bisect_left(tl, lo), bisect.bisect_right(tl, hi)
        else:
            i0, i1 = bisect.bisect_right(tl, lo), bisect.bisect_left(tl, hi)
        for t in tl[i0:i1]:
            k = ost[t].get(key)
            if k is None:
                continue
            mine, theirs = r["value"], records[k]["value"]
            if fields[side] not in mine or fields[1 - side] not in theirs:
                break
            if _canon(mine[fields[side]]) == _canon(theirs[fields[1 - side]]):
                out.append((i, k, max(ts, t)) if side == 0 else (k, i, max(ts, t)))
    return out


class JoinedStream:
    """Stream.joinStream (Stream.hs:222-250) with the SQL plan's joiner
    (genJoiner: the union of both values under "s1.f" / "s2.g"), backed by one
    valued GPU join: the join keeps the named numeric fields of every record in
    HBM and drains the joined records as columns.

    process(records) runs one poll batch of both streams' records ({"stream":
    s1 | s2 (or "side": 0 | 1), "key": record key or None, "value": object,
    "timestamp": ts}) and returns the joined records as the reference forwards
    them: {"key": {"SelectedKey": join key}, "value": {"s1.f": ..., "s2.g":
    ...}, "timestamp": max of the two}. The value holds the named fields only.
    process_into(records, op) leaves the joined batch on the device and pushes
    it into a Table's / Stream's op whose fields are `names`."""

    def __init__(self, engine, s1, s2, f1, f2, fields1, fields2, before_ms, after_ms, batch_capacity=1 << 20,
                 keys=None, join_keys=None):
        from .join import Join
        norm = lambda fs: [(f, False) if isinstance(f, str) else (f[0], bool(f[1])) for f in fs]
        self.s = (s1, s2)
        self.f = (f1, f2)
        self.fields = (norm(fields1), norm(fields2))
        self.names = [f"{s1}.{f}" for f, _ in self.fields[0]] + [f"{s2}.{f}" for f, _ in self.fields[1]]
        self.float_names = [n for n, (_, fl) in zip(self.names, self.fields[0] + self.fields[1]) if fl]
        self.keys = keys if keys is not None else KeyDict()                  # record keys
        self.join_keys = join_keys if join_keys is not None else KeyDict()   # join keys: a drained batch's key_id
        self.join = Join(engine, before_ms, after_ms, batch_capacity,
                         cols=tuple([abi.HSG_F64 if fl else abi.HSG_I64 for _, fl in fs] for fs in self.fields))

    def _side(self, rec):
        if "side" in rec:
            return int(rec["side"])
        if self.s[0] == self.s[1]:
            raise ValueError("a self-join's records name their side: {'side': 0 | 1}")
        return 0 if rec["stream"] == self.s[0] else 1

    def columns(self, records):
        """The poll batch as the arrays of Join.push: side, record key id, join
        key id, ts, value columns (the wider side's count; int64 storage, an f64
        field's bits) and their valid bytes. A present value that is no Number
        raises ValueError: the join carries numeric columns only."""
        n = len(records)
        vc = max(len(self.fields[0]), len(self.fields[1]))
        side = np.zeros(n, np.uint8)
        key = np.full(n, abi.HSG_KEY_NONE, np.uint32)
        jkey = np.full(n, abi.HSG_KEY_NONE, np.uint32)
        ts = np.empty(n, np.int64)
        cols = [np.zeros(n, np.int64) for _ in range(vc)]
        valid = [np.zeros(n, np.uint8) for _ in range(vc)]
        for i, rec in enumerate(records):
            sd = side[i] = self._side(rec)
            value = rec["value"]
            ts[i] = rec["timestamp"]
            if rec.get("key") is not None:
                key[i] = self.keys.encode(rec["key"])
            if self.f[sd] in value:
                jkey[i] = self.join_keys.encode(value[self.f[sd]])
            for c, (f, fl) in enumerate(self.fields[sd]):
                if f not in value:
                    continue
                v = value[f]
                if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                    raise ValueError(f"field {f}: the GPU join carries numeric columns only")
                if fl:
                    cols[c][i:i + 1].view(np.float64)[0] = float(v)
                else:
                    cols[c][i] = int(v)
                valid[c][i] = 1
        return side, key, jkey, ts, cols, valid

    def push(self, records):
        side, key, jkey, ts, cols, valid = self.columns(records)
        self.join.push(side, key, jkey, ts, cols=cols, valid=valid)

    def process(self, records):
        self.push(records)
        b = self.join.drain_batch(optional=("valid",))
        s1, s2 = self.s
        names = [(f"{s1}.{f}", 0) for f, _ in self.fields[0]] + [(f"{s2}.{f}", 1) for f, _ in self.fields[1]]
        out = []
        for i in range(len(b.ts)):
            value = {}
            for c in reversed(range(len(names))):  # (left-biased union: this side's value is written last)
                if b.valid[c][i] & 1:
                    value[names[c][0]] = b.cols[c][i].item()
            out.append({"key": {"SelectedKey": self.join_keys.decode(int(b.key_id[i]))},
                        "value": {nm: value[nm] for nm, _ in names if nm in value}, "timestamp": int(b.ts[i])})
        return out

    def process_into(self, records, target, key_col=None, watermark=-1):
        """One poll batch through the join and its joined rows, still on the
        device, into `target`: a Table (gen_group_by_node) or a Stream
        (gen_select_node) whose fields are among `names`; its op reads the
        drained tensors in place (HSG_MEM_DEVICE), each of its columns the
        joined column of that name. The group key of a Table: its key field
        names a joined i64 column, whose value is the key id (a key outside
        0 .. 2^32 - 2 or absent is HSG_KEY_NONE: the reference drops such a
        record too, getFieldByName throws); key_col = -1 groups by the join
        key instead, as ids of join_keys. Returns the stream time; the rows
        wait in target.op (drain)."""
        fields = target.fields
        index = []
        for f, fl in fields:
            if f not in self.names:
                raise ValueError(f"{f} is not a column of the joined stream {self.names}")
            index.append(self.names.index(f))
            if fl != (f in self.float_names):
                raise ValueError(f"{f}: the joined column and the target's field differ in type")
        if key_col is None:
            key_col = -1
            if isinstance(target, Table):
                kf = target.grouped.key_field
                if kf not in self.names or kf in self.float_names:
                    raise ValueError(f"GROUP BY {kf}: not an i64 column of the joined stream")
                key_col = self.names.index(kf)
        self.push(records)
        b = self.join.drain_batch(key_col=key_col, device=True, optional=("valid",))
        return target.op.push(b.key_id, b.ts, [b.cols[k] for k in index], [b.valid[k] for k in index],
                              watermark=watermark)

    def close(self):
        self.join.close()


def joinStream(engine, s1, s2, f1, f2, fields1, fields2, before_ms, after_ms, batch_capacity=1 << 20,
               keys=None, join_keys=None) -> JoinedStream:
    """Stream.joinStream (Stream.hs:222-250) as the SQL plan calls it
    (Codegen.hs:259-266): stream s1 joined with s2 on s1.f1 = s2.f2 within
    [ts - before_ms, ts + after_ms], the joiner being genJoiner over the named
    numeric fields of each side. See JoinedStream."""
    return JoinedStream(engine, s1, s2, f1, f2, fields1, fields2, before_ms, after_ms, batch_capacity, keys, join_keys)
