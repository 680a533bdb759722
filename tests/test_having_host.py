"""CPU: the HAVING program's host side -- hsg_having_check's accept / reject
table and the static typing of the aggregate outputs, compile_having over the
aliases, the hsg_stats layout (old offsets fixed, the two new fields last and
mirrored), and what gen_group_by_node does with having= by window kind."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import pytest

from hstream_amd import abi, engine, processing as P, sql
from hstream_amd.abi import (HSG_W_ADD, HSG_W_AND, HSG_W_BETWEEN, HSG_W_COL, HSG_W_EQ, HSG_W_F64, HSG_W_GT, HSG_W_I64,
                             HSG_W_LT, HSG_W_MUL, HSG_W_NOT)
from hstream_amd.columnar import OpSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64, F64 = abi.HSG_I64, abi.HSG_F64
CA, CN, S, MN, MX, AV, L = (abi.HSG_COUNT_ALL, abi.HSG_COUNT, abi.HSG_SUM, abi.HSG_MIN, abi.HSG_MAX, abi.HSG_AVG,
                            abi.HSG_LAST)
# outputs: 0 COUNT(*) i64, 1 SUM(a) i64, 2 MAX(b) f64, 3 COUNT(b) i64, 4 AVG(a) f64
SPEC = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[I64, F64],
              aggs=[(CA, 0), (S, 0), (MX, 1), (CN, 1), (AV, 0)])


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        from hstream_amd import build
        build.build()
    return engine.load_library()


def _gt(c, k):
    return [(HSG_W_COL, c), (HSG_W_I64, k), (HSG_W_GT,)]


ACCEPT = {
    "cnt > 1": _gt(0, 1),
    "cnt > 1 AND mx > 2.5": _gt(0, 1) + [(HSG_W_COL, 2), (HSG_W_F64, 2.5), (HSG_W_GT,), (HSG_W_AND,)],
    "NOT (s + cnt) * 2 < avg": [(HSG_W_COL, 1), (HSG_W_COL, 0), (HSG_W_ADD,), (HSG_W_I64, 2), (HSG_W_MUL,), (HSG_W_COL, 4),
                                (HSG_W_LT,), (HSG_W_NOT,)],
    "s BETWEEN cnt AND mx": [(HSG_W_COL, 0), (HSG_W_COL, 1), (HSG_W_COL, 2), (HSG_W_BETWEEN,)],
    "the last output": _gt(4, 0),
    "depth 8": [(HSG_W_COL, 0)] * 8 + [(HSG_W_ADD,)] * 7 + [(HSG_W_I64, 0), (HSG_W_GT,)],
}

REJECT = {
    "column = n_aggs": (_gt(5, 1), "column 5 out of range"),
    "a value column's number past the outputs": (_gt(16, 1), "out of range"),
    "negative column": (_gt(-1, 1), "out of range"),
    "value left on the stack": ([(HSG_W_COL, 0), (HSG_W_I64, 1), (HSG_W_ADD,)], "leaves a value"),
    "two results": (_gt(0, 1) + _gt(1, 1), "2 results"),
    "depth 9": ([(HSG_W_COL, 0)] * 9 + [(HSG_W_ADD,)] * 8 + [(HSG_W_I64, 0), (HSG_W_GT,)], "deeper than 8"),
    "nan constant": ([(HSG_W_COL, 2), (HSG_W_F64, math.nan), (HSG_W_LT,)], "not finite"),
    "inf constant": ([(HSG_W_COL, 2), (HSG_W_F64, math.inf), (HSG_W_LT,)], "not finite"),
    "empty": ([], "program length 0"),
    "65 instructions": (_gt(0, 1) + [(HSG_W_NOT,)] * 62, "program length 65"),
}


@pytest.mark.parametrize("name", list(ACCEPT))
def test_having_check_accepts(lib, name):
    assert engine.having_check(ACCEPT[name], SPEC) == (abi.HSG_OK, ""), name


@pytest.mark.parametrize("name", list(REJECT))
def test_having_check_rejects(lib, name):
    prog, part = REJECT[name]
    rc, msg = engine.having_check(prog, SPEC)
    assert rc == abi.HSG_E_INVALID, name
    assert msg.startswith("having: ") and part in msg, (name, msg)


def test_having_check_ranges_over_sixteen_outputs(lib):
    """COL ranges over [0, n_aggs), past the eight value columns a WHERE can name."""
    wide = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[I64] * 8,
                  aggs=[(S, c) for c in range(8)] + [(MX, c) for c in range(8)])
    assert engine.having_check(_gt(15, 0), wide) == (abi.HSG_OK, "")
    rc, msg = engine.having_check(_gt(16, 0), wide)
    assert rc == abi.HSG_E_INVALID and "column 16 out of range" in msg


def test_having_types_are_static(lib):
    """No program is accepted under one typing of an output and refused under
    the other (both kinds are values), so hsg_having_check's typing is read
    from its error text: a program that leaves a value is refused with that
    value's static type. COUNT(*) / COUNT -> i64 (over an f64 column too),
    AVG -> f64 (over an i64 column too), SUM / MIN / MAX / LAST -> the
    column's; i64 with i64 stays i64, anything with an f64 is f64."""
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[I64, F64],
                  aggs=[(CA, 0), (CN, 1), (AV, 0), (S, 0), (S, 1), (MN, 1), (MX, 0), (L, 1)])
    want = [False, False, True, False, True, True, False, True]
    assert spec.agg_is_f64() == want  # the mirror every row decoder uses agrees

    def typed(prog):
        rc, msg = engine.having_check(prog, spec)
        assert rc == abi.HSG_E_INVALID and "leaves a value" in msg, msg
        assert ("(an f64 value)" in msg) != ("(an i64 value)" in msg), msg
        return "(an f64 value)" in msg

    for c in range(8):
        assert typed([(HSG_W_COL, c)]) == want[c], c
        assert engine.having_check(_gt(c, 0), spec) == (abi.HSG_OK, "")
    assert not typed([(HSG_W_COL, 0), (HSG_W_COL, 1), (HSG_W_ADD,)])   # COUNT(*) + COUNT(b)
    assert typed([(HSG_W_COL, 0), (HSG_W_COL, 2), (HSG_W_MUL,)])       # COUNT(*) * AVG(a)
    assert typed([(HSG_W_COL, 3), (HSG_W_F64, 1.0), (HSG_W_ADD,)]) and not typed([(HSG_W_COL, 3), (HSG_W_I64, 1),
                                                                                  (HSG_W_ADD,)])
    # a config the op itself refuses is refused here too (the types come from it)
    bad = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[I64], aggs=[(S, 3)])
    rc, msg = engine.having_check(_gt(0, 0), bad)
    assert rc == abi.HSG_E_INVALID and "aggregate column out of range" in msg


def test_having_check_cuts_the_message_to_the_buffer(lib):
    prog, n = abi.where_array(REJECT["column = n_aggs"][0])
    cfg, keep = SPEC.to_config()
    buf = C.create_string_buffer(b"x" * 16, 16)
    assert lib.hsg_having_check(prog, n, C.byref(cfg), buf, 9) == abi.HSG_E_INVALID
    assert buf.raw[:9] == b"having: \0" and buf.raw[9:] == b"x" * 7
    assert lib.hsg_having_check(prog, n, C.byref(cfg), None, 0) == abi.HSG_E_INVALID


def test_tile_accessor(lib):
    t = engine.having_tile_rows()
    assert t >= 64 and t % 64 == 0


# ---- compile_having -----------------------------------------------------------------
def col(f):
    return sql.RExprCol(f, None, f)


def const(c):
    return sql.RExprConst(str(c), c)


def gt(l, r):
    return sql.RCondOp("RCompOpGT", l, r)


def test_compile_having_maps_aliases_to_aggregates(lib):
    aggs = sql.gen_aggregate_components([("SUM", "a"), ("COUNT(*)", "result"), ("COL", "b"), ("AVG", "a", "mean")])
    assert [a.alias for a in aggs] == ["SUM(a)", "result", "b", "mean"]
    assert sql.compile_having(gt(col("result"), const(2)), aggs) == _gt(1, 2)
    cond = sql.RCondAnd(gt(col("SUM(a)"), const(10)), sql.RCondBetween(const(0.5), col("mean"), col("b")))
    prog = sql.compile_having(cond, aggs)
    assert prog == _gt(0, 10) + [(HSG_W_F64, 0.5), (HSG_W_COL, 3), (HSG_W_COL, 2), (HSG_W_BETWEEN,), (HSG_W_AND,)]
    # the group key is nameable where it is a SELECT passthrough: no key-field rule
    assert sql.compile_having(sql.RCondOp("RCompOpEQ", col("b"), const(1)), aggs) == [(HSG_W_COL, 2), (HSG_W_I64, 1),
                                                                                      (HSG_W_EQ,)]
    # plain alias strings work as well
    assert sql.compile_having(gt(col("y"), const(0)), ["x", "y"]) == _gt(1, 0)


def test_compile_having_raises():
    aggs = sql.gen_aggregate_components([("SUM", "a", "s"), ("COUNT(*)", "cnt")])
    with pytest.raises(ValueError, match="alias"):
        sql.compile_having(gt(col("a"), const(0)), aggs)  # a field, not an alias
    with pytest.raises(ValueError, match="alias"):
        sql.compile_having(gt(col("SUM(a)"), const(0)), aggs)  # the aggregate was renamed
    dup = sql.gen_aggregate_components([("SUM", "a", "x"), ("COUNT(*)", "x")])
    with pytest.raises(ValueError, match="duplicate"):
        sql.compile_having(gt(col("x"), const(0)), dup)
    with pytest.raises(ValueError):
        sql.compile_having(gt(col("s"), const("text")), aggs)
    with pytest.raises(ValueError):
        sql.compile_having(gt(sql.RExprUnaryOp("ABS(s)", "OpAbs", col("s")), const(0)), aggs)


# ---- hsg_stats: old offsets fixed, the new fields last ---------------------------------
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "hstream_gpu.h"
#define F(f) printf(#f " %zu\n", offsetof(hsg_stats, f))
int main(void) {
  F(batches); F(records); F(records_owned); F(pairs); F(late_dropped); F(touched); F(state_rows); F(pending_rows);
  F(last_batch_ms); F(agg_kernel_ms); F(agg_kernel_launches); F(exchange_ms); F(exchange_bytes); F(pairs_total);
  F(touched_total); F(state_slots); F(state_row_bytes); F(spilled_rows); F(spill_events); F(table_slots);
  F(grow_events); F(lean_batches); F(direct_batches); F(replays); F(overflow_rows); F(overflow_rebuilds);
  F(where_dropped); F(where_dropped_total); F(having_dropped); F(having_dropped_total);
  printf("size %zu\n", sizeof(hsg_stats));
  return 0;
}
"""

# the fields as they were before HAVING, 8 bytes each, in order
OLD_FIELDS = ["batches", "records", "records_owned", "pairs", "late_dropped", "touched", "state_rows", "pending_rows",
              "last_batch_ms", "agg_kernel_ms", "agg_kernel_launches", "exchange_ms", "exchange_bytes", "pairs_total",
              "touched_total", "state_slots", "state_row_bytes", "spilled_rows", "spill_events", "table_slots",
              "grow_events", "lean_batches", "direct_batches", "replays", "overflow_rows", "overflow_rebuilds",
              "where_dropped", "where_dropped_total"]


def test_stats_layout():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write(LAYOUT_C)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        got = {k: int(v) for k, v in (ln.split(" ") for ln in subprocess.check_output([exe]).decode().strip().split("\n"))}
    for i, name in enumerate(OLD_FIELDS):
        assert got[name] == 8 * i == getattr(abi.hsg_stats, name).offset, name
    assert got["having_dropped"] == 8 * len(OLD_FIELDS) == abi.hsg_stats.having_dropped.offset
    assert got["having_dropped_total"] == 8 * len(OLD_FIELDS) + 8 == abi.hsg_stats.having_dropped_total.offset
    assert got["size"] == 8 * len(OLD_FIELDS) + 16 == C.sizeof(abi.hsg_stats)
    assert [n for n, _ in abi.hsg_stats._fields_][-2:] == ["having_dropped", "having_dropped_total"]
    assert {"hsg_having_check", "hsg_op_create_filtered"} <= set(abi.EXPORTED_SYMBOLS)


# ---- gen_group_by_node: having by window kind -------------------------------------------
class _NoEngine:
    """Table builds its op at once; this one only records the spec."""

    def op(self, spec):
        self.spec = spec
        return None


SEL = [("SUM", "a"), ("COUNT(*)", "result"), ("COL", "b")]
HAV = gt(col("result"), const(2))


def test_group_by_node_passes_having_for_an_unwindowed_query():
    eng = _NoEngine()
    t = sql.gen_group_by_node(eng, SEL, sql.RGroupBy("b"), having=HAV)
    assert eng.spec.window_kind == abi.HSG_UNWINDOWED
    assert eng.spec.having == _gt(1, 2) and eng.spec.where is None
    assert isinstance(t.having, P.Having)
    # with a WHERE beside it: both programs, each over its own columns
    sql.gen_group_by_node(eng, SEL, sql.RGroupBy("b"), where=gt(col("a"), const(0)), having=HAV)
    assert eng.spec.where == _gt(0, 0) and eng.spec.having == _gt(1, 2)
    # none given: none set
    sql.gen_group_by_node(eng, SEL, sql.RGroupBy("b"))
    assert eng.spec.having is None
    # a HAVING the program cannot say raises: it is not pushed down
    with pytest.raises(ValueError):
        sql.gen_group_by_node(eng, SEL, sql.RGroupBy("b"), having=gt(col("nope"), const(0)))


@pytest.mark.parametrize("window", [sql.RTumblingWindow(10), sql.RHoppingWindow(30, 10), sql.RSessionWindow(5)],
                         ids=["tumbling", "hopping", "session"])
def test_group_by_node_ignores_having_for_a_windowed_query(window):
    eng = _NoEngine()
    sel = [("SUM", "a"), ("COUNT(*)", "result")]
    t = sql.gen_group_by_node(eng, sel, sql.RGroupBy("b", window), having=HAV)
    assert eng.spec.window_kind != abi.HSG_UNWINDOWED and eng.spec.having is None and t.having is None
    # even one that names no alias: the reference never looks at it
    sql.gen_group_by_node(eng, sel, sql.RGroupBy("b", window), having=gt(col("nope"), const(0)))
    assert eng.spec.having is None


def test_group_by_node_drops_having_for_emit_none():
    eng = _NoEngine()
    sql.gen_group_by_node(eng, SEL, sql.RGroupBy("b"), emit=abi.HSG_EMIT_NONE, having=HAV)
    assert eng.spec.having is None


def test_dsl_aggregate_methods_take_having():
    eng = _NoEngine()
    aggs = [P.COUNT_ALL("cnt"), P.SUM("a", "s")]
    g = P.groupBy(eng, "k")
    hv = P.Having(gt(col("cnt"), const(1)))
    g.aggregate(aggs, P.Materialized(), having=hv)
    assert eng.spec.having == _gt(0, 1)
    g.timeWindowedBy(P.mkTumblingWindow(1000)).aggregate(aggs, P.Materialized(), having=hv)
    assert eng.spec.having == _gt(0, 1) and eng.spec.window_kind == abi.HSG_TUMBLING
    g.sessionWindowedBy(P.mkSessionWindows(1000)).aggregate(aggs, P.Materialized(), having=hv)
    assert eng.spec.having == _gt(0, 1) and eng.spec.window_kind == abi.HSG_SESSION
