"""CPU: the host side of computed columns -- hsg_map_check's accept / reject
table and the static typing of the expressions, the limits at their edges,
sql.compile_expr / gen_aggregate_components over expression trees, that
compile_where still refuses what it refused, and the layouts of hsg_map_expr
and hsg_map_stats against the header (hsg_stats keeps its size)."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import pytest

from hstream_amd import abi, engine, processing as P, sql
from hstream_amd.abi import (HSG_W_ADD, HSG_W_AND, HSG_W_COL, HSG_W_F64, HSG_W_GT, HSG_W_I64, HSG_W_MUL, HSG_W_NOT,
                             HSG_W_SUB)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64, F64 = abi.HSG_I64, abi.HSG_F64
TYPES = [I64, F64, I64]  # a, b, c


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        from hstream_amd import build
        build.build()
    return engine.load_library()


def col(name):
    return sql.RExprCol(name, None, name)


def const(c):
    return sql.RExprConst(str(c), c)


def binop(op, a, b):
    sym = {"OpAdd": "+", "OpSub": "-", "OpMul": "*"}.get(op, op)
    return sql.RExprBinOp(f"({a.name}{sym}{b.name})", op, a, b)


A_PLUS_C = [(HSG_W_COL, 0), (HSG_W_COL, 2), (HSG_W_ADD,)]
A_TIMES_B = [(HSG_W_COL, 0), (HSG_W_COL, 1), (HSG_W_MUL,)]
DEPTH8 = [(HSG_W_COL, 0)] * 8 + [(HSG_W_ADD,)] * 7
DEPTH9 = [(HSG_W_COL, 0)] * 9 + [(HSG_W_ADD,)] * 8


# ---- hsg_map_check ---------------------------------------------------------------------
def test_out_types(lib):
    exprs = [A_PLUS_C, A_TIMES_B, [(HSG_W_COL, 1)], [(HSG_W_COL, 2)], [(HSG_W_I64, 7)], [(HSG_W_F64, 2.0)],
             [(HSG_W_COL, 0), (HSG_W_F64, 0.5), (HSG_W_MUL,)], abi.MapExpr(DEPTH8, abi.HSG_MAP_STRICT)]
    rc, msg, types = engine.map_check(exprs, TYPES)
    assert rc == abi.HSG_OK, msg
    assert types == [I64, F64, F64, I64, I64, F64, F64, I64]
    # the Python mirror types them alike
    assert [abi.map_expr_type(e, TYPES) for e in exprs] == types


REJECT = {
    "comparison": ([A_PLUS_C + [(HSG_W_I64, 1), (HSG_W_GT,)]], "map: expr 0: ", "not a value instruction"),
    "logic": ([A_PLUS_C, [(HSG_W_COL, 0), (HSG_W_NOT,)]], "map: expr 1: ", "not a value instruction"),
    "bad opcode": ([[(99,)]], "map: expr 0: ", "not a value instruction"),
    "two values": ([[(HSG_W_COL, 0), (HSG_W_COL, 2)]], "map: expr 0: ", "2 values left"),
    "underflow": ([[(HSG_W_COL, 0), (HSG_W_ADD,)]], "map: expr 0: ", "underflow"),
    "empty": ([A_PLUS_C, []], "map: expr 1: ", "program length 0"),
    "depth 9": ([DEPTH9], "map: expr 0: ", "deeper than 8"),
    "column = n_cols": ([[(HSG_W_COL, 3)]], "map: expr 0: ", "column 3 out of range"),
    "negative column": ([A_PLUS_C, A_PLUS_C, [(HSG_W_COL, -1)]], "map: expr 2: ", "out of range"),
    "nan": ([[(HSG_W_F64, math.nan)]], "map: expr 0: ", "not finite"),
    "inf": ([[(HSG_W_COL, 1), (HSG_W_F64, -math.inf), (HSG_W_SUB,)]], "map: expr 0: ", "not finite"),
    "bad flags": ([abi.MapExpr(A_PLUS_C, 2)], "map: expr 0: ", "bad flags"),
}


@pytest.mark.parametrize("name", sorted(REJECT))
def test_refusals(lib, name):
    exprs, prefix, what = REJECT[name]
    rc, msg, _ = engine.map_check(exprs, TYPES)
    assert rc == abi.HSG_E_INVALID
    assert msg.startswith(prefix) and what in msg, msg


def test_a_program_of_two_instructions_is_not_taken_for_a_pair(lib):
    """A bare program is a program whatever its shape; flags come with abi.MapExpr alone."""
    two = [(HSG_W_I64, 1), (HSG_W_I64, 2)]
    rc, msg, _ = engine.map_check([two], TYPES)
    assert rc == abi.HSG_E_INVALID and "2 values left" in msg
    arr, n, _keep = abi.map_array([abi.MapExpr(A_PLUS_C, True), A_PLUS_C])
    assert n == 2 and (arr[0].n, arr[0].flags, arr[1].n, arr[1].flags) == (3, 1, 3, 0)


def test_grid_threads_come_from_the_library(lib):
    n = engine.map_grid_threads()
    assert n > 0 and n % 256 == 0


def test_limits_at_their_edges(lib):
    # 8 expressions pass, 9 do not; none neither
    assert engine.map_check([[(HSG_W_COL, 0)]] * 8, TYPES)[0] == abi.HSG_OK
    rc, msg, _ = engine.map_check([[(HSG_W_COL, 0)]] * 9, TYPES)
    assert rc == abi.HSG_E_INVALID and msg.startswith("map: ") and "9 expressions" in msg
    rc, msg, _ = engine.map_check([], TYPES)
    assert rc == abi.HSG_E_INVALID and msg.startswith("map: ")
    # 64 instructions in all pass (4 x 15 + 4), 65 do not
    assert engine.map_check([DEPTH8] * 4 + [[(HSG_W_COL, 0)]] * 4, TYPES)[0] == abi.HSG_OK
    rc, msg, _ = engine.map_check([DEPTH8] * 4 + [[(HSG_W_COL, 0)]] * 3 + [[(HSG_W_COL, 0), (HSG_W_I64, 1), (HSG_W_ADD,)]],
                                  TYPES)
    assert rc == abi.HSG_E_INVALID and msg.startswith("map: expr 7: ") and "66 instructions" in msg
    one64 = [(HSG_W_COL, 0)] + [(HSG_W_I64, 1), (HSG_W_ADD,)] * 31 + [(HSG_W_COL, 2)]
    assert len(one64) == 64
    rc, msg, _ = engine.map_check([one64 + [(HSG_W_ADD,)]], TYPES)
    assert rc == abi.HSG_E_INVALID and "program length 65" in msg
    # 63 + 1 = 64 in two expressions pass, 63 + 2 = 65 do not
    e63 = [(HSG_W_COL, 0)] + [(HSG_W_I64, 1), (HSG_W_ADD,)] * 31
    assert engine.map_check([e63, [(HSG_W_COL, 2)]], TYPES)[0] == abi.HSG_OK
    rc, msg, _ = engine.map_check([e63, [(HSG_W_COL, 2), (HSG_W_COL, 0)]], TYPES)
    assert rc == abi.HSG_E_INVALID and msg.startswith("map: expr 1: ") and "65 instructions" in msg


# ---- sql.compile_expr / gen_aggregate_components ---------------------------------------
def test_compile_expr_postfix_order_and_depth():
    a, b, c = col("a"), col("b"), col("c")
    e = binop("OpSub", binop("OpMul", a, c), b)  # a*c-b
    assert sql.compile_expr(e, ["a", "b", "c"]) == [(HSG_W_COL, 0), (HSG_W_COL, 2), (HSG_W_MUL,), (HSG_W_COL, 1),
                                                    (HSG_W_SUB,)]
    e = binop("OpMul", a, binop("OpAdd", b, const(0.25)))  # right-nested: the depth grows
    assert sql.compile_expr(e, ["a", "b"]) == [(HSG_W_COL, 0), (HSG_W_COL, 1), (HSG_W_F64, 0.25), (HSG_W_ADD,),
                                               (HSG_W_MUL,)]
    assert sql.compile_expr(const(3), []) == [(HSG_W_I64, 3)]
    # right-nested to depth 8 passes, depth 9 does not
    def nest(k):
        e = a
        for _ in range(k - 1):
            e = binop("OpAdd", a, e)
        return e
    assert len(sql.compile_expr(nest(8), ["a"])) == 15
    with pytest.raises(ValueError, match="stack of 9"):
        sql.compile_expr(nest(9), ["a"])
    # left-nested needs 2 however long; past 64 instructions it is refused
    e = a
    for _ in range(31):
        e = binop("OpAdd", e, a)
    assert len(sql.compile_expr(e, ["a"])) == 63
    with pytest.raises(ValueError, match="65 instructions"):
        sql.compile_expr(binop("OpAdd", e, a), ["a"])


def test_compile_expr_refuses_what_where_refuses():
    a = col("a")
    for bad in (sql.RExprUnaryOp("ABS(a)", "OpAbs", a), binop("OpDiv", a, a), binop("OpAdd", a, const("x")),
                binop("OpAdd", a, const(True)), binop("OpAdd", a, const(None)), binop("OpAdd", a, const(math.inf)),
                binop("OpAdd", a, const(2**63)), binop("OpAdd", a, col("nope"))):
        with pytest.raises(ValueError):
            sql.compile_expr(bad, ["a"])
    with pytest.raises(ValueError, match="group key"):
        sql.compile_expr(binop("OpAdd", a, col("k")), ["a", "k"], key_field="k")


def test_expr_value_is_the_exact_reference():
    e = binop("OpSub", binop("OpMul", col("a"), col("c")), col("b"))
    assert sql.expr_value(e, {"a": 3, "b": 0.25, "c": -2}) == sql._expr_value(e, {"a": 3, "b": 0.25, "c": -2}) == -6.25
    with pytest.raises(KeyError):
        sql.expr_value(e, {"a": 3, "c": 1})


class _NoEngine:
    def op(self, spec):
        self.spec = spec
        return None


def test_aggregate_components_over_expressions():
    a, b, c = col("a"), col("b"), col("c")
    ac = binop("OpMul", a, c)
    aggs = sql.gen_aggregate_components([("COL", a), ("SUM", ac), ("COUNT(*)",), ("COL", binop("OpAdd", a, b), "s"),
                                         ("AVG", binop("OpMul", b, const(0.01)))], float_fields=("b",))
    # a tree that is just a column is the plain path
    assert aggs[0] == P.LAST("a", "a", False)
    assert isinstance(aggs[1].field, P.Expr) and aggs[1].name == "SUM((a*c))" and not aggs[1].is_float and not aggs[1].strict
    assert aggs[3].name == "s" and aggs[3].is_float and aggs[3].strict and aggs[3].kind == abi.HSG_LAST
    assert aggs[4].is_float and not aggs[4].strict and aggs[4].name == "AVG((b*0.01))"
    # plain SELECT lists are what they were
    assert sql.gen_aggregate_components([("SUM", "a"), ("COL", "b")], ("b",)) == [P.SUM("a", "SUM(a)", False),
                                                                                 P.LAST("b", "b", True)]
    with pytest.raises(ValueError, match="unary"):
        sql.gen_aggregate_components([("SUM", sql.RExprUnaryOp("ABS(a)", "OpAbs", a))])
    with pytest.raises(ValueError, match="group key"):
        sql.gen_aggregate_components([("SUM", binop("OpAdd", a, col("k")))], key_field="k")


def test_group_by_node_builds_the_map():
    a, b, c = col("a"), col("b"), col("c")
    eng = _NoEngine()
    sel = [("COL", "a"), ("SUM", binop("OpMul", a, c)), ("COUNT(*)",), ("COL", binop("OpAdd", a, b), "s")]
    t = sql.gen_group_by_node(eng, sel, sql.RGroupBy("k"), float_fields=("b",),
                              where=sql.RCondOp("RCompOpGT", col("d"), const(0)))
    # batch columns: a (bare), then what the expressions read, then what only WHERE reads
    assert [f for f, _ in t.fields] == ["a", "c", "b", "d"] and t.numeric == [True] * 4
    assert list(eng.spec.col_types) == [I64, I64, F64, I64]
    # a bare column inside a mapped SELECT is a one-instruction program, not strict
    assert eng.spec.map == [abi.MapExpr([(HSG_W_COL, 0)]), abi.MapExpr([(HSG_W_COL, 0), (HSG_W_COL, 1), (HSG_W_MUL,)]),
                            abi.MapExpr([(HSG_W_COL, 0), (HSG_W_COL, 2), (HSG_W_ADD,)], abi.HSG_MAP_STRICT)]
    assert all(isinstance(e, abi.MapExpr) for e in eng.spec.map)
    assert list(eng.spec.aggs) == [(abi.HSG_LAST, 0), (abi.HSG_SUM, 1), (abi.HSG_COUNT_ALL, 0), (abi.HSG_LAST, 2)]
    assert eng.spec.where == [(HSG_W_COL, 3), (HSG_W_I64, 0), (HSG_W_GT,)]
    assert eng.spec.agg_is_f64() == [False, False, False, True]
    # no expression: no map, the spec it always was
    sql.gen_group_by_node(eng, [("SUM", "a"), ("COL", "b")], sql.RGroupBy("k"), float_fields=("b",))
    assert eng.spec.map is None and list(eng.spec.aggs) == [(abi.HSG_SUM, 0), (abi.HSG_LAST, 1)]
    # a SELECT expression over the key stays on the host
    with pytest.raises(ValueError, match="group key"):
        sql.gen_group_by_node(eng, [("SUM", binop("OpAdd", a, col("k")))], sql.RGroupBy("k"))


def test_compile_where_refuses_what_it_refused():
    a = col("a")
    gt = lambda x, y: sql.RCondOp("RCompOpGT", x, y)
    assert sql.compile_where(gt(binop("OpAdd", a, const(1)), const(2.5)), ["a"]) == [
        (HSG_W_COL, 0), (HSG_W_I64, 1), (HSG_W_ADD,), (HSG_W_F64, 2.5), (HSG_W_GT,)]
    for bad in (gt(sql.RExprUnaryOp("ABS(a)", "OpAbs", a), const(0)), gt(a, const("x")), gt(a, const(True)),
                gt(a, const(None)), gt(a, const(math.nan)), gt(a, const(2**63)), gt(binop("OpDiv", a, a), const(0)),
                gt(col("nope"), const(0)), sql.RCondOp("RCompOpLike", a, const(0)), a):
        with pytest.raises(ValueError):
            sql.compile_where(bad, ["a"])
    with pytest.raises(ValueError, match="group key"):
        sql.compile_where(gt(col("k"), const(0)), ["a", "k"], key_field="k")
    with pytest.raises(ValueError, match="not a value column"):
        sql.compile_where(gt(col("z"), const(0)), ["a"])
    with pytest.raises(ValueError, match="alias"):
        sql.compile_where(gt(col("z"), const(0)), ["a"], what="HAVING")
    deep = a
    for _ in range(8):
        deep = binop("OpAdd", a, deep)
    with pytest.raises(ValueError, match="stack of 9"):
        sql.compile_where(gt(deep, const(0)), ["a"])
    long = gt(a, const(0))
    for _ in range(16):
        long = sql.RCondAnd(long, gt(a, const(0)))
    with pytest.raises(ValueError, match="67 instructions"):
        sql.compile_where(long, ["a"])


# ---- layouts: the header and abi.py agree; hsg_stats did not grow -------------------------
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "hstream_gpu.h"
#define F(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void) {
  F(hsg_map_expr, prog); F(hsg_map_expr, n); F(hsg_map_expr, flags);
  F(hsg_map_stats, map_dropped); F(hsg_map_stats, map_dropped_total); F(hsg_map_stats, computed_cols);
  F(hsg_map_stats, aliased_cols);
  printf("sizeof.hsg_map_expr %zu\n", sizeof(hsg_map_expr));
  printf("sizeof.hsg_map_stats %zu\n", sizeof(hsg_map_stats));
  printf("sizeof.hsg_stats %zu\n", sizeof(hsg_stats));
  printf("const.strict %u\n", HSG_MAP_STRICT);
  printf("const.exprs %d\n", HSG_MAP_MAX_EXPRS);
  printf("const.ins %d\n", HSG_MAP_MAX_INS);
  return 0;
}
"""


def test_layouts():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write(LAYOUT_C)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        got = {k: int(v) for k, v in (ln.split(" ") for ln in subprocess.check_output([exe]).decode().strip().split("\n"))}
    for t in (abi.hsg_map_expr, abi.hsg_map_stats):
        for name, _ in t._fields_:
            assert got[f"{t.__name__}.{name}"] == getattr(t, name).offset, (t.__name__, name)
        assert got[f"sizeof.{t.__name__}"] == C.sizeof(t)
    assert [n for n, _ in abi.hsg_map_stats._fields_] == ["map_dropped", "map_dropped_total", "computed_cols",
                                                          "aliased_cols"]
    # hsg_stats is what it was: 30 words
    assert got["sizeof.hsg_stats"] == C.sizeof(abi.hsg_stats) == 8 * 30
    assert (got["const.strict"], got["const.exprs"], got["const.ins"]) == (abi.HSG_MAP_STRICT, abi.HSG_MAP_MAX_EXPRS,
                                                                            abi.HSG_MAP_MAX_INS) == (1, 8, 64)
    assert {"hsg_map_check", "hsg_op_create_mapped", "hsg_op_map_stats", "hsg_map_grid_threads"} <= set(abi.EXPORTED_SYMBOLS)
