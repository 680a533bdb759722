"""CPU: the WHERE program's host side -- hsg_where_check's accept / reject
table, the instruction's C layout, compile_where over the refined AST, the
per-record reference gen_filter_r on every rule of the semantics, and the
columns a Table with a filter-only field asks for."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import pytest

from hstream_amd import abi, engine, processing as P, sql
from hstream_amd.abi import (HSG_W_ADD, HSG_W_AND, HSG_W_BETWEEN, HSG_W_COL, HSG_W_EQ, HSG_W_F64, HSG_W_GE, HSG_W_GT,
                             HSG_W_I64, HSG_W_LE, HSG_W_LT, HSG_W_MUL, HSG_W_NE, HSG_W_NOT, HSG_W_OR, HSG_W_SUB)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64, F64 = abi.HSG_I64, abi.HSG_F64
TYPES = [I64, F64, I64]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        from hstream_amd import build
        build.build()
    return engine.load_library()


def _gt(c, k):
    return [(HSG_W_COL, c), (HSG_W_I64, k), (HSG_W_GT,)]


ACCEPT = {
    "a > 1": _gt(0, 1),
    "a > 1 AND b > 2.5": _gt(0, 1) + [(HSG_W_COL, 1), (HSG_W_F64, 2.5), (HSG_W_GT,), (HSG_W_AND,)],
    "NOT (a + c) * 2 <> b": [(HSG_W_COL, 0), (HSG_W_COL, 2), (HSG_W_ADD,), (HSG_W_I64, 2), (HSG_W_MUL,), (HSG_W_COL, 1),
                             (HSG_W_NE,), (HSG_W_NOT,)],
    "b BETWEEN a AND c - 1": [(HSG_W_COL, 0), (HSG_W_COL, 1), (HSG_W_COL, 2), (HSG_W_I64, 1), (HSG_W_SUB,),
                              (HSG_W_BETWEEN,)],
    "every comparison": _gt(0, 1) + sum(([(HSG_W_COL, 0), (HSG_W_I64, 1), (op,), (HSG_W_OR,)]
                                         for op in (HSG_W_EQ, HSG_W_NE, HSG_W_LT, HSG_W_LE, HSG_W_GE)), []),
    "64 instructions": _gt(0, 1) + [(HSG_W_NOT,)] * 61,
    # a + (a + (a + (a + (a + (a + (a + a)))))) > 0: the eighth push is the deepest allowed
    "depth 8": [(HSG_W_COL, 0)] * 8 + [(HSG_W_ADD,)] * 7 + [(HSG_W_I64, 0), (HSG_W_GT,)],
}

REJECT = {
    "stack underflow": ([(HSG_W_COL, 0), (HSG_W_GT,)], "underflow"),
    "bool used as value": (_gt(0, 1) + [(HSG_W_I64, 1), (HSG_W_ADD,)], "bool used as a value"),
    "value used as bool": ([(HSG_W_COL, 0), (HSG_W_NOT,)], "value used as a bool"),
    "value left at end": ([(HSG_W_COL, 0), (HSG_W_I64, 1), (HSG_W_ADD,)], "leaves a value"),
    "two results": (_gt(0, 1) + _gt(2, 1), "2 results"),
    "column out of range": (_gt(3, 1), "column 3 out of range"),
    "negative column": (_gt(-1, 1), "out of range"),
    "65 instructions": (_gt(0, 1) + [(HSG_W_NOT,)] * 62, "program length 65"),
    "empty": ([], "program length 0"),
    "depth 9": ([(HSG_W_COL, 0)] * 9 + [(HSG_W_ADD,)] * 8 + [(HSG_W_I64, 0), (HSG_W_GT,)], "deeper than 8"),
    "nan constant": ([(HSG_W_COL, 1), (HSG_W_F64, math.nan), (HSG_W_LT,)], "not finite"),
    "inf constant": ([(HSG_W_COL, 1), (HSG_W_F64, math.inf), (HSG_W_LT,)], "not finite"),
    "-inf constant": ([(HSG_W_COL, 1), (HSG_W_F64, -math.inf), (HSG_W_LT,)], "not finite"),
    "bad opcode": ([(HSG_W_COL, 0), (HSG_W_I64, 1), (16,)], "bad opcode 16"),
}


@pytest.mark.parametrize("name", list(ACCEPT))
def test_where_check_accepts(lib, name):
    rc, msg = engine.where_check(ACCEPT[name], TYPES)
    assert (rc, msg) == (abi.HSG_OK, ""), name


@pytest.mark.parametrize("name", list(REJECT))
def test_where_check_rejects(lib, name):
    prog, part = REJECT[name]
    rc, msg = engine.where_check(prog, TYPES)
    assert rc == abi.HSG_E_INVALID, name
    assert part in msg, (name, msg)


def test_where_check_cuts_the_message_to_the_buffer(lib):
    prog, n = abi.where_array(REJECT["column out of range"][0])
    types = (C.c_int32 * 3)(*TYPES)
    buf = C.create_string_buffer(b"x" * 16, 16)
    assert lib.hsg_where_check(prog, n, types, 3, buf, 8) == abi.HSG_E_INVALID
    assert buf.raw[:8] == b"where: \0" and buf.raw[8:] == b"x" * 8
    assert lib.hsg_where_check(prog, n, types, 3, None, 0) == abi.HSG_E_INVALID


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "hstream_gpu.h"
int main(void) {
  printf("size %zu\n", sizeof(hsg_where_ins));
  printf("op %zu\n", offsetof(hsg_where_ins, op));
  printf("arg %zu\n", offsetof(hsg_where_ins, arg));
  printf("imm %zu\n", offsetof(hsg_where_ins, imm));
  printf("where_dropped %zu\n", offsetof(hsg_stats, where_dropped));
  printf("where_dropped_total %zu\n", offsetof(hsg_stats, where_dropped_total));
  printf("stats %zu\n", sizeof(hsg_stats));
  printf("ops %d %d %d %d\n", HSG_W_COL, HSG_W_BETWEEN, HSG_W_NOT, HSG_WHERE_MAX_INS * 100 + HSG_WHERE_MAX_DEPTH);
  return 0;
}
"""


def test_where_ins_layout_matches_c():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write(LAYOUT_C)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        got = dict(ln.split(" ", 1) for ln in subprocess.check_output([exe]).decode().strip().split("\n"))
    assert int(got["size"]) == 16 == C.sizeof(abi.hsg_where_ins)
    assert int(got["op"]) == abi.hsg_where_ins.op.offset == 0
    assert int(got["arg"]) == abi.hsg_where_ins.arg.offset == 4
    assert int(got["imm"]) == abi.hsg_where_ins.imm.offset == 8
    assert int(got["where_dropped"]) == abi.hsg_stats.where_dropped.offset
    assert int(got["where_dropped_total"]) == abi.hsg_stats.where_dropped_total.offset
    assert int(got["stats"]) == C.sizeof(abi.hsg_stats)
    assert got["ops"] == f"{abi.HSG_W_COL} {abi.HSG_W_BETWEEN} {abi.HSG_W_NOT} " \
                         f"{abi.HSG_WHERE_MAX_INS * 100 + abi.HSG_WHERE_MAX_DEPTH}"
    ins = abi.where_ins(HSG_W_F64, 2.5)
    assert ins.imm.i == 0x4004000000000000
    assert abi.where_ins(HSG_W_I64, -1).imm.i == -1 and abi.where_ins(HSG_W_COL, 3).arg == 3


# ---- compile_where ------------------------------------------------------------
def col(f):
    return sql.RExprCol(f, None, f)


def const(c):
    return sql.RExprConst(str(c), c)


# ParseRefineSpec.hs:19-20: ... WHERE temperature > 30 AND humidity > 80
REF_EXAMPLE = sql.RCondAnd(sql.RCondOp("RCompOpGT", col("temperature"), const(30)),
                           sql.RCondOp("RCompOpGT", col("humidity"), const(80)))


def test_compile_where_reference_example(lib):
    prog = sql.compile_where(REF_EXAMPLE, ["temperature", "humidity"])
    assert prog == [(HSG_W_COL, 0), (HSG_W_I64, 30), (HSG_W_GT,), (HSG_W_COL, 1), (HSG_W_I64, 80), (HSG_W_GT,),
                    (HSG_W_AND,)]
    assert engine.where_check(prog, [I64, I64]) == (abi.HSG_OK, "")
    assert sql.where_fields(REF_EXAMPLE) == ["temperature", "humidity"]


def test_compile_where_every_node_kind(lib):
    a, b = col("a"), col("b")
    cases = [
        (sql.RCondOp("RCompOpEQ", a, const(1)), [(HSG_W_COL, 0), (HSG_W_I64, 1), (HSG_W_EQ,)]),
        (sql.RCondOp("RCompOpNE", a, const(1.5)), [(HSG_W_COL, 0), (HSG_W_F64, 1.5), (HSG_W_NE,)]),
        (sql.RCondOp("RCompOpLT", a, b), [(HSG_W_COL, 0), (HSG_W_COL, 1), (HSG_W_LT,)]),
        (sql.RCondOp("RCompOpLEQ", a, b), [(HSG_W_COL, 0), (HSG_W_COL, 1), (HSG_W_LE,)]),
        (sql.RCondOp("RCompOpGEQ", a, b), [(HSG_W_COL, 0), (HSG_W_COL, 1), (HSG_W_GE,)]),
        (sql.RCondOp("RCompOpGT", sql.RExprBinOp("a+b", "OpAdd", a, b), sql.RExprBinOp("a-b", "OpSub", a, b)),
         [(HSG_W_COL, 0), (HSG_W_COL, 1), (HSG_W_ADD,), (HSG_W_COL, 0), (HSG_W_COL, 1), (HSG_W_SUB,), (HSG_W_GT,)]),
        (sql.RCondOp("RCompOpGT", sql.RExprBinOp("a*2", "OpMul", a, const(2)), b),
         [(HSG_W_COL, 0), (HSG_W_I64, 2), (HSG_W_MUL,), (HSG_W_COL, 1), (HSG_W_GT,)]),
        (sql.RCondOr(sql.RCondOp("RCompOpGT", a, const(1)), sql.RCondOp("RCompOpGT", b, const(2))),
         _gt(0, 1) + _gt(1, 2) + [(HSG_W_OR,)]),
        (sql.RCondNot(sql.RCondOp("RCompOpGT", a, const(1))), _gt(0, 1) + [(HSG_W_NOT,)]),
        (sql.RCondBetween(const(1), a, b), [(HSG_W_I64, 1), (HSG_W_COL, 0), (HSG_W_COL, 1), (HSG_W_BETWEEN,)]),
    ]
    for cond, want in cases:
        prog = sql.compile_where(cond, ["a", "b"])
        assert prog == want, cond
        assert engine.where_check(prog, [I64, F64]) == (abi.HSG_OK, ""), cond
    # a stream-qualified column is the composed name
    assert sql.compile_where(sql.RCondOp("RCompOpGT", sql.RExprCol("s.a", "s", "a"), const(1)), ["s.a"]) == _gt(0, 1)


def test_compile_where_out_of_scope():
    a = col("a")
    gt = lambda l, r: sql.RCondOp("RCompOpGT", l, r)
    for cond in (gt(a, const("x")), gt(a, const(True)), gt(a, const(None)), gt(a, const(math.inf)), gt(a, const(2**63)),
                 gt(sql.RExprUnaryOp("SIN(a)", "OpSin", a), const(0)), gt(sql.RExprBinOp("x", "OpIfNull", a, a), const(0)),
                 gt(col("zz"), const(0))):
        with pytest.raises(ValueError):
            sql.compile_where(cond, ["a"])
    with pytest.raises(ValueError, match="group key"):
        sql.compile_where(gt(col("k"), const(0)), ["a", "k"], key_field="k")
    deep = a
    for _ in range(8):
        deep = sql.RExprBinOp("x", "OpAdd", a, deep)  # a + (a + (...)): nine operands at once
    with pytest.raises(ValueError, match="stack"):
        sql.compile_where(gt(deep, const(0)), ["a"])
    long = gt(a, const(0))
    for _ in range(16):
        long = sql.RCondAnd(long, gt(a, const(0)))  # 17 comparisons of 3 + 16 ANDs = 67
    with pytest.raises(ValueError, match="instructions"):
        sql.compile_where(long, ["a"])


# ---- gen_filter_r: every rule of the semantics -----------------------------------
def test_gen_filter_r_rules():
    a, b, c = col("a"), col("b"), col("c")
    gt = lambda l, r: sql.RCondOp("RCompOpGT", l, r)
    f = sql.gen_filter_r
    assert f(None, {}) is True
    # comparisons: both sides are needed
    assert f(gt(a, const(1)), {"a": 2}) and not f(gt(a, const(1)), {"a": 1})
    for op, want in (("RCompOpEQ", (0, 1, 0)), ("RCompOpNE", (1, 0, 1)), ("RCompOpLT", (1, 0, 0)),
                     ("RCompOpGT", (0, 0, 1)), ("RCompOpLEQ", (1, 1, 0)), ("RCompOpGEQ", (0, 1, 1))):
        got = tuple(int(f(sql.RCondOp(op, a, const(5)), {"a": v})) for v in (4, 5, 6))
        assert got == want, op
    with pytest.raises(KeyError):
        f(gt(a, const(1)), {"b": 2})
    with pytest.raises(KeyError):
        f(sql.RCondOp("RCompOpEQ", const(1), a), {})
    # exact mixed comparison: Scientific, not double
    assert f(gt(a, const(9007199254740992.0)), {"a": 2**53 + 1})
    assert not f(gt(a, const(9007199254740992.0)), {"a": 2**53})
    assert f(sql.RCondOp("RCompOpLT", a, const(2.0**63)), {"a": 2**63 - 1})
    # arithmetic is exact and the error goes through it
    assert f(sql.RCondOp("RCompOpEQ", sql.RExprBinOp("", "OpAdd", a, const(0.1)), const(0.1)), {"a": 0})
    assert f(sql.RCondOp("RCompOpEQ", sql.RExprBinOp("", "OpMul", a, b), const(2**64)), {"a": 2**32, "b": 2**32})
    assert f(sql.RCondOp("RCompOpEQ", sql.RExprBinOp("", "OpSub", a, b), const(-1)), {"a": 1, "b": 2})
    with pytest.raises(KeyError):
        f(gt(sql.RExprBinOp("", "OpAdd", a, b), const(0)), {"a": 1})
    # OR: l true -> true without r; l error -> error; l false -> r
    o = sql.RCondOr(gt(a, const(1)), gt(b, const(2)))
    assert f(o, {"a": 2}) is True
    assert f(o, {"a": 0, "b": 3}) is True and f(o, {"a": 0, "b": 0}) is False
    with pytest.raises(KeyError):
        f(o, {"b": 3})
    with pytest.raises(KeyError):
        f(o, {"a": 0})
    # AND: l false -> false without r; l error -> error; l true -> r
    n = sql.RCondAnd(gt(a, const(1)), gt(b, const(2)))
    assert f(n, {"a": 0}) is False
    assert f(n, {"a": 2, "b": 3}) is True and f(n, {"a": 2, "b": 0}) is False
    with pytest.raises(KeyError):
        f(n, {"b": 3})
    with pytest.raises(KeyError):
        f(n, {"a": 2})
    # NOT: of the decided value; NOT error = error
    assert f(sql.RCondNot(n), {"a": 0}) is True
    with pytest.raises(KeyError):
        f(sql.RCondNot(n), {"a": 2})
    # BETWEEN lo x hi: lo or x missing -> error; lo > x -> false without hi; hi missing -> error; x <= hi
    bt = sql.RCondBetween(a, b, c)
    assert f(bt, {"a": 5, "b": 1}) is False
    with pytest.raises(KeyError):
        f(bt, {"a": 1, "b": 5})
    with pytest.raises(KeyError):
        f(bt, {"b": 5, "c": 9})
    with pytest.raises(KeyError):
        f(bt, {"a": 1, "c": 9})
    assert f(bt, {"a": 1, "b": 5, "c": 5}) is True and f(bt, {"a": 5, "b": 5, "c": 9}) is True
    assert f(bt, {"a": 1, "b": 5, "c": 4}) is False


# ---- Table: the op's columns with a filter-only field -----------------------------
class _NoEngine:
    """Table builds its op at once; this one only records the spec."""

    def op(self, spec):
        self.spec = spec
        return None


def test_table_lists_filter_only_fields_after_the_aggregated_ones():
    eng = _NoEngine()
    cond = sql.RCondAnd(sql.RCondOp("RCompOpGT", col("humidity"), const(80.5)),
                        sql.RCondOp("RCompOpGT", col("temperature"), const(30)))
    t = sql.gen_group_by_node(eng, [("COUNT(*)",), ("SUM", "temperature"), ("COUNT", "note")], sql.RGroupBy("city"),
                              float_fields=("humidity",), where=cond)
    assert t.fields == [("temperature", False), ("note", False), ("humidity", True)]
    assert t.numeric == [True, False, True]
    assert eng.spec.col_types == [I64, I64, F64]
    assert eng.spec.aggs == [(abi.HSG_COUNT_ALL, 0), (abi.HSG_SUM, 0), (abi.HSG_COUNT, 1)]
    assert eng.spec.where == [(HSG_W_COL, 2), (HSG_W_F64, 80.5), (HSG_W_GT,), (HSG_W_COL, 0), (HSG_W_I64, 30),
                              (HSG_W_GT,), (HSG_W_AND,)]
    recs = [{"timestamp": 5, "value": {"city": "x", "temperature": 31, "humidity": 90.25}},
            {"timestamp": 6, "value": {"city": "x", "temperature": 31}},                      # filter field absent
            {"timestamp": 7, "value": {"city": "x", "temperature": 31, "humidity": "wet"}}]    # present non-number
    keys, ts, cols, valid = t.columns(recs)
    # the host masks nothing for the predicate: the absent field is a valid
    # byte of 0 (the program's error value), only the non-number drops here
    assert keys.tolist() == [0, 0, abi.HSG_KEY_NONE] and ts.tolist() == [5, 6, 7]
    assert len(cols) == 3 and cols[2][0] == 90.25 and cols[0].tolist()[:2] == [31, 31]
    assert [v.tolist() for v in valid] == [[1, 1, 1], [0, 0, 0], [1, 0, 1]]
    # no WHERE: nothing changes
    t0 = sql.gen_group_by_node(eng, [("SUM", "temperature")], sql.RGroupBy("city"))
    assert t0.fields == [("temperature", False)] and eng.spec.where is None
    # a WHERE the program cannot say is the caller's to run upstream
    with pytest.raises(ValueError):
        sql.gen_group_by_node(eng, [("COUNT(*)",)], sql.RGroupBy("city"),
                              where=sql.RCondOp("RCompOpEQ", col("city"), const("x")))
