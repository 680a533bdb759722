"""Host side of the scalar SELECT (no GPU): the exact mirror gen_map_r /
gen_select_rows of genMapR + genFilterR against hand-written expectations,
what gen_select_node refuses, hsg_select_check's verdicts and messages, and the
layout of the new structs against the header."""
import ctypes
import os
import subprocess
from fractions import Fraction as Fr

import pytest

from hstream_amd import abi, engine, sql

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I, F = abi.HSG_I64, abi.HSG_F64


def col(f):
    return sql.RExprCol(f, None, f)


def const(c):
    return sql.RExprConst(str(c), c)


def binop(op, l, r):
    return sql.RExprBinOp(f"({op})", {"+": "OpAdd", "-": "OpSub", "*": "OpMul"}[op], l, r)


def fn(name, e):
    return sql.RExprUnaryOp(f"{name}(..)", "Op" + name.capitalize(), e)


def cmp(op, l, r):
    return sql.RCondOp({"=": "RCompOpEQ", "<": "RCompOpLT", ">": "RCompOpGT", "<=": "RCompOpLEQ",
                        ">=": "RCompOpGEQ"}[op], l, r)


A, B, C_, X = col("a"), col("b"), col("c"), col("x")
SEL = [("COL", binop("+", A, B), "s"), ("COL", fn("SQRT", C_), "r"), ("COL", "a")]


def rec(ts, **value):
    return {"value": value, "timestamp": ts}


# ---- the mirror ---------------------------------------------------------------------------------
def test_gen_map_r_values_and_aliases():
    got = sql.gen_map_r(SEL, {"a": 2, "b": 0.25, "c": 9, "x": "ignored"})
    assert got == {"s": Fr(9, 4), "r": Fr(3), "a": Fr(2)}
    # exact: no double takes part in + - *
    assert sql.gen_map_r([("COL", binop("*", A, A), "q")], {"a": 2**40 + 1}) == {"q": Fr((2**40 + 1) ** 2)}
    # an item without an alias is named by its field / its expression's name
    assert list(sql.gen_map_r([("COL", "a"), ("COL", binop("-", A, B))], {"a": 1, "b": 1})) == ["a", "(-)"]
    # fromList keeps the later of two equal aliases
    assert sql.gen_map_r([("COL", "a", "v"), ("COL", "b", "v")], {"a": 1, "b": 2}) == {"v": Fr(2)}


def test_gen_map_r_is_strict():
    with pytest.raises(KeyError):
        sql.gen_map_r(SEL, {"a": 2, "c": 9})  # b is missing: the whole object throws
    with pytest.raises(sql.MathematicalError):
        sql.gen_map_r(SEL, {"a": 2, "b": 1, "c": -9})
    with pytest.raises(TypeError):
        sql.gen_map_r(SEL, {"a": 2, "b": "one", "c": 9})
    with pytest.raises(ValueError):
        sql.gen_map_r([("SUM", "a")], {"a": 1})


def test_gen_select_rows_chain():
    where = cmp(">", X, const(3))
    having = sql.RCondAnd(cmp("<", col("s"), const(10)), cmp(">=", col("r"), const(2)))
    records = [
        rec(10, a=1, b=2, c=4, x=4),        # kept: s = 3, r = 2
        rec(11, a=1, b=2, c=4, x=3),        # WHERE false
        rec(12, a=1, b=2, c=4),             # WHERE throws (x missing)
        rec(13, a=1, c=4, x=5),             # the map throws (b missing): strict
        rec(14, a=1, b=2, c=-4, x=5),       # SQRT of a negative number
        rec(15, a=9, b=2, c=4, x=5),        # HAVING false: s = 11
        rec(16, a=1, b=2.5, c=1, x=5),      # HAVING false: r = 1
        rec(9, a=-1, b=0.5, c=16, x=4.5),   # kept, with its own (earlier) timestamp
    ]
    got = sql.gen_select_rows(SEL, where, having, records)
    assert got == [(0, 10, {"s": Fr(3), "r": Fr(2), "a": Fr(1)}), (7, 9, {"s": Fr(-1, 2), "r": Fr(4), "a": Fr(-1)})]
    # no WHERE, no HAVING: only the strict map drops
    assert [i for i, _, _ in sql.gen_select_rows(SEL, None, None, records)] == [0, 1, 2, 5, 6, 7]
    # HAVING over an alias the list does not have throws for every record
    assert sql.gen_select_rows(SEL, None, cmp(">", col("nope"), const(0)), records) == []
    # SELECT *: the record's own object, WHERE only
    star = sql.gen_select_rows("*", where, None, records)
    assert [i for i, _, _ in star] == [0, 3, 4, 5, 6, 7] and star[1][2] is records[3]["value"]


# ---- the dispatch's refusals (no engine is touched: the op is built on first use) -----------------
def test_gen_select_node_compiles_without_a_gpu():
    st = sql.gen_select_node(None, SEL, cmp(">", X, const(3)), cmp("<", col("s"), const(10)), float_fields=("b",),
                             functions=True)
    assert st.fields == [("x", False), ("a", False), ("b", True), ("c", False)]
    assert st.aliases == ["s", "r", "a"]
    assert st.where_prog == [(abi.HSG_W_COL, 0), (abi.HSG_W_I64, 3), (abi.HSG_W_GT,)]
    assert st.exprs[0][1] == [(abi.HSG_W_COL, 1), (abi.HSG_W_COL, 2), (abi.HSG_W_ADD,)]
    assert st.exprs[1][1] == [(abi.HSG_W_COL, 3), (abi.HSG_W_FN, abi.HSG_FN_SQRT)]
    assert st.having_prog == [(abi.HSG_W_COL, 0), (abi.HSG_W_I64, 10), (abi.HSG_W_LT,)]
    rc, msg = engine.select_check([I, I, F, I], [p for _, p in st.exprs], st.where_prog, st.having_prog)
    assert (rc, msg) == (abi.HSG_OK, "")
    star = sql.gen_select_node(None, "*", cmp(">", X, const(3)))
    assert star.exprs is None and star.fields == [("x", False)]


@pytest.mark.parametrize("kw, text", [
    (dict(sel=[("SUM", "a", "t")]), "aggregate SUM"),
    (dict(sel=[("COUNT(*)",)]), "aggregate COUNT"),
    (dict(sel=[("COL", binop("+", A, const("one")), "s")]), "not a number"),
    (dict(sel=SEL, where=cmp("=", A, const("one"))), "not a number"),
    (dict(sel=SEL, where=cmp("=", A, const(True))), "not a number"),
    (dict(sel=SEL, where=cmp("=", A, const(None))), "not a number"),
    (dict(sel=[("COL", fn("SQRT", A), "r")], functions=False), "unary function OpSqrt"),
    (dict(sel=[("COL", binop("+", A, const(2**63)), "s")]), "does not fit an i64"),
    (dict(sel=[("COL", binop("*", A, const(float("inf"))), "s")]), "non-finite"),
    (dict(sel=[("COL", sql.RExprBinOp("", "OpDiv", A, B), "s")]), "OpDiv"),
    (dict(sel=SEL, having=cmp(">", col("nope"), const(0))), "not an alias"),
    (dict(sel=[("COL", "a", "v"), ("COL", "b", "v")]), "duplicate aliases"),
    (dict(sel=[("COL", binop("+", A, const(k)), f"e{k}") for k in range(9)]), "9 expressions"),
    (dict(sel=[("COL", "a")], where=sql.RCondNot(None)), "unsupported condition"),
])
def test_gen_select_node_refusals(kw, text):
    kw.setdefault("functions", True)
    with pytest.raises(ValueError) as ei:
        sql.gen_select_node(None, **kw)
    assert text in str(ei.value), str(ei.value)


def test_gen_select_node_refuses_a_stack_past_eight():
    deep = A
    for _ in range(8):  # a + (a + (a + ...)): nine operands down the right side
        deep = binop("+", A, deep)
    with pytest.raises(ValueError) as ei:
        sql.gen_select_node(None, [("COL", deep, "d")])
    assert "stack of 9" in str(ei.value)


# ---- hsg_select_check ---------------------------------------------------------------------------
COLI, ADD, GT = abi.HSG_W_COL, abi.HSG_W_ADD, abi.HSG_W_GT


def test_select_check_accepts():
    e0 = [(COLI, 0), (COLI, 1), (ADD,)]
    assert engine.select_check([I, F], [e0]) == (abi.HSG_OK, "")
    assert engine.select_check([I, F], []) == (abi.HSG_OK, "")  # SELECT *
    assert engine.select_check([], []) == (abi.HSG_OK, "")
    assert engine.select_check([I, F], [e0] * 8, [(COLI, 0), (abi.HSG_W_I64, 1), (GT,)],
                               [(COLI, 7), (abi.HSG_W_F64, 0.5), (GT,)]) == (abi.HSG_OK, "")
    # every expression is strict whatever its flags say: both flag values are taken
    assert engine.select_check([I], [abi.MapExpr([(COLI, 0)], abi.HSG_MAP_STRICT), abi.MapExpr([(COLI, 0)], 0)])[0] == 0


@pytest.mark.parametrize("args, text", [
    (([I, F], [[(COLI, 2)]]), "map: expr 0: instruction 0: column 2 out of range"),
    (([I, F], [[(COLI, 0)]] * 9), "map: 9 expressions outside 1..8"),
    (([I, F], [[(COLI, 0), (COLI, 1), (GT,)]]), "map: expr 0: instruction 2: opcode 9 is not a value instruction"),
    (([I, F], [[(COLI, 0), (COLI, 1)]]), "map: expr 0: 2 values left on the stack, not one"),
    (([I, F], [[(COLI, 0)] + [(abi.HSG_W_I64, 1), (ADD,)] * 16] * 2), "map: expr 1: 66 instructions with the expressions before it, more than 64"),
    (([I, F], [[(COLI, 0)]], [(COLI, 0), (COLI, 1), (ADD,)]), "where: the program leaves a value, not a bool"),
    (([I, F], [[(COLI, 0)]], [(COLI, 5), (COLI, 1), (GT,)]), "where: instruction 0: column 5 out of range"),
    (([I, F], [[(COLI, 0)]], None, [(COLI, 1), (abi.HSG_W_I64, 0), (GT,)]), "having: instruction 0: column 1 out of range"),
    (([I, F], [], None, [(COLI, 0), (abi.HSG_W_I64, 0), (GT,)]), "having: instruction 0: column 0 out of range"),
    (([I, F], [[(COLI, 0)]], None, [(COLI, 0)]), "having: the program leaves a value, not a bool (an i64 value)"),
    (([I, F], [[(COLI, 1)]], None, [(COLI, 0)]), "having: the program leaves a value, not a bool (an f64 value)"),
    (([I, 7], []), "select: bad column type"),
    (([I] * 9, []), "select: bad value columns (max 8)"),
    (([I], [[(abi.HSG_W_F64, float("nan"))]]), "f64 constant is not finite"),
    (([I], [[(COLI, 0), (abi.HSG_W_FN, 22)]]), "bad function 22"),
])
def test_select_check_refuses(args, text):
    rc, msg = engine.select_check(*args)
    assert rc == abi.HSG_E_INVALID and text in msg, msg


def test_select_check_types_having_by_the_expression():
    """HAVING's column j has expression j's static type: an f64 expression
    compared with 2^53 + 1 is typed f64 (the check only types; the message
    tells which type the leftover value has)."""
    exprs = [[(COLI, 0), (abi.HSG_W_F64, 0.25), (abi.HSG_W_MUL,)], [(COLI, 0), (abi.HSG_W_FN, abi.HSG_FN_SIGN)]]
    assert "an f64 value" in engine.select_check([I], exprs, None, [(COLI, 0)])[1]
    assert "an i64 value" in engine.select_check([I], exprs, None, [(COLI, 1)])[1]


def test_constants():
    assert engine.select_tile_rows() >= 64 and engine.select_tile_rows() % 64 == 0
    assert engine.select_grid_groups() >= 256


# ---- layouts -----------------------------------------------------------------------------------------
def test_layouts(tmp_path):
    src, exe = os.path.join(ROOT, "tests", "abi_layout_select.c"), str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    got = {k: int(v) for k, v in (ln.split(" ") for ln in subprocess.check_output([exe]).decode().strip().split("\n"))}
    for t in (abi.hsg_select_config, abi.hsg_select_stats):
        for name, _ in t._fields_:
            assert got[f"{t.__name__}.{name}"] == getattr(t, name).offset, (t.__name__, name)
        assert got[f"{t.__name__}.sizeof"] == ctypes.sizeof(t), t.__name__
    # the select op grew neither hsg_stats nor hsg_op_config
    assert got["hsg_stats.sizeof"] == ctypes.sizeof(abi.hsg_stats) == 30 * 8
    assert got["hsg_op_config.sizeof"] == ctypes.sizeof(abi.hsg_op_config)


def test_symbols_are_declared_and_exported():
    names = ["hsg_select_check", "hsg_op_create_select", "hsg_op_select_stats", "hsg_select_tile_rows",
             "hsg_select_grid_groups"]
    assert all(n in abi.EXPORTED_SYMBOLS for n in names)
    out = subprocess.check_output(["nm", "-D", "--defined-only", engine.LIB_PATH]).decode()
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert all(n in have for n in names)
