"""CPU: the host side of the numeric SQL functions (HSG_W_FN) -- the three
checkers' accept / reject tables and typing, hsg_prog_fn_class, the exact
mirror sql.expr_value against hand-written values, and the compilers'
`functions` switch."""
import math
from fractions import Fraction

import pytest

from hstream_amd import abi, engine, processing as P, sql
from hstream_amd.abi import HSG_W_ADD, HSG_W_COL, HSG_W_F64, HSG_W_FN, HSG_W_GT, HSG_W_I64, HSG_W_NOT
from hstream_amd.columnar import OpSpec
from test_where_host import ACCEPT as WHERE_ACCEPT

I64, F64 = abi.HSG_I64, abi.HSG_F64
TYPES = [I64, F64, I64]
FNS = list(range(abi.HSG_FN_COUNT))


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(engine.LIB_PATH):
        from hstream_amd import build
        build.build()
    return engine.load_library()


def want_type(fn, operand):
    """The typing table: ABS / CEIL / FLOOR / ROUND the operand's, SIGN i64, the other 17 f64."""
    if fn in (abi.HSG_FN_ABS, abi.HSG_FN_CEIL, abi.HSG_FN_FLOOR, abi.HSG_FN_ROUND):
        return operand
    return I64 if fn == abi.HSG_FN_SIGN else F64


def test_the_enum_is_the_references_list():
    assert abi.HSG_W_FN == 32 and abi.HSG_FN_COUNT == 22 == len(abi.HSG_FN_NAMES) == len(set(abi.HSG_FN_NAMES))
    assert (abi.HSG_FN_SIN, abi.HSG_FN_ABS, abi.HSG_FN_SIGN, abi.HSG_FN_LOG, abi.HSG_FN_EXP) == (0, 12, 17, 18, 21)
    assert [abi.HSG_FN_NAMES[f] for f in abi.HSG_FN_EXACT] == ["ABS", "CEIL", "FLOOR", "ROUND", "SQRT", "SIGN"]
    assert abi.where_ins(HSG_W_FN, abi.HSG_FN_SQRT).arg == abi.HSG_FN_SQRT
    assert {"hsg_prog_fn_class", "hsg_map_grid_threads_fn"} <= set(abi.EXPORTED_SYMBOLS)


# ---- the three checkers: accept, with the typing table ------------------------------
@pytest.mark.parametrize("c", [0, 1], ids=["i64", "f64"])
@pytest.mark.parametrize("fn", FNS, ids=abi.HSG_FN_NAMES)
def test_checkers_accept_every_function(lib, fn, c):
    e = [(HSG_W_COL, c), (HSG_W_FN, fn)]
    rc, msg, types = engine.map_check([e, e + [(HSG_W_FN, fn)], e + [(HSG_W_COL, 2), (HSG_W_ADD,)]], TYPES)
    t = want_type(fn, TYPES[c])
    assert (rc, msg) == (abi.HSG_OK, "")
    assert types == [t, want_type(fn, t), t] and abi.map_expr_type(e, TYPES) == t
    assert engine.where_check(e + [(HSG_W_I64, 1), (HSG_W_GT,)], TYPES) == (abi.HSG_OK, "")
    # HAVING: aggregate 0 is SUM over column c, so it has column c's type
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=TYPES, aggs=[(abi.HSG_SUM, c)])
    assert engine.having_check([(HSG_W_COL, 0), (HSG_W_FN, fn), (HSG_W_I64, 1), (HSG_W_GT,)], spec) == (abi.HSG_OK, "")


def test_a_function_keeps_the_stack_depth(lib):
    deep = [(HSG_W_COL, 0)] * 8 + [(HSG_W_FN, abi.HSG_FN_ABS)] + [(HSG_W_ADD,)] * 7
    assert engine.map_check([deep], TYPES)[0] == abi.HSG_OK
    assert engine.where_check(deep + [(HSG_W_FN, abi.HSG_FN_SIN), (HSG_W_I64, 0), (HSG_W_GT,)], TYPES)[0] == abi.HSG_OK


# ---- ... and reject ---------------------------------------------------------------------
HAVING_SPEC = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=TYPES,
                     aggs=[(abi.HSG_SUM, 0), (abi.HSG_SUM, 1), (abi.HSG_COUNT_ALL, 0)])
BOOL = [(HSG_W_COL, 0), (HSG_W_I64, 1), (HSG_W_GT,)]
REJECT = {
    "arg -1": ([(HSG_W_COL, 0), (HSG_W_FN, -1)], "instruction 1: bad function -1"),
    "arg 22": ([(HSG_W_COL, 0), (HSG_W_FN, 22)], "instruction 1: bad function 22"),
    "underflow": ([(HSG_W_FN, abi.HSG_FN_ABS)], "instruction 0: stack underflow"),
}


@pytest.mark.parametrize("name", list(REJECT))
def test_checkers_reject(lib, name):
    e, part = REJECT[name]
    tail = [(HSG_W_I64, 1), (HSG_W_GT,)]
    rc, msg, _ = engine.map_check([[(HSG_W_COL, 0)], e], TYPES)
    assert rc == abi.HSG_E_INVALID and msg.startswith("map: expr 1: ") and part in msg, msg
    rc, msg = engine.where_check(e + tail, TYPES)
    assert rc == abi.HSG_E_INVALID and msg.startswith("where: ") and part in msg, msg
    rc, msg = engine.having_check(e + tail, HAVING_SPEC)
    assert rc == abi.HSG_E_INVALID and msg.startswith("having: ") and part in msg, msg


@pytest.mark.parametrize("fn", [abi.HSG_FN_ABS, abi.HSG_FN_SIGN, abi.HSG_FN_SIN], ids=["ABS", "SIGN", "SIN"])
def test_a_function_of_a_bool_is_refused(lib, fn):
    prog = BOOL + [(HSG_W_FN, fn), (HSG_W_I64, 0), (HSG_W_GT,)]
    for rc, msg in (engine.where_check(prog, TYPES), engine.having_check(prog, HAVING_SPEC)):
        assert rc == abi.HSG_E_INVALID and "instruction 3: a bool used as a value" in msg, msg
    # (a map has no bool to apply one to: the comparison itself is no value instruction)
    rc, msg, _ = engine.map_check([BOOL + [(HSG_W_FN, fn)]], TYPES)
    assert rc == abi.HSG_E_INVALID and "is not a value instruction" in msg, msg


def test_opcodes_16_to_31_stay_invalid(lib):
    rc, msg = engine.where_check([(HSG_W_COL, 0), (HSG_W_I64, 1), (16,)], TYPES)
    assert rc == abi.HSG_E_INVALID and "bad opcode 16" in msg
    for op in (16, 31, 33):
        assert engine.where_check([(HSG_W_COL, 0), (op, 0), (HSG_W_I64, 1), (HSG_W_GT,)], TYPES)[0] == abi.HSG_E_INVALID
        rc, msg, _ = engine.map_check([[(HSG_W_COL, 0), (op, 0)]], TYPES)
        assert rc == abi.HSG_E_INVALID and f"opcode {op} is not a value instruction" in msg


# ---- hsg_prog_fn_class ----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(WHERE_ACCEPT))
def test_class_0_for_every_program_without_a_function(lib, name):
    assert engine.prog_fn_class(WHERE_ACCEPT[name]) == 0


def test_fn_class(lib):
    fc = engine.prog_fn_class
    gt = [(HSG_W_I64, 1), (HSG_W_GT,)]
    for fn in FNS:
        want = 1 if fn in abi.HSG_FN_EXACT else 2
        assert fc([(HSG_W_COL, 0), (HSG_W_FN, fn)] + gt) == want, abi.HSG_FN_NAMES[fn]
    assert fc([(HSG_W_COL, 0), (HSG_W_FN, abi.HSG_FN_ABS), (HSG_W_FN, abi.HSG_FN_SQRT)] + gt) == 1
    assert fc([(HSG_W_COL, 0), (HSG_W_FN, abi.HSG_FN_ABS), (HSG_W_FN, abi.HSG_FN_SIN)] + gt) == 2
    assert fc([(HSG_W_COL, 0), (HSG_W_FN, abi.HSG_FN_LOG), (HSG_W_FN, abi.HSG_FN_ABS)] + gt) == 2
    # `arg` is read for FN alone: column 13 is not CEIL
    assert fc([(HSG_W_COL, 13)] + gt) == 0
    assert load().hsg_prog_fn_class(None, 0) == 0


def load():
    return engine.load_library()


def test_map_grid_threads_per_class(lib):
    g = [engine.map_grid_threads_fn(c) for c in range(3)]
    assert g[0] == engine.map_grid_threads()
    assert all(x > 0 and x % 256 == 0 for x in g) and g[2] <= g[1] <= g[0]
    assert engine.map_grid_threads_fn(3) == 0 and engine.map_grid_threads_fn(-1) == 0


# ---- sql.expr_value: hand-written values ---------------------------------------------------------
def col(f):
    return sql.RExprCol(f, None, f)


def fn(name, e):
    return sql.RExprUnaryOp(f"{name}(..)", "Op" + name.capitalize(), e)


X = col("x")


def val(name, x):
    return sql.expr_value(fn(name, X), {"x": x})


def test_round_is_half_to_even():
    assert [val("ROUND", x) for x in (0.5, -0.5, 1.5, -1.5, 2.5, -2.5)] == [0, 0, 2, -2, 2, -2]
    assert val("ROUND", 0.75) == 1 and val("ROUND", 7) == 7
    assert isinstance(val("ROUND", 2.5), Fraction)


def test_ceil_floor_abs_sign():
    assert (val("CEIL", -0.25), val("FLOOR", -0.25)) == (0, -1)
    assert (val("CEIL", 0.25), val("FLOOR", 0.25)) == (1, 0)
    # the mirror is exact: 2^63 (the device's i64 wraps to -2^63)
    assert val("ABS", -2**63) == Fraction(2**63)
    assert val("ABS", -0.25) == Fraction(1, 4)
    assert [val("SIGN", x) for x in (0, 0.0, -0.0, -3, 0.25, -1e300)] == [0, 0, 0, -1, 1, -1]


def test_float_functions_are_the_double_functions():
    assert val("LOG10", 1000) == Fraction(math.log(1000) / math.log(10)) != 3
    assert val("LOG2", 8) == Fraction(math.log(8.0) / math.log(2.0))
    assert val("SQRT", 2) == Fraction(math.sqrt(2.0)) and val("SQRT", 2**52) == 2**26
    assert val("EXP", 0) == 1 and val("SIN", 0.5) == Fraction(math.sin(0.5))
    assert val("ATAN", -2**63) == Fraction(math.atan(-2.0**63))
    # nested, and under arithmetic
    e = sql.RExprBinOp("", "OpAdd", fn("SQRT", fn("ABS", X)), sql.RExprConst("1", 1))
    assert sql.expr_value(e, {"x": -16}) == 5


DOMAIN = [("ASIN", 1.25), ("ASIN", -2), ("ACOS", 1.25), ("ACOS", -1.5), ("ACOSH", 0.75), ("ACOSH", 0), ("ATANH", 1),
          ("ATANH", -1), ("ATANH", 3), ("LOG", 0), ("LOG", -1), ("LOG2", 0), ("LOG2", -0.5), ("LOG10", 0),
          ("LOG10", -7), ("SQRT", -1), ("SQRT", -0.25), ("EXP", 710), ("SINH", 711), ("COSH", -711), ("EXP", 1e308)]


@pytest.mark.parametrize("name,x", DOMAIN, ids=[f"{n}({x})" for n, x in DOMAIN])
def test_domain_errors_and_non_finite_results_raise(name, x):
    with pytest.raises(sql.MathematicalError):
        val(name, x)


def test_domain_edges_are_values():
    assert val("ASIN", 1) == Fraction(math.asin(1.0)) and val("ACOS", -1) == Fraction(math.pi)
    assert val("ACOSH", 1) == 0 and val("SQRT", 0) == 0 and val("SQRT", -0.0) == 0
    assert val("ATANH", 0.75) == Fraction(math.atanh(0.75))


def test_an_error_of_the_operand_carries_through():
    with pytest.raises(KeyError):
        sql.expr_value(fn("ABS", col("y")), {"x": 1})
    with pytest.raises(sql.MathematicalError):
        sql.expr_value(fn("ABS", fn("LOG", X)), {"x": 0})
    with pytest.raises(TypeError):
        sql.expr_value(sql.RExprUnaryOp("", "OpIsInt", X), {"x": 1})
    # gen_filter_r: the record's condition throws, the caller drops it
    cond = sql.RCondOp("RCompOpGT", fn("SQRT", X), sql.RExprConst("1", 1))
    assert sql.gen_filter_r(cond, {"x": 4}) is True and sql.gen_filter_r(cond, {"x": 1}) is False
    with pytest.raises(sql.MathematicalError):
        sql.gen_filter_r(cond, {"x": -4})


def test_expr_is_float_follows_the_typing_table():
    for name in abi.HSG_FN_NAMES:
        f = abi.HSG_FN_NAMES.index(name)
        for field, t in (("a", I64), ("b", F64)):
            assert sql.expr_is_float(fn(name, col(field)), ("b",)) == (want_type(f, t) == F64), (name, field)
    assert not sql.expr_is_float(fn("ABS", fn("SIGN", col("b"))), ("b",))
    assert sql.expr_is_float(sql.RExprBinOp("", "OpAdd", col("a"), fn("SQRT", col("a"))), ("b",))


# ---- the compilers: off by default ---------------------------------------------------------------
def test_compilers_emit_fn_after_the_operand():
    a, b = col("a"), col("b")
    e = sql.RExprBinOp("", "OpMul", fn("ABS", a), fn("LOG10", sql.RExprBinOp("", "OpAdd", b, sql.RExprConst("1", 1))))
    assert sql.compile_expr(e, ["a", "b"], functions=True) == [
        (HSG_W_COL, 0), (HSG_W_FN, abi.HSG_FN_ABS), (HSG_W_COL, 1), (HSG_W_I64, 1), (HSG_W_ADD,),
        (HSG_W_FN, abi.HSG_FN_LOG10), (abi.HSG_W_MUL,)]
    for name in abi.HSG_FN_NAMES:
        assert sql.compile_expr(fn(name, a), ["a"], functions=True) == [(HSG_W_COL, 0),
                                                                       (HSG_W_FN, abi.HSG_FN_NAMES.index(name))]
    cond = sql.RCondNot(sql.RCondOp("RCompOpLT", fn("ASIN", b), sql.RExprConst("0", 0)))
    want = [(HSG_W_COL, 1), (HSG_W_FN, abi.HSG_FN_ASIN), (HSG_W_I64, 0), (abi.HSG_W_LT,), (HSG_W_NOT,)]
    assert sql.compile_where(cond, ["a", "b"], functions=True) == want
    hv = sql.RCondOp("RCompOpGEQ", fn("ABS", col("s")), sql.RExprConst("5", 5))
    assert sql.compile_having(hv, ["n", "s"], functions=True) == [(HSG_W_COL, 1), (HSG_W_FN, abi.HSG_FN_ABS),
                                                                 (HSG_W_I64, 5), (abi.HSG_W_GE,)]
    aggs = sql.gen_aggregate_components([("SUM", fn("SQRT", a), "s"), ("MAX", fn("FLOOR", b), "m"),
                                         ("COL", fn("SIGN", b), "g")], float_fields=("b",), functions=True)
    assert [(g.is_float, g.strict, g.field.functions) for g in aggs] == [(True, False, True), (True, False, True),
                                                                         (False, True, True)]


def test_the_default_refuses_as_before():
    a = col("a")
    cond = sql.RCondOp("RCompOpGT", fn("ABS", a), sql.RExprConst("3", 3))
    with pytest.raises(ValueError, match="unary function OpAbs is not pushed down"):
        sql.compile_expr(fn("ABS", a), ["a"])
    with pytest.raises(ValueError, match="unary function OpAbs is not pushed down"):
        sql.compile_where(cond, ["a"])
    with pytest.raises(ValueError, match="unary function OpAbs is not pushed down"):
        sql.compile_having(cond, ["a"])
    with pytest.raises(ValueError, match="unary function OpSin is not pushed down"):
        sql.gen_aggregate_components([("SUM", fn("SIN", a), "s")])
    # a function outside the numeric list stays refused with the switch on
    with pytest.raises(ValueError, match="unary function OpIsInt is not pushed down"):
        sql.compile_expr(sql.RExprUnaryOp("", "OpIsInt", a), ["a"], functions=True)
    assert P.Expr(a).functions is False and P.Where(cond).functions is False and P.Having(cond).functions is False
