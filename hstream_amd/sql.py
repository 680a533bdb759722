"""Mirror of hstream-sql's windowed GROUP BY dispatch (the codegen side only;
the BNFC parser/validator are out of scope).

  refine_interval    Interval refinement, hstream-sql/src/HStream/SQL/AST.hs:66-74
                     (DAY/WEEK/MONTH/YEAR multiply by 60*24, not 3600*24: kept)
  diff_time_to_ms    Internal/Codegen.hs:222-223
  gen_group_by_node  Codegen.hs:479-521 (+ genAggregateComponents :393-469,
                     genMaterialized :372-385): the window clause picks the
                     operator, the SELECT list the aggregate components.
                     HAVING is not applied to windowed GROUP BY (Codegen.hs:554-559)
                     and only one GROUP BY column exists (Validate.hs:556-562).
  RExpr* / RCond*    the refined WHERE clause, AST.hs:123-128 and :294-325
  gen_filter_r       genFilterR, Codegen.hs:303-341 over genRExprValue :290-301,
                     one record at a time with exact arithmetic: what the
                     filter means (and the tests' reference)
  compile_where      the same clause as the postfix program the op runs on
                     the GPU ahead of the aggregate (include/hstream_gpu.h
                     hsg_where_ins), where the reference chains genFilterNode
                     in front of it (Codegen.hs:540)
  compile_expr       a value expression of the SELECT list as the postfix value
                     program the op's map pass runs per record (include/
                     hstream_gpu.h hsg_map_expr): genRExprValue, Codegen.hs:290-301
  gen_map_r          genMapR (Codegen.hs:349-353) for one record: the SELECT
                     list's object {alias: Number}, strict as the reference's
                     HashMap is; gen_select_rows is the whole RGroupByEmpty
                     chain over a batch (the tests' reference)
  gen_select_node    the RGroupByEmpty branch of genStreamBuilderWithStream
                     (Codegen.hs:542-550): filter -> map -> having on one
                     select op (hsg_op_create_select)
  compile_having     the HAVING condition as the same program over the
                     aggregates' aliases, run over the rows the op emits,
                     where the reference chains genFilteRNodeFromHaving
                     behind an unwindowed aggregate (Codegen.hs:524-529)
  gen_joiner         genJoiner, Internal/Codegen.hs:62-67
  RFromJoin /        the RFromJoin branch of genStreamWithSourceStream
  gen_join_node      (Codegen.hs:253-266) as one valued GPU join whose drained
                     batches feed gen_select_node / gen_group_by_node on the
                     device; gen_join_rows is its host mirror (the tests' reference)
"""
import math
from dataclasses import dataclass
from fractions import Fraction
from typing import Any, List, Optional, Sequence, Tuple, Union

from . import abi, processing as P

_UNIT_SECONDS = {
    "SECOND": 1,
    "MINUTE": 60,
    "DAY": 60 * 24,            # AST.hs:71 (sic)
    "WEEK": 60 * 24 * 7,       # AST.hs:72
    "MONTH": 60 * 24 * 30,     # AST.hs:73
    "YEAR": 60 * 24 * 365,     # AST.hs:74
}


def refine_interval(n: int, unit: str) -> int:
    """INTERVAL n UNIT -> seconds (DiffTime), as the reference refines it."""
    u = unit.upper().rstrip("S") if unit.upper() not in ("SECONDS",) else "SECOND"
    if u not in _UNIT_SECONDS:
        raise ValueError(f"unknown interval unit {unit}")
    if n <= 0:
        raise ValueError("Interval must be positive")  # Validate.hs:82-86
    return n * _UNIT_SECONDS[u]


def diff_time_to_ms(seconds: int) -> int:
    return int(seconds) * 1000  # picoseconds `div` 10^9


@dataclass(frozen=True)
class RTumblingWindow:
    seconds: int


@dataclass(frozen=True)
class RHoppingWindow:
    length: int
    hop: int


@dataclass(frozen=True)
class RSessionWindow:
    seconds: int


RWindow = Union[RTumblingWindow, RHoppingWindow, RSessionWindow]


@dataclass(frozen=True)
class RGroupBy:
    column: str
    window: Optional[RWindow] = None


# ---- WHERE: the refined search condition (AST.hs:123-128, 294-325) ----------
@dataclass(frozen=True)
class RExprCol:
    name: str
    stream: Optional[str]
    field: str


@dataclass(frozen=True)
class RExprConst:
    """constant: an int (ConstantInt) or a float (ConstantNum); a str
    (ConstantString), bool (ConstantBool) or None (ConstantNull) exists in the
    reference but is out of the GPU program's scope."""
    name: str
    constant: Any


@dataclass(frozen=True)
class RExprBinOp:
    name: str
    op: str  # "OpAdd" / "OpSub" / "OpMul"
    expr1: Any
    expr2: Any


@dataclass(frozen=True)
class RExprUnaryOp:
    name: str
    op: str
    expr: Any


@dataclass(frozen=True)
class RCondOp:
    op: str  # "RCompOpEQ" / "RCompOpNE" / "RCompOpLT" / "RCompOpGT" / "RCompOpLEQ" / "RCompOpGEQ"
    expr1: Any
    expr2: Any


@dataclass(frozen=True)
class RCondAnd:
    cond1: Any
    cond2: Any


@dataclass(frozen=True)
class RCondOr:
    cond1: Any
    cond2: Any


@dataclass(frozen=True)
class RCondNot:
    cond: Any


@dataclass(frozen=True)
class RCondBetween:
    """expr BETWEEN expr1 AND expr2, in the reference's order (AST.hs:309,317)."""
    expr1: Any
    expr: Any
    expr2: Any


RSearchCond = Union[RCondOp, RCondAnd, RCondOr, RCondNot, RCondBetween]

_COMP_OPS = {"RCompOpEQ": abi.HSG_W_EQ, "RCompOpNE": abi.HSG_W_NE, "RCompOpLT": abi.HSG_W_LT,
             "RCompOpGT": abi.HSG_W_GT, "RCompOpLEQ": abi.HSG_W_LE, "RCompOpGEQ": abi.HSG_W_GE}
_BIN_OPS = {"OpAdd": abi.HSG_W_ADD, "OpSub": abi.HSG_W_SUB, "OpMul": abi.HSG_W_MUL}
# the 22 numeric unary functions (unaryOpOnValue, Internal/Codegen.hs:139-179): "OpSin" ... "OpLog10"
_FN_OPS = {"Op" + n.capitalize(): i for i, n in enumerate(abi.HSG_FN_NAMES)}
_FLOAT_FNS = {
    abi.HSG_FN_SIN: math.sin, abi.HSG_FN_SINH: math.sinh, abi.HSG_FN_ASIN: math.asin, abi.HSG_FN_ASINH: math.asinh,
    abi.HSG_FN_COS: math.cos, abi.HSG_FN_COSH: math.cosh, abi.HSG_FN_ACOS: math.acos, abi.HSG_FN_ACOSH: math.acosh,
    abi.HSG_FN_TAN: math.tan, abi.HSG_FN_TANH: math.tanh, abi.HSG_FN_ATAN: math.atan, abi.HSG_FN_ATANH: math.atanh,
    abi.HSG_FN_SQRT: math.sqrt, abi.HSG_FN_LOG: math.log, abi.HSG_FN_EXP: math.exp,
    # as the reference divides (Internal/Codegen.hs:173-178), not log2 / log10
    abi.HSG_FN_LOG2: lambda x: math.log(x) / math.log(2.0),
    abi.HSG_FN_LOG10: lambda x: math.log(x) / math.log(10.0),
}


class MathematicalError(ArithmeticError):
    """unaryOpOnValue's "Mathematical error" (a domain error), and this
    engine's rule for a result that is not finite: the expression is the
    error value for the record, as for a missing field."""


def unary_value(fn: int, x: Fraction) -> Fraction:
    """unaryOpOnValue for the numeric function fn (abi.HSG_FN_*) of an exact
    Number. ABS, CEIL, FLOOR, ROUND (half to even, Haskell's round) and SIGN
    are exact; every other function is the double function of toRealFloat x.
    MathematicalError where the reference throws -- ASIN / ACOS outside
    [-1, 1], ACOSH below 1, ATANH outside (-1, 1), LOG* at or below 0 -- and,
    where the reference would make a meaningless finite number of a NaN or an
    infinity, for SQRT of a negative number and for an operand or a result
    that is not finite as a double."""
    if fn == abi.HSG_FN_ABS:
        return abs(x)
    if fn == abi.HSG_FN_CEIL:
        return Fraction(math.ceil(x))
    if fn == abi.HSG_FN_FLOOR:
        return Fraction(math.floor(x))
    if fn == abi.HSG_FN_ROUND:
        return Fraction(round(x))
    if fn == abi.HSG_FN_SIGN:
        return Fraction((x > 0) - (x < 0))
    if fn not in _FLOAT_FNS:
        raise TypeError(f"bad function {fn}")
    if (fn in (abi.HSG_FN_ASIN, abi.HSG_FN_ACOS) and not -1 <= x <= 1) or (fn == abi.HSG_FN_ACOSH and x < 1) or \
            (fn == abi.HSG_FN_ATANH and not -1 < x < 1) or \
            (fn in (abi.HSG_FN_LOG, abi.HSG_FN_LOG2, abi.HSG_FN_LOG10) and x <= 0) or (fn == abi.HSG_FN_SQRT and x < 0):
        raise MathematicalError("Mathematical error")
    try:
        r = _FLOAT_FNS[fn](float(x))
    except (OverflowError, ValueError):
        raise MathematicalError("the result is not finite")
    if not math.isfinite(r):
        raise MathematicalError("the result is not finite")
    return Fraction(r)


def _is_number(v) -> bool:
    # (a Fraction: a Number of an object gen_map_r built, read again by HAVING)
    return not isinstance(v, bool) and isinstance(v, (int, float, Fraction))


def _field_name(e: RExprCol) -> str:
    # composeColName (Internal/Codegen.hs): "stream.field" when the stream is named
    return e.field if e.stream is None else f"{e.stream}.{e.field}"


def _expr_value(e, value):
    """genRExprValue over a JSON object: the Number as an exact Fraction (a
    Scientific); raises KeyError for a missing field (getFieldByName,
    Internal/Codegen.hs:41-49), MathematicalError where a unary function
    does (unary_value) and TypeError for what binOpOnValue / compareValue /
    unaryOpOnValue have no numeric case for."""
    if isinstance(e, RExprCol):
        name = _field_name(e)
        if name not in value:
            raise KeyError(f"Key {name!r} is not found in object")
        v = value[name]
        if not _is_number(v):
            raise TypeError(f"field {name!r} is not a Number")
        return Fraction(v)
    if isinstance(e, RExprConst):
        if not _is_number(e.constant):
            raise TypeError("constant is not a Number")
        return Fraction(e.constant)
    if isinstance(e, RExprBinOp):
        a, b = _expr_value(e.expr1, value), _expr_value(e.expr2, value)
        if e.op == "OpAdd":
            return a + b
        if e.op == "OpSub":
            return a - b
        if e.op == "OpMul":
            return a * b
    if isinstance(e, RExprUnaryOp) and e.op in _FN_OPS:
        return unary_value(_FN_OPS[e.op], _expr_value(e.expr, value))
    raise TypeError(f"unsupported expression {e!r}")


expr_value = _expr_value


def gen_filter_r(cond, value) -> bool:
    """genFilterR (Codegen.hs:303-341) for one record's value object. Python
    evaluates as eagerly as Haskell evaluates lazily here: `or` / `and` look at
    the right side only when the left one did not decide, BETWEEN looks at its
    upper bound only when lower <= expr held, and every comparison needs both
    of its sides. Raises (KeyError) where the reference throws: the caller
    drops the record, as runTask does (Processor.hs:140-143)."""
    if cond is None:
        return True  # RWhereEmpty
    if isinstance(cond, RCondOp):
        a, b = _expr_value(cond.expr1, value), _expr_value(cond.expr2, value)
        return {"RCompOpEQ": a == b, "RCompOpNE": a != b, "RCompOpLT": a < b, "RCompOpGT": a > b,
                "RCompOpLEQ": a <= b, "RCompOpGEQ": a >= b}[cond.op]
    if isinstance(cond, RCondOr):
        return gen_filter_r(cond.cond1, value) or gen_filter_r(cond.cond2, value)
    if isinstance(cond, RCondAnd):
        return gen_filter_r(cond.cond1, value) and gen_filter_r(cond.cond2, value)
    if isinstance(cond, RCondNot):
        return not gen_filter_r(cond.cond, value)
    if isinstance(cond, RCondBetween):
        lo, x = _expr_value(cond.expr1, value), _expr_value(cond.expr, value)
        if lo > x:
            return False
        return not x > _expr_value(cond.expr2, value)
    raise TypeError(f"unsupported condition {cond!r}")


def where_fields(cond) -> List[str]:
    """The fields a condition reads, in first-use order."""
    out: List[str] = []

    def walk(n):
        if isinstance(n, RExprCol):
            if _field_name(n) not in out:
                out.append(_field_name(n))
        elif isinstance(n, (RExprBinOp, RCondOp)):
            walk(n.expr1), walk(n.expr2)
        elif isinstance(n, RExprUnaryOp):
            walk(n.expr)
        elif isinstance(n, (RCondAnd, RCondOr)):
            walk(n.cond1), walk(n.cond2)
        elif isinstance(n, RCondNot):
            walk(n.cond)
        elif isinstance(n, RCondBetween):
            walk(n.expr1), walk(n.expr), walk(n.expr2)

    walk(cond)
    return out


def _emit_expr(e, fields, key_field, what, prog, functions=False) -> int:
    """Append the value expression e to prog (postfix); returns the stack
    depth it needs. ValueError for what the program cannot say; a unary
    function is said (HSG_W_FN) only with functions=True."""
    if isinstance(e, RExprCol):
        name = _field_name(e)
        if key_field is not None and name == key_field:
            raise ValueError(f"{what} on the group key {name!r} is not pushed down")
        if name not in fields:
            raise ValueError(f"{what} reads {name!r}, which is not " +
                             ("an alias of the SELECT list" if what == "HAVING" else "a value column"))
        prog.append((abi.HSG_W_COL, fields.index(name)))
        return 1
    if isinstance(e, RExprConst):
        c = e.constant
        if not _is_number(c):
            raise ValueError(f"constant {c!r} is not a number: not pushed down")
        if isinstance(c, int):
            if not -2**63 <= c < 2**63:
                raise ValueError(f"integer constant {c} does not fit an i64")
            prog.append((abi.HSG_W_I64, c))
        else:
            if not math.isfinite(c):
                raise ValueError("non-finite constant")
            prog.append((abi.HSG_W_F64, c))
        return 1
    if isinstance(e, RExprBinOp):
        if e.op not in _BIN_OPS:
            raise ValueError(f"operator {e.op} is not pushed down")
        d1 = _emit_expr(e.expr1, fields, key_field, what, prog, functions)
        d2 = _emit_expr(e.expr2, fields, key_field, what, prog, functions)
        prog.append((_BIN_OPS[e.op],))
        return max(d1, 1 + d2)
    if isinstance(e, RExprUnaryOp):
        if not functions or e.op not in _FN_OPS:
            raise ValueError(f"unary function {e.op} is not pushed down")
        d = _emit_expr(e.expr, fields, key_field, what, prog, functions)
        prog.append((abi.HSG_W_FN, _FN_OPS[e.op]))
        return d
    raise ValueError(f"unsupported expression {e!r}")


def compile_expr(e, fields: Sequence[str], key_field: Optional[str] = None, what: str = "SELECT",
                 functions: bool = False) -> List[Tuple]:
    """A value expression (RExprCol / RExprConst / RExprBinOp / RExprUnaryOp
    tree) as a postfix value program, [(op,) | (op, arg)], over value columns
    named `fields` (column c = fields[c]): one expression of the op's map.
    ValueError for what the program cannot say, the same list as
    compile_where's. functions=True says the 22 numeric unary functions too
    ((HSG_W_FN, HSG_FN_*) after the operand); off by default, because the
    device's math library, not the host's, then rounds the float functions."""
    prog: List[Tuple] = []
    depth = _emit_expr(e, list(fields), key_field, what, prog, functions)
    if len(prog) > abi.HSG_MAP_MAX_INS:
        raise ValueError(f"{what} expression needs {len(prog)} instructions (max {abi.HSG_MAP_MAX_INS})")
    if depth > abi.HSG_WHERE_MAX_DEPTH:
        raise ValueError(f"{what} expression needs a stack of {depth} (max {abi.HSG_WHERE_MAX_DEPTH})")
    return prog


def expr_is_float(e, float_fields=()) -> bool:
    """The static type of a value expression: f64 iff a field that carries
    decimals or a float constant takes part; of the unary functions SIGN is
    an i64, ABS / CEIL / FLOOR / ROUND have their operand's type and every
    other one is an f64."""
    if isinstance(e, RExprCol):
        return _field_name(e) in float_fields
    if isinstance(e, RExprConst):
        return isinstance(e.constant, float)
    if isinstance(e, RExprBinOp):
        return expr_is_float(e.expr1, float_fields) or expr_is_float(e.expr2, float_fields)
    if isinstance(e, RExprUnaryOp) and e.op in _FN_OPS:
        fn = _FN_OPS[e.op]
        return expr_is_float(e.expr, float_fields) if fn in abi.HSG_FN_KEEP_TYPE else fn != abi.HSG_FN_SIGN
    return False


def compile_where(cond, fields: Sequence[str], key_field: Optional[str] = None, what: str = "WHERE",
                  functions: bool = False) -> List[Tuple]:
    """The condition as a postfix hsg_where_ins program, [(op,) | (op, arg)],
    over value columns named `fields` (column c = fields[c]). ValueError for
    what the program cannot say -- string / bool / null constants, a predicate
    on the group key, the reference's unary functions unless functions=True
    (compile_expr), a non-finite constant, a program past HSG_WHERE_MAX_INS or
    HSG_WHERE_MAX_DEPTH: such a WHERE stays upstream of the op (genFilterNode)."""
    fields = list(fields)
    prog: List[Tuple] = []

    def expr(e) -> int:
        return _emit_expr(e, fields, key_field, what, prog, functions)

    def search(c) -> int:
        if isinstance(c, RCondOp):
            if c.op not in _COMP_OPS:
                raise ValueError(f"bad comparison {c.op}")
            d1 = expr(c.expr1)
            d2 = expr(c.expr2)
            prog.append((_COMP_OPS[c.op],))
            return max(d1, 1 + d2)
        if isinstance(c, (RCondAnd, RCondOr)):
            d1 = search(c.cond1)
            d2 = search(c.cond2)
            prog.append((abi.HSG_W_AND if isinstance(c, RCondAnd) else abi.HSG_W_OR,))
            return max(d1, 1 + d2)
        if isinstance(c, RCondNot):
            d = search(c.cond)
            prog.append((abi.HSG_W_NOT,))
            return d
        if isinstance(c, RCondBetween):
            d1 = expr(c.expr1)
            d2 = expr(c.expr)
            d3 = expr(c.expr2)
            prog.append((abi.HSG_W_BETWEEN,))
            return max(d1, 1 + d2, 2 + d3)
        raise ValueError(f"unsupported condition {c!r}")

    depth = search(cond)
    if len(prog) > abi.HSG_WHERE_MAX_INS:
        raise ValueError(f"{what} needs {len(prog)} instructions (max {abi.HSG_WHERE_MAX_INS})")
    if depth > abi.HSG_WHERE_MAX_DEPTH:
        raise ValueError(f"{what} needs a stack of {depth} (max {abi.HSG_WHERE_MAX_DEPTH})")
    return prog


def compile_having(cond, aggs: Sequence, functions: bool = False) -> List[Tuple]:
    """The HAVING condition as the same postfix program over the op's
    aggregate outputs: column j is aggs[j] (P.Agg, or its alias), named by
    alias as the reference's filter reads the emitted object (genFilterR over
    {alias: Number}, Codegen.hs:524-529). The group key can be named only
    where it is also a SELECT passthrough (a LAST aggregate with that alias):
    no key-field rule. ValueError for a name that is no alias -- every record
    would throw in the reference -- for duplicate aliases, and for what
    compile_where cannot say; such a HAVING is not pushed down."""
    aliases = [a if isinstance(a, str) else a.alias for a in aggs]
    dup = sorted({a for a in aliases if aliases.count(a) > 1})
    if dup:
        raise ValueError(f"HAVING over duplicate aliases {dup} is not pushed down")
    return compile_where(cond, aliases, what="HAVING", functions=functions)


# SELECT items: ("COUNT(*)",) / ("COUNT", col) / ("SUM", col) / ("MIN", col) /
# ("MAX", col) / ("AVG", col) / ("COL", col); optional alias as last element.
# col: a field name, or a value expression (RExprCol / RExprConst / RExprBinOp).
SelItem = Tuple


def gen_aggregate_components(sel: List[SelItem], float_fields=(), key_field: Optional[str] = None,
                             functions: bool = False) -> List[P.Agg]:
    """genAggregateComponents (Codegen.hs:393-469). Where an item takes a
    column name it also takes a value expression (RExprBinOp / RExprConst /
    RExprCol tree): ("COL", expr) is genAggregateComponentsFromDerivedCol
    (Codegen.hs:463-469), the last record's genRExprValue, strict as the
    reference is (a record whose expression throws is dropped); an aggregate
    over an expression is this engine's, as AVG is, and skips such a record.
    The op's map pass evaluates the expression on the GPU. A tree that is just
    a column is the plain column. ValueError, and the query stays on the host,
    for what compile_expr cannot say (functions: as compile_expr)."""
    out = []
    for item in sel:
        kind, *rest = item
        alias = None
        if kind == "COUNT(*)":
            if rest:
                alias = rest[0]
            out.append(P.COUNT_ALL(alias or "COUNT(*)"))
            continue
        col = rest[0]
        alias = rest[1] if len(rest) > 1 else None
        strict = False
        if isinstance(col, RExprCol):
            col = _field_name(col)
        if isinstance(col, str):
            fl = col in float_fields
            cname = col
        else:
            names = where_fields(col)
            compile_expr(col, names, key_field, functions=functions)  # raises for what the program cannot say
            fl = expr_is_float(col, float_fields)
            cname = col.name
            col = P.Expr(col, tuple(f for f in names if f in float_fields), functions)
            strict = kind == "COL"
        if kind == "COUNT":
            out.append(P.COUNT(col, alias or f"COUNT({cname})"))
        elif kind == "SUM":
            out.append(P.SUM(col, alias or f"SUM({cname})", fl))
        elif kind == "MIN":
            out.append(P.MIN(col, alias or f"MIN({cname})", fl))
        elif kind == "MAX":
            out.append(P.MAX(col, alias or f"MAX({cname})", fl))
        elif kind == "AVG":
            # the reference throws "Unsupported aggregate function" (Codegen.hs:462);
            # this engine defines AVG = SUM(col) / COUNT(col)
            out.append(P.AVG(col, alias or f"AVG({cname})", fl))
        elif kind == "COL":
            out.append(P.LAST(col, alias or cname, fl, strict))
        else:
            raise ValueError(f"Unsupported aggregate function: {kind}")
    return out


def gen_group_by_node(engine, sel: List[SelItem], group_by: RGroupBy, emit=abi.HSG_EMIT_PER_RECORD,
                      float_fields=(), state_capacity=0, where=None, having=None, functions: bool = False) -> P.Table:
    """genGroupByNode: groupBy -> (timeWindowedBy | sessionWindowedBy)? -> aggregate.
    where: the query's RSearchCond, run by the op on the GPU where the
    reference chains genFilterNode in front (Codegen.hs:540); ValueError when
    compile_where cannot express it (the caller then filters upstream).
    having: the query's HAVING condition over the SELECT aliases, run by the
    op over the changelog rows it emits where the reference chains
    genFilteRNodeFromHaving behind the aggregate (Codegen.hs:524-529, :561-566);
    ValueError when compile_having cannot express it. As in the reference, it
    applies to an unwindowed GROUP BY only: for a windowed query (Codegen.hs:
    554-559 never looks at it) and for HSG_EMIT_NONE, which emits nothing, it
    is dropped silently. functions=True pushes the numeric unary functions of
    the SELECT list, WHERE and HAVING down too (compile_expr); by default a
    query that uses one raises ValueError and stays on the host."""
    grouped = P.groupBy(engine, group_by.column)
    aggs = gen_aggregate_components(sel, float_fields, key_field=group_by.column, functions=functions)
    mat = P.Materialized(state_capacity=state_capacity)
    if where is not None:
        where = P.Where(where, float_fields, functions)
    w = group_by.window
    if w is None:
        hv = P.Having(having, functions) if having is not None and emit != abi.HSG_EMIT_NONE else None
        return grouped.aggregate(aggs, mat, emit, where=where, having=hv)
    if isinstance(w, RTumblingWindow):
        return grouped.timeWindowedBy(P.mkTumblingWindow(diff_time_to_ms(w.seconds))).aggregate(aggs, mat, emit,
                                                                                               where=where)
    if isinstance(w, RHoppingWindow):
        return grouped.timeWindowedBy(
            P.mkHoppingWindow(diff_time_to_ms(w.length), diff_time_to_ms(w.hop))).aggregate(aggs, mat, emit,
                                                                                            where=where)
    if isinstance(w, RSessionWindow):
        return grouped.sessionWindowedBy(P.mkSessionWindows(diff_time_to_ms(w.seconds))).aggregate(aggs, mat, emit,
                                                                                                 where=where)
    raise ValueError("bad window")


# ---- SELECT without GROUP BY (RGroupByEmpty, Codegen.hs:542-550) ----------------
def _select_items(sel) -> List[Tuple[str, Any]]:
    """The SELECT list as [(alias, value expression)]; ValueError for an
    aggregate item (such a query has a GROUP BY branch of its own, or none)."""
    out = []
    for item in sel:
        kind, *rest = item
        if kind != "COL":
            raise ValueError(f"aggregate {kind} in a SELECT without GROUP BY is not pushed down")
        col = rest[0]
        alias = rest[1] if len(rest) > 1 else None
        if isinstance(col, str):
            col = RExprCol(col, None, col)
        out.append((alias or (_field_name(col) if isinstance(col, RExprCol) else col.name), col))
    return out


def gen_map_r(sel, value) -> dict:
    """genMapR (Codegen.hs:349-353) for one record's value object: the object
    {alias: Number} of the SELECT list's items (("COL", field or expression[,
    alias])), each an exact Fraction. Strict, as Data.HashMap.Strict.fromList
    is: raises (KeyError for a missing field, MathematicalError, TypeError)
    where any expression does, and the caller drops the record. Aliases given
    twice keep the later item, as fromList does."""
    return {alias: _expr_value(e, value) for alias, e in _select_items(sel)}


def gen_select_rows(sel, where, having, records) -> List[Tuple[int, int, Any]]:
    """The RGroupByEmpty chain over one batch of records ({"value": object,
    "timestamp": ts}): genFilterR where -> genMapR sel -> genFilterR having
    over the mapped object, a record that throws anywhere being dropped as
    runTask drops it. Returns [(index in the batch, timestamp, {alias:
    Fraction})] in arrival order; sel = "*" forwards the record's own object."""
    out = []
    for i, rec in enumerate(records):
        value = rec["value"]
        try:
            if not gen_filter_r(where, value):
                continue
            mapped = value if sel == "*" else gen_map_r(sel, value)
            if not gen_filter_r(having, mapped):
                continue
        except (KeyError, TypeError, ArithmeticError):
            continue
        out.append((i, rec["timestamp"], mapped))
    return out


def gen_select_node(engine, sel, where=None, having=None, float_fields=(), functions: bool = False,
                    literal_forms: bool = False, out_capacity: int = 0) -> P.Stream:
    """The RGroupByEmpty dispatch: genFilterNode whr -> genMapNode sel ->
    genFilteRNodeFromHaving hav (Codegen.hs:542-550) as one select op. The
    batch's columns are the fields WHERE and the SELECT list read, in first-use
    order. sel = "*" gives the index-only op (the host forwards the original
    records). ValueError -- the query then stays on the host -- for an
    aggregate item in the list, more than HSG_MAP_MAX_EXPRS items, duplicate
    aliases, a HAVING that names no alias, and everything compile_where /
    compile_expr / compile_having cannot say. The op is built on first use, so
    the refusals need no GPU."""
    items = None if sel == "*" else _select_items(sel)
    fields: List[str] = where_fields(where) if where is not None else []
    for _, e in items or []:
        for f in where_fields(e):
            if f not in fields:
                fields.append(f)
    st = P.Stream(engine, [(f, f in float_fields) for f in fields], literal_forms, out_capacity)
    if where is not None:
        st.filter(P.Where(where, float_fields, functions))
    if items is not None:
        st.map(items, functions)
    if having is not None:
        st.having(P.Having(having, functions))
    return st


# ---- FROM s1 INNER JOIN s2 WITHIN (...) ON s1.a = s2.b (Codegen.hs:219-266) ------
@dataclass(frozen=True)
class RFromJoin:
    """RFromJoin (s1, f1) (s2, f2) RJoinInner win (AST.hs:266): the two streams,
    the join field of each, and the WITHIN interval in seconds (a DiffTime)."""
    s1: str
    f1: str
    s2: str
    f2: str
    seconds: int
    join_type: str = "RJoinInner"


def gen_joiner(s1: str, s2: str, o1: dict, o2: dict) -> dict:
    """genJoiner (Internal/Codegen.hs:62-67): the union of both values with the
    field names prefixed "s1." / "s2.". HM.union is left-biased, so where a
    self-join (s1 == s2) gives both sides equal names, this side's value wins."""
    out = {f"{s2}.{k}": v for k, v in o2.items()}
    out.update({f"{s1}.{k}": v for k, v in o1.items()})
    return out


def gen_join_windows(frm: RFromJoin) -> Tuple[int, int]:
    """genJoinWindows (Codegen.hs:232-240): (jwBeforeMs, jwAfterMs), both the interval."""
    w = diff_time_to_ms(frm.seconds)
    return w, w


def _check_join(frm: RFromJoin):
    if frm.join_type != "RJoinInner":
        raise ValueError(f"join type {frm.join_type}: Impossible happened")  # Codegen.hs:267-268


def gen_join_rows(frm: RFromJoin, records, windows: Optional[Tuple[int, int]] = None) -> List[dict]:
    """The host mirror of the JOIN plan's source (genStreamWithSourceStream,
    Codegen.hs:253-266) over `records` of both streams in arrival order, each
    {"stream": s1 | s2, "key": record key or None, "value": object,
    "timestamp": ts}: joinStream's rows (processing.join_stream_rows) with
    genJoiner applied. Returns, in the order the reference forwards them,
    {"key": {"SelectedKey": join key}, "value": joined object, "timestamp":
    max of the two} -- the records gen_select_rows / a GROUP BY then read.
    windows = (before_ms, after_ms) replaces genJoinWindows' (the DSL's
    joinStream takes any JoinWindows)."""
    _check_join(frm)
    before, after = windows if windows is not None else gen_join_windows(frm)
    if frm.s1 == frm.s2 and any("side" not in r for r in records):
        raise ValueError("a self-join's records name their side: {'side': 0 | 1}")
    recs = [r if "side" in r else dict(r, side=0 if r["stream"] == frm.s1 else 1) for r in records]
    out = []
    for i, k, ts in P.join_stream_rows(before, after, recs, frm.f1, frm.f2):
        a, b = records[i], records[k]
        out.append({"key": {"SelectedKey": a["value"][frm.f1]}, "value": gen_joiner(frm.s1, frm.s2, a["value"], b["value"]),
                    "timestamp": ts})
    return out


def gen_join_node(engine, frm: RFromJoin, fields1: Sequence, fields2: Sequence, batch_capacity: int = 1 << 20,
                  windows: Optional[Tuple[int, int]] = None):
    """The RFromJoin branch of genStreamWithSourceStream as one valued GPU join
    (hsg_join_create_valued). fields1 / fields2: the numeric fields of each
    stream's value the rest of the query reads, each a name or (name,
    is_float). Returns (processing.JoinedStream, the joined column names
    "s1.f" ..., "s2.g" ...): gen_select_node / gen_group_by_node are then given
    those names as their fields, and JoinedStream.process_into hands every
    drained batch to their op on the device."""
    _check_join(frm)
    before, after = windows if windows is not None else gen_join_windows(frm)
    js = P.joinStream(engine, frm.s1, frm.s2, frm.f1, frm.f2, fields1, fields2, before, after, batch_capacity)
    return js, js.names
