"""GPU: the scalar SELECT op (hsg_op_create_select, k_select.hip): WHERE, the
SELECT list and HAVING of a query without GROUP BY, the kept rows compacted in
arrival order. The reference is always the host's: sql.gen_select_rows, the
exact-Fraction mirror of genFilterR + genMapR, or `expect`, a numpy
restatement of it in the manner of test_gpu_map.py::np_val that
test_restatement_is_the_mirror checks against the mirror once. Never the op.
Inputs are small integers and multiples of 1/4, so every + - * result is
exact and rows compare bit for bit, i64 and f64 alike."""
import ctypes as C
import json
import os
import uuid
from fractions import Fraction

import numpy as np
import pytest

from hstream_amd import abi, sql
from hstream_amd.columnar import Rows, narrow_columns
from util import F64_RTOL

pytestmark = pytest.mark.gpu

I, F = abi.HSG_I64, abi.HSG_F64
NONE = np.uint32(abi.HSG_KEY_NONE)
NAMES = ["a", "b", "c"]
TYPES = [I, F, I]
TSB = 1_700_000_000_000
FORMS = abi.HSG_OPF_LITERAL_FORMS
CAP = 1 << 19


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need cuda:0"
    from hstream_amd.engine import Engine
    e = Engine(device=0, batch_capacity=CAP)
    yield e
    e.close()


@pytest.fixture(scope="module")
def T():
    from hstream_amd.engine import select_tile_rows
    return select_tile_rows()


@pytest.fixture(scope="module")
def G():
    from hstream_amd.engine import select_grid_groups
    return select_grid_groups()


# ---- expressions and conditions ----------------------------------------------------------------------
def col(f):
    return sql.RExprCol(f, None, f)


def const(c):
    return sql.RExprConst(str(c), c)


def binop(op, l, r):
    return sql.RExprBinOp("", {"+": "OpAdd", "-": "OpSub", "*": "OpMul"}[op], l, r)


def fn(name, e):
    return sql.RExprUnaryOp(f"{name}(..)", "Op" + name.capitalize(), e)


def cmp(op, l, r):
    return sql.RCondOp({"=": "RCompOpEQ", "<": "RCompOpLT", ">": "RCompOpGT", "<=": "RCompOpLEQ",
                        ">=": "RCompOpGEQ"}[op], l, r)


A, B, C_ = col("a"), col("b"), col("c")
_d8 = A
for _k in range(7):  # a + (c + (a + (c + ...))): the stack reaches 8
    _d8 = binop("+", C_ if _k % 2 else A, _d8)


class Query:
    """where / having: conditions or None; sel: [(alias, tree)] (none: SELECT *)."""

    def __init__(self, sel=(), where=None, having=None, flags=0):
        self.sel, self.where, self.having, self.flags = list(sel), where, having, flags
        self.aliases = [a for a, _ in self.sel]

    def op(self, eng, **kw):
        return eng.select_op(
            TYPES, [sql.compile_expr(e, NAMES, functions=True) for _, e in self.sel],
            where=sql.compile_where(self.where, NAMES, functions=True) if self.where is not None else None,
            having=sql.compile_having(self.having, self.aliases, functions=True) if self.having is not None else None,
            flags=self.flags, **kw)

    def items(self):
        return [("COL", e, a) for a, e in self.sel]


# the workhorse: every stage can drop, i64 and f64 expressions, HAVING over both
Q = Query([("s", binop("+", A, C_)), ("p", binop("*", A, B)), ("q", binop("*", B, const(0.25)))],
          where=sql.RCondOr(cmp(">", A, const(-3)), cmp("<", B, const(-6.0))),
          having=sql.RCondAnd(cmp("<", col("s"), const(9)), cmp(">=", col("p"), const(-20.5))))


# ---- the numpy restatement -----------------------------------------------------------------------------
def np_val(e, names, cols, valids):
    """The value expression over whole columns, as the device types and computes
    it: (values, is f64, error, literal-form bit). ABS / FLOOR / SQRT are
    numpy's (IEEE: exact), LOG is the mirror's own sql.unary_value per element."""
    n = len(cols[0])
    if isinstance(e, sql.RExprCol):
        c = names.index(e.field)
        v = None if valids is None else valids[c]
        err = np.zeros(n, bool) if v is None else (v & 1) == 0
        form = np.zeros(n, bool) if v is None else (v & 2) != 0
        return cols[c], cols[c].dtype == np.float64, err, form
    if isinstance(e, sql.RExprConst):
        f = isinstance(e.constant, float)
        return (np.full(n, e.constant, np.float64 if f else np.int64), f, np.zeros(n, bool),
                np.full(n, f and not float(e.constant).is_integer()))
    if isinstance(e, sql.RExprBinOp):
        (x, fx, ex, mx), (y, fy, ey, my) = np_val(e.expr1, names, cols, valids), np_val(e.expr2, names, cols, valids)
        if fx or fy:
            x, y = x.astype(np.float64), y.astype(np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            return {"OpAdd": x + y, "OpSub": x - y, "OpMul": x * y}[e.op], fx or fy, ex | ey, mx | my
    x, fx, err, form = np_val(e.expr, names, cols, valids)
    name = e.op[2:].upper()
    if fx:
        err = err | ~np.isfinite(x)
    if name == "ABS":
        return np.abs(x), fx, err, form
    if name == "FLOOR":
        return (np.floor(x) + 0.0 if fx else x), fx, err, np.zeros(n, bool)
    xd = x.astype(np.float64)
    if name == "SQRT":
        err = err | (xd < 0)
        r = np.sqrt(np.where(err, 0.0, xd)) + 0.0
    else:
        assert name == "LOG"
        err = err.copy()
        r = np.zeros(n)
        for i in np.flatnonzero(~err):
            try:
                r[i] = float(sql.unary_value(abi.HSG_FN_LOG, Fraction(xd[i].item())))
            except sql.MathematicalError:
                err[i] = True
    r = np.where(err, 0.0, r)
    return r, True, err, ~err & (r != np.trunc(r))


def np_cond(c, names, cols, valids):
    """The condition, three-valued as include/hstream_gpu.h states it: (true, error)."""
    if isinstance(c, sql.RCondOp):
        (x, _, ex, _), (y, _, ey, _) = np_val(c.expr1, names, cols, valids), np_val(c.expr2, names, cols, valids)
        x, y = x.astype(np.float64), y.astype(np.float64)  # (small values: exact)
        with np.errstate(invalid="ignore"):
            t = {"RCompOpEQ": x == y, "RCompOpLT": x < y, "RCompOpGT": x > y, "RCompOpLEQ": x <= y,
                 "RCompOpGEQ": x >= y}[c.op]
        return t, ex | ey
    if isinstance(c, sql.RCondNot):
        t, e = np_cond(c.cond, names, cols, valids)
        return ~t, e
    if isinstance(c, sql.RCondBetween):
        (lo, _, elo, _), (x, _, ex, _), (hi, _, ehi, _) = (np_val(k, names, cols, valids)
                                                         for k in (c.expr1, c.expr, c.expr2))
        lo, x, hi = lo.astype(np.float64), x.astype(np.float64), hi.astype(np.float64)
        gt = lo > x
        return ~gt & (x <= hi), elo | ex | (~gt & ehi)
    (l, el), (r, er) = np_cond(c.cond1, names, cols, valids), np_cond(c.cond2, names, cols, valids)
    take_l = el | (~l if isinstance(c, sql.RCondAnd) else l)
    return np.where(take_l, l, r), np.where(take_l, el, er)


class Want:
    pass


def expect(q, batch, base=0):
    """The rows the op must append for the batch, and its four counters."""
    key, ts, cols, valids = batch
    n = len(ts)
    live = np.ones(n, bool) if key is None else key != NONE
    if q.where is not None:
        t, e = np_cond(q.where, NAMES, cols, valids)
        w = t & ~e
    else:
        w = np.ones(n, bool)
    vals = [np_val(e, NAMES, cols, valids) for _, e in q.sel]
    bad = np.zeros(n, bool)
    for _, _, err, _ in vals:
        bad |= err
    if q.having is not None:
        # HAVING reads the expressions by alias; an f64 value that is NaN is the error value
        hc = [np.where(err, 0, v).astype(v.dtype) for v, _, err, _ in vals]
        hv = [(~(err | (np.isnan(v) if f else False))).astype(np.uint8) for v, f, err, _ in vals]
        t, e = np_cond(q.having, q.aliases, hc, hv)
        h = t & ~e
    else:
        h = np.ones(n, bool)
    keep = live & w & ~bad & h
    k = np.flatnonzero(keep)
    out = Want()
    out.keep = keep
    out.rows = Rows((np.full(len(k), NONE) if key is None else key[k]).astype(np.uint32), ts[k], ts[k],
                    (base + k).astype(np.int64), [v[k] for v, _, _, _ in vals], None)
    form = np.zeros(n, np.uint32)
    for j, (_, _, _, fm) in enumerate(vals):
        form |= (~fm).astype(np.uint32) << (2 * j)
    out.rows.form = form[k]
    out.f64 = [f for _, f, _, _ in vals]
    out.stats = dict(where_dropped=int(np.count_nonzero(live & ~w)), expr_dropped=int(np.count_nonzero(live & w & bad)),
                     having_dropped=int(np.count_nonzero(live & w & ~bad & ~h)), emitted=len(k))
    out.wm = int(ts.max()) if n else None
    return out


def same_rows(got, want, f64, what, forms=False, close=()):
    assert len(got) == len(want.key_id), (what, len(got), len(want.key_id))
    np.testing.assert_array_equal(got.src_index, want.src_index, err_msg=f"{what}: src_index")
    np.testing.assert_array_equal(got.key_id, want.key_id, err_msg=f"{what}: key_id")
    np.testing.assert_array_equal(got.win_start, want.win_start, err_msg=f"{what}: win_start")
    np.testing.assert_array_equal(got.win_end, want.win_end, err_msg=f"{what}: win_end")
    assert len(got.aggs) == len(want.aggs), what
    for j, (g, w) in enumerate(zip(got.aggs, want.aggs)):
        assert g.dtype == (np.float64 if f64[j] else np.int64), (what, j)
        if j in close:
            np.testing.assert_allclose(g, w, rtol=F64_RTOL, atol=0.0, err_msg=f"{what}: expr {j}")
        else:
            np.testing.assert_array_equal(g.view(np.int64), np.ascontiguousarray(w).view(np.int64),
                                          err_msg=f"{what}: expr {j}")
    if forms:
        np.testing.assert_array_equal(got.form, want.form, err_msg=f"{what}: form")


def concat(ws):
    return Rows(*(np.concatenate([getattr(w, f) for w in ws]) for f in ("key_id", "win_start", "win_end", "src_index")),
                [np.concatenate([w.aggs[j] for w in ws]) for j in range(len(ws[0].aggs))],
                np.concatenate([w.form for w in ws]))


def check_stats(g, wants, what=""):
    st = g.select_stats()
    for k, v in wants[-1].stats.items():
        assert st[k] == v, (what, k, st)
        assert st[k + "_total"] == sum(w.stats[k] for w in wants), (what, k + "_total", st)


def push_check(g, q, batch, base=0, wm=-1, what="", forms=False, close=()):
    """One batch through the op, drained, against expect()."""
    key, ts, cols, valids = batch
    want = expect(q, batch, base)
    got_wm = g.push(key, ts, cols, valids, watermark=wm)
    assert got_wm == (max(wm, want.wm) if want.wm is not None else wm), what
    assert g.pending() == len(want.rows.key_id), what
    same_rows(g.drain(), want.rows, want.f64, what, forms, close)
    return want, got_wm


def gen(seed, n, absent=0.2, none=0.05, vr=8, t0=TSB, span=200_000):
    """Columns [I64, F64, I64]: small integers and multiples of 1/4, ~20 %
    absent per column, bit 1 of every valid byte random, a few HSG_KEY_NONE."""
    rng = np.random.default_rng(seed)
    key = rng.integers(0, 50, size=n).astype(np.uint32)
    key[rng.random(n) < none] = NONE
    ts = (t0 + (np.arange(n, dtype=np.int64) * span) // max(1, n) + rng.integers(0, 2000, size=n)).astype(np.int64)
    cols = [rng.integers(-vr, vr + 1, size=n).astype(np.int64),
            rng.integers(-4 * vr, 4 * vr + 1, size=n).astype(np.float64) / 4.0,
            rng.integers(-vr, vr + 1, size=n).astype(np.int64)]
    valids = [((rng.random(n) >= absent).astype(np.uint8) | (rng.integers(0, 2, size=n).astype(np.uint8) << 1))
              for _ in cols]
    return key, ts, cols, valids


def records_of(batch):
    key, ts, cols, valids = batch
    return [{"value": {f: c[i].item() for f, c, v in zip(NAMES, cols, valids) if v[i] & 1}, "timestamp": int(ts[i])}
            for i in range(len(ts))]


# ---- 0. the restatement is the mirror --------------------------------------------------------------------
QUERIES = {
    "workhorse": Q,
    "no where": Query(Q.sel, None, Q.having),
    "no having": Query(Q.sel, Q.where, None),
    "star": Query((), Q.where, None),
    "one expr": Query([("s", binop("-", A, C_))], None, cmp(">", col("s"), const(0))),
    "between, not": Query([("s", binop("+", A, C_)), ("b", B)], sql.RCondNot(cmp("=", A, const(0))),
                          sql.RCondBetween(const(-2), col("s"), col("b"))),
    "exact fns": Query([("f", fn("FLOOR", B)), ("r", fn("SQRT", A)), ("m", fn("ABS", binop("*", A, B)))],
                       cmp(">", fn("ABS", B), const(0.5)), cmp("<", col("r"), const(2.5))),
}


@pytest.mark.parametrize("name", list(QUERIES))
def test_restatement_is_the_mirror(name):
    """expect() gives, record by record, what sql.gen_select_rows gives (runs no GPU code)."""
    q = QUERIES[name]
    batch = gen(3, 1500)
    want = expect(q, batch)
    recs = records_of(batch)
    live = [i for i in range(len(recs)) if batch[0][i] != NONE]
    ref = sql.gen_select_rows(q.items() if q.sel else "*", q.where, q.having, [recs[i] for i in live])
    assert [live[i] for i, _, _ in ref] == list(want.rows.src_index)
    assert [t for _, t, _ in ref] == list(want.rows.win_start)
    for j, a in enumerate(q.aliases):
        assert [m[a] for _, _, m in ref] == [Fraction(v.item()) for v in want.rows.aggs[j]], (name, a)
    s = want.stats
    assert s["emitted"] > 20 and (q.where is None or s["where_dropped"] > 20), s
    assert (not q.sel or s["expr_dropped"] > 20) and (q.having is None or s["having_dropped"] > 20), s


# ---- 1. lengths: the tile, look-back and ticket edges -------------------------------------------------------
LENGTHS = {"0": lambda T, G: 0, "1": lambda T, G: 1, "63": lambda T, G: 63, "64": lambda T, G: 64,
           "65": lambda T, G: 65, "T-1": lambda T, G: T - 1, "T": lambda T, G: T, "T+1": lambda T, G: T + 1,
           "2T+1": lambda T, G: 2 * T + 1,
           "64T+1": lambda T, G: 64 * T + 1,          # the look-back's second round
           "(G+1)T+1": lambda T, G: (G + 1) * T + 1}  # workgroups take a second ticket


@pytest.mark.parametrize("length", list(LENGTHS))
def test_lengths(eng, T, G, length):
    n = LENGTHS[length](T, G)
    assert n <= CAP
    g = Q.op(eng)
    try:
        want, _ = push_check(g, Q, gen(n + 11, n), what=f"n={length}")
        check_stats(g, [want], length)
        if n > 64:
            assert 0 < want.stats["emitted"] < n
        assert g.stats()["records"] == n and g.stats()["batches"] == 1
    finally:
        g.close()


# ---- 2. keep patterns: every stage alone and together, the four counters --------------------------------------
# a > 0 is WHERE, b's presence the expression's error, c > 0 HAVING (over the alias h = c + 0)
PQ = Query([("v", binop("*", B, const(2))), ("h", binop("+", C_, const(0)))], cmp(">", A, const(0)),
           cmp(">", col("h"), const(0)))


def pattern_batch(w, e, h, none=None):
    n = len(w)
    key = (np.arange(n) % 7).astype(np.uint32)
    if none is not None:
        key[none] = NONE
    ts = TSB + np.arange(n, dtype=np.int64) * 3
    cols = [np.where(w, 2, -2).astype(np.int64), (np.arange(n) % 9 - 4).astype(np.float64) / 4.0,
            np.where(h, 1, -1).astype(np.int64)]
    valids = [np.ones(n, np.uint8), (~e).astype(np.uint8), np.ones(n, np.uint8)]
    return key, ts, cols, valids


def _patterns(n, T):
    rng = np.random.default_rng(n)
    yes, no = np.ones(n, bool), np.zeros(n, bool)
    i = np.arange(n)
    rnd = [rng.random(n) < 0.6 for _ in range(3)]
    return {
        "all kept": (yes, no, yes),
        "none kept": (no, no, yes),
        "alternating": (i % 2 == 0, no, yes),
        "a tile dropped then kept": (i >= T, no, yes),
        "a tile kept then dropped": (yes, no, i < T),
        "only the last": (yes, i != n - 1, yes),
        "where alone": (rnd[0], no, yes),
        "expression alone": (yes, ~rnd[1], yes),
        "having alone": (yes, no, rnd[2]),
        "all three": (rnd[0], ~rnd[1], rnd[2]),
    }


@pytest.mark.parametrize("name", list(_patterns(8, 4)))
def test_keep_patterns(eng, T, name):
    n = 3 * T + 5
    w, e, h = _patterns(n, T)[name]
    none = np.arange(n) % 41 == 40
    batch = pattern_batch(w, e, h, none)
    want = expect(PQ, batch)
    live = ~none
    assert want.stats == dict(where_dropped=int(np.count_nonzero(live & ~w)),
                              expr_dropped=int(np.count_nonzero(live & w & e)),
                              having_dropped=int(np.count_nonzero(live & w & ~e & ~h)),
                              emitted=int(np.count_nonzero(live & w & ~e & h))), name
    g = PQ.op(eng)
    try:
        w1, _ = push_check(g, PQ, batch, what=name)
        check_stats(g, [w1], name)
    finally:
        g.close()


# ---- 3. program shapes -------------------------------------------------------------------------------------
E8 = [("e0", binop("+", A, C_)), ("e1", binop("*", A, B)), ("e2", binop("-", A, C_)), ("e3", A), ("e4", B),
      ("e5", binop("*", binop("+", A, C_), binop("-", A, C_))), ("e6", const(7)), ("e7", binop("*", B, const(0.25)))]
SHAPES = {
    "0 expressions": Query((), cmp(">", A, const(0))),
    "0 expressions, no where": Query(()),
    "1 expression": Query(E8[:1], Q.where, cmp("<", col("e0"), const(4))),
    "8 expressions": Query(E8, Q.where, sql.RCondOr(cmp(">", col("e7"), const(0.25)), cmp("=", col("e6"), col("e3")))),
    "no where": Query(Q.sel, None, Q.having),
    "no having": Query(Q.sel, Q.where, None),
    "neither": Query(Q.sel),
    "depth 8": Query([("d", _d8)], None, cmp(">", col("d"), const(0))),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_program_shapes(eng, T, name):
    q = SHAPES[name]
    g = q.op(eng)
    try:
        want, _ = push_check(g, q, gen(31, 2 * T + 77), what=name)
        check_stats(g, [want], name)
        assert want.stats["emitted"] > 50, want.stats
        assert len(g.drain().aggs) == len(q.sel)
    finally:
        g.close()


def test_nan_under_having_drops_the_row(eng, T):
    """x = b * 1e308 * 1e308 is +-inf for b != 0 (no error: arithmetic has no
    finiteness rule), x - x is NaN: HAVING reads a NaN as its error value and
    drops the row; b = 0 gives 0 - 0 = 0 and stays."""
    big = binop("*", binop("*", B, const(1e308)), const(1e308))
    q = Query([("x", binop("-", big, big)), ("b", B)], None, cmp(">=", col("x"), const(0)))
    batch = gen(41, T + 9, none=0.0)
    want = expect(q, batch)
    b, present = batch[2][1], (batch[3][1] & 1) == 1
    np.testing.assert_array_equal(want.keep, present & (b == 0))
    assert want.stats["having_dropped"] == int(np.count_nonzero(present & (b != 0))) > 100
    assert want.stats["emitted"] > 2
    g = q.op(eng)
    try:
        w1, _ = push_check(g, q, batch, what="nan")
        check_stats(g, [w1], "nan")
    finally:
        g.close()
    # without HAVING the same rows are emitted, NaN and all
    q2 = Query(q.sel)
    g = q2.op(eng)
    try:
        push_check(g, q2, batch, what="nan, no having")
    finally:
        g.close()


# ---- 4. function classes --------------------------------------------------------------------------------------
def fn_gen(seed, n):
    """test_gpu_fn.py's operands: as gen, but b is never 0 or 1 (LOG(b) = 0 would hang a comparison on the last bit)."""
    key, ts, cols, valids = gen(seed, n)
    b = cols[1]
    cols[1] = np.where((b == 0) | (b == 1), b + 0.125, b)
    return key, ts, cols, valids


def test_function_class_1_exact(eng, T):
    from hstream_amd.engine import prog_fn_class
    q = QUERIES["exact fns"]
    assert prog_fn_class(sql.compile_where(q.where, NAMES, functions=True)) == 1
    g = q.op(eng)
    try:
        want, _ = push_check(g, q, fn_gen(51, 2 * T + 3), what="class 1")
        check_stats(g, [want], "class 1")
        # SQRT of a negative a is a domain error: the record is dropped by the expression
        assert want.stats["expr_dropped"] > want.stats["emitted"] > 10
    finally:
        g.close()


def test_function_class_2_domain_errors_drop_the_record(eng, T):
    """SQRT(a) and LOG(b): a < 0 and b <= 0 are domain errors and drop the
    record, exactly; LOG's values within F64_RTOL (test_gpu_fn.py's bound)."""
    q = Query([("r", fn("SQRT", A)), ("l", fn("LOG", B)), ("s", binop("+", A, C_))], cmp(">", C_, const(-6)),
              cmp("<", col("r"), const(2.9)))
    batch = fn_gen(52, 2 * T + 3)
    want = expect(q, batch)
    a, b = batch[2][0], batch[2][1]
    ok = (batch[0] != NONE) & (batch[3][0] & batch[3][1] & batch[3][2] & 1 == 1) & (batch[2][2] > -6)
    assert want.stats["expr_dropped"] >= int(np.count_nonzero(ok & ((a < 0) | (b <= 0)))) > 50
    assert not np.any(want.keep & ((a < 0) | (b <= 0))) and want.stats["emitted"] > 10
    g = q.op(eng)
    try:
        w1, _ = push_check(g, q, batch, what="class 2", close=(1,))
        check_stats(g, [w1], "class 2")
    finally:
        g.close()


# ---- 5. literal forms -----------------------------------------------------------------------------------------
def test_literal_forms(eng, T):
    """bit 2j = expression j prints as an integer: no operand's literal had a
    negative exponent (bit 1 of its valid byte) and no constant is a non-integral
    f64. a + c follows its operands, b * 0.25 is always decimal; bit 2j + 1 is never set."""
    q = Query([("s", binop("+", A, C_)), ("p", binop("*", A, B)), ("q", binop("*", B, const(0.25))), ("a", A)],
              Q.where, None, flags=FORMS)
    batch = gen(61, 2 * T + 9)
    want = expect(q, batch)
    kept = np.flatnonzero(want.keep)
    va, vb, vc = (v[kept] for v in batch[3])
    np.testing.assert_array_equal(want.rows.form & 1, ((va | vc) >> 1 & 1) ^ 1)
    np.testing.assert_array_equal(want.rows.form >> 2 & 1, ((va | vb) >> 1 & 1) ^ 1)
    assert not np.any(want.rows.form >> 4 & 1) and 0 < np.count_nonzero(want.rows.form & 1) < len(kept)
    np.testing.assert_array_equal(want.rows.form >> 6 & 1, (va >> 1 & 1) ^ 1)
    g = q.op(eng)
    try:
        push_check(g, q, batch, what="forms", forms=True)
        g.push(*batch[:2], batch[2], batch[3])
        assert not np.any(g.drain().form & 0xAAAAAAAA)
    finally:
        g.close()
    # without the flag the rows carry no form
    g = Query(q.sel, q.where).op(eng)
    try:
        g.push(*batch[:2], batch[2], batch[3])
        assert g.drain().form is None
    finally:
        g.close()


# ---- 6. segments: pending rows, drains, capacity ----------------------------------------------------------------
def test_two_pushes_without_a_drain(eng, T):
    g = Q.op(eng, out_capacity=8 * T)
    try:
        b1, b2 = gen(71, 2 * T + 3), gen(72, 3 * T + 1, t0=TSB + 300_000)
        w1, w2 = expect(Q, b1), expect(Q, b2, base=len(b1[0]))
        assert w1.stats["emitted"] % T != 0  # the second segment starts inside a tile's worth of rows
        wm = g.push(*b1, watermark=-1)
        assert g.pending() == w1.stats["emitted"]
        wm = g.push(*b2, watermark=wm)
        assert wm == max(w1.wm, w2.wm) and g.pending() == w1.stats["emitted"] + w2.stats["emitted"]
        same_rows(g.drain(), concat([w1.rows, w2.rows]), w1.f64, "two segments")
        check_stats(g, [w1, w2], "two segments")
        # a drain in between: the third batch starts at row 0 again, src_index goes on
        b3 = gen(73, T + 5, t0=TSB + 600_000)
        w3, _ = push_check(g, Q, b3, base=len(b1[0]) + len(b2[0]), wm=wm, what="after the drain")
        check_stats(g, [w1, w2, w3], "after the drain")
        assert g.stats()["records"] == len(b1[0]) + len(b2[0]) + len(b3[0]) and g.stats()["batches"] == 3
    finally:
        g.close()


def test_capacity_is_the_worst_case_and_changes_nothing(eng, T):
    n1, n2 = T + 7, 2 * T
    b1, b2 = gen(81, n1), gen(82, n2, t0=TSB + 300_000)
    w1 = expect(Q, b1)
    g = Q.op(eng, out_capacity=w1.stats["emitted"] + n2 - 1)  # one row short of pending + n
    try:
        wm = g.push(*b1, watermark=-1)
        st, ss = g.stats(), g.select_stats()
        with pytest.raises(abi.HStreamGpuError) as ei:
            g.push(*b2, watermark=wm)
        assert ei.value.status == abi.HSG_E_CAPACITY
        assert g.pending() == w1.stats["emitted"] and g.select_stats() == ss
        st2 = g.stats()
        assert all(st2[k] == st[k] for k in ("batches", "records", "pending_rows")), (st, st2)
        same_rows(g.drain(), w1.rows, w1.f64, "after the refusal")
        w2, _ = push_check(g, Q, b2, base=n1, wm=wm, what="retry after the drain")
        check_stats(g, [w1, w2], "retry")
    finally:
        g.close()


def test_registered_changelog_columns(eng, T):
    import torch
    cap = 1 << 12
    g = Q.op(eng)
    dev = {k: torch.empty(cap, dtype=t, device="cuda") for k, t in
           (("key", torch.int32), ("ws", torch.int64), ("we", torch.int64), ("src", torch.int64))}
    f64 = [False, True, True]
    aggs = [torch.empty(cap, dtype=torch.float64 if f else torch.int64, device="cuda") for f in f64]
    ap = (C.c_void_p * len(aggs))(*[a.data_ptr() for a in aggs])
    rows = abi.hsg_rows(capacity=cap, mem=abi.HSG_MEM_DEVICE, n_aggs=len(aggs), key_id=dev["key"].data_ptr(),
                        win_start=dev["ws"].data_ptr(), win_end=dev["we"].data_ptr(), src_index=dev["src"].data_ptr(),
                        aggs=C.cast(ap, C.POINTER(C.c_void_p)))
    try:
        g.set_changelog(rows)
        base = 0
        for bi in range(2):
            batch = gen(90 + bi, 3 * T + 5)
            want = expect(Q, batch, base)
            g.push(*batch)
            n = g.drain_count()
            assert n == want.stats["emitted"] > 0
            torch.cuda.synchronize()
            got = Rows(dev["key"][:n].cpu().numpy().view(np.uint32), dev["ws"][:n].cpu().numpy(),
                       dev["we"][:n].cpu().numpy(), dev["src"][:n].cpu().numpy(), [a[:n].cpu().numpy() for a in aggs])
            same_rows(got, want.rows, want.f64, f"registered columns batch {bi}")
            base += len(batch[0])
        # the registered columns bound the room check
        with pytest.raises(abi.HStreamGpuError) as ei:
            g.push(*gen(93, cap + 1))
        assert ei.value.status == abi.HSG_E_CAPACITY
        g.set_changelog(None)
        push_check(g, Q, gen(94, T), base=base, what="own buffer again")
    finally:
        g.close()


# ---- 7. transports ---------------------------------------------------------------------------------------------
def test_device_resident_batch(eng, T):
    import torch
    batch = gen(101, 2 * T + 1)
    key, ts, cols, valids = batch
    want = expect(Q, batch)
    g = Q.op(eng)
    try:
        d = lambda x: torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()
        dk, dts, dc, dv = d(key), d(ts), [d(c) for c in cols], [d(v) for v in valids]
        torch.cuda.synchronize()
        assert g.push(dk, dts, dc, dv, watermark=-1) == want.wm
        same_rows(g.drain(), want.rows, want.f64, "device batch")
        # the caller's arrays are only read
        np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint32), key)
        # a ready event instead of a synchronised producer
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            dk2 = d(key)
            ev = torch.cuda.Event()
            ev.record(s)
        from hstream_amd.columnar import make_batch
        b, keep = make_batch(dk2, dts, dc, dv)
        b.ready_event = ev.cuda_event
        g.push_batch(b)
        same_rows(g.drain(), expect(Q, batch, base=len(key)).rows, want.f64, "ready_event")
    finally:
        g.close()


def test_narrow_transport_batch(eng, T):
    batch = gen(111, 2 * T + 1)
    key, ts, cols, valids = batch
    nts, base, ncols, enc, scale = narrow_columns(ts, cols, TYPES, dec_scale=[None, 2, None])
    assert base is not None and enc == [abi.HSG_ENC_I32, abi.HSG_ENC_DEC32, abi.HSG_ENC_I32]
    want = expect(Q, batch)
    g = Q.op(eng)
    try:
        assert g.push(key, nts, ncols, valids, ts_base=base, col_enc=enc, col_scale=scale) == want.wm
        same_rows(g.drain(), want.rows, want.f64, "narrow")
    finally:
        g.close()


def test_batch_without_keys(eng, T):
    """key_id = NULL: every record is live and its row carries HSG_KEY_NONE."""
    _, ts, cols, valids = gen(121, 2 * T + 1)
    batch = (None, ts, cols, valids)
    want = expect(Q, batch)
    assert np.all(want.rows.key_id == NONE) and want.stats["emitted"] > 50
    g = Q.op(eng)
    try:
        w1, _ = push_check(g, Q, batch, what="no keys")
        check_stats(g, [w1], "no keys")
    finally:
        g.close()


def test_async_pushes(eng, T):
    batches = [gen(130 + k, 3 * T + k, t0=TSB + k * 250_000) for k in range(3)]
    g = Q.op(eng)
    try:
        wm = C.c_int64(-1)
        rcs = []
        for key, ts, cols, valids in batches:
            g.push_async(key, ts, cols, valids, watermark=wm, done=rcs.append)
        g.wait()
        assert rcs == [abi.HSG_OK] * 3
        wants, base = [], 0
        for b in batches:
            wants.append(expect(Q, b, base))
            base += len(b[0])
        assert wm.value == max(w.wm for w in wants)
        assert g.pending() == sum(w.stats["emitted"] for w in wants)
        same_rows(g.drain(), concat([w.rows for w in wants]), wants[0].f64, "async")
        check_stats(g, wants, "async")
    finally:
        g.close()


# ---- 8. the op among the other calls ------------------------------------------------------------------------------
def test_reset_keeps_the_programs_and_the_totals(eng, T):
    g = Q.op(eng)
    try:
        wants = []
        for bi in range(2):
            batch = gen(140 + bi, 2 * T + 9)
            g.push(*gen(149, T))  # rows left pending: the reset drops them
            wants.append(expect(Q, gen(149, T)))
            g.reset()
            assert g.pending() == 0
            w, _ = push_check(g, Q, batch, base=0, what=f"run {bi}")  # a reset op numbers its records from 0
            wants.append(w)
            check_stats(g, wants, f"run {bi}")
        assert g.stats()["batches"] == 4
    finally:
        g.close()


def test_state_calls_are_refused(eng, T):
    g = Q.op(eng)
    try:
        g.push(*gen(151, T))
        n = C.c_uint64(99)
        assert g._lib.hsg_state_rows(g._h, C.byref(n)) == abi.HSG_OK and n.value == 0
        for call in (g.dump_state, lambda: g.view_get([1]), lambda: g.table_join([1])):
            with pytest.raises(abi.HStreamGpuError) as ei:
                call()
            assert ei.value.status == abi.HSG_E_INVALID
        assert g.pending() == expect(Q, gen(151, T)).stats["emitted"]  # untouched
    finally:
        g.close()


def test_refusals(eng):
    with pytest.raises(abi.HStreamGpuError) as ei:
        eng.select_op(TYPES, [[(abi.HSG_W_COL, 3)]])
    assert ei.value.status == abi.HSG_E_INVALID and "column 3 out of range" in str(ei.value)
    with pytest.raises(abi.HStreamGpuError) as ei:
        eng.select_op(TYPES, [[(abi.HSG_W_COL, 0)]], flags=2)
    assert ei.value.status == abi.HSG_E_INVALID and "bad flags" in str(ei.value)
    # hsg_op_select_stats is the select op's alone
    from hstream_amd.columnar import OpSpec
    plain = eng.op(OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[I], aggs=[(abi.HSG_SUM, 0)],
                          state_capacity=1 << 10))
    try:
        with pytest.raises(abi.HStreamGpuError):
            plain.select_stats()
    finally:
        plain.close()


# ---- 9. two ranks over the host transport: the op is local ---------------------------------------------------------
def _rank_slices(R):
    out = []
    for b in range(3):
        key, ts, cols, valids = gen(200 + b, 4000, t0=TSB + b * 20_000, span=20_000)
        cuts = np.linspace(0, len(key), R + 1).astype(int)
        out.append([(key[cuts[r]:cuts[r + 1]], ts[cuts[r]:cuts[r + 1]], [c[cuts[r]:cuts[r + 1]] for c in cols],
                     [v[cuts[r]:cuts[r + 1]] for v in valids]) for r in range(R)])
    return out


def _rank_worker(rank, R, name, q):
    try:
        from hstream_amd.engine import Engine
        e = Engine(device=0, rank=rank, nranks=R, comm_id=name, batch_capacity=1 << 13,
                   transport=abi.HSG_TRANSPORT_HOST)
        op = Q.op(e)
        wm, out = -1, []
        for slices in _rank_slices(R):
            wm = op.push(*slices[rank], watermark=wm)
            rows = op.drain()
            out.append(([rows.key_id, rows.win_start, rows.win_end, rows.src_index] + rows.aggs, op.select_stats()))
        op.close()
        e.close()
        q.put((rank, wm, out))
    except Exception as ex:  # reported to the parent, which fails the test
        q.put((rank, "error", repr(ex)))


def test_two_ranks_filter_their_own_slices():
    import multiprocessing as mp
    R = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = f"hsgs-{os.getpid()}-{uuid.uuid4().hex[:12]}"
    procs = [ctx.Process(target=_rank_worker, args=(r, R, name, q)) for r in range(R)]
    for p in procs:
        p.start()
    try:
        outs = [q.get(timeout=100) for _ in range(R)]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    errs = [o for o in outs if o[1] == "error"]
    assert not errs, errs
    outs.sort(key=lambda o: o[0])
    for r in range(R):
        base, wm, wants = 0, -1, []
        for bi, slices in enumerate(_rank_slices(R)):
            # a rank's rows are its own slice's, numbered by its own records; no record crosses
            want = expect(Q, slices[r], base)
            wants.append(want)
            arrs, st = outs[r][2][bi]
            got = Rows(arrs[0], arrs[1], arrs[2], arrs[3], arrs[4:], None)
            same_rows(got, want.rows, want.f64, f"rank {r} batch {bi}")
            assert 0 < len(got) < len(slices[r][0])
            for k, v in want.stats.items():
                assert st[k] == v and st[k + "_total"] == sum(w.stats[k] for w in wants), (r, bi, k)
            base += len(slices[r][0])
            wm = max(wm, want.wm)
        assert outs[r][1] == wm  # stream time is the rank's own too


# ---- 10. DSL and SQL end to end ----------------------------------------------------------------------------------
def _json_records(batch):
    recs = records_of(batch)
    for i, r in enumerate(recs):
        if i % 17 == 3:
            r["value"]["note"] = "a string the query never reads"
    return recs


@pytest.mark.parametrize("forms", [False, True], ids=["plain", "literal forms"])
def test_sql_end_to_end_through_the_sink(eng, T, forms):
    from hstream_amd import ingest
    from hstream_amd.sink import member_order
    sel = [("COL", binop("+", A, C_), "s"), ("COL", binop("*", A, B), "p"), ("COL", "b"), ("COL", "a", "alpha")]
    where = cmp(">", A, const(-5))
    having = cmp("<", col("s"), const(6))
    st = sql.gen_select_node(eng, sel, where, having, float_fields=("b",), literal_forms=forms, out_capacity=1 << 12)
    try:
        batch = gen(301, 2 * T + 9)
        recs = _json_records(batch)
        ref = sql.gen_select_rows(sel, where, having, recs)
        assert 50 < len(ref) < len(recs) - 50
        buf, off = ingest.pack_records([json.dumps(r["value"]).encode() for r in recs])
        wm, out = st.process_json(buf, off, batch[1], watermark=-1)
        assert wm == int(batch[1].max())
        assert [o["timestamp"] for o in out] == [t for _, t, _ in ref]
        assert [{k: Fraction(v) for k, v in o["value"].items()} for o in out] == [m for _, _, m in ref]
        np.testing.assert_array_equal(st.last_rows.src_index, [i for i, _, _ in ref])
        # the sink: empty key records, the value object {alias: number} in aeson's member order
        sink = st.sink()
        pairs = sink.encode(st.last_rows)
        sink.close()
        aliases = ["s", "p", "b", "alpha"]
        order = [aliases[m] for m in member_order(aliases)]
        assert len(pairs) == len(ref)
        for (kb, vb), (_, _, m) in zip(pairs, ref):
            assert kb == b""
            members = json.loads(vb.decode(), object_pairs_hook=list, parse_float=Fraction, parse_int=Fraction)
            assert [k for k, _ in members] == order
            assert dict(members) == m
        # the same stream through process (the DSL's records), numbered on
        wm2, out2 = st.process(recs, watermark=wm)
        assert wm2 == wm and [o["value"] for o in out2] == [o["value"] for o in out]
        np.testing.assert_array_equal(st.last_rows.src_index, [len(recs) + i for i, _, _ in ref])
    finally:
        st.close()


def test_select_star_forwards_the_original_records(eng, T):
    from hstream_amd import ingest, processing as P
    where = sql.RCondAnd(cmp(">", A, const(0)), cmp("<=", B, const(4.0)))
    st = sql.gen_select_node(eng, "*", where, float_fields=("b",))
    try:
        batch = gen(311, T + 70)
        recs = _json_records(batch)
        ref = sql.gen_select_rows("*", where, None, recs)
        assert 20 < len(ref) < len(recs) - 20
        wm, out = st.process(recs)
        assert [o["value"] for o in out] == [m for _, _, m in ref] and wm == int(batch[1].max())
        vals = [json.dumps(r["value"]).encode() for r in recs]
        buf, off = ingest.pack_records(vals)
        wm, out = st.process_json(buf, off, batch[1], watermark=wm)
        assert [o["value"] for o in out] == [vals[i] for i, _, _ in ref]
        assert st.last_rows.aggs == [] and wm == int(batch[1].max())
        # runTask drives a Stream as it drives a Table
        polls = [recs[:100], recs[100:], None]
        seen = []
        st2 = P.Stream(eng, [("a", False), ("b", True)]).filter(P.Where(where, ("b",)))
        try:
            assert P.runTask(lambda: polls.pop(0), st2, sink=seen.append) == int(batch[1].max())
        finally:
            st2.close()
        assert [o["value"] for o in seen] == [m for _, _, m in ref]
    finally:
        st.close()
