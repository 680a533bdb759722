"""GPU: computed columns (hsg_op_create_mapped, k_map.hip). The op evaluates
the SELECT list's value expressions per record itself; the reference in every
case is computed on the host -- sql.expr_value, the exact-Fraction restatement
of genRExprValue (Codegen.hs:290-301), record by record, or for the larger
cases a numpy restatement of it that the values test first checks against
expr_value -- and handed to the CPU oracle, or to a plain op, as one more
column. Never the code under test."""
import ctypes
import os
import uuid

import numpy as np
import pytest

import pyoracle
from hstream_amd import abi, sql
from hstream_amd.columnar import OpSpec, narrow_columns, narrow_keys
from util import rows_equal

pytestmark = pytest.mark.gpu

I, F = abi.HSG_I64, abi.HSG_F64
NONE = np.uint32(abi.HSG_KEY_NONE)
CA, CN, S, MN, MX, AV, L = (abi.HSG_COUNT_ALL, abi.HSG_COUNT, abi.HSG_SUM, abi.HSG_MIN, abi.HSG_MAX, abi.HSG_AVG,
                            abi.HSG_LAST)
NAMES = ["a", "b", "c"]
TYPES = [I, F, I]
SIZE = 60_000
TSB = (1_700_000_000_000 // SIZE + 1) * SIZE
STRICT = abi.HSG_MAP_STRICT


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need cuda:0"
    from hstream_amd.engine import Engine
    e = Engine(device=0, batch_capacity=1 << 15)
    yield e
    e.close()


# ---- expressions ------------------------------------------------------------------------
def col(f):
    return sql.RExprCol(f, None, f)


def const(c):
    return sql.RExprConst(str(c), c)


def binop(op, l, r):
    return sql.RExprBinOp("", {"+": "OpAdd", "-": "OpSub", "*": "OpMul"}[op], l, r)


def cmp(op, l, r):
    return sql.RCondOp({"<": "RCompOpLT", ">": "RCompOpGT", ">=": "RCompOpGEQ"}[op], l, r)


A, B, C_ = col("a"), col("b"), col("c")
_d8 = A
for _k in range(7):  # a + (c + (a + (c + ...))): the stack reaches 8
    _d8 = binop("+", C_ if _k % 2 else A, _d8)
EXPRS = {
    "a+c": binop("+", A, C_),
    "a-c": binop("-", A, C_),
    "a*c": binop("*", A, C_),
    "a*b": binop("*", A, B),
    "b*0.25": binop("*", B, const(0.25)),
    "a*c-b": binop("-", binop("*", A, C_), B),
    "(a+c)*(a-c)": binop("*", binop("+", A, C_), binop("-", A, C_)),
    "7": const(7),
    "depth 8": _d8,
}


def np_val(e, names, cols, valids):
    """The expression over whole columns: (values, is f64, error). i64 wraps
    (numpy int64), anything with an f64 is f64; values here are small integers
    and multiples of 1/4, so every f64 result is exact."""
    n = len(cols[0])
    if isinstance(e, sql.RExprCol):
        c = names.index(e.field)
        err = np.zeros(n, bool) if valids is None or valids[c] is None else (valids[c] & 1) == 0
        return cols[c], cols[c].dtype == np.float64, err
    if isinstance(e, sql.RExprConst):
        f = isinstance(e.constant, float)
        return np.full(n, e.constant, np.float64 if f else np.int64), f, np.zeros(n, bool)
    (x, fx, ex), (y, fy, ey) = np_val(e.expr1, names, cols, valids), np_val(e.expr2, names, cols, valids)
    if fx or fy:
        x, y = x.astype(np.float64), y.astype(np.float64)
    with np.errstate(over="ignore"):
        return {"OpAdd": x + y, "OpSub": x - y, "OpMul": x * y}[e.op], fx or fy, ex | ey


def derive(exprs, batch, names=NAMES):
    """The batch the plain op / the oracle gets: one column per expression
    (error positions zeroed), its valid bytes (bit 0 = no error), and the
    per-expression error masks."""
    key, ts, cols, valids = batch
    out, ov, errs = [], [], []
    for e in exprs:
        v, _f, err = np_val(e, names, cols, valids)
        if isinstance(e, sql.RExprCol) and valids is not None:
            # an alias is the caller's column as it is, valid bytes included (the
            # aggregates take any non-zero byte as present; bit 0 is the map's and
            # the filter's reading, which a strict alias drops by)
            out.append(v)
            ov.append(valids[names.index(e.field)])
            errs.append(err)
            continue
        out.append(np.where(err, 0, v).astype(v.dtype))
        ov.append((~err).astype(np.uint8))
        errs.append(err)
    return out, ov, errs


def gen(seed, n, nkeys=50, absent=0.2, none=0.05, vr=8, t0=TSB, span=200_000, unique=False):
    """Columns [I64, F64, I64]: small integers and multiples of 1/4, ~20 %
    absent per column, bit 1 of every valid byte random, a few HSG_KEY_NONE."""
    rng = np.random.default_rng(seed)
    key = np.arange(n, dtype=np.uint32) if unique else rng.integers(0, nkeys, size=n).astype(np.uint32)
    key[rng.random(n) < none] = NONE
    ts = (t0 + (np.arange(n, dtype=np.int64) * span) // max(1, n) + rng.integers(0, 2000, size=n)).astype(np.int64)
    cols = [rng.integers(-vr, vr + 1, size=n).astype(np.int64),
            rng.integers(-4 * vr, 4 * vr + 1, size=n).astype(np.float64) / 4.0,
            rng.integers(-vr, vr + 1, size=n).astype(np.int64)]
    valids = [((rng.random(n) >= absent).astype(np.uint8) | (rng.integers(0, 2, size=n).astype(np.uint8) << 1))
              for _ in cols]
    return key, ts, cols, valids


def mapped_spec(spec, exprs, strict=(), names=NAMES, types=TYPES, **kw):
    """The op under test: `spec` (whose columns are the expressions) over the raw batch."""
    progs = [abi.MapExpr(sql.compile_expr(e, names), STRICT if j in strict else 0) for j, e in enumerate(exprs)]
    return OpSpec(**{**spec.__dict__, "col_types": types, "map": progs, **kw})


def derived_types(exprs, float_fields=("b",)):
    return [F if sql.expr_is_float(e, float_fields) else I for e in exprs]


def guard(batches, exprs, strict=(), where_keep=None, names=NAMES):
    """No vacuous pass: of the keyed records at least a quarter survive every
    expression, and at least one is dropped or absent."""
    keyed = ok = 0
    for bi, b in enumerate(batches):
        _, _, errs = derive(exprs, b, names)
        k = b[0] != NONE
        if where_keep is not None:
            k = k & where_keep[bi]
        bad = np.zeros(len(b[0]), bool)
        for e in errs:
            bad |= e
        keyed += int(np.count_nonzero(k))
        ok += int(np.count_nonzero(k & ~bad))
    assert keyed and 4 * ok >= keyed and ok < keyed, (keyed, ok)


def check(eng, spec, exprs, batches, strict=(), where=None, where_keep=None, ordered=None, dump=True, push=None,
          what="", engine_kw=None, guarded=True):
    """Each batch through the mapped op and through the oracle fed the
    host-computed columns, keys masked where WHERE or a strict expression
    drops; rows, watermarks, where_dropped / map_dropped. Returns (stats, map_stats)."""
    ordered = spec.emit_mode == abi.HSG_EMIT_PER_RECORD if ordered is None else ordered
    if guarded:
        guard(batches, exprs, strict, where_keep)
    gspec = mapped_spec(spec, exprs, strict, where=sql.compile_where(where, NAMES) if where is not None else None)
    g, o = eng.op(gspec), pyoracle.OracleOp(spec)
    f64 = spec.agg_is_f64()
    exact = [k in (MN, MX, L) for k, _ in spec.aggs]
    wg = wo = -1
    wtot = mtot = 0
    try:
        for bi, batch in enumerate(batches):
            key, ts, cols, valids = batch
            dcols, dval, errs = derive(exprs, batch)
            wkeep = where_keep[bi] if where_keep is not None else np.ones(len(key), bool)
            serr = np.zeros(len(key), bool)
            for j in strict:
                serr |= errs[j]
            wdrop = (key != NONE) & ~wkeep
            mdrop = (key != NONE) & wkeep & serr
            masked = np.where(wdrop | mdrop, NONE, key).astype(np.uint32)
            wtot += int(np.count_nonzero(wdrop))
            mtot += int(np.count_nonzero(mdrop))
            wg = (push or (lambda op, *a, **k: op.push(*a, **k)))(g, key, ts, cols, valids, watermark=wg)
            wo = o.push(masked, ts, dcols, dval, watermark=wo)
            assert wg == wo, f"{what} batch {bi}: watermark {wg} != {wo}"
            if spec.emit_mode != abi.HSG_EMIT_NONE:
                rows_equal(g.drain(), o.drain(), f64, ordered=ordered, exact_f64=exact, what=f"{what} batch {bi}")
            st, ms = g.stats(), g.map_stats()
            assert st["where_dropped"] == int(np.count_nonzero(wdrop)), (what, bi, st["where_dropped"])
            assert st["where_dropped_total"] == wtot, (what, bi)
            assert ms["map_dropped"] == int(np.count_nonzero(mdrop)), (what, bi, ms)
            assert ms["map_dropped_total"] == mtot, (what, bi, ms)
        if dump:
            rows_equal(g.dump_state(), o.dump_state(), f64, exact_f64=exact, what=f"{what} state")
        return g.stats(), g.map_stats()
    finally:
        g.close()
        o.close()


# ---- 1. values, bit-exact ------------------------------------------------------------------
@pytest.fixture(scope="module")
def val_batch():
    return gen(1, 4099, unique=True)


@pytest.mark.parametrize("name", list(EXPRS))
def test_values(eng, val_batch, name):
    """Unwindowed, EMIT per record, one key per record, LAST(expr): each
    changelog row carries the derived value of its own record."""
    key, ts, cols, valids = val_batch
    e = EXPRS[name]
    v, isf, err = np_val(e, NAMES, cols, valids)
    # the numpy restatement is expr_value, record by record
    for i in range(len(key)):
        obj = {f: c[i].item() for f, c, vv in zip(NAMES, cols, valids) if vv[i] & 1}
        try:
            want = sql.expr_value(e, obj)
            assert not err[i] and want == v[i].item(), (name, i)
        except KeyError:
            assert err[i], (name, i)
    if name != "7":
        guard([val_batch], [e])
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[F if isf else I], aggs=[(L, 0)],
                  state_capacity=1 << 14)
    g = eng.op(mapped_spec(spec, [e]))
    try:
        g.push(key, ts, cols, valids)
        rows = g.drain()
        # a record whose expression is the error value still emits its row: LAST left alone (0)
        keyed = np.flatnonzero(key != NONE)
        np.testing.assert_array_equal(rows.src_index, keyed)
        want = np.where(err, 0, v).astype(v.dtype)[keyed]
        np.testing.assert_array_equal(rows.aggs[0].view(np.int64), want.view(np.int64), err_msg=name)
        assert rows.aggs[0].dtype == (np.float64 if isf else np.int64)
    finally:
        g.close()


WRAP_A = np.array([2**32, 2**63 - 1, -2**63, 2**53 + 1, -(2**53) - 1, 3, 2**62, -1], dtype=np.int64)
WRAP_C = np.array([2**32, 1, -1, 1, 1, -2**62, 2, 2**63 - 1], dtype=np.int64)


def test_i64_wraps_and_converts_to_f64_once(eng):
    n = len(WRAP_A)
    key = np.arange(n, dtype=np.uint32)
    ts = TSB + np.arange(n, dtype=np.int64)
    b = np.full(n, 1.0)
    exprs = [binop("*", A, C_), binop("+", A, C_), binop("-", A, C_), binop("*", A, B), binop("+", A, const(0.0))]
    with np.errstate(over="ignore"):
        want = [WRAP_A * WRAP_C, WRAP_A + WRAP_C, WRAP_A - WRAP_C, WRAP_A.astype(np.float64) * b,
                WRAP_A.astype(np.float64) + 0.0]
    assert want[0][0] == 0 and want[1][1] == -2**63  # 2^32 * 2^32 and INT64_MAX + 1 wrap
    assert want[3][3] == 2.0**53  # 2^53 + 1 rounds to even on its way to f64
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[I, I, I, F, F],
                  aggs=[(L, j) for j in range(5)], state_capacity=1 << 10)
    g = eng.op(mapped_spec(spec, exprs))
    try:
        g.push(key, ts, [WRAP_A, b, WRAP_C], None)
        rows = g.drain()
        for j in range(5):
            np.testing.assert_array_equal(rows.aggs[j].view(np.int64), want[j].view(np.int64), err_msg=str(j))
        assert g.map_stats()["computed_cols"] == 5
    finally:
        g.close()


# ---- 2. the error value ----------------------------------------------------------------------
AC = binop("*", A, C_)


def test_error_value_absent_or_strict(eng):
    batches = [gen(10 + b, 3000, t0=TSB + b * 200_000) for b in range(2)]
    # not strict: the derived column is absent, COUNT(*) still counts the record
    soft = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[I], aggs=[(S, 0), (CN, 0), (CA, 0)],
                  state_capacity=1 << 12)
    _, ms = check(eng, soft, [AC], batches, what="soft")
    assert ms["map_dropped_total"] == 0
    # strict: the record is dropped, and has moved stream time
    hard = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[I], aggs=[(L, 0), (CA, 0)],
                  state_capacity=1 << 12)
    _, ms = check(eng, hard, [AC], batches, strict=(0,), what="strict")
    assert ms["map_dropped_total"] > 0


def test_every_record_dropped_still_moves_stream_time(eng):
    key, ts, cols, valids = gen(12, 1000, none=0.0)
    valids[2][:] = 0  # c is absent everywhere
    spec = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_RECORD, size_ms=SIZE, col_types=[I], aggs=[(L, 0), (CA, 0)],
                  state_capacity=1 << 12)
    g = eng.op(mapped_spec(spec, [AC], strict=(0,)))
    wm = g.push(key, ts, cols, valids, watermark=-1)
    assert wm == int(ts.max())
    assert len(g.drain()) == 0 and len(g.dump_state()) == 0
    assert g.map_stats()["map_dropped"] == 1000 and g.stats()["pairs"] == 0 and g.stats()["where_dropped"] == 0
    g.close()
    # (the one case whose point is that nothing survives: the survivors' guard cannot hold)
    check(eng, spec, [AC], [(key, ts, cols, valids)], strict=(0,), what="all dropped", guarded=False)


# ---- 3. the mapped op is the plain op ------------------------------------------------------------
def _stream(seed, nb=3, per=4000, nkeys=300, **kw):
    return [gen(seed + b, per, nkeys=nkeys, t0=TSB + b * SIZE, span=SIZE, **kw) for b in range(nb)]


def test_mapped_op_is_the_plain_op(eng):
    batches = _stream(20)
    guard(batches, [AC])
    plain = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=SIZE, col_types=[I], aggs=[(CA, 0), (S, 0)],
                   state_capacity=1 << 16)
    g, p = eng.op(mapped_spec(plain, [AC])), eng.op(plain)
    f64 = plain.agg_is_f64()
    wg = wp = -1
    try:
        for bi, batch in enumerate(batches):
            key, ts, cols, valids = batch
            dcols, dval, _ = derive([AC], batch)
            wg = g.push(key, ts, cols, valids, watermark=wg)
            wp = p.push(key, ts, dcols, dval, watermark=wp)
            assert wg == wp
            rows_equal(g.drain(), p.drain(), f64, what=f"batch {bi}")
        rows_equal(g.dump_state(), p.dump_state(), f64, what="state")
        sg, sp = g.stats(), p.stats()
        for f in ("state_slots", "state_row_bytes", "lean_batches", "direct_batches", "replays", "pairs_total"):
            assert sg[f] == sp[f], (f, sg[f], sp[f])
        assert sg["lean_batches"] == len(batches), sg
    finally:
        g.close()
        p.close()
    # ... and against the oracle
    check(eng, plain, [AC], batches, what="plain")


def test_aliases_are_not_computed(eng):
    """SELECT a, SUM(a*c): a is the caller's column, a*c the pass's."""
    batches = _stream(24, nb=2)
    spec = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=SIZE, col_types=[I, I], aggs=[(L, 0), (S, 1)],
                  state_capacity=1 << 16)
    _, ms = check(eng, spec, [A, AC], batches, what="alias")
    assert (ms["aliased_cols"], ms["computed_cols"]) == (1, 1)
    # only aliases: nothing is launched, the op is the plain op on the other column order
    spec = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=SIZE, col_types=[I, F], aggs=[(MX, 0), (MN, 1)],
                  state_capacity=1 << 16)
    _, ms = check(eng, spec, [C_, B], batches, what="aliases only")
    assert (ms["aliased_cols"], ms["computed_cols"]) == (2, 0)
    # a strict alias drops the records whose column is absent
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[F], aggs=[(L, 0), (CA, 0)],
                  state_capacity=1 << 12)
    _, ms = check(eng, spec, [B], batches, strict=(0,), what="strict alias")
    assert ms["map_dropped_total"] > 0 and ms["computed_cols"] == 0


# ---- 4. sizes ---------------------------------------------------------------------------------------
SIZES_SPEC = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[I, F], aggs=[(CA, 0), (S, 0), (MX, 1), (L, 1)],
                    state_capacity=1 << 12)
SIZES_EXPRS = [binop("+", A, C_), binop("*", A, B)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4096 * 3 + 1])
def test_sizes(eng, n):
    batches = [gen(30, 500), gen(31 + n, n, t0=TSB + 300_000)]
    check(eng, SIZES_SPEC, SIZES_EXPRS, batches, strict=(1,), what=f"n={n}")


def test_past_one_resident_grid_round():
    """More records than the pass's grid has threads: the grid-stride loop's second round."""
    from hstream_amd.engine import Engine, map_grid_threads
    n = map_grid_threads() + 65
    e = Engine(device=0, batch_capacity=n)
    try:
        batch = gen(33, n, nkeys=5000, span=SIZE)
        spec = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=SIZE, col_types=[I, F],
                      aggs=[(CA, 0), (S, 0), (MX, 1)], state_capacity=1 << 16)
        check(e, spec, SIZES_EXPRS, [batch], strict=(1,), what="grid + 65")
    finally:
        e.close()


# ---- 5. window kinds and emit modes ----------------------------------------------------------------------
KIND_EXPRS = [binop("-", AC, B), binop("+", A, C_)]


@pytest.mark.parametrize("emit", [abi.HSG_EMIT_PER_RECORD, abi.HSG_EMIT_PER_BATCH, abi.HSG_EMIT_NONE],
                         ids=["changes", "batch", "none"])
@pytest.mark.parametrize("kind,kw", [
    (abi.HSG_TUMBLING, dict(size_ms=SIZE)),
    (abi.HSG_HOPPING, dict(size_ms=SIZE, advance_ms=SIZE // 3)),
    (abi.HSG_SESSION, dict(gap_ms=40)),
    (abi.HSG_UNWINDOWED, {}),
], ids=["tumbling", "hopping", "session", "unwindowed"])
def test_window_kinds(eng, kind, emit, kw):
    batches = _stream(50, nb=2, per=2000)
    aggs = [(CA, 0), (S, 0), (AV, 0), (MN, 0), (MX, 1), (CN, 1)]
    if kind != abi.HSG_SESSION:
        aggs.append((L, 0))  # (LAST: time windows and unwindowed only)
    spec = OpSpec(kind, emit, col_types=[F, I], aggs=aggs, state_capacity=1 << 16, **kw)
    check(eng, spec, KIND_EXPRS, batches, strict=(1,), what=f"kind {kind} emit {emit}")


# ---- 6. WHERE plus map in one op ------------------------------------------------------------------------------
def _where_keep(cond, batch):
    key, ts, cols, valids = batch
    keep = np.zeros(len(key), bool)
    for i in range(len(key)):
        obj = {f: c[i].item() for f, c, v in zip(NAMES, cols, valids) if v[i] & 1}
        try:
            keep[i] = sql.gen_filter_r(cond, obj)
        except KeyError:
            keep[i] = False
    return keep


def test_where_and_map_in_one_pass(eng):
    """WHERE b > -1.25 (b: the filter's alone), SUM(a*c) (a, c: the map's
    alone): both counts exact, and the op aggregates as the one-column op."""
    batches = _stream(60, nb=2, per=3000)
    cond = cmp(">", B, const(-1.25))
    keeps = [_where_keep(cond, b) for b in batches]
    spec = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=SIZE, col_types=[I], aggs=[(CA, 0), (S, 0)],
                  state_capacity=1 << 16)
    st, ms = check(eng, spec, [AC], batches, strict=(0,), where=cond, where_keep=keeps, what="where+map")
    assert st["where_dropped_total"] > 0 and ms["map_dropped_total"] > 0
    p = eng.op(spec)
    sp = p.stats()
    p.close()
    assert st["state_slots"] == sp["state_slots"] and st["state_row_bytes"] == sp["state_row_bytes"]
    assert st["lean_batches"] == len(batches), st
    # WHERE over the columns the map reads too, not strict: map_dropped stays 0
    cond = sql.RCondAnd(cmp(">", A, const(-5)), cmp("<", binop("+", A, C_), const(6)))
    keeps = [_where_keep(cond, b) for b in batches]
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[I, F], aggs=[(S, 0), (MX, 1), (CA, 0)],
                  state_capacity=1 << 12)
    _, ms = check(eng, spec, [AC, binop("*", A, B)], batches, where=cond, where_keep=keeps, what="shared columns")
    assert ms["map_dropped_total"] == 0


# ---- 7. literal forms ----------------------------------------------------------------------------------------------
def sci_exp(e, names, valids, i):
    """The base-10 exponent class of the expression's Scientific for record
    i, as (coefficient, exponent) arithmetic gives it: a column is e = -2 when
    its literal carried decimals (bit 1) and 0 otherwise, a constant as
    fromFloatDigits normalises it; + and - take min e1 e2, * takes e1 + e2.
    The form bit says e < 0."""
    if isinstance(e, sql.RExprCol):
        return -2 if valids[names.index(e.field)][i] & 2 else 0
    if isinstance(e, sql.RExprConst):
        return 0 if float(e.constant).is_integer() else -2
    e1, e2 = sci_exp(e.expr1, names, valids, i), sci_exp(e.expr2, names, valids, i)
    return e1 + e2 if e.op == "OpMul" else min(e1, e2)


def test_literal_forms(eng):
    """One key per record, so each row's form word is its own record's:
    SUM 1 = no decimal literal reached it; MAX / LAST the literal's "prints as
    an integer" bit, 3 = the initial value (tests/test_gpu_sql_shape.py)."""
    batch = gen(70, 3000, unique=True)
    key, ts, cols, valids = batch
    exprs = [binop("+", A, B), binop("*", A, B), binop("*", B, const(2.5)), binop("+", A, const(2.0))]
    aggs = [(S, 0), (L, 1), (MX, 2), (L, 3)]
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[F, F, F, F], aggs=aggs,
                  flags=abi.HSG_OPF_LITERAL_FORMS, state_capacity=1 << 13)
    guard([batch], exprs)
    _, _, errs = derive(exprs, batch)
    g = eng.op(mapped_spec(spec, exprs))
    try:
        g.push(key, ts, cols, valids)
        rows = g.drain()
        keyed = np.flatnonzero(key != NONE)
        np.testing.assert_array_equal(rows.src_index, keyed)
        want = np.zeros(len(keyed), np.uint32)
        for r, i in enumerate(keyed):
            w = 0
            for j, (kind, _c) in enumerate(aggs):
                dec = sci_exp(exprs[j], NAMES, valids, i) < 0
                if kind == S:
                    bits = 0 if (dec and not errs[j][i]) else 1
                else:
                    bits = 3 if errs[j][i] else (0 if dec else 1)
                w |= bits << (2 * j)
            want[r] = w
        np.testing.assert_array_equal(rows.form, want)
        # the cases vary: every output takes each value it can (SUM 0 / 1; MAX, LAST 0 / 1 / 3,
        # but never 1 under b * 2.5, whose constant is a decimal literal)
        for j, can in enumerate([{0, 1}, {0, 1, 3}, {0, 3}, {0, 1, 3}]):
            assert {int(x) for x in (want >> (2 * j)) & 3} == can, j
        # a + 2.0: the constant is integral, the form follows a alone
        assert np.all(((want >> 6) & 3)[~errs[3][keyed] & ((valids[0][keyed] & 2) == 0)] == 1)
    finally:
        g.close()


def test_sink_prints_the_derived_form(eng):
    """SELECT x + y AS s with x = 2 and y = 4.0: Scientific 6.0 prints "6.0"."""
    from hstream_amd.ingest import Decoder, KeyDict, pack_records
    from hstream_amd.sink import Sink
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[I, F],
                  map=[abi.MapExpr([(abi.HSG_W_COL, 0), (abi.HSG_W_COL, 1), (abi.HSG_W_ADD,)], STRICT)], aggs=[(L, 0)],
                  flags=abi.HSG_OPF_LITERAL_FORMS, state_capacity=1 << 10)
    op = eng.op(spec)
    keys = KeyDict()
    dec = Decoder("k", [("x", I, True), ("y", F, True)], literal_forms=True)
    sink = Sink(op, keys, "k", [("s", 0), ("k", -1)], windowed=False)
    try:
        buf, off = pack_records([b'{"k":1,"x":2,"y":4.0}', b'{"k":2,"x":2,"y":4}', b'{"k":3,"x":2}'])
        kid, tb, cs, valid, _st, rej = dec.decode(keys, buf, off, np.array([TSB, TSB + 1, TSB + 2], np.int64))[:6]
        assert rej == 0
        op.push(kid, tb, cs, valid, watermark=-1)
        got = [v for _k, v in sink.encode(op.drain())]
        assert len(got) == 2 and op.map_stats()["map_dropped"] == 1  # the record without y is dropped
        assert b'"s":6.0' in got[0] and b'"s":6' in got[1] and b'"s":6.0' not in got[1], got
    finally:
        sink.close()
        op.close()


# ---- 8. transports and staging ---------------------------------------------------------------------------------------
T_SPEC = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=SIZE, col_types=[I, F],
                aggs=[(CA, 0), (S, 0), (MX, 1), (CN, 1)], state_capacity=1 << 16)
T_EXPRS = [AC, binop("*", A, B)]


def test_device_resident_batch_is_left_alone(eng):
    import torch
    batches = _stream(80, nb=2, per=5000)
    seen = []

    def push(op, key, ts, cols, valids, watermark):
        dev = torch.device("cuda:0")
        k = torch.from_numpy(key.view(np.int32)).to(dev)
        t = torch.from_numpy(ts).to(dev)
        c = [torch.from_numpy(x).to(dev) for x in cols]
        v = [torch.from_numpy(x).to(dev) for x in valids]
        torch.cuda.synchronize()
        wm = op.push(k, t, c, v, watermark=watermark)
        seen.append(np.array_equal(k.cpu().numpy().view(np.uint32), key)
                    and all(np.array_equal(x.cpu().numpy().view(np.int64), y.view(np.int64)) for x, y in zip(c, cols))
                    and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(v, valids)))
        return wm

    _, ms = check(eng, T_SPEC, T_EXPRS, batches, strict=(1,), push=push, what="device batch")
    assert seen == [True] * len(batches) and ms["map_dropped_total"] > 0


def test_device_batch_waits_for_its_ready_event(eng):
    import torch
    key, ts, cols, valids = batch = gen(84, 5000, span=SIZE)
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(device=dev)

    def push(op, key, ts, cols, valids, watermark):
        with torch.cuda.stream(side):  # the producer's stream: uploads, then the event
            k = torch.from_numpy(key.view(np.int32)).to(dev, non_blocking=True)
            t = torch.from_numpy(ts).to(dev, non_blocking=True)
            c = [torch.from_numpy(x).to(dev, non_blocking=True) for x in cols]
            v = [torch.from_numpy(x).to(dev, non_blocking=True) for x in valids]
            ev = torch.cuda.Event()
            ev.record(side)
        from hstream_amd.columnar import make_batch
        b, keep = make_batch(k, t, c, v)
        b.ready_event = ev.cuda_event
        wm = op.push_batch(b, watermark=watermark)
        side.synchronize()
        return wm

    check(eng, T_SPEC, T_EXPRS, [batch], strict=(1,), push=push, what="ready_event")


def test_narrow_transport(eng):
    """K16 keys, TS32 ts, I32 and DEC32 inputs: widened, then mapped."""
    batches = _stream(90, nb=2, per=5000, none=0.0)
    used = set()

    def push(op, key, ts, cols, valids, watermark):
        nts, base, ncols, enc, scale = narrow_columns(ts, cols, TYPES, dec_scale=[None, 2, None])
        used.update(enc)
        nk = narrow_keys(key)
        used.add(abi.HSG_ENC_K16 if nk.dtype == np.uint16 else 0)
        return op.push(nk, nts, ncols, valids, watermark=watermark, col_enc=enc, col_scale=scale, ts_base=base)

    check(eng, T_SPEC, T_EXPRS, batches, strict=(1,), push=push, what="narrow")
    assert {abi.HSG_ENC_K16, abi.HSG_ENC_I32, abi.HSG_ENC_DEC32} <= used


def test_async_pushes_over_both_prestage_sets(eng):
    batches = _stream(100, nb=4, per=6000)
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[I, F], aggs=[(CA, 0), (S, 0), (MX, 1)],
                  state_capacity=1 << 12, out_capacity=4 * 6000)
    guard(batches, T_EXPRS)
    g, o = eng.op(mapped_spec(spec, T_EXPRS, strict=(1,))), pyoracle.OracleOp(spec)
    wm = ctypes.c_int64(-1)
    rcs = []
    for key, ts, cols, valids in batches:
        g.push_async(key, ts, cols, valids, watermark=wm, done=rcs.append)
    g.wait()
    assert rcs == [abi.HSG_OK] * len(batches)
    wo, dropped = -1, 0
    for batch in batches:
        key, ts, _, _ = batch
        dcols, dval, errs = derive(T_EXPRS, batch)
        drop = (key != NONE) & errs[1]
        dropped += int(np.count_nonzero(drop))
        wo = o.push(np.where(drop, NONE, key).astype(np.uint32), ts, dcols, dval, watermark=wo)
    assert wm.value == wo
    rows_equal(g.drain(), o.drain(), spec.agg_is_f64(), ordered=True, exact_f64=[False, False, True], what="async")
    assert g.map_stats()["map_dropped_total"] == dropped > 0
    g.close()
    o.close()


def test_reset_keeps_the_map(eng):
    batches = _stream(110, nb=2, per=4000)
    g, o = eng.op(mapped_spec(T_SPEC, T_EXPRS, strict=(1,))), pyoracle.OracleOp(T_SPEC)
    key, ts, cols, valids = batches[0]
    g.push(key, ts, cols, valids)
    first = g.map_stats()["map_dropped"]
    assert first == int(np.count_nonzero((key != NONE) & derive(T_EXPRS, batches[0])[2][1])) > 0 and len(g.drain()) > 0
    g.reset()
    key, ts, cols, valids = batches[1]
    dcols, dval, errs = derive(T_EXPRS, batches[1])
    drop = (key != NONE) & errs[1]
    wg = g.push(key, ts, cols, valids)
    wo = o.push(np.where(drop, NONE, key).astype(np.uint32), ts, dcols, dval)
    assert wg == wo
    rows_equal(g.drain(), o.drain(), T_SPEC.agg_is_f64(), what="after reset")
    rows_equal(g.dump_state(), o.dump_state(), T_SPEC.agg_is_f64(), what="state after reset")
    ms = g.map_stats()
    second = int(np.count_nonzero(drop))
    assert ms["map_dropped"] == second and ms["map_dropped_total"] == first + second, ms
    g.close()
    o.close()


# ---- 9. HAVING over a derived-type aggregate ----------------------------------------------------------------------
def test_having_reads_the_derived_types(eng):
    """SUM(a*b) > 1.5 with i64 a and f64 b: the program's column 0 is the f64 sum."""
    W = abi
    batch = gen(120, 4000, nkeys=200)
    key, ts, cols, valids = batch
    exprs = [binop("*", A, B)]
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[F], aggs=[(S, 0), (CA, 0)],
                  state_capacity=1 << 12)
    having = [(W.HSG_W_COL, 0), (W.HSG_W_F64, 1.5), (W.HSG_W_GT,)]
    guard([batch], exprs)
    g, o = eng.op(mapped_spec(spec, exprs, having=having)), pyoracle.OracleOp(spec)
    try:
        dcols, dval, _ = derive(exprs, batch)
        g.push(key, ts, cols, valids)
        o.push(key, ts, dcols, dval)
        got, ref = g.drain(), o.drain()
        kept = ref.aggs[0] > 1.5
        assert 0 < np.count_nonzero(kept) < len(ref)
        np.testing.assert_array_equal(got.src_index, ref.src_index[kept])
        np.testing.assert_array_equal(got.key_id, ref.key_id[kept])
        np.testing.assert_allclose(got.aggs[0], ref.aggs[0][kept], rtol=1e-6)
        np.testing.assert_array_equal(got.aggs[1], ref.aggs[1][kept])
        assert g.stats()["having_dropped"] == int(np.count_nonzero(~kept))
    finally:
        g.close()
        o.close()
    # checked against the derived types: the message names the f64 the program leaves
    with pytest.raises(abi.HStreamGpuError, match=r"having: .*an f64 value"):
        eng.op(mapped_spec(spec, exprs, having=[(W.HSG_W_COL, 0)]))
    # ... and the aggregates index the expressions: a second one does not exist
    with pytest.raises(abi.HStreamGpuError, match="aggregate column out of range"):
        eng.op(mapped_spec(OpSpec(**{**spec.__dict__, "aggs": [(S, 1)]}), exprs))


# ---- 10. two ranks over the host transport -----------------------------------------------------------------------------
# name -> (spec over the expressions, expressions, the batch's field names and types, strict, classic knob).
# "wide": four expressions over a batch of two columns, so the kernels have more
# columns than the batch; the classic exchange (the knob, and what a session op
# takes anyway) unpacks the records a rank receives into the op's staging by
# the kernels' numbering.
_AB = ["a", "b"]
_WIDE = [binop("*", A, B), binop("+", A, B), binop("*", A, A), binop("-", B, A)]
_WIDE_AGGS = [(CA, 0), (S, 0), (MX, 1), (S, 2), (MN, 3), (CN, 3)]
RANK_CASES = {
    "sequenced": (OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_RECORD, size_ms=10_000, col_types=[I, F],
                         aggs=[(CA, 0), (S, 0), (MX, 1)], state_capacity=1 << 14),
                  [AC, binop("*", A, B)], NAMES, TYPES, (1,), False),
    "sequenced_wide": (OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_RECORD, size_ms=10_000, col_types=[F, F, I, F],
                              aggs=_WIDE_AGGS, state_capacity=1 << 14), _WIDE, _AB, [I, F], (1,), False),
    "classic_wide": (OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_RECORD, size_ms=10_000, col_types=[F, F, I, F],
                            aggs=_WIDE_AGGS, state_capacity=1 << 14), _WIDE, _AB, [I, F], (1,), True),
    "classic_wide_per_batch": (OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=10_000,
                                      col_types=[F, F, I, F], aggs=_WIDE_AGGS, state_capacity=1 << 14),
                               _WIDE, _AB, [I, F], (), True),
    "session_wide": (OpSpec(abi.HSG_SESSION, abi.HSG_EMIT_PER_BATCH, gap_ms=40, col_types=[F, F, I, F],
                            aggs=_WIDE_AGGS, state_capacity=1 << 14), _WIDE, _AB, [I, F], (1,), False),
}


def _rank_slices(G, ncols):
    out = []
    for b in range(3):
        key, ts, cols, valids = gen(200 + b, 4000, nkeys=300, t0=TSB + b * 20_000, span=20_000)
        cols, valids = cols[:ncols], valids[:ncols]
        cuts = np.linspace(0, len(key), G + 1).astype(int)
        out.append([(key[cuts[r]:cuts[r + 1]], ts[cuts[r]:cuts[r + 1]], [c[cuts[r]:cuts[r + 1]] for c in cols],
                     [v[cuts[r]:cuts[r + 1]] for v in valids]) for r in range(G)])
    return out


def _tuples(r, per_batch=False):
    return [(-1 if per_batch else int(r.src_index[i]), int(r.key_id[i]), int(r.win_start[i]), int(r.win_end[i]),
             tuple(a[i].item() for a in r.aggs)) for i in range(len(r))]


def _rank_worker(rank, G, name, case, q):
    try:
        from hstream_amd.engine import Engine, testing_knob
        spec, exprs, names, types, strict, classic = RANK_CASES[case]
        e = Engine(device=0, rank=rank, nranks=G, comm_id=name, batch_capacity=1 << 13,
                   transport=abi.HSG_TRANSPORT_HOST)
        with testing_knob(abi.HSG_KNOB_X_CLASSIC, 1 if classic else 0):
            op = e.op(mapped_spec(spec, exprs, strict=strict, names=names, types=types))
        wm, rows, dropped = -1, [], []
        for slices in _rank_slices(G, len(names)):
            key, ts, cols, valids = slices[rank]
            wm = op.push(key, ts, cols, valids, watermark=wm)
            rows.append(_tuples(op.drain(), spec.emit_mode == abi.HSG_EMIT_PER_BATCH))
            dropped.append(op.map_stats()["map_dropped"])
        state = op.dump_state().tuples()
        op.close()
        e.close()
        q.put((rank, wm, rows, state, dropped))
    except Exception as ex:  # reported to the parent, which fails the test
        q.put((rank, "error", repr(ex), None, None))


@pytest.mark.parametrize("case", list(RANK_CASES))
def test_two_ranks_map_their_own_slices(case):
    import multiprocessing as mp
    G = 2
    spec, exprs, names, types, strict, classic = RANK_CASES[case]
    per_batch = spec.emit_mode == abi.HSG_EMIT_PER_BATCH
    whole = []
    for slices in _rank_slices(G, len(names)):
        whole.append((np.concatenate([s[0] for s in slices]), np.concatenate([s[1] for s in slices]),
                      [np.concatenate([s[2][c] for s in slices]) for c in range(len(names))],
                      [np.concatenate([s[3][c] for s in slices]) for c in range(len(names))]))
    guard(whole, exprs, strict, names=names)
    assert len(exprs) > len(names) or "wide" not in case
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = f"hsgm-{os.getpid()}-{uuid.uuid4().hex[:12]}"
    procs = [ctx.Process(target=_rank_worker, args=(r, G, name, case, q)) for r in range(G)]
    for p in procs:
        p.start()
    try:
        outs = [q.get(timeout=100) for _ in range(G)]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    errs = [o for o in outs if o[1] == "error"]
    assert not errs, errs
    outs.sort(key=lambda o: o[0])
    o = pyoracle.OracleOp(spec)
    wm = -1
    total = 0
    for bi, (slices, batch) in enumerate(zip(_rank_slices(G, len(names)), whole)):
        key, ts, cols, valids = batch
        dcols, dval, derr = derive(exprs, batch, names)
        drop = np.zeros(len(key), bool)
        for j in strict:
            drop |= (key != NONE) & derr[j]
        total += int(np.count_nonzero(drop))
        wm = o.push(np.where(drop, NONE, key).astype(np.uint32), ts, dcols, dval, watermark=wm)
        ref = sorted(_tuples(o.drain(), per_batch))
        got = sorted(outs[0][2][bi] + outs[1][2][bi])
        assert got == ref, (bi, len(got), len(ref))
        at = 0
        for r in range(G):
            n = len(slices[r][0])
            assert outs[r][4][bi] == int(np.count_nonzero(drop[at:at + n])), (bi, r)
            at += n
    assert (total > 0) == bool(strict)
    assert all(out[1] == wm for out in outs)
    assert sorted(outs[0][3] + outs[1][3]) == sorted(o.dump_state().tuples())
    o.close()


# ---- 11. refusals -----------------------------------------------------------------------------------------------------------
def test_bad_map_is_refused_with_the_checkers_message(eng):
    from hstream_amd.engine import map_check
    W = abi
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=TYPES, aggs=[(S, 0)], state_capacity=1 << 10)
    bad = {
        "comparison": [[(W.HSG_W_COL, 0), (W.HSG_W_I64, 1), (W.HSG_W_GT,)]],
        "column": [[(W.HSG_W_COL, 3)]],
        "two values": [[(W.HSG_W_COL, 0), (W.HSG_W_COL, 2)]],
        "nan": [[(W.HSG_W_COL, 1), (W.HSG_W_F64, float("nan")), (W.HSG_W_MUL,)]],
        "nine": [[(W.HSG_W_COL, 0)]] * 9,
    }
    for name, m in bad.items():
        rc, msg, _ = map_check(m, TYPES)
        assert rc == abi.HSG_E_INVALID and msg.startswith("map: ")
        with pytest.raises(abi.HStreamGpuError) as ei:
            eng.op(OpSpec(**{**spec.__dict__, "map": m}))
        assert ei.value.status == abi.HSG_E_INVALID and msg in str(ei.value), (name, str(ei.value))


def test_no_expressions_is_the_filtered_op(eng):
    """hsg_op_create_mapped with n_exprs == 0 is hsg_op_create_filtered."""
    import ctypes as C
    W = abi
    batch = gen(130, 2000)
    key, ts, cols, valids = batch
    where = [(W.HSG_W_COL, 0), (W.HSG_W_I64, 1), (W.HSG_W_GT,)]
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=TYPES, aggs=[(CA, 0), (S, 2), (MX, 1)],
                  state_capacity=1 << 12, where=where)
    f = eng.op(spec)
    cfg, keep = spec.to_config()
    wprog, wn = abi.where_array(where)
    h = C.c_void_p()
    rc = eng._lib.hsg_op_create_mapped(eng._h, C.byref(cfg), None, 0, wprog, wn, None, 0, C.byref(h))
    assert rc == abi.HSG_OK
    from hstream_amd.columnar import OpHandle
    m = OpHandle(eng._lib, "hsg", h, spec)
    try:
        assert f.push(key, ts, cols, valids) == m.push(key, ts, cols, valids)
        rows_equal(m.drain(), f.drain(), spec.agg_is_f64(), ordered=True, what="n_exprs == 0")
        ms = abi.hsg_map_stats()
        assert eng._lib.hsg_op_map_stats(h, C.byref(ms)) == abi.HSG_OK
        assert ms.as_dict() == {"map_dropped": 0, "map_dropped_total": 0, "computed_cols": 0, "aliased_cols": 0}
        assert f.stats()["where_dropped"] > 0
    finally:
        m.close()
        f.close()


# ---- 12. through the SQL layer ------------------------------------------------------------------------------------------------
def test_select_expressions_through_gen_group_by_node(eng):
    """SELECT a + b AS s, SUM(a * c) AS t, COUNT(*) AS n ... GROUP BY k EMIT
    CHANGES: the reference row by row on the host (sql.expr_value): the
    passthrough is strict, the aggregate over an expression skips."""
    rng = np.random.default_rng(140)
    recs = []
    for i in range(600):
        v = {"k": int(rng.integers(0, 20))}
        if rng.random() >= 0.2:
            v["a"] = int(rng.integers(-8, 9))
        if rng.random() >= 0.2:
            v["b"] = float(rng.integers(-32, 33)) / 4.0
        if rng.random() >= 0.2:
            v["c"] = int(rng.integers(-8, 9))
        recs.append({"value": v, "timestamp": TSB + i})
    s_e, t_e = binop("+", A, B), binop("*", A, C_)
    sel = [("COL", s_e, "s"), ("SUM", t_e, "t"), ("COUNT(*)", "n")]
    t = sql.gen_group_by_node(eng, sel, sql.RGroupBy("k"), emit=abi.HSG_EMIT_PER_RECORD, float_fields=("b",),
                              state_capacity=1 << 10)
    try:
        wm, rows = t.process(recs)
        state, want, dropped = {}, [], 0
        for r in recs:
            v = r["value"]
            try:
                s = float(sql.expr_value(s_e, v))
            except KeyError:
                dropped += 1
                continue
            acc = state.setdefault(v["k"], {"s": 0.0, "t": 0, "n": 0})
            acc["s"] = s
            try:
                acc["t"] += int(sql.expr_value(t_e, v))
            except KeyError:
                pass
            acc["n"] += 1
            want.append((v["k"], dict(acc)))
        assert wm == TSB + 599 and 0 < dropped < 300 and len(want) > 150
        assert rows == want
        assert t.op.map_stats()["map_dropped"] == dropped
    finally:
        t.op.close()
