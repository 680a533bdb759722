"""GPU: WHERE pushdown (hsg_op_create_where, k_where.hip). The op filters each
staged batch itself; the reference in every case is the CPU oracle fed keys
that the host masked beforehand with sql.gen_filter_r -- the per-record
restatement of genFilterR (Codegen.hs:303-341) -- or, for the larger cases,
with a numpy restatement of it that the semantics test first checks against
gen_filter_r record by record. Never the code under test."""
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
CA, CN, S, MN, MX, L = (abi.HSG_COUNT_ALL, abi.HSG_COUNT, abi.HSG_SUM, abi.HSG_MIN, abi.HSG_MAX, abi.HSG_LAST)
NAMES = ["a", "b", "c"]
TYPES = [I, F, I]
AGGS = [(CA, 0), (S, 0), (MX, 1), (CN, 2)]
SIZE = 60_000
TSB = (1_700_000_000_000 // SIZE + 1) * SIZE


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need cuda:0"
    from hstream_amd.engine import Engine
    e = Engine(device=0, batch_capacity=1 << 15)
    yield e
    e.close()


# ---- conditions ---------------------------------------------------------------------
def col(f):
    return sql.RExprCol(f, None, f)


def const(c):
    return sql.RExprConst(str(c), c)


def cmp(op, l, r):
    return sql.RCondOp({"=": "RCompOpEQ", "<>": "RCompOpNE", "<": "RCompOpLT", ">": "RCompOpGT", "<=": "RCompOpLEQ",
                        ">=": "RCompOpGEQ"}[op], l, r)


def binop(op, l, r):
    return sql.RExprBinOp("", {"+": "OpAdd", "-": "OpSub", "*": "OpMul"}[op], l, r)


A, B, C_ = col("a"), col("b"), col("c")
CONDS = {
    "a > 1": cmp(">", A, const(1)),
    "NOT (a > 1 AND b > 2)": sql.RCondNot(sql.RCondAnd(cmp(">", A, const(1)), cmp(">", B, const(2)))),
    "a > 1 OR b > 2": sql.RCondOr(cmp(">", A, const(1)), cmp(">", B, const(2))),
    "a BETWEEN c AND b": sql.RCondBetween(C_, A, B),
    "a + c >= b * 2": cmp(">=", binop("+", A, C_), binop("*", B, const(2))),
    "a - c < 3": cmp("<", binop("-", A, C_), const(3)),
    "a * c <> 6": cmp("<>", binop("*", A, C_), const(6)),
    "a = c": cmp("=", A, C_),
    "b <= 0.5": cmp("<=", B, const(0.5)),
    "NOT b < a": sql.RCondNot(cmp("<", B, A)),
    "(a > 0 AND c > 0) OR (b > 1 AND NOT c = 2)": sql.RCondOr(
        sql.RCondAnd(cmp(">", A, const(0)), cmp(">", C_, const(0))),
        sql.RCondAnd(cmp(">", B, const(1)), sql.RCondNot(cmp("=", C_, const(2))))),
    "a + c BETWEEN -1 AND 3.5": sql.RCondBetween(const(-1), binop("+", A, C_), const(3.5)),
    "b - 0.25 BETWEEN a AND c * 1.5": sql.RCondBetween(A, binop("-", B, const(0.25)), binop("*", C_, const(1.5))),
}


def host_keep(cond, names, cols, valids):
    """gen_filter_r record by record over the JSON objects the columns stand
    for: a field is in the object iff bit 0 of its valid byte is set; a throw
    (missing field) drops the record, as runTask does."""
    n = len(cols[0]) if cols else 0
    keep = np.zeros(n, bool)
    for i in range(n):
        obj = {f: c[i].item() for f, c, v in zip(names, cols, valids) if v is None or v[i] & 1}
        try:
            keep[i] = sql.gen_filter_r(cond, obj)
        except KeyError:
            keep[i] = False
    return keep


def np_keep(cond, names, cols, valids):
    """The same over whole columns (for the larger cases): (value, error) pairs,
    the laziness as rules on them. Values here are small integers and
    multiples of 1/4, so float64 arithmetic and mixed comparisons are exact."""
    n = len(cols[0])

    def val(e):
        if isinstance(e, sql.RExprCol):
            c = names.index(e.field)
            err = np.zeros(n, bool) if valids is None or valids[c] is None else (valids[c] & 1) == 0
            return cols[c].astype(np.float64), err
        if isinstance(e, sql.RExprConst):
            return np.full(n, float(e.constant)), np.zeros(n, bool)
        (x, ex), (y, ey) = val(e.expr1), val(e.expr2)
        return {"OpAdd": x + y, "OpSub": x - y, "OpMul": x * y}[e.op], ex | ey

    def cond_(c):
        if isinstance(c, sql.RCondOp):
            (x, ex), (y, ey) = val(c.expr1), val(c.expr2)
            t = {"RCompOpEQ": x == y, "RCompOpNE": x != y, "RCompOpLT": x < y, "RCompOpGT": x > y, "RCompOpLEQ": x <= y,
                 "RCompOpGEQ": x >= y}[c.op]
            return t, ex | ey
        if isinstance(c, sql.RCondNot):
            t, e = cond_(c.cond)
            return ~t, e
        if isinstance(c, sql.RCondBetween):
            (lo, el), (x, ex), (hi, eh) = val(c.expr1), val(c.expr), val(c.expr2)
            gt = lo > x
            return ~gt & (x <= hi), el | ex | (~gt & eh)
        (l, el), (r, er) = cond_(c.cond1), cond_(c.cond2)
        take_l = el | (~l if isinstance(c, sql.RCondAnd) else l)
        return np.where(take_l, l, r), np.where(take_l, el, er)

    t, e = cond_(cond)
    return t & ~e


def gen(seed, n, nkeys=50, absent=0.2, none=0.05, vr=8, t0=TSB, span=200_000):
    """Columns [I64, F64, I64]: small integers and multiples of 1/4, ~20 %
    absent per column, bit 1 of every valid byte random (the literal form,
    which the filter must not read), a few HSG_KEY_NONE records."""
    rng = np.random.default_rng(seed)
    key = rng.integers(0, nkeys, size=n).astype(np.uint32)
    key[rng.random(n) < none] = NONE
    ts = (t0 + (np.arange(n, dtype=np.int64) * span) // max(1, n) + rng.integers(0, 2000, size=n)).astype(np.int64)
    cols = [rng.integers(-vr, vr + 1, size=n).astype(np.int64),
            rng.integers(-4 * vr, 4 * vr + 1, size=n).astype(np.float64) / 4.0,
            rng.integers(-vr, vr + 1, size=n).astype(np.int64)]
    valids = [((rng.random(n) >= absent).astype(np.uint8) | (rng.integers(0, 2, size=n).astype(np.uint8) << 1))
              for _ in cols]
    return key, ts, cols, valids


def check(eng, spec, cond, batches, keeps, names=NAMES, ordered=None, dump=True, push=None, what=""):
    """Each batch through the op with the program and through the oracle with
    the keys masked by keeps[b]; rows, watermarks, where_dropped; returns stats."""
    ordered = spec.emit_mode == abi.HSG_EMIT_PER_RECORD if ordered is None else ordered
    gspec = OpSpec(**{**spec.__dict__, "where": sql.compile_where(cond, names)})
    g, o = eng.op(gspec), pyoracle.OracleOp(spec)
    f64 = spec.agg_is_f64()
    wg = wo = -1
    total = 0
    try:
        for bi, ((key, ts, cols, valids), keep) in enumerate(zip(batches, keeps)):
            masked = np.where(keep, key, NONE).astype(np.uint32)
            dropped = int(np.count_nonzero((key != NONE) & ~keep))
            total += dropped
            wg = (push or (lambda op, *a, **k: op.push(*a, **k)))(g, key, ts, cols, valids, watermark=wg)
            wo = o.push(masked, ts, cols, valids, watermark=wo)
            assert wg == wo, f"{what} batch {bi}: watermark {wg} != {wo}"
            if spec.emit_mode != abi.HSG_EMIT_NONE:
                rows_equal(g.drain(), o.drain(), f64, ordered=ordered, what=f"{what} batch {bi}")
            st = g.stats()
            assert st["where_dropped"] == dropped, (what, bi, st["where_dropped"], dropped)
            assert st["where_dropped_total"] == total, (what, bi)
        if dump:
            rows_equal(g.dump_state(), o.dump_state(), f64, what=f"{what} state")
        return g.stats()
    finally:
        g.close()
        o.close()


UNWIN_PR = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=TYPES, aggs=AGGS, state_capacity=1 << 12)


# ---- 1. semantics -------------------------------------------------------------------
@pytest.fixture(scope="module")
def sem_batch():
    return gen(1, 4099)


@pytest.mark.parametrize("name", list(CONDS))
def test_semantics(eng, sem_batch, name):
    key, ts, cols, valids = sem_batch
    cond = CONDS[name]
    keep = host_keep(cond, NAMES, cols, valids)
    np.testing.assert_array_equal(np_keep(cond, NAMES, cols, valids), keep)  # (the restatement used below)
    kept = np.count_nonzero(keep)
    assert 0 < kept < len(keep), name
    check(eng, UNWIN_PR, cond, [sem_batch], [keep], what=name)


def test_semantics_cases_named_by_the_rules(sem_batch):
    """The batch holds the cases the laziness rules turn on."""
    _, _, (a, b, c), (va, vb, vc) = sem_batch
    pa, pb, pc = (va & 1) == 1, (vb & 1) == 1, (vc & 1) == 1
    assert np.any(pa & ~pb & (a > 1)) and np.any(pa & ~pb & (a <= 1))    # AND / OR / NOT with b absent
    assert np.any(pa & pc & ~pb & (c > a)) and np.any(pa & pc & ~pb & (c <= a))  # BETWEEN, hi absent
    assert np.any(((va | vb | vc) & 2) != 0) and np.any(((va & vb & vc) & 2) == 0)  # literal bits vary


# ---- 2. exact mixed comparison --------------------------------------------------------
MIXED = np.array([2**53, 2**53 + 1, 2**53 - 1, 2**63 - 1, -2**63, 2**53 + 2, -2**53 - 1, 0], dtype=np.int64)


@pytest.mark.parametrize("k", [2.0**53, 2.0**63], ids=["2^53", "2^63"])
@pytest.mark.parametrize("op", ["=", "<>", "<", ">", "<=", ">="])
def test_exact_mixed_comparison(eng, op, k):
    n = len(MIXED)
    key = np.arange(n, dtype=np.uint32)
    ts = TSB + np.arange(n, dtype=np.int64)
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[I], aggs=[(CA, 0), (MX, 0)],
                  state_capacity=1 << 10)
    for cond in (cmp(op, col("a"), const(k)), cmp(op, const(k), col("a"))):
        keep = host_keep(cond, ["a"], [MIXED], [None])
        check(eng, spec, cond, [(key, ts, [MIXED], None)], [keep], names=["a"], what=f"a {op} {k}")
    # what the exact order says, spelled out for the two neighbours of 2^53
    if k == 2.0**53:
        want = {"=": [1, 0, 0], "<>": [0, 1, 1], "<": [0, 0, 1], ">": [0, 1, 0], "<=": [1, 0, 1], ">=": [1, 1, 0]}[op]
        assert host_keep(cmp(op, col("a"), const(k)), ["a"], [MIXED], [None])[:3].astype(int).tolist() == want


# ---- 3. sizes ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4096 * 3 + 1])
def test_sizes(eng, n):
    cond = CONDS["a > 1 OR b > 2"]
    batches = [gen(30, 500), gen(31 + n, n, t0=TSB + 300_000)]
    keeps = [np_keep(cond, NAMES, b[2], b[3]) for b in batches]
    check(eng, UNWIN_PR, cond, batches, keeps, what=f"n={n}")


def test_everything_dropped_still_moves_stream_time(eng):
    key, ts, cols, valids = gen(40, 1000, none=0.0)
    cond = cmp(">", A, const(100))
    spec = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_RECORD, size_ms=SIZE, col_types=TYPES, aggs=AGGS,
                  state_capacity=1 << 12)
    g = eng.op(OpSpec(**{**spec.__dict__, "where": sql.compile_where(cond, NAMES)}))
    wm = g.push(key, ts, cols, valids, watermark=-1)
    assert wm == int(ts.max())
    assert len(g.drain()) == 0 and len(g.dump_state()) == 0
    st = g.stats()
    assert st["where_dropped"] == 1000 and st["pairs"] == 0, st
    g.close()
    check(eng, spec, cond, [(key, ts, cols, valids)], [np.zeros(1000, bool)], what="all dropped")


def test_nothing_dropped_and_no_valid_arrays(eng):
    key, ts, cols, _ = gen(41, 3000)
    cond = sql.RCondAnd(cmp(">", A, const(-100)), cmp("<", B, const(100.5)))
    st = check(eng, UNWIN_PR, cond, [(key, ts, cols, None)], [np.ones(3000, bool)], what="none dropped")
    assert st["where_dropped_total"] == 0
    # valid=None with a real filter, and one column's array alone
    cond = CONDS["a + c >= b * 2"]
    check(eng, UNWIN_PR, cond, [(key, ts, cols, None)], [np_keep(cond, NAMES, cols, None)], what="valid=None")
    _, _, _, valids = gen(41, 3000)
    some = [None, valids[1], None]
    check(eng, UNWIN_PR, cond, [(key, ts, cols, some)], [np_keep(cond, NAMES, cols, some)], what="one valid array")


# ---- 4. every window kind -------------------------------------------------------------------
def _stream(seed, nb=3, per=20_000, nkeys=500, **kw):
    return [gen(seed + b, per, nkeys=nkeys, t0=TSB + b * SIZE, span=SIZE, **kw) for b in range(nb)]


WINDOW_COND = sql.RCondAnd(cmp(">", A, const(-3)), sql.RCondBetween(const(-2.5), B, C_))


@pytest.mark.parametrize("kind,emit,kw", [
    (abi.HSG_HOPPING, abi.HSG_EMIT_PER_BATCH, dict(size_ms=SIZE, advance_ms=SIZE // 3)),
    (abi.HSG_HOPPING, abi.HSG_EMIT_PER_RECORD, dict(size_ms=SIZE, advance_ms=SIZE // 3)),
    (abi.HSG_SESSION, abi.HSG_EMIT_PER_BATCH, dict(gap_ms=40)),
    (abi.HSG_SESSION, abi.HSG_EMIT_PER_RECORD, dict(gap_ms=40)),
    (abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_BATCH, {}),
    (abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, {}),
    (abi.HSG_TUMBLING, abi.HSG_EMIT_PER_RECORD, dict(size_ms=SIZE)),
    (abi.HSG_TUMBLING, abi.HSG_EMIT_NONE, dict(size_ms=SIZE)),
], ids=["hopping_batch", "hopping_changes", "session_batch", "session_changes", "unwindowed_batch",
        "unwindowed_changes", "tumbling_changes", "tumbling_state_only"])
def test_window_kinds(eng, kind, emit, kw):
    batches = _stream(50)
    keeps = [np_keep(WINDOW_COND, NAMES, b[2], b[3]) for b in batches]
    spec = OpSpec(kind, emit, col_types=TYPES, aggs=AGGS, state_capacity=1 << 16, **kw)
    check(eng, spec, WINDOW_COND, batches, keeps, what=f"kind {kind} emit {emit}")


def test_tumbling_per_batch_stays_on_the_lean_path(eng):
    """The filter masks keys and nothing else: the plain COUNT(*) / SUM op and
    the SQL drop-in's q3 shape (tests/test_gpu_sql_wide.py: three LAST
    passthroughs and a SUM with literal forms) aggregate every batch on the
    lean kernels, as they do without it."""
    batches = _stream(60, absent=0.03)
    keeps = [np_keep(WINDOW_COND, NAMES, b[2], b[3]) for b in batches]
    # (the lean record kernels take one-column ops, k_agg_lean.hip
    # part_lean_eligible: b and c are columns of the filter alone)
    plain = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=SIZE, col_types=TYPES,
                   aggs=[(CA, 0), (S, 0)], state_capacity=1 << 16)
    st = check(eng, plain, WINDOW_COND, batches, keeps, what="plain")
    assert st["lean_batches"] == st["batches"] == len(batches), st
    q3_types = [I, I, I]
    q3b = [(k, t, [c[0], c[2], (c[1] * 4).astype(np.int64)], [v[0], v[2], v[1]]) for k, t, c, v in batches]
    names = ["a", "c", "b4"]
    cond = sql.RCondAnd(cmp(">", col("a"), const(-3)), sql.RCondBetween(const(-10), col("b4"), binop("*", col("c"), const(4))))
    keeps = [np_keep(cond, names, b[2], b[3]) for b in q3b]
    q3 = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=SIZE, col_types=q3_types,
                aggs=[(L, 0), (L, 1), (L, 2), (S, 0)], flags=abi.HSG_OPF_LITERAL_FORMS, state_capacity=1 << 16)
    st = check(eng, q3, cond, q3b, keeps, names=names, what="q3")
    assert st["lean_batches"] == st["batches"] == len(batches) and st["replays"] == 0, st


# ---- 5. a column only the filter reads ---------------------------------------------------------
@pytest.mark.parametrize("flags", [0, abi.HSG_OPF_LITERAL_FORMS], ids=["plain", "forms"])
def test_filter_only_column(eng, flags):
    """SUM(c0) WHERE c1 > k: the op aggregates as the one-column op does."""
    batches = [(k, t, [c[0], c[1]], [v[0], v[1]]) for k, t, c, v in _stream(70)]
    cond = cmp(">", col("b"), const(-1.25))
    names = ["a", "b"]
    keeps = [np_keep(cond, names, b[2], b[3]) for b in batches]
    aggs = [(S, 0), (L, 0)] if flags else [(CA, 0), (S, 0)]  # (k_agg_sql / k_agg_lean shapes of one column)
    two = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=SIZE, col_types=[I, F], aggs=aggs, flags=flags,
                 state_capacity=1 << 16)
    st2 = check(eng, two, cond, batches, keeps, names=names, what="filter-only")
    # the one-column op on pre-masked keys: the same rows (through the oracle
    # above and here), slots and kernels
    one = OpSpec(**{**two.__dict__, "col_types": [I]})
    g, o = eng.op(one), pyoracle.OracleOp(one)
    wg = wo = -1
    for (key, ts, cols, valids), keep in zip(batches, keeps):
        masked = np.where(keep, key, NONE).astype(np.uint32)
        wg = g.push(masked, ts, cols[:1], valids[:1], watermark=wg)
        wo = o.push(masked, ts, cols[:1], valids[:1], watermark=wo)
        rows_equal(g.drain(), o.drain(), one.agg_is_f64(), what="one column")
    st1 = g.stats()
    g.close()
    o.close()
    for f in ("state_slots", "state_row_bytes", "lean_batches", "direct_batches", "replays", "pairs_total"):
        assert st2[f] == st1[f], (f, st2[f], st1[f])
    assert st2["lean_batches"] == len(batches), st2
    # a wrong column count is still refused: the batch carries the filter's column
    g = eng.op(OpSpec(**{**two.__dict__, "where": sql.compile_where(cond, names)}))
    key, ts, cols, valids = batches[0]
    with pytest.raises(abi.HStreamGpuError, match="n_cols"):
        g.push(key, ts, cols[:1], valids[:1])
    g.close()


# ---- 6. transports --------------------------------------------------------------------------------
def test_device_resident_batch_leaves_the_callers_keys_alone(eng):
    import torch
    batches = _stream(80, per=5000)
    keeps = [np_keep(WINDOW_COND, NAMES, b[2], b[3]) for b in batches]
    seen = []

    def push(op, key, ts, cols, valids, watermark):
        dev = torch.device("cuda:0")
        k = torch.from_numpy(key.view(np.int32)).to(dev)
        t = torch.from_numpy(ts).to(dev)
        c = [torch.from_numpy(x).to(dev) for x in cols]
        v = [torch.from_numpy(x).to(dev) for x in valids]
        torch.cuda.synchronize()
        wm = op.push(k, t, c, v, watermark=watermark)
        seen.append(np.array_equal(k.cpu().numpy().view(np.uint32), key))
        return wm

    spec = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=SIZE, col_types=TYPES, aggs=AGGS,
                  state_capacity=1 << 16)
    st = check(eng, spec, WINDOW_COND, batches, keeps, push=push, what="device batch")
    assert seen == [True] * len(batches) and st["where_dropped_total"] > 0


def test_narrow_transport(eng):
    """K16 keys, TS16 / TS32 ts, I32 and DEC32 columns: widened, then filtered."""
    batches = _stream(90, per=6000, none=0.0)
    keeps = [np_keep(WINDOW_COND, NAMES, b[2], b[3]) for b in batches]
    used = set()
    for ts16 in (True, False):
        def push(op, key, ts, cols, valids, watermark):
            nts, base, ncols, enc, scale = narrow_columns(ts, cols, TYPES, dec_scale=[None, 2, None], ts16=ts16)
            nk = narrow_keys(key)
            used.update(enc)
            used.add(abi.HSG_ENC_K16 if nk.dtype == np.uint16 else 0)
            used.add(abi.HSG_ENC_TS16 if ts16 and base is not None and np.ndim(base) else abi.HSG_ENC_TS32)
            kw = dict(ts_frames=base) if np.ndim(base) else dict(ts_base=base)
            return op.push(nk, nts, ncols, valids, watermark=watermark, col_enc=enc, col_scale=scale, **kw)

        check(eng, UNWIN_PR, WINDOW_COND, batches, keeps, push=push, what=f"narrow ts16={ts16}")
    assert {abi.HSG_ENC_K16, abi.HSG_ENC_I32, abi.HSG_ENC_DEC32, abi.HSG_ENC_TS16, abi.HSG_ENC_TS32} <= used


@pytest.mark.parametrize("narrow", [False, True], ids=["full", "k16"])
def test_async_pushes_prestage(eng, narrow):
    """Two push_async batches back to back: the second is prestaged into its own
    staging set while the first runs, and filtered there in place."""
    import ctypes
    batches = _stream(100, nb=4, per=8000, none=0.0 if narrow else 0.05)
    keeps = [np_keep(WINDOW_COND, NAMES, b[2], b[3]) for b in batches]
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=TYPES, aggs=AGGS, state_capacity=1 << 12,
                  out_capacity=4 * 8000)
    g = eng.op(OpSpec(**{**spec.__dict__, "where": sql.compile_where(WINDOW_COND, NAMES)}))
    o = pyoracle.OracleOp(spec)
    wm = ctypes.c_int64(-1)
    rcs = []
    for key, ts, cols, valids in batches:
        g.push_async(narrow_keys(key) if narrow else key, ts, cols, valids, watermark=wm, done=rcs.append)
    g.wait()
    assert rcs == [abi.HSG_OK] * len(batches)
    wo = -1
    dropped = 0
    for (key, ts, cols, valids), keep in zip(batches, keeps):
        wo = o.push(np.where(keep, key, NONE).astype(np.uint32), ts, cols, valids, watermark=wo)
        dropped += int(np.count_nonzero((key != NONE) & ~keep))
    assert wm.value == wo
    rows_equal(g.drain(), o.drain(), spec.agg_is_f64(), ordered=True, what="async")
    assert g.stats()["where_dropped_total"] == dropped
    g.close()
    o.close()


def test_reset_keeps_the_program(eng):
    batches = _stream(110, per=5000)
    keeps = [np_keep(WINDOW_COND, NAMES, b[2], b[3]) for b in batches]
    spec = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=SIZE, col_types=TYPES, aggs=AGGS,
                  state_capacity=1 << 16)
    g = eng.op(OpSpec(**{**spec.__dict__, "where": sql.compile_where(WINDOW_COND, NAMES)}))
    key, ts, cols, valids = batches[0]
    g.push(key, ts, cols, valids)
    first = g.stats()["where_dropped"]
    assert first == int(np.count_nonzero((key != NONE) & ~keeps[0])) and len(g.drain()) > 0
    g.reset()
    o = pyoracle.OracleOp(spec)
    key, ts, cols, valids = batches[1]
    wg = g.push(key, ts, cols, valids)
    wo = o.push(np.where(keeps[1], key, NONE).astype(np.uint32), ts, cols, valids)
    assert wg == wo
    rows_equal(g.drain(), o.drain(), spec.agg_is_f64(), what="after reset")
    rows_equal(g.dump_state(), o.dump_state(), spec.agg_is_f64(), what="state after reset")
    st = g.stats()
    second = int(np.count_nonzero((key != NONE) & ~keeps[1]))
    assert st["where_dropped"] == second and st["where_dropped_total"] == first + second, st
    g.close()
    o.close()


# ---- 7. two ranks over the host transport ----------------------------------------------------------------
RANK_SPEC = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_RECORD, size_ms=10_000, col_types=[I, F, I],
                   aggs=[(CA, 0), (S, 0), (MX, 2)], state_capacity=1 << 14)
RANK_COND = sql.RCondOr(cmp(">", A, const(1)), cmp("<=", B, const(-0.5)))  # (c: aggregated; b: the filter's alone)


def _rank_slices(G):
    out = []
    for b in range(3):
        key, ts, cols, valids = gen(200 + b, 4000, nkeys=300, t0=TSB + b * 20_000, span=20_000)
        cuts = np.linspace(0, len(key), G + 1).astype(int)
        out.append([(key[cuts[r]:cuts[r + 1]], ts[cuts[r]:cuts[r + 1]], [c[cuts[r]:cuts[r + 1]] for c in cols],
                     [v[cuts[r]:cuts[r + 1]] for v in valids]) for r in range(G)])
    return out


def _tuples(r):
    return [(int(r.src_index[i]), int(r.key_id[i]), int(r.win_start[i]), int(r.win_end[i]),
             tuple(a[i].item() for a in r.aggs)) for i in range(len(r))]


def _rank_worker(rank, G, name, q):
    try:
        from hstream_amd.engine import Engine
        e = Engine(device=0, rank=rank, nranks=G, comm_id=name, batch_capacity=1 << 13,
                   transport=abi.HSG_TRANSPORT_HOST)
        op = e.op(OpSpec(**{**RANK_SPEC.__dict__, "where": sql.compile_where(RANK_COND, NAMES)}))
        wm, rows, dropped = -1, [], []
        for slices in _rank_slices(G):
            key, ts, cols, valids = slices[rank]
            wm = op.push(key, ts, cols, valids, watermark=wm)
            rows.append(_tuples(op.drain()))
            dropped.append(op.stats()["where_dropped"])
        state = op.dump_state().tuples()
        op.close()
        e.close()
        q.put((rank, wm, rows, state, dropped))
    except Exception as ex:  # reported to the parent, which fails the test
        q.put((rank, "error", repr(ex), None, None))


def test_two_ranks_filter_their_own_slices():
    import multiprocessing as mp
    G = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = f"hsgw-{os.getpid()}-{uuid.uuid4().hex[:12]}"
    procs = [ctx.Process(target=_rank_worker, args=(r, G, name, q)) for r in range(G)]
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
    o = pyoracle.OracleOp(RANK_SPEC)
    wm = -1
    for bi, slices in enumerate(_rank_slices(G)):
        key = np.concatenate([s[0] for s in slices])
        ts = np.concatenate([s[1] for s in slices])
        cols = [np.concatenate([s[2][c] for s in slices]) for c in range(3)]
        valids = [np.concatenate([s[3][c] for s in slices]) for c in range(3)]
        keep = host_keep(RANK_COND, NAMES, cols, valids)
        wm = o.push(np.where(keep, key, NONE).astype(np.uint32), ts, cols, valids, watermark=wm)
        ref = sorted(_tuples(o.drain()))
        got = sorted(outs[0][2][bi] + outs[1][2][bi])
        assert got == ref, (bi, len(got), len(ref))
        at = 0
        for r in range(G):
            n = len(slices[r][0])
            mine = int(np.count_nonzero((key[at:at + n] != NONE) & ~keep[at:at + n]))
            assert outs[r][4][bi] == mine, (bi, r)
            at += n
    assert all(out[1] == wm for out in outs)
    assert sorted(outs[0][3] + outs[1][3]) == sorted(o.dump_state().tuples())
    o.close()


# ---- 8. refusals ---------------------------------------------------------------------------------------------
def test_bad_program_is_refused_with_the_checkers_message(eng):
    from hstream_amd.engine import where_check
    W = abi
    bad = {
        "underflow": [(W.HSG_W_COL, 0), (W.HSG_W_GT,)],
        "column": [(W.HSG_W_COL, 3), (W.HSG_W_I64, 1), (W.HSG_W_GT,)],
        "value": [(W.HSG_W_COL, 0), (W.HSG_W_I64, 1), (W.HSG_W_ADD,)],
        "nan": [(W.HSG_W_COL, 1), (W.HSG_W_F64, float("nan")), (W.HSG_W_GT,)],
        "long": [(W.HSG_W_COL, 0), (W.HSG_W_I64, 1), (W.HSG_W_GT,)] + [(W.HSG_W_NOT,)] * 62,
    }
    for name, prog in bad.items():
        rc, msg = where_check(prog, TYPES)
        assert rc == abi.HSG_E_INVALID and msg
        with pytest.raises(abi.HStreamGpuError) as ei:
            eng.op(OpSpec(**{**UNWIN_PR.__dict__, "where": prog}))
        assert ei.value.status == abi.HSG_E_INVALID and msg in str(ei.value), (name, str(ei.value))
    # the engine is as usable as before
    cond = CONDS["a > 1"]
    b = gen(120, 700)
    check(eng, UNWIN_PR, cond, [b], [np_keep(cond, NAMES, b[2], b[3])], what="after refusals")
