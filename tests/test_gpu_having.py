"""GPU: HAVING pushdown (hsg_op_create_filtered, k_having.hip). The op filters
and compacts the changelog rows each push appends. The reference in every case
is the op's no-HAVING counterpart through the CPU oracle, its drained rows
filtered on the host by sql.gen_filter_r over the row's {alias: value} object
(a NaN f64 output is left out of the object: the engine's error value). Never
the code under test."""
import ctypes as C
import os
import uuid

import numpy as np
import pytest

import pyoracle
from hstream_amd import abi, sql
from hstream_amd.columnar import OpSpec, Rows
from util import rows_equal

pytestmark = pytest.mark.gpu

I, F = abi.HSG_I64, abi.HSG_F64
NONE = np.uint32(abi.HSG_KEY_NONE)
CA, CN, S, MN, MX, AV, L = (abi.HSG_COUNT_ALL, abi.HSG_COUNT, abi.HSG_SUM, abi.HSG_MIN, abi.HSG_MAX, abi.HSG_AVG,
                            abi.HSG_LAST)
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


@pytest.fixture(scope="module")
def T():
    from hstream_amd.engine import having_tile_rows
    return having_tile_rows()


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


def host_keep(cond, aliases, rows, f64):
    """gen_filter_r row by row over the emitted objects: every alias is in the
    object, except an f64 output that is NaN (the engine's error value); a
    throw drops the row, as a throwing filter drops the record."""
    keep = np.zeros(len(rows), bool)
    for i in range(len(rows)):
        obj = {}
        for a, x, f in zip(aliases, rows.aggs, f64):
            v = x[i].item()
            if not (f and v != v):
                obj[a] = v
        try:
            keep[i] = sql.gen_filter_r(cond, obj)
        except KeyError:
            keep[i] = False
    return keep


def select(rows, keep):
    return Rows(rows.key_id[keep], rows.win_start[keep], rows.win_end[keep], rows.src_index[keep],
                [a[keep] for a in rows.aggs], None)


def with_having(spec, cond, aliases, **more):
    return OpSpec(**{**spec.__dict__, "having": sql.compile_having(cond, aliases), **more})


def check(eng, spec, cond, aliases, batches, ordered=None, what="", gspec=None, opush=None):
    """Each batch through the op with the program and through the oracle
    without; the op's rows against the oracle's rows filtered on the host;
    watermarks, having_dropped, pending_rows; the state against the unfiltered
    state. Returns (stats, keeps per batch, oracle rows per batch)."""
    ordered = spec.emit_mode == abi.HSG_EMIT_PER_RECORD if ordered is None else ordered
    g, o = eng.op(gspec or with_having(spec, cond, aliases)), pyoracle.OracleOp(spec)
    f64 = spec.agg_is_f64()
    wg = wo = -1
    total = 0
    keeps, refs = [], []
    try:
        for bi, (key, ts, cols, valids) in enumerate(batches):
            wg = g.push(key, ts, cols, valids, watermark=wg)
            wo = (opush or (lambda op, *a, **k: op.push(*a, **k)))(o, key, ts, cols, valids, watermark=wo)
            assert wg == wo, f"{what} batch {bi}: watermark {wg} != {wo}"
            ref = o.drain()
            keep = host_keep(cond, aliases, ref, f64)
            keeps.append(keep)
            refs.append(ref)
            st = g.stats()
            dropped = int(np.count_nonzero(~keep))
            total += dropped
            assert st["pending_rows"] == g.pending() == int(np.count_nonzero(keep)), (what, bi, st["pending_rows"])
            assert st["having_dropped"] == dropped, (what, bi, st["having_dropped"], dropped)
            assert st["having_dropped_total"] == total, (what, bi)
            rows_equal(g.drain(), select(ref, keep), f64, ordered=ordered, what=f"{what} batch {bi}")
        # HAVING filters the emitted rows only: the state is the unfiltered op's
        rows_equal(g.dump_state(), o.dump_state(), f64, what=f"{what} state")
        return g.stats(), keeps, refs
    finally:
        g.close()
        o.close()


def gen(seed, n, nkeys=50, absent=0.2, none=0.05, vr=8, t0=TSB, span=200_000):
    """Columns [I64, F64]: small integers and multiples of 1/4 (f64 sums and
    the AVG division are then the same on both sides), ~20 % absent per
    column, a few HSG_KEY_NONE records."""
    rng = np.random.default_rng(seed)
    key = rng.integers(0, nkeys, size=n).astype(np.uint32)
    key[rng.random(n) < none] = NONE
    ts = (t0 + (np.arange(n, dtype=np.int64) * span) // max(1, n) + rng.integers(0, 2000, size=n)).astype(np.int64)
    cols = [rng.integers(-vr, vr + 1, size=n).astype(np.int64),
            rng.integers(-4 * vr, 4 * vr + 1, size=n).astype(np.float64) / 4.0]
    valids = [(rng.random(n) >= absent).astype(np.uint8) for _ in cols]
    return key, ts, cols, valids


# ---- 1. semantics -------------------------------------------------------------------
SEM_ALIASES = ["cnt", "s", "mx", "cb", "avg"]
SEM = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[I, F],
             aggs=[(CA, 0), (S, 0), (MX, 1), (CN, 1), (AV, 1)], state_capacity=1 << 12)
CNT, SUM_, MAX_, CB, AVG_ = (col(a) for a in SEM_ALIASES)
CONDS = {
    "comparison: s > 3": cmp(">", SUM_, const(3)),
    "comparison: avg >= -0.25": cmp(">=", AVG_, const(-0.25)),
    "logic: (cnt > 20 AND NOT mx < 6) OR s < -10": sql.RCondOr(
        sql.RCondAnd(cmp(">", CNT, const(20)), sql.RCondNot(cmp("<", MAX_, const(6)))), cmp("<", SUM_, const(-10))),
    "logic: cnt < 3 OR avg > 0": sql.RCondOr(cmp("<", CNT, const(3)), cmp(">", AVG_, const(0))),
    "logic: avg > 0 OR cnt < 3": sql.RCondOr(cmp(">", AVG_, const(0)), cmp("<", CNT, const(3))),
    "between: avg BETWEEN -1.5 AND mx - 6": sql.RCondBetween(const(-1.5), AVG_, binop("-", MAX_, const(6))),
    "between: cb BETWEEN 10 AND cnt - 8": sql.RCondBetween(const(10), CB, binop("-", CNT, const(8))),
    "arithmetic: s * 2 - cnt > cb + 1": cmp(">", binop("-", binop("*", SUM_, const(2)), CNT), binop("+", CB, const(1))),
    # (f64 arithmetic rounds where Scientific does not: the operands here are multiples of 1/4, exact in both)
    "arithmetic: mx * cb + 0.5 <= s * 4": cmp("<=", binop("+", binop("*", MAX_, CB), const(0.5)),
                                              binop("*", SUM_, const(4))),
    "mixed: cnt <= 40.5": cmp("<=", CNT, const(40.5)),
    "mixed: s <> 3.0": cmp("<>", SUM_, const(3.0)),
}


@pytest.fixture(scope="module")
def sem_batch():
    return gen(1, 4099)


@pytest.mark.parametrize("name", list(CONDS))
def test_semantics(eng, sem_batch, name):
    cond = CONDS[name]
    st, (keep,), (ref,) = check(eng, SEM, cond, SEM_ALIASES, [sem_batch], what=name)
    assert 0 < np.count_nonzero(keep) < len(keep), name
    nan = np.isnan(ref.aggs[4])
    assert np.any(nan), "no AVG row is NaN"
    if "avg" in name and "OR" not in name:
        assert not np.any(keep & nan), name  # the error value: dropped
    if name == "logic: cnt < 3 OR avg > 0":
        assert np.any(keep & nan)  # l true -> true without r
    if name == "logic: avg > 0 OR cnt < 3":
        assert not np.any(keep & nan)  # l error -> error


# ---- 2. tile edges ------------------------------------------------------------------
COUNT_PR = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, aggs=[(CA, 0)], state_capacity=1 << 12)
CNT1 = col("cnt")


def _one_key(n):
    return np.zeros(n, np.uint32)


def _pair_keys(n):
    return (np.arange(n) // 2).astype(np.uint32)


def _patterns(n, T):
    """(name, keys, condition, kept rows by construction); with one key the
    i-th row has cnt = i + 1, with a key per pair of rows cnt alternates 1, 2."""
    idx = np.arange(n)
    return [
        ("all", _one_key(n), cmp(">=", CNT1, const(1)), idx >= 0),
        ("none", _one_key(n), cmp("<", CNT1, const(1)), idx < 0),
        ("alternating", _pair_keys(n), cmp("=", CNT1, const(1)), idx % 2 == 0),
        ("first row only", _one_key(n), cmp("=", CNT1, const(1)), idx == 0),
        ("last row only", _one_key(n), cmp(">=", CNT1, const(max(n, 1))), idx == n - 1),
        ("a tile dropped, then kept", _one_key(n), cmp(">", CNT1, const(T)), idx >= T),
        ("a tile kept, then dropped", _one_key(n), cmp("<=", CNT1, const(T)), idx < T),
    ]


LENGTHS = {"0": lambda T: 0, "1": lambda T: 1, "63": lambda T: 63, "64": lambda T: 64, "65": lambda T: 65,
           "T-1": lambda T: T - 1, "T": lambda T: T, "T+1": lambda T: T + 1, "3T+17": lambda T: 3 * T + 17}


@pytest.mark.parametrize("length", list(LENGTHS))
def test_tile_edges(eng, T, length):
    n = LENGTHS[length](T)
    for name, key, cond, want in _patterns(n, T):
        if n == 0:
            key = np.full(5, NONE, np.uint32)  # records, but no row: a segment of length 0
        ts = TSB + np.arange(len(key), dtype=np.int64)
        st, (keep,), _ = check(eng, COUNT_PR, cond, ["cnt"], [(key, ts, [], None)], what=f"{length} {name}")
        np.testing.assert_array_equal(keep, want[:len(keep)], err_msg=f"{length} {name}")
        assert len(keep) == n and st["having_dropped"] == n - int(np.count_nonzero(want))


# ---- 3. a segment at a non-zero, unaligned offset --------------------------------------
def test_second_segment_starts_at_an_unaligned_pending(eng, T):
    n1, n2 = T + 77, 2 * T + 10
    k1 = np.arange(n1, dtype=np.uint32)                       # every cnt = 1: all kept
    fresh = np.arange(n1, n1 + n2, dtype=np.uint32)
    k2 = np.where(np.arange(n2) % 2 == 0, fresh, np.arange(n2, dtype=np.uint32) % n1).astype(np.uint32)
    k2[1::2] = np.arange(n2 // 2, dtype=np.uint32)            # odd rows: keys of batch 1 -> cnt = 2: dropped
    cond = cmp("=", CNT1, const(1))
    g, o = eng.op(with_having(COUNT_PR, cond, ["cnt"], out_capacity=4 * (n1 + n2))), pyoracle.OracleOp(COUNT_PR)
    try:
        ts1 = TSB + np.arange(n1, dtype=np.int64)
        ts2 = TSB + n1 + np.arange(n2, dtype=np.int64)
        g.push(k1, ts1, [], None)
        o.push(k1, ts1, [], None)
        r1 = o.drain()
        assert g.pending() == n1 and g.stats()["having_dropped"] == 0
        g.push(k2, ts2, [], None)
        o.push(k2, ts2, [], None)
        r2 = o.drain()
        keep2 = host_keep(cond, ["cnt"], r2, [False])
        assert np.count_nonzero(keep2) == n2 // 2 and np.array_equal(keep2, np.arange(n2) % 2 == 0)
        st = g.stats()
        assert st["pending_rows"] == g.pending() == n1 + n2 // 2
        assert st["having_dropped"] == n2 - n2 // 2 and st["having_dropped_total"] == n2 - n2 // 2
        got = g.drain()
        first = select(got, np.arange(len(got)) < n1)
        rest = select(got, np.arange(len(got)) >= n1)
        # the first batch's rows: bit-identical, untouched by the second pass
        for a, b in ((first.key_id, r1.key_id), (first.win_start, r1.win_start), (first.win_end, r1.win_end),
                     (first.src_index, r1.src_index), (first.aggs[0], r1.aggs[0])):
            assert a.tobytes() == b.tobytes()
        rows_equal(rest, select(r2, keep2), [False], ordered=True, what="second segment")
    finally:
        g.close()
        o.close()


# ---- 4. wide rows: 16 aggregates, literal forms -----------------------------------------
WIDE_TYPES = [I, I, I, I, F, F, F, F]
WIDE_AGGS = [(S, c) for c in range(8)] + [(CN, c) for c in range(7)] + [(CA, 0)]
WIDE_ALIASES = [f"s{c}" for c in range(8)] + [f"n{c}" for c in range(7)] + ["cnt"]
WIDE = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=WIDE_TYPES, aggs=WIDE_AGGS,
              flags=abi.HSG_OPF_LITERAL_FORMS, state_capacity=1 << 12)
WIDE_COND = sql.RCondOr(sql.RCondAnd(cmp(">", col("s0"), const(0)), cmp(">=", col("n1"), const(2))),
                        cmp("<", binop("+", col("s7"), col("cnt")), const(1.5)))


def test_wide_rows_and_literal_forms(eng, T):
    n = 3 * T + 41
    rng = np.random.default_rng(7)
    key = rng.integers(0, 40, size=n).astype(np.uint32)
    ts = TSB + np.arange(n, dtype=np.int64)
    cols = [rng.integers(-8, 9, size=n).astype(np.int64) if t == I else rng.integers(-32, 33, size=n) / 4.0
            for t in WIDE_TYPES]
    valids = [((rng.random(n) >= 0.2).astype(np.uint8) | (rng.integers(0, 2, size=n).astype(np.uint8) << 1))
              for _ in cols]
    batch = (key, ts, cols, valids)
    # the unfiltered op's rows carry the forms the oracle does not keep
    g0 = eng.op(WIDE)
    g0.push(*batch)
    full = g0.drain()
    g0.close()
    g = eng.op(with_having(WIDE, WIDE_COND, WIDE_ALIASES))
    o = pyoracle.OracleOp(WIDE)
    try:
        g.push(*batch)
        o.push(*batch)
        ref = o.drain()
        f64 = WIDE.agg_is_f64()
        keep = host_keep(WIDE_COND, WIDE_ALIASES, ref, f64)
        assert T < np.count_nonzero(keep) < n - T and len(ref) == len(full) == n
        got = g.drain()
        assert g.stats()["having_dropped"] == n - np.count_nonzero(keep)
        rows_equal(got, select(ref, keep), f64, ordered=True, what="wide")
        # every one of the 16 columns, and the form word, moved with its row
        assert got.form is not None and full.form is not None and np.any(full.form != full.form[0])
        assert got.form.tobytes() == full.form[keep].tobytes()
        for j in range(16):
            assert got.aggs[j].tobytes() == full.aggs[j][keep].tobytes(), j
        assert got.src_index.tobytes() == full.src_index[keep].tobytes()
    finally:
        g.close()
        o.close()


# ---- 5. exact comparison of an i64 output with an f64 constant -----------------------------
@pytest.mark.parametrize("op", [">", "="])
def test_exact_comparison_at_two_to_the_53(eng, op):
    # SUM(a) per key: 2^53 - 1, 2^53 | 2^53, 2^53 + 1 | 2^53 + 1, 2^53 + 2
    key = np.array([0, 1, 2, 0, 1, 2], dtype=np.uint32)
    a = np.array([2**53 - 1, 2**53, 2**53 + 1, 1, 1, 1], dtype=np.int64)
    ts = TSB + np.arange(6, dtype=np.int64)
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[I], aggs=[(S, 0)], state_capacity=1 << 10)
    cond = cmp(op, col("s"), const(9007199254740992.0))
    st, (keep,), (ref,) = check(eng, spec, cond, ["s"], [(key, ts, [a], None)], what=f"s {op} 2^53")
    assert ref.aggs[0].tolist() == [2**53 - 1, 2**53, 2**53 + 1, 2**53, 2**53 + 1, 2**53 + 2]
    want = {">": [0, 0, 1, 0, 1, 1], "=": [0, 1, 0, 1, 0, 0]}[op]
    assert keep.astype(int).tolist() == want


# ---- 6. every window kind, both emit modes ---------------------------------------------------
WIN_ALIASES = ["cnt", "s", "mx"]
WIN_AGGS = [(CA, 0), (S, 0), (MX, 1)]
WIN_COND = cmp(">", col("cnt"), const(2))


def _stream(seed, nb=3, per=1000, nkeys=60, **kw):
    return [gen(seed + b, per, nkeys=nkeys, t0=TSB + b * SIZE, span=SIZE, **kw) for b in range(nb)]


@pytest.mark.parametrize("emit", [abi.HSG_EMIT_PER_RECORD, abi.HSG_EMIT_PER_BATCH], ids=["changes", "batch"])
@pytest.mark.parametrize("kind,kw", [
    (abi.HSG_TUMBLING, dict(size_ms=SIZE)),
    (abi.HSG_HOPPING, dict(size_ms=SIZE, advance_ms=SIZE // 3)),
    (abi.HSG_SESSION, dict(gap_ms=2500)),
    # no grace: the records the jitter puts behind the next window's are late, and a
    # batch with late records runs its kernels a second time (filtered once)
    (abi.HSG_TUMBLING, dict(size_ms=SIZE, grace_ms=0)),
], ids=["tumbling", "hopping", "session", "tumbling_late"])
def test_window_kinds(eng, kind, kw, emit):
    spec = OpSpec(kind, emit, col_types=[I, F], aggs=WIN_AGGS, state_capacity=1 << 14, **kw)
    st, keeps, _ = check(eng, spec, WIN_COND, WIN_ALIASES, _stream(50), what=f"kind {kind} emit {emit}")
    kept = sum(int(np.count_nonzero(k)) for k in keeps)
    assert 0 < kept < sum(len(k) for k in keeps)
    if kw.get("grace_ms") == 0:
        assert st["late_dropped"] > 0, st


def test_tumbling_per_batch_stays_on_the_lean_path(eng):
    batches = [(k, t, c[:1], v[:1]) for k, t, c, v in _stream(60, per=20_000, nkeys=500, absent=0.03)]
    spec = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=SIZE, col_types=[I], aggs=[(CA, 0), (S, 0)],
                  state_capacity=1 << 16)
    cond = cmp(">", col("cnt"), const(38))
    st, keeps, _ = check(eng, spec, cond, ["cnt", "s"], batches, what="lean")
    assert st["lean_batches"] == st["batches"] == len(batches), st
    assert all(0 < np.count_nonzero(k) < len(k) for k in keeps)


# ---- 7. registered changelog columns -----------------------------------------------------------
def test_registered_changelog_columns(eng, T):
    import torch
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[I, F], aggs=WIN_AGGS,
                  state_capacity=1 << 12)
    cond = cmp(">", col("s"), const(0))
    g, o = eng.op(with_having(spec, cond, WIN_ALIASES)), pyoracle.OracleOp(spec)
    cap = 1 << 13
    cols = {k: torch.empty(cap, dtype=t, device="cuda") for k, t in
            (("key", torch.int32), ("ws", torch.int64), ("we", torch.int64), ("src", torch.int64))}
    f64 = spec.agg_is_f64()
    aggs = [torch.empty(cap, dtype=torch.float64 if f else torch.int64, device="cuda") for f in f64]
    ap = (C.c_void_p * len(aggs))(*[a.data_ptr() for a in aggs])
    rows = abi.hsg_rows(capacity=cap, mem=abi.HSG_MEM_DEVICE, n_aggs=len(aggs), key_id=cols["key"].data_ptr(),
                        win_start=cols["ws"].data_ptr(), win_end=cols["we"].data_ptr(),
                        src_index=cols["src"].data_ptr(), aggs=C.cast(ap, C.POINTER(C.c_void_p)))
    try:
        g.set_changelog(rows)
        wg = wo = -1
        for bi, (key, ts, cv, valid) in enumerate(_stream(70, nb=2, per=3 * T + 5)):
            wg = g.push(key, ts, cv, valid, watermark=wg)
            wo = o.push(key, ts, cv, valid, watermark=wo)
            ref = o.drain()
            keep = host_keep(cond, WIN_ALIASES, ref, f64)
            n = g.drain_count()
            assert n == np.count_nonzero(keep) and 0 < n < len(keep)
            torch.cuda.synchronize()
            got = Rows(cols["key"][:n].cpu().numpy().view(np.uint32), cols["ws"][:n].cpu().numpy(),
                       cols["we"][:n].cpu().numpy(), cols["src"][:n].cpu().numpy(), [a[:n].cpu().numpy() for a in aggs])
            rows_equal(got, select(ref, keep), f64, ordered=True, what=f"registered columns batch {bi}")
        g.set_changelog(None)
    finally:
        g.close()
        o.close()


# ---- 8. WHERE and HAVING on one op ----------------------------------------------------------------
def test_where_and_having_together(eng):
    names = ["a", "b"]
    where = cmp(">", col("a"), const(-2))
    having = sql.RCondAnd(cmp(">", col("cnt"), const(3)), cmp("<", col("mx"), const(7.5)))
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[I, F], aggs=WIN_AGGS, state_capacity=1 << 12)
    gspec = with_having(spec, having, WIN_ALIASES, where=sql.compile_where(where, names))
    batches = _stream(80, nb=2, per=3000)
    masks = []

    def opush(op, key, ts, cols, valids, watermark):
        m = np.zeros(len(key), bool)
        for i in range(len(key)):
            obj = {f: c[i].item() for f, c, v in zip(names, cols, valids) if v[i] & 1}
            try:
                m[i] = sql.gen_filter_r(where, obj)
            except KeyError:
                pass
        masks.append(int(np.count_nonzero((key != NONE) & ~m)))
        return op.push(np.where(m, key, NONE).astype(np.uint32), ts, cols, valids, watermark=watermark)

    st, keeps, _ = check(eng, spec, having, WIN_ALIASES, batches, gspec=gspec, opush=opush, what="where + having")
    assert st["where_dropped"] == masks[-1] > 0 and st["where_dropped_total"] == sum(masks)
    assert st["having_dropped"] == int(np.count_nonzero(~keeps[-1])) > 0
    assert st["having_dropped_total"] == sum(int(np.count_nonzero(~k)) for k in keeps)


# ---- 9. asynchronous pushes ------------------------------------------------------------------------
def test_async_pushes(eng):
    batches = _stream(90, nb=2, per=4000)
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[I, F], aggs=WIN_AGGS, state_capacity=1 << 12,
                  out_capacity=4 * 4000)
    cond = cmp(">", col("s"), const(1))
    g, o = eng.op(with_having(spec, cond, WIN_ALIASES)), pyoracle.OracleOp(spec)
    try:
        wm = C.c_int64(-1)
        rcs = []
        for key, ts, cols, valids in batches:
            g.push_async(key, ts, cols, valids, watermark=wm, done=rcs.append)
        g.wait()
        assert rcs == [abi.HSG_OK] * len(batches)
        wo = -1
        want, dropped = [], 0
        for key, ts, cols, valids in batches:
            wo = o.push(key, ts, cols, valids, watermark=wo)
            ref = o.drain()
            keep = host_keep(cond, WIN_ALIASES, ref, spec.agg_is_f64())
            want.append(select(ref, keep))
            dropped += int(np.count_nonzero(~keep))
        assert wm.value == wo
        both = Rows(*(np.concatenate([getattr(w, f) for w in want]) for f in ("key_id", "win_start", "win_end",
                                                                             "src_index")),
                    [np.concatenate([w.aggs[j] for w in want]) for j in range(3)], None)
        assert g.pending() == len(both)
        rows_equal(g.drain(), both, spec.agg_is_f64(), ordered=True, what="async")
        assert g.stats()["having_dropped_total"] == dropped > 0
    finally:
        g.close()
        o.close()


# ---- 10. reset ----------------------------------------------------------------------------------------
def test_reset_keeps_the_program_and_the_totals(eng):
    batches = _stream(110, nb=2, per=3000)
    spec = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_RECORD, size_ms=SIZE, col_types=[I, F], aggs=WIN_AGGS,
                  state_capacity=1 << 14)
    g = eng.op(with_having(spec, WIN_COND, WIN_ALIASES))
    try:
        firsts = []
        for bi in range(2):
            o = pyoracle.OracleOp(spec)  # a reset op is a fresh op
            key, ts, cols, valids = batches[bi]
            assert g.push(key, ts, cols, valids) == o.push(key, ts, cols, valids)
            ref = o.drain()
            keep = host_keep(WIN_COND, WIN_ALIASES, ref, spec.agg_is_f64())
            rows_equal(g.drain(), select(ref, keep), spec.agg_is_f64(), ordered=True, what=f"run {bi}")
            rows_equal(g.dump_state(), o.dump_state(), spec.agg_is_f64(), what=f"state {bi}")
            o.close()
            firsts.append(int(np.count_nonzero(~keep)))
            st = g.stats()
            assert st["having_dropped"] == firsts[-1] > 0 and st["having_dropped_total"] == sum(firsts), st
            g.reset()
            assert g.stats()["having_dropped_total"] == sum(firsts) and g.pending() == 0
    finally:
        g.close()


# ---- 11. two ranks over the host transport ---------------------------------------------------------------
RANK_SPEC = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[I, F], aggs=WIN_AGGS,
                   state_capacity=1 << 14)
RANK_COND = sql.RCondOr(cmp(">", col("cnt"), const(30)), cmp("<", col("s"), const(-3)))


def _rank_slices(G):
    out = []
    for b in range(3):
        key, ts, cols, valids = gen(200 + b, 4000, nkeys=300, t0=TSB + b * 20_000, span=20_000)
        cuts = np.linspace(0, len(key), G + 1).astype(int)
        out.append([(key[cuts[r]:cuts[r + 1]], ts[cuts[r]:cuts[r + 1]], [c[cuts[r]:cuts[r + 1]] for c in cols],
                     [v[cuts[r]:cuts[r + 1]] for v in valids]) for r in range(G)])
    return out


def _rank_worker(rank, G, name, q):
    try:
        from hstream_amd.engine import Engine
        from test_gpu_two_ranks import _rows
        e = Engine(device=0, rank=rank, nranks=G, comm_id=name, batch_capacity=1 << 13,
                   transport=abi.HSG_TRANSPORT_HOST)
        op = e.op(with_having(RANK_SPEC, RANK_COND, WIN_ALIASES))
        wm, rows, dropped = -1, [], []
        for slices in _rank_slices(G):
            key, ts, cols, valids = slices[rank]
            wm = op.push(key, ts, cols, valids, watermark=wm)
            rows.append(_rows(RANK_SPEC, op.drain()))
            dropped.append(op.stats()["having_dropped"])
        state = op.dump_state().tuples()
        op.close()
        e.close()
        q.put((rank, wm, rows, state, dropped))
    except Exception as ex:  # reported to the parent, which fails the test
        q.put((rank, "error", repr(ex), None, None))


def test_two_ranks_filter_their_own_rows():
    import multiprocessing as mp
    from test_gpu_two_ranks import _rows
    G = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = f"hsgh-{os.getpid()}-{uuid.uuid4().hex[:12]}"
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
    f64 = RANK_SPEC.agg_is_f64()
    for bi, slices in enumerate(_rank_slices(G)):
        key = np.concatenate([s[0] for s in slices])
        ts = np.concatenate([s[1] for s in slices])
        cols = [np.concatenate([s[2][c] for s in slices]) for c in range(2)]
        valids = [np.concatenate([s[3][c] for s in slices]) for c in range(2)]
        wm = o.push(key, ts, cols, valids, watermark=wm)
        ref = o.drain()
        keep = host_keep(RANK_COND, WIN_ALIASES, ref, f64)
        assert 0 < np.count_nonzero(keep) < len(keep)
        want = sorted(_rows(RANK_SPEC, select(ref, keep)), key=lambda t: t[3])
        got = sorted(outs[0][2][bi] + outs[1][2][bi], key=lambda t: t[3])
        assert got == want, (bi, len(got), len(want))
        # each rank's own rows stay in order, and the ranks' drops add up
        for r in range(G):
            src = [t[3] for t in outs[r][2][bi]]
            assert src == sorted(src), (bi, r)
        assert outs[0][4][bi] + outs[1][4][bi] == int(np.count_nonzero(~keep)), bi
    assert all(out[1] == wm for out in outs)
    assert sorted(outs[0][3] + outs[1][3]) == sorted(o.dump_state().tuples())
    o.close()


# ---- refusals ------------------------------------------------------------------------------------------------
def test_refusals(eng):
    from hstream_amd.engine import having_check
    bad = [(abi.HSG_W_COL, 3), (abi.HSG_W_I64, 1), (abi.HSG_W_GT,)]
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_RECORD, col_types=[I, F], aggs=WIN_AGGS)
    rc, msg = having_check(bad, spec)
    assert rc == abi.HSG_E_INVALID and "column 3 out of range" in msg
    with pytest.raises(abi.HStreamGpuError) as ei:
        eng.op(OpSpec(**{**spec.__dict__, "having": bad}))
    assert ei.value.status == abi.HSG_E_INVALID and msg in str(ei.value)
    # an op that emits nothing has nothing to filter
    with pytest.raises(abi.HStreamGpuError) as ei:
        eng.op(OpSpec(**{**spec.__dict__, "emit_mode": abi.HSG_EMIT_NONE, "having": [(abi.HSG_W_COL, 0), (abi.HSG_W_I64, 1),
                                                                                     (abi.HSG_W_GT,)]}))
    assert ei.value.status == abi.HSG_E_INVALID and "HSG_EMIT_NONE" in str(ei.value)
