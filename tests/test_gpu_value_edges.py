"""GPU: every aggregation path on full-width int64 and extreme f64 values.

The per-slot aggregate logic (S_SUM_I, S_MIN_F, f64_ord, the tie words, LAST)
is written once (csrc/hsg_slots.h) and instantiated per kernel family, each
over its own record layout, except that k_part_agg, k_pr_bucket / k_pr_keys,
k_agg_sql and k_ss_apply keep local forms of it (their register budgets);
the rest of the suite varies windows, emit modes, skew and transports over
values near 1e0 .. 1e9. Here one driver
pushes tests/valgen.py's columns -- int64 with a live high word, the int64
identities as real values, sums that cross +-2^63 in any order but arrival
order, doubles at the ends of the format, subnormal sums -- through
Engine.op(spec) and pyoracle.OracleOp(spec), once per kernel path. A column
under SUM / AVG takes the i64_wide / f64_samesign class, any other column the
extreme class (valgen.column_classes). Each case takes the input shape of the
existing test that reaches its path (named in its docstring) and that test's
hsg_stats assertion where a stat proves the path; only the values differ.

Compared after every batch: watermark, changelog, and dump_state at the end.
Integers, keys, windows, src_index bit-exact; f64 MIN / MAX / LAST equal with
no tolerance; f64 SUM / AVG (and an int64 AVG) within valgen.sum_rtol(n_max),
n_max the largest group of the case: the worst case of any summation order of
same-signed terms, derived, not measured. (atol 5e-324, one step of the
format: an AVG of subnormals rounds once more than the reference.) The SUM of
the subnormal keys: equal with no tolerance. Ops with HSG_OPF_LITERAL_FORMS:
hsg_rows.form against a restatement of the reference's sequential fold in
which the identities maxBound / minBound take part (Codegen.hs:438,451): a MIN
over values >= 2^63 - 1 keeps the initial value, a MAX whose value equals
INT64_MIN takes the record's literal.
"""
import numpy as np
import pytest

import pyoracle
import valgen
from hstream_amd import abi, datagen
from hstream_amd.columnar import OpSpec
from util import ALL_AGG_SETS, F64_RTOL, gen_small, rows_equal

pytestmark = pytest.mark.gpu

I, F = abi.HSG_I64, abi.HSG_F64
L, S, MN, MX, CA, CN, AV = (abi.HSG_LAST, abi.HSG_SUM, abi.HSG_MIN, abi.HSG_MAX, abi.HSG_COUNT_ALL, abi.HSG_COUNT,
                            abi.HSG_AVG)
PB, PR, NONE = abi.HSG_EMIT_PER_BATCH, abi.HSG_EMIT_PER_RECORD, abi.HSG_EMIT_NONE
FORMS = abi.HSG_OPF_LITERAL_FORMS
VT = pytest.mark.parametrize("vt", [I, F], ids=["i64", "f64"])
# one column under MIN / MAX / LAST / COUNT only: the extreme classes
EXT_AGGS = [(CA, 0), (CN, 0), (MN, 0), (MX, 0), (L, 0)]
FULL = ALL_AGG_SETS["full_i64"]  # every aggregate over one column (of either type)
SIZE = 60_000
TSB = (1_700_000_000_000 // SIZE + 1) * SIZE  # a window start


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need cuda:0"
    from hstream_amd.engine import Engine
    e = Engine(device=0, batch_capacity=1 << 20)
    yield e
    e.close()


# ---------------------------------------------------------------------------
# literal forms: the reference's sequential fold, identities included
# ---------------------------------------------------------------------------
def _entries(spec, key, ts):
    """(record, group id) of every (record, window) pair in arrival x window
    order; no record of a forms case is late."""
    ok = key != np.uint32(abi.HSG_KEY_NONE)
    k64 = key.astype(np.int64) << 32
    if spec.window_kind == abi.HSG_UNWINDOWED:
        rec = np.nonzero(ok)[0]
        return rec, k64[rec]
    rec = np.nonzero(ok & (ts >= 0))[0]
    adv = spec.advance_ms if spec.window_kind == abi.HSG_HOPPING else spec.size_ms
    first = np.maximum(0, ts[rec] - spec.size_ms + adv) // adv
    last = ts[rec] // adv
    rr, gg = [], []
    for j in range(int((last - first).max()) + 1 if len(rec) else 0):
        m = first + j <= last
        rr.append(rec[m])
        gg.append(k64[rec[m]] + first[m] + j)
    rr, gg = np.concatenate(rr), np.concatenate(gg)
    order = np.lexsort((gg, rr))
    return rr[order], gg[order]


def _seg_prev(x, first, init):
    """x shifted by one inside each segment, `init` at a segment's start."""
    p = np.empty_like(x)
    p[1:] = x[:-1]
    p[first] = init
    return p


def _column_forms(g_sorted, first, v, valid, f64):
    """Form bits of SUM / MIN / MAX / LAST over one column right after each
    entry (entries sorted by group, arrival order inside). The fold starts
    from maxBound / minBound, which take part: min n x = n keeps the initial
    value on a tie (bits 3), max n x = x takes the record's literal."""
    import pandas as pd
    present = (valid & 1) != 0
    dec = present & ((valid & 2) != 0)
    hi, lo = (2.0 ** 63, -(2.0 ** 63)) if f64 else (valgen.I64_MAX, valgen.I64_MIN)
    gb = lambda a: pd.Series(a).groupby(g_sorted, sort=False)
    vmin = np.where(present, v, hi)
    vmax = np.where(present, v, lo)
    # (the fold starts at the bounds: a double beyond them never moves it)
    run_min = gb(np.minimum(vmin, hi)).cummin().to_numpy()
    run_max = gb(np.maximum(vmax, lo)).cummax().to_numpy()
    new_min = present & (vmin < _seg_prev(run_min, first, hi))
    new_max = present & (vmax >= _seg_prev(run_max, first, lo))
    pos = np.arange(len(v))
    integral = ~dec

    def bits(flag):  # the literal of the last flagged entry so far; none: the initial value
        t = gb(np.where(flag, pos, -1)).cummax().to_numpy()
        return np.where(t < 0, 3, integral[np.maximum(t, 0)].astype(np.int64))

    return {S: (gb(dec.astype(np.int64)).cumsum().to_numpy() == 0).astype(np.int64), MN: bits(new_min),
            MX: bits(new_max), L: bits(present)}


def _form_words(spec, rec, gid, cols, valids):
    """hsg_rows.form of each entry's group right after the entry."""
    order = np.argsort(gid, kind="stable")
    gs, rs = gid[order], rec[order]
    first = np.r_[True, gs[1:] != gs[:-1]] if len(gs) else np.zeros(0, bool)
    word = np.zeros(len(gs), np.int64)
    per_col = {}
    for j, (kind, c) in enumerate(spec.aggs):
        if kind not in (S, MN, MX, L):
            continue
        if c not in per_col:
            per_col[c] = _column_forms(gs, first, cols[c][rs], valids[c][rs], spec.col_types[c] == F)
        word |= per_col[c][kind] << (2 * j)
    out = np.empty(len(gs), np.uint32)
    out[order] = word.astype(np.uint32)
    return out


def _row_gid(spec, rows):
    k64 = rows.key_id.astype(np.int64) << 32
    if spec.window_kind == abi.HSG_UNWINDOWED:
        return k64
    adv = spec.advance_ms if spec.window_kind == abi.HSG_HOPPING else spec.size_ms
    return k64 + rows.win_start // adv


class _Forms:
    def __init__(self, spec, batches):
        key = np.concatenate([b[0] for b in batches])
        ts = np.concatenate([b[1] for b in batches])
        cols = [np.concatenate([b[2][c] for b in batches]) for c in range(len(spec.col_types))]
        valids = [np.concatenate([b[3][c] for b in batches]) for c in range(len(spec.col_types))]
        self.spec = spec
        self.rec, self.gid = _entries(spec, key, ts)
        self.word = _form_words(spec, self.rec, self.gid, cols, valids)

    def _last_of_groups(self, lo, hi):
        """Per group touched by records lo .. hi - 1: its last entry's word."""
        a, b = np.searchsorted(self.rec, [lo, hi])
        g, w = self.gid[a:b][::-1], self.word[a:b][::-1]
        ug, at = np.unique(g, return_index=True)
        return ug, w[at]

    def check_batch(self, rows, lo, hi, what):
        rows = rows.sorted()
        rg = _row_gid(self.spec, rows)
        if self.spec.emit_mode == PR:  # one row per entry, in arrival x window order
            a, b = np.searchsorted(self.rec, [lo, hi])
            order = np.lexsort((rows.win_start, rows.src_index))
            np.testing.assert_array_equal(rows.src_index[order], self.rec[a:b], err_msg=f"{what}: entries")
            np.testing.assert_array_equal(rg[order], self.gid[a:b], err_msg=f"{what}: entry groups")
            np.testing.assert_array_equal(rows.form[order], self.word[a:b], err_msg=f"{what}: forms")
            return
        ug, w = self._last_of_groups(lo, hi)
        order = np.argsort(rg, kind="stable")
        np.testing.assert_array_equal(rg[order], ug, err_msg=f"{what}: groups")
        np.testing.assert_array_equal(rows.form[order], w, err_msg=f"{what}: forms")

    def check_state(self, rows, n):
        """dump_state after n records: every group's last entry (the default
        grace retires no window inside a case)."""
        mode, self.spec.emit_mode = self.spec.emit_mode, PB
        try:
            self.check_batch(rows, 0, n, "state")
        finally:
            self.spec.emit_mode = mode


# ---------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------
def _spec(kind, emit, col_types, aggs, forms=False, **kw):
    return OpSpec(kind, emit, col_types=col_types, aggs=aggs, flags=FORMS if forms else 0, **kw)


def _drive(eng, spec, shapes, seed=1, faithful=False):
    """shapes: [(key, ts)] per batch, an existing test's; valgen fills the
    columns. Returns (hsg_stats, the batches)."""
    n_total = sum(len(k) for k, _ in shapes)
    classes = valgen.column_classes(spec.col_types, spec.aggs)
    dedicated = valgen.dedicated_after([k for k, _ in shapes])
    pl = valgen.Planter(seed, classes, n_total, dedicated, decimal=0.3 if spec.literal_forms else 0.0)
    batches = [pl.batch(k, t) for k, t in shapes]
    rtol = valgen.sum_rtol(valgen.max_group(spec, batches))
    assert rtol <= F64_RTOL
    f64s, exact = spec.agg_is_f64(), valgen.exact_mask(spec)
    sub_sums = [j for j, (kind, c) in enumerate(spec.aggs) if kind == S and spec.col_types[c] == F]
    ordered = spec.emit_mode == PR
    forms = _Forms(spec, batches) if spec.literal_forms else None

    def same(a, b, what, ordered=False):
        rows_equal(a, b, f64s, ordered=ordered, what=what, exact_f64=exact, rtol=rtol, atol=5e-324)
        if sub_sums:  # the subnormal keys' sums: exact
            if not ordered:
                a, b = a.sorted(), b.sorted()
            m = np.isin(a.key_id, dedicated)
            for j in sub_sums:
                np.testing.assert_array_equal(a.aggs[j][m], b.aggs[j][m], err_msg=f"{what}: subnormal SUM {j}")

    g, o = eng.op(spec), pyoracle.OracleOp(spec, faithful_sessions=faithful)
    wg = wo = -1
    base = 0
    for bi, (k, t, c, va) in enumerate(batches):
        wg = g.push(k, t, c, va, watermark=wg)
        wo = o.push(k, t, c, va, watermark=wo)  # (HSG_E_RANGE here would be a generator bug)
        assert wg == wo, f"batch {bi}: watermark {wg} != {wo}"
        if spec.emit_mode != NONE:
            a, b = g.drain(), o.drain()
            same(a, b, f"batch {bi}", ordered)
            if forms is not None:
                forms.check_batch(a, base, base + len(k), f"batch {bi}")
        base += len(k)
    a, b = g.dump_state(), o.dump_state()
    same(a, b, "state")
    if forms is not None:
        forms.check_state(a, base)
    st = g.stats()
    g.close()
    o.close()
    return st, batches


# ---------------------------------------------------------------------------
# shapes (keys and timestamps of the tests named in each case)
# ---------------------------------------------------------------------------
def _uniform(rng, n, nkeys, t0, span):
    """tests/test_gpu_lean.py _uniform: sorted ts over `span` ms."""
    return rng.integers(0, nkeys, size=n).astype(np.uint32), (t0 + np.sort(rng.integers(0, span, size=n))).astype(np.int64)


def _lean_shapes(seed, hot):
    rng = np.random.default_rng(seed)
    out, t = [], 10_000_000
    for b in range(3):
        k, ts = _uniform(rng, 60_000 if not hot else 200_000, 2_000, t, 600_000)
        if hot and b == 1:
            k[rng.random(len(k)) < 0.8] = 7  # ~160K records of one key: its bucket exceeds a workgroup's chunk
        out.append((k, ts))
        t += 600_000
    return out


def _small(seed, nb, n, nkeys, span, base, step=None, **kw):
    """util.gen_small's keys and timestamps (its messy records included)."""
    out = []
    for b in range(nb):
        key, ts, _c, _v = gen_small(seed + b, n, nkeys, span=span, base=base + b * (span if step is None else step), **kw)
        out.append((key, ts))
    return out


def _sql_spread(rng, n, start, total, span):
    i = np.arange(start, start + n, dtype=np.int64)
    return TSB + (i * span) // total + rng.integers(0, 2000, size=n)


def _sql_uniform(seed=3, nb=3, per=60_000, nkeys=2_000):
    """tests/test_gpu_sql_wide.py _uniform."""
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, nkeys, size=per).astype(np.uint32), _sql_spread(rng, per, b * per, nb * per, 3 * SIZE))
            for b in range(nb)]


def _sql_hot(seed=7, nb=2, per=150_000):
    """tests/test_gpu_sql_wide.py test_sql_wide_hot_key: one key holds half of
    each batch, 75 000 records in one bucket: more than two aggregation chunks
    of 32 768 and more than kPrHot = 65 536."""
    rng = np.random.default_rng(seed)
    return [(np.where(rng.random(per) < 0.5, 77, rng.integers(100, 2_100, size=per)).astype(np.uint32),
             _sql_spread(rng, per, b * per, nb * per, 3 * SIZE)) for b in range(nb)]


def _one_window_ts(n, start):
    return TSB + (np.arange(start, start + n, dtype=np.int64) >> 6)


# ---------------------------------------------------------------------------
# the matrix
# ---------------------------------------------------------------------------
@VT
@pytest.mark.parametrize("hot", [False, True], ids=["uniform", "hot_key"])
def test_lean_one_window(eng, vt, hot):
    """k_agg_lean + k_pane_apply (baked C_AGGS_FULL programs of both types):
    test_gpu_lean.py test_lean_shape_transitions' uniform batch (at 60 000
    records) and its hot-key batch, whose bucket is split over workgroups.
    SUM and AVG read the column, so it holds the wide / same-sign class."""
    spec = _spec(abi.HSG_TUMBLING, PB, [vt], datagen.C_AGGS_FULL, size_ms=10_000, state_capacity=1 << 20)
    st, batches = _drive(eng, spec, _lean_shapes(5, hot))
    assert st["lean_batches"] == len(batches), st
    if hot:
        assert st["direct_batches"] < len(batches), st  # the split bucket: the changelog from the touched list


@VT
@pytest.mark.parametrize("kind", ["hop-pane", "hop-fanout"])
def test_part_agg_hopping(eng, vt, kind):
    """k_part_agg + k_seg_apply in pane mode (and the fan-out spill):
    test_gpu_parity.py test_dense_groups_rounds at 2 x 20 000 records over
    6 000 keys (every record in 12 windows: the oracle's time sets the size)."""
    kw = dict(size_ms=60_000, advance_ms=5_000) if kind == "hop-pane" else dict(size_ms=50_000, advance_ms=15_000)
    spec = _spec(abi.HSG_HOPPING, PB, [vt], [(CA, 0), (S, 0), (MN, 0), (MX, 0)], state_capacity=1_000_000, **kw)
    shapes = _small(7000, 2, 20_000, 6_000, 60_000, 50_000_000, very_late=False, none_frac=0.0, neg_frac=0.0)
    st, _b = _drive(eng, spec, shapes)
    assert st["lean_batches"] == 0, st


@pytest.mark.parametrize("types", [[I, F], [F, I]], ids=["i64_f64", "f64_i64"])
@pytest.mark.parametrize("emit", [PB, NONE], ids=["per_batch", "state_only"])
def test_part_agg_wide_records_runtime_program(eng, types, emit):
    """k_part_agg on two-column records with the runtime slot program
    (ALL_AGG_SETS["mixed"] without its LAST, which would move the op to the
    SQL kernels): test_gpu_parity.py test_time_windows_messy_batches, tumbling,
    without its late records (a batch with late records leaves the partition
    pipeline for the record kernels). Both columns are summed, in both type
    orders; not a lean shape (three-word records), no other stat."""
    aggs = [a for a in ALL_AGG_SETS["mixed"] if a[0] != L]
    spec = _spec(abi.HSG_TUMBLING, emit, types, aggs, size_ms=10_000)
    st, _b = _drive(eng, spec, _small(1000, 3, 5000, 37, 100_000, 10_000_000, very_late=False))
    assert st["lean_batches"] == 0, st


@VT
@pytest.mark.parametrize("cls", ["sum", "ext"])
def test_record_kernels_late_batch(eng, vt, cls):
    """k_tw_agg: test_gpu_lean.py test_lean_late_batch_after_prediction (at
    60 000 records): batch 2 has records beyond the grace and runs on the
    record kernels between lean batches. cls ext: MIN / MAX / COUNT / LAST
    over the extreme class (an op with LAST: the SQL kernels, then the record
    kernels with their LAST / tie pass for the late batch)."""
    aggs = datagen.C_AGGS_FULL if cls == "sum" else EXT_AGGS
    spec = _spec(abi.HSG_TUMBLING, PB, [vt], aggs, size_ms=10_000, state_capacity=1 << 20)
    rng = np.random.default_rng(9)
    # (from 200 000 s on: a record late by more than the 86 400 s grace still has a timestamp >= 0 and a closed window)
    shapes, t = [], 200_000_000
    for bi in range(4):
        k, ts = _uniform(rng, 60_000, 3_000, t, 300_000)
        if bi == 2:
            ts[::50] -= abi.HSG_DEFAULT_GRACE_MS + 400_000
        shapes.append((k, ts))
        t += 300_000
    st, batches = _drive(eng, spec, shapes)
    assert 1 <= st["lean_batches"] <= len(batches) - 1, st  # (the late batch at least is not a lean one)


@VT
@pytest.mark.parametrize("emit", [PB, PR], ids=["per_batch", "changes"])
def test_hopping_with_forms(eng, vt, emit):
    """Hopping ops with HSG_OPF_LITERAL_FORMS: the record kernels (k_tw_agg)
    per batch, the sort-based per-record path (k_perrecord) under EMIT
    CHANGES; no stat names either, the shape is test_time_windows_messy_batches'
    (in-time records, so the form restatement needs no drop rule). Values,
    and the forms of SUM / MIN / MAX / LAST over both column classes."""
    spec = _spec(abi.HSG_HOPPING, emit, [vt, vt], [(CA, 0), (S, 0), (AV, 0), (MN, 1), (MX, 1), (L, 1), (MN, 0)],
                 forms=True, size_ms=10_000, advance_ms=3_000)
    _drive(eng, spec, _small(1000, 3, 5000, 37, 100_000, 10_000_000, very_late=False))


SQL_PROGRAMS = {
    # baked C2 / C5 programs of k_agg_sql (test_gpu_sql_shape.py AGGS / AGGS_C5): SUM reads the column
    "c2": ([(L, 0), (CA, 0), (S, 0), (AV, 0), (MN, 0), (MX, 0)], None),
    "c5": ([(L, 0), (S, 0), (MX, 0)], None),
    # runtime programs, one and two columns
    "rt1": ([(L, 0), (MN, 0), (S, 0)], None),
    "rt1_ext": ([(L, 0), (MN, 0), (MX, 0), (CN, 0)], None),
    "rt2": ([(S, 0), (L, 1), (CA, 0)], "mixed"),
    "rt2_ext": ([(MX, 0), (MN, 1), (L, 1), (S, 1), (CA, 0)], "mixed"),
}


@VT
@pytest.mark.parametrize("hot", [False, True], ids=["uniform", "hot_key"])
@pytest.mark.parametrize("prog", sorted(SQL_PROGRAMS))
def test_sql_lean_narrow(eng, prog, hot, vt):
    """k_agg_sql / k_sql_apply with forms: the baked C2 and C5 programs and
    runtime programs of one and two columns (two: the other column has the
    other type), on test_gpu_sql_wide.py's uniform shape and its hot-key shape
    (the bucket split over workgroups, partials met under the row's lock).
    C5's baked program has no MIN; the baked programs all hold a SUM, so the
    extreme classes run on the runtime programs (rt1_ext, rt2_ext)."""
    aggs, two = SQL_PROGRAMS[prog]
    types = [vt, F if vt == I else I] if two else [vt]
    spec = _spec(abi.HSG_TUMBLING, PB, types, aggs, forms=True, size_ms=SIZE, state_capacity=1 << 20)
    st, batches = _drive(eng, spec, _sql_hot() if hot else _sql_uniform())
    nb = len(batches)
    assert st["lean_batches"] == nb and st["replays"] == 0, st
    if hot:
        assert st["direct_batches"] < nb, st


WIDE = {  # tests/test_gpu_sql_wide.py QUERIES: every query reads int64 and f64 columns of both classes
    "q4": ([I, F, I, F], [(L, 0), (CA, 0), (S, 1), (AV, 1), (MN, 2), (MX, 3)]),
    "q5big": ([I, F, I, I, F], [(L, 0), (L, 1), (L, 2), (L, 3), (L, 4), (MN, 0), (MX, 1), (S, 2), (CA, 0)]),
    "q8": ([I, F, I, I, F, I, I, F], [(L, 7), (S, 6), (MN, 5), (MX, 4), (CN, 3), (CA, 0)]),
    # q4 with the types swapped, so that an int64 SUM and an f64 MIN run at this width too
    "q4s": ([F, I, F, I], [(L, 0), (CA, 0), (S, 1), (AV, 1), (MN, 2), (MX, 3)]),
}


def _wide_spec(query, kind=abi.HSG_TUMBLING, state_capacity=1 << 20):
    types, aggs = WIDE[query]
    return _spec(kind, PB, types, aggs, forms=True, size_ms=0 if kind == abi.HSG_UNWINDOWED else SIZE,
                 state_capacity=state_capacity)


@pytest.mark.parametrize("query", sorted(WIDE))
def test_sql_wide_uniform(eng, query):
    """k_agg_sql_wide, one partial per group (test_sql_wide_uniform)."""
    st, batches = _drive(eng, _wide_spec(query), _sql_uniform())
    nb = len(batches)
    assert st["lean_batches"] == nb and st["replays"] == 0 and st["direct_batches"] == nb, st


@pytest.mark.parametrize("query", ["q4s", "q5big"])
def test_sql_wide_rounds(eng, query):
    """Key-hash rounds (test_sql_wide_rounds, its sizes: the rounds need
    ~3 700 groups in each of 16 buckets)."""
    rng = np.random.default_rng(5)
    shapes, start = [], 0
    for n, nk in zip([20_000, 200_000, 200_000], [50, 60_000, 60_000]):
        shapes.append((rng.integers(0, nk, size=n).astype(np.uint32), _one_window_ts(n, start)))
        start += n
    st, batches = _drive(eng, _wide_spec(query), shapes)
    nb = len(batches)
    assert st["lean_batches"] == nb and st["replays"] == 0, st


@pytest.mark.parametrize("query", ["q4", "q5big", "q8"])
def test_sql_wide_hot_key(eng, query):
    """A bucket split over workgroups (test_sql_wide_hot_key, its sizes)."""
    st, batches = _drive(eng, _wide_spec(query), _sql_hot())
    nb = len(batches)
    assert st["lean_batches"] == nb and st["replays"] == 0 and st["direct_batches"] < nb, st


def test_sql_wide_record_partials(eng):
    """Records that find no room in 64 rounds of the table, each a partial of
    its own (test_sql_wide_record_partials, its sizes: a chunk must hold more
    groups than 64 x 7/8 x 512)."""
    rng = np.random.default_rng(9)
    n0, n1 = 20_000, 1 << 19
    shapes = [(rng.integers(0, 50, size=n0).astype(np.uint32), _one_window_ts(n0, 0)),
              ((rng.permutation(n1) + 1_000).astype(np.uint32), _one_window_ts(n1, n0))]
    st, batches = _drive(eng, _wide_spec("q5big", state_capacity=1 << 22), shapes)
    nb = len(batches)
    assert st["lean_batches"] == nb and st["replays"] == 0 and st["direct_batches"] < nb, st


@VT
@pytest.mark.parametrize("sig", ["c2", "full", "ext", "sql_c2"])
def test_per_record_bucket(eng, vt, sig):
    """EMIT CHANGES of a one-window op on the bucket path (k_pr_bucket, its
    segments and lane-order folds): test_gpu_parity.py
    test_per_record_bucket_segments at 3 x 2^16 records (200 000 keys over 16
    buckets still hold far more groups than a bucket's LDS table, hot keys
    fill whole waves). Specialised (c2) and runtime programs, the SQL shape
    with forms; ordered row-for-row equality, no stat."""
    aggs = {"c2": datagen.C_AGGS_FULL, "full": FULL, "ext": EXT_AGGS, "sql_c2": SQL_PROGRAMS["c2"][0]}[sig]
    spec = _spec(abi.HSG_TUMBLING, PR, [vt], aggs, forms=sig == "sql_c2", size_ms=5_000)
    rng = np.random.default_rng(5)
    shapes = []
    for bi in range(3):
        n = 1 << 16
        key = rng.integers(0, 200_000, size=n).astype(np.uint32)
        key = np.where(rng.random(n) < 0.2, rng.integers(0, 4, size=n), key).astype(np.uint32)
        ts = (80_000_000 + bi * 20_000 + (np.arange(n) * 20_000) // n + rng.integers(0, 1_500, size=n)).astype(np.int64)
        shapes.append((key, ts))
    _drive(eng, spec, shapes)


@VT
@pytest.mark.parametrize("kind", ["tumbling", "unwindowed"])
def test_per_record_groups_span_chunks(eng, vt, kind):
    """EMIT CHANGES with three keys carrying whole batches: every group spans
    many k_pr_local chunks, k_pr_carry applies them in order
    (test_per_record_groups_span_chunks at 3 x 66 000 records)."""
    kw = dict(size_ms=10_000) if kind == "tumbling" else {}
    wk = abi.HSG_TUMBLING if kind == "tumbling" else abi.HSG_UNWINDOWED
    spec = _spec(wk, PR, [vt], FULL, **kw)
    _drive(eng, spec, _small(77, 3, 66_000, 3, 40_000, 5_000_000))


@VT
@pytest.mark.parametrize("shape", ["sql", "plain"])
def test_per_record_hot_key_chunked(eng, vt, shape):
    """EMIT CHANGES with a hot key whose partition bucket is over kPrHot =
    65 536 records (75 000 of each batch of 150 000, where
    test_per_record_hot_key_chunked holds ~1M: the threshold is what selects
    the chunked path): chunks in parallel, carries in order. No stat."""
    aggs = SQL_PROGRAMS["c2"][0] if shape == "sql" else [(CA, 0), (S, 0), (MX, 0), (MN, 0)]
    spec = _spec(abi.HSG_TUMBLING, PR, [vt], aggs, forms=shape == "sql", size_ms=SIZE)
    _drive(eng, spec, _sql_hot())


@VT
@pytest.mark.parametrize("cls", ["sum", "ext"])
def test_per_record_sort_path_hopping(eng, vt, cls):
    """EMIT CHANGES of hopping windows (k_pr_keys on the key-grouped replay;
    with LAST in the extreme set): test_per_record_key_replay long_runs at
    3 x 2^15 records, late records included."""
    aggs = [(CA, 0), (S, 0), (AV, 0), (MN, 0), (MX, 0), (CN, 0)] if cls == "sum" else EXT_AGGS
    spec = _spec(abi.HSG_HOPPING, PR, [vt], aggs, size_ms=60_000, advance_ms=5_000)
    _drive(eng, spec, _small(910, 3, 1 << 15, 500, 100_000, 7_000_000))


@VT
@pytest.mark.parametrize("gap", [0, 30_000])
def test_sessions_mirror(eng, vt, gap):
    """k_ss_sort / k_ss_apply specialised on COUNT(*) / SUM with the entry's
    mirror: test_gpu_sessions.py test_mirror_fast_and_slow_keys (its 5 x
    40 000 records: keys after their last session and keys reaching back)."""
    spec = _spec(abi.HSG_SESSION, PB, [vt], [(CA, 0), (S, 0)], gap_ms=gap)
    rng = np.random.default_rng(71 + gap)
    shapes = []
    for bi in range(3):
        n = 40_000
        key = rng.integers(0, 6_000, size=n).astype(np.uint32)
        ts = 50_000_000 + bi * 200_000 + rng.integers(0, 200_000, size=n)
        back = rng.random(n) < 0.15
        shapes.append((key, np.where(back, ts - rng.integers(100_000, 600_000, size=n), ts).astype(np.int64)))
    _drive(eng, spec, shapes)


@pytest.mark.parametrize("ncols", [3, 8])
def test_sessions_many_columns_list(eng, ncols):
    """The session merge path on the list (k_ss_apply, k_ss_merge_big for the
    hot key of batch 2) with records of 3 and 8 columns, int64 and f64
    alternating: test_many_columns_merge_path. SUM columns and MIN / MAX
    columns of both types."""
    types = [I if c % 2 == 0 else F for c in range(ncols)]
    aggs = ([(CA, 0)] + [((S, MX, MN)[c % 3], c) for c in range(ncols)])[:8]
    spec = _spec(abi.HSG_SESSION, PB, types, aggs, gap_ms=700)
    shapes = _small(900, 3, 60_000, 4_000, 150_000, 9_000_000, step=120_000)
    k, t = shapes[2]
    shapes[2] = (np.where((np.arange(k.size) % 3 == 0) & (k != abi.HSG_KEY_NONE), np.uint32(7), k).astype(np.uint32), t)
    _drive(eng, spec, shapes)


@pytest.mark.parametrize("types", [[I, F], [F, I]], ids=["i64_f64", "f64_i64"])
@pytest.mark.parametrize("mode", [PR, PB], ids=["changes", "per_batch_last"])
@pytest.mark.parametrize("hot", [False, True], ids=["bucket_replay", "hot_key_falls_back"])
def test_sessions_bucket_replay(eng, types, mode, hot):
    """k_br_*: test_gpu_sessions.py test_bucket_replay (3 x 60 000 records,
    gap 700) and test_bucket_replay_hot_key_falls_back (its sizes): a key
    over kBrCap records flags the batch onto the sort-based replay. Column 0
    under SUM / MAX, column 1 under LAST / MIN / MAX: the extreme class."""
    aggs = [(CA, 0), (S, 0), (MX, 0), (L, 1), (MN, 1), (MX, 1), (CN, 1)]
    spec = _spec(abi.HSG_SESSION, mode, types, aggs, gap_ms=400 if hot else 700)
    if hot:
        shapes = []
        for bi in range(2):
            key, ts, _c, _v = gen_small(31 + bi, 60_000, 50_000, span=200_000, base=20_000_000 + bi * 150_000)
            rng = np.random.default_rng(131 + bi)
            h = (rng.random(60_000) < 0.4) & (key != abi.HSG_KEY_NONE)
            shapes.append((np.where(h, rng.integers(0, 3, size=60_000).astype(np.uint32), key).astype(np.uint32), ts))
        shapes.insert(1, _small(700, 1, 60_000, 5_000, 200_000, 20_100_000)[0])
    else:
        shapes = _small(610, 3, 60_000, 20_000, 300_000, 9_000_000, step=200_000)
    st, _b = _drive(eng, spec, shapes)
    assert st["replays"] == (2 if hot else 0), st


@VT
@pytest.mark.parametrize("emit", [PB, PR], ids=["per_batch", "changes"])
@pytest.mark.parametrize("cls", ["sum", "ext"])
def test_unwindowed(eng, vt, emit, cls):
    """HSG_UNWINDOWED per batch and per record (test_time_windows_messy_batches'
    shape): a key's group lasts the whole case."""
    spec = _spec(abi.HSG_UNWINDOWED, emit, [vt], datagen.C_AGGS_FULL if cls == "sum" else EXT_AGGS)
    _drive(eng, spec, _small(1000, 3, 5000, 37, 100_000, 10_000_000))


@pytest.fixture(scope="module")
def xeng():
    import torch
    assert torch.cuda.is_available()
    from hstream_amd.engine import Engine, comm_unique_id
    e = Engine(device=0, rank=0, nranks=1, comm_id=comm_unique_id(), batch_capacity=1 << 20)
    yield e
    e.close()


@pytest.mark.parametrize("types", [[I, F], [F, I]], ids=["i64_f64", "f64_i64"])
@pytest.mark.parametrize("xpart", [None, "classic"], ids=["xpart1", "classic"])
def test_exchange_single_rank(xeng, types, xpart):
    """The exchange at one rank (owner partition, all-to-all with itself,
    unpack): test_exchange_path_single_rank's tumbling per-batch spec with
    late records, on the default and the classic exchange; every keyed record
    is owned (records_owned, as that test)."""
    from hstream_amd.engine import testing_knob
    aggs = [(CA, 0), (S, 0), (AV, 0), (MX, 0), (MN, 1), (MX, 1), (CN, 1), (L, 1)]
    spec = _spec(abi.HSG_TUMBLING, PB, types, aggs, size_ms=10_000)
    shapes = _small(2000, 3, 4000, 29, 60_000, 5_000_000)

    class _Knobbed:  # the knobs are read when the op is created
        def op(self, s):
            with testing_knob(abi.HSG_KNOB_XPART_LOG2, -1), \
                    testing_knob(abi.HSG_KNOB_X_CLASSIC, 1 if xpart == "classic" else 0):
                return xeng.op(s)

    st, batches = _drive(_Knobbed(), spec, shapes)
    keyed = sum(int((b[0] != abi.HSG_KEY_NONE).sum()) for b in batches)
    windowed = sum(int(((b[0] != abi.HSG_KEY_NONE) & (b[1] >= 0)).sum()) for b in batches)
    assert st["records_owned"] in ({keyed} if xpart == "classic" else {keyed, windowed}), st
