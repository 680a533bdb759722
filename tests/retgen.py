"""Inputs of tests/test_gpu_retention_ops.py: one stream per op family that
hstream_amd/csrc/retention.cpp rebuilds a table under, built from the
generators and host mirrors of those families' own tests. Host only: the GPU
file drives these through a GpuOp and the oracle, tests/test_retention_inputs_host.py
checks with the oracle alone that every randomised stream closes enough
windows to spill whatever the engine does, and the hand-built boundary
batches' stream-time arithmetic."""
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

import litforms
import pyoracle
import test_gpu_having as H
import test_gpu_lean as LN
import test_gpu_map as M
import test_gpu_regions as RG
import test_gpu_sql_shape as S
import test_gpu_sql_wide as W
import test_gpu_where as WH
from hstream_amd import abi, datagen, sql
from hstream_amd.columnar import OpSpec
from util import ALL_AGG_SETS, gen_small

I, F = abi.HSG_I64, abi.HSG_F64
CA, CN, SUM, MN, MX, AV, LAST = (abi.HSG_COUNT_ALL, abi.HSG_COUNT, abi.HSG_SUM, abi.HSG_MIN, abi.HSG_MAX,
                                 abi.HSG_AVG, abi.HSG_LAST)
NONE = np.uint32(abi.HSG_KEY_NONE)
GID = 1 << 40  # group id = key * GID + window index (ts // advance < 2^40)
PER_BATCH, CHANGES = abi.HSG_EMIT_PER_BATCH, abi.HSG_EMIT_PER_RECORD


@dataclass
class Case:
    spec: OpSpec                       # the op under test
    batches: List[tuple]               # (key, ts, cols, valids) it is pushed
    ospec: Optional[OpSpec] = None     # the oracle's op (a filtered / mapped op: its plain counterpart)
    obatches: Optional[List[tuple]] = None  # what the oracle is pushed (host-filtered, host-mapped)
    wms: Optional[List] = None         # per batch: a stream time the caller sets, or None = the last returned
    having: Optional[tuple] = None     # (condition, aliases): the changelog's host mirror
    forms: Optional[str] = None        # "sql" (litforms._prefix_forms) / "wide" (test_gpu_sql_wide's)

    def __post_init__(self):
        self.ospec = self.ospec or self.spec
        self.obatches = self.obatches or self.batches
        self.wms = self.wms or [None] * len(self.batches)

    @property
    def adv(self):
        return self.spec.advance_ms if self.spec.window_kind == abi.HSG_HOPPING else self.spec.size_ms

    def exact_f64(self):
        return [k in (MN, MX, LAST) for k, _ in self.ospec.aggs]

    def group_ids(self):
        key = np.concatenate([b[0] for b in self.batches]).astype(np.int64)
        ts = np.concatenate([b[1] for b in self.batches])
        return key * GID + ts // self.adv

    def accepted(self):
        """Tumbling ops: per record of the whole sequence, whether the grace
        check lets it into its window (TimeWindowedStream.hs:92 on the running
        stream time, Processor.hs:139), the caller's lowered watermarks included."""
        assert self.spec.window_kind == abi.HSG_TUMBLING
        out, w = [], -1
        for (key, ts, _c, _v), wm in zip(self.batches, self.wms):
            w = w if wm is None else wm
            run = np.maximum(np.maximum.accumulate(ts), w)
            we = (ts // self.adv + 1) * self.adv
            out.append((key != NONE) & (run < we + self.spec.grace_ms))
            w = int(run[-1])
        return np.concatenate(out)

    def form_words(self):
        """Literal-form word of each record's group right after the record,
        over the whole record sequence in arrival order (every record of these
        streams is accepted: asserted)."""
        assert bool(np.all(self.accepted())), "a record of a forms stream is late"
        gid = self.group_ids()
        nc = len(self.spec.col_types)
        cols = [np.concatenate([b[2][c] for b in self.batches]) for c in range(nc)]
        valids = [np.concatenate([b[3][c] for b in self.batches]) for c in range(nc)]
        if self.forms == "sql":
            return gid, litforms._prefix_forms(gid, cols[0], valids[0], self.spec.col_types[0] == F, self.spec.aggs)
        return gid, W._prefix_forms(gid, cols, valids, list(self.spec.col_types), list(self.spec.aggs))


def expected_forms(rows, gid, fw, lo, hi, adv):
    """The form word each row must carry: its group's word after the group's
    last record among records lo .. hi - 1."""
    groups, last_idx = W._last_of_groups(gid, lo, hi, np.ones(len(gid), bool))
    rg = rows.key_id.astype(np.int64) * GID + rows.win_start // adv
    pos = np.minimum(np.searchsorted(groups, rg), len(groups) - 1)
    assert np.array_equal(groups[pos], rg), "a row of a group no record of the range reached"
    return fw[last_idx[pos]]


def closed_groups(case):
    """(closed, total, final stream time) from the oracle alone: the groups of
    its final dump whose window no later record could enter."""
    o = pyoracle.OracleOp(case.ospec)
    w = -1
    for (key, ts, cols, valids), wm in zip(case.obatches, case.wms):
        w = o.push(key, ts, cols, valids, watermark=w if wm is None else wm)
    d = o.dump_state()
    o.close()
    return int(np.count_nonzero(d.win_end + case.ospec.grace_ms <= w)), len(d), w


def assert_spills_by_construction(case):
    """No engine could keep this stream resident in the op's table: closed
    groups are at least half of all groups and at least four times the
    state capacity."""
    closed, total, _ = closed_groups(case)
    assert 2 * closed >= total and closed >= 4 * case.spec.state_capacity, (closed, total, case.spec.state_capacity)
    return closed, total


# ---- 1. the SQL shape with literal forms ---------------------------------------------------------
# The engine sizes a rebuilt table for twice (resident rows + the batch's
# records), and rebuilds only when resident rows + records pass 3/4 of it: a
# stream spills only if its batches create groups at a rate comparable to their
# records, over more batches than such a table absorbs. The lean kernels take
# a batch only when its whole time span lies inside the grace
# (k_part.hip part_decide_body: stream time <= earliest ts + grace), so a lean
# stream advances in steps: each batch inside the grace, the next one several
# windows plus the grace later.
SQL_STEP = 5_000  # ms between batches: 2 windows + the 2 s grace, and one more


def _sql_batches(seed, f64, sizes, nkeys, first=0):
    """S._gen with its linear spread switched off (total = 10^12): every ts of a
    batch in [TS0, TS0 + 2 s), its 2 s of disorder; batch b then moved
    (first + b) * SQL_STEP later."""
    out = []
    for b, (n, nk) in enumerate(zip(sizes, nkeys)):
        k, t, v, va = S._gen(seed, n, (first + b) * 20_000, 10**12, nk, f64)
        assert int(t.max() - t.min()) < 2_000
        out.append((k, t + (first + b) * SQL_STEP, [v], [va]))
    return out


def sql_forms_spec(f64, emit, cap=256):
    return OpSpec(abi.HSG_TUMBLING, emit, size_ms=1000, grace_ms=2000, col_types=[F if f64 else I],
                  aggs=litforms.AGGS, flags=abi.HSG_OPF_LITERAL_FORMS, state_capacity=cap)


def sql_forms_case(f64, emit, cap=256, nb=10):
    """1 s tumbling windows, grace 2 s. A first batch of 2 000 records over 20
    keys (40 groups: inside a 256-row table's room, so the lean apply has no
    reason to hold back), then `nb` of 10 000 records over 2 500 keys: two
    windows and ~4 300 groups per batch, 5 s from batch to batch, so a batch's
    windows are closed when the batch after the next arrives. Each batch's 2 s
    of disorder stays inside the grace: no record is late, and every batch
    qualifies for the lean kernels."""
    b = _sql_batches(7 + f64, f64, [2_000] + [10_000] * nb, [20] + [2_500] * nb)
    return Case(sql_forms_spec(f64, emit, cap), b, forms="sql")


# ---- 2. the widest rows ------------------------------------------------------------------------------
def wide_case(emit, query="q8", cap=256, nb=10):
    """test_gpu_sql_wide's 8-column query (60 s windows), grace 600 s: 2 000
    records over 10 keys, then batches of 10 000 records over 500 keys, each
    over 8 windows (478 s + 2 s of disorder: inside the grace, none late, lean)
    and 20 windows after the one before: ~3 700 groups per batch."""
    col_types, aggs = W.QUERIES[query]
    spec = OpSpec(abi.HSG_TUMBLING, emit, size_ms=W.SIZE, grace_ms=10 * W.SIZE, col_types=col_types, aggs=aggs,
                  flags=abi.HSG_OPF_LITERAL_FORMS, state_capacity=cap)
    rng = np.random.default_rng(13)
    batches = []
    for bi, (n, nk) in enumerate(zip([2_000] + [10_000] * nb, [10] + [500] * nb)):
        ts = W._spread_ts(rng, n, 0, n, 8 * W.SIZE - 2_000) + bi * 20 * W.SIZE
        batches.append(W._batch(130 + bi, n, rng.integers(0, nk, size=n), ts, col_types))
    return Case(spec, batches, forms="wide")


# ---- 3. hopping: pane mode and fan-out -------------------------------------------------------------------
HOP_AGGS = [(CA, 0), (SUM, 0), (MN, 0), (MX, 0), (SUM, 1), (MN, 1), (MX, 1)]
HOPS = {"hop-pane": dict(size_ms=3_000, advance_ms=250), "hop-fanout": dict(size_ms=2_500, advance_ms=750)}
HOP_KEYS = {"hop-pane": (1_200, 5), "hop-fanout": (3_000, 7)}  # keys, batches


def hopping_case(name, cap=256):
    """test_gpu_parity.test_dense_groups_rounds' specs and generator at a
    twentieth of their windows: batches of 20 000 records and 20 s each, grace
    500 ms; 1 200 keys x ~90 windows (pane mode: 12 windows per record) and
    3 000 keys x ~30 windows (fan-out: 3 or 4 per record), so two or three
    batches fill the table the engine builds for one."""
    spec = OpSpec(abi.HSG_HOPPING, PER_BATCH, grace_ms=500, col_types=[I, F], aggs=HOP_AGGS, state_capacity=cap,
                  **HOPS[name])
    nkeys, nb = HOP_KEYS[name]
    batches = []
    for bi in range(nb):
        key, ts, cols, _valid = gen_small(7000 + bi, 20_000, nkeys, col_types=(I, F), span=20_000,
                                          base=50_000_000 + bi * 20_000, very_late=False, none_frac=0.0,
                                          neg_frac=0.0, absent_frac=0.0)
        batches.append((key, ts, cols, None))
    return Case(spec, batches)


# ---- 4. lean tumbling ------------------------------------------------------------------------------------------
def lean_case(cap=1 << 10, nb=10):
    """test_gpu_lean's uniform batches (sorted ts) on 1 s windows, grace 10 s:
    20 000 records over 1 000 keys and 10 s per batch (inside the grace: lean),
    25 s from batch to batch: ~8 600 groups per batch."""
    spec = OpSpec(abi.HSG_TUMBLING, PER_BATCH, size_ms=1000, grace_ms=10_000, col_types=[I],
                  aggs=datagen.C_AGGS_FULL, state_capacity=cap)
    rng = np.random.default_rng(17)
    batches = []
    for bi in range(nb):
        key, ts, cols = LN._uniform(rng, 20_000, 1_000, 10_000_000 + bi * 25_000, 10_000)
        batches.append((key, ts, cols, None))
    return Case(spec, batches)


# ---- 5. overflow rows and closed windows in one rebuild --------------------------------------------------------
def overflow_case(emit=PER_BATCH, cap=512, nb=4):
    """test_gpu_regions' hot keys: two keys with 5 000 open 1 s windows each
    (more than a 4096-slot region holds) beside 2 000 one-window keys. The
    batch is shuffled over its 5 000 s, so the grace is 5 000 s (none late);
    every batch starts 10 001 s after the one before, so the rebuild ahead of
    batch b + 2, which widens the regions batch b + 1 overflowed, also finds
    batch b's windows closed."""
    size = 1_000
    spec = OpSpec(abi.HSG_TUMBLING, emit, size_ms=size, grace_ms=5_000 * size, col_types=[I], state_capacity=cap,
                  aggs=[(CA, 0), (SUM, 0), (MN, 0), (MX, 0)])
    rng = np.random.default_rng(41)
    batches = []
    for bi in range(nb):
        key, ts, cols = RG._hot_batch(rng, 5_000_000 + bi * 10_001 * size, 2, 5_000, size, 2_000, 2_000)
        batches.append((key, ts, cols, None))
    return Case(spec, batches)


# ---- 6. WHERE + computed columns + HAVING ------------------------------------------------------------------------
FILT_WHERE = M.cmp(">", M.B, M.const(-1.25))
FILT_EXPRS = [M.AC, M.binop("*", M.A, M.B)]  # i64 a*c, f64 a*b
FILT_ALIASES = ["cnt", "s", "mx"]
FILT_HAVING = sql.RCondAnd(H.cmp(">", H.col("cnt"), H.const(1)), H.cmp("<", H.col("mx"), H.const(7.5)))


def filtered_case(emit, cap=256, nb=8, per=4_000):
    """SELECT COUNT(*), SUM(a*c), MAX(a*b) ... WHERE b > -1.25 ... HAVING cnt > 1
    AND mx < 7.5 on 1 s tumbling windows, grace 1 s: test_gpu_map's batches
    (50 keys, 20 s each). The oracle runs the plain op over the host-filtered
    (test_gpu_where.np_keep), host-mapped (test_gpu_map.derive) batch."""
    ospec = OpSpec(abi.HSG_TUMBLING, emit, size_ms=1000, grace_ms=1000, col_types=[I, F],
                   aggs=[(CA, 0), (SUM, 0), (MX, 1)], state_capacity=cap)
    spec = M.mapped_spec(ospec, FILT_EXPRS, where=sql.compile_where(FILT_WHERE, M.NAMES),
                         having=sql.compile_having(FILT_HAVING, FILT_ALIASES))
    batches, obatches = [], []
    for bi in range(nb):
        batch = M.gen(600 + bi, per, nkeys=50, t0=M.TSB + bi * 20_000, span=20_000)
        key, ts, cols, valids = batch
        keep = WH.np_keep(FILT_WHERE, M.NAMES, cols, valids)
        dcols, dval, _errs = M.derive(FILT_EXPRS, batch)
        batches.append(batch)
        obatches.append((np.where(keep, key, NONE).astype(np.uint32), ts, dcols, dval))
    return Case(spec, batches, ospec=ospec, obatches=obatches, having=(FILT_HAVING, FILT_ALIASES))


# ---- 7. the closing boundary (no randomness) -----------------------------------------------------------------------
K0 = 7
BOUNDARY_WINDOWS = {abi.HSG_TUMBLING: (500, 500, 500), abi.HSG_HOPPING: (600, 200, 300)}  # size, advance, grace


@dataclass
class Boundary:
    case: Case
    a_start: int
    a_end: int
    wm1: int           # stream time after batch 1: a_end + grace (A closed) or one less (A open)
    a_closed: bool
    a_batch1: tuple    # (COUNT(*), SUM) of k0's window A after batch 1
    a_both: tuple      # ... had A taken batch 2's record too


def boundary_case(kind, epoch, closed):
    """Key K0, windows A = [T, T + size) and, tumbling, B = [T + size, T + 2 size).
    Batch 1 creates them and ends, with 40 filler keys' records, at stream
    time exactly A.end + grace (closed) or A.end + grace - 1 (open); the
    fillers' windows end after that time. Batch 2 opens with K0's records
    into A and B (hopping: one record whose three windows include A), then
    1 000 more filler keys, enough new groups to make the op rebuild a 64-row
    table before the batch. T = 40 advances (window epoch 0) or the first
    window start past 1 700 000 000 000 ms (size < 792 ms: a non-zero epoch)."""
    size, adv, grace = BOUNDARY_WINDOWS[kind]
    t0 = ((1_700_000_000_000 // adv + 1) if epoch else 40) * adv
    a_end = t0 + size
    wm1 = a_end + grace - (0 if closed else 1)
    if kind == abi.HSG_TUMBLING:
        k1, t1, v1 = [K0, K0], [t0 + 10, t0 + size + 10], [5, 7]
        k2, t2, v2 = [K0, K0], [t0 + 20, t0 + size + 20], [11, 13]
        a1, a2 = (1, 5), (2, 16)
    else:
        k1, t1, v1 = [K0], [t0 + 450], [5]   # windows T, T + 200, T + 400
        k2, t2, v2 = [K0], [t0 + 500], [11]  # the same three
        a1, a2 = (1, 5), (2, 16)
    nf1, nf2 = 40, 1_000
    k1 += list(range(100, 100 + nf1))
    t1 += [wm1] * nf1
    v1 += [i % 9 - 4 for i in range(nf1)]
    k2 += list(range(1_000, 1_000 + nf2))
    t2 += [wm1 + 1 + (i % 8) * adv + i % 3 for i in range(nf2)]
    v2 += [i % 11 - 5 for i in range(nf2)]
    mk = lambda k, t, v: (np.array(k, np.uint32), np.array(t, np.int64), [np.array(v, np.int64)], None)
    kw = dict(size_ms=size) if kind == abi.HSG_TUMBLING else dict(size_ms=size, advance_ms=adv)
    spec = OpSpec(kind, PER_BATCH, grace_ms=grace, col_types=[I], aggs=[(CA, 0), (SUM, 0)], state_capacity=64, **kw)
    return Boundary(Case(spec, [mk(k1, t1, v1), mk(k2, t2, v2)]), t0, a_end, wm1, closed, a1, a2)


# ---- 8. reopen with every slot kind ------------------------------------------------------------------------------------
REOPEN_AT = 6  # the batch pushed at stream time -1


def reopen_mixed_case(cap=256):
    """test_gpu_retention's reopen stream over (i64, f64) columns with the
    `mixed` aggregates (f64 SUM / MIN / MAX / AVG, LAST): six batches of 20 s,
    the first batch's time range again at stream time -1, then ordinary
    batches again. The reopen leaves every row resident in a table built for
    all of them at load 1/2, so the next spill comes only once new groups fill
    that: four batches of 20 000 records over 50 000 keys."""
    spec = OpSpec(abi.HSG_TUMBLING, PER_BATCH, size_ms=1000, grace_ms=1000, col_types=[I, F],
                  aggs=ALL_AGG_SETS["mixed"], state_capacity=cap)
    bs = []
    for b in range(6):
        bs.append(gen_small(41 + b, 10_000, 300, col_types=(I, F), span=20_000, base=5_000_000 + b * 20_000,
                            late_frac=0.01))
    bs.append(gen_small(99, 10_000, 300, col_types=(I, F), span=20_000, base=5_000_000, very_late=False))
    for b in range(6, 10):
        bs.append(gen_small(41 + b, 20_000, 50_000, col_types=(I, F), span=20_000, base=5_000_000 + b * 20_000,
                            late_frac=0.01))
    return Case(spec, bs, wms=[None] * REOPEN_AT + [-1] + [None] * 4)


def reopen_forms_case(cap=256):
    """The same with case 1's i64 op: six batches of its stream, 10 000
    records of the second batch's time range at stream time -1, then five
    batches of 20 000 records over 10 000 keys."""
    b = _sql_batches(7, False, [2_000] + [10_000] * 5, [20] + [2_500] * 5)
    again = _sql_batches(77, False, [10_000], [2_500], first=1)
    more = _sql_batches(7, False, [20_000] * 5, [10_000] * 5, first=6)
    return Case(sql_forms_spec(False, PER_BATCH, cap), b + again + more, wms=[None] * REOPEN_AT + [-1] + [None] * 5,
                forms="sql")


# ---- 9. reset after a spill ------------------------------------------------------------------------------------------------
def reset_rounds(which, cap=256):
    """Three rounds, each a stream of its own that spills, each on lower
    timestamps than the one before (a stale spill watermark or left-over
    spilled rows would show). "forms": case 1's i64 op, 1 000 s lower per
    round; "changes": full_i64 under EMIT CHANGES, 3 000 s lower per round.
    (A reset keeps the table's size, so a round has the batches to fill the
    grown table, not only the first one: "forms" ten of 20 000 records over
    10 000 keys after its small first one, "changes" seven of 8 000.)"""
    rounds = []
    for r in range(3):
        if which == "forms":
            b = _sql_batches(70 + r, False, [2_000] + [20_000] * 10, [20] + [10_000] * 10)
            b = [(k, t - r * 1_000_000, c, v) for k, t, c, v in b]
            rounds.append(Case(sql_forms_spec(False, PER_BATCH, cap), b, forms="sql"))
        else:
            spec = OpSpec(abi.HSG_TUMBLING, CHANGES, size_ms=1000, grace_ms=2000, col_types=[I],
                          aggs=ALL_AGG_SETS["full_i64"], state_capacity=cap)
            b = []
            for bi in range(7):
                key, ts, cols, valid = gen_small(900 + 10 * r + bi, 8_000, 300, span=20_000,
                                                 base=9_000_000 - r * 3_000_000 + bi * 20_000, late_frac=0.01)
                b.append((key, ts, cols[:1], valid[:1]))
            rounds.append(Case(spec, b))
    return rounds


# ---- 10. pending changelog rows across a growth (no randomness) -------------------------------------------------------------
def pending_case(forms, nb=8, per=40):
    """EMIT per batch into the op's own changelog buffer of a 64-row table:
    `nb` batches of 40 records over 16 keys and 3 s of 1 s windows each
    (at most 48 groups, so at most 48 rows, per batch), grace 1 s."""
    spec = OpSpec(abi.HSG_TUMBLING, PER_BATCH, size_ms=1000, grace_ms=1000, col_types=[I], state_capacity=64,
                  aggs=litforms.AGGS if forms else [(CA, 0), (SUM, 0), (MN, 0), (MX, 0)],
                  flags=abi.HSG_OPF_LITERAL_FORMS if forms else 0)
    i = np.arange(per, dtype=np.int64)
    batches = []
    for b in range(nb):
        key = (i % 16).astype(np.uint32)
        ts = 2_000_000 + b * 3_000 + (i * 3_000) // per
        v = (i * 7 + b) % 9 - 4
        valid = ((i + b) % 5 != 0).astype(np.uint8) | ((((i + b) % 3 == 0) & ((i + b) % 5 != 0)).astype(np.uint8) << 1)
        if not forms:
            valid = valid & 1
        batches.append((key, ts, [v.astype(np.int64)], [valid.astype(np.uint8)]))
    return Case(spec, batches, forms="sql" if forms else None)


# every randomised case by the id its GPU test runs it under
RANDOMISED = {
    **{f"sql_forms-{t}-{e}": (lambda f=f, m=m: sql_forms_case(f, m))
       for t, f in (("i64", False), ("f64", True)) for e, m in (("per_batch", PER_BATCH), ("changes", CHANGES))},
    **{f"wide-{e}": (lambda m=m: wide_case(m)) for e, m in (("per_batch", PER_BATCH), ("changes", CHANGES))},
    **{f"hopping-{n}": (lambda n=n: hopping_case(n)) for n in HOPS},
    "lean": lean_case,
    "overflow": overflow_case,
    **{f"filtered-{e}": (lambda m=m: filtered_case(m)) for e, m in (("per_batch", PER_BATCH), ("changes", CHANGES))},
    "reopen-mixed": reopen_mixed_case,
    "reopen-forms": reopen_forms_case,
    **{f"reset-{w}-round{r}": (lambda w=w, r=r: reset_rounds(w)[r]) for w in ("forms", "changes") for r in range(3)},
}
