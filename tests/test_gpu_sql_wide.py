"""GPU: wide SQL GROUP BY on the SQL lean kernels -- 3 to 8 value columns, up
to 24 state slots (k_agg_sql_wide / k_sql_apply, hstream_amd/csrc/hsg_sql.h).

genGroupByNode builds a component set for any SELECT list: any number of
aggregates over any columns and one passthrough (HSG_LAST) per non-aggregate
column. Tumbling and unwindowed ops of that shape, per batch or state only,
run on the LDS fast path at every width the engine has. Here four such
queries run over the data shapes that reach each path of the kernels:

  * uniform: one partial per group, the apply writes the changelog itself;
  * rounds: more groups in a bucket than its LDS table holds, taken in
    key-hash rounds;
  * hot: a key whose bucket is split over aggregation workgroups, its
    partials combined under the rows' locks in any order;
  * record partials: more groups in a chunk than 64 rounds of the table hold
    (E = 512 entries in the 24-slot class: 64 x 448 = 28 672 < the 32 768
    records of a chunk), the records left over each a partial of its own;
  * fallback: a batch with late records runs on the record kernels.

Checked: values, keys, windows and watermarks against pyoracle.OracleOp
(integers bit-exact, f64 within F64_RTOL), dump_state at the end, and the
literal forms against a multi-column restatement of the reference's
sequential fold (test_gpu_sql_shape.py's _prefix_forms, per output over that
output's own column). The path: hsg_stats lean_batches counts every batch on
the SQL lean kernels (0 for these ops without k_agg_sql_wide), replays none.
"""
import numpy as np
import pytest

from hstream_amd import abi
from hstream_amd.columnar import OpSpec
from util import rows_equal

pytestmark = pytest.mark.gpu

SIZE = 60_000
TSB = (1_700_000_000_000 // SIZE + 1) * SIZE  # a window start
GID = 1 << 20  # group id = key * GID + window index
I, F = abi.HSG_I64, abi.HSG_F64
L, S, MN, MX, CA, CN, AV = (abi.HSG_LAST, abi.HSG_SUM, abi.HSG_MIN, abi.HSG_MAX, abi.HSG_COUNT_ALL, abi.HSG_COUNT,
                            abi.HSG_AVG)
FORM = {L: "last", S: "sum", MN: "min", MX: "max"}

QUERIES = {
    # HS352's shape: SELECT key1, key2, key3, SUM(key1) ... GROUP BY key1 (11 slots, 5 packed words)
    "q3": ([I, I, I], [(L, 0), (L, 1), (L, 2), (S, 0)]),
    # ties of both kinds over different columns (11 slots, 6 words)
    "q4": ([I, F, I, F], [(L, 0), (CA, 0), (S, 1), (AV, 1), (MN, 2), (MX, 3)]),
    # the 17 - 24 slot class (22 slots, 7 words)
    "q5big": ([I, F, I, I, F], [(L, 0), (L, 1), (L, 2), (L, 3), (L, 4), (MN, 0), (MX, 1), (S, 2), (CA, 0)]),
    # 8 columns (10 words): column 7's valid and decimal bits are bit 63 of the header / the sequence word
    "q8": ([I, F, I, I, F, I, I, F], [(L, 7), (S, 6), (MN, 5), (MX, 4), (CN, 3), (CA, 0)]),
}


def _columns(rng, n, col_types, absent=0.03, dec=0.3, vr=40):
    """Every column on its own: a narrow value range (ties are common), ~3 %
    absent, ~30 % decimal literals; valid byte: bit 0 present, bit 1 decimal."""
    cols, valids = [], []
    for ct in col_types:
        v = rng.integers(-vr, vr + 1, size=n)
        cols.append(v.astype(np.float64) / 4.0 if ct == F else v.astype(np.int64))
        present = rng.random(n) >= absent
        decimal = present & (rng.random(n) < dec)
        valids.append((present.astype(np.uint8) | (decimal.astype(np.uint8) << 1)).astype(np.uint8))
    return cols, valids


def _batch(seed, n, keys, ts, col_types):
    cols, valids = _columns(np.random.default_rng([seed, n]), n, col_types)
    return keys.astype(np.uint32), ts.astype(np.int64), cols, valids


def _spread_ts(rng, n, start, total, span):
    """Arrival order over `span` ms with 2 s of disorder."""
    i = np.arange(start, start + n, dtype=np.int64)
    return TSB + (i * span) // total + rng.integers(0, 2000, size=n)


def _column_forms(gid, v, valid, f64):
    """Per record, in arrival order: the form bits of a SUM / MIN / MAX / LAST
    over this column in the record's group right after the record (the
    reference's sequential fold; 3 = the aggregate's initial value)."""
    import pandas as pd
    n = len(gid)
    present = (valid & 1) != 0
    dec = (valid & 2) != 0
    idx = np.arange(n)
    hi, lo = (np.inf, -np.inf) if f64 else (np.iinfo(np.int64).max, np.iinfo(np.int64).min)
    df = pd.DataFrame({"g": gid, "i": idx, "p": present, "d": dec & present,
                       "vmin": np.where(present, v, hi), "vmax": np.where(present, v, lo)})
    df = df.sort_values(["g", "i"], kind="stable")
    gb = df.groupby("g", sort=False)
    sum_dec = gb["d"].cumsum().to_numpy()
    run_min = gb["vmin"].cummin()
    prev_min = run_min.groupby(df["g"]).shift(1).fillna(hi).to_numpy()
    run_max = gb["vmax"].cummax()
    prev_max = run_max.groupby(df["g"]).shift(1).fillna(lo).to_numpy()
    p = df["p"].to_numpy()
    i_s = df["i"].to_numpy()
    new_min = p & (df["vmin"].to_numpy() < prev_min)   # min n x = n: a tie keeps the earlier literal
    new_max = p & (df["vmax"].to_numpy() >= prev_max)  # max n x = x: a tie takes the later one
    tmp = pd.DataFrame({"g": df["g"].to_numpy(), "a": np.where(new_min, i_s, -1), "b": np.where(new_max, i_s, -1),
                        "c": np.where(p, i_s, -1)})
    g2 = tmp.groupby("g", sort=False)
    integral = ~dec

    def bits(t):  # the winning literal's "prints as an integer" bit; 3 = the initial value
        return np.where(t < 0, 3, integral[np.maximum(t, 0)].astype(np.int64))

    sorted_bits = {"sum": (sum_dec == 0).astype(np.int64), "min": bits(g2["a"].cummax().to_numpy()),
                   "max": bits(g2["b"].cummax().to_numpy()), "last": bits(g2["c"].cummax().to_numpy())}
    out = {}
    for k, b in sorted_bits.items():
        o = np.empty(n, np.int64)
        o[i_s] = b
        out[k] = o
    return out


def _prefix_forms(gid, cols, valids, col_types, aggs):
    """Literal-form word (hsg_rows.form: 2 bits per output) of each record's
    group right after the record: every output over its own column."""
    per_col = {}
    word = np.zeros(len(gid), np.int64)
    for j, (kind, c) in enumerate(aggs):
        if kind not in FORM:
            continue
        if c not in per_col:
            per_col[c] = _column_forms(gid, cols[c], valids[c], col_types[c] == F)
        word |= per_col[c][FORM[kind]] << (2 * j)
    return word.astype(np.uint32)


def _last_of_groups(gid, lo, hi, keep):
    """(sorted group ids, index of each group's last kept record) of records lo .. hi - 1."""
    sel = np.arange(lo, hi)[keep[lo:hi]]
    gg = gid[sel]
    order = np.argsort(gg, kind="stable")
    sg = gg[order]
    ends = np.r_[np.nonzero(sg[1:] != sg[:-1])[0], len(sg) - 1] if len(sg) else np.zeros(0, np.int64)
    return sg[ends], sel[order[ends]]


def _check_forms(rows, unwindowed, w0, groups, last_idx, fw, what):
    rows = rows.sorted()
    widx = np.zeros(len(rows), np.int64) if unwindowed else rows.win_start // SIZE - w0
    rg = rows.key_id.astype(np.int64) * GID + widx
    pos = np.searchsorted(groups, rg)
    assert len(groups) == len(rg) and np.array_equal(groups[pos], rg), f"{what}: groups"
    np.testing.assert_array_equal(rows.form, fw[last_idx[pos]], err_msg=f"{what}: forms")


def _run(query, batches, emit=abi.HSG_EMIT_PER_BATCH, kind=abi.HSG_TUMBLING, grace_ms=None, dropped=None,
         state_capacity=1 << 20):
    """Push the batches through the engine and the oracle; returns hsg_stats."""
    import pyoracle
    from hstream_amd.engine import Engine
    col_types, aggs = QUERIES[query]
    unwindowed = kind == abi.HSG_UNWINDOWED
    kw = {} if grace_ms is None else {"grace_ms": grace_ms}
    spec = OpSpec(kind, emit, size_ms=0 if unwindowed else SIZE, col_types=col_types, aggs=aggs,
                  flags=abi.HSG_OPF_LITERAL_FORMS, state_capacity=state_capacity, **kw)
    key = np.concatenate([b[0] for b in batches])
    ts = np.concatenate([b[1] for b in batches])
    cols = [np.concatenate([b[2][c] for b in batches]) for c in range(len(col_types))]
    valids = [np.concatenate([b[3][c] for b in batches]) for c in range(len(col_types))]
    w0 = TSB // SIZE
    gid = key.astype(np.int64) * GID + (0 if unwindowed else ts // SIZE - w0)
    keep = np.ones(len(key), bool) if dropped is None else ~dropped
    # (the fold of the records the op accepts: a dropped record reaches no group)
    fw = np.zeros(len(key), np.uint32)
    fw[keep] = _prefix_forms(gid[keep], [c[keep] for c in cols], [v[keep] for v in valids], col_types, aggs)
    eng = Engine(device=0, batch_capacity=max(len(b[0]) for b in batches))
    g = eng.op(spec)
    o = pyoracle.OracleOp(spec)
    f64s = spec.agg_is_f64()
    wg = wo = -1
    base = 0
    for bi, (k, t, c, va) in enumerate(batches):
        wg = g.push(k, t, c, va, watermark=wg)
        wo = o.push(k, t, c, va, watermark=wo)
        assert wg == wo, f"batch {bi}: watermark"
        if emit == abi.HSG_EMIT_PER_BATCH:
            a, b = g.drain(), o.drain()
            rows_equal(a, b, f64s, what=f"batch {bi}")
            # a touched group's row: its state after its last record of the batch
            groups, last_idx = _last_of_groups(gid, base, base + len(k), keep)
            _check_forms(a, unwindowed, w0, groups, last_idx, fw, f"batch {bi}")
        base += len(k)
    a, b = g.dump_state(), o.dump_state()
    rows_equal(a, b, f64s, what="state")
    groups, last_idx = _last_of_groups(gid, 0, len(key), keep)
    if grace_ms is None:  # (a finite grace retires closed windows from the state)
        _check_forms(a, unwindowed, w0, groups, last_idx, fw, "state")
    st = g.stats()
    g.close()
    eng.close()
    return st


def _uniform(query, nb=3, per=60_000, nkeys=2_000, seed=3):
    col_types = QUERIES[query][0]
    rng = np.random.default_rng(seed)
    return [_batch(seed + b, per, rng.integers(0, nkeys, size=per), _spread_ts(rng, per, b * per, nb * per, 3 * SIZE),
                   col_types) for b in range(nb)]


def _one_window_ts(n, start):
    return TSB + (np.arange(start, start + n, dtype=np.int64) >> 6)  # < 2^19 / 64 ms: one window


@pytest.mark.parametrize("emit", [abi.HSG_EMIT_PER_BATCH, abi.HSG_EMIT_NONE], ids=["per_batch", "state_only"])
@pytest.mark.parametrize("query", ["q3", "q4", "q5big", "q8"])
def test_sql_wide_uniform(query, emit):
    """One partial per group: every batch on the lean kernels, none run again."""
    batches = _uniform(query)
    st = _run(query, batches, emit=emit)
    assert st["lean_batches"] == len(batches) and st["replays"] == 0, st
    if emit == abi.HSG_EMIT_PER_BATCH:
        assert st["direct_batches"] == len(batches), st  # the apply wrote the changelog itself


def test_sql_wide_unwindowed():
    batches = _uniform("q3")
    st = _run("q3", batches, kind=abi.HSG_UNWINDOWED)
    assert st["lean_batches"] == len(batches) and st["replays"] == 0, st


@pytest.mark.parametrize("query", ["q3", "q5big"])
def test_sql_wide_rounds(query):
    """A small first batch brings the bucket count down to 16; then 60 000
    groups of one window in 200 000 records: ~3 700 groups per bucket, more
    than an LDS table of 1024 (512) entries takes at 7/8: key-hash rounds."""
    col_types = QUERIES[query][0]
    rng = np.random.default_rng(5)
    sizes, nkeys = [20_000, 200_000, 200_000], [50, 60_000, 60_000]
    batches, start = [], 0
    for b, (n, nk) in enumerate(zip(sizes, nkeys)):
        batches.append(_batch(50 + b, n, rng.integers(0, nk, size=n), _one_window_ts(n, start), col_types))
        start += n
    st = _run(query, batches)
    assert st["lean_batches"] == len(batches) and st["replays"] == 0, st


@pytest.mark.parametrize("query", ["q4", "q5big"])
def test_sql_wide_hot_key(query):
    """One key holds half of each batch: 75 000 records in one bucket, more
    than two chunks of 32 768, so the bucket is split over workgroups and
    their partials meet in k_sql_apply under the row's lock, the LAST pairs
    and tie words in any order; the changelog then comes from the touched
    list (direct_batches < batches)."""
    col_types = QUERIES[query][0]
    rng = np.random.default_rng(7)
    nb, per = 2, 150_000
    batches = []
    for b in range(nb):
        keys = np.where(rng.random(per) < 0.5, 77, rng.integers(100, 2_100, size=per))
        batches.append(_batch(70 + b, per, keys, _spread_ts(rng, per, b * per, nb * per, 3 * SIZE), col_types))
    st = _run(query, batches)
    assert st["lean_batches"] == nb and st["replays"] == 0, st
    assert st["direct_batches"] < nb, st


def test_sql_wide_record_partials():
    """2^19 records with all-distinct keys in one window over 16 buckets: each
    chunk of up to 32 768 records holds that many groups, more than the 64
    key-hash rounds of the 24-slot class's table take (64 x 7/8 x 512 =
    28 672), so records that find no room become partials of their own.
    (state_capacity 2^22: a windowed table keeps a key's windows in blocks of
    8 rows, so the groups of a single window can use an eighth of its rows.)"""
    col_types = QUERIES["q5big"][0]
    rng = np.random.default_rng(9)
    n0, n1 = 20_000, 1 << 19
    batches = [_batch(90, n0, rng.integers(0, 50, size=n0), _one_window_ts(n0, 0), col_types),
               _batch(91, n1, rng.permutation(n1) + 1_000, _one_window_ts(n1, n0), col_types)]
    st = _run("q5big", batches, state_capacity=1 << 22)
    assert st["lean_batches"] == len(batches) and st["replays"] == 0, st
    assert st["direct_batches"] < len(batches), st  # record partials: the changelog from the touched list


def test_sql_wide_late_batch_falls_back():
    """A final batch with late records (their window, the stream's first, closed
    under a 100 s grace once the stream time is 180 s on) does not pass the
    optimistic check: it runs on the record kernels, exact as every other.
    (The check is by batch extrema, stream time <= earliest ts + grace, so
    the 62 s batches before it pass under that grace.)"""
    col_types = QUERIES["q3"][0]
    nb, per = 4, 60_000
    rng = np.random.default_rng(11)
    batches = [_batch(110 + b, per, rng.integers(0, 2_000, size=per),
                      _spread_ts(rng, per, b * per, nb * per, 4 * SIZE), col_types) for b in range(nb)]
    k, t, c, va = batches[-1]
    t = t.copy()
    t[-500:] = TSB + rng.integers(0, 2000, size=500)  # the first window, ~3 windows behind the stream time
    batches[-1] = (k, t, c, va)
    dropped = np.zeros(nb * per, bool)
    dropped[-500:] = True
    st = _run("q3", batches, grace_ms=100_000, dropped=dropped)
    assert st["lean_batches"] == nb - 1, st
