#!/usr/bin/env python3
"""A/B of the wide SQL GROUP BY path: k_agg_sql_wide / k_sql_apply against
the record kernels (k_tw_agg and its LAST / tie resolution pass) that the
same ops ran on before, selected per op with HSG_SQL_WIDE_OFF (read when the
op is created).

Two queries in the SQL drop-in's shape (literal forms, a passthrough per
non-aggregate column), tumbling 60 s, per-batch changelog:

  q3     SELECT c0, c1, c2, SUM(c0)             3 columns, 11 slots
  q5big  SELECT c0 .. c4, MIN(c0), MAX(c1),
                SUM(c2), COUNT(*)               5 columns, 22 slots

over the same seeded batches (2^22 records, 65 536 keys by default) in one
process. First both paths must drain identical rows; then ops of either kind
alternate over the batches and the device time per batch that the engine
measures (hsg_stats agg_kernel_ms: aggregation + changelog rows, no copies)
is reported: the median over the timed batches of every repeat, and the
spread (min .. max) of the repeats' medians. An op's first batch (no window
epoch, no group count to size the buckets by) is not timed.

  python tools/sql_wide_ab.py [--records N] [--keys K] [--batches B] [--repeats R] [--json PATH]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from hstream_amd import abi  # noqa: E402
from hstream_amd.columnar import OpSpec  # noqa: E402
from hstream_amd.engine import Engine  # noqa: E402

I, F = abi.HSG_I64, abi.HSG_F64
QUERIES = {
    "q3": ([I, I, I], [(abi.HSG_LAST, 0), (abi.HSG_LAST, 1), (abi.HSG_LAST, 2), (abi.HSG_SUM, 0)]),
    "q5big": ([I, F, I, I, F], [(abi.HSG_LAST, 0), (abi.HSG_LAST, 1), (abi.HSG_LAST, 2), (abi.HSG_LAST, 3),
                                (abi.HSG_LAST, 4), (abi.HSG_MIN, 0), (abi.HSG_MAX, 1), (abi.HSG_SUM, 2),
                                (abi.HSG_COUNT_ALL, 0)]),
}
TS0 = 1_700_000_040_000
OFF = "HSG_SQL_WIDE_OFF"


def gen_batches(seed, nb, n, nkeys, col_types):
    out = []
    total = nb * n
    for b in range(nb):
        rng = np.random.default_rng([seed, b])
        key = rng.integers(0, nkeys, size=n).astype(np.uint32)
        i = np.arange(b * n, (b + 1) * n, dtype=np.int64)
        ts = (TS0 + (i * 150_000) // total + rng.integers(0, 2000, size=n)).astype(np.int64)
        cols, valids = [], []
        for ct in col_types:
            v = rng.integers(-40, 41, size=n)
            cols.append(v.astype(np.float64) / 4.0 if ct == F else v.astype(np.int64))
            present = rng.random(n) >= 0.03
            decimal = present & (rng.random(n) < 0.3)
            valids.append((present.astype(np.uint8) | (decimal.astype(np.uint8) << 1)).astype(np.uint8))
        out.append((key, ts, cols, valids))
    return out


def make_op(eng, spec, wide):
    if wide:
        os.environ.pop(OFF, None)
    else:
        os.environ[OFF] = "1"
    try:
        return eng.op(spec)
    finally:
        os.environ.pop(OFF, None)


def run(eng, spec, batches, wide, keep_rows):
    """Per-batch device ms, the drained rows (sorted) when asked, the stats."""
    g = make_op(eng, spec, wide)
    ms, rows = [], []
    wm = -1
    for k, t, c, va in batches:
        before = g.stats()["agg_kernel_ms"]
        wm = g.push(k, t, c, va, watermark=wm)
        r = g.drain()
        ms.append(g.stats()["agg_kernel_ms"] - before)
        if keep_rows:
            rows.append(r.sorted())
    st = g.stats()
    g.close()
    return ms, rows, st


def same_rows(a, b):
    if len(a) != len(b):
        return False
    cols = [(a.key_id, b.key_id), (a.win_start, b.win_start), (a.win_end, b.win_end), (a.form, b.form)]
    cols += list(zip(a.aggs, b.aggs))
    return all(np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")) for x, y in cols)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 22)
    ap.add_argument("--keys", type=int, default=65536)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    eng = Engine(device=0, batch_capacity=a.records)
    result = {"records": a.records, "keys": a.keys, "batches": a.batches, "repeats": a.repeats, "queries": {}}
    for name, (col_types, aggs) in QUERIES.items():
        spec = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=60_000, col_types=col_types, aggs=aggs,
                      flags=abi.HSG_OPF_LITERAL_FORMS, state_capacity=1 << 20)
        batches = gen_batches(a.seed, a.batches, a.records, a.keys, col_types)
        # both paths drain identical rows (also the warm-up of either)
        _, rw, sw = run(eng, spec, batches, True, True)
        _, ro, so = run(eng, spec, batches, False, True)
        same = all(same_rows(x, y) for x, y in zip(rw, ro))
        lean = (sw["lean_batches"], so["lean_batches"])
        if not same or lean != (a.batches, 0):
            print(json.dumps({"query": name, "identical_rows": same, "lean_batches": lean}))
            sys.exit(f"{name}: the two paths differ (rows identical: {same}, lean batches wide / off: {lean})")
        med = {True: [], False: []}
        for _ in range(a.repeats):
            for wide in (True, False):
                ms, _, _ = run(eng, spec, batches, wide, False)
                med[wide].append(float(np.median(ms[1:])))
        q = {}
        for wide, label in ((True, "wide"), (False, "off")):
            m = med[wide]
            q[label] = {"median_ms": float(np.median(m)), "min_ms": min(m), "max_ms": max(m)}
        q["rows_per_batch"] = int(np.mean([len(r) for r in rw]))
        result["queries"][name] = q
        print(f"{name}: wide {q['wide']['median_ms']:.3f} ms ({q['wide']['min_ms']:.3f} .. {q['wide']['max_ms']:.3f})"
              f"  off {q['off']['median_ms']:.3f} ms ({q['off']['min_ms']:.3f} .. {q['off']['max_ms']:.3f})"
              f"  per batch of {a.records} records, {q['rows_per_batch']} rows")
    eng.close()
    line = json.dumps(result)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
