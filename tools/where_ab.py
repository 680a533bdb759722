#!/usr/bin/env python3
"""A/B of WHERE pushdown (hsg_op_create_where, k_where.hip): what the filter
costs on the device, against the aggregation alone and against what a
filtered query needed before -- the predicate on the host and the masked key
column uploaded.

One query, tumbling 60 s, per-batch changelog, device-resident batches:

  SELECT COUNT(*), SUM(c0), MIN(c0), MAX(c0) ... WHERE c0 > k AND c1 BETWEEN a AND b

with k, a, b chosen so that about half of the records are kept (c1 is a
column of the filter alone). Three ways over the same seeded batches
(2^22 records, 65 536 keys by default) in one process:

  A  no program, keys masked in advance: the aggregation alone
  B  the op's program on the raw keys
  C  A, plus the numpy mask on the host and the upload of the masked keys

First all three must drain identical rows; then ops of either kind alternate
over the batches and the wall time of a push (hsg_stats last_batch_ms; C: plus
the mask and the upload, the upload timed to a device synchronise) is
reported: the median over the timed batches of every repeat, and the spread
(min .. max) of the repeats' medians. An op's first batch (no window epoch,
no group count to size the buckets by) is not timed. B - A is the filter; its
bytes are N * (8 + 9 * 2): the key in and out, a value and a valid byte for
each of the two columns the program names.

  python tools/where_ab.py [--records N] [--keys K] [--batches B] [--repeats R] [--json PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from hstream_amd import abi, sql  # noqa: E402
from hstream_amd.columnar import OpSpec  # noqa: E402
from hstream_amd.engine import Engine  # noqa: E402

I, F = abi.HSG_I64, abi.HSG_F64
AGGS = [(abi.HSG_COUNT_ALL, 0), (abi.HSG_SUM, 0), (abi.HSG_MIN, 0), (abi.HSG_MAX, 0)]
TS0 = 1_700_000_040_000
K, LO, HI = -400, -17.5, 17.5   # c0 uniform in -1000 .. 1000, c1 in -25 .. 25 by 1/4: 0.70 * 0.70 of the present
NONE = np.uint32(abi.HSG_KEY_NONE)
PEAK_BYTES_PER_S = 8e12         # the HBM bandwidth the project's rooflines use


def col(f):
    return sql.RExprCol(f, None, f)


def const(c):
    return sql.RExprConst(str(c), c)


COND = sql.RCondAnd(sql.RCondOp("RCompOpGT", col("c0"), const(K)),
                    sql.RCondBetween(const(LO), col("c1"), const(HI)))


def host_mask(key, cols, valids):
    """What the host did for such a query before: the predicate over the
    batch's columns (a missing field drops the record), keys masked."""
    keep = ((valids[0] & 1) != 0) & (cols[0] > K) & ((valids[1] & 1) != 0) & (cols[1] >= LO) & (cols[1] <= HI)
    return np.where(keep, key, NONE).astype(np.uint32)


def gen_batches(seed, nb, n, nkeys):
    out = []
    total = nb * n
    for b in range(nb):
        rng = np.random.default_rng([seed, b])
        key = rng.integers(0, nkeys, size=n).astype(np.uint32)
        i = np.arange(b * n, (b + 1) * n, dtype=np.int64)
        ts = (TS0 + (i * 150_000) // total + rng.integers(0, 2000, size=n)).astype(np.int64)
        cols = [rng.integers(-1000, 1001, size=n).astype(np.int64),
                rng.integers(-100, 101, size=n).astype(np.float64) / 4.0]
        valids = [(rng.random(n) >= 0.03).astype(np.uint8) for _ in cols]
        out.append((key, ts, cols, valids))
    return out


def to_device(torch, batches):
    dev = torch.device("cuda:0")
    out = []
    for key, ts, cols, valids in batches:
        out.append((torch.from_numpy(key.view(np.int32)).to(dev), torch.from_numpy(ts).to(dev),
                    [torch.from_numpy(c).to(dev) for c in cols], [torch.from_numpy(v).to(dev) for v in valids]))
    torch.cuda.synchronize()
    return out


def run(torch, eng, way, host, dev, masked_dev, keep_rows):
    """Per-batch ms of one op over the batches, the drained rows (sorted) when asked, the stats."""
    spec = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=60_000, col_types=[I], aggs=AGGS,
                  state_capacity=1 << 20)
    if way == "B":
        spec = OpSpec(**{**spec.__dict__, "col_types": [I, F], "where": sql.compile_where(COND, ["c0", "c1"])})
    g = eng.op(spec)
    ms, rows = [], []
    wm = -1
    for b, (key, ts, cols, valids) in enumerate(dev):
        extra = 0.0
        if way == "B":
            wm = g.push(key, ts, cols, valids, watermark=wm)
        else:
            mk = masked_dev[b]
            if way == "C":
                t0 = time.perf_counter()
                m = host_mask(*[host[b][j] for j in (0, 2, 3)])
                mk = torch.from_numpy(m.view(np.int32)).to(key.device)
                torch.cuda.synchronize()
                extra = (time.perf_counter() - t0) * 1e3
            wm = g.push(mk, ts, cols[:1], valids[:1], watermark=wm)
        ms.append(g.stats()["last_batch_ms"] + extra)
        r = g.drain()
        if keep_rows:
            rows.append(r.sorted())
    st = g.stats()
    g.close()
    return ms, rows, st


def same_rows(a, b):
    if len(a) != len(b):
        return False
    cols = [(a.key_id, b.key_id), (a.win_start, b.win_start), (a.win_end, b.win_end)] + list(zip(a.aggs, b.aggs))
    return all(np.array_equal(x, y) for x, y in cols)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 22)
    ap.add_argument("--keys", type=int, default=65536)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("where_ab: no GPU (nothing is measured without one)")
    eng = Engine(device=0, batch_capacity=a.records)
    host = gen_batches(a.seed, a.batches, a.records, a.keys)
    dev = to_device(torch, host)
    masked = [host_mask(k, c, v) for k, _, c, v in host]
    masked_dev = [torch.from_numpy(m.view(np.int32)).to(dev[0][0].device) for m in masked]
    torch.cuda.synchronize()
    kept = float(np.mean([np.count_nonzero(m != NONE) / len(m) for m in masked]))
    ways = ("A", "B", "C")
    # all three drain identical rows (also the warm-up of each)
    first = {w: run(torch, eng, w, host, dev, masked_dev, True) for w in ways}
    same = all(same_rows(x, y) and same_rows(x, z) for x, y, z in zip(*[first[w][1] for w in ways]))
    dropped = first["B"][2]["where_dropped_total"]
    want = int(sum(np.count_nonzero((k != NONE) & (m == NONE)) for (k, _, _, _), m in zip(host, masked)))
    lean = {w: first[w][2]["lean_batches"] for w in ways}
    if not same or dropped != want:
        print(json.dumps({"identical_rows": same, "where_dropped_total": dropped, "host_count": want}))
        sys.exit(f"where_ab: the three ways differ (rows identical: {same}, dropped {dropped}, host count {want})")
    med = {w: [] for w in ways}
    for _ in range(a.repeats):
        for w in ways:
            ms, _, _ = run(torch, eng, w, host, dev, masked_dev, False)
            med[w].append(float(np.median(ms[1:])))
    eng.close()
    res = {"records": a.records, "keys": a.keys, "batches": a.batches, "repeats": a.repeats, "kept_fraction": kept,
           "identical_rows": same, "lean_batches": lean, "ways": {}}
    for w in ways:
        res["ways"][w] = {"median_ms": float(np.median(med[w])), "min_ms": min(med[w]), "max_ms": max(med[w])}
    fa, fb, fc = (res["ways"][w]["median_ms"] for w in ways)
    nbytes = a.records * (8 + 9 * 2)
    res["filter_ms"] = fb - fa
    res["filter_bytes"] = nbytes
    res["filter_bytes_per_s"] = nbytes / ((fb - fa) * 1e-3) if fb > fa else None
    res["filter_share_of_peak"] = res["filter_bytes_per_s"] / PEAK_BYTES_PER_S if fb > fa else None
    for w in ways:
        q = res["ways"][w]
        print(f"{w}: {q['median_ms']:.3f} ms ({q['min_ms']:.3f} .. {q['max_ms']:.3f}) per batch of {a.records} records")
    if fb > fa:
        print(f"B - A = {fb - fa:.3f} ms for {nbytes} bytes: {res['filter_bytes_per_s'] / 1e12:.2f} TB/s, "
              f"{100 * res['filter_share_of_peak']:.1f} % of 8 TB/s;  C - B = {fc - fb:.3f} ms;  kept {kept:.3f}")
    else:
        print(f"B - A = {fb - fa:.3f} ms: within the spread, no bandwidth figure;  C - B = {fc - fb:.3f} ms")
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
