#!/usr/bin/env python3
"""A/B of computed columns (hsg_op_create_mapped, k_map.hip): what evaluating
the SELECT list's expressions costs on the device, against the aggregation
alone and against what such a query needed before -- the expressions in numpy
on the host and the computed columns uploaded.

One query, tumbling 60 s, per-batch changelog, device-resident batches:

  SELECT COUNT(*), SUM(c0 * c1), MAX(c0 - c2)      c0 i64, c1 f64, c2 i64

Three ways over the same seeded batches (2^22 records, 65 536 keys by
default) in one process:

  A  the plain two-column op, fed the host-computed columns already on the device
  B  the mapped op on the three raw columns
  C  A, plus numpy on the host and the upload of the two computed columns
     (values and valid bytes), the upload timed to a device synchronise

First all three must drain equal rows (integers bit-exact, the f64 SUM
within 1e-6 relative: the orders of summation differ between kernels, not
between ways); then ops of each kind alternate over the batches and the wall
time of a push (hsg_stats last_batch_ms; C: plus the host work) is reported:
the median over the timed batches of every repeat, and the spread (min ..
max) of the repeats' medians. An op's first batch is not timed. B - A is the
map pass; its algorithmic bytes are

  N * (8 * [keys written] + 9 * named inputs + (8 + [valid written]) * computed outputs)

here N * (0 + 9 * 3 + 9 * 2): no expression is strict and there is no WHERE,
so no key is written; every input has a valid array, so both outputs get one.

  python tools/map_ab.py [--records N] [--keys K] [--batches B] [--repeats R] [--plain-only] [--json PATH]

--plain-only times way A alone (for a comparison of the plain path between two
trees: it uses nothing a tree without the map lacks).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from hstream_amd import abi  # noqa: E402
from hstream_amd.columnar import OpSpec  # noqa: E402
from hstream_amd.engine import Engine  # noqa: E402

I, F = abi.HSG_I64, abi.HSG_F64
AGGS = [(abi.HSG_COUNT_ALL, 0), (abi.HSG_SUM, 0), (abi.HSG_MAX, 1)]
TS0 = 1_700_000_040_000
PEAK_BYTES_PER_S = 8e12         # the HBM bandwidth the project's rooflines use
W = abi
MAP = [[(W.HSG_W_COL, 0), (W.HSG_W_COL, 1), (W.HSG_W_MUL,)], [(W.HSG_W_COL, 0), (W.HSG_W_COL, 2), (W.HSG_W_SUB,)]]


def map_bytes(n, keys_written, named_inputs, computed, valid_written):
    """The pass's algorithmic bytes (csrc/k_map.hip)."""
    return n * (8 * int(keys_written) + 9 * named_inputs + (8 + int(valid_written)) * computed)


def host_columns(cols, valids):
    """What the host did for such a query before: the expressions over the
    batch's columns, absent where an input is."""
    c0, c1, c2 = cols
    p0, p1, p2 = [(v & 1) != 0 for v in valids]
    return ([c0.astype(np.float64) * c1, c0 - c2],
            [(p0 & p1).astype(np.uint8), (p0 & p2).astype(np.uint8)])


def gen_batches(seed, nb, n, nkeys):
    out = []
    total = nb * n
    for b in range(nb):
        rng = np.random.default_rng([seed, b])
        key = rng.integers(0, nkeys, size=n).astype(np.uint32)
        i = np.arange(b * n, (b + 1) * n, dtype=np.int64)
        ts = (TS0 + (i * 150_000) // total + rng.integers(0, 2000, size=n)).astype(np.int64)
        cols = [rng.integers(-1000, 1001, size=n).astype(np.int64),
                rng.integers(-100, 101, size=n).astype(np.float64) / 4.0,
                rng.integers(-1000, 1001, size=n).astype(np.int64)]
        valids = [(rng.random(n) >= 0.03).astype(np.uint8) for _ in cols]
        out.append((key, ts, cols, valids))
    return out


def to_device(torch, arrays):
    dev = torch.device("cuda:0")
    return [torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to(dev) for x in arrays]


def run(torch, eng, way, host, dev, derived_dev, keep_rows):
    """Per-batch ms of one op over the batches, the drained rows (sorted) when asked, the stats."""
    spec = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=60_000, col_types=[F, I], aggs=AGGS,
                  state_capacity=1 << 20)
    if way == "B":
        spec = OpSpec(**{**spec.__dict__, "col_types": [I, F, I], "map": MAP})
    g = eng.op(spec)
    ms, rows = [], []
    wm = -1
    for b, (key, ts, cols, valids) in enumerate(dev):
        extra = 0.0
        if way == "B":
            wm = g.push(key, ts, cols, valids, watermark=wm)
        else:
            dc, dv = derived_dev[b]
            if way == "C":
                t0 = time.perf_counter()
                hc, hv = host_columns(host[b][2], host[b][3])
                dc, dv = to_device(torch, hc), to_device(torch, hv)
                torch.cuda.synchronize()
                extra = (time.perf_counter() - t0) * 1e3
            wm = g.push(key, ts, dc, dv, watermark=wm)
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
    exact = [(a.key_id, b.key_id), (a.win_start, b.win_start), (a.win_end, b.win_end), (a.aggs[0], b.aggs[0]),
             (a.aggs[2], b.aggs[2])]
    return all(np.array_equal(x, y) for x, y in exact) and np.allclose(a.aggs[1], b.aggs[1], rtol=1e-6, atol=0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 22)
    ap.add_argument("--keys", type=int, default=65536)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("map_ab: no GPU (nothing is measured without one)")
    eng = Engine(device=0, batch_capacity=a.records)
    host = gen_batches(a.seed, a.batches, a.records, a.keys)
    dev = []
    for key, ts, cols, valids in host:
        k, t = to_device(torch, [key, ts])
        dev.append((k, t, to_device(torch, cols), to_device(torch, valids)))
    derived_dev = []
    for _, _, cols, valids in host:
        hc, hv = host_columns(cols, valids)
        derived_dev.append((to_device(torch, hc), to_device(torch, hv)))
    torch.cuda.synchronize()
    ways = ("A",) if a.plain_only else ("A", "B", "C")
    first = {w: run(torch, eng, w, host, dev, derived_dev, True) for w in ways}
    same = all(all(same_rows(x, y) for y in rest) for x, *rest in zip(*[first[w][1] for w in ways]))
    lean = {w: first[w][2]["lean_batches"] for w in ways}
    if not same:
        print(json.dumps({"equal_rows": same}))
        sys.exit("map_ab: the three ways differ")
    med = {w: [] for w in ways}
    for _ in range(a.repeats):
        for w in ways:
            ms, _, _ = run(torch, eng, w, host, dev, derived_dev, False)
            med[w].append(float(np.median(ms[1:])))
    eng.close()
    res = {"records": a.records, "keys": a.keys, "batches": a.batches, "repeats": a.repeats, "equal_rows": same,
           "lean_batches": lean, "ways": {}}
    for w in ways:
        res["ways"][w] = {"median_ms": float(np.median(med[w])), "min_ms": min(med[w]), "max_ms": max(med[w])}
        q = res["ways"][w]
        print(f"{w}: {q['median_ms']:.3f} ms ({q['min_ms']:.3f} .. {q['max_ms']:.3f}) per batch of {a.records} records")
    if not a.plain_only:
        fa, fb, fc = (res["ways"][w]["median_ms"] for w in ways)
        nbytes = map_bytes(a.records, keys_written=False, named_inputs=3, computed=2, valid_written=True)
        res["map_ms"] = fb - fa
        res["map_bytes"] = nbytes
        res["map_bytes_per_s"] = nbytes / ((fb - fa) * 1e-3) if fb > fa else None
        res["map_share_of_peak"] = res["map_bytes_per_s"] / PEAK_BYTES_PER_S if fb > fa else None
        res["c_over_b"] = fc / fb
        if fb > fa:
            print(f"B - A = {fb - fa:.3f} ms for {nbytes} bytes: {res['map_bytes_per_s'] / 1e12:.2f} TB/s, "
                  f"{100 * res['map_share_of_peak']:.1f} % of 8 TB/s;  C / B = {fc / fb:.1f}")
        else:
            print(f"B - A = {fb - fa:.3f} ms: within the spread, no bandwidth figure;  C / B = {fc / fb:.1f}")
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
