#!/usr/bin/env python3
"""A/B of the stream-table join (hsg_table_join, k_tjoin.hip) against the two
routes to "the table's row for each record of this batch, in arrival order"
that existed before it.

The state is one unwindowed op with C2's aggregate set (COUNT / SUM / AVG /
MIN / MAX) over 2^20 keys, every key present. A probe batch draws its keys
uniformly from twice that range, so half the records hit; sizes 2^16, 2^20 and
2^22 records, plus one Zipf(1.2) draw of 2^20 records (rank r probes key
r - 1, folded into the same range; its hit rate is reported).

  A   GpuOp.table_join_into: device keys, device output columns written in place
  B1  GpuOp.view_get in chunks of HSG_VIEW_MAX_KEYS keys of the batch, and the
      host reorder of each chunk's key-ordered, deduplicated rows back to
      arrival order; timed over the batch's first 64 chunks and scaled to the
      batch (2^16 records are exactly 64 chunks)
  B2  GpuOp.dump_state() into host columns, then a host np.searchsorted join

First A must equal B2 on the whole batch and B1 on the chunks B1 runs, column
by column, bit for bit. Then each is timed over repeats (wall clock of the
Python calls; A ends in the call's own stream synchronise): median, min ..
max, and A's algorithmic bytes -- per record the 4-byte key, one table row
and 8 + 8 bytes of slot scratch, per hit the output row -- with the bytes/s
they imply at A's median. Bytes actually moved are not measured here (that
takes hardware counters).

  python tools/lookup_ab.py [--repeats-a N] [--repeats-b N] [--json PATH]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from hstream_amd import abi, datagen  # noqa: E402
from hstream_amd.columnar import OpSpec, Rows  # noqa: E402
from hstream_amd.engine import Engine  # noqa: E402

KEYS = 1 << 20
SIZES = (1 << 16, 1 << 20, 1 << 22)
B1_CHUNKS = 64


def build_state(eng, torch):
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_NONE, col_types=[abi.HSG_I64], aggs=datagen.C_AGGS_FULL,
                  state_capacity=KEYS)
    g = eng.op(spec)
    gen = torch.Generator(device="cuda").manual_seed(10)
    wm = -1
    for b in range(2):  # every key twice, so the aggregates are not one value
        key = torch.randperm(KEYS, device="cuda", generator=gen).to(torch.int32)
        ts = 5_000_000 + b * KEYS + torch.arange(KEYS, device="cuda", dtype=torch.int64)
        val = torch.randint(-10**9, 10**9, (KEYS,), device="cuda", generator=gen, dtype=torch.int64)
        torch.cuda.synchronize()
        wm = g.push(key, ts, [val], None, watermark=wm)
    return g


def device_rows(torch, cap, f64):
    dk = torch.empty(cap, dtype=torch.int32, device="cuda")
    dws, dwe, dsrc = (torch.empty(cap, dtype=torch.int64, device="cuda") for _ in range(3))
    da = [torch.empty(cap, dtype=torch.float64 if f else torch.int64, device="cuda") for f in f64]
    ap = (C.c_void_p * max(1, len(da)))(*[a.data_ptr() for a in da])
    rows = abi.hsg_rows(capacity=cap, mem=abi.HSG_MEM_DEVICE, n_aggs=len(da), key_id=dk.data_ptr(),
                        win_start=dws.data_ptr(), win_end=dwe.data_ptr(), src_index=dsrc.data_ptr(),
                        aggs=C.cast(ap, C.POINTER(C.c_void_p)))

    def to_host(n):
        torch.cuda.synchronize()
        return Rows(dk[:n].cpu().numpy().view(np.uint32), dws[:n].cpu().numpy(), dwe[:n].cpu().numpy(),
                    dsrc[:n].cpu().numpy(), [a[:n].cpu().numpy() for a in da])

    return rows, to_host, (dk, dws, dwe, dsrc, da, ap)


def host_join(table: Rows, keys, base=0) -> Rows:
    """Rows of `table` (sorted by key, distinct keys) for each of `keys` that
    has one, in the order of `keys`; src_index = base + position."""
    if len(table) == 0:
        at = hit = np.zeros(0, dtype=np.int64)
    else:
        idx = np.minimum(np.searchsorted(table.key_id, keys), len(table) - 1)
        hit = np.flatnonzero(table.key_id[idx] == keys)
        at = idx[hit]
    return Rows(table.key_id[at], table.win_start[at], table.win_end[at], (base + hit).astype(np.int64),
                [a[at] for a in table.aggs])


def b1_chunk(g, keys, base):
    """Route B1 for one chunk: the keyed view read, then back to arrival order."""
    return host_join(g.view_get(keys), keys, base)


def concat(parts) -> Rows:
    return Rows(*[np.concatenate([getattr(p, f) for p in parts]) for f in ("key_id", "win_start", "win_end", "src_index")],
                [np.concatenate([p.aggs[j] for p in parts]) for j in range(len(parts[0].aggs))])


def same_rows(a: Rows, b: Rows):
    if len(a) != len(b):
        return False
    cols = [(a.key_id, b.key_id), (a.src_index, b.src_index), (a.win_start, b.win_start), (a.win_end, b.win_end)]
    cols += list(zip(a.aggs, b.aggs))
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
               for x, y in cols)


def head(rows: Rows, n_src) -> Rows:
    m = rows.src_index < n_src
    return Rows(rows.key_id[m], rows.win_start[m], rows.win_end[m], rows.src_index[m], [a[m] for a in rows.aggs])


def summary(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "n": len(ms)}


def measure(torch, g, name, keys, ra, rb, row_bytes, out_row_bytes):
    n = keys.size
    f64 = g.spec.agg_is_f64()
    dkeys = torch.from_numpy(keys.view(np.int32)).cuda()
    rows, to_host, keep = device_rows(torch, n, f64)
    torch.cuda.synchronize()
    rc, hits = g.table_join_into(dkeys, rows)
    a_rows = to_host(hits)
    # B2, and equality on the whole batch
    dump = g.dump_state()
    if not same_rows(a_rows, host_join(dump, keys)):
        sys.exit(f"lookup_ab: {name}: A and B2 differ")
    # B1 on the first chunks, and equality there
    chunk = abi.HSG_VIEW_MAX_KEYS
    nch = min(B1_CHUNKS, n // chunk)
    b1 = concat([b1_chunk(g, keys[c * chunk:(c + 1) * chunk], c * chunk) for c in range(nch)])
    if not same_rows(head(a_rows, nch * chunk), b1):
        sys.exit(f"lookup_ab: {name}: A and B1 differ")
    a_ms, b1_ms, b2_ms = [], [], []
    for _ in range(ra):
        t0 = time.perf_counter()
        g.table_join_into(dkeys, rows)
        a_ms.append((time.perf_counter() - t0) * 1e3)
    scale = (n / chunk) / nch
    for _ in range(rb):
        t0 = time.perf_counter()
        for c in range(nch):
            b1_chunk(g, keys[c * chunk:(c + 1) * chunk], c * chunk)
        b1_ms.append((time.perf_counter() - t0) * 1e3 * scale)
        t0 = time.perf_counter()
        host_join(g.dump_state(), keys)
        b2_ms.append((time.perf_counter() - t0) * 1e3)
    a, b1s, b2s = summary(a_ms), summary(b1_ms), summary(b2_ms)
    alg = n * (4 + row_bytes + 16) + hits * out_row_bytes
    res = {"records": int(n), "hits": int(hits), "hit_rate": hits / n, "A": a, "B1": b1s, "B2": b2s,
           "B1_chunks_timed": nch, "B1_scale": scale, "B1_over_A": b1s["median_ms"] / a["median_ms"],
           "B2_over_A": b2s["median_ms"] / a["median_ms"], "A_algorithmic_bytes": int(alg),
           "A_algorithmic_GBps": alg / (a["median_ms"] * 1e-3) / 1e9,
           "A_records_per_s": n / (a["median_ms"] * 1e-3)}
    print(f"{name:12s} {n:8d} rec {hits:8d} hits  A {a['median_ms']:8.3f} ms ({a['min_ms']:.3f} .. {a['max_ms']:.3f})"
          f"  B1 {b1s['median_ms']:10.1f} ms ({b1s['min_ms']:.1f} .. {b1s['max_ms']:.1f})"
          f"  B2 {b2s['median_ms']:9.1f} ms ({b2s['min_ms']:.1f} .. {b2s['max_ms']:.1f})"
          f"  A {alg / 1e6:.1f} MB, {res['A_algorithmic_GBps']:.1f} GB/s", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats-a", type=int, default=30)
    ap.add_argument("--repeats-b", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("lookup_ab: no GPU (nothing is measured without one)")
    eng = Engine(device=0, batch_capacity=max(SIZES))
    g = build_state(eng, torch)
    st = g.stats()
    slots = int(st["state_slots"])
    w, stride = 2 + slots, 4
    while stride < w and stride < 16:
        stride <<= 1
    row_bytes = (stride if stride >= w else (w + 7) & ~7) * 8
    out_row_bytes = 4 + 3 * 8 + 8 * len(g.spec.aggs)
    res = {"state_rows": int(st["state_rows"]), "table_slots": int(st["table_slots"]), "row_bytes": row_bytes,
           "out_row_bytes": out_row_bytes, "probes": {}}
    assert res["state_rows"] == KEYS
    rng = np.random.default_rng(11)
    for n in SIZES:
        keys = rng.integers(0, 2 * KEYS, n).astype(np.uint32)
        res["probes"][f"uniform_{n}"] = measure(torch, g, "uniform", keys, a.repeats_a, a.repeats_b, row_bytes,
                                                out_row_bytes)
    zipf = ((rng.zipf(1.2, 1 << 20) - 1) % (2 * KEYS)).astype(np.uint32)
    res["probes"]["zipf1.2_1048576"] = measure(torch, g, "zipf(1.2)", zipf, a.repeats_a, a.repeats_b, row_bytes,
                                               out_row_bytes)
    g.close()
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
