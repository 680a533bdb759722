#!/usr/bin/env python3
"""A/B of the keyed view read (hsg_view_get, k_view.hip) against what a keyed
read cost before it: a dump of the whole state and a filter on the host.

Two states, one op each:

  tw    C2's state shape: tumbling 60 s over one hour, 65 536 keys, COUNT / SUM /
        AVG / MIN / MAX, ~60 windows per key (3.9 M rows)
  sess  sessions, gap 30 s, at C4's per-key density (50 records per key over
        the hour, ~33 sessions each) over 200 000 keys

On each, for 1, 64 and 1024 keys drawn from the state's keys:

  A  GpuOp.view_get(keys)                      (hsg_view_get into host columns)
  B  GpuOp.dump_state(), then np.isin(key_id, keys) and the take of every column
     (hsg_dump_state into host columns: what ksGet over ksDump did)

First A and B must return equal rows, position by position. Then each is
timed over repeats (wall clock of the Python call; B's dump, which does not
depend on the keys, is timed once per repeat and the filter per key count):
median and min .. max, their ratio, and A's algorithmic bytes -- time windows:
distinct key-hash regions x region bytes + the overflow rows' bytes, which
both passes read; sessions: a 64-byte key entry per key + the rows -- with the
bandwidth they imply at A's median. Bytes actually read are not measured here
(that takes hardware counters).

  python tools/view_ab.py [--state tw|sess|both] [--repeats-a N] [--repeats-b N] [--json PATH]
"""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from hstream_amd import abi, datagen  # noqa: E402
from hstream_amd.columnar import Rows  # noqa: E402
from hstream_amd.engine import Engine  # noqa: E402

KEY_COUNTS = (1, 64, 1024)


def fmix32(h):
    h = h.astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h


def regions_touched(keys, rbits):
    """Distinct table regions of the keys: the top rbits of the key hash
    (hsg_internal.h key_hash / tw_region_base, single GPU: no owner bits)."""
    if rbits <= 0:
        return 1
    k = np.asarray(keys, dtype=np.uint64)
    h = fmix32((k * np.uint64(0x9E3779B1) + np.uint64(0x632BE59B)) & np.uint64(0xFFFFFFFF))
    return int(np.unique(h >> np.uint64(32 - rbits)).size)


def build_tw(eng, torch):
    cfg = dataclasses.replace(datagen.CONFIGS["C2"], n=1 << 25, batch=1 << 23)
    g = eng.op(cfg.spec(abi.HSG_EMIT_NONE))
    wm = -1
    for s in range(0, cfg.n, cfg.batch):
        d = datagen.generate_torch(cfg, cfg.batch, start=s, total=cfg.n)
        torch.cuda.synchronize()
        wm = g.push(d["key_id"], d["ts"], d["cols"], None, watermark=wm)
    return g


def build_sess(eng, torch):
    c4 = datagen.CONFIGS["C4"]
    keys = 200_000
    per_key = c4.n // c4.keys  # 50 records per key over the hour
    cfg = dataclasses.replace(c4, keys=keys, n=keys * per_key, batch=1 << 21)
    g = eng.op(cfg.spec(abi.HSG_EMIT_NONE))
    wm = -1
    for s in range(0, cfg.n, cfg.batch):
        n = min(cfg.batch, cfg.n - s)
        d = datagen.generate_torch(cfg, n, start=s, total=cfg.n)
        torch.cuda.synchronize()
        wm = g.push(d["key_id"], d["ts"], d["cols"], None, watermark=wm)
    return g


def take(rows, mask):
    return Rows(rows.key_id[mask], rows.win_start[mask], rows.win_end[mask], rows.src_index[mask],
                [a[mask] for a in rows.aggs])


def same_rows(a, b):
    if len(a) != len(b):
        return False
    cols = [(a.key_id, b.key_id), (a.win_start, b.win_start), (a.win_end, b.win_end)] + list(zip(a.aggs, b.aggs))
    return all(np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in cols)


def summary(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "n": len(ms)}


def measure(name, g, session, ra, rb):
    st = g.stats()
    full = g.dump_state()  # (also B's warm-up)
    present = np.unique(full.key_id)
    rng = np.random.default_rng(9)
    sets = {nk: present[rng.permutation(present.size)[:nk]].astype(np.uint32) for nk in KEY_COUNTS}
    # A and B return equal rows, in the same order
    for nk, keys in sets.items():
        a, b = g.view_get(keys), take(full, np.isin(full.key_id, keys))
        if not same_rows(a, b):
            sys.exit(f"view_ab: {name}, {nk} keys: A and B differ ({len(a)} vs {len(b)} rows)")
    slots = int(st["state_slots"])
    if session:
        row_bytes = (3 + slots) * 8
    else:
        w, stride = 2 + slots, 4
        while stride < w and stride < 16:
            stride <<= 1
        row_bytes = (stride if stride >= w else (w + 7) & ~7) * 8
    cap = int(st["table_slots"])
    region_log2 = 12 + int(st["overflow_rebuilds"])
    rbits = max(0, min(11, cap.bit_length() - 1 - region_log2))
    res = {"state_rows": int(st["state_rows"]), "table_slots": cap, "row_bytes": row_bytes, "keys": {}}
    dump_ms, isin_ms, a_ms = [], {nk: [] for nk in KEY_COUNTS}, {nk: [] for nk in KEY_COUNTS}
    for _ in range(rb):
        t0 = time.perf_counter()
        full = g.dump_state()
        dump_ms.append((time.perf_counter() - t0) * 1e3)
        for nk, keys in sets.items():
            t0 = time.perf_counter()
            b = take(full, np.isin(full.key_id, keys))
            isin_ms[nk].append((time.perf_counter() - t0) * 1e3)
    for nk, keys in sets.items():
        n_rows = len(g.view_get(keys))
        for _ in range(ra):
            t0 = time.perf_counter()
            g.view_get(keys, capacity=n_rows)
            a_ms[nk].append((time.perf_counter() - t0) * 1e3)
    for nk, keys in sets.items():
        n_rows = len(g.view_get(keys))
        if session:
            alg = nk * 64 + n_rows * row_bytes
        else:
            nreg = regions_touched(keys, rbits)
            alg = (nreg * (cap >> rbits) + max(cap // 8, 64)) * row_bytes
        a = summary(a_ms[nk])
        b = summary([d + f for d, f in zip(dump_ms, isin_ms[nk])])
        res["keys"][nk] = {"rows": n_rows, "A": a, "B": b, "B_over_A": b["median_ms"] / a["median_ms"],
                           "A_algorithmic_bytes": int(alg),
                           "A_algorithmic_GBps": alg / (a["median_ms"] * 1e-3) / 1e9}
        if not session:
            res["keys"][nk]["regions_touched"] = nreg
            res["keys"][nk]["table_bytes"] = (cap + max(cap // 8, 64)) * row_bytes
        print(f"{name} {nk:5d} keys {n_rows:6d} rows  A {a['median_ms']:9.3f} ms ({a['min_ms']:.3f} .. {a['max_ms']:.3f})"
              f"  B {b['median_ms']:10.1f} ms ({b['min_ms']:.1f} .. {b['max_ms']:.1f})  B/A {b['median_ms'] / a['median_ms']:9.0f}"
              f"  A bytes {alg / 1e6:.2f} MB")
    res["B_dump"] = summary(dump_ms)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--state", default="both", choices=["tw", "sess", "both"])
    ap.add_argument("--repeats-a", type=int, default=30)
    ap.add_argument("--repeats-b", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("view_ab: no GPU (nothing is measured without one)")
    eng = Engine(device=0, batch_capacity=1 << 23)
    res = {}
    for name, build, session in (("tw", build_tw, False), ("sess", build_sess, True)):
        if a.state not in (name, "both"):
            continue
        g = build(eng, torch)
        res[name] = measure(name, g, session, a.repeats_a, a.repeats_b)
        g.close()
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
