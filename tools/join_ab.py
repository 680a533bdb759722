#!/usr/bin/env python3
"""A/B of the valued stream-stream join's drain (hsg_join_drain_batch,
k_join_vals.hip) against the route to "the joined rows as device-resident
columns" that existed before it.

One stream, pushed to two joins in batches of 2^20 records (both sides
interleaved, 2^16 record keys, one join key, 1,024 records per millisecond,
window +-512 ms: about 4 joined rows per record, reaching into the batch
before). The value columns are random bits with random valid bytes.

  A   the handle join: Join.drain() to host arrays, a numpy gather of both
      records' columns and valid bytes from the host copy of the values, and
      the upload of the joined columns (torch .cuda())
  B   the valued join: Join.drain_batch(device=True) -- the gather kernel over
      the value rows in HBM, output columns written in place

First B must equal A column by column, bit for bit, on every batch. Each
batch's push and drain are timed apart (wall clock of the Python calls; every
call ends in its own stream synchronise): the claim is B's drain against A's
drain + gather + upload, from the same pending rows to the same device
columns. The pushes are reported too (B's carries the append of the value
rows). The gather kernel's share is the raw hsg_join_drain_batch call into
preallocated device arrays (the kernel, its launch and the synchronise),
set against its algorithmic bytes: 16 + 2 * 8 * stride read and 9 (c0 + c1) +
12 written per row. Bytes actually moved are not measured here.

  python tools/join_ab.py [--batches N] [--records N] [--cols 3,2 4,4] [--json PATH]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from hstream_amd import abi  # noqa: E402
from hstream_amd.engine import Engine  # noqa: E402
from hstream_amd.join import Join, value_stride  # noqa: E402

NKEYS = 1 << 16
PER_MS = 1 << 10
WINDOW = 512
T0 = 1_700_000_000_000


def gen_batch(rng, b, n, vc):
    side = (rng.random(n) < 0.5).astype(np.uint8)
    key = rng.integers(0, NKEYS, n).astype(np.uint32)
    jk = np.full(n, 7, np.uint32)
    ts = T0 + (b * n + np.arange(n, dtype=np.int64)) // PER_MS
    cols = [rng.integers(0, 2**63, n, dtype=np.int64) for _ in range(vc)]
    valid = [rng.integers(0, 2, n).astype(np.uint8) for _ in range(vc)]
    return side, key, jk, ts, cols, valid


def summary(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "n": len(ms)}


def raw_device_drain(torch, j, n, types):
    """hsg_join_drain_batch into preallocated device arrays: (ms, arrays)"""
    cols = [torch.empty(n, dtype=torch.float64 if t == abi.HSG_F64 else torch.int64, device="cuda") for t in types]
    valid = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in types]
    key_id = torch.empty(n, dtype=torch.int32, device="cuda")
    ts = torch.empty(n, dtype=torch.int64, device="cuda")
    cp = (C.c_void_p * max(1, len(types)))(*[c.data_ptr() for c in cols])
    vp = (C.c_void_p * max(1, len(types)))(*[v.data_ptr() for v in valid])
    o = abi.hsg_join_joined(capacity=n, mem=abi.HSG_MEM_DEVICE, key_col=-1, key_id=key_id.data_ptr(),
                            ts=ts.data_ptr(), cols=C.cast(cp, C.POINTER(C.c_void_p)),
                            valid=C.cast(vp, C.POINTER(C.c_void_p)))
    got = C.c_uint64()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = j._L.hsg_join_drain_batch(j._h, C.byref(o), C.byref(got))
    ms = (time.perf_counter() - t0) * 1e3
    if rc != abi.HSG_OK or got.value != n:
        sys.exit(f"join_ab: hsg_join_drain_batch: {rc}, {got.value} of {n} rows")
    return ms, (key_id, ts, cols, valid)


def run(torch, eng, c0, c1, nb, n):
    types = ([abi.HSG_I64, abi.HSG_F64] * 4)[:c0], ([abi.HSG_F64, abi.HSG_I64] * 4)[:c1]
    flat = list(types[0]) + list(types[1])
    vc, stride = max(c0, c1), value_stride(c0, c1)
    rng = np.random.default_rng(14)
    ja = Join(eng, WINDOW, WINDOW, batch_capacity=n)
    jb = Join(eng, WINDOW, WINDOW, batch_capacity=n, cols=types)
    V = [np.empty((nb + 1) * n, np.int64) for _ in range(vc)]
    VV = [np.empty((nb + 1) * n, np.uint8) for _ in range(vc)]
    t = {k: [] for k in ("A_push", "A_drain", "A_gather", "A_upload", "B_push", "B_drain", "B_kernel_call")}
    rows_per_batch = []
    up = lambda a: torch.from_numpy(a).cuda()
    for b in range(nb + 1):  # batch 0 warms both joins up and is not timed
        side, key, jk, ts, cols, valid = gen_batch(rng, b, n, vc)
        for k in range(vc):
            V[k][b * n:(b + 1) * n], VV[k][b * n:(b + 1) * n] = cols[k], valid[k]
        handle = np.arange(b * n, (b + 1) * n, dtype=np.int64)
        d = [up(side), up(key.view(np.int32)), up(jk.view(np.int32)), up(ts), up(handle)]
        dc, dv = [up(c) for c in cols], [up(v) for v in valid]
        torch.cuda.synchronize()
        # A
        t0 = time.perf_counter()
        ja.push(*d)
        t1 = time.perf_counter()
        th, oh, _, ats = ja.drain()
        t2 = time.perf_counter()
        th, oh = th.view(np.int64), oh.view(np.int64)
        acols = [V[k][th] for k in range(c0)] + [V[k][oh] for k in range(c1)]
        avalid = [VV[k][th] for k in range(c0)] + [VV[k][oh] for k in range(c1)]
        t3 = time.perf_counter()
        dev = [up(a) for a in acols] + [up(a) for a in avalid] + [up(ats)]
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        # B: odd batches through Join.drain_batch, even ones through the raw call
        t5 = time.perf_counter()
        jb.push(*d[:4], cols=dc, valid=dv)
        t6 = time.perf_counter()
        rows = jb.pending()
        if rows != len(ats):
            sys.exit(f"join_ab: batch {b}: {rows} rows pending, the handle join gave {len(ats)}")
        if b % 2:
            t7 = time.perf_counter()
            out = jb.drain_batch(device=True)
            kms, bms = None, (time.perf_counter() - t7) * 1e3
            bts, bcols, bvalid = out.ts, out.cols, out.valid
        else:
            kms, (_, bts, bcols, bvalid) = raw_device_drain(torch, jb, rows, flat)
            bms = None
        same = np.array_equal(bts.cpu().numpy(), ats)
        for k in range(c0 + c1):
            same = same and np.array_equal(bcols[k].cpu().numpy().view(np.int64), acols[k])
            same = same and np.array_equal(bvalid[k].cpu().numpy(), avalid[k])
        if not same:
            sys.exit(f"join_ab: ({c0}, {c1}) batch {b}: A and B differ")
        del dev
        if b == 0:
            continue
        rows_per_batch.append(rows)
        for name, ms in (("A_push", t1 - t0), ("A_drain", t2 - t1), ("A_gather", t3 - t2), ("A_upload", t4 - t3),
                         ("B_push", t6 - t5)):
            t[name].append(ms * 1e3)
        if bms is not None:
            t["B_drain"].append(bms)
        else:
            t["B_kernel_call"].append(kms)
    ja.close()
    jb.close()
    rows = float(np.mean(rows_per_batch))
    a_total = [x + y + z for x, y, z in zip(t["A_drain"], t["A_gather"], t["A_upload"])]
    res = {k: summary(v) for k, v in t.items() if v}
    res["A_total"] = summary(a_total)
    alg_r, alg_w = 16 + 2 * 8 * stride, 9 * (c0 + c1) + 12
    km = res["B_kernel_call"]["median_ms"]
    res.update({"c0": c0, "c1": c1, "stride_words": int(stride), "records_per_batch": n, "rows_per_batch": rows,
                "fan_out": rows / n, "A_over_B": res["A_total"]["median_ms"] / res["B_drain"]["median_ms"],
                "gather_bytes_read_per_row": alg_r, "gather_bytes_written_per_row": alg_w,
                "gather_algorithmic_GBps": rows * (alg_r + alg_w) / (km * 1e-3) / 1e9,
                "gather_rows_per_s": rows / (km * 1e-3)})
    print(f"({c0}, {c1}) stride {stride}: {rows:.0f} rows/batch (fan-out {rows / n:.2f})  "
          f"A drain {res['A_drain']['median_ms']:.1f} + gather {res['A_gather']['median_ms']:.1f} + upload "
          f"{res['A_upload']['median_ms']:.1f} = {res['A_total']['median_ms']:.1f} ms   B drain_batch "
          f"{res['B_drain']['median_ms']:.2f} ms ({res['A_over_B']:.0f}x)   raw call {km:.3f} ms = "
          f"{res['gather_algorithmic_GBps']:.0f} GB/s algorithmic   push A {res['A_push']['median_ms']:.1f} "
          f"B {res['B_push']['median_ms']:.1f} ms", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=6, help="timed batches per configuration (after one warm-up)")
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--cols", nargs="*", default=["3,2", "4,4"], help="c0,c1 per configuration")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("join_ab: no GPU (nothing is measured without one)")
    eng = Engine(device=0, batch_capacity=a.records)
    res = {"configs": []}
    for spec in a.cols:
        c0, c1 = (int(x) for x in spec.split(","))
        res["configs"].append(run(torch, eng, c0, c1, a.batches, a.records))
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
