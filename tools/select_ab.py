#!/usr/bin/env python3
"""The scalar SELECT op (hsg_op_create_select, k_select.hip) timed HBM-resident
against its byte model, at a few selectivities and expression counts.

One query shape over device-resident batches of three columns (c0 i64, c1 f64,
c2 i64, each with a valid array, every value present):

  SELECT <e expressions over c1, c2> FROM s WHERE c0 > 0        e = 1 or 8

c0 is 1 for the share of records the run keeps and 0 for the rest, so WHERE
sets the selectivity (0, 0.5, 1 by default) and nothing else drops a record.
The rows go to registered device columns (hsg_op_set_changelog), so a push is
the staging-free path: one k_select launch and the fetch of the scalars.

Per configuration one op; the ops are pushed alternately, batch by batch, so
each sees the same machine. The first pushes of an op are warm-up. Reported per
configuration: the kernel's time (device events around the launch,
hsg_stats.agg_kernel_ms; median and min .. max over the timed pushes), the wall
time of a push (last_batch_ms, median), the model's bytes

  read     N * (4 + 8 + 8 * 3 + 3)       key, ts, three named words and bytes
  written  K * (28 + 8 e)                key, ws, we, src, e expressions

and bytes / kernel time. Every push's row count is checked against the mask.

  python tools/select_ab.py [--records N] [--steps S] [--warmup W] [--sel 0,0.5,1] [--exprs 1,8] [--json PATH]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from hstream_amd import abi  # noqa: E402
from hstream_amd.engine import Engine  # noqa: E402

I, F = abi.HSG_I64, abi.HSG_F64
W = abi
TS0 = 1_700_000_040_000
PEAK_BYTES_PER_S = 8e12         # the HBM bandwidth the project's rooflines use


def exprs(e):
    """e value programs over c1 (f64) and c2 (i64): products and sums with small constants."""
    out = []
    for j in range(e):
        if j % 2 == 0:
            out.append([(W.HSG_W_COL, 1), (W.HSG_W_F64, 0.25 * (j + 1)), (W.HSG_W_MUL,), (W.HSG_W_COL, 2), (W.HSG_W_ADD,)])
        else:
            out.append([(W.HSG_W_COL, 2), (W.HSG_W_I64, j), (W.HSG_W_MUL,), (W.HSG_W_COL, 2), (W.HSG_W_SUB,)])
    return out


def model_bytes(n, kept, e):
    """The launch's algorithmic bytes (csrc/k_select.hip): (read, written)."""
    return n * (4 + 8 + 8 * 3 + 3), kept * (28 + 8 * e)


def gen(seed, n, sel):
    rng = np.random.default_rng(seed)
    key = rng.integers(0, 65536, size=n).astype(np.uint32)
    ts = (TS0 + (np.arange(n, dtype=np.int64) * 150_000) // n + rng.integers(0, 2000, size=n)).astype(np.int64)
    flag = (rng.random(n) < sel).astype(np.int64) if 0 < sel < 1 else np.full(n, int(sel >= 1), np.int64)
    cols = [flag, rng.integers(-100, 101, size=n).astype(np.float64) / 4.0,
            rng.integers(-1000, 1001, size=n).astype(np.int64)]
    valids = [np.ones(n, np.uint8) for _ in cols]
    return key, ts, cols, valids


def to_device(torch, arrays):
    dev = torch.device("cuda:0")
    return [torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to(dev) for x in arrays]


class Run:
    def __init__(self, torch, eng, n, sel, e, seed):
        key, ts, cols, valids = gen(seed, n, sel)
        self.n, self.sel, self.e = n, sel, e
        self.kept = int(np.count_nonzero(cols[0] > 0))
        (self.key, self.ts), self.cols, self.valids = to_device(torch, [key, ts]), to_device(torch, cols), \
            to_device(torch, valids)
        types = [F if (j % 2 == 0) else I for j in range(e)]
        self.op = eng.select_op([I, F, I], exprs(e), where=[(W.HSG_W_COL, 0), (W.HSG_W_I64, 0), (W.HSG_W_GT,)])
        d = {k: torch.empty(n, dtype=t, device="cuda") for k, t in
             (("key", torch.int32), ("ws", torch.int64), ("we", torch.int64), ("src", torch.int64))}
        aggs = [torch.empty(n, dtype=torch.float64 if t == F else torch.int64, device="cuda") for t in types]
        ap = (C.c_void_p * len(aggs))(*[a.data_ptr() for a in aggs])
        self.keep = (d, aggs, ap)
        self.rows = abi.hsg_rows(capacity=n, mem=abi.HSG_MEM_DEVICE, n_aggs=len(aggs), key_id=d["key"].data_ptr(),
                                 win_start=d["ws"].data_ptr(), win_end=d["we"].data_ptr(),
                                 src_index=d["src"].data_ptr(), aggs=C.cast(ap, C.POINTER(C.c_void_p)))
        self.op.set_changelog(self.rows)
        self.kernel_ms, self.push_ms = [], []
        self.wm = -1

    def step(self, timed):
        before = self.op.stats()["agg_kernel_ms"]
        self.wm = self.op.push(self.key, self.ts, self.cols, self.valids, watermark=self.wm)
        st = self.op.stats()
        got = self.op.drain_count()
        if got != self.kept:
            sys.exit(f"select_ab: {got} rows, the mask keeps {self.kept}")
        if timed:
            self.kernel_ms.append(st["agg_kernel_ms"] - before)
            self.push_ms.append(st["last_batch_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sel", default="0,0.5,1")
    ap.add_argument("--exprs", default="1,8")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("select_ab: no GPU (nothing is measured without one)")
    eng = Engine(device=0, batch_capacity=a.records)
    runs = [Run(torch, eng, a.records, float(s), int(e), a.seed) for e in a.exprs.split(",") for s in a.sel.split(",")]
    torch.cuda.synchronize()
    for k in range(a.warmup + a.steps):
        for r in runs:
            r.step(k >= a.warmup)
    res = {"records": a.records, "steps": a.steps, "warmup": a.warmup, "runs": []}
    for r in runs:
        rd, wr = model_bytes(r.n, r.kept, r.e)
        km = float(np.median(r.kernel_ms))
        q = {"exprs": r.e, "selectivity": r.sel, "kept": r.kept, "kernel_ms": km, "kernel_ms_min": min(r.kernel_ms),
             "kernel_ms_max": max(r.kernel_ms), "push_ms": float(np.median(r.push_ms)), "read_bytes": rd,
             "written_bytes": wr, "bytes_per_s": (rd + wr) / (km * 1e-3),
             "share_of_peak": (rd + wr) / (km * 1e-3) / PEAK_BYTES_PER_S}
        res["runs"].append(q)
        print(f"e={r.e} sel={r.sel:g}: kernel {km:.4f} ms ({q['kernel_ms_min']:.4f} .. {q['kernel_ms_max']:.4f}), "
              f"push {q['push_ms']:.4f} ms, {(rd + wr) / 1e6:.1f} MB, {q['bytes_per_s'] / 1e12:.2f} TB/s "
              f"({100 * q['share_of_peak']:.1f} % of 8 TB/s)")
        r.op.set_changelog(None)
        r.op.close()
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
