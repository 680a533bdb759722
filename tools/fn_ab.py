#!/usr/bin/env python3
"""A/B of the numeric SQL functions in the map pass (HSG_W_FN, k_map.hip): that
the kernel today's programs run (function class 0) is the parent's, and what
the functions cost per record in the kernels of classes 1 and 2.

Device time of k_map from a kernel trace: every step is a child process under
its own `timeout`, `rocprofv3 --kernel-trace` around one worker that pushes
the seeded, device-resident batches (2^22 records, 65 536 keys, tumbling 60 s,
per-batch changelog) through one mapped op per repeat; the step's figure is
the median duration of its k_map dispatches.

  1. SELECT COUNT(*), SUM(c0 * c1), MAX(c0 - c2)   c0 i64, c1 f64, c2 i64
     on the parent's build (--parent DIR: a checkout of the parent commit with
     its library built) and on this tree, alternately, --runs times each. This
     tree's median must lie within the quartiles of the parent's runs: nothing
     in class 0 changed, so the parent's own run-to-run spread is the margin.
  2. SUM(ABS(c0)), SUM(SQRT(c0)), SUM(LOG(c0)), SUM(SIN(c0)) on this tree,
     against the pass's byte model (csrc/k_map.hip):
       N * (8 * [keys written] + 9 * named inputs + (8 + [valid written]) * computed outputs)
     here N * (9 + 9): one input with a valid array, one output with one.
     Reported: achieved bytes/s and its share of 8 TB/s. No target is set.

  python tools/fn_ab.py [--parent DIR] [--records N] [--keys K] [--batches B] [--repeats R] [--runs M]
                        [--out DIR] [--json PATH]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TS0 = 1_700_000_040_000
PEAK_BYTES_PER_S = 8e12         # the HBM bandwidth the project's rooflines use
STEP_TIMEOUT_S = 240
FNS = ("ABS", "SQRT", "LOG", "SIN")


def map_bytes(n, keys_written, named_inputs, computed, valid_written):
    """The pass's algorithmic bytes (csrc/k_map.hip)."""
    return n * (8 * int(keys_written) + 9 * named_inputs + (8 + int(valid_written)) * computed)


def gen_batches(seed, nb, n, nkeys):
    """tools/map_ab.py's batches: c0 in [-1000, 1000] (half of SQRT's and LOG's
    operands are outside the domain: the error value, which costs what a
    value costs), 3 % absent per column."""
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


def worker(a):
    """One process, one tree: `repeats` ops over the batches. Prints the wall medians (the trace has the kernels)."""
    sys.path.insert(0, a.tree)
    import torch
    from hstream_amd import abi as W
    from hstream_amd.columnar import OpSpec
    from hstream_amd.engine import Engine
    if not torch.cuda.is_available():
        sys.exit("fn_ab: no GPU (nothing is measured without one)")
    I, F = W.HSG_I64, W.HSG_F64
    if a.worker == "arith":
        spec = dict(col_types=[I, F, I], aggs=[(W.HSG_COUNT_ALL, 0), (W.HSG_SUM, 0), (W.HSG_MAX, 1)],
                    map=[[(W.HSG_W_COL, 0), (W.HSG_W_COL, 1), (W.HSG_W_MUL,)],
                         [(W.HSG_W_COL, 0), (W.HSG_W_COL, 2), (W.HSG_W_SUB,)]])
    else:
        spec = dict(col_types=[I, F, I], aggs=[(W.HSG_COUNT_ALL, 0), (W.HSG_SUM, 0)],
                    map=[[(W.HSG_W_COL, 0), (W.HSG_W_FN, getattr(W, "HSG_FN_" + a.worker))]])
    eng = Engine(device=0, batch_capacity=a.records)
    dev = torch.device("cuda:0")
    batches = []
    for key, ts, cols, valids in gen_batches(a.seed, a.batches, a.records, a.keys):
        t = lambda x: torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to(dev)
        batches.append((t(key), t(ts), [t(c) for c in cols], [t(v) for v in valids]))
    torch.cuda.synchronize()
    med, rows = [], 0
    for _ in range(a.repeats):
        g = eng.op(OpSpec(W.HSG_TUMBLING, W.HSG_EMIT_PER_BATCH, size_ms=60_000, state_capacity=1 << 20, **spec))
        ms, wm = [], -1
        for key, ts, cols, valids in batches:
            wm = g.push(key, ts, cols, valids, watermark=wm)
            ms.append(g.stats()["last_batch_ms"])
            rows += len(g.drain())
        g.close()
        med.append(float(np.median(ms[1:])))
    eng.close()
    print(json.dumps({"worker": a.worker, "push_ms": float(np.median(med)), "rows": rows}))


def traced(a, name, query, tree):
    """One step: the worker for `query` on `tree` under a kernel trace of its own. Its k_map dispatches' microseconds."""
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), "rocprofv3", "--kernel-trace", "-d", a.out, "-o", name,
           "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--worker", query, "--tree", tree,
           "--records", str(a.records), "--keys", str(a.keys), "--batches", str(a.batches), "--repeats",
           str(a.repeats), "--seed", str(a.seed)]
    with open(os.path.join(a.out, name + ".log"), "w") as log:
        rc = subprocess.call(cmd, stdout=log, stderr=subprocess.STDOUT, cwd=tree)
    if rc != 0:
        # (a fault, an abort or a time limit: nothing more is started on the GPU)
        sys.exit(f"fn_ab: step {name} ended with status {rc}; see {a.out}/{name}.log")
    files = glob.glob(os.path.join(a.out, "**", name + "_kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"fn_ab: step {name} left no kernel trace")
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
          for r in csv.DictReader(open(files[0])) if "k_map" in r["Kernel_Name"]]
    if len(us) != a.batches * a.repeats:
        sys.exit(f"fn_ab: step {name}: {len(us)} k_map dispatches, not {a.batches * a.repeats}")
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, its library built")
    ap.add_argument("--records", type=int, default=1 << 22)
    ap.add_argument("--keys", type=int, default=65536)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "build", "fn_ab"),
                    help="where the traces and step logs go (default: build/fn_ab, which git ignores)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=os.path.abspath(os.path.join(HERE, "..")), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    a.out = os.path.abspath(a.out)  # (a step runs from its tree's root)
    res = {"records": a.records, "keys": a.keys, "batches": a.batches, "repeats": a.repeats, "runs": a.runs}
    # 1. class 0 against the parent, alternately
    runs = {"parent": [], "this": []}
    for r in range(a.runs):
        for who, tree in (("parent", a.parent), ("this", a.tree)):
            if tree is None:
                continue
            us = traced(a, f"arith_{who}_{r}", "arith", os.path.abspath(tree))
            runs[who].append(float(np.median(us)))
            print(f"arith {who} run {r}: k_map median {runs[who][-1]:.1f} us")
    nbytes = map_bytes(a.records, keys_written=False, named_inputs=3, computed=2, valid_written=True)
    res["class0"] = {"bytes": nbytes, "runs_us": runs}
    if runs["parent"]:
        q1, q3 = (float(x) for x in np.percentile(runs["parent"], [25, 75]))
        m = float(np.median(runs["this"]))
        res["class0"].update(parent_q1_us=q1, parent_q3_us=q3, parent_median_us=float(np.median(runs["parent"])),
                             this_median_us=m, within_parent_quartiles=bool(q1 <= m <= q3))
        side = "within" if q1 <= m <= q3 else ("OUTSIDE, below Q1 (faster)" if m < q1 else "OUTSIDE, above Q3 (slower)")
        print(f"class 0: this {m:.2f} us, the parent's quartiles {q1:.2f} .. {q3:.2f} us: {side}")
    # 2. the functions against the byte model
    fbytes = map_bytes(a.records, keys_written=False, named_inputs=1, computed=1, valid_written=True)
    res["functions"] = {}
    for f in FNS:
        us = traced(a, f"fn_{f}", f, a.tree)
        m = float(np.median(us))
        bps = fbytes / (m * 1e-6)
        res["functions"][f] = {"k_map_us": m, "min_us": min(us), "max_us": max(us), "bytes": fbytes, "bytes_per_s": bps,
                               "share_of_peak": bps / PEAK_BYTES_PER_S, "ns_per_record": m * 1e3 / a.records}
        print(f"SUM({f}(c0)): k_map {m:.1f} us ({min(us):.1f} .. {max(us):.1f}) for {fbytes} bytes: "
              f"{bps / 1e12:.2f} TB/s, {100 * bps / PEAK_BYTES_PER_S:.1f} % of 8 TB/s")
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fjson:
            fjson.write(line + "\n")
    if runs["parent"] and not res["class0"]["within_parent_quartiles"]:
        sys.exit("fn_ab: the class-0 k_map time is outside the parent's quartiles")


if __name__ == "__main__":
    main()
