#!/usr/bin/env python3
"""Push time of an op with a HAVING program (k_having.hip), for comparing two
trees: it imports hstream_amd from the working directory, so run it from the
root of the tree to be measured, alternating between the two.

Tumbling 60 s, per batch, SELECT COUNT(*), SUM(c0) ... HAVING COUNT(*) > 60 AND
SUM(c0) > 0.5, device-resident batches of 2^22 records over 65 536 keys; four
batches per op, the first untimed; prints the median (min .. max) over five ops
of the median push time (hsg_stats last_batch_ms), and the rows the filter
dropped, which two trees must agree on.

  cd TREE && python PATH/tools/having_ab.py
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
from hstream_amd import abi
from hstream_amd.columnar import OpSpec
from hstream_amd.engine import Engine
import torch
W = abi
N, K, NB, REP = 1 << 22, 65536, 4, 5
HAV = [(W.HSG_W_COL, 0), (W.HSG_W_I64, 60), (W.HSG_W_GT,), (W.HSG_W_COL, 1), (W.HSG_W_F64, 0.5), (W.HSG_W_GT,), (W.HSG_W_AND,)]
eng = Engine(device=0, batch_capacity=N)
dev = []
for b in range(NB):
    rng = np.random.default_rng([1, b])
    key = rng.integers(0, K, size=N).astype(np.uint32)
    i = np.arange(b * N, (b + 1) * N, dtype=np.int64)
    ts = (1_700_000_040_000 + (i * 150_000) // (NB * N) + rng.integers(0, 2000, size=N)).astype(np.int64)
    c0 = rng.integers(-1000, 1001, size=N).astype(np.int64)
    d = torch.device("cuda:0")
    dev.append((torch.from_numpy(key.view(np.int32)).to(d), torch.from_numpy(ts).to(d), [torch.from_numpy(c0).to(d)]))
torch.cuda.synchronize()
med, dropped = [], None
for _ in range(REP + 1):
    g = eng.op(OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=60_000, col_types=[abi.HSG_I64],
                      aggs=[(abi.HSG_COUNT_ALL, 0), (abi.HSG_SUM, 0)], state_capacity=1 << 20, having=HAV))
    ms, wm = [], -1
    for key, ts, cols in dev:
        wm = g.push(key, ts, cols, None, watermark=wm)
        ms.append(g.stats()["last_batch_ms"])
        g.drain()
    dropped = g.stats()["having_dropped_total"]
    g.close()
    med.append(float(np.median(ms[1:])))
med = med[1:]
print(json.dumps({"median_ms": float(np.median(med)), "min_ms": min(med), "max_ms": max(med), "having_dropped_total": dropped}))
