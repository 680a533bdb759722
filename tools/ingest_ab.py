#!/usr/bin/env python3
"""A/B of the device JSON decode (hsg_gpu_decode_json, k_ingest.hip) against
the host decoder it stands in for (hsg_decode_json_spelled).

Input: C2-shaped JSON records ({"k": int, "v": int, "x": decimal}), batches of
2^20 records over 65 536 keys, in steady state: a first batch makes every key
known (on the device path that batch runs at host speed and is not timed).

  A  GpuDecoder.decode(...), then the batch's ready_event: from the start of
     the upload to the last write of the device batch
  B  Decoder.decode(...) on 1, 8 and 16 host threads, same bytes

First A's batch, copied back, must equal B's arrays bit for bit, and A must
have decoded every record on the device (host_records == 0). Then each is
timed over repeats (wall clock of the Python call): median and min .. max
records/s. Two ratios are reported:

  vs_host16    A's median rate / B's at 16 threads (a GPU command's whole CPU
               allowance): expected >= 1, nothing more is asked
  of_link      A's median rate / (link bytes/s / bytes per record uploaded):
               the share of the input link's ceiling; --link-gbs defaults to
               the PCIe rate bench.py reports as input_link.achieved

  python tools/ingest_ab.py [--records N] [--repeats R] [--link-gbs G] [--json PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import jsongen  # noqa: E402
from hstream_amd import abi  # noqa: E402
from hstream_amd.engine import Engine  # noqa: E402
from hstream_amd.ingest import Decoder, GpuDecoder, KeyDict, pack_records  # noqa: E402

COLS = [("v", abi.HSG_I64, True), ("x", abi.HSG_F64, True)]


def rate(n, times):
    t = np.array(times)
    return {"median_rps": n / float(np.median(t)), "min_rps": n / float(t.max()), "max_rps": n / float(t.min()),
            "median_ms": 1e3 * float(np.median(t))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--keys", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--link-gbs", type=float, default=53.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = a.records
    warm = [b'{"k":%d,"v":0,"x":0.5}' % i for i in range(a.keys)]
    batches = [pack_records(jsongen.c2_records(100 + r, n, n_keys=a.keys)) for r in range(2)]
    ts = 1_700_000_000_000 + (np.arange(n, dtype=np.int64) * 3_600_000) // n
    nbytes = [len(b) for b, _ in batches]
    per_record_up = (nbytes[0] + 8 * (n + 1) + 8 * n) / n  # the bytes, the offsets, the timestamps

    eng = Engine(device=0, batch_capacity=max(n, 1 << 16))
    gk, hk = KeyDict(), KeyDict()
    gd = GpuDecoder(eng, gk, "k", COLS, max_records=max(n, a.keys), max_bytes=max(max(nbytes), 64 * a.keys),
                    table_slots=4 * a.keys)
    hd = Decoder("k", COLS)
    wbuf, woff = pack_records(warm)
    wts = np.zeros(len(warm), np.int64)
    s0 = gd.decode(wbuf, woff, wts, threads=16).stats
    hd.decode(hk, wbuf, woff, wts, threads=16)

    # equal first
    buf, off = batches[0]
    db = gd.decode(buf, off, ts, threads=16)
    key, t, cols, valid, _ = db.to_host()
    want = hd.decode(hk, buf, off, ts, threads=16)
    same = bool(np.array_equal(key, want[0]) and np.array_equal(t, want[1]) and
                all(np.array_equal(cols[c].view(np.uint64), want[2][c].view(np.uint64)) and
                    np.array_equal(valid[c], want[3][c]) for c in range(len(COLS))) and
                np.array_equal(db.status, want[4]) and len(gk) == len(hk))
    res = {"records": n, "keys": a.keys, "bytes_per_record_json": nbytes[0] / n,
           "bytes_per_record_uploaded": per_record_up, "identical": same, "first_batch": s0,
           "steady_host_records": db.stats["host_records"]}

    ta = []
    for r in range(a.repeats + 1):
        buf, off = batches[r & 1]
        t0 = time.perf_counter()
        db = gd.decode(buf, off, ts, threads=16)
        db.wait()
        ta.append(time.perf_counter() - t0)
        assert db.stats["host_records"] == 0
    res["device"] = rate(n, ta[1:])
    for th in (1, 8, 16):
        tb = []
        for r in range(a.repeats + 1):
            buf, off = batches[r & 1]
            t0 = time.perf_counter()
            hd.decode(hk, buf, off, ts, threads=th)
            tb.append(time.perf_counter() - t0)
        res[f"host_{th}"] = rate(n, tb[1:])
    ceiling = a.link_gbs * 1e9 / per_record_up
    res["vs_host16"] = res["device"]["median_rps"] / res["host_16"]["median_rps"]
    res["link_ceiling_rps"] = ceiling
    res["of_link"] = res["device"]["median_rps"] / ceiling
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    gd.close()
    hd.close()
    eng.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
