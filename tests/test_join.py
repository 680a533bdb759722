"""Stream-stream join (include/hstream_join.h) against the oracle
(oracle/joinref.py, a record-by-record restatement of joinStreamProcessor,
Stream.hs:267-300, over InMemoryTimestampedKVStore, Store.hs:316-385).

CPU: hand-derived vectors pin the oracle (window bounds, the end-point quirk
of tksRange, overwrite of an equal (key, ts), the missing-join-field abort).
GPU: batches of interleaved records compared row for row, in order.
The reference's one join vector (RegressionSpec.hs:24-40, #391_JOIN: join ->
unwindowed GROUP BY) runs through the oracle on CPU and the GPU join + GPU
op on the GPU.
"""
import numpy as np
import pytest

import joinref
import pyoracle
from joinref import NONE
from util import load_kat, run_join_kat

JOIN_KAT = load_kat()["joins"]


def _jarrays(b):
    return (np.asarray(b["side"], np.uint8), np.asarray(b["key_id"], np.uint32),
            np.asarray(b["join_key"], np.uint32), np.asarray(b["ts"], np.int64), np.asarray(b["handle"], np.uint64))


@pytest.mark.parametrize("case", JOIN_KAT, ids=lambda c: c["name"])
def test_reference_join_kat_oracle(case):
    ref = joinref.JoinRef(case["join"]["before_ms"], case["join"]["after_ms"])
    run_join_kat(case, lambda b: ref.push(*_jarrays(b)), lambda spec: pyoracle.OracleOp(spec))


@pytest.mark.gpu
@pytest.mark.parametrize("case", JOIN_KAT, ids=lambda c: c["name"])
def test_reference_join_kat_gpu(case):
    import torch
    assert torch.cuda.is_available()
    from hstream_amd.engine import Engine
    from hstream_amd.join import Join
    eng = Engine(device=0, batch_capacity=1 << 10)
    j = Join(eng, case["join"]["before_ms"], case["join"]["after_ms"], batch_capacity=1 << 10)

    def push(b):
        j.push(*_jarrays(b))
        return list(zip(*[x.tolist() for x in j.drain()]))

    run_join_kat(case, push, lambda spec: eng.op(spec))
    j.close()
    eng.close()


def _run(ref, recs):
    rows = []
    for side, key, jk, ts, h in recs:
        rows += ref.push_one(side, key, jk, ts, h)
    return rows


def test_window_and_orientation():
    # before 10, after 5: a this-record at t matches other-records in [t-10, t+5]
    r = joinref.JoinRef(10, 5)
    rows = _run(r, [(1, 7, 1, 100, 1), (1, 7, 1, 94, 2), (1, 7, 1, 106, 3), (0, 7, 1, 100, 4)])
    # endpoints 90 / 105 are not held by the other store: open interval (90, 105)
    assert rows == [(4, 2, 1, 100), (4, 1, 1, 100)]
    # an other-record at 112 matches this-records in [112-5, 112+10] = [107, 122]: none
    assert r.push_one(1, 7, 1, 112, 5) == []


def test_endpoints_need_both_ends_present():
    r = joinref.JoinRef(10, 10)
    # other store holds ts 90 and 110 (different keys fill them)
    _run(r, [(1, 7, 1, 90, 1), (1, 8, 1, 110, 2), (1, 7, 1, 95, 3)])
    # both end timestamps 90 and 110 present: inclusive -> key 7 at 90 and 95
    assert r.push_one(0, 7, 1, 100, 9) == [(9, 1, 1, 100), (9, 3, 1, 100)]
    r2 = joinref.JoinRef(10, 10)
    _run(r2, [(1, 7, 1, 90, 1), (1, 7, 1, 95, 3)])
    # only 90 present: exclusive -> 90 drops out
    assert r2.push_one(0, 7, 1, 100, 9) == [(9, 3, 1, 100)]
    # zero-width window never matches (splitLookup of the same point twice)
    r3 = joinref.JoinRef(0, 0)
    _run(r3, [(1, 7, 1, 100, 1)])
    assert r3.push_one(0, 7, 1, 100, 2) == []


def test_overwrite_and_missing_join_key():
    r = joinref.JoinRef(10, 10)
    _run(r, [(1, 7, 1, 100, 1), (1, 7, 2, 100, 2)])  # same (key, ts): the second replaces the first
    assert r.push_one(0, 7, 1, 101, 3) == []
    assert r.push_one(0, 7, 2, 101, 4) == [(4, 2, 2, 101)]
    r2 = joinref.JoinRef(10, 10)
    _run(r2, [(1, 7, 1, 95, 1), (1, 7, NONE, 97, 2), (1, 7, 1, 99, 3)])
    # ascending candidates: 95 joins, 97 has no join field -> the scan stops
    assert r2.push_one(0, 7, 1, 100, 9) == [(9, 1, 1, 100)]
    assert r2.push_one(0, 7, NONE, 100, 10) == []


# ---------------------------------------------------------------------------
# Hand-derived vectors of the rules the GPU edge tests (tests/
# test_gpu_join_edges.py) trust the oracle on. Each is (name, before, after,
# [(record (side, key, join key, ts, handle), the rows it forwards)], entries
# the two stores hold afterwards), derived from the reference's code alone:
#   put      Store.hs:342-353  tksPut: Map.insert under (ts, key), the last put wins
#   range    Store.hs:355-365  tksRange: splitLookup at both end timestamps of the
#                              *other* store as it stands at that moment; the end
#                              points come back only when both lookups are Just
#                              (any key's entry makes a timestamp present)
#   scan     Store.hs:370-380  genR: ascending timestamps, the record key's entry
#   record   Stream.hs:281-300 joinStreamProcessor: fromJust recordKey (283) throws
#                              before tksPut (286) for a record without a key;
#                              put first, then range over [ts - before, ts + after]
#                              of the other store (288); rows under max of the
#                              two timestamps (299)
#   sides    Stream.hs:238-241 the other side's processor swaps before / after
#                              and flips the joiner: rows are (this, other)
# ---------------------------------------------------------------------------
HAND_VECTORS = [
    # The holder of an end timestamp arrives after the probing record: the
    # range saw the other store without it (Stream.hs:288 runs per record,
    # Store.hs:356 reads the map then), so it is exclusive for record 3 and
    # inclusive for the identical record 5, which arrives after the holder
    # (record 4, another key: Store.hs:357-358 look timestamps up, not keys).
    ("endpoint_holder_arrives_later", 10, 10, [
        ((1, 7, 1, 90, 1), []),
        ((1, 7, 1, 95, 2), []),
        ((0, 7, 1, 100, 3), [(3, 2, 1, 100)]),                  # 110 absent: (90, 110), 90 drops out
        ((1, 8, 1, 110, 4), []),                                # key 8 has no side-0 entries
        ((0, 7, 1, 100, 5), [(5, 1, 1, 100), (5, 2, 1, 100)]),  # [90, 110]; replaces record 3 (Store.hs:347)
    ], 4),
    # An end timestamp held only by another record key counts (Store.hs:357-358).
    ("endpoint_held_by_other_key", 10, 10, [
        ((1, 7, 1, 90, 1), []),
        ((1, 7, 1, 95, 2), []),
        ((1, 8, 2, 110, 3), []),
        ((0, 7, 1, 100, 4), [(4, 1, 1, 100), (4, 2, 1, 100)]),
    ], 4),
    # One held only by a record without the join field counts: the record has
    # a key, so tksPut stores it (Stream.hs:286) before any key selector runs
    # (295-296); its own scan finds no candidate.
    ("endpoint_held_by_record_without_join_field", 10, 10, [
        ((1, 7, 1, 90, 1), []),
        ((1, 7, 1, 95, 2), []),
        ((1, 9, NONE, 110, 3), []),
        ((0, 7, 1, 100, 4), [(4, 1, 1, 100), (4, 2, 1, 100)]),
    ], 4),
    # One carried only by a record without a key does not: fromJust
    # (Stream.hs:283) throws before tksPut (286), nothing is stored.
    ("endpoint_carried_by_keyless_record", 10, 10, [
        ((1, 7, 1, 90, 1), []),
        ((1, 7, 1, 95, 2), []),
        ((1, NONE, 1, 110, 3), []),
        ((0, 7, 1, 100, 4), [(4, 2, 1, 100)]),
    ], 3),
    # Three versions of side 1's (key 7, ts 100) with probes between them:
    # each probe meets the version that stood when it arrived (Store.hs:347
    # replaces; Stream.hs:288 reads at that moment). The versions probe too
    # (side 1 over [100 - 10, 100 + 10] of side 0's store, Stream.hs:241): rows
    # are (this, other) whichever side arrived last.
    ("three_versions_between_probes", 10, 10, [
        ((1, 7, 1, 100, 1), []),
        ((0, 7, 1, 101, 11), [(11, 1, 1, 101)]),
        ((1, 7, 2, 100, 2), []),                                # side 0 holds (101, join key 1) only
        ((0, 7, 2, 102, 12), [(12, 2, 2, 102)]),
        ((1, 7, 1, 100, 3), [(11, 3, 1, 101)]),                 # 101 joins, 102 has join key 2
        ((0, 7, 1, 103, 13), [(13, 3, 1, 103)]),
    ], 4),
    # before 0, after 10: a side-0 record at t takes side-1 records in
    # [t, t + 10]; a side-1 record at u takes side-0 records in [u - 10, u]
    # (Stream.hs:238-241). Then the zero end itself (key 9): equal timestamps
    # join only once the far end (210) is present too.
    ("before_zero", 0, 10, [
        ((1, 7, 1, 105, 1), []),
        ((1, 7, 1, 95, 2), []),
        ((0, 7, 1, 100, 3), [(3, 1, 1, 105)]),                  # (100, 110): 105; 95 is before
        ((1, 7, 1, 108, 4), [(3, 4, 1, 108)]),                  # (98, 108): 100
        ((1, 7, 1, 99, 5), []),                                 # (89, 99): 100 is after
        ((1, 9, 1, 200, 6), []),
        ((0, 9, 1, 200, 7), []),                                # 210 absent: (200, 210) is empty of 200
        ((1, 8, 1, 210, 8), []),
        ((0, 9, 1, 200, 9), [(9, 6, 1, 200)]),                  # [200, 210]
    ], 8),
    # before 10, after 0: the mirror image.
    ("after_zero", 10, 0, [
        ((1, 7, 1, 105, 1), []),
        ((1, 7, 1, 95, 2), []),
        ((0, 7, 1, 100, 3), [(3, 2, 1, 100)]),                  # (90, 100): 95
        ((1, 7, 1, 92, 4), [(3, 4, 1, 100)]),                   # (92, 102): 100
        ((1, 7, 1, 101, 5), []),                                # (101, 111)
        ((1, 9, 1, 200, 6), []),
        ((0, 9, 1, 200, 7), []),                                # 190 absent
        ((1, 8, 1, 190, 8), []),
        ((0, 9, 1, 200, 9), [(9, 6, 1, 200)]),                  # [190, 200]
    ], 8),
]


@pytest.mark.parametrize("vec", HAND_VECTORS, ids=lambda v: v[0])
def test_hand_vectors(vec):
    _, before, after, steps, state = vec
    r = joinref.JoinRef(before, after)
    for i, (rec, rows) in enumerate(steps):
        assert r.push_one(*rec) == rows, f"record {i + 1}"
    assert r.state_rows() == state
    # the same records as one batch
    r = joinref.JoinRef(before, after)
    cols = list(zip(*[rec for rec, _ in steps]))
    assert r.push(*cols) == [row for _, rows in steps for row in rows]


def _gen(seed, n, nkeys=40, grid=5, span=40_000, none_frac=0.03):
    rng = np.random.default_rng(seed)
    side = (rng.random(n) < 0.5).astype(np.uint8)
    key = rng.integers(0, nkeys, n).astype(np.uint32)
    key[rng.random(n) < 0.01] = NONE
    jk = rng.integers(0, 3, n).astype(np.uint32)
    jk[rng.random(n) < none_frac] = NONE
    # near-sorted timestamps on a coarse grid: many equal timestamps and window end points
    ts = ((np.arange(n) * span) // n + rng.integers(0, 400, n)) // grid * grid
    ts = ts.astype(np.int64) + 1_700_000_000_000
    handle = np.arange(n, dtype=np.uint64) + (seed << 32)
    return side, key, jk, ts, handle


@pytest.mark.gpu
@pytest.mark.parametrize("before,after,grid", [(100, 50, 5), (30, 30, 10), (0, 0, 1), (250, 0, 25)])
def test_join_matches_oracle(before, after, grid):
    import torch
    assert torch.cuda.is_available()
    from hstream_amd.engine import Engine
    from hstream_amd.join import Join
    eng = Engine(device=0, batch_capacity=1 << 16)
    j = Join(eng, before, after, batch_capacity=1 << 14)
    ref = joinref.JoinRef(before, after)
    side, key, jk, ts, h = _gen(before * 7 + after + grid, 30_000, grid=grid)
    total = 0
    for s0 in range(0, len(ts), 7_000):
        sl = slice(s0, s0 + 7_000)
        j.push(side[sl], key[sl], jk[sl], ts[sl], h[sl])
        exp = ref.push(side[sl], key[sl], jk[sl], ts[sl], h[sl])
        th, oh, k, t = j.drain()
        got = list(zip(th.tolist(), oh.tolist(), k.tolist(), t.tolist()))
        assert got == exp, f"batch at {s0}: {len(got)} rows vs {len(exp)}"
        total += len(exp)
    assert j.state_rows() == ref.state_rows()
    assert total > 0 or (before == 0 and after == 0)
    j.close()
    eng.close()
