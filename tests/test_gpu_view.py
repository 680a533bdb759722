"""Keyed view reads (hsg_view_get): the rows of given keys out of an op's HBM
state, which is the reference's one read of a view (SELECT ... FROM view WHERE
key = x, SelectViewPlan, hstream/src/HStream/Server/Handler.hs:277-323).

The reference everywhere is the CPU oracle's dump_state() filtered with
np.isin(key_id, keys) in (key, start, end) order, compared position by
position: the returned order is part of the contract. Every case queries
after every batch with three key sets: one present key; 64 keys drawn with
duplicates plus HSG_KEY_NONE, an id never pushed and 0xFFFFFFFE; and all
present keys in chunks of <= HSG_VIEW_MAX_KEYS, whose union must be the full
dump (no row lost or doubled)."""
import ctypes as C

import numpy as np
import pytest

import pyoracle
from hstream_amd import abi
from hstream_amd.columnar import OpSpec, Rows, alloc_rows
from util import ALL_AGG_SETS, gen_small, rows_equal

pytestmark = pytest.mark.gpu

NEVER = 0x7FFF0000  # an id no test pushes
TYPES2 = [abi.HSG_I64, abi.HSG_F64]


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need cuda:0"
    from hstream_amd.engine import Engine
    e = Engine(device=0, batch_capacity=1 << 18)
    yield e
    e.close()


@pytest.fixture(scope="module")
def xeng():
    import torch
    assert torch.cuda.is_available()
    from hstream_amd.engine import Engine, comm_unique_id
    e = Engine(device=0, rank=0, nranks=1, comm_id=comm_unique_id(), batch_capacity=1 << 18)
    yield e
    e.close()


def _take(rows: Rows, mask) -> Rows:
    return Rows(rows.key_id[mask], rows.win_start[mask], rows.win_end[mask], np.full(int(mask.sum()), -1, np.int64),
                [a[mask] for a in rows.aggs], rows.form[mask] if rows.form is not None else None)


def _expected(dump_sorted: Rows, keys) -> Rows:
    """The reference answer: the dump's rows of `keys`, in the dump's order."""
    return _take(dump_sorted, np.isin(dump_sorted.key_id, np.asarray(keys, dtype=np.uint32)))


def _concat(parts) -> Rows:
    return Rows(*[np.concatenate([getattr(p, f) for p in parts]) for f in ("key_id", "win_start", "win_end", "src_index")],
                [np.concatenate([p.aggs[j] for p in parts]) for j in range(len(parts[0].aggs))])


def check_views(g, full: Rows, f64, rng, what, extra_keys=()):
    """The three key sets against `full` (a dump in (key, start, end) order)."""
    present = np.unique(full.key_id)
    assert present.size, what
    # (a) one present key
    k = int(present[rng.integers(0, present.size)])
    got = g.view_get([k])
    assert len(got) > 0 and np.all(got.src_index == -1)
    rows_equal(got, _expected(full, [k]), f64, ordered=True, what=f"{what}: one key {k}")
    # (b) 64 keys with duplicates, and ids that match nothing
    draw = present[rng.integers(0, present.size, size=40)]
    keys = np.concatenate([draw, draw[:21], np.asarray(list(extra_keys), dtype=np.uint32),
                           np.asarray([abi.HSG_KEY_NONE, NEVER, 0xFFFFFFFE], dtype=np.uint32)])[:64 + len(extra_keys)]
    keys = keys[rng.permutation(keys.size)]
    rows_equal(g.view_get(keys), _expected(full, keys), f64, ordered=True, what=f"{what}: 64 keys")
    # (c) every present key, in chunks: the union is the dump
    parts = [g.view_get(present[i:i + abi.HSG_VIEW_MAX_KEYS]) for i in range(0, present.size, abi.HSG_VIEW_MAX_KEYS)]
    rows_equal(_concat(parts), _take(full, np.ones(len(full), bool)), f64, ordered=True, what=f"{what}: all keys")


def drive(g, o, spec, batches, rng, what, each=None):
    f64 = spec.agg_is_f64()
    wg = wo = -1
    for bi, (key, ts, cols, valid) in enumerate(batches):
        wg = g.push(key, ts, cols, valid, watermark=wg)
        wo = o.push(key, ts, cols, valid, watermark=wo)
        assert wg == wo
        if spec.emit_mode != abi.HSG_EMIT_NONE:
            g.drain()
            o.drain()
        check_views(g, o.dump_state().sorted(), f64, rng, f"{what} batch {bi}")
        if each is not None:
            each(bi)


# ---- 1. tumbling and hopping ------------------------------------------------------------------
@pytest.mark.parametrize("emit", [abi.HSG_EMIT_PER_BATCH, abi.HSG_EMIT_PER_RECORD, abi.HSG_EMIT_NONE],
                         ids=["per_batch", "per_record", "state_only"])
@pytest.mark.parametrize("kind,kw", [(abi.HSG_TUMBLING, dict(size_ms=10_000)),
                                     (abi.HSG_HOPPING, dict(size_ms=10_000, advance_ms=3_000))],
                         ids=["tumbling", "hopping"])
def test_time_windows(eng, kind, kw, emit):
    """8 regions of 4096 slots: a key's windows come from its region alone."""
    spec = OpSpec(kind, emit, col_types=TYPES2, aggs=ALL_AGG_SETS["mixed"], state_capacity=1 << 15, **kw)
    g, o = eng.op(spec), pyoracle.OracleOp(spec)
    batches = [gen_small(3000 + bi, 4000, 2000, col_types=TYPES2, span=60_000, base=5_000_000 + bi * 60_000)
               for bi in range(3)]
    drive(g, o, spec, batches, np.random.default_rng(1), f"k{kind} m{emit}")
    g.close()
    o.close()


# ---- 2. overflow rows ------------------------------------------------------------------------
def _hot_batch(rng, t0, n_hot, hot_windows, size_ms, n_bg, bg_keys):
    """tests/test_gpu_regions.py's batch: n_hot keys with a record in each of
    hot_windows consecutive windows beside n_bg one-window background records."""
    hot = np.repeat(np.arange(n_hot, dtype=np.uint32) + 1_000_000, hot_windows)
    hts = t0 + np.tile(np.arange(hot_windows, dtype=np.int64) * size_ms, n_hot) + rng.integers(0, size_ms, hot.size)
    bg = rng.integers(0, bg_keys, n_bg).astype(np.uint32)
    bts = t0 + rng.integers(0, size_ms, n_bg).astype(np.int64)
    key = np.concatenate([hot, bg])
    ts = np.concatenate([hts, bts]).astype(np.int64)
    perm = rng.permutation(key.size)
    val = rng.integers(-10**6, 10**6, key.size, dtype=np.int64)
    return key[perm], ts[perm], [val], None


def test_overflow_rows_and_wider_regions(eng):
    """3 keys x 6000 windows fill their 4096-slot regions: after batch 1 their
    rows are read from the overflow rows; batches 2 and 3 rebuild the table
    with wider regions."""
    size = 1_000
    spec = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_NONE, size_ms=size, col_types=[abi.HSG_I64], state_capacity=1 << 15,
                  aggs=[(abi.HSG_COUNT_ALL, 0), (abi.HSG_SUM, 0), (abi.HSG_MIN, 0), (abi.HSG_MAX, 0)])
    g, o = eng.op(spec), pyoracle.OracleOp(spec)
    f64 = spec.agg_is_f64()
    rng = np.random.default_rng(41)
    hot = [1_000_000, 1_000_001, 1_000_002]
    wg = wo = -1
    t = 5_000_000
    for bi in range(3):
        key, ts, cols, valid = _hot_batch(rng, t, 3, 6_000, size, 8_000, 8_000)
        t += 6_000 * size
        wg = g.push(key, ts, cols, valid, watermark=wg)
        wo = o.push(key, ts, cols, valid, watermark=wo)
        assert wg == wo
        st = g.stats()
        if bi == 0:
            assert st["overflow_rows"] > 0, st
        else:
            assert st["overflow_rebuilds"] >= 1, st
        full = o.dump_state().sorted()
        # the hot keys and some background keys
        keys = hot + [int(k) for k in key[key < 8_000][:20]]
        got = g.view_get(keys)
        assert np.isin(hot, got.key_id).all()
        rows_equal(got, _expected(full, keys), f64, ordered=True, what=f"hot + background, batch {bi}")
        check_views(g, full, f64, rng, f"overflow batch {bi}", extra_keys=hot)
    g.close()
    o.close()


# ---- 3. closed windows on the host -----------------------------------------------------------
@pytest.mark.parametrize("capacity", [256, 32], ids=["cap256", "cap32_unblocked"])
def test_spilled_windows_merge_with_resident(eng, capacity):
    """test_tumbling_spills_closed_windows's stream: a key's answer holds its HBM
    rows and its spilled rows in one ordered run. The small tables are one
    region (rbits == 0); below 64 slots the table starts unblocked."""
    spec = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_NONE, size_ms=1000, grace_ms=2000, col_types=[abi.HSG_I64],
                  aggs=ALL_AGG_SETS["full_i64"], state_capacity=capacity)
    g, o = eng.op(spec), pyoracle.OracleOp(spec)
    batches = []
    for b in range(12):
        key, ts, cols, valid = gen_small(11 + b, 20_000, 500, span=20_000, base=5_000_000 + b * 20_000, late_frac=0.01)
        batches.append((key, ts, cols[:1], valid[:1]))
    drive(g, o, spec, batches, np.random.default_rng(3), f"spill cap {capacity}")
    st = g.stats()
    assert st["spilled_rows"] > 0 and st["grow_events"] > 0, st
    g.close()
    o.close()


# ---- 4. unwindowed -----------------------------------------------------------------------------
def test_unwindowed(eng):
    """Capacity 64 growing to 20 K keys: 1000 keys give one row each with
    win_start = win_end = 0, absent keys none."""
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_BATCH, col_types=[abi.HSG_I64], aggs=ALL_AGG_SETS["full_i64"],
                  state_capacity=64)
    g, o = eng.op(spec), pyoracle.OracleOp(spec)
    rng = np.random.default_rng(4)

    def thousand(bi):
        full = o.dump_state().sorted()
        present = np.unique(full.key_id)
        keys = present[rng.permutation(present.size)[:1000]]
        got = g.view_get(np.concatenate([keys, np.arange(30_000, 30_024, dtype=np.uint32)]))
        assert len(got) == keys.size and not got.win_start.any() and not got.win_end.any()
        np.testing.assert_array_equal(got.key_id, np.sort(keys))
        assert len(g.view_get(np.arange(30_000, 30_024, dtype=np.uint32))) == 0

    batches = [gen_small(31 + b, 30_000, 20_000, span=5_000, base=5_000_000 + b * 5_000, late_frac=0.01)
               for b in range(5)]
    batches = [(k, t, c[:1], v[:1]) for k, t, c, v in batches]
    drive(g, o, spec, batches, rng, "unwindowed", each=thousand)
    assert g.stats()["grow_events"] > 0
    g.close()
    o.close()


# ---- 5. sessions ------------------------------------------------------------------------------
@pytest.mark.parametrize("nkeys", [29, 2000])
@pytest.mark.parametrize("path", ["merge", "replay"])
def test_sessions(eng, path, nkeys):
    """Gap 2 s on the merge path (per batch, no LAST) and the replay path (per
    record, LAST): 29 keys make long lists that relocate, 2000 keys many short
    ones; the arena floor makes it compact and grow between the batches."""
    from hstream_amd.engine import testing_knob
    if path == "merge":
        spec = OpSpec(abi.HSG_SESSION, abi.HSG_EMIT_PER_BATCH, gap_ms=2_000, col_types=TYPES2,
                      aggs=[(abi.HSG_COUNT_ALL, 0), (abi.HSG_SUM, 0), (abi.HSG_MIN, 1), (abi.HSG_MAX, 0),
                            (abi.HSG_AVG, 1), (abi.HSG_COUNT, 1)], state_capacity=16)
    else:
        spec = OpSpec(abi.HSG_SESSION, abi.HSG_EMIT_PER_RECORD, gap_ms=2_000, col_types=TYPES2,
                      aggs=ALL_AGG_SETS["mixed"], state_capacity=16)
    with testing_knob(abi.HSG_KNOB_SESS_ARENA_MIN, 256):
        g = eng.op(spec)
    o = pyoracle.OracleOp(spec, faithful_sessions=False)
    batches = [gen_small(5000 + bi, 4000, nkeys, col_types=TYPES2, span=400_000, base=7_000_000 + bi * 300_000)
               for bi in range(4)]
    drive(g, o, spec, batches, np.random.default_rng(5), f"sessions {path} {nkeys}")
    g.close()
    o.close()


# ---- 6. literal forms -------------------------------------------------------------------------
@pytest.mark.parametrize("kind,kw", [(abi.HSG_TUMBLING, dict(size_ms=10_000)), (abi.HSG_SESSION, dict(gap_ms=2_000)),
                                     (abi.HSG_UNWINDOWED, {})], ids=["tumbling", "session", "unwindowed"])
def test_literal_forms(eng, kind, kw):
    """form and values equal those of the same rows in the GPU's own dump
    (the oracle keeps no forms)."""
    aggs = [(abi.HSG_SUM, 0), (abi.HSG_MIN, 1), (abi.HSG_MAX, 1), (abi.HSG_COUNT_ALL, 0)]
    if kind != abi.HSG_SESSION:
        aggs.append((abi.HSG_LAST, 0))
    spec = OpSpec(kind, abi.HSG_EMIT_PER_BATCH, col_types=TYPES2, aggs=aggs, flags=abi.HSG_OPF_LITERAL_FORMS,
                  state_capacity=1 << 15, **kw)
    g = eng.op(spec)
    rng = np.random.default_rng(6)
    wm = -1
    for bi in range(3):
        key, ts, cols, valid = gen_small(6000 + bi, 4000, 300, col_types=TYPES2, span=60_000,
                                         base=5_000_000 + bi * 60_000)
        # bit 1 of a valid byte: the value's literal was decimal
        valid = [np.where((v != 0) & (rng.random(v.size) < 0.4), 3, v).astype(np.uint8) for v in valid]
        wm = g.push(key, ts, cols, valid, watermark=wm)
        g.drain()
        full = g.dump_state().sorted()
        assert full.form is not None and full.form.any()
        present = np.unique(full.key_id)
        keys = np.concatenate([present[rng.integers(0, present.size, size=50)], [NEVER]]).astype(np.uint32)
        got, exp = g.view_get(keys), _expected(full, keys)
        rows_equal(got, exp, spec.agg_is_f64(), ordered=True, exact_f64=[True] * len(aggs), what=f"forms batch {bi}")
        np.testing.assert_array_equal(got.form, exp.form)
    g.close()


# ---- 7. exchange path at one rank ----------------------------------------------------------------
@pytest.mark.parametrize("kind,kw", [(abi.HSG_TUMBLING, dict(size_ms=10_000)), (abi.HSG_SESSION, dict(gap_ms=2_000))],
                         ids=["tumbling", "session"])
def test_exchange_path_owner_bits(xeng, kind, kw):
    """An engine with a communicator and 4 owner regions (bshift / hshift != 0):
    the regions and home slots skip the owner bits."""
    from hstream_amd.engine import testing_knob
    spec = OpSpec(kind, abi.HSG_EMIT_PER_BATCH, col_types=TYPES2, state_capacity=1 << 15,
                  aggs=[(abi.HSG_COUNT_ALL, 0), (abi.HSG_SUM, 0), (abi.HSG_MIN, 1), (abi.HSG_MAX, 0)], **kw)
    with testing_knob(abi.HSG_KNOB_XPART_LOG2, 2):
        g = xeng.op(spec)
    o = pyoracle.OracleOp(spec, faithful_sessions=False) if kind == abi.HSG_SESSION else pyoracle.OracleOp(spec)
    batches = [gen_small(7000 + bi, 4000, 2000, col_types=TYPES2, span=60_000, base=5_000_000 + bi * 60_000,
                         very_late=False) for bi in range(3)]
    drive(g, o, spec, batches, np.random.default_rng(7), f"exchange k{kind}")
    assert g.stats()["records_owned"] > 0
    g.close()
    o.close()


# ---- 8. contract -------------------------------------------------------------------------------
def _raw_view(g, keys, rows, n_keys=None):
    keys = np.ascontiguousarray(keys, dtype=np.uint32) if keys is not None else None
    got = C.c_uint64(0xDEAD)
    rc = g._lib.hsg_view_get(g._h, keys.ctypes.data if keys is not None else None,
                             n_keys if n_keys is not None else keys.size, C.byref(rows), C.byref(got))
    return rc, got.value


def test_contract(eng):
    spec = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=10_000, col_types=TYPES2,
                  aggs=ALL_AGG_SETS["mixed"], state_capacity=1 << 15)
    g, o = eng.op(spec), pyoracle.OracleOp(spec)
    f64 = spec.agg_is_f64()
    batches = [gen_small(8000 + bi, 4000, 500, col_types=TYPES2, span=60_000, base=5_000_000 + bi * 60_000)
               for bi in range(3)]
    wg = wo = -1
    for key, ts, cols, valid in batches[:2]:
        wg = g.push(key, ts, cols, valid, watermark=wg)
        wo = o.push(key, ts, cols, valid, watermark=wo)
        g.drain(), o.drain()
    key, ts, cols, valid = batches[2]
    wg = g.push(key, ts, cols, valid, watermark=wg)
    wo = o.push(key, ts, cols, valid, watermark=wo)
    full = o.dump_state().sorted()
    keys = np.unique(full.key_id)[:200]
    exp = _expected(full, keys)
    need = len(exp)
    assert need > 200

    # reads change nothing: pending rows, the drain and the dump that follow, the stats
    pend, st0 = g.pending(), g.stats()
    assert pend > 0
    # capacity too small: the count needed, the caller's arrays untouched, then a retry with that count
    rows, arrs, keep = alloc_rows(need - 1, f64)
    for a in [arrs.key_id, arrs.win_start, arrs.win_end, arrs.src_index] + arrs.aggs:
        a.view(np.uint8)[:] = 0xA5
    rc, n = _raw_view(g, keys, rows)
    assert rc == abi.HSG_E_CAPACITY and n == need
    for a in [arrs.key_id, arrs.win_start, arrs.win_end, arrs.src_index] + arrs.aggs:
        assert (a.view(np.uint8) == 0xA5).all()
    rows, arrs, keep = alloc_rows(need, f64)
    rc, n = _raw_view(g, keys, rows)
    assert rc == abi.HSG_OK and n == need
    rows_equal(arrs, exp, f64, ordered=True, what="retry with the reported count")
    # the binding's own retry
    rows_equal(g.view_get(keys, capacity=1), exp, f64, ordered=True, what="view_get retry")
    # arguments
    rc, n = _raw_view(g, keys[:0], rows)
    assert rc == abi.HSG_OK and n == 0
    rc, _ = _raw_view(g, np.arange(1025), rows)
    assert rc == abi.HSG_E_INVALID
    rc, _ = _raw_view(g, None, rows, n_keys=3)
    assert rc == abi.HSG_E_INVALID
    rc, n = _raw_view(g, None, rows, n_keys=0)
    assert rc == abi.HSG_OK and n == 0
    bad = abi.hsg_rows(capacity=need, mem=abi.HSG_MEM_HOST, n_aggs=len(f64) + 1)
    rc, _ = _raw_view(g, keys, bad)
    assert rc == abi.HSG_E_INVALID  # check_rows, as for a dump

    # a device-memory out equals the host-memory answer
    import torch
    dk = torch.empty(need, dtype=torch.int32, device="cuda")
    dws, dwe, dsrc = (torch.empty(need, dtype=torch.int64, device="cuda") for _ in range(3))
    da = [torch.empty(need, dtype=torch.float64 if f else torch.int64, device="cuda") for f in f64]
    ap = (C.c_void_p * len(da))(*[a.data_ptr() for a in da])
    drows = abi.hsg_rows(capacity=need, mem=abi.HSG_MEM_DEVICE, n_aggs=len(da), key_id=dk.data_ptr(),
                         win_start=dws.data_ptr(), win_end=dwe.data_ptr(), src_index=dsrc.data_ptr(),
                         aggs=C.cast(ap, C.POINTER(C.c_void_p)))
    rc, n = _raw_view(g, keys, drows)
    assert rc == abi.HSG_OK and n == need
    torch.cuda.synchronize()
    dev = Rows(dk.cpu().numpy().view(np.uint32), dws.cpu().numpy(), dwe.cpu().numpy(), dsrc.cpu().numpy(),
               [a.cpu().numpy() for a in da])
    host = g.view_get(keys)
    rows_equal(dev, host, f64, ordered=True, exact_f64=[True] * len(f64), what="device out")

    assert g.pending() == pend
    st1 = g.stats()
    assert st1 == st0, {k: (st0[k], st1[k]) for k in st0 if st0[k] != st1[k]}
    rows_equal(g.drain(), o.drain(), f64, what="drain after the reads")
    rows_equal(g.dump_state(), o.dump_state(), f64, what="dump after the reads")

    # after reset: nothing
    g.reset()
    assert len(g.view_get(keys)) == 0
    g.close()
    o.close()


@pytest.mark.parametrize("native", [False, True], ids=["python_dict", "native_dict"])
def test_dsl_table_get_and_select_view(eng, native):
    """Table.get / Table.select_view (SelectViewPlan, Handler.hs:277-323) over
    the three store kinds, against the same answer shaped from Table.dump; a
    key never seen gives the empty answer and does not grow the dictionary."""
    from hstream_amd import ingest, processing as P
    rng = np.random.default_rng(12)
    recs = [{"timestamp": int(1000 * i + rng.integers(0, 900)),
             "value": {"key": ["a", "b", 1, {"k": [1, 2]}][int(rng.integers(0, 4))], "v": int(rng.integers(-50, 50))}}
            for i in range(300)]
    mk = (lambda: P.Materialized(keys=ingest.KeyDict())) if native else P.Materialized
    tables = [
        P.groupBy(eng, "key").timeWindowedBy(P.mkHoppingWindow(3000, 1000)).aggregate(
            [P.COUNT_ALL("n"), P.SUM("v", "s")], mk()),
        P.groupBy(eng, "key").sessionWindowedBy(P.mkSessionWindows(1500)).aggregate(
            [P.COUNT_ALL("n"), P.SUM("v", "s")], mk(), emit=abi.HSG_EMIT_PER_BATCH),
        P.groupBy(eng, "key").aggregate([P.COUNT_ALL("n"), P.MAX("v", "m")], mk()),
    ]
    for t in tables:
        t.process(recs)
        session = t.spec.window_kind == abi.HSG_SESSION
        dump = t.dump()
        n_keys = len(t.mat.keys)
        for key in ("a", 1.0, {"k": [1.0, 2]}):
            kid = t.mat.keys.find(key)
            mine = [(k, v) for k, v in dump if t.mat.keys.find(k.twkKey if t.windowed else k) == kid]
            assert mine and t.get(key) == mine
            exp = P.select_view_result(mine, t.windowed, session, t.spec.size_ms)
            got = t.select_view(key)
            assert got == exp and (list(got) == list(exp) if t.windowed else True)
            if t.windowed:
                assert len(got) == len(mine)
        assert t.get("nobody") == []
        assert t.select_view("nobody") == ({} if t.windowed else None)
        assert len(t.mat.keys) == n_keys
        t.close()


def test_after_async_pushes(eng):
    """A call right after three push_async batches waits for them: it equals
    the oracle after those three."""
    spec = OpSpec(abi.HSG_HOPPING, abi.HSG_EMIT_NONE, size_ms=10_000, advance_ms=5_000, col_types=TYPES2,
                  aggs=ALL_AGG_SETS["mixed"], state_capacity=1 << 15)
    g, o = eng.op(spec), pyoracle.OracleOp(spec)
    batches = [gen_small(9000 + bi, 4000, 500, col_types=TYPES2, span=60_000, base=5_000_000 + bi * 60_000)
               for bi in range(3)]
    wm = C.c_int64(-1)
    wo = -1
    rcs = []
    for key, ts, cols, valid in batches:
        g.push_async(key, ts, cols, valid, watermark=wm, done=rcs.append)
        wo = o.push(key, ts, cols, valid, watermark=wo)
    full = o.dump_state().sorted()
    keys = np.unique(full.key_id)[:300]
    rows_equal(g.view_get(keys), _expected(full, keys), spec.agg_is_f64(), ordered=True, what="after push_async")
    g.wait()
    assert rcs == [abi.HSG_OK] * 3 and wm.value == wo
    g.close()
    o.close()
