"""Stream-table join (hsg_table_join): the keys of a poll batch probed against
an unwindowed op's HBM table, which is the reference's Stream.joinTable /
joinTableProcessor (hstream-processing/src/HStream/Processing/Stream.hs:
302-344): ksGet per stream record, a forward on a hit, nothing on a miss.

The table's state is driven beside the CPU oracle and compared with it. The
expected join is then a host dictionary join over the op's own dump_state():
one row per probe record whose key has a row, in arrival order, src_index =
the record's index. Every column is compared bit for bit, f64 columns as
their int64 images: the dump and the join render a row with the same
out_value, so no tolerance is involved."""
import ctypes as C

import numpy as np
import pytest

import pyoracle
from hstream_amd import abi
from hstream_amd.columnar import OpSpec, Rows, alloc_rows
from util import ALL_AGG_SETS, gen_small, rows_equal

pytestmark = pytest.mark.gpu

NONE = abi.HSG_KEY_NONE
TYPES2 = [abi.HSG_I64, abi.HSG_F64]
BATCH_CAP = 1 << 18


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need cuda:0"
    from hstream_amd.engine import Engine
    e = Engine(device=0, batch_capacity=BATCH_CAP)
    yield e
    e.close()


@pytest.fixture(scope="module")
def xeng():
    import torch
    assert torch.cuda.is_available()
    from hstream_amd.engine import Engine, comm_unique_id
    e = Engine(device=0, rank=0, nranks=1, comm_id=comm_unique_id(), batch_capacity=BATCH_CAP)
    yield e
    e.close()


@pytest.fixture(scope="module")
def tile():
    from hstream_amd.engine import table_join_tile
    return table_join_tile()


# ---- the reference answer ------------------------------------------------------------------------
def expected_join(dump: Rows, keys) -> Rows:
    """Host dictionary join: dump = the table's dump_state(), keys = the probe."""
    keys = np.asarray(keys, dtype=np.uint32)
    row_of = {int(k): i for i, k in enumerate(dump.key_id)}
    assert len(row_of) == len(dump), "an unwindowed dump has one row per key"
    src = [i for i, k in enumerate(keys) if int(k) in row_of]
    at = np.asarray([row_of[int(keys[i])] for i in src], dtype=np.int64)
    return Rows(dump.key_id[at], dump.win_start[at], dump.win_end[at], np.asarray(src, dtype=np.int64),
                [a[at] for a in dump.aggs], dump.form[at] if dump.form is not None else None)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_rows(got: Rows, exp: Rows, what=""):
    """Every column, position by position, bit for bit."""
    assert len(got) == len(exp), f"{what}: {len(got)} rows, expected {len(exp)}"
    np.testing.assert_array_equal(got.key_id, exp.key_id, err_msg=f"{what}: key_id")
    assert not got.win_start.any() and not got.win_end.any(), f"{what}: win_start = win_end = 0"
    np.testing.assert_array_equal(got.src_index, exp.src_index, err_msg=f"{what}: src_index")
    assert len(got.aggs) == len(exp.aggs)
    for j, (x, y) in enumerate(zip(got.aggs, exp.aggs)):
        assert x.dtype == y.dtype
        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=f"{what}: agg {j}")
    if exp.form is not None:
        np.testing.assert_array_equal(got.form, exp.form, err_msg=f"{what}: form")


def drive(g, o, spec, batches, what):
    """Push the batches into the op and the oracle; the states agree."""
    wg = wo = -1
    for key, ts, cols, valid in batches:
        wg = g.push(key, ts, cols, valid, watermark=wg)
        wo = o.push(key, ts, cols, valid, watermark=wo)
        assert wg == wo
        if spec.emit_mode != abi.HSG_EMIT_NONE:
            g.drain()
            o.drain()
    rows_equal(g.dump_state(), o.dump_state(), spec.agg_is_f64(), what=f"{what}: state")
    return wg


# ---- 1. tile and wave edges ----------------------------------------------------------------------
N_PRESENT = 3000   # keys 0 .. 2999 have a row
ABSENT0 = 100_000  # ids from here on were never pushed


@pytest.fixture(scope="module")
def small_table(eng):
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_NONE, col_types=TYPES2, aggs=ALL_AGG_SETS["mixed"],
                  state_capacity=1 << 13)
    g, o = eng.op(spec), pyoracle.OracleOp(spec)
    key, ts, cols, valid = gen_small(101, 12_000, N_PRESENT, col_types=TYPES2, none_frac=0.0)
    key[:N_PRESENT] = np.arange(N_PRESENT, dtype=np.uint32)  # every key at least once
    drive(g, o, spec, [(key, ts, cols, valid)], "small table")
    dump = g.dump_state()
    assert len(dump) == N_PRESENT
    o.close()
    yield g, dump
    g.close()


def _pattern(name, n, rng):
    hit = rng.integers(0, N_PRESENT, n).astype(np.uint32)
    miss = (ABSENT0 + rng.integers(0, 50_000, n)).astype(np.uint32)
    i = np.arange(n)
    if name == "all_hit":
        m = np.ones(n, bool)
    elif name == "all_miss":
        m = np.zeros(n, bool)
    elif name == "alternate":
        m = i % 2 == 0
    elif name == "lane0_lane63":
        m = (i % 64 == 0) | (i % 64 == 63)
    elif name == "last_only":
        m = i == n - 1
    return np.where(m, hit, miss).astype(np.uint32), int(m.sum())


@pytest.mark.parametrize("pattern", ["all_hit", "all_miss", "alternate", "lane0_lane63", "last_only"])
def test_tile_and_wave_edges(small_table, tile, pattern):
    g, dump = small_table
    rng = np.random.default_rng(7)
    for n in (1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 3):
        keys, hits = _pattern(pattern, n, rng)
        got = g.table_join(keys)
        assert len(got) == hits, (pattern, n)
        same_rows(got, expected_join(dump, keys), f"{pattern} n={n}")


# ---- 2. probing ------------------------------------------------------------------------------------
def test_grown_table_misses_and_duplicates(eng):
    """Capacity 64 growing to 20 K keys: present keys, ids never pushed,
    HSG_KEY_NONE and one key 5000 times."""
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_BATCH, col_types=[abi.HSG_I64], aggs=ALL_AGG_SETS["full_i64"],
                  state_capacity=64)
    g, o = eng.op(spec), pyoracle.OracleOp(spec)
    batches = [gen_small(31 + b, 30_000, 20_000, span=5_000, base=5_000_000 + b * 5_000, late_frac=0.01)
               for b in range(3)]
    batches = [(k, t, c[:1], v[:1]) for k, t, c, v in batches]
    drive(g, o, spec, batches, "grown")
    assert g.stats()["grow_events"] > 0
    dump = g.dump_state()
    present = np.unique(dump.key_id)
    rng = np.random.default_rng(2)
    dup = np.full(5_000, present[17], dtype=np.uint32)
    keys = np.concatenate([present[rng.integers(0, present.size, 9_000)], dup,
                           np.arange(30_000, 33_000, dtype=np.uint32), np.full(500, NONE, dtype=np.uint32),
                           np.asarray([0xFFFFFFFE, 0x7FFF0000], dtype=np.uint32)]).astype(np.uint32)
    keys = keys[rng.permutation(keys.size)]
    got = g.table_join(keys)
    assert len(got) == 14_000 and int((got.key_id == present[17]).sum()) >= 5_000
    same_rows(got, expected_join(dump, keys), "grown table")
    assert len(g.table_join(np.arange(30_000, 30_100, dtype=np.uint32))) == 0
    assert len(g.table_join(np.full(70, NONE, dtype=np.uint32))) == 0
    g.close()
    o.close()


def _fmix32(h):
    h = np.asarray(h, dtype=np.uint64)
    m = np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h


def _region_of(keys, rbits):
    """The table region of a key (hsg_internal.h key_hash / tw_region_base with
    no owner bits): the top rbits bits of fmix32(key * 0x9E3779B1 + 0x632BE59B)."""
    k = np.asarray(keys, dtype=np.uint64)
    h = _fmix32((k * np.uint64(0x9E3779B1) + np.uint64(0x632BE59B)) & np.uint64(0xFFFFFFFF))
    return (h >> np.uint64(32 - rbits)).astype(np.int64)


def test_overflow_rows(eng):
    """A region that drew more than its share of keys, as tests/
    test_gpu_regions.py fills one: state_capacity 2^14 is a table of 2^15 slots,
    8 regions of 4096; 5000 keys of region 0 beside 2000 others leave the table
    far below the load that grows it, and region 0's last keys in the overflow
    rows, where the probe's continuation finds them."""
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_NONE, col_types=[abi.HSG_I64], state_capacity=1 << 14,
                  aggs=[(abi.HSG_COUNT_ALL, 0), (abi.HSG_SUM, 0), (abi.HSG_MIN, 0), (abi.HSG_MAX, 0)])
    g, o = eng.op(spec), pyoracle.OracleOp(spec)
    ids = np.arange(60_000, dtype=np.uint32)
    reg = _region_of(ids, 3)
    hot, other = ids[reg == 0][:5_000], ids[reg != 0][:2_000]
    assert hot.size == 5_000
    rng = np.random.default_rng(5)
    key = np.concatenate([hot, other, hot[:1_000]])
    key = key[rng.permutation(key.size)]
    ts = (5_000_000 + np.arange(key.size)).astype(np.int64)
    val = rng.integers(-10**6, 10**6, key.size, dtype=np.int64)
    drive(g, o, spec, [(key, ts, [val], None)], "overflow")
    st = g.stats()
    assert st["table_slots"] == 1 << 15 and st["grow_events"] == 0, st
    assert st["overflow_rows"] > 0, {k: st[k] for k in ("overflow_rows", "table_slots", "state_rows")}
    dump = g.dump_state()
    assert len(dump) == 7_000
    absent = ids[reg == 0][5_000:5_600]  # same region, never pushed: the probe runs the full region and the overflow
    keys = np.concatenate([hot, other, absent, hot[::3]])
    keys = keys[rng.permutation(keys.size)]
    got = g.table_join(keys)
    assert g.stats()["overflow_rows"] > 0  # (still there at probe time: no push since)
    assert len(got) == hot.size + other.size + hot[::3].size
    same_rows(got, expected_join(dump, keys), "overflow rows")
    g.close()
    o.close()


# ---- 3. outputs -------------------------------------------------------------------------------------
OUTPUT_SETS = [("count", [abi.HSG_I64], ALL_AGG_SETS["count"]),
               ("full_i64", [abi.HSG_I64], ALL_AGG_SETS["full_i64"]),
               ("full_f64", [abi.HSG_F64], ALL_AGG_SETS["full_i64"]),
               ("mixed", TYPES2, ALL_AGG_SETS["mixed"])]


@pytest.mark.parametrize("name,types,aggs", OUTPUT_SETS, ids=[s[0] for s in OUTPUT_SETS])
def test_every_output_kind(eng, name, types, aggs):
    """Keys divisible by 7 never carry a field: COUNT(col) = 0, AVG = NaN."""
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_NONE, col_types=types, aggs=aggs, state_capacity=1 << 13)
    g, o = eng.op(spec), pyoracle.OracleOp(spec)
    batches = []
    for b in range(2):
        key, ts, cols, valid = gen_small(300 + b, 6_000, 1_500, col_types=types, base=5_000_000 + b * 200_000)
        valid = [np.where(key % 7 == 0, 0, v).astype(np.uint8) for v in valid]
        batches.append((key, ts, cols, valid))
    drive(g, o, spec, batches, name)
    dump = g.dump_state()
    if any(k == abi.HSG_AVG for k, _ in aggs):
        j = [k for k, _ in aggs].index(abi.HSG_AVG)
        assert np.isnan(dump.aggs[j]).any(), "no AVG over COUNT(col) = 0 in the state"
    rng = np.random.default_rng(3)
    keys = np.concatenate([rng.integers(0, 1_500, 2_500), np.arange(0, 1_500, 7), [NONE, 5_000]]).astype(np.uint32)
    keys = keys[rng.permutation(keys.size)]
    got = g.table_join(keys)
    assert len(got) > 2_000
    same_rows(got, expected_join(dump, keys), name)
    g.close()
    o.close()


def test_literal_forms(eng):
    """form as view_get returns it for the same key (the oracle keeps no forms)."""
    aggs = [(abi.HSG_SUM, 0), (abi.HSG_MIN, 1), (abi.HSG_MAX, 1), (abi.HSG_COUNT_ALL, 0), (abi.HSG_LAST, 0)]
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_BATCH, col_types=TYPES2, aggs=aggs,
                  flags=abi.HSG_OPF_LITERAL_FORMS, state_capacity=1 << 13)
    g = eng.op(spec)
    rng = np.random.default_rng(6)
    wm = -1
    for bi in range(2):
        key, ts, cols, valid = gen_small(6000 + bi, 4000, 300, col_types=TYPES2, span=60_000,
                                         base=5_000_000 + bi * 60_000)
        # bit 1 of a valid byte: the value's literal was decimal
        valid = [np.where((v != 0) & (rng.random(v.size) < 0.4), 3, v).astype(np.uint8) for v in valid]
        wm = g.push(key, ts, cols, valid, watermark=wm)
        g.drain()
    dump = g.dump_state()
    assert dump.form is not None and dump.form.any()
    present = np.unique(dump.key_id)
    keys = np.concatenate([present[rng.integers(0, present.size, 700)], [0x7FFF0000, NONE]]).astype(np.uint32)
    got = g.table_join(keys)
    assert got.form is not None and len(got) == 700
    same_rows(got, expected_join(dump, keys), "forms")
    uniq = np.unique(keys[:700])[:abi.HSG_VIEW_MAX_KEYS]
    view = g.view_get(uniq)  # (sorted by key)
    form_of = dict(zip(view.key_id.tolist(), view.form.tolist()))
    assert [form_of[k] for k in got.key_id.tolist()] == got.form.tolist()
    g.close()


# ---- 4. exchange path at one rank ------------------------------------------------------------------
def test_exchange_path_owner_bits(xeng):
    """An engine with a communicator and 4 owner regions (bshift != 0): the
    region base skips the owner bits; same answers."""
    from hstream_amd.engine import testing_knob
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_BATCH, col_types=TYPES2, state_capacity=1 << 15,
                  aggs=[(abi.HSG_COUNT_ALL, 0), (abi.HSG_SUM, 0), (abi.HSG_MIN, 1), (abi.HSG_MAX, 0)])
    with testing_knob(abi.HSG_KNOB_XPART_LOG2, 2):
        g = xeng.op(spec)
    o = pyoracle.OracleOp(spec)
    batches = [gen_small(7000 + bi, 8_000, 6_000, col_types=TYPES2, span=60_000, base=5_000_000 + bi * 60_000,
                         very_late=False) for bi in range(2)]
    drive(g, o, spec, batches, "exchange")
    assert g.stats()["records_owned"] > 0
    dump = g.dump_state()
    rng = np.random.default_rng(8)
    keys = rng.integers(0, 9_000, 5_000).astype(np.uint32)
    got = g.table_join(keys)
    assert 0 < len(got) < keys.size
    same_rows(got, expected_join(dump, keys), "exchange path")
    g.close()
    o.close()


# ---- 5. memory kinds ---------------------------------------------------------------------------------
def _device_rows(torch, cap, f64):
    dk = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    dws, dwe, dsrc = (torch.full((cap,), -7, dtype=torch.int64, device="cuda") for _ in range(3))
    da = [torch.zeros(cap, dtype=torch.float64 if f else torch.int64, device="cuda") for f in f64]
    ap = (C.c_void_p * max(1, len(da)))(*[a.data_ptr() for a in da])
    rows = abi.hsg_rows(capacity=cap, mem=abi.HSG_MEM_DEVICE, n_aggs=len(da), key_id=dk.data_ptr(),
                        win_start=dws.data_ptr(), win_end=dwe.data_ptr(), src_index=dsrc.data_ptr(),
                        aggs=C.cast(ap, C.POINTER(C.c_void_p)))

    def to_host(n):
        torch.cuda.synchronize()
        return Rows(dk[:n].cpu().numpy().view(np.uint32), dws[:n].cpu().numpy(), dwe[:n].cpu().numpy(),
                    dsrc[:n].cpu().numpy(), [a[:n].cpu().numpy() for a in da])

    return rows, to_host, (dk, dws, dwe, dsrc, da, ap)


def test_memory_kinds(small_table, tile):
    import torch
    g, dump = small_table
    f64 = g.spec.agg_is_f64()
    rng = np.random.default_rng(9)
    n = 3 * tile + 17
    keys, _ = _pattern("alternate", n, rng)
    exp = expected_join(dump, keys)
    need = len(exp)
    # host keys -> host out
    same_rows(g.table_join(keys), exp, "host -> host")
    # device keys written on a producer stream, ready_event recorded there -> device out, in place
    side = torch.cuda.Stream()
    dkeys = torch.zeros(n, dtype=torch.int32, device="cuda")
    hkeys = torch.from_numpy(keys.view(np.int32)).pin_memory()
    with torch.cuda.stream(side):
        torch.cuda._sleep(5_000_000)  # keep the copy behind a kernel: only the event orders the read
        dkeys.copy_(hkeys, non_blocking=True)
        ready = torch.cuda.Event()
        ready.record(side)
    rows, to_host, keep = _device_rows(torch, need + 5, f64)
    rc, got = g.table_join_into(dkeys, rows, ready_event=C.c_void_p(ready.cuda_event))
    assert rc == abi.HSG_OK and got == need
    same_rows(to_host(need), exp, "device -> device")
    tail = keep[0][need:].cpu().numpy()
    assert (tail == -1).all(), "rows past the matches were written"
    # mixed
    rows, to_host, keep = _device_rows(torch, need, f64)
    rc, got = g.table_join_into(keys, rows)
    assert rc == abi.HSG_OK and got == need
    same_rows(to_host(need), exp, "host -> device")
    torch.cuda.synchronize()
    same_rows(g.table_join(dkeys), exp, "device -> host")


# ---- 6. contract ----------------------------------------------------------------------------------------
def _raw(g, probe, rows):
    got = C.c_uint64(0xDEAD)
    rc = g._lib.hsg_table_join(g._h, C.byref(probe) if probe is not None else None,
                               C.byref(rows) if rows is not None else None, C.byref(got))
    return rc, got.value


def test_contract_reads_only_and_capacity(eng):
    from hstream_amd.engine import make_probe
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_PER_BATCH, col_types=TYPES2, aggs=ALL_AGG_SETS["mixed"],
                  state_capacity=1 << 13)
    g, o = eng.op(spec), pyoracle.OracleOp(spec)
    f64 = spec.agg_is_f64()
    batches = [gen_small(8000 + bi, 4000, 500, col_types=TYPES2, span=60_000, base=5_000_000 + bi * 60_000)
               for bi in range(3)]
    wg = wo = -1
    for key, ts, cols, valid in batches[:2]:
        wg = g.push(key, ts, cols, valid, watermark=wg)
        wo = o.push(key, ts, cols, valid, watermark=wo)
    assert wg == wo
    dump0, pend0, st0 = g.dump_state(), g.pending(), g.stats()
    assert pend0 > 0
    rng = np.random.default_rng(10)
    keys = rng.integers(0, 1_000, 3_000).astype(np.uint32)
    exp = expected_join(dump0, keys)
    need = len(exp)
    assert 0 < need < keys.size
    probe, keep = make_probe(keys)

    # capacity too small: the count needed, the caller's arrays untouched, then a retry with that count
    rows, arrs, keep_r = alloc_rows(need - 1, f64)
    cols_ = [arrs.key_id, arrs.win_start, arrs.win_end, arrs.src_index] + arrs.aggs
    for a in cols_:
        a.view(np.uint8)[:] = 0xA5
    rc, n = _raw(g, probe, rows)
    assert rc == abi.HSG_E_CAPACITY and n == need
    for a in cols_:
        assert (a.view(np.uint8) == 0xA5).all()
    rows, arrs, keep_r = alloc_rows(need, f64)
    rc, n = _raw(g, probe, rows)
    assert rc == abi.HSG_OK and n == need
    same_rows(arrs, exp, "retry with the reported count")
    same_rows(g.table_join(keys, capacity=1), exp, "the binding's own retry")
    # repeated equal-sized joins (the op's scratch reused) give equal results
    for _ in range(3):
        same_rows(g.table_join(keys), exp, "repeated")

    # arguments
    rc, n = _raw(g, make_probe(keys[:0])[0], rows)
    assert rc == abi.HSG_OK and n == 0
    assert len(g.table_join([])) == 0
    rc, _ = _raw(g, None, rows)
    assert rc == abi.HSG_E_INVALID
    rc, _ = _raw(g, abi.hsg_probe(n=3, mem=abi.HSG_MEM_HOST, key_id=None), rows)
    assert rc == abi.HSG_E_INVALID
    rc, _ = _raw(g, abi.hsg_probe(n=keys.size, mem=abi.HSG_MEM_HOST, reserved=1, key_id=keys.ctypes.data), rows)
    assert rc == abi.HSG_E_INVALID
    big = np.zeros(BATCH_CAP + 1, dtype=np.uint32)
    rc, _ = _raw(g, make_probe(big)[0], rows)
    assert rc == abi.HSG_E_INVALID
    bad = abi.hsg_rows(capacity=need, mem=abi.HSG_MEM_HOST, n_aggs=len(f64) + 1)
    rc, _ = _raw(g, probe, bad)
    assert rc == abi.HSG_E_INVALID  # check_rows, as for a dump

    # nothing changed: state, pending rows, stats, and the next push's watermark
    assert g.pending() == pend0
    st1 = g.stats()
    assert st1 == st0, {k: (st0[k], st1[k]) for k in st0 if st0[k] != st1[k]}
    same_dump = g.dump_state()
    for x, y in zip([same_dump.key_id] + same_dump.aggs, [dump0.key_id] + dump0.aggs):
        np.testing.assert_array_equal(_bits(x), _bits(y))
    key, ts, cols, valid = batches[2]
    wg = g.push(key, ts, cols, valid, watermark=wg)
    wo = o.push(key, ts, cols, valid, watermark=wo)
    assert wg == wo
    rows_equal(g.drain(), o.drain(), f64, what="drain after the joins")
    rows_equal(g.dump_state(), o.dump_state(), f64, what="dump after the joins")

    # after reset every probe misses
    g.reset()
    assert len(g.table_join(keys)) == 0
    g.close()
    o.close()


@pytest.mark.parametrize("kind,kw", [(abi.HSG_TUMBLING, dict(size_ms=10_000)),
                                     (abi.HSG_HOPPING, dict(size_ms=10_000, advance_ms=5_000)),
                                     (abi.HSG_SESSION, dict(gap_ms=2_000))], ids=["tumbling", "hopping", "session"])
def test_only_unwindowed_ops_are_tables(eng, kind, kw):
    from hstream_amd.engine import make_probe
    spec = OpSpec(kind, abi.HSG_EMIT_PER_BATCH, col_types=[abi.HSG_I64], aggs=ALL_AGG_SETS["count"], **kw)
    g = eng.op(spec)
    keys = np.arange(10, dtype=np.uint32)
    g.push(keys, np.arange(10, dtype=np.int64) + 5_000_000, [np.zeros(10, np.int64)], None)
    rows, arrs, keep = alloc_rows(16, spec.agg_is_f64())
    rc, _ = _raw(g, make_probe(keys)[0], rows)
    assert rc == abi.HSG_E_INVALID
    with pytest.raises(abi.HStreamGpuError, match="unwindowed"):
        g.table_join(keys)
    g.close()


def test_after_async_pushes(eng):
    """A join right after three push_async batches waits for them."""
    spec = OpSpec(abi.HSG_UNWINDOWED, abi.HSG_EMIT_NONE, col_types=TYPES2, aggs=ALL_AGG_SETS["mixed"],
                  state_capacity=1 << 13)
    g, o = eng.op(spec), pyoracle.OracleOp(spec)
    batches = [gen_small(9000 + bi, 4000, 300 * (bi + 1), col_types=TYPES2, span=60_000, base=5_000_000 + bi * 60_000)
               for bi in range(3)]
    wm = C.c_int64(-1)
    wo = -1
    rcs = []
    for key, ts, cols, valid in batches:
        g.push_async(key, ts, cols, valid, watermark=wm, done=rcs.append)
        wo = o.push(key, ts, cols, valid, watermark=wo)
    keys = np.arange(1_000, dtype=np.uint32)
    got = g.table_join(keys)
    g.wait()
    assert rcs == [abi.HSG_OK] * 3 and wm.value == wo
    rows_equal(g.dump_state(), o.dump_state(), spec.agg_is_f64(), what="state after push_async")
    dump = g.dump_state()
    assert (dump.key_id >= 600).any(), "the third batch's keys are in the state"
    same_rows(got, expected_join(dump, keys), "after push_async")
    g.close()
    o.close()


# ---- 7. DSL ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("native", [False, True], ids=["python_dict", "native_dict"])
def test_dsl_table_and_join_table(eng, native):
    """processing.table + joinTable against tableStoreProcessor /
    joinTableProcessor (Stream.hs:118-129, 334-344) restated here: a dict that
    takes each table record's value whole, and a lookup per stream record.
    Every table record carries every field, so LAST per field is the stored
    object. Arrival order: table batch, stream batch, table batch, stream batch."""
    from hstream_amd import ingest, processing as P
    rng = np.random.default_rng(12)
    names = ["a", "b", 1, {"k": [1, 2]}, "c", 2.5]

    def table_batch(t0, n):
        return [{"timestamp": t0 + i, "value": {"key": names[int(rng.integers(0, 4 + (t0 > 0) * 1))],
                                                "price": int(rng.integers(-50, 50)),
                                                "w": float(np.round(rng.uniform(-9, 9), 2))}} for i in range(n)]

    def stream_batch(t0, n):
        recs = [{"timestamp": t0 + i, "value": {"key": names[int(rng.integers(0, len(names)))], "qty": i}}
                for i in range(n)]
        recs[3] = {"timestamp": t0 + 3, "value": {"qty": -1}}            # no key field
        recs[5] = {"timestamp": t0 + 5, "value": {"key": "nobody", "qty": -2}}  # a key the table never saw
        return recs

    def joiner(v1, v2):
        return {"qty": v1["qty"], "price": v2["price"], "w": v2["w"]}

    mat = P.Materialized(keys=ingest.KeyDict()) if native else P.Materialized()
    tbl = P.table(eng, "key", ["price", ("w", True)], mat)
    assert tbl.spec.window_kind == abi.HSG_UNWINDOWED and tbl.spec.emit_mode == abi.HSG_EMIT_NONE
    assert [k for k, _ in tbl.spec.aggs] == [abi.HSG_LAST, abi.HSG_LAST]
    store = {}   # the reference's KV store, keys by the reference's key equality

    def canon(k):
        return P._canon(k)

    wm = -1
    joined = []
    for round_ in range(2):
        tb = table_batch(10_000 * round_, 200)
        for r in tb:  # tableStoreProcessor: ksPut key value
            store[canon(r["value"]["key"])] = r["value"]
        wm, _ = tbl.process(tb, watermark=wm)
        sb = stream_batch(10_000 * round_ + 5_000, 150)
        exp = []
        for r in sb:  # joinTableProcessor: ksGet, forward on Just
            k = r["value"].get("key")
            v2 = store.get(canon(k)) if "key" in r["value"] else None
            if v2 is not None:
                exp.append({"key": k, "value": joiner(r["value"], {"price": v2["price"], "w": v2["w"]}),
                            "timestamp": r["timestamp"]})
        n_keys = len(tbl.mat.keys)
        got = P.joinTable(tbl, joiner, sb)
        assert len(tbl.mat.keys) == n_keys, "an unknown stream key was inserted"
        assert got == exp and 0 < len(got) < len(sb)
        joined.append(got)
    # the second table batch brought key "c" and new prices: the second join saw them
    assert any(r["key"] == "c" for r in joined[1]) and not any(r["key"] == "c" for r in joined[0])
    tbl.close()
