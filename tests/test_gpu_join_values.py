"""GPU: the valued stream-stream join (include/hstream_join.h "valued join",
csrc/join.cpp, k_join_vals.hip): the join keeps the records' value columns in
HBM and drains the joined rows as the arrays of an hsg_batch.

The expected joined row is values[this_handle] ++ values[other_handle]: the
handles from oracle/joinref.py fed handle = global arrival number (what the
engine assigns), the values from the host copy of what was pushed. Every
comparison is bit-exact (f64 compared as bits); the values include +-0.0,
+-inf, NaNs with payloads and both ends of int64.

  1  parity over three pushes, with keyless records, records without the join
     field, and equal (key, side, ts) repeated inside and across batches
  2  every stride and an empty side
  3  pending rows around the wave and workgroup edges (the gather's tail lanes)
  4  arena growth
  5  the drain's contract and the refusals
  6  key_col
  7  join -> device drain -> a tumbling GROUP BY op and a select op
"""
import ctypes as C

import numpy as np
import pytest

import joinref
import pyoracle
from joinref import NONE
from hstream_amd import abi, sql
from util import F64_RTOL, rows_equal

pytestmark = pytest.mark.gpu

I, F = abi.HSG_I64, abi.HSG_F64
T0 = 1_700_000_000_000
I64_EDGES = np.array([-2**63, 2**63 - 1, 0, -1, 1, 2**32 - 1, 2**32 - 2, 2**53 + 1], np.int64).view(np.uint64)
F64_EDGES = np.array([0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
                      0x7FF8000000000000, 0x7FF8000000000123, 0xFFF800000000BEEF, 0x7FF0000000000001,
                      0x0000000000000001, 0x7FEFFFFFFFFFFFFF], np.uint64)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from hstream_amd.engine import Engine
    e = Engine(device=0, batch_capacity=1 << 13)
    yield e
    e.close()


def gen_stream(seed, n, types, nkeys=8, ts_slots=60, keyless=0.03, nojoin=0.04):
    """n records of both sides: (side, key, join key, ts), the value columns as
    uint64 bits (max of the sides' counts; record i owns the first
    len(types[side[i]])) and their valid bytes from {0, 1, 3}. Few keys on a
    coarse time grid: equal (key, side, ts) repeat."""
    rng = np.random.default_rng(seed)
    side = (rng.random(n) < 0.5).astype(np.uint8)
    key = rng.integers(0, nkeys, n).astype(np.uint32)
    key[rng.random(n) < keyless] = NONE
    jk = rng.integers(0, 2, n).astype(np.uint32)
    jk[rng.random(n) < nojoin] = NONE
    ts = T0 + 10 * ((np.arange(n) * ts_slots) // n + rng.integers(0, 6, n)).astype(np.int64)
    vc = max(len(types[0]), len(types[1]))
    cols, valid = [], []
    for c in range(vc):
        bits = rng.integers(0, 2**64, n, dtype=np.uint64)
        for sd in (0, 1):
            if c < len(types[sd]):
                edges = F64_EDGES if types[sd][c] == F else I64_EDGES
                m = (side == sd) & (rng.random(n) < 0.4)
                bits[m] = edges[rng.integers(0, len(edges), int(m.sum()))]
        cols.append(bits)
        valid.append(rng.choice(np.array([0, 1, 3], np.uint8), n, p=[0.15, 0.6, 0.25]))
    return side, key, jk, ts, cols, valid


def _slice(s, sl):
    side, key, jk, ts, cols, valid = s
    return side[sl], key[sl], jk[sl], ts[sl], [c[sl] for c in cols], [v[sl] for v in valid]


def _typed(cols):
    # the bits as the int64 arrays the binding passes through (it reads 8-byte values)
    return [c.view(np.int64) for c in cols]


def _push(j, part, device=False):
    side, key, jk, ts, cols, valid = part
    if device:
        import torch
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        j.push(t(side), t(key.view(np.int32)), t(jk.view(np.int32)), t(ts), cols=[t(c.view(np.int64)) for c in cols],
               valid=[t(v) for v in valid])
    else:
        j.push(side, key, jk, ts, cols=_typed(cols), valid=valid)


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def check_batch(b, n, rows, s, types, key_col=-1, what=""):
    """the first n rows of a drained JoinedBatch against joinref's rows over the
    host copy `s` of everything pushed"""
    c0 = len(types[0])
    assert n == len(rows), f"{what}: {n} rows, expected {len(rows)}"
    th = np.array([r[0] for r in rows], np.int64)
    oh = np.array([r[1] for r in rows], np.int64)
    _, _, _, _, cols, valid = s
    np.testing.assert_array_equal(_host(b.ts)[:n], np.array([r[3] for r in rows], np.int64), err_msg=f"{what}: ts")
    for k in range(c0 + len(types[1])):
        src, h = (k, th) if k < c0 else (k - c0, oh)
        np.testing.assert_array_equal(_host(b.cols[k])[:n].view(np.uint64), cols[src][h],
                                      err_msg=f"{what}: column {k}")
        if b.valid is not None:
            np.testing.assert_array_equal(_host(b.valid[k])[:n], valid[src][h], err_msg=f"{what}: valid {k}")
    if b.this_handle is not None:
        np.testing.assert_array_equal(_host(b.this_handle)[:n].view(np.uint64), th.view(np.uint64), err_msg=what)
    if b.other_handle is not None:
        np.testing.assert_array_equal(_host(b.other_handle)[:n].view(np.uint64), oh.view(np.uint64), err_msg=what)
    jks = np.array([r[2] for r in rows], np.uint32)
    if b.join_key is not None:
        np.testing.assert_array_equal(_host(b.join_key)[:n].view(np.uint32), jks, err_msg=what)
    if key_col < 0:
        want = jks
    else:
        src, h = (key_col, th) if key_col < c0 else (key_col - c0, oh)
        v = cols[src][h]
        ok = ((valid[src][h] & 1) == 1) & (v <= np.uint64(0xFFFFFFFE))
        want = np.where(ok, v, NONE).astype(np.uint32)
    np.testing.assert_array_equal(_host(b.key_id)[:n].view(np.uint32), want, err_msg=f"{what}: key_id")


def _ref_push(ref, part, base):
    side, key, jk, ts = part[:4]
    return ref.push(side, key, jk, ts, np.arange(base, base + len(ts), dtype=np.uint64))


def _overwrites(s, cuts):
    """(key, side, ts) replaced inside a batch / across batches"""
    side, key, jk, ts = s[:4]
    seen, inside, across = {}, 0, 0
    for bi, sl in enumerate(cuts):
        for i in range(*sl.indices(len(ts))):
            if key[i] == NONE:
                continue
            e = (int(key[i]), int(side[i]), int(ts[i]))
            if e in seen:
                if seen[e] == bi:
                    inside += 1
                else:
                    across += 1
            seen[e] = bi
    return inside, across


# ---- 1. parity -------------------------------------------------------------------------------
TYPES1 = ([I, F], [F, I, I])


def test_parity(eng):
    from hstream_amd.join import Join, value_stride
    s = gen_stream(11, 600, TYPES1)
    cuts = [slice(0, 200), slice(200, 400), slice(400, 600)]
    inside, across = _overwrites(s, cuts)
    assert inside >= 10 and across >= 10, (inside, across)
    assert (s[1] == NONE).sum() >= 5 and (s[2] == NONE).sum() >= 5
    assert value_stride(2, 3) == 4
    j = Join(eng, 60, 40, batch_capacity=256, cols=TYPES1)
    ref = joinref.JoinRef(60, 40)
    total = 0
    try:
        for bi, sl in enumerate(cuts):
            _push(j, _slice(s, sl))
            rows = _ref_push(ref, _slice(s, sl), sl.start)
            total += len(rows)
            assert j.pending() == len(rows)
            if bi == 1:
                # the handle drain of the same join: joinref's handles, row numbers
                th, oh, k, t = j.drain()
                assert list(zip(th.tolist(), oh.tolist(), k.tolist(), t.tolist())) == rows
            else:
                rc, n, b = j.drain_batch_into(len(rows))
                assert rc == abi.HSG_OK
                check_batch(b, n, rows, s, TYPES1, what=f"push {bi}")
            assert j.pending() == 0
        assert total >= 300, total
        assert j.value_rows() == (600, 1024)  # every record takes a row, keyless ones too
        assert j.state_rows() == ref.state_rows()
    finally:
        j.close()


# ---- 2. every stride, an empty side ------------------------------------------------------------
@pytest.mark.parametrize("c0,c1", [(0, 1), (1, 0), (1, 1), (3, 1), (1, 7), (4, 4), (8, 0), (0, 8)])
def test_strides(eng, c0, c1):
    from hstream_amd.join import Join, value_stride
    types = ([I, F, F, I, I, F, I, F][:c0], [F, I, I, F, F, I, F, I][:c1])
    assert value_stride(c0, c1) == {1: 2, 3: 4, 4: 8, 7: 8, 8: 16}[max(c0, c1)]
    s = gen_stream(100 + 10 * c0 + c1, 300, types)
    rows = joinref.JoinRef(50, 50).push(*s[:4], np.arange(300, dtype=np.uint64))
    assert len(rows) >= 100
    for device in (False, True):
        j = Join(eng, 50, 50, batch_capacity=512, cols=types)
        try:
            _push(j, s, device=device)
            rc, n, b = j.drain_batch_into(len(rows) + 3, device=device)
            assert rc == abi.HSG_OK
            check_batch(b, n, rows, s, types, what=f"({c0}, {c1}) device={device}")
        finally:
            j.close()


# ---- 3. pending rows around the wave and workgroup edges -----------------------------------------
def hot_key_stream(m, types, seed=5):
    """one key: m side-1 records at consecutive milliseconds, then one side-0
    record in their middle; window (m, m): m rows"""
    s = list(gen_stream(seed, m + 1, types))
    s[0] = np.r_[np.ones(m, np.uint8), np.zeros(1, np.uint8)]
    s[1] = np.full(m + 1, 0x80000001, np.uint32)
    s[2] = np.full(m + 1, 7, np.uint32)
    s[3] = np.r_[T0 + np.arange(m, dtype=np.int64), np.full(1, T0 + m // 2, np.int64)]
    return tuple(s)


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_output_sizes(eng, m):
    from hstream_amd.join import Join
    types = ([F, I], [I, F, I])
    s = hot_key_stream(m, types)
    rows = joinref.JoinRef(m + 5, m + 5).push(*s[:4], np.arange(m + 1, dtype=np.uint64))
    assert len(rows) == m
    j = Join(eng, m + 5, m + 5, batch_capacity=8192, cols=types)
    try:
        _push(j, s)
        assert j.pending() == m
        # guard rows past the pending ones: the tail lanes must not write them
        rc, n, b = j.drain_batch_into(m + 64, device=True)
        assert rc == abi.HSG_OK and n == m
        import torch
        torch.cuda.synchronize()
        check_batch(b, n, rows, s, types, what=f"m = {m}")
    finally:
        j.close()


def test_output_tail_is_untouched(eng):
    """rows past n of the caller's arrays keep what they held"""
    from hstream_amd.join import Join
    import torch
    types = ([I], [I])
    m = 65
    s = hot_key_stream(m, types)
    j = Join(eng, m + 5, m + 5, batch_capacity=256, cols=types)
    try:
        _push(j, s)
        cap = 256
        mk = lambda dt, v: torch.full((cap,), v, dtype=dt, device="cuda")
        cols = [mk(torch.int64, -7), mk(torch.int64, -7)]
        valid = [mk(torch.uint8, 0xAA), mk(torch.uint8, 0xAA)]
        key_id, ts = mk(torch.int32, -7), mk(torch.int64, -7)
        cp = (C.c_void_p * 2)(*[c.data_ptr() for c in cols])
        vp = (C.c_void_p * 2)(*[v.data_ptr() for v in valid])
        o = abi.hsg_join_joined(capacity=cap, mem=abi.HSG_MEM_DEVICE, key_col=-1, key_id=key_id.data_ptr(),
                                ts=ts.data_ptr(), cols=C.cast(cp, C.POINTER(C.c_void_p)),
                                valid=C.cast(vp, C.POINTER(C.c_void_p)))
        n = C.c_uint64()
        assert j._L.hsg_join_drain_batch(j._h, C.byref(o), C.byref(n)) == abi.HSG_OK and n.value == m
        for a in cols + [key_id, ts]:
            assert (a[m:] == -7).all() and not (a[:m] == -7).any()
        for a in valid:
            assert (a[m:] == 0xAA).all()
    finally:
        j.close()


# ---- 4. arena growth -------------------------------------------------------------------------------
def test_arena_growth(eng):
    from hstream_amd.join import Join
    types = ([I, F, I], [F])
    sizes = [200, 200, 0, 200, 200, 100]
    n = sum(sizes)
    s = list(gen_stream(21, n, types, nkeys=12, ts_slots=200))
    # record 3 (other side, key 999) waits for the last record (this side) of the last push
    for a, v0, v1 in ((s[0], 1, 0), (s[1], 999, 999), (s[2], 1, 1), (s[3], T0 + 5, T0 + 6)):
        a[3], a[n - 1] = v0, v1
    s = tuple(s)
    j = Join(eng, 70, 30, batch_capacity=256, cols=types)
    ref = joinref.JoinRef(70, 30)
    caps, base, last = [], 0, None
    try:
        assert j.value_rows() == (0, 256)
        for bi, sz in enumerate(sizes):
            part = _slice(s, slice(base, base + sz))
            _push(j, part)
            rows = _ref_push(ref, part, base)
            base += sz
            caps.append(j.value_rows())
            b = j.drain_batch(optional=("valid", "this_handle", "other_handle", "join_key"))
            check_batch(b, len(b.ts), rows, s, types, what=f"push {bi}")
            last = rows
        assert caps == [(200, 256), (400, 512), (400, 512), (600, 1024), (800, 1024), (900, 1024)]
        assert (n - 1, 3, 1, T0 + 6) in last
    finally:
        j.close()


# ---- 5. the drain's contract, the refusals -----------------------------------------------------------
def test_drain_contract(eng):
    from hstream_amd.join import Join
    s = gen_stream(31, 400, TYPES1)
    rows = joinref.JoinRef(60, 40).push(*s[:4], np.arange(400, dtype=np.uint64))
    p = len(rows)
    assert p > 100
    j = Join(eng, 60, 40, batch_capacity=512, cols=TYPES1)
    jd = Join(eng, 60, 40, batch_capacity=512, cols=TYPES1)
    try:
        _push(j, s)
        _push(jd, s, device=True)
        for device in (False, True):
            for cap in (0, p - 1):
                rc, n, _ = j.drain_batch_into(cap, device=device)
                assert rc == abi.HSG_E_CAPACITY and n == p and j.pending() == p
        # a key_col that names no column / an f64 column consumes nothing either
        for kc in (-2, 5, 1, 2):
            rc, n, _ = j.drain_batch_into(p, key_col=kc)
            assert rc == abi.HSG_E_INVALID and j.pending() == p, kc
        every = ("valid", "this_handle", "other_handle", "join_key")
        rc, n, host = j.drain_batch_into(p, optional=every)
        assert rc == abi.HSG_OK and j.pending() == 0
        check_batch(host, n, rows, s, TYPES1, what="host")
        rc, n2, dev = jd.drain_batch_into(p, device=True, optional=every)
        assert rc == abi.HSG_OK and n2 == n == p
        check_batch(dev, n2, rows, s, TYPES1, what="device")
        # an empty drain
        rc, n, _ = j.drain_batch_into(0)
        assert rc == abi.HSG_OK and n == 0
        # no optional array at all: the stream twice more (its records replace
        # the entries of the first copy and join them; the rows take the arena on)
        _push(j, s)
        _push(j, s, device=True)
        ref = joinref.JoinRef(60, 40)
        ref.push(*s[:4], np.arange(400, dtype=np.uint64))
        r2 = ref.push(*s[:4], np.arange(400, 800, dtype=np.uint64))
        r3 = ref.push(*s[:4], np.arange(800, 1200, dtype=np.uint64))
        s3 = s[:4] + ([np.tile(c, 3) for c in s[4]], [np.tile(v, 3) for v in s[5]])
        rc, n, b = j.drain_batch_into(len(r2) + len(r3), device=True, optional=())
        assert rc == abi.HSG_OK and b.valid is None and b.this_handle is None
        check_batch(b, n, r2 + r3, s3, TYPES1, what="no optional arrays")
    finally:
        j.close()
        jd.close()


def test_refusals(eng):
    from hstream_amd.join import Join
    plain = Join(eng, 10, 10, batch_capacity=64)
    valued = Join(eng, 10, 10, batch_capacity=64, cols=([I], [F]))
    L = plain._L
    try:
        one = lambda dt, v=0: np.array([v], dt)
        side, key, jk, ts, h, col = one(np.uint8), one(np.uint32, 1), one(np.uint32, 1), one(np.int64), \
            one(np.uint64), one(np.int64)
        b = abi.hsg_join_batch(n=1, mem=abi.HSG_MEM_HOST, side=side.ctypes.data, key_id=key.ctypes.data,
                               join_key=jk.ctypes.data, ts=ts.ctypes.data, handle=h.ctypes.data)
        cp = (C.c_void_p * 1)(col.ctypes.data)
        jc = abi.hsg_join_cols(cols=C.cast(cp, C.POINTER(C.c_void_p)), valid=None)
        assert L.hsg_join_push(valued._h, C.byref(b)) == abi.HSG_E_INVALID
        assert L.hsg_join_push_valued(plain._h, C.byref(b), C.byref(jc)) == abi.HSG_E_INVALID
        assert plain.drain_batch_into(4)[0] == abi.HSG_E_INVALID
        u = C.c_uint64()
        assert L.hsg_join_value_rows(plain._h, C.byref(u), C.byref(u)) == abi.HSG_E_INVALID
        assert valued.value_rows() == (0, 64) and valued.pending() == 0
        # the valued join still takes its own push (handle NULL, valid NULL = all present)
        b.handle = None
        assert L.hsg_join_push_valued(valued._h, C.byref(b), C.byref(jc)) == abi.HSG_OK
        assert valued.value_rows() == (1, 64)
        # a batch without its columns
        jc0 = abi.hsg_join_cols(cols=None, valid=None)
        assert L.hsg_join_push_valued(valued._h, C.byref(b), C.byref(jc0)) == abi.HSG_E_INVALID
        assert valued.value_rows() == (1, 64)
    finally:
        plain.close()
        valued.close()
    for cols in (([I] * 5, [I] * 4), ([I] * 9, []), ([7], [I])):
        with pytest.raises(abi.HStreamGpuError) as e:
            Join(eng, 10, 10, batch_capacity=64, cols=cols)
        assert e.value.status == abi.HSG_E_INVALID


# ---- 6. key_col ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_col", [-1, 0, 2])
def test_key_col(eng, key_col):
    from hstream_amd.join import Join
    types = ([I, F], [I])
    s = list(gen_stream(41, 500, types))
    rng = np.random.default_rng(42)
    ids = np.array([0, 5, 2**32 - 2, 2**32 - 1, 2**32, -1, -2**63, 2**63 - 1, 77], np.int64).view(np.uint64)
    s[4][0] = ids[rng.integers(0, len(ids), 500)]  # column 0 of either side: the key candidates
    s = tuple(s)
    rows = joinref.JoinRef(60, 60).push(*s[:4], np.arange(500, dtype=np.uint64))
    j = Join(eng, 60, 60, batch_capacity=512, cols=types)
    try:
        _push(j, s)
        b = j.drain_batch(key_col=key_col, device=True)
        check_batch(b, len(rows), rows, s, types, key_col=key_col, what=f"key_col {key_col}")
        got = _host(b.key_id).view(np.uint32)
        if key_col >= 0:
            # ids and every reason for HSG_KEY_NONE occur
            src = s[4][0][[r[0] if key_col == 0 else r[1] for r in rows]]
            val = s[5][0][[r[0] if key_col == 0 else r[1] for r in rows]]
            assert ((val & 1) == 0).any() and (src[(val & 1) == 1] == np.uint64(2**32 - 1)).any()
            assert (src[(val & 1) == 1].view(np.int64) < 0).any()
            assert (got == NONE).any() and (got == np.uint32(2**32 - 2)).any() and (got == 5).any()
    finally:
        j.close()


# ---- 7. end to end ------------------------------------------------------------------------------------------
def e2e_records(n=2000, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s1 = rng.random() < 0.5
        ts = T0 + (i * 20_000) // n + int(rng.integers(0, 300))
        if s1:
            v = {"a": int(rng.integers(0, 2)), "g": int(rng.integers(0, 16)), "v": int(rng.integers(-1000, 1000)),
                 "x": float(rng.normal())}
        else:
            v = {"b": int(rng.integers(0, 2)), "w": int(rng.integers(0, 12)), "y": float(rng.normal() * 1e3)}
        for f in [f for f in v if rng.random() < 0.04]:
            del v[f]
        out.append({"stream": "s1" if s1 else "s2", "key": int(rng.integers(0, 30)) if rng.random() > 0.02 else None,
                    "value": v, "timestamp": ts})
    return out


def test_end_to_end(eng):
    frm = sql.RFromJoin("s1", "a", "s2", "b", 2)
    recs = e2e_records()
    fields1, fields2 = ["a", "g", "v", ("x", True)], ["b", "w", ("y", True)]
    js, names = sql.gen_join_node(eng, frm, fields1, fields2, batch_capacity=1024)
    assert names == ["s1.a", "s1.g", "s1.v", "s1.x", "s2.b", "s2.w", "s2.y"]
    col = lambda n: sql.RExprCol(n, *n.split("."))
    tbl = sql.gen_group_by_node(eng, [("COUNT(*)",), ("SUM", "s2.y"), ("MAX", "s1.v"), ("SUM", "s2.w")],
                                sql.RGroupBy("s1.g", sql.RTumblingWindow(10)), float_fields=js.float_names)
    sel = [("COL", "s1.v"), ("COL", sql.RExprBinOp("t", "OpAdd", col("s1.v"), col("s2.w")), "t")]
    where = sql.RCondOp("RCompOpGT", col("s2.w"), sql.RExprConst("5", 5))
    st = sql.gen_select_node(eng, sel, where=where, float_fields=js.float_names)
    oracle = pyoracle.OracleOp(tbl.spec)
    f64s = tbl.spec.agg_is_f64()
    wg = wo = ws = -1
    total = 0
    try:
        for lo in (0, 1000):
            part = recs[lo:lo + 1000]
            # the reference's joined records of this poll batch (the host mirror sees the whole stream so far)
            joined = sql.gen_join_rows(frm, recs[:lo + 1000])[total:]
            total += len(joined)
            # GROUP BY s1.g over the joined stream, tumbling 10 s
            wg = js.process_into(part, tbl, watermark=wg)
            _, ts, cols, valid = tbl.columns(joined)
            keys = np.array([r["value"].get("s1.g", NONE) for r in joined], np.uint32)
            wo = oracle.push(keys, ts, cols, valid, watermark=wo)
            assert wg == wo
            rows_equal(tbl.op.drain(), oracle.drain(), f64s, ordered=True, what=f"group by, batch at {lo}",
                       rtol=F64_RTOL)
        assert total >= 1500, total
        rows_equal(tbl.op.dump_state(), oracle.dump_state(), f64s, what="state")
        # SELECT s1.v, s1.v + s2.w AS t ... WHERE s2.w > 5 over a join of its own
        js2, _ = sql.gen_join_node(eng, frm, fields1, fields2, batch_capacity=1024)
        try:
            got = []
            for lo in (0, 1000):
                base = st.op.stats()["records"]
                ws = js2.process_into(recs[lo:lo + 1000], st, watermark=ws)
                got += st._forward(st.op.drain(), base, None)
            joined = sql.gen_join_rows(frm, recs)
            exp = sql.gen_select_rows(sel, where, None, joined)
            assert len(exp) >= 300
            assert [(r["timestamp"], r["value"]) for r in got] == \
                [(ts, {a: int(v) for a, v in m.items()}) for _, ts, m in exp]
            # and the joined records themselves, drained to the host
            js3, _ = sql.gen_join_node(eng, frm, fields1, fields2, batch_capacity=2048)
            try:
                mine = js3.process(recs)
                keep = set(names)
                assert len(mine) == len(joined)
                for a, b in zip(mine, joined):
                    assert a["key"] == b["key"] and a["timestamp"] == b["timestamp"]
                    assert a["value"] == {k: v for k, v in b["value"].items() if k in keep}
            finally:
                js3.close()
        finally:
            js2.close()
    finally:
        js.close()
        tbl.close()
        st.close()
