"""GPU: the device JSON decoder (hsg_gpu_decode_json, k_ingest.hip) against the
host decoder (hsg_decode_json_spelled on a fresh dictionary fed the same
batches in the same order). Every comparison is bit-exact: key ids, ts, every
column word, valid bytes, status, rejected, spellings, the dictionary's size
and each key's text."""
import ctypes as C

import numpy as np
import pytest

import jsongen
from hstream_amd import abi
from hstream_amd.columnar import OpSpec
from hstream_amd.ingest import Decoder, FastProbe, GpuDecoder, KeyDict, pack_records

pytestmark = pytest.mark.gpu

C2_COLS = [("v", abi.HSG_I64, True), ("x", abi.HSG_F64, True)]


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need cuda:0"
    from hstream_amd.engine import Engine
    e = Engine(device=0, batch_capacity=1 << 16)
    yield e
    e.close()


def _text(d, i, spelling=False):
    """A key's (or a spelling's) text as bytes: the corpus has keys that are not UTF-8."""
    fn = d._L.hsg_keydict_spelling_text if spelling else d._L.hsg_keydict_text
    n = C.c_size_t()
    rc = fn(d.handle, int(i), None, 0, C.byref(n))
    assert rc in (abi.HSG_OK, abi.HSG_E_CAPACITY), rc
    buf = C.create_string_buffer(max(1, n.value))
    assert fn(d.handle, int(i), buf, n.value, C.byref(n)) == abi.HSG_OK
    return buf.raw[: n.value]


class Pair:
    """A device decoder and the host decoder, each with its own dictionary."""

    def __init__(self, eng, key_field, cols, literal_forms=False, spellings=False, gkeys=None, hkeys=None, **kw):
        self.cols, self.spellings, self.keyless = cols, spellings, key_field is None
        self.gk = None if self.keyless else (gkeys or KeyDict())
        self.hk = None if self.keyless else (hkeys or KeyDict())
        kw.setdefault("max_records", 1 << 14)
        kw.setdefault("max_bytes", 1 << 21)
        self.g = GpuDecoder(eng, self.gk, key_field, cols, literal_forms=literal_forms, **kw)
        self.h = Decoder(key_field, cols, literal_forms=literal_forms)

    def batch(self, recs, ts=None, what="", **kw):
        """One batch through both; asserts equality; returns the device call's stats."""
        buf, off = pack_records(recs)
        n = len(recs)
        ts = np.arange(n, dtype=np.int64) * 7 + 1000 if ts is None else ts
        want = self.h.decode(self.hk, buf, off, ts, threads=2, spellings=self.spellings and not self.keyless)
        got = self.g.decode(buf, off, ts, threads=2, spellings=self.spellings and not self.keyless, **kw)
        self.compare(got, want, what)
        return got.stats

    def compare(self, got, want, what=""):
        key, ts, cols, valid, spell = got.to_host()
        assert np.array_equal(key, want[0]), f"{what}: key ids"
        assert np.array_equal(ts, want[1]), f"{what}: ts"
        for c in range(len(self.cols)):
            assert np.array_equal(cols[c].view(np.uint64), want[2][c].view(np.uint64)), f"{what}: column {c}"
            assert np.array_equal(valid[c], want[3][c]), f"{what}: valid {c}"
        assert np.array_equal(got.status, want[4]), f"{what}: status"
        assert got.rejected == want[5], f"{what}: rejected"
        if self.spellings and not self.keyless:
            assert np.array_equal(spell, want[6]), f"{what}: spellings"
            for s in np.unique(want[6][want[6] != abi.HSG_KEY_NONE]):
                assert _text(self.gk, s, True) == _text(self.hk, s, True), f"{what}: spelling {s}"
        assert got.stats["records"] == got.n and got.stats["accepted"] + got.stats["host_records"] == got.n
        if not self.keyless:
            self.same_dictionary(what)

    def same_dictionary(self, what=""):
        assert len(self.gk) == len(self.hk), f"{what}: dictionary size"
        for i in range(len(self.hk)):
            assert _text(self.gk, i) == _text(self.hk, i), f"{what}: key {i}"

    def close(self):
        self.g.close()
        self.h.close()


@pytest.fixture(scope="module")
def corpus():
    return jsongen.corpus()


@pytest.mark.parametrize("forms", [True, False], ids=["forms", "noforms"])
@pytest.mark.parametrize("spellings", [True, False], ids=["spelled", "plain"])
def test_corpus_parity(eng, corpus, forms, spellings):
    """The messy corpus in three batches: every output and the dictionaries
    equal; a good part of it is decoded on the device once its keys are known."""
    p = Pair(eng, jsongen.KEY_FIELD, jsongen.COLS, literal_forms=forms, spellings=spellings)
    cuts = [0, 7000, 13_500, len(corpus)]
    stats = [p.batch(corpus[cuts[b]:cuts[b + 1]], what=f"batch {b}") for b in range(3)]
    assert stats[2]["accepted"] > 1000, stats
    assert all(s["host_records"] > 0 for s in stats)  # the corpus always has records for the host
    p.close()


def test_steady_state(eng):
    """Clean C2-shaped records: the first batch's keys are all new, so the host
    decodes it; the second batch, over the same keys, never leaves the device."""
    p = Pair(eng, "k", C2_COLS)
    n = 6000
    first = [b'{"k":%d,"v":1,"x":0.5}' % i for i in range(n)]  # every key new
    s1 = p.batch(first, what="batch 1")
    assert s1["host_records"] == n and s1["accepted"] == 0 and s1["new_keys"] == n
    s2 = p.batch(jsongen.c2_records(5, n, n_keys=n), what="batch 2")
    assert s2["host_records"] == 0 and s2["accepted"] == n and s2["new_keys"] == 0
    p.close()


@pytest.mark.parametrize("ty", [abi.HSG_F64, abi.HSG_I64], ids=["f64", "i64"])
@pytest.mark.parametrize("forms", [True, False], ids=["forms", "noforms"])
def test_number_grid_on_device(eng, ty, forms):
    """The number grid and the int64 edges through the kernel: the device's
    f64 multiply and divide against strtod. The accept set is the host
    compile's, so every in-rule number is decoded on the device."""
    lits = jsongen.number_grid() + jsongen.I64_EDGES
    recs = [b'{"x":' + s.encode() + b"}" for s in lits]
    cols = [("x", ty, True)]
    probe = FastProbe(None, cols, literal_forms=forms)
    want_acc = sum(int(probe(r).accept) for r in recs)
    p = Pair(eng, None, cols, literal_forms=forms)
    s = p.batch(recs, what="grid")
    assert s["accepted"] == want_acc and want_acc > 1000
    p.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_batch_sizes(eng, n):
    p = Pair(eng, "k", C2_COLS)
    recs = jsongen.c2_records(n, n, n_keys=50)
    p.batch(recs, what="first")
    s = p.batch(recs, what="second")
    assert s["host_records"] == 0 and s["accepted"] == n
    p.close()


def test_offset_base_and_odd_address(eng):
    """off[0] != 0, the bytes at an odd address, a byte count that is no
    multiple of 16."""
    p = Pair(eng, "k", C2_COLS)
    recs = jsongen.c2_records(3, 777, n_keys=30)
    while sum(len(r) for r in recs) % 16 == 0:
        recs.append(b'{"k":1}')
    buf, off = pack_records(recs)
    ts = np.arange(len(recs), dtype=np.int64)
    want = p.h.decode(p.hk, buf, off, ts)
    lead = 5
    store = C.create_string_buffer(len(buf) + lead + 2)
    addr = C.addressof(store)
    base = addr + (1 if addr % 2 == 0 else 0)  # odd
    C.memmove(base + lead, buf, len(buf))
    off2 = off + np.uint64(lead)
    assert base % 2 == 1 and off2[0] != 0 and int(off2[-1] - off2[0]) % 16 != 0
    for rnd in range(2):
        got = p.g.decode(None, off2, ts, base=base)
        if rnd:
            want = p.h.decode(p.hk, buf, off, ts)
        p.compare(got, want, f"round {rnd}")
    assert got.stats["host_records"] == 0
    p.close()


def test_long_record_takes_the_global_path(eng):
    """Tiles whose bytes do not fit the LDS buffer are scanned from HBM, and
    their records are decoded on the device all the same: a 4096-byte record
    (HSG_GPU_DEC_MAX_RECORD) in a tile of 320-byte ones, and a run of 4096-byte
    records, among tiles of 20-byte records that do fit. A record one byte
    longer is a fallback record."""
    big = abi.HSG_GPU_DEC_MAX_RECORD
    small = [b'{"k":%d,"v":%d}' % (i % 7, i) for i in range(300)]
    long1 = b'{"k":3,"v":5,"x":2.5' + b" " * (big - 21) + b"}"
    assert len(long1) == big
    mid = [b'{"k":%d,"v":%d,"pad":"%s"}' % (i % 7, i, b"w" * 300) for i in range(155)]
    recs = small[:100] + [long1] + mid + small[100:] + [long1] + small[:55] + [long1] * 12
    # tiles of 256 records against the 32 KiB LDS buffer (kIngestLds): tile 0 (100 small, the long record,
    # 155 of ~320 bytes) and tile 2 (the run of long records) exceed it and are scanned from HBM; tile 1
    # (small records and one long one) is staged in LDS
    tile_bytes = [sum(len(r) for r in recs[t:t + 256]) for t in range(0, len(recs), 256)]
    assert len(tile_bytes) == 3 and tile_bytes[0] > 40_000 and tile_bytes[1] < 16_000 and tile_bytes[2] > 40_000, tile_bytes
    p = Pair(eng, "k", C2_COLS)
    p.batch(recs, what="first")
    s = p.batch(recs, what="second")
    assert s["host_records"] == 0 and s["accepted"] == len(recs)
    over = b'{"k":3,"v":5,"x":2.5' + b" " * (big - 20) + b"}"
    assert len(over) == big + 1
    s = p.batch(small[:40] + [over] + small[40:90], what="over-long")
    assert s["host_records"] == 1
    p.close()


def test_empty_objects_keyless(eng):
    p = Pair(eng, None, C2_COLS)
    s = p.batch([b"{}", b" { } ", b'{"v":2}', b"{}", b"[]", b"{"] * 50, what="keyless")
    assert s["host_records"] == 100 and s["accepted"] == 200
    p.close()


def test_spellings_of_one_key(eng):
    """1, 1.0 and 10e-1 are one key spelled three ways: the alternate
    spellings come from the host and are the host decoder's."""
    recs = [b'{"k":1,"v":1}', b'{"k":1.0,"v":2}', b'{"k":10e-1,"v":3}', b'{"k":1E0,"v":4}', b'{"k":2.0,"v":5}',
            b'{"k":2,"v":6}', b'{"k":"1","v":7}'] * 40
    p = Pair(eng, "k", C2_COLS, spellings=True)
    p.batch(recs, what="first")
    s = p.batch(recs, what="second")
    # the first spelling of each key stays on the device, the others go to the host
    assert s["accepted"] == 4 * 40 and s["host_records"] == 3 * 40
    q = Pair(eng, "k", C2_COLS, spellings=False)
    q.batch(recs, what="plain first")
    assert q.batch(recs, what="plain second")["host_records"] == 0
    p.close()
    q.close()


def test_key_table_rebuilds(eng):
    """64 slots to start with and 5 000 distinct keys over four batches: the
    table grows by rebuild and every known key is still found."""
    p = Pair(eng, "k", C2_COLS, table_slots=64)
    rebuilds = 0
    for b in range(4):
        recs = [b'{"k":%d,"v":%d,"x":1.25}' % (k, b) for k in range(1250 * b, 1250 * (b + 1))]  # 1 250 new keys
        recs += jsongen.c2_records(40 + b, 2000, n_keys=1250 * (b + 1))
        recs += [b'{"k":"s%d","v":1}' % i for i in range(0, 1250 * (b + 1), 97)]
        s = p.batch(recs, what=f"batch {b}")
        rebuilds = s["table_rebuilds"]
    assert rebuilds > 0 and len(p.hk) >= 5000
    s = p.batch(recs, what="again")
    assert s["host_records"] == 0 and s["table_slots"] >= 2 * len(p.hk)
    p.close()


def test_keys_from_elsewhere(eng):
    """Keys another caller encodes between calls, and a dictionary that held
    keys before the decoder was created, are hits."""
    gk, hk = KeyDict(), KeyDict()
    for d in (gk, hk):
        for i in range(300):
            d.encode(i)
        d.encode("early")
    p = Pair(eng, "k", C2_COLS, gkeys=gk, hkeys=hk)
    recs = jsongen.c2_records(9, 2000, n_keys=300) + [b'{"k":"early","v":1}']
    s = p.batch(recs, what="pre-filled")
    assert s["host_records"] == 0 and s["new_keys"] == 0
    for d in (gk, hk):
        for i in range(300, 600):
            d.encode_json("%d.0" % i)  # (spelled 300.0: the key 300)
        d.encode("late")
    recs = jsongen.c2_records(10, 2000, n_keys=600) + [b'{"k":"late","v":1}']
    s = p.batch(recs, what="encoded between calls")
    assert s["host_records"] == 0 and s["new_keys"] == 0
    p.close()


def test_keys_the_table_cannot_hold(eng):
    """A 30-digit number, a 60-byte string and an object as keys: never in the
    table, decoded by the host on every batch."""
    odd = [b'{"k":123456789012345678901234567890,"v":1}', b'{"k":"%s","v":2}' % (b"z" * 60), b'{"k":{"a":1,"b":[2]},"v":3}',
           b'{"k":{"b":[2],"a":1.0},"v":4}']
    recs = (jsongen.c2_records(1, 50, n_keys=10) + odd) * 20
    p = Pair(eng, "k", C2_COLS)
    p.batch(recs, what="first")
    for b in range(2):
        s = p.batch(recs, what=f"again {b}")
        assert s["host_records"] == 4 * 20 and s["new_keys"] == 0
    assert len(p.hk) >= 4
    p.close()


def test_capacity(eng):
    p = Pair(eng, "k", C2_COLS, max_records=100, max_bytes=4000)
    recs = jsongen.c2_records(2, 101, n_keys=10)
    buf, off = pack_records(recs)
    with pytest.raises(abi.HStreamGpuError) as ei:
        p.g.decode(buf, off, np.zeros(101, np.int64))
    assert ei.value.status == abi.HSG_E_CAPACITY
    fat = [b'{"k":1,"v":2,"pad":"' + b"w" * 100 + b'"}'] * 50
    buf, off = pack_records(fat)
    with pytest.raises(abi.HStreamGpuError) as ei:
        p.g.decode(buf, off, np.zeros(50, np.int64))
    assert ei.value.status == abi.HSG_E_CAPACITY
    assert len(p.gk) == 0
    p.batch(recs[:100], what="after the refusals")
    s = p.batch(recs[:100], what="after the refusals, again")
    assert s["host_records"] == 0
    p.close()


def test_unsupported_configuration(eng):
    with pytest.raises(abi.HStreamGpuError) as ei:
        GpuDecoder(eng, KeyDict(), "k", [(f"c{j}", abi.HSG_I64, True) for j in range(9)])
    assert ei.value.status == abi.HSG_E_INVALID


def _sorted_rows(rows):
    order = np.lexsort((rows.win_start, rows.key_id))
    return [rows.key_id[order], rows.win_start[order], rows.win_end[order]] + \
        [np.asarray(a)[order].view(np.uint64) for a in rows.aggs]


def test_end_to_end_tumbling(eng):
    """Device-decoded batches pushed asynchronously with their ready_event,
    both output sets in use, against the same records through the host decoder
    and host batches: changelog and dump bit for bit."""
    spec = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=10_000, col_types=[abi.HSG_I64, abi.HSG_F64],
                  aggs=[(abi.HSG_COUNT_ALL, 0), (abi.HSG_SUM, 0), (abi.HSG_MIN, 1), (abi.HSG_MAX, 1), (abi.HSG_COUNT, 1)])
    g, h = eng.op(spec), eng.op(spec)
    gk, hk = KeyDict(), KeyDict()
    gd = GpuDecoder(eng, gk, "k", C2_COLS, max_records=1 << 12, max_bytes=1 << 19)
    hd = Decoder("k", C2_COLS)
    rng = np.random.default_rng(77)
    wm_g = C.c_int64(-1)
    wm_h = -1
    on_device = 0
    for b in range(3):
        n = 1700
        recs = jsongen.c2_records(60 + b, n, n_keys=200)
        recs[5::50] = [b'{"k":%d,"v":"oops"}' % i for i in range(len(recs[5::50]))]   # dropped records
        recs[7::50] = [b'{"k":%d,"x":1e0}' % i for i in range(len(recs[7::50]))]      # an absent field
        ts = 3_000_000 + 20_000 * b + np.sort(rng.integers(0, 20_000, n)).astype(np.int64)
        buf, off = pack_records(recs)
        if b == 2:
            g.wait()  # batch 0's arrays are written again by this call
        db = gd.decode(buf, off, ts)
        on_device += db.stats["accepted"]
        g.push_batch_async(db.batch, watermark=wm_g, keep=db)
        k, t, cs, valid, _st, _rej = hd.decode(hk, buf, off, ts)
        wm_h = h.push(k, t, cs, valid, watermark=wm_h)
    g.wait()
    assert on_device > 2500
    assert wm_g.value == wm_h
    a, w = g.drain(), h.drain()
    assert len(a) == len(w) and len(a) > 0
    for x, y in zip(_sorted_rows(a), _sorted_rows(w)):
        assert np.array_equal(x, y)
    a, w = g.dump_state(), h.dump_state()
    assert len(a) == len(w) and len(a) > 0
    for x, y in zip(_sorted_rows(a), _sorted_rows(w)):
        assert np.array_equal(x, y)
    assert len(gk) == len(hk) and all(_text(gk, i) == _text(hk, i) for i in range(len(hk)))
    for o in (g, h, gd, hd):
        o.close()


def test_table_process_json_device_decode(eng):
    """Table.process_json(device_decode=True) and runTask over raw poll
    batches: the rows and stream time of the host-decoded path."""
    from hstream_amd import processing as P

    def table():
        w = P.groupBy(eng, "k").timeWindowedBy(P.mkTumblingWindow(2000))
        return w.aggregate([P.COUNT_ALL("n"), P.SUM("v", "s"), P.MAX("v", "m")], P.Materialized(keys=KeyDict()))

    rng = np.random.default_rng(5)
    polls = []
    for b in range(3):
        recs = jsongen.c2_records(80 + b, 900, n_keys=40) + [b'{"k":"a\\u0041","v":3}', b'{"v":1}', b"nonsense"]
        buf, off = pack_records(recs)
        polls.append((buf, off, 5000 * b + np.sort(rng.integers(0, 5000, len(recs))).astype(np.int64)))
    td, th = table(), table()
    key = lambda r: (str(r[0].twkKey), r[0].twkWindow.tWindowStart)
    for buf, off, ts in polls[:2]:
        wd, rd = td.process_json(buf, off, ts, device_decode=True)
        wh, rh = th.process_json(buf, off, ts)
        assert wd == wh and sorted(rd, key=key) == sorted(rh, key=key) and len(rd) > 0
    assert td._gpu_decoder is not None and td._decoder is None
    seen_d, seen_h = [], []
    rest = [polls[2]]
    wd = P.runTask(lambda: rest.pop(0) if rest else None, td, sink=seen_d.append, device_decode=True)
    rest = [polls[2]]
    wh = P.runTask(lambda: rest.pop(0) if rest else None, th, sink=seen_h.append)
    assert sorted(seen_d, key=key) == sorted(seen_h, key=key) and len(seen_d) > 0
    assert sorted(td.dump(), key=key) == sorted(th.dump(), key=key)
    td.close()
    th.close()
