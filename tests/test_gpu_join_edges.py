"""GPU: the stream-stream join (include/hstream_join.h, csrc/join.cpp,
k_join.hip, the LSD sort and scans of k_sort.hip) at its value, size and growth
edges, row for row and in order against oracle/joinref.py (whose rules
tests/test_join.py pins by hand). Every comparison is exact.

What each case is for:
  a  full-width record keys / join keys / handles, timestamps that straddle
     0, multiples of 2^32 (the sort's low-word wrap and the high word's sign
     flip), +-2^62 and both ends of int64
  b  batch sizes around the wave (64), the workgroup (256), the sort tile
     (4096) and the single-workgroup scan's limit (8192), up to batch_capacity
  c  arrangements: one side first, descending timestamps, a batch of keyless
     records, a first push that cannot join
  d  many versions of one (key, side, ts) and end points that enter the other
     store inside the batch (the version pick and ts_present's arrival test)
  e  output rows past the initial 65,536 with rows pending, state entries
     past the initial 65,536
  f  device batches / device drains, the drain's capacity contract, refusals

Every generated case must clear guards computed from the oracle alone (its
stores just before each record, and its rows), so that a stream which no
longer reaches the edge fails instead of passing vacuously:
  rows        rows produced
  inclusive   probes whose range was inclusive (both ends present, hi > lo)
  stops       probes that had a candidate in range and met a missing join
              field, their own or a candidate's
  overwrites  puts that replaced an existing (key, ts)
Floors, and what the committed seeds give (observed):
  a  rows >= 1000 (1905), inclusive >= 200 (863), stops >= 50 (194),
     overwrites >= 50 (223); final state 2709; the same for all seven bases
  b  the n-batch gives >= 1 row: n = 1: 1, 2: 1, 63: 20, 64: 21, 65: 18,
     255: 76, 256: 83, 257: 74, 4095: 2603, 4096: 2574, 4097: 2598,
     8191: 5291, 8192: 5192, 8193: 5129, 16384: 10539
  c  rows >= 500: side 1 first 3153, side 0 first 3196, descending 668,
     after the keyless batch 1669
  d  overwrites >= 1500 (1952), inclusive >= 500 (1252), rows >= 1000 (2997),
     stops >= 20 (64), final state == 48 (48)
  e  one push gives > 65,536 rows (132,000); > 65,536 rows pending (66,000)
     before the push that adds the rest; > 65,536 entries (70,000) before the
     last push, which gives >= 100 rows (1496, with 504 overwrites)

Mutations of the library each turn these red (run on an MI355X):
  pass 1 of the sort without its ^ 0x80000000   a at base 0 (the only base
                                                whose high word changes sign)
  record key sorted on 24 bits                  a, b, c, e (state), f
  out_base + off[t] -> off[t]                   e (output), the undrained run
  ensure_out without the copy of pending rows   e (output), the undrained run
  ts_present without its arrival test           a - d, the hand vectors
`T[p].arr < arr` -> `<=` in ts_present changes nothing and no test can see it:
T[p] is an entry of the other side, whose arrival never equals the record's.
"""
import bisect
import copy

import numpy as np
import pytest

import joinref
from joinref import NONE
from hstream_amd import abi
from test_join import HAND_VECTORS

pytestmark = pytest.mark.gpu

CAP = 1 << 14  # every join's batch_capacity (the issue's ceiling)

KEYS = np.array([0, 1, 255, 256, 65535, 65536, 0x00FFFFFF, 0x01000000, 0x7FFFFFFF, 0x80000000, 0x80000001,
                 0xFFFFFFFE], np.uint32)
JOIN_KEYS = np.array([0, 0x80000000, 0xFFFFFFFE], np.uint32)
BASES = [0, -2**32, 396 * 2**32, -2**62, 2**62, -2**63 + 2**20, 2**63 - 2**20]


def full_width_stream(base, n=3000, seed=2024, span=4000):
    """(side, key, join key, ts, handle) of n records: keys and join keys at
    the byte and sign edges of 32 bits, handles over all 64, near-sorted
    timestamps on a 5 ms grid over [base - span/2, base + span/2 + 400)."""
    rng = np.random.default_rng(seed)
    side = (rng.random(n) < 0.5).astype(np.uint8)
    key = KEYS[rng.integers(0, len(KEYS), n)]
    key[rng.random(n) < 0.02] = NONE
    jk = JOIN_KEYS[rng.integers(0, len(JOIN_KEYS), n)]
    jk[rng.random(n) < 0.03] = NONE
    off = ((np.arange(n, dtype=np.int64) * span) // n + rng.integers(0, 400, n)) // 5 * 5 - span // 2
    ts = np.int64(base) + off
    handle = rng.integers(0, 2**64, n, dtype=np.uint64)
    return side, key, jk, ts, handle


class GuardedRef(joinref.JoinRef):
    """the oracle, counting the guards from its own stores just before each record"""

    def __init__(self, before_ms, after_ms):
        super().__init__(before_ms, after_ms)
        self.g = dict(rows=0, inclusive=0, stops=0, overwrites=0)

    def push_one(self, side, key, jkey, ts, handle):
        if key != NONE:
            st, ost, tl = self.stores[side], self.stores[1 - side], self.ts_lists[1 - side]
            self.g["overwrites"] += ts in st and key in st[ts]
            b, a = (self.before, self.after) if side == 0 else (self.after, self.before)
            lo, hi = ts - b, ts + a
            inclusive = lo in ost and hi in ost and hi > lo
            self.g["inclusive"] += inclusive
            i0 = bisect.bisect_left(tl, lo) if inclusive else bisect.bisect_right(tl, lo)
            i1 = bisect.bisect_right(tl, hi) if inclusive else bisect.bisect_left(tl, hi)
            for t in tl[i0:i1]:
                c = ost[t].get(key)
                if c is not None and (jkey == NONE or c[0] == NONE):
                    self.g["stops"] += 1
                    break
        rows = super().push_one(side, key, jkey, ts, handle)
        self.g["rows"] += len(rows)
        return rows


def _take(stream, idx):
    return tuple(a[idx] for a in stream)


def _drain_rows(j, device=False):
    th, oh, k, t = j.drain(device=device)
    if device:
        th, oh, k, t = (th.cpu().numpy().view(np.uint64), oh.cpu().numpy().view(np.uint64),
                        k.cpu().numpy().view(np.uint32), t.cpu().numpy())
    return list(zip(th.tolist(), oh.tolist(), k.tolist(), t.tolist()))


def _same(got, exp, what):
    if got == exp:
        return
    i = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
    pytest.fail(f"{what}: {len(got)} rows vs {len(exp)} expected; first difference at row {i}: "
                f"got {got[i] if i < len(got) else None}, expected {exp[i] if i < len(exp) else None}")


def _run(eng, before, after, pushes, what):
    """the pushes through a fresh join and the oracle, compared after each;
    returns the oracle (guards, stores) and each push's rows"""
    from hstream_amd.join import Join
    j = Join(eng, before, after, batch_capacity=CAP)
    ref = GuardedRef(before, after)
    per_push = []
    try:
        for pi, p in enumerate(pushes):
            j.push(*p)
            exp = ref.push(*p)
            assert j.pending() == len(exp), f"{what}, push {pi}"
            _same(_drain_rows(j), exp, f"{what}, push {pi}")
            assert j.state_rows() == ref.state_rows(), f"{what}, push {pi}"
            per_push.append(exp)
    finally:
        j.close()
    return ref, per_push


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from hstream_amd.engine import Engine
    e = Engine(device=0, batch_capacity=1 << 10)
    yield e
    e.close()


# ---------------------------------------------------------------------------
# a. full-width values
# ---------------------------------------------------------------------------
_oracle_a = {}


def _oracle_full_width(base):
    if base not in _oracle_a:
        ref = GuardedRef(100, 50)
        _oracle_a[base] = (ref.push(*full_width_stream(base)), ref)
    return _oracle_a[base]


@pytest.mark.parametrize("base", BASES, ids=[f"base{i}" for i in range(len(BASES))])
def test_full_width_values(eng, base):
    rows, ref = _oracle_full_width(base)
    g = ref.g
    assert g["rows"] >= 1000 and g["inclusive"] >= 200 and g["stops"] >= 50 and g["overwrites"] >= 50, g
    # every base gives base 0's rows shifted by it: none degenerates
    rows0, ref0 = _oracle_full_width(0)
    assert [(a, b, k, t - base) for a, b, k, t in rows] == rows0 and ref.g == ref0.g
    assert ref.state_rows() == ref0.state_rows()
    s = full_width_stream(base)
    assert int(s[3].min()) < base < int(s[3].max())  # the stream straddles base
    got, _ = _run(eng, 100, 50, [_take(s, slice(p, p + 1000)) for p in range(0, 3000, 1000)], f"base {base}")
    assert got.g == g


# ---------------------------------------------------------------------------
# b. batch sizes
# ---------------------------------------------------------------------------
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 16384]


def sized_stream(n):
    """500 warm records, a batch of n, 500 more: the generator of (a) at
    396 * 2^32 and (a)'s density; the n-batch's first record is made to join
    a warm record (the latest for which the oracle gives a row: the other
    side, its key and join key, 5 ms later), so that n = 1 gives a row."""
    total = 1000 + n
    s = full_width_stream(396 * 2**32, n=total, seed=77, span=max(4000, total * 4 // 3))
    side, key, jk, ts, handle = (a.copy() for a in s)
    warm = joinref.JoinRef(100, 50)
    warm.push(*_take(s, slice(0, 500)))
    for w in range(499, -1, -1):
        rec = (1 - int(side[w]), int(key[w]), int(jk[w]), int(ts[w]) + 5, 0x0123456789ABCDEF)
        if copy.deepcopy(warm).push_one(*rec):
            break
    side[500], key[500], jk[500], ts[500], handle[500] = rec
    return (side, key, jk, ts, handle), [slice(0, 500), slice(500, 500 + n), slice(500 + n, total)]


@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes(eng, n):
    s, cuts = sized_stream(n)
    assert n <= CAP
    _, per_push = _run(eng, 100, 50, [_take(s, c) for c in cuts], f"n {n}")
    assert len(per_push[1]) >= 1, "guard: the n-batch itself produces rows"
    if n == 1:
        assert per_push[1][0][int(s[0][500])] == 0x0123456789ABCDEF


def test_empty_batch(eng):
    from hstream_amd.join import Join
    s = full_width_stream(0, n=500)
    j = Join(eng, 100, 50, batch_capacity=CAP)
    try:
        empty = _take(s, slice(0, 0))
        j.push(*empty)  # into an empty join
        assert j.pending() == 0 and j.state_rows() == 0
        j.push(*s)
        pending, state = j.pending(), j.state_rows()
        assert pending > 0 and state > 0
        j.push(*empty)
        assert j.pending() == pending and j.state_rows() == state
        ref = joinref.JoinRef(100, 50)
        _same(_drain_rows(j), ref.push(*s), "rows kept across an empty push")
    finally:
        j.close()


# ---------------------------------------------------------------------------
# c. arrangement
# ---------------------------------------------------------------------------
def test_batch_arrangement(eng):
    s = full_width_stream(396 * 2**32, n=4000, seed=5)
    side = s[0]
    s1, s0 = np.flatnonzero(side == 1), np.flatnonzero(side == 0)
    # all of side 1 in one push, then all of side 0
    ref, per_push = _run(eng, 100, 50, [_take(s, s1), _take(s, s0)], "side 1 first")
    assert per_push[0] == [] and ref.g["rows"] >= 500, ref.g
    # the reverse; the first push, side 0 only into an empty join, cannot join
    ref, per_push = _run(eng, 100, 50, [_take(s, s0), _take(s, s1)], "side 0 first")
    assert per_push[0] == [] and ref.g["rows"] >= 500, ref.g
    # strictly descending timestamps, one batch
    d = list(_take(s, slice(0, 4000)))
    d[3] = np.int64(396 * 2**32) + 5 * np.arange(3999, -1, -1, dtype=np.int64)
    assert (np.diff(d[3]) < 0).all()
    ref, _ = _run(eng, 100, 50, [tuple(d)], "descending")
    assert ref.g["rows"] >= 500, ref.g
    # a batch of keyless records between two normal ones: no rows, state unchanged
    k = list(_take(full_width_stream(396 * 2**32, n=1000, seed=6), slice(0, 1000)))
    k[1] = np.full(1000, NONE, np.uint32)
    k[3] = s[3][1500:2500].copy()  # timestamps the stores hold and will hold
    ref, per_push = _run(eng, 100, 50, [_take(s, slice(0, 2000)), tuple(k), _take(s, slice(2000, 4000))], "keyless")
    assert per_push[1] == [] and len(per_push[2]) >= 500, ref.g
    plain = joinref.JoinRef(100, 50)
    assert plain.push(*s) == per_push[0] + per_push[2] and plain.state_rows() == ref.state_rows()


# ---------------------------------------------------------------------------
# d. versions and end points inside one batch
# ---------------------------------------------------------------------------
def versions_stream(n=2000, seed=11):
    rng = np.random.default_rng(seed)
    side = (rng.random(n) < 0.5).astype(np.uint8)
    key = rng.integers(0, 3, n).astype(np.uint32)
    jk = rng.integers(0, 2, n).astype(np.uint32)
    jk[rng.random(n) < 0.01] = NONE
    ts = np.int64(1_700_000_000_000) + 10 * rng.integers(0, 8, n).astype(np.int64)
    handle = rng.integers(0, 2**64, n, dtype=np.uint64)
    return side, key, jk, ts, handle


def test_versions_and_endpoints(eng):
    s = versions_stream()
    one, per1 = _run(eng, 20, 10, [s], "one push")
    g = one.g
    assert g["overwrites"] >= 1500 and g["inclusive"] >= 500 and g["rows"] >= 1000 and g["stops"] >= 20, g
    assert one.state_rows() == 48
    three, per3 = _run(eng, 20, 10, [_take(s, slice(0, 700)), _take(s, slice(700, 1400)), _take(s, slice(1400, 2000))],
                       "three pushes")
    assert three.g == g and per3[0] + per3[1] + per3[2] == per1[0]


@pytest.mark.parametrize("vec", HAND_VECTORS, ids=lambda v: v[0])
def test_hand_vectors_gpu(eng, vec):
    from hstream_amd.join import Join
    name, before, after, steps, state = vec
    recs = [rec for rec, _ in steps]
    # one batch
    j = Join(eng, before, after, batch_capacity=CAP)
    try:
        j.push(*zip(*recs))
        _same(_drain_rows(j), [row for _, rows in steps for row in rows], f"{name}, one batch")
        assert j.state_rows() == state
    finally:
        j.close()
    # one record per push
    j = Join(eng, before, after, batch_capacity=CAP)
    try:
        for i, (rec, rows) in enumerate(steps):
            j.push(*[[x] for x in rec])
            _same(_drain_rows(j), rows, f"{name}, record {i + 1}")
        assert j.state_rows() == state
    finally:
        j.close()


# ---------------------------------------------------------------------------
# e. growth and undrained output
# ---------------------------------------------------------------------------
def hot_key_stream():
    """one key: 600 side-1 records at consecutive milliseconds, then 220
    side-0 records at the middle one; window (1000, 1000): 600 rows each"""
    t0 = 1_700_000_000_000
    n1, n0 = 600, 220
    side = np.r_[np.ones(n1, np.uint8), np.zeros(n0, np.uint8)]
    key = np.full(n1 + n0, 0x80000001, np.uint32)
    jk = np.full(n1 + n0, 7, np.uint32)
    ts = np.r_[t0 + np.arange(n1, dtype=np.int64), np.full(n0, t0 + n1 // 2, np.int64)]
    handle = np.arange(n1 + n0, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    return side, key, jk, ts, handle


def test_growth_output(eng):
    from hstream_amd.join import Join
    s = hot_key_stream()
    exp = joinref.JoinRef(1000, 1000).push(*s)
    assert len(exp) == 132_000
    # all in one push: > 65,536 rows from one probe launch
    ref, per_push = _run(eng, 1000, 1000, [s], "one push")
    assert per_push[0] == exp and len(per_push[0]) > 65536
    # side 1, then two side-0 pushes with a drain in between
    cuts = [slice(0, 600), slice(600, 710), slice(710, 820)]
    ref, per_push = _run(eng, 1000, 1000, [_take(s, c) for c in cuts], "drained")
    assert per_push[0] + per_push[1] + per_push[2] == exp
    # and with none: the second side-0 push finds 66,000 rows pending (more
    # than the output arrays' first 65,536), which the larger arrays must
    # carry over and its own rows must follow
    j = Join(eng, 1000, 1000, batch_capacity=CAP)
    try:
        j.push(*_take(s, cuts[0]))
        j.push(*_take(s, cuts[1]))
        assert j.pending() == 66_000 > 65536
        j.push(*_take(s, cuts[2]))
        assert j.pending() == 132_000
        _same(_drain_rows(j), exp, "undrained")
        assert j.pending() == 0 and j.state_rows() == 601
    finally:
        j.close()


def unique_entry_stream(n=70_000, n_back=2_000, seed=3):
    """n records with unique (key, ts) (one per millisecond, keys over all 32
    bits), then n_back that revisit entries of the first 14,000: 3 in 4 from
    the other side (they join the entry), the rest from the same (they
    replace it)"""
    rng = np.random.default_rng(seed)
    side = (rng.random(n) < 0.5).astype(np.uint8)
    key = rng.integers(0, 0xFFFFFFFF, n, dtype=np.uint64).astype(np.uint32)  # (HSG_KEY_NONE excluded)
    jk = rng.integers(0, 3, n).astype(np.uint32)
    ts = np.int64(1_700_000_000_000) + np.arange(n, dtype=np.int64)
    handle = rng.integers(0, 2**64, n, dtype=np.uint64)
    back = rng.choice(14_000, n_back, replace=False)
    flip = rng.random(n_back) < 0.75
    b_side = np.where(flip, 1 - side[back], side[back]).astype(np.uint8)
    b = (b_side, key[back], jk[back], ts[back], rng.integers(0, 2**64, n_back, dtype=np.uint64))
    return (side, key, jk, ts, handle), b


def test_growth_state(eng):
    from hstream_amd.join import Join
    s, back = unique_entry_stream()
    j = Join(eng, 5, 5, batch_capacity=CAP)
    ref = GuardedRef(5, 5)
    try:
        for p in range(0, 70_000, 14_000):
            sl = _take(s, slice(p, p + 14_000))
            j.push(*sl)
            _same(_drain_rows(j), ref.push(*sl), f"push at {p}")
            assert j.state_rows() == ref.state_rows()
        assert ref.state_rows() == 70_000 and j.state_rows() > 65536
        j.push(*back)
        exp = ref.push(*back)
        assert len(exp) >= 100 and ref.g["overwrites"] >= 100, ref.g
        _same(_drain_rows(j), exp, "revisit")
        assert j.state_rows() == ref.state_rows()
    finally:
        j.close()


# ---------------------------------------------------------------------------
# f. device transport and the drain contract
# ---------------------------------------------------------------------------
def _to_device(p):
    import torch
    side, key, jk, ts, handle = p
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in
            (side, key.view(np.int32), jk.view(np.int32), ts, handle.view(np.int64))]


def test_device_batches_and_drain_contract(eng):
    import torch
    from hstream_amd.join import Join
    s = full_width_stream(0)
    pushes = [_take(s, slice(p, p + 1000)) for p in range(0, 3000, 1000)]
    _, host_rows = _run(eng, 100, 50, pushes, "host")  # the host path against the oracle
    assert sum(len(r) for r in host_rows) >= 1000
    j = Join(eng, 100, 50, batch_capacity=CAP)
    try:
        for pi, p in enumerate(pushes):
            dev = _to_device(p)
            keep = [t.clone() for t in dev]
            torch.cuda.synchronize()  # the producer's work is done before push (no ready event in the batch)
            j.push(*dev)
            got = j.drain(device=True)
            assert all(t.is_cuda for t in got)
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(dev, keep)), "the caller's tensors are read only"
            th, oh, k, t = got
            rows = list(zip(th.cpu().numpy().view(np.uint64).tolist(), oh.cpu().numpy().view(np.uint64).tolist(),
                            k.cpu().numpy().view(np.uint32).tolist(), t.cpu().numpy().tolist()))
            _same(rows, host_rows[pi], f"device push {pi}")
        with pytest.raises(ValueError):
            j.push(dev[0], *pushes[0][1:])  # mixed host / device arrays
        assert j.pending() == 0
    finally:
        j.close()

    # capacity < pending: HSG_E_CAPACITY, n_out = pending, the rows stay
    j = Join(eng, 100, 50, batch_capacity=CAP)
    try:
        j.push(*pushes[0])
        pend = j.pending()
        assert pend == len(host_rows[0]) > 1
        for cap in (pend - 1, 0):
            rc, n_out, _ = j.drain_into(cap)
            assert rc == abi.HSG_E_CAPACITY and n_out == pend and j.pending() == pend
        _same(_drain_rows(j), host_rows[0], "full drain after refused ones")
        assert j.pending() == 0
        # null other_handle / join_key: the other columns are filled, the queue empties
        j.push(*pushes[1])
        pend = j.pending()
        assert pend == len(host_rows[1]) > 1
        rc, n_out, cols = j.drain_into(pend + 3, columns=("this_handle", "ts"))
        assert rc == abi.HSG_OK and n_out == pend and set(cols) == {"this_handle", "ts"}
        assert cols["this_handle"][:pend].tolist() == [r[0] for r in host_rows[1]]
        assert cols["ts"][:pend].tolist() == [r[3] for r in host_rows[1]]
        assert j.pending() == 0
        # and on the device path
        j.push(*pushes[2])
        pend = j.pending()
        rc, n_out, cols = j.drain_into(pend, columns=("other_handle", "join_key"), device=True)
        assert rc == abi.HSG_OK and n_out == pend and j.pending() == 0
        assert cols["other_handle"].cpu().numpy().view(np.uint64).tolist() == [r[1] for r in host_rows[2]]
        assert cols["join_key"].cpu().numpy().view(np.uint32).tolist() == [r[2] for r in host_rows[2]]
    finally:
        j.close()

    # refusals
    j = Join(eng, 100, 50, batch_capacity=1000)
    try:
        with pytest.raises(abi.HStreamGpuError) as ei:
            j.push(*_take(s, slice(0, 1001)))
        assert ei.value.status == abi.HSG_E_CAPACITY and "batch_capacity" in j.last_error()
        assert j.pending() == 0 and j.state_rows() == 0
        for pi, p in enumerate(pushes):  # the join works afterwards
            j.push(*p)
            _same(_drain_rows(j), host_rows[pi], f"after the refusal, push {pi}")
    finally:
        j.close()
    for kw in (dict(before_ms=-1, after_ms=50, batch_capacity=1000), dict(before_ms=100, after_ms=50, batch_capacity=0),
               dict(before_ms=100, after_ms=50, batch_capacity=0x7FFFFFFF)):
        with pytest.raises(abi.HStreamGpuError) as ei:
            Join(eng, **kw)
        assert ei.value.status == abi.HSG_E_INVALID, kw
