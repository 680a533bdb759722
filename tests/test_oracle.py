"""CPU: the oracle against the reference's own test vectors, and the C++
restatement against the independent pure-Python one on seeded inputs."""
import numpy as np
import pytest

import axisgen
import pyoracle
import pyref
from hstream_amd import abi
from hstream_amd.columnar import OpSpec, Rows
from util import ALL_AGG_SETS, gen_small, load_kat, run_kat_case

KAT = load_kat()


@pytest.mark.parametrize("w", KAT["windows_for"], ids=lambda w: f"ts{w['ts']}_s{w['size']}_a{w['adv']}")
def test_windows_for_kat(w):
    got = pyoracle.windows_for(w["ts"], w["size"], w["adv"])
    assert [s for s, _ in got] == w["starts"]
    assert all(e == s + w["size"] for s, e in got)
    assert [s for s, _ in pyref.windows_for(w["ts"], w["size"], w["adv"])] == w["starts"]


@pytest.mark.parametrize("case", KAT["cases"], ids=lambda c: c["name"])
def test_reference_kat_oracle(case):
    run_kat_case(case, lambda spec: pyoracle.OracleOp(spec))


@pytest.mark.parametrize("case", KAT["cases"], ids=lambda c: c["name"])
def test_reference_kat_pyref(case):
    run_kat_case(case, lambda spec: _PyRefAdapter(spec))


class _PyRefAdapter:
    def __init__(self, spec):
        self.r = pyref.PyRefOp(spec)
        self.spec = spec

    def push(self, key, ts, cols, valid, watermark):
        return self.r.push(key, ts, cols, valid, watermark)

    def drain(self):
        return _rows(self.r.drain(), len(self.spec.aggs))

    def dump_state(self):
        return _rows(self.r.dump_state(), len(self.spec.aggs))


def _rows(tups, naggs):
    n = len(tups)
    return Rows(np.array([t[0] for t in tups], dtype=np.uint32), np.array([t[1] for t in tups], dtype=np.int64),
                np.array([t[2] for t in tups], dtype=np.int64), np.array([t[3] for t in tups], dtype=np.int64),
                [np.array([t[4][j] for t in tups]) for j in range(naggs)] if n else [np.array([]) for _ in range(naggs)])


def _specs():
    out = []
    for aggname, col_types in (("count", []), ("full_i64", [abi.HSG_I64]), ("mixed", [abi.HSG_I64, abi.HSG_F64])):
        aggs = ALL_AGG_SETS[aggname]
        for kind, kw in ((abi.HSG_TUMBLING, dict(size_ms=10_000)),
                         (abi.HSG_HOPPING, dict(size_ms=10_000, advance_ms=3_000)),
                         (abi.HSG_UNWINDOWED, {}),
                         (abi.HSG_SESSION, dict(gap_ms=2_000))):
            aggs_k = aggs
            for mode in (abi.HSG_EMIT_PER_RECORD, abi.HSG_EMIT_PER_BATCH):
                out.append(pytest.param(OpSpec(kind, mode, col_types=col_types, aggs=aggs_k, **kw),
                                        id=f"{aggname}-k{kind}-m{mode}"))
    return out


def _close(a, b):
    if isinstance(a, float) or isinstance(b, float):
        if np.isnan(a) and np.isnan(b):
            return True
        return abs(a - b) <= 1e-9 * max(1.0, abs(a), abs(b))
    return a == b


@pytest.mark.parametrize("spec", _specs())
def test_cpp_oracle_matches_pyref(spec):
    """Two independent restatements agree, batch by batch, on messy inputs."""
    ncols = len(spec.col_types)
    o = pyoracle.OracleOp(spec)
    r = pyref.PyRefOp(spec)
    wm_o = wm_r = -1
    for bi in range(3):
        key, ts, cols, valid = gen_small(100 + bi, 300, 7, col_types=spec.col_types or (abi.HSG_I64,),
                                         span=20_000, base=1_000_000 + bi * 20_000)
        cols, valid = cols[:ncols], valid[:ncols]
        wm_o = o.push(key, ts, cols, valid, watermark=wm_o)
        wm_r = r.push(key, ts, cols, valid, watermark=wm_r)
        assert wm_o == wm_r
        got = o.drain().tuples()
        exp = [(k, s, e, v) for k, s, e, _, v in r.drain()]
        if spec.emit_mode == abi.HSG_EMIT_PER_BATCH:
            got, exp = sorted(got), sorted(exp)
        assert len(got) == len(exp)
        for g, x in zip(got, exp):
            assert g[:3] == x[:3]
            assert all(_close(a, b) for a, b in zip(g[3], x[3])), (g, x)
    st = sorted(o.dump_state().tuples())
    ex = sorted((k, s, e, v) for k, s, e, _, v in r.dump_state())
    assert len(st) == len(ex)
    for g, x in zip(st, ex):
        assert g[:3] == x[:3] and all(_close(a, b) for a, b in zip(g[3], x[3]))


def _cross(spec, batches, wms=None):
    """OracleOp against PyRefOp batch by batch: watermark, changelog, state."""
    o, r = pyoracle.OracleOp(spec), pyref.PyRefOp(spec)
    wm_o = wm_r = -1
    for bi, (key, ts, cols, valid) in enumerate(batches):
        if wms is not None and wms[bi] is not None:
            wm_o = wm_r = wms[bi]
        wm_o = o.push(key, ts, cols, valid, watermark=wm_o)
        wm_r = r.push(key, ts, cols, valid, watermark=wm_r)
        assert wm_o == wm_r
        got = o.drain().tuples()
        exp = [(k, s, e, v) for k, s, e, _, v in r.drain()]
        if spec.emit_mode == abi.HSG_EMIT_PER_BATCH:
            got, exp = sorted(got), sorted(exp)
        assert len(got) == len(exp), bi
        for g, x in zip(got, exp):
            assert g[:3] == x[:3], (bi, g, x)
            assert all(_close(a, b) for a, b in zip(g[3], x[3])), (g, x)
    st = sorted(o.dump_state().tuples())
    ex = sorted((k, s, e, v) for k, s, e, _, v in r.dump_state())
    assert len(st) == len(ex)
    for g, x in zip(st, ex):
        assert g[:3] == x[:3] and all(_close(a, b) for a, b in zip(g[3], x[3])), (g, x)
    o.close()
    return st


# ---- the time-axis generators (tests/axisgen.py), reduced: the reference side of
# ---- tests/test_gpu_time_axis.py, proven without a GPU
@pytest.mark.parametrize("emit", [abi.HSG_EMIT_PER_BATCH, abi.HSG_EMIT_PER_RECORD], ids=["batch", "changes"])
@pytest.mark.parametrize("window", sorted(axisgen.WINDOWS))
def test_axis_family_batches(window, emit):
    """The three batches of a family case on a non-zero epoch (batch 0's first
    keyed record in the middle, batch 2 before batch 0), messy and sorted."""
    kind, kw = axisgen.window_kw(window)
    spec = OpSpec(kind, emit, col_types=[abi.HSG_I64, abi.HSG_F64], aggs=ALL_AGG_SETS["mixed"], **kw)
    for gen in ("messy", "uniform"):
        shapes = axisgen.family(window, gen, 200, 7, 10, seed=100)
        assert axisgen.epoch_is_nonzero(shapes, axisgen.WINDOWS[window][2])
        k0, t0 = shapes[0]
        first = axisgen.first_keyed_ts(k0, t0)
        live = t0[(k0 != axisgen.NONE) & (t0 > axisgen.T0)]
        assert live.min() < first < live.max()  # records of batch 0 on both sides of the first one
        assert shapes[2][1].max() < live.min() < shapes[1][1].max()
        st = _cross(spec, axisgen.with_columns(shapes, spec.col_types, 100))
        assert len(st) > 0


@pytest.mark.parametrize("first", [axisgen.T0, 5])
def test_axis_span_points(first):
    """The reference has no span limit: the four points around the op's
    2^32-window span are ordinary records to both restatements."""
    spec = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=1, col_types=[abi.HSG_I64],
                  aggs=ALL_AGG_SETS["full_i64"])
    accepted, refused = axisgen.span_points(first)
    batches = [(np.zeros(1, np.uint32), np.array([t], np.int64), [np.array([3], np.int64)], None)
               for t in [first] + accepted + refused]
    st = _cross(spec, batches, wms=[-1] * len(batches))
    assert [s[1] for s in st] == sorted([first] + accepted + refused)


@pytest.mark.parametrize("kind", ["tumbling", "hopping"])
@pytest.mark.parametrize("adv", axisgen.ADVANCES, ids=lambda a: f"adv{a}")
def test_axis_window_starts(adv, kind):
    """Window starts near 0, 2^31, 2^32, 2^53 and 2^62 for every advance of
    the GPU test: both restatements, and Python's own integers."""
    size = adv if kind == "tumbling" else 2 * adv + 1
    for anchor in axisgen.ANCHORS:
        key, ts, grace = axisgen.window_start_batch(adv, size, anchor)
        spec = OpSpec(abi.HSG_TUMBLING if kind == "tumbling" else abi.HSG_HOPPING, abi.HSG_EMIT_PER_BATCH,
                      size_ms=size, advance_ms=adv, grace_ms=grace, aggs=[(abi.HSG_COUNT_ALL, 0)])
        st = _cross(spec, [(key, ts, [], None)])
        want = {}
        for t in ts.tolist():
            if t < 0:
                continue
            s = max(0, t - size + adv) // adv * adv
            while s <= t:
                want[s] = want.get(s, 0) + 1
                s += adv
        assert [(s[1], s[2], s[3][0]) for s in st] == [(s, s + size, c) for s, c in sorted(want.items())]
        assert sum(want.values()) == axisgen.window_pairs(key, ts, size, adv)


@pytest.mark.parametrize("emit", [abi.HSG_EMIT_PER_BATCH, abi.HSG_EMIT_PER_RECORD], ids=["batch", "changes"])
@pytest.mark.parametrize("window", sorted(axisgen.WINDOWS))
def test_axis_top(window, emit):
    """Up to INT64_MAX - 1: window end + grace wraps (Int64) and the record is
    dropped for that window, in both restatements alike; the batch wholly
    above the wrap leaves no row."""
    kind, kw = axisgen.window_kw(window)
    _k, size, adv = axisgen.WINDOWS[window]
    spec = OpSpec(kind, emit, col_types=[abi.HSG_I64], aggs=ALL_AGG_SETS["full_i64"], grace_ms=5_000, **kw)
    shapes = axisgen.top_of_axis(size, adv, 5_000, n=150)
    _cross(spec, axisgen.with_columns(shapes, spec.col_types, 3))
    o = pyoracle.OracleOp(spec)
    wm = -1
    rows = []
    for key, ts, cols, valid in axisgen.with_columns(shapes, spec.col_types, 3):
        wm = o.push(key, ts, cols, valid, watermark=wm)
        rows.append(len(o.drain()))
    assert rows[0] > 0 and rows[1] > 0 and rows[2] > 0 and rows[3] == 0, rows
    assert np.all(o.dump_state().win_end > 0)  # no accepted window's end wrapped
    o.close()


@pytest.mark.parametrize("gap", [0, 700])
@pytest.mark.parametrize("base", sorted(axisgen.SESSION_BASES))
def test_axis_sessions(base, gap):
    spec = OpSpec(abi.HSG_SESSION, abi.HSG_EMIT_PER_RECORD, gap_ms=gap, col_types=[abi.HSG_I64, abi.HSG_F64],
                  aggs=ALL_AGG_SETS["mixed"])
    batches = axisgen.session_batches(axisgen.SESSION_BASES[base], spec.col_types, n=150)
    assert all(abs(int(t)) + gap < 2**63 for b in batches for t in (b[1].min(), b[1].max()))
    _cross(spec, batches)


def test_faithful_and_fast_session_store_agree():
    spec = OpSpec(abi.HSG_SESSION, abi.HSG_EMIT_PER_RECORD, gap_ms=1_500, col_types=[abi.HSG_I64],
                  aggs=[(abi.HSG_COUNT_ALL, 0), (abi.HSG_SUM, 0), (abi.HSG_MIN, 0)])
    a = pyoracle.OracleOp(spec, faithful_sessions=True)
    b = pyoracle.OracleOp(spec, faithful_sessions=False)
    wa = wb = -1
    for bi in range(4):
        key, ts, cols, valid = gen_small(7 + bi, 2000, 50, span=60_000, base=bi * 60_000)
        wa = a.push(key, ts, cols, valid, watermark=wa)
        wb = b.push(key, ts, cols, valid, watermark=wb)
        assert a.drain().tuples() == b.drain().tuples()
    assert a.dump_state().tuples() == b.dump_state().tuples()
