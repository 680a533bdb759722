"""CPU: the checker of the value-edge tests, checked itself.

tests/test_gpu_value_edges.py compares the engine with pyoracle.OracleOp on
tests/valgen.py's columns: int64 values whose high word is live, the int64
identities as real values, doubles at the ends of the format, subnormal sums.
Here the C++ oracle (__int128 / __float128) runs on such batches against the
independent restatement pyref.PyRefOp (Python ints and Fractions, exact):
integers equal, f64 MIN / MAX / LAST equal with no tolerance, f64 SUM / AVG
within valgen.sum_rtol of the largest group. And the generator's own promises:
the prefix-sum bound, one sign per key, every special value present, the four
identity situations each present in a group."""
import math

import numpy as np
import pytest

import pyoracle
import pyref
import valgen
from hstream_amd import abi
from hstream_amd.columnar import OpSpec
from util import F64_RTOL, gen_small

I, F = abi.HSG_I64, abi.HSG_F64
# the full aggregate set over all four column classes:
# column 0 i64 under SUM / AVG, 1 i64 extreme, 2 f64 under SUM / AVG, 3 f64 extreme
COLS = [I, I, F, F]
AGGS = [(abi.HSG_COUNT_ALL, 0), (abi.HSG_SUM, 0), (abi.HSG_AVG, 0), (abi.HSG_MIN, 0), (abi.HSG_MAX, 0),
        (abi.HSG_LAST, 0), (abi.HSG_COUNT, 0),
        (abi.HSG_MIN, 1), (abi.HSG_MAX, 1), (abi.HSG_LAST, 1), (abi.HSG_COUNT, 1),
        (abi.HSG_SUM, 2), (abi.HSG_AVG, 2), (abi.HSG_MIN, 2), (abi.HSG_MAX, 2), (abi.HSG_LAST, 2),
        (abi.HSG_MIN, 3), (abi.HSG_MAX, 3), (abi.HSG_LAST, 3), (abi.HSG_COUNT, 3)]
NB, PER, NKEYS = 3, 1000, 30
DEDICATED = [NKEYS + 17 + j for j in range(4)]
KINDS = {"tumbling": (abi.HSG_TUMBLING, dict(size_ms=10_000)),
         "hopping": (abi.HSG_HOPPING, dict(size_ms=10_000, advance_ms=3_000)),
         "session": (abi.HSG_SESSION, dict(gap_ms=2_000)),
         "unwindowed": (abi.HSG_UNWINDOWED, {})}


def _batches(seed=1):
    classes = valgen.column_classes(COLS, AGGS)
    assert classes == ["i64_sum", "i64_ext", "f64_sum", "f64_ext"]
    pl = valgen.Planter(seed, classes, NB * PER, DEDICATED, frac=0.06)
    out = []
    for b in range(NB):
        key, ts, _c, _v = gen_small(40 + b, PER, NKEYS, span=20_000, base=1_000_000 + b * 20_000)
        out.append(pl.batch(key, ts))
    return out


BATCHES = _batches()


def _same(spec, got, exp, exact, rtol, what):
    assert len(got) == len(exp), what
    for g, x in zip(got, exp):
        assert g[:3] == x[:3], (what, g, x)
        for j, (a, b) in enumerate(zip(g[3], x[3])):
            if not spec.agg_is_f64()[j] or exact[j]:
                assert a == b or (a != a and b != b), (what, j, g, x)
            else:
                assert (a != a and b != b) or abs(a - b) <= 5e-324 + rtol * abs(b), (what, j, a, b)


@pytest.mark.parametrize("mode", [abi.HSG_EMIT_PER_BATCH, abi.HSG_EMIT_PER_RECORD], ids=["per_batch", "per_record"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_oracle_matches_pyref_on_value_edges(kind, mode):
    wk, kw = KINDS[kind]
    spec = OpSpec(wk, mode, col_types=COLS, aggs=AGGS, **kw)
    exact = valgen.exact_mask(spec)
    rtol = valgen.sum_rtol(valgen.max_group(spec, BATCHES))
    assert rtol <= F64_RTOL
    o, r = pyoracle.OracleOp(spec), pyref.PyRefOp(spec)
    wo = wr = -1
    for bi, (key, ts, cols, valid) in enumerate(BATCHES):
        wo = o.push(key, ts, cols, valid, watermark=wo)  # (HSG_E_RANGE here would be a generator bug)
        wr = r.push(key, ts, cols, valid, watermark=wr)
        assert wo == wr
        got = o.drain().tuples()
        exp = [(k, s, e, v) for k, s, e, _, v in r.drain()]
        if mode == abi.HSG_EMIT_PER_BATCH:
            got, exp = sorted(got, key=lambda t: t[:3]), sorted(exp, key=lambda t: t[:3])
        _same(spec, got, exp, exact, rtol, f"{kind} batch {bi}")
    got = sorted(o.dump_state().tuples(), key=lambda t: t[:3])
    exp = sorted(((k, s, e, v) for k, s, e, _, v in r.dump_state()), key=lambda t: t[:3])
    _same(spec, got, exp, exact, rtol, f"{kind} state")
    o.close()


def test_i64_wide_bound_and_high_words():
    rng = np.random.default_rng(2)
    for n_total in (3_000, 210_000, 1 << 22):
        bound = valgen.wide_bound(n_total)
        v = np.concatenate([valgen.i64_wide(rng, n_total // 3, bound) for _ in range(3)])
        # every prefix sum of every grouping fits: the sum of the magnitudes does
        # (exact: high and low halves summed apart)
        mag = np.abs(v)
        assert (int((mag >> 32).sum()) << 32) + int((mag & 0xFFFFFFFF).sum()) < 1 << 63
        hi = v >> 32
        assert ((hi != 0) & (hi != -1)).mean() > 0.8  # the high word is no sign extension
        for s in valgen.I64_SPECIALS:
            assert (v == s).any(), s
    assert any((v == s).any() for s in valgen.I64_BIG_SPECIALS)
    with pytest.raises(AssertionError):
        valgen.i64_wide(rng, 10, (1 << 40) - 1)


def test_crossing_runs_stay_inside_int64():
    reached = set()
    for cycle in (valgen.I64_CROSSING_CYCLE, valgen.I64_CROSSING_CYCLE_B):
        cyc = valgen.i64_crossing(0, 64, cycle).tolist()
        for start in range(4):
            for length in range(1, 40):
                s = 0
                for x in cyc[start:start + length]:
                    s += x
                    assert valgen.I64_MIN <= s <= valgen.I64_MAX, (start, length)
                    reached.add(s)
    assert valgen.I64_MAX in reached and valgen.I64_MIN + 1 in reached
    cyc = valgen.i64_crossing(0, 8).tolist()
    # another grouping leaves int64 and wraps back
    assert cyc[0] + cyc[1] + cyc[4] + cyc[5] > valgen.I64_MAX


def test_planted_batches_keep_their_promises():
    key = np.concatenate([b[0] for b in BATCHES])
    ts = np.concatenate([b[1] for b in BATCHES])
    cols = [np.concatenate([b[2][c] for b in BATCHES]) for c in range(4)]
    valid = [np.concatenate([b[3][c] for b in BATCHES]) for c in range(4)]
    ded = np.isin(key, DEDICATED)
    assert 16 * NB <= ded.sum() <= len(key) // 8
    # arrival-order prefix sums of every key fit int64 (exact, Python ints)
    for k in np.unique(key):
        s = 0
        for x, p in zip(cols[0][key == k].tolist(), valid[0][key == k].tolist()):
            s += x if p else 0
            assert valgen.I64_MIN <= s <= valgen.I64_MAX, k
    # dedicated timestamps never go back (no window cuts their arrival order, none is late)
    assert (np.diff(ts[ded]) >= 0).all()
    assert (ts[ded] == np.maximum.accumulate(np.maximum(ts, 0))[ded]).all()
    # one sign per key in the f64 SUM column
    for k in np.unique(key):
        s = np.sign(cols[2][key == k])
        assert (s == s[0]).all() and s[0] != 0, k
    # subnormal keys: multiples of 5e-324 whose exact sum is a subnormal double
    sub = cols[2][ded & (valid[2] != 0)]
    assert (np.abs(sub) < 2.2250738585072014e-308).all() and (sub != 0).all()
    for k in DEDICATED[:3]:
        m = (key == k) & (valid[2] != 0)
        units = [int(round(abs(x) / 5e-324)) for x in cols[2][m]]
        assert all(u * 5e-324 == abs(x) for u, x in zip(units, cols[2][m]))
        assert math.fsum(np.abs(cols[2][m])) == sum(units) * 5e-324 < 2.2250738585072014e-308
    # every special value at least once
    for s in valgen.I64_EXTREMES:
        assert ((cols[1] == s) & (valid[1] != 0)).any(), s
    bits = cols[3].view(np.uint64)
    for s in valgen.F64_EXTREMES.view(np.uint64):
        assert ((bits == s) & (valid[3] != 0)).any(), hex(int(s))
    # the four identity situations, each in a (key, 10 s window) group
    w = ts // 10_000
    seen = {"min_identity": 0, "max_identity": 0, "both": 0, "nothing": 0}
    for k in DEDICATED:
        for win in np.unique(w[key == k]):
            m = (key == k) & (w == win)
            for c, at_hi, at_lo in ((1, cols[1] == valgen.I64_MAX, cols[1] == valgen.I64_MIN),
                                    (3, cols[3] >= 2.0 ** 63, cols[3] <= -2.0 ** 63)):
                p = m & (valid[c] != 0)
                if not p.any():
                    seen["nothing"] += 1
                elif at_hi[p].all():
                    seen["min_identity"] += 1
                elif at_lo[p].all():
                    seen["max_identity"] += 1
                elif (at_hi[p] | at_lo[p]).all():
                    seen["both"] += 1
    assert all(v >= 2 for v in seen.values()), seen
    # and outside the dedicated keys ~5 % absent fields
    assert 0.02 < (valid[1][~ded] == 0).mean() < 0.09
