"""Host side of tests/test_gpu_retention_ops.py (no GPU): the streams that file
pushes (tests/retgen.py), checked with the oracle alone.

  * every randomised stream closes windows by construction: of the groups in
    the oracle's final dump, those with win_end + grace <= the final stream
    time are at least half and at least four times the op's state_capacity,
    so the GPU file fails on its stream, not on the engine, should a
    generator change;
  * the closing boundary's arithmetic: the stream time the oracle returns
    after batch 1 is A.end + grace (A.end + grace - 1), and the oracle
    refuses (accepts) batch 2's record into A;
  * the moved litforms._prefix_forms on twelve hand-written records, the
    expected words written out.
"""
import numpy as np
import pytest

import litforms
import pyoracle
import retgen
from hstream_amd import abi


@pytest.mark.parametrize("name", list(retgen.RANDOMISED))
def test_stream_closes_windows_by_construction(name):
    case = retgen.RANDOMISED[name]()
    closed, total = retgen.assert_spills_by_construction(case)
    for key, ts, _c, _v in case.batches:
        assert 2_000 <= len(key) <= 20_000 and len(ts) == len(key)
    assert 64 <= case.spec.state_capacity <= 1 << 10
    if case.forms:
        gid, fw = case.form_words()  # (asserts that no record is late)
        assert len(gid) == len(fw) == sum(len(b[0]) for b in case.batches)


@pytest.mark.parametrize("closed", [True, False], ids=["closed", "open"])
@pytest.mark.parametrize("epoch", [0, 1], ids=["epoch0", "epoch_nonzero"])
@pytest.mark.parametrize("kind", [abi.HSG_TUMBLING, abi.HSG_HOPPING], ids=["tumbling", "hopping"])
def test_boundary_stream_time(kind, epoch, closed):
    b = retgen.boundary_case(kind, epoch, closed)
    spec = b.case.spec
    assert b.wm1 == b.a_end + spec.grace_ms - (0 if closed else 1)
    assert (b.a_start >= 1_700_000_000_000) == bool(epoch)
    o = pyoracle.OracleOp(spec)
    w = o.push(*b.case.batches[0], watermark=-1)
    assert w == b.wm1
    d = o.dump_state()
    at = np.nonzero((d.key_id == retgen.K0) & (d.win_start == b.a_start))[0]
    assert len(at) == 1 and (d.aggs[0][at[0]], d.aggs[1][at[0]]) == b.a_batch1
    # A, and only A, is closed at batch 2's entry -- or nothing is
    assert int(np.count_nonzero(d.win_end + spec.grace_ms <= w)) == (1 if closed else 0)
    o.drain()
    o.push(*b.case.batches[1], watermark=w)
    rows = o.drain()
    a_rows = np.nonzero((rows.key_id == retgen.K0) & (rows.win_start == b.a_start))[0]
    assert len(a_rows) == (0 if closed else 1)  # refused / accepted
    k0 = np.nonzero(rows.key_id == retgen.K0)[0]
    assert len(k0) == (1 if kind == abi.HSG_TUMBLING else 2) + (0 if closed else 1)  # B (T + 200, T + 400) accepted
    d = o.dump_state()
    at = np.nonzero((d.key_id == retgen.K0) & (d.win_start == b.a_start))[0]
    assert (d.aggs[0][at[0]], d.aggs[1][at[0]]) == (b.a_batch1 if closed else b.a_both)
    o.close()


def test_pending_case_has_no_randomness():
    for forms in (False, True):
        a, b = retgen.pending_case(forms), retgen.pending_case(forms)
        for x, y in zip(a.batches, b.batches):
            assert all(np.array_equal(p, q) for p, q in zip((x[0], x[1], x[2][0], x[3][0]), (y[0], y[1], y[2][0], y[3][0])))
        assert bool(np.all(a.accepted()))


def test_prefix_forms_hand_written():
    """SELECT v, COUNT(*), SUM(v), AVG(v), MIN(v), MAX(v): LAST bits 0-1, SUM
    bits 4-5, MIN bits 8-9, MAX bits 10-11 (COUNT and AVG carry none); per
    output 1 = prints as an integer, 0 = as a decimal, 3 = the initial value.
    Valid byte: bit 0 present, bit 1 a decimal literal.

      group 10: 5 (int), 5 (decimal: MIN keeps the earlier literal, MAX takes
                the later), 2.5 (decimal), absent, 5 (int: MAX tie, the later)
      group 20: absent, absent (every output still its initial value)
      group 30: 3 (decimal), 3 (int: MIN keeps the decimal 3, MAX takes this
                one), 1 (int), 1 (decimal: MIN keeps the integer 1), 4 (int)
    """
    gid = np.array([10, 20, 10, 30, 10, 30, 20, 10, 30, 30, 10, 30], np.int64)
    v = np.array([5, 0, 5, 3, 2.5, 3, 0, 0, 1, 1, 5, 4], np.float64)
    valid = np.array([1, 0, 3, 3, 3, 1, 0, 0, 1, 3, 1, 1], np.uint8)

    def word(last, sum_, mn, mx):
        return last | (sum_ << 4) | (mn << 8) | (mx << 10)

    want = np.array([
        word(1, 1, 1, 1),  # g10: 5
        word(3, 1, 3, 3),  # g20: absent -- an empty SUM is integral
        word(0, 0, 1, 0),  # g10: 5 decimal: LAST / MAX the later literal, MIN the earlier, SUM saw a decimal
        word(0, 0, 0, 0),  # g30: 3 decimal
        word(0, 0, 0, 0),  # g10: 2.5 decimal: the new MIN; MAX still the decimal 5
        word(1, 0, 0, 1),  # g30: 3: MAX tie takes it, MIN keeps the decimal
        word(3, 1, 3, 3),  # g20: absent again
        word(0, 0, 0, 0),  # g10: absent: nothing moves
        word(1, 0, 1, 1),  # g30: 1: the new MIN
        word(0, 0, 1, 1),  # g30: 1 decimal: LAST only, MIN keeps the integer 1
        word(1, 0, 0, 1),  # g10: 5: MAX tie takes it
        word(1, 0, 1, 1),  # g30: 4: the new MAX
    ], np.uint32)
    assert want.tolist() == [0x511, 0xF13, 0x100, 0x000, 0x000, 0x401, 0xF13, 0x000, 0x501, 0x500, 0x401, 0x501]
    got = litforms._prefix_forms(gid, v, valid, True)
    assert got.dtype == np.uint32
    assert got.tolist() == want.tolist()
    # the same literals as i64 values (2.5 -> 2: still the group's minimum)
    got = litforms._prefix_forms(gid, v.astype(np.int64), valid, False)
    assert got.tolist() == want.tolist()
