"""GPU: HAVING over per-batch changelogs whose batch is finished in more than
one step on the partition path (push_time_atomic): the emit chain the host had
not launched and runs after the fetch (a batch predicted direct that filled
the touched list: a hot key splits its bucket over workgroups), and the
hold-back for table room with its grow-and-rerun. Each batch is filtered once,
over its final rows. The reference is test_gpu_having's: the no-HAVING op
through the CPU oracle, its rows filtered on the host by sql.gen_filter_r.
Batches here exceed one aggregation chunk (32 768 records), so this engine is
larger than test_gpu_having's."""
import numpy as np
import pytest

from hstream_amd import abi
from hstream_amd.columnar import OpSpec
from test_gpu_having import check, cmp, col, const

pytestmark = pytest.mark.gpu

I = abi.HSG_I64
CA, S, MX = abi.HSG_COUNT_ALL, abi.HSG_SUM, abi.HSG_MAX
ALIASES = ["cnt", "s", "mx"]
AGGS = [(CA, 0), (S, 0), (MX, 0)]
# (a program the lean one-window kernels are built for: test_gpu_having's lean case)
LEAN_ALIASES = ["cnt", "s"]
LEAN_AGGS = [(CA, 0), (S, 0)]
T0 = 10_000_000
HOT = 7


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need cuda:0"
    from hstream_amd.engine import Engine
    e = Engine(device=0, batch_capacity=1 << 17)
    yield e
    e.close()


def _batches(seed, shapes, span):
    """(records, keys, share of the hot key) per batch; consecutive spans."""
    rng = np.random.default_rng(seed)
    out = []
    for b, (n, nkeys, hot) in enumerate(shapes):
        key = rng.integers(0, nkeys, size=n).astype(np.uint32)
        if hot:
            key[rng.random(n) < hot] = HOT
        ts = (T0 + b * span + np.sort(rng.integers(0, span, size=n))).astype(np.int64)
        out.append((key, ts, [rng.integers(-9, 10, size=n).astype(np.int64)], None))
    return out


# uniform batches leave the changelog to the apply (direct); ~70 000 records of
# one key are more than two aggregation chunks, so that bucket is split and its
# groups come from the touched list while the other buckets' rows stay direct
MIXED = [(60_000, 500, 0), (60_000, 500, 0), (100_000, 500, 0.7), (60_000, 500, 0), (100_000, 500, 0.7)]


def test_tumbling_direct_then_mixed_batches(eng):
    """A batch after a direct one is launched without the emit chain; when it
    turns out mixed the chain runs after the fetch and appends behind the rows
    the apply wrote. Those rows are filtered with the chain's, once."""
    spec = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=10_000, col_types=[I], aggs=LEAN_AGGS,
                  state_capacity=1 << 16)
    cond = cmp(">", col("cnt"), const(4))
    st, keeps, _ = check(eng, spec, cond, LEAN_ALIASES, _batches(31, MIXED, 200_000), what="mixed")
    print({k: st[k] for k in ("batches", "lean_batches", "direct_batches", "replays", "having_dropped_total")})
    assert st["lean_batches"] == st["batches"] == len(MIXED), st
    assert 2 <= st["direct_batches"] < len(MIXED) and st["replays"] >= 1, st
    assert all(0 < np.count_nonzero(k) < len(k) for k in keeps)


def test_hopping_direct_then_touched_list_batches(eng):
    """The same completion behind k_seg_apply (hopping: deferred window updates)."""
    spec = OpSpec(abi.HSG_HOPPING, abi.HSG_EMIT_PER_BATCH, size_ms=60_000, advance_ms=5_000, col_types=[I], aggs=AGGS,
                  state_capacity=1 << 18)
    shapes = [(40_000, 500, 0), (40_000, 500, 0), (100_000, 500, 0.7), (40_000, 500, 0)]
    cond = cmp(">", col("cnt"), const(28))
    st, keeps, _ = check(eng, spec, cond, ALIASES, _batches(32, shapes, 120_000), what="hopping")
    print({k: st[k] for k in ("batches", "lean_batches", "direct_batches", "replays", "having_dropped_total")})
    assert 1 <= st["direct_batches"] < len(shapes) and st["replays"] >= 1, st
    assert all(0 < np.count_nonzero(k) < len(k) for k in keeps)


def test_tumbling_batches_held_back_for_table_room(eng):
    """From a 2048-slot table: the first batch's groups exceed the room, so the
    lean apply holds back before claiming and the batch runs again on a grown
    table. The pass is idle at the held fetch and filters the rerun's rows."""
    spec = OpSpec(abi.HSG_TUMBLING, abi.HSG_EMIT_PER_BATCH, size_ms=10_000, col_types=[I], aggs=LEAN_AGGS,
                  state_capacity=1 << 10)
    shapes = [(40_000, 2_000, 0)] * 3  # ~20 000 groups a batch
    cond = cmp(">", col("cnt"), const(2))
    st, keeps, _ = check(eng, spec, cond, LEAN_ALIASES, _batches(33, shapes, 100_000), what="room")
    print({k: st[k] for k in ("batches", "lean_batches", "grow_events", "replays", "having_dropped_total")})
    assert st["lean_batches"] == len(shapes) and st["grow_events"] >= 1 and st["replays"] >= 1, st
    assert all(0 < np.count_nonzero(k) < len(k) for k in keeps)
