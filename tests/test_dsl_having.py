"""GPU: HAVING through the SQL dispatch mirror. The reference's #403 records
(RegressionSpec.hs:58-74, pinned in tests/golden/reference_kat.json) under
  SELECT SUM(a), COUNT(*) AS result, b FROM s GROUP BY b HAVING result > 2 EMIT CHANGES;
genFilteRNodeFromHaving behind the aggregate (Codegen.hs:524-529) forwards the
changelog rows whose result passes: rows 3 and 4 of the pinned four."""
import pytest

from hstream_amd import sql
from util import load_kat

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need cuda:0"
    from hstream_amd.engine import Engine
    e = Engine(device=0, batch_capacity=1 << 15)
    yield e
    e.close()


def test_sql_having_403_keeps_rows_3_and_4(eng):
    case = next(c for c in load_kat()["cases"] if c["name"] == "RegressionSpec#403_RAW")
    b = case["batch"]
    recs = [{"timestamp": t, "value": {"a": a, "b": 4}} for t, a in zip(b["ts"], b["cols"][0])]
    pinned = case["expect_changelog_aggs"]  # per record: SUM(a), a + 1, COUNT(*)
    assert len(recs) == len(pinned) == 4
    having = sql.RCondOp("RCompOpGT", sql.RExprCol("result", None, "result"), sql.RExprConst("2", 2))
    t = sql.gen_group_by_node(eng, [("SUM", "a"), ("COUNT(*)", "result"), ("COL", "b")], sql.RGroupBy("b"),
                              having=having)
    try:
        _, rows = t.process(recs)
        assert [(v["SUM(a)"], v["result"], v["b"]) for _, v in rows] == [(p[0], p[2], 4) for p in pinned[2:]]
        assert all(k == 4 or getattr(k, "twkKey", k) == 4 for k, _ in rows)
        st = t.op.stats()
        assert st["having_dropped"] == 2 and st["pending_rows"] == 0
        # the view is the aggregate's, unfiltered: the store sits before the filter
        dump = t.dump()
        assert [(v["SUM(a)"], v["result"], v["b"]) for _, v in dump] == [(pinned[3][0], pinned[3][2], 4)]
        # the same query without HAVING forwards all four
        t0 = sql.gen_group_by_node(eng, [("SUM", "a"), ("COUNT(*)", "result"), ("COL", "b")], sql.RGroupBy("b"))
        _, all_rows = t0.process(recs)
        assert [(v["SUM(a)"], v["result"], v["b"]) for _, v in all_rows] == [(p[0], p[2], 4) for p in pinned]
        assert [v for _, v in t0.dump()] == [v for _, v in dump]
        t0.close()
    finally:
        t.close()
