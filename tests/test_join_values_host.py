"""CPU: the host side of the valued stream-stream join (include/hstream_join.h
"valued join", hstream_amd/sql.py gen_joiner / gen_join_rows, processing.py
join_stream_rows): the joiner against hand vectors, the host mirror of the
JOIN plan against oracle/joinref.py on test_join.HAND_VECTORS, and the new
structs' layouts against the ctypes mirror."""
import ctypes
import os
import subprocess

import pytest

import joinref
from joinref import NONE
from hstream_amd import abi, engine, processing as P, sql
from test_join import HAND_VECTORS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- genJoiner (Internal/Codegen.hs:62-67) --------------------------------------------------
def test_gen_joiner_prefixes():
    assert sql.gen_joiner("s1", "s2", {"a": 1, "b": 2.5}, {"a": 7, "c": "x"}) == \
        {"s1.a": 1, "s1.b": 2.5, "s2.a": 7, "s2.c": "x"}
    assert sql.gen_joiner("left", "right", {}, {"v": None}) == {"right.v": None}
    assert sql.gen_joiner("s1", "s2", {}, {}) == {}
    # a field name that holds a dot is prefixed like any other
    assert sql.gen_joiner("s", "t", {"t.x": 1}, {"x": 2}) == {"s.t.x": 1, "t.x": 2}


def test_gen_joiner_self_join_is_left_biased():
    # HM.union keeps the left map's value: for equal names this side's wins
    assert sql.gen_joiner("s", "s", {"a": 1, "b": 2}, {"a": 9, "c": 3}) == {"s.a": 1, "s.b": 2, "s.c": 3}
    # (and "s.t" + "x" against "s" + "t.x" collide the same way)
    assert sql.gen_joiner("s", "s.t", {"t.x": 1}, {"x": 2}) == {"s.t.x": 1}


# ---- the host mirror against joinref ---------------------------------------------------------
def _records(steps):
    """HAND_VECTORS' records as the JOIN plan's: the handle travels as field h,
    the join key as field a (s1) / b (s2), absent for NONE"""
    out = []
    for (side, key, jk, ts, h), _ in steps:
        value = {"h": h}
        if jk != NONE:
            value["a" if side == 0 else "b"] = jk
        out.append({"stream": "s1" if side == 0 else "s2", "side": side, "key": None if key == NONE else key,
                    "value": value, "timestamp": ts})
    return out


@pytest.mark.parametrize("vec", HAND_VECTORS, ids=lambda v: v[0])
def test_join_stream_rows_match_joinref(vec):
    _, before, after, steps, _ = vec
    ref = joinref.JoinRef(before, after)
    exp = ref.push(*zip(*[rec for rec, _ in steps]))
    assert exp == [row for _, rows in steps for row in rows]
    recs = _records(steps)
    got = P.join_stream_rows(before, after, recs, "a", "b")
    assert [(recs[i]["value"]["h"], recs[k]["value"]["h"], recs[i]["value"]["a"], ts) for i, k, ts in got] == exp


@pytest.mark.parametrize("vec", HAND_VECTORS, ids=lambda v: v[0])
def test_gen_join_rows_match_joinref(vec):
    """joinref's rows with the joiner applied. The vectors' windows are in
    milliseconds and two are one-sided, so they go in as `windows`; those with
    before == after run through genJoinWindows too: `before` seconds, every
    timestamp times 1000 (the join has no scale of its own)."""
    _, before, after, steps, _ = vec
    exp = joinref.JoinRef(before, after).push(*zip(*[rec for rec, _ in steps]))
    runs = [(sql.RFromJoin("s1", "a", "s2", "b", 1), (before, after), 1)]
    if before == after:
        runs.append((sql.RFromJoin("s1", "a", "s2", "b", before), None, 1000))
    for frm, windows, scale in runs:
        recs = [dict(r, timestamp=r["timestamp"] * scale) for r in _records(steps)]
        got = sql.gen_join_rows(frm, recs, windows=windows)
        assert [(r["value"]["s1.h"], r["value"]["s2.h"], r["key"]["SelectedKey"], r["timestamp"]) for r in got] == \
            [(a, b, k, t * scale) for a, b, k, t in exp]
        for r in got:
            assert r["value"]["s1.a"] == r["value"]["s2.b"] == r["key"]["SelectedKey"]
            assert sorted(r["value"]) == ["s1.a", "s1.h", "s2.b", "s2.h"]


def test_gen_join_rows_refusals():
    with pytest.raises(ValueError):
        sql.gen_join_rows(sql.RFromJoin("s1", "a", "s2", "b", 1, "RJoinLeft"), [])
    with pytest.raises(ValueError):  # a self-join's records must say which side they are
        sql.gen_join_rows(sql.RFromJoin("s", "a", "s", "a", 1),
                          [{"stream": "s", "key": 1, "value": {"a": 1}, "timestamp": 0}])
    assert sql.gen_join_windows(sql.RFromJoin("s1", "a", "s2", "b", 7)) == (7000, 7000)


def test_self_join_rows():
    frm = sql.RFromJoin("s", "a", "s", "a", 10)
    recs = [{"stream": "s", "side": 1, "key": 1, "value": {"a": 5, "v": 1}, "timestamp": 1000},
            {"stream": "s", "side": 0, "key": 1, "value": {"a": 5, "v": 2, "w": 3}, "timestamp": 2000}]
    assert sql.gen_join_rows(frm, recs) == [
        {"key": {"SelectedKey": 5}, "value": {"s.a": 5, "s.v": 2, "s.w": 3}, "timestamp": 2000}]


# ---- layouts and symbols ---------------------------------------------------------------------
def test_layouts(tmp_path):
    src, exe = os.path.join(ROOT, "tests", "abi_layout_join_values.c"), str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    got = {k: int(v) for k, v in (ln.split(" ") for ln in subprocess.check_output([exe]).decode().strip().split("\n"))}
    for t in (abi.hsg_join_values, abi.hsg_join_cols, abi.hsg_join_joined):
        for name, _ in t._fields_:
            assert got[f"{t.__name__}.{name}"] == getattr(t, name).offset, (t.__name__, name)
        assert got[f"{t.__name__}.sizeof"] == ctypes.sizeof(t), t.__name__
    # the handle join's structs are as they were
    assert got["hsg_join_batch.sizeof"] == ctypes.sizeof(abi.hsg_join_batch) == 56
    assert got["hsg_join_rows.sizeof"] == ctypes.sizeof(abi.hsg_join_rows) == 48
    assert got["HSG_JOIN_MAX_COLS"] == abi.HSG_JOIN_MAX_COLS == 8


def test_symbols_are_declared_and_exported():
    names = ["hsg_join_create_valued", "hsg_join_push_valued", "hsg_join_drain_batch", "hsg_join_value_rows",
             "hsg_join_value_stride"]
    assert all(n in abi.JOIN_SYMBOLS for n in names)
    if not os.path.exists(engine.LIB_PATH):
        from hstream_amd import build
        build.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", engine.LIB_PATH]).decode()
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert all(n in have for n in names)


def test_value_stride():
    """the smallest power of two >= max(c0, c1) + 1, in {2, 4, 8, 16}; 0 for
    counts a valued join refuses (no GPU needed: the function is pure)"""
    from hstream_amd.join import value_stride
    want = {(0, 0): 2, (0, 1): 2, (1, 0): 2, (1, 1): 2, (2, 1): 4, (3, 1): 4, (3, 3): 4, (4, 4): 8, (1, 7): 8,
            (7, 1): 8, (8, 0): 16, (0, 8): 16, (5, 4): 0, (9, 0): 0, (-1, 1): 0, (8, 1): 0}
    for (c0, c1), s in want.items():
        assert value_stride(c0, c1) == s, (c0, c1)
