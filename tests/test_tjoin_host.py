"""Stream-table join (hsg_table_join), the parts that need no GPU: the ABI
surface, the argument checks that come before any device work, and the pure
assembly of the joined records (processing.join_table_result), which is
joinTableProcessor's forward (hstream-processing/src/HStream/Processing/
Stream.hs:334-344) given the table's answer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hstream_amd import abi, engine, processing as P
from hstream_amd.columnar import Rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["hsg_table_join", "hsg_table_join_tile"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        from hstream_amd import build
        build.build()
    return engine.load_library()


def test_symbols_listed_and_exported(lib):
    assert set(SYMBOLS) <= set(abi.EXPORTED_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "hstream_gpu.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
    assert "hsg_probe;" in header
    out = subprocess.check_output(["nm", "-D", "--defined-only", engine.LIB_PATH]).decode()
    exported = set(re.findall(r" T (hsg_\w+)", out))
    assert set(SYMBOLS) <= exported


def test_probe_struct_layout(tmp_path):
    """The ctypes hsg_probe against the header's, as a C compiler lays it out;
    hsg_stats keeps its size (the join adds no field)."""
    fields = ["n", "mem", "reserved", "key_id", "ready_event"]
    assert [n for n, _ in abi.hsg_probe._fields_] == fields
    src, exe = str(tmp_path / "probe.c"), str(tmp_path / "probe")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "hstream_gpu.h"\nint main(void) {\n')
        for name in fields:
            f.write('  printf("%s %%zu\\n", offsetof(hsg_probe, %s));\n' % (name, name))
        f.write('  printf("size %zu\\n", sizeof(hsg_probe));\n  printf("stats %zu\\n", sizeof(hsg_stats));\n')
        f.write("  return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    got = {k: int(v) for k, v in (ln.split(" ") for ln in subprocess.check_output([exe]).decode().strip().split("\n"))}
    for name in fields:
        assert got[name] == getattr(abi.hsg_probe, name).offset, name
    assert got["size"] == C.sizeof(abi.hsg_probe) == 32
    assert got["stats"] == C.sizeof(abi.hsg_stats)


def test_null_table_is_invalid(lib):
    keys = np.arange(4, dtype=np.uint32)
    probe = abi.hsg_probe(n=4, mem=abi.HSG_MEM_HOST, reserved=0, key_id=keys.ctypes.data)
    rows = abi.hsg_rows(capacity=0, mem=abi.HSG_MEM_HOST, n_aggs=0)
    got = C.c_uint64(7)
    assert lib.hsg_table_join(None, C.byref(probe), C.byref(rows), C.byref(got)) == abi.HSG_E_INVALID
    assert lib.hsg_table_join(None, None, C.byref(rows), C.byref(got)) == abi.HSG_E_INVALID
    assert lib.hsg_table_join(None, C.byref(probe), None, None) == abi.HSG_E_INVALID
    assert got.value == 7


def test_tile_is_a_positive_multiple_of_the_wave(lib):
    t = lib.hsg_table_join_tile()
    assert t > 0 and t % 64 == 0
    assert engine.table_join_tile() == t


def test_make_probe_host_keys():
    probe, keep = engine.make_probe([3, 1, abi.HSG_KEY_NONE])
    assert (probe.n, probe.mem, probe.reserved) == (3, abi.HSG_MEM_HOST, 0)
    assert keep.dtype == np.uint32 and probe.key_id == keep.ctypes.data
    probe, keep = engine.make_probe([])
    assert probe.n == 0 and not probe.key_id


# ---- join_table_result -------------------------------------------------------------------------
def _rows(src, key, a, b):
    n = len(src)
    return Rows(np.asarray(key, np.uint32), np.zeros(n, np.int64), np.zeros(n, np.int64), np.asarray(src, np.int64),
                [np.asarray(a, np.int64), np.asarray(b, np.float64)])


RECORDS = [{"timestamp": 100 + i, "value": {"key": k, "x": i}} for i, k in enumerate(["a", "b", "a", "zz", "c", "a"])]


def _joiner(v1, v2):
    return {"x": v1["x"], **v2}


def test_result_follows_src_index_order():
    # rows handed over out of order: the result is in arrival (src_index) order
    rows = _rows([4, 0, 1], [2, 0, 1], [30, 10, 20], [3.5, 1.5, 2.5])
    out = P.join_table_result(RECORDS, rows, ["n", "f"], _joiner)
    assert out == [
        {"key": "a", "value": {"x": 0, "n": 10, "f": 1.5}, "timestamp": 100},
        {"key": "b", "value": {"x": 1, "n": 20, "f": 2.5}, "timestamp": 101},
        {"key": "c", "value": {"x": 4, "n": 30, "f": 3.5}, "timestamp": 104},
    ]


def test_result_duplicate_keys_each_get_their_row():
    rows = _rows([0, 2, 5], [0, 0, 0], [10, 10, 10], [1.5, 1.5, 1.5])
    out = P.join_table_result(RECORDS, rows, ["n", "f"], _joiner)
    assert [r["timestamp"] for r in out] == [100, 102, 105]
    assert [r["value"]["x"] for r in out] == [0, 2, 5]
    assert all(r["key"] == "a" and r["value"]["n"] == 10 for r in out)


def test_result_no_matches():
    assert P.join_table_result(RECORDS, _rows([], [], [], []), ["n", "f"], _joiner) == []


def test_joiner_sees_stream_value_and_aliased_row():
    seen = []

    def joiner(v1, v2):
        seen.append((v1, v2))
        return "joined"

    rows = _rows([3], [9], [7], [0.25])
    out = P.join_table_result(RECORDS, rows, ["count", "avg"], joiner)
    assert seen == [(RECORDS[3]["value"], {"count": 7, "avg": 0.25})]
    assert seen[0][0] is RECORDS[3]["value"]
    assert type(seen[0][1]["count"]) is int and type(seen[0][1]["avg"]) is float
    assert out == [{"key": "zz", "value": "joined", "timestamp": 103}]


def test_result_key_field_names_the_stream_key():
    recs = [{"timestamp": 1, "value": {"user": "u1", "x": 5}}]
    out = P.join_table_result(recs, _rows([0], [0], [1], [1.0]), ["n", "f"], _joiner, key_field="user")
    assert out[0]["key"] == "u1"
