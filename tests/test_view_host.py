"""Host side of keyed view reads, no GPU: hsg_keydict_find (a lookup that
never inserts, so a view query for an unknown key leaves the dictionary as it
is) in both dictionaries, and the shape of the answer to SELECT ... FROM view
WHERE key = x (SelectViewPlan, hstream/src/HStream/Server/Handler.hs:287-323)."""
import ctypes as C

import numpy as np
import pytest

from hstream_amd import abi, ingest, processing
from hstream_amd.columnar import Rows
from hstream_amd.processing import TimeWindow, TimeWindowKey, select_view_result


def test_native_find_uses_aeson_equality_and_never_inserts():
    d = ingest.KeyDict()
    one, a, obj = d.encode_json("1"), d.encode_json('"a"'), d.encode_json('{"k":[1,2]}')
    assert (one, a, obj) == (0, 1, 2) and len(d) == 3
    assert d.find_json("1.0") == one          # Aeson Numbers are Scientific: 1 == 1.0
    assert d.find_json("10e-1") == one
    assert d.find_json(' "a" ') == a
    assert d.find_json('{ "k" : [1.0, 2] }') == obj
    assert d.find_json("2") == abi.HSG_KEY_NONE
    assert d.find_json('"1"') == abi.HSG_KEY_NONE  # a string is not a number
    assert d.find_json('{"k":[2,1]}') == abi.HSG_KEY_NONE
    for i in range(100):
        assert d.find(i + 5) == abi.HSG_KEY_NONE
        assert d.find(1.0) == one
    assert len(d) == 3                         # unchanged by any number of finds
    assert d.encode_json("2") == 3             # ids go on in first-seen order
    assert d.find_json("2.0") == 3
    d.close()


@pytest.mark.parametrize("text", ["{", "[1,", "1 2", "", "nul", '"a'])
def test_native_find_malformed_text_gives_encodes_error(text):
    d = ingest.KeyDict()
    L = d._L
    b = text.encode()
    out = C.c_uint32(7)
    rc_enc = L.hsg_keydict_encode(d._h, b, len(b), C.byref(out))
    rc_find = L.hsg_keydict_find(d._h, b, len(b), C.byref(out))
    assert rc_enc == abi.HSG_E_INVALID and rc_find == rc_enc
    assert len(d) == 0
    with pytest.raises(abi.HStreamGpuError):
        d.find_json(text)
    # null arguments, as encode
    assert L.hsg_keydict_find(None, b"1", 1, C.byref(out)) == abi.HSG_E_INVALID
    assert L.hsg_keydict_find(d._h, b"1", 1, None) == abi.HSG_E_INVALID
    d.close()


def test_python_find_behaves_the_same():
    d = processing.KeyDict()
    one, a, obj = d.encode(1), d.encode("a"), d.encode({"k": [1, 2]})
    assert d.find(1.0) == one and d.find("a") == a and d.find({"k": [1.0, 2]}) == obj
    assert d.find(2) == abi.HSG_KEY_NONE and d.find("1") == abi.HSG_KEY_NONE and d.find(True) == abi.HSG_KEY_NONE
    for i in range(100):
        assert d.find(i + 5) == abi.HSG_KEY_NONE
    assert len(d) == 3
    assert d.encode(2) == 3 and d.find(2.0) == 3


def _rows(starts, ends, aggs):
    n = len(starts)
    return Rows(np.full(n, 7, np.uint32), np.asarray(starts, np.int64), np.asarray(ends, np.int64),
                np.full(n, -1, np.int64), [np.asarray(a) for a in aggs])


def test_select_view_fixed_windows():
    """Handler.hs:299-312: one member per window start, "winStart = S ,winEnd = E"
    with E = S + size, in start order."""
    rows = _rows([20_000, 0, 10_000], [30_000, 10_000, 20_000], [np.asarray([3, 1, 2]), np.asarray([2.5, 0.5, 1.5])])
    got = select_view_result(rows, True, False, 10_000, names=["c", "s"])
    assert list(got.items()) == [("winStart = 0 ,winEnd = 10000", {"c": 1, "s": 0.5}),
                                 ("winStart = 10000 ,winEnd = 20000", {"c": 2, "s": 1.5}),
                                 ("winStart = 20000 ,winEnd = 30000", {"c": 3, "s": 2.5})]
    # hopping: the end is start + size whatever the advance
    rows = _rows([0, 3_000], [10_000, 13_000], [np.asarray([1, 2])])
    assert select_view_result(rows, True, False, 10_000) == {"winStart = 0 ,winEnd = 10000": {"0": 1},
                                                            "winStart = 3000 ,winEnd = 13000": {"0": 2}}
    # Table.get's pairs
    pairs = [(TimeWindowKey("k", TimeWindow(5_000, 6_000)), {"n": 4})]
    assert select_view_result(pairs, True, False, 1_000) == {"winStart = 5000 ,winEnd = 6000": {"n": 4}}
    # no row: the empty object (sendResp (Just mempty))
    assert select_view_result(_rows([], [], [np.asarray([], np.int64)]), True, False, 10_000) == {}
    assert select_view_result([], True, False, 10_000) == {}


def test_select_view_sessions():
    """Handler.hs:315-323: "winStart = S" per session, sorted by start."""
    rows = _rows([900, 100], [1_500, 400], [np.asarray([9, 1])])
    got = select_view_result(rows, True, True, 0, names=["n"])
    assert list(got.items()) == [("winStart = 100", {"n": 1}), ("winStart = 900", {"n": 9})]
    pairs = [(TimeWindowKey("k", TimeWindow(100, 400)), {"n": 1})]
    assert select_view_result(pairs, True, True, 0) == {"winStart = 100": {"n": 1}}
    assert select_view_result(_rows([], [], [np.asarray([], np.int64)]), True, True, 0) == {}
    assert select_view_result([], True, True, 0) == {}


def test_select_view_unwindowed():
    """Handler.hs:313: ksGet key store -- the key's values, or nothing."""
    rows = _rows([0], [0], [np.asarray([5]), np.asarray([1.25])])
    assert select_view_result(rows, False, False, 0, names=["c", "avg"]) == {"c": 5, "avg": 1.25}
    assert select_view_result([("k", {"c": 5})], False, False, 0) == {"c": 5}
    assert select_view_result(_rows([], [], [np.asarray([], np.int64)]), False, False, 0) is None
    assert select_view_result([], False, False, 0) is None
