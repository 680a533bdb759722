"""CPU: the device decoder's scanner (hstream_amd/csrc/hsg_json.h), compiled
for the host and driven through hsg_json_fast_probe, against

  - a Python restatement of the fast subset (include/hstream_ingest.h "GPU
    ingest", the key-independent part): the accept set must equal it exactly,
    so a scanner that falls back on everything does not pass, and
  - the host decoder (hsg_decode_json_spelled on a fresh dictionary): every
    accepted record's column words and valid bytes are its, bit for bit.

Then the number grid over the HSG_F64 rule, the int64 edges, and the scanner
under the host sanitizers over every record and every prefix of each
(tools/json_fast_check.cpp, a stand-alone program)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import jsongen
from hstream_amd import abi
from hstream_amd.ingest import Decoder, FastProbe, KeyDict, pack_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the fast subset, restated ---------------------------------------------------
_WS = re.compile(rb"[ \t\n\r]*")
_STR = re.compile(rb'"([\x20\x21\x23-\x5b\x5d-\x7e]*)"')
_NUM = re.compile(rb"(-?)(0|[1-9][0-9]*)(?:\.([0-9]+))?(?:[eE]([+-]?)([0-9]+))?")
_LIT = re.compile(rb"true|false|null")


def _members(rec):
    """[(name, value)] of a record inside the subset's grammar, else None. A
    value is ('n', neg, int digits, fraction digits, exponent sign, exponent
    digits), ('s', bytes) or ('l', b'true' | b'false' | b'null')."""
    if len(rec) > abi.HSG_GPU_DEC_MAX_RECORD:
        return None
    pos = _WS.match(rec, 0).end()
    if rec[pos:pos + 1] != b"{":
        return None
    pos = _WS.match(rec, pos + 1).end()
    out = []
    if rec[pos:pos + 1] == b"}":
        pos += 1
    else:
        while True:
            pos = _WS.match(rec, pos).end()
            m = _STR.match(rec, pos)
            if not m:
                return None
            name = m.group(1)
            pos = _WS.match(rec, m.end()).end()
            if rec[pos:pos + 1] != b":":
                return None
            pos = _WS.match(rec, pos + 1).end()
            m = _STR.match(rec, pos)
            if m:
                val = ("s", m.group(1))
            else:
                m = _LIT.match(rec, pos)
                if m:
                    val = ("l", m.group(0))
                else:
                    m = _NUM.match(rec, pos)
                    if not m:
                        return None
                    val = ("n", m.group(1) == b"-", m.group(2), m.group(3) or b"", m.group(4) or b"", m.group(5) or b"")
            out.append((name, val))
            pos = _WS.match(rec, m.end()).end()
            c = rec[pos:pos + 1]
            pos += 1
            if c == b"}":
                break
            if c != b",":
                return None
    return out if _WS.match(rec, pos).end() == len(rec) else None


def _m_se(val):
    """(m, se) of a number inside the digit and exponent rule, else None."""
    _, _neg, ip, fp, esign, ed = val
    if len(ip) + len(fp) > 19 or len(ed) > 3:
        return None
    e = int(ed) if ed else 0
    return int(ip + fp), (-e if esign == b"-" else e) - len(fp)


def predict(rec, key_field, cols):
    """The subset's verdict on one record, without the key table."""
    mem = _members(rec)
    if mem is None:
        return False
    last = dict(mem)  # the last occurrence wins
    decoded = ([key_field] if key_field is not None else []) + [f for f, _, _ in cols]
    for f in decoded:
        v = last.get(f.encode())
        if v is not None and v[0] == "n" and _m_se(v) is None:
            return False
    if key_field is not None:
        k = last.get(key_field.encode())
        if k is None or (k[0] == "s" and len(k[1]) > abi.HSG_GPU_DEC_MAX_KEY):
            return False
    for f, ty, numeric in cols:
        v = last.get(f.encode())
        if v is None or not numeric:
            continue
        if v[0] != "n":
            return False
        m, se = _m_se(v)
        if ty == abi.HSG_F64:
            if m > 2**53 or se < -22 or se > 22:
                return False
        else:
            if se >= 0:
                q = m * 10**se
            elif m % 10**(-se):
                return False
            else:
                q = m // 10**(-se)
            q = -q if v[1] else q
            if q < -2**63 or q > 2**63 - 1:
                return False
    return True


# ---- shared state: the corpus, the probe's answers, the host decoder's ----------------
class _Corpus:
    def __init__(self, literal_forms):
        self.recs = jsongen.corpus()
        self.probe = FastProbe(jsongen.KEY_FIELD, jsongen.COLS, literal_forms=literal_forms)
        self.got = [self.probe(r) for r in self.recs]
        buf, off = pack_records(self.recs)
        self.host = Decoder(jsongen.KEY_FIELD, jsongen.COLS, literal_forms=literal_forms).decode(
            KeyDict(), buf, off, np.zeros(len(self.recs), np.int64), threads=4)


@pytest.fixture(scope="module", params=[True, False], ids=["forms", "noforms"])
def corp(request):
    return _Corpus(request.param)


def test_corpus_has_every_kind():
    recs = jsongen.corpus()
    assert len(recs) == 20_000
    blob = b"\x1e".join(recs)
    for needle in (b"\t", b"\n", b"\r", b"\\u006b", b"\\n", "é".encode(), b'{"a":1}', b"[1,2]"):
        assert needle in blob
    assert sum(len(r) > abi.HSG_GPU_DEC_MAX_RECORD for r in recs) >= 3
    assert sum(r.count(b'"v"') >= 2 for r in recs) > 100  # duplicate members


def test_accept_set_is_the_subset(corp):
    want = [predict(r, jsongen.KEY_FIELD, jsongen.COLS) for r in corp.recs]
    got = [bool(g.accept) for g in corp.got]
    diff = [i for i in range(len(want)) if want[i] != got[i]]
    assert not diff, [(i, corp.recs[i][:120], want[i], got[i]) for i in diff[:5]]
    # not a lazy scanner, not a credulous one
    assert 4000 < sum(got) < 16000, sum(got)


def test_accepted_words_are_the_host_decoders(corp):
    _key, _ts, cols, valid, status, _rej = corp.host
    words = [c.view(np.uint64) for c in cols]
    n_acc = 0
    for i, g in enumerate(corp.got):
        if not g.accept:
            continue
        n_acc += 1
        assert status[i] == abi.HSG_DEC_OK, (i, corp.recs[i], status[i])
        for c in range(len(jsongen.COLS)):
            assert g.valid[c] == valid[c][i], (i, c, corp.recs[i])
            assert g.words[c] == int(words[c][i]), (i, c, corp.recs[i], hex(g.words[c]), hex(int(words[c][i])))
    assert n_acc > 4000


def test_key_class_matches_the_dictionary():
    """The key's class as the scanner reports it names the dictionary's
    equality classes: equal (tag, sign, m, e) or equal string bytes iff the
    host decoder gave equal key ids."""
    recs = jsongen.corpus()
    probe = FastProbe(jsongen.KEY_FIELD, jsongen.COLS)
    buf, off = pack_records(recs)
    key, *_ = Decoder(jsongen.KEY_FIELD, jsongen.COLS).decode(KeyDict(), buf, off, np.zeros(len(recs), np.int64))
    by_class, by_id = {}, {}
    for i, r in enumerate(recs):
        g = probe(r)
        if not g.accept:
            continue
        tag = chr(g.key_tag)
        cls = (tag, g.key_neg, g.key_m, g.key_e) if tag == "n" else \
            (tag, bytes(r[g.key_off:g.key_off + g.key_len])) if tag == "s" else (tag,)
        assert by_class.setdefault(cls, int(key[i])) == int(key[i]), (i, r, cls)
        assert by_id.setdefault(int(key[i]), cls) == cls, (i, r, cls)
    assert len(by_class) > 60


def _probe_numbers(lits, ty, literal_forms=True):
    probe = FastProbe(None, [("x", ty, True)], literal_forms=literal_forms)
    dec = Decoder(None, [("x", ty, True)], literal_forms=literal_forms)
    recs = [b'{"x":' + s.encode() + b"}" for s in lits]
    buf, off = pack_records(recs)
    _key, _ts, cols, valid, status, _rej = dec.decode(None, buf, off, np.zeros(len(recs), np.int64), threads=2)
    return recs, [probe(r) for r in recs], cols[0].view(np.uint64), valid[0], status


def test_number_grid_f64():
    lits = jsongen.number_grid()
    assert len(lits) >= 10_000
    recs, got, words, valid, status = _probe_numbers(lits, abi.HSG_F64)
    cols = [("x", abi.HSG_F64, True)]
    n_acc = 0
    for i, g in enumerate(got):
        assert bool(g.accept) == predict(recs[i], None, cols), (lits[i], g.accept)
        if g.accept:
            n_acc += 1
            assert status[i] == abi.HSG_DEC_OK
            assert g.words[0] == int(words[i]), (lits[i], hex(g.words[0]), hex(int(words[i])))
            assert g.valid[0] == valid[i], lits[i]
    assert 2000 < n_acc < len(lits) - 2000, n_acc
    acc = {lits[i]: bool(g.accept) for i, g in enumerate(got)}
    p53 = 2**53
    for s, want in ((str(p53), True), (str(p53 + 1), False), (f"{p53}e22", True), (f"{p53}e-22", True),
                    (f"{p53}e23", False), (f"{p53}e-23", False), ("1e22", True), ("1e23", False), ("1e-22", True),
                    ("1e-23", False), ("-0", True), ("-0.0", True), ("0e5", True), ("0.000", True), ("1E+07", True),
                    ("1e007", True), ("1e0007", False), ("1234567890123456789", False),
                    ("0.000000000000000000", True), ("0.0000000000000000000", False),
                    ("12345678901234567890", False), ("1234567890.123456789", False), ("0.1", True)):
        assert acc[s] == want, s
    # -0 stays -0.0, as strtod gives it
    for s in ("-0", "-0.0"):
        assert got[lits.index(s)].words[0] == 0x8000000000000000, s


def test_i64_edges():
    lits = list(jsongen.I64_EDGES)
    for forms in (True, False):
        recs, got, words, valid, status = _probe_numbers(lits, abi.HSG_I64, literal_forms=forms)
        cols = [("x", abi.HSG_I64, True)]
        for i, g in enumerate(got):
            assert bool(g.accept) == predict(recs[i], None, cols), lits[i]
            if g.accept:
                assert status[i] == abi.HSG_DEC_OK, lits[i]
                assert g.words[0] == int(words[i]) and g.valid[0] == valid[i], (lits[i], g.words[0], int(words[i]))
            else:
                # outside the subset for a reason the host decoder names, or by the digit rule
                assert status[i] in (abi.HSG_DEC_NOT_INTEGRAL, abi.HSG_DEC_RANGE) or len(re.sub(r"\D", "", lits[i].split("e")[0])) > 19, lits[i]
        acc = {lits[i]: bool(g.accept) for i, g in enumerate(got)}
        for s, want in (("9223372036854775807", True), ("-9223372036854775808", True), ("9223372036854775808", False),
                        ("1e18", True), ("1e19", False), ("10e-1", True), ("1.5", False),
                        ("92233720368547758070e-1", False), ("9223372036854775.807e3", True),
                        ("9223372036854775.808e3", False), ("-9223372036854775.808e3", True), ("100e-3", False),
                        ("1000000000000000000e-18", True), ("0e30", True), ("0e-30", True)):
            assert acc[s] == want, s
        w = {lits[i]: g.words[0] for i, g in enumerate(got) if g.accept}
        assert w["9223372036854775807"] == 2**63 - 1 and w["-9223372036854775808"] == 2**63 and w["10e-1"] == 1


def test_ctypes_layout_matches_c(tmp_path):
    import ctypes as C
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "abi_layout_ingest.c")])
    types = {"hsg_gpu_decode_stats": abi.hsg_gpu_decode_stats, "hsg_json_probe": abi.hsg_json_probe,
             "hsg_sink_spellings": abi.hsg_sink_spellings}
    lines = [ln.split() for ln in subprocess.check_output([exe]).decode().splitlines() if ln.strip()]
    assert len(lines) == 23
    for k, v in lines:
        t, m = k.split(".")
        assert (C.sizeof(types[t]) if m == "sizeof" else getattr(types[t], m).offset) == int(v), k


def test_configuration_limits():
    with pytest.raises(abi.HStreamGpuError) as ei:
        FastProbe("k", [(f"c{j}", abi.HSG_I64, True) for j in range(9)])
    assert ei.value.status == abi.HSG_E_INVALID
    with pytest.raises(abi.HStreamGpuError):
        FastProbe("k" * 65, [])
    with pytest.raises(abi.HStreamGpuError):
        FastProbe("k", [("é", abi.HSG_I64, True)])
    FastProbe("k" * 64, [(f"c{j}", abi.HSG_I64, True) for j in range(8)])


def test_scanner_under_sanitizers(tmp_path):
    """tools/json_fast_check.cpp with -fsanitize=address,undefined: every
    record and every prefix of each in an exact-size heap block. Its accept
    count is the probe's."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "json_fast_check")
    # the runtimes linked into the program: it needs nothing preloaded and runs whatever else is
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           *static, "-I", os.path.join(ROOT, "hstream_amd", "csrc"),
                           os.path.join(ROOT, "tools", "json_fast_check.cpp"), "-o", exe])
    recs = jsongen.corpus()
    path = str(tmp_path / "corpus.bin")
    jsongen.write_corpus_file(path, jsongen.KEY_FIELD, jsongen.COLS, True, recs)
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    m = re.match(r"records (\d+) accepted (\d+) prefixes (\d+) prefix_accepted (\d+)", out.stdout)
    assert m, out.stdout
    probe = FastProbe(jsongen.KEY_FIELD, jsongen.COLS, literal_forms=True)
    assert int(m.group(1)) == len(recs)
    assert int(m.group(2)) == sum(int(probe(r).accept) for r in recs)
    assert int(m.group(3)) == sum(len(r) for r in recs)
