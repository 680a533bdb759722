"""Seeded JSON record generators for the device-ingest tests
(test_ingest_fast_host.py, test_gpu_ingest.py) and tools/ingest_ab.py, and the
corpus file tools/json_fast_check.cpp reads.

The messy corpus mixes, by construction, every kind of text the fast subset
(include/hstream_ingest.h "GPU ingest") has to tell apart: every whitespace
kind, duplicate members, a key field that is also a column, presence-only
columns, escapes in names and values, non-ASCII bytes, nested values,
truncated records, trailing garbage and over-long records."""
import struct

import numpy as np

from hstream_amd import abi

KEY_FIELD = "k"
# (field, type, numeric): two columns read "v", the key field is a column too
# (presence only: a string key must not reject the record), "p" is presence only
COLS = [("v", abi.HSG_I64, True), ("x", abi.HSG_F64, True), ("p", abi.HSG_I64, False),
        ("k", abi.HSG_F64, False), ("v", abi.HSG_F64, True)]

_WS = [b"", b"", b"", b" ", b"\t", b"\n", b"\r", b"  ", b" \r\n\t"]


def _ws(rng):
    return _WS[int(rng.integers(0, len(_WS)))]


def _int_lit(rng):
    k = int(rng.integers(0, 8))
    if k == 0:
        return str(int(rng.integers(-10**18, 10**18)))
    if k == 1:
        return str(int(rng.integers(-5, 6)))
    return str(int(rng.integers(-10**6, 10**6)))


def _num_lit(rng):
    k = int(rng.integers(0, 12))
    if k <= 3:
        return _int_lit(rng)
    if k <= 6:
        return f"{int(rng.integers(-10**5, 10**5))}.{int(rng.integers(0, 10**4)):0{int(rng.integers(1, 5))}d}"
    if k == 7:
        return f"{int(rng.integers(1, 1000))}{'eE'[int(rng.integers(0, 2))]}{['', '+', '-'][int(rng.integers(0, 3))]}" \
               f"{int(rng.integers(0, 30))}"
    if k == 8:
        return f"{int(rng.integers(0, 100))}.{int(rng.integers(0, 100))}e{int(rng.integers(-25, 25))}"
    if k == 9:  # long: more than 19 digits, or a long exponent
        return ["123456789012345678901", "0.12345678901234567890", "1e0007", "12345678901234567890123.5"][
            int(rng.integers(0, 4))]
    if k == 10:
        return ["-0", "-0.0", "0e5", "0.000", "1E+07", "9007199254740993", "9223372036854775808", "1e19", "1.5",
                "10e-1"][int(rng.integers(0, 10))]
    return ["01", "1.", ".5", "-", "1e", "+1", "0x10", "1e+", "--1", "1.e3"][int(rng.integers(0, 10))]  # malformed


def _str_lit(rng):
    k = int(rng.integers(0, 10))
    if k <= 5:
        n = int(rng.integers(0, 12))
        return b'"' + bytes(rng.choice(list(b"abcXYZ 0123_-:/{}[],"), size=n).astype(np.uint8)) + b'"'
    if k == 6:
        return [b'"a\\nb"', b'"q\\"uote"', b'"\\u0041"', b'"back\\\\slash"', b'"bad\\x"'][int(rng.integers(0, 5))]
    if k == 7:
        return ['"café"'.encode(), '"日本"'.encode(), b'"\xff\xfe"'][int(rng.integers(0, 3))]
    if k == 8:
        return [b'"tab\there"', b'"nul\x00"', b'"del\x7f"'][int(rng.integers(0, 3))]
    return b'"' + b"y" * int(rng.integers(40, 70)) + b'"'


def _key_lit(rng):
    k = int(rng.integers(0, 12))
    if k <= 4:
        return str(int(rng.integers(0, 40))).encode()
    if k == 5:
        return [b"1", b"1.0", b"10e-1", b"1E0", b"100e-2", b"2.50", b"25e-1", b"-0", b"0.0"][int(rng.integers(0, 9))]
    if k <= 8:
        return b'"u%d"' % int(rng.integers(0, 25))
    if k == 9:
        return [b"true", b"false", b"null"][int(rng.integers(0, 3))]
    if k == 10:
        return [b'{"a":1}', b"[1,2]", b"123456789012345678901234567890", b'"' + b"z" * 60 + b'"',
                b'"k\\u0031"', '"ü"'.encode()][int(rng.integers(0, 6))]
    return _value(rng)


def _value(rng):
    k = int(rng.integers(0, 14))
    if k <= 6:
        return _num_lit(rng).encode()
    if k <= 9:
        return _str_lit(rng)
    if k == 10:
        return [b"true", b"false", b"null"][int(rng.integers(0, 3))]
    if k == 11:
        return [b"tru", b"nul", b"False", b"nil", b""][int(rng.integers(0, 5))]
    return [b"{}", b"[]", b'{"a":[1,{"b":2}]}', b"[1, 2, 3]", b'{"v":1}', b"[[", b'{"a":}'][int(rng.integers(0, 7))]


_NAMES = [b'"k"', b'"v"', b'"x"', b'"p"', b'"a"', b'"bb"', b'"other"', b'"kk"', b'"K"', b'""']
_ODD_NAMES = [b'"\\u006b"', b'"v\\u0000"', '"é"'.encode(), b'"' + b"n" * 70 + b'"', b"k", b"'v'"]


def _record(rng):
    m = []
    nm = int(rng.integers(0, 7))
    have_key = rng.random() < 0.9
    names = []
    if have_key:
        names.append(b'"k"')
    for _ in range(nm):
        if rng.random() < 0.04:
            names.append(_ODD_NAMES[int(rng.integers(0, len(_ODD_NAMES)))])
        else:
            names.append(_NAMES[int(rng.integers(0, len(_NAMES)))])
    rng.shuffle(names)
    for name in names:
        if name == b'"k"':
            val = _key_lit(rng)
        elif name in (b'"v"', b'"x"') and rng.random() < 0.85:
            val = _num_lit(rng).encode() if name == b'"x"' or rng.random() < 0.3 else _int_lit(rng).encode()
        else:
            val = _value(rng)
        m.append(_ws(rng) + name + _ws(rng) + b":" + _ws(rng) + val + _ws(rng))
    rec = _ws(rng) + b"{" + b",".join(m) + (_ws(rng) if not m else b"") + b"}" + _ws(rng)
    r = rng.random()
    if r < 0.03 and len(rec) > 1:
        rec = rec[: int(rng.integers(0, len(rec)))]               # truncated
    elif r < 0.06:
        rec += [b"x", b"}", b",", b"{}", b"\x00", b" 1"][int(rng.integers(0, 6))]  # trailing garbage
    elif r < 0.07:
        rec = rec.replace(b"}", b",}", 1) if rng.random() < 0.5 else rec.replace(b":", b"::", 1)
    elif r < 0.072:
        rec = [b"", b" ", b"[]", b"1", b'"s"', b"null", b"{", b"}"][int(rng.integers(0, 8))]
    return rec


def _over_long(rng, total):
    """A well-formed record of exactly `total` bytes (long by whitespace or by
    an ignored string member)."""
    head = b'{"k":%d,"v":%d,"x":%d.5' % (int(rng.integers(0, 40)), int(rng.integers(0, 99)), int(rng.integers(0, 99)))
    if rng.random() < 0.5:
        return head + b" " * (total - len(head) - 1) + b"}"
    pad = total - len(head) - len(b',"pad":""}')
    return head + b',"pad":"' + b"w" * pad + b'"}'


def corpus(seed=2024, n=20_000):
    """The seeded messy corpus: n records, a handful of them at and around
    HSG_GPU_DEC_MAX_RECORD bytes."""
    rng = np.random.default_rng(seed)
    recs = [_record(rng) for _ in range(n)]
    big = abi.HSG_GPU_DEC_MAX_RECORD
    for j, total in enumerate((big, big + 1, big - 1, big + 1, 2 * big, big)):
        recs[(j + 1) * (n // 8)] = _over_long(rng, total)
    return recs


def lit_of(m, se, rng, neg=False):
    """A JSON literal whose coefficient is m and Scientific exponent se, in a
    randomly chosen spelling: fraction digits (with leading zeros as in
    0.00012) and / or an exponent part."""
    digits = str(m)
    if rng.random() < 0.15:
        ip, fp = "0", "0" * int(rng.integers(0, 4)) + digits
    else:
        nfrac = int(rng.integers(0, len(digits)))
        ip, fp = digits[: len(digits) - nfrac], digits[len(digits) - nfrac:]
    exp = se + len(fp)
    s = ("-" if neg else "") + ip + ("." + fp if fp else "")
    if exp != 0 or rng.random() < 0.2:
        s += "eE"[int(rng.integers(0, 2))] + (["", "+"][int(rng.integers(0, 2))] if exp >= 0 else "") + str(exp)
    return s


def number_grid(seed=7, n=10_000):
    """Number literals over the HSG_F64 rule: n random (m, se) draws around
    its limits, then the named edge cases."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        k = int(rng.integers(0, 6))
        if k == 0:
            m = int(rng.integers(0, 2**53 + 1, dtype=np.uint64))
        elif k == 1:
            m = 2**53 + int(rng.integers(-3, 4))
        elif k == 2:
            m = int(rng.integers(0, 10**6))
        elif k == 3:
            m = int(rng.integers(0, 10**19, dtype=np.uint64))
        elif k == 4:
            m = int(rng.integers(1, 10**4)) * 10 ** int(rng.integers(0, 12))
        else:
            m = int(rng.integers(10**15, 10**16))
        se = int(rng.integers(-26, 27)) if rng.random() < 0.8 else int(rng.choice([-23, -22, 22, 23, -1, 0, 1]))
        out.append(lit_of(m, se, rng, neg=rng.random() < 0.3))
    p53 = 2**53
    out += [str(p53), str(p53 + 1), f"-{p53}", f"{p53}e22", f"{p53}e-22", f"{p53}e23", f"{p53}e-23", f"{p53 + 1}e-5",
            "1e22", "1e-22", "1e23", "1e-23", "9007199254740991e22", "123e-22", "-0", "-0.0", "0e5", "0.0e-5", "-0e-30",
            "0.000", "0.0000000000000000001", "0.00000000000000000001", "0.000000000000000000", "0.0000000000000000000",
            "1E+07", "1.5E+07", "2e-07", "1e007", "1e0007", "1234567890123456789", "12345678901234567890",
            "1234567890.123456789", "1234567890.1234567890", "0.1", "0.3", "2.675", "1.005", "123456.789e3",
            "9007199254740993", "4503599627370497.5", "0.1e1", "5e-324", "1.7976931348623157e308", "3.14159"]
    return out


I64_EDGES = ["9223372036854775807", "-9223372036854775808", "9223372036854775808", "-9223372036854775809", "1e18",
             "1e19", "-1e19", "9e18", "10e-1", "1.5", "92233720368547758070e-1", "9223372036854775807e0",
             "922337203685477580.7e1", "9223372036854775.807e3", "9223372036854775.808e3", "-9223372036854775.808e3",
             "100e-2", "100e-3", "0.0", "-0", "0e30", "0e-30", "5e-1", "1e-19", "1000000000000000000e-18",
             "1000000000000000000e-19", "12e17", "92e17", "93e17", "1.0e0", "7E0", "123.000"]


def c2_records(seed, n, n_keys=4096, key_base=0):
    """Clean C2-shaped records: an integer key, an i64 field, a decimal field."""
    rng = np.random.default_rng(seed)
    k = rng.integers(key_base, key_base + n_keys, n)
    v = rng.integers(-10**6, 10**6, n)
    x = rng.integers(-10**6, 10**6, n)
    return [b'{"k":%d,"v":%d,"x":%d.%02d}' % (int(k[i]), int(v[i]), int(x[i]) // 100, abs(int(x[i])) % 100)
            for i in range(n)]


def write_corpus_file(path, key_field, cols, literal_forms, records):
    """The file tools/json_fast_check.cpp reads: little-endian u32 words and
    raw bytes -- magic, keyless, literal_forms, n_cols, the key field (len,
    bytes), each column (type, numeric, len, bytes), the record count, each
    record (len, bytes)."""
    with open(path, "wb") as f:
        kf = (key_field or "").encode()
        f.write(struct.pack("<4I", 0x4A534643, 0 if key_field is not None else 1, 1 if literal_forms else 0, len(cols)))
        f.write(struct.pack("<I", len(kf)) + kf)
        for name, ty, num in cols:
            nb = name.encode()
            f.write(struct.pack("<3I", ty, 1 if num else 0, len(nb)) + nb)
        f.write(struct.pack("<I", len(records)))
        for r in records:
            f.write(struct.pack("<I", len(r)) + r)
