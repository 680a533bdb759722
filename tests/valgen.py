"""Adversarial value columns for the parity tests (seeded, numpy only).

The suite's generators keep values near 1e0 .. 1e9; here every int64 has a
live high word and every f64 class reaches the ends of the format. Four
column classes, picked by what aggregates read the column:

  i64 under SUM / AVG   i64_wide, and i64_crossing on the dedicated keys
  i64 otherwise         i64_extreme (MIN / MAX / LAST / COUNT only)
  f64 under SUM / AVG   f64_samesign, and f64_subnormal on the dedicated keys
  f64 otherwise         f64_extreme (MIN / MAX / LAST / COUNT only)

`Planter` builds a batch's columns and gives a few positions to four dedicated
keys (disjoint from the shape's own): one that sees only the MIN identity
(INT64_MAX, doubles >= 2^63), one only the MAX identity, one both, one only
absent fields. In SUM columns those keys hold the crossing / subnormal values.
"""
import numpy as np

from hstream_amd import abi

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
KEY_NONE = 0xFFFFFFFF
_KS = (1, 3, 0x7F, 0xFF)  # k << 32 stays below 2^40, the least bound

I64_SPECIALS = ([1 << 31, -(1 << 31), (1 << 31) + 1, (1 << 31) - 1, -(1 << 31) - 1, 1 << 32, -(1 << 32), (1 << 32) + 1,
                 (1 << 32) - 1, 0xFFFFFFFF]
                + [k << 32 for k in _KS] + [(k << 32) | 0xFFFFFFFF for k in _KS] + [-(k << 32) for k in _KS])
I64_BIG_SPECIALS = [(1 << 53) + 1, (1 << 53) - 1, -(1 << 53) - 1, -(1 << 53) + 1]  # rationed: see i64_wide
I64_EXTREMES = [I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX]

# One cycle sums to 0 and every contiguous run of the repeated cycle, from any
# start, keeps its prefix sums inside int64 (they reach INT64_MAX and
# INT64_MIN + 1), so the records of one key in arrival order can be cut into
# windows anywhere. Sums in any other grouping (records 0, 1, 4, 5 ...) leave
# int64 and have to wrap back. (-2^62 + 1, not + 3: a cycle with a positive
# net would drift over INT64_MAX.)
I64_CROSSING_CYCLE = [1 << 62, (1 << 62) - 1, -(1 << 62), -(1 << 62) + 1]
# The same property with the MIN identity as a real value: INT64_MAX under a
# SUM and a MIN at once (no such cycle can hold INT64_MIN: a cycle's prefix
# sums would have to span 2^63).
I64_CROSSING_CYCLE_B = [I64_MAX, I64_MIN + 1]

_P63 = 2.0 ** 63
_F64_PAIRS_BITS = [0x4005BF0A8B145769, 0x4005BF0A8B14576A,   # differ in the low word only
                   0x4005BF0A00000000, 0x4005BF0B00000000,   # differ in the high word only
                   0xC005BF0A8B145769, 0xC005BF0A8B14576A, 0xC005BF0A00000000, 0xC005BF0B00000000]
F64_EXTREMES = np.array(
    [1.7976931348623157e308, -1.7976931348623157e308, 5e-324, -5e-324, 2.2250738585072014e-308,
     -2.2250738585072014e-308, -0.0, 0.0, _P63, -_P63, np.nextafter(_P63, np.inf), np.nextafter(-_P63, -np.inf),
     np.nextafter(_P63, 0.0), np.nextafter(-_P63, 0.0), 1e19, 1.0, np.nextafter(1.0, 2.0), 2.0 ** 53 + 2.0]
    + list(np.array(_F64_PAIRS_BITS, np.uint64).view(np.float64)), np.float64)
F64_AT_MIN_IDENTITY = np.array([_P63, np.nextafter(_P63, np.inf), 1e19, 1.7976931348623157e308], np.float64)
F64_AT_MAX_IDENTITY = -F64_AT_MIN_IDENTITY
SUBNORMAL_UNIT = 5e-324


def wide_bound(n_total):
    """The bound of i64_wide for a case of n_total records in all."""
    return (1 << 62) // max(1, int(n_total))


def i64_wide(rng, n, bound):
    """Uniform in +-bound, ~10 % of the positions from I64_SPECIALS (all below
    2^40 <= bound in magnitude). The sum of |v| over the n_total = 2^62 //
    bound records of a case is then <= 2^62. The four values around 2^53 are
    larger than most bounds, so they are rationed: n * bound >> 54 of them,
    i.e. 256 over a whole case, another 2^61 at the most. Every sum of any
    subset therefore fits int64, whatever the grouping."""
    bound = int(bound)
    assert (1 << 40) <= bound <= (1 << 62), f"i64_wide: bound {bound} outside [2^40, 2^62]"
    v = rng.integers(-bound, bound, size=n, endpoint=True, dtype=np.int64)
    sp = rng.random(n) < 0.10
    v[sp] = rng.choice(np.array(I64_SPECIALS, np.int64), size=int(sp.sum()))
    n_big = min((n * bound) >> 54, n // 8)
    if n_big:
        at = rng.choice(n, size=n_big, replace=False)
        v[at] = rng.choice(np.array(I64_BIG_SPECIALS, np.int64), size=n_big)
    return v


def i64_extreme(rng, n):
    """MIN / MAX / LAST / COUNT only: half from I64_EXTREMES, half full-width
    values (uniform over all of int64 with the I64_SPECIALS mixed in)."""
    v = rng.integers(I64_MIN, I64_MAX, size=n, endpoint=True, dtype=np.int64)
    sp = rng.random(n) < 0.10
    v[sp] = rng.choice(np.array(I64_SPECIALS + I64_BIG_SPECIALS, np.int64), size=int(sp.sum()))
    ex = rng.random(n) < 0.5
    v[ex] = rng.choice(np.array(I64_EXTREMES, np.int64), size=int(ex.sum()))
    return v


def i64_crossing(start, n, cycle=None):
    """n values of a crossing cycle from cycle position `start`."""
    cyc = np.array(I64_CROSSING_CYCLE if cycle is None else cycle, np.int64)
    return cyc[(start + np.arange(n)) % len(cyc)]


def key_sign(key):
    """+1 / -1, fixed per key."""
    k = np.asarray(key).astype(np.uint64)
    return np.where(((k * np.uint64(2654435761)) >> np.uint64(7)) & np.uint64(1), 1.0, -1.0)


def f64_samesign(rng, n, key):
    """The SUM / AVG column: magnitudes 10**U(-3, 15), the sign fixed per key
    (no cancellation, so a relative bound on a sum holds)."""
    return key_sign(key) * 10.0 ** rng.uniform(-3.0, 15.0, size=n)


def f64_extreme(rng, n):
    """MIN / MAX / LAST / COUNT only: three quarters from F64_EXTREMES, the rest
    random finite bit patterns."""
    bits = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) | (rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(63))
    v = bits.view(np.float64).copy()
    v[~np.isfinite(v)] = 1.5
    ex = rng.random(n) < 0.75
    v[ex] = rng.choice(F64_EXTREMES, size=int(ex.sum()))
    return v


def f64_subnormal(rng, n, sign):
    """Same-signed multiples (1 .. 4096) of 5e-324: any sum of fewer than 2^40
    of them is a subnormal double, exactly. (The LDS and global f64 atomics of
    gfx950 keep subnormals: every path of test_gpu_value_edges.py returns
    these sums exactly.)"""
    return sign * (rng.integers(1, 4097, size=n).astype(np.float64) * SUBNORMAL_UNIT)


def column_classes(col_types, aggs):
    """Per column "i64_sum" / "i64_ext" / "f64_sum" / "f64_ext": _sum when a
    SUM or AVG reads the column."""
    summed = {c for kind, c in aggs if kind in (abi.HSG_SUM, abi.HSG_AVG)}
    return [("f64" if t == abi.HSG_F64 else "i64") + ("_sum" if c in summed else "_ext")
            for c, t in enumerate(col_types)]


def exact_mask(spec):
    """Per output: an f64 MIN / MAX / LAST, compared with no tolerance."""
    return [f and kind in (abi.HSG_MIN, abi.HSG_MAX, abi.HSG_LAST) for f, (kind, _c) in zip(spec.agg_is_f64(), spec.aggs)]


def sum_rtol(n_max):
    """Bound on the relative error of an f64 SUM / AVG of at most n_max
    same-signed terms against the exact sum rounded once: each of the n_max - 1
    additions, in any order, and the final division add at most 2^-53 relative
    (no cancellation), first order n_max * 2^-53; doubled for the higher-order
    terms and the reference's own rounding. Also covers an int64 AVG's two
    roundings (sum to f64, division)."""
    return 2.0 * max(1, int(n_max)) * 2.0 ** -53


def max_group(spec, batches):
    """Largest number of records any group of the case can hold: exact for
    tumbling, hopping (the records of each of a record's windows) and
    unwindowed ops when no record is dropped, else an upper bound; for
    sessions the records of the busiest key (a session can hold them all)."""
    key = np.concatenate([b[0] for b in batches]).astype(np.int64)
    ts = np.concatenate([b[1] for b in batches]).astype(np.int64)
    ok = key != KEY_NONE
    if spec.window_kind in (abi.HSG_SESSION, abi.HSG_UNWINDOWED):
        return int(np.unique(key[ok], return_counts=True)[1].max())
    ok &= ts >= 0
    key, ts = key[ok], ts[ok]
    adv = spec.advance_ms if spec.window_kind == abi.HSG_HOPPING else spec.size_ms
    first = np.maximum(0, ts - spec.size_ms + adv) // adv
    last = ts // adv
    gids = []
    for j in range(int((last - first).max()) + 1):
        m = first + j <= last
        gids.append(key[m] * (1 << 31) + (first[m] + j - first.min()))
    return int(np.unique(np.concatenate(gids), return_counts=True)[1].max())


ROLE_HI, ROLE_LO, ROLE_BOTH, ROLE_ABSENT = 0, 1, 2, 3


class Planter:
    """Columns for the batches of one case. `dedicated`: four key ids the
    shape itself never uses, in the roles ROLE_*. Carries the crossing cycle
    position of each dedicated key and a ts floor across batches: the
    dedicated records' timestamps never go back, so no window cuts their
    arrival order and none of them is late."""

    def __init__(self, seed, classes, n_total, dedicated, absent=0.05, decimal=0.0, frac=0.02):
        assert len(dedicated) == 4
        self.rng = np.random.default_rng(seed)
        self.classes = list(classes)
        self.bound = wide_bound(n_total)
        self.dedicated = np.array(dedicated, np.uint32)
        self.absent, self.decimal, self.frac = absent, decimal, frac
        self.pos = {int(k): j for j, k in enumerate(dedicated)}  # cycle position per key
        self.floor = None
        self.seen = 0

    def batch(self, key, ts):
        """-> (key, ts, cols, valids): the shape's keys and timestamps, except
        at the ~2 % of positions (16 at least) given to the dedicated keys."""
        rng = self.rng
        key = np.array(key, dtype=np.uint32)
        ts = np.array(ts, dtype=np.int64)
        n = len(key)
        assert not np.isin(key, self.dedicated).any(), "dedicated keys must be disjoint from the shape's"
        self.seen += n
        assert self.seen * self.bound <= (1 << 62), "more records than n_total"
        at = np.sort(rng.choice(n, size=min(n, max(16, int(n * self.frac))), replace=False))
        role = np.arange(len(at)) % 4
        key[at] = self.dedicated[role]
        run = np.maximum.accumulate(np.maximum(ts, 0 if self.floor is None else self.floor))
        ts[at] = run[at]
        if n:
            self.floor = int(max(run[-1], 0))
        cols, valids = [], []
        for cls in self.classes:
            valid = (rng.random(n) >= self.absent).astype(np.uint8)
            valid[at] = (role != ROLE_ABSENT).astype(np.uint8)
            if cls == "i64_sum":
                v = i64_wide(rng, n, self.bound)
            elif cls == "i64_ext":
                v = i64_extreme(rng, n)
                v[at] = np.choose(role, [I64_MAX, I64_MIN, np.where(np.arange(len(at)) % 8 < 4, I64_MAX, I64_MIN), 7])
            elif cls == "f64_sum":
                v = f64_samesign(rng, n, key)
                sub = f64_subnormal(rng, len(at), 1.0)
                v[at] = np.where(role == ROLE_LO, -sub, sub)
            elif cls == "f64_ext":
                v = f64_extreme(rng, n)
                hi = rng.choice(F64_AT_MIN_IDENTITY, size=len(at))
                lo = rng.choice(F64_AT_MAX_IDENTITY, size=len(at))
                v[at] = np.choose(role, [hi, lo, np.where(np.arange(len(at)) % 8 < 4, hi, lo), 7.0])
            else:
                raise ValueError(cls)
            if self.decimal:
                valid |= ((valid != 0) & (rng.random(n) < self.decimal)).astype(np.uint8) << 1
            cols.append(v)
            valids.append(valid)
        # the crossing cycle runs through each dedicated key's own records, in
        # arrival order, the same in every SUM column of int64
        for j, k in enumerate(self.dedicated):
            if j == ROLE_ABSENT:
                continue
            mine = at[role == j]
            cyc = i64_crossing(self.pos[int(k)], len(mine), I64_CROSSING_CYCLE_B if j == ROLE_LO else None)
            self.pos[int(k)] += len(mine)
            for c, cls in enumerate(self.classes):
                if cls == "i64_sum":
                    cols[c][mine] = cyc
        return key, ts, cols, valids


def dedicated_after(keys):
    """Four key ids above every id the shape's batches use."""
    top = 0
    for k in keys:
        k = np.asarray(k)
        k = k[k != np.uint32(KEY_NONE)]
        if k.size:
            top = max(top, int(k.max()))
    return [top + 17 + j for j in range(4)]
