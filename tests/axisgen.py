"""Keys and timestamps for the time-axis tests (tests/test_gpu_time_axis.py and
the oracle cross-checks of tests/test_oracle.py): batches on epoch-millisecond
timestamps with windows so small that the op's window epoch is not zero, the
edges of the 2^32-window span, window starts near 0 .. 2^62, the top of the
axis, and sessions rebased to the ends of int64. Numpy only; columns come from
util.gen_small, so the values are the ordinary ones of the rest of the suite.

The epoch: a time-window op keeps window indices relative to
max(0, k_first - 2^31), k_first = ts // advance of its first keyed record with
ts >= 0. With T0 and the advances of WINDOWS, k_first > 2^31: the epoch is
beyond 32 bits for the 250 ms advance and the first record sits at relative
index 2^31 exactly.
"""
import numpy as np

from hstream_amd import abi
from util import gen_small

T0 = 1_700_000_000_000
I64_MAX = (1 << 63) - 1
NONE = np.uint32(abi.HSG_KEY_NONE)

# name -> (window kind, size_ms, advance_ms)
WINDOWS = {
    "tumbling": (abi.HSG_TUMBLING, 250, 250),
    "hop_pane": (abi.HSG_HOPPING, 1000, 250),    # size % adv == 0
    "hop_fanout": (abi.HSG_HOPPING, 700, 300),   # size % adv != 0
}


def window_kw(name):
    kind, size, adv = WINDOWS[name]
    return kind, (dict(size_ms=size) if kind == abi.HSG_TUMBLING else dict(size_ms=size, advance_ms=adv))


def first_keyed_ts(key, ts):
    """ts of the first record that has a key and a window (ts >= 0), or None."""
    ok = np.nonzero((key != NONE) & (ts >= 0))[0]
    return int(ts[ok[0]]) if ok.size else None


def epoch_is_nonzero(batches, adv):
    """From the inputs alone: the op's first keyed record lies beyond window
    2^31 (the batch's minimum, which the careful path uses, as well)."""
    for key, ts in ((b[0], b[1]) for b in batches):
        t = first_keyed_ts(key, ts)
        if t is None:
            continue
        ok = (key != NONE) & (ts >= 0)
        return t // adv > 2**31 and int(ts[ok].min()) // adv > 2**31
    return False


def messy(seed, n, nkeys, span, base, jitter, late_frac=0.02, neg_frac=0.01, none_frac=0.02, very_late=True):
    """util.gen_small's keys and timestamps with the jitter as a parameter
    (gen_small's 3000 ms belongs to its 10 s windows)."""
    rng = np.random.default_rng(seed)
    key = rng.integers(0, nkeys, size=n).astype(np.uint32)
    ts = base + (np.arange(n, dtype=np.int64) * span) // max(1, n) + rng.integers(0, max(1, jitter), size=n)
    if very_late:
        late = rng.random(n) < late_frac
        ts = np.where(late, ts - abi.HSG_DEFAULT_GRACE_MS - rng.integers(0, 200_000, size=n), ts)
    neg = rng.random(n) < neg_frac
    ts = np.where(neg, -rng.integers(1, 50_000, size=n), ts).astype(np.int64)
    key = np.where(rng.random(n) < none_frac, NONE, key).astype(np.uint32)
    return key, ts


def uniform(seed, n, nkeys, span, base):
    """tests/test_gpu_lean.py _uniform: sorted ts over `span` ms."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, nkeys, size=n).astype(np.uint32), (base + np.sort(rng.integers(0, span, size=n))).astype(np.int64)


def three_bases(adv, reach, t0=T0):
    """Bases of the three batches of a family case, `reach` the time one batch
    covers (span + jitter): batch 0 at a window start above t0, batch 1 right
    after it, batch 2 ending three windows before batch 0 (late against the
    stream time, far inside the default grace)."""
    b0 = (t0 // adv + 1) * adv
    return [b0, b0 + reach, b0 - reach - 3 * adv]


def first_in_the_middle(key, ts):
    """Batch 0 of a case: a keyed record from the middle of the batch's time
    span moves to the front, so the records after it fall on both sides of
    the first one's window (relative indices below and from 2^31 on)."""
    ok = np.nonzero((key != NONE) & (ts >= 0))[0]
    hi = int(ts[ok].max())
    # (the late records of a messy batch lie a day below: the middle of the in-time part)
    intime = ok[ts[ok] >= hi - abi.HSG_DEFAULT_GRACE_MS // 2]
    mid = (int(ts[intime].min()) + hi) // 2
    j = int(intime[np.argmin(np.abs(ts[intime] - mid))])
    key, ts = key.copy(), ts.copy()
    key[[0, j]] = key[[j, 0]]
    ts[[0, j]] = ts[[j, 0]]
    assert int(ts[intime].min()) < first_keyed_ts(key, ts) < hi
    return key, ts


def with_columns(shapes, col_types, seed=1):
    """[(key, ts)] -> [(key, ts, cols, valid)] with gen_small's values."""
    out = []
    for b, (key, ts) in enumerate(shapes):
        if col_types:
            _k, _t, cols, valid = gen_small(seed + b, len(key), 1, col_types=col_types)
        else:
            cols, valid = [], None
        out.append((key, ts, cols, valid))
    return out


def family(window, gen, n, nkeys, wins, jitter_wins=0.3, seed=1, **kw):
    """Three batches of one family case on WINDOWS[window]: `wins` advances of
    time per batch (the borrowed shape's windows per batch) and a jitter of
    `jitter_wins` advances, at three_bases' places; batch 0 with its first
    keyed record in the middle."""
    _kind, _size, adv = WINDOWS[window]
    span, jitter = int(wins * adv), max(1, int(jitter_wins * adv))
    out = []
    for b, base in enumerate(three_bases(adv, span + jitter)):
        if gen == "uniform":
            key, ts = uniform(seed + b, n, nkeys, span, base)
        else:
            key, ts = messy(seed + b, n, nkeys, span, base, jitter, **kw)
        out.append(first_in_the_middle(key, ts) if b == 0 else (key, ts))
    assert epoch_is_nonzero(out, adv)
    return out


# ---------------------------------------------------------------------------
# the span limit (size 1: the window index is the timestamp)
# ---------------------------------------------------------------------------
def span_points(first):
    """(accepted, refused) timestamps of a size-1 tumbling op whose first
    keyed record is at `first`: the epoch is max(0, first - 2^31) and the op
    holds relative indices 0 .. 2^32 - 1."""
    epoch = max(0, first - 2**31)
    accepted = [epoch, epoch + 2**32 - 1]
    refused = [t for t in (epoch - 1, epoch + 2**32) if t >= 0]
    return accepted, refused


# ---------------------------------------------------------------------------
# window starts
# ---------------------------------------------------------------------------
ADVANCES = [1, 2, 3, 7, 2**20, 2**20 - 1, 2**20 + 1, 86_400_000, 2**40 + 1, 2**62 - 1]
ANCHORS = [0, 2**31, 2**32, 2**53, 2**62]


def window_start_batch(adv, size, anchor, seed=0):
    """Multiples of `adv` around `anchor`, each - 1, + 0 and + 1, with one key;
    returns (key, ts, grace_ms). Kept: ts >= -1 (a negative ts has no window)
    and every window's end + grace <= INT64_MAX, so nothing wraps and, with
    the returned grace, nothing is late: the grace covers the batch's span
    where it can (the order is then random), else the batch is ascending."""
    m = anchor // adv
    cand = sorted({(m + j) * adv + d for j in range(-3, 4) for d in (-1, 0, 1)})
    ts = [t for t in cand if -1 <= t and (t // adv) * adv + size <= I64_MAX]
    ends = [(t // adv) * adv + size for t in ts if t >= 0]
    starts = [max(0, t - size + adv) // adv * adv for t in ts if t >= 0]
    need = max(0, max(ts) - (min(starts) + size) + 1)  # stream time - the earliest window's end < need
    grace = min(need, I64_MAX - max(ends))
    ts = np.array(ts, dtype=np.int64)
    if grace >= need:
        ts = ts[np.random.default_rng(seed).permutation(ts.size)]
    assert ts.size <= 256 and grace >= 0
    return np.zeros(ts.size, np.uint32), ts, int(grace)


# ---------------------------------------------------------------------------
# the top of the axis
# ---------------------------------------------------------------------------
def top_of_axis(size, adv, grace, n=600, nkeys=5, seed=3):
    """Batches of (key, ts): the first just below the band
    [INT64_MAX - size - grace - 2 size, INT64_MAX - 1] (every window ends, with
    the grace added, at or below INT64_MAX: accepted); then, in rising order,
    one below the wrap, one across it (the minimum still below INT64_MAX -
    grace), one wholly above it (window end + grace wraps for every record: the
    reference drops them all), and the whole band at once."""
    rng = np.random.default_rng(seed)
    M, S, G = I64_MAX, size, grace
    assert G >= 3 * S
    ranges = [(M - G - 6 * S, M - G - 3 * S - 1), (M - G - 3 * S, M - G - S), (M - G - 2 * S, M - G + S),
              (M - G + 1, M - 1), (M - G - 3 * S, M - 1)]
    out = []
    for lo, hi in ranges:
        off = rng.integers(0, hi - lo + 1, size=n)
        ts = (lo + off).astype(np.int64)
        ts[0], ts[-1] = lo, hi
        out.append((rng.integers(0, nkeys, size=n).astype(np.uint32), ts))
    return out


def window_pairs(key, ts, size, adv):
    """(record, window) pairs of a batch before the grace check."""
    ok = (key != NONE) & (ts >= 0)
    t = ts[ok]
    return int((t // adv - np.maximum(0, t - size + adv) // adv + 1).sum())


# ---------------------------------------------------------------------------
# sessions at the ends of int64
# ---------------------------------------------------------------------------
SESSION_BASES = {"-2^62": -2**62, "2^62": 2**62, "-2^63+2^20": -2**63 + 2**20, "2^63-2^20": 2**63 - 2**20}


def session_batches(base, col_types, nb=3, n=5000, nkeys=37, seed=3000):
    """test_session_messy_batches' batches (gen_small: jitter, KEY_NONE,
    absent fields; without its late and negative records, which would leave
    the int64 range) moved so that the first batch's base is `base`. The
    stream covers 223 000 ms < 2^20 - gap."""
    out = []
    for b in range(nb):
        key, ts, cols, valid = gen_small(seed + b, n, nkeys, col_types=col_types, span=100_000,
                                         base=10_000_000 + b * 60_000, very_late=False, neg_frac=0.0)
        rel = [int(x) + base - 10_000_000 for x in (ts.min(), ts.max())]
        assert -2**63 + 2**19 < rel[0] and rel[1] < 2**63 - 2**19
        out.append((key, (ts - 10_000_000 + np.int64(base)).astype(np.int64), cols, valid))
    return out
