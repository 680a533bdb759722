"""Literal forms (hsg_rows.form, 2 bits per output) of the SQL shape's ops:
a vectorised restatement of the reference's sequential fold (Codegen.hs:436-469)
-- a SUM is integral iff no decimal literal reached it, a MIN keeps the
earliest literal among equal minima, a MAX the latest among equal maxima, a
passthrough its last present record's literal, an aggregate no present record
reached its initial value. Host only; shared by the GPU tests of ops with
HSG_OPF_LITERAL_FORMS."""
import numpy as np

from hstream_amd import abi

# SELECT v, COUNT(*), SUM(v), AVG(v), MIN(v), MAX(v): the passthrough first
AGGS = [(abi.HSG_LAST, 0), (abi.HSG_COUNT_ALL, 0), (abi.HSG_SUM, 0), (abi.HSG_AVG, 0), (abi.HSG_MIN, 0),
        (abi.HSG_MAX, 0)]
FORM = {abi.HSG_LAST: "last", abi.HSG_SUM: "sum", abi.HSG_MIN: "min", abi.HSG_MAX: "max"}


def _prefix_forms(gid, v, valid, f64, aggs=AGGS):
    """Literal-form word (hsg_rows.form) of each record's group right after
    the record, in arrival order: the reference's sequential fold."""
    import pandas as pd
    n = len(gid)
    present = (valid & 1) != 0
    dec = (valid & 2) != 0
    idx = np.arange(n)
    hi, lo = (np.inf, -np.inf) if f64 else (np.iinfo(np.int64).max, np.iinfo(np.int64).min)
    df = pd.DataFrame({"g": gid, "i": idx, "p": present, "d": dec & present,
                       "vmin": np.where(present, v, hi), "vmax": np.where(present, v, lo)})
    df = df.sort_values(["g", "i"], kind="stable")
    gb = df.groupby("g", sort=False)
    sum_dec = gb["d"].cumsum().to_numpy()
    run_min = gb["vmin"].cummin()
    prev_min = run_min.groupby(df["g"]).shift(1).fillna(hi).to_numpy()
    run_max = gb["vmax"].cummax()
    prev_max = run_max.groupby(df["g"]).shift(1).fillna(lo).to_numpy()
    p = df["p"].to_numpy()
    i_s = df["i"].to_numpy()
    new_min = p & (df["vmin"].to_numpy() < prev_min)   # min n x = n: a tie keeps the earlier literal
    new_max = p & (df["vmax"].to_numpy() >= prev_max)  # max n x = x: a tie takes the later one
    tmp = pd.DataFrame({"g": df["g"].to_numpy(), "a": np.where(new_min, i_s, -1), "b": np.where(new_max, i_s, -1),
                        "c": np.where(p, i_s, -1)})
    g2 = tmp.groupby("g", sort=False)
    tmin = g2["a"].cummax().to_numpy()
    tmax = g2["b"].cummax().to_numpy()
    tlast = g2["c"].cummax().to_numpy()
    integral = ~dec

    def bits(t):  # the winning literal's "prints as an integer" bit; 3 = the initial value
        return np.where(t < 0, 3, integral[np.maximum(t, 0)].astype(np.int64))

    per = {"sum": (sum_dec == 0).astype(np.int64), "min": bits(tmin), "max": bits(tmax), "last": bits(tlast)}
    word = np.zeros(n, np.int64)
    for j, (k, _c) in enumerate(aggs):
        if k in FORM:
            word |= per[FORM[k]] << (2 * j)
    out = np.empty(n, np.uint32)
    out[i_s] = word.astype(np.uint32)
    return out
