"""Golden vectors for +-inf in the rolling operators.

Test infrastructure only.  Run in the build container (where /root/reference exists):

    python tests/golden/make_golden_nonfinite.py

Imports the reference exactly as make_golden.py does and writes ``ops_nonfinite.npz``: the
reference's rolling operators (operations.py:6-51) at W in {1, 3, 5, 20} and
``ts_regression_fast`` (operations.py:185-246) at W = 5, lag in {0, 1}, every rettype, on a
60-date x 12-symbol panel whose columns hold +-inf, dense and ragged.  pandas' ``Rolling``
replaces +-inf by NaN before it aggregates (``_prep_values``), so an inf empties the W windows
that hold it and the column then recovers; diff / delay / ffill / decay(window < 1) keep it.
``ts_corr`` has no reference counterpart: its expected values are pandas ``rolling(w).corr``
as in make_golden.py:gen_ts_corr.

Columns (ROLES): one +inf; one -inf; +inf then -inf on adjacent rows; inf in the column's
first row; inf in its last row; two infs 28 rows apart (more than any W); inf right after a
NaN; an all-finite control without NaN; four noise columns with ties and 5 % NaN.  y (corr,
regression) has NaNs in the noise columns, one +inf (column 9) and one -inf (column 4).  The regression's own x
panel is finite but for one 1e200 cell (its square overflows: NaN in the mean of x^2 only) and
one +inf.  The ragged variant drops every ninth row of the first eight columns and the rows on
both sides of each inf, 15 % of the noise columns' rows, and the first row of column 8.

Outputs are stored as plain value arrays on the input's row index (the rolling operators
return their input's index); the regression, which drops rows, with its own (date, symbol)
codes.  The archive is written with fixed timestamps, so a rerun is byte-identical.
"""
from __future__ import annotations

import io
import json
import os
import sys
import warnings
import zipfile

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import enc_index, import_reference  # noqa: E402

D, A = 60, 12
WINDOWS = (1, 3, 5, 20)
ROLES = ("pos_inf", "neg_inf", "pos_then_neg", "first_row", "last_row", "two_far_apart", "after_nan",
         "control", "noise", "noise", "noise", "noise")
# (row, column, value)
INFS = ((25, 0, np.inf), (30, 1, -np.inf), (27, 2, np.inf), (28, 2, -np.inf), (0, 3, np.inf),
        (D - 1, 4, -np.inf), (6, 5, np.inf), (34, 5, -np.inf), (34, 6, np.inf))


def panel(rng, ragged):
    dates = pd.bdate_range("2022-01-03", periods=D)
    syms = [f"N{i:02d}" for i in range(A)]
    x = rng.standard_normal((D, A))
    tie = rng.random((D, A)) < 0.3
    x[tie] = np.round(x[tie], 1)
    noise = np.arange(A) >= 8
    x[(rng.random((D, A)) < 0.05) & noise[None, :]] = np.nan
    x[33, 6] = np.nan                                   # the NaN before column 6's inf
    y = 0.5 * np.nan_to_num(x) + rng.standard_normal((D, A))
    y[(rng.random((D, A)) < 0.05) & noise[None, :]] = np.nan
    xr = rng.standard_normal((D, A))                    # the regression's own x
    xr[rng.random((D, A)) < 0.05] = np.nan
    xr[22, 1] = 1e200
    xr[31, 2] = np.inf
    for d, a, v in INFS:
        x[d, a] = v
    y[20, 9] = np.inf
    y[30, 4] = -np.inf
    present = np.ones((D, A), dtype=bool)
    if ragged:
        present[:, 8:] = rng.random((D, 4)) > 0.15
        present[(np.arange(D) % 9 == 4), :8] = False
        for d, a, _ in INFS:
            present[d, a] = True
            for n in (d - 1, d + 1):
                if 0 <= n < D and not np.isinf(x[n, a]):
                    present[n, a] = False
        present[33, 6] = True                           # the NaN stays next to its inf
        present[32, 6] = False
        present[0, 8] = False
        present[22, 1] = present[31, 2] = present[20, 9] = present[30, 4] = True
    di, si = np.nonzero(present)
    idx = pd.MultiIndex.from_arrays([dates[di], [syms[k] for k in si]], names=["date", "symbol"])
    mk = lambda v, name: pd.Series(v[di, si], index=idx, name=name)  # noqa: E731
    return dates, syms, mk(x, "fx"), mk(y, "fy"), mk(xr, "fxr")


def gen(ref_ops, rng, ragged):
    dates, syms, x, y, xr = panel(rng, ragged)
    st = {"dates": np.array([str(d.date()) for d in dates]), "syms": np.array(syms), "roles": np.array(ROLES)}
    st["in__d"], st["in__s"] = enc_index(x.index, dates, syms)
    st["in_x__v"], st["in_y__v"], st["in_xr__v"] = (s.to_numpy(dtype=np.float64) for s in (x, y, xr))
    cases = []

    def add(key, ser):
        assert ser.index.equals(x.index), key
        st["out_" + key] = ser.to_numpy(dtype=np.float64, na_value=np.nan)
        cases.append(key)

    for w in WINDOWS:
        for op in ("ts_sum", "ts_mean", "ts_std", "ts_zscore", "ts_rank", "ts_decay", "ts_diff", "ts_delay"):
            add(f"{op}_{w}", getattr(ref_ops, op)(x, w))
        parts = [xs.rolling(w).corr(y.xs(sym, level="symbol", drop_level=False))
                 for sym, xs in x.groupby(level="symbol")]
        add(f"ts_corr_{w}", pd.concat(parts).reindex(x.index))
    add("ts_decay_0", ref_ops.ts_decay(x, 0))
    add("ts_backfill", ref_ops.ts_backfill(x))
    for lag in (0, 1):
        for rt in (0, 1, 2, 3, 6):
            key = f"ts_regression_fast_5_{lag}_{rt}"
            out = ref_ops.ts_regression_fast(y, xr, 5, lag=lag, rettype=rt)
            st[f"out_{key}__d"], st[f"out_{key}__s"] = enc_index(out.index, dates, syms)
            st[f"out_{key}__v"] = out.to_numpy(dtype=np.float64)
            cases.append(key)
    return st, cases


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (reproducible bytes)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    warnings.filterwarnings("ignore")
    os.environ["TQDM_DISABLE"] = "1"
    ref_ops, _, _, _ = import_reference()
    path = os.path.join(HERE, "manifest.json")
    manifest = json.load(open(path))
    out = {}
    entry = {"generator": "make_golden_nonfinite.py", "D": D, "A": A, "windows": list(WINDOWS),
             "ts_corr": "pandas Rolling.corr (no reference counterpart)"}
    for tag, seed, ragged in (("dense", 900, False), ("ragged", 901, True)):
        st, cases = gen(ref_ops, np.random.default_rng(seed), ragged)
        out.update({f"{tag}/{k}": v for k, v in st.items()})
        entry[tag] = {"seed": seed, "ragged": ragged, "cases": cases}
    manifest["files"]["ops_nonfinite.npz"] = entry
    write_npz(os.path.join(HERE, "ops_nonfinite.npz"), out)
    with open(path, "w") as f:
        json.dump(manifest, f, indent=1)
    print("wrote ops_nonfinite.npz")


if __name__ == "__main__":
    main()
