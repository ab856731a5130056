"""Golden vectors for the composite kernels at edge shapes, on ragged panels and with heavy ties.

Test infrastructure only.  Run where make_golden.py's reference checkout is available:

    python tests/golden/make_golden_composite_edges.py

Imports the reference exactly as make_golden.py does and writes ``composite_edges.npz``
(plain data, no pickles): seven panels of F = 10 factors x D = 10 dates whose asset counts
sit on the composite kernels' edges (a single row, two rows, one full wave, one past it, one
past two waves, one past the 256-thread block, a second stride), three of them ragged.

Per panel ``A{n}``: ``X[D][A][F]`` (NaN where a row is absent), ``present[D][A]``, and the
reference's ``composite_factor_calculation`` (all factors / the ``sub_idx`` subset) and
``weighted_composite_factor`` outputs for both methods as dense ``[D][A]`` arrays, NaN
(``cfc``) or 0 (``wcf``) where a row is absent.  Shared: ``names``, ``dates``, ``sub_idx``,
``sel_dates``, and per panel the selection weights ``A{n}_sel_W``.

The recipe (tests/test_composite_edges.py checks the conditions it is built to meet):

* factors 0-4 are rounded to a 0.5 grid, so ties straddle every percentile; 5-9 continuous;
* odd dates carry 5 % NaN, even dates none (a NaN in a proxy turns the whole date of the
  weighted rank composite into zeros, so the even dates are where it has values);
* date 3: factor 3 (``_short``) all NaN, and one NaN in factor 9 (``raw``, alone in its
  prefix group) whose weight on that date is positive: a whole date zero through NaN
  propagation on every panel;
* date 7: factor 1 constant; date 5: factor 5 half -0.0, half +0.0;
* 1e300, -1e300, -1e-310 and 5e-324 in suffixed columns (clipped or classified, never
  squared);
* ragged panels keep ~80 % of the rows, symbol 0 always; date 8 has a single present row,
  date 2 exactly two;
* the selection frame covers every date with 1 to 7 positive weights per row, the row of
  date 1 is all zeros, and one selection date is absent from the panel.
"""
from __future__ import annotations

import json
import os
import sys
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

SUF = ["eq", "flx", "long", "short", "raw"]
F, D = 10, 10
NAMES = [f"g{k // 3}_{k}_{SUF[k % 5]}" for k in range(F)]
SUB = [0, 1, 2, 4, 5, 6, 7, 9]
PANELS = [(1, False), (2, False), (64, False), (65, True), (129, True), (257, True), (300, False)]
SEED = 700


def edge_panel(rng, A, ragged):
    """X[D][A][F], present[D][A] and the selection weights [D + 1][F] of one panel."""
    X = rng.standard_normal((D, A, F))
    X[:, :, :5] = np.round(X[:, :, :5] * 2) / 2           # 0.5 grid: heavy ties
    nan = rng.random((D, A, F)) < 0.05
    nan[0::2] = False                                     # even dates are NaN-free
    X[nan] = np.nan
    X[3, :, 3] = np.nan                                   # an all-NaN column-date (_short)
    X[3, 0, 9] = np.nan                                   # one NaN in a single-column group
    X[7, :, 1] = 1.5                                      # a constant column-date (_flx)
    X[5, :, 5] = 0.0                                      # half -0.0, half +0.0 (_eq)
    X[5, : A // 2, 5] = -0.0
    if A >= 4:
        X[4, 0, 6], X[4, 1, 6] = 1e300, -1e300            # _flx
        X[4, 2, 7], X[4, 3, 7] = -1e-310, 5e-324          # _long
    else:
        X[4, 0, 6], X[6, A - 1, 6] = 1e300, -1e300
        X[4, 0, 7], X[6, A - 1, 7] = -1e-310, 5e-324
    present = np.ones((D, A), dtype=bool)
    if ragged:
        present = rng.random((D, A)) < 0.8
        present[:, 0] = True
        present[8, 1:] = False                            # a single present row
        present[2, 1:] = False
        present[2, A // 2] = True                         # exactly two present rows
    W = np.zeros((D + 1, F))
    for i in range(D + 1):
        k = rng.choice(F, size=rng.integers(1, 8), replace=False)
        W[i, k] = 0.05 + rng.random(len(k))
    W[1] = 0.0                                            # a date with no positive weight
    W[3] = 0.0
    W[3, [0, 3, 9]] = 0.05 + rng.random(3)                # factor 3 alone in the _short pool
    return X, present, W


def gen_composite_edges(ref_cf, rng):
    dates = pd.bdate_range("2022-01-03", periods=D)
    sel_dates = list(dates) + [pd.Timestamp("2030-01-01")]
    st = {"names": np.array(NAMES), "dates": np.array([str(d.date()) for d in dates]),
          "sub_idx": np.array(SUB, dtype=np.int32), "sel_dates": np.array([str(d.date()) for d in sel_dates]),
          "panels": np.array([A for A, _ in PANELS], dtype=np.int32)}
    cases = []
    for A, ragged in PANELS:
        X, present, W = edge_panel(rng, A, ragged)
        syms = [f"E{i:03d}" for i in range(A)]
        di, si = np.nonzero(present)                      # lexsorted (date, symbol)
        idx = pd.MultiIndex.from_arrays([dates[di], [syms[k] for k in si]], names=["date", "symbol"])
        df = pd.DataFrame(X[di, si], index=idx, columns=NAMES)
        seldf = pd.DataFrame(W, index=pd.DatetimeIndex(sel_dates, name="date"), columns=NAMES)
        seldf = seldf.div(seldf.sum(axis=1), axis=0).fillna(0)
        key = f"A{A}"
        st[f"{key}_X"] = np.where(present[..., None], X, np.nan)
        st[f"{key}_present"] = present
        st[f"{key}_sel_W"] = seldf.to_numpy()

        def put(name, ser, fill):
            assert ser.index.equals(df.index)
            out = np.full((D, A), fill)
            out[di, si] = ser.to_numpy(dtype=np.float64)
            st[f"{key}_out_{name}"] = out
            cases.append(f"{key}_{name}")

        for meth in ("zscore", "rank"):
            put(f"cfc_all_{meth}", ref_cf.composite_factor_calculation(df, NAMES, method=meth), np.nan)
            put(f"cfc_sub_{meth}",
                ref_cf.composite_factor_calculation(df, [NAMES[k] for k in SUB], method=meth), np.nan)
            put(f"wcf_{meth}", ref_cf.weighted_composite_factor(df, seldf, method=meth), 0.0)
    return st, cases


def main():
    warnings.filterwarnings("ignore")
    os.environ["TQDM_DISABLE"] = "1"
    _, _, _, ref_cf = import_reference()
    st, cases = gen_composite_edges(ref_cf, np.random.default_rng(SEED))
    np.savez_compressed(os.path.join(HERE, "composite_edges.npz"), **st)
    path = os.path.join(HERE, "manifest.json")
    manifest = json.load(open(path))
    manifest["files"]["composite_edges.npz"] = {
        "seed": SEED, "D": D, "F": F, "panels": [{"A": A, "ragged": r} for A, r in PANELS], "cases": cases,
        "generator": "make_golden_composite_edges.py"}
    with open(path, "w") as f:
        json.dump(manifest, f, indent=1)
    print("wrote composite_edges.npz")


if __name__ == "__main__":
    main()
