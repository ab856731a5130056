"""Golden vectors for ``Simulation(method="mvo")`` (portfolio_simulation.py:96-154, :183-204,
:315-374, :587-661), by running the REFERENCE in this container (test infrastructure only):

    python tests/golden/make_golden_sim_mvo.py      -> tests/golden/sim_mvo.npz

cvxpy is not installed, so it is stubbed and the reference's scipy SLSQP fallback
(``use_cvxpy=False``, ftol 1e-9) solves the QPs: a feasible but loose answer -- the tests use
it as an upper bound on the variance, not as the optimum.

The case: D = 14 dates, A = 11 symbols, lookback 5, max_weight 0.5, on a ragged panel --
S09 has no feature row on dates 2-3 and S10 none on dates 6-9; returns date 4 has a row for
S10 ONLY (so the windows of dates 6-9 skip it), the returns row (date 8, S03) is missing and
(date 9, S05) is NaN; the signal is 0 at (date 5, S02), NaN at (date 6, S04) and has no
negative cell on date 10 (flat day).  Date 0 has no returns history (equal-weight book) and
date 1 a one-row window.  Recorded: the inputs, ``_apply_shrinkage(_calculate_covariance_
matrix)`` for dates 2 (T = 2), 3 (T = 3 < lookback) and 7 (T = lookback, date 4 skipped), each
date's same-day book, the shifted weights and the counts.  Plain arrays only (no pickles).
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, import_reference, put_series  # noqa: E402

D, A, LOOKBACK, MAX_WEIGHT, SHRINK, PCT = 14, 11, 5, 0.5, 0.1, 0.25
SIGMA_DATES = (2, 3, 7)


def inputs():
    rng = np.random.default_rng(1401)
    dates = pd.bdate_range("2022-03-01", periods=D)
    syms = [f"S{k:02d}" for k in range(A)]
    full = pd.MultiIndex.from_product([dates, syms], names=["date", "symbol"])
    sig = pd.Series(rng.standard_normal(len(full)), index=full, name="sig")
    sig[(dates[5], "S02")] = 0.0
    sig[(dates[6], "S04")] = np.nan
    sig[sig.index.get_level_values(0) == dates[10]] = np.abs(sig[sig.index.get_level_values(0) == dates[10]]) + 0.01
    absent = [(dates[d], "S09") for d in (2, 3)] + [(dates[d], "S10") for d in (6, 7, 8, 9)]
    sig = sig.drop(absent)
    common = rng.standard_normal(D)
    scale = rng.uniform(0.3, 2.0, A)
    r = 0.01 * (0.6 * common[:, None] + rng.standard_normal((D, A)) * scale)
    ret = pd.Series(r.reshape(-1), index=full, name="ret")
    ret[(dates[9], "S05")] = np.nan
    ret = ret.drop([(dates[4], s) for s in syms if s != "S10"] + [(dates[8], "S03")])
    return dates, syms, sig, ret


def main():
    warnings.filterwarnings("ignore")
    import_reference()
    import portfolio_simulation as ps
    dates, syms, sig, ret = inputs()
    one = pd.Series(1.0, index=ret.index)
    settings = ps.SimulationSettings(returns=ret, cap_flag=one, investability_flag=one, factors_df=None, method="mvo",
                                     pct=PCT, max_weight=MAX_WEIGHT, lookback_period=LOOKBACK, use_cvxpy=False,
                                     shrinkage_intensity=SHRINK, plot=False)
    sim = ps.Simulation(name="g", custom_feature=sig, settings=settings)
    books = {}
    inner = sim._calculate_mvo_weights

    def record(x, pos, neg, date):
        w, kl, ks = inner(x, pos, neg, date)
        books[date] = w.copy()
        return w, kl, ks
    sim._calculate_mvo_weights = record
    shifted, counts = sim._daily_trade_list()

    st = {"dates": np.array([str(d.date()) for d in dates]), "syms": np.array(syms),
          "params": np.array([LOOKBACK, MAX_WEIGHT, SHRINK, PCT]), "sigma_dates": np.array(SIGMA_DATES)}
    put_series(st, "sig", sig, dates, syms)
    put_series(st, "ret", ret, dates, syms)
    put_series(st, "shifted", shifted, dates, syms)
    st["counts"] = counts.loc[dates].to_numpy(dtype=np.int64)
    raw = np.full((D, A), np.nan)                # same-day books; NaN where the feature has no row
    solved = np.zeros(D, dtype=bool)             # the date went through _calculate_mvo_weights
    for d, date in enumerate(dates):
        x = sig.xs(date, level=0)
        cols = pd.Index(syms).get_indexer(x.index)
        raw[d, cols] = 0.0
        if date in books:
            raw[d, pd.Index(syms).get_indexer(books[date].index)] = books[date].to_numpy()
            solved[d] = True
    st["raw"], st["solved"] = raw, solved
    for d in SIGMA_DATES:
        x = sig.xs(dates[d], level=0)
        S = sim._apply_shrinkage(sim._calculate_covariance_matrix(x.index, dates[d]))
        st[f"sigma_{d}"] = S.to_numpy()
        st[f"sigma_{d}_syms"] = np.array(list(S.index))
    np.savez_compressed(os.path.join(OUT, "sim_mvo.npz"), **st)
    print("wrote sim_mvo.npz:", len(st), "arrays;", "solved dates", np.flatnonzero(solved).tolist())
    print("counts", st["counts"].tolist())
    print("book of date 1 (one-row window):", raw[1])


if __name__ == "__main__":
    main()
