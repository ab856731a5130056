"""Golden vectors for ``single_factor_backtests`` / ``single_factor_returns``, by running the
REFERENCE ``Simulation`` once per factor column in this container (test infrastructure only):

    python tests/golden/make_golden_factor_returns.py      -> tests/golden/factor_returns.npz

Per case a factor frame, returns and cap flags over 2 more dates and 3 more symbols than the
factors (NaNs in both, an unmapped cap code 4), and two investability flags: ``inv_same`` on the
factors' own index and ``inv_diff`` on another one (some rows missing, some extra).  Each of
the four variants (transaction cost on / off x the two flags) stores, per factor, the frame
``Simulation(f, factors_df[f], settings).run()`` returns (portfolio_simulation.py:71-95 with
``plot=False, output_returns=True``) and the counts of ``_daily_trade_list()`` on the masked
signal (:96-154).  The signals are continuous: no exact tie falls at an 'equal' cut-off, where
the reference's order is implementation-defined.

* ``eq_ragged``  'equal',  F=5, D=16, A=45, 10 % of the rows dropped, one all-NaN column, one
  column with a day without a negative leg (flat);
* ``lin_dense``  'linear', F=3, D=12, A=300;
* ``lin_ragged`` 'linear', F=4, D=20, A=83: a symbol that lists late, a symbol with a
  multi-date gap, a date without any feature row (the returns have it).
Plain arrays only (no pickles).
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, import_reference, put_series  # noqa: E402
from make_golden_sim2 import market  # noqa: E402

COLS = ["log_return", "long_return", "short_return", "long_turnover", "short_turnover", "turnover"]
CASES = [("eq_ragged", "equal", 5, 16, 45, 0.03), ("lin_dense", "linear", 3, 12, 300, 0.02),
         ("lin_ragged", "linear", 4, 20, 83, 0.025)]


def factors(rng, name, F, D, A):
    dates = pd.bdate_range("2021-01-01", periods=D)
    syms = [f"S{k:04d}" for k in range(A)]
    idx = pd.MultiIndex.from_product([dates, syms], names=["date", "symbol"])
    X = rng.standard_normal((D * A, F)).astype(np.float32).astype(np.float64)   # 24-bit values: a smaller file
    X[rng.random(X.shape) < 0.02] = np.nan               # NaN values inside a date group
    df = pd.DataFrame(X, index=idx, columns=[f"f{k}" for k in range(F)])
    d = idx.get_level_values(0)
    s = idx.get_level_values(1)
    keep = np.ones(len(idx), dtype=bool)
    if name == "eq_ragged":
        df["f1"] = np.nan                                # an all-NaN column
        day = np.asarray(d == dates[3])
        df.loc[day, "f2"] = np.abs(df.loc[day, "f2"]) + 0.1   # no negative leg -> flat day
        keep &= ~(rng.random(len(idx)) < 0.10)
    if name == "lin_ragged":
        keep &= ~(rng.random(len(idx)) < 0.10)
        keep &= ~np.asarray((s == syms[0]) & (d < dates[7]))                       # lists late
        keep &= ~np.asarray((s == syms[5]) & (d >= dates[4]) & (d < dates[9]))     # multi-date gap
        keep &= ~np.asarray(d == dates[11])                                        # a date without feature rows
    return df[keep], dates, syms


def investability(rng, df, dd):
    """(flag on the factors' own index, flag on another index: ~8 % of the rows missing, an
    extra symbol on three dates and two of the symbols on a date past the factors' last)."""
    same = pd.Series(np.where(rng.random(len(df)) < 0.1, 0.0, 1.0), index=df.index)
    part = same[~(rng.random(len(same)) < 0.08)]
    fd = df.index.get_level_values(0).unique()
    extra = [(fd[1], "Q00"), (fd[2], "Q00"), (fd[5], "Q00"), (dd[-1], "S0001"), (dd[-1], "S0002")]
    more = pd.Series(1.0, index=pd.MultiIndex.from_tuples(extra, names=["date", "symbol"]))
    return same, pd.concat([part, more]).sort_index()


def main():
    warnings.filterwarnings("ignore")
    import_reference()
    import portfolio_simulation as ps
    rng = np.random.default_rng(2024)
    st = {}
    for name, method, F, D, A, mw in CASES:
        df, dates, syms = factors(rng, name, F, D, A)
        ret, cap, dd, ss = market(rng, dates, syms)
        ss = list(ss) + ["Q00"]
        inv_same, inv_diff = investability(rng, df, dd)
        st[f"{name}_dims"] = np.array([F, D, A, len(dd), len(ss)], dtype=np.int64)
        st[f"{name}_method"] = np.array(method)
        st[f"{name}_mw"] = np.array(mw)
        st[f"{name}_X"] = df.to_numpy(dtype=np.float64)
        put_series(st, f"{name}_rows", pd.Series(0.0, index=df.index), dd, ss)
        put_series(st, f"{name}_ret", ret, dd, ss)
        put_series(st, f"{name}_cap", cap, dd, ss)
        put_series(st, f"{name}_inv_same", inv_same, dd, ss)
        put_series(st, f"{name}_inv_diff", inv_diff, dd, ss)
        for ikey, inv in (("same", inv_same), ("diff", inv_diff)):
            for tc in (True, False):
                key = f"{name}_{ikey}_tc{int(tc)}"
                for f in df.columns:
                    frame = df.copy()
                    settings = ps.SimulationSettings(returns=ret, cap_flag=cap, investability_flag=inv,
                                                     factors_df=frame, method=method, pct=0.15, max_weight=mw,
                                                     plot=False, transaction_cost=tc, output_returns=True)
                    res = ps.Simulation(name=f, custom_feature=df[f], settings=settings).run()
                    res = res.set_index("date").sort_index()
                    st[f"{key}_{f}_res_d"] = pd.Index(dd).get_indexer(res.index).astype(np.int32)
                    st[f"{key}_{f}_res_v"] = res[COLS].to_numpy(dtype=np.float64)
                    if tc:
                        sim = ps.Simulation(name=f, custom_feature=df[f] * inv, settings=settings)
                        _, counts = sim._daily_trade_list()
                        st[f"{name}_{ikey}_{f}_cnt_d"] = pd.Index(dd).get_indexer(counts.index).astype(np.int32)
                        st[f"{name}_{ikey}_{f}_cnt_v"] = counts[["long_count", "short_count"]].to_numpy(dtype=np.int64)
    np.savez_compressed(os.path.join(OUT, "factor_returns.npz"), **st)
    print("wrote factor_returns.npz:", len(st), "arrays,", os.path.getsize(os.path.join(OUT, "factor_returns.npz")),
          "bytes")


if __name__ == "__main__":
    main()
