"""The ragged multi-manager panel shared by test_gpu_mm_mvo.py, test_mm_mvo_host.py and
tests/golden/make_golden_mm_mvo_ragged.py.  Plain numpy / pandas, written from the specification
of ``multi_manager.compute_multimanager_weights`` with MVO managers (multi_manager.py:32-81:
manager f is ``Simulation._daily_trade_list`` over ``factors_df[f].dropna()``), not from the
kernels.

``ragged_case(A)``: F = 5 managers over D = 12 feature dates and A symbols, 20 returns dates (10
before the second feature date, 10 between the later ones), lookback 5.  The builder asserts
every property the tests rely on:

* manager 0 is dense, manager 1 has scattered NaN cells, manager 2 has two consecutive dates
  that are entirely NaN in the middle, manager 3 has one date with a single non-NaN row and one
  date with only positive signals, manager 4 is NaN on its first three dates;
* the first feature date precedes all returns (no window: the equal-weight book);
* the returns panel is ragged, and at least one (manager, date) window differs from manager 0's
  window on the same date (a table shared by the managers would be wrong);
* every symbol has a non-NaN row in every manager at least once, so each manager's own grid has
  the panel's A columns.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pandas as pd

F, D, LOOKBACK, SHRINK, PCT = 5, 12, 5, 0.1, 0.1
GAP = (5, 6)            # manager 2: no rows on these dates
SINGLE, ONE_SIDED = 4, 8   # manager 3: one row / only positive signals
LATE = 3                # manager 4: no rows on dates 0 .. LATE - 1
THIN = 10               # the returns date (position in the returns calendar) with rows for two symbols only
NAMES = [f"m{k}" for k in range(F)]


def spec_window_dates(series: pd.Series, returns: pd.Series, date, lookback: int):
    """The returns dates of ``date``'s window for the manager ``series`` (:319-334): rows of the
    day's symbols dated before ``date``, the last ``lookback`` distinct dates among them."""
    syms = series.xs(date, level=0).index
    dl = returns.index.get_level_values(0)
    keep = np.asarray(returns.index.get_level_values(1).isin(syms)) & np.asarray(dl < date)
    return list(np.unique(dl[keep].values)[-lookback:])


@functools.lru_cache(maxsize=None)
def ragged_case(A: int):
    rng = np.random.default_rng(1000 + A)
    cal = pd.bdate_range("2023-03-01", periods=22)
    fdates = cal[[0] + list(range(11, 22))]            # day 0, then days 11 .. 21
    rdates = cal[1:21]                                 # days 1 .. 20
    syms = np.array([f"S{k:04d}" for k in range(A)], dtype=object)
    u = max(0.03, 6.0 / A)

    X = rng.standard_normal((F, D, A))
    X[1][rng.random((D, A)) < 0.12] = np.nan
    X[1, 1, :2] = np.nan                               # manager 1 lacks the THIN date's two symbols on date 1
    X[2, GAP[0]] = np.nan
    X[2, GAP[1]] = np.nan
    X[3, SINGLE] = np.nan
    X[3, SINGLE, 7] = 0.8
    X[3, ONE_SIDED] = np.abs(X[3, ONE_SIDED]) + 0.01
    X[4, :LATE] = np.nan
    idx = pd.MultiIndex.from_product([fdates, syms], names=["date", "symbol"])
    factors_df = pd.DataFrame(X.transpose(1, 2, 0).reshape(D * A, F), index=idx, columns=NAMES)

    common = rng.standard_normal((len(rdates), 1))
    R = 0.01 * (0.6 * common + rng.standard_normal((len(rdates), A)) * rng.uniform(0.3, 2.0, A))
    have = rng.random((len(rdates), A)) > 0.15
    have[THIN - 1] = False                             # rdates[THIN - 1] is the last returns date before fdates[1]
    have[THIN - 1, :2] = True
    ridx = pd.MultiIndex.from_product([rdates, syms], names=["date", "symbol"])
    returns = pd.Series(R.reshape(-1), index=ridx, name="ret")[have.reshape(-1)]

    wd = fdates[2:]
    fw = pd.DataFrame(rng.random((len(wd), F + 1)), index=pd.Index(wd, name="date"),
                      columns=["m2", "m0", "zz", "m4", "m1", "m3"])
    fw.iloc[::4, 1] = 0.0
    fw = fw.div(fw.sum(axis=1), axis=0)

    series = [factors_df[n].dropna() for n in NAMES]
    # ---- the properties the tests rely on
    ok = ~np.isnan(X)
    assert ok[0].all()
    assert 0 < (~ok[1]).sum() < ok[1].size and ok[1].any(axis=1).all()
    assert not ok[2, GAP[0]].any() and not ok[2, GAP[1]].any() and GAP[1] == GAP[0] + 1 and 0 < GAP[0] < D - 2
    assert ok[2, [d for d in range(D) if d not in GAP]].all()
    assert ok[3, SINGLE].sum() == 1 and ok[3, ONE_SIDED].all() and (X[3, ONE_SIDED] > 0).all()
    assert not ok[4, :LATE].any() and ok[4, LATE:].all()
    assert fdates[0] < rdates[0] and rdates[THIN - 1] < fdates[1] <= rdates[THIN]
    assert len(returns) < len(ridx)
    assert ok.any(axis=1).all(), "every symbol has a row in every manager"
    w0 = spec_window_dates(series[0], returns, fdates[1], LOOKBACK)
    w1 = spec_window_dates(series[1], returns, fdates[1], LOOKBACK)
    assert w0 != w1 and len(w0) == len(w1) == LOOKBACK and rdates[THIN - 1] in w0 and rdates[THIN - 1] not in w1
    return SimpleNamespace(A=A, X=X, factors_df=factors_df, returns=returns, fw=fw, fdates=fdates, rdates=rdates,
                           syms=syms, u=u, series=series, names=NAMES)


def settings_kw(case, method="mvo", **kw):
    """Keyword arguments of SimulationSettings for the case."""
    idx = case.factors_df.index
    out = dict(returns=case.returns, cap_flag=pd.Series(1.0, index=idx), investability_flag=pd.Series(1.0, index=idx),
               factors_df=case.factors_df, method=method, max_weight=case.u, pct=PCT, lookback_period=LOOKBACK,
               shrinkage_intensity=SHRINK, plot=False)
    out.update(kw)
    return out


def scatter(case, shifted: pd.Series, counts: pd.DataFrame):
    """One manager's (shifted, counts) on the panel grid: ([D][A] NaN = no row or a shifted-in
    NaN, [D][2] NaN = no book that date)."""
    W = np.full((D, case.A), np.nan)
    c = np.full((D, 2), np.nan)
    d = case.fdates.get_indexer(shifted.index.get_level_values(0))
    a = pd.Index(case.syms).get_indexer(shifted.index.get_level_values(1))
    W[d, a] = shifted.to_numpy(dtype=np.float64)
    c[case.fdates.get_indexer(counts.index)] = counts[["long_count", "short_count"]].to_numpy(dtype=np.float64)
    return W, c
