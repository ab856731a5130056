"""Backtest every factor column in one device pass: the ``factor_ret_df`` the selectors read.

``single_factor_backtests(factors_df, settings)`` returns, per result column of
``Simulation.run()`` (``log_return``, ``long_return``, ``short_return``, ``long_turnover``,
``short_turnover``, ``turnover``) and per count column of ``_daily_trade_list()``
(``long_count``, ``short_count``), one DataFrame of dates (ascending) x factors.  Column f is
what ``Simulation(f, factors_df[f], settings)`` produces with ``plot=False,
output_returns=True, output_summary=False, contributor=False``: ``run().set_index("date")
.sort_index()`` for the result columns, the counts of ``_daily_trade_list()`` on the
investability-masked signal for the two counts.  ``single_factor_returns`` is the
``log_return`` frame: the dates x factors table ``FactorSelector`` takes as ``factor_ret_df``.
Unlike the reference's ``run()`` (portfolio_simulation.py:72) nothing is written into
``factors_df`` or ``settings.factors_df``.

``backend="loop"`` is that per-factor loop over ``Simulation`` (the steps of ``run()``,
:73-75, without the reporting object, which does not change the result).
``backend="batched"`` does the work once for all factors ('equal' and 'linear'):

* the investability product ``factors_df[cols] * investability_flag`` as pandas aligns it
  (identical indexes keep their row order, otherwise ``Index.join(how="outer")``; a NaN cell
  is a row with weight 0), computed on the device from one upload of the columns;
* one union ``(date, symbol)`` grid of the feature's, the returns' and the cap flags' rows
  (``portfolio_simulation._Grid``), returns and cap flags uploaded once;
* the same-day books of a chunk of factors from ``engine.trade_books`` (``raw=True``,
  ``nan_absent=False``) directly on that grid;
* ``engine.pnl_books``: the six per-date sums of ``k_pnl_daily`` for every book of the chunk,
  the per-symbol ``shift(1)`` folded into the read through one shared previous-row table;
* the reference's outer-join index bookkeeping (:750-790) once, applied to all factors.

Both backends give the same bits: the books are the same kernels' output and
``fmx_pnl_books`` keeps ``k_pnl_daily``'s summation schedule per (book, date).
"""
from __future__ import annotations

import dataclasses

import numpy as np
import pandas as pd
import torch

from . import engine as E
from .panel import device, panel_index
from .simulation import MM_CHUNK_BYTES

COUNT_COLS = ["long_count", "short_count"]
BATCHED_METHODS = ("equal", "linear")


def _ps():
    from . import portfolio_simulation
    return portfolio_simulation


def _as_settings(settings):
    """A ``SimulationSettings`` from one or from a dict of its fields (as ``multi_manager``
    accepts), with the per-run reporting switched off."""
    cls = _ps().SimulationSettings
    if not isinstance(settings, cls):
        fields = dict(settings)
        for k in ("returns", "cap_flag", "investability_flag", "factors_df"):
            fields.setdefault(k, None)
        settings = cls(**fields)
    return dataclasses.replace(settings, plot=False, output_returns=True, output_summary=False, contributor=False)


def batched_ineligible(factors_df, settings):
    """Why the one-pass path cannot run these inputs (a sentence), or None when it can."""
    if settings.method not in BATCHED_METHODS:
        return (f"method {settings.method!r}: the batched path runs 'equal' and 'linear' "
                f"(the MVO methods take the per-factor loop)")
    for name, obj in (("factors_df", factors_df), ("returns", settings.returns), ("cap_flag", settings.cap_flag),
                      ("investability_flag", settings.investability_flag)):
        idx = getattr(obj, "index", None)
        if not isinstance(idx, pd.MultiIndex) or idx.nlevels != 2 or not idx.is_unique:
            return f"{name}: its index is not a unique two-level (date, symbol) MultiIndex"
    if not torch.cuda.is_available():
        return "no GPU is visible"
    return None


def _frames(result_index, results, count_index, counts, cols):
    """{field: DataFrame dates x cols} from [F][n] arrays."""
    out = {}
    for k, v in results.items():
        out[k] = pd.DataFrame(np.ascontiguousarray(v.T), index=result_index, columns=pd.Index(cols))
    for k, v in counts.items():
        out[k] = pd.DataFrame(np.ascontiguousarray(v.T), index=count_index, columns=pd.Index(cols))
    return out


# ----------------------------------------------------------------------------- loop
def _loop(factors_df, st, cols):
    ps = _ps()
    res, cnt = {}, {}
    for f in cols:
        sim = ps.Simulation(f, factors_df[f], st)
        sim.custom_feature = sim.custom_feature * sim.investability_flag          # run(), :73
        weights, counts = sim._daily_trade_list()
        result, _, _ = sim._daily_portfolio_returns(weights)
        res[f] = result.set_index("date").sort_index()
        cnt[f] = counts
    fields = {}
    for k in ps.RESULT_COLS:
        fields[k] = (pd.concat([res[f][k].rename(f) for f in cols], axis=1) if cols
                     else pd.DataFrame(index=pd.Index([], name="date")))
    for k in COUNT_COLS:
        fields[k] = (pd.concat([cnt[f][k].rename(f) for f in cols], axis=1) if cols
                     else pd.DataFrame(index=pd.Index([], name="date")))
    for v in fields.values():
        v.columns = pd.Index(cols)
    return fields


# ----------------------------------------------------------------------------- batched
def _feature_rows(factors_df, inv):
    """The index of ``factors_df[f] * inv`` (the same for every f) in the order the trade list
    walks it, with each row's source positions: (index, rows of factors_df, rows of inv), -1 =
    that side has no such row (pandas Series alignment: equal indexes are kept as they are,
    otherwise the outer join)."""
    fi, ii = factors_df.index, inv.index
    if fi.equals(ii):
        idx, li, ri = fi, None, None
    else:
        idx, li, ri = fi.join(ii, how="outer", return_indexers=True)
    n = len(idx)
    li = np.arange(n, dtype=np.int64) if li is None else np.asarray(li, dtype=np.int64)
    ri = np.arange(n, dtype=np.int64) if ri is None else np.asarray(ri, dtype=np.int64)
    dl = idx.get_level_values(0)
    if not dl.is_monotonic_increasing:                    # simulation.by_date
        order = np.argsort(dl.values, kind="stable")
        idx, li, ri = idx[order], li[order], ri[order]
    return idx, li, ri


def _prev_rows(present):
    """int32 [D][A]: the previous date on which the symbol has a feature row, -1 for a cell
    without a row and for a symbol's first row."""
    D, A = present.shape
    rows = np.where(present, np.arange(D, dtype=np.int32)[:, None], np.int32(-1))
    last = np.maximum.accumulate(rows, axis=0)
    prev = np.full((D, A), -1, dtype=np.int32)
    prev[1:] = last[:-1]
    return np.where(present, prev, np.int32(-1)).astype(np.int32)


def _factor_bytes(D, A, n):
    """Device bytes one factor needs in a chunk: the signal, the same-day and the shifted book
    ([D][A] doubles), the uploaded column and its product ([n] doubles), counts and sums."""
    return 8 * (3 * D * A + 3 * n + 8 * D)


def _batched(factors_df, st, cols, chunk_bytes):
    ps = _ps()
    dev = device()
    inv = st.investability_flag
    idx, li, ri = _feature_rows(factors_df, inv)
    pi = panel_index(idx)
    n = pi.n
    feature = pd.Series(np.zeros(n), index=idx)           # the weights' rows: index only
    g = ps._Grid(feature, st.returns, st.cap_flag)
    D, A = g.D, g.A
    gd = g.dates.get_indexer(pi.dates)                    # feature dates / symbols on the union grid
    gs = g.symbols.get_indexer(pd.Index(np.asarray(pi.symbols, dtype=object)))
    dG, sG = gd[pi.d], gs[pi.s]
    flat = dG * A + sG
    present = np.zeros(D * A, dtype=bool)
    present[flat] = True
    present = present.reshape(D, A)
    dense = bool(present.all())
    wmask, rmask, cmask = g.date_mask(feature), g.date_mask(st.returns), g.date_mask(st.cap_flag)
    wrows = np.flatnonzero(wmask)
    wprev = np.full(D, -1, dtype=np.int32)
    wprev[wrows[1:]] = wrows[:-1]                         # diff() over the weights' own dates

    R = torch.as_tensor(g.dense(st.returns), device=dev)
    CAP = torch.as_tensor(g.dense(st.cap_flag), device=dev) if st.cap_flag is not None else None
    pres_d = None if dense else torch.as_tensor(present.astype(np.uint8), device=dev)
    prev_d = None if dense else torch.as_tensor(_prev_rows(present), device=dev)
    iv = inv.to_numpy(dtype=np.float64, na_value=np.nan)
    iv = np.where(ri >= 0, iv[np.maximum(ri, 0)], np.nan) if len(iv) else np.full(n, np.nan)
    iv_d = torch.as_tensor(iv, device=dev)
    li_d = torch.as_tensor(np.maximum(li, 0), device=dev)
    lmiss_d = torch.as_tensor(li < 0, device=dev) if (li < 0).any() else None
    flat_d = torch.as_tensor(flat, device=dev)
    pos, width, sorted_within = pi.row_layout()
    by_rows = st.method == "linear" and not sorted_within  # pairwise sums in input order
    if by_rows:
        dG_d, sG_d, pos_d = (torch.as_tensor(a, device=dev) for a in (dG, sG, pos))
        pr = np.zeros((D, width), dtype=np.uint8)
        pr[dG, pos] = 1
        pr_d = torch.as_tensor(pr, device=dev)

    F = len(cols)
    budget = MM_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
    Fc = max(1, min(F, budget // max(1, _factor_bytes(D, max(A, width if by_rows else 0), n))))
    O = np.empty((F, D, 6))
    C = np.empty((F, D, 2))
    for f0 in range(0, F, Fc):
        v = factors_df[cols[f0:f0 + Fc]].to_numpy(dtype=np.float64, na_value=np.nan)    # [n0][k]
        fmajor = v.T.flags.c_contiguous
        t = torch.as_tensor(v.T if fmajor else np.ascontiguousarray(v), device=dev)
        t = t if fmajor else t.T                                                       # [k][n0] view
        k = t.shape[0]
        if len(factors_df.index):
            t = t[:, li_d]
        else:
            t = torch.full((k, n), float("nan"), dtype=torch.float64, device=dev)
        if lmiss_d is not None:
            t[:, lmiss_d] = float("nan")
        t = t * iv_d[None, :]                                                           # run(), :73
        if by_rows:
            X = torch.full((k, D, width), float("nan"), dtype=torch.float64, device=dev)
            X[:, dG_d, pos_d] = t
            _, counts, Wr = E.trade_books(X, st.method, st.pct, st.max_weight, present=pr_d, nan_absent=False,
                                          raw=True)
            W = torch.full((k, D, A), float("nan"), dtype=torch.float64, device=dev)
            W[:, dG_d, sG_d] = Wr[:, dG_d, pos_d]
        else:
            X = torch.full((k, D * A), float("nan"), dtype=torch.float64, device=dev)
            X[:, flat_d] = t
            _, counts, W = E.trade_books(X.reshape(k, D, A), st.method, st.pct, st.max_weight, present=pres_d,
                                         nan_absent=False, raw=True)
        O[f0:f0 + k] = E.pnl_books(W, R, CAP, wprev, prev_d).cpu().numpy()
        C[f0:f0 + k] = counts.cpu().numpy()
        del t, X, W, counts

    # the reference's outer-join bookkeeping (:750-790), once for all factors
    nan = np.nan
    m_wr, m_wc = wmask | rmask, wmask | cmask
    long_raw, short_raw = O[:, :, 0], -O[:, :, 1]
    if st.transaction_cost:
        keep, both = m_wr | m_wc, m_wr & m_wc
        long_ret = np.where(both[None, :], long_raw - O[:, :, 4], nan)
        short_ret = np.where(both[None, :], short_raw - O[:, :, 5], nan)
    else:
        keep = m_wr
        long_ret, short_ret = long_raw, short_raw
    net = long_ret + short_ret
    lt = np.where(wmask[None, :], O[:, :, 2], nan)
    stn = np.where(wmask[None, :], O[:, :, 3], nan)
    results = dict(zip(ps.RESULT_COLS, (a[:, keep] for a in (net, long_ret, short_ret, lt, stn, lt + stn))))
    counts = {c: C[:, gd, j].astype(np.int64) for j, c in enumerate(COUNT_COLS)}
    return _frames(pd.Index(g.dates[keep], name="date"), results, pd.Index(pi.dates, name=idx.names[0]), counts, cols)


# ----------------------------------------------------------------------------- public
def single_factor_backtests(factors_df: pd.DataFrame, settings, columns=None, backend: str = "auto",
                            chunk_bytes: int = None):
    """{field: DataFrame dates x factors} for the six result columns of ``Simulation.run()`` and
    the two counts of ``_daily_trade_list()``, one column per factor in ``columns`` (default:
    all of ``factors_df.columns``, in that order).  ``settings`` is a ``SimulationSettings`` or
    a dict of its fields; ``contributor``, ``output_summary`` and ``plot`` are ignored.
    ``backend``: "batched" (one pass; raises ``ValueError`` naming the reason when it cannot
    run the inputs), "loop" (``Simulation`` per factor) or "auto" (batched when eligible).
    ``chunk_bytes`` caps the device tensors of one chunk of factors (default
    ``simulation.MM_CHUNK_BYTES``); the result does not depend on it."""
    if backend not in ("auto", "batched", "loop"):
        raise ValueError(f"backend must be 'auto', 'batched' or 'loop', got {backend!r}")
    st = _as_settings(settings)
    cols = list(factors_df.columns) if columns is None else list(columns)
    missing = [c for c in cols if c not in factors_df.columns]
    if missing:
        raise KeyError(f"columns not in factors_df: {missing}")
    if backend != "loop":
        why = batched_ineligible(factors_df, st)
        if why is None:
            return _batched(factors_df, st, cols, chunk_bytes)
        if backend == "batched":
            raise ValueError(f"single_factor_backtests(backend='batched') cannot run these inputs: {why}")
    return _loop(factors_df, st, cols)


def single_factor_returns(factors_df: pd.DataFrame, settings, columns=None, field: str = "log_return", **kw):
    """One field of ``single_factor_backtests`` (default ``log_return``): the dates x factors
    table ``FactorSelector`` takes as ``factor_ret_df``."""
    if field not in _ps().RESULT_COLS + COUNT_COLS:
        raise ValueError(f"field must be one of {_ps().RESULT_COLS + COUNT_COLS}, got {field!r}")
    return single_factor_backtests(factors_df, settings, columns=columns, **kw)[field]


def cross_sectional_factor_returns(factors_df: pd.DataFrame, returns: pd.Series, lag: int = 1,
                                   intercept: bool = True, weights=None, full: bool = False):
    """Pure factor returns (Fama-MacBeth / Barra style; builder-defined): on every date the
    returns are regressed on ALL factor columns at once, each shifted ``lag`` rows per symbol
    (``ts_delay``, row-based on ragged panels), by ``engine.cs_ols``.  ``returns`` and
    ``weights`` are aligned to ``factors_df.index``.  Returns the ``dates x factors`` table of
    coefficients (index named ``date``, columns in input order; a collinear column's return is
    NaN on that date, and so is every column of a date with fewer rows than coefficients) --
    usable as ``FactorSelector``'s ``factor_ret_df``.  ``full=True`` returns
    ``(table, stats)`` with ``stats`` a DataFrame of ``alpha``, ``r2`` and ``n`` per date."""
    pi = panel_index(factors_df.index)
    dev = device()
    present = pi.present(dev)
    X = E.ts("delay", pi.to_device(factors_df.to_numpy(dtype=np.float64, na_value=np.nan), dev), int(lag), present)
    Y = pi.to_device(returns.reindex(factors_df.index).to_numpy(dtype=np.float64, na_value=np.nan), dev)
    W = None
    if weights is not None:
        W = pi.to_device(weights.reindex(factors_df.index).to_numpy(dtype=np.float64, na_value=np.nan), dev)[0]
    res = E.cs_ols(Y, X, W, present, intercept, want=("beta", "alpha", "r2", "n") if full else ("beta",))
    dates = pd.Index(pi.dates, name="date")
    table = pd.DataFrame(res["beta"][0].cpu().numpy(), index=dates, columns=factors_df.columns)
    if not full:
        return table
    stats = pd.DataFrame({"alpha": res["alpha"][0].cpu().numpy(), "r2": res["r2"][0].cpu().numpy(),
                          "n": res["n"][0].cpu().numpy()}, index=dates)
    return table, stats


def rolling_factor_exposures(returns: pd.Series, factor_ret_df: pd.DataFrame, window: int, intercept: bool = True):
    """Rolling factor betas per symbol (builder-defined): every symbol's returns regressed on
    the K factor-return series of ``factor_ret_df`` (a ``dates x factors`` table, exactly what
    ``cross_sectional_factor_returns`` or ``single_factor_returns`` produce; reindexed to the
    panel's dates) over the symbol's last ``window`` valid rows, in one ``engine.ts_ols`` call
    with the table shared by all symbols.  Returns ``(beta, resid, sigma)``: the exposures as a
    DataFrame on ``returns.index`` with the table's columns, the idiosyncratic return and its
    rolling volatility (the residual standard error of the window) as Series on the same
    index; NaN where the row is invalid or the symbol has fewer than ``window`` valid rows."""
    pi = panel_index(returns.index)
    dev = device()
    Y = pi.to_device(returns.to_numpy(dtype=np.float64, na_value=np.nan), dev)
    tab = factor_ret_df.reindex(pi.dates).to_numpy(dtype=np.float64, na_value=np.nan)
    X = torch.as_tensor(np.ascontiguousarray(tab.T), device=dev)
    res = E.ts_ols(Y, X, window, pi.present(dev), intercept, shared=True, want=("beta", "resid", "sigma"))
    beta = pd.DataFrame(pi.from_device(res["beta"][0]), index=returns.index, columns=factor_ret_df.columns)
    resid = pd.Series(pi.from_device(res["resid"])[:, 0], index=returns.index, name="resid")
    sigma = pd.Series(pi.from_device(res["sigma"])[:, 0], index=returns.index, name="sigma")
    return beta, resid, sigma
