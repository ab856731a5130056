"""multi_manager.compute_multimanager_weights on the GPU.

Reference: multi_manager.py:32-81.  Each factor is a manager whose book is
Simulation._daily_trade_list over ``factors_df[fac].dropna()`` with the settings' method
('equal' or 'linear'); all managers' books come from ONE batched launch (``fmx_trade_books``,
NaN cells = no row), and each weight date folds the managers' books and counts in
``factor_weights`` column order (``k_mm_combine``).  Returns the reference's
``(final_weights, final_counts)``: nonzero weights over ``(date, symbol)``, counts indexed
by date.  'mvo' / 'mvo_turnover' managers (a QP per date) are solved for all managers in one
device pass as well (``simulation.mvo_manager_books``: one returns upload, a window per
(manager, date), 'mvo' as one launch over all (manager, date) rows, 'mvo_turnover' as one
chain per manager over the manager's own dates) whenever the method runs natively
(``simulation.mvo_runs_natively``; 'mvo_turnover' needs ``FMX_SIM_MVO_TURNOVER=native`` on top,
``simulation.mvo_turnover_runs_natively``).  Otherwise -- ``use_cvxpy=False``,
``FMX_SIM_MVO=reference``, no GPU, inputs outside the kernels' caps -- their books come from
``compute_manager_weights``, the drop-in ``Simulation._daily_trade_list``, one manager at a
time (``_host_books``), and fold on the device like the others.  Columns
absent from ``factors_df`` log the reference's warning (:42-44).  Symbol order within a date: ``daily_weights.add(mgr_w_today * fac_w,
fill_value=0)`` (:63) aligns the first-appearance ``all_symbols`` index with a manager's
date-sorted book index; unless the two are identical pandas returns their sorted union,
and a date without any contribution holds only zeros (dropped by ``!= 0``), so the
surviving weights of every date are in sorted symbol order.
"""
from __future__ import annotations

import logging

import numpy as np
import pandas as pd
import torch

from . import engine as E
from .panel import device, panel_index
from .simulation import by_date, mvo_manager_books, mvo_runs_natively, mvo_turnover_runs_natively, trade_books

logger = logging.getLogger("multi_manager")
HOST_METHODS = ("mvo", "mvo_turnover")


def _setting(settings, key, default):
    if isinstance(settings, dict):
        return settings.get(key, default)
    return getattr(settings, key, default)


def _host_books(pi, factors_df, mgrs, settings, dev):
    """Books of host-solved managers (multi_manager.py:45-48): each factor's
    ``dropna()`` series through ``compute_manager_weights``, scattered onto the panel grid
    ([F][D][A] shifted weights, NaN = no row; [F][D][2] counts, NaN = no book that date)."""
    F, D, A = len(mgrs), pi.D, pi.A
    Wf = np.full((F, D, A), np.nan)
    cnt = np.full((F, D, 2), np.nan)
    for f, fac in enumerate(mgrs):
        w, c = compute_manager_weights(factors_df[fac].dropna(), settings, name=fac)
        if len(w):
            d = pi.dates.get_indexer(w.index.get_level_values(0))
            a = pi.symbols.get_indexer(w.index.get_level_values(1))
            Wf[f, d, a] = w.to_numpy(dtype=np.float64, na_value=np.nan)
        if len(c):
            cnt[f, pi.dates.get_indexer(c.index)] = c[["long_count", "short_count"]].to_numpy(dtype=np.float64)
    return torch.as_tensor(Wf, device=dev), torch.as_tensor(cnt, device=dev)


def _mvo_settings(settings):
    """The MVO fields of the settings, with SimulationSettings' defaults."""
    return {k: _setting(settings, k, d) for k, d in (("returns", None), ("use_cvxpy", True), ("lookback_period", 60),
                                                     ("shrinkage_intensity", 0.1), ("turnover_penalty", 0.1),
                                                     ("return_weight", 0.0))}


def _batched(method, factors_df, mgrs, settings) -> bool:
    """Whether all managers' books of ``method`` come from ``mvo_manager_books``: the conditions
    under which ``Simulation`` itself solves the method on the device."""
    m = _mvo_settings(settings)
    args = (factors_df[mgrs], m["returns"], m["use_cvxpy"], m["lookback_period"], m["shrinkage_intensity"])
    if method == "mvo":
        return mvo_runs_natively(*args)
    return mvo_turnover_runs_natively(*args, m["turnover_penalty"], m["return_weight"])


def _device_books(factors_df, mgrs, method, pct, max_weight, settings):
    """All MVO managers' books in one device pass; the iteration-limit / x0 report of
    ``Simulation._native_mvo_trade_list`` once for the batch."""
    m = _mvo_settings(settings)
    kw = {"turnover_penalty": float(m["turnover_penalty"]), "return_weight": float(m["return_weight"])} \
        if method == "mvo_turnover" else {}
    Wf, cnt, extra = mvo_manager_books(factors_df, mgrs, m["returns"], method, pct, max_weight, int(m["lookback_period"]),
                                       float(m["shrinkage_intensity"]), return_info=True, **kw)
    st = extra["info"][:, :, 0]
    n1, n2 = int((st == 1).sum()), int((st == 2).sum())
    if n1 or n2:
        logger.warning("%s: of %d manager days over %d managers, %d stopped at the iteration limit (last iterate kept) "
                       "and %d took the equal-leg fallback x0 (one-row window or max_weight too small for a leg)",
                       method, int((st != 5).sum()), len(mgrs), n1, n2)
    return Wf, cnt


def compute_multimanager_weights(factors_df: pd.DataFrame, factor_weights: pd.DataFrame, settings):
    method = _setting(settings, "method", "equal")
    pct = float(_setting(settings, "pct", 0.1))
    max_weight = float(_setting(settings, "max_weight", 0.03))
    mgrs = []
    for fac in factor_weights.columns:
        if fac not in factors_df.columns:
            logger.warning(f"Factor {fac} not in factors_df, skipping.")
            continue
        if fac not in mgrs:
            mgrs.append(fac)
    if mgrs and method not in ("equal", "linear") + HOST_METHODS:
        raise ValueError(f"Unknown method {method}")
    if method in HOST_METHODS and _setting(settings, "risk_model", None) is not None:
        raise ValueError("risk_model: the multi-manager MVO books against a factor risk model are out of scope; "
                         "run Simulation(method='mvo', risk_model=...) per manager")
    all_symbols = factors_df.index.get_level_values("symbol").unique()
    if len(factor_weights.index) == 0:
        return pd.Series(dtype=float), pd.DataFrame(columns=["long_count", "short_count"])
    factors_df = by_date(factors_df)
    pi = panel_index(factors_df.index)
    dev = device()
    F, D, A = len(mgrs), pi.D, pi.A
    if F and method in HOST_METHODS and _batched(method, factors_df, mgrs, settings):
        Wf, cnt = _device_books(factors_df, mgrs, method, pct, max_weight, settings)
    elif F and method in HOST_METHODS:
        Wf, cnt = _host_books(pi, factors_df, mgrs, settings, dev)
    elif F:
        Wf, cnt = trade_books(pi, factors_df[mgrs].to_numpy(dtype=np.float64), method, pct, max_weight, True)
    else:
        Wf = torch.empty((1, D, A), dtype=torch.float64, device=dev)
        cnt = torch.full((1, D, 2), float("nan"), dtype=torch.float64, device=dev)
    colmap = [mgrs.index(c) if c in mgrs else -1 for c in factor_weights.columns]
    wdate = pi.dates.get_indexer(factor_weights.index)
    out, oc = E.mm_combine(Wf, cnt, factor_weights.to_numpy(dtype=np.float64), colmap, wdate)
    perm = pi.symbols.get_indexer(all_symbols.sort_values())
    out = out.cpu().numpy()[:, perm]
    oc = oc.cpu().numpy()
    index = pd.MultiIndex.from_product([factor_weights.index, all_symbols.sort_values()], names=["date", "symbol"])
    final = pd.Series(out.reshape(-1), index=index)
    final = final[final != 0]
    counts = pd.DataFrame({"long_count": oc[:, 0], "short_count": oc[:, 1]},
                          index=pd.Index(factor_weights.index, name="date"))
    return final, counts


def compute_manager_weights(factor_series, settings, name="manager"):
    """multi_manager.py:15-29: one manager's book through Simulation._daily_trade_list."""
    from .portfolio_simulation import Simulation, SimulationSettings
    sim_settings = settings if isinstance(settings, SimulationSettings) else SimulationSettings(**settings)
    sim = Simulation(name=name, custom_feature=factor_series, settings=sim_settings)
    return sim._daily_trade_list()


def run_multimanager_backtest(factors_df, returns, cap_flag, factor_weights, settings):
    """multi_manager.py:84-100: combined book -> Simulation._daily_portfolio_returns (device)."""
    from .portfolio_simulation import Simulation, SimulationSettings
    weights, counts = compute_multimanager_weights(factors_df, factor_weights, settings)
    sim_settings = settings if isinstance(settings, SimulationSettings) else SimulationSettings(**settings)
    sim = Simulation(name="multimanager", custom_feature=weights, settings=sim_settings)
    result, top_longs, top_shorts = sim._daily_portfolio_returns(weights)
    return result, top_longs, top_shorts, counts
