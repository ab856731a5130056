"""Daily trade list of portfolio_simulation.Simulation on the GPU.

``daily_trade_list(custom_feature, pct)`` returns what ``Simulation._daily_trade_list()``
returns for ``method='equal'`` (portfolio_simulation.py:96-170): the per-symbol
``shift(1)`` of each day's equal-weight long/short book (a Series over the sorted
``(date, symbol)`` rows of ``custom_feature``) and the ``long_count`` / ``short_count``
DataFrame indexed by date.  Computed by ``k_trade_equal`` / ``k_trade_linear`` (normalised
legs + cap-and-redistribute, :172-181, :250-313) and the per-symbol shift (csrc/sim.hip).

``mvo_trade_list(custom_feature, returns, ...)`` returns the same pair for ``method='mvo'``
(:183-204, :315-461): ``mvo_window_rows`` lists each date's returns window (the last
``lookback_period`` distinct returns dates before it on which one of the day's symbols has a
row), ``k_sim_mvo`` (csrc/sim_mvo.hip) solves every date's minimum-variance QP in one launch,
and days without any returns history take the equal-weight book (:188-190).

``mvo_turnover_trade_list(custom_feature, returns, ...)`` is ``method='mvo_turnover'``
(:206-248, :463-585): the same windows and Sigma, each day's QP with an L1 penalty against
the previous day's book.  ``k_smt_setup`` prepares every date at once and ``k_smt_chain``
walks the dates in order on the device (csrc/sim_mvo_turnover.hip); the drop-in
``Simulation`` routes to it when ``FMX_SIM_MVO_TURNOVER=native`` is set.

``mvo_manager_books(factors_df, cols, returns, method, ...)`` is the books of ALL the MVO
managers of ``multi_manager.compute_multimanager_weights`` in one device pass: manager f is
``factors_df[cols[f]].dropna()``, with its own windows (``engine.sim_mvo_window_rows``) and, for
'mvo_turnover', its own date list (``engine.sim_mvo_turnover_chains``, one chain per manager).

``risk_mvo_trade_list(custom_feature, model, ...)`` is ``mvo_trade_list`` against a fitted
``risk_model.FactorRiskModel`` (Sigma = B'F B + diag(s2) of each date) instead of the returns
window: ``k_risk_mvo`` (csrc/sim_mvo_risk.hip), one launch for all dates.

``mvo_runs_natively`` / ``mvo_turnover_runs_natively`` are the conditions under which the MVO
methods run on the device, shared by ``Simulation`` and ``multi_manager``.
"""
from __future__ import annotations

import logging
import os

import numpy as np
import pandas as pd
import torch

from . import engine as E
from .panel import device, panel_index


def by_date(obj):
    """Rows stably reordered by date when they are not: the trade list groups by date and
    shifts per symbol after sort_index() (portfolio_simulation.py:99, :150-151), so the
    row order across dates does not matter -- but the order inside a date does (linear
    weights' pairwise sums), and a stable sort keeps it."""
    dl = obj.index.get_level_values(0)
    if dl.is_monotonic_increasing:
        return obj
    return obj.iloc[np.argsort(dl.values, kind="stable")]


def trade_books(pi, values: np.ndarray, method: str, pct: float, max_weight: float, nan_absent: bool):
    """Trade books of the F signal columns ``values`` [n][F] over ``pi``'s rows: (shifted
    books [F][D][A], counts [F][D][2]) on the device.  The 'linear' weights are numpy
    pairwise sums over each date's rows in INPUT order (groupby('date') keeps it), so when
    that order is not the sorted-symbol order the kernel runs on a per-date row layout
    and the same-day books are scattered back to symbol columns before the shift."""
    dev = device()
    v = np.asarray(values, dtype=np.float64)
    if v.ndim == 1:
        v = v[:, None]
    pos, width, sorted_within = pi.row_layout()
    if method == "equal" or sorted_within:
        X = torch.as_tensor(pi.to_dense(v), device=dev)
        return E.trade_books(X, method, pct, max_weight, present=pi.present(dev), nan_absent=nan_absent)
    F = v.shape[1]
    Xr = np.full((F, pi.D, width), np.nan)
    Xr[:, pi.d, pos] = v.T
    pr = np.zeros((pi.D, width), dtype=np.uint8)
    pr[pi.d, pos] = 1
    _, counts, Wr = E.trade_books(torch.as_tensor(Xr, device=dev), method, pct, max_weight,
                                  present=torch.as_tensor(pr, device=dev), nan_absent=nan_absent, raw=True)
    d_t = torch.as_tensor(pi.d, device=dev)
    W = torch.full((F, pi.D, pi.A), float("nan"), dtype=torch.float64, device=dev)
    W[:, d_t, torch.as_tensor(pi.s, device=dev)] = Wr[:, d_t, torch.as_tensor(pos, device=dev)]
    return E.shift_rows(W), counts


def daily_trade_list(custom_feature: pd.Series, pct: float = 0.1, method: str = "equal", max_weight: float = 0.03):
    if method not in ("equal", "linear"):
        raise NotImplementedError(f"method {method!r}: the device runs 'equal' and 'linear' (MVO is a host QP)")
    custom_feature = by_date(custom_feature)
    pi = panel_index(custom_feature.index)
    W, counts = trade_books(pi, custom_feature.to_numpy(dtype=np.float64), method, pct, max_weight, False)
    W = W[0].cpu().numpy().reshape(-1)
    counts = counts[0].cpu().numpy()
    order = np.sort(pi.flat)
    d, s = order // pi.A, order % pi.A
    index = pd.MultiIndex.from_arrays([pi.dates[d], pi.symbols[s]], names=list(custom_feature.index.names))
    shifted = pd.Series(W[order], index=index)
    counts_df = pd.DataFrame({"long_count": counts[:, 0].astype(np.int64),
                              "short_count": counts[:, 1].astype(np.int64)},
                             index=pd.Index(pi.dates, name=custom_feature.index.names[0]))
    return shifted, counts_df


def _levels(index: pd.MultiIndex):
    names = list(index.names)
    return (index.get_level_values("date" if "date" in names else 0),
            index.get_level_values("symbol" if "symbol" in names else 1))


def _returns_grid(pi, returns):
    """The returns' rows on the feature's symbol columns: (sorted distinct returns dates,
    row date codes, row symbol columns, keep mask) -- rows of other symbols are dropped."""
    index = returns.index if isinstance(returns, (pd.Series, pd.DataFrame)) else returns
    dl, sl = _levels(index)
    rd, rdates = pd.factorize(dl, sort=True)
    rs = pi.symbols.get_indexer(sl)
    return np.asarray(rdates), rd.astype(np.int64), rs.astype(np.int64), rs >= 0


def mvo_window_rows(feature_index, returns, lookback: int, device=None):
    """Each feature date's returns window (portfolio_simulation.py:319-334) as rows of the
    sorted distinct returns dates: (win_rows int32 [J][Lmax], win_T int32 [J]), ascending
    inside a window, Lmax = min(lookback, number of returns dates) (at least 1).  A returns
    date belongs to date d's candidates when it is < d and one of d's symbols has a returns
    row on it (NaN values included) -- a presence product [J][A] x [A][Dr]; the window is the
    last ``lookback`` candidates, so on a ragged panel it is not a contiguous date range.
    ``feature_index`` is the feature's (date, symbol) MultiIndex (or its PanelIndex),
    ``returns`` the returns Series or its index.  torch ops only: runs on any device."""
    pi = feature_index if hasattr(feature_index, "present_np") else panel_index(feature_index)
    rdates, rd, rs, keep = _returns_grid(pi, returns)
    dev = torch.device(device) if device is not None else torch.device("cpu")
    J, A, Dr = pi.D, pi.A, len(rdates)
    L = max(1, min(int(lookback), Dr))
    if Dr == 0:
        return (torch.zeros((J, L), dtype=torch.int32, device=dev), torch.zeros((J,), dtype=torch.int32, device=dev))
    rp = np.zeros((Dr, A), dtype=np.float32)
    rp[rd[keep], rs[keep]] = 1.0
    fp = np.ones((J, A), dtype=np.float32) if pi.present_np is None else pi.present_np.astype(np.float32)
    hit = (torch.as_tensor(fp, device=dev) @ torch.as_tensor(rp, device=dev).T) > 0.5          # [J][Dr]
    nbefore = np.searchsorted(rdates, np.asarray(pi.dates), side="left")                      # returns dates < d
    hit &= torch.arange(Dr, device=dev)[None, :] < torch.as_tensor(nbefore, device=dev)[:, None]
    after = hit.flip(1).cumsum(1).flip(1)                 # candidates at or after each position
    sel = hit & (after <= L)
    win_T = sel.sum(1)
    jj, rr = sel.nonzero(as_tuple=True)
    win_rows = torch.zeros((J, L), dtype=torch.int32, device=dev)
    win_rows[jj, win_T[jj] - after[jj, rr]] = rr.to(torch.int32)
    return win_rows, win_T.to(torch.int32)


def _series_out(pi, custom_feature, W, counts):
    """(shifted Series over the sorted (date, symbol) rows, counts DataFrame by date)."""
    W = W.cpu().numpy().reshape(-1)
    counts = counts.cpu().numpy()
    order = np.sort(pi.flat)
    d, s = order // pi.A, order % pi.A
    index = pd.MultiIndex.from_arrays([pi.dates[d], pi.symbols[s]], names=list(custom_feature.index.names))
    shifted = pd.Series(W[order], index=index)
    counts_df = pd.DataFrame({"long_count": counts[:, 0].astype(np.int64),
                              "short_count": counts[:, 1].astype(np.int64)},
                             index=pd.Index(pi.dates, name=custom_feature.index.names[0]))
    return shifted, counts_df


def _mvo_inputs(custom_feature, returns, lookback_period, dev):
    """(pi, R0 [Dr][A] zero-filled returns, win_rows, win_T, X [1][D][A], present) on ``dev``."""
    pi = panel_index(custom_feature.index)
    rdates, rd, rs, keep = _returns_grid(pi, returns)
    r0 = np.zeros((max(len(rdates), 1), pi.A))
    rv = returns.to_numpy(dtype=np.float64, na_value=np.nan)[keep]
    r0[rd[keep], rs[keep]] = np.where(np.isnan(rv), 0.0, rv)                                  # fillna(0), :337
    win_rows, win_T = mvo_window_rows(pi, returns, lookback_period, device=dev)
    X = torch.as_tensor(pi.to_dense(custom_feature.to_numpy(dtype=np.float64)), device=dev)      # [1][D][A]
    return pi, torch.as_tensor(r0, device=dev), win_rows, win_T, X, pi.present(dev)


def mvo_turnover_trade_list(custom_feature: pd.Series, returns: pd.Series, pct: float = 0.1, max_weight: float = 0.03,
                            lookback_period: int = 60, shrinkage_intensity: float = 0.1, turnover_penalty: float = 0.1,
                            return_weight: float = 0.0, return_info: bool = False, max_iter: int = 20000,
                            eps: float = 1e-9):
    """``Simulation._daily_trade_list()`` for ``method='mvo_turnover'`` on the device
    (:206-248, :463-585): the same ``(shifted, counts_df)`` pair as ``mvo_trade_list``.  The
    dates form one chain: every date's QP carries the L1 penalty ``turnover_penalty`` against
    the previous date's book and the reward ``return_weight`` on the signal, is solved to its
    optimum and then pruned / renormalised as the reference does
    (engine.sim_mvo_turnover_books).  Days without returns history carry the equal-weight book
    (``k_trade_equal``), which is the next day's previous book like any other.  With
    ``return_info`` a third value holds ``info`` [D][6], the same-day ``books`` [D][A], the
    solver's ``opt`` [D][A] before the prune / renormalise step and their ``dates`` / ``symbols``."""
    custom_feature = by_date(custom_feature)
    dev = device()
    pi, R0, win_rows, win_T, X, present = _mvo_inputs(custom_feature, returns, lookback_period, dev)
    W = torch.zeros_like(X)
    eq = win_T == 0
    ce = None
    if bool(eq.any()):
        _, ce, we = E.trade_books(X, "equal", pct, max_weight, present=present, nan_absent=False, raw=True)
        W[0][eq] = we[0][eq]
    W, counts, info, Wopt = E.sim_mvo_turnover_books(R0, win_rows, win_T, X, present, W, shrinkage_intensity,
                                                     max_weight, turnover_penalty, return_weight, max_iter, eps,
                                                     return_opt=True)
    W, counts, info = W[0], counts[0], info[0]
    eq = info[:, 0] == 4
    if bool(eq.any()):
        counts[eq] = ce[0][eq]
    shifted, counts_df = _series_out(pi, custom_feature, E.shift_rows(W)[0], counts)
    if return_info:
        return shifted, counts_df, {"info": info.cpu().numpy(), "books": W.cpu().numpy(), "opt": Wopt[0].cpu().numpy(),
                                    "dates": pi.dates, "symbols": pi.symbols}
    return shifted, counts_df


def mvo_trade_list(custom_feature: pd.Series, returns: pd.Series, pct: float = 0.1, max_weight: float = 0.03,
                   lookback_period: int = 60, shrinkage_intensity: float = 0.1, max_iter: int = 20000,
                   eps: float = 1e-9, return_info: bool = False):
    """``Simulation._daily_trade_list()`` for ``method='mvo'`` on the device: the same
    ``(shifted, counts_df)`` pair as ``daily_trade_list``.  Every date's QP is solved to its
    optimum (engine.sim_mvo_books); days without returns history carry the equal-weight book.
    With ``return_info`` a third value holds the solver's ``info`` [D][6], the same-day
    ``books`` [D][A] (NaN where the feature has no row) and their ``dates`` / ``symbols``."""
    custom_feature = by_date(custom_feature)
    pi, R0, win_rows, win_T, X, present = _mvo_inputs(custom_feature, returns, lookback_period, device())
    W, counts, info = E.sim_mvo_books(R0, win_rows, win_T, X[0], present, shrinkage_intensity, max_weight, max_iter, eps)
    eq = info[:, 0] == 4
    if bool(eq.any()):
        _, ce, we = E.trade_books(X, "equal", pct, max_weight, present=present, nan_absent=False, raw=True)
        W[eq] = we[0][eq]
        counts[eq] = ce[0][eq]
    shifted, counts_df = _series_out(pi, custom_feature, E.shift_rows(W)[0], counts)
    if return_info:
        return shifted, counts_df, {"info": info.cpu().numpy(), "books": W.cpu().numpy(), "dates": pi.dates,
                                    "symbols": pi.symbols}
    return shifted, counts_df


def risk_mvo_trade_list(custom_feature: pd.Series, model, pct: float = 0.1, max_weight: float = 0.03,
                        return_info: bool = False, max_iter: int = 20000, eps: float = 1e-9, neutral=None):
    """``mvo_trade_list`` against a fitted ``risk_model.FactorRiskModel`` instead of the returns
    window: every date's book minimises w'Sigma w under the model's Sigma of that date
    (engine.risk_mvo_books), with the constraints, statuses and the
    ``(shifted, counts_df[, extra])`` result of ``mvo_trade_list``.  A date the model does not
    have, or has as invalid, carries the equal-weight book (status 4).  The feature's symbols
    must be symbols of the model.

    ``neutral`` (default: ``model.neutral``, see ``FactorRiskModel.neutral_to``): names of model
    factors every solved book is also neutral to, B_k . w = 0.  A date on which the
    legs, the box and neutrality cannot hold together ends at ``max_iter`` with status 1 and its
    last iterate; one warning per call names such dates.  ``extra`` then also holds ``expo``
    [D][K], the exposures of the books to every factor, and ``neutral``, the names."""
    neutral = tuple(model.neutral if neutral is None else ((neutral,) if isinstance(neutral, str) else neutral))
    nidx = model.columns.get_indexer(list(neutral))
    if (nidx < 0).any():
        raise ValueError(f"risk_mvo_trade_list: {[n for n, k in zip(neutral, nidx) if k < 0]} are not factors "
                         f"of the risk model ({list(model.columns)})")
    custom_feature = by_date(custom_feature)
    dev = device()
    pi = panel_index(custom_feature.index)
    mp = model.panel_index
    scol = mp.symbols.get_indexer(pi.symbols)
    if (scol < 0).any():
        raise ValueError("risk_mvo_trade_list: the feature has symbols the risk model does not")
    cols = scol[pi.s]
    xh = np.full((pi.D, mp.A), np.nan)
    xh[pi.d, cols] = custom_feature.to_numpy(dtype=np.float64)
    ph = np.zeros((pi.D, mp.A), dtype=np.uint8)
    ph[pi.d, cols] = 1
    mrow = mp.dates.get_indexer(pi.dates).astype(np.int32)
    ok = model.valid.to_numpy()
    mrow[mrow >= 0] = np.where(ok[mrow[mrow >= 0]], mrow[mrow >= 0], -1)
    X, present = torch.as_tensor(xh, device=dev), torch.as_tensor(ph, device=dev)
    expo = None
    if len(neutral):
        W, counts, info, expo = E.risk_mvo_books(model.B, model.Fc, model.S2, X, present, mrow, max_weight, max_iter,
                                                 eps, neutral=nidx, return_expo=True)
        _warn_not_neutral(model, pi.dates, mrow, X, present, info, expo, nidx)
    else:
        W, counts, info = E.risk_mvo_books(model.B, model.Fc, model.S2, X, present, mrow, max_weight, max_iter, eps)
    eq = info[:, 0] == 4
    if bool(eq.any()):
        _, ce, we = E.trade_books(X[None], "equal", pct, max_weight, present=present, nan_absent=False, raw=True)
        W[eq] = we[0][eq]
        counts[eq] = ce[0][eq]
    Ws = E.shift_rows(W)[0].cpu().numpy()
    order = np.argsort(pi.flat)
    d, s = pi.d[order], pi.s[order]
    index = pd.MultiIndex.from_arrays([pi.dates[d], pi.symbols[s]], names=list(custom_feature.index.names))
    shifted = pd.Series(Ws[d, scol[s]], index=index)
    cn = counts.cpu().numpy()
    counts_df = pd.DataFrame({"long_count": cn[:, 0].astype(np.int64), "short_count": cn[:, 1].astype(np.int64)},
                             index=pd.Index(pi.dates, name=custom_feature.index.names[0]))
    if return_info:
        extra = {"info": info.cpu().numpy(), "books": W.cpu().numpy()[:, scol], "dates": pi.dates, "symbols": pi.symbols}
        if expo is not None:
            extra.update(expo=expo.cpu().numpy(), neutral=neutral)
        return shifted, counts_df, extra
    return shifted, counts_df


def _warn_not_neutral(model, dates, mrow, X, present, info, expo, nidx):
    """One warning naming the dates that ran to max_iter (status 1) with an exposure to a
    neutral factor k above 1e-8 max|B_k| (the maximum over the date's active cells)."""
    st1 = np.flatnonzero(info[:, 0].cpu().numpy() == 1)
    if not len(st1):
        return
    rows = torch.as_tensor(mrow[st1], dtype=torch.long, device=expo.device)
    k = torch.as_tensor(nidx, dtype=torch.long, device=expo.device)
    Bn = torch.nan_to_num(model.B[k][:, rows], nan=0.0, posinf=0.0, neginf=0.0)        # [n][dates][A]
    active = (present[st1] != 0) & ((X[st1] > 0) | (X[st1] < 0))
    bmax = (Bn.abs() * active).amax(dim=2).T                                            # [dates][n]
    off = (expo[st1][:, k].abs() > 1e-8 * bmax).any(dim=1).cpu().numpy()
    if off.any():
        names = ", ".join(str(pd.Timestamp(d).date()) if isinstance(d, np.datetime64) else str(d)
                          for d in np.asarray(dates)[st1[off]])
        logging.getLogger("simulation").warning(
            "risk_mvo_trade_list: %d date(s) reached max_iter without a book neutral to %s (the constraints may be "
            "infeasible there): %s", int(off.sum()), list(model.columns[nidx]), names)


# ----------------------------------------------------------------------------- routing
def risk_mvo_runs_natively(feature, model, use_cvxpy) -> bool:
    """'mvo' against a factor risk model runs on the device under ``mvo_runs_natively``'s
    conditions without the lookback and shrinkage caps (the model replaces the window), with
    at most 32 factors."""
    if not use_cvxpy or os.environ.get("FMX_SIM_MVO", "").lower() == "reference":
        return False
    if not torch.cuda.is_available() or not isinstance(feature, pd.Series):
        return False
    idx = feature.index
    if not isinstance(idx, pd.MultiIndex) or idx.nlevels != 2 or not idx.is_unique:
        return False
    if not 1 <= getattr(model, "K", 0) <= E.RISK_MAX_K:
        return False
    return model.panel_index.A <= E.SIM_MVO_MAX_A


def mvo_runs_natively(feature, returns, use_cvxpy, lookback_period, shrinkage_intensity) -> bool:
    """'mvo' solves every date's QP on the device unless the caller asked for the host SLSQP
    solver (``use_cvxpy=False``) or the reference (``FMX_SIM_MVO=reference``), no GPU is
    visible, or the inputs are outside the kernel's caps (more than 16,384 symbols, a lookback
    outside 1..64, a shrinkage intensity above 1) or not two unique (date, symbol) indexes.
    ``feature`` is one manager's Series or the managers' DataFrame, ``returns`` a Series."""
    if not use_cvxpy or os.environ.get("FMX_SIM_MVO", "").lower() == "reference":
        return False
    if not torch.cuda.is_available():
        return False
    if not (isinstance(feature, (pd.Series, pd.DataFrame)) and isinstance(returns, pd.Series)):
        return False
    for idx in (feature.index, returns.index):
        if not isinstance(idx, pd.MultiIndex) or idx.nlevels != 2 or not idx.is_unique:
            return False
    try:
        if not 1 <= int(lookback_period) <= E.SIM_MVO_MAX_T or not shrinkage_intensity <= 1.0:
            return False
    except (TypeError, ValueError):
        return False
    return feature.index.get_level_values(1).nunique() <= E.SIM_MVO_MAX_A


def mvo_turnover_runs_natively(feature, returns, use_cvxpy, lookback_period, shrinkage_intensity, turnover_penalty,
                               return_weight) -> bool:
    """'mvo_turnover' stays the reference's host loop unless ``FMX_SIM_MVO_TURNOVER=native`` is
    set; then it runs on the device under the conditions of ``mvo_runs_natively``, with a
    ``turnover_penalty`` >= 0 and a finite ``return_weight``."""
    if os.environ.get("FMX_SIM_MVO_TURNOVER", "").lower() != "native":
        return False
    try:
        tau, r = float(turnover_penalty), float(return_weight)
    except (TypeError, ValueError):
        return False
    if not (tau >= 0.0 and np.isfinite(tau) and np.isfinite(r)):
        return False
    return mvo_runs_natively(feature, returns, use_cvxpy, lookback_period, shrinkage_intensity)


# ----------------------------------------------------------------------------- all managers at once
MM_CHUNK_BYTES = 4 << 30      # device tensors of one chunk of managers in mvo_manager_books


def _manager_bytes(method, D, A, Lmax):
    """Device bytes one manager needs in ``mvo_manager_books``: X, W, the equal-weight pair and
    the shifted book ([D][A] doubles), the presence mask, the window tables and, for
    'mvo_turnover', the chain kernel's workspace slot per date."""
    per_date = A * (5 * 8 + 1) + 4 * (Lmax + 1) + 8 * 8
    if method == "mvo_turnover":
        per_date += 8 * (16 + Lmax * Lmax)
    return D * per_date


def mvo_manager_books(factors_df: pd.DataFrame, cols, returns: pd.Series, method: str, pct: float = 0.1,
                      max_weight: float = 0.03, lookback_period: int = 60, shrinkage_intensity: float = 0.1,
                      turnover_penalty: float = 0.1, return_weight: float = 0.0, max_iter: int = 20000,
                      eps: float = 1e-9, return_info: bool = False, chunk_bytes: int = None):
    """The books of the managers ``cols`` of ``compute_multimanager_weights`` for ``method``
    'mvo' or 'mvo_turnover': (Wf [F][D][A] per-symbol-shifted books, NaN = no row; cnt [F][D][2]
    counts, NaN = no book that date) on the device, on ``panel_index(factors_df.index)``'s grid.
    Manager f is ``Simulation._daily_trade_list`` over ``factors_df[cols[f]].dropna()``: a cell
    is a row of manager f when the frame has the row and the value is not NaN, and a date on
    which manager f has no row is not one of its dates (the turnover chain's previous book is
    the one of its last date with rows).  The returns panel goes up once; every (manager, date)
    gets its own window (``engine.sim_mvo_window_rows``); 'mvo' is one ``engine.sim_mvo_books``
    launch over the F * D rows, 'mvo_turnover' one chain per manager
    (``engine.sim_mvo_turnover_chains``); dates without returns history carry the batched
    equal-weight book.  Managers are processed in chunks of at most ``chunk_bytes`` (default
    ``MM_CHUNK_BYTES``) of device tensors; every manager is independent of the others, so the
    results do not depend on the chunking.  With ``return_info`` a third value holds ``info``
    [F][D][6] (status 5: not a date of the manager), the same-day ``books`` [F][D][A] and, for
    'mvo_turnover', the solver's ``opt`` [F][D][A], as numpy arrays."""
    if method not in ("mvo", "mvo_turnover"):
        raise NotImplementedError(f"method {method!r}: mvo_manager_books runs 'mvo' and 'mvo_turnover'")
    factors_df = by_date(factors_df)
    cols = list(cols)
    dev = device()
    pi = panel_index(factors_df.index)
    F, D, A = len(cols), pi.D, pi.A
    rdates, rd, rs, keep = _returns_grid(pi, returns)
    Dr = len(rdates)
    r0 = np.zeros((max(Dr, 1), A))
    rv = returns.to_numpy(dtype=np.float64, na_value=np.nan)[keep]
    r0[rd[keep], rs[keep]] = np.where(np.isnan(rv), 0.0, rv)                                  # fillna(0), :337
    rp = np.zeros((Dr, A), dtype=np.uint8)
    rp[rd[keep], rs[keep]] = 1
    R0, RP = torch.as_tensor(r0, device=dev), torch.as_tensor(rp, device=dev)
    nbefore = torch.as_tensor(np.searchsorted(rdates, np.asarray(pi.dates), side="left").astype(np.int32), device=dev)
    Lmax = max(1, min(int(lookback_period), Dr))
    budget = MM_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
    Fc = max(1, min(F, budget // max(1, _manager_bytes(method, D, A, Lmax))))
    Wf = torch.empty((F, D, A), dtype=torch.float64, device=dev)
    cnt = torch.empty((F, D, 2), dtype=torch.float64, device=dev)
    keep_info = {"info": [], "books": [], "opt": []}
    for f0 in range(0, F, Fc):
        X = pi.to_device(factors_df[cols[f0:f0 + Fc]].to_numpy(dtype=np.float64), dev)           # [n][D][A], NaN = no row
        n = X.shape[0]
        has_rows = (X == X).any(dim=2)                                                       # [n][D]
        pres = (X == X).to(torch.uint8)
        win_rows, win_T = E.sim_mvo_window_rows(pres.reshape(n * D, A), RP, nbefore.repeat(n), lookback_period)
        _, ce, we = E.trade_books(X, "equal", pct, max_weight, present=pi.present(dev), nan_absent=True, raw=True)
        if method == "mvo":
            W, counts, info = E.sim_mvo_books(R0, win_rows, win_T, X.reshape(n * D, A), pres.reshape(n * D, A),
                                              shrinkage_intensity, max_weight, max_iter, eps)
            W, counts, info = W.reshape(n, D, A), counts.reshape(n, D, 2), info.reshape(n, D, 6)
            Wopt = None
            eq = (info[:, :, 0] == 4) & has_rows
            W[eq] = we[eq]
            info[:, :, 0][~has_rows] = 5.0
        else:
            win_rows, win_T = win_rows.reshape(n, D, -1), win_T.reshape(n, D)
            W = torch.zeros_like(X)
            eq = (win_T == 0) & has_rows
            W[eq] = we[eq]
            out = E.sim_mvo_turnover_chains(R0, win_rows, win_T, X, pres, W, shrinkage_intensity, max_weight,
                                            turnover_penalty, return_weight, max_iter, eps, skip_absent=True,
                                            return_opt=return_info)
            W, counts, info = out[:3]
            Wopt = out[3] if return_info else None
            eq = info[:, :, 0] == 4
        counts[eq] = ce[eq]
        counts[~has_rows] = float("nan")
        Wf[f0:f0 + n] = E.shift_rows(W)
        cnt[f0:f0 + n] = counts
        if return_info:
            keep_info["info"].append(info.cpu().numpy())
            keep_info["books"].append(W.cpu().numpy())
            if Wopt is not None:
                keep_info["opt"].append(Wopt.cpu().numpy())
    if return_info:
        extra = {k: np.concatenate(v) for k, v in keep_info.items() if v}
        extra.update(dates=pi.dates, symbols=pi.symbols)
        return Wf, cnt, extra
    return Wf, cnt
