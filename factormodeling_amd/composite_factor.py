"""Drop-in replacement for the reference's ``composite_factor.py``.

``composite_factor_calculation`` (composite_factor.py:137-218) and
``weighted_composite_factor`` (:220-342) keep their signatures and outputs (Series named
``composite_factor`` on ``factors_df.index``); the per-date percentiles, suffix scaling,
prefix-group proxies, z-score / rank normalisation, weighting and demeaning run in the
gfx950 kernels of ``csrc/composite.hip`` and ``csrc/cs_ops.hip``.  The two plotting helpers
the notebook imports (pipeline.ipynb:55) draw with host-side matplotlib, as in the
reference.

``quantile_backtest_log`` returns the numbers ``plot_quantile_backtests_log`` (:47-134)
draws: per factor column, the mean return of every per-date quantile bucket, the buckets
lagged one row per symbol.  The reference computes them with one ``pd.qcut`` call per date
(:63-98); here the bucket labels (``fmx_cs_qlabel``: ordinal ranks and the qcut label from a
host table of pandas' own cut points) and the bucket means (``fmx_qbucket_mean``: exact
sums) run in ``csrc/qbacktest.hip`` on the union grid of the two indexes, the factor
columns uploaded in chunks of at most ``QBACKTEST_DEVICE_BUDGET`` bytes.  Inputs the
kernels do not take (more than 32 groups or 8,192 symbols, rows of a date not in sorted
symbol order, no GPU) keep the reference's pandas loop, ``_quantile_backtest_host``.
"""
from __future__ import annotations

import math

import numpy as np
import pandas as pd
import torch

from . import engine
from .panel import device, panel_index
from .profiling import phase


def _prefix_groups(names):
    groups = {}
    for k, n in enumerate(names):
        groups.setdefault(n.split("_", 1)[0], []).append(k)
    return groups


def composite_factor_calculation(factors_df: pd.DataFrame, selected_factors: list, method: str = "zscore"):
    """composite_factor.py:137-218"""
    if method not in ("zscore", "rank"):
        raise ValueError("method must be 'zscore' or 'rank'")
    pos = list(selected_factors)
    P = panel_index(factors_df.index)
    dev = device()
    X = P.to_device(factors_df[pos].to_numpy(dtype=np.float64, na_value=np.nan), dev)
    pres = P.present(dev)
    Adj = engine.comp_adj(X, list(range(len(pos))), [engine.suffix_code(n) for n in pos])
    if pres is not None:
        Adj.masked_fill_(pres.unsqueeze(0) == 0, float("nan"))
    groups = list(_prefix_groups(pos).values())
    Prox = engine.comp_proxy(Adj, groups)
    if method == "zscore":
        Nrm = engine.cs_moment("market_neutralize", Prox, pres)   # safe_zcol == market_neutralize
        comp = engine.comp_combine(Nrm, 0, pres)
    else:
        Nrm = engine.cs_rank(Prox, "scipy_average", pres)
        comp = engine.comp_combine(Nrm, 1, pres)
    vals = P.from_device(comp.unsqueeze(0))[:, 0]
    return pd.Series(vals, index=factors_df.index, name="composite_factor")


def weighted_plan(pdate, W, names):
    """Per selection row j (panel date index pdate[j], -1 = not a panel date; weights
    W[j] over ``names`` in selection_df column order): the selected columns (w > 0, column
    order), their suffix codes, prefix groups numbered by first appearance among them,
    the group weights (composite_factor.py:276-290: sums in column order, normalised, or
    equal when all zero) and the pooled suffix column lists (:251-268)."""
    W = np.asarray(W, dtype=np.float64)
    J, F = W.shape
    suffix = np.array([engine.suffix_code(n) for n in names], dtype=np.int32)
    _, pid = np.unique(np.array([n.split("_", 1)[0] for n in names], dtype=object).astype(str),
                       return_inverse=True)
    P = int(pid.max()) + 1 if F else 1
    sel = W > 0
    KMAX = int(max(1, sel.sum(axis=1).max() if J else 1))
    sel &= (np.asarray(pdate) >= 0)[:, None]
    col = np.zeros((J, KMAX), np.int32)
    suf = np.zeros((J, KMAX), np.int32)
    grp = np.full((J, KMAX), -1, np.int32)
    gwa = np.zeros((J, KMAX), np.float64)
    ncol = sel.sum(axis=1).astype(np.int32)
    pd_out = np.where(ncol > 0, np.asarray(pdate), -1).astype(np.int32)
    # selected entries in row-major order = each row's columns in column order
    jj, cc = np.nonzero(sel)
    kk = np.arange(jj.size) - np.concatenate([[0], np.cumsum(ncol)])[jj]
    col[jj, kk] = cc
    suf[jj, kk] = suffix[cc]
    # prefix groups numbered by first appearance within the row
    key = jj.astype(np.int64) * P + pid[cc]
    uk, first, inv = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")           # unique groups in (row, first position) order
    urow = (uk // P)[order]
    starts = np.flatnonzero(np.r_[True, urow[1:] != urow[:-1]]) if urow.size else np.zeros(0, np.int64)
    run = np.repeat(starts, np.diff(np.r_[starts, urow.size]))
    gnum = np.empty(uk.size, np.int64)
    gnum[order] = np.arange(urow.size) - run
    grp[jj, kk] = gnum[inv]
    ngrp = np.bincount(uk // P, minlength=J).astype(np.int32) if uk.size else np.zeros(J, np.int32)
    # group sums (composite_factor.py:281: pandas Series.sum = numpy sum over the members in
    # column order: sequential from 0 below 8 members, numpy's pairwise sum from 8)
    vals = W[jj, cc]
    gsum = np.zeros(uk.size)
    np.add.at(gsum, inv, vals)
    big = np.flatnonzero(np.bincount(inv, minlength=uk.size) >= 8)
    for u in big:
        gsum[u] = vals[inv == u].sum()
    tot = np.zeros(J)                                   # Python sum over groups in order (:282)
    np.add.at(tot, urow, gsum[order])
    r = uk // P
    gw = np.where(tot[r] > 0, gsum / np.where(tot[r] > 0, tot[r], 1.0), 1.0 / np.maximum(ngrp[r], 1))
    gwa[r, gnum] = gw
    # pooled suffix column lists per (row, suffix 1..4), columns in column order (:251-268)
    sc = suffix[cc]
    m = (sc >= 1) & (sc <= 4)
    idx = np.flatnonzero(m)
    idx = idx[np.lexsort((kk[idx], sc[idx], jj[idx]))]
    scol = cc[idx].astype(np.int32)
    cnt = np.bincount(jj[m] * 4 + (sc[m] - 1), minlength=4 * J) if J else np.zeros(0, np.int64)
    soff = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    return {"pdate": pd_out, "ncol": ncol, "col": col, "suf": suf, "grp": grp, "ngrp": ngrp, "gw": gwa,
            "KMAX": KMAX, "soff": soff, "scol": scol if scol.size else np.zeros(1, np.int32)}


def _weighted_plan(P, selection_df: pd.DataFrame, used: list):
    """weighted_plan for a selection DataFrame restricted to the ``used`` columns."""
    pdate = P.dates.get_indexer(selection_df.index) if len(P.dates) else np.full(len(selection_df), -1)
    W = selection_df[used].to_numpy(dtype=np.float64) if used else np.zeros((len(selection_df), 0))
    return weighted_plan(pdate, W, used)


def weighted_composite_factor(factors_df: pd.DataFrame, selection_df: pd.DataFrame, method: str = "zscore") -> pd.Series:
    """composite_factor.py:220-342"""
    if method not in ("zscore", "rank"):
        raise ValueError("method must be 'zscore' or 'rank'")
    if len(selection_df) == 0:
        raise ValueError("No objects to concatenate")
    used = [c for c in selection_df.columns if (selection_df[c] > 0).any()]
    P = panel_index(factors_df.index)
    dev = device()
    if used:
        with phase("pandas->dense"):
            xv = factors_df[used].to_numpy(dtype=np.float64, na_value=np.nan)
        X = P.to_device(xv, dev)
    else:
        X = torch.zeros((1, P.D, P.A), dtype=torch.float64, device=dev)
    with phase("host plan"):
        plan = _weighted_plan(P, selection_df, used)
    out = engine.wcomp(X, plan, method, P.present(dev))
    vals = P.from_device(out.unsqueeze(0))[:, 0]
    return pd.Series(vals, index=factors_df.index, name="composite_factor")


# ----------------------------------------------------------------------------- plotting (host)
def plot_factor_distributions(factors_df: pd.DataFrame, exclude: list = None, bins: int = 50, ncols: int = 3,
                              figsize: tuple = (15, 5)):
    """composite_factor.py:17-44 -- histogram grid of factor columns (host matplotlib)."""
    import matplotlib.pyplot as plt
    exclude = exclude or []
    cols = [c for c in factors_df.columns if c not in exclude]
    nrows = max(1, math.ceil(len(cols) / ncols))
    fig, axes = plt.subplots(nrows, ncols, figsize=(figsize[0], figsize[1] * nrows), squeeze=False)
    flat = axes.ravel()
    for ax, c in zip(flat, cols):
        ax.hist(factors_df[c].dropna(), bins=bins, density=True, alpha=0.7)
        ax.set_title(c)
        ax.set_xlabel("Value")
        ax.set_ylabel("Density")
    for ax in flat[len(cols):]:
        ax.axis("off")
    plt.tight_layout()
    plt.show()


# ----------------------------------------------------------------------------- quantile backtest
# Device bytes one chunk of factor columns may take in quantile_backtest_log.  Per cell: the
# fp64 panel (8), on a ragged grid the uploaded rows it is scattered from, alive with it (up to
# 8), the valid-cell mask of the count pass (1) and the label byte (1).  The per-row counts and
# the [F][D][n] means are not per cell and are left out.
QBACKTEST_DEVICE_BUDGET = 1 << 30
_QB_CELL_BYTES = 18


def _quantile_backtest_host(feature: pd.Series, returns: pd.Series, n_groups: int) -> pd.DataFrame:
    """composite_factor.py:63-98, restated: one ``pd.qcut`` call per date on the host."""
    lbl = feature.groupby(level="date").transform(
        lambda x: pd.qcut(x.rank(method="first"), n_groups, labels=False, duplicates="drop"))
    q = (n_groups - lbl).astype("Int64").groupby(level="symbol").shift(1)
    df = pd.DataFrame({"log_ret": returns, "group": q}).dropna(subset=["group", "log_ret"])
    g = df.reset_index().groupby(["date", "group"])["log_ret"].mean().unstack(level="group").sort_index()
    return g.reindex(columns=range(1, n_groups + 1))


class _QbPlan:
    """The union (date, symbol) grid of the factor frame's and the returns' indexes (what the
    reference's outer join aligns on; portfolio_simulation._Grid does the same), the feature
    rows' cells on it, the previous-row table and the dense returns panel."""

    def __init__(self, findex: pd.MultiIndex, returns: pd.Series):
        rindex = returns.index
        fd, fs = findex.get_level_values(0), findex.get_level_values(1)
        rd, rs = rindex.get_level_values(0), rindex.get_level_values(1)
        self.dates = fd.unique().union(rd.unique()).sort_values()
        self.symbols = fs.unique().union(rs.unique()).sort_values()
        self.D, self.A = len(self.dates), len(self.symbols)
        D, A = self.D, self.A
        self.flat = self.dates.get_indexer(fd).astype(np.int64) * A + self.symbols.get_indexer(fs)
        self.dense = len(findex) == D * A and bool(np.all(self.flat == np.arange(D * A)))
        self.present = self.prev_row = None
        if not self.dense:
            pres = np.zeros(D * A, dtype=bool)
            pres[self.flat] = True
            pres = pres.reshape(D, A)
            # previous feature row of the symbol: its rows are in date order (PanelIndex), so
            # the previous row in index order is the latest earlier date on which it has one
            at = np.where(pres, np.arange(D, dtype=np.int32)[:, None], np.int32(-1))
            last = np.maximum.accumulate(at, axis=0)
            prev = np.vstack([np.full((1, A), -1, np.int32), last[:-1]]) if D else at
            prev[~pres] = -1
            self.present = pres.astype(np.uint8)
            self.prev_row = np.ascontiguousarray(prev, dtype=np.int32)
        R = np.full(D * A, np.nan)
        R[self.dates.get_indexer(rd).astype(np.int64) * A + self.symbols.get_indexer(rs)] = \
            returns.to_numpy(dtype=np.float64, na_value=np.nan)
        self.R = R.reshape(D, A)


def _qb_device_reason(com_factors_df, returns, n_groups):
    """None when the device path can take the input, else why not."""
    if not (isinstance(n_groups, (int, np.integer)) and 2 <= n_groups <= engine.QLABEL_MAX_GROUPS):
        return f"n_groups must be an integer in [2, {engine.QLABEL_MAX_GROUPS}]"
    if not isinstance(returns, pd.Series):
        return "returns must be a Series"
    for name, idx in (("com_factors_df", com_factors_df.index), ("returns", returns.index)):
        if not isinstance(idx, pd.MultiIndex) or idx.nlevels != 2 or list(idx.names) != ["date", "symbol"]:
            return f"{name} needs a two-level (date, symbol) MultiIndex"
        if not idx.is_unique:
            return f"{name} has duplicate (date, symbol) rows"
    if com_factors_df.columns.has_duplicates:
        return "duplicate factor columns"
    with np.errstate(invalid="ignore"):
        if (np.abs(returns.to_numpy(dtype=np.float64, na_value=np.nan)) >= 2.0 ** 79).any():
            return "infinite (or >= 2^79) returns do not fit the exact fixed-point sums"
    try:
        P = panel_index(com_factors_df.index)
    except ValueError as e:
        return str(e)
    if not P.row_layout()[2]:
        return "the rows of a date are not in sorted-symbol order (rank 'first' ties go by row order)"
    try:
        nsym = len(com_factors_df.index.get_level_values(1).unique().union(returns.index.get_level_values(1).unique()))
    except TypeError as e:
        return f"symbols of the two indexes do not sort together: {e}"
    if nsym > engine.QLABEL_MAX_A:
        return f"{nsym} symbols exceed the label kernel's {engine.QLABEL_MAX_A}-asset rows"
    return None


def _quantile_backtest_device(com_factors_df, returns, n_groups):
    n = int(n_groups)
    cols = list(com_factors_df.columns)
    dev = device()
    with phase("host plan"):
        plan = _QbPlan(com_factors_df.index, returns)
    D, A = plan.D, plan.A
    Rd = torch.as_tensor(plan.R, device=dev)
    prev = torch.as_tensor(plan.prev_row, device=dev) if plan.prev_row is not None else None
    pres = torch.as_tensor(plan.present, device=dev) if plan.present is not None else None
    flat = torch.as_tensor(plan.flat, device=dev) if not plan.dense else None
    step = max(1, int(QBACKTEST_DEVICE_BUDGET // max(1, _QB_CELL_BYTES * D * A)))
    means, counts = [], []
    for c0 in range(0, len(cols), step):
        with phase("pandas->dense"):
            v = com_factors_df.iloc[:, c0:c0 + step].to_numpy(dtype=np.float64, na_value=np.nan)
            host = np.ascontiguousarray(v.T)
        with phase("H2D"):
            t = torch.as_tensor(host, device=dev)
        if plan.dense:
            X = t.reshape(-1, D, A)
        else:
            X = torch.full((t.shape[0], D * A), float("nan"), dtype=torch.float64, device=dev)
            X[:, flat] = t
            X = X.reshape(-1, D, A)
        labels = engine.cs_qlabel(X, n, pres)
        del X, t
        m, c = engine.qbucket_mean(labels, Rd, n, prev_row=prev)
        del labels
        means.append(m)
        counts.append(c)
    if not cols:
        return {}
    with phase("D2H"):
        mean = torch.cat(means).cpu().numpy()
        count = torch.cat(counts).cpu().numpy()
    columns = pd.Index(np.arange(1, n + 1, dtype=np.int64), name="group")
    out = {}
    for k, col in enumerate(cols):
        keep = count[k].sum(axis=1) > 0
        out[col] = pd.DataFrame(mean[k][keep], index=plan.dates[keep].rename("date"), columns=columns)
    return out


def quantile_backtest_log(com_factors_df: pd.DataFrame, returns: pd.Series, n_groups: int = 5,
                          backend: str = "auto") -> dict:
    """The numbers behind ``plot_quantile_backtests_log``: for every column of
    ``com_factors_df`` the frame the reference's inner ``quantile_backtest_log``
    (composite_factor.py:63-98) computes -- index the sorted dates that have a kept cell
    (named ``date``), columns the groups 1..n_groups (int64, named ``group``, 1 = top),
    values the mean log return of the group, NaN for an empty one.

    ``backend``: ``"host"`` is the reference's pandas loop; ``"device"`` the gfx950 kernels of
    ``csrc/qbacktest.hip`` (raises when they cannot take the input); ``"auto"`` the device
    when a GPU is visible, 2 <= n_groups <= 32, both indexes are unique two-level
    (date, symbol) MultiIndexes, every date's rows are in sorted-symbol order and the union
    grid has at most 8,192 symbols -- otherwise the host loop."""
    if backend not in ("auto", "host", "device"):
        raise ValueError("backend must be 'auto', 'host' or 'device'")
    if backend != "host":
        reason = _qb_device_reason(com_factors_df, returns, n_groups)
        if backend == "device":
            if reason is not None:
                raise ValueError(f"quantile_backtest_log: the device path cannot take this input: {reason}")
            return _quantile_backtest_device(com_factors_df, returns, n_groups)
        if reason is None and torch.cuda.is_available():
            return _quantile_backtest_device(com_factors_df, returns, n_groups)
    return {c: _quantile_backtest_host(com_factors_df[c], returns, n_groups) for c in com_factors_df.columns}


def plot_quantile_backtests_log(com_factors_df: pd.DataFrame, returns: pd.Series, n_groups: int = 5, ncols: int = 2,
                                figsize: tuple = (20, 6)):
    """composite_factor.py:47-134 -- per-date quantile buckets (1 = top), lagged one row
    per symbol, mean log return per bucket, cumulative P&L and the L1-S{n} spread.  The
    bucket means of all columns come from one ``quantile_backtest_log`` call."""
    import matplotlib.pyplot as plt

    frames = quantile_backtest_log(com_factors_df, returns, n_groups, backend="auto")
    facs = list(com_factors_df.columns)
    nrows = max(1, math.ceil(len(facs) / ncols))
    fig, axes = plt.subplots(nrows, ncols, figsize=(figsize[0], figsize[1] * nrows), squeeze=False)
    for i, fac in enumerate(facs):
        ax = axes[i // ncols][i % ncols]
        g = frames[fac]
        cum = np.expm1(g.cumsum())
        cum[f"DN_L1-S{n_groups}"] = np.expm1((g[1] - g[n_groups]).cumsum())
        for line in cum.columns:
            if str(line).startswith("DN_L1-S"):
                ax.plot(cum.index, cum[line], label=line, color="black", linewidth=2)
            else:
                ax.plot(cum.index, cum[line], label=line)
        ax.set_title(fac)
        ax.set_xlabel("Date")
        ax.set_ylabel("Cumulative Return")
        ax.legend(loc="upper left", fontsize="small")
        ax.grid(True)
    for k in range(len(facs), nrows * ncols):
        fig.delaxes(axes[k // ncols][k % ncols])
    plt.tight_layout()
    plt.show()
