"""Oracle restatement of composite_factor.py (composite_factor_calculation,
weighted_composite_factor).  Test infrastructure only (see oracle/__init__.py).

``X[F][D][A]`` panel, factor ``names``.  ``present[D][A]`` (optional) marks the (date,
symbol) rows the long frame holds: every date is computed on its present rows alone, as the
reference's ``groupby('date')`` / ``factors_df.loc[date]`` sees them, so ``len(x)`` of the
rank formula and every row sum run over the compacted present rows.  ``present=None`` is
the dense panel.

The two entry points are compositions of the stage functions below, which the per-stage GPU
tests compare the kernels with:

  composite_factor_calculation = combine(normalise(proxies(adjusted(X))))
  weighted_composite_factor    = weighted_combine(weighted_normalise(weighted_proxies(
                                     X, weighted_percentiles(X))))
"""
from __future__ import annotations

import numpy as np

from . import numerics as nm

SUFFIX = {  # composite_factor.py:158-163 / :244-249
    "_eq": (10, 90), "_flx": (2, 98), "_long": (2, 98), "_short": (2, 98),
}


def _scale(suffix, s, lo, hi):
    with np.errstate(all="ignore"):
        if suffix == "_eq":
            return np.where(s <= lo, -1.0, np.where(s >= hi, 1.0, 0.0))
        c = np.clip(s, lo, hi)
        if suffix == "_flx":
            return ((c - lo) / (hi - lo)) * 2 - 1
        if suffix == "_long":
            return (c - lo) / (hi - lo)
        return (c - hi) / (hi - lo)


def _pct(clean, p):
    s = np.sort(clean)
    q = np.true_divide(np.asarray([p], dtype=np.float64), 100)[0]
    return nm.percentile_linear(s, q)


def _prefix_groups(names):
    groups = {}
    for k, n in enumerate(names):
        groups.setdefault(n.split("_", 1)[0], []).append(k)
    return groups


def _rowmean_skipna(M):
    """DataFrame.mean(axis=1) skipna over columns ``M[k][A]`` -> [A]."""
    return nm.nanmean(np.ascontiguousarray(M.T))


def _safe_z(v):
    mu = nm.nanmean(v[None, :])[0]
    sd = nm.nanstd(v[None, :], 0)[0]
    if sd == 0 or np.isnan(sd):
        return np.zeros_like(v)
    return (v - mu) / sd


def _rank01(v):
    """(scipy.stats.rankdata(x) - 1) / (len - 1); any NaN -> all NaN (scipy>=1.10)."""
    n = len(v)
    if np.isnan(v).any():
        return np.full(n, np.nan)
    with np.errstate(all="ignore"):
        return (nm.rank_1d(v, "average") - 1) / (n - 1)


def _rows(present, d, A):
    """Column indices of date d's present rows (all of them on a dense panel)."""
    return np.arange(A) if present is None else np.flatnonzero(np.asarray(present)[d])


# ------------------------------------------------------- composite_factor_calculation stages
def adjusted(X, names, selected, present=None):
    """:157-178, the suffix preprocessing per (selected column, date) with that column's own
    percentiles.  Returns ``adj[K][D][A]`` (NaN at absent cells)."""
    pos = [names.index(s) for s in selected]
    sel_names = [names[k] for k in pos]
    F, D, A = X.shape
    adj = np.full((len(pos), D, A), np.nan)
    for d in range(D):
        r = _rows(present, d, A)
        day = X[pos, d][:, r].copy()
        for suffix, (ql, qh) in SUFFIX.items():
            for j, n in enumerate(sel_names):
                if not n.endswith(suffix):
                    continue
                arr = day[j]
                clean = arr[~np.isnan(arr)]
                if clean.size == 0:
                    day[j] = 0.0
                    continue
                lo, hi = _pct(clean, ql), _pct(clean, qh)
                day[j] = 0.0 if hi == lo else _scale(suffix, arr, lo, hi)
        adj[:, d, r] = day
    return adj


def proxies(adj, sel_names, present=None):
    """:181-190, the skipna mean over each prefix group's columns.  ``[G][D][A]``, groups in
    order of first appearance, NaN at absent cells."""
    K, D, A = adj.shape
    groups = _prefix_groups(sel_names)
    prox = np.full((len(groups), D, A), np.nan)
    for d in range(D):
        r = _rows(present, d, A)
        for g, idx in enumerate(groups.values()):
            prox[g, d, r] = _rowmean_skipna(adj[idx, d][:, r])
    return prox


def normalise(prox, method, present=None):
    """:193-210, safe_zcol / the [0, 1] rank of every proxy per date over the present rows."""
    G, D, A = prox.shape
    fn = _safe_z if method == "zscore" else _rank01
    nrm = np.full((G, D, A), np.nan)
    for d in range(D):
        r = _rows(present, d, A)
        for g in range(G):
            nrm[g, d, r] = fn(prox[g, d, r])
    return nrm


def combine(nrm, mode, present=None):
    """:204 / :210 and :216: skipna mean (mode 0) or skipna sum (mode 1) over the normalised
    proxies, then the per-date demeaning.  ``[D][A]``, NaN at absent cells."""
    G, D, A = nrm.shape
    out = np.full((D, A), np.nan)
    for d in range(D):
        r = _rows(present, d, A)
        z = nrm[:, d][:, r]
        if mode == 0:
            comp = _rowmean_skipna(z)
        else:
            comp = nm.pairwise_sum(np.where(np.isnan(z), 0.0, z).T)   # skipna sum
        out[d, r] = comp - nm.nanmean(comp[None, :])[0]
    return out


def composite_factor_calculation(X, names, selected, method="zscore", present=None):
    """composite_factor.py:137-218.  Returns [D][A] (NaN at absent cells)."""
    if method not in ("zscore", "rank"):
        raise ValueError("method must be 'zscore' or 'rank'")
    sel_names = [names[names.index(s)] for s in selected]
    adj = adjusted(X, names, selected, present)
    prox = proxies(adj, sel_names, present)
    nrm = normalise(prox, method, present)
    return combine(nrm, 0 if method == "zscore" else 1, present)


# ---------------------------------------------------------- weighted_composite_factor stages
def weighted_rows(names, sel_dates_idx, W):
    """Per selection row i: ``None`` when it yields nothing (date not in the panel or no
    positive weight: NaN -> fillna(0)), else ``(d, today, groups, gw)``: the panel date, the
    selected column indices (w > 0, column order), the prefix groups as lists of positions
    into ``today`` (first appearance order) and the normalised group weights (:307-319)."""
    F = len(names)
    rows = []
    for i, d in enumerate(sel_dates_idx):
        wrow = W[i]
        today = [k for k in range(F) if wrow[k] > 0]
        if d < 0 or not today:
            rows.append(None)
            continue
        groups = list(_prefix_groups([names[k] for k in today]).values())
        gw = [sum(wrow[today[j]] for j in idx) for idx in groups]      # Python sum
        gws = sum(gw)
        if gws > 0:
            gw = [g / gws for g in gw]
        else:
            gw = [1 / len(gw)] * len(gw)
        rows.append((d, today, groups, gw))
    return rows


def weighted_percentiles(X, names, sel_dates_idx, W, present=None):
    """:251-268, the percentiles pooled over a selection row's columns that share a suffix.
    ``lohi[J][4][3]`` = (lo, hi, nv) per (row, suffix in SUFFIX order); nv is the number of
    pooled non-NaN values, -1 (lo = hi = NaN) when the row has no column of that suffix,
    0 (lo = hi = NaN) when all its values are NaN."""
    F, D, A = X.shape
    rows = weighted_rows(names, sel_dates_idx, W)
    lohi = np.full((len(rows), 4, 3), np.nan)
    lohi[:, :, 2] = -1.0
    for i, row in enumerate(rows):
        if row is None:
            continue
        d, today, _, _ = row
        r = _rows(present, d, A)
        for s, (suffix, (ql, qh)) in enumerate(SUFFIX.items()):
            cols = [k for k in today if names[k].endswith(suffix)]
            if not cols:
                continue
            vals = X[cols, d][:, r]
            clean = vals[~np.isnan(vals)]
            lohi[i, s, 2] = clean.size
            if clean.size:
                lohi[i, s, 0], lohi[i, s, 1] = _pct(clean, ql), _pct(clean, qh)
    return lohi


def weighted_proxies(X, names, sel_dates_idx, W, lohi, present=None):
    """:251-300, suffix scaling with the pooled ``lohi`` and the skipna group means.
    ``[G][J][A]`` with G the largest group count of a row; NaN for a group the row does not
    have, for a row that yields nothing and at absent cells."""
    F, D, A = X.shape
    rows = weighted_rows(names, sel_dates_idx, W)
    G = max([1] + [len(row[2]) for row in rows if row is not None])
    prox = np.full((G, len(rows), A), np.nan)
    for i, row in enumerate(rows):
        if row is None:
            continue
        d, today, groups, _ = row
        r = _rows(present, d, A)
        adj = X[today, d][:, r].copy()                         # [k][present rows]
        for s, suffix in enumerate(SUFFIX):
            cols = [j for j, k in enumerate(today) if names[k].endswith(suffix)]
            if not cols:
                continue
            lo, hi, nv = lohi[i, s]
            if nv == 0 or lo == hi:
                adj[cols] = 0.0
            else:
                for j in cols:
                    adj[j] = _scale(suffix, adj[j], lo, hi)
        for g, idx in enumerate(groups):
            prox[g, i, r] = _rowmean_skipna(adj[idx])
    return prox


def weighted_normalise(prox, sel_dates_idx, method, present=None):
    """:321-327, safe_z / safe_rank of every proxy of a selection row over the present rows
    of its date."""
    G, J, A = prox.shape
    fn = _safe_z if method == "zscore" else _rank01
    nrm = np.full((G, J, A), np.nan)
    for i, d in enumerate(sel_dates_idx):
        if d < 0:
            continue
        r = _rows(present, d, A)
        for g in range(G):
            nrm[g, i, r] = fn(prox[g, i, r])
    return nrm


def weighted_combine(nrm, names, sel_dates_idx, W, D, present=None, fillna=True):
    """:329-341, the weighted Python sum of a row's normalised proxies (NaN propagates), the
    demeaning and the final reindex().fillna(0).  ``[D][A]``, 0 at every cell no selection
    row writes.  ``fillna=False`` leaves out the last step: NaN at every cell the reference
    fills with 0 (a NaN composite, a date no row yields anything for, an absent row)."""
    G, J, A = nrm.shape
    out = np.full((D, A), np.nan)
    for i, row in enumerate(weighted_rows(names, sel_dates_idx, W)):
        if row is None:
            continue
        d, _, groups, gw = row
        r = _rows(present, d, A)
        comp = 0
        for g in range(len(groups)):                          # Python sum(): NaN propagates
            comp = comp + nrm[g, i, r] * gw[g]
        comp = comp - nm.nanmean(np.asarray(comp)[None, :])[0]
        out[d, r] = comp
    return np.where(np.isnan(out), 0.0, out) if fillna else out


def weighted_composite_factor(X, names, sel_dates_idx, W, method="zscore", present=None, fillna=True):
    """composite_factor.py:220-342.  ``sel_dates_idx[i]`` is the panel date index of
    selection row i (or -1 when the date is not in the panel).  Returns [D][A] with
    non-selected dates and absent cells 0 (the final reindex().fillna(0); ``fillna=False``
    keeps them NaN, see weighted_combine)."""
    if method not in ("zscore", "rank"):
        raise ValueError("method must be 'zscore' or 'rank'")
    F, D, A = X.shape
    lohi = weighted_percentiles(X, names, sel_dates_idx, W, present)
    prox = weighted_proxies(X, names, sel_dates_idx, W, lohi, present)
    nrm = weighted_normalise(prox, sel_dates_idx, method, present)
    return weighted_combine(nrm, names, sel_dates_idx, W, D, present, fillna)
