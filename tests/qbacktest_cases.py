"""Specification helpers of the quantile backtest (reference composite_factor.py:47-134),
plain pandas / numpy, written from the specification in DESIGN 15, not from the kernels.

* ``pandas_buckets``  the reference's inner expression (:63-89): the authority.
* ``pandas_labels``   its first step per date on a dense row: ``n - qcut label`` of
                      ``rank(method="first")``, 0 where pandas has NaN.
* ``model``           a dense-grid numpy model of the same rules (label panel, previous-row
                      pointer, per-bucket sums); test_qbacktest_host.py pins it to
                      ``pandas_buckets``.
* ``panel`` / ``label_panel``  the ragged / NaN / tied inputs the tests share.
"""
from __future__ import annotations

import math

import numpy as np
import pandas as pd


def pandas_buckets(feature: pd.Series, returns: pd.Series, n_groups: int) -> pd.DataFrame:
    lbl = feature.groupby(level="date").transform(
        lambda x: pd.qcut(x.rank(method="first"), n_groups, labels=False, duplicates="drop"))
    q = (n_groups - lbl).astype("Int64").groupby(level="symbol").shift(1)
    df = pd.DataFrame({"log_ret": returns, "group": q}).dropna(subset=["group", "log_ret"])
    g = df.reset_index().groupby(["date", "group"])["log_ret"].mean().unstack(level="group").sort_index()
    return g.reindex(columns=range(1, n_groups + 1))


def pandas_labels(row: np.ndarray, present, n_groups: int) -> np.ndarray:
    """Groups of one date: ``row`` [A] float64, ``present`` [A] bool or None.  The rows of the
    date are the present cells in column order (so 'first' ties go to the lower column)."""
    A = len(row)
    cols = np.arange(A) if present is None else np.flatnonzero(present)
    out = np.zeros(A, dtype=np.int64)
    if len(cols) == 0:
        return out
    x = pd.Series(row[cols])
    lbl = pd.qcut(x.rank(method="first"), n_groups, labels=False, duplicates="drop")
    lbl = np.asarray(lbl, dtype=np.float64)
    ok = ~np.isnan(lbl)
    out[cols[ok]] = n_groups - lbl[ok].astype(np.int64)
    return out


def qcut_counts(m: int, n_groups: int) -> np.ndarray:
    """Number of ranks 1..m with qcut label <= k, from pd.qcut itself."""
    lbl = pd.qcut(pd.Series(np.arange(1.0, m + 1)), n_groups, labels=False, duplicates="drop")
    lbl = np.asarray(lbl, dtype=np.float64)
    lbl = lbl[~np.isnan(lbl)].astype(np.int64)
    return np.cumsum(np.bincount(lbl, minlength=n_groups))


def model(feature: pd.Series, returns: pd.Series, n: int) -> pd.DataFrame:
    """Dense-grid numpy model of DESIGN 15's rules."""
    fd, fs = feature.index.get_level_values(0), feature.index.get_level_values(1)
    rd, rs = returns.index.get_level_values(0), returns.index.get_level_values(1)
    dates = pd.Index(np.unique(np.r_[fd.values, rd.values]))
    syms = pd.Index(np.unique(np.r_[np.asarray(fs, dtype=object), np.asarray(rs, dtype=object)]))
    D, A = len(dates), len(syms)

    def dense(s, d, a):
        o = np.full((D, A), np.nan)
        p = np.zeros((D, A), bool)
        di, ai = dates.get_indexer(d), syms.get_indexer(a)
        o[di, ai] = s.to_numpy(float)
        p[di, ai] = True
        return o, p
    X, PX = dense(feature, fd, fs)
    R, PR = dense(returns, rd, rs)
    lab = np.zeros((D, A), np.int64)                    # 0 = none, else group 1..n (1 = top)
    for d in range(D):
        v = ~np.isnan(X[d]) & PX[d]
        m = int(v.sum())
        if m < 2:
            continue
        idx = np.flatnonzero(v)
        rank = np.empty(m, np.int64)
        rank[np.argsort(X[d][idx], kind="stable")] = np.arange(1, m + 1)   # ties: lower column first
        lab[d, idx] = n - np.searchsorted(qcut_counts(m, n), rank, side="left")
    members = [[[] for _ in range(n)] for _ in range(D)]
    prev = np.full(A, -1)
    for d in range(D):
        for a in np.flatnonzero(PX[d]):
            g = lab[prev[a], a] if prev[a] >= 0 else 0
            prev[a] = d
            if g == 0 or not PR[d, a] or np.isnan(R[d, a]):
                continue
            members[d][g - 1].append(R[d, a])
    # the exactly rounded sum (math.fsum) over the count: two roundings
    out = np.array([[math.fsum(b) / len(b) if b else np.nan for b in row] for row in members]).reshape(D, n)
    keep = np.array([any(len(b) for b in row) for row in members], dtype=bool)
    return pd.DataFrame(out[keep], index=pd.Index(dates[keep], name="date"),
                        columns=pd.Index(np.arange(1, n + 1, dtype=np.int64), name="group"))


def members_mean_abs(feature: pd.Series, returns: pd.Series, n: int) -> pd.DataFrame:
    """mean |r| over the members of every kept (date, group): the scale of the value bound."""
    return pandas_buckets(feature, returns.abs(), n)


def panel(D, A, F, seed, drop=0.2, ties=True, nan_date=None, extra_ret_symbols=2, names=None):
    """Ragged factor frame (F columns) and returns on (date, symbol): NaN features and
    returns, rows dropped independently from the two indexes, ``extra_ret_symbols`` symbols
    only in the returns and the last feature symbol absent from the returns."""
    rng = np.random.default_rng(seed)
    dts = pd.bdate_range("2021-01-04", periods=D)
    sy = [f"S{i:04d}" for i in range(A)]
    idx = pd.MultiIndex.from_product([dts, sy], names=["date", "symbol"])
    x = rng.standard_normal((D * A, F))
    if ties:
        x[:, ::2] = np.round(x[:, ::2], 1)
    x[rng.random((D * A, F)) < 0.1] = np.nan
    df = pd.DataFrame(x, index=idx, columns=names or [f"f{k}" for k in range(F)])
    if nan_date is not None:
        df.loc[df.index.get_level_values(0) == dts[nan_date], :] = np.nan
    rsy = sy[:-1] + [f"T{i:04d}" for i in range(extra_ret_symbols)] if A > 2 else sy
    ridx = pd.MultiIndex.from_product([dts, rsy], names=["date", "symbol"])
    r = pd.Series(0.01 * rng.standard_normal(len(ridx)), index=ridx, name="log_ret")
    r[rng.random(len(ridx)) < 0.05] = np.nan
    if drop > 0:
        df = df[rng.random(D * A) >= drop]
        r = r[rng.random(len(ridx)) >= drop / 2]
    return df, r


def label_panel(A, seed, F=2):
    """[F][3][A] float64 and a ragged [3][A] presence mask.  Factor 0: a row rounded to one
    decimal (many ties), an all-equal row, an all-NaN row; factor 1: a row with +-inf cells
    and NaNs, a row with ONE valid cell, a random row."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((F, 3, A))
    X[0, 0] = np.round(X[0, 0], 1)
    X[0, 1] = 0.25
    X[0, 2] = np.nan
    if A >= 3:
        X[1, 0, rng.choice(A, max(1, A // 8), replace=False)] = np.inf
        X[1, 0, rng.choice(A, max(1, A // 8), replace=False)] = -np.inf
        X[1, 0, rng.choice(A, max(1, A // 10), replace=False)] = np.nan
    X[1, 1] = np.nan
    X[1, 1, A // 2] = 1.5
    present = rng.random((3, A)) >= 0.15
    present[1, A // 2] = True                            # the one valid cell of X[1, 1] is a row
    return X, present
