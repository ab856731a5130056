"""Shared by the rolling order-statistic tests (host and GPU): the brute-force numpy reference
of ts_min / ts_max / ts_argmin / ts_argmax / ts_median / ts_quantile and the seeded case
panels.  No GPU needed, no fixture file.

The reference sorts every window (``sliding_window_view`` + ``np.sort``) and applies the
formulas of DESIGN §21; tests/test_ts_order_host.py pins it to pandas bit for bit, and the GPU
tests compare the kernels with it.  A panel is ``x [F][D][A]`` float64 and ``present [D][A]``
bool or None; a ragged column's window is its last W PRESENT rows, so the reference compacts
each column's present rows, runs the dense reference on them and scatters the result back.
Absent cells are NaN.
"""
from __future__ import annotations

import numpy as np
import pandas as pd
from numpy.lib.stride_tricks import sliding_window_view

OPS = ("min", "max", "argmin", "argmax", "median", "quantile")
EXTREMES = ("min", "max", "argmin", "argmax")
INTERPOLATIONS = ("linear", "lower", "higher", "midpoint", "nearest")
QS = (0.0, 0.1, 0.5, 0.99, 1.0)

# engine.ts_order's LDS-capacity switch: W 16-bit ranks x 64 lanes in 160 KiB (ts_order.hip
# TSO_LDS_MAXW); longer windows run the stateless bisection kernel
LDS_MAX_W = 1280


def _quantile_sorted(v, W, q, interpolation):
    """v [..., W] sorted windows -> pandas' roll_quantile value."""
    f = q * (W - 1)
    i = int(f)
    if f == i:
        return v[..., i]
    lo, hi = v[..., i], v[..., i + 1]
    if interpolation == "linear":
        return lo + (hi - lo) * (f - i)
    if interpolation == "lower":
        return lo
    if interpolation == "higher":
        return hi
    if interpolation == "midpoint":
        return (lo + hi) / 2
    if interpolation == "nearest":                      # round half to even
        g = f - i
        if g == 0.5:
            return lo if i % 2 == 0 else hi
        return lo if g < 0.5 else hi
    raise ValueError(interpolation)


def ref_dense(x, op, W, q=0.5, interpolation="linear"):
    """x [N][C] (every row present) -> [N][C]; NaN where the window is short or holds a NaN."""
    N = x.shape[0]
    out = np.full(x.shape, np.nan)
    if W > N:
        return out
    win = sliding_window_view(x, W, axis=0)             # [N - W + 1][C][W], oldest first
    bad = np.isnan(win).any(axis=-1)
    with np.errstate(invalid="ignore"):
        if op == "min":
            r = win.min(axis=-1)
        elif op == "max":
            r = win.max(axis=-1)
        elif op == "argmin":                            # first hit of the reversed window = most recent
            r = np.argmin(win[..., ::-1], axis=-1).astype(np.float64)
        elif op == "argmax":
            r = np.argmax(win[..., ::-1], axis=-1).astype(np.float64)
        else:
            v = np.sort(win, axis=-1)
            if op == "median":
                r = v[..., W // 2] if W % 2 else (v[..., W // 2] + v[..., W // 2 - 1]) / 2
            elif op == "quantile":
                r = _quantile_sorted(v, W, q, interpolation)
            else:
                raise ValueError(op)
    out[W - 1:] = np.where(bad, np.nan, r)
    return out


def ref_panel(x, present, op, W, q=0.5, interpolation="linear"):
    """x [F][D][A], present [D][A] bool or None -> [F][D][A]."""
    F, D, A = x.shape
    if present is None:
        return np.stack([ref_dense(x[f], op, W, q, interpolation) for f in range(F)])
    out = np.full(x.shape, np.nan)
    for a in range(A):
        rows = np.flatnonzero(present[:, a])
        if rows.size:
            out[:, rows, a] = ref_dense(x[:, rows, a].T, op, W, q, interpolation).T
    return out


def has_finite(ref):
    return bool(np.isfinite(ref).any())


# ------------------------------------------------------------------------------------ panels
def make_values(F, D, A, seed, nan_frac=0.02):
    """Tie-heavy values (rounded to quarters) with ~2 % NaN."""
    rng = np.random.default_rng(seed)
    x = np.round(rng.standard_normal((F, D, A)) * 4) / 4
    x[rng.random((F, D, A)) < nan_frac] = np.nan
    return x


def make_present(D, A, seed, short_rows=2):
    """Ragged mask: a third of the symbols list late, 10 % of all cells are gaps, every fourth
    symbol keeps all its rows (so a window of D rows exists), and the last symbol has only
    ``short_rows`` rows (fewer than any window > short_rows)."""
    rng = np.random.default_rng(seed + 1000)
    p = rng.random((D, A)) >= 0.10
    late = rng.random(A) < 1 / 3
    start = np.where(late, rng.integers(1, max(2, D // 2 + 1), A), 0)
    p &= np.arange(D)[:, None] >= start[None, :]
    p[:, ::4] = True                                    # every fourth symbol has all D rows
    p[:, A - 1] = False
    p[np.linspace(0, D - 1, min(short_rows, D)).astype(int), A - 1] = True
    return p


def make_panel(F, D, A, seed, ragged):
    x = make_values(F, D, A, seed)
    present = make_present(D, A, seed) if ragged else None
    return x, present


def content_panel(with_inf):
    """[1][40][8]: a constant column, a strictly increasing and a strictly decreasing one, a
    column with one NaN that enters and leaves every window, plain noise; with_inf adds +inf /
    -inf cells and an all-+inf stretch (the four extremes only)."""
    D = 40
    rng = np.random.default_rng(77)
    x = np.round(rng.standard_normal((1, D, 8)) * 4) / 4
    x[0, :, 0] = 1.25
    x[0, :, 1] = np.arange(D) * 0.5 - 3.0
    x[0, :, 2] = 7.0 - np.arange(D) * 0.25
    x[0, 17, 3] = np.nan
    x[0, :, 4] = np.where(np.arange(D) % 2 == 0, 0.0, -0.0)     # the two zeros tie
    if with_inf:
        x[0, 5, 5] = np.inf
        x[0, 21, 5] = -np.inf
        x[0, 10:20, 6] = np.inf
        x[0, 25:33, 7] = -np.inf
    return x


# ------------------------------------------------------------------------------------ pandas
def panel_index(D, A, present):
    dates = pd.bdate_range("2020-01-01", periods=D)
    syms = [f"S{a:04d}" for a in range(A)]
    idx = pd.MultiIndex.from_product([dates, syms], names=["date", "symbol"])
    if present is not None:
        idx = idx[present.reshape(-1)]
    return idx


def to_series(x2, present, name="x"):
    """x2 [D][A] -> (date, symbol) Series holding the present cells."""
    D, A = x2.shape
    v = x2.reshape(-1)
    if present is not None:
        v = v[present.reshape(-1)]
    return pd.Series(v, index=panel_index(D, A, present), name=name)


def from_series(s, D, A, present):
    """Inverse of to_series: values back onto [D][A], absent cells NaN."""
    out = np.full(D * A, np.nan)
    if present is None:
        out[:] = s.to_numpy()
    else:
        out[present.reshape(-1)] = s.to_numpy()
    return out.reshape(D, A)


def _arg_back(fn):
    return lambda w: np.nan if np.isnan(w).any() else float(fn(w[::-1]))


def pandas_op(s, op, W, q=0.5, interpolation="linear"):
    """The pandas expression each operator is defined by, on a (date, symbol) Series or frame."""
    def roll(c):
        r = c.rolling(W)
        if op == "min":
            return r.min()
        if op == "max":
            return r.max()
        if op == "argmin":
            return r.apply(_arg_back(np.argmin), raw=True)
        if op == "argmax":
            return r.apply(_arg_back(np.argmax), raw=True)
        if op == "median":
            return r.median()
        return r.quantile(q, interpolation=interpolation)
    return s.groupby(level="symbol").transform(roll)
