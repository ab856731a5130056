"""Shared by the exponentially weighted operator tests (host and GPU): the numpy restatement of
pandas' ewm / ewmcov recursions, vectorised across columns and assets, and the
seeded panels.  No GPU needed, no fixture file.

tests/test_ts_ewm_host.py pins ``ref_panel`` to pandas bit for bit; the GPU tests compare the
kernels with it.  A panel is ``x [F][D][A]`` float64, ``y [D][A]`` (shared by the F columns) or
None, and ``present [D][A]`` bool or None.  An absent cell is no row of its symbol: it changes
no state and its output is NaN.
"""
from __future__ import annotations

import itertools

import numpy as np
import pandas as pd

from ts_order_cases import from_series, panel_index, to_series  # noqa: F401  (re-exported)

SINGLE = ("mean", "var", "std", "zscore")
PAIR = ("cov", "corr")
OUTS = SINGLE + PAIR
PANDAS_OUTS = ("mean", "var", "std", "cov", "corr")     # zscore is defined from mean and std

# the decay parameters of the host grid; the GPU main panel uses DECAYS_GPU
DECAYS = (("span", 3), ("span", 20), ("halflife", 0.5), ("halflife", 10), ("com", 0), ("com", 7.3),
          ("alpha", 1 / 3), ("alpha", 0.03))
DECAYS_GPU = (("span", 20), ("halflife", 0.5), ("com", 0), ("alpha", 0.03))
PREFETCH = 8                                            # ts_ewm.hip EWM_B: rows per register batch


def com_of(kind, v):
    """pandas.core.window.common.get_center_of_mass."""
    if kind == "com":
        return float(v)
    if kind == "span":
        return float((v - 1) / 2)
    if kind == "halflife":
        return float(1 / (1 - np.exp(np.log(0.5) / v)) - 1)
    return float((1 - v) / v)


def decay_id(p):
    return f"{p[0]}{p[1]:.3g}"


def grid(decays, minps):
    """(kind, value, adjust, ignore_na, min_periods)"""
    return [(k, v, adj, ign, mp) for (k, v), adj, ign, mp in itertools.product(decays, (True, False), (False, True),
                                                                               minps)]


# ------------------------------------------------------------------------------------ reference
def _debias(sw, sw2, cov):
    num = sw * sw
    den = num - sw2
    return np.where(den > 0, (num / den) * cov, np.nan)


def _zsqrt(v):
    r = np.sqrt(v)
    return np.where(v < 0, 0.0, r)


def ref_panel(x, y, present, com, adjust=True, ignore_na=False, min_periods=0, want=OUTS):
    """x [F][D][A], y [D][A] or None, present [D][A] bool or None -> {name: [F][D][A]}.

    pandas' ewm (mean) and ewmcov (the rest) row by row, every operation in pandas' order; the
    state starts at (mean NaN, cov 0, sum_wt = sum_wt2 = old_wt = 1, nobs 0), from which the
    general step reproduces pandas' first-row rule."""
    F, D, A = x.shape
    alpha = 1.0 / (1.0 + com)
    f = 1.0 - alpha
    nw = 1.0 if adjust else alpha
    minp = max(int(min_periods), 1)
    out = {k: np.full(x.shape, np.nan) for k in want}
    with np.errstate(all="ignore"):
        for pair in (False, True):
            names = [k for k in want if k in (PAIR if pair else SINGLE)]
            if not names:
                continue
            mx = np.full((F, A), np.nan)
            my = np.full((F, A), np.nan)
            cxy, cxx, cyy = np.zeros((F, A)), np.zeros((F, A)), np.zeros((F, A))
            sw, sw2, ow = np.ones((F, A)), np.ones((F, A)), np.ones((F, A))
            nobs = np.zeros((F, A), dtype=np.int64)
            for d in range(D):
                pr = np.ones((F, A), dtype=bool) if present is None else np.broadcast_to(present[d], (F, A))
                raw = x[:, d, :]
                cx = np.where(np.isfinite(raw), raw, np.nan)                # +-inf count as NaN
                cy = np.broadcast_to(np.where(np.isfinite(y[d]), y[d], np.nan), (F, A)) if pair else cx
                obs = pr & ~np.isnan(cx) & ~np.isnan(cy)
                nobs = nobs + obs
                live = ~np.isnan(mx)
                dec = pr & live & (obs | (not ignore_na))
                upd = dec & obs
                first = pr & ~live & obs
                ow = np.where(dec, ow * f, ow)
                sw = np.where(dec, sw * f, sw)
                sw2 = np.where(dec, sw2 * (f * f), sw2)
                wsum = ow + nw
                omx, omy = mx, my
                mx = np.where(upd & (omx != cx), ((ow * omx) + (nw * cx)) / wsum, mx)
                my = np.where(upd & (omy != cy), ((ow * omy) + (nw * cy)) / wsum, my)
                dmx, dmy, dcx, dcy = omx - mx, omy - my, cx - mx, cy - my
                cxy = np.where(upd, ((ow * (cxy + (dmx * dmy))) + (nw * (dcx * dcy))) / wsum, cxy)
                cxx = np.where(upd, ((ow * (cxx + (dmx * dmx))) + (nw * (dcx * dcx))) / wsum, cxx)
                cyy = np.where(upd, ((ow * (cyy + (dmy * dmy))) + (nw * (dcy * dcy))) / wsum, cyy)
                sw = np.where(upd, sw + nw, sw)
                sw2 = np.where(upd, sw2 + nw * nw, sw2)
                ow = np.where(upd, wsum, ow)
                if not adjust:
                    sw = np.where(upd, sw / ow, sw)
                    sw2 = np.where(upd, sw2 / (ow * ow), sw2)
                    ow = np.where(upd, 1.0, ow)
                mx = np.where(first, cx, mx)
                my = np.where(first, cy, my)
                full = pr & (nobs >= minp)
                if pair:
                    if "cov" in out:
                        out["cov"][:, d, :] = np.where(full, _debias(sw, sw2, cxy), np.nan)
                    if "corr" in out:
                        out["corr"][:, d, :] = np.where(full, cxy / _zsqrt(cxx * cyy), np.nan)
                else:
                    mean = np.where(full, mx, np.nan)
                    var = np.where(full, _debias(sw, sw2, cxx), np.nan)
                    std = _zsqrt(var)
                    for k, v in (("mean", mean), ("var", var), ("std", std), ("zscore", (raw - mean) / std)):
                        if k in out:
                            out[k][:, d, :] = v
    return out


def same_bits(a, b):
    """NaN positions equal, every other value equal as an int64 view."""
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return np.array_equal(np.ascontiguousarray(a)[~na].view(np.int64), np.ascontiguousarray(b)[~nb].view(np.int64))


# ------------------------------------------------------------------------------------ panels
def make_values(F, D, A, seed, nan_frac=0.05):
    """Normal values on per-column scales over six decades, ``nan_frac`` NaN."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((F, D, A)) * np.exp(rng.standard_normal((F, 1, A)) * 3)
    x[rng.random((F, D, A)) < nan_frac] = np.nan
    return x


def make_pair(F, D, A, seed, nan_frac=0.05):
    """x [F][D][A] and a correlated y [D][A] with its own, independently placed NaN."""
    x = make_values(F, D, A, seed, nan_frac)
    rng = np.random.default_rng(seed + 500)
    y = rng.standard_normal((D, A)) + 0.3 * np.nan_to_num(x[0]) / np.exp(1.5)
    y[rng.random((D, A)) < nan_frac] = np.nan
    return x, y


def make_present(D, A, seed):
    """Ragged mask: a third of the symbols list late, 10 % of all cells are gaps, every fourth
    symbol keeps all its rows and the last symbol has exactly one row."""
    rng = np.random.default_rng(seed + 1000)
    p = rng.random((D, A)) >= 0.10
    late = rng.random(A) < 1 / 3
    start = np.where(late, rng.integers(1, max(2, D // 2 + 1), A), 0)
    p &= np.arange(D)[:, None] >= start[None, :]
    p[:, ::4] = True
    p[:, A - 1] = False
    p[D // 2, A - 1] = True
    return p


def special_columns(n, seed):
    """x, y [n][7]: 0 / 5 / 15 % NaN (independently in x and y), leading NaNs, a column in
    quarters with a constant stretch, +-inf cells in x and in y, a constant column."""
    rng = np.random.default_rng(seed)
    C = 7
    x = rng.standard_normal((n, C)) * np.exp(rng.standard_normal(C) * 3)
    y = rng.standard_normal((n, C)) + 0.3 * x / np.abs(x).max(axis=0)
    for c, frac in ((1, 0.05), (2, 0.15), (3, 0.05)):
        x[rng.random(n) < frac, c] = np.nan
        y[rng.random(n) < frac, c] = np.nan
    x[: min(3, n), 3] = np.nan                              # leading NaNs
    x[:, 4] = np.round(x[:, 4] / np.abs(x[:, 4]).max() * 16) / 4
    if n > 30:
        x[10:30, 4] = x[10, 4]                              # a constant stretch: the != guard
    for i, (col, val) in enumerate(((x, np.inf), (x, -np.inf), (y, np.inf), (y, -np.inf))):
        if n > 1:
            col[(5 + 11 * i) % n, 5] = val
    x[:, 6] = 1.25
    return x, y


def nan_run_column(D=1300, run=(40, 1240), seed=1):
    """x, y [D]: a NaN run of 1,200 rows (old_wt passes through the subnormals to 0 at alpha
    0.5), +-inf cells, and a short NaN stretch in y near the end."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(D)
    y = rng.standard_normal(D)
    x[run[0]:run[1]] = np.nan
    x[5] = np.inf
    x[D - 50] = -np.inf
    y[D - 20:D - 10] = np.nan
    return x, y


# ------------------------------------------------------------------------------------ pandas
def pandas_series(sx, sy, out, kind, v, adjust, ignore_na, min_periods):
    """One column through Series.ewm."""
    e = sx.ewm(**{kind: v}, adjust=adjust, ignore_na=ignore_na, min_periods=min_periods)
    if out in ("cov", "corr"):
        return getattr(e, out)(sy).to_numpy()
    return getattr(e, out)().to_numpy()


def pandas_grouped(obj, sy, out, kind, v, adjust, ignore_na, min_periods):
    """The expression each operator is defined by, on a (date, symbol) Series or frame: the
    symbol's own rows in date order through ewm, back on ``obj``'s index."""
    def one(c):
        e = c.ewm(**{kind: v}, adjust=adjust, ignore_na=ignore_na, min_periods=min_periods)
        if out in ("cov", "corr"):
            return getattr(e, out)(sy.reindex(c.index))
        if out == "zscore":
            return (c - e.mean()) / e.std()
        return getattr(e, out)()
    return obj.groupby(level="symbol").transform(one)


def pandas_groupby_ewm(s, out, kind, v, adjust, ignore_na, min_periods):
    """``s.groupby(level="symbol").ewm(...).mean() / .var() / .std()`` itself, realigned to
    ``s``'s index.  (``.cov(y)`` / ``.corr(y)`` of the grouped object align ``y`` on the union
    of ALL symbols' rows inside every group, so other symbols' rows become NaN rows that decay
    the weights: not a per-symbol operator.  The pair operators are pinned by pandas_grouped,
    which hands each symbol its own rows of ``y``.)"""
    e = s.groupby(level="symbol").ewm(**{kind: v}, adjust=adjust, ignore_na=ignore_na, min_periods=min_periods)
    return getattr(e, out)().droplevel(0).reindex(s.index)
