"""Shared by the rolling higher-moment tests (host and GPU): the numpy reference of ts_skew /
ts_kurt / ts_cov and the seeded case panels.  No GPU needed, no fixture file.

The reference restates pandas 2.3's ``roll_skew`` / ``roll_kurt``: the symbol's
whole series is centred first (plain-order mean, C ``round`` -- half away from zero -- unless
the minimum lies far below the mean), then the power sums walk the rows with Kahan
compensation on both the add and the remove side, never reset.  It is vectorised over columns
and sequential over rows.  ts_cov is ``Rolling.cov`` built from ``oracle.numerics.roll_mean``
as ``oracle.ops.ts_corr`` builds its numerator.  tests/test_ts_moments_host.py pins all three
to pandas bit for bit on every panel below; the GPU tests compare the kernels with them.

A panel is ``x [F][D][A]`` float64 and ``present [D][A]`` bool or None; a ragged column's
window is its last W PRESENT rows, so ``ref_panel`` compacts each column's present rows, runs
the dense reference on them and scatters the result back.  Absent cells are NaN.
"""
from __future__ import annotations

import numpy as np
import pandas as pd

import oracle.numerics as nm
from ts_order_cases import from_series, make_present, panel_index, to_series  # noqa: F401  (re-exported)

OPS = ("skew", "kurt", "cov")
MIN_W = {"skew": 3, "kurt": 4, "cov": 2}            # shorter windows are all NaN
CENTRE_BELOW = {"skew": -1e5, "kurt": -1e4}         # centred iff min - mean > this

F, D, A = 3, 75, 130                                # A: two waves and two lanes
WINDOWS = (1, 2, 3, 4, 5, 8, 9, 20, 64, 75, 80)     # 75 = D; 80 > D: all NaN
EDGE_ASSETS = (1, 63, 64, 65)
EDGE_WINDOWS = (3, 4, 7)
DATE_WINDOWS = (4, 5)
PREFETCH = 8                                        # ts_moments.hip TSM_B: dates per register batch
CONTENT_D = 40
CONTENT_WINDOWS = (3, 4, 5, 9)
COV_WINDOWS = (1, 2, 5, 20)


def date_edges(W):
    """D around the 8-date prefetch group (one batch less one, one, one and a row, two batches
    and their neighbours: the tail loop runs 7, 0, 1, 7, 0, 1 rows) and around the window."""
    B = PREFETCH
    return sorted({1, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, W, W + 1, 2 * W + 3})


def prep(v):
    """Rolling._prep_values: +-inf count as NaN."""
    v = np.asarray(v, dtype=np.float64)
    return np.where(np.isfinite(v), v, np.nan)


def c_round(m):
    """C ``round``: to the nearest integer, halves away from zero (np.round is half-even)."""
    t = np.trunc(m)
    return np.where(np.abs(m - t) >= 0.5, t + np.copysign(1.0, m), t)


def centre(v, op):
    """v [N][C] prepped -> (the value subtracted from every row of a column, 0.0 where the
    column is not centred; whether it is centred)."""
    ok = v == v
    s = np.zeros(v.shape[1])
    for i in range(v.shape[0]):                      # plain adds in row order
        s = np.where(ok[i], s + v[i], s)
    n = ok.sum(axis=0)
    with np.errstate(all="ignore"):
        mean = s / n
        mn = np.where(ok, v, np.inf).min(axis=0) if v.shape[0] else np.full(v.shape[1], np.inf)
        cen = (mn - mean) > CENTRE_BELOW[op]         # False for an all-NaN column
    return np.where(cen, c_round(np.where(cen, mean, 0.0)), 0.0), cen


def ref_dense_moment(x, op, W):
    """roll_skew / roll_kurt: x [N][C] (every row present) -> [N][C]."""
    P = MIN_W[op]
    minp = max(W, P)
    v = prep(x)
    N, C = v.shape
    out = np.full((N, C), np.nan)
    if N == 0:
        return out
    m, cen = centre(v, op)
    vc = np.where(cen[None, :], v - m[None, :], v)
    S = [np.zeros(C) for _ in range(P)]
    CA = [np.zeros(C) for _ in range(P)]
    CR = [np.zeros(C) for _ in range(P)]
    nobs = np.zeros(C, dtype=np.int64)
    same = np.zeros(C, dtype=np.int64)
    prev = np.full(C, np.nan)
    with np.errstate(all="ignore"):
        for i in range(N):
            if i >= W:
                val = vc[i - W]
                ok = val == val
                nobs = nobs - ok
                p = val
                for k in range(P):
                    if k:
                        p = p * val                  # val*val*val, left to right
                    y = -p - CR[k]
                    t = S[k] + y
                    CR[k] = np.where(ok, t - S[k] - y, CR[k])
                    S[k] = np.where(ok, t, S[k])
            val = vc[i]
            ok = val == val
            nobs = nobs + ok
            p = val
            for k in range(P):
                if k:
                    p = p * val
                y = p - CA[k]
                t = S[k] + y
                CA[k] = np.where(ok, t - S[k] - y, CA[k])
                S[k] = np.where(ok, t, S[k])
            same = np.where(ok, np.where(val == prev, same + 1, 1), same)
            prev = np.where(ok, val, prev)
            dn = nobs.astype(np.float64)
            if op == "skew":
                a = S[0] / dn
                b = S[1] / dn - a * a
                c = S[2] / dn - a * a * a - 3 * a * b
                r = np.sqrt(b)
                res = (np.sqrt(dn * (dn - 1.0)) * c) / ((dn - 2) * r * r * r)
                res = np.where(same >= nobs, 0.0, np.where(b <= 1e-14, np.nan, res))
            else:
                a = S[0] / dn
                r = a * a
                b = S[1] / dn - r
                r = r * a
                c = S[2] / dn - r - 3 * a * b
                r = r * a
                d = S[3] / dn - r - 6 * b * a * a - 4 * c * a
                k_ = (dn * dn - 1.0) * d / (b * b) - 3 * ((dn - 1.0) * (dn - 1.0))
                res = k_ / ((dn - 2.0) * (dn - 3.0))
                res = np.where(same >= nobs, -3.0, np.where(b <= 1e-14, np.nan, res))
            out[i] = np.where(nobs >= minp, res, np.nan)
    return out


def ref_dense_cov(x, y, W):
    """Rolling.cov (ddof 1, min_periods W): x, y [N][C] -> [N][C]."""
    with np.errstate(all="ignore"):
        xv = prep(x + 0 * y)
        yv = prep(y + 0 * x)
        ok = ~np.isnan(xv + yv)
        cs = np.concatenate([np.zeros((1,) + ok.shape[1:]), np.cumsum(ok, axis=0, dtype=np.float64)])
        lo = np.maximum(np.arange(ok.shape[0]) + 1 - W, 0)
        cnt = cs[1:] - cs[lo]
        return (nm.roll_mean(xv * yv, W) - nm.roll_mean(xv, W) * nm.roll_mean(yv, W)) * (cnt / (cnt - 1))


def ref_dense(x, op, W, y=None):
    return ref_dense_cov(x, y, W) if op == "cov" else ref_dense_moment(x, op, W)


def ref_panel(x, present, op, W, y=None):
    """x [F][D][A], present [D][A] bool or None, y [D][A] or [F][D][A] (cov) -> [F][D][A].  Ragged:
    every symbol's present rows move to the top in date order and NaN rows pad the bottom (a NaN
    row after the last real one changes no centre, no state and no earlier output)."""
    Fn, Dn, An = x.shape
    if y is not None:
        y = np.broadcast_to(y, x.shape)
    if present is None:
        return np.stack([ref_dense(x[f], op, W, None if y is None else y[f]) for f in range(Fn)])
    order = np.argsort(~present, axis=0, kind="stable")                 # [D][A]: present rows first
    keep = np.take_along_axis(present, order, axis=0)

    def compact(v):
        return np.where(keep[None], np.take_along_axis(v, np.broadcast_to(order, v.shape), axis=1), np.nan)
    r = np.stack([ref_dense(compact(x)[f], op, W, None if y is None else compact(y)[f]) for f in range(Fn)])
    out = np.full(x.shape, np.nan)
    np.put_along_axis(out, np.broadcast_to(order, x.shape), np.where(keep[None], r, np.nan), axis=1)
    return out


def eligible(shape, present, W):
    """[D][A] bool: the cells on which the symbol has at least W rows (itself included)."""
    Dn, An = shape
    p = np.ones((Dn, An), dtype=bool) if present is None else present
    return p & (np.cumsum(p, axis=0) >= W)


# ------------------------------------------------------------------------------------ panels
def make_values(Fn, Dn, An, seed, nan_frac=0.01):
    """Noise at a scale of its own per column block, a fifth of it rounded to one decimal
    (ties), ~1 % NaN: 0.99 ** 75 = 0.47 of the longest windows stay whole."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((Fn, Dn, An)) * (10.0 ** rng.integers(-3, 4, (Fn, 1, An)))
    x = np.where(rng.random(x.shape) < 0.2, np.round(x, 1), x)
    x = x + np.where(rng.random((Fn, 1, An)) < 0.3, 7.3, 0.0)
    x[rng.random(x.shape) < nan_frac] = np.nan
    return x


def make_y(Dn, An, seed, per_column=0):
    """The cov partner: [D][A], or [per_column][D][A]; 0.3 % NaN of its own."""
    rng = np.random.default_rng(seed + 500)
    shape = (per_column, Dn, An) if per_column else (Dn, An)
    y = 0.01 * rng.standard_normal(shape)
    y = np.where(rng.random(shape) < 0.2, np.round(y, 2), y)
    y[rng.random(shape) < 0.003] = np.nan
    return y


def make_panel(Fn, Dn, An, seed, ragged):
    x = make_values(Fn, Dn, An, seed)
    present = make_present(Dn, An, seed) if ragged else None
    return x, present


def edge_present(Dn, An, seed):
    return np.random.default_rng(seed).random((Dn, An)) >= 0.15


CONTENT = ("const", "const_run", "near_const", "mean7", "mean1e3", "far_low", "low_3e4", "dyadic2.5",
           "dyadic-1.5", "dyadic-2.5", "dyadic0.5", "zeros", "one_nan", "nan_run", "infs", "all_nan", "one_valid",
           "big", "tiny", "short", "never")
RUN0 = 10                                            # first row of the runs


def _dyadic(rng, Dn, mean):
    """Quarters whose plain-order sum is exactly mean * Dn."""
    z = np.round(rng.standard_normal(Dn) * 8) / 4
    z[-1] = mean * Dn - z[:-1].sum()
    assert z.sum() / Dn == mean
    return z


def content_panel(W, ragged=False):
    """[1][40][21] (CONTENT names the columns) and its mask.  The last two columns matter on the
    ragged panel only (W - 1 rows; never present); dense, they are noise."""
    Dn = CONTENT_D
    rng = np.random.default_rng(77)
    x = rng.standard_normal((1, Dn, len(CONTENT)))
    c = {n: x[0, :, i] for i, n in enumerate(CONTENT)}                   # views
    c["const"][:] = 1.25
    c["const_run"][RUN0:RUN0 + W + 2] = 0.75
    c["near_const"][RUN0:RUN0 + W + 3] = 1.0 + 1e-9 * (-1.0) ** np.arange(W + 3)
    c["mean7"][:] += 7.3
    c["mean1e3"][:] += 1e3
    c["far_low"][13] = -3e5
    c["low_3e4"][:] += 5.0
    c["low_3e4"][13] = -3e4
    for name, m in (("dyadic2.5", 2.5), ("dyadic-1.5", -1.5), ("dyadic-2.5", -2.5), ("dyadic0.5", 0.5)):
        c[name][:] = _dyadic(rng, Dn, m)
    c["zeros"][:20] = np.where(np.arange(20) % 2 == 0, 0.0, -0.0)
    c["one_nan"][17] = np.nan
    c["nan_run"][RUN0 + 2:RUN0 + 2 + W + 2] = np.nan
    c["infs"][5] = np.inf
    c["infs"][21] = -np.inf
    c["all_nan"][:] = np.nan
    c["one_valid"][:] = np.nan
    c["one_valid"][19] = 0.5
    c["big"][:] = rng.uniform(-1, 1, Dn) * 1e60
    c["tiny"][:] = rng.uniform(-1, 1, Dn) * 1e-60
    if not ragged:
        return x, None
    present = np.ones((Dn, len(CONTENT)), dtype=bool)
    present[0, ::2] = False                                              # an absent first row
    present[3, :] = False
    present[30, 1::2] = False
    present[:, CONTENT.index("short")] = False
    present[np.arange(W - 1) * 3 + 2, CONTENT.index("short")] = True     # W - 1 rows
    present[:, CONTENT.index("never")] = False
    return poison(x, present), present


def poison(x, present):
    """+inf (even columns) or 12345.0 (odd ones) at the absent cells: not rows, never read as such."""
    fill = np.where(np.arange(x.shape[-1]) % 2 == 0, np.inf, 12345.0)
    return np.where(np.broadcast_to(present, x.shape), x, np.broadcast_to(fill, x.shape))


def content_y(W, ragged=False):
    """The cov partner of content_panel: NaN / inf in y only (rows 9, 25), and in both (17)."""
    Dn = CONTENT_D
    y = 0.5 * np.random.default_rng(78).standard_normal((Dn, len(CONTENT)))
    y[9, :] = np.nan
    y[25, ::3] = np.inf
    y[26, 1::3] = -np.inf
    y[17, CONTENT.index("one_nan")] = np.nan
    y[5, CONTENT.index("infs")] = -np.inf
    if ragged:
        y = poison(y[None], content_panel(W, True)[1])[0]
    return y


# ------------------------------------------------------------------------------------ pandas
def pandas_op(s, op, W, y=None):
    """The pandas expression each operator is defined by, on a (date, symbol) Series or frame."""
    if op == "skew":
        return s.groupby(level="symbol").transform(lambda c: c.rolling(W).skew())
    if op == "kurt":
        return s.groupby(level="symbol").transform(lambda c: c.rolling(W).kurt())
    if isinstance(s, pd.DataFrame):
        cols = {k: pandas_op(s[k], op, W, y[k] if isinstance(y, pd.DataFrame) else y) for k in s.columns}
        return pd.DataFrame(cols, index=s.index)
    ys = dict(list(y.groupby(level="symbol")))
    parts = [g.rolling(W).cov(ys[k]) for k, g in s.groupby(level="symbol")]
    return pd.concat(parts).reindex(s.index).rename(s.name)


def pandas_panel(x, present, op, W, y=None):
    """pandas_op on every column of x [F][D][A] -> [F][D][A], absent cells NaN."""
    Fn, Dn, An = x.shape
    if y is not None:
        y = np.broadcast_to(y, x.shape)
    out = []
    for f in range(Fn):
        ys = None if y is None else to_series(y[f], present, "y")
        out.append(from_series(pandas_op(to_series(x[f], present), op, W, ys), Dn, An, present))
    return np.stack(out)
