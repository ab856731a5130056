"""Shared by the ts_ols tests: seeded generators and a brute-force reference of the rolling
multi-factor OLS DESIGN §22 specifies.  No GPU needed.

Panels are ``Y [Fy][D][A]``, ``X [K][D][A]`` (per-symbol regressors) or, shared, ``X [K][D]``
(one table for every symbol), optional ``present [D][A]``.

The reference builds each output's window by the row rule (the column's last W valid rows
ending at a valid row d), takes the kept set from the numpy model of the fit
(``cs_ols_cases.model_one`` with unit weights: the very algorithm of DESIGN §19) and the values
from ``np.linalg.lstsq`` on the kept columns, each divided by its window norm and the
coefficients rescaled afterwards: lstsq on the raw design of the scaled generator (columns
spanning nine decades) is itself off by up to 7.8e-9 in resid, and a tolerance must not
measure lstsq's error.

A reference over every cell of a 75 x 130 x 2 panel is 14,000 Python-level fits per case, a
few seconds each over a grid of 160: the VALUES are therefore computed for the asset columns
``CHECK_ASSETS`` (both waves of the 130-asset panel, their first and last lanes and the
two-lane tail; every thread of the kernel computes its own output from its own rows), the NaN
pattern -- where an output exists -- for every cell.
"""
from __future__ import annotations

import numpy as np

import cs_ols_cases as CS

D, A, FY = 75, 130, 2
CHECK_ASSETS = (0, 1, 2, 31, 32, 62, 63, 64, 65, 66, 95, 96, 126, 127, 128, 129)
GRID_K = (1, 2, 3, 5, 8)
GRID_GENS = ("plain", "scaled", "corr", "shared")
OUTPUTS = ("beta", "alpha", "fitted", "resid", "r2", "sigma")


def grid_windows(K, intercept):
    """W in {2p + 4, 20 where >= 2p + 4, 64, 75}: below 2p + 4 random windows are nearly
    singular (kept pivots down to 1.9e-9 at W = p + 1) and cannot carry a value tolerance."""
    p = K + int(bool(intercept))
    ws = {2 * p + 4, 64, 75}
    if 20 >= 2 * p + 4:
        ws.add(20)
    return sorted(ws)


# ---- bounds ------------------------------------------------------------------------------
# DESIGN §19's rule: 25 x the worst difference of the model from the reference over the parity
# grid (tests/test_ts_ols_host.py::test_model_worst_against_reference prints the maxima recorded
# here), rounded up to a power of ten.  resid / fitted / alpha / sigma relative to the window's
# max|y|, beta in standardised units |d beta_k| sd_k / max|y|, r2 absolute.
# The smallest kept pivot over the grid is 3.0e-3 and no column is dropped.
MEASURED_MODEL_WORST = dict(resid=2.8e-14, fitted=2.9e-14, beta=3.0e-14, alpha=6.1e-14, sigma=3.0e-16, r2=6.7e-16)
BOUNDS = dict(resid=1e-12,      # 25 x 2.8e-14 = 7.0e-13
              fitted=1e-12,     # 25 x 2.9e-14 = 7.3e-13
              beta=1e-12,       # 25 x 3.0e-14 = 7.5e-13
              alpha=1e-11,      # 25 x 6.1e-14 = 1.6e-12
              sigma=1e-14,      # 25 x 3.0e-16 = 7.5e-15
              r2=1e-13)         # 25 x 6.7e-16 = 1.7e-14
# K = 1 against the reference's raw-moment rolling regression (oracle.ops.ts_regression_fast_long,
# and on the GPU engine.ts_regression) on well-conditioned N(0, 1) data: same rule, from
# tests/test_ts_ols_host.py::test_row_rule_against_ts_regression_fast.  resid / fitted / alpha
# relative to the window's max|y|, beta standardised, r2 absolute.
MEASURED_K1_WORST = dict(resid=9.1e-16, fitted=9.1e-16, beta=4.2e-16, alpha=5.4e-16, r2=9.5e-16)
K1_BOUNDS = dict(resid=1e-13, fitted=1e-13, beta=1e-13, alpha=1e-13, r2=1e-13)   # 25 x each = 1.1e-14 .. 2.4e-14


def rule_bound(worst):
    """25 x worst, rounded up to a power of ten."""
    return 10.0 ** np.ceil(np.log10(25.0 * worst))


# ---- generators --------------------------------------------------------------------------
def make_case(gen, K, D=D, A=A, Fy=FY, seed=0, nans=True):
    """(Y, X, shared) of one generator; regressors carry 1 % NaN cells and y 3 % when ``nans``."""
    rng = np.random.default_rng([seed, K, D, A])
    shared = gen == "shared"
    X = rng.standard_normal((K, D) if shared else (K, D, A))
    if gen == "scaled":
        off = rng.integers(-10, 11, size=K).astype(np.float64)
        e = rng.integers(-4, 5, size=K)
        X = (X + off[:, None, None]) * (10.0 ** e)[:, None, None]
    elif gen == "corr":
        if K >= 2:
            X[1] = 0.9 * X[0] + np.sqrt(1.0 - 0.81) * X[1]
    elif gen not in ("plain", "shared"):
        raise ValueError(gen)
    Xp = np.broadcast_to(X[:, :, None], (K, D, A)) if shared else X
    Y = CS.make_y(Xp, rng, Fy)
    if nans:
        X[rng.random(X.shape) < 0.01] = np.nan
        Y[rng.random(Y.shape) < 0.03] = np.nan
    return Y, X, shared


def as_panel(X, A):
    """A shared table [K][D] broadcast to a panel [K][D][A]."""
    return np.ascontiguousarray(np.broadcast_to(X[:, :, None], X.shape + (A,)))


# ---- the row rule ------------------------------------------------------------------------
def valid_rows(Y, X, present=None, shared=False):
    """bool [Fy][D][A]: present, y finite, all K regressors finite (+-inf invalidates)."""
    xok = np.isfinite(X).all(axis=0)
    ok = np.isfinite(Y) & (xok[:, None] if shared else xok)[None]
    if present is not None:
        ok &= (np.asarray(present) != 0)[None]
    return ok


def exists(valid, W):
    """bool like ``valid``: row d is valid and the column has >= W valid rows up to d."""
    return valid & (np.cumsum(valid, axis=1) >= W)


# ---- one window --------------------------------------------------------------------------
def scaled_lstsq(y, X, intercept, kept):
    """lstsq on [1, X_kept], every column divided by its window norm, coefficients rescaled."""
    n, K = X.shape
    cols = np.flatnonzero(kept)
    Dm = np.concatenate([np.ones((n, 1)), X[:, cols]], axis=1) if intercept else X[:, cols]
    if Dm.shape[1]:
        nrm = np.sqrt((Dm * Dm).sum(axis=0))
        coef = np.linalg.lstsq(Dm / nrm, y, rcond=None)[0] / nrm
    else:
        coef = np.zeros(0)
    fitted = Dm @ coef
    beta = np.full(K, np.nan)
    beta[cols] = coef[1:] if intercept else coef
    return beta, (coef[0] if intercept else np.nan), fitted


def window_fit(y, X, intercept, which):
    """One window (y [W], X [W][K], oldest row first) -> the six outputs at the window's last
    row, plus kept / pivots / sd / ymax; ``which`` = "lstsq", "model" or "both" (a pair)."""
    Wn, K = X.shape
    m = CS.model_one(y, X, np.ones(Wn), intercept)
    kept = m["kept"]
    yc = y - y.mean() if intercept else y
    sst = (yc * yc).sum()
    dof = Wn - (int(kept.sum()) + int(bool(intercept)))
    common = dict(kept=kept, pivots=m["pivots"], sd=X.std(axis=0), ymax=np.abs(y).max())

    def finish(beta, alpha, fitted):
        resid = y - fitted
        ssr = (resid * resid).sum()
        return dict(common, beta=beta, alpha=alpha, fitted=fitted[-1], resid=resid[-1],
                    r2=(1.0 - ssr / sst) if sst != 0 else np.nan, sigma=np.sqrt(ssr / dof) if dof > 0 else np.nan)

    if which == "model":
        return finish(m["beta"], m["alpha"], m["fitted"])
    ref = finish(*scaled_lstsq(y, X, intercept, kept))
    return (ref, finish(m["beta"], m["alpha"], m["fitted"])) if which == "both" else ref


# ---- the brute-force reference -----------------------------------------------------------
def ref_panel(Y, X, W, present=None, intercept=True, shared=False, assets=CHECK_ASSETS, which="lstsq"):
    """The reference (``which="lstsq"``), the numpy model of the algorithm (``"model"``) or the
    pair of them (``"both"``).  Values at the asset columns ``assets`` (None: all), NaN
    elsewhere; ``exists`` [Fy][D][A] for every cell.  Returns dict(beta / kept / pivots / sd
    [Fy][K][D][A], alpha / fitted / resid / r2 / sigma / ymax [Fy][D][A], exists, assets)."""
    Fy, Dn, An = Y.shape
    K = X.shape[0]
    assets = [a for a in (range(An) if assets is None else assets) if a < An]
    valid = valid_rows(Y, X, present, shared)
    outs = []
    for _ in range(2 if which == "both" else 1):
        out = {k: np.full((Fy, K, Dn, An), np.nan) for k in ("beta", "pivots", "sd")}
        out["kept"] = np.zeros((Fy, K, Dn, An), dtype=bool)
        for k in ("alpha", "fitted", "resid", "r2", "sigma", "ymax"):
            out[k] = np.full((Fy, Dn, An), np.nan)
        out["exists"] = exists(valid, W)
        out["assets"] = np.asarray(assets, dtype=np.int64)
        outs.append(out)
    for f in range(Fy):
        for a in assets:
            rows = np.flatnonzero(valid[f, :, a])
            if rows.size < W:
                continue
            yv = Y[f, rows, a]
            Xv = (X[:, rows] if shared else X[:, rows, a]).T
            for i in range(W - 1, rows.size):
                r = window_fit(yv[i - W + 1:i + 1], np.ascontiguousarray(Xv[i - W + 1:i + 1]), intercept, which)
                d = rows[i]
                for out, ri in zip(outs, r if which == "both" else (r,)):
                    for k in ("beta", "kept", "pivots", "sd"):
                        out[k][f, :, d, a] = ri[k]
                    for k in ("alpha", "fitted", "resid", "r2", "sigma", "ymax"):
                        out[k][f, d, a] = ri[k]
    return tuple(outs) if which == "both" else outs[0]


# ---- comparison --------------------------------------------------------------------------
def errors(got, ref, all_cells=True):
    """Worst errors of ``got`` (dict of numpy arrays: any of the six outputs, full panels) against
    ``ref`` (from ref_panel) in the units of the bounds.  Asserted exactly: where an output
    exists, on every cell (``all_cells``; off when ``got`` is itself a ref_panel, which holds
    values at the asset columns only); the kept set (beta's NaN pattern) and every NaN pattern
    on the reference's asset columns."""
    ex, cols = ref["exists"], ref["assets"]
    if not all_cells:
        ex = ex & np.isin(np.arange(ex.shape[-1]), cols)
    err = {}
    for k in OUTPUTS:
        if k not in got:
            continue
        g = np.asarray(got[k])
        r = ref[k]
        assert g.shape == r.shape, (k, g.shape, r.shape)
        if k == "beta":
            assert not (~np.isnan(g) & ~ex[:, None]).any(), "beta: a value where no output exists"
            gc, rc = g[..., cols], r[..., cols]
            assert np.array_equal(~np.isnan(gc), ref["kept"][..., cols]), "beta: the kept set differs"
            e = np.abs(gc - rc) * ref["sd"][..., cols] / ref["ymax"][..., cols][:, None]
        else:
            if k == "fitted" or k == "resid":
                assert np.array_equal(~np.isnan(g), ex), f"{k}: NaN pattern differs from the row rule"
            else:
                assert not (~np.isnan(g) & ~ex).any(), f"{k}: a value where no output exists"
            gc, rc = g[..., cols], r[..., cols]
            assert np.array_equal(np.isnan(gc), np.isnan(rc)), f"{k}: NaN pattern differs"
            e = np.abs(gc - rc) / (1.0 if k == "r2" else ref["ymax"][..., cols])
        err[k] = float(np.nanmax(e)) if np.isfinite(e).any() else 0.0
    return err


def assert_within(err, where="", bounds=None):
    bounds = BOUNDS if bounds is None else bounds
    bad = {k: v for k, v in err.items() if not v <= bounds[k]}
    assert not bad, f"{where}: outside the bounds {bad} (bounds {bounds})"


merge_worst = CS.merge_worst


# ---- K = 1 against the one-regressor rolling regression ------------------------------------
def k1_panel(gapped):
    """K = 1, N(0, 1) x and y = 0.05 + 0.5 x + noise on 60 x 12, dense or with NaN gaps."""
    rng = np.random.default_rng(17 + gapped)
    Dn, An = 60, 12
    x = rng.standard_normal((Dn, An))
    y = 0.05 + 0.5 * x + 0.5 * rng.standard_normal((Dn, An))
    if gapped:
        x[rng.random((Dn, An)) < 0.06] = np.nan
        y[rng.random((Dn, An)) < 0.06] = np.nan
        y[:9, 3] = np.nan                                  # a late listing
        x[20:31, 5] = np.nan                               # a long gap
    return y, x


def k1_errors(got, y, x, W, fast):
    """Worst differences of the K = 1 outputs ``got`` (dict of [D][A]: resid, alpha, beta,
    fitted, r2) from ``fast(rettype) -> [D][A]`` (NaN where it has no value), in the units of
    K1_BOUNDS; the NaN patterns must agree exactly."""
    valid = np.isfinite(y) & np.isfinite(x)
    err = {}
    ymax = np.full(y.shape, np.nan)
    sd = np.full(y.shape, np.nan)
    for a in range(y.shape[1]):
        rows = np.flatnonzero(valid[:, a])
        for i in range(W - 1, rows.size):
            win = rows[i - W + 1:i + 1]
            ymax[rows[i], a] = np.abs(y[win, a]).max()
            sd[rows[i], a] = x[win, a].std()
    for name, rt in (("resid", 0), ("alpha", 1), ("beta", 2), ("fitted", 3), ("r2", 6)):
        ref = fast(rt)
        assert np.array_equal(np.isnan(got[name]), np.isnan(ref)), f"{name}: the row rule differs"
        scale = 1.0 if name == "r2" else (ymax / sd if name == "beta" else ymax)
        e = np.abs(got[name] - ref) / scale
        err[name] = float(np.nanmax(e)) if np.isfinite(e).any() else 0.0
    return err
