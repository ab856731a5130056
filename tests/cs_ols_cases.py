"""Shared by the cs_ols tests: seeded generators, the numpy ``lstsq`` reference and a plain
numpy model of the algorithm DESIGN §19 specifies (the GPU kernel differs from the model in
summation order only).  No GPU needed.

Panels are ``Y [Fy][D][A]``, ``X [K][D][A]``, optional ``W [D][A]`` and ``present [D][A]``.
"""
from __future__ import annotations

import numpy as np

PIVOT_MIN = 1e-10
CONST_REL = 1e-13

# ---- bounds ------------------------------------------------------------------------------
# resid / fitted, relative to max|y| of the (column, date) row: the bound the feature was
# specified with.  With this file's seeding the model's worst difference from lstsq over the
# grid is 3.2e-10 (see below: lstsq's own error), a margin of 3x.
RESID_BOUND = 1e-9
# beta in standardised units |d beta_k| sd_k / max|y|, alpha as |d alpha| / max|y|, r2 absolute.
# Each is 25x the model's worst difference from lstsq over the parity grid (measured by
# tests/test_cs_ols_host.py::test_model_worst_against_lstsq, which prints the maxima recorded
# below), rounded up to a power of ten.  The worst cases are the
# scaled generator at A = 65, K = 32: against an 80-bit evaluation the model is within 1e-13
# there and lstsq (an SVD of the raw design, whose columns span nine decades) within 3.2e-10, so
# these figures -- and the 3.2e-10 the model shows for resid there -- are lstsq's own error.
MEASURED_MODEL_WORST = dict(resid=3.2e-10, beta=7.9e-11, alpha=5.0e-10, r2=6.7e-16)
BETA_BOUND = 1e-8       # 25 x 7.9e-11 = 2.0e-9
ALPHA_BOUND = 1e-7      # 25 x 5.0e-10 = 1.3e-8
R2_BOUND = 1e-13        # 25 x 6.7e-16 = 1.7e-14

GRID_A = (1, 2, 5, 63, 64, 65, 257, 1100, 5000)
GRID_K = (1, 2, 7, 16, 32)
GRID_GENS = ("plain", "scaled", "corr", "weights")


# ---- generators --------------------------------------------------------------------------
def make_y(X, rng, Fy):
    """y = 0.01 (sum of the first min(K, 3) columns) + 0.01 N(0, 1), per y column."""
    K = X.shape[0]
    sig = 0.01 * X[:min(K, 3)].sum(axis=0)
    return sig[None] + 0.01 * rng.standard_normal((Fy,) + X.shape[1:])


def make_case(gen, K, D, A, Fy=3, seed=0):
    """(Y, X, W or None) of one generator."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((K, D, A))
    W = None
    if gen == "plain":
        pass
    elif gen == "scaled":
        off = rng.integers(-10, 11, size=K).astype(np.float64)
        e = rng.integers(-4, 5, size=K)
        X = (X + off[:, None, None]) * (10.0 ** e)[:, None, None]
    elif gen == "corr":
        if K >= 2:
            X[1] = 0.9 * X[0] + np.sqrt(1.0 - 0.81) * X[1]
    elif gen == "weights":
        W = rng.uniform(0.1, 1.1, size=(D, A))
    elif gen == "const":
        X[K // 2] = 3.25
    elif gen == "dup":
        if K >= 2:
            X[K - 1] = X[0]
    elif gen == "dummies":
        # columns 0 .. K-2: complete 0/1 group columns (every asset in exactly one group, no
        # group empty), column K-1 free.  With an intercept the dummies sum to the constant, so
        # the in-order factorisation drops the LAST dummy, column K-2.
        assert K >= 3 and A >= 4 * (K - 1)
        g = np.arange(A) % (K - 1)
        for d in range(D):
            gd = rng.permutation(g)
            for k in range(K - 1):
                X[k, d] = (gd == k).astype(np.float64)
    else:
        raise ValueError(gen)
    return make_y(X, rng, Fy), X, W


def expected_dropped(gen, K):
    """The columns the specification drops for a collinearity generator (with an intercept)."""
    return {"const": [K // 2], "dup": [K - 1] if K >= 2 else [], "dummies": [K - 2]}[gen]


# ---- validity ----------------------------------------------------------------------------
def valid_rows(y, Xd, w, pres):
    """y [A], Xd [K][A], w [A] or None, pres [A] or None -> bool [A]."""
    ok = np.isfinite(y) & np.isfinite(Xd).all(axis=0)
    if pres is not None:
        ok &= pres != 0
    if w is not None:
        with np.errstate(invalid="ignore"):
            ok &= np.isfinite(w) & (w > 0)
    return ok


# ---- the model of the specified algorithm ------------------------------------------------
def model_one(y, X, w, intercept):
    """One (column, date) on compacted rows: y [n], X [n][K], w [n].  n >= K + intercept.
    Returns dict(beta [K] with NaN at dropped columns, alpha, r2, fitted [n], resid [n],
    kept bool [K], pivots [K])."""
    n, K = X.shape
    sw = w.sum()
    if intercept:
        xbar = (w[:, None] * X).sum(axis=0) / sw
        ybar = (w * y).sum() / sw
    else:
        xbar = np.zeros(K)
        ybar = 0.0
    Xc = X - xbar
    yc = y - ybar
    G = Xc.T @ (w[:, None] * Xc)
    g = Xc.T @ (w * yc)
    sst = (w * yc * yc).sum()
    s = np.sqrt(np.diag(G))
    kept = s > 0
    if intercept:
        kept &= ~(s <= CONST_REL * np.sqrt((w[:, None] * X * X).sum(axis=0)))
    with np.errstate(divide="ignore", invalid="ignore"):
        C = G / np.outer(s, s)
        c = g / s
    L = np.zeros((K, K))
    z = np.zeros(K)
    pivots = np.full(K, np.nan)
    for k in range(K):
        if not kept[k]:
            continue
        prev = [j for j in range(k) if kept[j]]
        piv = C[k, k] - sum(L[k, j] * L[k, j] for j in prev)
        pivots[k] = piv
        if not piv >= PIVOT_MIN:
            kept[k] = False
            continue
        L[k, k] = np.sqrt(piv)
        for i in range(k + 1, K):
            if kept[i]:
                L[i, k] = (C[i, k] - sum(L[i, j] * L[k, j] for j in prev)) / L[k, k]
        z[k] = (c[k] - sum(z[j] * L[k, j] for j in prev)) / L[k, k]
    b = np.zeros(K)
    for k in range(K - 1, -1, -1):
        if kept[k]:
            b[k] = (z[k] - sum(L[j, k] * b[j] for j in range(k + 1, K) if kept[j])) / L[k, k]
    with np.errstate(divide="ignore", invalid="ignore"):
        bk = np.where(kept, b / s, 0.0)
    fitted = ybar + Xc @ bk
    resid = y - fitted
    ssr = (w * resid * resid).sum()
    return dict(beta=np.where(kept, bk, np.nan), alpha=(ybar - (bk * xbar).sum()) if intercept else np.nan,
                r2=(1.0 - ssr / sst) if sst != 0 else np.nan, fitted=fitted, resid=resid, kept=kept, pivots=pivots)


def lstsq_one(y, X, w, intercept, kept):
    """numpy lstsq on [1, X_kept] sqrt(w)."""
    n, K = X.shape
    cols = np.flatnonzero(kept)
    Xk = X[:, cols]
    Dm = np.concatenate([np.ones((n, 1)), Xk], axis=1) if intercept else Xk
    rw = np.sqrt(w)
    if Dm.shape[1]:
        coef = np.linalg.lstsq(Dm * rw[:, None], y * rw, rcond=None)[0]
    else:
        coef = np.zeros(0)
    fitted = Dm @ coef
    resid = y - fitted
    beta = np.full(K, np.nan)
    beta[cols] = coef[1:] if intercept else coef
    ybar = (w * y).sum() / w.sum() if intercept else 0.0
    sst = (w * (y - ybar) ** 2).sum()
    ssr = (w * resid * resid).sum()
    return dict(beta=beta, alpha=coef[0] if intercept else np.nan, r2=(1.0 - ssr / sst) if sst != 0 else np.nan,
                fitted=fitted, resid=resid, kept=np.asarray(kept, dtype=bool))


def run_panel(Y, X, W=None, present=None, intercept=True, which="lstsq"):
    """The model (``which="model"``) or the lstsq reference on the model's kept columns over a
    whole panel.  Returns dict(beta [Fy][D][K], alpha, r2 [Fy][D], n int32 [Fy][D], resid,
    fitted [Fy][D][A], kept bool [Fy][D][K], pivots [Fy][D][K], sd [Fy][D][K], ymax [Fy][D])."""
    Fy, D, A = Y.shape
    K = X.shape[0]
    p = K + int(bool(intercept))
    out = dict(beta=np.full((Fy, D, K), np.nan), alpha=np.full((Fy, D), np.nan), r2=np.full((Fy, D), np.nan),
               n=np.zeros((Fy, D), dtype=np.int32), resid=np.full((Fy, D, A), np.nan),
               fitted=np.full((Fy, D, A), np.nan), kept=np.zeros((Fy, D, K), dtype=bool),
               pivots=np.full((Fy, D, K), np.nan), sd=np.full((Fy, D, K), np.nan), ymax=np.full((Fy, D), np.nan))
    for f in range(Fy):
        for d in range(D):
            w = None if W is None else W[d]
            ok = valid_rows(Y[f, d], X[:, d], w, None if present is None else present[d])
            n = int(ok.sum())
            out["n"][f, d] = n
            if n < p:
                continue
            yv = Y[f, d][ok]
            Xv = np.ascontiguousarray(X[:, d][:, ok].T)
            wv = np.ones(n) if w is None else w[ok]
            m = model_one(yv, Xv, wv, intercept)
            r = m if which == "model" else lstsq_one(yv, Xv, wv, intercept, m["kept"])
            out["beta"][f, d] = r["beta"]
            out["alpha"][f, d] = r["alpha"]
            out["r2"][f, d] = r["r2"]
            out["resid"][f, d][ok] = r["resid"]
            out["fitted"][f, d][ok] = r["fitted"]
            out["kept"][f, d] = m["kept"]
            out["pivots"][f, d] = m["pivots"]
            out["sd"][f, d] = Xv.std(axis=0)
            out["ymax"][f, d] = np.abs(yv).max()
    return out


# ---- comparison --------------------------------------------------------------------------
def errors(got, ref):
    """Worst errors of ``got`` (dict of numpy arrays: any of beta, alpha, r2, n, resid, fitted)
    against ``ref`` (from run_panel), in the units of the bounds.  NaN patterns and n must
    match exactly (asserted)."""
    ymax = ref["ymax"]
    err = {}
    if "n" in got:
        assert np.array_equal(got["n"], ref["n"]), "n differs"
    for k in ("resid", "fitted", "beta", "alpha", "r2"):
        if k not in got:
            continue
        g, r = np.asarray(got[k]), ref[k]
        assert g.shape == r.shape, (k, g.shape, r.shape)
        assert np.array_equal(np.isnan(g), np.isnan(r)), f"{k}: NaN pattern differs"
        with np.errstate(invalid="ignore"):
            if k in ("resid", "fitted"):
                e = np.abs(g - r) / ymax[..., None]
            elif k == "beta":
                e = np.abs(g - r) * ref["sd"] / ymax[..., None]
            elif k == "alpha":
                e = np.abs(g - r) / ymax
            else:
                e = np.abs(g - r)
        err[k] = float(np.nanmax(e)) if np.isfinite(e).any() else 0.0
    return err


BOUNDS = dict(resid=RESID_BOUND, fitted=RESID_BOUND, beta=BETA_BOUND, alpha=ALPHA_BOUND, r2=R2_BOUND)


def assert_within(err, where=""):
    bad = {k: v for k, v in err.items() if not v <= BOUNDS[k]}
    assert not bad, f"{where}: outside the bounds {bad} (bounds {BOUNDS})"


def merge_worst(worst, err):
    for k, v in err.items():
        worst[k] = max(worst.get(k, 0.0), v)
    return worst
