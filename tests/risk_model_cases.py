"""Inputs and host-side oracles shared by the factor-risk-model tests (test_risk_model_host.py,
test_gpu_risk_model.py, test_gpu_risk_capi.py).  Plain numpy / pandas, written from the
specification of the model, not from the kernels:

    Sigma_t = B_t' F_t B_t + diag(s2_t)   over the symbols present on date t,

B_t the K x A exposures (a NaN exposure on a present symbol counts as 0), F_t the K x K factor
covariance (its lower triangle is what counts) and s2_t the specific variances.

* ``sigma``: the dense matrix;  ``risk_terms``: every output of ``engine.risk_books`` for one
  book and date, each with the sum of the absolute values of its terms (the scale of the
  a-priori fp64 summation bound the GPU test applies);
* ``fit_oracle``: the pandas fit -- ``ewm().cov()`` of the shifted factor returns,
  ``groupby(level="symbol").ewm().var()`` of the shifted residuals, lower-median fill, floor,
  valid dates;
* ``risk_case`` / ``mvo_case``: generators on ``sim_mvo_cases.make_panel``'s per-asset scales:
  s2 = (0.01 U(0.3, 2))^2, Fc = Q Q' 1e-4 with Q K x K normal, exposures N(0, 1) with some NaN.

``kkt_violation``, ``signs`` and ``tight_slsqp`` are sim_mvo_cases', unchanged.
"""
import numpy as np
import pandas as pd

from sim_mvo_cases import kkt_violation, make_panel, signs, tight_slsqp  # noqa: F401

EPS53 = 2.0 ** -53


def sym_lower(F):
    """The symmetric matrix whose lower triangle is F's."""
    L = np.tril(np.asarray(F, dtype=float))
    return L + np.tril(L, -1).T


def clean_b(B, present=None):
    """Exposures as the model reads them: NaN (and absent cells) as 0.  B [K][A]."""
    B = np.where(np.isfinite(B), B, 0.0)
    if present is not None:
        B = np.where(np.asarray(present)[None, :] != 0, B, 0.0)
    return B


def sigma(B, Fc, s2, present=None):
    """Dense Sigma [n][n] over the present symbols (all of them when ``present`` is None)."""
    keep = np.ones(B.shape[1], dtype=bool) if present is None else np.asarray(present) != 0
    Bc = clean_b(B)[:, keep]
    fac = Bc.T @ sym_lower(Fc) @ Bc
    return 0.5 * (fac + fac.T) + np.diag(np.asarray(s2, dtype=float)[keep])      # symmetric in bits


def sigma_times(B, Fc, s2, w, present=None):
    """sigma(...) @ w over the present symbols without forming the matrix."""
    keep = np.ones(B.shape[1], dtype=bool) if present is None else np.asarray(present) != 0
    Bc = clean_b(B)[:, keep]
    return Bc.T @ (sym_lower(Fc) @ (Bc @ w)) + np.asarray(s2, dtype=float)[keep] * w


def risk_terms(B, Fc, s2, w, present=None):
    """One book on one date -> dict name -> (value, sum of |terms|) with var [3], expo [K],
    contrib [K], marginal [A] (absent cells NaN, scale 0).  A NaN weight is not held (0)."""
    K, A = B.shape
    pr = np.ones(A, dtype=bool) if present is None else np.asarray(present) != 0
    Bc = clean_b(B, pr)
    wv = np.where(np.isfinite(w) & pr, w, 0.0)
    F = sym_lower(Fc)
    s2c = np.where(pr, s2, 0.0)
    b, b_abs = Bc @ wv, np.abs(Bc) @ np.abs(wv)
    Fb, Fb_abs = F @ b, np.abs(F) @ b_abs
    contrib, contrib_abs = b * Fb, b_abs * Fb_abs
    fvar, fvar_abs = contrib.sum(), contrib_abs.sum()
    svar = (wv * wv * s2c).sum()
    marg = Bc.T @ Fb + s2c * wv
    marg_abs = np.abs(Bc).T @ Fb_abs + np.abs(s2c * wv)
    marg = np.where(pr, marg, np.nan)
    return {"var": (np.array([fvar + svar, fvar, svar]), np.array([fvar_abs + svar, fvar_abs, svar])),
            "expo": (b, b_abs), "contrib": (contrib, contrib_abs), "marginal": (marg, np.where(pr, marg_abs, 0.0))}


# ---------------------------------------------------------------------------- generators
def model_arrays(Dm, A, K, seed, nan_frac=0.02, variant=None):
    """(B [K][Dm][A], Fc [Dm][K][K], S2 [Dm][A]) of ``Dm`` model dates.  ``variant``: 'fc0'
    (Fc = 0: a diagonal Sigma), 'dup' (factor 1 duplicates factor 0: Fc singular), 'spread'
    (s2 log-uniform over three decades)."""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((K, Dm, A))
    B[rng.random(B.shape) < nan_frac] = np.nan
    Q = rng.standard_normal((Dm, K, K))
    if variant == "dup" and K >= 2:
        Q[:, 1, :] = Q[:, 0, :]
        B[1] = B[0]
    Fc = 1e-4 * (Q @ Q.transpose(0, 2, 1))
    if variant == "fc0":
        Fc = np.zeros_like(Fc)
    S2 = (0.01 * rng.uniform(0.3, 2.0, (Dm, A))) ** 2
    if variant == "spread":
        S2 = 10.0 ** rng.uniform(-6.0, -3.0, (Dm, A))
    return np.ascontiguousarray(B), np.ascontiguousarray(Fc), np.ascontiguousarray(S2)


def min_leg(u):
    """Symbols a leg needs for the box to be feasible."""
    return int(np.ceil(1.0 / u)) if u < 1 else 1


# (A, K, u, variant): 63 / 64 / 65 straddle a wave, 1100 takes 2 elements per thread, 4100 / 8200
# take 8 / 16, (3, 5) has K > n, K = 32 is the factor cap and (16384, 32) is both caps.
MVO_CASES = [(9, 2, 0.5, None), (12, 12, 0.3, None), (3, 5, 1.0, None), (40, 8, 0.1, None), (63, 8, 0.1, None),
             (64, 8, 0.1, None), (65, 8, 0.1, None), (1100, 6, 0.03, None), (200, 32, 0.03, None),
             (4100, 5, 0.03, None), (8200, 4, 0.03, None), (16384, 32, 0.03, None), (12, 4, 0.3, "fc0"),
             (40, 8, 0.1, "dup"), (40, 8, 0.1, "spread")]


def mvo_case(A, K, u, variant=None):
    """Two book dates over three model dates: (B, Fc, S2, X [2][A], P [2][A] uint8,
    model_row int32 [2] = (0, 2)).  Signals and presence are make_panel's."""
    B, Fc, S2 = model_arrays(3, A, K, 7000 * A + K, variant=variant)
    ab = 2 if A >= 9 else 0
    _, x0, p0 = make_panel(2, A, 1000 * A + K, absent=ab, min_leg=min_leg(u))
    _, x1, p1 = make_panel(2, A, 1000 * A + K + 1, absent=ab, min_leg=min_leg(u))
    return B, Fc, S2, np.stack([x0, x1]), np.stack([p0, p1]), np.array([0, 2], dtype=np.int32)


def risk_case(A, K, M=3, D=3):
    """(B, Fc, S2, W [M][D][A], present [D][A] uint8, valid [D] uint8): book 0 has NaN cells,
    book 1 is all zero, book 2 is dense; date 1 is invalid; two absent symbols where A >= 9."""
    B, Fc, S2 = model_arrays(D, A, K, 31 * A + K, nan_frac=0.05)
    rng = np.random.default_rng(17 * A + K)
    W = rng.standard_normal((M, D, A)) / A
    W[0][rng.random((D, A)) < 0.3] = np.nan
    W[1] = 0.0
    present = np.ones((D, A), dtype=np.uint8)
    if A >= 9:
        for d in range(D):
            present[d, rng.choice(A, 2, replace=False)] = 0
    valid = np.ones(D, dtype=np.uint8)
    valid[1] = 0
    return B, Fc, S2, np.ascontiguousarray(W), present, valid


# ---------------------------------------------------------------------------- the pandas fit
def lower_median_fill(s2_dense, present):
    """Per date: a present symbol whose value is not finite takes sorted(finite)[(n - 1) // 2]."""
    out = np.array(s2_dense, dtype=float)
    for d in range(out.shape[0]):
        pr = present[d] != 0
        fin = pr & np.isfinite(out[d])
        if fin.any():
            med = np.sort(out[d][fin])[(fin.sum() - 1) // 2]
            out[d][pr & ~fin] = med
        out[d][~pr] = np.nan
    return out


def fit_oracle(f: pd.DataFrame, e: pd.Series, cov_halflife, spec_halflife, min_periods, spec_floor=1e-6):
    """The model from its factor returns ``f`` (dates x K) and residuals ``e`` ((date, symbol)):
    (factor_cov (date, factor) x factor, specific_var Series on e.index, valid Series by date)."""
    f = f.copy()
    f[f.isna().any(axis=1)] = np.nan
    cov = f.shift(1).ewm(halflife=cov_halflife, min_periods=min_periods).cov()
    sym = "symbol" if "symbol" in e.index.names else e.index.names[1]
    lagged = e.groupby(level=sym).shift(1)
    raw = (lagged.groupby(level=sym).ewm(halflife=spec_halflife, min_periods=min_periods).var()
           .droplevel(0).reindex(e.index))
    dates = f.index
    dl = e.index.get_level_values(0)
    s2 = raw.copy()
    has_finite = pd.Series(False, index=dates)
    for d in dates:
        m = np.asarray(dl == d)
        v = raw.to_numpy()[m]
        fin = np.isfinite(v)
        if fin.any():
            has_finite[d] = True
            v = np.where(fin, v, np.sort(v[fin])[(fin.sum() - 1) // 2])
        s2.iloc[np.flatnonzero(m)] = v
    s2 = s2.where(~(s2 < spec_floor), spec_floor)          # max(s2, floor); NaN stays NaN
    K = f.shape[1]
    cov_ok = ~np.isnan(cov.to_numpy().reshape(len(dates), K * K)).any(axis=1)
    valid = pd.Series(cov_ok & has_finite.to_numpy(), index=dates)
    return cov, s2, valid
