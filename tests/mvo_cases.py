"""Inputs and host-side checks shared by the MVO selection tests (test_gpu_mvo.py).

The returns generator is the one the CPU prototype of the solver used: a common component,
idiosyncratic noise of per-factor scale U(0.3, 2), all at scale 0.01, plus a per-factor
drift of 0.001.  ``kkt_violation`` certifies a solution of

    max_w  mu'w - gamma w'Sigma w - tau |w - p|_1    s.t.  sum w = 1, 0 <= w <= u

with no reference solver: with g = mu - 2 gamma Sigma w, w is optimal iff some nu puts every
g_i - nu inside  d(tau |w_i - p_i|) + N_[0,u](w_i), an interval [lo_i, hi_i].  The largest
distance max_i dist(g_i - nu, [lo_i, hi_i]) = max(0, a + nu, b - nu), a = max_i(lo_i - g_i),
b = max_i(g_i - hi_i), is piecewise linear in nu and smallest at max(0, (a + b) / 2).
"""
import numpy as np


def make_returns(D, F, seed, const_col=None):
    rng = np.random.default_rng(seed)
    common = rng.standard_normal((D, 1))
    scale = rng.uniform(0.3, 2.0, F)
    noise = rng.standard_normal((D, F)) * scale
    drift = 0.001 * rng.standard_normal(F)
    R = 0.01 * (0.6 * common + noise) + drift
    if const_col is not None:
        R[:, const_col] = 0.0025
    return np.ascontiguousarray(R)


def windows(D, W):
    """Every full window [i, i + W) of D rows."""
    d0 = np.arange(0, D - W + 1, dtype=np.int32)
    return d0, d0 + np.int32(W)


def kkt_violation(mu, Sigma, w, gamma, u, tau=0.0, p=None):
    """(smallest max stationarity violation over nu, the scale max(|mu|_inf, |2 gamma Sigma w|_inf))."""
    F = len(w)
    q = 2.0 * gamma * (Sigma @ w)
    g = mu - q
    lo = np.zeros(F)
    hi = np.zeros(F)
    if tau > 0 and p is not None:
        lo = np.where(w > p, tau, -tau).astype(float)
        hi = np.where(w < p, -tau, tau).astype(float)
    lo = np.where(w == 0.0, -np.inf, lo)      # N_[0,u](0) = (-inf, 0]
    hi = np.where(w == u, np.inf, hi)         # N_[0,u](u) = [0, +inf)
    a = np.max(lo - g)
    b = np.max(g - hi)
    viol = max(0.0, 0.5 * (a + b)) if np.isfinite(a) and np.isfinite(b) else 0.0
    return viol, max(np.abs(mu).max(), np.abs(q).max())


def objective(mu, Sigma, w, gamma, tau=0.0, p=None):
    v = mu @ w - gamma * (w @ Sigma @ w)
    if tau > 0 and p is not None:
        v -= tau * np.abs(w - p).sum()
    return v


def slsqp(mu, Sigma, gamma, u):
    """The QP (no turnover term) by scipy's SLSQP, from the equal-weight start."""
    from scipy.optimize import minimize
    F = len(mu)
    res = minimize(lambda w: gamma * (w @ Sigma @ w) - mu @ w, np.full(F, 1.0 / F),
                   jac=lambda w: 2.0 * gamma * (Sigma @ w) - mu, method="SLSQP", bounds=[(0.0, u)] * F,
                   constraints=[{"type": "eq", "fun": lambda w: w.sum() - 1.0, "jac": lambda w: np.ones(F)}],
                   options={"ftol": 1e-16, "maxiter": 2000})
    return res.x
