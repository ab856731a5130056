"""Inputs and host-side checks shared by the simulator-MVO tests (test_sim_mvo_host.py,
test_gpu_sim_mvo.py).  Plain numpy / pandas, written from the specification of
``Simulation(method="mvo")`` (portfolio_simulation.py:315-461), not from the kernel:

* ``spec_window`` / ``sigma_from_window`` / ``spec_sigma``: the day's returns window and
  Sigma = (1 - s) (cov + 1e-6 I) + s avg_var I over the day's present symbols;
* ``kkt_violation``: a certificate for

      min w'Sigma w   s.t.  sum_pos w = 1, sum_neg w = -1, 0 <= w <= u on pos,
                            -u <= w <= 0 on neg, w = 0 elsewhere

  with no reference solver.  With g = -2 Sigma w, w is optimal iff each leg has a multiplier
  nu that puts every g_i - nu inside the normal cone of the leg's box at w_i, an interval
  [lo_i, hi_i] (lo = -inf at the box's lower end, hi = +inf at its upper end, else 0).  The
  largest distance max_i dist(g_i - nu, [lo_i, hi_i]) = max(0, a + nu, b - nu) with
  a = max_i(lo_i - g_i), b = max_i(g_i - hi_i) is smallest at max(0, (a + b) / 2); the
  certificate is the larger of the two legs' values (mvo_cases.kkt_violation, one multiplier
  per leg);
* ``tight_slsqp``: scipy's SLSQP on the active variables with the analytic Jacobian,
  ftol 1e-16 and the objective scaled by 1 / mean(diag Sigma) (the unscaled objective is of
  order 1e-5 and stops SLSQP early).
"""
import numpy as np
import pandas as pd


def make_panel(Dr, A, seed, zero_frac=0.1, nan_signal=1, absent=0, min_leg=1):
    """(R0 [Dr][A] returns, x [A] signal, present [A] uint8): a common component plus
    idiosyncratic noise of per-asset scale U(0.3, 2) at scale 0.01 (the generator of the
    solver's numpy model); the signal is N(0,1) with some exact zeros.  The first ``min_leg``
    symbols are long and the next ``min_leg`` short (so a box of 1 / min_leg is feasible);
    among the others (A >= 8) ``nan_signal`` present symbols carry a NaN and ``absent`` have no row."""
    rng = np.random.default_rng(seed)
    common = rng.standard_normal((Dr, 1))
    scale = rng.uniform(0.3, 2.0, A)
    R0 = np.ascontiguousarray(0.01 * (0.6 * common + rng.standard_normal((Dr, A)) * scale))
    x = rng.standard_normal(A)
    x[rng.random(A) < zero_frac] = 0.0
    x[:min_leg] = np.abs(x[:min_leg]) + 0.1
    x[min_leg:2 * min_leg] = -np.abs(x[min_leg:2 * min_leg]) - 0.1
    present = np.ones(A, dtype=np.uint8)
    free = 2 * min_leg + rng.permutation(A - 2 * min_leg)
    if A >= 8:
        x[free[:nan_signal]] = np.nan
        present[free[nan_signal:nan_signal + absent]] = 0
    return R0, x, present


def spec_window(returns: pd.Series, symbols, date, lookback: int) -> np.ndarray:
    """The [T][len(symbols)] returns window of ``date`` (:315-346): rows of the day's symbols
    dated before ``date``, the last ``lookback`` distinct dates among THOSE rows, missing
    cells and NaN as 0.  None when there is no such row."""
    symbols = list(symbols)
    dl = returns.index.get_level_values(0)
    sl = returns.index.get_level_values(1)
    keep = np.asarray(sl.isin(symbols)) & np.asarray(dl < date)
    if not keep.any():
        return None
    dates = np.unique(dl[keep].values)[-lookback:]
    out = np.zeros((len(dates), len(symbols)))
    sub = returns[keep]
    dcode = pd.Index(dates).get_indexer(sub.index.get_level_values(0))
    scode = pd.Index(symbols).get_indexer(sub.index.get_level_values(1))
    v = sub.to_numpy(dtype=float)
    ok = (dcode >= 0) & np.isfinite(v)
    out[dcode[ok], scode[ok]] = v[ok]
    return out


def sigma_from_window(Xw: np.ndarray, s: float) -> np.ndarray:
    """Sigma over all the window's columns (:349-374)."""
    T = Xw.shape[0]
    c = Xw - Xw.mean(axis=0)
    with np.errstate(all="ignore"):
        C = (c.T @ c) / (T - 1)
    C = C + 1e-6 * np.eye(C.shape[0])
    if s <= 0:
        return C
    return (1.0 - s) * C + s * np.mean(np.diag(C)) * np.eye(C.shape[0])


def sigma_times(Xw: np.ndarray, s: float, w: np.ndarray) -> np.ndarray:
    """sigma_from_window(Xw, s) @ w without forming the matrix (thousands of columns)."""
    T = Xw.shape[0]
    c = Xw - Xw.mean(axis=0)
    dg = (c * c).sum(axis=0) / (T - 1) + 1e-6
    Cw = c.T @ (c @ w) / (T - 1) + 1e-6 * w
    return Cw if s <= 0 else (1.0 - s) * Cw + s * dg.mean() * w


def spec_sigma(returns, symbols, date, lookback, s):
    Xw = spec_window(returns, symbols, date, lookback)
    return None if Xw is None else sigma_from_window(Xw, s)


def signs(x, present=None):
    """+1 / -1 on the legs, 0 elsewhere (NaN and absent cells included)."""
    x = np.asarray(x, dtype=float)
    with np.errstate(invalid="ignore"):
        sg = np.where(x > 0, 1, np.where(x < 0, -1, 0))
    if present is not None:
        sg = np.where(np.asarray(present) != 0, sg, 0)
    return sg


def kkt_violation(q, w, sg, u):
    """(violation, scale) for q = 2 Sigma w restricted to the cells of w, sg their signs."""
    q, w, sg = (np.asarray(v) for v in (q, w, sg))
    viol = 0.0
    for leg, lo_end, hi_end in ((1, 0.0, u), (-1, -u, 0.0)):
        k = sg == leg
        g = -q[k]
        lo = np.where(w[k] == lo_end, -np.inf, 0.0)
        hi = np.where(w[k] == hi_end, np.inf, 0.0)
        a, b = np.max(lo - g), np.max(g - hi)
        if np.isfinite(a) and np.isfinite(b):
            viol = max(viol, 0.5 * (a + b))
    return viol, np.abs(q[sg != 0]).max()


def tight_slsqp(Sigma, sg, u):
    """The optimum over the cells of Sigma (signs sg; cells with sg == 0 stay 0)."""
    from scipy.optimize import minimize
    sg = np.asarray(sg)
    act = np.flatnonzero(sg != 0)
    S = Sigma[np.ix_(act, act)] / np.mean(np.diag(Sigma))
    s = sg[act]
    ep, en = (s > 0).astype(float), (s < 0).astype(float)
    x0 = ep / ep.sum() - en / en.sum()
    res = minimize(lambda w: w @ S @ w, x0, jac=lambda w: 2.0 * (S @ w), method="SLSQP",
                   bounds=[(0.0, u) if v > 0 else (-u, 0.0) for v in s],
                   constraints=[{"type": "eq", "fun": lambda w: ep @ w - 1.0, "jac": lambda w: ep},
                                {"type": "eq", "fun": lambda w: en @ w + 1.0, "jac": lambda w: en}],
                   options={"ftol": 1e-16, "maxiter": 5000})
    w = np.zeros(len(sg))
    w[act] = res.x
    return w
