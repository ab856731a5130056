"""Host-side oracles of the factor-neutral MVO books (test_risk_neutral_host.py,
test_gpu_risk_neutral.py).  numpy / scipy only, written from the specification:

    min w'Sigma w   s.t.  sum_pos w = 1, sum_neg w = -1, B_k . w = 0 for k in N,
                          0 <= w <= u on pos, -u <= w <= 0 on neg

on the day's active cells, Sigma = B'F B + diag(s2) (risk_model_cases.sigma).

* ``neutral_model``: the kernel's scheme with a dense K^-1 = (2 Sigma + rho I)^-1: the ADMM of
  DESIGN 26 whose x-step carries the rows C = [e+; e-; B_N] exactly, the Schur matrix
  S = C K^-1 C' eliminated legs first and then the neutral rows in factor order (a pivot at or
  below 1e-10 of the row's diagonal entry drops the row, a negative one or a non-finite entry is
  the x0 fallback), the stop rule with the neutrality confirmation;
* ``feasible``: a linprog feasibility problem;
* ``kkt_violation_eq``: the exact min-max certificate as a small LP over (nu, t);
* ``tight_slsqp_eq``: ``sim_mvo_cases.tight_slsqp`` with the extra equality rows;
* ``NEUTRAL_CASES``: the cases on ``risk_model_cases.mvo_case`` with their feasibility.
"""
import numpy as np

import risk_model_cases as RC

PIVOT_REL = 1e-10           # RMV_PIVOT_REL
RATIO_FLOOR = 1e-3          # SMV_RATIO_FLOOR

# ((A, K, u, variant), N, (feasible on date 0, on date 1))
ALL8, ALL32 = tuple(range(8)), tuple(range(32))
NEUTRAL_CASES = [
    ((12, 12, 0.3, None), (0,), (True, True)),            # n <= K: section 14's rho
    ((40, 8, 0.1, None), (0,), (True, True)),
    ((40, 8, 0.1, None), ALL8, (False, True)),            # a status-1 and a status-0 date in one call
    ((63, 8, 0.1, None), (0, 3, 7), (True, True)),
    ((64, 8, 0.1, None), (0, 3, 7), (True, True)),
    ((65, 8, 0.1, None), (0, 3, 7), (True, True)),
    ((200, 32, 0.03, None), ALL32, (True, True)),         # m = 34 rows, the cap
    ((1100, 6, 0.03, None), (0, 1), (True, True)),
    ((4100, 5, 0.03, None), (2,), (True, True)),
    ((8200, 4, 0.03, None), (0, 3), (True, True)),
    ((16384, 32, 0.03, None), ALL32, (True, True)),       # both caps, LDS at its limit
    ((12, 4, 0.3, "fc0"), (0,), (True, True)),            # L = 0, P = 0, Q = I
    ((40, 8, 0.1, "dup"), (0, 1), (True, True)),          # dependent rows: one dropped
    ((40, 8, 0.1, "spread"), (0, 1, 2), (True, True)),
    ((9, 2, 0.5, None), (0,), (False, False)),
    ((12, 4, 0.3, None), (0, 1), (False, False)),
]


def case_id(c):
    (A, K, u, variant), N, _ = c
    return f"{A}-{K}-{u}-{variant}-N{len(N)}"


def day(case, j):
    """One date of a case on its active cells: (Bc [K][n], Fc, s2 [n], sg [n], act [A] bool, model row)."""
    B, Fc, S2, X, P, mrow = RC.mvo_case(*case)
    r = mrow[j]
    sg = RC.signs(X[j], P[j])
    act = sg != 0
    return RC.clean_b(B[:, r])[:, act], Fc[r], S2[r][act], sg[act], act, r


def constraint_rows(Bc, sg, N):
    """C [2 + |N|][n] and d."""
    C = np.vstack([(sg > 0).astype(float), (sg < 0).astype(float)] + [Bc[k] for k in N])
    return C, np.concatenate([[1.0, -1.0], np.zeros(len(N))])


def box(sg, u):
    return np.where(sg > 0, 0.0, -u), np.where(sg > 0, u, 0.0)


def feasible(Bc, sg, u, N):
    from scipy.optimize import linprog
    C, d = constraint_rows(Bc, sg, N)
    lo, hi = box(sg, u)
    res = linprog(np.zeros(len(sg)), A_eq=C, b_eq=d, bounds=list(zip(lo, hi)), method="highs")
    return res.status == 0


def kkt_violation_eq(g, w, sg, u, C):
    """(violation, scale) for g = 2 Sigma w on the active cells and the equality rows C: the
    smallest t for which some nu has |g + C'nu| <= t strictly inside the box, >= -t at the
    box's lower end and <= t at its upper end."""
    from scipy.optimize import linprog
    g, w, sg = (np.asarray(v, dtype=float) for v in (g, w, sg))
    lo, hi = box(sg, u)
    at_lo, at_hi = w == lo, w == hi
    m = C.shape[0]
    scale = np.abs(g).max()
    gs, Ct = g / scale, C.T
    rows, rhs = [], []
    up = ~at_lo           # g + C'nu <= t  unless at the lower end
    dn = ~at_hi           # g + C'nu >= -t unless at the upper end
    rows.append(np.hstack([Ct[up], -np.ones((up.sum(), 1))]))
    rhs.append(-gs[up])
    rows.append(np.hstack([-Ct[dn], -np.ones((dn.sum(), 1))]))
    rhs.append(gs[dn])
    cost = np.zeros(m + 1)
    cost[m] = 1.0
    res = linprog(cost, A_ub=np.vstack(rows), b_ub=np.concatenate(rhs), bounds=[(None, None)] * m + [(0.0, None)],
                  method="highs", options={"primal_feasibility_tolerance": 1e-10, "dual_feasibility_tolerance": 1e-10})
    assert res.status == 0, res.message
    # the LP's nu, evaluated in numpy: an upper bound of the minimum whatever the LP's own tolerances
    r = gs + Ct @ res.x[:m]
    viol = max(np.max(r[up], initial=0.0), np.max(-r[dn], initial=0.0))
    return viol * scale, scale


def tight_slsqp_eq(Sigma, sg, u, C):
    """The optimum over the active cells (Sigma, sg and C on those cells)."""
    from scipy.optimize import minimize
    S = Sigma / np.mean(np.diag(Sigma))
    ep, en = (sg > 0).astype(float), (sg < 0).astype(float)
    d = np.concatenate([[1.0, -1.0], np.zeros(C.shape[0] - 2)])
    first = [i for i in range(C.shape[0]) if not any(np.array_equal(C[i], C[j]) for j in range(i))]
    C, d = C[first], d[first]                      # SLSQP's QP needs independent rows ('dup')
    sc = np.maximum(np.abs(C).max(axis=1), 1e-300)
    cons = [{"type": "eq", "fun": (lambda w, r=C[i] / sc[i], t=d[i] / sc[i]: r @ w - t),
             "jac": (lambda w, r=C[i] / sc[i]: r)} for i in range(C.shape[0])]
    res = minimize(lambda w: w @ S @ w, ep / ep.sum() - en / en.sum(), jac=lambda w: 2.0 * (S @ w), method="SLSQP",
                   bounds=[(0.0, u) if v > 0 else (-u, 0.0) for v in sg], constraints=cons,
                   options={"ftol": 1e-16, "maxiter": 5000})
    return res.x


def model_rho(Sigma, s2, K):
    """DESIGN 26's rho: the top of the bulk with more cells than factors, else section 14's
    sqrt(l_min l_max) (the factor part's l_max exactly, where the kernel takes 32 power steps)."""
    n = len(s2)
    if n > K:
        return 2.0 * s2.max()
    lmax = max(np.linalg.eigvalsh(Sigma - np.diag(s2)).max(), 0.0)
    l_lo, l_hi = 2.0 * s2.min(), 2.0 * s2.max() + 2.0 * lmax
    ratio = l_lo / l_hi if l_lo > RATIO_FLOOR * l_hi else RATIO_FLOOR
    return l_hi * np.sqrt(ratio)


def schur_kept(S, nrow_ok):
    """Elimination order and the drop rule: (kept row indices, bad).  Rows 0 and 1 (the legs)
    first, then the neutral rows in order; ``nrow_ok[i]`` False drops neutral row i up front."""
    if not np.isfinite(S).all():
        return [], True
    kept = [0, 1]
    for r in range(2, S.shape[0]):
        if not nrow_ok[r - 2]:
            continue
        piv = S[r, r] - S[r, kept] @ np.linalg.solve(S[np.ix_(kept, kept)], S[kept, r])
        tol = PIVOT_REL * abs(S[r, r])
        if piv < -tol:
            return kept, True
        if piv > tol:
            kept.append(r)
    return kept, False


def neutral_model(Sigma, Bc, s2, sg, u, N, max_iter=20000, eps=1e-9, confirm=True):
    """Returns (w, status, iterations, info dict).  ``confirm=False`` leaves the neutrality
    confirmation out of the stop rule (to count what it costs)."""
    K, n = Bc.shape
    N = list(N)
    npos, nneg = (sg > 0).sum(), (sg < 0).sum()
    x0 = np.where(sg > 0, 1.0 / npos, -1.0 / nneg)
    rho = model_rho(Sigma, s2, K)
    info = {"rho": rho, "dropped": [], "checks": 0}
    if not (np.isfinite(Sigma).all() and rho > 0 and np.isfinite(rho)):
        return x0, 2, 0, info
    Kinv = np.linalg.inv(2.0 * Sigma + rho * np.eye(n))
    C, d = constraint_rows(Bc, sg, N)
    bmax = np.abs(C[2:]).max(axis=1) if N else np.zeros(0)
    KC = Kinv @ C.T
    kept, bad = schur_kept(C @ KC, bmax > 0)
    if bad:
        return x0, 2, 0, info
    info["dropped"] = [N[r - 2] for r in range(2, C.shape[0]) if r not in kept]
    Ck, dk, KCk = C[kept], d[kept], KC[:, kept]
    Sinv = np.linalg.inv(Ck @ KCk)
    chk = bmax > 0
    lo, hi = box(sg, u)
    z, y = x0.copy(), np.zeros(n)
    st, it = 1, 0
    while it < max_iter:
        it += 1
        b = rho * (z - y)
        lam = Sinv @ (KCk.T @ b - dk)
        x = Kinv @ b - KCk @ lam
        zn = np.clip(x + y, lo, hi)
        rp = np.abs(x - zn).max()
        rd = rho * np.abs(zn - z).max()
        y = x + y - zn
        z = zn
        eb = max(abs(z[sg > 0].sum() - 1.0), abs(z[sg < 0].sum() + 1.0))
        gs = max(abs(lam[0]), abs(lam[1]))
        if rp <= eps and eb <= 0.1 * eps and rd <= eps * gs:
            if confirm and chk.any():
                info["checks"] += 1
                if (np.abs(C[2:][chk] @ z) / bmax[chk]).max() > eps:
                    continue
            st = 0
            break
    return z, st, it, info
