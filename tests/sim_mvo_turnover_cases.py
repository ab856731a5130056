"""Inputs and host-side checks shared by the mvo_turnover tests (test_sim_mvo_turnover_host.py,
test_gpu_sim_mvo_turnover.py).  Plain numpy / scipy, written from the specification of
``Simulation(method="mvo_turnover")`` (portfolio_simulation.py:96-154, :206-248, :463-585),
not from the kernel.  Windows, Sigma and signs come from sim_mvo_cases.

Per date, with p the chain's last book aligned to today's rows (0 where the symbol had no row
on the previous date, all zeros on the first date):

    min  w'Sigma w + tau sum |w_i - p_i| - r sum x_i w_i
    s.t. sum_pos w = 1, sum_neg w = -1, 0 <= w <= u on pos, -u <= w <= 0 on neg, 0 elsewhere

* ``kkt_violation_l1``: sim_mvo_cases.kkt_violation with each cell's interval widened by the
  subdifferential of tau |w_i - p_i|;
* ``post_solve``: the reference's prune / renormalise step (:553-573) with exactly rounded leg
  sums (math.fsum), which is what the kernel computes;
* ``align_prev`` / ``chain_step``: the p alignment and one date of the chain (exits included);
* ``admm_model``: a dense numpy model of the solver, used on the CPU only;
* ``slsqp_dominant`` / ``slsqp_split``: two independent optima for small n.
"""
import math

import numpy as np

import sim_mvo_cases as SC

PRUNE = 1e-6
RELAX = 1.6          # ADMM over-relaxation of the model


def box(sg, u):
    sg = np.asarray(sg)
    return np.where(sg > 0, 0.0, np.where(sg < 0, -u, 0.0)), np.where(sg > 0, u, 0.0)


def kkt_violation_l1(q, w, sg, u, p, tau):
    """(violation, scale) for q = 2 Sigma w - r x on the cells of w.  w is optimal iff each leg
    has a multiplier nu with -q_i - nu inside [lo_i, hi_i] for every cell of the leg, where
    [lo_i, hi_i] = tau d|w_i - p_i| ([tau, tau] above p_i, [-tau, -tau] below, [-tau, tau] at
    p_i), lo_i = -inf at the box's lower end and hi_i = +inf at its upper end.  The smallest
    achievable largest distance is max(0, (a + b) / 2), a = max(lo - g), b = max(g - hi)."""
    q, w, sg, p = (np.asarray(v, dtype=float) for v in (q, w, sg, p))
    viol = 0.0
    for leg, lo_end, hi_end in ((1, 0.0, u), (-1, -u, 0.0)):
        k = sg == leg
        g, wk, pk = -q[k], w[k], p[k]
        lo = np.where(wk > pk, tau, -tau)
        hi = np.where(wk < pk, -tau, tau)
        lo = np.where(wk == lo_end, -np.inf, lo)
        hi = np.where(wk == hi_end, np.inf, hi)
        a, b = np.max(lo - g), np.max(g - hi)
        if np.isfinite(a) and np.isfinite(b):
            viol = max(viol, 0.5 * (a + b))
    return viol, np.abs(q[sg != 0]).max()


def post_solve(w, sg):
    """:553-573 on a solved day: per leg |w| < 1e-6 -> 0; when both leg sums are then > 0 each
    leg is divided by its sum (math.fsum: rounded once), else the unpruned w is kept."""
    w, sg = np.asarray(w, dtype=float), np.asarray(sg)
    act = sg != 0
    o = np.where(act & (np.abs(w) < PRUNE), 0.0, w)
    dl, ds = math.fsum(np.abs(o[sg > 0])), math.fsum(np.abs(o[sg < 0]))
    if dl > 0 and ds > 0:
        o = o.copy()
        o[sg > 0] = o[sg > 0] / dl
        o[sg < 0] = o[sg < 0] / ds
        return o
    return w.copy()


def align_prev(prev_book, prev_present):
    """Yesterday's book on today's columns: its value where the symbol had a row, else 0."""
    if prev_book is None:
        return None
    prev_book = np.asarray(prev_book, dtype=float)
    ok = np.isfinite(prev_book) if prev_present is None else (np.asarray(prev_present) != 0)
    return np.where(ok, np.nan_to_num(prev_book), 0.0)


def day_status(x, present, T, u):
    """The exit decided before any solve: 3 flat, 4 no history, 2 x0, -1 a QP day."""
    sg = SC.signs(x, present)
    npos, nneg = int((sg > 0).sum()), int((sg < 0).sum())
    npres = len(sg) if present is None else int((np.asarray(present) != 0).sum())
    if npos == 0 or nneg == 0 or npres < 2:
        return 3
    if T == 0:
        return 4
    if T == 1 or u * npos < 1 - 1e-12 or u * nneg < 1 - 1e-12:
        return 2
    return -1


def x0_book(sg):
    sg = np.asarray(sg)
    return np.where(sg > 0, 1.0 / max((sg > 0).sum(), 1), np.where(sg < 0, -1.0 / max((sg < 0).sum(), 1), 0.0))


def admm_model(Sigma, sg, u, p, x, tau, r, eps=1e-9, max_iter=200000, warm=True):
    """(w, iterations, status) on the cells of Sigma: the scheme of DESIGN 16 with a dense K^-1."""
    sg = np.asarray(sg)
    act = sg != 0
    S2 = 2.0 * Sigma[np.ix_(act, act)]
    ev = np.linalg.eigvalsh(S2)
    rho = ev[-1] * np.sqrt(max(ev[0] / ev[-1], 1e-3))
    s = sg[act]
    n = len(s)
    Kinv = np.linalg.inv(S2 + rho * np.eye(n))
    ep, en = (s > 0).astype(float), (s < 0).astype(float)
    pp, pn = Kinv @ ep, Kinv @ en
    a11, a12, a22 = ep @ pp, ep @ pn, en @ pn
    rdet = 1.0 / (a11 * a22 - a12 * a12)
    lo, hi = box(s, u)
    pa = np.asarray(p, dtype=float)[act]
    xa = np.nan_to_num(np.asarray(x, dtype=float)[act])
    z = ep / ep.sum() - en / en.sum()
    k = tau / rho
    # y is the scaled dual minus its start y0 = sgn k per leg (sgn the way the leg's sum has to
    # move): in the x-step a constant on a leg only shifts the leg's multiplier, so y0 appears
    # in the dead zone [tlo, thi] of the soft threshold alone and never meets the small numbers
    y = np.zeros(n)
    sgn = np.zeros(n)
    if warm:
        cp = np.clip(pa, lo, hi)
        sgn = np.where(s > 0, np.sign(1.0 - cp[s > 0].sum()), np.sign(-1.0 - cp[s < 0].sum()))
    tlo, thi = -k * (1.0 + sgn), k * (1.0 - sgn)
    st = 1
    for it in range(1, max_iter + 1):
        b = r * xa + rho * (z - y)
        r1, r2 = pp @ b - 1.0, pn @ b + 1.0
        nup, nun = (r1 * a22 - r2 * a12) * rdet, (a11 * r2 - a12 * r1) * rdet
        xx = Kinv @ b - nup * pp - nun * pn
        gs = np.abs(rho * (z - y - xx) - np.where(s > 0, nup, nun)).max()
        xv = RELAX * xx + (1.0 - RELAX) * z + y
        d = xv - pa
        zn = np.clip(pa + np.where(d > thi, d - thi, np.where(d < tlo, d - tlo, 0.0)), lo, hi)
        rp, rd = np.abs(xx - zn).max(), rho * np.abs(zn - z).max()
        y, z = xv - zn, zn
        eb = max(abs(z[s > 0].sum() - 1.0), abs(z[s < 0].sum() + 1.0))
        if rp <= eps and eb <= 0.1 * eps and rd <= eps * gs:
            st = 0
            break
    w = np.zeros(len(sg))
    w[act] = z
    return w, it, st


def chain_step(Xw, x, present, prev_book, prev_present, u, s, tau, r, equal_book=None, solver=admm_model):
    """One date of the chain on the day's full column set: (book [A] with NaN on absent cells,
    wopt or None, status, p).  Xw is the [T][A] window (None or T = 0: no history)."""
    x = np.asarray(x, dtype=float)
    pr = np.ones(len(x), bool) if present is None else np.asarray(present) != 0
    sg = SC.signs(x, None if present is None else present)
    p = align_prev(prev_book, prev_present)
    p = np.zeros(len(x)) if p is None else np.where(pr, p, 0.0)
    T = 0 if Xw is None else Xw.shape[0]
    st = day_status(x, present, T, u)
    wopt = None
    if st == 3:
        book = np.zeros(len(x))
    elif st == 4:
        book = np.nan_to_num(np.asarray(equal_book, dtype=float))
    elif st == 2:
        book = x0_book(sg)
    else:
        Sig = SC.sigma_from_window(Xw[:, pr], s)
        w, _, st = solver(Sig, sg[pr], u, p[pr], x[pr], tau, r)
        wopt = np.zeros(len(x))
        wopt[pr] = w
        book = post_solve(wopt, sg)
        wopt = np.where(pr, wopt, np.nan)
    return np.where(pr, book, np.nan), wopt, st, p


def _slsqp(S, lin, s, lo, hi, x0):
    from scipy.optimize import minimize
    ep, en = (s > 0).astype(float), (s < 0).astype(float)
    res = minimize(lambda w: w @ S @ w - lin @ w, x0, jac=lambda w: 2.0 * (S @ w) - lin, method="SLSQP",
                   bounds=list(zip(lo, hi)),
                   constraints=[{"type": "eq", "fun": lambda w: ep @ w - 1.0, "jac": lambda w: ep},
                                {"type": "eq", "fun": lambda w: en @ w + 1.0, "jac": lambda w: en}],
                   options={"ftol": 1e-16, "maxiter": 5000})
    return res.x


def slsqp_dominant(Sigma, sg, u, p, x, r):
    """The optimum when tau dominates (2 tau > the spread of q over each leg): the L1 term is then
    constant on the optimal face and the problem is the plain box QP with tightened bounds: a leg
    whose sum of clip(p) is below its target keeps w >= clip(p), one above it keeps w <= clip(p)."""
    sg = np.asarray(sg)
    act = np.flatnonzero(sg != 0)
    sc = 1.0 / np.mean(np.diag(Sigma))
    s = sg[act]
    lo, hi = box(s, u)
    cp = np.clip(np.asarray(p, dtype=float)[act], lo, hi)
    for leg, target in ((1, 1.0), (-1, -1.0)):
        k = s == leg
        if cp[k].sum() < target:
            lo = np.where(k, cp, lo)
        elif cp[k].sum() > target:
            hi = np.where(k, cp, hi)
        else:
            lo, hi = np.where(k, cp, lo), np.where(k, cp, hi)
    x0 = np.clip((s > 0) / max((s > 0).sum(), 1) - (s < 0) / max((s < 0).sum(), 1), lo, hi)
    w = np.zeros(len(sg))
    w[act] = _slsqp(Sigma[np.ix_(act, act)] * sc, r * sc * np.nan_to_num(np.asarray(x, dtype=float)[act]), s, lo, hi, x0)
    return w


def slsqp_split(Sigma, sg, u, p, x, tau, r):
    """The optimum by the split w = p + a - b, a, b >= 0 (smooth; reliable for small tau only)."""
    from scipy.optimize import minimize
    sg = np.asarray(sg)
    act = np.flatnonzero(sg != 0)
    sc = 1.0 / np.mean(np.diag(Sigma))
    S = Sigma[np.ix_(act, act)] * sc
    s = sg[act]
    n = len(s)
    lo, hi = box(s, u)
    pa = np.asarray(p, dtype=float)[act]
    lin = r * sc * np.nan_to_num(np.asarray(x, dtype=float)[act])
    t = tau * sc
    ep, en = (s > 0).astype(float), (s < 0).astype(float)
    D = np.hstack([np.eye(n), -np.eye(n)])

    def f(v):
        w = pa + D @ v
        return w @ S @ w - lin @ w + t * v.sum()

    def g(v):
        w = pa + D @ v
        return D.T @ (2.0 * (S @ w) - lin) + t
    w0 = np.clip(ep / ep.sum() - en / en.sum(), lo, hi)
    v0 = np.r_[np.maximum(w0 - pa, 0.0), np.maximum(pa - w0, 0.0)]
    cons = [{"type": "eq", "fun": lambda v: ep @ (pa + D @ v) - 1.0, "jac": lambda v: ep @ D},
            {"type": "eq", "fun": lambda v: en @ (pa + D @ v) + 1.0, "jac": lambda v: en @ D},
            {"type": "ineq", "fun": lambda v: pa + D @ v - lo, "jac": lambda v: D},
            {"type": "ineq", "fun": lambda v: hi - pa - D @ v, "jac": lambda v: -D}]
    res = minimize(f, v0, jac=g, method="SLSQP", bounds=[(0.0, None)] * (2 * n), constraints=cons,
                   options={"ftol": 1e-16, "maxiter": 5000})
    w = np.zeros(len(sg))
    w[act] = pa + D @ res.x
    return w


def leg_spread(q, sg):
    """The largest spread of q over a leg (the dominant regime needs 2 tau above it)."""
    q, sg = np.asarray(q), np.asarray(sg)
    return max(np.ptp(q[sg == leg]) for leg in (1, -1) if (sg == leg).any())


def make_chain(A, T, J, seed, ragged=False, flip=0.1, u=None):
    """(R0 [T + J][A], rows [J][T], X [J][A], P [J][A] uint8, u): J chained dates whose windows
    slide over one returns panel; the signal changes sign on ``flip`` of the cells each day, so
    yesterday's book falls outside today's box there.  The first 2 * min_leg symbols keep their
    sign and their rows, so every day stays a feasible QP.  ``ragged``: other symbols enter and
    leave (absent cells carry a NaN signal)."""
    u = min(1.0, 6.0 / A) if u is None else u
    ml = int(np.ceil(1.0 / u)) if u < 1 else 1
    R0, x, _ = SC.make_panel(T + J, A, seed, nan_signal=1 if A >= 8 else 0, min_leg=ml)
    rng = np.random.default_rng(seed + 7)
    X, P = [x], []
    for j in range(1, J):
        f = rng.random(A) < flip
        f[:2 * ml] = False
        X.append(np.where(f, -X[-1], X[-1]))
    for j in range(J):
        pr = np.ones(A, dtype=np.uint8)
        if ragged and A > 2 * ml:
            gone = 2 * ml + np.flatnonzero(rng.random(A - 2 * ml) < 0.25)
            pr[gone] = 0
        P.append(pr)
    X, P = np.stack(X), np.stack(P)
    rows = np.stack([np.arange(j, j + T) for j in range(J)]).astype(np.int32)
    return R0, rows, np.where(P != 0, X, np.nan), P, u
