#!/usr/bin/env python
"""The numpy model of k_risk_mvo_neutral (csrc/sim_mvo_risk.hip) in the kernel's own
algebra: no dense K^-1, only E^-1, the K x K matrices P, G, Q = I - P G, the Schur matrix of the
rows C = [e+; e-; B_N] swept legs first and then the neutral rows in factor order, and the loop
on (gv, t1, t2).  It is checked here against tests/risk_neutral_cases.neutral_model (the same
scheme with a dense K^-1) and prints both iteration counts:

    python tools/risk_neutral_model.py            # every case with A <= 200
    python tools/risk_neutral_model.py --max-a 1100

No GPU is used.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from risk_mvo_model import POWER_ITERS, RATIO_FLOOR, PIVOT_REL, psd_cholesky  # noqa: E402


def solve_day(Bc, Fc, s2, sg, u, N, max_iter=20000, eps=1e-9):
    """Bc [K][n] clean exposures, s2 [n], sg [n] in {+1, -1} (active cells only), N the neutral
    factors.  Returns (w, status, iterations, dropped rows)."""
    K, n = Bc.shape
    npos, nneg = (sg > 0).sum(), (sg < 0).sum()
    x0 = np.where(sg > 0, 1.0 / npos, -1.0 / nneg)
    L, bad = psd_cholesky(Fc)
    if bad:
        return x0, 2, 0, []
    if n > K:
        rho = 2.0 * s2.max()
    else:
        C0 = L.T @ (Bc @ Bc.T) @ L
        v = 1.0 + 0.01 * ((np.arange(K) * 37) % 11)
        lmax = 0.0
        for _ in range(POWER_ITERS):
            t = C0 @ v
            vv, tt = v @ v, t @ t
            lmax = np.sqrt(tt / vv) if vv > 0 else 0.0
            v = t / np.sqrt(tt) if tt > 0 else 0.0 * t
        l_lo, l_hi = 2.0 * s2.min(), 2.0 * s2.max() + 2.0 * lmax
        rho = l_hi * np.sqrt(l_lo / l_hi if l_lo > RATIO_FLOOR * l_hi else RATIO_FLOOR)
    ie = 1.0 / (2.0 * s2 + rho)
    G = (Bc * ie) @ Bc.T
    P = L @ np.linalg.inv(0.5 * np.eye(K) + L.T @ G @ L) @ L.T
    ep_, en_ = (sg > 0).astype(float), (sg < 0).astype(float)

    def kapply(vv):
        gv = Bc @ (vv * ie)
        return ie * (vv - Bc.T @ (P @ gv)), gv
    (pp, gp), (pn, gn) = kapply(ep_), kapply(en_)
    a11, a12, a22 = ep_ @ pp, ep_ @ pn, en_ @ pn
    rdet = 1.0 / (a11 * a22 - a12 * a12)
    ai11, ai12, ai22 = a22 * rdet, -a12 * rdet, a11 * rdet
    Q = np.eye(K) - P @ G
    H = G @ Q
    sp, sn, d0 = Q.T @ gp, Q.T @ gn, np.diag(H).copy()
    bmax = np.abs(Bc).max(axis=1)
    inN = np.array([k in N and bmax[k] > 0 for k in range(K)])
    if not (np.isfinite(H[np.ix_(inN, inN)]).all() and np.isfinite(sp[inN]).all() and np.isfinite(sn[inN]).all()
            and np.isfinite([ai11, ai12, ai22]).all()):
        return x0, 2, 0, []
    X = H - (np.outer(sp, ai11 * sp + ai12 * sn) + np.outer(sn, ai12 * sp + ai22 * sn))
    kept = np.zeros(K, dtype=bool)
    for k in np.flatnonzero(inN):
        row = X[k].copy()
        piv, tol = row[k], PIVOT_REL * abs(d0[k])
        if piv < -tol or not np.isfinite(piv):
            return x0, 2, 0, []
        if not piv > tol:
            continue
        kept[k] = True
        ip = 1.0 / piv
        X = X - np.outer(row * ip, row)
        X[k, :] = row * ip
        X[:, k] = row * ip
        X[k, k] = -ip
    T = np.where(np.outer(kept, kept), -X, 0.0)
    tp, tn = T @ sp, T @ sn
    w11, w12, w22 = sp @ tp, sp @ tn, sn @ tn
    m11, m12 = ai11 * w11 + ai12 * w12, ai11 * w12 + ai12 * w22
    m21, m22 = ai12 * w11 + ai22 * w12, ai12 * w12 + ai22 * w22
    s11, s12, s22 = ai11 + (m11 * ai11 + m12 * ai12), ai12 + (m11 * ai12 + m12 * ai22), ai22 + (m21 * ai12 + m22 * ai22)
    cp, cn = Q @ -(tp * ai11 + tn * ai12), Q @ -(tp * ai12 + tn * ai22)
    Pn = P + Q @ (T @ Q.T)
    lo, hi = np.where(sg > 0, 0.0, -u), np.where(sg > 0, u, 0.0)
    z, y = x0.copy(), np.zeros(n)
    st, it = 1, 0
    while it < max_iter:
        it += 1
        b = rho * (z - y)
        gv = Bc @ (b * ie)
        r1, r2 = pp @ b - 1.0, pn @ b + 1.0
        hv = Pn.T @ gv + cp * r1 + cn * r2
        nup, nun = cp @ gv + s11 * r1 + s12 * r2, cn @ gv + s12 * r1 + s22 * r2
        x = (b - Bc.T @ hv) * ie - nup * pp - nun * pn
        zn = np.clip(x + y, lo, hi)
        rp = np.abs(x - zn).max()
        rd = rho * np.abs(zn - z).max()
        y = x + y - zn
        z = zn
        eb = max(abs(z[sg > 0].sum() - 1.0), abs(z[sg < 0].sum() + 1.0))
        if rp <= eps and eb <= 0.1 * eps and rd <= eps * max(abs(nup), abs(nun)):
            if inN.any() and (np.abs(Bc[inN] @ z) / bmax[inN]).max() > eps:
                continue
            st = 0
            break
    return z, st, it, [int(k) for k in np.flatnonzero(inN) if not kept[k]]


def main():
    import risk_model_cases as RC
    import risk_neutral_cases as NC
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-a", type=int, default=200)
    a = ap.parse_args()
    for case in NC.NEUTRAL_CASES:
        c, N, feas = case
        if c[0] > a.max_a:
            continue
        for j in range(2):
            Bc, Fc, s2, sg, _, _ = NC.day(c, j)
            mi = 20000 if feas[j] else 2000
            w, st, it, dropped = solve_day(Bc, Fc, s2, sg, c[2], N, max_iter=mi)
            wd, std, itd, _ = NC.neutral_model(RC.sigma(Bc, Fc, s2), Bc, s2, sg, c[2], N, max_iter=mi)
            wu, stu, itu, _ = NC.neutral_model(RC.sigma(Bc, Fc, s2), Bc, s2, sg, c[2], (), max_iter=mi)
            print(f"{NC.case_id(case)} date {j}: status {st} ({std} dense), {it} iterations ({itd} dense, {itu} un-neutral), "
                  f"dropped {dropped}, max |w - w_dense| {np.abs(w - wd).max():.2e}, "
                  f"worst |B_k.w| {max((abs(Bc[k] @ w) for k in N), default=0.0):.2e}", flush=True)


if __name__ == "__main__":
    main()
