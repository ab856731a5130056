#!/usr/bin/env python
"""The numpy model of k_risk_mvo (csrc/sim_mvo_risk.hip): the same ADMM, Woodbury
x-step, rho and stopping rule, one date at a time on the host.  Run it over the cases of
tests/test_gpu_risk_model.py to see the iteration counts before the kernel does:

    python tools/risk_mvo_model.py            # every MVO case of the GPU test
    python tools/risk_mvo_model.py --floor 1e-2

No GPU is used.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

RATIO_FLOOR = 1e-3          # SMV_RATIO_FLOOR
PIVOT_REL = 1e-10           # the semidefinite Cholesky drops pivots <= PIVOT_REL * diagonal
POWER_ITERS = 32


def psd_cholesky(F):
    """(L lower with dropped columns zero, bad): bad when a pivot is negative beyond round-off."""
    K = F.shape[0]
    Mx = np.tril(F).copy()
    Mx = Mx + np.tril(Mx, -1).T
    L = np.zeros((K, K))
    W = Mx.copy()
    diag0 = np.diag(Mx).copy()
    for k in range(K):
        piv = W[k, k]
        tol = PIVOT_REL * abs(diag0[k])
        if piv < -tol or diag0[k] < 0:
            return L, True
        if not piv > tol:
            continue
        lkk = np.sqrt(piv)
        L[k:, k] = W[k:, k] / lkk
        L[k, k] = lkk
        W[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], L[k + 1:, k])
    return L, False


def solve_day(Bc, Fc, s2, sg, u, max_iter=20000, eps=1e-9, floor=RATIO_FLOOR, rho_fn=None, sec14=False):
    """Bc [K][n] clean exposures, s2 [n], sg [n] in {+1, -1} (active cells only).
    Returns (w, status, iterations, rp, rd, rho)."""
    K, n = Bc.shape
    npos, nneg = (sg > 0).sum(), (sg < 0).sum()
    x0 = np.where(sg > 0, 1.0 / npos, -1.0 / nneg)
    if not (np.isfinite(s2).all() and (s2 >= 0).all() and np.isfinite(np.tril(Fc)).all()):
        return x0, 2, 0, 0.0, 0.0, 0.0
    L, bad = psd_cholesky(Fc)
    if bad:
        return x0, 2, 0, 0.0, 0.0, 0.0
    C0 = L.T @ (Bc @ Bc.T) @ L
    v = 1.0 + 0.01 * ((np.arange(K) * 37) % 11)
    lmax = 0.0
    for _ in range(POWER_ITERS):
        t = C0 @ v
        vv, tt = v @ v, t @ t
        lmax = np.sqrt(tt / vv) if vv > 0 else 0.0
        v = t / np.sqrt(tt) if tt > 0 else 0.0 * t
    if n > K and not sec14:
        # the n - K bulk eigenvalues of 2 Sigma lie in [2 min s2, 2 max s2]; the <= K outliers the
        # x-step inverts exactly are left out of rho (section 14's rule stalls here)
        rho = 2.0 * s2.max()
    else:
        l_lo, l_hi = 2.0 * s2.min(), 2.0 * s2.max() + 2.0 * lmax
        ratio = l_lo / l_hi if l_lo > floor * l_hi else floor
        rho = l_hi * np.sqrt(ratio)
    if rho_fn is not None:
        rho = rho_fn(s2, lmax)
    if not (rho > 0 and np.isfinite(rho)):
        return x0, 2, 0, 0.0, 0.0, rho
    ie = 1.0 / (2.0 * s2 + rho)
    Mm = 0.5 * np.eye(K) + L.T @ ((Bc * ie) @ Bc.T) @ L
    P = L @ np.linalg.inv(Mm) @ L.T

    def kapply(vv):
        t = vv * ie
        return t - ie * (Bc.T @ (P @ (Bc @ t)))
    ep_, en_ = (sg > 0).astype(float), (sg < 0).astype(float)
    pp, pn = kapply(ep_), kapply(en_)
    a11, a12, a22 = ep_ @ pp, ep_ @ pn, en_ @ pn
    rdet = 1.0 / (a11 * a22 - a12 * a12)
    lo, hi = np.where(sg > 0, 0.0, -u), np.where(sg > 0, u, 0.0)
    z, y = x0.copy(), np.zeros(n)
    st, it, rp, rd = 1, 0, 0.0, 0.0
    while it < max_iter:
        it += 1
        b = rho * (z - y)
        kb = kapply(b)
        r1, r2 = pp @ b - 1.0, pn @ b + 1.0
        nup, nun = (r1 * a22 - r2 * a12) * rdet, (a11 * r2 - a12 * r1) * rdet
        x = kb - nup * pp - nun * pn
        zn = np.clip(x + y, lo, hi)
        rp = np.abs(x - zn).max()
        rd = rho * np.abs(zn - z).max()
        y = x + y - zn
        z = zn
        eb = max(abs(z[sg > 0].sum() - 1.0), abs(z[sg < 0].sum() + 1.0))
        gs = max(abs(nup), abs(nun))
        done = rp <= eps and eb <= 0.1 * eps and rd <= eps * gs
        rp = max(rp, eb)
        rd = rd / gs if gs > 0 else rd
        if done:
            st = 0
            break
    return z, st, it, rp, rd, rho


def main():
    import risk_model_cases as RC
    ap = argparse.ArgumentParser()
    ap.add_argument("--floor", type=float, default=RATIO_FLOOR)
    ap.add_argument("--max-a", type=int, default=16384)
    ap.add_argument("--sec14", action="store_true", help="section 14's rho rule on every day (stalls; DESIGN 26)")
    a = ap.parse_args()
    for A, K, u, variant in RC.MVO_CASES:
        if A > a.max_a:
            continue
        B, Fc, S2, X, P, mrow = RC.mvo_case(A, K, u, variant)
        for j in range(2):
            r = mrow[j]
            sg = RC.signs(X[j], P[j])
            act = sg != 0
            Bc = RC.clean_b(B[:, r, :])[:, act]
            t0 = time.time()
            w, st, it, rp, rd, rho = solve_day(Bc, Fc[r], S2[r][act], sg[act], u, floor=a.floor, sec14=a.sec14)
            q = 2.0 * RC.sigma_times(Bc, Fc[r], S2[r][act], w)
            viol, scale = RC.kkt_violation(q, w, sg[act], u)
            print(f"({A}, {K}, {u}, {variant}) date {j}: status {st}, {it} iterations, residuals {rp:.2e} / {rd:.2e}, "
                  f"rho {rho:.3e}, KKT {viol:.2e} (bound {1e-6 * scale:.2e}) [{time.time() - t0:.1f} s]", flush=True)


if __name__ == "__main__":
    main()
