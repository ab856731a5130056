"""Native ``Simulation(method="mvo_turnover")`` on the GPU: fmx_sim_mvo_turnover_books behind
``engine.sim_mvo_turnover_books``, ``simulation.mvo_turnover_trade_list`` and the routing in
``Simulation._daily_trade_list`` (FMX_SIM_MVO_TURNOVER=native).

The reference's cvxpy loop cannot run here and stops at eps 1e-4, so the specification is the
exact optimum of each day's L1-penalised QP given the previous book the kernel itself returned:
certified by the KKT conditions in numpy (sim_mvo_turnover_cases.kkt_violation_l1) on ``Wopt``,
cross-checked against two independent SLSQP forms on the small cases, and the chain semantics
(p alignment, exits, prune / renormalise) against the numpy stepper.  Every chain has 4 dates
(2 at the caps) whose signal changes sign on a tenth of the cells each day.
Each test prints the figures it asserts on (DESIGN 16 records them).
"""
import functools
import logging
import math
import sys

import numpy as np
import pandas as pd
import pytest

import sim_mvo_cases as SC
import sim_mvo_turnover_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 0.1                      # shrinkage
TAU_MIXED, R_MIXED = 1e-6, 1e-4


def _engine():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import factormodeling_amd.engine as E
    return E, torch


# (A, T, J, ragged).  (3, 4) has T > n, 257 is the first width on 512 threads, 1025 / 2100 take 2 / 4
# elements per thread (4: the first width that spills), T = 64 is the window cap and at
# (16384, 64) the T x T matrix is read from the workspace instead of the LDS.
SHAPES = [(3, 4, 4, False), (9, 5, 4, False), (40, 20, 4, False), (40, 20, 4, True), (200, 64, 4, False),
          (257, 10, 4, True), (1025, 16, 4, False), (2100, 32, 4, False), (16384, 64, 2, False)]
REGIMES = {"dominant": (0.1, 0.0), "mixed": (TAU_MIXED, R_MIXED)}
# At the caps only the mixed regime runs: the dominant one needs 10,558 iterations there (9 s).
CASES = [(sh, rg) for sh in SHAPES for rg in REGIMES if not (sh[0] == 16384 and rg == "dominant")]
_IDS = ["-".join(str(v) for v in sh) + "-" + rg for sh, rg in CASES]


@functools.lru_cache(maxsize=None)
def _inputs(A, T, J, ragged):
    return TC.make_chain(A, T, J, 1000 * A + T, ragged=ragged)


def _call(E, torch, R0, rows, Tn, X, P, u, tau, r, W=None, **kw):
    out = E.sim_mvo_turnover_books(torch.as_tensor(R0, device=DEV), rows, Tn, torch.as_tensor(X, device=DEV),
                                   None if P is None else torch.as_tensor(P, device=DEV),
                                   None if W is None else torch.as_tensor(W, device=DEV), S, u, tau, r,
                                   return_opt=True, **kw)
    return [t.cpu().numpy() for t in out]


@functools.lru_cache(maxsize=None)
def _solved(shape, regime):
    E, torch = _engine()
    A, T, J, ragged = shape
    R0, rows, X, P, u = _inputs(*shape)
    tau, r = REGIMES[regime]
    W, counts, info, Wopt = _call(E, torch, R0, rows, np.full(J, T, dtype=np.int32), X, P, u, tau, r)
    return W[0], counts[0], info[0], Wopt[0]


def _certify(R0, rows_j, x, pres, w, p, u, tau, r):
    """(violation, scale, q) of date j's QP at w [A] given p [A] (full width, NaN-free on present cells)."""
    pr = pres != 0
    sg = SC.signs(x, pres)
    q = 2.0 * SC.sigma_times(R0[rows_j][:, pr], S, w[pr]) - r * np.nan_to_num(x[pr])
    viol, scale = TC.kkt_violation_l1(q, w[pr], sg[pr], u, p[pr], tau)
    return viol, scale, q


# ---------------------------------------------------------------------------- 1. optimality
@pytest.mark.parametrize("shape,regime", CASES, ids=_IDS)
def test_kkt_certificate_and_chain(shape, regime):
    A, T, J, ragged = shape
    R0, rows, X, P, u = _inputs(*shape)
    tau, r = REGIMES[regime]
    W, counts, info, Wopt = _solved(shape, regime)
    for j in range(J):
        pr = P[j] != 0
        sg = SC.signs(X[j], P[j])
        p = np.zeros(A) if j == 0 else TC.align_prev(W[j - 1], P[j - 1])
        w = Wopt[j]
        viol, scale, q = _certify(R0, rows[j], X[j], P[j], w, p, u, tau, r)
        sp, sn = math.fsum(w[sg > 0]), math.fsum(w[sg < 0])
        print(f"{shape} {regime} date {j}: status {info[j, 0]:.0f}, {info[j, 1]:.0f} iterations, residuals "
              f"{info[j, 2]:.2e} / {info[j, 3]:.2e}, rho {info[j, 5]:.3e}, leg sums - 1: {sp - 1:.2e} {-sn - 1:.2e}, "
              f"{int(((w != p) & (sg != 0)).sum())} of {int((sg != 0).sum())} cells moved, KKT violation {viol:.3e} "
              f"(bound {1e-6 * scale:.3e})")
        assert info[j, 0] == 0
        assert np.isnan(w[~pr]).all() and not np.isnan(w[pr]).any()
        assert abs(sp - 1.0) <= 1e-10 and abs(sn + 1.0) <= 1e-10
        assert (w[sg > 0] >= 0.0).all() and (w[sg > 0] <= u).all()
        assert (w[sg < 0] <= 0.0).all() and (w[sg < 0] >= -u).all()
        assert (w[pr & (sg == 0)] == 0.0).all()
        assert counts[j, 0] == (sg > 0).sum() and counts[j, 1] == (sg < 0).sum()
        assert viol <= 1e-6 * scale
        # the book is the reference's post-solve step on Wopt, bit for bit: the kernel's leg sums
        # are exactly rounded (as math.fsum), so no reduction order enters, and the division is IEEE
        want = np.where(pr, TC.post_solve(np.nan_to_num(w), sg), np.nan)
        assert W[j].tobytes() == want.tobytes()
        if A <= 40:
            Sig = SC.sigma_from_window(R0[rows[j]][:, pr], S)
            if regime == "dominant":
                spread = TC.leg_spread(q, sg[pr])
                assert 2.0 * tau > spread, "the tightened-bounds form needs a dominant tau"
                ref = TC.slsqp_dominant(Sig, sg[pr], u, p[pr], X[j][pr], r)
            else:
                ref = TC.slsqp_split(Sig, sg[pr], u, p[pr], X[j][pr], tau, r)
            err = np.abs(w[pr] - ref).max()
            print(f"{shape} {regime} date {j}: max |w - w_slsqp| = {err:.3e}")
            assert err <= 1e-6


def test_mixed_regime_moves_a_leg_both_ways():
    """On the numpy spec solution (no GPU involved) some leg has up- and down-movers at the mixed
    tau, so the certificate above sees all three branches of the subdifferential; the kernel's
    books agree with that chain to the solver's tolerance."""
    shape = (40, 20, 4, False)
    R0, rows, X, P, u = _inputs(*shape)
    both, prev, worst = 0, None, 0.0
    W, _, _, Wopt = _solved(shape, "mixed")
    for j in range(4):
        book, wopt, st, p = TC.chain_step(R0[rows[j]], X[j], P[j], prev, None if j == 0 else P[j - 1], u, S,
                                          TAU_MIXED, R_MIXED)
        sg = SC.signs(X[j], P[j])
        for leg in (1, -1):
            k = sg == leg
            both += bool(j > 0 and (wopt[k] > p[k]).any() and (wopt[k] < p[k]).any())
        worst = max(worst, np.abs(wopt - Wopt[j]).max())
        prev = book
    print(f"legs with movers both ways: {both}; largest |w_model - w_kernel| over the chain {worst:.2e}")
    assert both >= 1
    assert worst <= 1e-6


# ---------------------------------------------------------------------------- 2. chain semantics
def test_flat_equal_and_x0_days_become_the_next_p():
    E, torch = _engine()
    A, T = 40, 6
    R0, rows, X, P, u = TC.make_chain(A, T, 7, 91, ragged=True)
    X[1] = np.where(P[1] != 0, np.abs(np.nan_to_num(X[1])) + 0.01, np.nan)        # date 1: one leg only -> flat
    Tn = np.array([T, T, T, 0, T, 1, T], dtype=np.int32)                           # date 3: no history; date 5: one row
    _, ce, we = E.trade_books(torch.as_tensor(X[None], device=DEV), "equal", 0.3, u, present=torch.as_tensor(P, device=DEV),
                              nan_absent=False, raw=True)
    eq = we[0].cpu().numpy()
    W0 = np.zeros((1, 7, A))
    W0[0, 3] = eq[3]
    tau, r = 0.1, 0.0
    W, counts, info, Wopt = (v[0] for v in _call(E, torch, R0, rows, Tn, X, P, u, tau, r, W=W0))
    assert list(info[:, 0]) == [0, 3, 0, 4, 0, 2, 0]
    sg5 = SC.signs(X[5], P[5])
    assert np.array_equal(np.nan_to_num(W[1]), np.zeros(A)) and list(counts[1]) == [0, 0]
    assert W[3].tobytes() == eq[3].tobytes() and list(counts[3]) == [0, 0]         # the caller's row, untouched
    assert np.array_equal(np.nan_to_num(W[5]), np.where(P[5] != 0, TC.x0_book(sg5), 0.0))
    assert list(counts[5]) == [(sg5 > 0).sum(), (sg5 < 0).sum()]
    for j in (1, 3, 5):
        assert np.array_equal(np.isnan(W[j]), P[j] == 0)
        assert np.array_equal(np.nan_to_num(Wopt[j]), np.nan_to_num(W[j]))
    for j in (2, 4, 6):                                                            # the day after each of them
        p = TC.align_prev(W[j - 1], P[j - 1])
        viol, scale, _ = _certify(R0, rows[j], X[j], P[j], Wopt[j], p, u, tau, r)
        sg = SC.signs(X[j], P[j])
        stay = int(((Wopt[j] == p) & (sg != 0)).sum())
        print(f"date {j} after status {info[j - 1, 0]:.0f}: {stay} cells stay at p, KKT violation {viol:.3e} "
              f"(bound {1e-6 * scale:.3e})")
        assert viol <= 1e-6 * scale
        # with another p the certificate fails: the check does see which book was carried
        wrong = TC.align_prev(W[j - 2], P[j - 2])
        v2, s2, _ = _certify(R0, rows[j], X[j], P[j], Wopt[j], wrong, u, tau, r)
        assert v2 > 1e-6 * s2


def test_zero_penalty_is_the_plain_mvo_book():
    E, torch = _engine()
    for shape in ((9, 5, 4, False), (200, 64, 4, False)):
        A, T, J, _ = shape
        R0, rows, X, P, u = _inputs(*shape)
        Tn = np.full(J, T, dtype=np.int32)
        _, _, info, Wopt = (v[0] for v in _call(E, torch, R0, rows, Tn, X, P, u, 0.0, 0.0))
        Wm, _, im = E.sim_mvo_books(torch.as_tensor(R0, device=DEV), rows, Tn, torch.as_tensor(X, device=DEV),
                                    torch.as_tensor(P, device=DEV), S, u)
        err = np.nanmax(np.abs(Wopt - Wm.cpu().numpy()))
        print(f"{shape}: max |Wopt(tau = 0) - W_mvo| = {err:.3e}; iterations {info[:, 1]} vs {im.cpu().numpy()[:, 1]}")
        assert (info[:, 0] == 0).all() and err <= 1e-6


def test_chains_do_not_depend_on_the_batch_or_on_later_dates():
    E, torch = _engine()
    A, T, J, B = 300, 12, 4, 5
    R0, rows, X0, P0, u = TC.make_chain(A, T, J, 77, ragged=True)
    Xs, Ps = [X0], [P0]
    for b in range(1, B):
        _, _, Xb, Pb, _ = TC.make_chain(A, T, J, 77 + b, ragged=True)
        Xs.append(Xb)
        Ps.append(Pb)
    X, P = np.stack(Xs), np.stack(Ps)
    Tn = np.full(J, T, dtype=np.int32)
    full = _call(E, torch, R0, rows, Tn, X, P, u, 0.1, 1e-4)
    assert (full[2][:, :, 0] == 0).all()
    for b in (0, 3):
        one = _call(E, torch, R0, rows, Tn, X[b], P[b], u, 0.1, 1e-4)
        for a, c in zip(full, one):
            assert a[b].tobytes() == c[0].tobytes()
    head = _call(E, torch, R0, rows[:2], Tn[:2], X[:, :2].copy(), P[:, :2].copy(), u, 0.1, 1e-4)
    for a, c in zip(full, head):
        assert np.ascontiguousarray(a[:, :2]).tobytes() == c.tobytes()


def test_argument_errors():
    E, torch = _engine()
    from factormodeling_amd import _lib as L
    R0, rows, X, P, u = _inputs(9, 5, 4, False)
    Tn = np.full(4, 5, dtype=np.int32)
    with pytest.raises(L.FmxError, match="turnover_penalty"):
        _call(E, torch, R0, rows, Tn, X, P, u, -1e-3, 0.0)
    with pytest.raises(L.FmxError, match="return_weight"):
        _call(E, torch, R0, rows, Tn, X, P, u, 0.1, float("inf"))
    bad = rows.copy()
    bad[2, 1] = R0.shape[0]
    with pytest.raises(L.FmxError, match="outside the returns panel"):
        _call(E, torch, R0, bad, Tn, X, P, u, 0.1, 0.0)
    with pytest.raises(L.FmxError, match="win_T"):
        _call(E, torch, R0, rows, np.array([5, 5, 6, 5], dtype=np.int32), X, P, u, 0.1, 0.0)
    # an undersized workspace is refused before any launch
    t = lambda a, dt=None: torch.as_tensor(a, device=DEV) if dt is None else torch.as_tensor(a, dtype=dt, device=DEV)
    R0d, rd, Td, Xd, Pd = t(R0), t(rows, torch.int32), t(Tn, torch.int32), t(X), t(P)
    W, cn, inf = torch.zeros((1, 4, 9), dtype=torch.float64, device=DEV), t(np.zeros((1, 4, 2))), t(np.zeros((1, 4, 6)))
    need = int(L.load().fmx_sim_mvo_turnover_books_work_bytes(9, 5, 4, 1))
    work = torch.zeros(need // 8, dtype=torch.float64, device=DEV)
    args = [L.ptr(R0d), R0.shape[0], 9, L.ptr(rd), L.ptr(Td), 5, L.ptr(Xd), L.ptr(Pd), 4, 1, S, u, 0.1, 0.0, 100, 1e-9,
            L.ptr(W), None, L.ptr(cn), L.ptr(inf), L.ptr(work)]
    with pytest.raises(L.FmxError, match="workspace too small"):
        L.call("fmx_sim_mvo_turnover_books", *args, need - 8, L.stream_ptr())
    L.call("fmx_sim_mvo_turnover_books", *args, need, L.stream_ptr())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- 3. drop-in
def test_simulation_mvo_turnover_runs_natively(monkeypatch, caplog):
    E, torch = _engine()
    import factormodeling_amd._refload as RL
    import factormodeling_amd.portfolio_simulation as PS
    from factormodeling_amd.simulation import mvo_trade_list
    monkeypatch.delenv("FMX_REFERENCE_DIR", raising=False)
    monkeypatch.delenv("FMX_SIM_MVO", raising=False)
    monkeypatch.setenv("FMX_SIM_MVO_TURNOVER", "native")

    def boom(*a, **k):
        raise AssertionError("method='mvo_turnover' reached the reference loader")
    monkeypatch.setattr(RL, "load", boom)
    rng = np.random.default_rng(4)
    D, A = 12, 40
    dates = pd.bdate_range("2021-01-04", periods=D)
    idx = pd.MultiIndex.from_product([dates, [f"S{i:02d}" for i in range(A)]], names=["date", "symbol"])
    idx = idx[rng.random(len(idx)) > 0.05]                                           # a ragged panel
    ret = pd.Series(0.01 * rng.standard_normal(len(idx)), index=idx, name="ret")
    feat = pd.Series(rng.standard_normal(len(idx)), index=idx, name="sig")
    s = PS.SimulationSettings(returns=ret, cap_flag=pd.Series(1.0, index=idx), investability_flag=pd.Series(1.0, index=idx),
                              factors_df=pd.DataFrame(index=idx), method="mvo_turnover", max_weight=0.2, lookback_period=6,
                              plot=False)
    sim = PS.Simulation("sig", feat, s)
    with caplog.at_level(logging.WARNING, logger="portfolio_simulation"):
        w, counts = sim._daily_trade_list()
    w_mvo, counts_mvo = mvo_trade_list(feat, ret, 0.1, 0.2, 6, 0.1)
    assert w.index.equals(w_mvo.index) and w.index.equals(feat.sort_index().index)
    assert np.array_equal(np.isnan(w.to_numpy()), np.isnan(w_mvo.to_numpy()))          # the shift pattern
    pd.testing.assert_frame_equal(counts, counts_mvo)
    assert any("1 took the equal-leg fallback" in r.getMessage() for r in caplog.records)
    assert not [k for k in sys.modules if k.startswith("_fmx_reference_")]
