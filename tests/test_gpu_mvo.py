"""Native MVO factor selection on the GPU: fmx_mvo_covariance / fmx_mvo_windows behind
``engine.mvo_covariance`` / ``engine.mvo_windows`` and the device branch of
``FactorSelector.prepare_selection`` for ``method="mvo"``.

cvxpy is not a dependency, so parity with its answer cannot be pinned; the specification is
the exact optimum of the QP, certified by the KKT conditions in numpy (mvo_cases.kkt_violation)
and cross-checked against scipy's SLSQP on the small cases.
"""
import functools
import logging
import sys

import numpy as np
import pandas as pd
import pytest

import mvo_cases as MC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _engine():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import factormodeling_amd.engine as E
    return E, torch


def _host_lambda(R):
    """The reference's shrinkage intensity by its definition (per-observation F x F terms)."""
    n, p = R.shape
    S = np.cov(R, rowvar=False)
    sd = np.sqrt(np.diag(S))
    iu = np.triu_indices(p, 1)
    ok = (sd[iu[0]] > 0) & (sd[iu[1]] > 0)
    c = S[iu][ok] / (sd[iu[0]][ok] * sd[iu[1]][ok])
    mc = np.mean(c) if c.size else 0
    T = (mc * sd)[:, None] * sd[None, :]
    np.fill_diagonal(T, np.diag(S))
    rc = R - R.mean(axis=0)
    num = sum(np.sum((np.outer(r, r) - S) ** 2) for r in rc) / n
    with np.errstate(all="ignore"):
        return max(0, min(1, num / np.sum((S - T) ** 2)))


@functools.lru_cache(maxsize=None)
def _host_moments(W, F, const_col, use_shrinkage, J):
    """(R, d0, d1, [mu_j], [Sigma_j], [lambda_j]) of the case's J windows -- computed once."""
    from factormodeling_amd.factor_selection_methods import ledoit_wolf_shrinkage
    R = MC.make_returns(W + J - 1, F, 1000 * W + F, const_col)
    d0, d1 = MC.windows(W + J - 1, W)
    mus, covs, lams = [], [], []
    for a, b in zip(d0, d1):
        Rw = R[a:b]
        mus.append(Rw.mean(axis=0))
        with np.errstate(all="ignore"):
            if use_shrinkage:
                covs.append(ledoit_wolf_shrinkage(Rw))
                lams.append(_host_lambda(Rw))
            else:
                covs.append(pd.DataFrame(Rw).cov().to_numpy())
                lams.append(0.0)
    return R, d0, d1, mus, covs, lams


def _nwin(F):
    return 2 if F >= 100 else 3


# ---------------------------------------------------------------------------- 1. covariance
# the last three have windows whose lambda lies strictly inside (0, 1): the reference's intensity
# has no 1/n factor, so every larger window clamps at 1 and only these exercise the closed form
COV_CASES = [(8, 2, None), (8, 3, None), (60, 12, None), (40, 5, 2), (6, 9, None), (120, 200, None),
             (2, 5, None), (3, 12, None), (2, 40, None)]


@pytest.mark.parametrize("W,F,const_col", COV_CASES)
def test_covariance_matches_host_ledoit_wolf(W, F, const_col):
    E, torch = _engine()
    R, d0, d1, mus, covs, lams = _host_moments(W, F, const_col, True, _nwin(F))
    mu, cov, lam = (t.cpu().numpy() for t in E.mvo_covariance(torch.as_tensor(R, device=DEV), d0, d1, True))
    for j in range(len(d0)):
        e_mu = np.abs(mu[j] - mus[j]).max() / np.abs(mus[j]).max()
        e_cov = np.abs(cov[j] - covs[j]).max() / np.abs(covs[j]).max()
        print(f"W={W} F={F} window {j}: mu rel err {e_mu:.3e}, cov rel err {e_cov:.3e}, "
              f"lambda {lam[j]:.12f} host {lams[j]:.12f}")
        assert e_mu <= 1e-10
        assert e_cov <= 1e-10
        assert abs(lam[j] - lams[j]) <= 1e-9
    if F == 2:
        assert (lam == 1.0).all()          # T == S: the inf / nan -> 1 clamp
    if W <= 3:
        assert ((lam > 0.0) & (lam < 1.0)).any()


@pytest.mark.parametrize("W,F", [(60, 12), (6, 9)])
def test_covariance_without_shrinkage_matches_pandas(W, F):
    E, torch = _engine()
    R, d0, d1, mus, covs, _ = _host_moments(W, F, None, False, 3)
    mu, cov, lam = (t.cpu().numpy() for t in E.mvo_covariance(torch.as_tensor(R, device=DEV), d0, d1, False))
    for j in range(len(d0)):
        assert np.abs(mu[j] - mus[j]).max() <= 1e-10 * np.abs(mus[j]).max()
        assert np.abs(cov[j] - covs[j]).max() <= 1e-10 * np.abs(covs[j]).max()
    assert (lam == 0.0).all()


# ---------------------------------------------------------------------------- 2. optimality
# (W, F, gamma, u, tau); F = 128 / 129 sit on either side of the switch between K^-1 in LDS
# (F <= 128) and K^-1 streamed from the workspace; the last has lambda < 1 (S takes part)
QP_CASES = [(8, 3, 1, 1, 0), (60, 12, 1, 1, 0), (60, 12, 5, 0.3, 0), (60, 12, 50, 0.2, 1e-3), (40, 50, 10, 0.1, 0),
            (120, 200, 10, 1, 0), (120, 200, 100, 0.05, 5e-4), (40, 128, 10, 0.1, 0), (40, 129, 10, 0.1, 0),
            (3, 12, 5, 0.3, 0)]


@functools.lru_cache(maxsize=None)
def _solved(W, F, gamma, u, tau, use_shrinkage=True):
    E, torch = _engine()
    R, d0, d1, mus, covs, _ = _host_moments(W, F, None, use_shrinkage, _nwin(F))
    p = np.random.default_rng(7).dirichlet(np.ones(F)) if tau > 0 else None
    w, info = E.mvo_windows(torch.as_tensor(R, device=DEV), d0, d1, risk_aversion=gamma, max_weight=u,
                            turnover_penalty=tau, prev=None if p is None else torch.as_tensor(p, device=DEV),
                            use_shrinkage=use_shrinkage)
    return w.cpu().numpy(), info.cpu().numpy(), p, mus, [0.5 * (c + c.T) for c in covs]


def _assert_kkt(case, use_shrinkage=True):
    W, F, gamma, u, tau = case
    w, info, p, mus, covs = _solved(*case, use_shrinkage)
    ub = u if u < 1 else 1.0
    for j in range(len(w)):
        viol, scale = MC.kkt_violation(mus[j], covs[j], w[j], gamma, ub, tau, p)
        print(f"{case} window {j}: status {info[j, 0]:.0f}, {info[j, 1]:.0f} iterations, residuals "
              f"{info[j, 2]:.2e} / {info[j, 3]:.2e}, rho {info[j, 5]:.3e}, sum - 1 {w[j].sum() - 1:.2e}, "
              f"KKT violation {viol:.3e} (bound {1e-6 * scale:.3e})")
    for j in range(len(w)):
        viol, scale = MC.kkt_violation(mus[j], covs[j], w[j], gamma, ub, tau, p)
        assert info[j, 0] == 0
        assert abs(w[j].sum() - 1.0) <= 1e-9
        assert (w[j] >= 0.0).all() and (w[j] <= ub).all()
        assert viol <= 1e-6 * scale


@pytest.mark.parametrize("case", QP_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_kkt_certificate(case):
    _assert_kkt(case)


# ---------------------------------------------------------------------------- 3. independent solver
@pytest.mark.parametrize("case", [c for c in QP_CASES[:7] if c[1] <= 50 and c[4] == 0],
                         ids=lambda c: "-".join(str(v) for v in c))
def test_matches_slsqp(case):
    W, F, gamma, u, tau = case
    w, info, p, mus, covs = _solved(*case, True)
    for j in range(len(w)):
        ref = MC.slsqp(mus[j], covs[j], gamma, u)
        err = np.abs(w[j] - ref).max()
        print(f"{case} window {j}: max |w - w_slsqp| = {err:.3e}")
        assert err <= 1e-6


# ---------------------------------------------------------------------------- 4. singular Sigma
def test_singular_covariance_reaches_the_optimal_value():
    case = (6, 9, 10, 0.5, 0)
    _assert_kkt(case, use_shrinkage=False)
    W, F, gamma, u, tau = case
    w, info, p, mus, covs = _solved(*case, False)
    for j in range(len(w)):
        ref = MC.slsqp(mus[j], covs[j], gamma, u)
        o, o_ref = MC.objective(mus[j], covs[j], w[j], gamma), MC.objective(mus[j], covs[j], ref, gamma)
        print(f"window {j}: objective {o:.15e}, SLSQP {o_ref:.15e}")
        assert abs(o - o_ref) <= 1e-9 * abs(o_ref)


# ---------------------------------------------------------------------------- 5. rejected windows
def test_nan_window_is_rejected_alone():
    E, torch = _engine()
    W, F = 20, 7
    R = MC.make_returns(3 * W, F, 5)
    d0 = np.array([0, W, 2 * W], dtype=np.int32)
    d1 = d0 + np.int32(W)
    clean_w, clean_i = (t.cpu().numpy() for t in E.mvo_windows(torch.as_tensor(R, device=DEV), d0, d1, 5.0, 0.5))
    Rn = R.copy()
    Rn[W + 3, 4] = np.nan
    w, info = (t.cpu().numpy() for t in E.mvo_windows(torch.as_tensor(Rn, device=DEV), d0, d1, 5.0, 0.5))
    assert info[1, 0] == 2 and (w[1] == 0.0).all()
    for j in (0, 2):
        assert info[j, 0] == 0
        assert w[j].tobytes() == clean_w[j].tobytes()
        assert info[j].tobytes() == clean_i[j].tobytes()
    # a window of one row is rejected as well
    w1, i1 = E.mvo_windows(torch.as_tensor(R, device=DEV), [0, 3], [W, 4], 5.0, 0.5)
    assert i1[1, 0].item() == 2 and (w1[1] == 0).all().item() and i1[0, 0].item() == 0


def test_infeasible_box_gives_zero_rows():
    """F u < 1: no w in the box sums to one (cvxpy: infeasible -> the reference's zeros)."""
    E, torch = _engine()
    R = MC.make_returns(22, 7, 5)
    w, info = E.mvo_windows(torch.as_tensor(R, device=DEV), [0, 1, 2], [20, 21, 22], 5.0, 0.1)
    assert (info[:, 0] == 2).all().item() and (w == 0).all().item()
    w, info = E.mvo_windows(torch.as_tensor(R[:, :5].copy(), device=DEV), [0, 1], [20, 21], 5.0, 0.2)
    assert (info[:, 0] == 0).all().item()            # F u = 1: the one feasible point
    assert torch.allclose(w, torch.full_like(w, 0.2), rtol=0, atol=1e-9)


# ---------------------------------------------------------------------------- 6. FactorSelector
def _frame():
    rng = np.random.default_rng(3)
    D, A, F = 70, 30, 6
    dates = pd.bdate_range("2021-01-01", periods=D)
    syms = [f"S{i:02d}" for i in range(A)]
    idx = pd.MultiIndex.from_product([dates, syms], names=["date", "symbol"])
    names = [f"g{k // 3}_{k}_{['eq', 'flx', 'raw'][k % 3]}" for k in range(F)]
    df = pd.DataFrame(rng.standard_normal((D * A, F)), index=idx, columns=names)
    ret = pd.Series(0.01 * rng.standard_normal(D * A), index=idx, name="log_return")
    fret = pd.DataFrame(0.01 * rng.standard_normal((D, F)), index=pd.Index(dates, name="date"), columns=names)
    return df, ret, fret, dates, names


@pytest.mark.parametrize("turnover", [False, True])
def test_factor_selector_mvo_runs_natively(monkeypatch, turnover):
    E, torch = _engine()
    import factormodeling_amd._refload as RL
    import factormodeling_amd.factor_selector as fs
    monkeypatch.delenv("FMX_REFERENCE_DIR", raising=False)

    def boom(*a, **k):
        raise AssertionError("method='mvo' reached the reference loader")
    monkeypatch.setattr(RL, "load", boom)
    df, ret, fret, dates, names = _frame()
    kw = {"risk_aversion": 5, "max_weight": 0.5}
    prev = None
    if turnover:
        # a partial Series: the missing factors count as 0
        prev = pd.Series([0.4, 0.35, 0.25], index=[names[4], names[0], names[2]])
        kw.update(turnover_penalty=1e-3, previous_weights=prev)
    sel = fs.FactorSelector(df, ret, fret, window=20, method="mvo", method_kwargs=kw).prepare_selection()
    assert list(sel.index) == list(dates[20:-1])
    assert sorted(sel.columns) == sorted(names)
    np.testing.assert_allclose(sel.sum(axis=1).to_numpy(), 1.0, rtol=0, atol=1e-12)
    J = len(dates) - 21
    p = None if prev is None else prev.reindex(names).fillna(0).to_numpy()
    w, info = E.mvo_windows(torch.as_tensor(fret.to_numpy(), device=DEV), np.arange(J), np.arange(J) + 20, 5, 0.5,
                            1e-3 if turnover else 0.0, p)
    w = w.cpu().numpy()
    assert (info[:, 0] == 0).all().item()
    if turnover:
        plain = E.mvo_windows(torch.as_tensor(fret.to_numpy(), device=DEV), np.arange(J), np.arange(J) + 20, 5, 0.5)[0]
        assert np.abs(plain.cpu().numpy() - w).max() > 1e-6          # the L1 term took part
    w = w / w.sum(axis=1, keepdims=True)
    np.testing.assert_allclose(sel[names].to_numpy(), w / w.sum(axis=1, keepdims=True), rtol=1e-13, atol=0)
    assert not [k for k in sys.modules if k.startswith("_fmx_reference_")]


def test_factor_selector_mvo_warns_on_rejected_days(caplog):
    E, torch = _engine()
    import factormodeling_amd.factor_selector as fs
    df, ret, fret, dates, names = _frame()
    fret = fret.copy()
    fret.iloc[5, 2] = np.nan                   # inside the windows of the first processed days only
    with caplog.at_level(logging.WARNING, logger="factor_selector"):
        sel = fs.FactorSelector(df, ret, fret, window=20, method="mvo",
                                method_kwargs={"risk_aversion": 5, "max_weight": 0.5}).prepare_selection()
    assert (sel.iloc[:6] == 0).all().all() and np.allclose(sel.iloc[6:].sum(axis=1), 1.0)
    assert any("6 had a rejected window" in r.getMessage() for r in caplog.records)
