"""Factor-neutral MVO books on the GPU: fmx_risk_mvo_neutral_books behind
``engine.risk_mvo_books(neutral=...)``, ``simulation.risk_mvo_trade_list(neutral=...)`` and
``FactorRiskModel.neutral_to``.

The specification is pinned on the host (risk_neutral_cases.py, checked by
test_risk_neutral_host.py): the LP certificate with the extra equality rows, a tight SLSQP, the
numpy model of the scheme and the feasibility table.  Each test prints the figures it asserts on.

Figures of the first run on an MI355X are in DESIGN 27.
"""
import ctypes
import functools
import logging

import numpy as np
import pandas as pd
import pytest

import risk_model_cases as RC
import risk_neutral_cases as NC

pytestmark = pytest.mark.gpu
DEV = "cuda"
_IDS = [NC.case_id(c) for c in NC.NEUTRAL_CASES]


def _engine():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import factormodeling_amd.engine as E
    return E, torch


def _dev(torch, *arrays):
    return [torch.as_tensor(np.ascontiguousarray(a), device=DEV) for a in arrays]


def _inputs(torch, c):
    B, Fc, S2, X, P, mrow = RC.mvo_case(*c)
    return _dev(torch, B, Fc, S2, np.where(P != 0, X, np.nan), P), mrow


@functools.lru_cache(maxsize=None)
def _solved(i):
    """(W, counts, info, expo) of case i; a case with an infeasible date runs 2000 rounds."""
    E, torch = _engine()
    c, N, feas = NC.NEUTRAL_CASES[i]
    dev, mrow = _inputs(torch, c)
    out = E.risk_mvo_books(*dev, mrow, c[2], max_iter=20000 if all(feas) else 2000, neutral=N, return_expo=True)
    return tuple(t.cpu().numpy() for t in out)


def _check_solved_row(tag, Bd, Fd, s2d, x, p, u, N, w, info_row, expo_row, small=None):
    """Check 1 on one status-0 row: Bd [K][A], Fd, s2d the model date, x / p the signal row."""
    A, K = len(x), Bd.shape[0]
    pr = p != 0
    sg = RC.signs(x, p)
    act = sg != 0
    assert np.isnan(w[~pr]).all() and not np.isnan(w[pr]).any()
    assert (w[pr & ~act] == 0.0).all()
    Bc = RC.clean_b(Bd)[:, act]
    wa, sa = w[act], sg[act]
    g = 2.0 * RC.sigma_times(Bd, Fd, s2d, w[pr], p)[act[pr]]
    C, _ = NC.constraint_rows(Bc, sa, N)
    viol, scale = NC.kkt_violation_eq(g, wa, sa, u, C)
    bmax = np.abs(C[2:]).max(axis=1)
    ex = np.abs(expo_row[list(N)]) / bmax
    ref, ref_abs = RC.clean_b(Bd, p) @ np.where(pr, w, 0.0), np.abs(RC.clean_b(Bd, p)) @ np.abs(np.where(pr, w, 0.0))
    print(f"{tag}: status {info_row[0]:.0f}, {info_row[1]:.0f} iterations, residuals {info_row[2]:.2e} / "
          f"{info_row[3]:.2e}, rho {info_row[5]:.3e}, leg sums - 1: {wa[sa > 0].sum() - 1:.2e} {-wa[sa < 0].sum() - 1:.2e}, "
          f"KKT {viol:.3e} (bound {1e-6 * scale:.3e}), worst |expo_k| / bmax_k {ex.max():.2e}, "
          f"expo vs numpy {np.abs(expo_row - ref).max():.2e}")
    assert info_row[0] == 0
    assert viol <= 1e-6 * scale
    assert abs(wa[sa > 0].sum() - 1.0) <= 1e-10 and abs(wa[sa < 0].sum() + 1.0) <= 1e-10
    assert (wa[sa > 0] >= 0.0).all() and (wa[sa > 0] <= u).all()
    assert (wa[sa < 0] <= 0.0).all() and (wa[sa < 0] >= -u).all()
    assert (ex <= 2e-9).all()
    assert (np.abs(expo_row - ref) <= (A + 4) * RC.EPS53 * ref_abs).all()
    if small is not None:
        Sig = RC.sigma(Bc, Fd, s2d[act])
        if A <= 40:
            err = np.abs(wa - NC.tight_slsqp_eq(Sig, sa, u, C)).max()
            print(f"{tag}: max |w - w_slsqp| = {err:.3e}")
            assert err <= 1e-6
        wm, stm, itm, _ = NC.neutral_model(Sig, Bc, s2d[act], sa, u, N)
        err = np.abs(wa - wm).max()
        print(f"{tag}: max |w - w_model| = {err:.3e}; iterations kernel {info_row[1]:.0f}, model {itm}")
        assert stm == 0 and err <= 1e-8


# ---------------------------------------------------------------------------- 1. every feasible row
@pytest.mark.parametrize("i", range(len(NC.NEUTRAL_CASES)), ids=_IDS)
def test_feasible_rows_are_optimal_and_neutral(i):
    c, N, feas = NC.NEUTRAL_CASES[i]
    A, K, u, variant = c
    B, Fc, S2, X, P, mrow = RC.mvo_case(*c)
    W, counts, info, expo = _solved(i)
    for j in range(2):
        if not feas[j]:
            continue
        r = mrow[j]
        _check_solved_row(f"{_IDS[i]} date {j}", B[:, r], Fc[r], S2[r], X[j], P[j], u, N, W[j], info[j], expo[j],
                          small=True if A <= 200 else None)
        sg = RC.signs(X[j], P[j])
        assert counts[j, 0] == (sg > 0).sum() and counts[j, 1] == (sg < 0).sum()


# ---------------------------------------------------------------------------- 2. the empty mask
@pytest.mark.parametrize("c", [(40, 8, 0.1, None), (1100, 6, 0.03, None), (200, 32, 0.03, None)], ids=str)
def test_the_empty_mask_is_todays_kernel(c):
    E, torch = _engine()
    dev, mrow = _inputs(torch, c)
    want = E.risk_mvo_books(*dev, mrow, c[2])
    got = E.risk_mvo_books(*dev, mrow, c[2], neutral=(), return_expo=True)       # fmx_risk_mvo_neutral_books, mask 0
    for a, b in zip(got[:3], want):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    B, Fc, S2, X, P, _ = RC.mvo_case(*c)
    W, expo = got[0].cpu().numpy(), got[3].cpu().numpy()
    for j in range(2):
        Bc = RC.clean_b(B[:, mrow[j]], P[j])
        w = np.where(P[j] != 0, W[j], 0.0)
        assert (np.abs(expo[j] - Bc @ w) <= (c[0] + 4) * RC.EPS53 * (np.abs(Bc) @ np.abs(w))).all()


# ---------------------------------------------------------------------------- 3. batch invariance
@pytest.mark.parametrize("i", [_IDS.index("65-8-0.1-None-N3"), _IDS.index("1100-6-0.03-None-N2")],
                         ids=["65-8", "1100-6"])
def test_a_row_does_not_depend_on_the_batch(i):
    E, torch = _engine()
    c, N, _ = NC.NEUTRAL_CASES[i]
    (B, Fc, S2, X, P), mrow = _inputs(torch, c)
    full = _solved(i)
    rev = E.risk_mvo_books(B, Fc, S2, X.flip(0).contiguous(), P.flip(0).contiguous(), mrow[::-1].copy(), c[2],
                           neutral=N, return_expo=True)
    for j in range(2):
        alone = E.risk_mvo_books(B, Fc, S2, X[j:j + 1], P[j:j + 1], mrow[j:j + 1], c[2], neutral=N, return_expo=True)
        for a, b, f in zip(alone, rev, full):
            assert a.cpu().numpy()[0].tobytes() == f[j].tobytes()
            assert b.cpu().numpy()[1 - j].tobytes() == f[j].tobytes()


# ---------------------------------------------------------------------------- 4. variance ordering
@pytest.mark.parametrize("i", [k for k, c in enumerate(NC.NEUTRAL_CASES) if all(c[2])],
                         ids=[s for s, c in zip(_IDS, NC.NEUTRAL_CASES) if all(c[2])])
def test_predicted_variance_ordering(i):
    E, torch = _engine()
    c, N, _ = NC.NEUTRAL_CASES[i]
    A, K, u, variant = c
    B, Fc, S2, X, P, mrow = RC.mvo_case(*c)
    dev, _ = _inputs(torch, c)
    W = _solved(i)[0]
    W0 = E.risk_mvo_books(*dev, mrow, u)[0].cpu().numpy()
    books = np.full((3, 3, A), np.nan)
    present = np.ones((3, A), dtype=np.uint8)
    x0s = []
    for j in range(2):
        sg = RC.signs(X[j], P[j])
        x0 = np.where(sg > 0, 1.0 / (sg > 0).sum(), np.where(sg < 0, -1.0 / (sg < 0).sum(), 0.0))
        books[0, mrow[j]], books[1, mrow[j]], books[2, mrow[j]] = W[j], W0[j], x0
        present[mrow[j]] = P[j]
        x0s.append(x0)
    var = E.risk_books(*_dev(torch, B, Fc, S2, books, present))["var"].cpu().numpy()
    for j in range(2):
        v, v_un, v_x0 = (var[m, mrow[j], 0] for m in range(3))
        Bc = RC.clean_b(B[:, mrow[j]], P[j])[list(N)]
        x0_neutral = (np.abs(Bc @ x0s[j]) <= 1e-9 * np.abs(Bc).max(axis=1)).all()
        print(f"{_IDS[i]} date {j}: predicted variance neutral {v:.6e}, un-neutral {v_un:.6e}, x0 {v_x0:.6e} "
              f"(x0 neutral: {x0_neutral})")
        assert v >= v_un * (1.0 - 1e-12)
        if x0_neutral:
            assert v <= v_x0


# ---------------------------------------------------------------------------- 5. infeasible rows
def _case_model(torch, c):
    """mvo_case as a FactorRiskModel over three dates and a feature with rows on dates 0 and 2."""
    from factormodeling_amd.panel import panel_index
    from factormodeling_amd.risk_model import FactorRiskModel
    B, Fc, S2, X, P, mrow = RC.mvo_case(*c)
    A, K = c[0], c[1]
    dates = pd.bdate_range("2021-03-01", periods=3)
    syms = [f"S{i:05d}" for i in range(A)]
    idx = pd.MultiIndex.from_product([dates, syms], names=["date", "symbol"])
    cols = pd.Index([f"f{k}" for k in range(K)])
    fr = pd.DataFrame(np.zeros((3, K)), index=pd.Index(dates, name="date"), columns=cols)
    model = FactorRiskModel(panel_index(idx), cols, *_dev(torch, B, Fc, S2, np.ones(3, dtype=np.uint8)), fr, idx)
    parts = [pd.Series(X[j][P[j] != 0], index=pd.MultiIndex.from_product([[dates[mrow[j]]], np.array(syms)[P[j] != 0]],
                                                                         names=["date", "symbol"])) for j in range(2)]
    return model, pd.concat(parts), dates


@pytest.mark.parametrize("i", [k for k, c in enumerate(NC.NEUTRAL_CASES) if not all(c[2])],
                         ids=[s for s, c in zip(_IDS, NC.NEUTRAL_CASES) if not all(c[2])])
def test_infeasible_rows_end_with_status_1_and_a_warning(i, caplog):
    E, torch = _engine()
    from factormodeling_amd.simulation import risk_mvo_trade_list
    c, N, feas = NC.NEUTRAL_CASES[i]
    W, counts, info, expo = _solved(i)
    for j in range(2):
        print(f"{_IDS[i]} date {j}: status {info[j, 0]:.0f}, {info[j, 1]:.0f} iterations, expo {expo[j]}")
        if feas[j]:
            assert info[j, 0] == 0                     # test_feasible_rows_are_optimal_and_neutral checks the row
        else:
            assert info[j, 0] == 1 and info[j, 1] == 2000 and np.isfinite(expo[j]).all()
    model, feat, dates = _case_model(torch, c)
    names = [f"f{k}" for k in N]
    with caplog.at_level(logging.WARNING, logger="simulation"):
        _, _, extra = risk_mvo_trade_list(feat, model.neutral_to(names), 0.1, c[2], return_info=True, max_iter=2000)
    assert extra["neutral"] == tuple(names)
    assert extra["info"].tobytes() == info.tobytes() and extra["expo"].tobytes() == expo.tobytes()
    held = np.flatnonzero((RC.mvo_case(*c)[4] != 0).any(axis=0))          # the feature's symbols
    assert extra["books"].tobytes() == np.ascontiguousarray(W[:, held]).tobytes()
    recs = [r.getMessage() for r in caplog.records if "neutral" in r.getMessage()]
    print(recs)
    assert len(recs) == 1 and "equal-leg fallback" not in recs[0]
    for j, d in enumerate((dates[0], dates[2])):
        assert (str(d.date()) in recs[0]) == (not feas[j])


# ---------------------------------------------------------------------------- 6. dependent rows
def test_both_duplicated_factors_end_with_zero_exposure():
    i = _IDS.index("40-8-0.1-dup-N2")
    c, N, _ = NC.NEUTRAL_CASES[i]
    B, Fc, S2, X, P, mrow = RC.mvo_case(*c)
    W, counts, info, expo = _solved(i)
    for j in range(2):
        Bc = RC.clean_b(B[:, mrow[j]], P[j])
        assert np.array_equal(Bc[0], Bc[1])
        bmax = np.abs(Bc[:2][:, RC.signs(X[j], P[j]) != 0]).max(axis=1)
        print(f"dup date {j}: status {info[j, 0]:.0f}, expo {expo[j, 0]:.3e} {expo[j, 1]:.3e}")
        assert info[j, 0] == 0 and (np.abs(expo[j, :2]) <= 2e-9 * bmax).all()


# ---------------------------------------------------------------------------- 7. the drop-in
def test_simulation_with_a_neutral_model(monkeypatch):
    E, torch = _engine()
    import test_gpu_risk_model as TG

    import factormodeling_amd.portfolio_simulation as PS
    from factormodeling_amd.simulation import risk_mvo_trade_list
    monkeypatch.delenv("FMX_SIM_MVO", raising=False)
    fdf, ret, dates = TG._fit_panel()
    rm = TG._fitted()
    feat = pd.Series(np.random.default_rng(9).standard_normal(len(fdf)), index=fdf.index, name="sig")
    view = rm.neutral_to(["val"])
    w, counts = PS.Simulation("sig", feat, TG._settings(PS, ret, fdf.index, method="mvo", risk_model=view))._daily_trade_list()
    want_w, want_c, extra = risk_mvo_trade_list(feat, view, 0.1, 0.4, return_info=True)
    pd.testing.assert_series_equal(w, want_w, check_exact=True)
    pd.testing.assert_frame_equal(counts, want_c)
    assert extra["neutral"] == ("val",)
    st = extra["info"][:, 0]
    print("statuses:", {int(k): int((st == k).sum()) for k in np.unique(st)})
    assert (st == 0).sum() >= 1 and (st == 4).sum() >= 1
    mp = rm.panel_index
    Bh, Fh, Sh = rm.B.cpu().numpy(), rm.Fc.cpu().numpy(), rm.S2.cpu().numpy()
    from factormodeling_amd.panel import panel_index
    fpi = panel_index(feat.index)
    xh = np.full((fpi.D, mp.A), np.nan)
    cols = mp.symbols.get_indexer(fpi.symbols)
    xh[fpi.d, cols[fpi.s]] = feat.to_numpy()
    ph = np.zeros((fpi.D, mp.A), dtype=np.uint8)
    ph[fpi.d, cols[fpi.s]] = 1
    mrow = mp.dates.get_indexer(fpi.dates)
    books = np.full((fpi.D, mp.A), np.nan)
    books[:, cols] = extra["books"]
    _, _, we = E.trade_books(torch.as_tensor(xh[None], device=DEV), "equal", 0.1, 0.4,
                             present=torch.as_tensor(ph, device=DEV), nan_absent=False, raw=True)
    we = we[0].cpu().numpy()
    for d in range(fpi.D):
        if st[d] == 0:
            _check_solved_row(f"fitted panel date {d}", Bh[:, mrow[d]], Fh[mrow[d]], Sh[mrow[d]], xh[d], ph[d], 0.4, (0,),
                              books[d], extra["info"][d], extra["expo"][d])
        elif st[d] == 4:
            assert books[d].tobytes() == we[d].tobytes()
    # without neutral_to: today's bytes
    w0, c0 = PS.Simulation("sig", feat, TG._settings(PS, ret, fdf.index, method="mvo", risk_model=rm))._daily_trade_list()
    w1, c1, e1 = risk_mvo_trade_list(feat, rm, 0.1, 0.4, return_info=True)
    assert w0.to_numpy().tobytes() == w1.to_numpy().tobytes() and "expo" not in e1
    pd.testing.assert_frame_equal(c0, c1)
    assert w0.to_numpy().tobytes() != w.to_numpy().tobytes()


# ---------------------------------------------------------------------------- 8. the C ABI
def test_the_c_abi():
    E, torch = _engine()
    import factormodeling_amd._lib as L
    lib = L.load()

    def p(t):
        return ctypes.c_void_p(t.data_ptr())
    f64 = dict(dtype=torch.float64, device=DEV)
    B = torch.tensor([[[1.0, -0.5, 2.0, -1.0]], [[0.3, 0.2, -0.1, 0.4]]], **f64)      # [K=2][Dm=1][A=4]
    Fc = torch.tensor([[[4e-4, 0.0], [1e-4, 2e-4]]], **f64)
    S2 = torch.tensor([[1e-4, 2e-4, 3e-4, 1.5e-4]], **f64)
    X = torch.tensor([[1.0, 2.0, -1.0, -3.0]], **f64)
    mrow = torch.tensor([0], dtype=torch.int32, device=DEV)
    W, W2 = torch.empty((1, 4), **f64), torch.empty((1, 4), **f64)
    counts, info, expo = torch.empty((1, 2), **f64), torch.empty((1, 6), **f64), torch.empty((1, 2), **f64)
    stream = L.stream_ptr()
    assert lib.fmx_risk_mvo_neutral_books_work_bytes(4, 2, 1) == 0

    def run(mask, Wout, ex):
        return lib.fmx_risk_mvo_neutral_books(p(B), p(Fc), p(S2), 2, 1, 4, p(mrow), p(X), None, 1, mask, 1.0, 20000, 1e-9,
                                              p(Wout), p(counts), p(info), ex, None, 0, stream)
    assert run(1, W, p(expo)) == 0
    torch.cuda.synchronize()
    w, e = W.cpu().numpy()[0], expo.cpu().numpy()[0]
    print("w", w, "expo", e, "info", info.cpu().numpy())
    assert info.cpu().numpy()[0, 0] == 0 and abs(e[0]) <= 2e-9 * 2.0
    np.testing.assert_allclose(e, B.cpu().numpy()[:, 0] @ w, rtol=0, atol=1e-14)
    assert abs(w[:2].sum() - 1) <= 1e-10 and abs(w[2:].sum() + 1) <= 1e-10
    assert run(1, W2, None) == 0                                   # a null expo is accepted
    torch.cuda.synchronize()
    assert W2.cpu().numpy().tobytes() == W.cpu().numpy().tobytes()
    for bad in (4, 1 << 31, 5):                                    # a bit at or above K
        assert run(bad, W2, None) == 1
        assert b"neutral" in lib.fmx_last_error()
