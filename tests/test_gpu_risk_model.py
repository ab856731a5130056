"""The factor risk model on the GPU: fmx_risk_books behind ``engine.risk_books``,
fmx_risk_mvo_books behind ``engine.risk_mvo_books`` / ``simulation.risk_mvo_trade_list``,
``risk_model.FactorRiskModel`` and the routing in ``Simulation._daily_trade_list``.

Nothing in the reference does this, so the specification is pinned by numpy / pandas / SLSQP
(risk_model_cases.py, checked on the host by test_risk_model_host.py): the dense Sigma, the
a-priori fp64 summation bound for the risk sums, the KKT certificate and a tight SLSQP for the
books, pandas' ewm for the fit.  Each test prints the figures it asserts on.
"""
import functools
import logging

import numpy as np
import pandas as pd
import pytest

import risk_model_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _engine():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import factormodeling_amd.engine as E
    return E, torch


def _dev(torch, *arrays):
    return [torch.as_tensor(np.ascontiguousarray(a), device=DEV) for a in arrays]


# ---------------------------------------------------------------------------- 1. risk vs dense numpy
RISK_CASES = [(3, 1), (9, 2), (63, 3), (64, 8), (65, 8), (1100, 32), (4100, 5), (16384, 32)]
RISK_OUT = ("var", "expo", "contrib", "marginal")


@functools.lru_cache(maxsize=None)
def _risk_run(A, K):
    E, torch = _engine()
    B, Fc, S2, W, present, valid = RC.risk_case(A, K)
    out = E.risk_books(*_dev(torch, B, Fc, S2, W, present, valid), marginal=True)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("A,K", RISK_CASES)
def test_risk_against_dense_numpy(A, K):
    B, Fc, S2, W, present, valid = RC.risk_case(A, K)
    got = _risk_run(A, K)
    bound = (A + K + 4) * RC.EPS53
    worst = dict.fromkeys(RISK_OUT, 0.0)
    for m in range(W.shape[0]):
        for d in range(W.shape[1]):
            if not valid[d]:
                for k in RISK_OUT:
                    assert np.isnan(got[k][m, d]).all(), (k, m, d)
                continue
            want = RC.risk_terms(B[:, d], Fc[d], S2[d], W[m, d], present[d])
            for k in RISK_OUT:
                w, scale = want[k]
                g = got[k][m, d]
                assert np.array_equal(np.isnan(g), np.isnan(w)), (k, m, d)
                fin = ~np.isnan(w)
                err = np.abs(g - w)[fin]
                assert (err <= bound * scale[fin]).all(), (k, m, d, err.max())
                with np.errstate(invalid="ignore", divide="ignore"):
                    worst[k] = max(worst[k], np.nanmax(np.where(scale[fin] > 0, err / scale[fin], 0.0), initial=0.0))
            fsum_err = abs(got["contrib"][m, d].sum() - got["var"][m, d, 1])
            assert fsum_err <= bound * want["var"][1][1], (m, d, fsum_err)
            if m == 1:
                assert (got["var"][m, d] == 0).all() and (got["expo"][m, d] == 0).all()
    print(f"(A, K) = ({A}, {K}): worst error / sum|terms| " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items())
          + f" (bound {bound:.2e})")


# ---------------------------------------------------------------------------- 2. batch invariance
@pytest.mark.parametrize("A,K", [(65, 8), (1100, 32)])
def test_a_book_and_a_date_do_not_depend_on_the_batch(A, K):
    E, torch = _engine()
    B, Fc, S2, W, present, valid = RC.risk_case(A, K)
    valid = np.ones_like(valid)
    full = {k: v.cpu().numpy() for k, v in
            E.risk_books(*_dev(torch, B, Fc, S2, W, present, valid), marginal=True).items()}
    alone = E.risk_books(*_dev(torch, B, Fc, S2, W[2:3], present, valid), marginal=True)
    for k in RISK_OUT:
        assert alone[k].cpu().numpy()[0].tobytes() == full[k][2].tobytes(), k
    wide = np.concatenate([W] * 6)                                         # 18 books: two tiles of 16
    tile = E.risk_books(*_dev(torch, B, Fc, S2, wide, present, valid), marginal=True)
    for k in RISK_OUT:
        assert tile[k].cpu().numpy()[3:6].tobytes() == full[k].tobytes(), k
        assert tile[k].cpu().numpy()[15:18].tobytes() == full[k].tobytes(), k     # books 15 | 16, 17 straddle the tiles
    day = E.risk_books(*_dev(torch, B[:, 1:2], Fc[1:2], S2[1:2], W[:, 1:2], present[1:2], valid[1:2]), marginal=True)
    for k in RISK_OUT:
        assert day[k].cpu().numpy()[:, 0].tobytes() == full[k][:, 1].tobytes(), k


# ---------------------------------------------------------------------------- 3. MVO optimality
_IDS = ["-".join(str(v) for v in c) for c in RC.MVO_CASES]


@functools.lru_cache(maxsize=None)
def _solved(A, K, u, variant):
    E, torch = _engine()
    B, Fc, S2, X, P, mrow = RC.mvo_case(A, K, u, variant)
    W, counts, info = E.risk_mvo_books(*_dev(torch, B, Fc, S2, np.where(P != 0, X, np.nan), P), mrow, u)
    return W.cpu().numpy(), counts.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("case", RC.MVO_CASES, ids=_IDS)
def test_kkt_certificate(case):
    A, K, u, variant = case
    B, Fc, S2, X, P, mrow = RC.mvo_case(A, K, u, variant)
    W, counts, info = _solved(*case)
    for j in range(2):
        r, pr = mrow[j], P[j] != 0
        sg = RC.signs(X[j], P[j])
        assert u * (sg > 0).sum() >= 1 and u * (sg < 0).sum() >= 1, "the case must be a feasible QP day"
        w = W[j]
        assert np.isnan(w[~pr]).all() and not np.isnan(w[pr]).any()
        q = 2.0 * RC.sigma_times(B[:, r], Fc[r], S2[r], w[pr], P[j])
        viol, scale = RC.kkt_violation(q, w[pr], sg[pr], u)
        print(f"{case} date {j}: status {info[j, 0]:.0f}, {info[j, 1]:.0f} iterations, residuals {info[j, 2]:.2e} / "
              f"{info[j, 3]:.2e}, min s2 {info[j, 4]:.3e}, rho {info[j, 5]:.3e}, leg sums - 1: "
              f"{w[sg > 0].sum() - 1:.2e} {-w[sg < 0].sum() - 1:.2e}, KKT violation {viol:.3e} "
              f"(bound {1e-6 * scale:.3e})")
        assert info[j, 0] == 0
        assert abs(w[sg > 0].sum() - 1.0) <= 1e-9 and abs(w[sg < 0].sum() + 1.0) <= 1e-9
        assert (w[sg > 0] >= 0.0).all() and (w[sg > 0] <= u).all()
        assert (w[sg < 0] <= 0.0).all() and (w[sg < 0] >= -u).all()
        assert (w[pr & (sg == 0)] == 0.0).all()
        assert counts[j, 0] == (sg > 0).sum() and counts[j, 1] == (sg < 0).sum()
        assert viol <= 1e-6 * scale
        if A <= 40:
            ref = RC.tight_slsqp(RC.sigma(B[:, r], Fc[r], S2[r], P[j]), sg[pr], u)
            err = np.abs(w[pr] - ref).max()
            print(f"{case} date {j}: max |w - w_slsqp| = {err:.3e}")
            assert err <= 1e-6


# ---------------------------------------------------------------------------- 4. the model's own terms
@pytest.mark.parametrize("case", RC.MVO_CASES, ids=_IDS)
def test_the_solved_book_has_no_more_predicted_variance_than_x0(case):
    E, torch = _engine()
    A, K, u, variant = case
    B, Fc, S2, X, P, mrow = RC.mvo_case(A, K, u, variant)
    W, _, info = _solved(*case)
    books = np.full((2, 3, A), np.nan)
    present = np.ones((3, A), dtype=np.uint8)
    for j in range(2):
        sg = RC.signs(X[j], P[j])
        books[0, mrow[j]] = W[j]
        books[1, mrow[j]] = np.where(sg > 0, 1.0 / (sg > 0).sum(), np.where(sg < 0, -1.0 / (sg < 0).sum(), 0.0))
        present[mrow[j]] = P[j]
    var = E.risk_books(*_dev(torch, B, Fc, S2, books, present))["var"].cpu().numpy()
    for j in range(2):
        v, v0 = var[0, mrow[j], 0], var[1, mrow[j], 0]
        print(f"{case} date {j}: predicted variance {v:.6e} vs x0 {v0:.6e} (ratio {v / v0:.4f})")
        assert info[j, 0] == 0 and v <= v0


# ---------------------------------------------------------------------------- 5. edge days
def _edge_panel():
    """7 dates x 12 symbols, six long and six short: date 0 has no valid model row, date 2 three
    positive cells under a 0.25 box, date 3 one leg only, date 4 a NaN signal, date 5 a NaN in Fc."""
    rng = np.random.default_rng(21)
    D, A, K = 7, 12, 3
    dates = pd.bdate_range("2021-03-01", periods=D)
    syms = [f"S{i:02d}" for i in range(A)]
    idx = pd.MultiIndex.from_product([dates, syms], names=["date", "symbol"])
    x = rng.standard_normal((D, A))
    x[:, :6] = np.abs(x[:, :6]) + 0.05
    x[:, 6:] = -np.abs(x[:, 6:]) - 0.05
    x[2, 3:6] = -x[2, 3:6]
    x[3] = np.abs(x[3])
    x[4, 5] = np.nan
    sig = pd.Series(x.reshape(-1), index=idx, name="sig")
    B, Fc, S2 = RC.model_arrays(D, A, K, 99)
    Fc[5, 2, 1] = np.nan
    valid = np.ones(D, dtype=np.uint8)
    valid[0] = 0
    return dates, syms, idx, sig, x, B, Fc, S2, valid


def _edge_model(torch):
    from factormodeling_amd.panel import panel_index
    from factormodeling_amd.risk_model import FactorRiskModel
    dates, syms, idx, sig, x, B, Fc, S2, valid = _edge_panel()
    cols = pd.Index(["f0", "f1", "f2"])
    fr = pd.DataFrame(np.zeros((len(dates), 3)), index=pd.Index(dates, name="date"), columns=cols)
    return FactorRiskModel(panel_index(idx), cols, *_dev(torch, B, Fc, S2, valid), fr, idx)


def test_edge_days():
    E, torch = _engine()
    from factormodeling_amd._lib import FmxError
    from factormodeling_amd.simulation import risk_mvo_trade_list
    dates, syms, idx, sig, x, B, Fc, S2, valid = _edge_panel()
    model = _edge_model(torch)
    shifted, counts, extra = risk_mvo_trade_list(sig, model, pct=0.4, max_weight=0.25, return_info=True)
    info, books = extra["info"], extra["books"]
    assert list(info[:, 0]) == [4, 0, 2, 3, 0, 2, 0]
    # date 0: an invalid model date -> the equal-weight book, bit for bit
    _, ce, we = E.trade_books(torch.as_tensor(x[None], device=DEV), "equal", 0.4, 0.25, nan_absent=False, raw=True)
    assert books[0].tobytes() == we[0, 0].cpu().numpy().tobytes()
    assert list(counts.iloc[0]) == [int(v) for v in ce[0, 0].cpu().numpy()] == [2, 2]
    # date 2: an infeasible long leg -> x0; date 5: a NaN in Fc on a valid-flagged row -> x0
    for d, (npos, nneg) in ((2, (3, 9)), (5, (6, 6))):
        assert np.array_equal(books[d], np.where(x[d] > 0, 1.0 / npos, -1.0 / nneg))
        assert list(counts.iloc[d]) == [npos, nneg]
    # date 3: one leg only -> flat, counts (0, 0)
    assert (books[3] == 0.0).all() and list(counts.iloc[3]) == [0, 0]
    # date 4: the NaN-signal symbol is in the book with weight 0
    assert books[4, 5] == 0.0 and not np.isnan(books[4]).any() and list(counts.iloc[4]) == [5, 6]
    for d in (1, 4, 6):
        assert abs(books[d][x[d] > 0].sum() - 1) <= 1e-9 and abs(books[d][x[d] < 0].sum() + 1) <= 1e-9
        assert np.abs(books[d]).max() <= 0.25
    # the result is the per-symbol shift of the books
    want = pd.Series(books.reshape(-1), index=sig.index).groupby(level="symbol").shift(1)
    pd.testing.assert_series_equal(shifted, want, check_names=False, check_exact=True)
    assert list(counts.columns) == ["long_count", "short_count"] and counts.index.name == "date"
    # a model row outside the model is an argument error, before any launch
    Xd = torch.as_tensor(x[:2], device=DEV)
    for bad in ([0, len(dates)], [-2, 1]):
        with pytest.raises(FmxError, match="model_row"):
            E.risk_mvo_books(model.B, model.Fc, model.S2, Xd, None, np.array(bad, dtype=np.int32), 0.25)
    W, _, inf2 = E.risk_mvo_books(model.B, model.Fc, model.S2, Xd, None, np.array([-1, 1], dtype=np.int32), 0.25)
    assert list(inf2.cpu().numpy()[:, 0]) == [4, 0] and W.cpu().numpy()[1].tobytes() == books[1].tobytes()


# ---------------------------------------------------------------------------- 6. fit vs pandas
@functools.lru_cache(maxsize=None)
def _fit_panel():
    rng = np.random.default_rng(5)
    D, A, K = 40, 12, 3
    dates = pd.bdate_range("2022-01-03", periods=D)
    syms = [f"S{i:02d}" for i in range(A)]
    idx = pd.MultiIndex.from_product([dates, syms], names=["date", "symbol"])
    keep = rng.random(len(idx)) > 0.08
    keep[(idx.get_level_values(0) < dates[9]) & (idx.get_level_values(1) == "S11")] = False    # a late listing
    thin = idx.get_level_values(0) == dates[20]
    keep[thin] = np.isin(idx.get_level_values(1)[thin], ["S00", "S01", "S02"])                 # 3 rows < 4 coefficients
    idx = idx[keep]
    fdf = pd.DataFrame(rng.standard_normal((len(idx), K)), index=idx, columns=["val", "mom", "size"])
    fdf.iloc[rng.choice(len(idx), 6, replace=False), 1] = np.nan
    scale = pd.Series(rng.uniform(0.3, 2.0, A), index=syms)
    ret = pd.Series(0.01 * rng.standard_normal(len(idx)) * scale.reindex(idx.get_level_values(1)).to_numpy(),
                    index=idx, name="ret")
    return fdf, ret, dates


@functools.lru_cache(maxsize=None)
def _fitted():
    _engine()
    from factormodeling_amd.risk_model import FactorRiskModel
    fdf, ret, _ = _fit_panel()
    return FactorRiskModel.fit(fdf, ret, lag=1, cov_halflife=5, spec_halflife=4, min_periods=5)


def _same_values(got, want):
    """NaN where NaN, otherwise equal bits."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and \
        got[~np.isnan(got)].tobytes() == want[~np.isnan(want)].tobytes()


def test_fit_against_pandas():
    from factormodeling_amd.factor_backtest import cross_sectional_factor_returns
    fdf, ret, dates = _fit_panel()
    rm = _fitted()
    table = cross_sectional_factor_returns(fdf, ret, 1, True, None)
    assert rm.factor_returns.index.equals(table.index) and list(rm.factor_returns.columns) == list(table.columns)
    assert _same_values(rm.factor_returns.to_numpy(), table.to_numpy())
    assert table.loc[dates[20]].isna().all() and table.loc[dates[25]].notna().all()       # the thin date
    cov, s2, valid = RC.fit_oracle(rm.factor_returns, rm.residuals, 5, 4, 5, spec_floor=1e-6)
    assert rm.factor_cov.shape == cov.shape and list(rm.factor_cov.columns) == list(cov.columns)
    assert _same_values(rm.factor_cov.to_numpy(), cov.to_numpy())
    assert rm.specific_var.index.equals(fdf.index)
    assert _same_values(rm.specific_var.to_numpy(), s2.to_numpy())
    assert list(rm.valid) == list(valid) and 5 <= int(rm.valid.sum()) < len(dates)
    filled = rm.residuals.groupby(level="symbol").shift(1).groupby(level="symbol").ewm(halflife=4, min_periods=5) \
        .var().droplevel(0).reindex(fdf.index).isna() & rm.specific_var.notna()
    print(f"valid dates {int(rm.valid.sum())} of {len(dates)}, {int(filled.sum())} filled cells, "
          f"{int((rm.specific_var == 1e-6).sum())} floored")
    assert filled.any()
    d = int(np.flatnonzero(rm.valid.to_numpy())[-1])
    pres = rm.panel_index.present_np[d]
    want = RC.sigma(rm.B[:, d].cpu().numpy(), rm.Fc[d].cpu().numpy(), rm.S2[d].cpu().numpy(), pres)
    got = rm.covariance(dates[d])
    assert list(got.index) == list(rm.panel_index.symbols[pres != 0])
    np.testing.assert_allclose(got.to_numpy(), want, rtol=1e-13, atol=0)


def test_model_risk_methods_agree_with_the_dense_covariance():
    fdf, ret, dates = _fit_panel()
    rm = _fitted()
    rng = np.random.default_rng(2)
    w = pd.Series(rng.standard_normal(len(fdf)) / 12, index=fdf.index)
    risk, con, marg = rm.portfolio_risk(w), rm.risk_contributions(w), rm.marginal_risk(w)
    assert list(risk.columns) == ["total_var", "factor_var", "specific_var", "vol"]
    assert list(con.columns) == list(fdf.columns) + ["specific"]
    d = int(np.flatnonzero(rm.valid.to_numpy())[-1])
    S = rm.covariance(dates[d])
    wd = w.xs(dates[d], level=0).reindex(S.index)
    v = float(wd.to_numpy() @ S.to_numpy() @ wd.to_numpy())
    assert abs(risk["total_var"].iloc[d] - v) <= 1e-12 * v and abs(risk["vol"].iloc[d] - np.sqrt(v)) <= 1e-12
    assert abs(con.iloc[d].sum() - v) <= 1e-12 * v
    np.testing.assert_allclose(marg.xs(dates[d], level=0).reindex(S.index).to_numpy(), S.to_numpy() @ wd.to_numpy(),
                               rtol=1e-9, atol=1e-15)
    assert risk.iloc[0].isna().all() and not bool(rm.valid.iloc[0])
    both = rm.portfolio_risk(pd.DataFrame({"a": w, "b": 2.0 * w}))
    assert both["a"]["total_var"].to_numpy().tobytes() == risk["total_var"].to_numpy().tobytes()


# ---------------------------------------------------------------------------- 7. routing
def _settings(PS, ret, idx, **kw):
    return PS.SimulationSettings(returns=ret, cap_flag=pd.Series(1.0, index=idx),
                                 investability_flag=pd.Series(1.0, index=idx), factors_df=pd.DataFrame(index=idx),
                                 max_weight=0.4, lookback_period=10, plot=False, **kw)


def test_simulation_routes_mvo_to_the_risk_model(monkeypatch, caplog):
    _engine()
    import factormodeling_amd.portfolio_simulation as PS
    from factormodeling_amd.simulation import mvo_trade_list, risk_mvo_trade_list
    monkeypatch.delenv("FMX_SIM_MVO", raising=False)
    fdf, ret, dates = _fit_panel()
    rm = _fitted()
    feat = pd.Series(np.random.default_rng(9).standard_normal(len(fdf)), index=fdf.index, name="sig")
    sim = PS.Simulation("sig", feat, _settings(PS, ret, fdf.index, method="mvo", risk_model=rm))
    with caplog.at_level(logging.WARNING, logger="portfolio_simulation"):
        w, counts = sim._daily_trade_list()
    want_w, want_c, extra = risk_mvo_trade_list(feat, rm, 0.1, 0.4, return_info=True)
    pd.testing.assert_series_equal(w, want_w, check_exact=True)
    pd.testing.assert_frame_equal(counts, want_c)
    st = extra["info"][:, 0]
    print("statuses:", {int(k): int((st == k).sum()) for k in np.unique(st)})
    assert (st == 0).sum() >= 5 and 1 <= (st == 4).sum() <= int((~rm.valid).sum())      # a flat day is status 3 first
    assert len([r for r in caplog.records if "equal-leg fallback" in r.getMessage()]) == int(((st == 1) | (st == 2)).any())
    with pytest.raises(ValueError, match="out of scope"):
        PS.Simulation("sig", feat, _settings(PS, ret, fdf.index, method="mvo_turnover", risk_model=rm))._daily_trade_list()
    # without the field set: today's mvo_trade_list bytes
    plain = PS.Simulation("sig", feat, _settings(PS, ret, fdf.index, method="mvo"))
    assert plain.risk_model is None
    w0, c0 = plain._daily_trade_list()
    w1, c1 = mvo_trade_list(feat, ret, 0.1, 0.4, 10, 0.1)
    assert w0.to_numpy().tobytes() == w1.to_numpy().tobytes() and w0.index.equals(w1.index)
    pd.testing.assert_frame_equal(c0, c1)
    assert w0.to_numpy().tobytes() != w.to_numpy().tobytes()


def test_multi_manager_with_a_model_is_out_of_scope():
    _engine()
    from factormodeling_amd.multi_manager import compute_multimanager_weights
    fdf, ret, dates = _fit_panel()
    fw = pd.DataFrame(1.0, index=pd.Index(dates, name="date"), columns=["val"])
    with pytest.raises(ValueError, match="out of scope"):
        compute_multimanager_weights(fdf, fw, {"method": "mvo", "returns": ret, "risk_model": _fitted()})
