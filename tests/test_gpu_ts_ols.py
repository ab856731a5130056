"""Rolling multi-factor OLS on the GPU (fmx_ts_ols, engine.ts_ols, operations.ts_regression_multi,
factor_backtest.rolling_factor_exposures) against the brute-force reference of ts_ols_cases.py
(numpy's lstsq on the kept, norm-scaled columns of every window).  Bounds and generators:
ts_ols_cases.py; DESIGN §22 records the maxima these tests print.  Shapes are D = 75, A = 130
(two waves plus two lanes), Fy = 2 unless a test says otherwise."""
import numpy as np
import pandas as pd
import pytest

import ts_ols_cases as C

pytestmark = pytest.mark.gpu

ALL = C.OUTPUTS


def _dev(a, dtype=None):
    import torch
    if a is None:
        return None
    t = torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    return t.to(dtype) if dtype else t


def gpu_ts_ols(Y, X, W, present=None, intercept=True, shared=False, want=ALL):
    import torch
    import factormodeling_amd.engine as E
    out = E.ts_ols(_dev(Y), _dev(X), W, _dev(present, torch.uint8), intercept, shared, want)
    torch.cuda.synchronize()
    assert set(out) == set(want)
    return {k: v.cpu().numpy() for k, v in out.items()}


def check(Y, X, W, present=None, intercept=True, shared=False, assets=C.CHECK_ASSETS, where=""):
    """One call against the reference: NaN patterns and the kept set exact, values within the
    bounds.  Returns (got, ref, err)."""
    ref = C.ref_panel(Y, X, W, present, intercept, shared, assets)
    got = gpu_ts_ols(Y, X, W, present, intercept, shared)
    err = C.errors(got, ref)
    C.assert_within(err, where)
    return got, ref, err


# ------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("intercept", [True, False], ids=["intercept", "origin"])
@pytest.mark.parametrize("gen", C.GRID_GENS)
def test_parity_grid(gen, intercept):
    """K in {1, 2, 3, 5, 8} x W in {2p + 4, 20, 64, 75}; regressors with 1 % NaN, y with 3 %."""
    worst, nvalues = {}, 0
    for K in C.GRID_K:
        Y, X, shared = C.make_case(gen, K)
        for W in C.grid_windows(K, intercept):
            _, ref, err = check(Y, X, W, None, intercept, shared, where=f"{gen} intercept={intercept} K={K} W={W}")
            C.merge_worst(worst, err)
            nvalues += int(ref["exists"][..., ref["assets"]].sum())
    print(f"ts_ols parity {gen} intercept={intercept}: worst {worst} over {nvalues} checked outputs")
    assert nvalues > 5000


# ------------------------------------------------------------------------------------ 2
def ragged_case(K, shared, seed=5):
    """A ragged panel: absent cells, a late listing (asset 5), a symbol with only 9 valid rows
    (asset 7), rows whose y is valid but one regressor is +-inf, an all-NaN date (40)."""
    rng = np.random.default_rng(seed)
    Y, X, _ = C.make_case("shared" if shared else "plain", K, seed=seed)
    pres = (rng.random((C.D, C.A)) > 0.1).astype(np.uint8)
    pres[:30, 5] = 0
    pres[:, 7] = 0
    pres[3:70:8, 7] = 1
    if shared:
        X[K - 1, 33] = np.inf
        X[0, 52] = -np.inf
    else:
        X[K - 1, 33, ::3] = np.inf
        X[0, 52, 1::4] = -np.inf
    Y[:, 40, :] = np.nan
    return Y, X, pres


@pytest.mark.parametrize("shared", [False, True], ids=["panel", "shared"])
def test_row_rule(shared):
    K = 3
    Y, X, pres = ragged_case(K, shared)
    assets = C.CHECK_ASSETS + (5, 7)
    for ic in (True, False):
        p = K + ic
        W = 2 * p + 4
        got, ref, err = check(Y, X, W, pres, ic, shared, assets, where=f"ragged intercept={ic}")
        print(f"ts_ols row rule shared={shared} intercept={ic} W={W}: {err}")
        ex = ref["exists"]
        assert not ex[:, :, 7].any() and not ex[:, 40].any() and not ex[:, :30, 5].any() and ex[:, 60:, 5].any()
        assert not ex[:, 33, 0].any() and not ex[:, 52, 1].any()              # the inf rows drop out
        # W = p and W = p + 1: such windows are nearly singular (kept pivots down to 1e-9), so
        # only the NaN pattern and finiteness are checked, not the values
        for Wn in (p, p + 1):
            got = gpu_ts_ols(Y, X, Wn, pres, ic, shared)
            ex = C.exists(C.valid_rows(Y, X, pres, shared), Wn)
            for k in ("resid", "fitted") + (("alpha",) if ic else ()):
                assert np.array_equal(np.isfinite(got[k]), ex), (k, Wn)
            if not ic:
                assert np.isnan(got["alpha"]).all()
            assert not (np.isfinite(got["beta"]) & ~ex[:, None]).any() and not np.isinf(got["beta"]).any()
            for k in ("r2", "sigma"):
                assert not (~np.isnan(got[k]) & ~ex).any() and not np.isinf(got[k]).any(), (k, Wn)
            if Wn == p:                                   # no degrees of freedom unless a column was dropped
                full = ex & ~np.isnan(got["beta"]).any(axis=1)
                assert np.isnan(got["sigma"][full]).all()
    got = gpu_ts_ols(Y, X, 80, pres, True, shared)       # W > D: all NaN, not refused
    assert all(np.isnan(v).all() for v in got.values())


# ------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("A", [1, 63, 64, 65])
def test_edge_widths(A):
    K, Dn = 3, 40
    for gen in ("plain", "shared"):
        Y, X, shared = C.make_case(gen, K, Dn, A, 1, seed=A)
        _, ref, err = check(Y, X, 12, None, True, shared, assets=None, where=f"A={A} {gen}")
        print(f"ts_ols A={A} {gen}: {err} over {int(ref['exists'].sum())} outputs")
        assert A == 1 or ref["exists"].sum() > 100


def test_single_date():
    """D = 1: a window of one row exists only for W = 1 (K = 1 through the origin: an exact fit)."""
    rng = np.random.default_rng(8)
    Y, X = rng.standard_normal((2, 1, 70)), rng.standard_normal((1, 1, 70)) + 3.0
    Y[0, 0, 4] = np.nan
    got = gpu_ts_ols(Y, X, 1, None, False)
    ok = np.isfinite(Y)
    assert np.array_equal(np.isfinite(got["beta"][:, 0]), ok) and np.isnan(got["alpha"]).all()
    np.testing.assert_allclose(got["beta"][:, 0][ok], (Y / X)[ok], rtol=1e-14)
    assert np.abs(got["resid"][ok]).max() <= 1e-14 * np.abs(Y[ok]).max()    # a handful of roundings
    assert np.isnan(got["sigma"]).all()                  # W - p = 0
    got = gpu_ts_ols(Y, X, 2, None, True)                # W = 2 > D
    assert all(np.isnan(v).all() for v in got.values())


# ------------------------------------------------------------------------------------ 4
def test_constant_runs_inside_windows():
    """A regressor constant over a run of dates longer than W is dropped exactly in the windows
    that lie inside the run (0.1: the 1e-13 rule; 3.25: an exactly zero scale), kept elsewhere."""
    K, W = 4, 14
    Y, X, _ = C.make_case("plain", K, nans=False)
    X[1, 20:50] = 0.1
    X[2, 35:60] = 3.25
    got, ref, err = check(Y, X, W, None, True, False, where="constant runs")
    d = np.arange(C.D)
    inside1 = (d - W + 1 >= 20) & (d <= 49)
    inside2 = (d - W + 1 >= 35) & (d <= 59)
    nb = np.isnan(got["beta"])
    has = d >= W - 1
    assert (nb[:, 1] == (inside1 | ~has)[None, :, None]).all() and (nb[:, 2] == (inside2 | ~has)[None, :, None]).all()
    assert (nb[:, 0] == ~has[None, :, None]).all() and (nb[:, 3] == ~has[None, :, None]).all()
    assert (inside1 & inside2).any()
    print(f"ts_ols constant runs: {err}")


@pytest.mark.parametrize("shared", [False, True], ids=["panel", "shared"])
def test_duplicate_column(shared):
    K, W = 5, 16
    Y, X, _ = C.make_case("shared" if shared else "plain", K)
    X[K - 1] = X[0]
    got, ref, err = check(Y, X, W, None, True, shared, where="duplicate")
    ex = ref["exists"]
    assert np.isnan(got["beta"][:, K - 1]).all() and np.array_equal(np.isfinite(got["beta"][:, 0]), ex)
    pv = ref["pivots"][:, K - 1][ex & np.isin(np.arange(C.A), ref["assets"])]
    assert np.abs(pv).max() <= 1e-12
    print(f"ts_ols duplicate column shared={shared}: {err}")


def test_full_dummies_with_intercept():
    """Three 0/1 columns that sum to the constant in every window, then a free column: with an
    intercept the in-order factorisation drops the LAST dummy; without one nothing is dropped."""
    K, W = 4, 14
    Y, X, _ = C.make_case("plain", K, nans=False)
    g = (np.arange(C.D)[:, None] + np.arange(C.A)[None, :]) % 3
    for k in range(3):
        X[k] = (g == k).astype(np.float64)
    Y[0][np.random.default_rng(3).random((C.D, C.A)) < 0.03] = np.nan
    got, ref, err = check(Y, X, W, None, True, False, where="dummies")
    ex = ref["exists"]
    assert np.isnan(got["beta"][:, 2]).all()
    for k in (0, 1, 3):
        assert np.array_equal(np.isfinite(got["beta"][:, k]), ex)
    got0, _, err0 = check(Y, X, W, None, False, False, where="dummies, no intercept")
    assert np.array_equal(np.isfinite(got0["beta"]), np.broadcast_to(ex[:, None], got0["beta"].shape))
    print(f"ts_ols dummies: {err} / without intercept {err0}")


# ------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("K,W", [(3, 12), (8, 22)])
def test_determinism(K, W):
    Y, Xs, _ = C.make_case("shared", K)
    Xp = C.as_panel(Xs, C.A)
    a = gpu_ts_ols(Y, Xp, W)
    b = gpu_ts_ols(Y, Xp, W)
    s = gpu_ts_ols(Y, Xs, W, shared=True)
    assert np.isfinite(a["resid"]).sum() > 1000
    for k in ALL:
        assert a[k].tobytes() == b[k].tobytes(), f"{k}: two runs differ"
        assert a[k].tobytes() == s[k].tobytes(), f"{k}: a shared table differs from its broadcast panel"
    for f in range(C.FY):                                # a y column alone
        one = gpu_ts_ols(Y[f:f + 1], Xp, W)
        for k in ALL:
            assert one[k][0].tobytes() == a[k][f].tobytes(), f"{k}: y column {f} alone differs from the batch"
    for col in (0, 63, 64, 129):                         # an asset column alone: another lane, another geometry
        one = gpu_ts_ols(Y[:, :, col:col + 1], Xp[:, :, col:col + 1], W)
        for k in ALL:
            assert np.ascontiguousarray(one[k][..., 0]).tobytes() == np.ascontiguousarray(a[k][..., col]).tobytes(), \
                f"{k}: asset column {col} alone differs from the batch"


# ------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("gapped", [False, True], ids=["dense", "gapped"])
def test_k1_matches_ts_regression(gapped):
    """K = 1 against the existing one-regressor kernel (engine.ts_regression, rettypes 0-3 and
    6) on well-conditioned N(0, 1) data, within the bound measured on the host."""
    import torch
    import factormodeling_amd.engine as E
    y, x = C.k1_panel(gapped)
    valid = (np.isfinite(y) & np.isfinite(x)).astype(np.uint8)
    worst = {}
    for W in (8, 20):
        got = gpu_ts_ols(y[None], x[None], W)
        mine = {k: (got[k][0, 0] if k == "beta" else got[k][0]) for k in ("resid", "alpha", "beta", "fitted", "r2")}
        yv, xv = _dev(np.nan_to_num(y)), _dev(np.nan_to_num(x))

        def fast(rt):
            return E.ts_regression(yv, xv, _dev(valid, torch.uint8), W, rt).cpu().numpy()

        C.merge_worst(worst, C.k1_errors(mine, y, x, W, fast))
    print(f"ts_ols K=1 vs engine.ts_regression gapped={gapped}: worst {worst}")
    C.assert_within(worst, "K = 1 vs ts_regression", C.K1_BOUNDS)


# ------------------------------------------------------------------------------------ 7
def test_refusals():
    import torch
    import factormodeling_amd.engine as E
    from factormodeling_amd._lib import FmxError, call, ptr, stream_ptr
    Dn, An = 6, 8
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    for K, W, ic in ((9, 20, 1), (3, 3, 1), (3, 2, 0), (0, 5, 1)):
        Y, X = z(1, Dn, An), torch.ones((max(K, 1), Dn, An), dtype=torch.float64, device="cuda")
        outs = [torch.full((1, max(K, 1), Dn, An) if i == 0 else (1, Dn, An), 7.0, dtype=torch.float64, device="cuda")
                for i in range(6)]
        work = torch.full((1, Dn, An), 7, dtype=torch.uint8, device="cuda")
        with pytest.raises(FmxError, match="ts_ols"):
            call("fmx_ts_ols", ptr(Y), ptr(X), None, 1, K, Dn, An, An, W, ic, 0, *(ptr(o) for o in outs), ptr(work),
                 stream_ptr())
        torch.cuda.synchronize()
        assert all(bool((o == 7).all()) for o in outs) and bool((work == 7).all()), "touched by a refused call"
        if K >= 1:
            with pytest.raises(FmxError):
                E.ts_ols(Y, X, W, intercept=bool(ic))
    with pytest.raises(FmxError):
        call("fmx_ts_ols", ptr(z(1, Dn, An)), ptr(z(2, Dn, An)), None, 1, 2, Dn, An, An - 1, 5, 1, 0, *([None] * 6),
             ptr(torch.zeros((1, Dn, An), dtype=torch.uint8, device="cuda")), stream_ptr())          # ld < A
    with pytest.raises(FmxError):
        call("fmx_ts_ols", ptr(z(1, Dn, An)), None, None, 1, 2, Dn, An, An, 5, 1, 0, *([None] * 7), stream_ptr())
    for bad in (lambda: E.ts_ols(z(2, Dn, An), z(2, Dn, An + 1), 4),                   # shape mismatches
                lambda: E.ts_ols(z(2, Dn, An), z(2, Dn + 1, An), 4),
                lambda: E.ts_ols(z(2, Dn, An), z(2, Dn), 4),                          # a table, not declared shared
                lambda: E.ts_ols(z(2, Dn, An), z(2, Dn, An), 4, shared=True),
                lambda: E.ts_ols(z(2, Dn, An), z(2, Dn + 1), 4, shared=True),
                lambda: E.ts_ols(z(2, Dn, An), z(0, Dn, An), 4),
                lambda: E.ts_ols(z(2, Dn, An), z(2, Dn, An), 4,
                                 present=torch.ones((Dn, An - 1), dtype=torch.uint8, device="cuda")),
                lambda: E.ts_ols(z(2, Dn, An), z(2, Dn, An).float(), 4)):
        with pytest.raises(FmxError):
            bad()
    with pytest.raises(ValueError):
        E.ts_ols(z(2, Dn, An), z(2, Dn, An), 4, want=("beta", "tstat"))


# ------------------------------------------------------------------------------------ 8
def _ragged_frame(nd, ns, K, seed):
    """Long (date, symbol) frame with ~8 % of the rows missing and one symbol listed late."""
    rng = np.random.default_rng(seed)
    dates = pd.bdate_range("2021-01-04", periods=nd)
    syms = [f"S{i:02d}" for i in range(ns)]
    idx = pd.MultiIndex.from_product([dates, syms], names=["date", "symbol"])
    keep = rng.random(len(idx)) > 0.08
    keep &= ~((idx.get_level_values("symbol") == syms[3]) & (idx.get_level_values("date") < dates[nd // 3]))
    idx = idx[keep]
    Xv = rng.standard_normal((len(idx), K))
    Xv[rng.random(Xv.shape) < 0.02] = np.nan
    X = pd.DataFrame(Xv, index=idx, columns=[f"x{k}" for k in range(K)])
    return idx, X, rng


def _symbol_loop(y, Xrows, W, intercept):
    """Per-symbol numpy loop: ``Xrows`` holds every row's regressors (on y.index).  Returns a
    frame on y.index with resid, fitted, alpha, r2, sigma, ymax and the beta / sd columns."""
    K = Xrows.shape[1]
    names = ["resid", "fitted", "alpha", "r2", "sigma", "ymax"] + [f"b{k}" for k in range(K)] + [f"sd{k}" for k in range(K)]
    out = pd.DataFrame(np.nan, index=y.index, columns=names)
    pos = pd.Series(np.arange(len(y)), index=y.index)
    yv, Xv, ov = y.to_numpy(), Xrows.to_numpy(), out.to_numpy()
    for _, rows in pos.groupby(level="symbol"):
        r = rows.to_numpy()                               # the symbol's rows, in date order
        r = r[np.isfinite(yv[r]) & np.isfinite(Xv[r]).all(axis=1)]
        for i in range(W - 1, r.size):
            win = r[i - W + 1:i + 1]
            w = C.window_fit(yv[win], Xv[win], intercept, "lstsq")
            ov[r[i]] = [w["resid"], w["fitted"], w["alpha"], w["r2"], w["sigma"], w["ymax"], *w["beta"], *w["sd"]]
    return pd.DataFrame(ov, index=y.index, columns=names)


def _frame_errors(got, ref, rt, K):
    if rt == "beta":
        g, r = got.to_numpy(), ref[[f"b{k}" for k in range(K)]].to_numpy()
        e = np.abs(g - r) * ref[[f"sd{k}" for k in range(K)]].to_numpy() / ref[["ymax"]].to_numpy()
    else:
        g, r = got.to_numpy(), ref[rt].to_numpy()
        e = np.abs(g - r) / (1.0 if rt == "r2" else ref["ymax"].to_numpy())
    assert np.array_equal(np.isnan(g), np.isnan(r)), f"{rt}: NaN pattern differs"
    return float(np.nanmax(e)) if np.isfinite(e).any() else 0.0


@pytest.mark.parametrize("lag", [0, 1])
def test_dropin_ragged_frame(lag):
    """ts_regression_multi on a ragged 40 x 30 frame, K = 3: per-symbol X, then a shared table."""
    import factormodeling_amd.operations as ops
    K, W = 3, 12
    idx, X, rng = _ragged_frame(40, 30, K, 31)
    y = pd.Series(0.01 * X.fillna(0.0).to_numpy().sum(axis=1) + 0.01 * rng.standard_normal(len(idx)), index=idx, name="ret")
    y[rng.random(len(idx)) < 0.03] = np.nan
    dates = idx.get_level_values("date").unique().sort_values()
    tab = pd.DataFrame(rng.standard_normal((len(dates), K)), index=dates, columns=["mkt", "smb", "hml"])
    tab.iloc[17, 1] = np.nan
    ys = pd.Series(0.01 * tab.fillna(0.0).to_numpy().sum(axis=1)[dates.get_indexer(idx.get_level_values("date"))] * rng.uniform(0.5, 1.5, len(idx))
                   + 0.01 * rng.standard_normal(len(idx)), index=idx, name="ret")
    worst = {}
    for kind, yy, Xin, Xrows in (
            ("panel", y, X.sample(frac=1.0, random_state=1).iloc[:-7], None),
            ("shared", ys, tab.iloc[::-1].drop(dates[5]), None)):
        if kind == "panel":
            Xrows = Xin.reindex(idx).groupby(level="symbol").shift(lag) if lag else Xin.reindex(idx)
        else:
            t = Xin.reindex(dates).shift(lag)
            Xrows = pd.DataFrame(t.to_numpy()[dates.get_indexer(idx.get_level_values("date"))], index=idx, columns=t.columns)
        for ic in (True, False):
            ref = _symbol_loop(yy, Xrows, W, ic)
            assert ref["resid"].notna().sum() > 300
            for rt in ("resid", "fitted", "alpha", "r2", "sigma", "beta"):
                got = ops.ts_regression_multi(yy, Xin, W, lag=lag, rettype=rt, intercept=ic)
                assert got.index.equals(idx)
                if rt == "beta":
                    assert isinstance(got, pd.DataFrame) and list(got.columns) == list(Xin.columns)
                else:
                    assert isinstance(got, pd.Series) and got.name == "ret" and got.dtype == np.float64
                e = _frame_errors(got, ref, rt, K)
                worst[rt] = max(worst.get(rt, 0.0), e)
                assert e <= C.BOUNDS[rt], (kind, rt, ic, e)
    y2 = pd.DataFrame({"a": y, "b": y * 2.0 + 0.01 * rng.standard_normal(len(idx))})
    gf = ops.ts_regression_multi(y2, X, W, lag=lag, rettype="sigma")      # a DataFrame y: one batched call
    assert isinstance(gf, pd.DataFrame) and list(gf.columns) == ["a", "b"] and gf.index.equals(idx)
    for c in y2.columns:
        one = ops.ts_regression_multi(y2[c], X, W, lag=lag, rettype="sigma")
        assert one.name == c and one.to_numpy().tobytes() == gf[c].to_numpy().tobytes()
    print(f"ts_regression_multi ragged 40 x 30 x 3 lag={lag}: worst {worst}")


def test_rolling_factor_exposures():
    """60 x 40 x 4, the factor returns from cross_sectional_factor_returns."""
    from factormodeling_amd.factor_backtest import cross_sectional_factor_returns, rolling_factor_exposures
    nd, ns, K, W = 60, 40, 4, 14
    idx, F, rng = _ragged_frame(nd, ns, K, 41)
    ret = pd.Series(0.01 * rng.standard_normal(len(idx)), index=idx, name="ret")
    table = cross_sectional_factor_returns(F, ret, lag=1)
    assert table.shape == (nd, K) and table.iloc[0].isna().all() and table.iloc[2:].notna().all().all()
    beta, resid, sigma = rolling_factor_exposures(ret, table, W)
    assert isinstance(beta, pd.DataFrame) and beta.index.equals(idx) and list(beta.columns) == list(F.columns)
    assert isinstance(resid, pd.Series) and resid.index.equals(idx) and sigma.index.equals(idx)
    Xrows = pd.DataFrame(table.to_numpy()[table.index.get_indexer(idx.get_level_values("date"))], index=idx,
                         columns=table.columns)
    ref = _symbol_loop(ret, Xrows, W, True)
    assert ref["resid"].notna().sum() > 1000
    err = {rt: _frame_errors(g, ref, rt, K) for rt, g in (("beta", beta), ("resid", resid), ("sigma", sigma))}
    print(f"rolling_factor_exposures 60 x 40 x 4: {err}")
    C.assert_within(err, "rolling_factor_exposures")
    b0, r0, s0 = rolling_factor_exposures(ret, table, W, intercept=False)
    ref0 = _symbol_loop(ret, Xrows, W, False)
    C.assert_within({rt: _frame_errors(g, ref0, rt, K) for rt, g in (("beta", b0), ("resid", r0), ("sigma", s0))},
                    "rolling_factor_exposures, no intercept")
