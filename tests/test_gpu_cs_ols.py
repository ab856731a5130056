"""cs_ols on the GPU (fmx_cs_ols, engine.cs_ols, operations.cs_regression_multi,
factor_backtest.cross_sectional_factor_returns) against numpy's lstsq on the kept columns.
Bounds and generators: cs_ols_cases.py (DESIGN §19 records the maxima these tests print)."""
import numpy as np
import pandas as pd
import pytest

import cs_ols_cases as C

pytestmark = pytest.mark.gpu

ALL = ("beta", "alpha", "r2", "n", "resid", "fitted")
D, FY = 4, 3


def _dev(a, dtype=None):
    import torch
    if a is None:
        return None
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(dtype) if dtype else \
        torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def gpu_ols(Y, X, W=None, present=None, intercept=True, want=ALL):
    import torch
    import factormodeling_amd.engine as E
    out = E.cs_ols(_dev(Y), _dev(X), _dev(W), _dev(present, torch.uint8), intercept, want)
    torch.cuda.synchronize()
    assert set(out) == set(want)
    return {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("intercept", [True, False], ids=["intercept", "origin"])
@pytest.mark.parametrize("gen", C.GRID_GENS)
def test_parity_grid(gen, intercept):
    worst = {}
    for A in C.GRID_A:
        for K in C.GRID_K:
            Y, X, W = C.make_case(gen, K, D, A, FY)
            ref = C.run_panel(Y, X, W, None, intercept, "lstsq")
            got = gpu_ols(Y, X, W, None, intercept)
            assert got["n"].dtype == np.int32
            err = C.errors(got, ref)
            C.merge_worst(worst, err)
            C.assert_within(err, f"{gen} intercept={intercept} A={A} K={K}")
            nb = np.isnan(got["beta"])
            assert (nb == ~ref["kept"]).all()
    print(f"cs_ols parity {gen} intercept={intercept}: worst {worst}")


# ------------------------------------------------------------------------------------ 2
def test_validity():
    K, Dv, A = 4, 9, 70
    p = K + 1
    Y, X, _ = C.make_case("plain", K, Dv, A, FY)
    rng = np.random.default_rng(3)
    W = rng.uniform(0.1, 1.1, (Dv, A))
    pres = np.ones((Dv, A), dtype=np.uint8)
    Y[0][rng.random((Dv, A)) < 0.1] = np.nan           # NaNs that differ per y column
    Y[1][rng.random((Dv, A)) < 0.2] = np.nan
    Y[2, 0, 3] = np.inf
    X[2, 1, ::5] = np.nan                               # NaNs in a single x column
    X[0, 1, 4] = -np.inf
    pres[2, rng.random(A) < 0.3] = 0                    # absent rows
    Y[:, 3, :] = np.nan                                 # an all-NaN date
    for d, n in ((4, p - 1), (5, p), (6, p + 1)):       # n = p - 1, p, p + 1
        Y[:, d, :n] = 0.01 * rng.standard_normal((FY, n))
        Y[:, d, n:] = np.nan
    W[7, :10] = 0.0                                     # zero, negative and NaN weights
    W[7, 10:13] = np.nan
    W[7, 13] = -1.0
    pres[8, :] = 0                                      # a date with no rows at all
    for w in (W, None):
        for ic in (True, False):
            ref = C.run_panel(Y, X, w, pres, ic, "lstsq")
            got = gpu_ols(Y, X, w, pres, ic)
            err = C.errors(got, ref)
            print(f"cs_ols validity weights={w is not None} intercept={ic}: {err}")
            C.assert_within(err, "validity")
            if ic:
                assert got["n"][:, 4].tolist() == [p - 1] * FY and np.isnan(got["beta"][:, 4]).all()
                assert np.isfinite(got["beta"][:, 5:7]).all()
            assert (got["n"][:, 3] == 0).all() and (got["n"][:, 8] == 0).all()
            if w is not None:
                assert np.isnan(got["resid"][:, 7, :14]).all()


# ------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("gen,K,A", [("const", 3, 65), ("const", 32, 1100), ("dup", 2, 64), ("dup", 16, 257),
                                     ("dup", 32, 1100), ("dummies", 3, 63), ("dummies", 7, 257),
                                     ("dummies", 32, 1100)])
def test_collinearity(gen, K, A):
    Y, X, W = C.make_case(gen, K, D, A, FY)
    ref = C.run_panel(Y, X, W, None, True, "lstsq")
    got = gpu_ols(Y, X, W, None, True)
    exp = np.zeros(K, dtype=bool)
    exp[C.expected_dropped(gen, K)] = True
    assert (np.isnan(got["beta"]) == exp).all(), "NaN betas exactly at the dropped columns"
    assert (ref["kept"] == ~exp).all()
    err = C.errors(got, ref)
    print(f"cs_ols collinearity {gen} K={K} A={A}: {err}")
    C.assert_within(err, gen)


# ------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("A", [2, 5, 65, 1100, 5000])
def test_k1_matches_cs_regression(A):
    """K = 1 with an intercept and no weights is cs_regression: same operations in another
    order, so 1e-12 relative (to the largest magnitude of the date's reference values; for
    resid, of the date's y)."""
    import torch
    import factormodeling_amd.engine as E
    Y, X, _ = C.make_case("plain", 1, D, A, 1)
    Y = Y + 0.05                                        # alpha away from zero: a relative bound
    rng = np.random.default_rng(5)
    Y[0][rng.random((D, A)) < 0.05] = np.nan
    X[0][rng.random((D, A)) < 0.05] = np.nan
    pres = (rng.random((D, A)) > 0.1).astype(np.uint8)
    got = gpu_ols(Y, X, None, pres, True)
    valid = ~np.isnan(got["resid"][0])
    worst = {}
    for rt in ("resid", "beta", "alpha", "fitted", "r2"):
        ref = E.cs_regression(_dev(Y[0]), _dev(X[0]), rt, _dev(pres, torch.uint8)).cpu().numpy()
        assert (np.isnan(ref) == ~valid).all(), rt
        mine = got[rt][0] if rt in ("resid", "fitted") else np.where(
            valid, (got["beta"][0, :, 0] if rt == "beta" else got[rt][0])[:, None], np.nan)
        for d in range(D):
            if valid[d].any():
                # resid is y minus fitted: its rounding error scales with y (an exact fit, n = 2,
                # leaves residuals that are nothing but that error)
                scale = np.abs((Y[0, d] if rt == "resid" else ref[d])[valid[d]]).max()
                e = np.abs(mine[d] - ref[d])[valid[d]].max() / scale
                worst[rt] = max(worst.get(rt, 0.0), float(e))
    print(f"cs_ols K=1 vs cs_regression A={A}: {worst}")
    assert all(v <= 1e-12 for v in worst.values()), worst


# ------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("K,A", [(7, 1100), (32, 257)])
def test_determinism(K, A):
    Y, X, W = C.make_case("weights", K, D, A, FY)
    Y[1][np.random.default_rng(2).random((D, A)) < 0.1] = np.nan
    a = gpu_ols(Y, X, W, None, True)
    b = gpu_ols(Y, X, W, None, True)
    for k in ALL:
        assert a[k].tobytes() == b[k].tobytes(), f"{k}: two runs differ"
    for f in range(FY):
        one = gpu_ols(Y[f:f + 1], X, W, None, True)
        for k in ALL:
            assert one[k][0].tobytes() == a[k][f].tobytes(), f"{k}: column {f} alone differs from the batch"


# ------------------------------------------------------------------------------------ 6
def _raw_call(Fy, K, Dn, A, Y, X, outs):
    from factormodeling_amd._lib import call, ptr, stream_ptr
    call("fmx_cs_ols", ptr(Y), ptr(X), None, None, Fy, K, Dn, A, A, 1, *(ptr(o) for o in outs), stream_ptr())


@pytest.mark.parametrize("K,A", [(33, 8), (1, 16385)])
def test_refusals_caps(K, A):
    import torch
    import factormodeling_amd.engine as E
    from factormodeling_amd._lib import FmxError
    Y = torch.zeros((1, 1, A), dtype=torch.float64, device="cuda")
    X = torch.ones((K, 1, A), dtype=torch.float64, device="cuda")
    outs = [torch.full(s, 7, dtype=t, device="cuda") for s, t in
            (((1, 1, K), torch.float64), ((1, 1), torch.float64), ((1, 1), torch.float64), ((1, 1), torch.int32),
             ((1, 1, A), torch.float64), ((1, 1, A), torch.float64))]
    with pytest.raises(FmxError, match="cs_ols"):
        _raw_call(1, K, 1, A, Y, X, outs)
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs), "outputs touched by a refused call"
    with pytest.raises(FmxError):
        E.cs_ols(Y, X)


def test_refusals_shapes():
    import torch
    import factormodeling_amd.engine as E
    from factormodeling_amd._lib import FmxError
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    with pytest.raises(FmxError):
        E.cs_ols(z(2, 3, 8), z(2, 3, 9))
    with pytest.raises(FmxError):
        E.cs_ols(z(2, 3, 8), z(2, 4, 8))
    with pytest.raises(FmxError):
        E.cs_ols(z(2, 3, 8), z(2, 3, 8), W=z(3, 7))
    with pytest.raises(FmxError):
        E.cs_ols(z(2, 3, 8), z(2, 3, 8), present=torch.ones((3, 7), dtype=torch.uint8, device="cuda"))
    with pytest.raises(FmxError):
        E.cs_ols(z(2, 3, 8), z(0, 3, 8))


# ------------------------------------------------------------------------------------ 7
def _ragged_panel(nd, ns, K, seed):
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


def _host_loop(y, X, w, intercept):
    """Per-date lstsq on the date's valid rows (pandas groupby)."""
    K = X.shape[1]
    cols = {k: pd.Series(np.nan, index=y.index) for k in ("resid", "fitted", "alpha", "r2")}
    beta = {}
    df = pd.concat([y.rename("__y"), X, (w if w is not None else pd.Series(1.0, index=y.index)).rename("__w")], axis=1)
    for date, g in df.groupby(level="date"):
        ok = np.isfinite(g.to_numpy()).all(axis=1) & (g["__w"].to_numpy() > 0)
        beta[date] = np.full(K, np.nan)
        if ok.sum() < K + intercept:
            continue
        gv = g[ok]
        r = C.lstsq_one(gv["__y"].to_numpy(), gv[X.columns].to_numpy(), gv["__w"].to_numpy(), intercept,
                        np.ones(K, dtype=bool))
        cols["resid"].loc[gv.index] = r["resid"]
        cols["fitted"].loc[gv.index] = r["fitted"]
        cols["alpha"].loc[gv.index] = r["alpha"]
        cols["r2"].loc[gv.index] = r["r2"]
        beta[date] = r["beta"]
    return cols, pd.DataFrame.from_dict(beta, orient="index", columns=X.columns)


def test_dropin_ragged_panel():
    import factormodeling_amd.operations as ops
    K = 5
    idx, X, rng = _ragged_panel(40, 30, K, 11)
    y = pd.Series(0.01 * X.fillna(0.0).to_numpy()[:, :3].sum(axis=1) + 0.01 * rng.standard_normal(len(idx)),
                  index=idx, name="ret")
    y[rng.random(len(idx)) < 0.03] = np.nan
    y2 = pd.DataFrame({"a": y, "b": y * 2.0 + 0.01 * rng.standard_normal(len(idx))})
    w = pd.Series(rng.uniform(0.1, 1.1, len(idx)), index=idx)
    # X and weights on other row sets: they are reindexed onto y.index
    Xs = X.sample(frac=1.0, random_state=1).iloc[:-7]
    ws = w.iloc[5:]
    X_al, w_al = Xs.reindex(idx), ws.reindex(idx)
    worst = {}
    for ic, wt, wal in ((True, None, None), (False, None, None), (True, ws, w_al)):
        ref, ref_beta = _host_loop(y, X_al, wal, ic)
        fit_rows = ref["resid"].notna()
        ymax = y.abs().where(fit_rows).groupby(level="date").transform("max")
        for rt in ("resid", "fitted", "alpha", "r2"):
            got = ops.cs_regression_multi(y, Xs, rettype=rt, intercept=ic, weights=wt)
            assert isinstance(got, pd.Series) and got.index is y.index or got.index.equals(y.index)
            assert got.name == "ret" and got.dtype == np.float64
            assert (got.isna() == ref[rt].isna()).all(), rt
            scale = 1.0 if rt == "r2" else ymax
            e = ((got - ref[rt]).abs() / scale).max()
            e = 0.0 if np.isnan(e) else float(e)          # alpha is NaN everywhere without an intercept
            worst[rt] = max(worst.get(rt, 0.0), e)
            assert e <= C.BOUNDS[rt], (rt, ic, e)
        gb = ops.cs_regression_multi(y, Xs, rettype="beta", intercept=ic, weights=wt)
        assert isinstance(gb, pd.DataFrame) and list(gb.columns) == list(X.columns) and gb.index.name == "date"
        assert gb.index.equals(pd.Index(idx.get_level_values("date").unique().sort_values(), name="date"))
        assert (gb.isna().to_numpy() == ref_beta.isna().to_numpy()).all()
        sd = X_al.where(np.broadcast_to(fit_rows.to_numpy()[:, None], X_al.shape)) \
            .groupby(level="date").std(ddof=0).to_numpy()
        ym = y.abs().where(fit_rows).groupby(level="date").max().to_numpy()[:, None]
        e = float(np.nanmax(np.abs(gb.to_numpy() - ref_beta.to_numpy()) * sd / ym))
        worst["beta"] = max(worst.get("beta", 0.0), e)
        assert e <= C.BETA_BOUND, e
    # a DataFrame y is one batched call: same bits as its columns one by one
    for rt in ("resid", "r2"):
        gf = ops.cs_regression_multi(y2, Xs, rettype=rt)
        assert isinstance(gf, pd.DataFrame) and list(gf.columns) == ["a", "b"] and gf.index.equals(y2.index)
        assert (gf.dtypes == np.float64).all()
        for c in y2.columns:
            one = ops.cs_regression_multi(y2[c], Xs, rettype=rt)
            assert one.name == c and one.to_numpy().tobytes() == gf[c].to_numpy().tobytes()
    with pytest.raises(ValueError):
        ops.cs_regression_multi(y2, Xs, rettype="beta")
    print(f"cs_regression_multi ragged 40 x 30 x 5: worst {worst}")


# ------------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("lag", [1, 2])
def test_pure_factor_returns(lag):
    import factormodeling_amd.factor_selector as fs
    from factormodeling_amd.factor_backtest import cross_sectional_factor_returns
    nd, ns, K = 60, 40, 6
    idx, X, rng = _ragged_panel(nd, ns, K, 20 + lag)
    ret = pd.Series(0.01 * rng.standard_normal(len(idx)), index=idx, name="ret")
    got, stats = cross_sectional_factor_returns(X, ret, lag=lag, full=True)
    assert cross_sectional_factor_returns(X, ret, lag=lag).equals(got)
    dates = pd.Index(idx.get_level_values("date").unique().sort_values(), name="date")
    assert got.index.equals(dates) and got.index.name == "date" and list(got.columns) == list(X.columns)
    assert list(stats.columns) == ["alpha", "r2", "n"] and stats.index.equals(dates)
    Xl = X.groupby(level="symbol").shift(lag)
    ref, ref_beta = _host_loop(ret, Xl, None, True)
    assert (got.isna().to_numpy() == ref_beta.isna().to_numpy()).all()
    assert got.iloc[:lag].isna().all().all() and got.iloc[lag + 1:].notna().all().all()
    ok = np.isfinite(pd.concat([ret, Xl], axis=1).to_numpy()).all(axis=1)
    sd = Xl.where(np.broadcast_to(ok[:, None], Xl.shape)).groupby(level="date").std(ddof=0).to_numpy()
    ym = ret.abs().where(ok).groupby(level="date").max().to_numpy()[:, None]
    e = float(np.nanmax(np.abs(got.to_numpy() - ref_beta.to_numpy()) * sd / ym))
    ea = float(np.nanmax(np.abs(stats["alpha"].to_numpy() - ref["alpha"].groupby(level="date").first().to_numpy())
                         / ym[:, 0]))
    er = float(np.nanmax(np.abs(stats["r2"].to_numpy() - ref["r2"].groupby(level="date").first().to_numpy())))
    print(f"cross_sectional_factor_returns lag={lag}: beta {e} alpha {ea} r2 {er}")
    assert e <= C.BETA_BOUND and ea <= C.ALPHA_BOUND and er <= C.R2_BOUND
    assert (stats["n"].to_numpy() == pd.Series(ok, index=idx).groupby(level="date").sum().to_numpy()).all()
    sel = fs.FactorSelector(X, ret, got, window=20, method="momentum", method_kwargs={}).prepare_selection()
    assert len(sel) > 0 and np.isfinite(sel.to_numpy()).all()
