"""cs_ols without a GPU: the numpy model of DESIGN §19's algorithm against numpy's lstsq on
every generator, the dropped sets, the public surface, and the loud failure without a device."""
import inspect
import os

import numpy as np
import pandas as pd
import pytest

import cs_ols_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def grid_worst():
    """Worst model-vs-lstsq error per quantity over the parity grid (computed once)."""
    worst, min_kept = {}, np.inf
    for gen in C.GRID_GENS:
        for ic in (True, False):
            for A in C.GRID_A:
                for K in C.GRID_K:
                    Y, X, W = C.make_case(gen, K, 4, A)
                    ref = C.run_panel(Y, X, W, None, ic, "lstsq")
                    mod = C.run_panel(Y, X, W, None, ic, "model")
                    assert mod["kept"][mod["n"] >= K + ic].all(), (gen, ic, A, K)   # nothing dropped
                    C.merge_worst(worst, C.errors(mod, ref))
                    pv = ref["pivots"][ref["kept"]]
                    if pv.size:
                        min_kept = min(min_kept, float(pv.min()))
    return worst, min_kept


def test_model_worst_against_lstsq(grid_worst):
    """The model's worst difference from lstsq (printed: cs_ols_cases.MEASURED_MODEL_WORST
    records these figures, and the beta / alpha / r2 bounds are 25 x them) is within the
    bounds; the kept pivots stay far above the drop threshold."""
    worst, min_kept = grid_worst
    print("model vs lstsq, worst over the grid:", worst, "min kept pivot:", min_kept)
    C.assert_within(worst, "model vs lstsq")
    assert min_kept > 1e4 * C.PIVOT_MIN


def test_bounds_follow_the_rule():
    """beta / alpha / r2: 25 x the model's measured worst, rounded up to a power of ten."""
    for k, b in (("beta", C.BETA_BOUND), ("alpha", C.ALPHA_BOUND), ("r2", C.R2_BOUND)):
        assert b == 10.0 ** np.ceil(np.log10(25 * C.MEASURED_MODEL_WORST[k])), k
    assert C.RESID_BOUND == 1e-9


@pytest.mark.parametrize("gen", ["const", "dup", "dummies"])
@pytest.mark.parametrize("K", [3, 7, 32])
def test_dropped_sets(gen, K):
    Y, X, W = C.make_case(gen, K, 4, 257)
    ref = C.run_panel(Y, X, W, None, True, "lstsq")
    mod = C.run_panel(Y, X, W, None, True, "model")
    exp = np.ones(K, dtype=bool)
    exp[C.expected_dropped(gen, K)] = False
    assert (mod["kept"] == exp).all()
    assert (np.isnan(mod["beta"]) == ~exp).all()
    dropped_piv = mod["pivots"][..., ~exp]
    if np.isfinite(dropped_piv).any():                  # a constant column is dropped before it has a pivot
        assert np.nanmax(np.abs(dropped_piv)) < 1e-2 * C.PIVOT_MIN
    assert mod["pivots"][..., exp].min() > 1e4 * C.PIVOT_MIN
    C.assert_within(C.errors(mod, ref), f"{gen} K={K}")


def test_model_validity_and_small_n():
    """n < p gives NaN everywhere but n; zero / NaN weights, absent rows and NaNs drop rows."""
    K, D, A = 3, 5, 40
    Y, X, _ = C.make_case("plain", K, D, A, Fy=2)
    W = np.random.default_rng(1).uniform(0.1, 1.1, (D, A))
    W[0, :5] = 0.0
    W[0, 5:8] = np.nan
    pres = np.ones((D, A), dtype=np.uint8)
    pres[1, ::3] = 0
    X[1, 2, 7] = np.nan
    Y[0, 2, 9] = np.inf
    Y[1, 3, K:] = np.nan            # n = p - 1 for column 1 on date 3
    Y[:, 4, :] = np.nan
    mod = C.run_panel(Y, X, W, pres, True, "model")
    assert mod["n"][0].tolist() == [32, 26, 38, 40, 0] and mod["n"][1].tolist() == [32, 26, 39, 3, 0]
    assert np.isnan(mod["beta"][1, 3]).all() and np.isnan(mod["alpha"][1, 3]) and np.isnan(mod["resid"][1, 3]).all()
    assert np.isnan(mod["resid"][0, 0, :8]).all() and np.isfinite(mod["resid"][0, 0, 8:]).all()
    C.assert_within(C.errors(mod, C.run_panel(Y, X, W, pres, True, "lstsq")), "validity")


def test_api_present():
    """The surface the issue names (fails before the feature exists)."""
    import factormodeling_amd.engine as E
    import factormodeling_amd.factor_backtest as FB
    import factormodeling_amd.operations as ops
    from factormodeling_amd import _lib
    assert list(inspect.signature(E.cs_ols).parameters) == ["Y", "X", "W", "present", "intercept", "want"]
    assert inspect.signature(E.cs_ols).parameters["want"].default == ("beta", "alpha", "r2", "n", "resid", "fitted")
    assert list(inspect.signature(ops.cs_regression_multi).parameters) == ["y", "X", "rettype", "intercept", "weights"]
    assert "cs_regression_multi" in ops.__all__
    sig = inspect.signature(FB.cross_sectional_factor_returns)
    assert list(sig.parameters) == ["factors_df", "returns", "lag", "intercept", "weights", "full"]
    assert sig.parameters["lag"].default == 1 and sig.parameters["full"].default is False
    assert len(_lib.SIGNATURES["fmx_cs_ols"]) == 17
    with open(os.path.join(ROOT, "include", "fmx.h")) as f:
        assert "fmx_status fmx_cs_ols(" in f.read()
    with open(os.path.join(ROOT, "factormodeling_amd", "csrc", "Makefile")) as f:
        assert "cs_ols.hip" in f.read()


def test_dropin_exports_cs_regression_multi():
    import importlib
    import sys
    dropin = os.path.join(ROOT, "factormodeling_amd", "dropin")
    sys.path.insert(0, dropin)
    try:
        sys.modules.pop("operations", None)
        m = importlib.import_module("operations")
        assert m.__file__.startswith(dropin) and hasattr(m, "cs_regression_multi")
    finally:
        sys.path.remove(dropin)
        sys.modules.pop("operations", None)


def test_beta_needs_a_series():
    import factormodeling_amd.operations as ops
    idx = pd.MultiIndex.from_product([pd.bdate_range("2020-01-01", periods=3), ["a", "b", "c"]],
                                     names=["date", "symbol"])
    df = pd.DataFrame(np.arange(18.0).reshape(9, 2), index=idx, columns=["u", "v"])
    with pytest.raises(ValueError):
        ops.cs_regression_multi(df, df, rettype="beta")
    with pytest.raises(ValueError):
        ops.cs_regression_multi(df["u"], df, rettype="tstat")


def test_no_gpu_raises():
    """No host fallback: without a HIP device the calls raise FmxError."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import factormodeling_amd.operations as ops
    from factormodeling_amd._lib import FmxError
    from factormodeling_amd.factor_backtest import cross_sectional_factor_returns
    idx = pd.MultiIndex.from_product([pd.bdate_range("2020-01-01", periods=4), list("abcdef")],
                                     names=["date", "symbol"])
    rng = np.random.default_rng(0)
    X = pd.DataFrame(rng.standard_normal((24, 2)), index=idx, columns=["u", "v"])
    y = pd.Series(rng.standard_normal(24), index=idx, name="y")
    with pytest.raises(FmxError):
        ops.cs_regression_multi(y, X)
    with pytest.raises(FmxError):
        cross_sectional_factor_returns(X, y)
