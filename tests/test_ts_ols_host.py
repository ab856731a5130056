"""ts_ols without a GPU: the numpy model of DESIGN §22's algorithm against the brute-force
reference over the parity grid (the source of the bounds), the pivot separation that makes the
kept set unambiguous, the row rule against the reference's one-regressor rolling regression,
the Python surface, the host-side refusals and the loud failure without a device."""
import ctypes
import importlib
import inspect
import os
import sys

import numpy as np
import pandas as pd
import pytest

import ts_ols_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------ 1
@pytest.fixture(scope="module")
def grid_worst():
    """Worst model-vs-reference error per quantity over the parity grid, the smallest kept and
    the largest dropped pivot (computed once)."""
    worst, min_kept, max_dropped = {}, np.inf, 0.0
    for gen in C.GRID_GENS:
        for ic in (True, False):
            for K in C.GRID_K:
                Y, X, shared = C.make_case(gen, K)
                for W in C.grid_windows(K, ic):
                    ref, mod = C.ref_panel(Y, X, W, None, ic, shared, which="both")
                    C.merge_worst(worst, C.errors(mod, ref, all_cells=False))
                    pv, kept = ref["pivots"], ref["kept"]
                    if kept.any():
                        min_kept = min(min_kept, float(pv[kept].min()))
                    dropped = ~kept & np.isfinite(pv)
                    if dropped.any():
                        max_dropped = max(max_dropped, float(np.abs(pv[dropped]).max()))
    return worst, min_kept, max_dropped


def test_model_worst_against_reference(grid_worst):
    """The figures ts_ols_cases.MEASURED_MODEL_WORST records; the bounds are 25 x them."""
    worst, min_kept, max_dropped = grid_worst
    print("ts_ols model vs reference, worst over the grid:", worst, "min kept pivot:", min_kept,
          "max dropped pivot:", max_dropped)
    C.assert_within(worst, "model vs reference")


def test_pivot_separation(grid_worst):
    """Kept pivots >= 1e-3 and dropped ones <= 1e-12 on every grid case: the GPU and the model
    cannot disagree on a kept set."""
    _, min_kept, max_dropped = grid_worst
    assert min_kept >= 1e-3 and max_dropped <= 1e-12, (min_kept, max_dropped)


def test_bounds_follow_the_rule():
    for k, b in C.BOUNDS.items():
        assert b == C.rule_bound(C.MEASURED_MODEL_WORST[k]), k
        assert b <= 1e-6, "a bound above 1e-6 means ill-conditioned windows in the grid"
    for k, b in C.K1_BOUNDS.items():
        assert b == C.rule_bound(C.MEASURED_K1_WORST[k]), k


# ------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("gapped", [False, True], ids=["dense", "gapped"])
def test_row_rule_against_ts_regression_fast(gapped):
    """K = 1, lag 0: the same rows and windows as the reference's ts_regression_fast (dropna,
    then roll per symbol), values within the bound measured here (K1_BOUNDS; the reference uses
    raw moments)."""
    import oracle.ops as O
    y, x = C.k1_panel(gapped)
    Dn, An = y.shape
    dcode, scode = np.repeat(np.arange(Dn), An), np.tile(np.arange(An), Dn)
    worst = {}
    for W in (8, 20):
        ref = C.ref_panel(y[None], x[None], W, None, True, False, assets=None)
        got = {k: (ref[k][0, 0] if k == "beta" else ref[k][0]) for k in ("resid", "alpha", "beta", "fitted", "r2")}

        def fast(rt):
            od, os_, ov = O.ts_regression_fast_long(dcode, scode, y.reshape(-1), x.reshape(-1), W, 0, rt)
            out = np.full((Dn, An), np.nan)
            out[od, os_] = ov
            return out

        C.merge_worst(worst, C.k1_errors(got, y, x, W, fast))
    print(f"ts_ols K=1 reference vs ts_regression_fast gapped={gapped}: worst {worst}")
    C.assert_within(worst, "K = 1 vs ts_regression_fast", C.K1_BOUNDS)


def test_reference_row_rule_by_hand():
    """A column with a gap and an inf regressor: windows skip the invalid rows."""
    Dn = 9
    y = np.arange(1.0, Dn + 1)[None, :, None] ** 1.5
    x = np.array([0.3, -1.0, 2.0, np.inf, 0.7, np.nan, -0.4, 1.1, 0.2])[None, :, None]
    y = y.copy()
    y[0, 1, 0] = np.nan
    ref = C.ref_panel(y, x, 3, None, True, False, assets=None)
    assert np.flatnonzero(ref["exists"][0, :, 0]).tolist() == [4, 6, 7, 8]     # valid rows 0, 2, 4, 6, 7, 8
    rows = [0, 2, 4]
    coef = np.polyfit(x[0, rows, 0], y[0, rows, 0], 1)
    assert abs(ref["beta"][0, 0, 4, 0] - coef[0]) < 1e-12 and abs(ref["alpha"][0, 4, 0] - coef[1]) < 1e-12
    assert np.isnan(ref["resid"][0, [0, 1, 2, 3, 5], 0]).all()


# ------------------------------------------------------------------------------------ 3
def test_api_present():
    import factormodeling_amd.engine as E
    import factormodeling_amd.factor_backtest as FB
    import factormodeling_amd.operations as ops
    from factormodeling_amd import _lib as L
    assert list(inspect.signature(E.ts_ols).parameters) == ["Y", "X", "window", "present", "intercept", "shared", "want"]
    sig = inspect.signature(E.ts_ols).parameters
    assert sig["want"].default == E.TS_OLS_OUTPUTS == ("beta", "alpha", "fitted", "resid", "r2", "sigma")
    assert sig["intercept"].default is True and sig["shared"].default is False and sig["present"].default is None
    sig = inspect.signature(ops.ts_regression_multi).parameters
    assert list(sig) == ["y", "X", "window", "lag", "rettype", "intercept"]
    assert sig["lag"].default == 0 and sig["rettype"].default == "resid" and sig["intercept"].default is True
    assert "ts_regression_multi" in ops.__all__
    assert "global" in ops.ts_regression_multi.__doc__ and "NOT" in ops.ts_regression_multi.__doc__
    sig = inspect.signature(FB.rolling_factor_exposures).parameters
    assert list(sig) == ["returns", "factor_ret_df", "window", "intercept"] and sig["intercept"].default is True
    assert len(L.SIGNATURES["fmx_ts_ols"]) == 19
    assert hasattr(L.load(), "fmx_ts_ols")
    with open(os.path.join(ROOT, "include", "fmx.h")) as f:
        assert "fmx_status fmx_ts_ols(" in f.read()
    with open(os.path.join(ROOT, "factormodeling_amd", "csrc", "Makefile")) as f:
        assert "ts_ols.hip" in f.read()


def test_dropin_exports_ts_regression_multi():
    dropin = os.path.join(ROOT, "factormodeling_amd", "dropin")
    sys.path.insert(0, dropin)
    try:
        sys.modules.pop("operations", None)
        m = importlib.import_module("operations")
        assert m.__file__.startswith(dropin) and hasattr(m, "ts_regression_multi")
    finally:
        sys.path.remove(dropin)
        sys.modules.pop("operations", None)


def _frames(nd=6, syms="abc"):
    idx = pd.MultiIndex.from_product([pd.bdate_range("2020-01-01", periods=nd), list(syms)], names=["date", "symbol"])
    rng = np.random.default_rng(0)
    X = pd.DataFrame(rng.standard_normal((len(idx), 2)), index=idx, columns=["u", "v"])
    y = pd.Series(rng.standard_normal(len(idx)), index=idx, name="y")
    return idx, y, X


def test_rettype_errors():
    import factormodeling_amd.operations as ops
    idx, y, X = _frames()
    with pytest.raises(ValueError):
        ops.ts_regression_multi(y, X, 4, rettype="tstat")
    with pytest.raises(ValueError):
        ops.ts_regression_multi(y, X, 4, rettype=2)                       # the one-regressor codes are not taken
    with pytest.raises(ValueError):
        ops.ts_regression_multi(pd.DataFrame({"a": y, "b": y}), X, 4, rettype="beta")
    with pytest.raises(ValueError):
        ops.ts_regression_multi(y, X["u"], 4)                             # a Series is not a regressor frame


def test_surface_shared_detection_and_lag(monkeypatch):
    """What reaches engine.ts_ols: a (date, symbol) X is a per-symbol panel (delayed by
    engine.ts("delay") when lag > 0), a date-indexed X a shared table reindexed to the panel's
    dates and shifted ``lag`` table rows.  The engine is replaced by a recorder: no device."""
    import torch
    import factormodeling_amd.operations as ops
    idx, y, X = _frames()
    calls = []

    def fake_ts_ols(Y, Xd, window, present=None, intercept=True, shared=False, want=()):
        calls.append(dict(Y=Y, X=Xd, window=window, present=present, intercept=intercept, shared=shared, want=want))
        Fy, Dn, An = Y.shape
        K = Xd.shape[0]
        return {k: torch.full((Fy, K, Dn, An) if k == "beta" else (Fy, Dn, An), 2.0, dtype=torch.float64) for k in want}

    def fake_ts(op, Xd, window, present=None, out=None):
        calls.append(dict(op=op, window=window))
        return Xd + 100.0

    monkeypatch.setattr(ops, "device", lambda: torch.device("cpu"))
    monkeypatch.setattr(ops.engine, "ts_ols", fake_ts_ols)
    monkeypatch.setattr(ops.engine, "ts", fake_ts)
    # panel X, lag 0
    out = ops.ts_regression_multi(y, X, 4)
    assert len(calls) == 1 and calls[0]["shared"] is False and tuple(calls[0]["X"].shape) == (2, 6, 3)
    assert calls[0]["want"] == ("resid",) and calls[0]["window"] == 4 and calls[0]["intercept"] is True
    assert isinstance(out, pd.Series) and out.index.equals(y.index) and out.name == "y" and (out == 2.0).all()
    # panel X, lag 2: the symbol's own rows, by engine.ts("delay")
    del calls[:]
    ops.ts_regression_multi(y, X, 4, lag=2, rettype="sigma", intercept=False)
    assert calls[0] == dict(op="delay", window=2) and calls[1]["shared"] is False
    assert float(calls[1]["X"][0, 0, 0]) == X["u"].iloc[0] + 100.0 and calls[1]["intercept"] is False
    assert calls[1]["want"] == ("sigma",)
    # shared X on other dates (one missing, one extra, unsorted), lag 1: table rows
    dates = idx.get_level_values("date").unique()
    tab = pd.DataFrame({"m": np.arange(6.0), "s": 10.0 + np.arange(6.0)}, index=dates)
    tab = pd.concat([tab.drop(dates[2]), pd.DataFrame({"m": [9.0], "s": [9.0]}, index=[dates[-1] + pd.Timedelta(days=30)])])
    tab = tab.iloc[::-1]
    del calls[:]
    ops.ts_regression_multi(y, tab, 3)
    assert len(calls) == 1 and calls[0]["shared"] is True and tuple(calls[0]["X"].shape) == (2, 6)
    np.testing.assert_array_equal(calls[0]["X"][0].numpy(), [0.0, 1.0, np.nan, 3.0, 4.0, 5.0])
    del calls[:]
    ops.ts_regression_multi(y, tab, 3, lag=1)
    assert len(calls) == 1                                                  # no per-symbol delay of a shared table
    np.testing.assert_array_equal(calls[0]["X"][1].numpy(), [np.nan, 10.0, 11.0, np.nan, 13.0, 14.0])
    # beta: a frame on y.index with X's columns; a frame y is one batched call
    del calls[:]
    b = ops.ts_regression_multi(y, X, 4, rettype="beta")
    assert isinstance(b, pd.DataFrame) and b.index.equals(y.index) and list(b.columns) == ["u", "v"]
    y2 = pd.DataFrame({"a": y, "b": 2.0 * y})
    r = ops.ts_regression_multi(y2, X, 4, rettype="r2")
    assert isinstance(r, pd.DataFrame) and list(r.columns) == ["a", "b"] and r.index.equals(y.index)
    assert tuple(calls[-1]["Y"].shape) == (2, 6, 3)


# ------------------------------------------------------------------------------------ 4
def test_bad_arguments_fail_before_device_work():
    """Empty panels (a valid call returns before any launch) with host buffers as the panel
    pointers: every bad argument is refused with FMX_ERR_ARG and a message."""
    from factormodeling_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(K=2, window=5, intercept=1, shared=0, Y=p, X=p, A=0, ld=0):
        return lib.fmx_ts_ols(Y, X, None, 0, K, 0, A, ld, window, intercept, shared, *([None] * 7), None)

    assert call() == 0
    assert call(K=8, window=9) == 0 and call(K=8, window=8, intercept=0) == 0 and call(shared=1) == 0
    for kw, msg in ((dict(K=0), b"regressors"), (dict(K=9, window=20), b"regressors"), (dict(K=-1), b"regressors"),
                    (dict(K=2, window=2), b"window"), (dict(K=2, window=1, intercept=0), b"window"),
                    (dict(K=8, window=8), b"window"), (dict(window=-4), b"window"), (dict(Y=None), b"null"),
                    (dict(X=None), b"null"), (dict(A=4, ld=3), b"dims"), (dict(ld=-1), b"dims"),
                    (dict(intercept=2), b"intercept"), (dict(shared=7), b"shared")):
        assert call(**kw) == 1, kw
        assert msg in lib.fmx_last_error(), (kw, lib.fmx_last_error())


def test_no_gpu_raises():
    """No host fallback: without a HIP device the calls raise FmxError."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import factormodeling_amd.engine as E
    import factormodeling_amd.operations as ops
    from factormodeling_amd._lib import FmxError
    from factormodeling_amd.factor_backtest import rolling_factor_exposures
    idx, y, X = _frames()
    tab = pd.DataFrame({"m": np.arange(6.0)}, index=idx.get_level_values("date").unique())
    with pytest.raises(FmxError):
        ops.ts_regression_multi(y, X, 4)
    with pytest.raises(FmxError):
        ops.ts_regression_multi(y, tab, 4, rettype="beta")
    with pytest.raises(FmxError):
        rolling_factor_exposures(y, tab, 4)
    with pytest.raises(FmxError):
        E.ts_ols(torch.zeros((1, 6, 3), dtype=torch.float64), torch.zeros((2, 6, 3), dtype=torch.float64), 4)
