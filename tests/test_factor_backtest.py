"""single_factor_backtests / single_factor_returns (factormodeling_amd/factor_backtest.py):
the parts that need no GPU.

The golden tests/golden/factor_returns.npz (the reference ``Simulation`` run once per factor)
is checked against a plain numpy restatement of ``_daily_portfolio_returns``
(portfolio_simulation.py:748-797) applied to the oracle's trade books; the library exports
``fmx_pnl_books``; ineligible inputs are refused by ``backend="batched"`` with the reason.
"""
import ctypes
import os
import re

import numpy as np
import pandas as pd
import pytest

import factor_backtest_cases as FC
import oracle.simulation as OS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dense(s, dates, syms):
    out = np.full((len(dates), len(syms)), np.nan)
    out[dates.get_indexer(s.index.get_level_values(0)), syms.get_indexer(s.index.get_level_values(1))] = s.to_numpy()
    return out


def _numpy_pnl(W, wd, R, rd, CAP, cd, tc):
    """portfolio_simulation.py:748-797 on dense [D][A] grids (NaN = no cell; wd / rd / cd = the
    dates each frame has): (kept dates, [D][6] result columns)."""
    w = np.nan_to_num(W)                                        # unstack().fillna(0), :759
    r = np.nan_to_num(R)
    longs, shorts = np.clip(w, 0, None), np.abs(np.clip(w, None, 0))
    rows = np.flatnonzero(wd)
    dl, ds = np.full(W.shape, np.nan), np.full(W.shape, np.nan)  # diff() over the weights' dates, :767
    dl[rows[1:]] = np.abs(longs[rows[1:]] - longs[rows[:-1]])
    ds[rows[1:]] = np.abs(shorts[rows[1:]] - shorts[rows[:-1]])
    c = np.trunc(np.nan_to_num(CAP))                            # fillna(0).astype(int).replace, :769-770
    rate = np.select([c == 1, c == 2, c == 3], [0.0025, 0.0015, 0.0010], c)
    nan = np.nan
    long_raw = np.where(wd | rd, (longs * r).sum(axis=1), nan)
    short_raw = np.where(wd | rd, -(shorts * r).sum(axis=1), nan)
    lt = np.where(wd, np.nansum(dl, axis=1), nan)
    st = np.where(wd, np.nansum(ds, axis=1), nan)
    if tc:
        l_cost = np.where(wd | cd, np.nansum(dl * rate, axis=1), nan)
        s_cost = np.where(wd | cd, np.nansum(ds * rate, axis=1), nan)
        long_ret, short_ret = long_raw - l_cost, short_raw - s_cost
        keep = wd | rd | cd
    else:
        long_ret, short_ret = long_raw, short_raw
        keep = wd | rd
    return keep, np.stack([long_ret + short_ret, long_ret, short_ret, lt, st, lt + st], axis=1)


@pytest.mark.parametrize("name", FC.CASES)
@pytest.mark.parametrize("inv,tc", FC.VARIANTS)
def test_golden_matches_numpy_restatement(name, inv, tc):
    dates, syms = FC.axes(name)
    syms = pd.Index(syms)
    df = FC.factors_df(name)
    st = FC.settings(name, inv, tc)
    R, CAP = _dense(st["returns"], dates, syms), _dense(st["cap_flag"], dates, syms)
    rd = np.isin(np.arange(len(dates)), dates.get_indexer(st["returns"].index.get_level_values(0)))
    cd = np.isin(np.arange(len(dates)), dates.get_indexer(st["cap_flag"].index.get_level_values(0)))
    ref = FC.reference_frames(name, inv, tc)
    for f in df.columns:
        x = df[f] * st["investability_flag"]                    # run(), :73
        X = _dense(x, dates, syms)
        pres = np.zeros(X.shape, dtype=bool)
        pres[dates.get_indexer(x.index.get_level_values(0)), syms.get_indexer(x.index.get_level_values(1))] = True
        if st["method"] == "equal":
            W, counts = OS.trade_equal(X, pres, st["pct"])
        else:
            W, counts = OS.trade_linear(X, pres, st["max_weight"])
        wd = pres.any(axis=1)
        keep, cols = _numpy_pnl(W, wd, R, rd, CAP, cd, tc)
        got = pd.DataFrame(cols[keep], index=pd.Index(dates[keep], name="date"), columns=FC.COLS)
        for c in FC.COLS:
            want = ref[c][f]
            assert got.index.equals(want.index), (name, f, c)
            np.testing.assert_allclose(got[c].to_numpy(), want.to_numpy(), rtol=1e-12, atol=1e-15, err_msg=f"{f} {c}")
        for j, c in enumerate(FC.COUNTS):
            want = ref[c][f]
            assert list(want.index) == list(dates[wd])
            np.testing.assert_array_equal(counts[wd, j], want.to_numpy())


def test_golden_covers_the_cases():
    """The fixture holds what the tests lean on: an all-NaN column, a flat day, a date without
    feature rows inside the returns' range, a late listing and a gap."""
    df = FC.factors_df("eq_ragged")
    assert df["f1"].isna().all()
    flat = FC.reference_frames("eq_ragged", "same", True)["long_count"]["f2"]
    assert (flat == 0).any()
    rows = FC.factors_df("lin_ragged").index
    dates, _ = FC.axes("lin_ragged")
    assert dates[11] not in rows.get_level_values(0)
    assert dates[11] in FC.series("lin_ragged", "ret").index.get_level_values(0)
    s0 = rows[rows.get_level_values(1) == "S0000"].get_level_values(0)
    assert s0.min() == dates[7]
    s5 = rows[rows.get_level_values(1) == "S0005"].get_level_values(0)
    assert not s5.isin(dates[4:9]).any() and (s5 < dates[4]).any() and (s5 >= dates[9]).any()
    assert (FC.series("lin_ragged", "cap") == 4.0).any()
    assert not FC.index("lin_ragged", "inv_diff").equals(rows)


def test_symbol_exported_and_declared():
    from factormodeling_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "fmx_pnl_books")
    assert "fmx_pnl_books" in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    assert re.search(r"fmx_status\s+fmx_pnl_books\s*\(", header)
    assert "portfolio_simulation.py:748-797" in header[:header.index("fmx_pnl_books(")][-1500:]
    assert _lib.load().fmx_abi_version() == 1


def test_public_names():
    import factormodeling_amd.factor_backtest as FB
    import factormodeling_amd.portfolio_simulation as PS
    from factormodeling_amd.dropin import portfolio_simulation as DPS
    assert PS.single_factor_returns is FB.single_factor_returns is DPS.single_factor_returns
    assert PS.single_factor_backtests is FB.single_factor_backtests is DPS.single_factor_backtests


def test_batched_refuses_mvo_naming_the_method():
    from factormodeling_amd.factor_backtest import single_factor_backtests
    df = FC.factors_df("eq_ragged")
    with pytest.raises(ValueError, match="method 'mvo'"):
        single_factor_backtests(df, FC.settings("eq_ragged", "same", True, method="mvo"), backend="batched")


@pytest.mark.parametrize("which", ["factors_df", "returns", "cap_flag", "investability_flag"])
def test_batched_refuses_duplicated_index(which):
    from factormodeling_amd.factor_backtest import single_factor_backtests
    df = FC.factors_df("eq_ragged")
    st = FC.settings("eq_ragged", "same", True)
    if which == "factors_df":
        df = pd.concat([df, df.iloc[:2]])
    else:
        st[which] = pd.concat([st[which], st[which].iloc[:2]])
    with pytest.raises(ValueError, match=f"{which}.*unique"):
        single_factor_backtests(df, st, backend="batched")


def test_bad_backend_field_and_columns():
    from factormodeling_amd.factor_backtest import single_factor_backtests, single_factor_returns
    df = FC.factors_df("eq_ragged")
    st = FC.settings("eq_ragged", "same", True)
    with pytest.raises(ValueError, match="backend"):
        single_factor_backtests(df, st, backend="fast")
    with pytest.raises(ValueError, match="field"):
        single_factor_returns(df, st, field="sharpe")
    with pytest.raises(KeyError, match="nope"):
        single_factor_backtests(df, st, columns=["f0", "nope"])
