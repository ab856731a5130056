"""CPU checks of the quantile backtest (``composite_factor.quantile_backtest_log``): the
host cut table against ``pd.qcut``, the numpy model of qbacktest_cases.py against the pandas
expression, the routing to the host loop, and the host loop against the reference golden."""
import numpy as np
import pandas as pd
import pytest

import golden_io as G
import qbacktest_cases as QC


def _cf():
    import factormodeling_amd.composite_factor as cf
    return cf


# ---------------------------------------------------------------------------- cut table
def _check_cut(m, n):
    from factormodeling_amd.engine import qcut_cum
    got = qcut_cum(m, n)
    want = QC.qcut_counts(m, n)
    assert got.dtype == np.int32 and got.shape == (n,)
    assert np.array_equal(got, want), (m, n, got, want)


@pytest.mark.parametrize("n", [2, 3, 5, 10])
def test_cut_table_small(n):
    """cum[m] == the label counts of pd.qcut(arange(1..m)) for every m in 1..2048."""
    for m in range(1, 2049):
        _check_cut(m, n)


@pytest.mark.parametrize("n", [5, 10, 32])
def test_cut_table_large(n):
    for m in (4999, 5000, 5001, 8191, 8192, 16383, 16384):
        _check_cut(m, n)


def test_cut_table_labels_from_cum():
    """label = first k with cum[k] >= r reproduces pd.qcut's label of every rank."""
    from factormodeling_amd.engine import qcut_cum
    for m, n in ((2, 5), (3, 5), (4, 5), (9, 10), (63, 5), (1100, 10), (8192, 32)):
        r = np.arange(1, m + 1)
        want = pd.qcut(pd.Series(r.astype(float)), n, labels=False, duplicates="drop").to_numpy()
        assert np.array_equal(np.searchsorted(qcut_cum(m, n), r, side="left"), want)


# ---------------------------------------------------------------------------- the model
CASES = [(12, 30, 5, 0.0, False, None), (15, 23, 5, 0.25, True, None), (10, 9, 10, 0.3, True, 4),
         (20, 64, 3, 0.1, True, None), (8, 4, 5, 0.3, False, None)]


def assert_frames(got, want, what=""):
    assert got.index.equals(want.index), (what, got.index, want.index)
    assert got.index.name == want.index.name == "date"
    assert np.array_equal(np.asarray(got.columns), np.asarray(want.columns)), what
    assert got.columns.dtype == want.columns.dtype == np.int64
    assert got.columns.name == want.columns.name == "group"
    g, w = got.to_numpy(dtype=np.float64), want.to_numpy(dtype=np.float64)
    assert np.array_equal(np.isnan(g), np.isnan(w)), what
    return g, w


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}x{c[1]}-n{c[2]}" for c in CASES])
def test_model_matches_pandas(case):
    D, A, n, drop, ties, nan_date = case
    df, r = QC.panel(D, A, 2, 31 * D + A, drop=drop, ties=ties, nan_date=nan_date)
    for c in df.columns:
        want = QC.pandas_buckets(df[c], r, n)
        g, w = assert_frames(QC.model(df[c], r, n), want, c)
        scale = QC.members_mean_abs(df[c], r, n).to_numpy(dtype=np.float64)
        ok = ~np.isnan(w)
        assert (np.abs(g - w)[ok] <= 4 * 2.0 ** -52 * scale[ok]).all()


# ---------------------------------------------------------------------------- routing
def _spy(monkeypatch):
    cf = _cf()
    calls = {"host": 0, "device": 0}
    host = cf._quantile_backtest_host

    def h(*a, **k):
        calls["host"] += 1
        return host(*a, **k)

    def d(*a, **k):
        calls["device"] += 1
        raise AssertionError("the device path must not run")
    monkeypatch.setattr(cf, "_quantile_backtest_host", h)
    monkeypatch.setattr(cf, "_quantile_backtest_device", d)
    return cf, calls


def test_routing_unsorted_within_date(monkeypatch):
    cf, calls = _spy(monkeypatch)
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    df, r = QC.panel(8, 9, 1, 5, drop=0.0)
    # reverse the symbols inside every date: each symbol's rows stay in date order
    order = np.lexsort((-np.arange(len(df)) % 9, df.index.get_level_values(0)))
    dfu = df.iloc[order]
    assert not dfu.index.equals(df.index)
    got = cf.quantile_backtest_log(dfu, r, 5, backend="auto")
    assert calls == {"host": 1, "device": 0}
    assert_frames(got["f0"], QC.pandas_buckets(dfu["f0"], r, 5))
    with pytest.raises(ValueError, match="sorted-symbol order"):
        cf.quantile_backtest_log(dfu, r, 5, backend="device")


def test_routing_too_many_groups(monkeypatch):
    cf, calls = _spy(monkeypatch)
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    df, r = QC.panel(6, 40, 1, 6, drop=0.0)
    got = cf.quantile_backtest_log(df, r, 33, backend="auto")
    assert calls == {"host": 1, "device": 0}
    assert list(got["f0"].columns) == list(range(1, 34))
    with pytest.raises(ValueError, match="n_groups"):
        cf.quantile_backtest_log(df, r, 33, backend="device")


def test_routing_no_gpu(monkeypatch):
    cf, calls = _spy(monkeypatch)
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    df, r = QC.panel(8, 9, 2, 7)
    got = cf.quantile_backtest_log(df, r, 5, backend="auto")
    assert calls == {"host": 2, "device": 0}
    assert sorted(got) == ["f0", "f1"]
    # an eligible input: with a GPU visible "auto" takes the device path
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    with pytest.raises(AssertionError, match="device path"):
        cf.quantile_backtest_log(df, r, 5, backend="auto")
    with pytest.raises(ValueError, match="backend"):
        cf.quantile_backtest_log(df, r, 5, backend="gpu")


def test_dropin_reexport():
    from factormodeling_amd.dropin import composite_factor as dcf
    assert dcf.quantile_backtest_log is _cf().quantile_backtest_log


# ---------------------------------------------------------------------------- golden
def golden_case():
    st = G.load("qbacktest.npz")
    dates = pd.to_datetime(st["dates"])
    facs = [str(c) for c in st["factors"]]
    df = pd.DataFrame({c: G.series(st, f"x_{c}", dates) for c in facs})
    ret = G.series(st, "ret", dates, name="log_ret")
    return st, dates, facs, df, ret, int(st["n_groups"])


def curves(frame, n):
    """What plot_quantile_backtests_log draws from one frame (composite_factor.py:106-109)."""
    cum = np.expm1(frame.cumsum())
    cum[f"DN_L1-S{n}"] = np.expm1((frame[1] - frame[n]).cumsum())
    return cum


def assert_golden(frames, st, dates, facs, n, tol=1e-12):
    for c in facs:
        cum = curves(frames[c], n)
        assert cum.index.equals(dates[st[f"curve_dates_{c}"]]), c
        got, want = cum.to_numpy(dtype=np.float64).T, st[f"curves_{c}"]
        assert got.shape == want.shape
        assert np.array_equal(np.isnan(got), np.isnan(want)), c
        ok = ~np.isnan(want)
        assert np.abs(got - want)[ok].max() <= tol, (c, np.abs(got - want)[ok].max())


def test_host_matches_reference_golden():
    st, dates, facs, df, ret, n = golden_case()
    frames = _cf().quantile_backtest_log(df, ret, n, backend="host")
    assert_golden(frames, st, dates, facs, n)
