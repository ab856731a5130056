"""The numpy oracle of the performance statistics (analyzer_cases.py) against the reference
class's recorded results (tests/golden/analyzer.npz), bit for bit, on every case and method; the
content cases hold the cells they were built for; the drop-in module exposes the reference's
methods; the C entry points and the Python layer refuse bad arguments.  No GPU."""
import ctypes
import importlib
import inspect
import os
import sys

import numpy as np
import pandas as pd
import pytest

import analyzer_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "factormodeling_amd", "dropin")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "analyzer.npz"))


def same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def test_golden_holds_the_cases():
    cases = C.class_cases()
    assert list(GOLD["case_names"]) == list(cases)
    for name, df in cases.items():
        assert same(GOLD[f"{name}__log_return"], df["log_return"])
        assert np.array_equal(GOLD[f"{name}__date"], pd.to_datetime(df["date"]).to_numpy().astype("datetime64[ns]")
                              .astype(np.int64))
    assert set(GOLD["method_names"]) >= {"__init__", "average_return", "summary", "plot_full_performance"}


@pytest.mark.parametrize("name", list(C.class_cases()))
def test_oracle_equals_the_reference(name):
    df = C.class_cases()[name]
    for td in C.TDS:
        o = C.class_oracle(df, td)
        key = f"{name}__td{td}"
        got = np.array([o[k] for k in C.SCALARS])
        assert same(got, GOLD[f"{key}__scalars"]), (td, dict(zip(C.SCALARS, zip(got, GOLD[f"{key}__scalars"]))))
        assert bool(GOLD[f"{key}__zde"]) == o["zde"]
        assert list(GOLD[f"{key}__summary"]) == o["summary"]
    assert same(o["return"], GOLD[f"{name}__return"])
    assert same(o["cum"], GOLD[f"{name}__cum"])
    assert same(o["dd"], GOLD[f"{name}__dd"])
    for k in ("monthly", "yearly"):
        v, lab = o[k]
        assert same(v, GOLD[f"{name}__{k}_v"])
        assert np.array_equal(lab.to_numpy().astype("datetime64[ns]").astype(np.int64), GOLD[f"{name}__{k}_d"])


def test_pairwise_sum_is_numpys():
    rng = np.random.default_rng(0)
    for n in (0, 1, 7, 8, 9, 127, 128, 129, 136, 257, 1100, 8192, 8193, 16384):
        a = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)
        assert C.pairwise_sum(a) == a.sum()


@pytest.mark.parametrize("T", C.LONG_TS)
def test_oracle_past_one_buffer(T):
    """Past 8192 rows numpy adds the sums of 8192-element buffers in order; for T = 8193 .. 8199 the
    last one holds 1 .. 7 elements and is summed sequentially.  The oracle against pandas itself."""
    tab = C.long_table(T)
    for k in range(2):
        r = np.exp(pd.Series(tab[k])) - 1
        for rf in (0.0, 0.02 / 252):
            s = C.stats(r.to_numpy(), rf)
            e = r - rf
            down = e[e < 0]
            want = [r.mean(), r.std(), r.max(), r.min(), r.count(), e.mean(), e.std(), len(down), down.mean(),
                    down.std()]
            assert same(s[:10], want), (T, k, rf)
    assert C.stats(np.exp(tab[1]) - 1, 0.0)[C.STAT["down_count"]] == min(C.LONG_NEG, T)
    assert 8193 <= min(C.LONG_NEG, T) <= 8199


def test_content_cases_hold_their_cells():
    T = C.T_CONTENT
    for rf in C.RFS:
        for n in C.NEGS:
            R = np.exp(C.column(f"neg{n}", T, 2)) - 1
            assert C.stats(R, rf / 252)[C.STAT["down_count"]] == n
    for T in C.TS:
        tab = C.table(T)
        assert tab.shape == (T, 65)
        for k, kind in enumerate(C.KINDS):
            x = tab[:, k]
            if kind.startswith("neg"):
                assert (x < 0).sum() == min(int(kind[3:]), T) and not np.isnan(x).any()
    T_ = C.T_CONTENT
    s = C.stats(np.exp(C.column("all_nan", T_, 2)) - 1, 0.0)
    assert s[C.STAT["count"]] == 0 and np.isnan(s[[0, 1, 2, 3, 5, 6, 8, 9, 10, 11]]).all()
    assert s[C.STAT["maxdd_row"]] == -1 and s[C.STAT["dd_run"]] == 0
    s = C.stats(np.exp(C.column("no_dd", T_, 2)) - 1, 0.0)
    assert s[C.STAT["maxdd"]] == 0.0 and s[C.STAT["dd_run"]] == 0 and s[C.STAT["maxdd_row"]] == 0
    s = C.stats(np.exp(C.column("equal", T_, 2)) - 1, 0.0)
    assert s[C.STAT["max"]] == s[C.STAT["min"]] and s[C.STAT["down_count"]] == 0
    assert np.isnan(C.column("nan_first", T_, 2)[0]) and np.isnan(C.column("nan_last", T_, 2)[-1])
    x = C.column("nan_mid", T_, 2)
    assert np.isnan(x[1:-1]).any() and not np.isnan(x[[0, -1]]).any()
    assert np.isnan(C.stats(np.exp(C.column("nan_last", T_, 2)) - 1, 0.0)[C.STAT["final"]])
    # one negative excess return: a count of 1 gives a NaN downside std
    s = C.stats(np.exp(C.column("neg1", T_, 2)) - 1, 0.0)
    assert np.isnan(s[C.STAT["down_std"]]) and not np.isnan(s[C.STAT["down_mean"]])
    # unsorted rows and the gap calendar
    d = C.class_cases()["unsorted"]["date"]
    assert not d.is_monotonic_increasing
    seg, nseg, lab = C.buckets(C.gap_dates(), "M")
    assert nseg == 6 and set(seg) == {0, 1, 4, 5}
    m = C.class_oracle(C.class_cases()["gap"], 252)["monthly"][0]
    assert m[1] == 0.0 and m[2] == 0.0 and m[3] == 0.0 and m[0] != 0.0
    assert C.buckets(C.gap_dates(), "Y")[1] == 2


def test_batched_exp_equals_the_columns_own():
    """performance_table exponentiates the contiguous [K][T] table; the class a column alone."""
    for T in (9, 136, 1100):
        tab = C.table(T)
        R = np.exp(np.ascontiguousarray(tab.T)) - 1
        for k in range(tab.shape[1]):
            assert same(R[k], np.exp(pd.Series(tab[:, k])) - 1)


def test_dropin_exposes_the_reference_class():
    sys.path.insert(0, DROPIN)
    try:
        sys.modules.pop("portfolio_analyzer", None)
        m = importlib.import_module("portfolio_analyzer")
        assert m.__file__.startswith(DROPIN), m.__file__
        for name, params in zip(GOLD["method_names"], GOLD["method_params"]):
            fn = getattr(m.PortfolioAnalyzer, str(name))
            assert ",".join(inspect.signature(fn).parameters) == str(params), name
        for name in ("performance_table", "performance_curves", "period_returns", "rolling_sharpe"):
            assert hasattr(m, name)
    finally:
        sys.path.remove(DROPIN)
        sys.modules.pop("portfolio_analyzer", None)


def _lib():
    from factormodeling_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libfmx.so not built (run __graft_entry__.build())")
    return L.load()


def test_c_entries_refuse_bad_arguments():
    """Status 1 and a message, before any device work (no GPU here): the pointers are host
    buffers that a launch would never be given."""
    lib = _lib()
    buf = (ctypes.c_double * 64)()
    other = (ctypes.c_double * 64)()
    third = (ctypes.c_double * 64)()
    seg = (ctypes.c_int32 * 8)()
    p, q, r3, s = (ctypes.cast(b, ctypes.c_void_p) for b in (buf, other, third, seg))
    bad_stats = [
        (None, 1, 4, 4, 0.0, q, None, None, None),            # null returns
        (p, 1, 4, 4, 0.0, None, None, None, None),            # null stats
        (p, 0, 4, 4, 0.0, q, None, None, None),               # K < 1
        (p, 1, 0, 4, 0.0, q, None, None, None),               # T < 1
        (p, 1, 4, 3, 0.0, q, None, None, None),               # ld < T
        (p, 1, 16385, 16385, 0.0, q, None, None, None),       # past the cap on T
        (p, 1, 4, 4, 0.0, q, p, None, None),                  # cum aliases R
        (p, 1, 4, 4, 0.0, q, r3, r3, None),                   # cum aliases dd
    ]
    for args in bad_stats:
        assert lib.fmx_perf_stats(*args) == 1, args
        assert b"perf_stats" in lib.fmx_last_error()
    assert lib.fmx_perf_stats(p, 1, 16385, 16385, 0.0, q, None, None, None) == 1
    assert b"16384" in lib.fmx_last_error()
    bad_periods = [
        (None, 1, 4, 4, s, 2, q, None),                       # null returns
        (p, 1, 4, 4, None, 2, q, None),                       # null seg
        (p, 1, 4, 4, s, 2, None, None),                       # null out
        (p, 0, 4, 4, s, 2, q, None),                          # K < 1
        (p, 1, 0, 4, s, 2, q, None),                          # T < 1
        (p, 1, 4, 3, s, 2, q, None),                          # ld < T
        (p, 1, 4, 4, s, 0, q, None),                          # nseg < 1
        (p, 1, 4, 4, s, 2, p, None),                          # out aliases R
    ]
    for args in bad_periods:
        assert lib.fmx_perf_periods(*args) == 1, args
        assert b"perf_periods" in lib.fmx_last_error()


def test_python_layer_names_the_cap():
    """Past FMX_PERF_TMAX rows the class raises before it needs a device."""
    from factormodeling_amd import _lib as L
    from factormodeling_amd.portfolio_analyzer import PortfolioAnalyzer, performance_table
    T = L.PERF_TMAX + 1
    df = pd.DataFrame({"date": pd.date_range("1950-01-01", periods=T), "log_return": np.zeros(T)})
    with pytest.raises(ValueError, match=str(L.PERF_TMAX)):
        PortfolioAnalyzer(df)
    with pytest.raises(ValueError, match=str(L.PERF_TMAX)):
        performance_table(df.set_index("date"))
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    assert f"#define FMX_PERF_TMAX {L.PERF_TMAX}" in header
    assert f"#define FMX_PERF_NSTAT {L.PERF_NSTAT}" in header
    for name, row in L.PERF.items():
        assert f"#define FMX_PERF_{name.upper()} {row}\n" in header
    assert L.PERF == C.STAT


def test_run_does_not_hide_a_broken_analyzer_module(tmp_path, monkeypatch):
    """Only a MISSING ``portfolio_analyzer`` makes ``Simulation.run()`` take the package's class: an
    import error raised inside a module of that name (a checkout whose own imports fail) surfaces."""
    from factormodeling_amd.portfolio_simulation import Simulation, SimulationSettings
    (tmp_path / "portfolio_analyzer.py").write_text("import a_module_nobody_has_installed_xyz\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    monkeypatch.delitem(sys.modules, "portfolio_analyzer", raising=False)
    s = pd.Series(dtype=float)
    sim = Simulation("f", s, SimulationSettings(returns=s, cap_flag=s, investability_flag=s, factors_df=pd.DataFrame()))
    with pytest.raises(ModuleNotFoundError, match="a_module_nobody_has_installed_xyz"):
        sim.run()
    sys.modules.pop("portfolio_analyzer", None)
