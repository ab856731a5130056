"""Golden vectors for ``PortfolioAnalyzer``, by running the REFERENCE class in this container
(test infrastructure only):

    python tests/golden/make_golden_analyzer.py      -> tests/golden/analyzer.npz

The cases are those of tests/analyzer_cases.py (``class_cases()``: one frame per T at the edges
of numpy's pairwise leaf / block / split, one per content kind, unsorted rows, a calendar with a
gap of whole months across a year boundary and a month of NaN rows only).  Per case the inputs
(dates as int64 ns, log returns) and, for trading_days 252 and 365, every public method's result:
the scalars of ``analyzer_cases.SCALARS`` (Sharpe / Sortino at risk-free rates 0 and 0.02), the
``return`` / ``cumulative_return`` / ``max_drawdown_curve()`` series, ``monthly_return()`` /
``yearly_return()`` (values and labels) and the eight ``summary()`` values as strings.  Where the
class raises ZeroDivisionError (one date: zero years) ``annualized_return`` is stored as NaN with
the flag ``zde`` and the summary is empty.  Also the class's public method names with their
parameter names, and the number of axes ``plot_full_performance`` builds without and with the
turnover columns and ``counts_df``.  Plain arrays only (no pickles).
"""
from __future__ import annotations

import inspect
import os
import sys
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import OUT, REF  # noqa: E402
import analyzer_cases as C  # noqa: E402


def plot_frames():
    """(frame without the optional columns, frame with them, counts_df) for the axes counts."""
    T = 300
    base = pd.DataFrame({"date": C.dates_for(T), "log_return": C.column("rand", T, 11)})
    full = base.copy()
    rng = np.random.default_rng(12)
    full["long_return"] = 0.01 * rng.standard_normal(T)
    full["short_return"] = 0.01 * rng.standard_normal(T)
    full["long_turnover"] = rng.uniform(0, 1, T)
    full["short_turnover"] = rng.uniform(0, 1, T)
    full["turnover"] = full["long_turnover"] + full["short_turnover"]
    counts = pd.DataFrame({"long_count": rng.integers(5, 50, T), "short_count": rng.integers(5, 50, T)},
                          index=C.dates_for(T))
    return base, full, counts


def main():
    warnings.filterwarnings("ignore")
    sys.dont_write_bytecode = True
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import portfolio_analyzer as ref

    st = {}
    names = [n for n, f in inspect.getmembers(ref.PortfolioAnalyzer, inspect.isfunction)
             if not n.startswith("_") or n == "__init__"]
    st["method_names"] = np.array(names)
    st["method_params"] = np.array([",".join(inspect.signature(getattr(ref.PortfolioAnalyzer, n)).parameters)
                                    for n in names])
    st["case_names"] = np.array(list(C.class_cases()))
    for name, df in C.class_cases().items():
        st[f"{name}__date"] = pd.to_datetime(df["date"]).to_numpy().astype("datetime64[ns]").astype(np.int64)
        st[f"{name}__log_return"] = df["log_return"].to_numpy(dtype=np.float64)
        for td in C.TDS:
            a = ref.PortfolioAnalyzer(df, trading_days_per_year=td)
            key = f"{name}__td{td}"
            zde = False
            try:
                ann = a.annualized_return()
            except ZeroDivisionError:
                ann, zde = np.nan, True
            vals = [a.average_return(), a.daily_volatility(), a.yearly_volatility(), ann, a.sharpe_ratio(),
                    a.sortino_ratio(), a.sharpe_ratio(0.02), a.sortino_ratio(0.02), a.max_drawdown(),
                    a.max_daily_return(), a.min_daily_return()]
            st[f"{key}__scalars"] = np.array(vals, dtype=np.float64)
            st[f"{key}__zde"] = np.array(zde)
            st[f"{key}__summary"] = np.array([] if zde else [str(v) for v in a.summary().values()], dtype=str)
            if td == C.TDS[0]:
                st[f"{name}__return"] = a.df["return"].to_numpy(dtype=np.float64)
                st[f"{name}__cum"] = a.df["cumulative_return"].to_numpy(dtype=np.float64)
                st[f"{name}__dd"] = a.max_drawdown_curve().to_numpy(dtype=np.float64)
                for k, ser in (("monthly", a.monthly_return()), ("yearly", a.yearly_return())):
                    st[f"{name}__{k}_v"] = ser.to_numpy(dtype=np.float64)
                    st[f"{name}__{k}_d"] = ser.index.to_numpy().astype("datetime64[ns]").astype(np.int64)
    base, full, counts = plot_frames()
    axes = []
    for frame, cnt in ((base, None), (full, counts)):
        plt.close("all")
        ref.PortfolioAnalyzer(frame).plot_full_performance(counts_df=cnt)
        axes.append(len(plt.gcf().axes))
    plt.close("all")
    st["plot_axes"] = np.array(axes, dtype=np.int64)
    st["versions"] = np.array([f"pandas {pd.__version__}", f"numpy {np.__version__}"])
    path = os.path.join(OUT, "analyzer.npz")
    np.savez_compressed(path, **st)
    print("wrote analyzer.npz:", len(st), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
