"""Golden vectors for the quantile backtest (composite_factor.py:47-134), by running the
REFERENCE's ``plot_quantile_backtests_log`` in this container (test infrastructure only):

    python tests/golden/make_golden_qbacktest.py      -> tests/golden/qbacktest.npz

The inner ``quantile_backtest_log`` is a closure, so what is recorded is what the function
draws: under the Agg backend with ``plt.show`` patched out, every axis's lines -- the
cumulative curve ``expm1(cumsum(grp_log))`` of the buckets 1..n and the black ``DN_L1-S{n}``
spread -- and their dates.

The case: D = 12 dates, A = 30 symbols, F = 2 factor columns (the first rounded to one
decimal: ties), n = 5; 10 % NaN features, 5 % NaN returns, a fifth of the feature rows and
a tenth of the returns rows dropped independently, two symbols only in the returns and
one only in the features, an all-NaN feature date.  Plain arrays only (no pickles).
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import OUT, import_reference, put_series  # noqa: E402
from qbacktest_cases import panel  # noqa: E402

D, A, F, N_GROUPS, SEED = 12, 30, 2, 5, 1501


def main():
    warnings.filterwarnings("ignore")
    ref_cf = import_reference()[3]
    import matplotlib.pyplot as plt
    df, ret = panel(D, A, F, SEED, drop=0.2, nan_date=7)
    plt.show = lambda *a, **k: None
    ref_cf.plt.show = plt.show
    ref_cf.plot_quantile_backtests_log(df, ret, n_groups=N_GROUPS)
    fig = plt.gcf()
    dates = np.unique(np.r_[df.index.get_level_values(0).values, ret.index.get_level_values(0).values])
    syms = np.unique(np.r_[np.asarray(df.index.get_level_values(1)), np.asarray(ret.index.get_level_values(1))])
    st = {"dates": np.array([str(pd.Timestamp(d).date()) for d in dates]), "syms": np.array(list(syms)),
          "n_groups": np.array(N_GROUPS), "factors": np.array(list(df.columns))}
    for c in df.columns:
        put_series(st, f"x_{c}", df[c], dates, syms)
    put_series(st, "ret", ret, dates, syms)
    assert len(fig.axes) == F
    for ax, c in zip(fig.axes, df.columns):
        assert ax.get_title() == c
        lines = ax.get_lines()
        assert [ln.get_label() for ln in lines] == [str(k) for k in range(1, N_GROUPS + 1)] + [f"DN_L1-S{N_GROUPS}"]
        x = pd.DatetimeIndex(lines[0].get_xdata(orig=True))
        st[f"curve_dates_{c}"] = pd.Index(dates).get_indexer(x).astype(np.int32)
        st[f"curves_{c}"] = np.stack([np.asarray(ln.get_ydata(orig=True), dtype=np.float64) for ln in lines])
        print(c, "dates", len(x), "curves", st[f"curves_{c}"].shape, "NaN", int(np.isnan(st[f"curves_{c}"]).sum()))
    np.savez_compressed(os.path.join(OUT, "qbacktest.npz"), **st)
    print("wrote qbacktest.npz:", len(st), "arrays")


if __name__ == "__main__":
    main()
