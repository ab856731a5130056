"""Loader of tests/golden/factor_returns.npz (tests/golden/make_golden_factor_returns.py): the
inputs of each case as pandas objects and the reference's per-factor results."""
import os

import numpy as np
import pandas as pd

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "factor_returns.npz"))
CASES = ["eq_ragged", "lin_dense", "lin_ragged"]
VARIANTS = [(inv, tc) for inv in ("same", "diff") for tc in (True, False)]
COLS = ["log_return", "long_return", "short_return", "long_turnover", "short_turnover", "turnover"]
COUNTS = ["long_count", "short_count"]
PCT = 0.15


def dims(name):
    return tuple(int(v) for v in GOLD[f"{name}_dims"])          # F, D, A, Dm, Am


def axes(name):
    F, D, A, Dm, Am = dims(name)
    dates = pd.bdate_range("2021-01-01", periods=Dm)
    syms = np.array([f"S{k:04d}" for k in range(A)] + [f"X{k:02d}" for k in range(Am - A - 1)] + ["Q00"], dtype=object)
    return dates, syms


def index(name, key):
    dates, syms = axes(name)
    return pd.MultiIndex.from_arrays([dates[GOLD[f"{name}_{key}__d"]], syms[GOLD[f"{name}_{key}__s"]]],
                                     names=["date", "symbol"])


def series(name, key):
    return pd.Series(GOLD[f"{name}_{key}__v"], index=index(name, key))


def factors_df(name):
    F = dims(name)[0]
    return pd.DataFrame(GOLD[f"{name}_X"], index=index(name, "rows"), columns=[f"f{k}" for k in range(F)])


def settings(name, inv, tc, **kw):
    """The case's settings as a dict of SimulationSettings fields."""
    out = dict(returns=series(name, "ret"), cap_flag=series(name, "cap"), investability_flag=series(name, f"inv_{inv}"),
               factors_df=None, method=str(GOLD[f"{name}_method"]), pct=PCT, max_weight=float(GOLD[f"{name}_mw"]),
               plot=False, transaction_cost=tc)
    out.update(kw)
    return out


def reference_frames(name, inv, tc):
    """{field: DataFrame dates x factors} as the reference produced them, factor by factor."""
    dates, _ = axes(name)
    F = dims(name)[0]
    cols = [f"f{k}" for k in range(F)]
    key = f"{name}_{inv}_tc{int(tc)}"
    out = {}
    for j, c in enumerate(COLS):
        out[c] = pd.concat([pd.Series(GOLD[f"{key}_{f}_res_v"][:, j], index=pd.Index(dates[GOLD[f"{key}_{f}_res_d"]],
                                                                                    name="date"), name=f)
                            for f in cols], axis=1)
    for j, c in enumerate(COUNTS):
        out[c] = pd.concat([pd.Series(GOLD[f"{name}_{inv}_{f}_cnt_v"][:, j],
                                      index=pd.Index(dates[GOLD[f"{name}_{inv}_{f}_cnt_d"]], name="date"), name=f)
                            for f in cols], axis=1)
    return out
