"""Cases and a plain numpy oracle for the performance statistics (fmx_perf_stats /
fmx_perf_periods, factormodeling_amd.portfolio_analyzer).

The oracle restates pandas' operation sequences with scalar code written here: numpy's pairwise
sum (``pairwise_sum``), nanmean / nanvar on it, the left-to-right cumprod / cummax walk and the
bucket products.  tests/test_analyzer_host.py pins it to the reference class through the golden
vectors of tests/golden/analyzer.npz; tests/test_gpu_analyzer.py compares the kernels with it.

Content columns (``column(kind, T, seed)``, LOG returns): positive log returns lie in
[0.001, 0.02] and negative ones in [-0.02, -0.0005], so a column's number of negative EXCESS
returns is the same under risk-free rates 0 and 0.02 (0.02 / 252 = 7.9e-5 a day).
"""
from __future__ import annotations

import functools

import numpy as np
import pandas as pd

TS = (1, 2, 7, 8, 9, 127, 128, 129, 136, 257, 1100)     # numpy's leaf, block and split edges
KS = (1, 2, 65)
NEGS = (0, 1, 2, 7, 8, 9, 129)
KINDS = tuple(f"neg{n}" for n in NEGS) + ("rand", "nan_first", "nan_mid", "nan_last", "all_nan", "no_dd", "equal")
RFS = (0, 0.02)
TDS = (252, 365)
T_CONTENT = 257                                         # the class-level content cases
LONG_TS = (8193, 8199, 8200, 12000)                     # past one 8192-element buffer: a 1-, 7-, 8-element and a long tail
LONG_NEG = 8195                                         # a downside series whose own tail is 3 elements
STAT = dict(mean=0, std=1, max=2, min=3, count=4, ex_mean=5, ex_std=6, down_count=7, down_mean=8, down_std=9,
            final=10, maxdd=11, maxdd_row=12, maxdd_peak_row=13, dd_run=14)
SCALARS = ("average_return", "daily_volatility", "yearly_volatility", "annualized_return", "sharpe_0", "sortino_0",
           "sharpe_002", "sortino_002", "max_drawdown", "max_daily_return", "min_daily_return")
SUMMARY_KEYS = ("Average Daily Return", "Annualized Return", "Yearly Volatility", "Max Daily Return", "Sharpe Ratio",
                "Sortino Ratio", "Max Drawdown", "Min Daily Return")


# ----------------------------------------------------------------------------- cases
def column(kind: str, T: int, seed: int) -> np.ndarray:
    """One column of LOG returns of the given content kind."""
    rng = np.random.default_rng([seed, T, KINDS.index(kind) if kind in KINDS else len(KINDS)])
    pos = rng.uniform(0.001, 0.02, T)
    neg = -rng.uniform(0.0005, 0.02, T)
    if kind.startswith("neg"):
        n = min(int(kind[3:]), T)
        x = pos.copy()
        at = rng.choice(T, size=n, replace=False)
        x[at] = neg[at]
        return x
    if kind == "no_dd":
        return pos
    if kind == "equal":
        return np.full(T, 0.001)
    if kind == "all_nan":
        return np.full(T, np.nan)
    x = 0.01 * rng.standard_normal(T)
    if kind == "nan_first":
        x[0] = np.nan
    elif kind == "nan_mid" and T >= 3:
        x[rng.choice(np.arange(1, T - 1), size=max(1, (T - 2) // 9), replace=False)] = np.nan
    elif kind == "nan_last":
        x[-1] = np.nan
    return x


def dates_for(T: int) -> pd.DatetimeIndex:
    return pd.bdate_range("2019-01-01", periods=T)


def table(T: int, K: int = 65) -> np.ndarray:
    """[T][K] LOG returns: column k is of kind KINDS[k % len(KINDS)]."""
    return np.stack([column(KINDS[k % len(KINDS)], T, 100 + k) for k in range(K)], axis=1)


def long_table(T: int) -> np.ndarray:
    """[2][T] LOG returns past numpy's 8192-element buffer: a random column with NaNs, and a column
    with min(LONG_NEG, T) negative returns, so that its downside series ends in a short buffer too."""
    x = column("rand", T, 31)
    x[[0, 4000, 8192, T - 1]] = np.nan
    return np.stack([x, column(f"neg{min(LONG_NEG, T)}", T, 32)])


def gap_dates() -> pd.DatetimeIndex:
    """October 2020, a November of NaN rows only, December and January without a row (a gap of
    whole months across the year boundary), February and three days of March 2021."""
    return pd.DatetimeIndex(list(pd.bdate_range("2020-10-05", periods=10)) + list(pd.bdate_range("2020-11-09", periods=5))
                            + list(pd.bdate_range("2021-02-01", periods=8)) + list(pd.bdate_range("2021-03-01", periods=3)))


def gap_column(seed: int = 7) -> np.ndarray:
    x = 0.01 * np.random.default_rng(seed).standard_normal(26)
    x[10:15] = np.nan                                   # the November rows
    return x


@functools.lru_cache(maxsize=None)
def class_cases():
    """name -> frame with 'date' and 'log_return' (and the columns the plot reads, unused by the
    numbers): one per T, one per content kind at T_CONTENT, unsorted rows, the gap calendar."""
    out = {}
    for T in TS:
        kind = "nan_mid" if T >= 9 else "rand"
        out[f"T{T}"] = pd.DataFrame({"date": dates_for(T), "log_return": column(kind, T, 1)})
    for kind in KINDS:
        out[kind] = pd.DataFrame({"date": dates_for(T_CONTENT), "log_return": column(kind, T_CONTENT, 2)})
    df = pd.DataFrame({"date": dates_for(136), "log_return": column("nan_mid", 136, 3)})
    out["unsorted"] = df.iloc[np.random.default_rng(5).permutation(136)].reset_index(drop=True)
    out["gap"] = pd.DataFrame({"date": gap_dates(), "log_return": gap_column()})
    return out


# ----------------------------------------------------------------------------- oracle
def _leaf(a: np.ndarray) -> float:
    """numpy's unrolled block: 8 accumulators over the multiple-of-8 head, then the tail."""
    n = len(a)
    r = [a[j] for j in range(8)]
    for i in range(8, n - n % 8, 8):
        for j in range(8):
            r[j] = r[j] + a[i + j]
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for i in range(n - n % 8, n):
        res = res + a[i]
    return res


def _pairwise(a: np.ndarray) -> float:
    n = len(a)
    if n < 8:
        res = np.float64(0.0)
        for v in a:
            res = res + v
        return res
    if n <= 128:
        return _leaf(a)
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise(a[:n2]) + _pairwise(a[n2:])


def pairwise_sum(a) -> np.float64:
    """np.add.reduce of a contiguous float64 vector: pairwise inside 8192-element buffers, whose
    sums are added in order."""
    a = np.asarray(a, dtype=np.float64)
    if len(a) == 0:
        return np.float64(0.0)
    res = _pairwise(a[:8192])
    for lo in range(8192, len(a), 8192):
        res = res + _pairwise(a[lo:lo + 8192])
    return np.float64(res)


def mean_std(v: np.ndarray):
    """(Series.mean(), Series.std()) of a float64 vector with NaNs: nanops.nanmean / nanvar."""
    mask = np.isnan(v)
    cnt = int((~mask).sum())
    with np.errstate(all="ignore"):
        s = pairwise_sum(np.where(mask, 0.0, v))
        avg = s / np.float64(cnt)
        mean = avg if cnt > 0 else np.float64(np.nan)
        d = avg - np.where(mask, 0.0, v)
        q = pairwise_sum(np.where(mask, 0.0, d * d))
        std = np.sqrt(q / np.float64(cnt - 1)) if cnt > 1 else np.float64(np.nan)
    return np.float64(mean), np.float64(std), cnt


def curves(R: np.ndarray):
    """(cum, dd, final, maxdd, maxdd_row, maxdd_peak_row, dd_run) of one series of simple returns."""
    T = len(R)
    cum = np.full(T, np.nan)
    dd = np.full(T, np.nan)
    cp, peak, mdd = np.float64(1.0), -np.inf, np.inf
    mrow = prow = mprow = -1
    run = best = 0
    with np.errstate(all="ignore"):
        for t in range(T):
            v = R[t]
            if v != v:
                continue
            cp = cp * (np.float64(1.0) + v)
            cum[t] = cp - np.float64(1.0)
            c1 = cum[t] + np.float64(1.0)
            if c1 > peak:
                peak, prow = c1, t
            d = c1 / peak - np.float64(1.0)
            dd[t] = d
            if d < mdd:
                mdd, mrow, mprow = d, t, prow
            if d < 0:
                run += 1
                best = max(best, run)
            else:
                run = 0
    final = cum[-1] + 1.0
    return cum, dd, final, (mdd if mrow >= 0 else np.nan), mrow, mprow, best


def stats(R: np.ndarray, rf_daily: float) -> np.ndarray:
    """The FMX_PERF_NSTAT statistics of one series of simple returns."""
    R = np.asarray(R, dtype=np.float64)
    out = np.empty(len(STAT))
    ok = ~np.isnan(R)
    out[0], out[1], cnt = mean_std(R)
    out[2] = R[ok].max() if cnt else np.nan
    out[3] = R[ok].min() if cnt else np.nan
    out[4] = cnt
    E = R - rf_daily
    out[5], out[6], _ = mean_std(E)
    with np.errstate(invalid="ignore"):
        down = E[E < 0]
    out[8], out[9], out[7] = mean_std(down)
    _, _, out[10], out[11], out[12], out[13], out[14] = curves(R)
    return out


def periods(R: np.ndarray, seg: np.ndarray, nseg: int) -> np.ndarray:
    out = np.empty(nseg)
    for s in range(nseg):
        p = np.float64(1.0)
        for v in R[seg == s]:
            if v == v:
                p = p * (np.float64(1.0) + v)
        out[s] = p - np.float64(1.0)
    return out


def buckets(dates, freq: str):
    """(seg, nseg, period-end labels) of sorted dates: calendar months ('M') or years ('Y') from
    the first date's to the last date's."""
    d = pd.DatetimeIndex(dates)
    if freq == "M":
        o = d.year * 12 + d.month - 1
        lab = [pd.Timestamp(year=int(q // 12), month=int(q % 12) + 1, day=1) + pd.offsets.MonthEnd(0)
               for q in range(o[0], o[-1] + 1)]
    else:
        o = d.year
        lab = [pd.Timestamp(year=int(q), month=12, day=31) for q in range(o[0], o[-1] + 1)]
    seg = np.asarray(o - o[0], dtype=np.int32)
    return seg, int(seg[-1]) + 1, pd.DatetimeIndex(lab)


@functools.lru_cache(maxsize=None)
def table_oracle(T: int, rf: float, td: int = 252):
    """Oracle of the 65-column table at T: (R [65][T] simple returns, stats [NSTAT][65], cum, dd
    [65][T]); batches of 1 and 2 are its first columns."""
    R = np.ascontiguousarray(np.exp(np.ascontiguousarray(table(T).T)) - 1)
    st = np.stack([stats(R[k], rf / td) for k in range(R.shape[0])], axis=1)
    cv = [curves(R[k]) for k in range(R.shape[0])]
    for a in (R, st):
        a.setflags(write=False)
    return R, st, np.stack([c[0] for c in cv]), np.stack([c[1] for c in cv])


def class_oracle(df: pd.DataFrame, td: int):
    """What the reference class gives on ``df``: the host prep of its constructor, then the
    oracle.  Returns a dict: the SCALARS (annualized_return NaN and 'zde' True where the class
    raises ZeroDivisionError), 'return' / 'cum' / 'dd' curves, 'monthly' / 'yearly' (values,
    labels) and 'summary' (the eight values as strings; empty where summary() raises)."""
    f = df.copy()
    f["date"] = pd.to_datetime(f["date"])
    f.sort_values("date", inplace=True)
    f.reset_index(drop=True, inplace=True)
    R = (np.exp(f["log_return"]) - 1).to_numpy(dtype=np.float64)
    root = np.sqrt(td)
    res = {}
    with np.errstate(all="ignore"):
        s0, s2 = stats(R, 0 / td), stats(R, 0.02 / td)
        total_years = (f["date"].iloc[-1] - f["date"].iloc[0]).days / 365.25
        res["zde"] = total_years == 0
        ann = np.float64(np.nan) if res["zde"] else np.float64(s0[10])**(1 / total_years) - 1
        vals = [s0[0], s0[1], s0[1] * root, ann, (s0[5] / s0[6]) * root, (s0[5] / s0[9]) * root,
                (s2[5] / s2[6]) * root, (s2[5] / s2[9]) * root, s0[11], s0[2], s0[3]]
    res.update({k: np.float64(v) for k, v in zip(SCALARS, vals)})
    res["return"] = R
    res["cum"], res["dd"] = curves(R)[:2]
    for key, freq in (("monthly", "M"), ("yearly", "Y")):
        seg, nseg, lab = buckets(f["date"], freq)
        res[key] = (periods(R, seg, nseg), lab)
    if res["zde"]:
        res["summary"] = []
    else:
        pct = lambda v: f"{round(v * 100, 2)}%"          # noqa: E731
        res["summary"] = [pct(res["average_return"]), pct(res["annualized_return"]), pct(res["yearly_volatility"]),
                          pct(res["max_daily_return"]), str(round(res["sharpe_0"], 2)), str(round(res["sortino_0"], 2)),
                          pct(res["max_drawdown"]), pct(res["min_daily_return"])]
    return res
