"""Drop-in replacement for the reference's ``portfolio_analyzer.py`` plus its batched form.

``PortfolioAnalyzer`` keeps the reference's constructor, attributes and public methods
(portfolio_analyzer.py:9-260).  The host prepares the frame with the reference's own pandas /
numpy calls (``to_datetime``, ``sort_values('date')``, ``np.exp(log_return) - 1``); every number
between that and the final host arithmetic (the Sharpe / Sortino ratio, ``sqrt(trading_days)``,
``final_value ** (1 / years)``) is the K = 1 case of ``fmx_perf_stats`` / ``fmx_perf_periods``
(csrc/perf_stats.hip), which restate pandas' operation sequences, so each method returns the
reference's value bit for bit and ``summary()`` the same strings.

``performance_table`` / ``performance_curves`` / ``period_returns`` / ``rolling_sharpe`` take a
dates x K frame of returns (one column per factor, book or manager, as
``single_factor_returns`` produces) and give every column's numbers from one upload; column k
equals ``PortfolioAnalyzer`` on column k alone, bit for bit.
"""
from __future__ import annotations

import numpy as np
import pandas as pd
import torch

from . import engine as E
from .panel import device

# ----------------------------------------------------------------------------- host helpers
def _upload(rows: np.ndarray):
    """[K][T] float64 host array -> device tensor (the one upload of a call)."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    if rows.shape[1] > E.PERF_TMAX:
        raise ValueError(f"a return series may hold at most {E.PERF_TMAX} rows (got {rows.shape[1]})")
    if rows.shape[1] < 1:
        raise ValueError("a return series needs at least one row")
    return torch.as_tensor(rows, device=device())


def _period_buckets(dates: pd.Series, freq: str):
    """(seg int32 [T], labels DatetimeIndex): the calendar bucket of each (sorted) date counted
    from the first date's, and pandas' period-end label of every bucket from the first date's to
    the last date's -- the bins of ``resample('M' | 'Y')``."""
    f = {"M": "M", "ME": "M", "Y": "Y", "YE": "Y", "A": "Y"}.get(freq)
    if f is None:
        raise ValueError(f"freq must be 'M' or 'Y' (got {freq!r})")
    per = pd.DatetimeIndex(dates).to_period(f)
    if per.isna().any():
        raise ValueError("period returns need valid dates")
    first, last = per[0], per[-1]
    seg = (per.asi8 - first.ordinal).astype(np.int32)
    end = pd.offsets.MonthEnd() if f == "M" else pd.offsets.YearEnd()
    labels = pd.date_range(first.to_timestamp(how="end").normalize(), periods=last.ordinal - first.ordinal + 1,
                           freq=end, name="date")
    return seg, labels


def _years(dates: pd.Series):
    total_days = (dates.iloc[-1] - dates.iloc[0]).days
    return total_days / 365.25


class PortfolioAnalyzer:
    """portfolio_analyzer.py:9-260 (after-cost clean portfolio), numbers from the GPU."""

    def __init__(self, df: pd.DataFrame, trading_days_per_year: int = 252):
        # host prep with the reference's own pandas / numpy calls: their results (the row order of
        # a non-stable sort, numpy's exp) are part of the bits every method has to reproduce
        frame = df.copy()
        frame['date'] = pd.to_datetime(frame['date'])
        frame.sort_values('date', inplace=True)
        frame.reset_index(drop=True, inplace=True)
        frame['return'] = np.exp(frame['log_return']) - 1
        self.df = frame
        self.trading_days = trading_days_per_year
        self._cache = None
        self.df['cumulative_return'] = self._curves()[0]       # the device's cumprod - 1

    # ------------------------------------------------------------------ device passes
    def _returns(self) -> np.ndarray:
        return self.df['return'].to_numpy(dtype=np.float64, na_value=np.nan)

    def _run(self, rf_daily: float, curves: bool):
        """(stats [NSTAT], cum [T], dd [T]) of the frame's current 'return' column; the last
        pass is kept while the column and rf_daily stay the same."""
        r = self._returns()
        c = self._cache
        if c is not None and c[1] == rf_daily and (c[3] is not None or not curves) and \
                np.array_equal(c[0], r, equal_nan=True):
            return c[2], c[3], c[4]
        R = _upload(r[None, :])
        stats, cum, dd = E.perf_stats(R, rf_daily, curves=curves)
        stats = stats.cpu().numpy()[:, 0]
        cum = cum.cpu().numpy()[0] if curves else None
        dd = dd.cpu().numpy()[0] if curves else None
        self._cache = (r.copy(), rf_daily, stats, cum, dd)
        return stats, cum, dd

    def _stat(self, name: str, rf_daily: float = 0.0):
        return np.float64(self._run(rf_daily, False)[0][E.PERF[name]])

    def _curves(self):
        _, cum, dd = self._run(0.0, True)
        return cum, dd

    def _periods(self, freq: str) -> pd.Series:
        seg, labels = _period_buckets(self.df['date'], freq)
        out = E.perf_periods(_upload(self._returns()[None, :]), seg, len(labels))
        return pd.Series(out.cpu().numpy()[:, 0], index=labels, name='return')

    # ------------------------------------------------------------------ the reference's methods
    def average_return(self):
        return self._stat("mean")

    def daily_volatility(self):
        return self._stat("std")

    def yearly_volatility(self):
        return self.daily_volatility() * np.sqrt(self.trading_days)

    def annualized_return(self):
        total_days = (self.df['date'].iloc[-1] - self.df['date'].iloc[0]).days
        total_years = total_days / 365.25
        final_value = self._stat("final")
        return final_value**(1 / total_years) - 1

    def sharpe_ratio(self, risk_free_rate=0):
        rf = risk_free_rate / self.trading_days
        return (self._stat("ex_mean", rf) / self._stat("ex_std", rf)) * np.sqrt(self.trading_days)

    def sortino_ratio(self, risk_free_rate=0):
        rf = risk_free_rate / self.trading_days
        downside_std = self._stat("down_std", rf)
        return (self._stat("ex_mean", rf) / downside_std) * np.sqrt(self.trading_days)

    def max_drawdown(self):
        return self._stat("maxdd")

    def max_drawdown_curve(self):
        return pd.Series(self._curves()[1], index=self.df.index, name='cumulative_return')

    def max_daily_return(self):
        return self._stat("max")

    def min_daily_return(self):
        return self._stat("min")

    def monthly_return(self):
        return self._periods('M')

    def yearly_return(self):
        return self._periods('Y')

    def summary(self):
        """The reference's eight entries, in its order: percentages rounded to two places as
        strings, the two ratios rounded to two places as numbers."""
        def pct(v):
            return f"{round(v * 100, 2)}%"
        return {
            'Average Daily Return': pct(self.average_return()),
            'Annualized Return': pct(self.annualized_return()),
            'Yearly Volatility': pct(self.yearly_volatility()),
            'Max Daily Return': pct(self.max_daily_return()),
            'Sharpe Ratio': round(self.sharpe_ratio(), 2),
            'Sortino Ratio': round(self.sortino_ratio(), 2),
            'Max Drawdown': pct(self.max_drawdown()),
            'Min Daily Return': pct(self.min_daily_return()),
        }

    # ------------------------------------------------------------------ the figure
    def _rolling(self, window: int):
        """(rolling mean, rolling std) of log_return: ts_mean / ts_std on the column viewed as a
        one-factor, one-symbol panel (pinned to ``rolling(w).mean() / .std()``)."""
        x = self.df['log_return'].to_numpy(dtype=np.float64, na_value=np.nan)
        X = torch.as_tensor(np.ascontiguousarray(x[None, :, None]), device=device())
        m = E.ts("mean", X, window).cpu().numpy()[0, :, 0]
        s = E.ts("std", X, window).cpu().numpy()[0, :, 0]
        return pd.Series(m, index=self.df.index), pd.Series(s, index=self.df.index)

    def plot_full_performance(self, counts_df: pd.DataFrame = None):
        """The reference's figure, one column of panels sharing the date axis: the summary as a
        table; the cumulative return with the drawdown curve, the long / short legs where the frame
        has them, and monthly returns as bars on a twin axis; the 120- and 252-row rolling means of
        log_return; the turnover (where the frame has it); the leg counts (where ``counts_df`` is
        given); the rolling Sharpe ratios.  Like the reference it adds the plotted series to
        ``self.df`` and zeroes turnover rows above 1.5 there.  The series come from the device."""
        import matplotlib.pyplot as plt
        from matplotlib.dates import DateFormatter, YearLocator
        from matplotlib.ticker import PercentFormatter

        frame, dates = self.df, self.df['date']
        windows = {120: 'darkred', 252: 'navy'}
        rolled = {w: self._rolling(w) for w in windows}
        for w in windows:
            frame[f'log_return_ma{w}'] = rolled[w][0]
        legs = {'long_return': ('cumulative_long_return', 'Long Leg', 'green', ':'),
                'short_return': ('cumulative_short_return', 'Short Leg', 'orange', '-.')}
        for src, (dst, _, _, _) in legs.items():
            if src in frame.columns:
                frame[dst] = frame[src].fillna(0).cumsum().map(np.exp) - 1
        monthly = self.monthly_return().dropna()
        show_turnover = 'turnover' in frame.columns
        show_counts = counts_df is not None and not counts_df.empty

        heights = [0.6, 2, 0.8, 0.8] + [0.8] * (int(show_turnover) + int(show_counts))
        fig = plt.figure(figsize=(14, 4 * len(heights)))
        grid = fig.add_gridspec(len(heights), 1, height_ratios=heights, hspace=0.3)
        percent = PercentFormatter(xmax=1.0)

        # the summary, two (metric, value) pairs per table row
        ax = fig.add_subplot(grid[0])
        ax.axis('off')
        entries = list(self.summary().items())
        half = len(entries) // 2
        cells = [[*l, *r] for l, r in zip(entries[:half], entries[half:])]
        table = ax.table(cellText=cells, colLabels=['Metric', 'Value'] * 2, cellLoc='center', colLoc='center',
                         loc='center')
        table.auto_set_font_size(False)
        table.set_fontsize(12)
        table.scale(1, 1.5)

        # cumulative return, drawdown and legs; monthly bars on the twin axis
        top = fig.add_subplot(grid[1])
        bars = top.twinx()
        top.plot(dates, frame['cumulative_return'], color='black', label='Total')
        top.plot(dates, self.max_drawdown_curve(), color='red', linestyle='--', label='Max Drawdown Curve')
        for dst, label, colour, style in legs.values():
            if dst in frame.columns:
                top.plot(dates, frame[dst], color=colour, linestyle=style, label=label)
        top.set_title('Cumulative Return (Total / Long / Short) with Monthly Bars')
        top.set_ylabel('Cumulative Return')
        top.yaxis.set_major_formatter(percent)
        top.legend(loc='upper left')
        top.grid(True)
        bars.bar(monthly.index, monthly.to_numpy(), width=20, alpha=0.4,
                 color=np.where(monthly.to_numpy() >= 0, 'green', 'red').tolist())
        bars.set_ylabel('Monthly Return', color='gray')
        bars.tick_params(axis='y', labelcolor='gray')
        bars.yaxis.set_major_formatter(percent)

        # rolling means
        ax = fig.add_subplot(grid[2], sharex=top)
        for w, colour in windows.items():
            ax.fill_between(dates, frame[f'log_return_ma{w}'], color=colour, alpha=0.5,
                            label='120d MA' if w == 120 else '250d MA')
        ax.set_title('Rolling MA of Daily Returns')
        ax.set_ylabel('MA(Return)')
        ax.yaxis.set_major_formatter(percent)
        ax.xaxis.set_major_locator(YearLocator())
        ax.xaxis.set_major_formatter(DateFormatter('%Y'))
        ax.legend(loc='upper left')
        ax.grid(True)

        row = 3
        if show_turnover:
            ax = fig.add_subplot(grid[row], sharex=top)
            row += 1
            mean_turnover = frame['turnover'].mean()
            frame.loc[frame['turnover'] > 1.5, ['turnover', 'long_turnover', 'short_turnover']] = 0
            ax.plot(dates, frame['turnover'], color='purple', linewidth=1.2, label='Total Turnover')
            for col, colour, label in (('long_turnover', 'green', 'Long Turnover'),
                                       ('short_turnover', 'red', 'Short Turnover')):
                if col in frame.columns:
                    ax.plot(dates, frame[col], color=colour, linestyle='--', label=label)
            ax.axhline(mean_turnover, color='gray', linestyle=':', linewidth=1.2, label=f'Avg: {mean_turnover:.2%}')
            ax.set_title('Portfolio Turnover (Total / Long / Short)')
            ax.set_ylabel('Turnover')
            ax.yaxis.set_major_formatter(percent)
            ax.legend(loc='upper right')
            ax.grid(True)

        if show_counts:
            ax = fig.add_subplot(grid[row], sharex=top)
            row += 1
            for col, colour, label in (('long_count', 'green', 'Long Count'), ('short_count', 'red', 'Short Count')):
                ax.plot(counts_df.index, counts_df[col], color=colour, label=label)
            ax.set_title('Number of Symbols in Long and Short Legs Over Time')
            ax.set_xlabel('Date')
            ax.set_ylabel('Count')
            ax.legend()
            ax.grid(True)

        # rolling Sharpe of log_return (annualised with 252, as the reference draws it)
        ax = fig.add_subplot(grid[row], sharex=top)
        with np.errstate(divide='ignore', invalid='ignore'):
            for w, colour in windows.items():
                mean, std = rolled[w]
                ax.plot(dates, mean / std * np.sqrt(252), color=colour, linewidth=1.5, label=f'{w}d Sharpe')
        for level in ax.get_yticks():
            if abs(level - round(level)) < 1e-6:               # a faint line at every integer tick
                ax.axhline(level, color='gray', linestyle='--', linewidth=0.5, alpha=0.3)
        ax.set_title('Rolling Sharpe Ratios')
        ax.set_xlabel('Date')
        ax.set_ylabel('Sharpe')
        ax.legend(loc='upper left', fontsize='small')
        ax.grid(True)

        plt.show()


# ----------------------------------------------------------------------------- batched form
def _table_rows(returns_df: pd.DataFrame, kind: str):
    """(sorted dates Series, columns, [K][T] simple returns, [K][T] raw values) of a dates x K
    frame, rows ordered as the class orders them (``sort_values`` of the dates)."""
    if kind not in ("log", "simple"):
        raise ValueError(f"kind must be 'log' or 'simple' (got {kind!r})")
    if not isinstance(returns_df, pd.DataFrame) or returns_df.shape[1] < 1 or returns_df.shape[0] < 1:
        raise ValueError("returns_df must be a dates x K DataFrame with at least one row and one column")
    dates = pd.Series(pd.to_datetime(returns_df.index)).sort_values()
    order = dates.index.to_numpy()
    dates = dates.reset_index(drop=True)
    raw = np.ascontiguousarray(returns_df.to_numpy(dtype=np.float64, na_value=np.nan)[order].T)
    simple = np.exp(raw) - 1 if kind == "log" else raw      # on contiguous series, as the class does
    return dates, returns_df.columns, simple, raw


def performance_table(returns_df: pd.DataFrame, kind: str = "log", trading_days_per_year: int = 252,
                      risk_free_rate: float = 0.0) -> pd.DataFrame:
    """K x metrics table of a dates x K frame of returns (``kind``: 'log' as the class takes them,
    or 'simple'): the reference's eight summary quantities unrounded (Sharpe and Sortino at
    ``risk_free_rate``), the daily volatility, the counts and the drawdown rows as dates / row
    counts.  One upload and one launch; row k equals ``PortfolioAnalyzer`` on column k alone bit
    for bit.  Fewer than two distinct dates give NaN for the annualised return."""
    dates, cols, simple, _ = _table_rows(returns_df, kind)
    td = trading_days_per_year
    rf = risk_free_rate / td
    stats = E.perf_stats(_upload(simple), rf, curves=False)[0].cpu().numpy()
    s = {k: stats[i] for k, i in E.PERF.items()}
    years = _years(dates)
    if years > 0:
        ann = np.array([np.float64(f)**(1 / years) - 1 for f in s["final"]], dtype=np.float64)   # K scalar powers
    else:
        ann = np.full(len(cols), np.nan)
    root = np.sqrt(td)
    dvals = dates.to_numpy()

    def row_dates(rows):
        r = rows.astype(np.int64)
        out = np.full(len(r), np.datetime64("NaT"), dtype=dvals.dtype)
        out[r >= 0] = dvals[r[r >= 0]]
        return out

    with np.errstate(divide="ignore", invalid="ignore"):
        table = pd.DataFrame({
            "Average Daily Return": s["mean"],
            "Annualized Return": ann,
            "Yearly Volatility": s["std"] * root,
            "Max Daily Return": s["max"],
            "Sharpe Ratio": (s["ex_mean"] / s["ex_std"]) * root,
            "Sortino Ratio": (s["ex_mean"] / s["down_std"]) * root,
            "Max Drawdown": s["maxdd"],
            "Min Daily Return": s["min"],
            "Daily Volatility": s["std"],
            "Observations": s["count"],
            "Negative Excess Days": s["down_count"],
            "Max Drawdown Date": row_dates(s["maxdd_row"]),
            "Max Drawdown Peak Date": row_dates(s["maxdd_peak_row"]),
            "Longest Drawdown (rows)": s["dd_run"],
        }, index=cols)
    return table


def performance_curves(returns_df: pd.DataFrame, kind: str = "log"):
    """The ``return``, ``cumulative_return`` and ``drawdown`` frames (sorted dates x K) of a dates
    x K frame of returns: column k holds the class's ``df['return']``,
    ``df['cumulative_return']`` and ``max_drawdown_curve()`` of column k alone."""
    dates, cols, simple, _ = _table_rows(returns_df, kind)
    _, cum, dd = E.perf_stats(_upload(simple), 0.0, curves=True)
    idx = pd.DatetimeIndex(dates, name="date")
    return {"return": pd.DataFrame(simple.T, index=idx, columns=cols),
            "cumulative_return": pd.DataFrame(cum.cpu().numpy().T, index=idx, columns=cols),
            "drawdown": pd.DataFrame(dd.cpu().numpy().T, index=idx, columns=cols)}


def period_returns(returns_df: pd.DataFrame, freq: str = "M", kind: str = "log") -> pd.DataFrame:
    """Calendar-month ('M') or calendar-year ('Y') returns of every column, periods x K under
    pandas' period-end labels, every period from the first date's to the last date's (an empty
    one is 0.0): column k equals the class's ``monthly_return()`` / ``yearly_return()``."""
    dates, cols, simple, _ = _table_rows(returns_df, kind)
    seg, labels = _period_buckets(dates, freq)
    out = E.perf_periods(_upload(simple), seg, len(labels))
    return pd.DataFrame(out.cpu().numpy(), index=labels, columns=cols)


def rolling_sharpe(returns_df: pd.DataFrame, window: int, trading_days_per_year: int = 252) -> pd.DataFrame:
    """``rolling(window).mean() / rolling(window).std() * sqrt(trading_days_per_year)`` of every
    column of a dates x K frame of log returns (what ``plot_full_performance`` draws), through
    the ``ts_mean`` / ``ts_std`` kernels on the table viewed as a one-factor panel."""
    dates, cols, _, raw = _table_rows(returns_df, "simple")
    X = torch.as_tensor(np.ascontiguousarray(raw.T[None]), device=device())      # [1][T][K]
    m = E.ts("mean", X, int(window)).cpu().numpy()[0]
    s = E.ts("std", X, int(window)).cpu().numpy()[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        sr = m / s * np.sqrt(trading_days_per_year)
    return pd.DataFrame(sr, index=pd.DatetimeIndex(dates, name="date"), columns=cols)
