"""Drop-in replacement for the reference's ``operations.py`` (operator library).

Same function names, arguments, return types, index order and Series names as
Yuming-Yang/FactorModeling ``operations.py``; the arithmetic runs in the gfx950 kernels
of libfmx (``engine``).  Every operator accepts a ``(date, symbol)``-indexed Series or a
DataFrame of factor columns (processed as one batched ``[F][D][A]`` panel).

Parity: rolling sums/means/stds/zscores/ranks, shifts, cross-sectional ranks, moments,
quantile ops, group ops and regressions reproduce pandas bit-for-bit; ``ts_decay``
(BLAS dot order) and ``log``/``power`` with general exponents agree to <= 1e-12
relative (tests/test_gpu_parity.py).

Non-finite inputs: like pandas' ``rolling``, the rolling aggregations (``ts_sum / mean / std /
zscore / rank / decay``, ``ts_corr``, the five means of ``ts_regression_fast``) take +-inf as
NaN -- the ``window`` windows that hold it are NaN, then the column recovers; ``ts_diff``,
``ts_delay``, ``ts_backfill`` and ``ts_decay(window < 1)`` pass it through
(tests/test_ts_nonfinite_host.py, tests/test_gpu_ts_paths.py).
"""
from __future__ import annotations

import numpy as np
import pandas as pd
import torch

from . import engine
from .panel import device, panel_index
from .profiling import phase

__all__ = [
    "ts_sum", "ts_mean", "ts_std", "ts_zscore", "ts_rank", "ts_diff", "ts_delay", "ts_decay", "ts_backfill",
    "ts_corr", "ts_skew", "ts_kurt", "ts_cov", "ts_min", "ts_max", "ts_argmin", "ts_argmax", "ts_median", "ts_quantile",
    "ts_ewm_mean", "ts_ewm_var", "ts_ewm_std", "ts_ewm_zscore", "ts_ewm_cov", "ts_ewm_corr", "cs_rank", "cs_winsor", "cs_filter_center", "cs_zscore", "cs_bool", "cs_mean", "sign", "power",
    "log", "abs_", "clip", "bucket", "group_mean", "group_neutralize", "group_normalize",
    "group_rank_normalized", "market_neutralize", "ts_regression_fast", "cs_regression",
    "cs_regression_multi", "ts_regression_multi",
]


def _matrix(obj):
    if isinstance(obj, pd.DataFrame):
        return obj.to_numpy(dtype=np.float64, na_value=np.nan)
    return obj.to_numpy(dtype=np.float64, na_value=np.nan)


def _wrap(obj, vals, name=None, keep_name=True):
    if isinstance(obj, pd.DataFrame):
        return pd.DataFrame(vals, index=obj.index, columns=obj.columns)
    return pd.Series(vals[:, 0] if vals.ndim == 2 else vals, index=obj.index,
                     name=(obj.name if keep_name else name))


def _panel_apply(obj, fn, name=None, keep_name=True):
    """Densify ``obj`` onto the device, run ``fn(X, present)`` and gather back."""
    P = panel_index(obj.index)
    dev = device()
    with phase("pandas->dense"):
        xv = _matrix(obj)
    X = P.to_device(xv, dev)
    Y = fn(X, P.present(dev))
    vals = P.from_device(Y)
    with phase("dense->pandas"):
        return _wrap(obj, vals, name, keep_name)


def _ew(obj, op, a=0.0, b=0.0):
    dev = device()
    v = torch.as_tensor(_matrix(obj), device=dev).contiguous()
    out = engine.elementwise(op, v, a, b).cpu().numpy()
    if isinstance(obj, pd.DataFrame):
        return pd.DataFrame(out, index=obj.index, columns=obj.columns)
    return pd.Series(out, index=obj.index, name=obj.name)


# ========== Time-Series Operations (operations.py:5-51) ==========
def ts_sum(series, window: int):
    """operations.py:6-7"""
    return _panel_apply(series, lambda X, p: engine.ts("sum", X, window, p))


def ts_mean(series, window: int):
    """operations.py:10-11"""
    return _panel_apply(series, lambda X, p: engine.ts("mean", X, window, p))


def ts_std(series, window: int):
    """operations.py:14-15"""
    return _panel_apply(series, lambda X, p: engine.ts("std", X, window, p))


def ts_zscore(series, window: int):
    """operations.py:18-21"""
    return _panel_apply(series, lambda X, p: engine.ts("zscore", X, window, p))


def ts_rank(series, window: int):
    """operations.py:23-32"""
    return _panel_apply(series, lambda X, p: engine.ts("rank", X, window, p))


def ts_diff(series, window: int):
    """operations.py:34-35"""
    return _panel_apply(series, lambda X, p: engine.ts("diff", X, window, p))


def ts_delay(series, window: int):
    """operations.py:37-38"""
    return _panel_apply(series, lambda X, p: engine.ts("delay", X, window, p))


def ts_decay(series, window: int):
    """operations.py:40-48 (window < 1 returns the input object itself)."""
    if window < 1:
        return series
    return _panel_apply(series, lambda X, p: engine.ts("decay", X, window, p))


def ts_backfill(series):
    """operations.py:50-51"""
    return _panel_apply(series, lambda X, p: engine.ts("backfill", X, 1, p))


def ts_corr(x, y, window: int):
    """Builder-defined (no reference counterpart): per-symbol ``x.rolling(window).corr(y)``
    with pandas semantics; ``y`` is aligned to ``x``'s index.  Series or DataFrame ``x``."""
    yv = y.reindex(x.index).to_numpy(dtype=np.float64, na_value=np.nan)
    P = panel_index(x.index)
    dev = device()
    Yd = P.to_device(yv, dev)[0]

    return _panel_apply(x, lambda X, p: engine.ts_corr(X, Yd, window, p))


# ---- rolling higher moments (builder-defined, no reference counterpart; pinned to pandas) ----
def ts_skew(series, window: int):
    """Per-symbol ``x.rolling(window).skew()``; all NaN for ``window < 3``.  pandas centres a
    symbol's series by the rounded mean of all its rows, so the last bits of a value can depend
    on later rows."""
    return _panel_apply(series, lambda X, p: engine.ts_moment("skew", X, window, p))


def ts_kurt(series, window: int):
    """Per-symbol ``x.rolling(window).kurt()`` (excess kurtosis); all NaN for ``window < 4``.
    Centred as ts_skew."""
    return _panel_apply(series, lambda X, p: engine.ts_moment("kurt", X, window, p))


def ts_cov(x, y, window: int):
    """Per-symbol ``x.rolling(window).cov(y)`` (ddof 1); ``y`` is aligned to ``x``'s index.  A
    Series ``y`` is shared by all columns of a DataFrame ``x``; a DataFrame ``y`` with ``x``'s
    columns pairs column with column."""
    per_column = isinstance(y, pd.DataFrame)
    if per_column:
        if not isinstance(x, pd.DataFrame) or list(y.columns) != list(x.columns):
            raise ValueError("ts_cov: a DataFrame y needs a DataFrame x with the same columns")
    yv = y.reindex(x.index).to_numpy(dtype=np.float64, na_value=np.nan)
    Yd = panel_index(x.index).to_device(yv, device())
    if not per_column:
        Yd = Yd[0]
    return _panel_apply(x, lambda X, p: engine.ts_moment("cov", X, window, p, Yd))


# ---- rolling order statistics (builder-defined, no reference counterpart; pinned to pandas) ----
def ts_min(series, window: int):
    """Per-symbol ``x.rolling(window).min()``."""
    return _panel_apply(series, lambda X, p: engine.ts_order("min", X, window, p))


def ts_max(series, window: int):
    """Per-symbol ``x.rolling(window).max()``."""
    return _panel_apply(series, lambda X, p: engine.ts_order("max", X, window, p))


def ts_argmin(series, window: int):
    """Rows back from the current row to the window's minimum (0.0 = the current row; ties go
    to the most recent row); NaN unless the window holds ``window`` non-NaN rows."""
    return _panel_apply(series, lambda X, p: engine.ts_order("argmin", X, window, p))


def ts_argmax(series, window: int):
    """Rows back from the current row to the window's maximum (see ts_argmin)."""
    return _panel_apply(series, lambda X, p: engine.ts_order("argmax", X, window, p))


def ts_median(series, window: int):
    """Per-symbol ``x.rolling(window).median()``."""
    return _panel_apply(series, lambda X, p: engine.ts_order("median", X, window, p))


def ts_quantile(series, window: int, q: float, interpolation: str = "linear"):
    """Per-symbol ``x.rolling(window).quantile(q, interpolation=interpolation)``."""
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"quantile value {q} not in [0, 1]")
    if interpolation not in engine.TSO_INTERP:
        raise ValueError(f"interpolation {interpolation!r} is not one of {sorted(engine.TSO_INTERP)}")
    return _panel_apply(series, lambda X, p: engine.ts_order("quantile", X, window, p, q, interpolation))


# ---- exponentially weighted operators (builder-defined, no reference counterpart; pinned to pandas) ----
def _ewm_com(com=None, span=None, halflife=None, alpha=None) -> float:
    """The centre of mass of exactly one decay parameter, by pandas' own ranges and arithmetic
    (pandas.core.window.common.get_center_of_mass): the kernel's alpha = 1 / (1 + com) then
    carries pandas' rounding."""
    given = [v is not None for v in (com, span, halflife, alpha)]
    if sum(given) > 1:
        raise ValueError("com, span, halflife and alpha are mutually exclusive")
    if not any(given):
        raise ValueError("Must pass one of com, span, halflife or alpha")
    if com is not None:
        if not com >= 0:
            raise ValueError("com must satisfy: com >= 0")
    elif span is not None:
        if not span >= 1:
            raise ValueError("span must satisfy: span >= 1")
        com = (span - 1) / 2
    elif halflife is not None:
        if not halflife > 0:
            raise ValueError("halflife must satisfy: halflife > 0")
        decay = 1 - np.exp(np.log(0.5) / halflife)
        com = 1 / decay - 1
    else:
        if not 0 < alpha <= 1:
            raise ValueError("alpha must satisfy: 0 < alpha <= 1")
        com = (1 - alpha) / alpha
    return float(com)


def _ewm_apply(x, name, y, com, span, halflife, alpha, adjust, ignore_na, min_periods):
    c = _ewm_com(com, span, halflife, alpha)
    if int(min_periods) != min_periods or min_periods < 0:
        raise ValueError("min_periods must be an integer >= 0")
    Yd = None
    if y is not None:
        yv = y.reindex(x.index).to_numpy(dtype=np.float64, na_value=np.nan)
        Yd = panel_index(x.index).to_device(yv, device())[0]
    return _panel_apply(x, lambda X, p: engine.ts_ewm(X, {name: None}, c, adjust, ignore_na, int(min_periods),
                                                      p, Yd)[name])


def ts_ewm_mean(x, com=None, span=None, halflife=None, alpha=None, adjust=True, ignore_na=False, min_periods=0):
    """Per-symbol ``x.ewm(...).mean()``; exactly one of com / span / halflife / alpha."""
    return _ewm_apply(x, "mean", None, com, span, halflife, alpha, adjust, ignore_na, min_periods)


def ts_ewm_var(x, com=None, span=None, halflife=None, alpha=None, adjust=True, ignore_na=False, min_periods=0):
    """Per-symbol ``x.ewm(...).var()`` (bias=False)."""
    return _ewm_apply(x, "var", None, com, span, halflife, alpha, adjust, ignore_na, min_periods)


def ts_ewm_std(x, com=None, span=None, halflife=None, alpha=None, adjust=True, ignore_na=False, min_periods=0):
    """Per-symbol ``x.ewm(...).std()`` (bias=False)."""
    return _ewm_apply(x, "std", None, com, span, halflife, alpha, adjust, ignore_na, min_periods)


def ts_ewm_zscore(x, com=None, span=None, halflife=None, alpha=None, adjust=True, ignore_na=False, min_periods=0):
    """``(x - ts_ewm_mean(x)) / ts_ewm_std(x)`` from one pass over ``x``."""
    return _ewm_apply(x, "zscore", None, com, span, halflife, alpha, adjust, ignore_na, min_periods)


def ts_ewm_cov(x, y, com=None, span=None, halflife=None, alpha=None, adjust=True, ignore_na=False, min_periods=0):
    """Per-symbol ``x.ewm(...).cov(y)`` (bias=False); ``y`` is a Series aligned to ``x``'s index,
    shared by all columns of a DataFrame ``x``."""
    return _ewm_apply(x, "cov", y, com, span, halflife, alpha, adjust, ignore_na, min_periods)


def ts_ewm_corr(x, y, com=None, span=None, halflife=None, alpha=None, adjust=True, ignore_na=False, min_periods=0):
    """Per-symbol ``x.ewm(...).corr(y)``; ``y`` as in ts_ewm_cov."""
    return _ewm_apply(x, "corr", y, com, span, halflife, alpha, adjust, ignore_na, min_periods)


# ========== Cross section (operations.py:53-86) ==========
def cs_rank(series, method="average"):
    """operations.py:54-62"""
    return _panel_apply(series, lambda X, p: engine.cs_rank(X, method, p))


def _pandas_q(q):
    # pandas Series.quantile hands q*100 to np.percentile, which divides by 100 again
    return float(np.true_divide(np.asarray([q], dtype=np.float64) * 100.0, 100)[0])


def cs_winsor(series, limits=(0.01, 0.99)):
    """operations.py:64-68"""
    qlo, qhi = _pandas_q(limits[0]), _pandas_q(limits[1])
    return _panel_apply(series, lambda X, p: engine.cs_quantile_op("winsor", X, qlo, qhi, p))


def cs_filter_center(series, center=(0.3, 0.7)):
    """operations.py:70-75"""
    qlo, qhi = _pandas_q(center[0]), _pandas_q(center[1])
    return _panel_apply(series, lambda X, p: engine.cs_quantile_op("filter_center", X, qlo, qhi, p))


def cs_zscore(series):
    """operations.py:77-78"""
    return _panel_apply(series, lambda X, p: engine.cs_moment("zscore", X, p))


def cs_bool(condition, true_value: float, false_value: float):
    """operations.py:80-84 -- unnamed Series on condition.index."""
    dev = device()
    c = torch.as_tensor(np.asarray(condition, dtype=bool).astype(np.float64), device=dev)
    out = engine.elementwise("where", c, true_value, false_value).cpu().numpy()
    return pd.Series(out, index=condition.index)


def cs_mean(series):
    """operations.py:85-86"""
    return _panel_apply(series, lambda X, p: engine.cs_moment("mean", X, p))


# ========== Math (operations.py:88-101) ==========
def sign(series):
    return _ew(series, "sign")


def power(series, exp: float):
    return _ew(series, "power", float(exp))


def log(series):
    return _ew(series, "log")


def abs_(series):
    return _ew(series, "abs")


def clip(series, lower, upper):
    return _ew(series, "clip", float(lower), float(upper))


# ========== Group Operations (operations.py:103-168) ==========
def bucket(series, bin_range=(0.2, 1.0, 0.2)):
    """operations.py:104-110 -- categorical labels group1..groupK (pd.cut, right-closed,
    include_lowest); rows come out in date-group order like groupby(...).apply."""
    low, up, step = bin_range
    edges = np.arange(low, up + 1e-8, step)
    labels = [f"group{i + 1}" for i in range(len(edges) - 1)]
    dev = device()
    v = torch.as_tensor(series.to_numpy(dtype=np.float64, na_value=np.nan), device=dev)
    codes = engine.bucket_codes(v, edges).cpu().numpy()
    P = panel_index(series.index)
    order = np.argsort(P.d, kind="stable")
    cat = pd.Categorical.from_codes(codes[order], categories=labels, ordered=True)
    return pd.Series(cat, index=series.index[order], name=series.name)


def _group_ids(series, group):
    g = group.reindex(series.index) if not group.index.equals(series.index) else group
    codes, uniq = pd.factorize(g, sort=True)
    return codes.astype(np.int32), len(uniq)


def _group_apply(series, group, op, method="average"):
    P = panel_index(series.index)
    dev = device()
    codes, ng = _group_ids(series, group)
    Gd = np.full(P.D * P.A, -1, dtype=np.int32)
    Gd[P.flat] = codes
    G = torch.as_tensor(Gd.reshape(P.D, P.A), device=dev)
    X = P.to_device(_matrix(series), dev)
    Y = engine.group_op(op, X, G, ng, method, P.present(dev))
    return pd.Series(P.from_device(Y)[:, 0], index=series.index, name="val")


def group_mean(series, group):
    """operations.py:112-122"""
    return _group_apply(series, group, "mean")


def group_neutralize(series, group):
    """operations.py:124-134"""
    return _group_apply(series, group, "neutralize")


def group_normalize(series, group):
    """operations.py:137-149"""
    return _group_apply(series, group, "normalize")


def group_rank_normalized(series, group, method="average"):
    """operations.py:152-168"""
    return _group_apply(series, group, "rank", method)


def market_neutralize(series):
    """operations.py:171-182"""
    return _panel_apply(series, lambda X, p: engine.cs_moment("market_neutralize", X, p))


# ========== Regressions (operations.py:185-304) ==========
def ts_regression_fast(y, x, window: int, lag: int = 0, rettype: int = 2):
    """operations.py:185-246 -- rolling per-symbol OLS via moments.  ``x.shift(lag)`` is
    the reference's global row shift; rows with NaN y or shifted x are dropped; the
    result keeps non-NaN rows only, sorted by (date, symbol)."""
    if rettype not in (0, 1, 2, 3, 6):
        raise ValueError("rettype not implemented")
    xs = x.shift(lag)
    df = pd.DataFrame({"y": y, "x": xs})
    P = panel_index(df.index)
    dev = device()
    yv = df["y"].to_numpy(dtype=np.float64, na_value=np.nan)
    xv = df["x"].to_numpy(dtype=np.float64, na_value=np.nan)
    ok = ~np.isnan(yv) & ~np.isnan(xv)
    Yd = P.to_device(yv, dev)[0]
    Xd = P.to_device(xv, dev)[0]
    valid = np.zeros(P.D * P.A, dtype=np.uint8)
    valid[P.flat[ok]] = 1
    Vd = torch.as_tensor(valid.reshape(P.D, P.A), device=dev)
    out = engine.ts_regression(Yd, Xd, Vd, window, rettype).cpu().numpy().reshape(-1)
    cells = P.flat[ok]
    vals = out[cells]
    keep = ~np.isnan(vals)
    cells, vals = cells[keep], vals[keep]
    order = np.argsort(cells, kind="stable")           # (date, symbol) lexicographic
    cells, vals = cells[order], vals[order]
    idx = pd.MultiIndex.from_arrays([P.dates[cells // P.A], P.symbols[cells % P.A]], names=["date", "symbol"])
    return pd.Series(vals, index=idx)


def cs_regression(y, x, rettype: str = "resid"):
    """operations.py:248-304 -- per-date OLS, reindexed onto y.index."""
    if rettype not in ("resid", "beta", "alpha", "fitted", "r2"):
        raise ValueError(f"ERROR: rettype={rettype}")
    P = panel_index(y.index)
    dev = device()
    xv = x.reindex(y.index).to_numpy(dtype=np.float64, na_value=np.nan)
    Yd = P.to_device(y.to_numpy(dtype=np.float64, na_value=np.nan), dev)[0]
    Xd = P.to_device(xv, dev)[0]
    out = engine.cs_regression(Yd, Xd, rettype, P.present(dev))
    return pd.Series(P.from_device(out[None])[:, 0], index=y.index)


def cs_regression_multi(y, X, rettype: str = "resid", intercept: bool = True, weights=None):
    """Builder-defined (no reference counterpart): per-date least squares of ``y`` on the K
    columns of the DataFrame ``X`` (``engine.cs_ols``), optionally weighted and with an
    intercept; ``X`` and ``weights`` are aligned to ``y``'s index.  ``y`` is a Series or a
    DataFrame of columns (one batched call).  A row enters a date's fit when y, every X column
    and the weight (> 0) are finite; columns collinear with the ones before them are dropped.

    ``rettype`` in resid | fitted | alpha | r2 returns an object like ``y`` (alpha and r2
    broadcast over the fitted rows, NaN elsewhere); ``"beta"`` returns a ``dates x X.columns``
    DataFrame and needs a Series ``y``."""
    if rettype not in ("resid", "fitted", "alpha", "r2", "beta"):
        raise ValueError(f"ERROR: rettype={rettype}")
    if not isinstance(X, pd.DataFrame):
        raise ValueError("X must be a DataFrame of regressor columns")
    frame = isinstance(y, pd.DataFrame)
    if rettype == "beta" and frame:
        raise ValueError("rettype='beta' needs a Series y (one coefficient table per y column)")
    P = panel_index(y.index)
    dev = device()
    Yd = P.to_device(_matrix(y), dev)
    Xd = P.to_device(X.reindex(y.index).to_numpy(dtype=np.float64, na_value=np.nan), dev)
    Wd = None
    if weights is not None:
        Wd = P.to_device(weights.reindex(y.index).to_numpy(dtype=np.float64, na_value=np.nan), dev)[0]
    present = P.present(dev)
    if rettype == "beta":
        beta = engine.cs_ols(Yd, Xd, Wd, present, intercept, want=("beta",))["beta"][0]
        return pd.DataFrame(beta.cpu().numpy(), index=pd.Index(P.dates, name="date"), columns=X.columns)
    if rettype in ("resid", "fitted"):
        out = engine.cs_ols(Yd, Xd, Wd, present, intercept, want=(rettype,))[rettype]
    else:
        # the per-date scalar on the rows of the fit: resid is non-NaN exactly there
        res = engine.cs_ols(Yd, Xd, Wd, present, intercept, want=(rettype, "resid"))
        out = torch.where(torch.isnan(res["resid"]), res["resid"], res[rettype].unsqueeze(-1))
    vals = P.from_device(out)
    if frame:
        return pd.DataFrame(vals, index=y.index, columns=y.columns)
    return pd.Series(vals[:, 0], index=y.index, name=y.name)


def ts_regression_multi(y, X, window: int, lag: int = 0, rettype: str = "resid", intercept: bool = True):
    """Builder-defined (no reference counterpart): rolling per-symbol least squares of ``y`` on
    the K columns of the DataFrame ``X`` over the symbol's last ``window`` valid rows
    (``engine.ts_ols``; the rolling counterpart of ``cs_regression_multi``).  ``y`` is a Series
    or a DataFrame of columns (one batched call).  ``X`` with a (date, symbol) MultiIndex holds
    per-symbol regressors and is aligned to ``y``'s index; ``X`` with a plain date index holds
    regressors shared by all symbols (factor returns) and is reindexed to the panel's dates.

    A row is valid when y and every X column are finite; invalid rows drop out of the symbol's
    sequence (``ts_regression_fast``'s dropna-then-roll, per symbol), and a result exists on a
    valid row once the symbol has ``window`` valid rows.  Columns collinear with the ones
    before them inside a window are dropped there.  ``lag`` delays the regressors by ``lag`` of
    the symbol's OWN rows (``ts_delay``); a shared table is delayed by ``lag`` table rows.  This
    is NOT the reference's ``x.shift(lag)``, a global row shift that crosses symbols.

    ``rettype`` in resid | fitted | alpha | r2 | sigma returns an object like ``y`` on ``y``'s
    index, NaN where undefined (nothing is dropped); ``"beta"`` needs a Series ``y`` and
    returns a DataFrame on ``y.index`` with ``X.columns``."""
    if rettype not in ("resid", "fitted", "alpha", "r2", "sigma", "beta"):
        raise ValueError(f"ERROR: rettype={rettype}")
    if not isinstance(X, pd.DataFrame):
        raise ValueError("X must be a DataFrame of regressor columns")
    frame = isinstance(y, pd.DataFrame)
    if rettype == "beta" and frame:
        raise ValueError("rettype='beta' needs a Series y (one coefficient table per y column)")
    if int(lag) < 0:
        raise ValueError("lag must be >= 0")
    P = panel_index(y.index)
    dev = device()
    Yd = P.to_device(_matrix(y), dev)
    present = P.present(dev)
    shared = not isinstance(X.index, pd.MultiIndex)
    if shared:
        tab = X.reindex(P.dates).shift(int(lag)).to_numpy(dtype=np.float64, na_value=np.nan)
        Xd = torch.as_tensor(np.ascontiguousarray(tab.T), device=dev)
    else:
        Xd = P.to_device(X.reindex(y.index).to_numpy(dtype=np.float64, na_value=np.nan), dev)
        if lag:
            Xd = engine.ts("delay", Xd, int(lag), present)
    out = engine.ts_ols(Yd, Xd, window, present, intercept, shared, want=(rettype,))[rettype]
    if rettype == "beta":
        return pd.DataFrame(P.from_device(out[0]), index=y.index, columns=X.columns)
    vals = P.from_device(out)
    if frame:
        return pd.DataFrame(vals, index=y.index, columns=y.columns)
    return pd.Series(vals[:, 0], index=y.index, name=y.name)
