"""Device-tensor API over libfmx: every function takes/returns torch CUDA (HIP) tensors
laid out ``[F][D][A]`` float64 (asset fastest) and launches the gfx950 kernels on the
current torch stream.  Shapes are validated on the host before any launch.

This is the layer the drop-in pandas modules, the benchmark and the date-sharded
multi-GPU driver are built on.
"""
from __future__ import annotations

import os
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import CS, CSREG, EW, EWM, GROUP, RANK, TS, TSM, TSO, TSO_INTERP, call, ptr, stream_ptr

F64 = torch.float64


def _check_panel(X, name="X"):
    if not isinstance(X, torch.Tensor) or X.device.type != "cuda":
        raise _lib.FmxError(f"{name} must be a HIP device tensor")
    if X.dtype != F64:
        raise _lib.FmxError(f"{name} must be float64")
    if X.dim() != 3:
        raise _lib.FmxError(f"{name} must be [F][D][A]")
    if not X.is_contiguous():
        raise _lib.FmxError(f"{name} must be contiguous")


def _check_present(present, D, A):
    if present is None:
        return None
    if present.dtype != torch.uint8 or tuple(present.shape) != (D, A) or not present.is_contiguous():
        raise _lib.FmxError("present must be a contiguous uint8 [D][A] device tensor")
    return present


def as3(X):
    return X if X.dim() == 3 else X.unsqueeze(0)


def empty_like(X):
    return torch.empty_like(X)


# ----------------------------------------------------------------------------- time series
def ts(op: str, X, window: int, present=None, out=None):
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    _check_present(present, D, A)
    Y = _out(X, out)
    call("fmx_ts_op", TS[op], ptr(X), ptr(Y), F, D, A, A, int(window), ptr(present), stream_ptr())
    return Y


def ts_order(op: str, X, window: int, present=None, q=0.5, interpolation="linear", out=None):
    """Rolling order statistic (fmx_ts_order): ``op`` in min / max / argmin / argmax / median /
    quantile; ``q`` and ``interpolation`` are read for quantile only."""
    if op not in TSO:
        raise ValueError(f"ts_order: unknown op {op!r}")
    if interpolation not in TSO_INTERP:
        raise ValueError(f"ts_order: unknown interpolation {interpolation!r}")
    if op == "quantile" and not 0.0 <= q <= 1.0:
        raise ValueError(f"quantile value {q} not in [0, 1]")
    if int(window) < 1:
        raise ValueError("window must be >= 1")
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    _check_present(present, D, A)
    Y = _out(X, out)
    call("fmx_ts_order", TSO[op], ptr(X), ptr(Y), F, D, A, A, int(window), float(q), TSO_INTERP[interpolation],
         ptr(present), stream_ptr())
    return Y


def ts_moment(op: str, X, window: int, present=None, y=None, out=None):
    """Rolling higher moment (fmx_ts_moment): ``op`` in skew / kurt / cov, pandas'
    ``rolling(window).skew() / .kurt() / .cov(y)`` per symbol.  ``y`` is read for cov only: a
    [D][A] series shared by all columns or a [F][D][A] panel, float64, on X's device."""
    if op not in TSM:
        raise ValueError(f"ts_moment: unknown op {op!r}")
    if int(window) < 1:
        raise ValueError("window must be >= 1")
    if op == "cov" and y is None:
        raise ValueError("ts_moment: cov needs y")
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    _check_present(present, D, A)
    ystride = 0
    if op != "cov":
        y = None
    else:
        if not isinstance(y, torch.Tensor) or y.device != X.device or y.dtype != F64 or \
                tuple(y.shape) not in ((D, A), (F, D, A)):
            raise _lib.FmxError("y must be a float64 [D][A] or [F][D][A] tensor on X's device")
        ystride = D * A if y.dim() == 3 else 0
        y = y.contiguous()
    Y = _out(X, out)
    call("fmx_ts_moment", TSM[op], ptr(X), ptr(y), ptr(Y), F, D, A, A, ystride, int(window), ptr(present),
         stream_ptr())
    return Y


TS_SET = ("mean", "std", "zscore", "rank", "decay")


def ts_set(X, outs: dict, window: int, rank_window: int, present=None):
    """Fused rolling set (fmx_ts_set): ``outs`` maps a subset of TS_SET to output
    tensors shaped like X; mean/std/zscore/decay use ``window``, rank ``rank_window``."""
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    _check_present(present, D, A)
    bad = set(outs) - set(TS_SET)
    if bad:
        raise ValueError(f"ts_set: unsupported ops {sorted(bad)}")
    ps = [ptr(_out(X, outs[k])) if k in outs else None for k in TS_SET]
    call("fmx_ts_set", ptr(X), *ps, F, D, A, A, int(window), int(rank_window), ptr(present), stream_ptr())
    return outs


TS_EWM = tuple(EWM)          # mean var std zscore cov corr, fmx_ts_ewm's argument order


def ts_ewm(X, outs: dict, com: float, adjust=True, ignore_na=False, min_periods=0, present=None, y=None):
    """Exponentially weighted operators (fmx_ts_ewm): ``outs`` maps a subset of TS_EWM to output
    tensors shaped like X (None: allocated here) and is returned filled.  mean / var / std /
    zscore share one pass over X; cov / corr need ``y``, a [D][A] series shared by all columns.
    ``com`` is the centre of mass (alpha = 1 / (1 + com)); pandas' ewm semantics."""
    bad = set(outs) - set(TS_EWM)
    if bad:
        raise ValueError(f"ts_ewm: unsupported outputs {sorted(bad)}")
    if not outs:
        raise ValueError("ts_ewm: no output requested")
    com = float(com)
    if not com >= 0.0:
        raise ValueError("ts_ewm: com must be >= 0")
    if int(min_periods) < 0:
        raise ValueError("ts_ewm: min_periods must be >= 0")
    if ("cov" in outs or "corr" in outs) and y is None:
        raise ValueError("ts_ewm: cov / corr need y")
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    _check_present(present, D, A)
    if y is not None:
        if not isinstance(y, torch.Tensor) or y.device != X.device or y.dtype != F64 or tuple(y.shape) != (D, A):
            raise _lib.FmxError("y must be a float64 [D][A] tensor on X's device")
        y = y.contiguous()
    for k in outs:
        outs[k] = _out(X, outs[k])
    ps = [ptr(outs.get(k)) for k in TS_EWM]
    call("fmx_ts_ewm", ptr(X), ptr(y), *ps, F, D, A, A, com, int(bool(adjust)), int(bool(ignore_na)),
         int(min_periods), ptr(present), stream_ptr())
    return outs


def ts_corr(X, Ycol, window: int, present=None, out=None):
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    _check_present(present, D, A)
    if Ycol.dim() == 2:
        if tuple(Ycol.shape) != (D, A):
            raise _lib.FmxError("Ycol must be [D][A] or [F][D][A]")
        ystride = 0
    else:
        if tuple(Ycol.shape) != (F, D, A):
            raise _lib.FmxError("Ycol must be [D][A] or [F][D][A]")
        ystride = D * A
    Ycol = Ycol.contiguous()
    out = _out(X, out)
    call("fmx_ts_corr", ptr(X), ptr(Ycol), ptr(out), F, D, A, A, ystride, int(window), ptr(present), stream_ptr())
    return out


# fmx_ts_corr_feature keeps the window's reciprocal table in LDS up to this window
# (ts_ops.hip TSC_MAXW); longer windows take ts_corr + corr_vol_feature
CORR_FEATURE_MAX_W = 4096


def corr_feature(X, Ycol, window: int, out=None, corr_out=None):
    """C5's feature sign(ts_corr(X, Ycol, window)) * (X / ts_std(X, window)) in one pass
    (fmx_ts_corr_feature): bit-identical to ts_corr + corr_vol_feature, without the corr
    panel's round trip.  ``corr_out`` (optional) also receives the corr.  Dense panels."""
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    if Ycol.dim() == 2:
        if tuple(Ycol.shape) != (D, A):
            raise _lib.FmxError("Ycol must be [D][A] or [F][D][A]")
        ystride = 0
    else:
        if tuple(Ycol.shape) != (F, D, A):
            raise _lib.FmxError("Ycol must be [D][A] or [F][D][A]")
        ystride = D * A
    Ycol = Ycol.contiguous()
    out = _out(X, out)
    if corr_out is not None:
        corr_out = _out(X, corr_out)
    call("fmx_ts_corr_feature", ptr(X), ptr(Ycol), ptr(corr_out), ptr(out), F, D, A, A, ystride, int(window),
         stream_ptr())
    return out


def corr_vol_feature(X, C, window: int, out=None):
    """C5's feature sign(C) * (X / ts_std(X, window)) (fmx_ts_corr_vol_feature); C is
    ts_corr(X, R, window) of the same rows (same shape as X)."""
    X = as3(X)
    _check_panel(X)
    C = as3(C)
    _check_panel(C, "C")
    if C.shape != X.shape:
        raise _lib.FmxError("C must be shaped like X")
    F, D, A = X.shape
    out = _out(X, out)
    call("fmx_ts_corr_vol_feature", ptr(X), ptr(C), ptr(out), F, D, A, A, int(window), stream_ptr())
    return out


def ts_regression(Yv, Xv, valid, window: int, rettype: int):
    D, A = Yv.shape
    if tuple(Xv.shape) != (D, A) or tuple(valid.shape) != (D, A) or valid.dtype != torch.uint8:
        raise _lib.FmxError("ts_regression: shape mismatch")
    out = torch.empty_like(Yv)
    call("fmx_ts_regression", ptr(Yv), ptr(Xv), ptr(valid), ptr(out), D, A, A, int(window), int(rettype),
         stream_ptr())
    return out


TS_OLS_MAX_K = 8            # fmx_ts_ols: the (K + 1)(K + 2) / 2 Gram entries live in registers
TS_OLS_OUTPUTS = ("beta", "alpha", "fitted", "resid", "r2", "sigma")


def ts_ols(Y, X, window: int, present=None, intercept=True, shared=False, want=TS_OLS_OUTPUTS):
    """Rolling multi-factor OLS (fmx_ts_ols): for every column of ``Y`` [Fy][D][A]
    (or [D][A]) and every symbol and date, the least squares of the symbol's last ``window``
    valid rows on K regressors -- ``X`` [K][D][A] per symbol or, with ``shared``, a table
    [K][D] common to all symbols (factor returns).  A row is valid when it is present and y
    and all K regressors are finite; invalid rows drop out of the symbol's sequence.  Returns
    a dict of device tensors for the names in ``want``: beta [Fy][K][D][A]; alpha, fitted,
    resid, r2, sigma [Fy][D][A]; NaN where the row is invalid or the symbol has fewer than
    ``window`` valid rows so far.  Collinear columns are dropped in column order (beta NaN)."""
    Y = as3(Y)
    _check_panel(Y, "Y")
    Fy, D, A = Y.shape
    if not isinstance(X, torch.Tensor) or X.device.type != "cuda" or X.dtype != F64 or not X.is_contiguous():
        raise _lib.FmxError("ts_ols: X must be a contiguous float64 HIP device tensor")
    if shared:
        if X.dim() != 2 or X.shape[1] != D:
            raise _lib.FmxError(f"ts_ols: shared X is {tuple(X.shape)}, expected [K][{D}] to match Y")
    elif X.dim() != 3 or tuple(X.shape[1:]) != (D, A):
        raise _lib.FmxError(f"ts_ols: X is {tuple(X.shape)}, expected [K][{D}][{A}] to match Y")
    K = X.shape[0]
    _check_present(present, D, A)
    if not 1 <= K <= TS_OLS_MAX_K:
        raise _lib.FmxError(f"ts_ols: K = {K} regressors; the kernel takes 1..{TS_OLS_MAX_K}")
    p = K + int(bool(intercept))
    if int(window) < p:
        raise _lib.FmxError(f"ts_ols: window = {window} is shorter than the {p} coefficients")
    bad = set(want) - set(TS_OLS_OUTPUTS)
    if bad:
        raise ValueError(f"ts_ols: unknown outputs {sorted(bad)}")
    dev = Y.device
    out = {k: torch.empty((Fy, K, D, A) if k == "beta" else (Fy, D, A), dtype=F64, device=dev) for k in want}
    work = torch.empty((Fy, D, A), dtype=torch.uint8, device=dev)
    call("fmx_ts_ols", ptr(Y), ptr(X), ptr(present), Fy, K, D, A, A, int(window), int(bool(intercept)),
         int(bool(shared)), *(ptr(out.get(k)) for k in TS_OLS_OUTPUTS), ptr(work), stream_ptr())
    return out


# ----------------------------------------------------------------------------- cross section
def _out(X, out):
    if out is None:
        return torch.empty_like(X)
    if out.shape != X.shape or out.dtype != X.dtype or not out.is_contiguous() or out.data_ptr() == X.data_ptr():
        raise _lib.FmxError("out must be a distinct contiguous tensor shaped like X")
    return out


def cs_moment(op: str, X, present=None, out=None):
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    _check_present(present, D, A)
    Y = _out(X, out)
    call("fmx_cs_moment", CS[op], ptr(X), ptr(Y), F, D, A, A, ptr(present), stream_ptr())
    return Y


def cs_moment_stats(op: str, X, present=None, out=None):
    """fmx_cs_moment plus the per-row (mean, std ddof=0) [F][D][2]; op 'stats' returns
    (None, stats) without writing an output panel."""
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    _check_present(present, D, A)
    Y = None if op == "stats" else _out(X, out)
    stats = torch.empty((F, D, 2), dtype=F64, device=X.device)
    call("fmx_cs_moment_stats", CS[op], ptr(X), ptr(Y), F, D, A, A, ptr(present), ptr(stats), stream_ptr())
    return Y, stats


def cs_zscore_neutralize(X, out_z=None, out_n=None, present=None, with_stats=False):
    """cs_zscore and market_neutralize from one set of row moments (fmx_cs_zscore_neutralize).
    Returns (Yz, Yn) or (Yz, Yn, stats[F][D][2])."""
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    _check_present(present, D, A)
    Yz, Yn = _out(X, out_z), _out(X, out_n)
    stats = torch.empty((F, D, 2), dtype=F64, device=X.device) if with_stats else None
    call("fmx_cs_zscore_neutralize", ptr(X), ptr(Yz), ptr(Yn), F, D, A, A, ptr(present), ptr(stats), stream_ptr())
    return (Yz, Yn, stats) if with_stats else (Yz, Yn)


RANKED_IC_MAX_A = 16384
FINE_RANK_MAX_A = 16384     # fine-bucket rank / quantile kernels; longer rows are sorted in HBM
RANK2_DTYPE = torch.int16   # fmx_rank2_t: doubled ranks <= 2A as uint16 bit patterns
BITONIC_RANK_MAX_A = 8192   # fmx_cs_rank's LDS bitonic path (methods first / dense)
_WORK = {}


def _workspace(device, n):
    """Device scratch of >= n int32 words for the library calls that take a workspace
    (fmx_*_work_len / fmx_*_work_bytes): one buffer per (device, stream), grown on demand
    and reused, so the hot path never allocates.  Calls on one stream are ordered, so
    consecutive ops share it safely; another stream gets its own buffer."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    w = _WORK.get(key)
    if w is None or w.numel() < n:
        w = torch.empty(max(n, 1), dtype=torch.int32, device=device)
        _WORK[key] = w
    return w


def _workspace_bytes(device, nbytes):
    n = (int(nbytes) + 3) // 4
    return _workspace(device, n), 4 * max(n, 1)


def cs_rank_winsor(X, qlo=0.01, qhi=0.99, out_rank=None, out_winsor=None, present=None, rank2=None):
    """cs_rank(average) and cs_winsor(qlo, qhi) in one pass (fmx_cs_rank_winsor).
    ``rank2`` (int16 tensor shaped like X, bit pattern uint16): also the doubled ranks that
    ``ic_daily(..., rank2=)`` starts from."""
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    _check_present(present, D, A)
    Yr, Yw = _out(X, out_rank), _out(X, out_winsor)
    if rank2 is not None:
        if rank2.dtype != RANK2_DTYPE or tuple(rank2.shape) != (F, D, A) or not rank2.is_contiguous():
            raise _lib.FmxError("rank2 must be a contiguous int16 (bit pattern uint16) [F][D][A] tensor")
    if A > FINE_RANK_MAX_A and rank2 is None:
        # rows past the fused kernel: both operators from rows sorted in HBM
        cs_rank(X, "average", present, out=Yr)
        cs_quantile_op("winsor", X, qlo, qhi, present, out=Yw)
        return Yr, Yw
    call("fmx_cs_rank_winsor", ptr(X), ptr(Yr), ptr(Yw), F, D, A, A, float(qlo), float(qhi), ptr(present),
         ptr(rank2), stream_ptr())
    return Yr, Yw


def cs_rank_winsor_zn(X, qlo=0.01, qhi=0.99, out_rank=None, out_winsor=None, out_zscore=None, out_neutralize=None,
                      rank2=None, dates=None):
    """cs_rank(average), cs_winsor(qlo, qhi), cs_zscore and market_neutralize of the same
    dense rows in one pass (fmx_cs_rank_winsor_zn: each row read once); every output is
    bit-identical to its own kernel.  ``rank2``: also the doubled ranks (as cs_rank_winsor).
    ``dates`` = (d0, d1): only the rows of those dates (fmx_cs_rank_winsor_zn_dates; the other
    rows of the outputs are left as they are; A <= 16384).
    Returns (Yrank, Ywinsor, Yzscore, Yneutralize)."""
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    outs = [_out(X, o) for o in (out_rank, out_winsor, out_zscore, out_neutralize)]
    if rank2 is not None:
        if rank2.dtype != RANK2_DTYPE or tuple(rank2.shape) != (F, D, A) or not rank2.is_contiguous():
            raise _lib.FmxError("rank2 must be a contiguous int16 (bit pattern uint16) [F][D][A] tensor")
    if dates is not None:
        d0, d1 = (int(d) for d in dates)
        call("fmx_cs_rank_winsor_zn_dates", ptr(X), *[ptr(o) for o in outs], F, D, A, A, d0, d1, float(qlo),
             float(qhi), ptr(rank2), stream_ptr())
        return tuple(outs)
    if A > FINE_RANK_MAX_A and rank2 is None:
        cs_rank_winsor(X, qlo, qhi, outs[0], outs[1])
        cs_zscore_neutralize(X, outs[2], outs[3])
        return tuple(outs)
    call("fmx_cs_rank_winsor_zn", ptr(X), *[ptr(o) for o in outs], F, D, A, A, float(qlo), float(qhi), ptr(rank2),
         stream_ptr())
    return tuple(outs)


def cs_rank_winsor_ic(X, R, lags=(1, 2), qlo=0.01, qhi=0.99, out_rank=None, out_winsor=None, ranks_only=False,
                      rank2=None):
    """cs_rank(average) + cs_winsor(qlo, qhi) and the daily IC records of the same rows in
    ONE pass (fmx_cs_rank_winsor_ic): returns (Yrank, Ywinsor, daily [L][4][F][D]);
    ``ranks_only``: no operator outputs (the IC's rank pass alone; Yrank = Ywinsor = None).
    ``rank2``: int16 [F][D][A] scratch for rows with long NaN-return lists (allocated when
    None).  Dense rows, A <= 16384, one or two lags."""
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    if tuple(R.shape) != (D, A) or R.dtype != F64 or not R.is_contiguous() or R.device != X.device:
        raise _lib.FmxError("R must be a contiguous float64 [D][A] tensor on X's device")
    if len(lags) not in (1, 2):
        raise _lib.FmxError("cs_rank_winsor_ic: one or two lags")
    Yr = Yw = None
    if not ranks_only:
        Yr, Yw = _out(X, out_rank), _out(X, out_winsor)
    if rank2 is None:
        rank2 = torch.empty((F, D, A), dtype=RANK2_DTYPE, device=X.device)
    elif rank2.dtype != RANK2_DTYPE or tuple(rank2.shape) != (F, D, A) or not rank2.is_contiguous():
        raise _lib.FmxError("rank2 must be a contiguous int16 [F][D][A] tensor")
    lag_h = (ctypes.c_int32 * len(lags))(*[int(v) for v in lags])
    n = int(_lib.load().fmx_rank_ic_work_len(F, D, A))
    work = _workspace(X.device, n)
    out = torch.empty((len(lags), 4, F, D), dtype=F64, device=X.device)
    call("fmx_cs_rank_winsor_ic", ptr(X), ptr(Yr), ptr(Yw), ptr(R), F, D, A, A, float(qlo), float(qhi),
         ctypes.cast(lag_h, ctypes.c_void_p), len(lags), ptr(rank2), ptr(work), n, ptr(out), stream_ptr())
    return Yr, Yw, out


def cs_rank2(X, rank2=None, dates=None):
    """Doubled average ranks only (fmx_cs_rank2): the rank pass ``ic_daily(..., rank2=)``
    starts from when no operator output of the rows is wanted (dense rows, A <= 16384).
    ``dates`` = (d0, d1): only the rows of those dates (fmx_cs_rank2_dates)."""
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    if rank2 is None:
        rank2 = torch.empty((F, D, A), dtype=RANK2_DTYPE, device=X.device)
    elif rank2.dtype != RANK2_DTYPE or tuple(rank2.shape) != (F, D, A) or not rank2.is_contiguous():
        raise _lib.FmxError("rank2 must be a contiguous int16 [F][D][A] tensor")
    if dates is not None:
        d0, d1 = (int(d) for d in dates)
        call("fmx_cs_rank2_dates", ptr(X), ptr(rank2), F, D, A, A, d0, d1, stream_ptr())
        return rank2
    call("fmx_cs_rank2", ptr(X), ptr(rank2), F, D, A, A, stream_ptr())
    return rank2


def cs_rank(X, method="average", present=None, out=None):
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    _check_present(present, D, A)
    if method not in RANK:
        raise ValueError(f"unknown rank method {method!r}")
    Y = _out(X, out)
    if (method in ("first", "dense") and A > BITONIC_RANK_MAX_A) or A > FINE_RANK_MAX_A:
        # rows past the LDS bitonic kernel (first / dense) or the fine-bucket kernels (the
        # other methods): sorted in HBM (fmx_cs_rank_sorted)
        nb = int(_lib.load().fmx_cs_rank_sorted_work_bytes(F, D, A))
        work, wb = _workspace_bytes(X.device, nb)
        call("fmx_cs_rank_sorted", ptr(X), ptr(Y), F, D, A, A, RANK[method], ptr(present), ptr(work), wb,
             stream_ptr())
        return Y
    call("fmx_cs_rank", ptr(X), ptr(Y), F, D, A, A, RANK[method], ptr(present), stream_ptr())
    return Y


def cs_quantile_op(kind: str, X, qlo: float, qhi: float, present=None, out=None):
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    _check_present(present, D, A)
    Y = _out(X, out)
    if A > FINE_RANK_MAX_A:
        # past the fine-bucket quantile kernels: order statistics of rows sorted in HBM
        nb = int(_lib.load().fmx_cs_rank_sorted_work_bytes(F, D, A))
        work, wb = _workspace_bytes(X.device, nb)
        call("fmx_cs_quantile_sorted", 0 if kind == "winsor" else 1, ptr(X), ptr(Y), F, D, A, A, float(qlo),
             float(qhi), ptr(present), ptr(work), wb, stream_ptr())
        return Y
    fn = "fmx_cs_winsor" if kind == "winsor" else "fmx_cs_filter_center"
    call(fn, ptr(X), ptr(Y), F, D, A, A, float(qlo), float(qhi), ptr(present), stream_ptr())
    return Y


def group_op(op: str, X, G, ngroups: int, method="average", present=None, long_rows=None):
    """Group ops (operations.py:104-168).  Rows past 16,384 assets (or ``long_rows=True``):
    rank from rows sorted by (group, value) in HBM, mean / neutralize / normalize with the
    members compacted in HBM scratch (fmx_group_op_long).  ``G`` [D][A] int32 is shared by
    every factor; an absent cell or a code outside [0, ngroups) belongs to no group and
    yields NaN on every path."""
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    _check_present(present, D, A)
    if G.dtype != torch.int32 or tuple(G.shape) != (D, A):
        raise _lib.FmxError("G must be int32 [D][A]")
    if op == "rank" and A > 4096:
        big = A > FINE_RANK_MAX_A
        if not big and ngroups > 0:
            # codes outside [0, ngroups) belong to no group; clamp the index so the count
            # never writes out of bounds (ngroups = 0: no group at all, nothing to count)
            ok = (G >= 0) & (G < ngroups)
            if present is not None:
                ok &= present != 0
            cnt = torch.zeros((D, ngroups), dtype=torch.int32, device=G.device)
            cnt.scatter_add_(1, G.clamp(0, ngroups - 1).long(), ok.int())
            big = int(cnt.max()) > 8192          # the per-group LDS sort takes <= 8192 members
        if big:
            # rows sorted by (group, value) in HBM (fmx_group_rank_sorted): any group size
            Y = torch.empty_like(X)
            nb = int(_lib.load().fmx_group_rank_sorted_work_bytes(F, D, A))
            work, wb = _workspace_bytes(X.device, nb)
            call("fmx_group_rank_sorted", ptr(X), ptr(G), ptr(Y), F, D, A, A, int(ngroups), RANK[method],
                 ptr(present), ptr(work), wb, stream_ptr())
            return Y
    elif op != "rank" and (long_rows or (long_rows is None and A > FINE_RANK_MAX_A)):
        Y = torch.empty_like(X)
        nb = int(_lib.load().fmx_group_op_long_work_bytes(F, D, A))
        work, wb = _workspace_bytes(X.device, nb)
        call("fmx_group_op_long", GROUP[op], ptr(X), ptr(G), ptr(Y), F, D, A, A, int(ngroups), ptr(present),
             ptr(work), wb, stream_ptr())
        return Y
    Y = torch.empty_like(X)
    call("fmx_group_op", GROUP[op], ptr(X), ptr(G), ptr(Y), F, D, A, A, int(ngroups), RANK[method], ptr(present),
         stream_ptr())
    return Y


def cs_regression(Yv, Xv, rettype: str, present=None):
    D, A = Yv.shape
    if tuple(Xv.shape) != (D, A):
        raise _lib.FmxError("cs_regression: shape mismatch")
    _check_present(present, D, A)
    out = torch.empty_like(Yv)
    call("fmx_cs_regression", ptr(Yv), ptr(Xv), ptr(out), D, A, A, CSREG[rettype], ptr(present), stream_ptr())
    return out


CS_OLS_MAX_K = 32           # fmx_cs_ols: the factor is a 33 x 33 matrix in LDS
CS_OLS_MAX_A = 16384        # the row kernels' cap (uint16 positions)
CS_OLS_OUTPUTS = ("beta", "alpha", "r2", "n", "resid", "fitted")


def cs_ols(Y, X, W=None, present=None, intercept=True, want=CS_OLS_OUTPUTS):
    """Per-date multi-factor OLS (fmx_cs_ols): every column of ``Y`` [Fy][D][A]
    (or [D][A]) regressed per date on the K columns of ``X`` [K][D][A] over the valid rows,
    optionally weighted by ``W`` [D][A].  Returns a dict of device tensors for the names in
    ``want``: beta [Fy][D][K], alpha / r2 [Fy][D], n [Fy][D] int32, resid / fitted
    [Fy][D][A].  Collinear columns are dropped in column order (beta NaN)."""
    Y = as3(Y)
    _check_panel(Y, "Y")
    _check_panel(X, "X")
    Fy, D, A = Y.shape
    K = X.shape[0]
    if tuple(X.shape[1:]) != (D, A):
        raise _lib.FmxError(f"cs_ols: X is {tuple(X.shape)}, expected [K][{D}][{A}] to match Y")
    if W is not None:
        if (not isinstance(W, torch.Tensor) or W.device.type != "cuda" or W.dtype != F64
                or tuple(W.shape) != (D, A) or not W.is_contiguous()):
            raise _lib.FmxError(f"cs_ols: W must be a contiguous float64 [{D}][{A}] device tensor")
    _check_present(present, D, A)
    if not 1 <= K <= CS_OLS_MAX_K:
        raise _lib.FmxError(f"cs_ols: K = {K} regressors; the kernel takes 1..{CS_OLS_MAX_K}")
    if A > CS_OLS_MAX_A:
        raise _lib.FmxError(f"cs_ols: A = {A} assets; the kernel takes rows up to {CS_OLS_MAX_A}")
    bad = set(want) - set(CS_OLS_OUTPUTS)
    if bad:
        raise ValueError(f"cs_ols: unknown outputs {sorted(bad)}")
    dev = Y.device
    shapes = dict(beta=(Fy, D, K), alpha=(Fy, D), r2=(Fy, D), n=(Fy, D), resid=(Fy, D, A), fitted=(Fy, D, A))
    out = {k: torch.empty(shapes[k], dtype=torch.int32 if k == "n" else F64, device=dev) for k in want}
    call("fmx_cs_ols", ptr(Y), ptr(X), ptr(W), ptr(present), Fy, K, D, A, A, int(bool(intercept)),
         *(ptr(out.get(k)) for k in CS_OLS_OUTPUTS), stream_ptr())
    return out


def elementwise(op: str, X, a=0.0, b=0.0):
    X = X.contiguous()
    Y = torch.empty_like(X)
    call("fmx_elementwise", EW[op], ptr(X), ptr(Y), X.numel(), float(a), float(b), stream_ptr())
    return Y


def bucket_codes(X, edges: np.ndarray):
    X = X.contiguous()
    e = torch.as_tensor(np.asarray(edges, dtype=np.float64), device=X.device)
    codes = torch.empty(X.shape, dtype=torch.int32, device=X.device)
    call("fmx_bucket", ptr(X), ptr(codes), X.numel(), ptr(e), len(edges), stream_ptr())
    return codes


# ----------------------------------------------------------------------------- IC / selection
def ic_daily(X, R, lags=(1,), rank2=None, sorted_rows=None):
    """[n_lags][4][F][D] = (n_pairs, IC, rank_IC, beta) for pairs (X[f][t-L], R[t]).
    ``rank2``: the doubled ranks of X from ``cs_rank_winsor(X, rank2=...)`` -- the rows
    are then not ranked again (fmx_ic_daily_ranked, identical records).  Rows past 16,384
    assets (or ``sorted_rows=True``) are sorted in HBM (fmx_ic_daily_sorted)."""
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    if tuple(R.shape) != (D, A) or R.dtype != F64 or not R.is_contiguous():
        raise _lib.FmxError("R must be a contiguous float64 [D][A] device tensor")
    lag_h = (ctypes.c_int32 * len(lags))(*[int(v) for v in lags])
    out = torch.empty((len(lags), 4, F, D), dtype=F64, device=X.device)
    if rank2 is not None:
        if rank2.dtype != RANK2_DTYPE or tuple(rank2.shape) != (F, D, A) or not rank2.is_contiguous():
            raise _lib.FmxError("rank2 must be a contiguous int16 [F][D][A] tensor")
        n = int(_lib.load().fmx_ic_ranked_work_len(F, D))
        work = _workspace(X.device, n)
        call("fmx_ic_daily_ranked", ptr(X), ptr(rank2), ptr(R), F, D, A, A, ctypes.cast(lag_h, ctypes.c_void_p),
             len(lags), ptr(work), n, ptr(out), stream_ptr())
        return out
    if sorted_rows or (sorted_rows is None and A > RANKED_IC_MAX_A):
        # rows past the fine / LDS kernels: sorted in HBM, ranks read off the sorted rows
        nb = int(_lib.load().fmx_ic_daily_sorted_work_bytes(F, D, A))
        work, wb = _workspace_bytes(X.device, nb)
        call("fmx_ic_daily_sorted", ptr(X), ptr(R), F, D, A, A, ctypes.cast(lag_h, ctypes.c_void_p), len(lags),
             ptr(out), ptr(work), wb, stream_ptr())
        return out
    call("fmx_ic_daily", ptr(X), ptr(R), F, D, A, A, ctypes.cast(lag_h, ctypes.c_void_p), len(lags), ptr(out),
         stream_ptr())
    return out


def ic_window(daily, d0, d1):
    """daily [4][F][D]; windows [d0[j], d1[j]) -> [J][F][8]."""
    _, F, D = daily.shape
    daily = daily.contiguous()
    d0t = torch.as_tensor(np.asarray(d0, dtype=np.int32), device=daily.device)
    d1t = torch.as_tensor(np.asarray(d1, dtype=np.int32), device=daily.device)
    J = len(d0t)
    out = torch.empty((J, F, 8), dtype=F64, device=daily.device)
    call("fmx_ic_window", ptr(daily), F, D, ptr(d0t), ptr(d1t), J, ptr(out), stream_ptr())
    return out


def select_icir_top(metrics, use_rank_icir=True, threshold=0.03, top_x=5):
    J, F, _ = metrics.shape
    metrics = metrics.contiguous()
    order = torch.empty((J, F), dtype=torch.int32, device=metrics.device)
    w = torch.empty((J, F), dtype=F64, device=metrics.device)
    call("fmx_select_icir_top", ptr(metrics), J, F, int(bool(use_rank_icir)), float(threshold), int(top_x),
         ptr(order), ptr(w), stream_ptr())
    return order, w


MVO_MAX_F = 256


def _mvo_inputs(fret, d0, d1):
    if not isinstance(fret, torch.Tensor) or fret.device.type != "cuda" or fret.dtype != F64 or fret.dim() != 2:
        raise _lib.FmxError("mvo: fret must be a float64 [D][F] HIP device tensor")
    D, F = fret.shape
    if not 2 <= F <= MVO_MAX_F:
        raise _lib.FmxError(f"mvo: 2 <= F <= {MVO_MAX_F} factors supported, got {F}")
    d0t = torch.as_tensor(np.asarray(d0, dtype=np.int32), device=fret.device)
    d1t = torch.as_tensor(np.asarray(d1, dtype=np.int32), device=fret.device)
    if d0t.dim() != 1 or d0t.shape != d1t.shape:
        raise _lib.FmxError("mvo: d0 and d1 must be 1-D and of equal length")
    return fret.contiguous(), int(D), int(F), d0t, d1t, len(d0t)


def mvo_covariance(fret, d0, d1, use_shrinkage=True):
    """Per-window moments of the factor returns fret [D][F] over the rows [d0[j], d1[j])
    (fmx_mvo_covariance): mu [J][F], cov [J][F][F] (Ledoit-Wolf constant-correlation shrunk,
    or the ddof=1 sample covariance), lam [J].  Rejected windows (n < 2, NaN / inf) are NaN."""
    fret, D, F, d0t, d1t, J = _mvo_inputs(fret, d0, d1)
    mu = torch.empty((J, F), dtype=F64, device=fret.device)
    cov = torch.empty((J, F, F), dtype=F64, device=fret.device)
    lam = torch.empty((J,), dtype=F64, device=fret.device)
    call("fmx_mvo_covariance", ptr(fret), D, F, ptr(d0t), ptr(d1t), J, int(bool(use_shrinkage)), ptr(mu), ptr(cov),
         ptr(lam), stream_ptr())
    return mu, cov, lam


def mvo_windows(fret, d0, d1, risk_aversion=1.0, max_weight=1.0, turnover_penalty=0.0, prev=None, use_shrinkage=True,
                max_iter=20000, eps=1e-9):
    """mvo_selector's QP for every window at once (fmx_mvo_windows): w [J][F] and info [J][6]
    = status (0 converged, 1 max_iter reached, 2 no solution: window rejected or
    F * max_weight < 1; zero row), iterations, primal residual, dual residual, lambda, rho.
    prev: [F] previous weights (device or host) or None."""
    fret, D, F, d0t, d1t, J = _mvo_inputs(fret, d0, d1)
    if prev is not None:
        prev = torch.as_tensor(prev, dtype=F64).to(fret.device).contiguous()
        if tuple(prev.shape) != (F,):
            raise _lib.FmxError("mvo_windows: prev must hold one weight per factor")
    w = torch.empty((J, F), dtype=F64, device=fret.device)
    info = torch.empty((J, 6), dtype=F64, device=fret.device)
    nb = int(_lib.load().fmx_mvo_windows_work_bytes(D, F, J))
    work, wb = _workspace_bytes(fret.device, nb)
    call("fmx_mvo_windows", ptr(fret), D, F, ptr(d0t), ptr(d1t), J, float(risk_aversion), float(max_weight),
         float(turnover_penalty), ptr(prev), int(bool(use_shrinkage)), int(max_iter), float(eps), ptr(w), ptr(info),
         ptr(work), wb, stream_ptr())
    return w, info


def zscore_exposures(X, stats=None):
    """Z (per-date z-score, NaN -> 0, sigma in {0, NaN} -> row 0) and M (bf16 0/1) from
    the numpy-pairwise row moments of cs_moment_stats (the oracle's, bit for bit)."""
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    if stats is None:
        _, stats = cs_moment_stats("stats", X)
    Z = torch.empty_like(X)
    M = torch.empty(X.shape, dtype=torch.bfloat16, device=X.device)   # 0/1 validity
    call("fmx_zscore_exposures", ptr(X), ptr(stats), ptr(Z), ptr(M), F, D, A, A, stream_ptr())
    return Z, M


def gram(Z, M=None, d0=0, d1=None):
    F, D, A = Z.shape
    d1 = D if d1 is None else d1
    G = torch.empty((F, F), dtype=F64, device=Z.device)
    N = torch.empty((F, F), dtype=F64, device=Z.device) if M is not None else None
    nb = int(_lib.load().fmx_gram_work_bytes(F, D, A, int(d0), int(d1), int(M is not None)))
    work, wb = _workspace_bytes(Z.device, nb)
    call("fmx_gram", ptr(Z), ptr(M), ptr(G), ptr(N), F, D, A, A, int(d0), int(d1), 0, ptr(work), wb, stream_ptr())
    return G, N


FUSED_GRAM_MAX_F = 256
GRAM_EXACT_SLOTS = 7            # fmx.h FMX_GRAM_EXACT_SLOTS: 6 payload limbs + flag


def _check_stats(stats, F, D):
    """Row stats given by the caller (None: the callee computes or does not need them)."""
    if stats is not None and (tuple(stats.shape) != (F, D, 2) or stats.dtype != F64 or not stats.is_contiguous()):
        raise _lib.FmxError("stats must be a contiguous float64 [F][D][2] device tensor")


def _exact_outputs(limbs, counts, n, device, msg):
    """The exact Gram's (limbs int64 [7][n][n], counts int64 [n][n]): allocated where None,
    else validated (``msg`` on a mismatch)."""
    if limbs is None:
        limbs = torch.empty((GRAM_EXACT_SLOTS, n, n), dtype=torch.int64, device=device)
    if counts is None:
        counts = torch.empty((n, n), dtype=torch.int64, device=device)
    if tuple(limbs.shape) != (GRAM_EXACT_SLOTS, n, n) or limbs.dtype != torch.int64 or not limbs.is_contiguous() \
            or tuple(counts.shape) != (n, n) or counts.dtype != torch.int64 or not counts.is_contiguous():
        raise _lib.FmxError(msg)
    return limbs, counts


def gram_fused(X, stats, d0=0, d1=None):
    """G, N straight from the raw panel with row stats (F <= 256): one pass over X.
    ``stats=None``: X already holds the z-scores (the cs_zscore output of the rows)."""
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    _check_stats(stats, F, D)
    d1 = D if d1 is None else d1
    G = torch.empty((F, F), dtype=F64, device=X.device)
    N = torch.empty((F, F), dtype=F64, device=X.device)
    nb = int(_lib.load().fmx_gram_fused_work_bytes(F, D, A, int(d0), int(d1)))
    work, wb = _workspace_bytes(X.device, nb)
    call("fmx_gram_fused", ptr(X), ptr(stats), ptr(G), ptr(N), F, D, A, A, int(d0), int(d1), 0, ptr(work), wb,
         stream_ptr())
    return G, N


def gram_exact(X, stats=None, d0=0, d1=None, limbs=None, counts=None, accumulate=False):
    """Exact fixed-point Gram partials over dates [d0, d1) (fmx_gram_exact, F <= 256):
    (limbs int64 [7][F][F], counts int64 [F][F]), upper triangles.  Integer sums: ranks
    add them with any all-reduce and gram_exact_finalize gives the same G / N bits at every
    GPU count.  ``stats=None``: X holds the z-scores (the step's cs_zscore output)."""
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    if F > FUSED_GRAM_MAX_F:
        raise _lib.FmxError("gram_exact: F <= 256")
    _check_stats(stats, F, D)
    d1 = D if d1 is None else d1
    limbs, counts = _exact_outputs(limbs, counts, F, X.device, "gram_exact: limbs int64 [7][F][F], counts int64 [F][F]")
    nb = int(_lib.load().fmx_gram_exact_work_bytes(F, D, A, int(d0), int(d1)))
    work, wb = _workspace_bytes(X.device, nb)
    call("fmx_gram_exact", ptr(X), ptr(stats), ptr(limbs), ptr(counts), F, D, A, A, int(d0), int(d1),
         int(bool(accumulate)), ptr(work), wb, stream_ptr())
    return limbs, counts


def gram_exact_finalize(limbs, counts):
    """G, N [F][F] float64 (symmetric) from (all-reduced) exact limbs / counts."""
    F = limbs.shape[1]
    G = torch.empty((F, F), dtype=F64, device=limbs.device)
    N = torch.empty((F, F), dtype=F64, device=limbs.device)
    call("fmx_gram_exact_finalize", ptr(limbs.contiguous()), ptr(counts.contiguous()), ptr(G), ptr(N), F,
         stream_ptr())
    return G, N


GRAM_HEAD_MAX = 64              # fmx_gram_exact_rows / fmx_prune_head: rows of a head block


def gram_exact_rows(Z, rows, d0=0, d1=None, limbs=None, counts=None, accumulate=False):
    """gram_exact of the z-score panel ``Z`` restricted to the rows the device index list
    ``rows`` (int64 [H], H <= 64) names, read in place (fmx_gram_exact_rows): (limbs int64
    [7][H][H], counts int64 [H][H]) by position in the list, each entry the bits gram_exact
    gives that factor pair.  An index outside [0, F) is an all-invalid row.  The host never
    reads ``rows``: no sync."""
    Z = as3(Z)
    _check_panel(Z)
    F, D, A = Z.shape
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int64 or rows.dim() != 1 or rows.device != Z.device \
            or not rows.is_contiguous():
        raise _lib.FmxError("gram_exact_rows: rows must be a contiguous int64 [H] tensor on the panel's device")
    H = int(rows.numel())
    if not 1 <= H <= GRAM_HEAD_MAX:
        raise _lib.FmxError(f"gram_exact_rows: 1 <= H <= {GRAM_HEAD_MAX}")
    d1 = D if d1 is None else d1
    limbs, counts = _exact_outputs(limbs, counts, H, Z.device,
                                   "gram_exact_rows: limbs int64 [7][H][H], counts int64 [H][H]")
    nb = int(_lib.load().fmx_gram_exact_rows_work_bytes(H, D, A, int(d0), int(d1)))
    work, wb = _workspace_bytes(Z.device, nb)
    call("fmx_gram_exact_rows", ptr(Z), ptr(rows), H, ptr(limbs), ptr(counts), F, D, A, A, int(d0), int(d1),
         int(bool(accumulate)), ptr(work), wb, stream_ptr())
    return limbs, counts


def prune_head(limbs, counts, order, F, rho=0.7, top_x=5):
    """The greedy prune from the (all-reduced) head block of gram_exact_rows(Z, order[:H])
    (fmx_prune_head: finalize + walk in one launch, one host read).  Returns (kept factor
    list, done); ``done``: the walk of the whole order over the full correlation matrix
    returns the same list (top_x kept inside the head, or the head is the whole order) --
    else ``kept`` is only its prefix."""
    H = int(limbs.shape[1])
    msg = "prune_head: limbs int64 [7][H][H], counts int64 [H][H], H <= 64"
    _exact_outputs(limbs, counts, H, limbs.device, msg)
    if counts is None or not 1 <= H <= GRAM_HEAD_MAX:
        raise _lib.FmxError(msg)
    ordt = order.to(device=limbs.device, dtype=torch.int64).contiguous()
    lim = max(int(top_x), 1)                        # as greedy_prune: top_x <= 0 keeps one
    cap = min(lim, H)
    out = torch.empty(cap + 2, dtype=torch.int32, device=limbs.device)     # kept | n_kept | done
    call("fmx_prune_head", ptr(limbs), ptr(counts), ptr(ordt), H, int(ordt.numel()), int(F), float(rho), lim,
         ptr(out), ptr(out[cap:]), ptr(out[cap + 1:]), stream_ptr())
    res = out.cpu().tolist()
    return [int(v) for v in res[:res[cap]]], bool(res[cap + 1])


GRAM_CHUNK_BYTES = 8 << 30     # Z + M workspace of one date chunk of the wide Gram


def gram_chunked(X, d0=0, d1=None, chunk=None):
    """G, N over dates [d0, d1) for wide factor sets (F > 256, e.g. C4's 2000): Z / M are
    materialised one date chunk at a time (fmx_zscore_exposures_range, <= GRAM_CHUNK_BYTES)
    and accumulated into G / N by the tiled fp64 / bf16 MFMA kernels in chunk order
    (deterministic), so the panel never needs a full-size Z next to it."""
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    d1 = D if d1 is None else d1
    if chunk is None:
        chunk = max(1, min(d1 - d0, int(GRAM_CHUNK_BYTES // max(1, F * A * 10))))
    _, stats = cs_moment_stats("stats", X)
    G = torch.zeros((F, F), dtype=F64, device=X.device)
    N = torch.zeros((F, F), dtype=F64, device=X.device)
    Z = M = None
    for c0 in range(d0, d1, chunk):
        c1 = min(d1, c0 + chunk)
        n = c1 - c0
        if Z is None or Z.shape[1] != n:
            Z = torch.empty((F, n, A), dtype=F64, device=X.device)
            M = torch.empty((F, n, A), dtype=torch.bfloat16, device=X.device)
        call("fmx_zscore_exposures_range", ptr(X), ptr(stats), ptr(Z), ptr(M), F, D, A, A, c0, c1, stream_ptr())
        nb = int(_lib.load().fmx_gram_work_bytes(F, n, A, 0, n, 1))
        work, wb = _workspace_bytes(X.device, nb)
        call("fmx_gram", ptr(Z), ptr(M), ptr(G), ptr(N), F, n, A, A, 0, n, 1, ptr(work), wb, stream_ptr())
    return G, N


def gram_direct(X, d0=0, d1=None, stats=None):
    """G, N over dates [d0, d1) for wide factor sets (F > 256, C4's 2000) straight from
    the panel (fmx_gram_direct): the z-score (row stats of fmx_cs_moment_stats, computed
    here unless given) is applied while each tile chunk is staged and N comes from the
    validity bits on the i8 matrix cores -- no Z / M panels in HBM."""
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    d1 = D if d1 is None else d1
    _check_stats(stats, F, D)
    if stats is None:
        _, stats = cs_moment_stats("stats", X)
    G = torch.empty((F, F), dtype=F64, device=X.device)
    N = torch.empty((F, F), dtype=F64, device=X.device)
    nb = int(_lib.load().fmx_gram_direct_work_bytes(F, D, A, int(d0), int(d1)))
    work, wb = _workspace_bytes(X.device, nb)
    call("fmx_gram_direct", ptr(X), ptr(stats), ptr(G), ptr(N), F, D, A, A, int(d0), int(d1), 0, ptr(work), wb,
         stream_ptr())
    return G, N


GRAM_DATE_BLOCK = 16            # fmx.h FMX_GRAM_DATE_BLOCK: date shards align to it (wide Gram)


def gram_direct_exact(X, d0=0, d1=None, d_origin=0, stats=None, limbs=None, counts=None, accumulate=False):
    """Exact fixed-point partials of the wide Gram over dates [d0, d1) (fmx_gram_direct_exact,
    any F): (limbs int64 [7][F][F], counts int64 [F][F]).  Slices are absolute blocks of
    GRAM_DATE_BLOCK dates (local row 0 = absolute date ``d_origin``), so shards aligned to
    the block sum (int64 all-reduce) to the same bits at any GPU count; gram_exact_finalize
    gives G, N."""
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    d1 = D if d1 is None else d1
    # stats None: the kernel's z pass (or, past its row size, its own stats pass) computes the moments
    _check_stats(stats, F, D)
    limbs, counts = _exact_outputs(limbs, counts, F, X.device,
                                   "gram_direct_exact: limbs int64 [7][F][F], counts int64 [F][F]")
    nb = int(_lib.load().fmx_gram_direct_exact_work_bytes(F, D, A, int(d0), int(d1), int(d_origin)))
    work, wb = _workspace_bytes(X.device, nb)
    call("fmx_gram_direct_exact", ptr(X), ptr(stats), ptr(limbs), ptr(counts), F, D, A, A, int(d0), int(d1),
         int(d_origin), int(bool(accumulate)), ptr(work), wb, stream_ptr())
    return limbs, counts


def corr_matrix(X, d0=0, d1=None, stats=None):
    """Builder-defined factor correlation: C = G / N on fp64 MFMA.  F <= 256
    takes the fused path (row stats from cs_moment, one pass over X); wider panels take
    the direct tile kernel (gram_direct), also straight from the panel."""
    X = as3(X)
    if X.shape[0] <= FUSED_GRAM_MAX_F:
        if stats is None:
            _, stats = cs_moment_stats("stats", X)
        G, N = gram_fused(X, stats, d0, d1)
    else:
        G, N = gram_direct(X, d0, d1)
    return torch.where(N > 0, G / N.clamp_min(1.0), torch.zeros_like(G))


def corr_prune_windows(X, stats, metrics, order, window: int, s0, use_rank_icir=True, threshold=-np.inf, rho=0.7,
                       top_x=5):
    """Rolling corr_prune selection on the device (fmx_corr_prune_windows): weights [J][F]."""
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    J = metrics.shape[0]
    if tuple(metrics.shape) != (J, F, 8) or tuple(order.shape) != (J, F) or order.dtype != torch.int32:
        raise _lib.FmxError("corr_prune_windows: metrics [J][F][8] and int32 order [J][F] expected")
    s0h = (ctypes.c_int32 * J)(*[int(v) for v in s0])
    w = torch.empty((J, F), dtype=F64, device=X.device)
    top = F if top_x is None else int(top_x)
    s0p = ctypes.cast(s0h, ctypes.c_void_p)
    nb = int(_lib.load().fmx_corr_prune_windows_work_bytes(F, D, J, int(window), s0p))
    work, wb = _workspace_bytes(X.device, nb)
    call("fmx_corr_prune_windows", ptr(X), ptr(stats.contiguous()), F, D, A, A, J, int(window), s0p,
         ptr(order.contiguous()), ptr(metrics.contiguous()), int(bool(use_rank_icir)), float(threshold), float(rho),
         top, ptr(w), ptr(work), wb, stream_ptr())
    return w


def _greedy_prune_device(C, order, rho, top_x):
    if C.dim() != 2 or C.shape[0] != C.shape[1] or C.dtype != F64:
        raise _lib.FmxError("greedy_prune: C must be a square float64 matrix")
    C = C.contiguous()
    F = C.shape[0]
    if isinstance(order, torch.Tensor):
        ordt = order.to(device=C.device, dtype=torch.int64).contiguous()
    else:
        ordt = torch.as_tensor(np.asarray(order, dtype=np.int64), device=C.device)
    # the host walk returns once len(kept) >= top_x after an append: top_x <= 0 keeps one
    lim = F if top_x is None else max(int(top_x), 1)
    # the walk appends at most one entry per element of ``order`` (a repeated index can be kept
    # twice, as in the host walk): the bound handed to the kernel is also the buffer's capacity
    lim = min(lim, max(int(ordt.numel()), 1))
    kept = torch.empty(lim, dtype=torch.int32, device=C.device)
    nk = torch.zeros(1, dtype=torch.int32, device=C.device)
    call("fmx_greedy_prune", ptr(C), F, F, ptr(ordt), int(ordt.numel()), float(rho), lim, ptr(kept), ptr(nk),
         stream_ptr())
    n = int(nk.item())
    return [int(v) for v in kept[:n].cpu().tolist()]


def greedy_prune(C, order, rho=0.7, top_x=None):
    """Walk ``order``; keep f iff max |C[f, kept]| < rho (NaN: kept).  A device C runs the
    walk on the GPU (fmx_greedy_prune: no F x F copy to the host); a host C the numpy walk."""
    if isinstance(C, torch.Tensor) and C.is_cuda:
        return _greedy_prune_device(C, order, rho, top_x)
    Cn = C.detach().cpu().numpy() if isinstance(C, torch.Tensor) else np.asarray(C)
    # f is kept iff max_k |C[f, k]| over the kept k is < rho or NaN (np.max propagates NaN
    # and NaN >= rho is False).  Blocks of candidates: mx[g] = that max over the kept
    # columns of earlier blocks (np.maximum propagates NaN too); inside a block the walk is
    # sequential on the block's own |C| sub-matrix; then mx absorbs the block's kept columns.
    mx = np.full(Cn.shape[0], -np.inf)
    order = np.asarray(order, dtype=np.int64)
    kept = []
    B = 64
    for b0 in range(0, order.size, B):
        cand = order[b0:b0 + B]
        prior = mx[cand]
        sub = np.abs(Cn[np.ix_(cand, cand)])
        kin = []
        bm = np.full(cand.size, -np.inf)     # max over this block's kept columns so far
        for i in range(cand.size):
            p, m = prior[i], bm[i]
            if p == p and m == m and max(p, m) >= rho:
                continue                     # (a NaN among the kept columns keeps it)
            np.maximum(bm, sub[:, i], out=bm)
            kin.append(i)
            kept.append(int(cand[i]))
            if top_x is not None and len(kept) >= top_x:
                return kept
        if not kin:
            continue
        np.maximum(mx, np.abs(Cn[:, cand[kin]]).max(axis=1), out=mx)
    return kept


def device_info():
    buf = ctypes.create_string_buffer(256)
    call("fmx_device_info", buf, 256)
    return buf.value.decode()


# ----------------------------------------------------------------------------- composites
SUFFIXES = ["_eq", "_flx", "_long", "_short"]          # codes 1..4 (composite_factor.py:158-163)
_QLO = np.array([0, 10, 2, 2, 2], dtype=np.float64)
_QHI = np.array([0, 90, 98, 98, 98], dtype=np.float64)


def suffix_code(name: str) -> int:
    """composite_factor.py applies the suffix rules in this order; first match wins."""
    for k, s in enumerate(SUFFIXES):
        if name.endswith(s):
            return k + 1
    return 0


def _qfrac(dev):
    # np.nanpercentile(clean, [q_low, q_high]) divides integer percents by 100
    lo = torch.as_tensor(np.true_divide(_QLO, 100), device=dev)
    hi = torch.as_tensor(np.true_divide(_QHI, 100), device=dev)
    return lo, hi


def _i32(a, dev):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.int32)), device=dev)


def comp_adj(X, cols, suffix_codes):
    _check_panel(X)
    F, D, A = X.shape
    K = len(cols)
    dev = X.device
    lo, hi = _qfrac(dev)
    c, s = _i32(cols, dev), _i32(suffix_codes, dev)
    Adj = torch.empty((K, D, A), dtype=F64, device=dev)
    call("fmx_comp_adj", ptr(X), ptr(c), ptr(s), ptr(lo), ptr(hi), ptr(Adj), K, D, A, stream_ptr())
    return Adj


def comp_proxy(Adj, groups):
    """groups: list of column-index lists into Adj."""
    K, D, A = Adj.shape
    dev = Adj.device
    gcols = _i32([c for g in groups for c in g], dev)
    goff = _i32(np.concatenate([[0], np.cumsum([len(g) for g in groups])]), dev)
    G = len(groups)
    P = torch.empty((G, D, A), dtype=F64, device=dev)
    call("fmx_comp_proxy", ptr(Adj), ptr(gcols), ptr(goff), ptr(P), G, D, A, stream_ptr())
    return P


def comp_combine(Nrm, mode, present=None):
    G, D, A = Nrm.shape
    out = torch.empty((D, A), dtype=F64, device=Nrm.device)
    call("fmx_comp_combine", ptr(Nrm), G, D, A, int(mode), ptr(present), ptr(out), stream_ptr())
    return out


def wcomp(X, plan, method, present=None):
    """weighted_composite_factor device stages for a host-built ``plan`` (see
    composite_factor._weighted_plan).  Returns the [D][A] composite (0 where unselected)."""
    _check_panel(X)
    F, D, A = X.shape
    dev = X.device
    J = len(plan["pdate"])
    out = torch.zeros((D, A), dtype=F64, device=dev)
    if J == 0:
        return out
    KMAX = plan["KMAX"]
    pdate, ncol = _i32(plan["pdate"], dev), _i32(plan["ncol"], dev)
    col, suf, grp = _i32(plan["col"], dev), _i32(plan["suf"], dev), _i32(plan["grp"], dev)
    soff, scol = _i32(plan["soff"], dev), _i32(plan["scol"], dev)
    ngrp = _i32(plan["ngrp"], dev)
    gw = torch.as_tensor(plan["gw"], device=dev)
    lo, hi = _qfrac(dev)
    lohi = torch.empty((J, 4, 3), dtype=F64, device=dev)
    call("fmx_wcomp_pct", ptr(X), ptr(pdate), ptr(soff), ptr(scol), J, D, A, ptr(lo), ptr(hi), ptr(lohi),
         stream_ptr())
    G = max(1, int(plan["ngrp"].max()))
    P = torch.empty((G, J, A), dtype=F64, device=dev)
    call("fmx_wcomp_proxy", ptr(X), ptr(pdate), ptr(ncol), ptr(col), ptr(suf), ptr(grp), KMAX, J, D, A, ptr(lohi), G,
         ptr(P), stream_ptr())
    presJ = None
    if present is not None:
        pd_idx = torch.as_tensor(np.maximum(plan["pdate"], 0), device=dev, dtype=torch.long)
        presJ = present[pd_idx].contiguous()
        P.masked_fill_(presJ.unsqueeze(0) == 0, float("nan"))
    if method == "zscore":
        Nrm = cs_moment("market_neutralize", P, presJ)
    else:
        Nrm = cs_rank(P, "scipy_average", presJ)
    call("fmx_wcomp_combine", ptr(Nrm), ptr(pdate), ptr(ngrp), ptr(gw), KMAX, J, D, A, ptr(present), ptr(out),
         stream_ptr())
    return out


# ----------------------------------------------------------------------------- trade list
def trade_equal(X, pct: float, present=None):
    """Simulation._daily_trade_list, method 'equal' (portfolio_simulation.py:96-170) on one
    [D][A] signal panel: (per-symbol shift(1) of the day's weights [D][A], counts [D][2])."""
    if X.dim() != 2 or X.dtype != F64 or not X.is_cuda:
        raise _lib.FmxError("X must be a float64 [D][A] device tensor")
    X = X.contiguous()
    D, A = X.shape
    _check_present(present, D, A)
    Wraw = torch.empty_like(X)
    Wout = torch.empty_like(X)
    counts = torch.empty((D, 2), dtype=F64, device=X.device)
    call("fmx_trade_equal", ptr(X), ptr(present), ptr(Wraw), ptr(Wout), ptr(counts), D, A, float(pct),
         stream_ptr())
    return Wout, counts


def trade_linear(X, max_weight: float, present=None):
    """Simulation._daily_trade_list, method 'linear' (portfolio_simulation.py:172-181,
    :250-313) on one [D][A] panel: (shifted weights [D][A], counts [D][2])."""
    if X.dim() != 2 or X.dtype != F64 or not X.is_cuda:
        raise _lib.FmxError("X must be a float64 [D][A] device tensor")
    X = X.contiguous()
    D, A = X.shape
    _check_present(present, D, A)
    Wraw, Wout = torch.empty_like(X), torch.empty_like(X)
    counts = torch.empty((D, 2), dtype=F64, device=X.device)
    call("fmx_trade_linear", ptr(X), ptr(present), ptr(Wraw), ptr(Wout), ptr(counts), D, A, float(max_weight),
         stream_ptr())
    return Wout, counts


TRADE_METHODS = {"equal": 0, "linear": 1}


def trade_books(X, method: str, pct=0.1, max_weight=0.03, present=None, nan_absent=True, raw=False):
    """F trade books in one launch (fmx_trade_books): X [F][D][A] -> (shifted [F][D][A],
    counts [F][D][2]) (+ the same-day books with ``raw``); with nan_absent a NaN cell is no row."""
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    _check_present(present, D, A)
    if method not in TRADE_METHODS:
        raise NotImplementedError(f"method {method!r}: the device runs 'equal' and 'linear'")
    Wraw, Wout = torch.empty_like(X), torch.empty_like(X)
    counts = torch.empty((F, D, 2), dtype=F64, device=X.device)
    call("fmx_trade_books", TRADE_METHODS[method], ptr(X), ptr(present), int(bool(nan_absent)), ptr(Wraw),
         ptr(Wout), ptr(counts), F, D, A, float(pct), float(max_weight), stream_ptr())
    return (Wout, counts, Wraw) if raw else (Wout, counts)


def shift_rows(W):
    """Per-symbol shift(1) over each book's present (non-NaN) rows (fmx_shift_rows)."""
    W = as3(W).contiguous()
    F, D, A = W.shape
    out = torch.empty_like(W)
    call("fmx_shift_rows", ptr(W), ptr(out), F, D, A, stream_ptr())
    return out


SIM_MVO_MAX_A = 16384
SIM_MVO_MAX_T = 64


def _is_f64_device(t, dims, device=None):
    """t is a float64 tensor with t.dim() in dims on ``device`` (None: any HIP device)."""
    return (isinstance(t, torch.Tensor) and t.dtype == F64 and t.dim() in dims
            and (t.device.type == "cuda" if device is None else t.device == device))


def _mvo_assets(fn, first, A, XA):
    if XA != A or not 1 <= A <= SIM_MVO_MAX_A:
        raise _lib.FmxError(f"{fn}: {first} and X must share 1 <= A <= {SIM_MVO_MAX_A} asset columns")


def _check_present_chains(present, B, J, A):
    if present is not None:
        if present.dtype != torch.uint8 or tuple(as3(present).shape) != (B, J, A) or not present.is_contiguous():
            raise _lib.FmxError("present must be a contiguous uint8 [B][J][A] device tensor")


def _mvo_windows(fn, win_rows, win_T, device, J, B=None):
    """The window tables as contiguous int32 device tensors, win_rows [J][Lmax] / win_T [J] or,
    when ``B`` is given, also [B][J][Lmax] / [B][J].  Returns (win_rows, win_T, Lmax, shared)."""
    win_rows = torch.as_tensor(win_rows, dtype=torch.int32).to(device).contiguous()
    win_T = torch.as_tensor(win_T, dtype=torch.int32).to(device).contiguous()
    shared = B is None or win_T.dim() == 1
    lead = (J,) if shared else (B, J)
    if win_rows.dim() != len(lead) + 1 or tuple(win_rows.shape[:-1]) != lead or tuple(win_T.shape) != lead:
        raise _lib.FmxError(f"{fn}: win_rows must be [J][Lmax] and win_T [J]" if B is None else
                            f"{fn}: win_rows must be [B][J][Lmax] and win_T [B][J] "
                            "(or [J][Lmax] and [J], shared by the chains)")
    Lmax = int(win_rows.shape[-1])
    if not 1 <= Lmax <= SIM_MVO_MAX_T:
        raise _lib.FmxError(f"{fn}: 1 <= Lmax <= {SIM_MVO_MAX_T} window rows supported, got {Lmax}")
    return win_rows, win_T, Lmax, shared


def _mvo_outputs(lead, lasts, device):
    """One uninitialised float64 tensor lead + (n,) per n in lasts: W (A), counts (2), info (6)."""
    return [torch.empty(tuple(lead) + (n,), dtype=F64, device=device) for n in lasts]


def sim_mvo_books(R0, win_rows, win_T, X, present=None, shrinkage=0.1, max_weight=0.03, max_iter=20000, eps=1e-9):
    """Simulation._daily_trade_list, method 'mvo' (portfolio_simulation.py:183-204, :315-461)
    for J dates in one launch (fmx_sim_mvo_books): R0 [Dr][A] the zero-filled returns panel,
    win_rows [J][Lmax] / win_T [J] int32 each date's window rows of R0, X [J][A] the signal,
    present [J][A] uint8 or None.  Returns (W [J][A] same-day weights: 0 outside the legs, NaN
    on absent cells; counts [J][2]; info [J][6] = status, iterations, primal residual, dual
    residual relative to the leg multipliers, delta, rho).  status 0 converged, 1 max_iter reached, 2 x0 fallback, 3 flat day,
    4 no returns history (the caller supplies the equal-weight book)."""
    for t, name in ((R0, "R0"), (X, "X")):
        if not _is_f64_device(t, (2,)):
            raise _lib.FmxError(f"sim_mvo_books: {name} must be a float64 2-D HIP device tensor")
    R0, X = R0.contiguous(), X.contiguous()
    (Dr, A), J = R0.shape, X.shape[0]
    _mvo_assets("sim_mvo_books", "R0", A, X.shape[1])
    _check_present(present, J, A)
    win_rows, win_T, Lmax, _ = _mvo_windows("sim_mvo_books", win_rows, win_T, X.device, J)
    W, counts, info = _mvo_outputs((J,), (A, 2, 6), X.device)
    nb = int(_lib.load().fmx_sim_mvo_books_work_bytes(A, Lmax, J))
    work, wb = _workspace_bytes(X.device, nb)
    call("fmx_sim_mvo_books", ptr(R0), int(Dr), int(A), ptr(win_rows), ptr(win_T), Lmax, ptr(X), ptr(present), int(J),
         float(shrinkage), float(max_weight), int(max_iter), float(eps), ptr(W), ptr(counts), ptr(info), ptr(work), wb,
         stream_ptr())
    return W, counts, info


RISK_MAX_K = 32             # fmx_risk_books / fmx_risk_mvo_books: the K x K matrices live in LDS (fmx_cs_ols' cap)


def _check_risk_model(fn, B, Fc, S2):
    """(K, D, A) of the factor model's three device arrays B [K][D][A], Fc [D][K][K], S2 [D][A]."""
    for t, name, nd in ((B, "B", 3), (Fc, "Fc", 3), (S2, "S2", 2)):
        if (not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != F64 or t.dim() != nd
                or not t.is_contiguous()):
            raise _lib.FmxError(f"{fn}: {name} must be a contiguous float64 {nd}-D HIP device tensor")
    K, D, A = B.shape
    if not 1 <= K <= RISK_MAX_K:
        raise _lib.FmxError(f"{fn}: K = {K} factors; the kernel takes 1..{RISK_MAX_K}")
    if tuple(Fc.shape) != (D, K, K) or tuple(S2.shape) != (D, A):
        raise _lib.FmxError(f"{fn}: B is {tuple(B.shape)}, so Fc must be [{D}][{K}][{K}] and S2 [{D}][{A}]")
    return K, D, A


def risk_books(B, Fc, S2, W, present=None, valid=None, marginal=False):
    """Predicted risk and attribution of M books under Sigma_d = B_d' F_d B_d + diag(s2_d)
    (fmx_risk_books): B [K][D][A] exposures (NaN: 0), Fc [D][K][K] (lower triangle),
    S2 [D][A], W [M][D][A] (or [D][A]) books (NaN: not held), present [D][A] uint8 or None, valid
    [D] uint8 / bool or None (an invalid date is NaN everywhere).  Returns a dict: var [M][D][3]
    (total, factor, specific), expo [M][D][K], contrib [M][D][K] and, with ``marginal``, marginal
    [M][D][A] = Sigma w (NaN on absent cells)."""
    K, D, A = _check_risk_model("risk_books", B, Fc, S2)
    if not isinstance(W, torch.Tensor) or W.device != B.device or W.dtype != F64 or W.dim() not in (2, 3):
        raise _lib.FmxError("risk_books: W must be a float64 [M][D][A] tensor on B's device")
    W = as3(W).contiguous()
    M = W.shape[0]
    if tuple(W.shape[1:]) != (D, A):
        raise _lib.FmxError(f"risk_books: W is {tuple(W.shape)}, expected [M][{D}][{A}]")
    _check_present(present, D, A)
    if valid is not None:
        valid = torch.as_tensor(valid).to(device=B.device, dtype=torch.uint8).contiguous()
        if tuple(valid.shape) != (D,):
            raise _lib.FmxError(f"risk_books: valid must be [{D}]")
    dev = B.device
    out = {"var": torch.empty((M, D, 3), dtype=F64, device=dev), "expo": torch.empty((M, D, K), dtype=F64, device=dev),
           "contrib": torch.empty((M, D, K), dtype=F64, device=dev)}
    if marginal:
        out["marginal"] = torch.empty((M, D, A), dtype=F64, device=dev)
    call("fmx_risk_books", ptr(B), ptr(Fc), ptr(S2), ptr(W), ptr(present), ptr(valid), int(K), int(D), int(A), int(M),
         ptr(out["var"]), ptr(out["expo"]), ptr(out["contrib"]), ptr(out.get("marginal")), stream_ptr())
    return out


def risk_mvo_books(B, Fc, S2, X, present=None, model_row=None, max_weight=0.03, max_iter=20000, eps=1e-9,
                   neutral=None, return_expo=False):
    """``sim_mvo_books``' QP against the factor model (fmx_risk_mvo_books): book j is
    the minimum-variance long/short book of signal X[j] under diag(S2[r]) + B[:, r]' Fc[r] B[:, r],
    r = model_row[j] (default: j, for a model with one date per book; -1: no model, status 4).
    B [K][Dm][A], Fc [Dm][K][K], S2 [Dm][A], X [J][A], present [J][A] uint8 or None.  Returns
    (W [J][A], counts [J][2], info [J][6]) as ``sim_mvo_books`` (info[:, 4] = the smallest
    specific variance of the active cells).  A model_row outside [-1, Dm) raises FmxError.
    ``neutral``: factor indices k the book is also neutral to, B[k, r] . w = 0 on the active cells
    (fmx_risk_mvo_neutral_books); a date on which that is infeasible ends with status
    1.  ``return_expo`` appends expo [J][K] = B . w of the returned rows (NaN on status 3 / 4)."""
    K, Dm, A = _check_risk_model("risk_mvo_books", B, Fc, S2)
    if not _is_f64_device(X, (2,), B.device):
        raise _lib.FmxError("risk_mvo_books: X must be a float64 [J][A] tensor on B's device")
    X = X.contiguous()
    J = X.shape[0]
    _mvo_assets("risk_mvo_books", "B", A, X.shape[1])
    _check_present(present, J, A)
    if model_row is None:
        if J != Dm:
            raise _lib.FmxError(f"risk_mvo_books: model_row is needed when X has {J} rows and the model {Dm} dates")
        model_row = torch.arange(J, dtype=torch.int32)
    model_row = torch.as_tensor(model_row, dtype=torch.int32).to(X.device).contiguous()
    if tuple(model_row.shape) != (J,):
        raise _lib.FmxError(f"risk_mvo_books: model_row must be [{J}]")
    W, counts, info = _mvo_outputs((J,), (A, 2, 6), X.device)
    mask = 0
    for k in (() if neutral is None else neutral):
        if not 0 <= int(k) < K:
            raise _lib.FmxError(f"risk_mvo_books: neutral factor {k} outside [0, {K})")
        mask |= 1 << int(k)
    if mask == 0 and not return_expo:
        call("fmx_risk_mvo_books", ptr(B), ptr(Fc), ptr(S2), int(K), int(Dm), int(A), ptr(model_row), ptr(X),
             ptr(present), int(J), float(max_weight), int(max_iter), float(eps), ptr(W), ptr(counts), ptr(info),
             stream_ptr())
        return W, counts, info
    expo = torch.empty((J, K), dtype=F64, device=X.device) if return_expo else None
    nb = int(_lib.load().fmx_risk_mvo_neutral_books_work_bytes(A, K, J))
    work, wb = _workspace_bytes(X.device, nb)
    call("fmx_risk_mvo_neutral_books", ptr(B), ptr(Fc), ptr(S2), int(K), int(Dm), int(A), ptr(model_row), ptr(X),
         ptr(present), int(J), mask, float(max_weight), int(max_iter), float(eps), ptr(W), ptr(counts), ptr(info),
         ptr(expo), ptr(work), wb, stream_ptr())
    return (W, counts, info, expo) if return_expo else (W, counts, info)


def _mvo_turnover_inputs(fn, R0, win_rows, win_T, X, present, W, return_opt, chain_windows):
    """What ``sim_mvo_turnover_books`` and ``sim_mvo_turnover_chains`` (``fn``, for the error
    texts) check and allocate alike.  ``chain_windows``: the window tables may be per chain.
    Returns (R0, win_rows, win_T, Lmax, shared, X, W, Wopt, counts, info)."""
    for t, name, nd in ((R0, "R0", (2,)), (X, "X", (2, 3))):
        if not _is_f64_device(t, nd):
            raise _lib.FmxError(f"{fn}: {name} must be a float64 HIP device tensor "
                                f"({' or '.join(str(n) for n in nd)}-D)")
    R0, X = R0.contiguous(), as3(X).contiguous()
    A, (B, J, _) = R0.shape[1], X.shape
    _mvo_assets(fn, "R0", A, X.shape[2])
    _check_present_chains(present, B, J, A)
    win_rows, win_T, Lmax, shared = _mvo_windows(fn, win_rows, win_T, X.device, J, B if chain_windows else None)
    if W is None:
        W = torch.zeros((B, J, A), dtype=F64, device=X.device)
    elif not _is_f64_device(W, (2, 3), X.device) or tuple(as3(W).shape) != (B, J, A) or not W.is_contiguous():
        raise _lib.FmxError(f"{fn}: W must be a contiguous float64 [B][J][A] tensor on X's device")
    Wopt = torch.empty((B, J, A), dtype=F64, device=X.device) if return_opt else None
    counts, info = _mvo_outputs((B, J), (2, 6), X.device)
    return R0, win_rows, win_T, Lmax, shared, X, as3(W), Wopt, counts, info


def sim_mvo_turnover_books(R0, win_rows, win_T, X, present=None, W=None, shrinkage=0.1, max_weight=0.03,
                           turnover_penalty=0.1, return_weight=0.0, max_iter=20000, eps=1e-9, return_opt=False):
    """Simulation._daily_trade_list, method 'mvo_turnover' (portfolio_simulation.py:206-248,
    :463-585) for B independent chains of J dates (fmx_sim_mvo_turnover_books): R0, win_rows and
    win_T as ``sim_mvo_books``, shared by the chains; X [B][J][A] (or [J][A]: one chain) the
    signals, present [B][J][A] / [J][A] uint8 or None.  ``W`` [B][J][A] (optional) carries the
    caller's equal-weight book on the rows of the dates without returns history (win_T = 0):
    the kernel reads those rows as the next date's previous weights and writes every other row.
    Returns (W, counts [B][J][2], info [B][J][6]) and, with ``return_opt``, Wopt [B][J][A]: the
    solver's iterate before the prune / renormalise step."""
    R0, win_rows, win_T, Lmax, _, X, W, Wopt, counts, info = _mvo_turnover_inputs(
        "sim_mvo_turnover_books", R0, win_rows, win_T, X, present, W, return_opt, chain_windows=False)
    (Dr, A), (B, J, _) = R0.shape, X.shape
    nb = int(_lib.load().fmx_sim_mvo_turnover_books_work_bytes(A, Lmax, J, B))
    work, wb = _workspace_bytes(X.device, nb)
    call("fmx_sim_mvo_turnover_books", ptr(R0), int(Dr), int(A), ptr(win_rows), ptr(win_T), Lmax, ptr(X), ptr(present),
         int(J), int(B), float(shrinkage), float(max_weight), float(turnover_penalty), float(return_weight),
         int(max_iter), float(eps), ptr(W), ptr(Wopt), ptr(counts), ptr(info), ptr(work), wb, stream_ptr())
    return (W, counts, info, Wopt) if return_opt else (W, counts, info)


def sim_mvo_turnover_chains(R0, win_rows, win_T, X, present=None, W=None, shrinkage=0.1, max_weight=0.03,
                            turnover_penalty=0.1, return_weight=0.0, max_iter=20000, eps=1e-9, skip_absent=True,
                            return_opt=False):
    """``sim_mvo_turnover_books`` for B chains with their own windows and their own date lists
    (fmx_sim_mvo_turnover_chains): win_rows [B][J][Lmax] / win_T [B][J] hold every chain's
    tables ([J][Lmax] / [J]: one table shared by the chains).  With ``skip_absent`` a (chain,
    date) without a present cell is not a date of that chain: NaN row, NaN counts, info[0] = 5,
    and the chain's previous book stays the one of its last date with rows.  Returns
    (W [B][J][A], counts [B][J][2], info [B][J][6]) and Wopt with ``return_opt``."""
    R0, win_rows, win_T, Lmax, shared, X, W, Wopt, counts, info = _mvo_turnover_inputs(
        "sim_mvo_turnover_chains", R0, win_rows, win_T, X, present, W, return_opt, chain_windows=True)
    (Dr, A), (B, J, _) = R0.shape, X.shape
    nb = int(_lib.load().fmx_sim_mvo_turnover_chains_work_bytes(A, Lmax, J, B))
    work, wb = _workspace_bytes(X.device, nb)
    call("fmx_sim_mvo_turnover_chains", ptr(R0), int(Dr), int(A), ptr(win_rows), ptr(win_T), Lmax, 0 if shared else int(J),
         ptr(X), ptr(present), int(J), int(B), float(shrinkage), float(max_weight), float(turnover_penalty),
         float(return_weight), int(max_iter), float(eps), int(bool(skip_absent)), ptr(W), ptr(Wopt), ptr(counts),
         ptr(info), ptr(work), wb, stream_ptr())
    return (W, counts, info, Wopt) if return_opt else (W, counts, info)


def sim_mvo_window_rows(fpresent, rpresent, nbefore, lookback: int):
    """The returns windows of N (manager, date) rows in one pass (fmx_sim_mvo_window_rows;
    the rule of ``simulation.mvo_window_rows``): fpresent [N][A] uint8 the rows' present
    symbols, rpresent [Dr][A] uint8 the returns' rows, nbefore [N] int32 the number of returns
    dates before each row's date.  Returns (win_rows int32 [N][Lmax] ascending, unused tail 0;
    win_T int32 [N]) with Lmax = min(lookback, Dr), at least 1."""
    for t, name in ((fpresent, "fpresent"), (rpresent, "rpresent")):
        if (not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != torch.uint8 or t.dim() != 2
                or not t.is_contiguous()):
            raise _lib.FmxError(f"sim_mvo_window_rows: {name} must be a contiguous uint8 2-D HIP device tensor")
    (N, A), Dr = fpresent.shape, rpresent.shape[0]
    if rpresent.shape[1] != A or not 1 <= A <= SIM_MVO_MAX_A:
        raise _lib.FmxError(f"sim_mvo_window_rows: the masks must share 1 <= A <= {SIM_MVO_MAX_A} asset columns")
    if not 1 <= int(lookback) <= SIM_MVO_MAX_T:
        raise _lib.FmxError(f"sim_mvo_window_rows: 1 <= lookback <= {SIM_MVO_MAX_T} supported, got {lookback}")
    nbefore = torch.as_tensor(nbefore, dtype=torch.int32).to(fpresent.device).contiguous()
    if tuple(nbefore.shape) != (N,):
        raise _lib.FmxError("sim_mvo_window_rows: nbefore must be [N]")
    Lmax = max(1, min(int(lookback), Dr))
    win_rows = torch.empty((N, Lmax), dtype=torch.int32, device=fpresent.device)
    win_T = torch.empty((N,), dtype=torch.int32, device=fpresent.device)
    nb = int(_lib.load().fmx_sim_mvo_window_rows_work_bytes(N, A, Dr))
    work, wb = _workspace_bytes(fpresent.device, nb)
    call("fmx_sim_mvo_window_rows", ptr(fpresent), ptr(rpresent), ptr(nbefore), int(N), int(A), int(Dr), Lmax,
         ptr(win_rows), ptr(win_T), ptr(work), wb, stream_ptr())
    return win_rows, win_T


def mm_combine(Wf, counts, fw, colmap, wdate):
    """multi_manager combination (multi_manager.py:51-72) of fmx_trade_equal outputs."""
    F, D, A = Wf.shape
    Dw, Fw = fw.shape
    if tuple(counts.shape) != (F, D, 2) or len(colmap) != Fw or len(wdate) != Dw:
        raise _lib.FmxError("mm_combine: shape mismatch")
    cm = np.asarray(colmap, dtype=np.int32)
    wd = np.asarray(wdate, dtype=np.int32)
    if (cm >= F).any() or (wd >= D).any():
        raise _lib.FmxError("mm_combine: colmap/wdate out of range")
    dev = Wf.device
    fw_d = torch.as_tensor(np.ascontiguousarray(fw, dtype=np.float64), device=dev)
    cm_d = torch.as_tensor(cm, device=dev)
    wd_d = torch.as_tensor(wd, device=dev)
    out = torch.empty((Dw, A), dtype=F64, device=dev)
    oc = torch.empty((Dw, 2), dtype=F64, device=dev)
    call("fmx_mm_combine", ptr(Wf.contiguous()), ptr(counts.contiguous()), ptr(fw_d), ptr(cm_d), ptr(wd_d),
         ptr(out), ptr(oc), Fw, Dw, D, A, stream_ptr())
    return out, oc


# ----------------------------------------------------------------------------- P&L
def _dense2(X, name):
    if X.dim() != 2 or X.dtype != F64 or not X.is_cuda or not X.is_contiguous():
        raise _lib.FmxError(f"{name} must be a contiguous float64 [D][A] device tensor")


def pnl_daily(W, R, CAP, wprev, contrib=False):
    """Simulation._daily_portfolio_returns per-date sums (fmx_pnl_daily): [D][6] and the
    optional per-symbol [A][2] contributions."""
    _dense2(W, "W")
    _dense2(R, "R")
    D, A = W.shape
    if tuple(R.shape) != (D, A) or (CAP is not None and (tuple(CAP.shape) != (D, A))):
        raise _lib.FmxError("pnl_daily: shape mismatch")
    if CAP is not None:
        _dense2(CAP, "CAP")
    wp = torch.as_tensor(np.ascontiguousarray(np.asarray(wprev, dtype=np.int32)), device=W.device)
    if wp.numel() != D or (wp >= D).any():
        raise _lib.FmxError("pnl_daily: wprev must be [D] row indices < D (or -1)")
    out = torch.empty((D, 6), dtype=F64, device=W.device)
    cb = torch.empty((A, 2), dtype=F64, device=W.device) if contrib else None
    call("fmx_pnl_daily", ptr(W), ptr(R), ptr(CAP), ptr(wp), ptr(out), ptr(cb), D, A, stream_ptr())
    return out, cb


def pnl_books(Wraw, R, CAP, wprev, prev_row=None):
    """The six per-date sums of ``pnl_daily`` for F books in one launch (fmx_pnl_books):
    Wraw [F][D][A] SAME-DAY books (``trade_books(..., raw=True)``: NaN = no row), R / CAP
    [D][A] and wprev [D] shared by the books, prev_row int32 [D][A] (each cell's previous
    feature row of its symbol, -1 = none / not a feature row) or None for the dense grid
    (row d - 1).  Returns out [F][D][6]; out[f] has the bits of
    ``pnl_daily(shift_rows(Wraw)[f], R, CAP, wprev)[0]``."""
    _check_panel(Wraw, "Wraw")
    _dense2(R, "R")
    F, D, A = Wraw.shape
    if tuple(R.shape) != (D, A) or (CAP is not None and (tuple(CAP.shape) != (D, A))):
        raise _lib.FmxError("pnl_books: shape mismatch")
    if CAP is not None:
        _dense2(CAP, "CAP")
    wp = torch.as_tensor(np.ascontiguousarray(np.asarray(wprev, dtype=np.int32)), device=Wraw.device)
    if wp.numel() != D:
        raise _lib.FmxError("pnl_books: wprev must be [D] row indices < D (or -1)")
    if prev_row is not None:
        prev_row = torch.as_tensor(prev_row, dtype=torch.int32).to(Wraw.device).contiguous()
        if tuple(prev_row.shape) != (D, A):
            raise _lib.FmxError("pnl_books: prev_row must be int32 [D][A]")
    out = torch.zeros((F, D, 6), dtype=F64, device=Wraw.device)
    if Wraw.numel() == 0:
        return out
    call("fmx_pnl_books", ptr(Wraw), ptr(R), ptr(CAP), ptr(prev_row), ptr(wp), ptr(out), F, D, A, stream_ptr())
    return out


def daily_corr(X, R):
    """Per-date Pearson (np.corrcoef) of pair-valid cells (fmx_daily_corr): [D][2] = (n, corr)."""
    _dense2(X, "X")
    _dense2(R, "R")
    D, A = X.shape
    if tuple(R.shape) != (D, A):
        raise _lib.FmxError("daily_corr: shape mismatch")
    out = torch.empty((D, 2), dtype=F64, device=X.device)
    call("fmx_daily_corr", ptr(X), ptr(R), ptr(out), D, A, stream_ptr())
    return out


# ----------------------------------------------------------------------------- quantile backtest
QLABEL_MAX_A = 8192         # fmx_cs_qlabel / fmx_qbucket_mean: one row's (key, asset) pairs in LDS
QLABEL_MAX_GROUPS = 32
_QCUT: dict = {}            # n_groups -> {m: cum row}


def qcut_cum(m: int, n_groups: int) -> np.ndarray:
    """cum[k] = number of ordinal ranks 1..m whose label under
    ``pd.qcut(ranks, n_groups, labels=False, duplicates="drop")`` is <= k (int32 [n_groups];
    composite_factor.py:71-74).  qcut's bins are ``Series(ranks).quantile(linspace(0, 1,
    n + 1))`` and a rank r gets the first bin whose right edge is >= r, so cum[k] is the
    floor of pandas' own (k + 1)-th edge -- taken from pandas, because the floating-point
    edges do not follow a closed form.  m <= 1: all zero (qcut labels nothing).  Cached."""
    import pandas as pd
    tab = _QCUT.setdefault(int(n_groups), {})
    row = tab.get(int(m))
    if row is None:
        if m <= 1:
            row = np.zeros(n_groups, dtype=np.int32)
        else:
            edges = pd.Series(np.arange(1.0, m + 1)).quantile(np.linspace(0, 1, n_groups + 1)).to_numpy()
            row = np.floor(edges[1:]).astype(np.int32)
        row.setflags(write=False)
        tab[int(m)] = row
    return row


def cs_qlabel(X, n_groups: int, present=None):
    """Per-date quantile groups (fmx_cs_qlabel): uint8 [F][D][A], 0 = none (absent, NaN or a
    date of <= 1 valid cells), else ``n_groups - qcut label`` of the cell's
    rank(method="first") (1 = top; composite_factor.py:71-77).  The cut table holds the
    distinct valid-cell counts of the panel's rows (one device count pass)."""
    X = as3(X)
    _check_panel(X)
    F, D, A = X.shape
    _check_present(present, D, A)
    n = int(n_groups)
    if not 2 <= n <= QLABEL_MAX_GROUPS:
        raise _lib.FmxError(f"cs_qlabel: 2 <= n_groups <= {QLABEL_MAX_GROUPS}, got {n_groups}")
    if A > QLABEL_MAX_A:
        raise _lib.FmxError(f"cs_qlabel: rows of A <= {QLABEL_MAX_A} assets, got {A}")
    labels = torch.empty((F, D, A), dtype=torch.uint8, device=X.device)
    if labels.numel() == 0:
        return labels
    valid = ~torch.isnan(X)
    if present is not None:
        valid &= present.unsqueeze(0) != 0
    ms = torch.unique(valid.sum(dim=2)).cpu().numpy()
    del valid
    ms = [int(m) for m in ms if m >= 2]
    m_index = np.full(A + 1, -1, dtype=np.int32)
    m_index[ms] = np.arange(len(ms), dtype=np.int32)
    cum = np.stack([qcut_cum(m, n) for m in ms]) if ms else np.zeros((1, n), dtype=np.int32)
    cum_d = torch.as_tensor(np.ascontiguousarray(cum, dtype=np.int32), device=X.device)
    mi_d = torch.as_tensor(m_index, device=X.device)
    call("fmx_cs_qlabel", ptr(X), ptr(present), ptr(cum_d), ptr(mi_d), ptr(labels), F, D, A, A, n, stream_ptr())
    return labels


def qbucket_mean(labels, R, n_groups: int, prev_row=None, rpresent=None):
    """Mean return per (factor, date, group) of the groups lagged one row per symbol
    (fmx_qbucket_mean; composite_factor.py:79-98): labels uint8 [F][D][A] from cs_qlabel,
    R [D][A] float64 (NaN = no return), prev_row int32 [D][A] (the symbol's previous feature
    row, -1 = none / not a feature row) or None for the dense grid (row d - 1), rpresent
    uint8 [D][A] or None.  Returns (mean float64 [F][D][n], count int32 [F][D][n]); the sums
    are exact, so the result is independent of chunking and of dense-vs-gather addressing."""
    if (not isinstance(labels, torch.Tensor) or labels.device.type != "cuda" or labels.dtype != torch.uint8
            or labels.dim() != 3 or not labels.is_contiguous()):
        raise _lib.FmxError("qbucket_mean: labels must be a contiguous uint8 [F][D][A] device tensor")
    F, D, A = labels.shape
    _dense2(R, "R")
    if tuple(R.shape) != (D, A):
        raise _lib.FmxError("qbucket_mean: R must be [D][A]")
    _check_present(rpresent, D, A)
    if prev_row is not None:
        prev_row = torch.as_tensor(prev_row, dtype=torch.int32).to(labels.device).contiguous()
        if tuple(prev_row.shape) != (D, A):
            raise _lib.FmxError("qbucket_mean: prev_row must be int32 [D][A]")
    n = int(n_groups)
    nn = max(n, 0)
    mean = torch.empty((F, D, nn), dtype=F64, device=labels.device)
    count = torch.empty((F, D, nn), dtype=torch.int32, device=labels.device)
    call("fmx_qbucket_mean", ptr(labels), ptr(R), ptr(rpresent), ptr(prev_row), ptr(mean), ptr(count), F, D, A, n,
         stream_ptr())
    return mean, count


# ----------------------------------------------------------------------------- performance statistics
PERF = _lib.PERF
PERF_NSTAT = _lib.PERF_NSTAT
PERF_TMAX = _lib.PERF_TMAX


def _check_table(R, name="R"):
    """A [K][T] float64 device table, one series per row with unit stride; rows may be padded
    (a column slice of a wider contiguous table).  Returns the row stride ld >= T."""
    if not isinstance(R, torch.Tensor) or R.device.type != "cuda":
        raise _lib.FmxError(f"{name} must be a HIP device tensor")
    if R.dtype != F64 or R.dim() != 2:
        raise _lib.FmxError(f"{name} must be a float64 [K][T] tensor (one series per row)")
    K, T = R.shape
    if K < 1 or T < 1:
        raise ValueError(f"{name} must hold at least one series and one row")
    ld = R.stride(0) if K > 1 else T
    if (T > 1 and R.stride(1) != 1) or ld < T:
        raise _lib.FmxError(f"{name} must hold each series contiguously, rows at most padded")
    return ld


def _table_out(out, key, shape, R, ld=None):
    """Output ``key``: the caller's tensor (checked) or a new one.  With ``ld`` the output is a
    [K][T] curve that shares R's row stride."""
    t = None if out is None else out.get(key)
    if t is None:
        if ld is None or ld == shape[1]:
            return torch.empty(shape, dtype=F64, device=R.device)
        return torch.empty((shape[0], ld), dtype=F64, device=R.device)[:, :shape[1]]
    ok = (isinstance(t, torch.Tensor) and t.device == R.device and t.dtype == F64 and tuple(t.shape) == tuple(shape)
          and t.data_ptr() != R.data_ptr())
    if ok and ld is None:
        ok = t.is_contiguous()
    elif ok:
        ok = _check_table(t, f"out[{key!r}]") == ld
    if not ok:
        raise _lib.FmxError(f"out[{key!r}] must be a distinct float64 {tuple(shape)} tensor on R's device"
                            + ("" if ld is None else " with R's row stride"))
    return t


def perf_stats(R, rf_daily=0.0, curves=True, out=None):
    """Performance statistics of K return series (fmx_perf_stats): R is [K][T] float64 SIMPLE
    returns, one series per row (rows may be padded: the row stride is passed as ld), NaN = no
    observation.  Returns ``(stats, cum, dd)``: stats [PERF_NSTAT][K] with the rows named by
    ``PERF``, and with ``curves`` the cumulative-return and drawdown curves [K][T] with R's row
    stride (None otherwise).  ``out`` may hold preallocated tensors under 'stats' / 'cum' / 'dd'.
    pandas' bits per series, whatever K.  T <= PERF_TMAX."""
    ld = _check_table(R)
    K, T = R.shape
    if T > PERF_TMAX:
        raise ValueError(f"perf_stats: a series may hold at most {PERF_TMAX} rows (got {T})")
    bad = set(out or ()) - {"stats", "cum", "dd"}
    if bad:
        raise ValueError(f"perf_stats: unknown outputs {sorted(bad)}")
    stats = _table_out(out, "stats", (PERF_NSTAT, K), R)
    cum = _table_out(out, "cum", (K, T), R, ld) if curves else None
    dd = _table_out(out, "dd", (K, T), R, ld) if curves else None
    if curves and cum.data_ptr() == dd.data_ptr():
        raise _lib.FmxError("out['cum'] and out['dd'] must be distinct")
    call("fmx_perf_stats", ptr(R), K, T, ld, float(rf_daily), ptr(stats), ptr(cum), ptr(dd), stream_ptr())
    return stats, cum, dd


def perf_periods(R, seg, nseg: int, out=None):
    """Period returns of K return series (fmx_perf_periods): ``seg`` gives each of the T rows its
    bucket, non-decreasing in [0, nseg) (checked here, on the host); returns [nseg][K], the
    left-to-right product of 1 + R over a bucket's non-NaN rows minus 1 (0.0 for an empty one)."""
    ld = _check_table(R)
    K, T = R.shape
    nseg = int(nseg)
    if nseg < 1:
        raise ValueError("perf_periods: nseg must be >= 1")
    seg_h = seg.detach().cpu().numpy() if isinstance(seg, torch.Tensor) else np.asarray(seg)
    if seg_h.shape != (T,) or seg_h.dtype.kind not in "iu":
        raise ValueError("perf_periods: seg must be T integers")
    if seg_h.min() < 0 or seg_h.max() >= nseg or (np.diff(seg_h.astype(np.int64)) < 0).any():
        raise ValueError("perf_periods: seg must be non-decreasing with values in [0, nseg)")
    seg_d = torch.as_tensor(np.ascontiguousarray(seg_h, dtype=np.int32), device=R.device)
    O = _table_out(None if out is None else {"out": out}, "out", (nseg, K), R)
    call("fmx_perf_periods", ptr(R), K, T, ld, ptr(seg_d), nseg, ptr(O), stream_ptr())
    return O
