"""Panels, case table and dispatch restatement for the rolling kernels of ts_ops.hip (DESIGN
"Rolling kernels: what the tests pin").  tests/test_ts_paths_host.py pins this module without a
GPU; tests/test_gpu_ts_paths.py runs every case against the oracle.

A panel is ``[F][D][A]`` with F = 3 and A in {1, 63, 64, 65, 257}: F * A is never a multiple of
256, so the last block of the column kernels is partial, waves straddle factor boundaries, and
k_ts_win has partial 64-asset chunks and an A = 1 chunk.  Its content is laid out by column
(COLS) for the case's window: noise with ties and NaN, a NaN run longer than W, a constant run
of W + 2, signed zeros, an all-NaN column, a column with one valid cell, columns scaled by 1e150
and 1e-200, the +-inf placements of tests/golden/make_golden_nonfinite.py and an all-finite
control.  The ragged variant adds absent runs of 1 / 9 / 17 / 40 rows from row 3 and from row
14 (across k_ts_win's 8-row walk-back groups and its 16-date tiles), an absent first row, a
column with W - 1 present rows, a column never present; every absent cell of X holds +inf or
12345.0, which must never reach a state or an output.

Windows and dates come from the kernels' own constants (see each ``*_cases`` function).
"""
from __future__ import annotations

import contextlib
import functools
import itertools

import numpy as np

F = 3
ASSETS = (1, 63, 64, 65, 257)
POISON = 12345.0
TSC_MAXW = 4096                 # ts_ops.hip: reciprocal table in LDS up to this window
REG_PF = {5: 5, 10: 10, 20: 5}  # ts_reg_kernel: window -> prefetch depth
TSW_T = 16                      # k_ts_win's date tile

MOMENTS = ("sum", "mean", "std", "var", "zscore")
SHIFTS = ("diff", "delay")
WINDOWED = ("rank", "decay")
SET_OUTS = ("mean", "std", "zscore", "rank", "decay")

COLS = dict(nanrun=2, const=3, zeros=4, allnan=5, onevalid=6, big=7, tiny=8, pinf=9, ninf=10, pair=11,
            first=12, last=13, far=14, nan_inf=15, control=16, gap1=17, gap9=18, gap17=19, gap40=20,
            first_absent=21, short=22, never=23, gap1b=24, gap9b=25, gap17b=26, gap40b=27)
INF_COLS = ("pinf", "ninf", "pair", "first", "last", "far", "nan_inf")
GAPS = dict(gap1=(3, 1), gap9=(3, 9), gap17=(3, 17), gap40=(3, 40), gap1b=(14, 1), gap9b=(14, 9),
            gap17b=(14, 17), gap40b=(14, 40))


# --------------------------------------------------------------------------- dispatch
def expected_path(op, W, ragged):
    """The kernel fmx_ts_op runs for (op, window, dense or ragged), decided the way it decides."""
    if op == "backfill":
        return "k_ts_ptr<8>"
    if op == "decay" and W < 1:
        return "copy+k_ts_window0" if ragged else "copy"
    if op in SHIFTS and W == 0:
        return "k_ts_window0"
    if op in SHIFTS and W < 0:
        return "k_ts_lead_ptr"
    if W < 1:
        raise ValueError("window must be >= 1")
    if not ragged and W in REG_PF:
        return f"k_ts_reg<{W},{REG_PF[W]}>"
    if op in WINDOWED:
        return f"k_ts_win<{TSW_T}>"
    return "k_ts_ptr<8>" if ragged else "k_ts_rl<8>"


def expected_set_path(W, WR, ragged):
    """fmx_ts_set: the fused kernel, or the three moments in one pass and rank / decay on the
    kernels fmx_ts_op gives them."""
    if not ragged and W == 20 and WR == 10:
        return ("k_ts_set<20,10,5>",)
    return ("k_ts_mom3<4>", expected_path("rank", WR, ragged), expected_path("decay", W, ragged))


def expected_corr_path(W, ragged):
    if ragged:
        return "k_ts_corr_ptr"
    return "k_ts_corr_fast<2>" if W <= TSC_MAXW else "k_ts_corr_rl<2>"


def expected_cvf_path(W):
    return "k_ts_cvf_rl<8,true>" if W <= TSC_MAXW else "k_ts_cvf_rl<8,false>"


# --------------------------------------------------------------------------- panels
def layout_window(W, D):
    """The window the panel's runs are laid out for: W itself when a full window fits."""
    return W if 1 <= W <= D else 3


def inf_rows(D, wp):
    """name -> rows that hold +-inf (signs alternate down the list and flip with the factor)."""
    mid = D // 2
    return dict(pinf=[mid], ninf=[mid], pair=[mid, mid + 1], first=[0], last=[D - 1], far=[1, wp + 4],
                nan_inf=[mid + 1])


@functools.lru_cache(maxsize=None)
def panel(D, A, W, ragged, nf=F, scaled=True):
    """(X [nf][D][A], present [D][A] or None), read-only.  ``scaled`` = False leaves the 1e150 /
    1e-200 columns at unit scale (ts_corr: the product x * y must not overflow)."""
    rng = np.random.default_rng([D, A, abs(W) % 7919, int(ragged), nf])
    wp = layout_window(W, D)
    X = rng.standard_normal((nf, D, A))
    tie = rng.random(X.shape) < 0.3
    X[tie] = np.round(X[tie], 1)
    X[rng.random(X.shape) < 0.05] = np.nan
    c = {k: v for k, v in COLS.items() if v < A}

    def rows(lo, n):
        return slice(min(lo, D), min(lo + n, D))

    if "nanrun" in c:
        for f in range(nf):
            X[f, rows(D // 3 + f, wp + 1), c["nanrun"]] = np.nan
        X[:, rows(2, wp + 2), c["const"]] = 0.3
        X[:, 1::5, c["zeros"]] = -0.0
        X[:, 3::5, c["zeros"]] = 0.0
        X[:, :, c["allnan"]] = np.nan
        X[:, :, c["onevalid"]] = np.nan
        X[:, D // 2, c["onevalid"]] = 1.5 + np.arange(nf)
        if scaled:
            X[:, :, c["big"]] *= 1e150
            X[:, :, c["tiny"]] *= 1e-200
        X[:, :, c["control"]] = rng.standard_normal((nf, D))
        for name, rr in inf_rows(D, wp).items():
            X[:, :, c[name]] = rng.standard_normal((nf, D))
            for i, r in enumerate(rr):
                if 0 <= r < D:
                    X[:, r, c[name]] = np.inf * (-1.0) ** (i + (name == "ninf") + np.arange(nf))
        if 0 <= D // 2 < D:
            X[:, D // 2, c["nan_inf"]] = np.nan
    else:                                             # A = 1: one column, one feature per factor
        X[:, :, 0] = rng.standard_normal((nf, D))
        X[0, D // 3, 0] = np.nan
        X[1 % nf, D // 2, 0] = np.inf
        X[2 % nf, D // 3, 0] = -0.0
    present = None
    if ragged:
        present = rng.random((D, A)) > 0.15
        if "nanrun" in c:
            for name in INF_COLS + ("control",):
                present[:, c[name]] = True
            for name, rr in inf_rows(D, wp).items():      # absent rows on both sides of the infs
                for r in rr:
                    for n in (r - 1, r + 1):
                        if 0 <= n < D and 0 <= r < D and not np.isinf(X[0, n, c[name]]) and n != D // 2:
                            present[n, c[name]] = False
            for name, (lo, n) in GAPS.items():
                present[:, c[name]] = True
                present[rows(lo, n), c[name]] = False
            present[:, c["first_absent"]] = True
            present[0, c["first_absent"]] = False
            present[:, c["short"]] = False
            present[rows(D // 4, 2 * (wp - 1)), c["short"]][::2] = True    # W - 1 present rows
            present[:, c["never"]] = False
        fill = np.where(np.arange(A) % 2 == 0, np.inf, POISON)
        X = np.where(present[None], X, fill[None, None, :])
    X.setflags(write=False)
    if present is not None:
        present.setflags(write=False)
    return X, present


@functools.lru_cache(maxsize=None)
def y_panel(D, A, nf, per_factor, seed=0):
    """The second series of ts_corr: [D][A], or [nf][D][A] with another draw per factor; NaN and
    +-inf of its own, |y| < 1e150."""
    rng = np.random.default_rng([D, A, nf, int(per_factor), seed, 77])
    Y = 0.01 * rng.standard_normal((nf if per_factor else 1, D, A))
    Y[rng.random(Y.shape) < 0.05] = np.nan
    Y[:, D // 3, 1 % A] = np.inf
    Y[:, (2 * D) // 3, min(COLS["control"], A - 1)] = -np.inf
    Y[:, :, min(COLS["tiny"], A - 1)] *= 1e120
    Y = Y if per_factor else Y[0]
    Y.setflags(write=False)
    return Y


# --------------------------------------------------------------------------- case tables
def _rot(i):
    return ASSETS[i % len(ASSETS)]


def reg_cases():
    """k_ts_reg (dense, W in {5, 10, 20}): all nine ops; D on both sides of the unchecked main
    loop's condition d0 + W + PF <= D.  -> (ops, W, D, A, ragged)"""
    out, i = [], 0
    for W, PF in REG_PF.items():
        for D in (1, W - 1, W, W + 1, W + PF - 1, W + PF, 2 * W + PF + 1, 3 * W + 7):
            out.append((MOMENTS + WINDOWED + SHIFTS, W, D, _rot(i), False))
            i += 1
    return out


def _col_wd():
    wd = []
    for W in (1, 2, 3, 21, 40):
        wd += [(W, D) for D in sorted({1, 7, 8, 9, W, W + 1, 2 * W + 3})]
    for D in (1, 7, 8, 9, 40):
        wd += [(D + 1, D)] * (D + 1 not in REG_PF) + [(5000, D)]
    return wd


def rl_cases():
    """k_ts_rl<8> (dense, other windows): D around the 8-date prefetch group and the window."""
    return [(MOMENTS + SHIFTS, W, D, _rot(i), False) for i, (W, D) in enumerate(_col_wd())]


def ptr_cases():
    """k_ts_ptr<8> (ragged; backfill also dense).  A ragged panel at W in {5, 10, 20} must not
    take the register ring."""
    wd = _col_wd() + [(W, D) for W in REG_PF for D in (W - 1, W, W + 1, 2 * W + 3)]
    out = [(MOMENTS + SHIFTS + ("backfill",), W, D, _rot(i + 2), True) for i, (W, D) in enumerate(wd)]
    out += [(("backfill",), 1, D, _rot(i), False) for i, D in enumerate((1, 7, 8, 9, 33))]
    return out


def win_cases():
    """k_ts_win<., 16> (rank / decay; dense with W not in {5, 10, 20}, ragged with any W): D
    around the 16-date tile."""
    out, i = [], 0
    for ragged in (False, True):
        for W in (1, 2, 3, 16, 17, 21, 40, "D+1") + ((5, 10, 20) if ragged else ()):
            for D in (1, 15, 16, 17, 31, 33, "2W+19"):
                w = W if W != "D+1" else (D if D != "2W+19" else 33) + 1
                d = D if D != "2W+19" else (2 * w + 19 if W != "D+1" else 33)
                out.append((WINDOWED, w, d, _rot(i), ragged))
                i += 1
    return sorted(set(out), key=out.index)


def lead_cases():
    """k_ts_lead_ptr: diff / delay with a negative window (a lead)."""
    out, i = [], 0
    for ragged in (False, True):
        for D in (8, 33):
            for W in (-1, -7, -(D - 1), -D, -(D + 5)):
                out.append((SHIFTS, W, D, _rot(i), ragged))
                i += 1
    return out


def window0_cases():
    """k_ts_window0: diff / delay at W = 0; decay at W in {0, -3} (a copy, masked when ragged)."""
    out = []
    for i, ragged in enumerate((False, True)):
        for j, A in enumerate((65, 257, 1)):
            out.append((SHIFTS + ("decay",), 0, 33 + j, A, ragged))
            out.append((("decay",), -3, 33 + j, A, ragged))
    return out


TS_ARMS = dict(reg=reg_cases, rl=rl_cases, ptr=ptr_cases, win=win_cases, lead=lead_cases, window0=window0_cases)


def set_cases():
    """fmx_ts_set -> (arm, W, WR, D, A, ragged).  The fused k_ts_set<20, 10, 5> at k_ts_reg's D
    list; k_ts_mom3<4> (+ single-op rank / decay) dense and ragged with D mod 4 in {0, 1, 3}."""
    out = [("fused", 20, 10, D, _rot(i), False) for i, D in enumerate((1, 19, 20, 21, 24, 25, 46, 67))]
    i = 0
    for W, WR, ragged in ((20, 5, False), (33, 10, False), (20, 10, True)):
        for D in (40, 41, 43):
            out.append(("mom3", W, WR, D, _rot(i + 1), ragged))
            i += 1
    return out


SUBSET_SHAPES = (("fused", 20, 10, 46, 65, False), ("mom3", 20, 10, 43, 65, True))


def subsets():
    return [s for n in range(1, 6) for s in itertools.combinations(SET_OUTS, n)]


def corr_cases():
    """fmx_ts_corr -> (arm, nf, W, D, A, ragged, per_factor_y).  k_ts_corr_fast<2>: four factors
    share a block, so F in {1, 3, 4, 5}; D odd and even (two dates in flight); y as [D][A] and
    per factor.  k_ts_corr_rl<2>: W = 4097 and 5000 on 40 dates (all NaN), and the 4108-date panel
    of long_case, whose +-inf and NaN rows enter and leave full windows.  k_ts_corr_ptr: ragged."""
    out, i = [], 0
    for nf in (1, 3, 4, 5):
        for W, D in ((2, 40), (5, 41), (20, 41), (20, 40), (TSC_MAXW, 41)):
            out.append(("fast", nf, W, D, _rot(i + 1), False, i % 2 == 1))
            i += 1
    for W in (TSC_MAXW + 1, 5000):
        for pf in (False, True):
            out.append(("rl", 3, W, 40, _rot(i), False, pf))
            i += 1
    for W, D in ((2, 41), (5, 41), (60, 100), (5, 40)):
        for pf in (False, True):
            out.append(("ptr", 3, W, D, _rot(i), True, pf))
            i += 1
    return out


LONG_D, LONG_A = TSC_MAXW + 12, 3     # full windows on each side of TSC_MAXW: 13 / 12 rows
# (row, column): what the first rows of the long panel hold; all of it has left the window W rows on
LONG_X_INF, LONG_X_NAN, LONG_Y_NAN, LONG_Y_INF = (1, 0), (3, 0), (0, 1), (2, 1)
LONG_CLEAR = {0: 4, 1: 3, 2: 0}       # column -> first row whose window of W rows is clean: W - 1 + this


def feature_cases():
    """-> (arm, nf, W, D, A).  k_ts_cvf_rl<8, true / false> on both sides of TSC_MAXW and
    k_ts_corr_feat<true / false> (with and without the corr output), F in {1, 5}."""
    out = []
    for i, nf in enumerate((1, 5)):
        out += [("cvf", nf, 20, 41, _rot(i + 2)), ("cvf", nf, TSC_MAXW, 40, _rot(i + 3)),
                ("cvf", nf, TSC_MAXW + 1, 40, _rot(i + 3)),
                ("feat", nf, 3, 40, _rot(i + 1)), ("feat", nf, 20, 41, _rot(i + 2))]
    return out


REG_ENGINE_W = (1, 2, 5, 40, "D+1")
REG_ENGINE_SHAPE = (60, 33)


def regression_cases():
    """k_ts_regression_ptr through engine.ts_regression -> (W, rettype): every rettype at W = 5,
    the residual and R^2 (the one that reads all five means) at the other windows."""
    D = REG_ENGINE_SHAPE[0]
    out = []
    for W in REG_ENGINE_W:
        w = D + 1 if W == "D+1" else W
        out += [(w, rt) for rt in ((0, 1, 2, 3, 6) if w == 5 else (0, 6))]
    return out


# --------------------------------------------------------------------------- references
@contextlib.contextmanager
def legacy_rule():
    """The oracle as it was before the non-finite contract (+-inf enters the machines): what the
    inf-bearing columns must NOT equal."""
    import oracle.ops as O
    keep = O._prep
    O._prep = lambda c: c
    try:
        yield
    finally:
        O._prep = keep


def oracle_ts(op, x, W, p):
    """One [D][A] factor through oracle.ops; ``var`` is ts_std without the square root."""
    import oracle.numerics as nm
    import oracle.ops as O
    with np.errstate(all="ignore"):
        if op == "var":
            return O._ts(x, p, lambda c: nm.roll_var(O._prep(c), W, 1))
        if op == "backfill":
            return O.ts_backfill(x, p)
        return getattr(O, "ts_" + op)(x, W, p)


def _freeze(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def ts_reference(op, W, D, A, ragged):
    """[F][D][A]; computed once per process and shared: callers must not modify it."""
    X, p = panel(D, A, W, ragged)
    return _freeze(np.stack([oracle_ts(op, X[f], W, p) for f in range(F)]))


@functools.lru_cache(maxsize=None)
def decay_bound(W, D, A, ragged):
    """tests/test_longwin.py's _decay_bound: 1e-13 * decay(|x|) + 1e-300 (the reference's dot
    product sums in BLAS order)."""
    X, p = panel(D, A, W, ragged)
    with np.errstate(all="ignore"):
        scale = np.stack([oracle_ts("decay", np.abs(X[f]), W, p) for f in range(F)])
    return _freeze(1e-13 * np.nan_to_num(scale, nan=0.0, posinf=0.0) + 1e-300)


def corr_inputs(nf, W, D, A, ragged, per_factor):
    X, p = panel(D, A, W, ragged, nf, False)
    return X, y_panel(D, A, nf, per_factor), p


@functools.lru_cache(maxsize=None)
def corr_reference(nf, W, D, A, ragged, per_factor):
    import oracle.ops as O
    X, Y, p = corr_inputs(nf, W, D, A, ragged, per_factor)
    with np.errstate(all="ignore"):
        return _freeze(np.stack([O.ts_corr(X[f], Y[f] if per_factor else Y, W, p) for f in range(nf)]))


@functools.lru_cache(maxsize=None)
def feature_reference(nf, W, D, A):
    import oracle.ops as O
    X, Y, _ = corr_inputs(nf, W, D, A, False, False)
    with np.errstate(all="ignore"):
        return _freeze(np.stack([O.corr_vol_feature(X[f], Y, W) for f in range(nf)]))


def _long_inputs(W):
    rng = np.random.default_rng(W)
    X = rng.standard_normal((1, LONG_D, LONG_A))
    Y = 0.01 * rng.standard_normal((LONG_D, LONG_A))
    X[0][LONG_X_INF] = np.inf
    X[0][LONG_X_NAN] = np.nan
    Y[LONG_Y_NAN] = np.nan
    Y[LONG_Y_INF] = -np.inf
    return X, Y


@functools.lru_cache(maxsize=None)
def long_case(W):
    """(X [1][LONG_D][LONG_A], Y, corr, feature) for a window at TSC_MAXW or just past it: noise
    with a +inf and a NaN in x (column 0) and a NaN and a -inf in y (column 1) in rows 0..3, and a
    clean column 2.  The first full windows hold them, so each must LEAVE the window (the only
    place the long-window kernels' remove side sees a non-finite pair); the last rows are finite
    in every column."""
    import oracle.ops as O
    X, Y = _long_inputs(W)
    with np.errstate(all="ignore"):
        return tuple(map(_freeze, (X, Y, O.ts_corr(X[0], Y, W)[None], O.corr_vol_feature(X[0], Y, W)[None])))


def long_case_legacy(W):
    """long_case's corr and feature under the oracle's pre-change rule."""
    import oracle.ops as O
    X, Y = _long_inputs(W)
    with legacy_rule(), np.errstate(all="ignore"):
        return O.ts_corr(X[0], Y, W)[None], O.corr_vol_feature(X[0], Y, W)[None]


def regression_inputs():
    """(y [D][A], x [D][A], valid uint8 [D][A], dcode, scode, yv, xv): the long arrays are the
    present cells in (date, symbol) order; +-inf rows are valid rows (dropna keeps them)."""
    D, A = REG_ENGINE_SHAPE
    X, p = panel(D, A, 5, True, F, False)
    x = X[0].copy()
    y = np.array(y_panel(D, A, 1, False, seed=3)) * 100.0
    x[D // 2, COLS["big"]] = 1e200                     # its square overflows
    y[~p] = POISON
    di, si = np.nonzero(p)
    xv, yv = x[di, si], y[di, si]
    valid = np.zeros((D, A), np.uint8)
    ok = ~np.isnan(xv) & ~np.isnan(yv)
    valid[di[ok], si[ok]] = 1
    return y, x, valid, di, si, yv, xv


@functools.lru_cache(maxsize=None)
def regression_reference(W, rettype):
    import oracle.ops as O
    D, A = REG_ENGINE_SHAPE
    _, _, _, di, si, yv, xv = regression_inputs()
    od, os_, ov = O.ts_regression_fast_long(di, si, yv, xv, W, 0, rettype)
    out = np.full((D, A), np.nan)
    out[od, os_] = ov
    return _freeze(out)
