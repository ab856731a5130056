"""The numpy reference of ts_skew / ts_kurt / ts_cov (ts_moments_cases.py) against pandas 2.3,
bit for bit as values and NaN pattern, on every panel and window the GPU test uses -- per-symbol
``rolling(w).skew() / .kurt() / .cov(y)`` on the compacted (date, symbol) Series, dense and
ragged -- and each panel's promise: the cells a GPU test relies on are there, so it cannot pass
on NaN alone.  No GPU."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest

import ts_moments_cases as C


def same(got, ref):
    return np.array_equal(got, ref, equal_nan=True)


def pin(x, present, op, W, y=None):
    """reference == pandas on the whole panel; returns the reference."""
    ref = C.ref_panel(x, present, op, W, y)
    pdv = C.pandas_panel(x, present, op, W, y)
    bad = ~((ref == pdv) | (np.isnan(ref) & np.isnan(pdv)))
    assert same(ref, pdv), (op, W, int(bad.sum()), np.argwhere(bad)[:5].tolist(), ref[bad][:5], pdv[bad][:5])
    return ref


@functools.lru_cache(maxsize=None)
def main_panel(ragged):
    x, present = C.make_panel(C.F, C.D, C.A, 11, ragged)
    return x, present, C.make_y(C.D, C.A, 11)


# ------------------------------------------------------------------------------------ main panel
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("W", C.WINDOWS)
def test_main_panel_is_pandas_and_keeps_its_promise(W, ragged):
    x, present, y = main_panel(ragged)
    el = C.eligible((C.D, C.A), present, W)
    for op in C.OPS:
        ref = pin(x, present, op, W, y if op == "cov" else None)
        if W <= C.D and W >= C.MIN_W[op]:
            frac = np.isfinite(ref[:, el]).mean()
            assert el.any() and frac >= 0.25, (op, W, frac)
        else:
            assert np.isnan(ref).all(), (op, W)
        assert np.isnan(ref[:, ~el]).all()


def test_main_panel_ragged_has_its_edge_symbols():
    _, present, _ = main_panel(True)
    rows = present.sum(axis=0)
    assert rows.max() == C.D and rows[-1] == 2 and (~present[0]).any() and (rows < C.D).any()


# ------------------------------------------------------------------------------------ edge shapes
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("A_", C.EDGE_ASSETS)
def test_asset_edges(A_, ragged):
    x = C.make_values(2, 20, A_, 20 + A_)
    y = C.make_y(20, A_, 20 + A_)
    present = C.edge_present(20, A_, A_) if ragged else None
    for W in C.EDGE_WINDOWS:
        for op in C.OPS:
            ref = pin(x, present, op, W, y if op == "cov" else None)
            assert np.isfinite(ref).any() == (W >= C.MIN_W[op]), (op, W)


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("W", C.DATE_WINDOWS)
def test_date_edges(W, ragged):
    for Dn in C.date_edges(W):
        x = C.make_values(2, Dn, 70, 30 + Dn, nan_frac=0.0)
        y = C.make_y(Dn, 70, 30 + Dn)
        present = C.edge_present(Dn, 70, Dn) if ragged else None
        for op in C.OPS:
            ref = pin(x, present, op, W, y if op == "cov" else None)
            if Dn >= W >= C.MIN_W[op] and not ragged:
                assert np.isfinite(ref[:, Dn - 1]).any(), (op, W, Dn)      # the last row is an output
            if Dn < W:
                assert np.isnan(ref).all()


# ------------------------------------------------------------------------------------ content
def _col(ref, name):
    return ref[0, :, C.CONTENT.index(name)]


@pytest.mark.parametrize("W", C.CONTENT_WINDOWS)
def test_content_columns_dense(W):
    x, _ = C.content_panel(W)
    sk, ku = pin(x, None, "skew", W), pin(x, None, "kurt", W)
    run = np.arange(C.CONTENT_D)
    full = run >= W - 1
    # the centres
    v = C.prep(x[0])
    ms, cs = C.centre(v, "skew")
    mk, ck = C.centre(v, "kurt")
    want = {"mean7": 7.0, "mean1e3": 1000.0, "dyadic2.5": 3.0, "dyadic-1.5": -2.0, "dyadic-2.5": -3.0,
            "dyadic0.5": 1.0}
    for name, m in want.items():
        i = C.CONTENT.index(name)
        assert cs[i] and ck[i] and ms[i] == m and mk[i] == m, (name, ms[i], mk[i])
    i = C.CONTENT.index("far_low")
    assert not cs[i] and not ck[i]
    i = C.CONTENT.index("low_3e4")
    assert cs[i] and not ck[i] and ms[i] != 0.0
    i = C.CONTENT.index("big")
    assert not cs[i] and not ck[i]
    for ref, op, flat in ((sk, "skew", 0.0), (ku, "kurt", -3.0)):
        if W < C.MIN_W[op]:
            assert np.isnan(ref).all()
            continue
        # same-value rule: the constant column, the windows inside the constant run, the +-0.0 tie
        in_run = (run >= C.RUN0 + W - 1) & (run < C.RUN0 + W + 2)
        assert (_col(ref, "const")[full] == flat).all()
        assert (_col(ref, "const_run")[in_run] == flat).all()
        assert np.isfinite(_col(ref, "const_run")[~in_run & full]).all()
        assert not (_col(ref, "const_run")[~in_run & full] == flat).any()
        z = full & (run < 20)
        assert (_col(ref, "zeros")[z] == flat).all()
        # B <= 1e-14: NaN though the window is full and not constant
        in_near = (run >= C.RUN0 + W - 1) & (run < C.RUN0 + W + 3)
        assert np.isnan(_col(ref, "near_const")[in_near]).all()
        assert np.isfinite(_col(ref, "near_const")[~in_near & full]).all()
        for name in ("mean7", "mean1e3", "far_low", "low_3e4", "dyadic2.5", "dyadic-1.5", "dyadic-2.5",
                     "dyadic0.5", "big"):
            assert np.isfinite(_col(ref, name)[full]).all(), name
        # NaN enters at 17 and leaves at 17 + W; the run and the infinities likewise
        c = _col(ref, "one_nan")
        assert np.isnan(c[17:17 + W]).all() and np.isfinite(c[17 + W:]).all() and np.isfinite(c[W - 1:17]).all()
        c = _col(ref, "nan_run")
        last = C.RUN0 + 2 + W + 2 - 1
        assert np.isnan(c[C.RUN0 + 2:last + W]).all() and np.isfinite(c[last + W:]).all()
        c = _col(ref, "infs")
        assert np.isnan(c[5:5 + W]).all() and np.isnan(c[21:21 + W]).all()
        assert np.isfinite(c[5 + W:21]).all() and np.isfinite(c[21 + W:]).all()
        assert np.isnan(_col(ref, "all_nan")).all() and np.isnan(_col(ref, "one_valid")).all()
        assert np.isnan(_col(ref, "tiny")).all()                          # variance 1e-120 <= 1e-14


@pytest.mark.parametrize("W", C.CONTENT_WINDOWS)
def test_content_columns_ragged(W):
    x, present = C.content_panel(W, ragged=True)
    assert not present[0, 0] and present[:, C.CONTENT.index("short")].sum() == W - 1
    assert not present[:, C.CONTENT.index("never")].any()
    assert np.isinf(x[0][~present]).any() and (x[0][~present] == 12345.0).any()
    for op in ("skew", "kurt"):
        ref = pin(x, present, op, W)
        assert np.isnan(_col(ref, "short")).all() and np.isnan(_col(ref, "never")).all()
        assert np.isnan(ref[0][~present]).all()
        if W >= C.MIN_W[op]:
            assert np.isfinite(_col(ref, "mean7")).sum() == present[:, C.CONTENT.index("mean7")].sum() - (W - 1)


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("W", C.COV_WINDOWS)
def test_cov_content(W, ragged):
    """NaN / inf in x only (one_nan, nan_run, infs), in y only (rows 9, 25, 26) and in both."""
    x, present = C.content_panel(5, ragged)
    y = C.content_y(5, ragged)
    ref = pin(x, present, "cov", W, y)
    if W >= 2:
        c = _col(ref, "far_low")
        p = np.ones(C.CONTENT_D, bool) if present is None else present[:, C.CONTENT.index("far_low")]
        rows = np.flatnonzero(p)
        k9 = int(np.searchsorted(rows, 9))                                # y's NaN at date 9 is a row of the symbol
        assert np.isnan(c[rows[k9:k9 + W]]).all()
        assert np.isfinite(c[rows[-1]])
        assert np.isfinite(_col(ref, "big")).any() and np.isfinite(_col(ref, "dyadic-1.5")).any()
        assert np.isnan(_col(ref, "all_nan")).all() and np.isnan(_col(ref, "one_valid")).all()
    else:
        assert np.isnan(ref).all()
    # the per-column y: a different partner per column of a 3-column batch
    x3 = np.concatenate([x, x[:, ::-1], 2.0 * x])
    y3 = np.stack([y, y[::-1], -y])
    pin(x3, present, "cov", W, y3)
    if present is not None:
        assert np.isinf(y[~present]).any() and (y[~present] == 12345.0).any()


def test_c_round_is_half_away_from_zero():
    m = np.array([0.5, 2.5, -1.5, -2.5, 4.5, 0.49999999999999994, -0.3, 7.3, 1e17, -0.0])
    assert same(C.c_round(m), np.array([1.0, 3.0, -2.0, -3.0, 5.0, 0.0, -0.0, 7.0, 1e17, -0.0]))


def test_dropin_path_exports_the_operators():
    """``import operations`` from the drop-in directory re-exports ``__all__``."""
    import factormodeling_amd.operations as ops
    dropin = os.path.join(os.path.dirname(os.path.abspath(ops.__file__)), "dropin")
    saved = sys.modules.pop("operations", None)
    sys.path.insert(0, dropin)
    try:
        m = importlib.import_module("operations")
        assert m.__file__.startswith(dropin)
        for name in ("ts_skew", "ts_kurt", "ts_cov"):
            assert name in ops.__all__ and getattr(m, name) is getattr(ops, name)
    finally:
        sys.path.remove(dropin)
        sys.modules.pop("operations", None)
        if saved is not None:
            sys.modules["operations"] = saved
