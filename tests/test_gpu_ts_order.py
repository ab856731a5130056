"""Rolling order statistics on the GPU (fmx_ts_order through engine.ts_order and the six
drop-in operators) against the brute-force reference of ts_order_cases.py, bit-exact as
values (``np.array_equal(..., equal_nan=True)``: -0.0 == 0.0).  tests/test_ts_order_host.py
pins that reference to pandas."""
import functools

import numpy as np
import pandas as pd
import pytest

import ts_order_cases as C

pytestmark = pytest.mark.gpu

F, D, A = 3, 75, 130              # D: no multiple of the 16-date tile; A: two waves + two lanes
WINDOWS = (1, 2, 3, 5, 16, 17, 20, 64, 75, 80)


def _dev(a, dtype=None):
    import torch
    if a is None:
        return None
    t = torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    return t.to(dtype) if dtype else t


def gpu(x, present, op, W, q=0.5, interpolation="linear"):
    import torch
    import factormodeling_amd.engine as E
    y = E.ts_order(op, _dev(x), W, _dev(present, torch.uint8), q, interpolation)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def check(x, present, op, W, q=0.5, interpolation="linear", expect_values=True):
    ref = C.ref_panel(x, present, op, W, q, interpolation)
    if expect_values:
        assert C.has_finite(ref), (op, W, q, interpolation)       # there is something to compare
    else:
        assert np.isnan(ref).all()
    got = gpu(x, present, op, W, q, interpolation)
    bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
    assert np.array_equal(got, ref, equal_nan=True), \
        (op, W, q, interpolation, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5], ref[bad][:5])


def check_all_ops(x, present, W, qs=C.QS, expect_values=True, ops=C.OPS):
    for op in ops:
        if op == "quantile":
            for q in qs:
                check(x, present, op, W, q, expect_values=expect_values)
        else:
            check(x, present, op, W, expect_values=expect_values)


@functools.lru_cache(maxsize=None)
def main_panel(ragged):
    return C.make_panel(F, D, A, 11, ragged)


# ------------------------------------------------------------------------------------ main panel
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("W", WINDOWS)
def test_main_panel(W, ragged):
    x, present = main_panel(ragged)
    check_all_ops(x, present, W, expect_values=W <= D)


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("W", [5, 20])
def test_interpolations(W, ragged):
    x, present = main_panel(ragged)
    for interpolation in C.INTERPOLATIONS:
        for q in C.QS + (0.25, 0.7):
            check(x, present, "quantile", W, q, interpolation)


# ------------------------------------------------------------------------------------ edge shapes
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("A_", [1, 63, 64, 65])
def test_asset_edges(A_, ragged):
    x = C.make_values(2, 20, A_, 20 + A_)
    present = None
    if ragged:
        present = np.random.default_rng(A_).random((20, A_)) >= 0.15
    for W in (1, 4, 7):
        check_all_ops(x, present, W, qs=(0.3,))


def test_single_date():
    x = C.make_values(2, 1, 70, 3, nan_frac=0.1)
    check_all_ops(x, None, 1, qs=(0.0, 0.4, 1.0))
    check_all_ops(x, None, 2, qs=(0.4,), expect_values=False)


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
def test_single_factor(ragged):
    x, present = C.make_panel(1, 50, 33, 4, ragged)
    for W in (3, 10, 33):
        check_all_ops(x, present, W, qs=(0.1, 0.5))


# ------------------------------------------------------------------------------------ content
@pytest.mark.parametrize("W", [1, 2, 4, 7, 18])
def test_content_columns(W):
    """Constant (full ties), strictly increasing / decreasing, +-0.0 ties, a NaN entering and
    leaving the window."""
    x = C.content_panel(with_inf=False)
    check_all_ops(x, None, W, qs=(0.0, 0.3, 0.5, 1.0))
    ref = C.ref_panel(x, None, "argmin", W)[0]
    assert (ref[W - 1:, 0] == 0.0).all() and (ref[W - 1:, 1] == W - 1).all() and (ref[W - 1:, 2] == 0.0).all()
    assert np.isnan(ref[17:17 + W, 3]).all() and np.isfinite(ref[17 + W:, 3]).all()


@pytest.mark.parametrize("W", [1, 3, 9])
def test_infinities_are_ordinary_for_the_extremes(W):
    x = C.content_panel(with_inf=True)
    check_all_ops(x, None, W, ops=C.EXTREMES)
    assert np.isinf(C.ref_panel(x, None, "max", W)[0, :, 6]).any()


# ------------------------------------------------------------------------------------ long windows
def test_long_window_ragged():
    x, present = C.make_panel(1, 230, 70, 8, True)
    x[np.isnan(x)] = 0.5                                  # 200 rows without a NaN have to exist
    x[0, 100, ::7] = np.nan
    check_all_ops(x, present, 200, qs=(0.1, 0.5, 0.99))


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("W", [C.LDS_MAX_W, C.LDS_MAX_W + 1], ids=["lds-ring", "bisection"])
def test_lds_capacity_switch(W, ragged):
    """The last window whose rank ring fits the 160 KiB LDS and the first that runs the
    bisection kernel; D = W + 20, A = 64."""
    Dn = W + 20
    x = C.make_values(1, Dn, 64, 9, nan_frac=0.0)
    x[0, 5, ::9] = np.nan                                 # leaves the window after 6 outputs
    present = None
    if ragged:
        present = np.ones((Dn, 64), dtype=bool)
        present[3, ::2] = False                           # a gap: those columns have W + 19 rows
        present[:40, 63] = False                          # fewer than W rows: all NaN
    check(x, present, "median", W)
    check(x, present, "quantile", W, 0.37)
    check(x, present, "quantile", W, 0.5, "nearest")
    check(x, present, "quantile", W, 1.0)
    check(x, present, "argmax", W)


# ------------------------------------------------------------------------------------ drop-in
def _same(got, ref):
    assert np.array_equal(got.to_numpy(), ref.to_numpy(), equal_nan=True)
    assert got.index.equals(ref.index)
    assert np.isfinite(ref.to_numpy()).any()


def test_dropin_operators_against_pandas():
    import factormodeling_amd.operations as ops
    Dn, An = 40, 30
    x, present = C.make_panel(3, Dn, An, 21, True)
    idx = C.panel_index(Dn, An, present)
    sel = present.reshape(-1)
    df = pd.DataFrame({f"f{k}": x[k].reshape(-1)[sel] for k in range(3)}, index=idx)
    s = df["f1"].rename("alpha")
    calls = [("min", ops.ts_min, ()), ("max", ops.ts_max, ()), ("argmin", ops.ts_argmin, ()),
             ("argmax", ops.ts_argmax, ()), ("median", ops.ts_median, ()),
             ("quantile", ops.ts_quantile, (0.3,)), ("quantile", ops.ts_quantile, (0.8, "midpoint"))]
    for W in (4, 9):
        for op, fn, extra in calls:
            q = extra[0] if extra else 0.5
            interpolation = extra[1] if len(extra) > 1 else "linear"
            got = fn(s, W, *extra)
            assert isinstance(got, pd.Series) and got.name == "alpha"
            _same(got, C.pandas_op(s, op, W, q, interpolation))
            gdf = fn(df, W, *extra)
            assert isinstance(gdf, pd.DataFrame) and list(gdf.columns) == list(df.columns)
            _same(gdf, C.pandas_op(df, op, W, q, interpolation))


def test_bad_arguments_raise():
    import factormodeling_amd.engine as E
    x = _dev(C.make_values(1, 8, 4, 2))
    with pytest.raises(Exception):
        E.ts_order("median", x, 0)
    with pytest.raises(ValueError):
        E.ts_order("quantile", x, 3, q=1.5)
    with pytest.raises(ValueError):
        E.ts_order("quantile", x, 3, interpolation="cubic")
