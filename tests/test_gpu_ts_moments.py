"""Rolling higher moments on the GPU (fmx_ts_moment through engine.ts_moment and the drop-in
ts_skew / ts_kurt / ts_cov) against the numpy reference of ts_moments_cases.py, bit-exact as
values over the whole [F][D][A] output (``np.array_equal(..., equal_nan=True)``).
tests/test_ts_moments_host.py pins that reference to pandas on the same panels and windows and
proves that each panel holds the cells it was built for.  Every output buffer goes in filled
with 12345.0, which must not survive."""
import functools

import numpy as np
import pandas as pd
import pytest

import ts_moments_cases as C

pytestmark = pytest.mark.gpu

FILL = 12345.0


def _dev(a, dtype=None):
    import torch
    if a is None:
        return None
    t = torch.as_tensor(np.array(a, order="C"), device="cuda")           # a writable copy
    return t.to(dtype) if dtype else t


def gpu(x, present, op, W, y=None):
    import torch
    import factormodeling_amd.engine as E
    X = _dev(x)
    out = torch.full_like(X, FILL)
    got = E.ts_moment(op, X, W, _dev(present, torch.uint8), _dev(y) if op == "cov" else None, out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    return got.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _ref(key, op, W):
    """One reference per (panel, op, W), shared by the tests and never written to."""
    x, present, y = PANELS[key]()
    r = C.ref_panel(x, present, op, W, y if op == "cov" else None)
    r.setflags(write=False)
    return r


def check(key, op, W, y=None):
    x, present, y0 = PANELS[key]()
    ref = _ref(key, op, W) if y is None else C.ref_panel(x, present, op, W, y)
    got = gpu(x, present, op, W, y0 if y is None else y)
    assert not (got == FILL).any(), (key, op, W)
    bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
    assert np.array_equal(got, ref, equal_nan=True), \
        (key, op, W, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5], ref[bad][:5])
    return got, ref


# ------------------------------------------------------------------------------------ panels
@functools.lru_cache(maxsize=None)
def main_panel(ragged):
    x, present = C.make_panel(C.F, C.D, C.A, 11, ragged)
    return x, present, C.make_y(C.D, C.A, 11)


@functools.lru_cache(maxsize=None)
def asset_panel(A_, ragged):
    return (C.make_values(2, 20, A_, 20 + A_), C.edge_present(20, A_, A_) if ragged else None,
            C.make_y(20, A_, 20 + A_))


@functools.lru_cache(maxsize=None)
def date_panel(Dn, ragged):
    return (C.make_values(2, Dn, 70, 30 + Dn, nan_frac=0.0), C.edge_present(Dn, 70, Dn) if ragged else None,
            C.make_y(Dn, 70, 30 + Dn))


@functools.lru_cache(maxsize=None)
def content(W, ragged):
    x, present = C.content_panel(W, ragged)
    return x, present, C.content_y(W, ragged)


class _Panels(dict):
    def __missing__(self, key):
        kind, *args = key
        fn = {"main": main_panel, "asset": asset_panel, "date": date_panel, "content": content}[kind]
        return lambda: fn(*args)


PANELS = _Panels()


# ------------------------------------------------------------------------------------ main panel
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("W", C.WINDOWS)
def test_main_panel(W, ragged):
    for op in C.OPS:
        _, ref = check(("main", ragged), op, W)
        assert np.isfinite(ref).any() == (C.MIN_W[op] <= W <= C.D), (op, W)


# ------------------------------------------------------------------------------------ edge shapes
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("A_", C.EDGE_ASSETS)
def test_asset_edges(A_, ragged):
    for W in C.EDGE_WINDOWS:
        for op in C.OPS:
            check(("asset", A_, ragged), op, W)


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("W", C.DATE_WINDOWS)
def test_date_edges(W, ragged):
    """D = 1, around the 8-date register batch (7, 8, 9, 15, 16, 17: the tail loop runs 7, 0, 1
    rows after zero, one or two whole batches) and around the window (W, W + 1, 2W + 3)."""
    for Dn in C.date_edges(W):
        for op in C.OPS:
            check(("date", Dn, ragged), op, W)


# ------------------------------------------------------------------------------------ content
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("W", C.CONTENT_WINDOWS)
def test_content_columns(W, ragged):
    """Constant column and run (0.0 / -3.0), B <= 1e-14 (NaN), centred and uncentred columns, the
    half-away rounding of dyadic means, +-0.0, NaN and +-inf entering and leaving, all-NaN and
    one-valid columns, 1e60 / 1e-60 scales; ragged: +inf / 12345.0 under absent cells, an absent
    first row, a symbol with W - 1 rows and one never present (test_ts_moments_host.py asserts
    that each of these cells is there)."""
    for op in ("skew", "kurt"):
        got, _ = check(("content", W, ragged), op, W)
        if not ragged and W >= C.MIN_W[op]:
            assert (got[0, W - 1:, C.CONTENT.index("const")] == (0.0 if op == "skew" else -3.0)).all()


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("W", C.COV_WINDOWS)
def test_cov_shared_and_per_column_y(W, ragged):
    """NaN / +-inf in x only, in y only and in both; the shared [D][A] y and the per-column
    [F][D][A] y agree with the reference, and a broadcast y with the shared one in bits."""
    key = ("content", 5, ragged)
    x, present, y = PANELS[key]()
    shared, _ = check(key, "cov", W)
    yb = np.ascontiguousarray(np.broadcast_to(y, x.shape))
    assert gpu(x, present, "cov", W, yb).tobytes() == shared.tobytes()
    # a different partner per column of a 3-column batch
    x3 = np.concatenate([x, x[:, ::-1], 2.0 * x])
    y3 = np.stack([y, y[::-1], -y])
    ref = C.ref_panel(x3, present, "cov", W, y3)
    got = gpu(x3, present, "cov", W, y3)
    assert np.array_equal(got, ref, equal_nan=True) and not (got == FILL).any()
    assert np.isfinite(ref).any() == (W >= 2)


def test_main_panel_per_column_y():
    x, present, _ = main_panel(True)
    y3 = C.make_y(C.D, C.A, 12, per_column=C.F)
    for W in (5, 20):
        ref = C.ref_panel(x, present, "cov", W, y3)
        got = gpu(x, present, "cov", W, y3)
        assert np.array_equal(got, ref, equal_nan=True) and np.isfinite(ref).any()


# ------------------------------------------------------------------------------------ batch
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
def test_batch_independence(ragged):
    """A column alone equals the column in the batch, bytes for bytes."""
    x, present, y = main_panel(ragged)
    for op in C.OPS:
        full = gpu(x, present, op, 9, y)
        for f in range(C.F):
            alone = gpu(x[f:f + 1], present, op, 9, y)
            assert alone[0].tobytes() == full[f].tobytes(), (op, f)


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
    ydf = pd.DataFrame({f"f{k}": v.reshape(-1)[sel] for k, v in enumerate(C.make_y(Dn, An, 21, per_column=3))},
                       index=idx)
    s = df["f1"].rename("alpha")
    sy = ydf["f0"].rename("mkt")
    for W in (4, 9):
        for op, fn in (("skew", ops.ts_skew), ("kurt", ops.ts_kurt)):
            got = fn(s, W)
            assert isinstance(got, pd.Series) and got.name == "alpha"
            _same(got, C.pandas_op(s, op, W))
            gdf = fn(df, W)
            assert isinstance(gdf, pd.DataFrame) and list(gdf.columns) == list(df.columns)
            _same(gdf, C.pandas_op(df, op, W))
        got = ops.ts_cov(s, sy, W)
        assert isinstance(got, pd.Series) and got.name == "alpha"
        _same(got, C.pandas_op(s, "cov", W, sy))
        got = ops.ts_cov(s, sy.iloc[::-1], W)               # y is aligned to x's index
        _same(got, C.pandas_op(s, "cov", W, sy))
        for yy in (sy, ydf):                                # shared and per-column partner
            gdf = ops.ts_cov(df, yy, W)
            assert isinstance(gdf, pd.DataFrame) and list(gdf.columns) == list(df.columns)
            _same(gdf, C.pandas_op(df, "cov", W, yy))


def test_bad_arguments_raise():
    import factormodeling_amd.engine as E
    from factormodeling_amd import _lib
    x = _dev(C.make_values(1, 8, 4, 2))
    with pytest.raises(ValueError):
        E.ts_moment("skew", x, 0)
    with pytest.raises(ValueError):
        E.ts_moment("median", x, 3)
    with pytest.raises(ValueError):
        E.ts_moment("cov", x, 3)
    with pytest.raises(_lib.FmxError):
        E.ts_moment("cov", x, 3, y=x[0, :4])
    with pytest.raises(_lib.FmxError):
        E.ts_moment("cov", x, 3, y=x[0].float())
