"""Exponentially weighted operators on the GPU (fmx_ts_ewm through engine.ts_ewm and the six
drop-in operators) against the numpy restatement of ts_ewm_cases.py, bit-exact as values
(``np.array_equal(..., equal_nan=True)``).  tests/test_ts_ewm_host.py pins that reference to
pandas."""
import functools

import numpy as np
import pandas as pd
import pytest

import ts_ewm_cases as C

pytestmark = pytest.mark.gpu

F, D, A = 3, 75, 130              # D: no multiple of the prefetch batch; A: two waves + two lanes


def _dev(a, dtype=None):
    import torch
    if a is None:
        return None
    t = torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    return t.to(dtype) if dtype else t


def gpu(x, y, present, com, adjust=True, ignore_na=False, min_periods=0, want=C.OUTS):
    import torch
    import factormodeling_amd.engine as E
    outs = E.ts_ewm(_dev(x), {k: None for k in want}, com, adjust, ignore_na, min_periods,
                    _dev(present, torch.uint8), _dev(y))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


def check(x, y, present, com, adjust=True, ignore_na=False, min_periods=0, want=C.OUTS, finite=("mean",)):
    ref = C.ref_panel(x, y, present, com, adjust, ignore_na, min_periods, want)
    got = gpu(x, y, present, com, adjust, ignore_na, min_periods, want)
    for k in want:
        if k in finite and (com > 0 or k == "mean"):              # alpha = 1 forgets: no variance anywhere
            assert np.isfinite(ref[k]).any(), k                   # there is something to compare
        g, r = got[k], ref[k]
        bad = ~((g == r) | (np.isnan(g) & np.isnan(r)))
        assert np.array_equal(g, r, equal_nan=True), \
            (k, com, adjust, ignore_na, min_periods, int(bad.sum()), np.argwhere(bad)[:5].tolist(), g[bad][:5],
             r[bad][:5])
    return got


def check_grid(x, y, present, decays=(("span", 20), ("com", 0)), minps=(1,), finite=("mean",)):
    for kind, v, adjust, ignore_na, mp in C.grid(decays, minps):
        check(x, y, present, C.com_of(kind, v), adjust, ignore_na, mp, finite=finite)


@functools.lru_cache(maxsize=None)
def main_panel():
    return C.make_pair(F, D, A, 11)


# ------------------------------------------------------------------------------------ main panel
@pytest.mark.parametrize("decay", C.DECAYS_GPU, ids=C.decay_id)
def test_main_panel(decay):
    x, y = main_panel()
    check_grid(x, y, None, (decay,), (1, 5), finite=C.OUTS)


# ------------------------------------------------------------------------------------ edge shapes
@pytest.mark.parametrize("A_", [1, 63, 64, 65])
def test_asset_edges(A_):
    x, y = C.make_pair(2, 20, A_, 20 + A_)
    check_grid(x, y, None, finite=("mean", "var", "corr"))
    check_grid(x, y, C.make_present(20, A_, A_) if A_ > 1 else None)


@pytest.mark.parametrize("D_", [1, 2])
def test_short_histories(D_):
    x, y = C.make_pair(2, D_, 70, 3 + D_, nan_frac=0.1)
    check_grid(x, y, None, (("span", 3), ("com", 0)), (0, 1))
    check_grid(x, y, None, (("span", 3),), (2,), finite=("mean",) if D_ >= 2 else ())


@pytest.mark.parametrize("D_", [C.PREFETCH - 1, C.PREFETCH, C.PREFETCH + 1, 2 * C.PREFETCH, 2 * C.PREFETCH + 1])
def test_prefetch_edges(D_):
    """The batch edges and the remainder of the row loop."""
    x, y = C.make_pair(2, D_, 70, 40 + D_)
    check_grid(x, y, None, (("span", 5),), finite=("mean", "var", "corr"))
    check_grid(x, y, C.make_present(D_, 70, D_), (("span", 5),))


# ------------------------------------------------------------------------------------ content
@pytest.mark.parametrize("adjust", [True, False])
@pytest.mark.parametrize("ignore_na", [False, True])
def test_long_nan_run(adjust, ignore_na):
    """A NaN run of 1,200 rows at alpha 0.5, D = 1,300, A = 64: old_wt passes through the
    subnormals to 0, and the GPU's subnormals must be the host's.  Lanes differ in where the
    run starts."""
    Dn, An = 1300, 64
    x0, y0 = C.nan_run_column(Dn)
    rng = np.random.default_rng(5)
    x = np.repeat(x0[None, :, None], An, axis=2) * (1 + np.arange(An))[None, None, :]
    x[0, 30:40, :] = rng.standard_normal((10, An))
    for a in range(An):
        x[0, 40:40 + a, a] = 1.0                                  # the run is 1,200 - a rows long
    y = np.repeat(y0[:, None], An, axis=1)
    assert np.isnan(x[0, 110:1240]).all()
    got = check(x, y, None, C.com_of("alpha", 0.5), adjust, ignore_na, 1, finite=C.OUTS)
    assert np.isfinite(got["mean"][0, 1241:]).all() and np.isfinite(got["corr"][0, 1245:]).any()


def test_special_columns():
    """0 / 5 / 15 % NaN, leading NaNs, a constant stretch and a constant column (the != guard),
    +-inf cells in x and y, all-NaN columns."""
    xs, ys = C.special_columns(75, 175)
    x = np.concatenate([xs, np.full((75, 2), np.nan), xs[:, :1]], axis=1)[None]
    y = np.concatenate([ys, ys[:, :1], np.full((75, 2), np.nan)], axis=1)       # all-NaN x, all-NaN y
    check_grid(x, y, None, (("span", 20), ("alpha", 0.03), ("halflife", 0.5)), (0, 5), finite=C.OUTS)
    got = gpu(x, y, None, C.com_of("alpha", 0.03))
    assert (got["mean"][0, :, 6] == 1.25).all() and (got["var"][0, 1:, 6] == 0.0).all()
    assert np.isnan(got["mean"][0, :, 7:9]).all() and np.isnan(got["corr"][0, :, 7:]).all()
    xn, yn = np.where(np.isinf(x), np.nan, x), np.where(np.isinf(y), np.nan, y)
    clean = gpu(xn, yn, None, C.com_of("alpha", 0.03), want=C.PANDAS_OUTS)      # +-inf behave as NaN
    for k in C.PANDAS_OUTS:
        assert np.array_equal(got[k], clean[k], equal_nan=True), k


# ------------------------------------------------------------------------------------ ragged
def test_ragged_panel():
    """Late listings, gaps and a symbol with one row: the kernel matches the reference on each
    symbol's own rows, and differs from the same data run dense with the gaps as NaN rows."""
    x, y = main_panel()
    present = C.make_present(D, A, 11)
    assert present[:, A - 1].sum() == 1 and (present.argmax(axis=0) > 0).any()
    check_grid(x, y, present, C.DECAYS_GPU[:2], (1, 5), finite=C.OUTS)
    com = C.com_of("span", 20)
    xf = np.where(np.isnan(x), 0.5, x)                             # the only NaN rows are the gaps
    ragged = gpu(xf, y, present, com, want=("mean", "var"))
    dense = gpu(np.where(present[None], xf, np.nan), y, None, com, want=("mean", "var"))
    for k in ("mean", "var"):
        assert np.isnan(ragged[k][:, ~present]).all()
        both = np.broadcast_to(present, x.shape) & np.isfinite(ragged[k]) & np.isfinite(dense[k])
        gaps = (present.cumsum(axis=0) > 0) & ~present            # absent cells after the listing
        gapped = np.broadcast_to(gaps.cumsum(axis=0) > 0, x.shape) & both         # rows after a symbol's first gap
        assert gapped.any() and (ragged[k][gapped] != dense[k][gapped]).mean() > 0.9, k
    skip = gpu(np.where(present[None], xf, np.nan), y, None, com, ignore_na=True, want=("mean",))["mean"]
    assert np.array_equal(skip[:, present], ragged["mean"][:, present])


# ------------------------------------------------------------------------------------ fused
def test_fused_equals_single_outputs():
    x, y = main_panel()
    y = y.copy()
    y[np.isnan(x[0])] = 1.0
    y[~np.isnan(x[0]) & (np.random.default_rng(2).random((D, A)) < 0.1)] = np.nan   # y NaN where x is not
    present = C.make_present(D, A, 12)
    for pres in (None, present):
        for adjust in (True, False):
            com = C.com_of("halflife", 10)
            fused = gpu(x, y, pres, com, adjust, False, 3)
            for k in C.OUTS:
                single = gpu(x, y, pres, com, adjust, False, 3, want=(k,))[k]
                assert np.array_equal(fused[k], single, equal_nan=True), (k, adjust)
            check(x, y, pres, com, adjust, False, 3, want=("cov", "corr"), finite=("cov", "corr"))


# ------------------------------------------------------------------------------------ drop-in
def _same(got, ref):
    assert np.array_equal(got.to_numpy(), ref.to_numpy(), equal_nan=True)
    assert got.index.equals(ref.index)
    assert np.isfinite(ref.to_numpy()).any()


def test_dropin_operators_against_pandas():
    import factormodeling_amd.operations as ops
    Dn, An = 40, 30
    x, y = C.make_pair(3, Dn, An, 21)
    present = C.make_present(Dn, An, 21)
    idx = C.panel_index(Dn, An, present)
    sel = present.reshape(-1)
    df = pd.DataFrame({f"f{k}": x[k].reshape(-1)[sel] for k in range(3)}, index=idx)
    s = df["f1"].rename("alpha")
    sy = pd.Series(y.reshape(-1)[sel], index=idx, name="mkt").sample(frac=1.0, random_state=0)   # aligned by index
    for kw in (dict(span=20), dict(halflife=0.5, adjust=False, min_periods=3), dict(com=7.3, ignore_na=True),
               dict(alpha=0.03, adjust=False, ignore_na=True, min_periods=5)):
        kind, v = next((k, kw[k]) for k in ("com", "span", "halflife", "alpha") if k in kw)
        pa = (kind, v, kw.get("adjust", True), kw.get("ignore_na", False), kw.get("min_periods", 0))
        for out in C.OUTS:
            fn = getattr(ops, "ts_ewm_" + out)
            extra = (sy,) if out in C.PAIR else ()
            got = fn(s, *extra, **kw)
            assert isinstance(got, pd.Series) and got.name == "alpha"
            _same(got, C.pandas_grouped(s, sy, out, *pa))
            if out in ("mean", "var", "std"):
                _same(got, C.pandas_groupby_ewm(s, out, *pa))
            gdf = fn(df, *extra, **kw)
            assert isinstance(gdf, pd.DataFrame) and list(gdf.columns) == list(df.columns)
            _same(gdf, C.pandas_grouped(df, sy, out, *pa))


def test_bad_arguments_raise():
    import factormodeling_amd.engine as E
    from factormodeling_amd._lib import FmxError
    x = _dev(C.make_values(1, 8, 4, 2))
    y = _dev(C.make_values(1, 8, 4, 3)[0])
    for outs, kw in (({}, {}), ({"median": None}, {}), ({"mean": None}, dict(com=-1.0)),
                     ({"mean": None}, dict(com=float("nan"))), ({"mean": None}, dict(min_periods=-2)),
                     ({"cov": None}, {}), ({"mean": None, "corr": None}, {})):
        args = dict(com=3.0)
        args.update(kw)
        with pytest.raises(ValueError):
            E.ts_ewm(x, outs, **args)
    with pytest.raises(FmxError):
        E.ts_ewm(x, {"corr": None}, 3.0, y=y[:4])
    with pytest.raises(FmxError):
        E.ts_ewm(x, {"mean": x}, 3.0)                              # an output may not alias X
    got = E.ts_ewm(x, {"corr": None}, 3.0, y=y)["corr"]
    assert tuple(got.shape) == (1, 8, 4)
