"""Exponentially weighted operators without a GPU: the numpy restatement of ts_ewm_cases.py
against pandas bit for bit (NaN positions equal, other values equal as int64 views; this pins
the recursions the kernels implement), the public surface, and the host-side argument checks
of fmx_ts_ewm and the operators."""
import ctypes
import importlib
import inspect
import os
import sys

import numpy as np
import pandas as pd
import pytest

import ts_ewm_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ts_ewm_mean", "ts_ewm_var", "ts_ewm_std", "ts_ewm_zscore", "ts_ewm_cov", "ts_ewm_corr")
LENGTHS = (1, 2, 75, 300)
MINPS = (0, 1, 5)


def _lib():
    from factormodeling_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libfmx.so not built (run __graft_entry__.build())")
    return L.load()


@pytest.fixture(scope="module")
def columns():
    cols = {n: C.special_columns(n, 100 + n) for n in LENGTHS}
    x, y = cols[300]
    assert not np.isnan(x[:, 0]).any() and 0.01 < np.isnan(x[:, 1]).mean() < np.isnan(x[:, 2]).mean()
    assert (np.isnan(x[:, 2]) != np.isnan(y[:, 2])).any()          # placed independently
    assert np.isnan(x[:3, 3]).all() and np.isinf(x[:, 5]).sum() == 2 and np.isinf(y[:, 5]).sum() == 2
    assert (x[10:30, 4] == x[10, 4]).all() and (x[:, 4] * 4 % 1 == 0).all()
    return cols


# ------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("decay", C.DECAYS, ids=C.decay_id)
def test_reference_equals_pandas_per_column(columns, decay):
    """Series.ewm, column by column: five outputs x adjust x ignore_na x min_periods."""
    kind, v = decay
    for n in LENGTHS:
        x, y = columns[n]
        sx = [pd.Series(x[:, c]) for c in range(x.shape[1])]
        sy = [pd.Series(y[:, c]) for c in range(x.shape[1])]
        for _, _, adjust, ignore_na, mp in C.grid((decay,), MINPS):
            ref = C.ref_panel(x[None], y, None, C.com_of(kind, v), adjust, ignore_na, mp)
            for c in range(x.shape[1]):
                for out in C.PANDAS_OUTS:
                    pdv = C.pandas_series(sx[c], sy[c], out, kind, v, adjust, ignore_na, mp)
                    assert C.same_bits(ref[out][0, :, c], pdv), (n, c, out, kind, v, adjust, ignore_na, mp)
            with np.errstate(all="ignore"):
                z = (x - ref["mean"][0]) / ref["std"][0]
            assert C.same_bits(ref["zscore"][0], z)
    assert np.isfinite(ref["mean"]).any()
    if C.com_of(kind, v) > 0:                            # alpha = 1 forgets everything: no variance
        assert np.isfinite(ref["corr"]).any() and np.isfinite(ref["var"]).any()


def test_infinities_behave_as_nan(columns):
    x, y = columns[75]
    xn, yn = np.where(np.isinf(x), np.nan, x), np.where(np.isinf(y), np.nan, y)
    a = C.ref_panel(x[None], y, None, 3.0, want=C.PANDAS_OUTS)
    b = C.ref_panel(xn[None], yn, None, 3.0, want=C.PANDAS_OUTS)
    assert np.isinf(x).any() and np.isinf(y).any()
    for k in C.PANDAS_OUTS:
        assert C.same_bits(a[k], b[k]), k


@pytest.mark.parametrize("adjust", [True, False])
@pytest.mark.parametrize("ignore_na", [False, True])
def test_long_nan_run_equals_pandas(adjust, ignore_na):
    """A NaN run of 1,200 rows at alpha 0.5: old_wt passes through the subnormals to 0."""
    x, y = C.nan_run_column()
    assert np.isnan(x[40:1240]).all() and 0.5 ** 1100 == 0.0
    ref = C.ref_panel(x[None, :, None], y[:, None], None, C.com_of("alpha", 0.5), adjust, ignore_na, 1)
    for out in C.PANDAS_OUTS:
        pdv = C.pandas_series(pd.Series(x), pd.Series(y), out, "alpha", 0.5, adjust, ignore_na, 1)
        assert C.same_bits(ref[out][0, :, 0], pdv), out
        assert np.isfinite(pdv[1240:]).any()


@pytest.mark.parametrize("decay", C.DECAYS, ids=C.decay_id)
def test_reference_equals_pandas_on_the_ragged_panel(decay):
    """groupby(level="symbol").ewm on a panel with late listings, gaps and a one-row symbol."""
    kind, v = decay
    D, A = 40, 9
    x, y = C.make_pair(1, D, A, 3)
    present = C.make_present(D, A, 3)
    assert present[:, A - 1].sum() == 1 and (present.argmax(axis=0) > 0).any() and not present[:, 1:3].all()
    s, sy = C.to_series(x[0], present), C.to_series(y, present, "y")
    for _, _, adjust, ignore_na, mp in C.grid((decay,), MINPS):
        ref = C.ref_panel(x, y, present, C.com_of(kind, v), adjust, ignore_na, mp)
        for out in C.OUTS:
            pdv = C.from_series(C.pandas_grouped(s, sy, out, kind, v, adjust, ignore_na, mp), D, A, present)
            assert C.same_bits(ref[out][0], pdv), (out, kind, v, adjust, ignore_na, mp)
            if out in ("mean", "var", "std"):
                gb = C.from_series(C.pandas_groupby_ewm(s, out, kind, v, adjust, ignore_na, mp), D, A, present)
                assert C.same_bits(ref[out][0], gb), (out, kind, v, adjust, ignore_na, mp)
    assert np.isfinite(ref["mean"]).any() and (C.com_of(kind, v) == 0 or np.isfinite(ref["corr"]).any())


def test_absent_cells_are_not_nan_rows():
    """The row rule: the same data dense, with the gaps as NaN rows, decays where the ragged
    panel does not."""
    D, A = 40, 9
    x, y = C.make_pair(1, D, A, 3, nan_frac=0.0)
    present = C.make_present(D, A, 3)
    ragged = C.ref_panel(x, y, present, 3.0, want=("mean",))["mean"]
    dense = C.ref_panel(np.where(present, x, np.nan), y, None, 3.0, want=("mean",))["mean"]
    both = present[None] & np.isfinite(ragged) & np.isfinite(dense)
    assert (ragged[both] != dense[both]).any()
    same = C.ref_panel(np.where(present, x, np.nan), y, None, 3.0, ignore_na=True, want=("mean",))["mean"]
    assert np.array_equal(ragged[present[None]], same[present[None]], equal_nan=True)


def test_the_constant_guard_changes_bits():
    """Without `if weighted != cur`, a constant series drifts off its value."""
    alpha, w, ow, drift = 0.03, 0.1, 1.0, False
    for _ in range(200):
        ow *= 1.0 - alpha
        w = ((ow * w) + (1.0 * 0.1)) / (ow + 1.0)
        ow += 1.0
        drift |= w != 0.1
    assert drift
    ref = C.ref_panel(np.full((1, 200, 1), 0.1), None, None, C.com_of("alpha", alpha), want=("mean",))["mean"]
    assert (ref == 0.1).all()


# ------------------------------------------------------------------------------------ 2
def test_api_present():
    """The surface the feature adds (fails without it)."""
    import factormodeling_amd.engine as E
    import factormodeling_amd.operations as ops
    from factormodeling_amd import _lib as L
    with open(os.path.join(ROOT, "include", "fmx.h")) as f:
        header = f.read()
    assert "fmx_status fmx_ts_ewm(" in header
    assert "#define FMX_ABI_VERSION 1\n" in header
    for name, code in L.EWM.items():
        assert f"#define FMX_EWM_{name.upper()} {code}\n" in header
    assert L.SIGNATURES["fmx_ts_ewm"] == [L.c_vp] * 8 + [L.c_i64] * 4 + [L.c_dbl, L.c_i32, L.c_i32, L.c_i32, L.c_vp,
                                                                         L.c_vp]
    assert hasattr(_lib(), "fmx_ts_ewm")
    with open(os.path.join(ROOT, "factormodeling_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert "ts_ewm.hip" in mk and "-ffp-contract=off -fno-fast-math" in mk
    assert list(inspect.signature(E.ts_ewm).parameters) == ["X", "outs", "com", "adjust", "ignore_na", "min_periods",
                                                            "present", "y"]
    for n in NAMES:
        assert n in ops.__all__ and callable(getattr(ops, n))
        params = inspect.signature(getattr(ops, n)).parameters
        lead = ["x", "y"] if n in ("ts_ewm_cov", "ts_ewm_corr") else ["x"]
        assert list(params) == lead + ["com", "span", "halflife", "alpha", "adjust", "ignore_na", "min_periods"]
        assert params["adjust"].default is True and params["ignore_na"].default is False
        assert params["min_periods"].default == 0 and "times" not in params


def test_dropin_exports_the_six():
    dropin = os.path.join(ROOT, "factormodeling_amd", "dropin")
    sys.path.insert(0, dropin)
    try:
        sys.modules.pop("operations", None)
        m = importlib.import_module("operations")
        assert m.__file__.startswith(dropin)
        for n in NAMES:
            assert hasattr(m, n) and n in m.__all__
    finally:
        sys.path.remove(dropin)
        sys.modules.pop("operations", None)


def test_decay_parameter_follows_pandas():
    """The operators' helper gives com_of's centre of mass, which the tests above hand to the
    reference while pandas gets the parameter itself."""
    from factormodeling_amd.operations import _ewm_com
    for kind, v in C.DECAYS + (("span", 1), ("alpha", 1.0), ("halflife", 1e-3), ("com", 1e6)):
        kw = dict(com=None, span=None, halflife=None, alpha=None)
        kw[kind] = v
        got = _ewm_com(**kw)
        assert isinstance(got, float) and got == C.com_of(kind, v)


# ------------------------------------------------------------------------------------ 3
def test_bad_arguments_fail_before_device_work():
    """Empty panels (F = D = A = 0: a valid call returns before any launch) with host buffers
    as the panel pointers: every bad argument is refused with FMX_ERR_ARG and a message."""
    lib = _lib()
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(X=p, Y=None, outs=(p, None, None, None, None, None), ld=0, com=3.0, minp=0):
        return lib.fmx_ts_ewm(X, Y, *outs, 0, 0, 0, ld, com, 1, 0, minp, None, None)

    assert call() == 0                                   # the checks pass on good arguments
    assert call(Y=p, outs=(p, p, p, p, p, p)) == 0
    assert call(com=0.0) == 0
    for kw, msg in ((dict(X=None), b"null"), (dict(ld=-1), b"dims"), (dict(com=-0.5), b"com"),
                    (dict(com=float("nan")), b"com"), (dict(minp=-1), b"min_periods"),
                    (dict(outs=(None,) * 6), b"no output"), (dict(outs=(None, None, None, None, p, None)), b"Ycol"),
                    (dict(outs=(p, None, None, None, None, p)), b"Ycol")):
        assert call(**kw) == 1, kw
        assert msg in lib.fmx_last_error(), (kw, lib.fmx_last_error())


def test_python_argument_checks():
    """Raised by the operators themselves, before any device work (no GPU needed)."""
    import factormodeling_amd.operations as ops
    s = C.to_series(C.make_values(1, 6, 3, 1)[0], None)
    for kw in (dict(), dict(com=1.0, span=3), dict(alpha=0.5, halflife=2), dict(com=-0.1), dict(span=0.5),
               dict(halflife=0), dict(halflife=-1.0), dict(alpha=0.0), dict(alpha=1.5), dict(alpha=-0.2),
               dict(com=float("nan")), dict(span=3, min_periods=-1)):
        for n in NAMES:
            args = (s, s) if n in ("ts_ewm_cov", "ts_ewm_corr") else (s,)
            with pytest.raises(ValueError):
                getattr(ops, n)(*args, **kw)
    for kw in (dict(), dict(com=1.0, span=3), dict(com=-0.1), dict(span=0.5), dict(halflife=0), dict(alpha=1.5)):
        with pytest.raises(ValueError):                  # pandas raises the same way
            s.ewm(**kw)
    with pytest.raises(TypeError):
        ops.ts_ewm_mean(s, span=3, times=s.index.get_level_values("date"))


def test_no_gpu_raises():
    """No host fallback: without a HIP device the operators raise FmxError."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import factormodeling_amd.operations as ops
    from factormodeling_amd._lib import FmxError
    s = C.to_series(C.make_values(1, 6, 3, 1)[0], None)
    for n in NAMES:
        args = (s, s) if n in ("ts_ewm_cov", "ts_ewm_corr") else (s,)
        with pytest.raises(FmxError):
            getattr(ops, n)(*args, span=3)
