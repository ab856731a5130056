"""Rolling order statistics without a GPU: the brute-force reference of ts_order_cases.py
against pandas bit for bit (this pins the median / quantile / argmin formulas the kernels
implement), the public surface, and the host-side argument checks of fmx_ts_order."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pandas as pd
import pytest

import ts_order_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, A = 48, 9
WINDOWS = (1, 2, 3, 5, 8, 20)


def _lib():
    from factormodeling_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libfmx.so not built (run __graft_entry__.build())")
    return L.load()


@pytest.fixture(scope="module", params=[False, True], ids=["dense", "ragged"])
def panel(request):
    x, present = C.make_panel(1, D, A, 5, request.param)
    if present is not None:
        assert present[:, A - 1].sum() == 2                        # a symbol with fewer rows than W
        first = present.argmax(axis=0)
        assert (first > 0).any()                                   # late listings
        assert any((~present[first[a]:, a]).any() for a in range(A - 1))   # gaps after listing
        assert present.sum(axis=0).min() < min(w for w in WINDOWS if w > 2)
    assert np.isnan(x).mean() > 0.005 and (x[np.isfinite(x)] * 4 % 1 == 0).all()
    return x, present, C.to_series(x[0], present)


def _check(panel, op, W, q=0.5, interpolation="linear"):
    x, present, s = panel
    ref = C.ref_panel(x, present, op, W, q, interpolation)[0]
    pdv = C.from_series(C.pandas_op(s, op, W, q, interpolation), D, A, present)
    assert C.has_finite(ref)
    assert np.array_equal(ref, pdv, equal_nan=True), (op, W, q, interpolation)


@pytest.mark.parametrize("op", ["min", "max", "argmin", "argmax", "median"])
def test_reference_equals_pandas(panel, op):
    for W in WINDOWS:
        _check(panel, op, W)


@pytest.mark.parametrize("interpolation", C.INTERPOLATIONS)
def test_reference_quantile_equals_pandas(panel, interpolation):
    for W in WINDOWS:
        for q in (0.0, 0.1, 0.25, 0.5, 0.7, 0.99, 1.0):
            _check(panel, "quantile", W, q, interpolation)


def test_median_is_not_the_half_quantile_formula():
    """Even windows: (v[W/2] + v[W/2 - 1]) / 2 against v[i] + (v[i + 1] - v[i]) * 0.5."""
    x = np.array([[0.1], [0.7]])
    assert C.ref_dense(x, "median", 2)[1, 0] == (0.7 + 0.1) / 2
    assert C.ref_dense(x, "quantile", 2, 0.5)[1, 0] == 0.1 + (0.7 - 0.1) * 0.5


def test_argmin_ties_go_to_the_most_recent_row():
    x = np.array([[1.0], [0.0], [-0.0], [0.0], [2.0]])
    assert C.ref_dense(x, "argmin", 5)[4, 0] == 1.0
    assert C.ref_dense(x, "argmax", 3)[3, 0] == 0.0


# ------------------------------------------------------------------------------------ 2
def test_api_present():
    """The surface the feature adds (fails without it)."""
    import inspect
    import factormodeling_amd.engine as E
    import factormodeling_amd.operations as ops
    from factormodeling_amd import _lib as L
    with open(os.path.join(ROOT, "include", "fmx.h")) as f:
        header = f.read()
    assert "fmx_status fmx_ts_order(" in header
    for name in ("MIN", "MAX", "ARGMIN", "ARGMAX", "MEDIAN", "QUANTILE", "LINEAR", "LOWER", "HIGHER", "MIDPOINT",
                 "NEAREST"):
        assert f"#define FMX_TSO_{name} " in header
    for name, code in list(L.TSO.items()) + list(L.TSO_INTERP.items()):        # the Python tables mirror it
        define = f"#define FMX_TSO_{name.upper()} {code}"
        assert define + " " in header or define + "\n" in header, define
    assert L.SIGNATURES["fmx_ts_order"] == [L.c_i32, L.c_vp, L.c_vp, L.c_i64, L.c_i64, L.c_i64, L.c_i64, L.c_i32,
                                            L.c_dbl, L.c_i32, L.c_vp, L.c_vp]
    assert hasattr(_lib(), "fmx_ts_order")
    with open(os.path.join(ROOT, "factormodeling_amd", "csrc", "Makefile")) as f:
        assert "ts_order.hip" in f.read()
    assert list(inspect.signature(E.ts_order).parameters) == ["op", "X", "window", "present", "q", "interpolation",
                                                              "out"]
    for n in ("ts_min", "ts_max", "ts_argmin", "ts_argmax", "ts_median", "ts_quantile"):
        assert n in ops.__all__ and callable(getattr(ops, n))
    assert list(inspect.signature(ops.ts_quantile).parameters) == ["series", "window", "q", "interpolation"]
    assert inspect.signature(ops.ts_quantile).parameters["interpolation"].default == "linear"


def test_dropin_exports_the_six():
    dropin = os.path.join(ROOT, "factormodeling_amd", "dropin")
    sys.path.insert(0, dropin)
    try:
        sys.modules.pop("operations", None)
        m = importlib.import_module("operations")
        assert m.__file__.startswith(dropin)
        for n in ("ts_min", "ts_max", "ts_argmin", "ts_argmax", "ts_median", "ts_quantile"):
            assert hasattr(m, n) and n in m.__all__
    finally:
        sys.path.remove(dropin)
        sys.modules.pop("operations", None)


# ------------------------------------------------------------------------------------ 3
def test_bad_arguments_fail_before_device_work():
    """Empty panels (F = D = A = 0: a valid call returns before any launch) with host buffers
    as the panel pointers: every bad argument is refused with FMX_ERR_ARG and a message."""
    lib = _lib()
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(op, window, q, interp, X=p, Y=p, ld=0):
        return lib.fmx_ts_order(op, X, Y, 0, 0, 0, ld, window, q, interp, None, None)

    assert call(5, 20, 0.5, 0) == 0                      # the checks pass on good arguments
    for args, msg in (((0, 0, 0.5, 0), b"window"), ((4, -3, 0.5, 0), b"window"), ((6, 5, 0.5, 0), b"unknown ts order op"),
                      ((-1, 5, 0.5, 0), b"unknown ts order op"), ((5, 5, 1.5, 0), b"quantile"),
                      ((5, 5, -0.1, 0), b"quantile"), ((5, 5, float("nan"), 0), b"quantile"),
                      ((5, 5, 0.5, 5), b"interpolation"), ((5, 5, 0.5, -1), b"interpolation")):
        assert call(*args) == 1, args
        assert msg in lib.fmx_last_error(), (args, lib.fmx_last_error())
    assert call(0, 5, 0.5, 0, X=None) == 1 and b"null" in lib.fmx_last_error()
    assert call(0, 5, 0.5, 0, ld=-1) == 1 and b"dims" in lib.fmx_last_error()
    assert call(0, 5, 7.0, 9) == 0                       # q / interp are read for the quantile only


def test_python_argument_checks():
    import factormodeling_amd.operations as ops
    s = C.to_series(C.make_values(1, 6, 3, 1)[0], None)
    with pytest.raises(ValueError):
        ops.ts_quantile(s, 3, 1.5)
    with pytest.raises(ValueError):
        ops.ts_quantile(s, 3, -0.01)
    with pytest.raises(ValueError):
        ops.ts_quantile(s, 3, 0.5, interpolation="cubic")
    with pytest.raises(ValueError):                      # pandas raises the same way
        s.rolling(3).quantile(1.5)
    with pytest.raises(ValueError):
        s.rolling(3).quantile(0.5, interpolation="cubic")


def test_no_gpu_raises():
    """No host fallback: without a HIP device the operators raise FmxError."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import factormodeling_amd.operations as ops
    from factormodeling_amd._lib import FmxError
    s = C.to_series(C.make_values(1, 6, 3, 1)[0], None)
    for fn in (ops.ts_min, ops.ts_max, ops.ts_argmin, ops.ts_argmax, ops.ts_median):
        with pytest.raises(FmxError):
            fn(s, 3)
    with pytest.raises(FmxError):
        ops.ts_quantile(s, 3, 0.25)
