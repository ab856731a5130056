"""The rolling operators' non-finite contract (DESIGN "Rolling kernels: what the tests pin"),
on the CPU: pandas' ``Rolling`` replaces +-inf by NaN before it aggregates, so one inf empties
the W windows that hold it and the column then recovers; diff / delay / backfill and
decay(window < 1) keep it.  The oracle against tests/golden/ops_nonfinite.npz (the reference's
own output on panels whose columns hold +-inf, dense and ragged; tests/golden/
make_golden_nonfinite.py), the fixture's own content, and the contract in one line: the infs
replaced by NaN give the same output."""
import numpy as np
import pytest

import oracle.ops as O
from golden_io import assert_close, load

D, A = 60, 12
WINDOWS = (1, 3, 5, 20)
AGG = ("ts_sum", "ts_mean", "ts_std", "ts_zscore", "ts_rank", "ts_decay")
SHIFT = ("ts_diff", "ts_delay")


@pytest.fixture(scope="module", params=["dense", "ragged"])
def fx(request):
    st = {k.split("/", 1)[1]: v for k, v in load("ops_nonfinite.npz").items() if k.startswith(request.param + "/")}
    d, s = st["in__d"], st["in__s"]
    pan = {}
    for k in ("x", "y", "xr"):
        pan[k] = np.full((D, A), np.nan)
        pan[k][d, s] = st[f"in_{k}__v"]
    present = np.zeros((D, A), dtype=bool)
    present[d, s] = True
    assert present.all() == (request.param == "dense")
    return {"tag": request.param, "st": st, "d": d, "s": s, "present": None if present.all() else present,
            "pmask": present, **pan}


def _dense(fx, key):
    out = np.full((D, A), np.nan)
    out[fx["d"], fx["s"]] = fx["st"]["out_" + key]
    return out


def _oracle(op, x, w, p):
    with np.errstate(all="ignore"):
        return O.ts_backfill(x, p) if op == "ts_backfill" else getattr(O, op)(x, w, p)


def _decay_check(got, ref, x, w, p, what):
    """tests/test_longwin.py's _decay_bound: the reference's np.dot sums in BLAS order."""
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), f"{what}: NaN mismatch at {np.argwhere(gn != rn)[:8].tolist()}"
    with np.errstate(all="ignore"):
        bound = 1e-13 * np.nan_to_num(O.ts_decay(np.abs(x), w, p), nan=0.0) + 1e-300
    assert (np.abs(got[~gn] - ref[~gn]) <= bound[~gn]).all(), what


def test_oracle_vs_reference(fx):
    x, y, p = fx["x"], fx["y"], fx["present"]
    for w in WINDOWS:
        for op in AGG + SHIFT:
            got, ref, what = _oracle(op, x, w, p), _dense(fx, f"{op}_{w}"), f"{fx['tag']}:{op}_{w}"
            if op == "ts_decay":
                _decay_check(got, ref, x, w, p, what)
            else:
                assert_close(got, ref, exact=True, what=what)
        with np.errstate(all="ignore"):
            got = O.ts_corr(x, y, w, p)
        assert_close(got, _dense(fx, f"ts_corr_{w}"), rtol=1e-6, atol=1e-9, what=f"{fx['tag']}:ts_corr_{w}")
    assert_close(_oracle("ts_decay", x, 0, p), _dense(fx, "ts_decay_0"), exact=True, what="ts_decay_0")
    assert_close(_oracle("ts_backfill", x, 0, p), _dense(fx, "ts_backfill"), exact=True, what="ts_backfill")


def test_oracle_regression_vs_reference(fx):
    st = fx["st"]
    for lag in (0, 1):
        for rt in (0, 1, 2, 3, 6):
            key = f"out_ts_regression_fast_5_{lag}_{rt}"
            od, os_, ov = O.ts_regression_fast_long(st["in__d"], st["in__s"], st["in_y__v"], st["in_xr__v"], 5, lag, rt)
            assert np.array_equal(od, st[key + "__d"]) and np.array_equal(os_, st[key + "__s"]), key
            assert_close(ov, st[key + "__v"], exact=True, what=f"{fx['tag']}:{key}")


def _present_rank(fx, a):
    """Row d of column a -> its index among the column's present rows."""
    return np.cumsum(fx["pmask"][:, a]) - 1


def test_fixture_is_not_degenerate(fx):
    """Every inf-bearing column has, in every aggregation's expected output, a NaN the inf caused
    (the inf's own row) and a finite value once it has left the window; the control column has
    no NaN past its row W - 1.  Two exemptions that follow from the operators' definitions, not
    from the data: ts_std / ts_zscore at W = 1 are NaN everywhere (one observation, ddof 1), and
    nothing follows an inf in the column's last row -- there the row before it must be finite.
    The shift operators must carry the inf through."""
    x, roles = fx["x"], list(fx["st"]["roles"])
    assert roles.index("control") == 7 and not np.isnan(x[:, 7][fx["pmask"][:, 7]]).any()
    infcols = [a for a in range(A) if np.isinf(x[:, a]).any()]
    assert infcols == [0, 1, 2, 3, 4, 5, 6]
    assert np.isinf(x[0, 3]) and np.isinf(x[D - 1, 4]) and np.isnan(x[33, 6]) and np.isinf(x[34, 6])
    assert np.isposinf(x[27, 2]) and np.isneginf(x[28, 2])
    r5 = _present_rank(fx, 5)
    assert np.isinf(x[[6, 34], 5]).all() and r5[34] - r5[6] > max(WINDOWS)
    if fx["tag"] == "ragged":                       # absent rows on both sides of the infs
        for a in infcols:
            for d in np.nonzero(np.isinf(x[:, a]))[0]:
                for n in (d - 1, d + 1):
                    if 0 <= n < D and not np.isinf(x[n, a]) and not (a == 6 and n == 33):
                        assert not fx["pmask"][n, a], (a, d, n)
    for w in WINDOWS:
        for op in AGG + ("ts_corr",):
            if w == 1 and op in ("ts_std", "ts_zscore", "ts_corr"):
                assert np.isnan(_dense(fx, f"{op}_{w}")).all()
                continue
            ref = _dense(fx, f"{op}_{w}")
            ctl, k7 = ref[:, 7], _present_rank(fx, 7)
            if op != "ts_corr":                     # corr's y has NaNs of its own
                assert not np.isnan(ctl[fx["pmask"][:, 7] & (k7 >= w - 1)]).any(), (op, w)
            for a in infcols:
                k = _present_rank(fx, a)
                rows = np.nonzero(np.isinf(x[:, a]))[0]
                assert np.isnan(ref[rows, a]).all(), (op, w, a)
                last = rows[-1]
                if last == D - 1:
                    before = np.nonzero(fx["pmask"][:last, a])[0][-1]
                    assert np.isfinite(ref[before, a]), (op, w, a)
                    continue
                after = fx["pmask"][:, a] & (k >= k[last] + w)
                assert np.isfinite(ref[after, a]).any(), (op, w, a)
        for op in SHIFT:
            assert np.isinf(_dense(fx, f"{op}_{w}")[:, :7]).any(), (op, w)
    for key in ("ts_decay_0", "ts_backfill"):
        assert np.isinf(_dense(fx, key)[:, :7]).sum() >= 9, key
    # the regression's x: one cell whose square overflows, one inf; rows come back after both
    xr = fx["xr"]
    assert xr[22, 1] == 1e200 and np.isposinf(xr[31, 2]) and np.isinf(fx["y"][:, [4, 9]]).sum() == 2
    st = fx["st"]
    for a, row in ((1, 22), (2, 31)):
        d, s = st["out_ts_regression_fast_5_0_2__d"], st["out_ts_regression_fast_5_0_2__s"]
        got = d[s == a]
        assert row not in got and (got > row + 5).any() and (got < row).any()


def test_inf_is_nan_to_every_aggregation(fx):
    """The contract in one line: with the infs replaced by NaN the oracle gives the same output."""
    x, y, p = fx["x"], fx["y"], fx["present"]
    xn, yn = np.where(np.isinf(x), np.nan, x), np.where(np.isinf(y), np.nan, y)
    assert np.isinf(x).sum() == 9 and np.isinf(y).sum() == 2
    for w in WINDOWS:
        for op in AGG:
            assert np.array_equal(_oracle(op, x, w, p), _oracle(op, xn, w, p), equal_nan=True), (op, w)
        with np.errstate(all="ignore"):
            assert np.array_equal(O.ts_corr(x, y, w, p), O.ts_corr(xn, yn, w, p), equal_nan=True), w
            assert np.array_equal(O.corr_vol_feature(x, y, w), O.corr_vol_feature(xn, yn, w), equal_nan=True), w


def test_shift_operators_keep_inf(fx):
    x, p = fx["x"], fx["present"]
    for op, w in (("ts_diff", 1), ("ts_delay", 3), ("ts_delay", -2), ("ts_backfill", 0), ("ts_decay", 0),
                  ("ts_decay", -3)):
        assert np.isinf(_oracle(op, x, w, p)).any(), (op, w)
