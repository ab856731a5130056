"""Every kernel path of ts_ops.hip (DESIGN "Rolling kernels: what the tests pin") against the
oracle on the whole ``[F][D][A]`` output, no cell masked out: k_ts_reg, k_ts_rl, k_ts_ptr,
k_ts_win, k_ts_lead_ptr, k_ts_window0, the fused k_ts_set and the k_ts_mom3 + single-op arm of
fmx_ts_set (every subset of outputs), k_ts_corr_fast / _rl / _ptr with y shared and per factor,
k_ts_cvf_rl on both sides of its table limit, k_ts_corr_feat with and without the corr output,
and k_ts_regression_ptr -- at the dates, windows and row lengths where each kernel changes
path (tests/ts_path_cases.py, pinned by tests/test_ts_paths_host.py), on panels that hold NaN
runs, constant runs, signed zeros, huge and tiny scales, +-inf (NaN to every aggregation, kept
by the shifts) and, when ragged, absent cells filled with +inf / 12345.0.

Every output tensor is handed in filled with 12345.0, which must not survive.  Bit-exact but
for ts_decay (|delta| <= 1e-13 decay(|x|) + 1e-300 with equal NaN patterns, as
tests/test_longwin.py: the reference's dot product sums in BLAS order)."""
import numpy as np
import pytest

import ts_path_cases as TC
from golden_io import assert_close, load, series

pytestmark = pytest.mark.gpu

POISON = TC.POISON


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _put(dev, X, p=None):
    import torch
    Xt = torch.tensor(np.ascontiguousarray(X), device=dev)
    return Xt, (None if p is None else torch.tensor(p.astype(np.uint8), device=dev))


def _poisoned(Xt):
    import torch
    return torch.full_like(Xt, POISON)


def _check(got, ref, what, bound=None):
    assert got.shape == ref.shape, what
    assert not (got == POISON).any(), f"{what}: {int((got == POISON).sum())} cells were never written"
    if bound is None:
        assert_close(got.ravel(), ref.ravel(), exact=True, what=what)
        return
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), f"{what}: NaN mismatch at {np.argwhere(gn != rn)[:8].tolist()}"
    assert (np.abs(got[~gn] - ref[~gn]) <= bound[~gn]).all(), what


def _check_op(got, op, W, D, A, ragged, what):
    bound = TC.decay_bound(W, D, A, ragged) if op == "decay" and W >= 1 else None
    _check(got, TC.ts_reference(op, W, D, A, ragged), what, bound)


ARM_PATHS = {"reg": "k_ts_reg", "rl": "k_ts_rl<8>", "ptr": "k_ts_ptr<8>", "win": "k_ts_win<16>",
             "lead": "k_ts_lead_ptr", "window0": ("k_ts_window0", "copy", "copy+k_ts_window0")}


@pytest.mark.parametrize("arm", list(TC.TS_ARMS))
def test_ts_op_arm_vs_oracle(dev, arm):
    import factormodeling_amd.engine as E
    for ops, W, D, A, ragged in TC.TS_ARMS[arm]():
        X, p = TC.panel(D, A, W, ragged)
        Xt, pt = _put(dev, X, p)
        for op in ops:
            path = TC.expected_path(op, W, ragged)
            assert path.startswith(ARM_PATHS[arm]) if arm != "window0" else path in ARM_PATHS[arm], (arm, op, W)
            got = E.ts(op, Xt, W, present=pt, out=_poisoned(Xt)).cpu().numpy()
            _check_op(got, op, W, D, A, ragged, f"{path} {op} W={W} D={D} A={A} ragged={ragged}")


def _run_set(E, Xt, pt, W, WR, names):
    outs = {k: _poisoned(Xt) for k in names}
    E.ts_set(Xt, outs, W, WR, present=pt)
    return {k: v.cpu().numpy() for k, v in outs.items()}


@pytest.mark.parametrize("arm", ["fused", "mom3"])
def test_ts_set_arm_vs_oracle(dev, arm):
    import factormodeling_amd.engine as E
    for a, W, WR, D, A, ragged in TC.set_cases():
        if a != arm:
            continue
        assert (TC.expected_set_path(W, WR, ragged)[0] == "k_ts_set<20,10,5>") == (arm == "fused")
        X, p = TC.panel(D, A, W, ragged)
        Xt, pt = _put(dev, X, p)
        got = _run_set(E, Xt, pt, W, WR, TC.SET_OUTS)
        for op in ("mean", "std", "zscore", "decay"):
            _check_op(got[op], op, W, D, A, ragged, f"ts_set[{arm}] {op} W={W} WR={WR} D={D} A={A}")
        # rank at its own window, on the panel laid out for W
        ref = np.stack([TC.oracle_ts("rank", X[f], WR, p) for f in range(TC.F)])
        _check(got["rank"], ref, f"ts_set[{arm}] rank W={W} WR={WR} D={D} A={A}")


@pytest.mark.parametrize("shape", TC.SUBSET_SHAPES, ids=lambda s: s[0])
def test_ts_set_every_subset_of_outputs(dev, shape):
    """A null output skips its stores and nothing else: each of the 31 subsets gives the bits of
    the full set, which is checked against the oracle."""
    import factormodeling_amd.engine as E
    arm, W, WR, D, A, ragged = shape
    X, p = TC.panel(D, A, W, ragged)
    Xt, pt = _put(dev, X, p)
    full = _run_set(E, Xt, pt, W, WR, TC.SET_OUTS)
    for op in ("mean", "std", "zscore", "decay"):
        _check_op(full[op], op, W, D, A, ragged, f"ts_set[{arm}] full {op}")
    rank = np.stack([TC.oracle_ts("rank", X[f], WR, p) for f in range(TC.F)])
    _check(full["rank"], rank, f"ts_set[{arm}] full rank")
    for names in TC.subsets():
        got = _run_set(E, Xt, pt, W, WR, names)
        for k in names:
            assert not (got[k] == POISON).any(), (names, k)
            assert np.array_equal(got[k], full[k], equal_nan=True), f"ts_set[{arm}] {names}: {k} differs"


@pytest.mark.parametrize("arm", ["fast", "rl", "ptr"])
def test_ts_corr_arm_vs_oracle(dev, arm):
    import torch
    import factormodeling_amd.engine as E
    for a, nf, W, D, A, ragged, pf in TC.corr_cases():
        if a != arm:
            continue
        assert TC.expected_corr_path(W, ragged).startswith("k_ts_corr_" + arm)
        X, Y, p = TC.corr_inputs(nf, W, D, A, ragged, pf)
        Xt, pt = _put(dev, X, p)
        Yt = torch.tensor(np.ascontiguousarray(Y), device=dev)
        assert Yt.dim() == (3 if pf else 2)
        got = E.ts_corr(Xt, Yt, W, present=pt, out=_poisoned(Xt)).cpu().numpy()
        _check(got, TC.corr_reference(nf, W, D, A, ragged, pf),
               f"k_ts_corr_{arm} F={nf} W={W} D={D} A={A} per-factor y={pf}")


@pytest.mark.parametrize("W", [TC.TSC_MAXW, TC.TSC_MAXW + 1])
def test_corr_and_feature_full_window_at_table_limit(dev, W):
    """Full windows on each side of TSC_MAXW (4108 dates, 3 columns): k_ts_corr_fast and
    k_ts_cvf_rl<true> at 4096, k_ts_corr_rl and k_ts_cvf_rl<false> at 4097.  Rows 0..3 hold a +inf
    and a NaN in x and a NaN and a -inf in y, so the first full windows are NaN, each non-finite
    pair has to leave through the kernels' remove side, and the last rows are finite."""
    import torch
    import factormodeling_amd.engine as E
    X, Y, corr, feat = TC.long_case(W)
    Xt, _ = _put(dev, X)
    Yt = torch.tensor(Y, device=dev)
    C = E.ts_corr(Xt, Yt, W, out=_poisoned(Xt))
    _check(C.cpu().numpy(), corr, f"{TC.expected_corr_path(W, False)} W={W}")
    got = E.corr_vol_feature(Xt, C, W, out=_poisoned(Xt)).cpu().numpy()
    _check(got, feat, f"{TC.expected_cvf_path(W)} W={W}")


def test_corr_vol_feature_and_fused_feature_vs_oracle(dev):
    import torch
    import factormodeling_amd.engine as E
    for arm, nf, W, D, A in TC.feature_cases():
        X, Y, _ = TC.corr_inputs(nf, W, D, A, False, False)
        Xt, _ = _put(dev, X)
        Yt = torch.tensor(np.ascontiguousarray(Y), device=dev)
        ref = TC.feature_reference(nf, W, D, A)
        cref = TC.corr_reference(nf, W, D, A, False, False)
        what = f"{arm} F={nf} W={W} D={D} A={A}"
        if arm == "cvf":
            C = E.ts_corr(Xt, Yt, W, out=_poisoned(Xt))
            _check(C.cpu().numpy(), cref, what + " corr")
            _check(E.corr_vol_feature(Xt, C, W, out=_poisoned(Xt)).cpu().numpy(), ref, what)
        else:
            C = _poisoned(Xt)
            got = E.corr_feature(Xt, Yt, W, out=_poisoned(Xt), corr_out=C).cpu().numpy()
            _check(got, ref, what + " k_ts_corr_feat<true>")
            _check(C.cpu().numpy(), cref, what + " k_ts_corr_feat<true> corr")
            _check(E.corr_feature(Xt, Yt, W, out=_poisoned(Xt)).cpu().numpy(), ref, what + " k_ts_corr_feat<false>")


def _fill_pool(shape, dev):
    """engine.ts_regression allocates its own output: leave freed blocks of its size filled with
    12345.0 for it to pick up, so a cell it never writes shows.  Best effort only -- nothing
    obliges the caching allocator to hand one of them back; the bit-exact comparison of the whole
    panel is what carries the test."""
    import torch
    blocks = [torch.full(shape, POISON, dtype=torch.float64, device=dev) for _ in range(4)]
    torch.cuda.synchronize()
    del blocks


def test_regression_engine_vs_oracle(dev):
    import torch
    import factormodeling_amd.engine as E
    y, x, valid, *_ = TC.regression_inputs()
    D, A = TC.REG_ENGINE_SHAPE
    Yt, Xt, Vt = (torch.tensor(a, device=dev) for a in (y, x, valid))
    for w, rt in TC.regression_cases():
        _fill_pool((D, A), dev)
        got = E.ts_regression(Yt, Xt, Vt, w, rt).cpu().numpy()
        _check(got, TC.regression_reference(w, rt), f"k_ts_regression_ptr W={w} rettype={rt}")


@pytest.mark.parametrize("tag", ["dense", "ragged"])
def test_regression_dropin_vs_reference_fixture(dev, tag):
    """operations.ts_regression_fast on tests/golden/ops_nonfinite.npz: an x cell of 1e200 (its
    square overflows), +inf in x, -inf in y.  Same rows as the reference, same bits."""
    from factormodeling_amd import operations as ops
    st = {k.split("/", 1)[1]: v for k, v in load("ops_nonfinite.npz").items() if k.startswith(tag + "/")}
    for k in ("in_y", "in_xr"):
        st[k + "__d"], st[k + "__s"] = st["in__d"], st["in__s"]
    sy, sx = series(st, "in_y"), series(st, "in_xr")
    for lag in (0, 1):
        for rt in (0, 1, 2, 3, 6):
            key = f"out_ts_regression_fast_5_{lag}_{rt}"
            got = ops.ts_regression_fast(sy, sx, 5, lag=lag, rettype=rt)
            want = series(st, key)
            assert got.index.equals(want.index), f"{tag}:{key}: rows differ ({len(got)} vs {len(want)})"
            assert_close(got.to_numpy(dtype=np.float64), st[key + "__v"], exact=True, what=f"{tag}:{key}")
