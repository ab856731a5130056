"""single_factor_backtests on the GPU: ``fmx_pnl_books`` against the per-book path, the two
backends against each other (bit for bit) and against the reference golden
(tests/golden/factor_returns.npz), chunking, and the table as ``FactorSelector``'s
``factor_ret_df``.

Tolerance against the reference: rtol 1e-12, atol 1e-15 on the six result columns (the
per-date sums are reduced in another order than numpy's; tests/test_simulation2.py uses the
same bound for the same columns); counts are exact.
"""
import os

import numpy as np
import pandas as pd
import pytest
from pandas.testing import assert_frame_equal

import factor_backtest_cases as FC

pytestmark = pytest.mark.gpu

PB_TILE = 4                     # csrc/sim.hip PB_TF: books per workgroup of k_pnl_books


def _panel(seed, F, D, A, ragged):
    """Same-day books [F][D][A] (NaN = no row; the rows are shared by the books), returns, cap
    flags, wprev: random long/short weights, a date without rows and a late listing when
    ragged, NaNs in the returns and the flags, an unmapped cap code 4."""
    rng = np.random.default_rng(seed)
    present = np.ones((D, A), dtype=bool)
    if ragged:
        present = rng.random((D, A)) > 0.15
        present[: D // 2, 0] = False                  # lists late
        present[1:4, A - 1] = False                   # a gap
        present[D // 2] = False                       # a date without rows
    W = rng.standard_normal((F, D, A)) / A
    W[rng.random(W.shape) < 0.2] = 0.0
    W[:, ~present] = np.nan
    R = 0.01 * rng.standard_normal((D, A))
    R[rng.random((D, A)) < 0.05] = np.nan
    CAP = rng.integers(1, 5, (D, A)).astype(np.float64)
    CAP[rng.random((D, A)) < 0.05] = np.nan
    rows = np.flatnonzero(present.any(axis=1))
    wprev = np.full(D, -1, dtype=np.int32)
    wprev[rows[1:]] = rows[:-1]
    return W, present, R, CAP, wprev


def _per_book(E, Wd, Rd, CAPd, wprev):
    import torch
    S = E.shift_rows(Wd)
    return torch.stack([E.pnl_daily(S[f].contiguous(), Rd, CAPd, wprev)[0] for f in range(Wd.shape[0])])


@pytest.mark.parametrize("F,D,A,ragged,table,cap", [
    (5, 20, 83, True, True, True),                    # ragged, one book past the tile
    (4, 12, 300, False, True, True),                  # dense with the table given
    (4, 12, 300, False, False, True),                 # dense, prev_row=None
    (PB_TILE + 1, 12, 300, True, True, False),        # CAP=None
    (1, 9, 7, True, True, True),
    (1, 9, 7, False, False, True),
    (4, 9, 256, True, True, True),
    (5, 9, 257, True, True, True),
    (5, 9, 257, False, False, False),
    (2 * PB_TILE + 1, 6, 300, True, True, True),
])
def test_pnl_books_equals_per_book_path(F, D, A, ragged, table, cap):
    import torch
    import factormodeling_amd.engine as E
    from factormodeling_amd.factor_backtest import _prev_rows
    W, present, R, CAP, wprev = _panel(1000 * F + A, F, D, A, ragged)
    dev = torch.device("cuda")
    Wd, Rd = torch.as_tensor(W, device=dev), torch.as_tensor(R, device=dev)
    CAPd = torch.as_tensor(CAP, device=dev) if cap else None
    prev = _prev_rows(present) if table else None
    got = E.pnl_books(Wd, Rd, CAPd, wprev, prev)
    want = _per_book(E, Wd, Rd, CAPd, wprev)
    assert got.shape == (F, D, 6)
    assert torch.equal(got, want)
    assert bool(torch.isfinite(got).all())
    if ragged:
        assert float(got[:, :, 2].abs().sum()) > 0.0  # the turnover sums are not trivially zero


def test_pnl_books_wprev_skipping_dates():
    """wprev may point further back than the previous row (returns-only dates in between)."""
    import torch
    import factormodeling_amd.engine as E
    from factormodeling_amd.factor_backtest import _prev_rows
    W, present, R, CAP, _ = _panel(5, 3, 10, 70, True)
    present[[2, 3, 7]] = False
    W[:, ~present] = np.nan
    rows = np.flatnonzero(present.any(axis=1))
    wprev = np.full(10, -1, dtype=np.int32)
    wprev[rows[1:]] = rows[:-1]
    dev = torch.device("cuda")
    Wd, Rd, CAPd = (torch.as_tensor(x, device=dev) for x in (W, R, CAP))
    assert torch.equal(E.pnl_books(Wd, Rd, CAPd, wprev, _prev_rows(present)), _per_book(E, Wd, Rd, CAPd, wprev))


@pytest.mark.parametrize("d,bad", [(3, 3), (3, 7), (0, 0), (5, -2)])
def test_pnl_books_rejects_bad_prev_row(d, bad):
    import torch
    import factormodeling_amd.engine as E
    from factormodeling_amd._lib import FmxError
    from factormodeling_amd.factor_backtest import _prev_rows
    W, present, R, CAP, wprev = _panel(3, 2, 8, 40, False)
    dev = torch.device("cuda")
    prev = _prev_rows(present)
    prev[d, 11] = bad
    with pytest.raises(FmxError, match="prev_row"):
        E.pnl_books(torch.as_tensor(W, device=dev), torch.as_tensor(R, device=dev), None, wprev, prev)
    with pytest.raises(FmxError):
        E.pnl_books(torch.as_tensor(W, device=dev), torch.as_tensor(R[:-1], device=dev), None, wprev, None)
    bad_wprev = wprev.copy()
    bad_wprev[2] = 8
    with pytest.raises(FmxError, match="wprev"):
        E.pnl_books(torch.as_tensor(W, device=dev), torch.as_tensor(R, device=dev), None, bad_wprev, None)


# ----------------------------------------------------------------------------- the public function
_RUNS = {}


def _run(name, inv, tc, backend):
    """Each (case, variant, backend) is computed once and shared by the tests below."""
    key = (name, inv, tc, backend)
    if key not in _RUNS:
        from factormodeling_amd.factor_backtest import single_factor_backtests
        _RUNS[key] = single_factor_backtests(FC.factors_df(name), FC.settings(name, inv, tc), backend=backend)
    return _RUNS[key]


@pytest.mark.parametrize("name", FC.CASES)
@pytest.mark.parametrize("inv,tc", FC.VARIANTS)
def test_backends_agree_bit_for_bit(name, inv, tc):
    a, b = _run(name, inv, tc, "batched"), _run(name, inv, tc, "loop")
    assert list(a) == list(b) == FC.COLS + FC.COUNTS
    for k in a:
        assert_frame_equal(a[k], b[k], check_exact=True, obj=f"{name} {inv} tc={tc} {k}")


@pytest.mark.parametrize("backend", ["batched", "loop"])
@pytest.mark.parametrize("name", FC.CASES)
@pytest.mark.parametrize("inv,tc", FC.VARIANTS)
def test_backend_matches_reference(name, inv, tc, backend):
    got, ref = _run(name, inv, tc, backend), FC.reference_frames(name, inv, tc)
    cols = list(FC.factors_df(name).columns)
    for k in FC.COLS:
        assert list(got[k].columns) == cols
        assert got[k].index.equals(ref[k].index) and got[k].index.name == "date", k
        np.testing.assert_allclose(got[k].to_numpy(), ref[k].to_numpy(), rtol=1e-12, atol=1e-15, err_msg=k)
        assert np.array_equal(np.isnan(got[k].to_numpy()), np.isnan(ref[k].to_numpy())), k
    for k in FC.COUNTS:
        assert got[k].index.equals(ref[k].index), k
        np.testing.assert_array_equal(got[k].to_numpy(), ref[k].to_numpy(), err_msg=k)


@pytest.mark.parametrize("name,inv", [("eq_ragged", "diff"), ("lin_ragged", "same")])
def test_chunking_does_not_change_the_bits(name, inv):
    from factormodeling_amd.factor_backtest import single_factor_backtests
    one = single_factor_backtests(FC.factors_df(name), FC.settings(name, inv, True), backend="batched", chunk_bytes=1)
    full = _run(name, inv, True, "batched")
    for k in full:
        assert_frame_equal(one[k], full[k], check_exact=True, obj=k)


def test_linear_rows_out_of_symbol_order():
    """'linear' sums each date's rows in input order: a frame whose rows are not in sorted
    symbol order inside a date takes the per-date row layout; the backends still agree."""
    from factormodeling_amd.factor_backtest import single_factor_backtests
    df = FC.factors_df("lin_ragged")
    rng = np.random.default_rng(11)
    d = df.index.get_level_values(0)
    order = np.lexsort((rng.random(len(df)), d.values))          # dates ascending, symbols shuffled
    df = df.iloc[order]
    st = FC.settings("lin_ragged", "same", True)
    st["investability_flag"] = st["investability_flag"].iloc[order]
    a = single_factor_backtests(df, st, backend="batched")
    b = single_factor_backtests(df, st, backend="loop")
    for k in a:
        assert_frame_equal(a[k], b[k], check_exact=True, obj=k)


@pytest.mark.parametrize("backend", ["batched", "loop", "auto"])
def test_columns_filter_and_inputs_unmodified(backend):
    from factormodeling_amd.factor_backtest import single_factor_backtests, single_factor_returns
    from factormodeling_amd.portfolio_simulation import SimulationSettings
    df = FC.factors_df("eq_ragged")
    st = SimulationSettings(**FC.settings("eq_ragged", "diff", True, factors_df=df, contributor=True))
    before = df.copy()
    kept = {k: getattr(st, k).copy() for k in ("returns", "cap_flag", "investability_flag")}
    out = single_factor_backtests(df, st, columns=["f3", "f0"], backend=backend)
    full = _run("eq_ragged", "diff", True, "batched")
    for k in out:
        assert list(out[k].columns) == ["f3", "f0"]
        assert_frame_equal(out[k], full[k][["f3", "f0"]], check_exact=True, obj=k)
    fr = single_factor_returns(df, st, columns=["f3", "f0"], backend=backend)
    assert_frame_equal(fr, out["log_return"], check_exact=True)
    tn = single_factor_returns(df, st, field="turnover", backend=backend)
    assert_frame_equal(tn, full["turnover"], check_exact=True)
    assert_frame_equal(df, before, check_exact=True)             # no column added (the reference's run() adds one)
    assert st.factors_df is df and list(df.columns) == list(before.columns)
    assert st.contributor is True and st.plot is False
    for k, v in kept.items():
        pd.testing.assert_series_equal(getattr(st, k), v, check_exact=True)


def test_eligibility_predicate():
    """With a GPU the golden inputs are eligible for the one-pass path; settings without cap
    flags are not (the loop takes them), and the reason names the field."""
    from factormodeling_amd.factor_backtest import batched_ineligible, _as_settings
    st = FC.settings("eq_ragged", "same", True)
    assert batched_ineligible(FC.factors_df("eq_ragged"), _as_settings(st)) is None
    st["cap_flag"] = None
    assert "cap_flag" in batched_ineligible(FC.factors_df("eq_ragged"), _as_settings(st))


def test_factor_selector_takes_the_table():
    """The selector.npz-sized panel (70 x 40 x 8): FactorSelector(method="momentum", the
    factor_momentum selector) fed with the batched table runs and equals the loop's table."""
    import factormodeling_amd.factor_selector as fs
    from factormodeling_amd.factor_backtest import single_factor_returns
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "selector.npz"))
    dates, syms, names = pd.to_datetime(g["dates"]), list(g["syms"]), list(g["names"])
    D, A, F = g["X"].shape
    idx = pd.MultiIndex.from_product([dates, syms], names=["date", "symbol"])
    df = pd.DataFrame(g["X"].reshape(D * A, F), index=idx, columns=names)
    ret = pd.Series(g["R"].reshape(-1), index=idx, name="log_return")
    rng = np.random.default_rng(8)
    st = dict(returns=ret, cap_flag=pd.Series(rng.integers(1, 4, len(idx)).astype(np.float64), index=idx),
              investability_flag=pd.Series(1.0, index=idx), method="equal", pct=0.2)
    tables = {b: single_factor_returns(df, st, backend=b) for b in ("batched", "loop")}
    assert tables["batched"].shape == (D, F) and list(tables["batched"].columns) == names
    assert_frame_equal(tables["batched"], tables["loop"], check_exact=True)
    outs = {b: fs.FactorSelector(df, ret, t, window=20, method="momentum", method_kwargs={}).prepare_selection()
            for b, t in tables.items()}
    assert len(outs["batched"]) > 0 and float(outs["batched"].to_numpy().sum()) > 0.0
    assert_frame_equal(outs["batched"], outs["loop"], check_exact=True)
