"""Every kernel path of the group operators (DESIGN "Group operators: dispatch and code
contract") against the oracle, bit-exact on the whole ``[F][D][A]`` output with no cell
masked out: k_group (A <= 4096), the four k_group_long instantiations (EMAX 5 / 8 / 12 / 16,
both ends of each bucket), k_group_xl and fmx_group_rank_sorted; dense and with absent cells;
two factors sharing one group table; codes outside [0, ngroups); singleton, empty, all-NaN
and constant groups; a (date, group) of exactly 8192 and 8193 present members.

The panels come from tests/group_cases.py, which tests/test_group_cases_host.py pins.  Before
every call a few blocks of the output's size are filled with 12345.0 and freed, so that the
``torch.empty_like`` of the call most likely gets one of them back: a cell the kernel never
writes then shows as a finite 12345.0, not as a NaN that happens to match."""
import numpy as np
import pytest

import group_cases as GC
from golden_io import assert_close

pytestmark = pytest.mark.gpu

POISON = 12345.0


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _poison(shape, dev):
    import torch
    blocks = [torch.full(shape, POISON, dtype=torch.float64, device=dev) for _ in range(4)]
    torch.cuda.synchronize()
    del blocks


def _device_case(c, dev):
    import torch
    xt = torch.tensor(c["x"], device=dev)
    gt = torch.tensor(c["codes"], device=dev)
    pt = None if c["present"] is None else torch.tensor(c["present"].astype(np.uint8), device=dev)
    return xt, gt, pt


def _group_op(op, xt, gt, ngroups, method="average", present=None, long_rows=None):
    import factormodeling_amd.engine as E
    _poison(tuple(xt.shape), xt.device)
    return E.group_op(op, xt, gt, ngroups, method, present=present, long_rows=long_rows).cpu().numpy()


def _check(got, ref, what):
    assert got.shape == ref.shape, what
    assert not (got == POISON).any(), f"{what}: {int((got == POISON).sum())} cells were never written"
    assert_close(got.ravel(), ref.ravel(), exact=True, what=what)


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("A", GC.LENGTHS)
def test_group_paths_vs_oracle(dev, A, ragged):
    """The three moments and the five rank methods at every row length at which the dispatch
    changes kernel, both factors, ngroups = 61."""
    c, ref = GC.case_and_reference(A, ragged)
    xt, gt, pt = _device_case(c, dev)
    for op in GC.MOMENTS:
        _check(_group_op(op, xt, gt, GC.NG, present=pt), ref[op], f"{op} A={A} ragged={ragged}")
    want = "k_group" if A <= 4096 else f"k_group_long<{GC.emax_bucket(A)}>" if A <= 16384 else None
    assert GC.expected_path("mean", A, c["codes"], GC.NG, c["present"]) == (want or "k_group_xl")
    assert GC.expected_path("rank", A, c["codes"], GC.NG, c["present"]) == (want or "fmx_group_rank_sorted")
    for m in GC.METHODS:
        _check(_group_op("rank", xt, gt, GC.NG, m, present=pt), ref["rank", m], f"rank {m} A={A} ragged={ragged}")


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("A,members", GC.BIG_VARIANTS)
def test_group_rank_8192_switch(dev, A, members, ragged):
    """A (date, group) of exactly 8192 present members is the last the per-group LDS sort of
    k_group_long takes; 8193 is the first that sends the call to the rows sorted in HBM."""
    c, ref = GC.case_and_reference(A, ragged, members)
    path = GC.expected_path("rank", A, c["codes"], GC.NG, c["present"])
    assert path == ("fmx_group_rank_sorted" if members > 8192 else f"k_group_long<{GC.emax_bucket(A)}>")
    xt, gt, pt = _device_case(c, dev)
    for m in GC.METHODS:
        _check(_group_op("rank", xt, gt, GC.NG, m, present=pt), ref["rank", m],
               f"rank {m} A={A} members={members} ragged={ragged} ({path})")


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("A", [4096, 5121, 16384])
def test_group_long_rows_flag_is_bit_identical(dev, A, ragged):
    """k_group_xl (long_rows=True) equals k_group / k_group_long (long_rows=False) bit for bit,
    and both equal the oracle."""
    c, ref = GC.case_and_reference(A, ragged)
    xt, gt, pt = _device_case(c, dev)
    assert GC.expected_path("mean", A, c["codes"], GC.NG, c["present"], long_rows=True) == "k_group_xl"
    assert GC.expected_path("mean", A, c["codes"], GC.NG, c["present"], long_rows=False) != "k_group_xl"
    for op in GC.MOMENTS:
        xl = _group_op(op, xt, gt, GC.NG, present=pt, long_rows=True)
        short = _group_op(op, xt, gt, GC.NG, present=pt, long_rows=False)
        assert np.array_equal(xl, short, equal_nan=True), f"{op} A={A}: long_rows changes the result"
        _check(xl, ref[op], f"{op} A={A} long_rows=True")
        _check(short, ref[op], f"{op} A={A} long_rows=False")


@pytest.mark.parametrize("A", [100, 5000, 20000])
def test_group_no_groups(dev, A):
    """ngroups = 0: every code is out of range, so every op returns NaN everywhere."""
    import torch
    rng = np.random.default_rng(A)
    x = rng.standard_normal((2, 3, A))
    codes = rng.integers(0, 5, size=(3, A)).astype(np.int32)
    xt, gt = torch.tensor(x, device=dev), torch.tensor(codes, device=dev)
    nan = np.full(x.shape, np.nan)
    for op in GC.MOMENTS:
        _check(_group_op(op, xt, gt, 0), nan, f"{op} A={A} ngroups=0")
    for m in GC.METHODS:
        _check(_group_op("rank", xt, gt, 0, m), nan, f"rank {m} A={A} ngroups=0")


def test_group_ops_dropin_long_row(dev):
    """operations.group_* on a ragged (date, symbol) Series of 4 dates x 4100 symbols (the
    k_group_long row with absent cells, reached through _group_ids / _group_apply): string
    labels, some NaN, handed over in another row order than the values."""
    import pandas as pd
    import torch
    import oracle.ops as O
    from factormodeling_amd import operations as ops
    from factormodeling_amd.panel import panel_index
    rng = np.random.default_rng(4100)
    D, A = 4, 4100
    dates = pd.date_range("2021-03-01", periods=D)
    syms = np.array([f"S{i:05d}" for i in range(A)])
    x = rng.standard_normal((D, A))
    x = np.where(rng.random(x.shape) < 0.2, np.round(x, 1), x)
    x[rng.random(x.shape) < 0.03] = np.nan
    labels = np.array([f"sector {k:02d}" for k in range(13)])
    lab = rng.integers(0, 13, size=(D, A))
    g = lab.astype(np.float64)                      # label k sorts k-th: the dense id is k
    g[rng.random(g.shape) < 0.02] = np.nan
    present = rng.random((D, A)) >= 0.1
    present[0] = True                               # every symbol has a row: the panel is 4100 wide
    d_i, s_i = np.nonzero(present)
    index = pd.MultiIndex.from_arrays([dates[d_i], syms[s_i]], names=["date", "symbol"])
    series = pd.Series(x[d_i, s_i], index=index, name="f")
    gv = g[d_i, s_i]
    group = pd.Series(np.where(np.isnan(gv), None, labels[np.nan_to_num(gv).astype(int)]), index=index,
                      dtype=object)
    group = group.where(group.notna(), np.nan).iloc[rng.permutation(len(group))]
    assert panel_index(series.index).A == A and not group.index.equals(series.index)
    assert group.isna().sum() > 0
    calls = [("mean", ops.group_mean, O.group_mean), ("neutralize", ops.group_neutralize, O.group_neutralize),
             ("normalize", ops.group_normalize, O.group_normalize),
             ("rank", ops.group_rank_normalized, O.group_rank_normalized)]
    for name, fn, oracle in calls:
        _poison((1, D, A), torch.device("cuda", torch.cuda.current_device()))
        got = fn(series, group)
        with np.errstate(all="ignore"):
            ref = oracle(x, g, present)
        assert got.index.equals(series.index) and got.name == "val"
        _check(got.to_numpy(), ref[d_i, s_i], f"operations.group_{name}")
