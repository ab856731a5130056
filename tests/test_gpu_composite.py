"""The composite kernels (csrc/composite.hip) at the shapes where they can go wrong.

* the drop-in functions against ``golden/composite_edges.npz`` (the reference's outputs on
  seven panels from a single row to a second thread stride, three of them ragged);
* every stage (``k_comp_adj``, ``k_comp_proxy``, ``k_comp_combine``, ``k_wcomp_pct``,
  ``k_wcomp_proxy``, ``k_wcomp_combine``) against the oracle's stage of the same name, fed
  the oracle's output of the stage before it;
* the block radix select on single rows that pin each of its digit passes;
* the combine kernels' host LDS check at its boundary.

The kernels restate numpy's arithmetic and the library is built with -ffp-contract=off, so
the stages are compared bit for bit.  The one exception is the combine of a ragged panel:
the kernel sums the length-A row with zeros at the absent cells over numpy's tree for A,
numpy sums the compacted present rows over its tree for their count, so the two means may
differ in the last bits; there the project tolerance |d| <= 1e-9 + 1e-6 |ref| applies."""
import numpy as np
import pytest

import oracle.composite as OC
from composite_edge_cases import (SUFFIXES, frames, panel_ids, panels, percentiles, pooled_rows,
                                  select_rows)
from golden_io import assert_close

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-9
LDS_LIMIT = 160 * 1024


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import factormodeling_amd.composite_factor as cf
    import factormodeling_amd.engine as E
    from factormodeling_amd import _lib
    return torch, cf, E, _lib


def _up(torch, a, dtype=None):
    return torch.as_tensor(np.array(a, order="C"), device="cuda", dtype=dtype)   # a writable copy


def _pres(torch, p):
    return None if p["P"] is None else _up(torch, p["P"].astype(np.uint8))


def _codes(E, names):
    return [E.suffix_code(n) for n in names]


def _check(got, ref, exact, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    with np.errstate(all="ignore"):
        d = np.abs(got - ref)
    print(f"{what}: max |got - ref| = {np.max(d[~np.isnan(d)], initial=0.0):.3e}")
    assert_close(got, ref, rtol=RTOL, atol=ATOL, exact=exact, what=what)


# ------------------------------------------------------------------ a. drop-in vs fixture
@pytest.mark.parametrize("p", panels(), ids=panel_ids())
def test_dropin_vs_reference(gpu, p):
    torch, cf, E, _ = gpu
    df, seldf, di, si = frames(p)
    for meth in ("zscore", "rank"):
        for sk, sel in (("all", p["names"]), ("sub", p["sub"])):
            out = cf.composite_factor_calculation(df, sel, method=meth)
            assert out.name == "composite_factor" and out.index.equals(df.index)
            _check(out.to_numpy(), p["out"][f"cfc_{sk}_{meth}"][di, si], False, f"cfc_{sk}_{meth}")
        out = cf.weighted_composite_factor(df, seldf, method=meth)
        assert out.name == "composite_factor" and out.index.equals(df.index)
        ref = p["out"][f"wcf_{meth}"]
        got = np.zeros_like(ref)
        got[di, si] = out.to_numpy()
        _check(got[di, si], ref[di, si], False, f"wcf_{meth}")
        filled = ~ref.any(axis=1)                         # whole dates of fillna(0)
        assert filled.any() and not got[filled].any(), f"wcf_{meth}: fillna(0) dates are not exactly 0"
        # every cell the reference's fillna(0) fills (its composite is NaN there): exactly 0
        raw = OC.weighted_composite_factor(p["X"], p["names"], p["sd"], p["W"], meth, p["P"], fillna=False)
        cells = np.isnan(raw) & p["present"]
        assert cells.any() and not ref[cells].any()
        assert not got[cells].any(), f"wcf_{meth}: {np.count_nonzero(got[cells])} fillna(0) cells are not exactly 0"


# ------------------------------------------------------------------ b. stage vs oracle stage
@pytest.mark.parametrize("p", panels(), ids=panel_ids())
def test_comp_adj_vs_oracle(gpu, p):
    """k_comp_adj: bit-exact on the present cells (the caller masks the absent ones)."""
    torch, cf, E, _ = gpu
    Xd = _up(torch, p["X"])
    for sel in (p["names"], p["sub"]):
        cols = [p["names"].index(n) for n in sel]
        got = E.comp_adj(Xd, cols, _codes(E, sel)).cpu().numpy()
        ref = OC.adjusted(p["X"], p["names"], sel, p["P"])
        _check(got[:, p["present"]], ref[:, p["present"]], True, f"adj K={len(sel)}")


@pytest.mark.parametrize("p", panels(), ids=panel_ids())
def test_comp_proxy_vs_oracle(gpu, p):
    torch, cf, E, _ = gpu
    for sel in (p["names"], p["sub"]):
        adj = OC.adjusted(p["X"], p["names"], sel, p["P"])
        groups = list(OC._prefix_groups(sel).values())
        got = E.comp_proxy(_up(torch, adj), groups).cpu().numpy()
        _check(got, OC.proxies(adj, sel, p["P"]), True, f"proxy K={len(sel)}")


@pytest.mark.parametrize("p", panels(), ids=panel_ids())
def test_normalise_vs_oracle(gpu, p):
    """The normalisation between proxy and combine, as both composites call it: the moment
    kernel (market_neutralize == safe_zcol) and the rank kernel with scipy's NaN propagation
    and ``len(x)`` = the present rows.  Both work on the compacted present rows, so they are
    bit-exact on ragged panels too; in the [G][D][A] layout of composite_factor_calculation
    and the [G][J][A] layout (mask rows gathered per selection row) of the weighted one."""
    torch, cf, E, _ = gpu
    prox = OC.proxies(OC.adjusted(p["X"], p["names"], p["names"], p["P"]), p["names"], p["P"])
    lohi = OC.weighted_percentiles(p["X"], p["names"], p["sd"], p["W"], p["P"])
    wprox = OC.weighted_proxies(p["X"], p["names"], p["sd"], p["W"], lohi, p["P"])
    presJ = p["present"][np.maximum(p["sd"], 0)]
    layouts = (("cfc", prox, p["present"], lambda m: OC.normalise(prox, m, p["P"])),
               ("wcf", wprox, presJ, lambda m: OC.weighted_normalise(wprox, [max(d, 0) for d in p["sd"]], m, p["P"])))
    for name, px, mask, ref_fn in layouts:
        pres = None if p["P"] is None else _up(torch, mask.astype(np.uint8))
        Pd = _up(torch, px)
        for meth in ("zscore", "rank"):
            got = (E.cs_moment("market_neutralize", Pd, pres) if meth == "zscore"
                   else E.cs_rank(Pd, "scipy_average", pres)).cpu().numpy()
            ref = ref_fn(meth)
            _check(got[:, mask], ref[:, mask], True, f"normalise {name} {meth}")


@pytest.mark.parametrize("p", panels(), ids=panel_ids())
def test_comp_combine_vs_oracle(gpu, p):
    """k_comp_combine, mode 0 on the oracle's z-scores and mode 1 on its ranks: bit-exact on
    the dense panels, the project tolerance on the ragged ones (see the module docstring;
    measured on the MI355X: max |got - ref| 2.2e-16 in mode 0, 4.4e-16 in mode 1)."""
    torch, cf, E, _ = gpu
    prox = OC.proxies(OC.adjusted(p["X"], p["names"], p["names"], p["P"]), p["names"], p["P"])
    for mode, meth in ((0, "zscore"), (1, "rank")):
        nrm = OC.normalise(prox, meth, p["P"])
        got = E.comp_combine(_up(torch, nrm), mode, _pres(torch, p)).cpu().numpy()
        _check(got, OC.combine(nrm, mode, p["P"]), not p["ragged"], f"combine mode {mode}")


def _plan(torch, cf, p):
    plan = cf.weighted_plan(np.asarray(p["sd"]), p["W"], p["names"])
    dev = {k: _up(torch, plan[k], torch.int32) for k in ("pdate", "ncol", "col", "suf", "grp", "ngrp", "soff", "scol")}
    dev["gw"] = _up(torch, plan["gw"])
    return plan, dev


def _wcomp_pct(gpu, Xd, pdate, soff, scol):
    torch, cf, E, _lib = gpu
    F, D, A = Xd.shape
    J = pdate.numel()
    lo, hi = E._qfrac(Xd.device)
    lohi = torch.full((J, 4, 3), -7.0, dtype=torch.float64, device=Xd.device)
    _lib.call("fmx_wcomp_pct", _lib.ptr(Xd), _lib.ptr(pdate), _lib.ptr(soff), _lib.ptr(scol), J, D, A, _lib.ptr(lo),
              _lib.ptr(hi), _lib.ptr(lohi), _lib.stream_ptr())
    return lohi.cpu().numpy()


@pytest.mark.parametrize("p", panels(), ids=panel_ids())
def test_wcomp_pct_vs_oracle(gpu, p):
    """k_wcomp_pct: (lo, hi, nv) of every (selection row, suffix) pool, bit-exact."""
    torch, cf, E, _ = gpu
    plan, dev = _plan(torch, cf, p)
    got = _wcomp_pct(gpu, _up(torch, p["X"]), dev["pdate"], dev["soff"], dev["scol"])
    ref = OC.weighted_percentiles(p["X"], p["names"], p["sd"], p["W"], p["P"])
    assert np.array_equal(got[..., 2], ref[..., 2])
    _check(got, ref, True, "lohi")


@pytest.mark.parametrize("p", panels(), ids=panel_ids())
def test_wcomp_proxy_vs_oracle(gpu, p):
    """k_wcomp_proxy on the oracle's pooled percentiles: bit-exact on the present cells."""
    torch, cf, E, _lib = gpu
    plan, dev = _plan(torch, cf, p)
    F, D, A = p["X"].shape
    J, G = len(p["sd"]), max(1, int(plan["ngrp"].max()))
    lohi = OC.weighted_percentiles(p["X"], p["names"], p["sd"], p["W"], p["P"])
    Xd, lh = _up(torch, p["X"]), _up(torch, lohi)
    P = torch.full((G, J, A), -7.0, dtype=torch.float64, device="cuda")
    _lib.call("fmx_wcomp_proxy", _lib.ptr(Xd), _lib.ptr(dev["pdate"]), _lib.ptr(dev["ncol"]), _lib.ptr(dev["col"]),
              _lib.ptr(dev["suf"]), _lib.ptr(dev["grp"]), int(plan["KMAX"]), J, D, A, _lib.ptr(lh), G, _lib.ptr(P),
              _lib.stream_ptr())
    got = P.cpu().numpy()
    ref = OC.weighted_proxies(p["X"], p["names"], p["sd"], p["W"], lohi, p["P"])
    assert ref.shape == got.shape
    presJ = p["present"][np.maximum(p["sd"], 0)]          # [J][A]; rows that yield nothing are all NaN
    for i, d in enumerate(plan["pdate"]):
        if d < 0:
            presJ[i] = True
    _check(got[:, presJ], ref[:, presJ], True, "weighted proxy")


@pytest.mark.parametrize("p", panels(), ids=panel_ids())
def test_wcomp_combine_vs_oracle(gpu, p):
    """k_wcomp_combine on the oracle's normalised proxies: bit-exact on the dense panels, the
    project tolerance on the ragged ones (measured on the MI355X: max |got - ref| 2.2e-16);
    every cell the reference's fillna(0) fills (a NaN composite, a date no row selects, an
    absent row) is exactly 0 on every panel."""
    torch, cf, E, _lib = gpu
    plan, dev = _plan(torch, cf, p)
    F, D, A = p["X"].shape
    J = len(p["sd"])
    lohi = OC.weighted_percentiles(p["X"], p["names"], p["sd"], p["W"], p["P"])
    prox = OC.weighted_proxies(p["X"], p["names"], p["sd"], p["W"], lohi, p["P"])
    pres = _pres(torch, p)
    for meth in ("zscore", "rank"):
        nrm = OC.weighted_normalise(prox, p["sd"], meth, p["P"])
        Nd = _up(torch, nrm)
        out = torch.zeros((D, A), dtype=torch.float64, device="cuda")
        _lib.call("fmx_wcomp_combine", _lib.ptr(Nd), _lib.ptr(dev["pdate"]), _lib.ptr(dev["ngrp"]), _lib.ptr(dev["gw"]),
                  int(plan["KMAX"]), J, D, A, _lib.ptr(pres), _lib.ptr(out), _lib.stream_ptr())
        ref = OC.weighted_combine(nrm, p["names"], p["sd"], p["W"], D, p["P"])
        got = out.cpu().numpy()
        _check(got, ref, not p["ragged"], f"weighted combine {meth}")
        filled = np.isnan(OC.weighted_combine(nrm, p["names"], p["sd"], p["W"], D, p["P"], fillna=False))
        assert filled.any() and not got[filled].any(), f"weighted combine {meth}: fillna(0) cells are not exactly 0"


# ------------------------------------------------------------------ c. radix-select rows
@pytest.mark.parametrize("label,row", select_rows(), ids=[r[0] for r in select_rows()])
def test_select_row_percentiles(gpu, label, row):
    """One row as a D = 1 panel: k_wcomp_pct must return numpy's (lo, hi) of the sorted
    non-NaN values bit for bit, and k_comp_adj the four suffix scalings built on them."""
    torch, cf, E, _ = gpu
    A = row.size
    Xd = _up(torch, row.reshape(1, 1, A))
    # selection row j pools column 0 under suffix j + 1
    soff = np.zeros(17, dtype=np.int32)
    for j in range(4):
        soff[j * 4 + j + 1:] += 1
    got = _wcomp_pct(gpu, Xd, _up(torch, np.zeros(4, np.int32)), _up(torch, soff), _up(torch, np.zeros(4, np.int32)))
    adj = E.comp_adj(Xd, [0, 0, 0, 0], [1, 2, 3, 4]).cpu().numpy()
    for j in range(4):
        lo, hi, nv = percentiles(row, j + 1)
        assert got[j, j, 2] == nv, (label, j)
        assert_close(got[j, j, :2], np.array([lo, hi]), exact=True, what=f"{label} lohi suffix {j + 1}")
        others = np.delete(got[j], j, axis=0)
        assert np.isnan(others[:, :2]).all() and (others[:, 2] == -1).all()
        ref = np.zeros(A) if lo == hi else OC._scale(SUFFIXES[j], row, lo, hi)
        assert_close(adj[j, 0], ref, exact=True, what=f"{label} adj suffix {j + 1}")


@pytest.mark.parametrize("label,X", pooled_rows(), ids=[r[0] for r in pooled_rows()])
def test_pooled_percentiles_cross_columns(gpu, label, X):
    """Three columns pooled under one suffix (the middle one all NaN): n = 3 A values walked
    across the column boundaries."""
    torch, cf, E, _ = gpu
    soff = np.zeros(17, dtype=np.int32)
    for j in range(4):
        soff[j * 4 + j + 1:] += 3
    scol = np.tile(np.array([0, 1, 2], np.int32), 4)
    got = _wcomp_pct(gpu, _up(torch, X), _up(torch, np.zeros(4, np.int32)), _up(torch, soff), _up(torch, scol))
    for j in range(4):
        lo, hi, nv = percentiles(X, j + 1)
        assert got[j, j, 2] == nv
        assert_close(got[j, j, :2], np.array([lo, hi]), exact=True, what=f"{label} pooled suffix {j + 1}")


# ------------------------------------------------------------------ d. combine_lds boundary
def _combine_lds(A):
    return 8 * A + 8 * (2 * (A // 64) + 8) + 128


def _combine_input(A):
    rng = np.random.default_rng(A)
    nrm = rng.standard_normal((2, 1, A))
    nrm[rng.random(nrm.shape) < 0.03] = np.nan
    nrm[:, 0, 5] = np.nan                                 # a cell no proxy covers
    return nrm


@pytest.mark.parametrize("A", [8200, 19838])
def test_combine_large_rows_vs_oracle(gpu, A):
    """Rows whose LDS footprint passes 64 KiB (the kernel's dynamic-LDS attribute is raised)
    up to the largest row the host check accepts, exactly 160 KiB: bit-exact in both modes."""
    torch, cf, E, _ = gpu
    assert 64 * 1024 < _combine_lds(A) <= LDS_LIMIT and (A != 19838 or _combine_lds(A) == LDS_LIMIT)
    nrm = _combine_input(A)
    Nd = _up(torch, nrm)
    for mode in (0, 1):
        got = E.comp_combine(Nd, mode).cpu().numpy()
        _check(got, OC.combine(nrm, mode), True, f"combine A={A} mode {mode}")


def test_combine_refuses_rows_past_the_lds_limit(gpu):
    """A = 19 839 needs more than 160 KiB: refused on the host, before any launch, and the
    output is left as it was."""
    torch, cf, E, _lib = gpu
    A = 19839
    assert _combine_lds(A) > LDS_LIMIT >= _combine_lds(A - 1)
    Nd = _up(torch, _combine_input(A))
    for mode in (0, 1):
        out = torch.full((1, A), 7.0, dtype=torch.float64, device="cuda")
        with pytest.raises(_lib.FmxError, match="too large"):
            _lib.call("fmx_comp_combine", _lib.ptr(Nd), 2, 1, A, mode, None, _lib.ptr(out), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
    pdate, ngrp = _up(torch, np.zeros(1, np.int32)), _up(torch, np.full(1, 2, np.int32))
    gw = _up(torch, np.array([[0.25, 0.75]]))
    out = torch.full((1, A), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.FmxError, match="too large"):
        _lib.call("fmx_wcomp_combine", _lib.ptr(Nd), _lib.ptr(pdate), _lib.ptr(ngrp), _lib.ptr(gw), 2, 1, 1, A, None,
                  _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
