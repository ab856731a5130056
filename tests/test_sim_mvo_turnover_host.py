"""Host side of the native ``Simulation(method="mvo_turnover")`` (no GPU needed):

* the L1 certificate ``kkt_violation_l1`` accepts the numpy model's optimum and rejects it after
  one mover is displaced by 1e-4; the two SLSQP forms agree with the model where each applies;
* the stepper's p alignment equals what the reference's ``_get_previous_weights`` describes
  (yesterday's weight for the symbols both days share, 0 for the others);
* routing: only ``FMX_SIM_MVO_TURNOVER=native`` (with a GPU, the cvxpy path, tau >= 0, a finite
  return weight and inputs inside the caps) leaves the reference loader;
* the new C symbols are exported and bound.
"""
import os

import numpy as np
import pandas as pd
import pytest

import sim_mvo_cases as SC
import sim_mvo_turnover_cases as TC


def _chain(A, T, J, seed, tau, r):
    """The spec chain on the CPU: [(Sigma, sg, p, x, wopt, book, status)] per date."""
    R0, rows, X, P, u = TC.make_chain(A, T, J, seed)
    out, prev = [], None
    for j in range(J):
        book, wopt, st, p = TC.chain_step(R0[rows[j]], X[j], P[j], prev, None if j == 0 else P[j - 1], u, 0.1, tau, r)
        out.append((SC.sigma_from_window(R0[rows[j]], 0.1), SC.signs(X[j], P[j]), p, np.nan_to_num(X[j]), wopt, book, st))
        prev = book
    return out, u


@pytest.mark.parametrize("tau,r", [(0.1, 0.0), (1e-6, 1e-4)], ids=["dominant", "mixed"])
def test_certificate_accepts_the_optimum_and_rejects_a_displaced_mover(tau, r):
    days, u = _chain(12, 10, 4, 5, tau, r)
    moved_days = 0
    for j, (Sig, sg, p, x, w, book, st) in enumerate(days):
        assert st == 0
        q = 2.0 * Sig @ w - r * x
        viol, scale = TC.kkt_violation_l1(q, w, sg, u, p, tau)
        print(f"tau {tau} date {j}: violation {viol:.2e} of scale {scale:.2e}")
        assert viol <= 1e-6 * scale
        lo, hi = TC.box(sg, u)
        movers = np.flatnonzero((sg != 0) & (w != p) & (w > lo + 1e-3) & (w < hi - 1e-3))
        same = [i for i in movers if ((sg == sg[i]) & (w > lo + 1e-3) & (w < hi - 1e-3)).sum() >= 2]
        if not same:
            continue
        i = same[0]                                           # move weight 1e-4 between two interior cells of a leg
        k = [m for m in np.flatnonzero((sg == sg[i]) & (w > lo + 1e-3) & (w < hi - 1e-3)) if m != i][0]
        w2 = w.copy()
        w2[i] += 1e-4
        w2[k] -= 1e-4
        viol2, scale2 = TC.kkt_violation_l1(2.0 * Sig @ w2 - r * x, w2, sg, u, p, tau)
        print(f"tau {tau} date {j}: displaced violation {viol2:.2e} of scale {scale2:.2e}")
        assert viol2 > 1e-6 * scale2
        moved_days += 1
    assert moved_days >= 1


def test_mixed_regime_has_up_and_down_movers_in_one_leg():
    days, u = _chain(12, 10, 4, 5, 1e-6, 1e-4)
    both = 0
    for Sig, sg, p, x, w, book, st in days[1:]:
        for leg in (1, -1):
            k = sg == leg
            both += bool((w[k] > p[k]).any() and (w[k] < p[k]).any())
    assert both >= 1


def test_slsqp_forms_agree_with_the_model():
    """Dominant tau: the tightened-bounds QP (its precondition asserted); small tau: the split."""
    days, u = _chain(12, 10, 4, 5, 0.1, 0.0)
    for j, (Sig, sg, p, x, w, book, st) in enumerate(days):
        assert 2 * 0.1 > TC.leg_spread(2.0 * Sig @ w, sg)
        err = np.abs(w - TC.slsqp_dominant(Sig, sg, u, p, x, 0.0)).max()
        print(f"dominant date {j}: |w - slsqp| = {err:.2e}")
        assert err <= 1e-6
    days, u = _chain(12, 10, 4, 5, 1e-6, 1e-4)
    for j, (Sig, sg, p, x, w, book, st) in enumerate(days):
        err = np.abs(w - TC.slsqp_split(Sig, sg, u, p, x, 1e-6, 1e-4)).max()
        print(f"split date {j}: |w - slsqp| = {err:.2e}")
        assert err <= 1e-6


def _previous_weights(prev: pd.Series, current_symbols):
    """portfolio_simulation.py:206-225 in one line: the last book on today's symbols, 0 for new ones."""
    return prev.reindex(current_symbols).fillna(0.0)


def test_p_alignment_on_a_ragged_panel():
    syms = np.array(["A", "B", "C", "D", "E"])
    #            A  B  C  D  E
    P = np.array([[1, 1, 1, 0, 1],      # day 0
                  [1, 0, 1, 1, 1],      # day 1: B absent, D appears
                  [1, 1, 0, 1, 1]],     # day 2: B back (absent on day 1 -> p = 0), C disappears
                 dtype=np.uint8)
    books = np.array([[0.5, 0.5, -1.0, np.nan, 0.0],
                      [1.0, np.nan, -0.25, -0.75, 0.0]])
    for j in (1, 2):
        got = TC.align_prev(books[j - 1], P[j - 1])
        prev = pd.Series(books[j - 1][P[j - 1] != 0], index=syms[P[j - 1] != 0])
        want = _previous_weights(prev, syms[P[j] != 0])
        assert np.array_equal(got[P[j] != 0], want.to_numpy())
    assert TC.align_prev(books[1], P[1])[1] == 0.0            # B: no row on day 1
    assert TC.align_prev(books[0], P[0])[3] == 0.0            # D: appears on day 1
    assert TC.align_prev(None, None) is None                  # the first date: all zeros in chain_step
    # and through the stepper: a flat day's zeros are the next day's p
    R0, rows, X, Pc, u = TC.make_chain(9, 5, 3, 3)
    X[1] = np.abs(X[1])                                        # day 1: one leg only
    b0, _, st0, _ = TC.chain_step(R0[rows[0]], X[0], Pc[0], None, None, u, 0.1, 0.1, 0.0)
    b1, _, st1, p1 = TC.chain_step(R0[rows[1]], X[1], Pc[1], b0, Pc[0], u, 0.1, 0.1, 0.0)
    b2, _, st2, p2 = TC.chain_step(R0[rows[2]], X[2], Pc[2], b1, Pc[1], u, 0.1, 0.1, 0.0)
    assert (st0, st1, st2) == (0, 3, 0) and np.array_equal(p1, np.nan_to_num(b0)) and not p2.any()


def test_post_solve_prunes_and_renormalises():
    sg = np.array([1, 1, 1, -1, -1, 0])
    w = np.array([0.6, 0.4 - 5e-7, 5e-7, -1.0 + 2e-7, -2e-7, 0.0])
    o = TC.post_solve(w, sg)
    assert o[2] == 0.0 and o[4] == 0.0 and o[5] == 0.0
    assert o[0] == 0.6 / (0.6 + (0.4 - 5e-7)) and o[3] == -1.0
    # a leg that prunes to nothing: the unpruned solution is kept
    w = np.array([1.0, 0.0, 0.0, -5e-7, -5e-7, 0.0])
    assert np.array_equal(TC.post_solve(w, sg), w)


# ---------------------------------------------------------------------------- routing
def _sim(PS, **kw):
    rng = np.random.default_rng(0)
    dates = pd.bdate_range("2021-01-04", periods=8)
    idx = pd.MultiIndex.from_product([dates, [f"S{i}" for i in range(6)]], names=["date", "symbol"])
    ret = pd.Series(0.01 * rng.standard_normal(len(idx)), index=idx)
    one = pd.Series(1.0, index=idx)
    feat = pd.Series(rng.standard_normal(len(idx)), index=idx)
    s = PS.SimulationSettings(returns=ret, cap_flag=one, investability_flag=one, factors_df=pd.DataFrame(index=idx),
                              method="mvo_turnover", lookback_period=5, plot=False, **kw)
    return PS.Simulation("sig", feat, s)


@pytest.fixture
def routes(monkeypatch):
    """A faked GPU, the reference loader and the native trade list replaced by recorders."""
    import torch
    import factormodeling_amd._refload as RL
    import factormodeling_amd.portfolio_simulation as PS
    calls = []

    class Reached(Exception):
        pass

    def load(filename, what):
        calls.append(("reference", filename))
        raise Reached(filename)

    def native(*a, **k):
        calls.append(("native", a[2:], k))
        raise Reached("native")
    monkeypatch.setattr(RL, "load", load)
    monkeypatch.setattr(PS, "mvo_turnover_trade_list", native, raising=False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.delenv("FMX_SIM_MVO", raising=False)
    monkeypatch.delenv("FMX_SIM_MVO_TURNOVER", raising=False)
    return PS, calls, Reached


def test_routing_native_switch_reaches_the_device_path(routes, monkeypatch):
    PS, calls, Reached = routes
    monkeypatch.setenv("FMX_SIM_MVO_TURNOVER", "native")
    with pytest.raises(Reached):
        _sim(PS, turnover_penalty=0.05, return_weight=1e-4, max_weight=0.4, pct=0.3,
             shrinkage_intensity=0.2)._daily_trade_list()
    assert len(calls) == 1 and calls[0][0] == "native"
    # pct, max_weight, lookback_period, shrinkage_intensity, turnover_penalty, return_weight
    assert calls[0][1] == (0.3, 0.4, 5, 0.2, 0.05, 1e-4) and calls[0][2] == {"return_info": True}


def test_routing_keeps_the_reference_otherwise(routes, monkeypatch):
    PS, calls, Reached = routes

    def reaches_reference(sim):
        del calls[:]
        with pytest.raises(Reached):
            sim._daily_trade_list()
        return calls == [("reference", "portfolio_simulation.py")]
    assert reaches_reference(_sim(PS))                                     # the variable unset
    monkeypatch.setenv("FMX_SIM_MVO_TURNOVER", "native")
    assert reaches_reference(_sim(PS, use_cvxpy=False))
    assert reaches_reference(_sim(PS, turnover_penalty=-0.1))
    assert reaches_reference(_sim(PS, return_weight=float("nan")))
    sim = _sim(PS)
    sim.lookback_period = 65                                               # past the window cap
    assert reaches_reference(sim)
    monkeypatch.setenv("FMX_SIM_MVO", "reference")
    assert reaches_reference(_sim(PS))
    monkeypatch.delenv("FMX_SIM_MVO")
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert reaches_reference(_sim(PS))


# ---------------------------------------------------------------------------- C ABI
def test_new_symbols_are_declared_exported_and_bound():
    from factormodeling_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "fmx.h")).read()
    names = ("fmx_sim_mvo_turnover_books", "fmx_sim_mvo_turnover_books_work_bytes")
    for n in names:
        assert n + "(" in header and n in L.SIGNATURES
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libfmx.so not built (run __graft_entry__.build())")
    lib = L.load()
    for n in names:
        assert hasattr(lib, n)
    # one 16-double header and an Lmax x Lmax matrix per (chain, date)
    assert lib.fmx_sim_mvo_turnover_books_work_bytes(5000, 20, 7, 3) == 8 * 3 * 7 * (16 + 400)
    assert lib.fmx_sim_mvo_turnover_books_work_bytes(5000, 65, 7, 3) == 0
