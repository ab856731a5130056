"""All MVO managers of ``compute_multimanager_weights`` in one device pass:
``engine.sim_mvo_window_rows`` (fmx_sim_mvo_window_rows), ``engine.sim_mvo_turnover_chains``
(fmx_sim_mvo_turnover_chains), ``simulation.mvo_manager_books`` and the routing in
``multi_manager.compute_multimanager_weights``.

The panel is tests/mm_mvo_cases.ragged_case (5 managers, 12 dates, lookback 5) at A = 24 and at
A = 1,030 (two elements per thread).  Three yardsticks: the per-manager native path
(``mvo_trade_list`` / ``mvo_turnover_trade_list`` on each manager's dropna() series: same bits),
the KKT certificates of sim_mvo_cases / sim_mvo_turnover_cases on Sigma from the specification's
window, and the reference's own run (tests/golden/mm_mvo_ragged.npz).  Each test prints the
figures it asserts on.
"""
import functools
import logging
import math
import os

import numpy as np
import pandas as pd
import pytest

import mm_mvo_cases as MC
import sim_mvo_cases as SC
import sim_mvo_turnover_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = (24, 1030)
F, D, L, S = MC.F, MC.D, MC.LOOKBACK, MC.SHRINK
RW = 1e-4                       # the run with return_weight != 0
RUNS = [("mvo", 0.0), ("mvo_turnover", 0.0), ("mvo_turnover", RW)]
RUN_IDS = ["mvo", "turnover", "turnover-rw"]


def _engine():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import factormodeling_amd.engine as E
    return E, torch


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@functools.lru_cache(maxsize=None)
def _batched(A, method, rw, chunk_bytes=None):
    """mvo_manager_books on the case: (Wf, cnt, extra) as numpy."""
    _engine()
    from factormodeling_amd.simulation import mvo_manager_books
    c = MC.ragged_case(A)
    Wf, cnt, extra = mvo_manager_books(c.factors_df, c.names, c.returns, method, MC.PCT, c.u, L, S, return_weight=rw,
                                       return_info=True, chunk_bytes=chunk_bytes)
    return Wf.cpu().numpy(), cnt.cpu().numpy(), extra


@functools.lru_cache(maxsize=None)
def _per_manager(A, method, rw):
    """The parent's native path, one manager at a time, scattered onto the panel grid:
    (Wf [F][D][A], cnt [F][D][2], books [F][D][A], status [F][D] (NaN: not a date of the manager))."""
    _engine()
    from factormodeling_amd.simulation import mvo_trade_list, mvo_turnover_trade_list
    c = MC.ragged_case(A)
    Wf, cnt = np.full((F, D, A), np.nan), np.full((F, D, 2), np.nan)
    books, status = np.full((F, D, A), np.nan), np.full((F, D), np.nan)
    for f, ser in enumerate(c.series):
        if method == "mvo":
            sh, cn, ex = mvo_trade_list(ser, c.returns, MC.PCT, c.u, L, S, return_info=True)
        else:
            sh, cn, ex = mvo_turnover_trade_list(ser, c.returns, MC.PCT, c.u, L, S, return_weight=rw, return_info=True)
        Wf[f], cnt[f] = MC.scatter(c, sh, cn)
        assert list(ex["symbols"]) == list(c.syms), "the manager's own grid has the panel's columns"
        d = c.fdates.get_indexer(ex["dates"])
        books[f, d] = ex["books"]
        status[f, d] = ex["info"][:, 0]
    return Wf, cnt, books, status


def _masks(c):
    """(fpresent [F][D][A] uint8, rpresent [Dr][A] uint8, nbefore [D]) from the specification."""
    fp = (~np.isnan(c.X)).astype(np.uint8)
    rp = np.zeros((len(c.rdates), c.A), dtype=np.uint8)
    rp[c.rdates.get_indexer(c.returns.index.get_level_values(0)),
       pd.Index(c.syms).get_indexer(c.returns.index.get_level_values(1))] = 1
    nb = np.searchsorted(c.rdates.values, c.fdates.values, side="left").astype(np.int32)
    return fp, rp, nb


# ---------------------------------------------------------------------------- 1. windows
@pytest.mark.parametrize("A", SIZES)
@pytest.mark.parametrize("lookback", [L, 1, 64])
def test_windows_match_the_single_manager_search(A, lookback):
    E, torch = _engine()
    from factormodeling_amd.simulation import mvo_window_rows
    c = MC.ragged_case(A)
    fp, rp, nb = _masks(c)
    rows, T = E.sim_mvo_window_rows(torch.as_tensor(fp.reshape(F * D, A), device=DEV), torch.as_tensor(rp, device=DEV),
                                    torch.as_tensor(np.tile(nb, F), device=DEV), lookback)
    rows, T = rows.cpu().numpy().reshape(F, D, -1), T.cpu().numpy().reshape(F, D)
    assert rows.shape[2] == min(lookback, len(c.rdates)) and rows.dtype == np.int32 and T.dtype == np.int32
    differ = 0
    for f, ser in enumerate(c.series):
        wr, wt = mvo_window_rows(ser.index, c.returns, lookback, device="cpu")
        wr, wt = wr.numpy(), wt.numpy()
        own = c.fdates.get_indexer(ser.index.get_level_values(0).unique().sort_values())
        assert len(own) == len(wt)
        for k, d in enumerate(own):
            assert T[f, d] == wt[k]
            assert list(rows[f, d, :T[f, d]]) == list(wr[k, :wt[k]])
            assert (rows[f, d, T[f, d]:] == 0).all()
            differ += list(rows[f, d, :T[f, d]]) != list(rows[0, d, :T[0, d]])
        absent = np.setdiff1d(np.arange(D), own)
        assert (T[f, absent] == 0).all()                      # no present symbol: no candidate
    assert (T[:, 0] == 0).all()                               # the first date precedes all returns
    if lookback < 64:
        assert differ > 0, "some manager's window differs from manager 0's on the same date"
    print(f"A {A} lookback {lookback}: window lengths {sorted(set(T.reshape(-1).tolist()))}, "
          f"{differ} (manager, date) windows differ from manager 0's")


def test_windows_without_any_earlier_returns_date():
    E, torch = _engine()
    c = MC.ragged_case(24)
    fp, rp, _ = _masks(c)
    zero = torch.zeros(F * D, dtype=torch.int32, device=DEV)     # every returns date is later than every feature date
    rows, T = E.sim_mvo_window_rows(torch.as_tensor(fp.reshape(F * D, 24), device=DEV), torch.as_tensor(rp, device=DEV),
                                    zero, L)
    assert not T.any() and not rows.any() and tuple(rows.shape) == (F * D, L)
    rows, T = E.sim_mvo_window_rows(torch.as_tensor(fp.reshape(F * D, 24), device=DEV),
                                    torch.zeros((0, 24), dtype=torch.uint8, device=DEV), zero, L)   # no returns at all
    assert not T.any() and not rows.any() and tuple(rows.shape) == (F * D, 1)


# ---------------------------------------------------------------------------- 2. the per-manager bits
@pytest.mark.parametrize("A", SIZES)
@pytest.mark.parametrize("method,rw", RUNS, ids=RUN_IDS)
def test_same_bits_as_the_per_manager_native_path(A, method, rw):
    Wf, cnt, extra = _batched(A, method, rw)
    Wp, cp, bp, sp = _per_manager(A, method, rw)
    st = extra["info"][:, :, 0]
    print(f"A {A} {method} rw {rw}: statuses {sorted(set(st.reshape(-1).tolist()))}, "
          f"{int(np.isnan(Wf).sum())} NaN weights, iterations up to {extra['info'][:, :, 1].max():.0f}")
    assert np.array_equal(np.isnan(Wf), np.isnan(Wp)) and np.array_equal(np.isnan(cnt), np.isnan(cp))
    assert _same(Wf, Wp), f"largest difference {np.nanmax(np.abs(Wf - Wp)):.3e}"
    assert _same(cnt, cp)
    assert _same(extra["books"], bp)
    assert np.array_equal(np.where(st == 5, np.nan, st), sp, equal_nan=True)


# ---------------------------------------------------------------------------- 3. independent optimality
def _prev_book(books, f, d):
    """(book, date) of manager f's last date before d on which it had rows, or (None, None)."""
    for k in range(d - 1, -1, -1):
        if not np.isnan(books[f, k]).all():
            return books[f, k], k
    return None, None


@pytest.mark.parametrize("A", SIZES)
@pytest.mark.parametrize("method,rw", RUNS, ids=RUN_IDS)
def test_kkt_certificates_on_the_specification_sigma(A, method, rw):
    c = MC.ragged_case(A)
    _, _, extra = _batched(A, method, rw)
    info, books = extra["info"], extra["books"]
    opt = extra["opt"] if method == "mvo_turnover" else books
    tau = 0.1
    solved, worst = 0, 0.0
    for f, ser in enumerate(c.series):
        for d in range(D):
            if info[f, d, 0] != 0:
                continue
            solved += 1
            x = ser.xs(c.fdates[d], level=0)
            cols = pd.Index(c.syms).get_indexer(x.index)
            Xw = SC.spec_window(c.returns, list(x.index), c.fdates[d], L)
            w, sg = opt[f, d, cols], SC.signs(x.to_numpy())
            assert np.isnan(np.delete(opt[f, d], cols)).all() and not np.isnan(w).any()
            q = 2.0 * SC.sigma_times(Xw, S, w)
            if method == "mvo":
                viol, scale = SC.kkt_violation(q, w, sg, c.u)
            else:
                pb, k = _prev_book(books, f, d)
                p = np.zeros(A) if pb is None else TC.align_prev(pb, None)
                viol, scale = TC.kkt_violation_l1(q - rw * x.to_numpy(), w, sg, c.u, p[cols], tau)
            worst = max(worst, viol / scale)
            assert viol <= 1e-6 * scale, (f, d, viol, scale)
            assert abs(math.fsum(w[sg > 0]) - 1.0) <= 1e-9 and abs(math.fsum(w[sg < 0]) + 1.0) <= 1e-9
            assert (w[sg > 0] >= 0).all() and (w[sg > 0] <= c.u).all()
            assert (w[sg < 0] <= 0).all() and (w[sg < 0] >= -c.u).all() and (w[sg == 0] == 0).all()
    print(f"A {A} {method} rw {rw}: {solved} solved (manager, date) pairs, largest KKT violation / scale {worst:.3e}")
    assert solved >= 40


@pytest.mark.parametrize("A", SIZES)
def test_the_book_before_a_gap_is_the_previous_book_after_it(A):
    """Manager 2 has no rows on two dates: the day after, p is the book from before the gap."""
    c = MC.ragged_case(A)
    _, _, extra = _batched(A, "mvo_turnover", 0.0)
    _, _, plain = _batched(A, "mvo", 0.0)
    info, books, opt = extra["info"], extra["books"], extra["opt"]
    f, d, before = 2, MC.GAP[1] + 1, MC.GAP[0] - 1
    assert list(info[f, MC.GAP[0]:d + 1, 0]) == [5, 5, 0] and info[f, before, 0] == 0
    pb, k = _prev_book(books, f, d)
    assert k == before
    p = TC.align_prev(pb, None)
    assert np.abs(p).sum() > 1.9                                  # a full book, not zeros
    x = c.X[f, d]
    sg = SC.signs(x)
    Xw = SC.spec_window(c.returns, list(c.syms), c.fdates[d], L)
    w = opt[f, d]
    q = 2.0 * SC.sigma_times(Xw, S, w)
    viol, scale = TC.kkt_violation_l1(q, w, sg, c.u, p, 0.1)
    v0, s0 = TC.kkt_violation_l1(q, w, sg, c.u, np.zeros(A), 0.1)
    # A weight that is what it is only through the turnover term: the shrunk Sigma is close to a
    # multiple of I, so the plain minimum-variance book has no zeros to compare against (every
    # cell of a leg gets weight); what the variance alone cannot produce is a nonzero weight equal
    # TO THE BIT to the pre-gap book's -- the kink of tau |w - p| at p -- and away from the plain book.
    held = (w == p) & (p != 0) & (sg != 0)
    pw = plain["books"][f, d]
    only_turnover = held & (np.abs(w - pw) > 1e-3 * c.u)
    print(f"A {A}: p from date {k}; KKT violation {viol:.3e} with it (bound {1e-6 * scale:.3e}), {v0:.3e} with zeros; "
          f"{int(held.sum())} cells held at p != 0, {int(only_turnover.sum())} of them more than {1e-3 * c.u:.1e} from "
          f"the plain mvo book ({int((pw[sg != 0] == 0).sum())} zeros in it)")
    assert viol <= 1e-6 * scale
    assert v0 > 1e-6 * s0, "with p = 0 the certificate fails: the check sees which book was carried"
    assert only_turnover.any(), "a weight that is nonzero only because the turnover term holds it at p"


# ---------------------------------------------------------------------------- 4. absent and degenerate dates
@pytest.mark.parametrize("A", SIZES)
def test_absent_and_degenerate_dates_of_the_chains(A):
    E, torch = _engine()
    c = MC.ragged_case(A)
    Wf, cnt, extra = _batched(A, "mvo_turnover", 0.0)
    info, books, opt = extra["info"], extra["books"], extra["opt"]
    st = info[:, :, 0]
    absent = [(2, MC.GAP[0]), (2, MC.GAP[1])] + [(4, d) for d in range(MC.LATE)]
    assert sorted(zip(*np.nonzero(st == 5))) == sorted(absent)
    for f, d in absent:
        assert np.isnan(books[f, d]).all() and np.isnan(opt[f, d]).all() and np.isnan(cnt[f, d]).all()
    for d in (MC.SINGLE, MC.ONE_SIDED):                           # one row; one leg only: flat, zero book, counts 0
        assert st[3, d] == 3 and list(cnt[3, d]) == [0, 0]
        pr = ~np.isnan(c.X[3, d])
        assert (books[3, d][pr] == 0).all() and np.isnan(books[3, d][~pr]).all()
    # the flat zero book does become the next p: the next date's certificate holds with p = 0 on
    # every cell and fails with the book of the date before the one-row date
    d = MC.SINGLE + 1
    assert st[3, d] == 0 and st[3, MC.SINGLE - 1] == 0
    w, sg = opt[3, d], SC.signs(c.X[3, d])
    q = 2.0 * SC.sigma_times(SC.spec_window(c.returns, list(c.syms), c.fdates[d], L), S, w)
    v_zero, s_zero = TC.kkt_violation_l1(q, w, sg, c.u, np.zeros(A), 0.1)
    v_old, s_old = TC.kkt_violation_l1(q, w, sg, c.u, TC.align_prev(books[3, MC.SINGLE - 1], None), 0.1)
    print(f"A {A}: after the one-row date, KKT violation {v_zero:.3e} with p = 0 (bound {1e-6 * s_zero:.3e}), "
          f"{v_old:.3e} with the book before it")
    assert v_zero <= 1e-6 * s_zero and v_old > 1e-6 * s_old
    # status 4: the batched equal-weight book
    X = torch.as_tensor(c.X, device=DEV)
    _, ce, we = E.trade_books(X, "equal", MC.PCT, c.u, nan_absent=True, raw=True)
    four = sorted(zip(*np.nonzero(st == 4)))
    assert four == [(f, 0) for f in range(4)]
    for f, d in four:
        assert _same(books[f, d], we[f, d].cpu().numpy()) and _same(cnt[f, d], ce[f, d].cpu().numpy())
        assert _same(opt[f, d], books[f, d])
    print(f"A {A}: statuses by manager {[sorted(set(st[f].tolist())) for f in range(F)]}")


def test_shared_tables_without_skipping_are_the_books_entry_point():
    E, torch = _engine()
    A, T, J, B = 300, 12, 4, 3
    R0, rows, X0, P0, u = TC.make_chain(A, T, J, 77, ragged=True)
    Xs, Ps = [X0], [P0]
    for b in range(1, B):
        _, _, Xb, Pb, _ = TC.make_chain(A, T, J, 77 + b, ragged=True)
        Xs.append(Xb)
        Ps.append(Pb)
    Ps[1][2] = 0                                                  # chain 1 has no row on date 2
    X, P = np.where(np.stack(Ps) != 0, np.stack(Xs), np.nan), np.stack(Ps)
    t = lambda a: torch.as_tensor(a, device=DEV)
    Tn = np.full(J, T, dtype=np.int32)
    ref = E.sim_mvo_turnover_books(t(R0), rows, Tn, t(X), t(P), None, S, u, 0.1, RW, return_opt=True)
    got = E.sim_mvo_turnover_chains(t(R0), rows, Tn, t(X), t(P), None, S, u, 0.1, RW, skip_absent=False, return_opt=True)
    for a, b in zip(ref, got):
        assert _same(a.cpu().numpy(), b.cpu().numpy())
    assert ref[2][1, 2, 0] == 3                                   # without skipping an empty date is a flat day
    # the same tables per chain, and skipping: only chain 1 changes, from its empty date on
    per = E.sim_mvo_turnover_chains(t(R0), np.broadcast_to(rows, (B, J, T)).copy(), np.broadcast_to(Tn, (B, J)).copy(),
                                    t(X), t(P), None, S, u, 0.1, RW, skip_absent=True, return_opt=True)
    assert per[2][1, 2, 0] == 5 and torch.isnan(per[1][1, 2]).all() and torch.isnan(per[0][1, 2]).all()
    for a, b in zip(ref, per):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert _same(a[[0, 2]], b[[0, 2]]) and _same(a[1, :2], b[1, :2])
    assert not _same(ref[0][1, 3].cpu().numpy(), per[0][1, 3].cpu().numpy())   # p is date 1's book, not zeros


# ---------------------------------------------------------------------------- 5. chunking
@pytest.mark.parametrize("method,rw", RUNS[:2], ids=RUN_IDS[:2])
def test_results_do_not_depend_on_the_chunking(method, rw):
    from factormodeling_amd import simulation as SIM
    A = 24
    Wf, cnt, extra = _batched(A, method, rw)
    one = SIM._manager_bytes(method, D, A, L)
    for per_chunk in (1, 2):
        W2, c2, e2 = _batched(A, method, rw, chunk_bytes=per_chunk * one + one // 2)
        assert _same(Wf, W2) and _same(cnt, c2)
        for k in extra:
            if k not in ("dates", "symbols"):
                assert _same(extra[k], e2[k])


def test_the_byte_budget_sets_the_chunk(monkeypatch):
    E, torch = _engine()
    from factormodeling_amd import simulation as SIM
    c = MC.ragged_case(24)
    calls = []
    real = E.sim_mvo_books
    monkeypatch.setattr(E, "sim_mvo_books", lambda R0, wr, wt, X, *a, **k: (calls.append(X.shape[0] // D), real(R0, wr, wt, X, *a, **k))[1])
    one = SIM._manager_bytes("mvo", D, 24, L)
    SIM.mvo_manager_books(c.factors_df, c.names, c.returns, "mvo", MC.PCT, c.u, L, S, chunk_bytes=2 * one)
    assert calls == [2, 2, 1]
    del calls[:]
    SIM.mvo_manager_books(c.factors_df, c.names, c.returns, "mvo", MC.PCT, c.u, L, S, chunk_bytes=1)
    assert calls == [1] * F
    del calls[:]
    SIM.mvo_manager_books(c.factors_df, c.names, c.returns, "mvo", MC.PCT, c.u, L, S)
    assert calls == [F]


# ---------------------------------------------------------------------------- 6. routing
def _no_loop(monkeypatch):
    import factormodeling_amd.multi_manager as MM

    def boom(*a, **k):
        raise AssertionError("compute_manager_weights: the per-manager loop ran")
    monkeypatch.setattr(MM, "compute_manager_weights", boom)
    return MM


def _fold(E, torch, c, Wf, cnt):
    cols = list(c.fw.columns)
    colmap = [c.names.index(v) if v in c.names else -1 for v in cols]
    out, oc = E.mm_combine(torch.as_tensor(Wf, device=DEV), torch.as_tensor(cnt, device=DEV), c.fw.to_numpy(), colmap,
                           c.fdates.get_indexer(c.fw.index))
    return out.cpu().numpy(), oc.cpu().numpy()


def _dense(c, w: pd.Series):
    out = np.zeros((len(c.fw.index), c.A))
    out[c.fw.index.get_indexer(w.index.get_level_values(0)), pd.Index(c.syms).get_indexer(w.index.get_level_values(1))] = w
    return out


@pytest.mark.parametrize("A", SIZES)
def test_mvo_managers_take_the_batched_route(A, monkeypatch, caplog):
    E, torch = _engine()
    from factormodeling_amd.portfolio_simulation import SimulationSettings
    monkeypatch.delenv("FMX_SIM_MVO", raising=False)
    MM = _no_loop(monkeypatch)
    c = MC.ragged_case(A)
    with caplog.at_level(logging.WARNING, logger="multi_manager"):
        w, counts = MM.compute_multimanager_weights(c.factors_df, c.fw, SimulationSettings(**MC.settings_kw(c, "mvo")))
    Wp, cp, _, sp = _per_manager(A, "mvo", 0.0)
    out, oc = _fold(E, torch, c, Wp, cp)
    assert _same(_dense(c, w), np.where(out == 0, 0.0, out))
    assert _same(counts.to_numpy(), oc) and list(counts.index) == list(c.fw.index)
    assert (w != 0).all() and w.index.is_unique
    assert any("Factor zz not in factors_df" in r.getMessage() for r in caplog.records)
    n2 = int((sp == 2).sum())
    reports = [r.getMessage() for r in caplog.records if "equal-leg fallback" in r.getMessage()]
    assert len(reports) == (1 if n2 else 0) and all(f"{n2} took" in m for m in reports)


def test_mvo_turnover_managers_route_by_the_environment(monkeypatch):
    E, torch = _engine()
    from factormodeling_amd.portfolio_simulation import SimulationSettings
    monkeypatch.delenv("FMX_SIM_MVO", raising=False)
    monkeypatch.delenv("FMX_SIM_MVO_TURNOVER", raising=False)
    MM = _no_loop(monkeypatch)
    c = MC.ragged_case(24)
    settings = SimulationSettings(**MC.settings_kw(c, "mvo_turnover"))
    with pytest.raises(AssertionError, match="the per-manager loop ran"):
        MM.compute_multimanager_weights(c.factors_df, c.fw, settings)
    with pytest.raises(AssertionError, match="the per-manager loop ran"):                # 'mvo' with the SLSQP request
        MM.compute_multimanager_weights(c.factors_df, c.fw, SimulationSettings(**MC.settings_kw(c, "mvo", use_cvxpy=False)))
    monkeypatch.setenv("FMX_SIM_MVO_TURNOVER", "native")
    w, counts = MM.compute_multimanager_weights(c.factors_df, c.fw, settings)
    Wp, cp, _, _ = _per_manager(24, "mvo_turnover", 0.0)          # settings' defaults: penalty 0.1, return_weight 0
    out, oc = _fold(E, torch, c, Wp, cp)
    assert _same(_dense(c, w), np.where(out == 0, 0.0, out)) and _same(counts.to_numpy(), oc)


# ---------------------------------------------------------------------------- 7. argument errors
def test_argument_errors_of_the_window_entry_point():
    E, torch = _engine()
    from factormodeling_amd import _lib as LB
    c = MC.ragged_case(24)
    fp, rp, nb = _masks(c)
    Dr = len(c.rdates)
    fpd, rpd = torch.as_tensor(fp[0], device=DEV), torch.as_tensor(rp, device=DEV)
    bad = nb.copy()
    bad[3] = Dr + 1
    with pytest.raises(LB.FmxError, match="nbefore"):
        E.sim_mvo_window_rows(fpd, rpd, bad, L)
    bad[3] = -1
    with pytest.raises(LB.FmxError, match="nbefore"):
        E.sim_mvo_window_rows(fpd, rpd, bad, L)
    for lb in (0, 65):
        with pytest.raises(LB.FmxError, match="lookback"):
            E.sim_mvo_window_rows(fpd, rpd, nb, lb)
    nbd = torch.as_tensor(nb, device=DEV)
    rows = torch.full((D, 64), -7, dtype=torch.int32, device=DEV)
    T = torch.full((D,), -7, dtype=torch.int32, device=DEV)
    need = int(LB.load().fmx_sim_mvo_window_rows_work_bytes(D, 24, Dr))
    work = torch.zeros(need // 8 + 1, dtype=torch.int64, device=DEV)

    def raw(fpp, rpp, nbp, Lmax, rowsp, Tp, workp, nbytes):
        LB.call("fmx_sim_mvo_window_rows", fpp, rpp, nbp, D, 24, Dr, Lmax, rowsp, Tp, workp, nbytes, LB.stream_ptr())
    ok = (LB.ptr(fpd), LB.ptr(rpd), LB.ptr(nbd), L, LB.ptr(rows), LB.ptr(T), LB.ptr(work), need)
    for Lmax in (0, 65):
        with pytest.raises(LB.FmxError, match="Lmax"):
            raw(*ok[:3], Lmax, *ok[4:])
    for k in (0, 1, 2, 4, 5):
        with pytest.raises(LB.FmxError, match="null pointer"):
            raw(*[None if i == k else v for i, v in enumerate(ok)])
    with pytest.raises(LB.FmxError, match="workspace too small"):
        raw(*ok[:6], None, need)
    with pytest.raises(LB.FmxError, match="workspace too small"):
        raw(*ok[:7], need - 8)
    torch.cuda.synchronize()
    assert (rows == -7).all() and (T == -7).all()                 # nothing was launched
    raw(*ok)
    torch.cuda.synchronize()
    assert (T.cpu().numpy() >= 0).all()


def test_argument_errors_of_the_chain_entry_point():
    E, torch = _engine()
    from factormodeling_amd import _lib as LB
    B, J, A, T = 2, 4, 9, 5
    R0, rows, X, P, u = TC.make_chain(A, T, J, 1000 * A + T)
    t = lambda a, dt=None: torch.as_tensor(a, device=DEV) if dt is None else torch.as_tensor(a, dtype=dt, device=DEV)
    X2, P2 = np.stack([X, X]), np.stack([P, P])
    rows2, Tn2 = np.stack([rows, rows]), np.full((B, J), T, dtype=np.int32)

    def run(wr, wt, **kw):
        return E.sim_mvo_turnover_chains(t(R0), wr, wt, t(X2), t(P2), None, S, u, kw.pop("tau", 0.1), kw.pop("rw", 0.0), **kw)
    bad = rows2.copy()
    bad[1, 2, 1] = R0.shape[0]                                    # in the second chain's table only
    with pytest.raises(LB.FmxError, match="outside the returns panel"):
        run(bad, Tn2)
    bad[1, 2, 1] = -1
    with pytest.raises(LB.FmxError, match="outside the returns panel"):
        run(bad, Tn2)
    badT = Tn2.copy()
    badT[1, 3] = T + 1
    with pytest.raises(LB.FmxError, match="win_T"):
        run(rows2, badT)
    with pytest.raises(LB.FmxError, match="turnover_penalty"):
        run(rows2, Tn2, tau=-1e-3)
    with pytest.raises(LB.FmxError, match="return_weight"):
        run(rows2, Tn2, rw=float("nan"))
    with pytest.raises(LB.FmxError, match="win_rows must be"):
        run(rows2[:1], Tn2)
    with pytest.raises(LB.FmxError, match="window rows supported"):
        run(np.zeros((B, J, 65), dtype=np.int32), Tn2)
    # the C entry point itself: Lmax, the chain stride, null pointers, the workspace
    R0d, rd, Td, Xd, Pd = t(R0), t(rows2, torch.int32), t(Tn2, torch.int32), t(X2), t(P2)
    W = torch.full((B, J, A), -7.0, dtype=torch.float64, device=DEV)
    cn, inf = t(np.zeros((B, J, 2))), t(np.zeros((B, J, 6)))
    need = int(LB.load().fmx_sim_mvo_turnover_chains_work_bytes(A, T, J, B))
    assert need == int(LB.load().fmx_sim_mvo_turnover_books_work_bytes(A, T, J, B))
    work = torch.zeros(need // 8, dtype=torch.float64, device=DEV)
    ok = [LB.ptr(R0d), R0.shape[0], A, LB.ptr(rd), LB.ptr(Td), T, J, LB.ptr(Xd), LB.ptr(Pd), J, B, S, u, 0.1, 0.0, 100,
          1e-9, 1, LB.ptr(W), None, LB.ptr(cn), LB.ptr(inf), LB.ptr(work), need]

    def raw(args):
        LB.call("fmx_sim_mvo_turnover_chains", *args, LB.stream_ptr())

    def with_(k, v):
        return [v if i == k else a for i, a in enumerate(ok)]
    for Lmax in (0, 65):
        with pytest.raises(LB.FmxError, match="Lmax"):
            raw(with_(5, Lmax))
    with pytest.raises(LB.FmxError, match="chain stride"):
        raw(with_(6, 1))
    for k in (0, 3, 4, 7, 18, 20, 21):
        with pytest.raises(LB.FmxError, match="null pointer"):
            raw(with_(k, None))
    with pytest.raises(LB.FmxError, match="workspace too small"):
        raw(with_(23, need - 8))
    with pytest.raises(LB.FmxError, match="workspace too small"):
        raw(with_(22, None))
    torch.cuda.synchronize()
    assert (W == -7.0).all()                                      # nothing was launched
    W.zero_()
    raw(ok)
    torch.cuda.synchronize()
    assert (inf.cpu().numpy()[:, :, 0] <= 1).all()


# ---------------------------------------------------------------------------- 8. the reference's run
def test_structure_and_variance_against_the_reference_golden():
    _engine()
    A = 24
    c = MC.ragged_case(A)
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", "mm_mvo_ragged.npz"))
    assert _same(G["X"], c.X) and _same(G["R_v"], c.returns.to_numpy()) and _same(G["fw"], c.fw.to_numpy())
    Wf, cnt, extra = _batched(A, "mvo", 0.0)
    info, books = extra["info"], extra["books"]
    worst, days = 0.0, 0
    for f, fac in enumerate(c.names):
        gd, gs, gv = G[f"book_{fac}__d"], G[f"book_{fac}__s"], G[f"book_{fac}__v"]
        rows = np.zeros((D, A), dtype=bool)
        rows[gd, gs] = True
        assert np.array_equal(~np.isnan(books[f]), rows), "the manager's book index"
        ref = np.full((D, A), np.nan)
        ref[gd, gs] = gv
        assert np.array_equal(np.isnan(Wf[f]), np.isnan(ref)), "the rows that exist after the shift, and its NaNs"
        gc = np.full((D, 2), np.nan)
        gc[G[f"book_{fac}__cd"]] = G[f"book_{fac}__c"]
        assert np.array_equal(cnt[f], gc, equal_nan=True), "the manager's counts"
        # the reference's same-day books: undo the per-symbol shift (each symbol's last row is lost)
        ser = pd.Series(gv, index=pd.MultiIndex.from_arrays([gd, gs])).sort_index()
        raw = ser.groupby(level=1).shift(-1)
        same_day = np.full((D, A), np.nan)
        same_day[raw.index.get_level_values(0), raw.index.get_level_values(1)] = raw.to_numpy()
        for d in range(D):
            pr = rows[d]
            if info[f, d, 0] != 0 or np.isnan(same_day[d][pr]).any():
                continue
            Xw = SC.spec_window(c.returns, list(c.syms[pr]), c.fdates[d], L)
            Sig = SC.sigma_from_window(Xw, S)
            w, w_ref = books[f, d][pr], same_day[d][pr]
            v, v_ref = w @ Sig @ w, w_ref @ Sig @ w_ref
            worst, days = max(worst, np.abs(w - w_ref).max()), days + 1
            assert v <= v_ref * (1 + 1e-9), (f, d, v, v_ref)
    out, oc = _fold(*_engine(), c, Wf, cnt)
    nz = np.zeros_like(out, dtype=bool)
    nz[pd.Index(G["fw_dates"]).get_indexer(G["w_d"]), G["w_s"]] = True
    assert np.array_equal(out != 0, nz), "the combined weights' index"
    np.testing.assert_array_equal(oc, G["counts"])
    gw = np.zeros_like(out)
    gw[pd.Index(G["fw_dates"]).get_indexer(G["w_d"]), G["w_s"]] = G["w_v"]
    print(f"{days} solved days compared; largest |w - w_ref| over the managers' books {worst:.3e}, "
          f"over the combined weights {np.abs(out - gw).max():.3e}")
    assert days >= 30
