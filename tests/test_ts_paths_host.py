"""tests/ts_path_cases.py pinned without a GPU: the case table reaches every dispatch arm of
fmx_ts_op / fmx_ts_set / fmx_ts_corr on both sides of each boundary, the panels hold what they
claim, every case has finite values in its oracle output unless its window is longer than the
panel, and the inf-bearing columns differ from what the pre-change oracle rule gives -- so the
GPU comparison in tests/test_gpu_ts_paths.py cannot pass vacuously."""
import numpy as np
import pytest

import ts_path_cases as TC


def _ts_cases():
    return [(arm,) + c for arm, fn in TC.TS_ARMS.items() for c in fn()]


def test_dispatch_restatement():
    P = TC.expected_path
    assert P("mean", 20, False) == "k_ts_reg<20,5>" and P("mean", 21, False) == "k_ts_rl<8>"
    assert P("rank", 10, False) == "k_ts_reg<10,10>" and P("decay", 5, False) == "k_ts_reg<5,5>"
    assert P("rank", 21, False) == P("decay", 20, True) == P("rank", 5, True) == "k_ts_win<16>"
    assert P("sum", 20, True) == P("zscore", 5, True) == P("backfill", 1, False) == "k_ts_ptr<8>"
    assert P("diff", -1, False) == P("delay", -40, True) == "k_ts_lead_ptr"
    assert P("diff", 0, True) == P("delay", 0, False) == "k_ts_window0"
    assert P("decay", 0, False) == P("decay", -3, False) == "copy" and P("decay", -3, True) == "copy+k_ts_window0"
    with pytest.raises(ValueError):
        P("mean", 0, False)
    assert TC.expected_set_path(20, 10, False) == ("k_ts_set<20,10,5>",)
    assert TC.expected_set_path(20, 5, False) == ("k_ts_mom3<4>", "k_ts_reg<5,5>", "k_ts_reg<20,5>")
    assert TC.expected_set_path(33, 10, False) == ("k_ts_mom3<4>", "k_ts_reg<10,10>", "k_ts_win<16>")
    assert TC.expected_set_path(20, 10, True) == ("k_ts_mom3<4>", "k_ts_win<16>", "k_ts_win<16>")
    assert TC.expected_corr_path(4096, False) == "k_ts_corr_fast<2>"
    assert TC.expected_corr_path(4097, False) == "k_ts_corr_rl<2>" and TC.expected_corr_path(2, True) == "k_ts_corr_ptr"
    assert TC.expected_cvf_path(4096) == "k_ts_cvf_rl<8,true>" and TC.expected_cvf_path(4097) == "k_ts_cvf_rl<8,false>"


def test_table_reaches_every_arm_and_boundary():
    want = {"reg": {"k_ts_reg<5,5>", "k_ts_reg<10,10>", "k_ts_reg<20,5>"}, "rl": {"k_ts_rl<8>"},
            "ptr": {"k_ts_ptr<8>"}, "win": {"k_ts_win<16>"}, "lead": {"k_ts_lead_ptr"},
            "window0": {"k_ts_window0", "copy", "copy+k_ts_window0"}}
    seen = {arm: set() for arm in want}
    sizes = {arm: set() for arm in want}
    for arm, ops, W, D, A, ragged in _ts_cases():
        assert 1 <= D <= 110 and A in TC.ASSETS, (arm, W, D, A)
        for op in ops:
            seen[arm].add(TC.expected_path(op, W, ragged))
        sizes[arm].add(A)
    assert seen == want
    for arm in ("reg", "rl", "ptr", "win", "lead"):
        assert sizes[arm] == set(TC.ASSETS), arm
    # k_ts_reg: both sides of the unchecked main loop (d0 + W + PF <= D), all nine ops
    for W, PF in TC.REG_PF.items():
        ds = {D for ops, w, D, A, r in TC.reg_cases() if w == W}
        assert {1, W - 1, W, W + 1, W + PF - 1, W + PF, 2 * W + PF + 1, 3 * W + 7} == ds
    assert all(len(c[0]) == 9 and not c[4] for c in TC.reg_cases())
    # the register ring's last window and the first past it; a ragged panel never takes the ring
    rl_w = {c[1] for c in TC.rl_cases()}
    assert {1, 2, 3, 21, 40, 5000} <= rl_w and not rl_w & set(TC.REG_PF)
    assert set(TC.REG_PF) <= {c[1] for c in TC.ptr_cases() if c[4]}
    assert any(c[0] == ("backfill",) and not c[4] for c in TC.ptr_cases())
    assert {(W, D) for _, W, D, _, _ in TC.rl_cases() if W == 21} >= {(21, 8), (21, 9), (21, 21), (21, 22), (21, 45)}
    assert any(W == D + 1 for _, W, D, _, _ in TC.rl_cases())
    # k_ts_win: the 16-date tile's last date and the first of the next; W around the tile
    for ragged in (False, True):
        wins = [(W, D) for _, W, D, _, r in TC.win_cases() if r == ragged]
        assert {D for _, D in wins} >= {1, 15, 16, 17, 31, 33} and {W for W, _ in wins} >= {1, 2, 3, 16, 17, 21, 40}
        assert any(D == 2 * W + 19 for W, D in wins) and any(W == D + 1 for W, D in wins)
        assert ({5, 10, 20} <= {W for W, _ in wins}) == ragged
    for D in (8, 33):
        assert {W for _, W, d, _, _ in TC.lead_cases() if d == D} == {-1, -7, -(D - 1), -D, -(D + 5)}
    assert {r for *_, r in TC.lead_cases()} == {r for *_, r in TC.window0_cases()} == {False, True}
    # fmx_ts_set
    sc = TC.set_cases()
    assert {D for arm, W, WR, D, A, r in sc if arm == "fused"} == {1, 19, 20, 21, 24, 25, 46, 67}
    for arm, W, WR, D, A, r in sc:
        assert (TC.expected_set_path(W, WR, r) == ("k_ts_set<20,10,5>",)) == (arm == "fused")
    mom = [(W, WR, r) for arm, W, WR, D, A, r in sc if arm == "mom3"]
    assert set(mom) == {(20, 5, False), (33, 10, False), (20, 10, True)}
    assert {D % 4 for arm, *_, D, A, r in sc if arm == "mom3"} == {0, 1, 3}
    assert len(TC.subsets()) == 31 and len(set(TC.subsets())) == 31
    # fmx_ts_corr
    cc = TC.corr_cases()
    fast = [c for c in cc if c[0] == "fast"]
    assert {c[1] for c in fast} == {1, 3, 4, 5} and {c[3] % 2 for c in fast} == {0, 1}
    assert {c[6] for c in fast} == {False, True} and TC.TSC_MAXW in {c[2] for c in fast}
    assert {c[2] for c in cc if c[0] == "rl"} == {TC.TSC_MAXW + 1, 5000}
    assert {c[2] for c in cc if c[0] == "ptr"} == {2, 5, 60}
    for arm, nf, W, D, A, r, pf in cc:
        assert TC.expected_corr_path(W, r) == {"fast": "k_ts_corr_fast<2>", "rl": "k_ts_corr_rl<2>",
                                               "ptr": "k_ts_corr_ptr"}[arm]
    fc = TC.feature_cases()
    assert {TC.expected_cvf_path(W) for arm, nf, W, D, A in fc if arm == "cvf"} == {"k_ts_cvf_rl<8,true>",
                                                                                   "k_ts_cvf_rl<8,false>"}
    assert {nf for _, nf, *_ in fc} == {1, 5} and {arm for arm, *_ in fc} == {"cvf", "feat"}
    assert TC.LONG_D > TC.TSC_MAXW + 1


@pytest.mark.parametrize("A", [63, 64, 65, 257])
@pytest.mark.parametrize("W,D", [(5, 33), (20, 67), (3, 17)])
def test_panels_hold_what_they_claim(A, W, D):
    assert (TC.F * A) % 256 != 0
    X, none = TC.panel(D, A, W, False)
    Xr, p = TC.panel(D, A, W, True)
    assert none is None and X.shape == Xr.shape == (TC.F, D, A) and p.shape == (D, A)
    c = TC.COLS
    assert not np.array_equal(X[0], X[1], equal_nan=True)                       # per-factor draws
    assert (np.round(X, 1) == X).mean() > 0.2 and 0.02 < np.isnan(X[:, :, 28:]).mean() < 0.09
    for f in range(TC.F):
        run = np.isnan(X[f, :, c["nanrun"]])
        longest = max(len(s) for s in "".join("n" if v else " " for v in run).split())
        assert longest >= min(W + 1, D - D // 3 - f)
        assert (X[f, 2:2 + W + 2, c["const"]] == 0.3).all()
        z = X[f, :, c["zeros"]]
        assert np.signbit(z[z == 0]).any() and (~np.signbit(z[z == 0])).any()
        assert np.isnan(X[f, :, c["allnan"]]).all() and np.isfinite(X[f, :, c["onevalid"]]).sum() == 1
        assert np.nanmax(np.abs(X[f, :, c["big"]])) > 1e149 and 0 < np.nanmax(np.abs(X[f, :, c["tiny"]])) < 1e-199
        assert np.isfinite(X[f, :, c["control"]]).all()
        for name, rr in TC.inf_rows(D, W).items():
            col = X[f, :, c[name]]
            assert sorted(np.nonzero(np.isinf(col))[0]) == sorted(r for r in rr if r < D), name
        assert np.isposinf(X[f, D // 2, c["pinf"]]) == (f % 2 == 0) and np.isinf(X[f, 0, c["first"]])
        pair = X[f, D // 2:D // 2 + 2, c["pair"]]
        assert np.isinf(pair).all() and pair[0] == -pair[1]
        far = TC.inf_rows(D, W)["far"]
        assert far[1] - far[0] > W and np.isnan(X[f, D // 2, c["nan_inf"]]) and np.isinf(X[f, D // 2 + 1, c["nan_inf"]])
    # the ragged variant
    for name, (lo, n) in TC.GAPS.items():
        gone = ~p[:, c[name]]
        assert gone[lo:lo + n].all() and gone.sum() == len(gone[lo:lo + n]), name
    assert not p[0, c["first_absent"]] and p[1:, c["first_absent"]].all()
    assert p[:, c["short"]].sum() == min(W - 1, len(range(D // 4, D, 2))) and not p[:, c["never"]].any()
    for name, rr in TC.inf_rows(D, W).items():
        for r in rr:
            assert p[r, c[name]]
            for n in (r - 1, r + 1):
                if 0 <= n < D and n not in rr and n != D // 2:
                    assert not p[n, c[name]], (name, r, n)
    hidden = Xr[:, ~p]
    assert np.isposinf(hidden).any() and (hidden == TC.POISON).any()
    assert (np.isposinf(hidden) | (hidden == TC.POISON)).all()
    assert np.array_equal(TC.panel(D, A, W, True, TC.F, False)[1], p)
    assert np.nanmax(np.abs(np.where(np.isinf(X), 0, TC.panel(D, A, W, False, TC.F, False)[0]))) < 1e3


def test_single_asset_panel():
    X, _ = TC.panel(33, 1, 5, False)
    Xr, p = TC.panel(33, 1, 5, True)
    assert X.shape == (3, 33, 1) and np.isposinf(X[1, 16, 0]) and 0 < p.sum() < 33


def _has_full_window(W, D):
    return 1 <= abs(W) <= D or W == 0


@pytest.mark.parametrize("arm", list(TC.TS_ARMS))
def test_every_ts_case_has_finite_reference(arm):
    for ops, W, D, A, ragged in TC.TS_ARMS[arm]():
        for op in ops:
            ref = TC.ts_reference(op, W, D, A, ragged)
            assert ref.shape == (TC.F, D, A)
            if op in ("std", "var", "zscore") and W == 1:          # one observation, ddof 1
                assert np.isnan(ref).all()
            elif op in TC.SHIFTS and abs(W) >= D:
                assert np.isnan(ref).all()
            elif op == "backfill" or op == "decay" and W < 1 or _has_full_window(W, D) and (A > 1 or not ragged):
                assert np.isfinite(ref).any(), (arm, op, W, D, A, ragged)
            elif not _has_full_window(W, D):
                assert np.isnan(ref).all(), (arm, op, W, D, A, ragged)
            if ragged:
                _, p = TC.panel(D, A, W, True)
                assert np.isnan(ref[:, ~p]).all() and not (ref == TC.POISON).any()


def test_set_corr_feature_regression_references_are_finite():
    for arm, W, WR, D, A, ragged in TC.set_cases():
        if D >= W:
            for op, w in (("mean", W), ("std", W), ("zscore", W), ("rank", WR), ("decay", W)):
                assert np.isfinite(TC.ts_reference(op, w, D, A, ragged)).any() or (A == 1 and ragged)
    for arm, nf, W, D, A, ragged, pf in TC.corr_cases():
        ref = TC.corr_reference(nf, W, D, A, ragged, pf)
        assert ref.shape == (nf, D, A)
        assert np.isfinite(ref).any() if W <= D and A > 1 else W <= D or np.isnan(ref).all(), (arm, nf, W, D, A)
    for arm, nf, W, D, A in TC.feature_cases():
        assert np.isfinite(TC.feature_reference(nf, W, D, A)).any() == (W <= D), (arm, W)
    for W in (TC.TSC_MAXW, TC.TSC_MAXW + 1):
        X, Y, corr, feat = TC.long_case(W)
        assert np.isposinf(X[0][TC.LONG_X_INF]) and np.isnan(X[0][TC.LONG_X_NAN])
        assert np.isneginf(Y[TC.LONG_Y_INF]) and np.isnan(Y[TC.LONG_Y_NAN])
        assert np.isfinite(np.delete(X[0].ravel(), [3, 9])).all() and np.isfinite(np.delete(Y.ravel(), [1, 7])).all()
        assert np.isnan(corr[0, :W - 1]).all()
        for a, k in TC.LONG_CLEAR.items():
            # NaN while a non-finite pair is in the window, finite once it has left
            assert W - 1 + k + 4 <= TC.LONG_D
            assert np.isnan(corr[0, W - 1:W - 1 + k, a]).all() and np.isfinite(corr[0, W - 1 + k:, a]).all(), (W, a)
            assert np.isfinite(feat[0, W - 1 + k:, a]).all(), (W, a)
        assert np.isnan(feat[0, W - 1:W - 1 + 4, 0]).all() and np.isnan(feat[0, W - 1:W - 1 + 3, 1]).all()
        # the oracle's old rule never recovers from the inf: the cases cannot pass vacuously
        lc, lf = TC.long_case_legacy(W)
        assert np.isnan(lc[0, W - 1:, :2]).all() and np.isnan(lf[0, W - 1:, :2]).all()
        assert np.array_equal(lc[0, :, 2], corr[0, :, 2], equal_nan=True)
    y, x, valid, di, si, yv, xv = TC.regression_inputs()
    assert np.isinf(xv).any() and np.isinf(yv).any() and (xv == 1e200).any() and valid.sum() < len(xv)
    cases = TC.regression_cases()
    assert {w for w, _ in cases} == {1, 2, 5, 40, TC.REG_ENGINE_SHAPE[0] + 1}
    assert {rt for w, rt in cases if w == 5} == {0, 1, 2, 3, 6}
    for w, rt in cases:
        ref = TC.regression_reference(w, rt)
        assert np.isfinite(ref).any() == (1 < w <= TC.REG_ENGINE_SHAPE[0]), (w, rt)   # one row: 0 / 0
        assert np.isnan(ref[valid == 0]).all()


def test_inf_cases_cannot_pass_vacuously():
    """With the oracle's pre-change rule (+-inf enters the machines) every aggregation differs in
    the inf-bearing columns and nowhere else; the shift operators do not differ at all."""
    c = TC.COLS
    infc = sorted(c[n] for n in TC.INF_COLS)
    for ragged in (False, True):
        D, A, W = 46, 65, 5
        X, p = TC.panel(D, A, W, ragged)
        new = {op: TC.ts_reference(op, W, D, A, ragged) for op in TC.MOMENTS + TC.WINDOWED + TC.SHIFTS}
        with TC.legacy_rule():
            old = {op: np.stack([TC.oracle_ts(op, X[f], W, p) for f in range(TC.F)]) for op in new}
        for op in TC.MOMENTS + TC.WINDOWED:
            diff = ~((new[op] == old[op]) | (np.isnan(new[op]) & np.isnan(old[op])))
            cols = sorted(set(np.nonzero(diff)[2]))
            # (an inf in the last row makes std / var / zscore NaN under either rule)
            assert set(infc) - {c["last"]} <= set(cols) <= set(infc), (op, ragged, cols)
        for op in TC.SHIFTS:
            assert np.array_equal(new[op], old[op], equal_nan=True)
    Xc, Y, _ = TC.corr_inputs(3, 5, 41, 65, False, False)
    new = TC.corr_reference(3, 5, 41, 65, False, False)
    with TC.legacy_rule():
        import oracle.ops as O
        with np.errstate(all="ignore"):
            old = np.stack([O.ts_corr(Xc[f], Y, 5) for f in range(3)])
    diff = ~((new == old) | (np.isnan(new) & np.isnan(old)))
    assert set(infc) - {c["last"]} <= set(np.nonzero(diff)[2])
    for rt in (0, 2, 6):
        new = TC.regression_reference(5, rt)
        with TC.legacy_rule():
            TC.regression_reference.cache_clear()
            old = np.array(TC.regression_reference(5, rt))
        TC.regression_reference.cache_clear()
        assert np.isfinite(new).sum() > np.isfinite(old).sum()
