"""Host-side checks of the factor risk model's test oracles (risk_model_cases.py) and of its
C / Python surface: no GPU.  The generators, the dense Sigma, the KKT certificate and the tight
SLSQP must agree with each other before any kernel is involved, and the fill / floor /
valid-date rules are pinned on a hand-made panel."""
import os

import numpy as np
import pandas as pd
import pytest

import risk_model_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("A,K,variant", [(9, 2, None), (40, 8, None), (12, 4, "fc0"), (40, 8, "dup"), (40, 8, "spread"),
                                         (3, 5, None)])
def test_sigma_is_symmetric_psd(A, K, variant):
    B, Fc, S2 = RC.model_arrays(3, A, K, 5 * A + K, variant=variant)
    for d in range(3):
        S = RC.sigma(B[:, d], Fc[d], S2[d])
        assert np.array_equal(S, S.T)
        lam = np.linalg.eigvalsh(S)
        assert lam.min() >= S2[d].min() * (1 - 1e-9)        # diag(s2) + a PSD matrix
        w = np.random.default_rng(d).standard_normal(A)
        assert np.allclose(RC.sigma_times(B[:, d], Fc[d], S2[d], w), S @ w, rtol=1e-12, atol=1e-18)
    if variant == "dup":
        assert np.linalg.matrix_rank(Fc[0]) == K - 1
    if variant == "fc0":
        assert np.array_equal(RC.sigma(B[:, 0], Fc[0], S2[0]), np.diag(S2[0]))


def test_only_the_lower_triangle_of_fc_counts_and_nan_exposures_are_zero():
    B, Fc, S2 = RC.model_arrays(1, 9, 3, 4, nan_frac=0.2)
    assert np.isnan(B).any()
    junk = Fc[0] + np.triu(np.full((3, 3), 7.0), 1)
    assert np.array_equal(RC.sigma(B[:, 0], junk, S2[0]), RC.sigma(B[:, 0], Fc[0], S2[0]))
    assert np.array_equal(RC.sigma(B[:, 0], Fc[0], S2[0]), RC.sigma(np.nan_to_num(B[:, 0]), Fc[0], S2[0]))
    pres = np.r_[np.ones(7), 0, 0].astype(np.uint8)
    assert RC.sigma(B[:, 0], Fc[0], S2[0], pres).shape == (7, 7)


@pytest.mark.parametrize("case", [c for c in RC.MVO_CASES if c[0] <= 40], ids=str)
def test_slsqp_passes_the_kkt_certificate(case):
    A, K, u, variant = case
    B, Fc, S2, X, P, mrow = RC.mvo_case(A, K, u, variant)
    for j in range(2):
        r, pr = mrow[j], P[j] != 0
        sg = RC.signs(X[j], P[j])[pr]
        assert u * (sg > 0).sum() >= 1 and u * (sg < 0).sum() >= 1, "the case must be a feasible QP day"
        S = RC.sigma(B[:, r], Fc[r], S2[r], P[j])
        w = RC.tight_slsqp(S, sg, u)
        # the GPU tests trust SLSQP's weights to 1e-6: cells within 1e-9 of a box end are at it, and
        # weights of order u >= 0.1 known to 1e-6 give the gradient 2 Sigma w to 1e-5 of its size
        for end in (0.0, u, -u):
            w[np.abs(w - end) < 1e-9] = end
        viol, scale = RC.kkt_violation(2.0 * S @ w, w, sg, u)
        print(f"{case} date {j}: KKT violation {viol:.3e}, scale {scale:.3e}")
        assert abs(w[sg > 0].sum() - 1) <= 1e-9 and abs(w[sg < 0].sum() + 1) <= 1e-9
        assert viol <= 1e-5 * scale, (viol, scale)


def test_risk_terms_add_up():
    B, Fc, S2, W, present, valid = RC.risk_case(65, 8)
    for m in range(3):
        t = RC.risk_terms(B[:, 0], Fc[0], S2[0], W[m, 0], present[0])
        pr = present[0] != 0
        w = np.where(np.isnan(W[m, 0]), 0.0, W[m, 0])[pr]
        S = RC.sigma(B[:, 0], Fc[0], S2[0], present[0])
        assert np.isclose(t["var"][0][0], w @ S @ w, rtol=1e-10, atol=1e-30)
        assert np.isclose(t["contrib"][0].sum(), t["var"][0][1], rtol=1e-12, atol=1e-30)
        assert np.allclose(t["marginal"][0][pr], S @ w, rtol=1e-9, atol=1e-18)
        assert np.isnan(t["marginal"][0][~pr]).all()
        for v, s in t.values():
            assert (np.abs(np.nan_to_num(v)) <= s * (1 + 1e-12) + 1e-300).all()


def test_fill_floor_and_valid_dates_on_a_hand_made_panel():
    """6 dates x 5 symbols, min_periods 2, halflives 2.  f has one NaN on date 2 (the whole row
    then counts as NaN).  Symbol S4 is absent on the dates 1-2; S3's residuals are all NaN (its
    s2 is always the fill); S2's are tiny (the floor)."""
    dates = pd.bdate_range("2022-01-03", periods=6)
    syms = [f"S{i}" for i in range(5)]
    idx = pd.MultiIndex.from_product([dates, syms], names=["date", "symbol"])
    drop = [(dates[1], "S4"), (dates[2], "S4")]
    idx = idx.drop(drop)
    rng = np.random.default_rng(1)
    e = pd.Series(0.01 * rng.standard_normal(len(idx)), index=idx)
    e[e.index.get_level_values(1) == "S3"] = np.nan
    e[e.index.get_level_values(1) == "S2"] *= 1e-3
    f = pd.DataFrame(0.01 * rng.standard_normal((6, 2)), index=pd.Index(dates, name="date"), columns=["a", "b"])
    f.iloc[2, 1] = np.nan
    cov, s2, valid = RC.fit_oracle(f, e, 2, 2, 2, spec_floor=1e-6)
    # valid dates: F at t uses rows < t with the NaN row skipped -> two observations from date 2 on
    # (rows 0, 1); s2 at t uses residual rows < t -> two from date 2 on
    assert list(valid) == [False, False, True, True, True, True]
    assert np.isnan(cov.loc[dates[1]].to_numpy()).all() and not np.isnan(cov.loc[dates[2]].to_numpy()).any()
    # row 2 of f counts as NaN in BOTH columns: var(a) on date 3 is not what column a alone gives
    alone = f.shift(1).ewm(halflife=2, min_periods=2).cov()
    f_row = f.copy()
    f_row.iloc[2] = np.nan
    whole = f_row.shift(1).ewm(halflife=2, min_periods=2).cov()
    assert cov.loc[dates[3]].loc["a", "a"] == whole.loc[dates[3]].loc["a", "a"] != alone.loc[dates[3]].loc["a", "a"]
    lam = np.linalg.eigvalsh(cov.loc[dates[5]].to_numpy())
    assert lam.min() >= -1e-12 * lam.max()
    d3 =s2.xs(dates[3], level=0)
    raw = (e.groupby(level="symbol").shift(1).groupby(level="symbol").ewm(halflife=2, min_periods=2).var()
           .droplevel(0).reindex(e.index).xs(dates[3], level=0))
    fin = np.sort(raw.dropna().to_numpy())
    assert len(fin) == 3                                    # S0, S1, S2: S3 is NaN, S4 has one lagged row
    lower_median = fin[(len(fin) - 1) // 2]
    assert d3["S3"] == max(lower_median, 1e-6) and d3["S4"] == max(lower_median, 1e-6)
    assert d3["S2"] == 1e-6 and raw["S2"] < 1e-6            # the floor
    assert d3["S0"] == max(raw["S0"], 1e-6)
    # an even count takes the LOWER middle value
    filled = RC.lower_median_fill(np.array([[4.0, np.nan, 1.0, 3.0, 2.0, np.nan]]), np.array([[1, 1, 1, 1, 1, 0]]))
    assert filled[0, 1] == 2.0 and np.isnan(filled[0, 5])
    # before any finite s2 exists the date is invalid and nothing is filled
    assert s2.xs(dates[0], level=0).isna().all() and not valid.iloc[0]


def test_header_and_signatures_agree():
    import factormodeling_amd._lib as L
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    for name, nargs in (("fmx_risk_books", 15), ("fmx_risk_mvo_books", 17), ("fmx_risk_mvo_books_work_bytes", 3)):
        assert name + "(" in header and len(L.SIGNATURES[name]) == nargs
        decl = header[header.index(name + "("):]
        decl = decl[:decl.index(";")]
        assert decl.count(",") + 1 == nargs
    assert L._RESTYPES["fmx_risk_mvo_books_work_bytes"] is L.c_i64


def test_settings_field_is_last_and_defaults_to_none():
    from dataclasses import fields
    from factormodeling_amd.portfolio_simulation import SimulationSettings
    assert fields(SimulationSettings)[-1].name == "risk_model" and fields(SimulationSettings)[-1].default is None
