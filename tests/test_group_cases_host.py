"""The panels of tests/group_cases.py are what they claim to be (no GPU): the constructed
group sizes, the empty / all-NaN / one-valid / constant groups, the out-of-range cells, and
the oracle outputs the GPU comparison (tests/test_gpu_group_paths.py) is held to -- so that
comparison cannot pass on a degenerate panel.

Waived on short rows (``facts["waived"]``): A < 26 has no room for date 2's 26 special cells
("date2": the row is singletons only); A < 24 has no second block of out-of-range codes
("oor_tail", and A < 12 takes the first A codes of the list); a ragged row with fewer than
200 absent cells that have a group gives code 3 all of them ("extra_absent", A < 1000).  From
A = 1000 on nothing is waived."""
import numpy as np
import pytest

import group_cases as GC

CASES = [(A, r, None) for A in GC.LENGTHS for r in (False, True)] + \
        [(A, r, m) for A, m in GC.BIG_VARIANTS for r in (False, True)]


def _count(c, d, code, present_only=True):
    sel = c["codes"][d] == code
    if present_only and c["present"] is not None:
        sel &= c["present"][d]
    return int(sel.sum())


def test_lengths_cover_every_emax_bucket_at_both_ends():
    ends = {}
    for A in GC.LENGTHS:
        if GC.K_GROUP_MAX_A < A <= GC.LONG_MAX_A:
            ends.setdefault(GC.emax_bucket(A), []).append(A)
    assert ends == {5: [4097, 5120], 8: [5121, 8192], 12: [8193, 12288], 16: [12289, 16384]}
    for e, (lo, hi) in ends.items():
        assert -(-lo // 1024) == {5: 5, 8: 6, 12: 9, 16: 13}[e] and -(-hi // 1024) == e
    # and both neighbours of the range: k_group below it, the HBM paths above it
    assert 4096 in GC.LENGTHS and 16385 in GC.LENGTHS


@pytest.mark.parametrize("A,ragged,members", CASES)
def test_case_is_what_it_claims(A, ragged, members):
    c, ref = GC.case_and_reference(A, ragged, members)
    x, g, codes, p, facts = c["x"], c["g"], c["codes"], c["present"], c["facts"]
    pres = np.ones((GC.D, A), bool) if p is None else p
    waived = facts["waived"]
    if A >= 1000:
        assert not waived
    assert x.shape == (GC.F, GC.D, A) and g.shape == codes.shape == (GC.D, A) and codes.dtype == np.int32
    assert c["ngroups"] == GC.NG == 61
    assert (p is None) == (not ragged)
    if ragged and A >= 63:
        assert all(0 < (~pres[d]).sum() for d in (0, 1, 4))          # the mask bites
    # g is the codes with NaN for "no group", exactly on the negative and out-of-range cells
    in_range = (codes >= 0) & (codes < GC.NG)
    assert np.array_equal(np.isnan(g), ~in_range)
    assert np.array_equal(g[in_range], codes[in_range].astype(np.float64))
    assert not np.array_equal(x[0], x[1], equal_nan=True)            # factor 1 is its own draw
    if A >= 63:
        for d in (0, 2, 4):
            assert not np.array_equal(codes[d], codes[1])             # G differs between dates

    # date 0: codes in [0, 11) or none
    assert set(np.unique(codes[0])) <= set(range(-1, 11))

    # date 1: the big group's exact sizes
    want = min(facts["big_cells_with_group"], GC.SORT_MAX) if members is None else members
    assert facts["big_present"] == want == _count(c, 1, GC.BIG)
    raw = _count(c, 1, GC.BIG, present_only=False)
    assert raw == facts["big_raw"]
    if ragged and "extra_absent" not in waived:
        assert raw == want + GC.EXTRA_ABSENT
    if not ragged:
        assert raw == want
    if A > GC.SORT_MAX + 200:
        assert want == (members or GC.SORT_MAX)
        assert raw > GC.SORT_MAX if ragged else raw == want
    assert set(np.unique(codes[1])) <= {-1} | set(range(3, 11))

    # date 2: the special groups
    sizes = np.bincount(codes[2][(codes[2] >= 0) & pres[2]], minlength=GC.NG)
    assert len(sizes) == GC.NG and sizes[59] == 0 and sizes[60] == 0 and sizes[GC.EMPTY] == 0
    if "date2" not in waived:
        assert (sizes == 1).sum() >= 5 and all(sizes[s] == 1 for s in GC.SINGLETONS)
        assert sizes[GC.ALLNAN] == GC.N_ALLNAN and sizes[GC.ONEVALID] == GC.N_ONEVALID >= 3
        assert sizes[GC.CONST] == GC.N_CONST
        for f in range(GC.F):
            assert np.isnan(x[f, 2, codes[2] == GC.ALLNAN]).all()
            assert (~np.isnan(x[f, 2, codes[2] == GC.ONEVALID])).sum() == 1
            assert (x[f, 2, codes[2] == GC.CONST] == GC.CONST_VALUE).all()
            assert np.isnan(x[f, 2, codes[2] == GC.SINGLETONS[-1]]).all()
        assert {0, A - 1} <= set(facts["special_cells"])
    else:
        assert (sizes == 1).sum() == A

    # date 3: the out-of-range cells
    oor = facts["oor"]
    assert not oor[[0, 1, 2, 4]].any()
    n_head = min(12, A)
    assert oor[3, :n_head].all() and pres[3, :n_head].all()
    assert list(codes[3, :n_head]) == list(GC.OOR_CODES[:n_head])
    if "oor_tail" not in waived:
        assert list(codes[3, -12:]) == list(GC.OOR_CODES) and oor[3].sum() == 24
    assert not in_range[oor].any() and in_range[3][~oor[3]].sum() == (codes[3][~oor[3]] >= 0).sum()

    # date 4: degenerate values
    assert np.isnan(x[0, 4]).all() and (x[1, 4] == 1.5).all()
    assert np.array_equal(codes[4], codes[0])

    # the oracle outputs
    assert set(ref) == set(GC.MOMENTS) | {("rank", m) for m in GC.METHODS}
    for key, r in ref.items():
        assert r.shape == x.shape
        assert np.isnan(r[:, ~in_range]).all(), key                   # no group (out of range incl.)
        assert np.isnan(r[:, ~pres]).all(), key                       # absent
        if A >= 1000:
            assert np.isnan(r[:, oor]).all() and oor.sum() == 24
            for d in range(GC.D):
                assert max(np.isfinite(r[f, d]).sum() for f in range(GC.F)) > 0, (key, d)
    if "date2" not in waived:
        for f in range(GC.F):
            assert (ref["normalize"][f, 2, codes[2] == GC.CONST] == 0.0).all()
            assert (ref["normalize"][f, 2, codes[2] == GC.ALLNAN] == 0.0).all()
            assert np.isnan(ref["mean"][f, 2, codes[2] == GC.ALLNAN]).all()
            for m in GC.METHODS:
                assert (ref["rank", m][f, 2, codes[2] == GC.ONEVALID] == 0.5).all()
                assert (ref["rank", m][f, 2, codes[2] == GC.SINGLETONS[-1]] == 0.5).all()


@pytest.mark.parametrize("A,ragged,members", [(A, r, m) for A, m in GC.BIG_VARIANTS for r in (False, True)])
def test_big_group_variants_sit_on_the_sort_switch(A, ragged, members):
    c = GC.make_case(A, ragged, members=members)
    want = "fmx_group_rank_sorted" if members > GC.SORT_MAX else f"k_group_long<{GC.emax_bucket(A)}>"
    assert GC.expected_path("rank", A, c["codes"], GC.NG, c["present"]) == want
    # the big group decides it: every other (date, group) is far below the switch
    pres = np.ones((GC.D, A), bool) if c["present"] is None else c["present"]
    for d in range(GC.D):
        sel = (c["codes"][d] >= 0) & (c["codes"][d] < GC.NG) & pres[d]
        sizes = np.bincount(c["codes"][d][sel], minlength=GC.NG)
        if d == 1:
            assert sizes[GC.BIG] == members
            sizes[GC.BIG] = 0
        assert sizes.max() < GC.SORT_MAX // 2


def test_expected_path_over_lengths():
    for A in GC.LENGTHS:
        for ragged in (False, True):
            c = GC.make_case(A, ragged)
            long = "k_group" if A <= 4096 else f"k_group_long<{GC.emax_bucket(A)}>" if A <= 16384 else None
            assert GC.expected_path("mean", A, c["codes"], GC.NG, c["present"]) == (long or "k_group_xl")
            assert GC.expected_path("mean", A, c["codes"], GC.NG, c["present"], True) == "k_group_xl"
            assert GC.expected_path("rank", A, c["codes"], GC.NG, c["present"]) == (long or "fmx_group_rank_sorted")
