"""Shared by the group-operator tests (host and GPU): one seeded case builder whose panels
reach every kernel path of ``engine.group_op`` (DESIGN "Group operators: dispatch and code
contract") and the oracle outputs of a case, computed once per process.  No GPU needed.

A case is ``x [F=2][D=5][A]`` float64, ``g [D][A]`` float64 (NaN = no group: what the oracle
reads), ``codes [D][A]`` int32 (what the kernels read), ``ngroups`` = 61, ``present [D][A]``
bool or None, and ``facts``: what the construction guarantees, asserted by
tests/test_group_cases_host.py.  The five dates (positions are asset indices before the mask):

0  ordinary: codes uniform in [0, 11), 1 % of cells without a group.
1  one big group: code 3 on every cell that has a group, trimmed so that its present
   members number exactly ``min(cells present with a group, 8192)`` (or ``members`` when
   given); the other cells go to codes 4..10.  Ragged: another 200 absent cells carry code
   3, so the raw count of the code exceeds the present one.
2  many groups: codes in [0, 59) with >= 5 singleton groups (one of them a lone NaN), code 17
   without a member, code 23 all NaN, code 29 with one non-NaN value among 4 members, code 31
   constant 0.25; codes 59 and 60 unused, so the last groups are empty.
3  date 0's codes with OOR_CODES written over the first 12 cells and, where A >= 24, the last
   12: codes outside [0, ngroups), NaN in ``g``.  The first 12 are present in every variant.
4  degenerate: factor 0 all NaN, factor 1 all one value; date 0's codes.

Values: standard normal, 20 % rounded to one decimal (ties), 3 % NaN; factor 1 is an
independent draw.  Ragged variants drop 10 % of the cells of every date (date 1: at least
min(250, A // 4), so that the 200 absent cells of code 3 exist from A = 1000 on).
"""
from __future__ import annotations

import functools

import numpy as np

F, D, NG = 2, 5, 61
BIG, SORT_MAX = 3, 8192           # date 1's group; the per-group LDS sort takes <= 8192 members
EMPTY, ALLNAN, ONEVALID, CONST = 17, 23, 29, 31
CONST_VALUE = 0.25
SINGLETONS = (50, 51, 52, 53, 54, 55)             # 55: its one member is NaN in both factors
N_ALLNAN, N_ONEVALID, N_CONST = 7, 4, 9
N_SPECIAL = len(SINGLETONS) + N_ALLNAN + N_ONEVALID + N_CONST      # 26 cells of date 2
OOR_CODES = (61, 66, 65534, 65535, 65536, 65536 + 3, 65536 + 60, 2 ** 31 - 1, -7, -2 ** 31, 61, 65536)
EXTRA_ABSENT = 200

LENGTHS = [1, 2, 63, 64, 65, 1000, 4096, 4097, 5120, 5121, 8192, 8193, 12288, 12289, 16384, 16385]
# (A, members of date 1's group among the present cells): last size on the LDS sort, first on
# the HBM sort
BIG_VARIANTS = [(A, m) for A in (10000, 16384) for m in (SORT_MAX, SORT_MAX + 1)]
MOMENTS = ("mean", "neutralize", "normalize")
METHODS = ("average", "min", "max", "first", "dense")

K_GROUP_MAX_A = 4096              # k_group sorts the whole row in LDS
LONG_MAX_A = 16384                # k_group_long holds the row in registers


def emax_bucket(A):
    """The EMAX of the k_group_long instantiation fmx_group_op launches for a row of A cells
    (4096 < A <= 16384): ceil(A / 1024) rounded up to 5, 8, 12 or 16."""
    assert K_GROUP_MAX_A < A <= LONG_MAX_A
    e = -(-A // 1024)
    return 5 if e <= 5 else 8 if e <= 8 else 12 if e <= 12 else 16


def _values(rng, A):
    x = rng.standard_normal((D, A))
    x = np.where(rng.random(x.shape) < 0.2, np.round(x, 1), x)
    x[rng.random(x.shape) < 0.03] = np.nan
    return x


def make_case(A, ragged, seed=0, members=None):
    rng = np.random.default_rng([seed, A, int(ragged), members or 0])
    x = np.stack([_values(rng, A) for _ in range(F)])
    present = None
    if ragged:
        present = rng.random((D, A)) >= 0.1
        n_abs = max(int(round(0.1 * A)), min(250, A // 4))
        present[1] = True
        present[1, rng.choice(A, n_abs, replace=False)] = False
    pres = np.ones((D, A), bool) if present is None else present
    g = np.full((D, A), np.nan)
    facts = {"waived": set()}

    # date 0 (and the pattern of dates 3 and 4)
    g[0] = rng.integers(0, 11, size=A)
    g[0, rng.random(A) < 0.01] = np.nan

    # date 1: one big group
    has = rng.random(A) >= 0.01
    cand = np.nonzero(has & pres[1])[0]
    target = min(len(cand), SORT_MAX) if members is None else members
    assert target <= len(cand), "the row is too short for the requested group"
    keep = np.sort(rng.choice(cand, target, replace=False))
    rest = np.setdiff1d(np.nonzero(has)[0], keep)
    g[1, keep] = BIG
    g[1, rest] = rng.integers(4, 11, size=len(rest))
    absent = np.nonzero(has & ~pres[1])[0]
    extra = min(EXTRA_ABSENT, len(absent))
    g[1, absent[:extra]] = BIG
    if ragged and extra < EXTRA_ABSENT:
        facts["waived"].add("extra_absent")
    facts.update(big_present=target, big_raw=target + extra, big_cells_with_group=len(cand))

    # date 2: many groups
    ordinary = np.setdiff1d(np.arange(59), (EMPTY, ALLNAN, ONEVALID, CONST) + SINGLETONS)
    g[2] = rng.choice(ordinary, size=A)
    g[2, rng.random(A) < 0.01] = np.nan
    if A >= N_SPECIAL:
        # the special cells: both ends of the row and random positions between them
        pos = np.concatenate(([0, A - 1], 1 + rng.choice(A - 2, N_SPECIAL - 2, replace=False)))
        pos = rng.permutation(pos)
        o = 0
        for c in SINGLETONS:
            g[2, pos[o]] = c
            o += 1
        x[:, 2, pos[o - 1]] = np.nan                                  # code 55: a lone NaN
        x[:, 2, pos[:o - 1]] = rng.standard_normal((F, o - 1))
        g[2, pos[o:o + N_ALLNAN]] = ALLNAN
        x[:, 2, pos[o:o + N_ALLNAN]] = np.nan
        o += N_ALLNAN
        g[2, pos[o:o + N_ONEVALID]] = ONEVALID
        x[:, 2, pos[o:o + N_ONEVALID]] = np.nan
        x[:, 2, pos[o + 1]] = (0.75, -1.5)
        o += N_ONEVALID
        g[2, pos[o:o + N_CONST]] = CONST
        x[:, 2, pos[o:o + N_CONST]] = CONST_VALUE
        pres[2, pos] = True
        facts["special_cells"] = np.sort(pos)
    else:
        # rows too short for the construction: singletons as far as they fit
        g[2] = SINGLETONS[:A]
        x[:, 2] = rng.standard_normal((F, A))
        pres[2] = True
        facts["waived"].add("date2")

    # date 3: out-of-range codes
    g[3] = g[0]
    codes3 = np.where(np.isnan(g[3]), -1, g[3]).astype(np.int64)
    n_head = min(len(OOR_CODES), A)
    oor = np.zeros((D, A), bool)
    codes3[:n_head] = OOR_CODES[:n_head]
    oor[3, :n_head] = True
    pres[3, :n_head] = True
    if A >= 2 * len(OOR_CODES):
        codes3[-len(OOR_CODES):] = OOR_CODES
        oor[3, -len(OOR_CODES):] = True
    else:
        facts["waived"].add("oor_tail")
    g[3, oor[3]] = np.nan

    # date 4: degenerate values
    g[4] = g[0]
    x[0, 4] = np.nan
    x[1, 4] = 1.5

    codes = np.where(np.isnan(g), -1, g).astype(np.int64)
    codes[3] = codes3
    codes = codes.astype(np.int32)
    assert np.array_equal(codes[3].astype(np.int64), codes3)          # every code fits int32
    facts["oor"] = oor
    if present is not None:
        present = pres
    return dict(A=A, ragged=bool(ragged), x=x, g=g, codes=codes, ngroups=NG, present=present, facts=facts)


@functools.lru_cache(maxsize=None)
def case_and_reference(A, ragged, members=None):
    """(case, ref): ``ref[op]`` for the three moments and ``ref["rank", method]`` for the five
    rank methods, each ``[F][D][A]`` from oracle.ops.  Computed once per process and shared:
    callers must not modify the arrays."""
    import oracle.ops as O
    c = make_case(A, ragged, members=members)
    x, g, p = c["x"], c["g"], c["present"]
    ref = {}
    with np.errstate(all="ignore"):
        for op in MOMENTS:
            fn = getattr(O, "group_" + op)
            ref[op] = np.stack([fn(x[f], g, p) for f in range(F)])
        for m in METHODS:
            ref["rank", m] = np.stack([O.group_rank_normalized(x[f], g, p, method=m) for f in range(F)])
    for a in (x, g, c["codes"]) + tuple(ref.values()):
        a.setflags(write=False)
    return c, ref


def expected_path(op, A, codes, ngroups, present, long_rows=None):
    """The kernel ``engine.group_op`` runs for this call, decided the way it decides:
    'k_group', 'k_group_long<EMAX>', 'k_group_xl' or 'fmx_group_rank_sorted'."""
    if op == "rank":
        if A > LONG_MAX_A:
            return "fmx_group_rank_sorted"
        if A > K_GROUP_MAX_A and ngroups > 0:
            ok = (codes >= 0) & (codes < ngroups)
            if present is not None:
                ok &= present
            largest = max((int(np.bincount(codes[d][ok[d]], minlength=1).max()) for d in range(codes.shape[0])),
                          default=0)
            if largest > SORT_MAX:
                return "fmx_group_rank_sorted"
    elif long_rows or (long_rows is None and A > LONG_MAX_A):
        return "k_group_xl"
    return "k_group" if A <= K_GROUP_MAX_A else f"k_group_long<{emax_bucket(A)}>"
