"""fmx_gram_exact_rows: the exact Gram of a device row list is, entry for entry, the bits
fmx_gram_exact gives the same factor pair -- limbs and counts, at any date range and any
split of the dates (torch.equal: integer outputs, no tolerance).

Panels: cs_zscore outputs, F = 40, D = 9, with 1 % NaN, one all-NaN factor and one
(factor, date) row of +-inf.  Assets: 31 (one partial 32-asset chunk), 96, 2561 (two units per
date, split 40 / 41 chunks) and 5000.  Row lists (shuffled, unsorted): H = 16 and 32 (one and
three MFMA blocks), one with a repeated index, one with indices outside [0, F), and H = 48 /
64 (the kernel's other two instantiations; more rows than factors, so with repeats)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F, D = 40, 9
NAN_FACTOR, INF_ROW = 7, (11, 4)


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


_FULL = {}


def _panel(dev, A):
    """(z, limbs, counts) of the full exact Gram over all dates, made once per A."""
    import torch
    import factormodeling_amd.engine as E
    if A not in _FULL:
        rng = np.random.default_rng(100 + A)
        X = rng.standard_normal((F, D, A))
        X[rng.random(X.shape) < 0.01] = np.nan
        X[NAN_FACTOR] = np.nan
        z = E.cs_moment("zscore", torch.as_tensor(X, device=dev))
        sign = torch.as_tensor(np.where(rng.random(A) < 0.5, -np.inf, np.inf), device=dev)
        z[INF_ROW[0], INF_ROW[1]] = sign
        L, N = E.gram_exact(z, None, 0, D)
        _FULL[A] = (z, L, N)
    return _FULL[A]


def _rows(kind):
    rng = np.random.default_rng(len(kind))
    perm = rng.permutation(F)
    if kind == "h16":
        r = perm[:16]
    elif kind == "h32":
        r = perm[:32]
    elif kind == "repeat":
        r = perm[:32].copy()
        r[20] = r[3]
        r[5] = INF_ROW[0]
        r[9] = NAN_FACTOR
    elif kind == "out_of_range":
        r = perm[:16].copy()
        r[2], r[7], r[15] = -1, F, 1 << 40
    elif kind == "h48":
        r = np.concatenate([perm, perm[:8]])
    else:
        r = rng.integers(0, F, 64)
    return np.asarray(r, dtype=np.int64)


def _expected(L, N, rows):
    """The (min, max) entries of the full limbs / counts by list position (upper triangle);
    a position whose index is outside [0, F) is an all-invalid row: zeros."""
    import torch
    r = torch.as_tensor(rows, device=L.device)
    ok = (r >= 0) & (r < F)
    rc = r.clamp(0, F - 1)
    lo, hi = torch.minimum(rc[:, None], rc[None, :]), torch.maximum(rc[:, None], rc[None, :])
    H = len(rows)
    up = torch.triu(torch.ones((H, H), dtype=torch.bool, device=L.device)) & ok[:, None] & ok[None, :]
    return L[:, lo, hi] * up, N[lo, hi] * up


@pytest.mark.parametrize("kind", ["h16", "h32", "repeat", "out_of_range", "h48", "h64"])
@pytest.mark.parametrize("A", [31, 96, 2561, 5000])
def test_gram_exact_rows_equals_full_entries(dev, A, kind):
    import torch
    import factormodeling_amd.engine as E
    z, L, N = _panel(dev, A)
    rows = _rows(kind)
    rd = torch.as_tensor(rows, device=dev)
    Lh, Nh = E.gram_exact_rows(z, rd, 0, D)
    eL, eN = _expected(L, N, rows)
    assert torch.equal(Nh, eN)
    assert torch.equal(Lh, eL)
    # a date sub-range: the same units of the same dates
    L2, N2 = E.gram_exact(z, None, 2, D)
    Lh2, Nh2 = E.gram_exact_rows(z, rd, 2, D)
    eL2, eN2 = _expected(L2, N2, rows)
    assert torch.equal(Lh2, eL2) and torch.equal(Nh2, eN2)
    # two date halves, the second accumulated into the first: the whole
    La, Na = E.gram_exact_rows(z, rd, 0, 4)
    E.gram_exact_rows(z, rd, 4, D, limbs=La, counts=Na, accumulate=True)
    assert torch.equal(La, eL) and torch.equal(Na, eN)


def test_gram_exact_rows_panel_is_not_trivial(dev):
    """The fixtures exercise what they claim: the inf row and the NaN factor are invalid in
    the full Gram, and 2561 assets are two units per date."""
    import factormodeling_amd.engine as E
    from factormodeling_amd import _lib
    z, L, N = _panel(dev, 2561)
    assert int(_lib.load().fmx_gram_exact_units_per_date(2561)) == 2
    assert int(N[NAN_FACTOR, NAN_FACTOR]) == 0
    full = int(N[0, 0])
    assert 0 < int(N[INF_ROW[0], INF_ROW[0]]) < full
    assert int(L[E.GRAM_EXACT_SLOTS - 1].abs().sum()) == 0      # no flagged term: inf rows are masked
