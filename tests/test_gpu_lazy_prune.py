"""The lazy Gram: fmx_prune_head against the spec's greedy walk over the full correlation
matrix, and run_step with StepConfig.lazy_gram on against off (no ``collect``: the lazy path
is taken only then), one shard and two LocalComm shards.

The head's limbs / counts handed to fmx_prune_head are the (min, max) entries of the full
exact Gram gathered by position -- what fmx_gram_exact_rows returns
(tests/test_gpu_gram_rows.py) -- so this file checks the walk and the step's plumbing, not
the Gram kernel again.  Everything compared is discrete (kept lists, done flags) or must be
bit-identical (the selection weights): no tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = 40


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _zoo(kind, seed, D=6, A=300):
    """independent: F unrelated factors.  grouped: groups of 1-8 factors sharing a component
    (within-group correlations from ~0.5 to ~0.98, spread around every rho tested)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((F, D, A))
    if kind == "grouped":
        f = 0
        while f < F:
            n = int(rng.integers(1, 9))
            comp = rng.standard_normal((D, A))
            for g in range(f, min(F, f + n)):
                X[g] = comp + rng.uniform(0.2, 1.0) * X[g]
            f += n
    X[rng.random(X.shape) < 0.01] = np.nan
    return X


_ZOO = {}


def _full(dev, kind, nan_row):
    """(limbs, counts, C) of the zoo's full exact Gram; C as run_step forms it.  ``nan_row``:
    the flag limb of one factor's entries is set (a non-finite term), making its row of C NaN."""
    import torch
    import factormodeling_amd.engine as E
    key = (kind, nan_row)
    if key not in _ZOO:
        z = E.cs_moment("zscore", torch.as_tensor(_zoo(kind, 3 if kind == "grouped" else 4), device=dev))
        L, N = E.gram_exact(z, None)
        if nan_row:
            L[E.GRAM_EXACT_SLOTS - 1, 17, :] = 1
            L[E.GRAM_EXACT_SLOTS - 1, :, 17] = 1
        G, Nf = E.gram_exact_finalize(L, N)
        C = torch.where(Nf > 0, G / Nf.clamp_min(1.0), torch.zeros_like(G))
        _ZOO[key] = (L, N, C.cpu().numpy())
    return _ZOO[key]


def _head(L, N, rows):
    import torch
    r = torch.as_tensor(rows, device=L.device)
    lo, hi = torch.minimum(r[:, None], r[None, :]), torch.maximum(r[:, None], r[None, :])
    up = torch.triu(torch.ones((len(rows),) * 2, dtype=torch.bool, device=L.device))
    return (L[:, lo, hi] * up).contiguous(), (N[lo, hi] * up).contiguous()


@pytest.mark.parametrize("H", [16, 32])
@pytest.mark.parametrize("kind,nan_row", [("independent", False), ("grouped", False), ("grouped", True)])
def test_prune_head_matches_oracle_walk(dev, kind, nan_row, H):
    import torch
    import factormodeling_amd.engine as E
    import oracle.gram as OG
    L, N, C = _full(dev, kind, nan_row)
    if nan_row:
        assert np.isnan(C[17]).all()
    rng = np.random.default_rng(H + len(kind))
    n_done = n_fall = 0
    for trial in range(4):
        order = rng.permutation(F).astype(np.int64)
        if trial == 3:
            order[[1, 6]] = [-1, F + 3]             # out-of-range entries are skipped
        od = torch.as_tensor(order, device=dev)
        Lh, Nh = _head(L, N, np.clip(order[:H], 0, F - 1))
        walk = [int(f) for f in order if 0 <= f < F]
        for rho in (0.3, 0.7, 0.95):
            for top in range(1, 12):
                want = OG.greedy_prune(C, walk, rho, top)
                kept, done = E.prune_head(Lh, Nh, od, F, rho, top)
                assert done == (len(kept) == top), (trial, rho, top)     # H < len(order) here
                if done:
                    assert kept == want, (trial, rho, top)
                    n_done += 1
                else:
                    assert len(kept) < top and kept == want[:len(kept)], (trial, rho, top)
                    n_fall += 1
    assert n_done > 0
    if kind == "grouped" and H == 16:
        assert n_fall > 0                           # both branches are exercised


def test_prune_head_whole_order_is_done(dev):
    """H >= n_order: the head is the whole order, so the walk is complete whatever it kept."""
    import torch
    import factormodeling_amd.engine as E
    import oracle.gram as OG
    L, N, C = _full(dev, "grouped", False)
    order = np.random.default_rng(1).permutation(F)[:16].astype(np.int64)
    Lh, Nh = _head(L, N, order)
    kept, done = E.prune_head(Lh, Nh, torch.as_tensor(order, device=dev), F, 0.3, 11)
    assert done and kept == OG.greedy_prune(C, order, 0.3, 11)


# ---- run_step: lazy_gram on against off --------------------------------------------------------

SA, SD, SW = 257, 100, 30
# F = 48 admits only a 16-row head (2 H <= F), set with FMX_GRAM_HEAD; F = 80 takes the default 32
SHAPES = {"f48_h16": (48, "16"), "f80_h32": (80, None)}


def _shape(monkeypatch, shape):
    SF, head = SHAPES[shape]
    if head is None:
        monkeypatch.delenv("FMX_GRAM_HEAD", raising=False)
    else:
        monkeypatch.setenv("FMX_GRAM_HEAD", head)
    monkeypatch.delenv("FMX_LAZY_GRAM", raising=False)
    return SF


def _step_panel(kind, dev, SF):
    """Full-size (SF, SD, SA) factors and returns on the device.  independent: the order's head
    holds unrelated factors (the prune finishes inside it).  copies: 32 factors are near-copies
    of three signals that drive the next day's returns, so they lead the rank-ICIR order and the
    head keeps three of top_x = 5: the step must fall back to the full Gram."""
    import torch
    rng = np.random.default_rng(21)
    X = rng.standard_normal((SF, SD, SA))
    R = 0.01 * rng.standard_normal((SD, SA))
    if kind == "copies":
        S = rng.standard_normal((3, SD, SA))
        for f in range(32):
            X[f + 8] = S[f % 3] + 0.05 * X[f + 8]
        R[1:] += 0.01 * S.sum(axis=0)[:-1] / np.sqrt(3.0)
    X[rng.random(X.shape) < 0.01] = np.nan
    return torch.as_tensor(X, device=dev), torch.as_tensor(R, device=dev)


def _run(dev, X, R, cfg, comm=None):
    """run_step (no collect) on the given panel: (w, kept, stage names)."""
    import torch
    from factormodeling_amd import pipeline as PL
    SF = X.shape[0]
    if comm is None:
        sp = PL.ShardedPanel(SD, SA, SF, 0, 1, dev, seed=1, halo=cfg.halo)
    else:
        sp = PL.ShardedPanel(SD, SA, SF, device=dev, seed=1, halo=cfg.halo, comm=comm)
    sp.X[:, sp.halo:] = X[:, sp.d_lo:sp.d_hi]
    sp.R[sp.halo:] = R[sp.d_lo:sp.d_hi]
    timers = []
    w, kept = PL.run_step(sp, cfg, timers=timers)
    torch.cuda.current_stream().synchronize()
    return w.cpu().numpy(), kept, [n for n, _, _ in timers]


CASES = {  # name -> (panel, top_x, lazy path taken, full Gram run when lazy)
    "head": ("independent", 5, True, False),
    "fallback": ("copies", 5, True, True),
    "wide_top": ("independent", 20, False, True),
}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("case", list(CASES))
def test_run_step_lazy_equals_full(dev, monkeypatch, case, shape):
    from factormodeling_amd import pipeline as PL
    kind, top, lazy, full = CASES[case]
    X, R = _step_panel(kind, dev, _shape(monkeypatch, shape))
    w0, kept0, st0 = _run(dev, X, R, PL.StepConfig(sel_window=SW, top_x=top, lazy_gram=False))
    w1, kept1, st1 = _run(dev, X, R, PL.StepConfig(sel_window=SW, top_x=top, lazy_gram=True))
    assert "gram_head" not in st0 and "gram" in st0
    assert ("gram_head" in st1) == lazy and ("gram" in st1) == full, st1
    assert kept1 == kept0 and len(kept0) == top
    assert np.array_equal(w1, w0, equal_nan=True)
    if case == "fallback":
        assert sum(1 for f in kept0 if 8 <= f < 40) == 3        # one factor per copied signal


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("case", ["head", "fallback"])
def test_run_step_lazy_two_shards(dev, monkeypatch, case, shape):
    from factormodeling_amd import pipeline as PL
    from factormodeling_amd.comm import run_local_shards
    kind, top, lazy, full = CASES[case]
    X, R = _step_panel(kind, dev, _shape(monkeypatch, shape))
    w0, kept0, _ = _run(dev, X, R, PL.StepConfig(sel_window=SW, top_x=top, lazy_gram=False))
    cfg = PL.StepConfig(sel_window=SW, top_x=top, lazy_gram=True)
    for w, kept, st in run_local_shards(2, lambda rank, comm: _run(dev, X, R, cfg, comm)):
        assert "gram_head" in st and ("gram" in st) == full, st
        assert kept == kept0
        assert np.array_equal(w, w0, equal_nan=True)
