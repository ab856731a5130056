"""The fused cross-sectional pass (fmx_cs_rank_winsor_zn) and the kernels instantiated from
the same template (cs_rank + cs_winsor, the ranks-only pass), bit for bit against the host
oracle (oracle.ops) -- not against the two-pass kernels, which share the code.

Panels are F = 2, D = 3 (six rows); the row kinds below are spread over three such panels.
Row lengths: the edges of the 512 x 10 instantiation (4609: last slot nearly empty, 5000 /
5119: partly full, 5120: full), 4100 (9 x 512 > A: the instantiation's slot count is rounded
up from 9, so its last slot is wholly past the row and the one before partly; also a row
length whose numpy pairwise tree is not complete over 64 leaves, the other moment variant)
and 5000 (the 64-leaf variant).  ld = A and ld = A + 3: row bases aligned to 8 bytes only."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F, D = 2, 3
QLO, QHI = 0.01, 0.99
PAD_IN, PAD_OUT, PAD_RK = 777.0, 7.0, 12345


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _generic(rng, A):
    x = rng.standard_normal(A)
    x[rng.random(A) < 0.01] = np.nan
    return x


def _few(rng, A, n):
    x = np.full(A, np.nan)
    x[rng.choice(A, n, replace=False)] = rng.standard_normal(n)
    return x


def _all_nan(rng, A):
    return np.full(A, np.nan)


def _const(rng, A):
    return np.full(A, 0.75)                    # sd = 0: zscore NaN, neutralize 0


def _tiny_spread(rng, A):
    # |x - mean| < 2^-895 around a mean 2^35 times larger: the divide guards' small side
    return 2.0 ** -860 + rng.integers(0, 32, A) * 2.0 ** -900


def _tiny(rng, A):
    return 1e-290 * rng.standard_normal(A)


def _huge(rng, A):
    x = 1e300 * rng.uniform(0.5, 1.0, A) * rng.choice([-1.0, 1.0], A)   # squares overflow
    x[rng.random(A) < 0.01] = np.nan
    return x


def _big(rng, A):
    return 1e140 * rng.standard_normal(A)      # finite moments, exponents far from 1023


def _zeros(rng, A):
    # +0.0 / -0.0 among quarter-integers in +/- pairs: every partial sum is exact, the mean is
    # exactly 0, so x - mean = 0 at the zeros
    h = A // 4
    v = rng.integers(-8, 9, h) / 4.0
    x = np.concatenate([v, -v, np.zeros(A - 2 * h - (A - 2 * h) // 2), -np.zeros((A - 2 * h) // 2)])
    return rng.permutation(x)


def _ties(rng, A):
    x = np.round(rng.standard_normal(A), 1)
    x[rng.random(A) < 0.02] = np.nan
    return x


def _unique_min(rng, A):
    x = np.round(rng.standard_normal(A), 1)    # ties everywhere but at the minimum
    x[rng.integers(A)] = -10.0
    return x


def _one_owner(rng, A):
    # all four winsor order statistics fall in one tie group
    x = np.full(A, 1.0)
    i = rng.choice(A, 20, replace=False)
    x[i[:10]] = -3.0 - rng.random(10)
    x[i[10:]] = 3.0 + rng.random(10)
    return x


ROWS = [
    [_all_nan, lambda r, A: _few(r, A, 1), lambda r, A: _few(r, A, 4), lambda r, A: _few(r, A, 5), _const, _generic],
    [_tiny_spread, _huge, _zeros, _ties, _unique_min, _one_owner],
    [_tiny, _big, _generic, _ties, lambda r, A: _few(r, A, 6), _generic],
]
LENGTHS = [4100, 4609, 5000, 5119, 5120]


@functools.lru_cache(maxsize=None)
def _case(A, group):
    """(X [F][D][A], oracle outputs); made once per (A, group) and not modified."""
    import oracle.numerics as nm
    import oracle.ops as O
    rng = np.random.default_rng(1000 * group + A)
    X = np.stack([fn(rng, A) for fn in ROWS[group]]).reshape(F, D, A)
    with np.errstate(all="ignore"):
        ref = {
            "rank": np.stack([O.cs_rank(X[f]) for f in range(F)]),
            "winsor": np.stack([O.cs_winsor(X[f], limits=(QLO, QHI)) for f in range(F)]),
            "zscore": np.stack([O.cs_zscore(X[f]) for f in range(F)]),
            "neutralize": np.stack([O.market_neutralize(X[f]) for f in range(F)]),
        }
    r2 = np.zeros(X.shape, dtype=np.int64)
    for f in range(F):
        for d in range(D):
            r = nm.series_rank(X[f, d], "average")
            ok = ~np.isnan(r)
            r2[f, d, ok] = np.rint(2 * r[ok]).astype(np.int64)
    ref["rank2"] = r2
    for v in (X, *ref.values()):
        v.setflags(write=False)
    return X, ref


def _same(got, ref, what):
    """the exact comparison of tests/test_gpu_parity.py: NaN in the same places, every other
    value equal, and the same sign bit (cs_winsor excepted: its -0.0 comes back as +0.0, the
    rank keys fold the two zeros)."""
    from golden_io import assert_close
    assert_close(got, ref, exact=True, what=what)
    if what != "winsor":                       # == takes -0.0 for +0.0: the sign of zero apart
        ok = ~np.isnan(ref)
        assert np.array_equal(np.signbit(got[ok]), np.signbit(ref[ok])), what + ": sign of zero"


def _padded(X, ld, dev):
    import torch
    Xp = np.full(X.shape[:2] + (ld,), PAD_IN)
    Xp[:, :, :X.shape[2]] = X
    return torch.as_tensor(Xp, device=dev)


def _check(outs, rk, ref, A, names=("rank", "winsor", "zscore", "neutralize"), rows=slice(None)):
    for name, o in zip(names, outs):
        g = o.cpu().numpy()
        _same(g[:, rows, :A], ref[name][:, rows], name)
        assert (g[:, :, A:] == PAD_OUT).all(), name + ": wrote past the row"
    g = rk.cpu().numpy().view(np.uint16).astype(np.int64)
    assert np.array_equal(g[:, rows, :A], ref["rank2"][:, rows]), "rank2"
    assert (g[:, :, A:] == PAD_RK).all(), "rank2: wrote past the row"


@pytest.mark.parametrize("group", range(len(ROWS)))
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("A", LENGTHS)
def test_fused_pass_vs_oracle(dev, A, pad, group):
    import torch
    import factormodeling_amd.engine as E
    from factormodeling_amd._lib import call, ptr, stream_ptr
    X, ref = _case(A, group)
    ld = A + pad
    Xd = _padded(X, ld, dev)
    outs = [torch.full_like(Xd, PAD_OUT) for _ in range(4)]
    rk = torch.full(Xd.shape, PAD_RK, dtype=E.RANK2_DTYPE, device=dev)
    call("fmx_cs_rank_winsor_zn", ptr(Xd), *[ptr(o) for o in outs], F, D, A, ld, QLO, QHI, ptr(rk), stream_ptr())
    torch.cuda.synchronize()
    _check(outs, rk, ref, A)


@pytest.mark.parametrize("group", range(len(ROWS)))
@pytest.mark.parametrize("A", [700, 3000, 6000, 7000, 10000])
def test_fused_pass_other_slot_counts_vs_oracle(dev, A, group):
    """The fused pass's other instantiations: 512 threads x 2, 6, 12 and 16 slots (7000: the
    slot count rounded up from 14) and 1024 x 10, ld = A + 3."""
    test_fused_pass_vs_oracle(dev, A, 3, group)


@pytest.mark.parametrize("A", [4100, 5000])
def test_fused_pass_date_range_vs_oracle(dev, A):
    """dates = (1, 3): the rows of those dates as the oracle has them, date 0 untouched."""
    import torch
    import factormodeling_amd.engine as E
    X, ref = _case(A, 1)
    Xd = _padded(X, A, dev)
    outs = [torch.full_like(Xd, PAD_OUT) for _ in range(4)]
    rk = torch.full(Xd.shape, PAD_RK, dtype=E.RANK2_DTYPE, device=dev)
    E.cs_rank_winsor_zn(Xd, QLO, QHI, *outs, rank2=rk, dates=(1, 3))
    _check(outs, rk, ref, A, rows=slice(1, 3))
    for o in outs:
        assert (o[:, 0] == PAD_OUT).all()
    assert (rk[:, 0] == PAD_RK).all()


@pytest.mark.parametrize("group", range(len(ROWS)))
@pytest.mark.parametrize("A", [513, 3000])
def test_rank_winsor_and_ranks_only_vs_oracle(dev, A, group):
    """The template's other instantiations: cs_rank + cs_winsor (with doubled ranks) and the
    ranks-only pass, at row lengths of one-and-a-bit and six slots, ld = A + 3."""
    import torch
    import factormodeling_amd.engine as E
    from factormodeling_amd._lib import call, ptr, stream_ptr
    X, ref = _case(A, group)
    ld = A + 3
    Xd = _padded(X, ld, dev)
    outs = [torch.full_like(Xd, PAD_OUT) for _ in range(2)]
    rk = torch.full(Xd.shape, PAD_RK, dtype=E.RANK2_DTYPE, device=dev)
    call("fmx_cs_rank_winsor", ptr(Xd), ptr(outs[0]), ptr(outs[1]), F, D, A, ld, QLO, QHI, None, ptr(rk),
         stream_ptr())
    torch.cuda.synchronize()
    _check(outs, rk, ref, A, names=("rank", "winsor"))
    rk2 = torch.full(Xd.shape, PAD_RK, dtype=E.RANK2_DTYPE, device=dev)
    call("fmx_cs_rank2", ptr(Xd), ptr(rk2), F, D, A, ld, stream_ptr())
    torch.cuda.synchronize()
    _check([], rk2, ref, A, names=())
