"""Host-side checks of the native MVO selection: the library exports and binds the new entry
points, and ``FactorSelector.prepare_selection`` routes ``method="mvo"`` to the device solver
or to the host loop as documented.  No GPU: the two paths are replaced by recorders."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import mvo_cases as MC


def test_mvo_entries_exported_and_bound():
    from factormodeling_amd import _lib
    lib = _lib.load()
    for name in ("fmx_mvo_windows", "fmx_mvo_windows_work_bytes", "fmx_mvo_covariance"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]
    assert lib.fmx_mvo_windows_work_bytes.restype is ctypes.c_int64
    assert lib.fmx_abi_version() == 1
    # mu [J][F] + Sigma [J][F][F] + lambda [J] doubles and one int32 status per window
    J, F = 2400, 200
    nb = lib.fmx_mvo_windows_work_bytes(2520, F, J)
    assert nb >= 8 * (J * F + J * F * F + J) + 4 * J
    assert lib.fmx_mvo_windows_work_bytes(10, 2, 0) == 0


def test_mvo_windows_rejects_bad_arguments_before_any_launch():
    from factormodeling_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(8)      # never dereferenced: the checks come first
    for F, max_iter, eps in ((1, 10, 1e-9), (257, 10, 1e-9), (4, 0, 1e-9), (4, 10, 0.0)):
        st = lib.fmx_mvo_windows(one, 10, F, one, one, 1, 1.0, 1.0, 0.0, None, 1, max_iter, eps, one, one, one,
                                 1 << 30, None)
        assert st != 0
    assert lib.fmx_mvo_windows(one, 10, 4, one, one, 1, 1.0, 1.0, 0.0, None, 1, 10, 1e-9, one, one, one, 8, None) != 0


def _selector(monkeypatch, F=4, dup=False, **kw):
    import factormodeling_amd.factor_selector as fs
    D, A = 12, 3
    dates = pd.bdate_range("2022-01-03", periods=D)
    idx = pd.MultiIndex.from_product([dates, [f"S{i}" for i in range(A)]], names=["date", "symbol"])
    names = [f"f{k}" for k in range(F)]
    rng = np.random.default_rng(0)
    df = pd.DataFrame(rng.standard_normal((D * A, F)), index=idx, columns=names)
    ret = pd.Series(0.01 * rng.standard_normal(D * A), index=idx)
    fret = pd.DataFrame(0.01 * rng.standard_normal((D, F)), index=dates, columns=names)
    if dup:
        fret = pd.concat([fret, fret.iloc[[3]]])
    sel = fs.FactorSelector(df, ret, fret, window=4, method="mvo", method_kwargs=kw)
    taken = []

    def path(name):
        def run(self, *a):
            taken.append(name)
            return pd.DataFrame(1.0, index=pd.Index(self.dates[self.window:-1]), columns=names)
        return run
    monkeypatch.setattr(fs.FactorSelector, "_select_mvo_device", path("device"))
    monkeypatch.setattr(fs.FactorSelector, "_select_general", path("host"))
    out = sel.prepare_selection()
    assert out.shape == (D - 5, F)
    return taken


def test_mvo_takes_the_device_branch(monkeypatch):
    assert _selector(monkeypatch) == ["device"]
    assert _selector(monkeypatch, F=2, risk_aversion=5, max_weight=0.5) == ["device"]
    assert _selector(monkeypatch, F=256) == ["device"]
    assert _selector(monkeypatch, backend="native") == ["device"]


@pytest.mark.parametrize("kw", [dict(backend="reference"), dict(F=1), dict(dup=True), dict(F=257)],
                         ids=["backend-reference", "one-factor", "duplicate-date", "too-many-factors"])
def test_mvo_falls_back_to_the_host_loop(monkeypatch, kw):
    assert _selector(monkeypatch, **kw) == ["host"]


def test_replaced_registry_entry_keeps_the_host_loop(monkeypatch):
    import factormodeling_amd.factor_selector as fs

    def mine(metrics_df, *a, **k):
        return pd.Series(1.0, index=metrics_df.index)
    monkeypatch.setitem(fs.FACTOR_SELECTION_METHODS, "mvo", mine)
    assert _selector(monkeypatch) == ["host"]


def test_kkt_certificate_separates_optimal_from_perturbed():
    """The certificate the GPU tests rely on: ~0 at SLSQP's optimum, large off it."""
    R = MC.make_returns(60, 8, 11)
    mu, S = R.mean(axis=0), np.cov(R, rowvar=False)
    w = MC.slsqp(mu, S, 5.0, 0.3)
    w = np.where(w < 1e-12, 0.0, np.where(w > 0.3 - 1e-12, 0.3, w))
    viol, scale = MC.kkt_violation(mu, S, w, 5.0, 0.3)
    assert viol <= 1e-6 * scale
    w2 = w.copy()                    # still feasible, no longer optimal
    w2[np.argmax(w)] -= 0.01
    w2[np.argmin(w)] += 0.01
    viol2, scale2 = MC.kkt_violation(mu, S, w2, 5.0, 0.3)
    assert viol2 > 1e-3 * scale2
