"""Per-kernel timing harness (development tool, not the driver bench).

    python tools/kbench.py [--dates D --assets A --factors F] [--ops cs_rank,ic,...] [--reps N]
    python tools/kbench.py --ops mvo [--mvo-windows J --factors F --mvo-window W] [--reps N]
    python tools/kbench.py --ops sim_mvo [--dates D --assets A --lookback L --max-weight U] [--reps N]
    python tools/kbench.py --ops sim_mvo_turnover [--dates D --assets A --lookback L --max-weight U --penalty T
                                                  --return-weight R --chains B] [--reps N]
    python tools/kbench.py --ops qbacktest [--dates D --assets A --factors F --groups 5,10 --e2e] [--reps N]

The panel is generated on the host with numpy (SURVEY 8(d) statistics: N(0,1), 1% NaN,
5% rounded to one decimal) for a small factor block and tiled along the factor axis on
the device, so no torch RNG kernels run (rocprofv3 --pmc passes stay clean).  Each op is
timed with HIP events on the current stream; GB/s uses the algorithmic 16 B per
factor·asset·day of a unary operator (8 B for the IC stage).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if "--phases" in sys.argv:   # phase-timer build of libfmx (make -C factormodeling_amd/csrc prof)
    os.environ["FMX_LIB"] = os.path.join(ROOT, "factormodeling_amd", "libfmx_prof.so")
from factormodeling_amd import engine as E  # noqa: E402
from factormodeling_amd import _lib  # noqa: E402


def read_phases():
    import ctypes
    lib = _lib.load()
    out = {}
    for tu in ("cs", "hot", "q", "ic"):
        buf = (ctypes.c_ulonglong * 32)()
        getattr(lib, "fmx_debug_phase_" + tu)(buf)
        v = [int(x) for x in buf]
        if any(v):
            tot = sum(v)
            out[tu] = [round(x / tot, 3) for x in v if x] + [f"total {tot * 10 / 1e6:.1f} ms-WG"]
    return out


def panel(D, A, F, seed=0, block=8):
    rng = np.random.default_rng(seed)
    fb = min(F, block)
    x = rng.standard_normal((fb, D, A))
    u = rng.random((fb, D, A))
    x = np.where(u < 0.05, np.round(x, 1), x)
    x[u > 0.99] = np.nan
    r = 0.01 * rng.standard_normal((D, A))
    r[rng.random((D, A)) < float(os.environ.get("KB_R_NAN", "0.005"))] = np.nan
    Xb = torch.as_tensor(x, device="cuda")
    reps = (F + fb - 1) // fb
    X = Xb.repeat(reps, 1, 1)[:F].contiguous()
    return X, torch.as_tensor(r, device="cuda")


_SET = {}


def _set_outs(X):
    if not _SET:
        _SET.update({k: torch.empty_like(X) for k in E.TS_SET})
    return _SET


_RK = {}


def _rank2(X):
    """doubled ranks of X (made once, by the fused rank pass)."""
    if "rk" not in _RK:
        _RK["rk"] = torch.empty(X.shape, dtype=E.RANK2_DTYPE, device=X.device)
        E.cs_rank_winsor(X, 0.01, 0.99, rank2=_RK["rk"])
    return _RK["rk"]


_PR = {}


def _pres(X):
    """a ragged presence mask (10 % of rows absent), made once."""
    if "p" not in _PR:
        g = torch.Generator(device="cpu").manual_seed(5)
        _PR["p"] = (torch.rand(X.shape[1:], generator=g) > 0.1).to(torch.uint8).to(X.device)
    return _PR["p"]


_HR = {}


def _head_rows_n(F):
    return min(int(os.environ.get("KB_GRAM_HEAD", "32")), F)


def _head_rows(X):
    """a device list of distinct rows in no order (made once): the head of a prune order."""
    if "r" not in _HR:
        g = torch.Generator(device="cpu").manual_seed(7)
        _HR["r"] = torch.randperm(X.shape[0], generator=g)[:_head_rows_n(X.shape[0])].to(X.device)
    return _HR["r"]


OPS = {
    "ts_mean":(lambda X, R, Y: E.ts("mean", X, 20, out=Y), 16),
    "ts_std": (lambda X, R, Y: E.ts("std", X, 20, out=Y), 16),
    "ts_zscore": (lambda X, R, Y: E.ts("zscore", X, 20, out=Y), 16),
    "ts_rank": (lambda X, R, Y: E.ts("rank", X, 10, out=Y), 16),
    "ts_decay": (lambda X, R, Y: E.ts("decay", X, 20, out=Y), 16),
    # long windows (any W: k_ts_win tiles for rank / decay, k_ts_rl / k_ts_ptr for moments)
    "ts_decay80": (lambda X, R, Y: E.ts("decay", X, 80, out=Y), 16),
    "ts_decay150": (lambda X, R, Y: E.ts("decay", X, 150, out=Y), 16),
    "ts_decay350": (lambda X, R, Y: E.ts("decay", X, 350, out=Y), 16),
    "ts_rank60": (lambda X, R, Y: E.ts("rank", X, 60, out=Y), 16),
    "ts_rank200": (lambda X, R, Y: E.ts("rank", X, 200, out=Y), 16),
    "ts_mean175": (lambda X, R, Y: E.ts("mean", X, 175, out=Y), 16),
    "ts_mean20_rg": (lambda X, R, Y: E.ts("mean", X, 20, present=_pres(X), out=Y), 16),
    "ts_std175_rg": (lambda X, R, Y: E.ts("std", X, 175, present=_pres(X), out=Y), 16),
    "ts_decay150_rg": (lambda X, R, Y: E.ts("decay", X, 150, present=_pres(X), out=Y), 16),
    "ts_rank10_rg": (lambda X, R, Y: E.ts("rank", X, 10, present=_pres(X), out=Y), 16),
    "cs_rank": (lambda X, R, Y: E.cs_rank(X, out=Y), 16),
    "cs_zscore": (lambda X, R, Y: E.cs_moment("zscore", X, out=Y), 16),
    "market_neutralize": (lambda X, R, Y: E.cs_moment("market_neutralize", X, out=Y), 16),
    "winsor": (lambda X, R, Y: E.cs_quantile_op("winsor", X, 0.01, 0.99, out=Y), 16),
    "ic": (lambda X, R, Y: E.ic_daily(X, R, (1, 2)), 8),
    "ts_set": (lambda X, R, Y: E.ts_set(X, _set_outs(X), 20, 10), 48),
    "ts_set60_20": (lambda X, R, Y: E.ts_set(X, _set_outs(X), 60, 20), 48),
    "cs_zn": (lambda X, R, Y: E.cs_zscore_neutralize(X, Y, _set_outs(X)["mean"]), 24),
    "cs_rw": (lambda X, R, Y: E.cs_rank_winsor(X, 0.01, 0.99, Y, _set_outs(X)["mean"]), 24),
    "cs_rw_rk": (lambda X, R, Y: E.cs_rank_winsor(X, 0.01, 0.99, Y, _set_outs(X)["mean"], rank2=_rank2(X)), 26),
    "cs_rwzn_rk": (lambda X, R, Y: E.cs_rank_winsor_zn(X, 0.01, 0.99, Y, _set_outs(X)["mean"], _set_outs(X)["std"],
                                                      _set_outs(X)["zscore"], rank2=_rank2(X)), 42),
    "ic_ranked": (lambda X, R, Y: E.ic_daily(X, R, (1, 2), rank2=_rank2(X)), 10),
    "cs_rw_ic": (lambda X, R, Y: E.cs_rank_winsor_ic(X, R, (1, 2), 0.01, 0.99, Y, _set_outs(X)["mean"],
                                                     rank2=_RK.setdefault("rk", torch.empty(X.shape, dtype=E.RANK2_DTYPE,
                                                                                            device=X.device))), 24),
    "ts_corr60": (lambda X, R, Y: E.ts_corr(X, R, 60, out=Y), 16),
    "cvf60": (lambda X, R, Y: E.corr_vol_feature(X, Y, 60, out=_set_outs(X)["mean"]), 24),
    "corr_feat60": (lambda X, R, Y: E.corr_feature(X, R, 60, out=Y), 16),
    "rank2": (lambda X, R, Y: E.cs_rank2(X, _RK.setdefault("rk2", torch.empty(X.shape, dtype=E.RANK2_DTYPE,
                                                                              device=X.device))), 10),
    "gram": (lambda X, R, Y: E.corr_matrix(X), 8),
    # the C2 step's Gram: exact fixed-point partials from the cs_zscore output (Y after cs_zn)
    "gram_exact_z": (lambda X, R, Y: E.gram_exact(Y, None), 8),
    # the lazy step's head block: the exact Gram of KB_GRAM_HEAD (32) scattered rows of Y, read in
    # place (bytes: those rows only)
    "gram_rows": (lambda X, R, Y: E.gram_exact_rows(Y, _head_rows(X)), lambda F: 8.0 * _head_rows_n(F) / F),
    # the C4 step's Gram straight from the panel (row stats + validity bits + tiles + popcount)
    "gram_direct": (lambda X, R, Y: E.gram_direct(X), 8),
    # the C4 step's exact Gram (absolute 16-date blocks folded into fixed-point limbs)
    "gram_direct_exact": (lambda X, R, Y: E.gram_direct_exact(X), 8),
    "gram_unfused": (lambda X, R, Y: E.gram(*E.zscore_exposures(X)), 8),
    "cs_stats": (lambda X, R, Y: E.cs_moment_stats("stats", X), 8),
}


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps, out


def bench_mvo(J, F, W, reps):
    """--ops mvo: the rolling MVO selection (engine.mvo_windows) over J windows of W rows of
    F factor returns, for two (risk_aversion, max_weight, turnover_penalty) settings.  Stage A
    is timed alone (engine.mvo_covariance), stage B is the whole call minus stage A; the
    K^-1 rate counts one F x F fp64 read per ADMM iteration."""
    rng = np.random.default_rng(0)
    D = J + W
    R = 0.01 * (0.6 * rng.standard_normal((D, 1)) + rng.standard_normal((D, F)) * rng.uniform(0.3, 2.0, F))
    R += 0.001 * rng.standard_normal(F)
    fret = torch.as_tensor(R, device="cuda")
    prev = torch.as_tensor(rng.dirichlet(np.ones(F)), device="cuda")
    d0 = np.arange(J, dtype=np.int32)
    d1 = d0 + np.int32(W)
    ms_a, _ = _timed(lambda: E.mvo_covariance(fret, d0, d1, True), reps)
    res = {"stage_a_ms": round(ms_a, 3), "settings": []}
    print(f"mvo J={J} F={F} W={W}: stage A {ms_a:.3f} ms", flush=True)
    for gamma, u, tau in ((10.0, 1.0, 0.0), (100.0, 0.05, 5e-4)):
        ms, (w, info) = _timed(lambda: E.mvo_windows(fret, d0, d1, gamma, u, tau, prev if tau > 0 else None), reps)
        info = info.cpu().numpy()
        it = info[:, 1]
        ms_b = ms - ms_a
        r = {"gamma": gamma, "max_weight": u, "tau": tau, "total_ms": round(ms, 3), "stage_b_ms": round(ms_b, 3),
             "iter_mean": round(float(it.mean()), 1), "iter_max": int(it.max()),
             "not_converged": int((info[:, 0] != 0).sum()),
             "kinv_GBs": round(float(it.sum()) * F * F * 8 / (ms_b * 1e-3) / 1e9, 1)}
        res["settings"].append(r)
        print("   ", r, flush=True)
    print(json.dumps({"mvo": {"J": J, "F": F, "W": W, **res}}))


def bench_sim_mvo(D, A, lookback, u, reps):
    """--ops sim_mvo: the simulator's MVO trade list (engine.sim_mvo_books) for D dates of A
    assets, every date's window the `lookback` returns rows before it (dates 0 and 1 take the
    equal-weight / x0 exits).  Reports ms per call and the histogram of ADMM iterations; the
    panel rate counts the 2 T A fp64 panel reads of one iteration."""
    rng = np.random.default_rng(0)
    R = 0.01 * (0.6 * rng.standard_normal((D, 1)) + rng.standard_normal((D, A)) * rng.uniform(0.3, 2.0, A))
    X = rng.standard_normal((D, A))
    X[rng.random((D, A)) < 0.05] = 0.0
    T = np.minimum(np.arange(D), lookback).astype(np.int32)
    L = min(lookback, max(D - 1, 1))
    rows = np.zeros((D, L), dtype=np.int32)
    for j in range(D):
        rows[j, :T[j]] = np.arange(j - T[j], j)
    R0, Xd = torch.as_tensor(R, device="cuda"), torch.as_tensor(X, device="cuda")
    rows_d, T_d = torch.as_tensor(rows, device="cuda"), torch.as_tensor(T, device="cuda")
    ms, (W, counts, info) = _timed(lambda: E.sim_mvo_books(R0, rows_d, T_d, Xd, None, 0.1, u), reps)
    info = info.cpu().numpy()
    qp = info[:, 0] <= 1
    it = info[qp, 1]
    edges = [0, 10, 20, 30, 40, 60, 80, 120, 200, 500, 20000]
    hist = {f"<={b}": int(((it > a) & (it <= b)).sum()) for a, b in zip(edges[:-1], edges[1:])}
    reads = float((it * T[qp]).sum()) * 2 * A * 8
    res = {"D": D, "A": A, "lookback": lookback, "max_weight": u, "ms": round(ms, 3),
           "status_counts": {int(k): int((info[:, 0] == k).sum()) for k in np.unique(info[:, 0])},
           "iter_mean": round(float(it.mean()), 1), "iter_max": int(it.max()), "iter_hist": hist,
           "panel_GBs": round(reads / (ms * 1e-3) / 1e9, 1)}
    print(json.dumps({"sim_mvo": res}))


def bench_sim_mvo_turnover(D, A, lookback, u, tau, rw, B, reps):
    """--ops sim_mvo_turnover: the chained mvo_turnover trade list
    (engine.sim_mvo_turnover_books) for B independent chains of D dates over one returns panel.
    Each chain's signal keeps its sign from one day to the next on all but a tenth of the cells
    (a fresh draw there).  Reports ms per call (set-up and chain kernels together), ADMM
    iterations mean / max and the histogram of statuses."""
    rng = np.random.default_rng(0)
    R = 0.01 * (0.6 * rng.standard_normal((D, 1)) + rng.standard_normal((D, A)) * rng.uniform(0.3, 2.0, A))
    X = np.empty((B, D, A))
    X[:, 0] = rng.standard_normal((B, A))
    for j in range(1, D):
        redraw = rng.random((B, A)) < 0.1
        X[:, j] = np.where(redraw, rng.standard_normal((B, A)), X[:, j - 1])
    X[rng.random((B, 1, A)).repeat(D, axis=1) < 0.05] = 0.0
    T = np.minimum(np.arange(D), lookback).astype(np.int32)
    L = min(lookback, max(D - 1, 1))
    rows = np.zeros((D, L), dtype=np.int32)
    for j in range(D):
        rows[j, :T[j]] = np.arange(j - T[j], j)
    R0, Xd = torch.as_tensor(R, device="cuda"), torch.as_tensor(X, device="cuda")
    rows_d, T_d = torch.as_tensor(rows, device="cuda"), torch.as_tensor(T, device="cuda")
    W0 = torch.zeros_like(Xd)
    W0[:, 0] = E.trade_books(Xd[:, :1].contiguous(), "equal", 0.1, u, nan_absent=False, raw=True)[2][:, 0]
    ms, (W, counts, info) = _timed(lambda: E.sim_mvo_turnover_books(R0, rows_d, T_d, Xd, None, W0, 0.1, u, tau, rw), reps)
    info = info.cpu().numpy().reshape(-1, 6)
    it = info[info[:, 0] <= 1, 1]
    res = {"D": D, "A": A, "lookback": lookback, "max_weight": u, "penalty": tau, "return_weight": rw, "chains": B,
           "ms": round(ms, 3), "ms_per_chain_date": round(ms / max(len(it), 1) * B, 4),
           "status_counts": {int(k): int((info[:, 0] == k).sum()) for k in np.unique(info[:, 0])},
           "iter_mean": round(float(it.mean()), 1), "iter_max": int(it.max()),
           "work_MiB": round(_lib.load().fmx_sim_mvo_turnover_books_work_bytes(A, L, D, B) / 2 ** 20, 1)}
    print(json.dumps({"sim_mvo_turnover": res}))


def bench_qbacktest(D, A, F, groups, reps, e2e):
    """--ops qbacktest: the quantile backtest's two kernels (engine.cs_qlabel, whose cut table
    and count pass are timed apart from the fmx_cs_qlabel launch, and engine.qbucket_mean on
    the plain-row and the gather path) and, in the same call and on the same rows,
    fmx_cs_rank(method="first").  Fractions of the 8 TB/s HBM peak count 9 B per cell for the
    labels (16 B for the rank) and 1 B per cell plus the returns rows for the means.  --e2e:
    the public function, pandas in and frames out, device against host."""
    import time
    from factormodeling_amd._lib import call, ptr, stream_ptr
    PEAK = 8e12
    X, R = panel(D, A, F)
    cells = float(D) * A * F
    res = {"dims": [D, A, F], "groups": {}}
    Y = torch.empty_like(X)
    ms_rank, _ = _timed(lambda: E.cs_rank(X, "first", out=Y), reps)
    del Y
    res["cs_rank_first_ms"] = round(ms_rank, 3)
    res["cs_rank_first_hbm_frac"] = round(16 * cells / (ms_rank * 1e-3) / PEAK, 4)
    print(f"cs_rank(first)      {ms_rank:9.3f} ms  {16 * cells / ms_rank / 1e6:8.1f} GB/s", flush=True)
    prev = torch.as_tensor(np.repeat(np.arange(-1, D - 1, dtype=np.int32)[:, None], A, axis=1), device="cuda")
    for n in groups:
        ms_all, lab = _timed(lambda: E.cs_qlabel(X, n), reps)
        ms = np.unique((~torch.isnan(X)).sum(dim=2).cpu().numpy())
        ms = [int(m) for m in ms if m >= 2]
        mi = np.full(A + 1, -1, dtype=np.int32)
        mi[ms] = np.arange(len(ms), dtype=np.int32)
        cum = torch.as_tensor(np.stack([E.qcut_cum(m, n) for m in ms]).astype(np.int32), device="cuda")
        mi = torch.as_tensor(mi, device="cuda")
        ms_k, _ = _timed(lambda: call("fmx_cs_qlabel", ptr(X), None, ptr(cum), ptr(mi), ptr(lab), F, D, A, A, n,
                                      stream_ptr()), reps)
        ms_m, (m0, c0) = _timed(lambda: E.qbucket_mean(lab, R, n), reps)
        ms_g, (m1, c1) = _timed(lambda: E.qbucket_mean(lab, R, n, prev_row=prev), reps)
        same = bool(torch.equal(c0, c1)) and m0.cpu().numpy().tobytes() == m1.cpu().numpy().tobytes()
        mbytes = cells + 8.0 * D * A * -(-F // 16)
        r = {"qlabel_kernel_ms": round(ms_k, 3), "qlabel_hbm_frac": round(9 * cells / (ms_k * 1e-3) / PEAK, 4),
             "qlabel_engine_ms": round(ms_all, 3), "distinct_m": len(ms),
             "vs_cs_rank_first": round(ms_k / ms_rank, 3),
             "qbucket_mean_ms": round(ms_m, 3), "qbucket_hbm_frac": round(mbytes / (ms_m * 1e-3) / PEAK, 4),
             "qbucket_gather_ms": round(ms_g, 3), "gather_equals_plain": same}
        res["groups"][n] = r
        print(f"n={n}:", r, flush=True)
        del lab, m0, c0, m1, c1
    if e2e:
        import pandas as pd
        from factormodeling_amd import composite_factor as cf
        idx = pd.MultiIndex.from_product([pd.bdate_range("2015-01-01", periods=D), [f"S{i:05d}" for i in range(A)]],
                                         names=["date", "symbol"])
        df = pd.DataFrame(X.reshape(F, D * A).T.cpu().numpy(), index=idx, columns=[f"f{k}" for k in range(F)])
        ret = pd.Series(R.reshape(-1).cpu().numpy(), index=idx)
        n = groups[0]
        cf.quantile_backtest_log(df.iloc[:, :1], ret, n, backend="device")          # warm-up
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            dv = cf.quantile_backtest_log(df, ret, n, backend="device")
            t.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        hs = cf.quantile_backtest_log(df, ret, n, backend="host")
        th = time.perf_counter() - t0
        err = max(float(np.nanmax(np.abs(dv[c].to_numpy() - hs[c].to_numpy(dtype=np.float64)))) for c in df.columns)
        res["e2e"] = {"n_groups": n, "device_s": round(min(t), 4), "host_s": round(th, 3),
                      "speedup": round(th / min(t), 1), "max_abs_diff": err}
        print("e2e:", res["e2e"], flush=True)
    print(json.dumps({"qbacktest": res}))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--groups", default="5,10")
    p.add_argument("--e2e", action="store_true")
    p.add_argument("--lookback", type=int, default=60)
    p.add_argument("--max-weight", type=float, default=0.03)
    p.add_argument("--penalty", type=float, default=0.1)
    p.add_argument("--return-weight", type=float, default=0.0)
    p.add_argument("--chains", type=int, default=1)
    p.add_argument("--mvo-windows", type=int, default=2400)
    p.add_argument("--mvo-window", type=int, default=120)
    p.add_argument("--dates", type=int, default=2520)
    p.add_argument("--assets", type=int, default=5000)
    p.add_argument("--factors", type=int, default=200)
    p.add_argument("--ops", default=",".join(OPS))
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--phases", action="store_true")
    a = p.parse_args()
    D, A, F = a.dates, a.assets, a.factors
    if a.ops == "mvo":            # no panel: factor returns only
        return bench_mvo(a.mvo_windows, F, a.mvo_window, a.reps)
    if a.ops == "sim_mvo":        # signal + returns panels only
        return bench_sim_mvo(D, A, a.lookback, a.max_weight, a.reps)
    if a.ops == "sim_mvo_turnover":
        return bench_sim_mvo_turnover(D, A, a.lookback, a.max_weight, a.penalty, a.return_weight, a.chains, a.reps)
    if a.ops == "qbacktest":      # its own panel, labels and the cs_rank(first) comparison
        return bench_qbacktest(D, A, F, [int(g) for g in a.groups.split(",")], a.reps, a.e2e)
    X, R = panel(D, A, F)
    Y = torch.empty_like(X)
    units = float(D) * A * F
    res = {}
    for name in a.ops.split(","):
        fn, bpu = OPS[name]
        if callable(bpu):
            bpu = bpu(F)
        fn(X, R, Y)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.reps):
            fn(X, R, Y)
        e.record()
        torch.cuda.synchronize()
        ms = s.elapsed_time(e) / a.reps
        res[name] = {"ms": round(ms, 3), "GBs": round(bpu * units / (ms * 1e-3) / 1e9, 1)}
        print(f"{name:18s} {ms:9.3f} ms  {res[name]['GBs']:8.1f} GB/s", flush=True)
        if a.phases:
            print("   phases:", read_phases(), flush=True)
    print(json.dumps({"dims": [D, A, F], "ops": res}))


if __name__ == "__main__":
    main()
