#!/usr/bin/env python
"""End-to-end time of single_factor_backtests: the one-pass route (backend="batched") against
the per-factor loop over Simulation (backend="loop"), back to back in one process, on
synthetic panels.

    python tools/time_factor_returns.py [--sizes 500x1000x20,252x5000x24] [--method equal] [--out FILE]

Sizes are D x A x F: C1 (500 x 1000 x 20) and a slice of C2 (one year of its 5000 symbols, 24
of its 200 factors: the loop's pandas work on the full 2520 x 5000 x 200 frame does not fit a
timing run).  Each route is timed once after a warm-up, wall clock around a device
synchronise; the loop's warm-up runs the first ``--loop-warmup`` factors only (it loads the
same kernels).  The two routes' tables are compared (they must be the same bits).  Also timed:
``engine.pnl_books`` alone on all F books (median of 5 calls, each with its range check's
read-back of the row tables), with the bytes of its traffic model (8 B per (factor, date,
asset) cell: every book row read once from HBM, its second use served by L2) over that time.
``--kernel-only`` runs just those calls, for a profiler run of its own.  One JSON line per size.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_inputs(D, A, F, seed=7):
    """Continuous signals with 3 % NaN cells and 2 % of the rows missing; returns and cap flags
    on two more dates, 2 % of their rows missing; an investability flag (5 % zeros) on the
    factors' own index."""
    rng = np.random.default_rng(seed)
    cal = pd.bdate_range("2015-01-01", periods=D + 2)
    syms = np.array([f"S{k:05d}" for k in range(A)], dtype=object)
    X = rng.standard_normal((D * A, F))
    X[rng.random(X.shape) < 0.03] = np.nan
    idx = pd.MultiIndex.from_product([cal[:D], syms], names=["date", "symbol"])
    factors_df = pd.DataFrame(X, index=idx, columns=[f"f{k:03d}" for k in range(F)])[rng.random(len(idx)) > 0.02]
    midx = pd.MultiIndex.from_product([cal, syms], names=["date", "symbol"])
    returns = pd.Series(0.01 * rng.standard_normal(len(midx)), index=midx, name="ret")[rng.random(len(midx)) > 0.02]
    cap = pd.Series(rng.integers(1, 4, len(midx)).astype(np.float64), index=midx)[rng.random(len(midx)) > 0.02]
    inv = pd.Series(np.where(rng.random(len(factors_df)) < 0.05, 0.0, 1.0), index=factors_df.index)
    return factors_df, returns, cap, inv


def time_kernel(factors_df, st, reps=6):
    """engine.pnl_books alone on all F books of the panel's union grid."""
    import torch
    import factormodeling_amd.engine as E
    import factormodeling_amd.factor_backtest as FB
    import factormodeling_amd.portfolio_simulation as PS
    from factormodeling_amd.panel import device, panel_index
    dev = device()
    pi = panel_index(factors_df.index)
    g = PS._Grid(factors_df.iloc[:, 0], st.returns, st.cap_flag)
    dG = g.dates.get_indexer(pi.dates)[pi.d]
    sG = g.symbols.get_indexer(pd.Index(np.asarray(pi.symbols, dtype=object)))[pi.s]
    present = np.zeros((g.D, g.A), dtype=bool)
    present[dG, sG] = True
    F = factors_df.shape[1]
    X = torch.full((F, g.D * g.A), float("nan"), dtype=torch.float64, device=dev)
    X[:, torch.as_tensor(dG * g.A + sG, device=dev)] = torch.as_tensor(
        np.ascontiguousarray(factors_df.to_numpy(dtype=np.float64).T), device=dev)
    _, _, W = E.trade_books(X.reshape(F, g.D, g.A), st.method, st.pct, st.max_weight,
                            present=torch.as_tensor(present.astype(np.uint8), device=dev), nan_absent=False, raw=True)
    del X
    rows = np.flatnonzero(present.any(axis=1))
    wprev = np.full(g.D, -1, dtype=np.int32)
    wprev[rows[1:]] = rows[:-1]
    R = torch.as_tensor(g.dense(st.returns), device=dev)
    CAP = torch.as_tensor(g.dense(st.cap_flag), device=dev)
    prev = torch.as_tensor(FB._prev_rows(present), device=dev)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        E.pnl_books(W, R, CAP, wprev, prev)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times[1:])), 8.0 * F * g.D * g.A


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500x1000x20,252x5000x24")
    ap.add_argument("--method", default="equal", choices=["equal", "linear"])
    ap.add_argument("--loop-warmup", type=int, default=2)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_factor_returns.py needs a GPU")
    import factormodeling_amd.engine as E
    from factormodeling_amd.factor_backtest import single_factor_backtests
    from factormodeling_amd.portfolio_simulation import SimulationSettings
    lines, bad = [], []
    for size in args.sizes.split(","):
        D, A, F = (int(v) for v in size.split("x"))
        factors_df, returns, cap, inv = make_inputs(D, A, F)
        st = SimulationSettings(returns=returns, cap_flag=cap, investability_flag=inv, factors_df=None,
                                method=args.method, plot=False)
        res = {"D": D, "A": A, "F": F, "method": args.method, "device": E.device_info()}

        def run(backend, cols=None):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = single_factor_backtests(factors_df, st, columns=cols, backend=backend)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        if not args.kernel_only:
            run("batched")
            tb, ob = run("batched")
            print(f"{size}: batched {tb:.3f} s", flush=True)
            run("loop", list(factors_df.columns[:args.loop_warmup]) if args.loop_warmup else None)
            tl, ol = run("loop")
            same = all(ob[k].index.equals(ol[k].index) and ob[k].to_numpy().tobytes() == ol[k].to_numpy().tobytes()
                       for k in ob)
            print(f"{size}: per-factor loop {tl:.3f} s, ratio {tl / tb:.2f}, same bits: {same}", flush=True)
            res.update(batched_s=tb, loop_s=tl, ratio=tl / tb, same_bits=bool(same))
            if not same:
                bad.append(size)
        tk, model_bytes = time_kernel(factors_df, st)
        res.update(pnl_books_call_s=tk, pnl_books_model_bytes=model_bytes, pnl_books_model_gbps=model_bytes / tk / 1e9)
        print(f"{size}: pnl_books on {F} books {1e3 * tk:.3f} ms (median of 5 calls, with the range check's "
              f"read-back); model bytes over that time {model_bytes / tk / 1e9:.0f} GB/s", flush=True)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if bad:
        sys.exit(f"the two routes differ for {bad}")


if __name__ == "__main__":
    main()
