#!/usr/bin/env python
"""End-to-end time of compute_multimanager_weights with MVO managers: the batched device
route (simulation.mvo_manager_books) against the per-manager loop (multi_manager._host_books,
forced), back to back in one process, for 'mvo' and 'mvo_turnover'.

    python tools/time_mm_mvo.py [--F 32 --D 500 --A 1000 --lookback 60] [--out FILE]

Each route is timed once after one warm-up, wall clock around a device synchronise.  The loop's
warm-up for 'mvo_turnover' runs the first ``--loop-warmup`` managers only (default 2; 0 = all):
it loads the same kernels and sizes the same buffers, and the full loop takes minutes.  Also
timed: the window kernel alone (fmx_sim_mvo_window_rows on the F * D rows, median of 5).  The
two routes' results are compared (they must be the same bits) and one JSON line is printed.
'mvo_turnover' runs with FMX_SIM_MVO_TURNOVER=native on both routes: the loop is then the
per-manager native chain, one workgroup at a time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_inputs(F, D, A, lookback, seed=7):
    """Persistent signals (AR(1) over dates, 3% NaN cells), returns on ``lookback`` dates before
    the first feature date and on every feature date, 2% of the returns rows missing."""
    rng = np.random.default_rng(seed)
    cal = pd.bdate_range("2015-01-01", periods=lookback + D)
    fdates, syms = cal[lookback:], np.array([f"S{k:05d}" for k in range(A)], dtype=object)
    X = np.empty((D, A, F))
    X[0] = rng.standard_normal((A, F))
    for d in range(1, D):
        X[d] = 0.95 * X[d - 1] + np.sqrt(1 - 0.95 ** 2) * rng.standard_normal((A, F))
    X[rng.random(X.shape) < 0.03] = np.nan
    idx = pd.MultiIndex.from_product([fdates, syms], names=["date", "symbol"])
    names = [f"f{k:03d}" for k in range(F)]
    factors_df = pd.DataFrame(X.reshape(D * A, F), index=idx, columns=names)
    common = rng.standard_normal((len(cal), 1))
    R = 0.01 * (0.6 * common + rng.standard_normal((len(cal), A)) * rng.uniform(0.3, 2.0, A))
    ridx = pd.MultiIndex.from_product([cal, syms], names=["date", "symbol"])
    returns = pd.Series(R.reshape(-1), index=ridx, name="ret")[rng.random(len(ridx)) > 0.02]
    fw = pd.DataFrame(rng.random((D, F)), index=pd.Index(fdates, name="date"), columns=names)
    fw = fw.div(fw.sum(axis=1), axis=0)
    return factors_df, returns, fw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--F", type=int, default=32)
    ap.add_argument("--D", type=int, default=500)
    ap.add_argument("--A", type=int, default=1000)
    ap.add_argument("--lookback", type=int, default=60)
    ap.add_argument("--methods", default="mvo,mvo_turnover")
    ap.add_argument("--loop-warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_mm_mvo.py needs a GPU")
    os.environ["FMX_SIM_MVO_TURNOVER"] = "native"
    os.environ.pop("FMX_SIM_MVO", None)
    import factormodeling_amd.engine as E
    import factormodeling_amd.multi_manager as MM
    from factormodeling_amd.portfolio_simulation import SimulationSettings
    F, D, A = args.F, args.D, args.A
    factors_df, returns, fw = make_inputs(F, D, A, args.lookback)
    ones = pd.Series(1.0, index=factors_df.index)
    real_batched = MM._batched

    def run(method, batched, nm=F):
        cols = list(fw.columns[:nm])
        s = SimulationSettings(returns=returns, cap_flag=ones, investability_flag=ones, factors_df=factors_df,
                               method=method, lookback_period=args.lookback, plot=False)
        MM._batched = real_batched if batched else (lambda *a, **k: False)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w, c = MM.compute_multimanager_weights(factors_df[cols], fw[cols], s)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, w, c
        finally:
            MM._batched = real_batched

    res = {"F": F, "D": D, "A": A, "lookback": args.lookback, "device": E.device_info()}
    for method in args.methods.split(","):
        run(method, True)
        tb, wb, cb = run(method, True)
        print(f"{method}: batched {tb:.3f} s", flush=True)
        run(method, False, args.loop_warmup if method == "mvo_turnover" and args.loop_warmup else F)
        tl, wl, cl = run(method, False)
        same = bool(wb.index.equals(wl.index) and wb.to_numpy().tobytes() == wl.to_numpy().tobytes()
                    and cb.to_numpy().tobytes() == cl.to_numpy().tobytes())
        res[method] = {"batched_s": tb, "loop_s": tl, "ratio": tl / tb, "solved_per_s_batched": F * D / tb,
                       "solved_per_s_loop": F * D / tl, "same_bits": same}
        print(f"{method}: per-manager loop {tl:.3f} s, ratio {tl / tb:.2f}, same bits: {same}", flush=True)
    # the window kernel alone on the F * D rows
    from factormodeling_amd.panel import panel_index
    from factormodeling_amd.simulation import _returns_grid
    pi = panel_index(factors_df.index)
    rdates, rd, rs, keep = _returns_grid(pi, returns)
    rp = np.zeros((len(rdates), A), dtype=np.uint8)
    rp[rd[keep], rs[keep]] = 1
    X = pi.to_device(factors_df.to_numpy(dtype=np.float64), "cuda")
    fp = (X == X).to(torch.uint8).reshape(F * D, A)
    nb = torch.as_tensor(np.searchsorted(rdates, np.asarray(pi.dates)).astype(np.int32), device="cuda").repeat(F)
    RP = torch.as_tensor(rp, device="cuda")
    times = []
    for k in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        E.sim_mvo_window_rows(fp, RP, nb, args.lookback)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    res["window_rows_s"] = float(np.median(times[1:]))
    print(f"window kernel on {F * D} rows: {1e3 * res['window_rows_s']:.3f} ms (median of 5, with its range check's read-back)")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    bad = [m for m in args.methods.split(",") if not res[m]["same_bits"]]
    if bad:
        sys.exit(f"the two routes differ for {bad}")


if __name__ == "__main__":
    main()
