#!/usr/bin/env python
"""Times of the batched performance statistics (fmx_perf_stats / fmx_perf_periods,
factormodeling_amd.portfolio_analyzer) on synthetic dates x K tables of log returns, against a
per-column pandas loop written here (the reference class's expressions, one column at a time).

    python tools/time_analyzer.py [--sizes 2520x200,2520x2000] [--reps 7] [--pandas-cols 200] [--out FILE]

Sizes are T x K.  Values: 0.01 * standard normal, 1 % NaN, business days from 2015-01-01.
One JSON line per (table, job); the jobs are ``table`` (``performance_table``: fmx_perf_stats
without curves), ``curves`` (``performance_curves``: fmx_perf_stats with both curves) and
``periods_M`` / ``periods_Y`` (``period_returns``: fmx_perf_periods).

* ``kernel_ms``: the launch alone between two device events, table resident, outputs
  preallocated (median of ``--reps`` calls after a warm-up call); the periods are timed on the
  raw entry point with ``seg`` resident, without the engine's host check and upload of it;
* ``bytes_per_cell``: what the job must move -- one 8-byte read of the table (``table``,
  ``periods``), plus two 8-byte curve writes (``curves``); ``gbps`` = bytes_per_cell * T * K /
  kernel_ms and ``of_copy`` = gbps over the rate of ``Tensor.copy_`` on the same table (16 B per
  cell); both tables are cache-resident, and at 2,520 x 200 (4 MB) the copy is a launch's
  latency, so ``of_copy`` carries little meaning there;
* ``end_to_end_ms``: wall clock of the public function on the DataFrame (sort, exp, upload,
  launch, download, frame assembly; median of 3 calls after a warm-up call);
* ``pandas_ms``: wall clock of the per-column pandas loop over the first ``--pandas-cols`` columns,
  scaled to K columns where K is larger (``pandas_cols_timed`` says how many were timed);
  ``equal_to_pandas``: the timed columns compared as values, bit for bit.
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pandas_table(col, td=252):
    """The reference class's eight summary quantities of one column of log returns."""
    r = np.exp(col) - 1
    cum = (1 + r).cumprod() - 1
    days = (col.index[-1] - col.index[0]).days
    dd = (cum + 1) / (cum + 1).cummax() - 1
    root = np.sqrt(td)
    return [r.mean(), (cum.iloc[-1] + 1)**(1 / (days / 365.25)) - 1, r.std() * root, r.max(),
            (r.mean() / r.std()) * root, (r.mean() / r[r < 0].std()) * root, dd.min(), r.min()]


def pandas_curves(col):
    r = np.exp(col) - 1
    cum = (1 + r).cumprod() - 1
    return r, cum, (cum + 1) / (cum + 1).cummax() - 1


def pandas_periods(col, freq):
    return (np.exp(col) - 1).resample(freq).apply(lambda x: (1 + x).prod() - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2520x200,2520x2000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pandas-cols", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_analyzer.py needs a GPU")
    import pandas as pd
    import factormodeling_amd.engine as E
    import factormodeling_amd.portfolio_analyzer as PA
    from factormodeling_amd import _lib as L
    warnings.filterwarnings("ignore")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(r):
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)

    def timed(launch):
        launch()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    def wall(fn, n=3):
        fn()
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            ts.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ts)), out

    for size in args.sizes.split(","):
        T, K = (int(v) for v in size.split("x"))
        rng = np.random.default_rng(5)
        x = 0.01 * rng.standard_normal((T, K))
        x[rng.random(x.shape) < 0.01] = np.nan
        dates = pd.bdate_range("2015-01-01", periods=T)
        df = pd.DataFrame(x, index=dates, columns=[f"f{k:04d}" for k in range(K)])
        R = torch.as_tensor(np.ascontiguousarray(np.exp(x.T) - 1), device=dev)
        O = torch.empty_like(R)
        copy_ms = timed(lambda: O.copy_(R))
        copy_gbps = 16 * T * K / (copy_ms * 1e-3) / 1e9
        base = dict(T=T, K=K, copy_ms=copy_ms, copy_gbps=copy_gbps, device=E.device_info())
        outs = {"stats": torch.empty((E.PERF_NSTAT, K), dtype=torch.float64, device=dev), "cum": torch.empty_like(R),
                "dd": torch.empty_like(R)}
        npc = min(K, args.pandas_cols)
        cols = list(df.columns[:npc])

        def pandas_loop(fn):
            t0 = time.perf_counter()
            res = [fn(pd.Series(np.ascontiguousarray(df[c].to_numpy()), index=dates)) for c in cols]   # a contiguous column
            return 1e3 * (time.perf_counter() - t0) * (K / npc), res

        jobs = []
        k_ms = timed(lambda: E.perf_stats(R, 0.0, curves=False, out={"stats": outs["stats"]}))
        e_ms, tab = wall(lambda: PA.performance_table(df))
        p_ms, ref = pandas_loop(pandas_table)
        eq = np.array_equal(tab.iloc[:npc, :8].to_numpy(dtype=np.float64), np.array(ref, dtype=np.float64), equal_nan=True)
        jobs.append(("table", k_ms, 8, e_ms, p_ms, eq))
        k_ms = timed(lambda: E.perf_stats(R, 0.0, curves=True, out=outs))
        e_ms, cur = wall(lambda: PA.performance_curves(df))
        p_ms, ref = pandas_loop(pandas_curves)
        eq = all(np.array_equal(cur[name][c].to_numpy(), ref[j][i].to_numpy(), equal_nan=True)
                 for j, c in enumerate(cols) for i, name in enumerate(("return", "cumulative_return", "drawdown")))
        jobs.append(("curves", k_ms, 24, e_ms, p_ms, eq))
        for freq in ("M", "Y"):
            seg, labels = PA._period_buckets(pd.Series(dates), freq)
            po = torch.empty((len(labels), K), dtype=torch.float64, device=dev)
            seg_d = torch.as_tensor(np.ascontiguousarray(seg, dtype=np.int32), device=dev)
            k_ms = timed(lambda: L.call("fmx_perf_periods", L.ptr(R), K, T, T, L.ptr(seg_d), len(labels), L.ptr(po),
                                        L.stream_ptr()))
            e_ms, per = wall(lambda: PA.period_returns(df, freq))
            p_ms, ref = pandas_loop(lambda c: pandas_periods(c, "ME" if freq == "M" else "YE"))
            eq = all(np.array_equal(per[c].to_numpy(), ref[j].to_numpy(), equal_nan=True) for j, c in enumerate(cols))
            jobs.append((f"periods_{freq}", k_ms, 8, e_ms, p_ms, eq))
        for job, k_ms, bpc, e_ms, p_ms, eq in jobs:
            gbps = bpc * T * K / (k_ms * 1e-3) / 1e9
            emit(dict(base, job=job, kernel_ms=k_ms, bytes_per_cell=bpc, gbps=gbps, of_copy=gbps / copy_gbps,
                      end_to_end_ms=e_ms, pandas_ms=p_ms, pandas_cols_timed=npc, pandas_over_end_to_end=p_ms / e_ms,
                      equal_to_pandas=bool(eq)))
        del R, O, outs
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
