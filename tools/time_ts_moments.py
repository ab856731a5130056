#!/usr/bin/env python
"""Kernel time of the rolling higher moments (fmx_ts_moment: ts_skew / ts_kurt / ts_cov) on
synthetic panels, dense and ragged, with the streaming ``fmx_ts_op(FMX_TS_STD)`` (skew / kurt)
and ``fmx_ts_corr`` (cov) at the same shape and window in the same process as comparators, a
device copy of the panel as the bandwidth yardstick and, for panels up to
``--pandas-max-cells``, the drop-in calls against the pandas expressions on the host.

    python tools/time_ts_moments.py [--sizes 2520x5000x8] [--windows 20,60] [--out FILE]

Sizes are D x A x F.  Values: standard normal, 1 % NaN; the pair series is one [D][A] panel;
the ragged mask has 10 % gaps and a third of the symbols listing late.

* ``kernel_ms``: one call between two device events, outputs preallocated (median of ``--reps``
  calls after a warm-up call);
* ``vs_comparator``: kernel_ms over the comparator's kernel_ms (``comparator`` names it);
* ``bytes_per_cell``: what the operator must move -- skew / kurt read X twice (the centre, then
  the walk), read the leaving row and write the result (32 B); cov reads x and the shared y, both
  again as the leaving pair, and writes (24 + 16 / F B); ts_std 24 B, ts_corr as cov;
* ``gbps`` = bytes_per_cell * cells / kernel_ms, ``of_copy`` = gbps over the rate of
  ``Tensor.copy_`` on the same panel (16 B per cell);
* ``waves``: the one-wave workgroups of the launch, F * ceil(A / 64) (dates are not split);
* ``dropin_ms`` / ``pandas_ms``: wall clock of ``operations.ts_*`` on a (date, symbol) frame of F
  columns (densify, upload, kernel, gather back) and of the pandas expression (one run);
  ``equal_to_pandas`` compares the two results as values.
One JSON line per (panel, layout, window, op).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_panel(F, D, A, seed=7):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((F, D, A))
    x[rng.random(x.shape) < 0.01] = np.nan
    y = rng.standard_normal((D, A)) + 0.2 * np.nan_to_num(x[0])
    y[rng.random(y.shape) < 0.01] = np.nan
    p = rng.random((D, A)) >= 0.10
    late = rng.random(A) < 1 / 3
    start = np.where(late, rng.integers(1, max(2, D // 2 + 1), A), 0)
    p &= np.arange(D)[:, None] >= start[None, :]
    return x, y, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2520x5000x8")
    ap.add_argument("--windows", default="20,60")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pandas-max-cells", type=int, default=110_000_000)
    ap.add_argument("--pandas-window", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_ts_moments.py needs a GPU")
    import pandas as pd
    import factormodeling_amd.engine as E
    import factormodeling_amd.operations as ops
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

    for size in args.sizes.split(","):
        D, A, F = (int(v) for v in size.split("x"))
        xh, yh, ph = make_panel(F, D, A)
        X = torch.as_tensor(xh, device=dev)
        Yc = torch.as_tensor(yh, device=dev)
        O = torch.empty_like(X)
        cells = F * D * A
        copy_ms = timed(lambda: O.copy_(X))
        copy_gbps = 16 * cells / (copy_ms * 1e-3) / 1e9
        base = dict(D=D, A=A, F=F, waves=F * ((A + 63) // 64), copy_ms=copy_ms, copy_gbps=copy_gbps,
                    device=E.device_info())
        pair_bytes = 24 + 16 / F
        for layout in ("dense", "ragged"):
            P = torch.as_tensor(ph.astype(np.uint8), device=dev) if layout == "ragged" else None
            for W in (int(w) for w in args.windows.split(",")):
                std_ms = timed(lambda: E.ts("std", X, W, P, O))
                corr_ms = timed(lambda: E.ts_corr(X, Yc, W, P, O))
                rows = [dict(op="ts_std", kernel_ms=std_ms, bytes_per_cell=24, comparator="ts_std", cmp_ms=std_ms),
                        dict(op="ts_corr", kernel_ms=corr_ms, bytes_per_cell=pair_bytes, comparator="ts_corr",
                             cmp_ms=corr_ms)]
                for op in ("skew", "kurt", "cov"):
                    ms = timed(lambda: E.ts_moment(op, X, W, P, Yc if op == "cov" else None, O))
                    rows.append(dict(op="ts_" + op, kernel_ms=ms, bytes_per_cell=pair_bytes if op == "cov" else 32,
                                     comparator="ts_corr" if op == "cov" else "ts_std",
                                     cmp_ms=corr_ms if op == "cov" else std_ms))
                for r in rows:
                    r["vs_comparator"] = r["kernel_ms"] / r.pop("cmp_ms")
                    r["gbps"] = r["bytes_per_cell"] * cells / (r["kernel_ms"] * 1e-3) / 1e9
                    r["of_copy"] = r["gbps"] / copy_gbps
                    emit(dict(base, layout=layout, window=W, **r))
        if cells <= args.pandas_max_cells:
            W = args.pandas_window
            idx = pd.MultiIndex.from_product([pd.bdate_range("2015-01-01", periods=D), [f"S{a:05d}" for a in range(A)]],
                                             names=["date", "symbol"])
            df = pd.DataFrame(xh.reshape(F, D * A).T, index=idx, columns=[f"f{k}" for k in range(F)])
            sy = pd.Series(yh.reshape(-1), index=idx, name="y")
            ops.ts_skew(df, W)                                   # warm the drop-in path (panel index, allocator)
            ysym = dict(list(sy.groupby(level="symbol")))

            def pandas_cov():
                parts = [g.rolling(W).cov(ysym[k]) for k, g in df.groupby(level="symbol")]
                return pd.concat(parts).reindex(idx)
            for name, fn, extra, expr in (
                    ("ts_skew", ops.ts_skew, (), lambda: df.groupby(level="symbol").transform(
                        lambda c: c.rolling(W).skew())),
                    ("ts_kurt", ops.ts_kurt, (), lambda: df.groupby(level="symbol").transform(
                        lambda c: c.rolling(W).kurt())),
                    ("ts_cov", ops.ts_cov, (sy,), pandas_cov)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = fn(df, *extra, W)
                r = dict(base, layout="frame", window=W, op=name, dropin_ms=1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter()
                ref = expr()
                r["pandas_ms"] = 1e3 * (time.perf_counter() - t0)
                r["pandas_over_dropin"] = r["pandas_ms"] / r["dropin_ms"]
                r["equal_to_pandas"] = bool(np.array_equal(got.to_numpy(), ref.to_numpy(), equal_nan=True))
                emit(r)
        del X, Yc, O
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
