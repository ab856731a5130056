#!/usr/bin/env python
"""Kernel time of the rolling order statistics (fmx_ts_order) on synthetic dense panels, with
the unchanged ``fmx_ts_op(FMX_TS_RANK)`` on the same panel and window as the yardstick, and,
for panels up to ``--pandas-max-cells``, the drop-in call against the pandas
``groupby(level="symbol").transform(rolling ...)`` expression on the host.

    python tools/time_ts_order.py [--sizes 2520x5000x8,500x1000x20] [--windows 20,60] [--out FILE]

Sizes are D x A x F.  Values: standard normal, 20 % rounded to one decimal (ties), 1 % NaN.

* ``kernel_ms``: one launch between two device events, output preallocated (median of
  ``--reps`` launches after a warm-up launch);
* ``vs_rank``: kernel_ms over ts_rank's kernel_ms in the same run;
* ``gbps``: the algorithmic 16 B per output (8 read + 8 written) over kernel_ms;
* ``dropin_ms`` / ``pandas_ms``: wall clock of ``operations.ts_*`` on a (date, symbol) frame of
  F columns (densify, upload, kernel, gather back) and of the pandas expression (one run;
  ``rolling.apply`` for argmin / argmax runs on ``--apply-symbols`` symbols, scaled to A);
  ``equal_to_pandas`` compares the two results as values.
One JSON line per (panel, window, operator).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OPS = (("min", ()), ("max", ()), ("argmin", ()), ("argmax", ()), ("median", ()), ("quantile", (0.25, "linear")))


def make_panel(F, D, A, seed=7):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((F, D, A))
    x = np.where(rng.random(x.shape) < 0.2, np.round(x, 1), x)
    x[rng.random(x.shape) < 0.01] = np.nan
    return x


def _arg_back(fn):
    return lambda w: np.nan if np.isnan(w).any() else float(fn(w[::-1]))


def pandas_expr(df, op, W, extra):
    def roll(c):
        r = c.rolling(W)
        if op in ("min", "max", "median"):
            return getattr(r, op)()
        if op == "argmin":
            return r.apply(_arg_back(np.argmin), raw=True)
        if op == "argmax":
            return r.apply(_arg_back(np.argmax), raw=True)
        return r.quantile(extra[0], interpolation=extra[1])
    return df.groupby(level="symbol").transform(roll)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2520x5000x8,500x1000x20")
    ap.add_argument("--windows", default="20,60")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pandas-max-cells", type=int, default=10_000_000)
    ap.add_argument("--apply-symbols", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_ts_order.py needs a GPU")
    import pandas as pd
    import factormodeling_amd.engine as E
    import factormodeling_amd.operations as ops
    from factormodeling_amd._lib import TS, TSO, TSO_INTERP, call, ptr, stream_ptr
    dev = torch.device("cuda", 0)
    lines = []

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
        xh = make_panel(F, D, A)
        X = torch.as_tensor(xh, device=dev)
        Y = torch.empty_like(X)
        with_pandas = F * D * A <= args.pandas_max_cells
        if with_pandas:
            idx = pd.MultiIndex.from_product([pd.bdate_range("2015-01-01", periods=D), [f"S{a:05d}" for a in range(A)]],
                                             names=["date", "symbol"])
            df = pd.DataFrame(xh.reshape(F, D * A).T, index=idx, columns=[f"f{k}" for k in range(F)])
            ops.ts_min(df, 5)                                    # warm the drop-in path (panel index, allocator)
        for W in (int(v) for v in args.windows.split(",")):
            rank_ms = timed(lambda: call("fmx_ts_op", TS["rank"], ptr(X), ptr(Y), F, D, A, A, W, None, stream_ptr()))
            base = dict(D=D, A=A, F=F, window=W, device=E.device_info())
            rows = [dict(base, op="ts_rank", kernel_ms=rank_ms, vs_rank=1.0)]
            for op, extra in OPS:
                q = extra[0] if extra else 0.5
                interp = TSO_INTERP[extra[1]] if extra else 0
                ms = timed(lambda: call("fmx_ts_order", TSO[op], ptr(X), ptr(Y), F, D, A, A, W, q, interp, None,
                                        stream_ptr()))
                rows.append(dict(base, op="ts_" + op, kernel_ms=ms, vs_rank=ms / rank_ms))
            for r in rows:
                r["gbps"] = 16.0 * F * D * A / (r["kernel_ms"] * 1e-3) / 1e9
                if with_pandas and r["op"] != "ts_rank":
                    op = r["op"][3:]
                    extra = dict(OPS)[op]
                    fn = getattr(ops, r["op"])
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got = fn(df, W, *extra)
                    r["dropin_ms"] = 1e3 * (time.perf_counter() - t0)
                    # rolling.apply calls Python once per row: argmin / argmax run pandas on the
                    # first --apply-symbols symbols and scale the time to A
                    ns = min(A, args.apply_symbols) if op.startswith("arg") else A
                    keep = idx.get_level_values("symbol") < f"S{ns:05d}"
                    sub = df[keep]
                    t0 = time.perf_counter()
                    ref = pandas_expr(sub, op, W, extra)
                    r["pandas_ms"] = 1e3 * (time.perf_counter() - t0) * A / ns
                    r["pandas_symbols"] = ns
                    r["pandas_over_dropin"] = r["pandas_ms"] / r["dropin_ms"]
                    r["equal_to_pandas"] = bool(np.array_equal(got[keep].to_numpy(), ref.to_numpy(), equal_nan=True))
                lines.append(json.dumps(r))
                print(lines[-1], flush=True)
        del X, Y
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
