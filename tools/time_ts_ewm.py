#!/usr/bin/env python
"""Kernel time of the exponentially weighted operators (fmx_ts_ewm) on synthetic dense panels,
with the unchanged ``fmx_ts_op(FMX_TS_STD, 20)`` and ``fmx_ts_corr(60)`` on the same panel as
yardsticks, and, for panels up to ``--pandas-max-cells``, the drop-in call against pandas
``groupby(level="symbol").ewm`` on the host.

    python tools/time_ts_ewm.py [--sizes 2520x5000x8,500x1000x20] [--span 20] [--out FILE]

Sizes are D x A x F.  Values: standard normal, 1 % NaN; the pair series is one [D][A] panel.

* ``kernel_ms``: one call between two device events, outputs preallocated (median of
  ``--reps`` calls after a warm-up call);
* ``vs_ts_std`` / ``vs_ts_corr``: kernel_ms over the yardstick's kernel_ms in the same run;
* ``gbps``: the algorithmic bytes (8 read, 16 for the pair, + 8 per output written) over
  kernel_ms;
* ``waves``: the one-wave workgroups of the launch, F * ceil(A / 64) (dates are not split);
* ``dropin_ms`` / ``pandas_ms``: wall clock of ``operations.ts_ewm_*`` on a (date, symbol) frame
  of F columns (densify, upload, kernel, gather back) and of the pandas expression (one run);
  ``equal_to_pandas`` compares the two results as values.
One JSON line per (panel, variant).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = (("mean", ("mean",)), ("mean+var+std+zscore", ("mean", "var", "std", "zscore")), ("corr", ("corr",)))


def make_panel(F, D, A, seed=7):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((F, D, A))
    x[rng.random(x.shape) < 0.01] = np.nan
    y = rng.standard_normal((D, A)) + 0.2 * np.nan_to_num(x[0])
    y[rng.random(y.shape) < 0.01] = np.nan
    return x, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2520x5000x8,500x1000x20")
    ap.add_argument("--span", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pandas-max-cells", type=int, default=10_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_ts_ewm.py needs a GPU")
    import pandas as pd
    import factormodeling_amd.engine as E
    import factormodeling_amd.operations as ops
    from factormodeling_amd._lib import TS, call, ptr, stream_ptr
    dev = torch.device("cuda", 0)
    com = (args.span - 1) / 2
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
        xh, yh = make_panel(F, D, A)
        X = torch.as_tensor(xh, device=dev)
        Yc = torch.as_tensor(yh, device=dev)
        O = [torch.empty_like(X) for _ in range(4)]
        cells = F * D * A
        std_ms = timed(lambda: call("fmx_ts_op", TS["std"], ptr(X), ptr(O[0]), F, D, A, A, 20, None, stream_ptr()))
        corr_ms = timed(lambda: call("fmx_ts_corr", ptr(X), ptr(Yc), ptr(O[0]), F, D, A, A, 0, 60, None, stream_ptr()))
        base = dict(D=D, A=A, F=F, span=args.span, waves=F * ((A + 63) // 64), device=E.device_info())
        rows = [dict(base, op="ts_std(20)", kernel_ms=std_ms, bytes_per_cell=16),
                dict(base, op="ts_corr(60)", kernel_ms=corr_ms, bytes_per_cell=16 + 8 / F)]
        for name, want in VARIANTS:
            outs = {k: O[i] for i, k in enumerate(want)}
            y = Yc if "corr" in want else None
            ms = timed(lambda: E.ts_ewm(X, dict(outs), com, True, False, 0, None, y))
            rows.append(dict(base, op="ts_ewm " + name, kernel_ms=ms,
                             bytes_per_cell=8 + (8 / F if y is not None else 0) + 8 * len(want)))
        for r in rows:
            r["vs_ts_std"] = r["kernel_ms"] / std_ms
            r["vs_ts_corr"] = r["kernel_ms"] / corr_ms
            r["gbps"] = r["bytes_per_cell"] * cells / (r["kernel_ms"] * 1e-3) / 1e9
        if cells <= args.pandas_max_cells:
            idx = pd.MultiIndex.from_product([pd.bdate_range("2015-01-01", periods=D), [f"S{a:05d}" for a in range(A)]],
                                             names=["date", "symbol"])
            df = pd.DataFrame(xh.reshape(F, D * A).T, index=idx, columns=[f"f{k}" for k in range(F)])
            sy = pd.Series(yh.reshape(-1), index=idx, name="y")
            ops.ts_ewm_mean(df, span=args.span)                  # warm the drop-in path (panel index, allocator)
            for r, fn, extra, expr in (
                    (rows[2], ops.ts_ewm_mean, (),
                     lambda: df.groupby(level="symbol").ewm(span=args.span).mean().droplevel(0).reindex(idx)),
                    (rows[4], ops.ts_ewm_corr, (sy,),
                     lambda: df.groupby(level="symbol").transform(
                         lambda c: c.ewm(span=args.span).corr(sy.reindex(c.index))))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = fn(df, *extra, span=args.span)
                r["dropin_ms"] = 1e3 * (time.perf_counter() - t0)
                t0 = time.perf_counter()
                ref = expr()
                r["pandas_ms"] = 1e3 * (time.perf_counter() - t0)
                r["pandas_over_dropin"] = r["pandas_ms"] / r["dropin_ms"]
                r["equal_to_pandas"] = bool(np.array_equal(got.to_numpy(), ref.to_numpy(), equal_nan=True))
        for r in rows:
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
        del X, Yc, O
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
