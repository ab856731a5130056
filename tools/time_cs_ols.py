#!/usr/bin/env python
"""Time of the per-date multi-factor OLS (engine.cs_ols / fmx_cs_ols) on synthetic panels,
against the same computation as a numpy ``lstsq`` loop over dates on the host.

    python tools/time_cs_ols.py [--sizes 500x1000,2520x5000] [--K 8,32] [--Fy 1,20] [--out FILE]

Per (D x A, K, Fy): N(0, 1) regressors with 0.1 % NaN cells, y = 0.01 (sum of the first three
columns) + noise with 3 % NaN cells, an intercept, no weights, all six outputs.

* ``call_ms``: wall clock of ``engine.cs_ols`` around a device synchronise (median of
  ``--reps`` calls after a warm-up) -- the launch plus the allocation of the outputs;
* ``kernel_ms``: the ``fmx_cs_ols`` launch alone between two device events, outputs
  preallocated; ``coef_kernel_ms`` the same with only beta / alpha / r2 / n wanted (no
  residual panel written);
* ``host_ms``: the lstsq loop (one ``np.linalg.lstsq`` per date on the rows where every X
  column is finite, all y columns as right-hand sides; y NaNs zeroed, so the host does a
  little LESS work than the kernel) over the first ``--host-dates`` dates, scaled to D.
One JSON line per case.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_inputs(D, A, K, Fy, dev, seed=7):
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    X = torch.randn((K, D, A), dtype=torch.float64, device=dev, generator=g)
    X[torch.rand((K, D, A), device=dev, generator=g) < 0.001] = float("nan")
    Y = 0.01 * X[:min(K, 3)].nan_to_num(0.0).sum(dim=0)[None] \
        + 0.01 * torch.randn((Fy, D, A), dtype=torch.float64, device=dev, generator=g)
    Y[torch.rand((Fy, D, A), device=dev, generator=g) < 0.03] = float("nan")
    return Y.contiguous(), X.contiguous()


def host_loop(Y, X, nd):
    """lstsq per date over the first nd dates; returns seconds."""
    Yh, Xh = Y[:, :nd].cpu().numpy(), X[:, :nd].cpu().numpy()
    t0 = time.perf_counter()
    for d in range(nd):
        ok = np.isfinite(Xh[:, d]).all(axis=0)
        Dm = np.concatenate([np.ones((int(ok.sum()), 1)), Xh[:, d][:, ok].T], axis=1)
        np.linalg.lstsq(Dm, np.nan_to_num(Yh[:, d][:, ok].T), rcond=None)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500x1000,2520x5000")
    ap.add_argument("--K", default="8,32")
    ap.add_argument("--Fy", default="1,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-dates", type=int, default=48)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_cs_ols.py needs a GPU")
    import factormodeling_amd.engine as E
    from factormodeling_amd._lib import call, ptr, stream_ptr
    dev = torch.device("cuda", 0)
    lines = []
    for size in args.sizes.split(","):
        D, A = (int(v) for v in size.split("x"))
        for K in (int(v) for v in args.K.split(",")):
            for Fy in (int(v) for v in args.Fy.split(",")):
                Y, X = make_inputs(D, A, K, Fy, dev)
                E.cs_ols(Y, X)
                calls = []
                for _ in range(args.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = E.cs_ols(Y, X)
                    torch.cuda.synchronize()
                    calls.append(time.perf_counter() - t0)

                def kernel(names):
                    ps = [ptr(out[k]) if k in names else None for k in E.CS_OLS_OUTPUTS]
                    ts = []
                    for _ in range(args.reps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        call("fmx_cs_ols", ptr(Y), ptr(X), None, None, Fy, K, D, A, A, 1, *ps, stream_ptr())
                        e1.record()
                        torch.cuda.synchronize()
                        ts.append(e0.elapsed_time(e1))
                    return float(np.median(ts))

                k_all = kernel(E.CS_OLS_OUTPUTS)
                k_coef = kernel(("beta", "alpha", "r2", "n"))
                nd = min(D, args.host_dates)
                host = host_loop(Y, X, nd) * D / nd
                res = dict(D=D, A=A, K=K, Fy=Fy, call_ms=1e3 * float(np.median(calls)), kernel_ms=k_all,
                           coef_kernel_ms=k_coef, host_ms=1e3 * host, host_dates=nd,
                           x_gbps=8.0 * K * D * A / (k_all * 1e-3) / 1e9, device=E.device_info())
                lines.append(json.dumps(res))
                print(lines[-1], flush=True)
                del Y, X, out
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
