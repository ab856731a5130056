#!/usr/bin/env python
"""Time of the rolling multi-factor OLS (engine.ts_ols / fmx_ts_ols) on synthetic panels,
against a per-window ``np.linalg.lstsq`` loop on the host and, at K = 1, against the
one-regressor kernel ``fmx_ts_regression`` on the same panel in the same run.

    python tools/time_ts_ols.py [--sizes 500x1000,2520x5000] [--K 1,3,8] [--windows 20,60]
                                [--Fy 1,20] [--out FILE]

Per (D x A, K, W, Fy, shared or panel X): N(0, 1) regressors with 0.1 % NaN cells (table rows
for a shared X), y = 0.01 (sum of the first three columns) + noise with 3 % NaN cells, an
intercept, all six outputs.

* ``kernel_ms``: the ``fmx_ts_ols`` call (validity pre-kernel + fit kernel) between two device
  events, outputs preallocated, median of ``--reps`` launches after a warm-up;
* ``call_ms``: wall clock of ``engine.ts_ols`` around a device synchronise (launch plus the
  allocation of the outputs), median of ``--reps``;
* ``host_ms``: one lstsq per window over ``--host-cols`` columns of the first y column, scaled
  to Fy * A columns;
* ``ts_regression_ms`` (K = 1): one ``fmx_ts_regression`` call -- ONE output of one y column --
  between events, and ``ts_regression_all_ms`` that time x 5 outputs x Fy, what the same
  results would cost through it (it has no sigma);
* ``read_bytes_per_output``: what a thread reads by the kernel's structure -- three passes over
  W rows of (K per-symbol regressors +) y and a validity byte, plus the walk; a shared table
  goes through the scalar unit and is not counted -- and ``implied_read_tbps``, that traffic
  over the kernel time (cache traffic: the panel itself is read from HBM about once).
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
    """(Y [Fy][D][A], X panel [K][D][A], X table [K][D])."""
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    X = torch.randn((K, D, A), dtype=torch.float64, device=dev, generator=g)
    T = torch.randn((K, D), dtype=torch.float64, device=dev, generator=g)
    sig = 0.01 * X[:min(K, 3)].sum(dim=0)[None]
    Y = sig + 0.01 * torch.randn((Fy, D, A), dtype=torch.float64, device=dev, generator=g)
    Y[torch.rand((Fy, D, A), device=dev, generator=g) < 0.03] = float("nan")
    X[torch.rand((K, D, A), device=dev, generator=g) < 0.001] = float("nan")
    T[torch.rand((K, D), device=dev, generator=g) < 0.001] = float("nan")
    return Y.contiguous(), X.contiguous(), T.contiguous()


def host_loop(y, X, W):
    """lstsq per window of every column of y [D][c] on X [K][D][c] (or [K][D]); seconds."""
    D, c = y.shape
    t0 = time.perf_counter()
    for a in range(c):
        Xa = (X if X.ndim == 2 else X[:, :, a]).T
        rows = np.flatnonzero(np.isfinite(y[:, a]) & np.isfinite(Xa).all(axis=1))
        Dm = np.concatenate([np.ones((rows.size, 1)), Xa[rows]], axis=1)
        ya = y[rows, a]
        for i in range(W - 1, rows.size):
            np.linalg.lstsq(Dm[i - W + 1:i + 1], ya[i - W + 1:i + 1], rcond=None)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500x1000,2520x5000")
    ap.add_argument("--K", default="1,3,8")
    ap.add_argument("--windows", default="20,60")
    ap.add_argument("--Fy", default="1,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-cols", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_ts_ols.py needs a GPU")
    import factormodeling_amd.engine as E
    from factormodeling_amd._lib import call, ptr, stream_ptr
    dev = torch.device("cuda", 0)
    info = E.device_info()
    lines = []

    def events(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    for size in args.sizes.split(","):
        D, A = (int(v) for v in size.split("x"))
        for K in (int(v) for v in args.K.split(",")):
            for Fy in (int(v) for v in args.Fy.split(",")):
                Y, Xp, Xt = make_inputs(D, A, K, Fy, dev)
                nc = min(A, args.host_cols)
                yh, xph, xth = Y[0, :, :nc].cpu().numpy(), Xp[:, :, :nc].cpu().numpy(), Xt.cpu().numpy()
                for W in (int(v) for v in args.windows.split(",")):
                    for shared in (True, False):
                        X = Xt if shared else Xp
                        out = E.ts_ols(Y, X, W, shared=shared)
                        work = torch.empty((Fy, D, A), dtype=torch.uint8, device=dev)
                        calls = []
                        for _ in range(args.reps):
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            res = E.ts_ols(Y, X, W, shared=shared)
                            torch.cuda.synchronize()
                            calls.append(time.perf_counter() - t0)
                            del res
                        ps = [ptr(out[k]) for k in E.TS_OLS_OUTPUTS]
                        k_ms = events(lambda: call("fmx_ts_ols", ptr(Y), ptr(X), None, Fy, K, D, A, A, W, 1, int(shared),
                                                   *ps, ptr(work), stream_ptr()))
                        nout = int(torch.isfinite(out["resid"]).sum())
                        host = host_loop(yh, xth if shared else xph, W) * Fy * A / nc
                        per = 3 * W * (8 * ((0 if shared else K) + 1) + 1) + W
                        res = dict(D=D, A=A, K=K, W=W, Fy=Fy, shared=shared, kernel_ms=k_ms,
                                   call_ms=1e3 * float(np.median(calls)), host_ms=1e3 * host, host_cols=nc,
                                   outputs=nout, ns_per_output=1e6 * k_ms / max(nout, 1), read_bytes_per_output=per,
                                   implied_read_tbps=per * Fy * D * A / (k_ms * 1e-3) / 1e12, device=info)
                        if K == 1 and not shared:
                            valid = (torch.isfinite(Y[0]) & torch.isfinite(Xp[0])).to(torch.uint8)
                            o1 = torch.empty_like(Y[0])
                            r_ms = events(lambda: call("fmx_ts_regression", ptr(Y[0]), ptr(Xp[0]), ptr(valid), ptr(o1), D, A,
                                                       A, W, 0, stream_ptr()))
                            res.update(ts_regression_ms=r_ms, ts_regression_all_ms=r_ms * 5 * Fy)
                        lines.append(json.dumps(res))
                        print(lines[-1], flush=True)
                        del out, work
                del Y, Xp, Xt
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
