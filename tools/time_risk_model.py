#!/usr/bin/env python
"""Times of the factor risk model's two kernels on synthetic panels.

    python tools/time_risk_model.py [--risk 2520x5000] [--mvo 500x1000,2520x5000] [--K 8,32] [--neutral 1,8,K]
                                      [--out FILE]

* ``risk_books`` (fmx_risk_books) at ``--risk`` with K = 32 and M = 1 / 32 books: ms between two
  device events (a warm-up, then the median of ``--reps`` runs) and the bytes it must read
  (B once, W, S2, Fc) per second as a fraction of the device's copy rate (a ``copy_`` of the
  exposure panel, bytes read + written per second, timed the same way);
* ``risk_mvo_books`` (fmx_risk_mvo_books) at every ``--mvo`` size and K: ms, mean / max ADMM
  iterations and the iteration histogram; ``sim_mvo_books`` (fmx_sim_mvo_books, a 60-row
  returns window, shrinkage 0.1) on the same signal panel in the same process -- the only
  meaningful comparison: the same QP under the other covariance;
* with ``--neutral 1,8,K`` the same books neutral to the first n factors
  (fmx_risk_mvo_neutral_books): ms, iterations, statuses and ms per mean iteration
  beside the un-neutral call's at the same shape in the same process.
Signals N(0, 1), exposures N(0, 1) with 0.1 % NaN, Fc = Q Q' 1e-4, s2 = (0.01 U(0.3, 2))^2,
box 0.03.  One JSON line per case.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HIST_EDGES = [0, 1, 100, 200, 400, 800, 1600, 3200, 6400, 12800, 20000]


def _events(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), out


def make_model(torch, D, A, K, dev, seed=3):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    B = torch.randn((K, D, A), dtype=torch.float64, device=dev, generator=g)
    B[torch.rand((K, D, A), device=dev, generator=g) < 0.001] = float("nan")
    Q = torch.randn((D, K, K), dtype=torch.float64, device=dev, generator=g)
    Fc = (1e-4 * Q @ Q.transpose(1, 2)).contiguous()
    S2 = ((0.01 * (0.3 + 1.7 * torch.rand((D, A), dtype=torch.float64, device=dev, generator=g))) ** 2).contiguous()
    return B.contiguous(), Fc, S2


def _iters(info):
    it = info[:, 1].cpu().numpy()
    st = info[:, 0].cpu().numpy()
    hist, _ = np.histogram(it, bins=HIST_EDGES)
    return dict(iters_mean=float(it.mean()), iters_max=int(it.max()), iters_hist=[int(v) for v in hist],
                status_counts={str(int(k)): int((st == k).sum()) for k in np.unique(st)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--risk", default="2520x5000")
    ap.add_argument("--mvo", default="500x1000,2520x5000")
    ap.add_argument("--K", default="8,32")
    ap.add_argument("--neutral", default="", help="numbers of neutral factors (the first n; 'K' = all), e.g. 0,1,8,K")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_risk_model.py needs a GPU")
    import factormodeling_amd.engine as E
    dev = torch.device("cuda", 0)
    lines = []

    def emit(res):
        res["device"] = E.device_info()
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)

    for size in [s for s in args.risk.split(",") if s]:
        D, A = (int(v) for v in size.split("x"))
        K = 32
        B, Fc, S2 = make_model(torch, D, A, K, dev)
        dst = torch.empty_like(B)
        copy_ms, _ = _events(torch, lambda: dst.copy_(B), args.reps)
        copy_gbps = 2.0 * B.numel() * 8 / (copy_ms * 1e-3) / 1e9
        del dst
        for M in (1, 32):
            W = torch.randn((M, D, A), dtype=torch.float64, device=dev) / A
            ms, _ = _events(torch, lambda: E.risk_books(B, Fc, S2, W), args.reps)
            ms_marg, _ = _events(torch, lambda: E.risk_books(B, Fc, S2, W, marginal=True), args.reps)
            nbytes = 8.0 * (B.numel() + W.numel() + S2.numel() + Fc.numel())
            emit(dict(op="risk_books", D=D, A=A, K=K, M=M, ms=ms, ms_with_marginal=ms_marg, read_gb=nbytes / 1e9,
                      read_gbps=nbytes / (ms * 1e-3) / 1e9, copy_gbps=copy_gbps,
                      fraction_of_copy_rate=nbytes / (ms * 1e-3) / 1e9 / copy_gbps))
            del W
        del B, Fc, S2
    for size in [s for s in args.mvo.split(",") if s]:
        D, A = (int(v) for v in size.split("x"))
        g = torch.Generator(device=dev)
        g.manual_seed(11)
        X = torch.randn((D, A), dtype=torch.float64, device=dev, generator=g)
        scale = 0.3 + 1.7 * torch.rand((1, A), dtype=torch.float64, device=dev, generator=g)
        R0 = 0.01 * (0.6 * torch.randn((D, 1), dtype=torch.float64, device=dev, generator=g)
                     + torch.randn((D, A), dtype=torch.float64, device=dev, generator=g) * scale)
        L = 60
        win_T = np.minimum(np.arange(D), L).astype(np.int32)
        rows = np.zeros((D, L), dtype=np.int32)
        for j in range(D):
            rows[j, :win_T[j]] = np.arange(j - win_T[j], j)
        ms0, out0 = _events(torch, lambda: E.sim_mvo_books(R0, rows, win_T, X, None, 0.1, 0.03), args.reps)
        emit(dict(op="sim_mvo_books", D=D, A=A, window=L, ms=ms0, **_iters(out0[2])))
        for K in (int(v) for v in args.K.split(",")):
            B, Fc, S2 = make_model(torch, D, A, K, dev)
            ms, out = _events(torch, lambda: E.risk_mvo_books(B, Fc, S2, X, None, None, 0.03), args.reps)
            emit(dict(op="risk_mvo_books", D=D, A=A, K=K, ms=ms, sim_mvo_books_ms=ms0, **_iters(out[2])))
            base = ms / (float(out[2][:, 1].sum()) / D)                    # ms per mean iteration, the comparator
            for n in sorted({min(int(v) if v != "K" else K, K) for v in args.neutral.split(",") if v}):
                if n == 0:
                    continue                                               # the empty mask is the call above
                msn, outn = _events(torch, lambda: E.risk_mvo_books(B, Fc, S2, X, None, None, 0.03, neutral=range(n),
                                                                    return_expo=True), args.reps)
                it = _iters(outn[2])
                emit(dict(op="risk_mvo_books_neutral", D=D, A=A, K=K, neutral=n, ms=msn, un_neutral_ms=ms,
                          ms_per_mean_iter=msn / it["iters_mean"], un_neutral_ms_per_mean_iter=base, **it))
            del B, Fc, S2
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
