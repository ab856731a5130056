"""Fallback cost of the lazy Gram at full C2 size (development tool).

    python tools/lazy_gram_fallback.py

32 factors are near-copies of three signals that drive the next day's returns, so they lead
the prune order, the 32-row head keeps 3 of 5 and the step runs the full Gram too.  Prints
ms/step and stage times for lazy_gram on and off (3 steps each, twice, alternating) and checks
that kept and the weights agree."""
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from factormodeling_amd import pipeline as PL  # noqa: E402

D, A, F = 2520, 5000, 200
dev = torch.device("cuda", 0)
cfg0 = PL.StepConfig()
sp = PL.ShardedPanel(D, A, F, 0, 1, dev, seed=0, halo=cfg0.halo)
g = torch.Generator(device=dev)
g.manual_seed(99)
S = torch.randn((3, D, A), generator=g, dtype=torch.float64, device=dev)
for f in range(32):
    sp.X[f + 8] = S[f % 3] + 0.05 * sp.X[f + 8]
sp.R[1:] += 0.01 * S.sum(dim=0)[:-1] / math.sqrt(3.0)
del S
torch.cuda.synchronize()
out = {}
for name, lazy in (("lazy_on", True), ("lazy_off", False), ("lazy_on2", True), ("lazy_off2", False)):
    cfg = PL.StepConfig(lazy_gram=lazy)
    PL.run_step(sp, cfg)
    torch.cuda.synchronize()
    timers = []
    t0 = time.perf_counter()
    for _ in range(3):
        w, kept = PL.run_step(sp, cfg, timers=timers)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / 3 * 1e3
    st = {k: round(v / 3, 3) for k, v in PL.stage_times(timers).items()}
    out[name] = {"ms_per_step": round(ms, 3), "kept": kept, "stages_ms": st, "w_sum": float(w.nan_to_num().sum())}
    print(name, json.dumps(out[name]), flush=True)
assert "gram" in out["lazy_on"]["stages_ms"] and "gram_head" in out["lazy_on"]["stages_ms"]
assert out["lazy_on"]["kept"] == out["lazy_off"]["kept"]
assert out["lazy_on"]["w_sum"] == out["lazy_off"]["w_sum"]
print("FALLBACK_OK")
