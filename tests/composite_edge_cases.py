"""Shared inputs of the composite edge tests (tests/test_composite_edges.py on the host,
tests/test_gpu_composite.py on the device): the panels of ``golden/composite_edges.npz`` and
the single rows that drive the block radix select of ``csrc/composite.hip``."""
from __future__ import annotations

import functools

import numpy as np
import pandas as pd

import oracle.numerics as nm
from golden_io import load

SUFFIXES = ["_eq", "_flx", "_long", "_short"]            # suffix codes 1..4
PCT = {1: (10, 90), 2: (2, 98), 3: (2, 98), 4: (2, 98)}  # composite_factor.py:158-163
CASES = [f"{fn}_{meth}" for fn in ("cfc_all", "cfc_sub", "wcf") for meth in ("zscore", "rank")]


@functools.lru_cache(maxsize=None)
def panels():
    """The fixture's panels, in file order: dicts with ``A``, ``ragged``, ``names``, ``sub``
    (the 8-factor subset), ``X[F][D][A]`` (NaN where absent), ``present[D][A]`` (bool),
    ``P`` (``present``, or None on a dense panel), ``W[J][F]``, ``sd`` (panel date index of
    every selection row, -1 = not a panel date), ``dates``, ``sel_dates`` and ``out[case]``
    (the reference's dense [D][A] outputs)."""
    st = load("composite_edges.npz")
    names = [str(n) for n in st["names"]]
    dates = [str(d) for d in st["dates"]]
    sd = [dates.index(str(d)) if str(d) in dates else -1 for d in st["sel_dates"]]
    out = []
    for A in st["panels"]:
        k = f"A{int(A)}"
        present = st[f"{k}_present"].astype(bool)
        out.append({"A": int(A), "ragged": not present.all(), "names": names,
                    "sub": [names[i] for i in st["sub_idx"]],
                    "X": np.ascontiguousarray(np.moveaxis(st[f"{k}_X"], 2, 0)), "present": present,
                    "P": None if present.all() else present, "W": st[f"{k}_sel_W"], "sd": sd,
                    "dates": dates, "sel_dates": [str(d) for d in st["sel_dates"]],
                    "out": {c: st[f"{k}_out_{c}"] for c in CASES}})
    for p in out:                                     # shared by every test: read-only
        for a in [p["X"], p["present"], p["W"], *p["out"].values()]:
            a.setflags(write=False)
    return out


def panel_ids():
    return [f"A{p['A']}{'r' if p['ragged'] else ''}" for p in panels()]


def frames(p):
    """The long (date, symbol) factor frame of a panel (present rows only), its selection
    frame and the (date, symbol) positions of the frame's rows."""
    dates = pd.to_datetime(p["dates"])
    syms = [f"E{i:03d}" for i in range(p["A"])]
    di, si = np.nonzero(p["present"])
    idx = pd.MultiIndex.from_arrays([dates[di], [syms[k] for k in si]], names=["date", "symbol"])
    df = pd.DataFrame(np.ascontiguousarray(p["X"][:, di, si].T), index=idx, columns=p["names"])
    seldf = pd.DataFrame(p["W"], index=pd.DatetimeIndex(pd.to_datetime(p["sel_dates"]), name="date"),
                         columns=p["names"])
    return df, seldf, di, si


def percentiles(values, code):
    """(lo, hi, nv) of suffix ``code`` over the non-NaN ``values`` (numpy 'linear')."""
    v = np.asarray(values, dtype=np.float64).ravel()
    s = np.sort(v[~np.isnan(v)])
    if s.size == 0:
        return np.nan, np.nan, 0
    ql, qh = (np.true_divide(np.asarray([q], dtype=np.float64), 100)[0] for q in PCT[code])
    return nm.percentile_linear(s, ql), nm.percentile_linear(s, qh), s.size


@functools.lru_cache(maxsize=None)
def select_rows():
    """(label, row) pairs for the radix select.  ``nv`` = 1, 2, 3, 11, 51, 101 put
    (nv - 1) q on an integer for 10 % / 90 % or 2 % / 98 % (interpolation weight 0);
    255 / 256 / 257 / 1000 sit around the 256-thread block; the rest pin one digit pass."""
    rng = np.random.default_rng(2024)
    rows = []
    for nv in (1, 2, 3, 11, 51, 101, 255, 256, 257, 1000):
        rows.append((f"nv{nv}", rng.standard_normal(nv)))
    for nv, A in ((3, 9), (101, 130), (257, 300)):           # the same counts between NaNs
        x = np.full(A, np.nan)
        x[rng.permutation(A)[:nv]] = np.round(rng.standard_normal(nv), 1)
        rows.append((f"nv{nv}_of{A}", x))
    rows.append(("all_equal", np.full(77, 3.25)))
    rows.append(("low_byte", 1.0 + rng.permutation(256) * 2.0 ** -52))
    top = np.array([-1e300, -1.0, -1e-300, -5e-324, -0.0, 0.0, 5e-324, 1e-310, 1e-300, 1.0, 1e300])
    rows.append(("top_byte", top[rng.permutation(top.size)]))
    rows.append(("top_byte_x7", np.repeat(top, 7)[rng.permutation(7 * top.size)]))
    x = rng.standard_normal(300)
    x[17], x[203] = np.inf, -np.inf
    rows.append(("infs", x))
    rows.append(("two_values", np.repeat([1.0, 2.0], 50)[rng.permutation(100)]))
    return rows


def pooled_rows():
    """(label, X[3][1][A]) for the pooled percentiles: three columns of one suffix, the
    middle one all NaN, so n = 3 A crosses column boundaries inside a thread's stride."""
    rng = np.random.default_rng(2025)
    out = []
    for A in (65, 257):
        X = np.round(rng.standard_normal((3, 1, A)) * 4) / 4
        X[1] = np.nan
        X[2, 0, rng.random(A) < 0.1] = np.nan
        out.append((f"A{A}", X))
    return out
