"""Golden vectors for multi_manager.compute_multimanager_weights with 'mvo' managers on the
ragged panel of tests/mm_mvo_cases.py (A = 24), by running the REFERENCE here (test
infrastructure only):

    python tests/golden/make_golden_mm_mvo_ragged.py      -> tests/golden/mm_mvo_ragged.npz

Like make_golden_mm_mvo.py: cvxpy is absent from this image, so it is stubbed and
``use_cvxpy=False`` runs the scipy SLSQP path.  Stored: the inputs (to detect a changed case
builder), each manager's book from the reference's ``compute_manager_weights`` (index, shifted
values, counts) and the combined ``final_weights`` / ``final_counts``.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from make_golden import OUT, import_reference  # noqa: E402

import mm_mvo_cases as MC  # noqa: E402


def main():
    warnings.filterwarnings("ignore")
    os.environ["TQDM_DISABLE"] = "1"
    import_reference()
    import multi_manager as mm
    from portfolio_simulation import SimulationSettings
    case = MC.ragged_case(24)
    dates, syms = case.fdates, pd.Index(case.syms)
    settings = SimulationSettings(**MC.settings_kw(case, "mvo", use_cvxpy=False))
    w, counts = mm.compute_multimanager_weights(case.factors_df, case.fw, settings)
    st = {"X": case.X, "R_v": case.returns.to_numpy(),
          "R_d": case.rdates.get_indexer(case.returns.index.get_level_values(0)).astype(np.int32),
          "R_s": syms.get_indexer(case.returns.index.get_level_values(1)).astype(np.int32),
          "fw": case.fw.to_numpy(), "fw_cols": np.array(list(case.fw.columns)),
          "fw_dates": dates.get_indexer(case.fw.index).astype(np.int32),
          "w_d": dates.get_indexer(w.index.get_level_values(0)).astype(np.int32),
          "w_s": syms.get_indexer(w.index.get_level_values(1)).astype(np.int32),
          "w_v": w.to_numpy(dtype=np.float64),
          "counts": counts[["long_count", "short_count"]].to_numpy(dtype=np.float64)}
    for fac in case.names:
        bw, bc = mm.compute_manager_weights(case.factors_df[fac].dropna(), settings, name=fac)
        st[f"book_{fac}__d"] = dates.get_indexer(bw.index.get_level_values(0)).astype(np.int32)
        st[f"book_{fac}__s"] = syms.get_indexer(bw.index.get_level_values(1)).astype(np.int32)
        st[f"book_{fac}__v"] = bw.to_numpy(dtype=np.float64)
        st[f"book_{fac}__cd"] = dates.get_indexer(bc.index).astype(np.int32)
        st[f"book_{fac}__c"] = bc[["long_count", "short_count"]].to_numpy(dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, "mm_mvo_ragged.npz"), **st)
    print("wrote mm_mvo_ragged.npz", len(w), "weights;", counts.shape)


if __name__ == "__main__":
    main()
