"""Fundamental (Barra-style) factor risk model on the device (builder-defined):

    Sigma_t = B_t' F_t B_t + diag(s2_t)

* B_t, K x A: the factor panel itself on date t (exposures are known at t; a NaN exposure on a
  present symbol counts as 0, an absent symbol is outside Sigma);
* f, e: the pure factor returns and residuals of ONE ``engine.cs_ols`` call -- f is exactly what
  ``cross_sectional_factor_returns(factors_df, returns, lag, intercept, weights)`` returns; a
  row of f with any NaN is NaN in every column before the covariance, so all pairs share one
  set of weights and F is positive semidefinite by construction;
* F_t = ``f.shift(1).ewm(halflife=cov_halflife, min_periods=min_periods).cov()`` at t: one
  ``engine.ts_ewm`` covariance call on a broadcast K x D x K panel, bit for bit as pandas;
* s2 = ``ts_ewm_var(ts_delay(e, 1), halflife=spec_halflife, min_periods=min_periods)`` per
  symbol over its own rows; a present symbol without a finite value takes the date's LOWER
  median of the finite ones (``sorted[(n - 1) // 2]``: a data value, no arithmetic), then
  ``max(s2, spec_floor)``;
* a date is valid when F_t holds no NaN and some symbol has a finite s2; the risk outputs of
  an invalid date are NaN and its MVO book is the equal-weight book.

``FactorRiskModel.fit`` keeps the three device arrays (``B`` [K][D][A], ``Fc`` [D][K][K],
``S2`` [D][A]) and the ``panel_index``; ``portfolio_risk`` / ``risk_contributions`` /
``marginal_risk`` are one ``engine.risk_books`` pass, and ``simulation.risk_mvo_trade_list``
optimises ``Simulation(method="mvo")`` against the model (``engine.risk_mvo_books``);
``model.neutral_to(names)`` makes those books neutral to factors of the model.
"""
from __future__ import annotations

import copy

import numpy as np
import pandas as pd
import torch

from . import engine as E
from .operations import _ewm_com
from .panel import device, panel_index

RISK_FIELDS = ["total_var", "factor_var", "specific_var", "vol"]


def lower_median_fill(s2, present):
    """Per date (row) of the device panel ``s2`` [D][A]: a present cell that is not finite takes
    the lower median of the date's finite present cells.  Returns (filled, n_finite [D])."""
    pres = torch.ones_like(s2, dtype=torch.bool) if present is None else present != 0
    fin = pres & torch.isfinite(s2)
    n = fin.sum(dim=1)
    srt = torch.sort(torch.where(fin, s2, torch.full_like(s2, float("inf"))), dim=1).values
    med = srt.gather(1, ((n - 1).clamp(min=0) // 2)[:, None])[:, 0]
    fill = pres & ~fin & (n > 0)[:, None]
    out = torch.where(fill, med[:, None].expand_as(s2), s2)
    return torch.where(pres, out, torch.full_like(s2, float("nan"))), n


class FactorRiskModel:
    """The fitted model; build it with ``FactorRiskModel.fit``."""

    def __init__(self, pi, columns, B, Fc, S2, valid, factor_returns, index, residuals=None):
        self.residuals = residuals
        self.panel_index = pi
        self.columns = pd.Index(columns)
        self.B, self.Fc, self.S2 = B, Fc, S2
        self.valid_dev = valid
        self.index = index
        self.factor_returns = factor_returns
        dates = pd.Index(pi.dates, name="date")
        K = len(self.columns)
        self.factor_cov = pd.DataFrame(
            Fc.cpu().numpy().reshape(pi.D * K, K),
            index=pd.MultiIndex.from_product([dates, self.columns], names=["date", self.columns.name]),
            columns=self.columns)
        self.specific_var = pd.Series(pi.from_device(S2[None])[:, 0], index=index, name="specific_var")
        self.valid = pd.Series(valid.cpu().numpy().astype(bool), index=dates, name="valid")

    @property
    def K(self):
        return len(self.columns)

    neutral = ()        # the factors ``simulation.risk_mvo_trade_list`` holds its books neutral to

    def neutral_to(self, names):
        """A shallow view of the model (the same device arrays and frames, no copy) whose MVO
        books are neutral to the factors ``names`` of ``columns``."""
        names = (names,) if isinstance(names, str) else tuple(names)
        unknown = [n for n in names if n not in self.columns]
        if unknown:
            raise ValueError(f"neutral_to: {unknown} are not factors of the model ({list(self.columns)})")
        view = copy.copy(self)
        view.neutral = names
        return view

    @classmethod
    def fit(cls, factors_df: pd.DataFrame, returns: pd.Series, lag: int = 1, cov_halflife: float = 126,
            spec_halflife: float = 63, min_periods: int = 60, intercept: bool = True, weights=None,
            spec_floor: float = 1e-6):
        K = factors_df.shape[1]
        if not 1 <= K <= E.RISK_MAX_K:
            raise ValueError(f"FactorRiskModel.fit: {K} factor columns; the model takes 1..{E.RISK_MAX_K}")
        if int(min_periods) != min_periods or min_periods < 0:
            raise ValueError("min_periods must be an integer >= 0")
        pi = panel_index(factors_df.index)
        dev = device()
        present = pi.present(dev)
        D, A = pi.D, pi.A
        B = pi.to_device(factors_df.to_numpy(dtype=np.float64, na_value=np.nan), dev)
        # factor returns and residuals: one cs_ols call (factor_backtest.cross_sectional_factor_returns)
        X = E.ts("delay", B, int(lag), present)
        Y = pi.to_device(returns.reindex(factors_df.index).to_numpy(dtype=np.float64, na_value=np.nan), dev)
        Wt = None
        if weights is not None:
            Wt = pi.to_device(weights.reindex(factors_df.index).to_numpy(dtype=np.float64, na_value=np.nan), dev)[0]
        res = E.cs_ols(Y, X, Wt, present, intercept, want=("beta", "resid"))
        del X
        f = res["beta"][0]                                                   # [D][K]
        dates = pd.Index(pi.dates, name="date")
        factor_returns = pd.DataFrame(f.cpu().numpy(), index=dates, columns=factors_df.columns)
        # F[t]: ewm covariance of the rows strictly before t, a row with any NaN all NaN
        nan = torch.full_like(f, float("nan"))
        fs = torch.where(torch.isnan(f).any(dim=1, keepdim=True), nan, f)
        fs = torch.cat([nan[:1], fs[:-1]], dim=0).contiguous()               # shift(1)
        xp = fs.T.contiguous()[:, :, None].expand(K, D, K).contiguous()      # x[i][d][j] = fs[d][i]
        cov = E.ts_ewm(xp, {"cov": None}, _ewm_com(halflife=cov_halflife), True, False, int(min_periods), None,
                       y=fs)["cov"]                                          # cov[i][d][j], y[d][j] = fs[d][j]
        Fc = cov.permute(1, 0, 2).contiguous()
        del xp, cov
        # s2: per-symbol ewm variance of the lagged residual, lower-median fill, floor
        e_lag = E.ts("delay", res["resid"], 1, present)
        s2 = E.ts_ewm(e_lag, {"var": None}, _ewm_com(halflife=spec_halflife), True, False, int(min_periods),
                      present)["var"][0]
        s2, n_fin = lower_median_fill(s2, present)
        S2 = torch.clamp(s2, min=float(spec_floor)).contiguous()             # NaN stays NaN
        valid = (~torch.isnan(Fc).reshape(D, K * K).any(dim=1) & (n_fin > 0)).to(torch.uint8).contiguous()
        resid = pd.Series(pi.from_device(res["resid"])[:, 0], index=factors_df.index, name="resid")
        return cls(pi, factors_df.columns, B, Fc, S2, valid, factor_returns, factors_df.index, resid)

    # ------------------------------------------------------------------ books
    def _books(self, weights):
        """(W [M][D][A] on the model's grid, book names or None for a Series)."""
        if not isinstance(weights, (pd.Series, pd.DataFrame)):
            raise TypeError("weights must be a (date, symbol) Series or a DataFrame of books")
        if not weights.index.isin(self.index).all():
            raise ValueError("weights has (date, symbol) rows outside the model's index")
        w = weights.reindex(self.index)
        names = None if isinstance(w, pd.Series) else list(w.columns)
        return self.panel_index.to_device(w.to_numpy(dtype=np.float64, na_value=np.nan), self.B.device), names

    def _risk(self, weights, marginal=False):
        W, names = self._books(weights)
        out = E.risk_books(self.B, self.Fc, self.S2, W, self.panel_index.present(self.B.device), self.valid_dev,
                           marginal=marginal)
        return out, names

    @staticmethod
    def _by_book(frames, names):
        return frames[0] if names is None else pd.concat(dict(zip(names, frames)), axis=1)

    def portfolio_risk(self, weights):
        """Predicted ``total_var``, ``factor_var``, ``specific_var`` and ``vol`` = sqrt(total_var)
        per date; a DataFrame of books gives (book, field) columns."""
        out, names = self._risk(weights)
        var = out["var"].cpu().numpy()
        frames = [pd.DataFrame(np.column_stack([v, np.sqrt(v[:, 0])]), index=self.valid.index, columns=RISK_FIELDS)
                  for v in var]
        return self._by_book(frames, names)

    def risk_contributions(self, weights):
        """dates x (factors + "specific"): b_k (F b)_k per factor and the specific variance;
        the row sums to ``total_var``."""
        out, names = self._risk(weights)
        con, var = out["contrib"].cpu().numpy(), out["var"].cpu().numpy()
        cols = list(self.columns) + ["specific"]
        frames = [pd.DataFrame(np.column_stack([c, v[:, 2]]), index=self.valid.index, columns=cols)
                  for c, v in zip(con, var)]
        return self._by_book(frames, names)

    def factor_exposures(self, weights):
        """dates x factors: b = B w."""
        out, names = self._risk(weights)
        frames = [pd.DataFrame(b, index=self.valid.index, columns=self.columns) for b in out["expo"].cpu().numpy()]
        return self._by_book(frames, names)

    def marginal_risk(self, weights):
        """Sigma w per (date, symbol) row of the model's index (a Series, or one column per book)."""
        out, names = self._risk(weights, marginal=True)
        v = self.panel_index.from_device(out["marginal"])
        if names is None:
            return pd.Series(v[:, 0], index=self.index, name="marginal_risk")
        return pd.DataFrame(v, index=self.index, columns=names)

    def covariance(self, date, symbols=None) -> pd.DataFrame:
        """The dense Sigma of ``date`` over its present symbols (or ``symbols``, all of which must
        be present), on the host: for inspection and tests."""
        pi = self.panel_index
        d = int(pi.dates.get_indexer([pd.Timestamp(date) if isinstance(pi.dates, pd.DatetimeIndex) else date])[0])
        if d < 0:
            raise KeyError(f"{date!r} is not a date of the model")
        keep = np.ones(pi.A, dtype=bool) if pi.present_np is None else pi.present_np[d] != 0
        if symbols is not None:
            cols = pi.symbols.get_indexer(list(symbols))
            if (cols < 0).any() or not keep[cols].all():
                raise KeyError("symbols must all have a row on the date")
        else:
            cols = np.flatnonzero(keep)
        Bd = self.B[:, d, :].cpu().numpy()[:, cols]
        Bd = np.where(np.isfinite(Bd), Bd, 0.0)
        L = np.tril(self.Fc[d].cpu().numpy())
        F = L + np.tril(L, -1).T
        s2 = self.S2[d].cpu().numpy()[cols]
        fac = Bd.T @ F @ Bd
        sig = 0.5 * (fac + fac.T) + np.diag(s2)                              # symmetric in bits
        if not bool(self.valid.iloc[d]):
            sig = np.full_like(sig, np.nan)
        names = pi.symbols[cols]
        return pd.DataFrame(sig, index=names, columns=names)
