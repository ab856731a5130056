"""Drop-in ``portfolio_analyzer`` module."""
from factormodeling_amd.portfolio_analyzer import PortfolioAnalyzer  # noqa: F401
from factormodeling_amd.portfolio_analyzer import (performance_curves, performance_table, period_returns,  # noqa: F401
                                                   rolling_sharpe)
