"""Drop-in ``portfolio_simulation`` module."""
from factormodeling_amd.portfolio_simulation import Simulation, SimulationSettings  # noqa: F401
from factormodeling_amd.portfolio_simulation import single_factor_backtests, single_factor_returns  # noqa: F401
