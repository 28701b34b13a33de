"""The algorithms, one module each (``oprl_amd.algos.ddpg`` ...).  ``D4PG``, ``TD3BC``, ``IQL``, ``CQL`` and ``CalQL`` are also served
from here, resolved on first use so that importing the package stays free of torch."""


def __getattr__(name: str):
    if name == "D4PG":
        from oprl_amd.algos.d4pg import D4PG
        return D4PG
    if name == "TD3BC":
        from oprl_amd.algos.td3_bc import TD3BC
        return TD3BC
    if name == "IQL":
        from oprl_amd.algos.iql import IQL
        return IQL
    if name == "CQL":
        from oprl_amd.algos.cql import CQL
        return CQL
    if name == "CalQL":
        from oprl_amd.algos.calql import CalQL
        return CalQL
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
