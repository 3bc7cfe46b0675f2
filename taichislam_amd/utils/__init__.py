from .nav import frontier_reach, inflation_lut  # noqa: F401
