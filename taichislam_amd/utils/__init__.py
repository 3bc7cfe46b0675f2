from .nav import frontier_reach, inflation_lut, terrain_slope2, terrain_slope_deg  # noqa: F401
