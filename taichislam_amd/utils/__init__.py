from .nav import frontier_reach, inflation_lut, terrain_slope2, terrain_slope_deg  # noqa: F401
from .nav import corridor_metres, distance_cost, flight_lut, frontier_reach3d  # noqa: F401
from .nav import bspline_basis, bspline_from_path, bspline_points  # noqa: F401
from .depth import bilateral_tables, depth_tolerance, halved_intrinsics  # noqa: F401
from .pose import pose_information  # noqa: F401
