"""taichislam_amd.mapping -- drop-in for taichi_slam.mapping (reference taichi_slam/mapping/__init__.py:1-6)."""
from .mapping_common import BaseMap  # noqa: F401
from .dense_tsdf import DenseTSDF, brick_key_ijk, depth_to_mm, frontier_view_candidates, metric_box_to_voxels  # noqa: F401
from .taichi_octomap import Octomap  # noqa: F401
from .marching_cube_mesher import MarchingCubeMesher  # noqa: F401
from .submap_mapping import SubmapMapping  # noqa: F401
from .topo_graph import TopoGraphGen  # noqa: F401
from .depth_conditioner import DepthConditioner  # noqa: F401
from .pose_graph import PoseGraph  # noqa: F401
