"""The PointCloud2 payload (taichislam_amd.utils.ros_adapters, csrc k_pack_pointcloud2) against the reference's own helper,
taichi_slam/utils/ros_pcl_transfer.py:point_cloud, and the names the reference node uses on the maps against the shims.  What the reference
produced is recorded in tests/golden/pointcloud2_ref.npz and tests/golden/ref_node_map_names.json by tools/gen_ref_api_golden.py, which imports
the helper unmodified with the ROS message classes it needs (rospy / sensor_msgs / std_msgs / geometry_msgs / ros_numpy) replaced by plain records."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class _Rec:
    def __init__(self, *a, **kw):
        self.__dict__.update(kw)


def _load_reference_helper(path):
    """ros_pcl_transfer.py of a reference tree, loaded by path (tools/gen_ref_api_golden.py)"""
    mods = {}
    for name in ("ros_numpy", "rospy", "sensor_msgs", "sensor_msgs.msg", "geometry_msgs", "geometry_msgs.msg", "std_msgs", "std_msgs.msg"):
        mods[name] = types.ModuleType(name)
    mods["sensor_msgs.msg"].PointField = type("PointField", (_Rec,), {"FLOAT32": 7})
    mods["sensor_msgs.msg"].PointCloud2 = type("PointCloud2", (_Rec,), {})
    mods["sensor_msgs.msg"].PointCloud = type("PointCloud", (_Rec,), {})
    mods["geometry_msgs.msg"].Point32 = type("Point32", (_Rec,), {})
    mods["geometry_msgs.msg"].PoseStamped = type("PoseStamped", (_Rec,), {})
    mods["std_msgs.msg"].Header = type("Header", (_Rec,), {})
    mods["rospy"].Time = type("Time", (), {"now": staticmethod(lambda: 0)})
    mods["sensor_msgs"].msg, mods["geometry_msgs"].msg, mods["std_msgs"].msg = mods["sensor_msgs.msg"], mods["geometry_msgs.msg"], mods["std_msgs.msg"]
    saved = {k: sys.modules.get(k) for k in mods}
    sys.modules.update(mods)
    try:
        spec = importlib.util.spec_from_file_location("ref_ros_pcl_transfer", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def payload_inputs(has_rgb):
    rng = np.random.default_rng(1)
    xyz = rng.normal(size=(257, 3)).astype(np.float32)
    rgb = rng.uniform(size=(257, 3)).astype(np.float32)
    return xyz, rgb


def reference_payload(ref, has_rgb):
    """The reference helper's message for the seeded points, as recorded in tests/golden/pointcloud2_ref.npz"""
    xyz, rgb = payload_inputs(has_rgb)
    # scripts/taichislam_node.py:420-425 (pub_to_ros): xyz | colours as float, or xyz alone
    pts = np.concatenate((xyz, rgb.astype(float)), axis=1) if has_rgb else xyz
    msg = ref.point_cloud(pts, "world", has_rgb=has_rgb)
    return {"header": np.array([msg.height, msg.width, msg.is_dense, msg.is_bigendian, msg.point_step, msg.row_step], np.int64),
            "fields": json.dumps([[f.name, f.offset, f.datatype, f.count] for f in msg.fields]), "data": np.frombuffer(bytes(msg.data), np.uint8)}


def node_map_names(src):
    """The attributes / methods scripts/taichislam_node.py uses on the map, the mesher and the submap orchestration"""
    import re
    return sorted(set(re.findall(r"(?:self\.mapping|mapping|self\.mesher|mesher)\.([A-Za-z_][A-Za-z0-9_]*)", src)))


@pytest.mark.parametrize("has_rgb", [False, True])
def test_pointcloud2_payload_equals_the_reference_helper(has_rgb):
    from taichislam_amd.utils import ros_adapters
    z = np.load(os.path.join(GOLD, "pointcloud2_ref.npz"))
    tag = "rgb" if has_rgb else "xyz"
    header, fields, data = z[f"{tag}_header"], json.loads(str(z[f"{tag}_fields"])), z[f"{tag}_data"].tobytes()
    xyz, rgb = payload_inputs(has_rgb)
    mine = ros_adapters.pointcloud2_payload(np.concatenate([xyz, rgb], axis=1) if has_rgb else xyz, has_rgb)
    assert tuple(int(v) for v in header) == \
        (mine["height"], mine["width"], mine["is_dense"], mine["is_bigendian"], mine["point_step"], mine["row_step"])
    assert [tuple(f) for f in fields] == [(f["name"], f["offset"], f["datatype"], f["count"]) for f in mine["fields"]]
    assert len(data) == header[5] * header[0] > 0
    assert data == mine["data"]


def test_every_name_the_reference_node_uses_on_the_maps_exists_in_the_shims():
    """scripts/taichislam_node.py drives the map, the mesher and the submap orchestration through these attributes / methods; a drop-in must have them all."""
    import re
    used = set(json.load(open(os.path.join(GOLD, "ref_node_map_names.json"))))
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "taichislam_amd", "mapping")
    mine = "".join(open(os.path.join(root, f)).read() for f in os.listdir(root) if f.endswith(".py"))
    missing = [n for n in sorted(used) if not re.search(r"\b" + re.escape(n) + r"\b", mine)]
    assert len(used) >= 20 and not missing, missing
