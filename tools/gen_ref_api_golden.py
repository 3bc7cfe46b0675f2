"""Dev-box tool: record what the REFERENCE's own API-level code produces, for the tests that compare the package against it without the
reference tree being present:
  * tests/golden/ref_callers_scenario.json -- taichi_slam/mapping/submap_mapping.py (loaded by path, unmodified) driven through
    tests/test_reference_callers.py:_scenario on the recording stand-ins, for both map kinds;
  * tests/golden/pointcloud2_ref.npz -- taichi_slam/utils/ros_pcl_transfer.py:point_cloud on the seeded points of tests/test_ros_payload_ref.py;
  * tests/golden/ref_node_map_names.json -- the names scripts/taichislam_node.py uses on the map, the mesher and the orchestration.
    python tools/gen_ref_api_golden.py REFERENCE_ROOT"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_reference_callers as trc      # noqa: E402
import test_ros_payload_ref as trp        # noqa: E402

if __name__ == "__main__":
    ref = sys.argv[1]
    gold = os.path.join(ROOT, "tests", "golden")
    trc.REF = os.path.join(ref, "taichi_slam", "mapping", "submap_mapping.py")
    json.dump({kind: trc.reference_scenario(kind) for kind in ("tsdf", "octo")}, open(os.path.join(gold, "ref_callers_scenario.json"), "w"))
    helper = trp._load_reference_helper(os.path.join(ref, "taichi_slam", "utils", "ros_pcl_transfer.py"))
    out = {}
    for has_rgb in (False, True):
        for k, v in trp.reference_payload(helper, has_rgb).items():
            out[("rgb_" if has_rgb else "xyz_") + k] = v
    np.savez_compressed(os.path.join(gold, "pointcloud2_ref.npz"), **out)
    names = trp.node_map_names(open(os.path.join(ref, "scripts", "taichislam_node.py")).read())
    json.dump(names, open(os.path.join(gold, "ref_node_map_names.json"), "w"), indent=0)
    print(f"{len(names)} node names; " + ", ".join(f"{f}: {os.path.getsize(os.path.join(gold, f))} B"
                                                   for f in ("ref_callers_scenario.json", "pointcloud2_ref.npz", "ref_node_map_names.json")))
