#!/usr/bin/env python3
"""Regenerate tests/golden/gn_restatement_sums.json: what the numpy restatements of the Gauss-Newton family (tests/track_ref.py, register_ref.py,
register_search_ref.py) return over the oracle's maps of tests/*_scenes.py.  The GPU tests compare the kernels with the restatements; this file pins the
restatements themselves, so that a change of both at once cannot go unnoticed (tests/test_gn_golden_cpu.py).  Integers as they are, float64 as hex.
The test calls compute() below, so the cases and the check are one piece of code: after an edit of compute(), record the file again at a commit whose
restatements are trusted (one the GPU tests passed against), never at the commit that rewrites them."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import register_ref as rr  # noqa: E402
import register_scenes as rs  # noqa: E402
import register_search_ref as sr  # noqa: E402
import register_search_scenes as ss  # noqa: E402
import track_ref as tr  # noqa: E402
import track_scenes as ts  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "gn_restatement_sums.json")
TRACK_HUBER, REGISTER_HUBER = 0.05, 0.02                 # below most residuals of the perturbed poses: the weight is not 1
SCORE_N_T, SCORE_N_R = (1, 0, 0), (0, 0, 2)             # 3 x 5 = 15 poses of the default steps around guess "B"


def _ints(a):
    return [int(v) for v in np.asarray(a).reshape(-1)]


def _run(R, T, info):
    return dict(R=[float(v).hex() for v in np.asarray(R).reshape(-1)], T=[float(v).hex() for v in np.asarray(T).reshape(-1)], status=int(info["status"]),
                iterations=int(info["iterations"]))


def compute():
    out = {}
    _, _, depth = ts.tracked_frame()
    K, grid = ts.intrinsics(), ts.oracle_grid()
    for n, (R, T) in enumerate(ts.perturbed_poses()):
        for stride in (8, 1):
            out[f"track/{n}/stride{stride}"] = _ints(tr.linearize(depth, R, T, K, stride, ts.VS, grid, **ts.GATES))
    R, T = ts.perturbed_poses()[1]
    out["track/1/stride8/huber"] = _ints(tr.linearize(depth, R, T, K, 8, ts.VS, grid, huber=TRACK_HUBER, **ts.GATES))
    out["track/2/run"] = _run(*ts.reference_tracks()[2])

    src, dst = rs.src_voxels(), rs.dst_grid()
    for n, (R, T) in enumerate(rs.perturbed_poses()):
        for stride in (4, 1):
            out[f"register/{n}/stride{stride}"] = _ints(rr.linearize(src, R, T, stride, rs.VS, dst, **rs.GATES))
    R, T = rs.perturbed_poses()[1]
    out["register/1/stride4/huber"] = _ints(rr.linearize(src, R, T, 4, rs.VS, dst, **dict(rs.GATES, huber=REGISTER_HUBER)))
    out["register/outside/stride4"] = _ints(rr.linearize(src, *rs.outside_pose(), 4, rs.VS, dst, **rs.GATES))
    out["register/2/run"] = _run(*rs.reference_runs()[2])

    R0, T0 = ss.guess("B")
    pivot, _ = sr.auto_pivot(src, R0, T0, ss.STRIDE, ss.VOXEL, **rs.GATES)
    Rs, Ts = sr.candidates(R0, T0, pivot, SCORE_N_T, ss.STEPS_T, SCORE_N_R, ss.STEPS_R)
    for name, gates in (("score", rs.GATES), ("score/huber", dict(rs.GATES, huber=REGISTER_HUBER))):
        sc = sr.score(src, Rs, Ts, ss.STRIDE, rs.VS, dst, **gates)
        out[name] = {f: _ints(sc[f]) for f in sr.FIELDS}
    return out


if __name__ == "__main__":
    with open(PATH, "w") as f:                           # one case per line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in sorted(compute().items())) + "\n}\n")
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
