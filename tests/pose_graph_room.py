"""The end-to-end scene of the pose graph: three overlapping submaps of the box room of tests/track_scenes.py at SMALL.  Submap 0 holds frames 0..5 (the
destination of tests/register_scenes.py), submap 1 its source (frames 3..8, grid displaced by D), submap 2 frames 1..6 with a grid displaced by D2.  All
three are integrated at the identity, so the true base poses are I, D and D2.  The pose table starts with D and D2 moved by the first of PERTURBATIONS;
the three pairs are registered from it, and the graph of the three constraints and two (loose: the submaps were all opened at the identity) odometry
edges is solved.  chain() runs that over the oracle's maps with the restatements (a few seconds: tests/test_pose_graph_cpu.py runs it and holds it to the
figures recorded here, tests/test_pose_graph_submaps_gpu.py takes its bound from them)."""
import functools

import numpy as np

import register_ref as rr
import register_scenes as rs
import render_view_scenes as rsc
import track_scenes as ts
from util import SMALL

# The largest error of the three base poses at the end of chain(), as tests/test_pose_graph_cpu.py::test_room_chain measures it: status 0 after 10
# iterations, every registration status 0.  The bound of the GPU run is twice that, as REGISTER_BOUND_M is made.
MEASURED_M, MEASURED_DEG = 0.000573, 0.009888
ROOM_BOUND_M, ROOM_BOUND_DEG = 2 * MEASURED_M, 2 * MEASURED_DEG
FRAMES = (0, 6, 12)                                             # the frame ids that open the three submaps
PAIRS = ((6, 0), (12, 0), (12, 6))                              # (frame_a, frame_b) of the registrations, in the order they are added
D2_AXIS, D2_DEG, D2_T = (-0.5, 1.0, 2.0), 2.5, np.array([-0.04, 0.02, 0.03])
THIRD_FIRST = 1
ODOM_SIGMA = (0.5, 0.5)                                         # metres, radians: the submaps were opened at the same pose, 5 cm and 3 degrees from the truth
WRONG = (12, 0, 25.0)                                           # the deliberately wrong fourth constraint: the truth of this pair turned by 25 degrees about z
SOLVER = dict(iters=20, pcg_tol=1e-6)


def displacement2():
    return ts.rotation(D2_AXIS, D2_DEG), D2_T.copy()


def third_frames():
    """[(R, T, depth)]: frames 1..6 at the poses the third submap integrates them at, D2^-1 P"""
    Rd, Td = displacement2()
    out = []
    for f in range(THIRD_FIRST, THIRD_FIRST + rs.N_FRAMES):
        R, T = ts.pose(f)
        out.append((Rd.T @ R, Rd.T @ (T - Td), ts.box_depth(R, T)))
    return out


def truth():
    """{frame: (R, T)}: the true base poses"""
    return {0: (np.eye(3), np.zeros(3)), 6: rs.displacement(), 12: displacement2()}


def start():
    """{frame: (R, T)}: the pose table the run starts from: submap 0 at the identity, the others 3 cm / 1.5 degrees off (directions from default_rng(29))"""
    rng = np.random.default_rng(29)
    out = {0: (np.eye(3), np.zeros(3))}
    m, deg = rs.PERTURBATIONS[0]
    for f in (6, 12):
        R, T = truth()[f]
        tdir, axis = rng.standard_normal(3), rng.standard_normal(3)
        out[f] = (ts.rotation(axis, deg) @ R, T + m * tdir / np.linalg.norm(tdir))
    return out


def relative(Pa, Pb):
    """P_b^-1 P_a"""
    return Pb[0].T @ Pa[0], Pb[0].T @ (Pa[1] - Pb[1])


def wrong_constraint():
    """(frame_a, frame_b, R, T): the true relative pose of WRONG's pair turned by its angle"""
    fa, fb, deg = WRONG
    R, T = relative(truth()[fa], truth()[fb])
    return fa, fb, R @ ts.rotation((0.0, 0.0, 1.0), deg), T


def errors(poses):
    """the largest (metres, degrees) between {frame: (R, T)} and the truth"""
    e = [ts.pose_error(poses[f][0], poses[f][1], *truth()[f]) for f in FRAMES]
    return max(x[0] for x in e), max(x[1] for x in e)


def graph(constraints, poses):
    """the arrays SubmapMapping._graph builds from the three submaps at `poses`: two odometry edges (identity: all opened at one pose), then the
    constraints [(frame_a, frame_b, R, T, L 6 x 6)]"""
    from taichislam_amd.utils import pose_information
    import pose_graph_ref as ref
    at = {f: n for n, f in enumerate(FRAMES)}
    R, T = np.stack([poses[f][0] for f in FRAMES]), np.stack([poses[f][1] for f in FRAMES])
    ij = [(1, 0), (2, 1)] + [(at[c[0]], at[c[1]]) for c in constraints]
    Z = np.array([np.concatenate([np.eye(3).reshape(9), np.zeros(3)])] * 2 + [np.concatenate([np.asarray(c[2]).reshape(9), np.asarray(c[3]).reshape(3)]) for c in constraints])
    L = ref.pack_upper(np.array([pose_information(*ODOM_SIGMA)] * 2 + [np.asarray(c[4]) for c in constraints]))
    return R, T, np.array([1, 0, 0], np.uint8), np.array(ij, np.int32), Z, L


@functools.lru_cache(maxsize=None)
def chain():
    """The CPU chain: the three registrations by tests/register_ref.py over the oracle's maps from the start table, then the graph by
    tests/pose_graph_ref.py.  Computed once; shared and never written."""
    import pose_graph_ref as ref
    K = ts.intrinsics()
    maps = {0: rs.dst_oracle(), 6: rs.src_oracle(), 12: rsc.room_oracle(K, third_frames(), SMALL)}
    grids = {0: rs.dst_grid(), 6: rsc.oracle_grid(maps[6])}
    src = {6: rs.src_voxels(), 12: rr.source(maps[12].export_sparse())}
    st = start()
    constraints = []
    for fa, fb in PAIRS:
        R0, T0 = relative(st[fa], st[fb])
        R, T, info = rr.register(src[fa], R0, T0, rs.VS, grids[fb], **rs.GATES)
        v = np.asarray(info["records"][-1]["sums"])[:21].astype(np.float64) * 2.0 ** -20      # the last linearisation's H: the information matrix
        H = np.zeros((6, 6))
        iu = np.triu_indices(6)
        H[iu] = v
        H[(iu[1], iu[0])] = v
        constraints.append((fa, fb, R, T, H, int(info["status"])))
    out = ref.solve(*graph(constraints, st), **SOLVER)[0]
    poses = {f: (out["R"][n], out["T"][n]) for n, f in enumerate(FRAMES)}
    return {"constraints": constraints, "poses": poses, "status": out["status"], "iterations": out["iterations"], "cost": out["cost"], "errors": errors(poses)}
