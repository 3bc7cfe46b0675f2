"""Hand-built maps and facelet stores for the topology-graph tests (tests/test_topo_graph_cpu.py, tests/test_topo_graph_gpu.py).  Maps are dictionaries of
load_numpy / import_sparse arrays as in tests/frontier_scenes.py (box and scene come from there): every listed voxel is observed, free at FREE_T and occupied at
OCC_T; an unlisted voxel is unobserved, reads TSDF 0 and so counts as occupied for a ray and as unobserved for is_pos_unobserved."""
import numpy as np

from frontier_scenes import FREE_T, OCC_T, box, scene
from util import SMALL, lin

F32 = np.float32

# ---- the whole graph: a corridor longer than twice max_raycast_dist with a side room behind a door and an alcove ----------------------------------------
# Chosen on the CPU with the restatement so that with 32 and with 64 rays, 8 frontiers examined: at least 3 nodes come out, frontiers are accepted and rejected,
# the expansion inside the alcove is refused by detect_collisions (every ray black, mean length below thres_size), and facelets fail to be frontiers for each
# of the three reasons.  With 32 rays node 4 gets an edge to node 2 through a type-1 hit of a frontier ray; with 64 rays no such edge comes up.
GRAPH_CFG = dict(SMALL, voxel_scale=0.1, map_scale=[12.0, 6.0])           # N = 128, Nz = 64
GRAPH_VS = 0.1
GRAPH_PARAMS = dict(max_raycast_dist=1.0, thres_size=0.5, frontier_creation_threshold=0.5, frontier_verify_threshold=0.5)
GRAPH_START = (-1.5, 0.0, 0.0)
GRAPH_MAX_FRONTIERS = 8
CORRIDOR = ((-30, -5, -5), (29, 4, 4))                                     # 6 m x 1 m x 1 m
DOOR = ((2, 5, -5), (7, 7, 4))                                             # 0.6 m wide, through a 0.3 m wall
ROOM = ((-4, 8, -5), (13, 19, 4))                                          # 1.8 m x 1.2 m x 1 m
ALCOVE = ((-19, -11, -5), (-13, -6, 4))                                    # 0.7 m x 0.6 m x 1 m, off the corridor beside the start: too small for a node
WINDOW = ((-20, -5, 5), (-10, 4, 6))                                       # a patch of the corridor's ceiling that was never observed


def dilate(vox, r):
    out = [vox + np.array(d) for d in box((-r, -r, -r), (r, r, r))]
    return np.unique(np.concatenate(out), axis=0)


def without(a, b):
    return a[~np.isin(lin(a), lin(b))]


def graph_scene():
    """free space = corridor + door + room + alcove; a two-voxel observed wall around it, except behind WINDOW, where the map ends"""
    free = np.unique(np.concatenate([box(*CORRIDOR), box(*DOOR), box(*ROOM), box(*ALCOVE)]), axis=0)
    wall = without(without(dilate(free, 2), free), box(*WINDOW))
    return scene([(free, FREE_T), (wall, OCC_T)])


def reordered(sc, seed=1):
    """the same voxels in another order: the bricks are allocated in another order"""
    o = np.random.default_rng(seed).permutation(sc["indices"].shape[0])
    return {k: np.ascontiguousarray(v[o]) for k, v in sc.items()}


# ---- hand-built stores -----------------------------------------------------------------------------------------------------------------------------------
HAND_CFG = dict(SMALL, voxel_scale=0.05, map_scale=[12.8, 6.4])           # a 0.05 m voxel: 80 steps at 4 m
HAND_VS = 0.05


HAND_LO, HAND_HI = (-40, -20, -20), (100, 20, 20)
# rows of y (voxel index j) -> the voxel index i of an occupied wall across the row; the rays of the cases run along +x through the middle of a row
HAND_ROWS = {"wall12": ((-20, -11), 12), "wall63": ((-10, -1), 63), "wall64": ((0, 9), 64), "open": ((10, 20), None)}
HAND_Y = {"wall12": -0.75, "wall63": -0.25, "wall64": 0.25, "open": 0.75}


def hand_map():
    """one map for every hand-built case: a block of free space, -2 .. 5 m along x and +-1 m across, that ends in unobserved space (where a ray stops), with
    a one-voxel occupied wall at x = 0.6 m (step 12 of a ray from x = 0), 3.15 m (step 63), 3.2 m (step 64) or none, depending on the row of y"""
    free = box(HAND_LO, HAND_HI)
    walls = np.concatenate([box((i, j[0], HAND_LO[2]), (i, j[1], HAND_HI[2])) for j, i in HAND_ROWS.values() if i is not None])
    return scene([(without(free, walls), FREE_T), (walls, OCC_T)])


def strip(n, x, y0=-1.0, y1=1.0, z0=-1.0, z1=1.0):
    """n triangles (n even or odd) that tile the rectangle x = const, y0 .. y1, z0 .. z1 as a strip along y: f32 [n, 3, 3]; triangle 2 c and 2 c + 1 share the
    diagonal of cell c"""
    cells = (n + 1) // 2
    ys = np.linspace(y0, y1, cells + 1)
    out = []
    for c in range(cells):
        a, b = ys[c], ys[c + 1]
        out.append([[x, a, z0], [x, b, z0], [x, b, z1]])
        out.append([[x, a, z0], [x, b, z1], [x, a, z1]])
    return np.array(out[:n], F32)


def square(x, half=1.0, y=0.0, z=0.0):
    """two triangles that tile the square x = const, |y' - y|, |z' - z| <= half; they share the diagonal y' - y = z' - z"""
    a, b, c, d = y - half, y + half, z - half, z + half
    return np.array([[[x, a, c], [x, b, c], [x, b, d]], [[x, a, c], [x, b, d], [x, a, d]]], F32)


def rays(pos, dir, max_dist, skip=None, backward=-0.01, facelets_only=False):
    pos = np.asarray(pos, F32).reshape(-1, 3)
    dir = np.ascontiguousarray(np.broadcast_to(np.asarray(dir, F32).reshape(-1, 3), pos.shape))
    return dict(pos=pos, dir=dir, max_dist=max_dist, skip=skip, backward=backward, facelets_only=facelets_only)


def along_x(y, z=0.0, x=0.0):
    return np.array([x, y, z], F32)


def cull_ys():
    """(y_in, y_out): neighbouring f32 values of y at which a ray origin (0, y, 0) lies just inside / exactly on the reach 2.0 of a node centred at (0.5, 0, 0):
    sqrt((0.25 + y * y) + 0) < 2 holds for y_in and fails for y_out"""
    def dist(y):
        return np.sqrt((F32(0.25) + y * y) + F32(0.0))
    y = F32(np.sqrt(3.75))
    while dist(y) < F32(2.0):
        y = np.nextafter(y, F32(np.inf))
    while not dist(y) < F32(2.0):
        y = np.nextafter(y, F32(-np.inf))
    return y, np.nextafter(y, F32(np.inf))


ORIGIN = (0.0, 0.0, 0.0)
COUNTS = (1, 63, 64, 65, 130)
STEP = F32(HAND_VS)


def hand_cases():
    """name -> dict(polys=[(triangles, start)], rays=[ray set]); every case starts from an empty store on hand_map(), with max_raycast_dist = 1.0"""
    X = (1.0, 0.0, 0.0)
    cases = {}
    # facelet counts that straddle the waves: two nodes of n facelets each, the second in front of half of the first
    ys = np.linspace(-0.97, 0.97, 31)
    fan = np.stack([np.zeros(31), ys, np.full(31, 0.1)], 1)
    slant = np.array([1.0, 0.3, 0.2]) / np.linalg.norm([1.0, 0.3, 0.2])
    for n in COUNTS:
        cases[f"count{n}"] = dict(polys=[(strip(n, 0.5), ORIGIN), (strip(n, 0.3, y0=0.0, y1=1.0), ORIGIN)],
                                  rays=[rays(fan, X, 1.0), rays(fan, slant, 1.0), rays(fan, X, 1.0, facelets_only=True), rays(fan, X, 0.4)])
    # ties: the two triangles of a square as two nodes, the rays through their shared edge: equal t, the lower facelet (node 0) wins
    sq = square(0.5)
    diag = [(0.0, 0.25, 0.25), (0.0, -0.5, -0.5), (0.0, 0.0, 0.0), (0.0, 0.25, 0.0), (0.0, 0.0, 0.25)]
    cases["tie"] = dict(polys=[(sq[1:2], ORIGIN), (sq[0:1], ORIGIN)], rays=[rays(diag, X, 1.0), rays(diag, X, 1.0, facelets_only=True)])
    # a ray in the plane of the triangles (a = 0), one with |a| = 8e-6 <= 1e-5 and one with |a| = 1.6e-5
    inplane = [(0.5, 0.1, -0.5)] * 3
    cases["parallel"] = dict(polys=[(sq, ORIGIN)], rays=[rays(inplane, [(0.0, 0.0, 1.0), (2e-6, 0.0, 1.0), (4e-6, 0.0, 1.0)], 1.0, facelets_only=True),
                                                         rays(inplane, [(0.0, 0.0, 1.0), (2e-6, 0.0, 1.0), (4e-6, 0.0, 1.0)], 1.0)])
    # the backward window: origins just behind the square
    behind = [(0.505, 0.1, 0.0), (0.5099, 0.1, 0.0), (0.5101, 0.1, 0.0), (0.52, 0.1, 0.0)]
    far_behind = [(0.6, 0.1, 0.0), (0.6999, 0.1, 0.0), (0.7001, 0.1, 0.0), (0.75, 0.1, 0.0)]
    cases["backward"] = dict(polys=[(sq, ORIGIN)], rays=[rays(behind, X, 1.0), rays(behind, X, 1.0, facelets_only=True),
                                                         rays(far_behind, X, 0.5, backward=-0.2, facelets_only=True)])
    # skip_idx hides the only hit
    three = [(0.0, 0.1, 0.0)] * 3
    cases["skip"] = dict(polys=[(sq, ORIGIN)], rays=[rays(three, X, 1.0, skip=np.array([-1, 0, 1], np.int32)),
                                                     rays(three, X, 1.0, skip=np.array([-1, 0, 1], np.int32), facelets_only=True)])
    # a node exactly on either side of the cull radius: max_dist + max_raycast_dist = 2.0 from the centre (0.5, 0, 0) of a square of 6 m
    y_in, y_out = cull_ys()
    edge = [(0.0, y_in, 0.0), (0.0, y_out, 0.0), (0.0, -y_in, 0.0), (0.0, -y_out, 0.0)]
    cases["cull"] = dict(polys=[(square(0.5, half=3.0), ORIGIN)], rays=[rays(edge, X, 1.0, facelets_only=True), rays(edge, X, 1.0)])
    # map against facelets, along the row whose wall is step 12 of the ray (len 12 * voxel): a patch behind the wall, in front of it, at 12 and 13 voxels,
    # and inside the wall voxel behind the step (the facelet hit cuts the walk to int(0.62 / voxel) = 12 steps, 0 .. 11, so the wall is never seen)
    y = HAND_Y["wall12"]
    for name, x in (("map_nearer", 0.8), ("facelet_nearer", 0.4), ("equal_len", F32(12) * STEP), ("one_step_more", F32(13) * STEP), ("cut_short", 0.62)):
        cases[name] = dict(polys=[(square(x, half=0.2, y=y), (0.0, y, 0.0))], rays=[rays([along_x(y), along_x(y, 0.1), along_x(y, -0.1)], X, 1.0)])
    # step counts on an empty store: none, 63, 64, 65, 80 steps; a wall at step 63 (the last lane of the first chunk) and at step 64 (the first of the second)
    rows = [along_x(HAND_Y[r]) for r in ("wall12", "wall63", "wall64", "open")]
    cases["steps"] = dict(polys=[], rays=[rays(rows, X, d) for d in (0.0, 0.04, 3.16, 3.21, 3.26, 4.01)])
    # origins outside the volume and origins / directions that are not finite, without and with a store
    nan, inf = float("nan"), float("inf")
    odd_pos = [(100.0, 0.0, 0.0), (nan, 0.0, 0.0), (0.0, nan, 0.0), (inf, 0.0, 0.0), (0.0, 0.1, 0.0), (0.0, 0.1, 0.0), (-1.0e30, 0.0, 0.0)]
    odd_dir = [X, X, X, X, (nan, 0.0, 0.0), (inf, 0.0, 0.0), X]
    cases["odd_empty"] = dict(polys=[], rays=[rays(odd_pos, odd_dir, 1.0)])
    cases["odd_store"] = dict(polys=[(sq, ORIGIN)], rays=[rays(odd_pos, odd_dir, 1.0), rays(odd_pos, odd_dir, 1.0, facelets_only=True)])
    return cases
