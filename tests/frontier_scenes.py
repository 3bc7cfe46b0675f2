"""Hand-built maps for the frontier tests (tests/test_frontier_cpu.py, tests/test_frontier_gpu.py): each is a few bricks, the smallest shape at which
one part of the extraction can go wrong.  A scene is a dictionary of load_numpy / import_sparse arrays; place() moves it onto a brick corner of the
geometry at hand (the brick faces of SLAB lie at 8 mod 16) and can swap x and z (TALL is narrow in x and long in z)."""
import numpy as np

from util import SLAB, SMALL, TALL

FREE_T, OCC_T, MID_T = 0.5, 0.0, 0.1          # TSDF values: free / occupied at every threshold used here; MID_T is free at the default threshold, occupied at 0.2

GEOMETRIES = {"SMALL": dict(cfg=SMALL, N=256, Nz=256, o=(0, 0, 0), swap=False),
              "SLAB": dict(cfg=SLAB, N=144, Nz=48, o=(8, 8, 8), swap=False),
              "TALL": dict(cfg=TALL, N=64, Nz=128, o=(0, 0, 0), swap=True)}


def box(lo, hi):
    """int64 [n, 3]: the voxels lo <= (i, j, k) <= hi"""
    r = [np.arange(lo[a], hi[a] + 1) for a in range(3)]
    return np.stack(np.meshgrid(*r, indexing="ij"), -1).reshape(-1, 3).astype(np.int64)


def scene(parts):
    """parts: [(voxels int [n, 3], tsdf value)] -> the arrays of load_numpy / import_sparse"""
    idx = np.concatenate([np.asarray(p, np.int64).reshape(-1, 3) for p, _ in parts])
    t = np.concatenate([np.full(np.asarray(p).reshape(-1, 3).shape[0], v, np.float16) for p, v in parts])
    assert np.unique(idx, axis=0).shape[0] == idx.shape[0], "a voxel is listed twice"
    return {"indices": idx.astype(np.int16), "TSDF": t, "W_TSDF": np.ones(t.shape[0], np.float16), "occupy": np.zeros(t.shape[0], np.int8)}


def place(sc, geo):
    """the scene moved by the geometry's brick-corner offset, x and z swapped first where the geometry asks for it; asserts that it fits the volume"""
    g = GEOMETRIES[geo]
    idx = sc["indices"].astype(np.int64)
    if g["swap"]:
        idx = idx[:, ::-1]
    idx = idx + np.array(g["o"])
    h = np.array([g["N"] // 2, g["N"] // 2, g["Nz"] // 2])
    assert (idx >= -h).all() and (idx < h).all(), f"the scene does not fit {geo}"
    return dict(sc, indices=np.ascontiguousarray(idx.astype(np.int16)))


def load_pair(g, o, sc, sid=0):
    """the same voxels into the GPU map and the oracle"""
    g.load_numpy(sid, sc["indices"], sc["TSDF"], sc["W_TSDF"], sc["occupy"], None)
    o.import_sparse(sid, sc["indices"], sc["TSDF"], sc["W_TSDF"], sc["occupy"])


# ---- (a) a free cube across the corner where eight bricks meet, surrounded by unknown: the frontier is its shell, one cluster
def shell():
    return scene([(box((-10, -10, -10), (9, 9, 9)), FREE_T)])


SHELL_VOXELS, SHELL_EDGES_CORNERS, SHELL_CORNERS = 20 ** 3 - 18 ** 3, 12 * 18 + 8, 8


# ---- (b) blobs whose only contact is diagonal: A / B across a brick corner, C / D across a brick edge (the edge along x through y = z = 0)
def diagonal():
    return scene([(box((-2, -2, -2), (-1, -1, -1)), FREE_T), (box((0, 0, 0), (1, 1, 1)), FREE_T),
                  (box((20, -2, -2), (21, -1, -1)), FREE_T), (box((20, 0, 0), (21, 1, 1)), FREE_T)])


DIAGONAL_CLUSTERS = {26: 2, 18: 3, 6: 4}          # every blob is 8 voxels, all of them frontier voxels


# ---- (c) a free block flush against the +x wall of the volume (+z wall when x and z are swapped): no frontier on that face
def wall(geo):
    g = GEOMETRIES[geo]
    top = (g["Nz"] if g["swap"] else g["N"]) // 2 - 1 - g["o"][2 if g["swap"] else 0]      # (place() adds the offset again)
    return scene([(box((top - 7, 0, 0), (top, 7, 7)), FREE_T)])


WALL_VOXELS = 8 ** 3 - 6 ** 3 - 6 * 6          # the shell without the interior of the face on the wall


# ---- (d) two kinds of unknown: a whole free brick; its -x neighbour brick is absent, its +x neighbour is allocated by one lone voxel and otherwise unobserved
def two_unknowns():
    return scene([(box((0, 0, 0), (15, 15, 15)), FREE_T), (box((24, 8, 8), (24, 8, 8)), FREE_T)])


TWO_UNKNOWNS_VOXELS = 16 ** 3 - 14 ** 3 + 1


# ---- (e) a one-voxel tube through many bricks that returns next to its start; the least key (the least x) lies in the middle of the chain
def polyline(points):
    out = [np.array(points[0], np.int64)]
    for p in points[1:]:
        p = np.array(p, np.int64)
        while not np.array_equal(out[-1], p):
            out.append(out[-1] + np.sign(p - out[-1]))
    return np.stack(out)


def tube():
    pts = [(40, 5, 5), (20, 5, 5), (20, 5, -12), (-20, 5, -12), (-20, 5, 5), (-40, 5, 5), (-40, 9, 5), (-20, 9, 5), (-20, 9, -12), (20, 9, -12), (20, 9, 5), (40, 9, 5)]
    return scene([(polyline(pts), FREE_T)])


# ---- (f) a one-voxel spiral inside one brick: eight square spirals in the even layers, joined alternately at the centre and at the outer end
def spiral_cells(n=16):
    cells, seen = [], set()
    x, y, dx, dy = 0, 0, 1, 0
    while True:
        cells.append((x, y)); seen.add((x, y))
        for _ in range(2):
            nx, ny = x + dx, y + dy
            ok = 0 <= nx < n and 0 <= ny < n and (nx, ny) not in seen and not any((nx + a, ny + b) in seen and (nx + a, ny + b) != (x, y) for a, b in ((1, 0), (-1, 0), (0, 1), (0, -1)))
            if ok:
                break
            dx, dy = -dy, dx
        if not ok:
            return cells
        x, y = nx, ny


def spiral_path():
    """int64 [n, 3]: the path in order, brick-local coordinates 0 .. 15"""
    cells, out = spiral_cells(), []
    for layer in range(8):
        z = 2 * layer
        run = cells if layer % 2 == 0 else cells[::-1]
        out += [(x, y, z) for x, y in run]
        if layer < 7:
            out.append((run[-1][0], run[-1][1], z + 1))
    return np.array(out, np.int64)


def spiral():
    return scene([(spiral_path(), FREE_T)])


# ---- (g) an occupied plate beside half of the cube's +x face: with clear_of_occupied the frontier voxels one step from it (diagonally) go as well
def plate():
    return scene([(box((-10, -10, -10), (9, 9, 9)), FREE_T), (box((10, -10, -10), (10, -1, 9)), OCC_T)])


def two_values():
    """the cube with its lower half at a TSDF value between the default threshold and 0.2"""
    return scene([(box((-10, -10, -10), (9, 9, -1)), MID_T), (box((-10, -10, 0), (9, 9, 9)), FREE_T)])


SCENES = {"shell": shell, "diagonal": diagonal, "two_unknowns": two_unknowns, "tube": tube, "spiral": spiral, "plate": plate, "two_values": two_values}
