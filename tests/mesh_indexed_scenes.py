"""Hand-built maps for the indexed-mesh tests (tests/test_mesh_indexed_cpu.py, tests/test_mesh_indexed_gpu.py), in the style of tests/frontier_scenes.py:
each is a few bricks, the smallest shape at which one part of the mesher can go wrong.  A scene is the dictionary of load_numpy / import_sparse arrays
plus "thres", the surface threshold it is meshed with; frontier_scenes.place() moves it onto a brick corner of the geometry at hand (the brick faces of
SLAB lie at 8 mod 16) and swaps x and z on TALL.  Every scene fits x in [-64, 63], y in [-32, 31], z in [-32, 15], which all three geometries hold."""
import numpy as np

import mesh_indexed_ref as ref
from frontier_scenes import GEOMETRIES, box, place

V = 0.02                              # |TSDF| of the plain voxels


def scene(idx, values, thres=0.1):
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    t = np.asarray(values, np.float16).reshape(-1)
    assert idx.shape[0] == t.shape[0] and np.unique(idx, axis=0).shape[0] == idx.shape[0], "a voxel is listed twice"
    return {"indices": idx.astype(np.int16), "TSDF": t, "W_TSDF": np.ones(t.shape[0], np.float16), "occupy": np.zeros(t.shape[0], np.int8), "thres": thres}


def join(*scs):
    return scene(np.concatenate([s["indices"].astype(np.int64) for s in scs]), np.concatenate([s["TSDF"] for s in scs]), scs[0]["thres"])


def placed(sc, geo):
    return dict(place(sc, geo), thres=sc["thres"])


# ---- (a) every case of the table: 256 isolated cells on a lattice of pitch 3 (8 x 8 x 4, across the brick corner), cell n with corner signs n
def cases():
    idx, val = [], []
    for n in range(256):
        o = np.array([-12 + 3 * (n % 8), -12 + 3 * ((n // 8) % 8), -6 + 3 * (n // 64)])
        for q in range(8):
            idx.append(o + ref.CORNER[q])
            val.append(-V if (n >> q) & 1 else V)
    return scene(np.array(idx), val)


CASES_TRIANGLES = int(ref.NTRI.sum())


# ---- (b) a sphere of radius 6.3 voxels about the point where eight bricks meet, in a fully observed 20^3 box; the threshold is above every value
BALL_THRES = 1.0


def ball():
    idx = box((-10, -10, -10), (9, 9, 9))
    r = np.sqrt(((idx + 0.5) ** 2).sum(1))
    return scene(idx, (r - 6.3) * 0.04, BALL_THRES)


def ball_parts():
    """the ball as its eight octants (one per brick), for loading part by part"""
    sc = ball()
    idx = sc["indices"].astype(np.int64)
    octant = (idx[:, 0] >= 0) * 4 + (idx[:, 1] >= 0) * 2 + (idx[:, 2] >= 0)
    return [scene(idx[octant == o], sc["TSDF"][octant == o], BALL_THRES) for o in range(8)]


# ---- (c) valid cells in the last layer of brick A along one axis; the edges of their far face belong to voxels of brick B, which holds only that one
#          voxel layer, every value at or above the (negative) threshold: B owns vertices and has no triangle
ORPHAN_THRES = -0.05


def _orphan(axis, base, last):
    """the A layer at coordinate `last` of `axis` (value -0.1, below the threshold), the B layer at last + 1 (a checkerboard of +-0.02)"""
    idx, val = [], []
    for u in range(2, 10):
        for w in range(2, 10):
            for layer in (0, 1):
                p = [0, 0, 0]
                p[axis] = last + layer
                p[(axis + 1) % 3] = base[(axis + 1) % 3] + u
                p[(axis + 2) % 3] = base[(axis + 2) % 3] + w
                idx.append(p)
                val.append(-0.1 if layer == 0 else (V if (u + w) % 2 else -V))
    return scene(np.array(idx), val, ORPHAN_THRES)


def orphan():
    return join(_orphan(0, (0, 0, 0), 15), _orphan(1, (-32, 0, -16), 15), _orphan(2, (32, -32, 0), -1))


ORPHAN_CELLS = 3 * 7 * 7             # the valid cells: those of the A layers whose eight corners are listed


# ---- (d) a plane through the last voxel layers of the volume at its +++ and its --- corner (built in the geometry's own coordinates)
RIM_THRES = 1.0


def rim(geo):
    """already placed: the scene depends on where the volume ends"""
    g = GEOMETRIES[geo]
    h = np.array([g["N"] // 2, g["N"] // 2, g["Nz"] // 2])
    a = box(h - 6, h - 1)                              # the six last layers on every axis
    b = box(-h, -h + 5)                                # and the six first
    va = ((a - (h - 1)).sum(1) + 7.5) * 0.01
    vb = ((b + h).sum(1) - 7.5) * 0.01
    sc = scene(np.concatenate([a, b]), np.concatenate([va, vb]), RIM_THRES)
    return dict(sc, indices=np.ascontiguousarray(sc["indices"]))


# ---- (e) the eps snap: a plane of exact zeros through a 4^3 block across the brick corner (many edges end in one corner: coincident vertices, distinct
#          rows), and one cell with a pair of opposite-sign f16 subnormals on its edge 0 (both below the eps: the vertex is the lower corner)
SUB = 6e-8
SNAP_SUB_EDGE = (8, 8, 8, 0)


def snap():
    blk = box((-2, -2, -2), (1, 1, 1))
    a = scene(blk, blk.sum(1) * 0.01)
    cell = np.array([8, 8, 8]) + ref.CORNER
    v = np.full(8, V)
    v[0], v[1] = SUB, -SUB
    return join(a, scene(cell, v))


SCENES = {"cases": cases, "ball": ball, "orphan": orphan, "snap": snap}
SCENE_NAMES = sorted(SCENES) + ["rim"]


def build(name, geo):
    """the scene placed on the geometry"""
    return rim(geo) if name == "rim" else placed(SCENES[name](), geo)


def load_pair(g, o, sc, sid=0):
    g.load_numpy(sid, sc["indices"], sc["TSDF"], sc["W_TSDF"], sc["occupy"], None)
    o.import_sparse(sid, sc["indices"], sc["TSDF"], sc["W_TSDF"], sc["occupy"])
