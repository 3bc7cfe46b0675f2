"""Hand-built maps for the navigation-grid tests (tests/test_nav_grid_gpu.py), made with the helpers of tests/frontier_scenes.py: each is a few bricks,
the smallest shape at which one part of the pass can go wrong.  Scenes given in scene coordinates go through put(), which moves them onto a brick corner
of the geometry (the brick faces of SLAB lie at 8 mod 16) WITHOUT swapping x and z -- the bands are along z on every geometry; scenes that must touch the
edges of the grid are built in the geometry's own voxel indices."""
import numpy as np

from frontier_scenes import FREE_T, GEOMETRIES, OCC_T, box, place, scene

NAN_T = float("nan")


def put(sc, geo):
    """place() without its swap of x and z: on a geometry that swaps, the scene is swapped first, so that place() puts it back"""
    if GEOMETRIES[geo]["swap"]:
        sc = dict(sc, indices=np.ascontiguousarray(sc["indices"][:, ::-1]))
    return place(sc, geo)


def dims(geo):
    g = GEOMETRIES[geo]
    return g["N"], g["Nz"], g["o"][2]


# ---- (a) columns: one feature per (i, j) column, all inside -12 .. 24 in i and j and -20 .. 8 in k (scene coordinates; fits every geometry)
COL_GAP = (2, -3)            # an occupied voxel at k = -20 and a free one at k = 5: the brick between them (k = -16 .. -1) is absent
COL_LONE = (24, 8)           # a brick allocated by one lone free voxel at k = 8 and otherwise unobserved
COL_NAN = (5, -5)            # free at k = 0 and 2, an observed NaN between them
# layers k = 0 .. 5 of the columns (n, -10): (occupied, free) voxels from the bottom, the rest unobserved
LIMIT_COLUMNS = [(1, 5), (2, 4), (1, 2), (1, 3), (0, 6), (0, 5), (0, 3), (0, 2), (2, 0), (1, 0)]
LIMIT_BAND = (0, 5)


def columns():
    parts = [(box(COL_GAP + (-20,), COL_GAP + (-20,)), OCC_T), (box(COL_GAP + (5,), COL_GAP + (5,)), FREE_T),
             (box(COL_LONE + (8,), COL_LONE + (8,)), FREE_T),
             (box(COL_NAN + (0,), COL_NAN + (0,)), FREE_T), (box(COL_NAN + (1,), COL_NAN + (1,)), NAN_T), (box(COL_NAN + (2,), COL_NAN + (2,)), FREE_T),
             (box((-12, 0, 0), (12, 12, 0)), FREE_T)]                                          # a free plate: free cells for flags bit 0
    for n, (no, nf) in enumerate(LIMIT_COLUMNS):
        if no:
            parts.append((box((n - 10, -10, 0), (n - 10, -10, no - 1)), OCC_T))
        if nf:
            parts.append((box((n - 10, -10, no), (n - 10, -10, no + nf - 1)), FREE_T))
    return scene(parts)


def limit_classes(min_occ, min_free, max_unknown):
    """the classes of the LIMIT_COLUMNS over LIMIT_BAND, worked out from the definition (0 free, 1 occupied, 2 unknown)"""
    out = []
    for no, nf in LIMIT_COLUMNS:
        nu = 6 - no - nf
        out.append(1 if no >= min_occ else 0 if nf >= min_free and (max_unknown is None or nu <= max_unknown) else 2)
    return out


# ---- (b) obstacle columns in one layer (scene coordinates): [(i, j)] occupied at k = 0
def posts(cells):
    c = np.asarray(cells, np.int64).reshape(-1, 2)
    return scene([(np.concatenate([c, np.zeros((c.shape[0], 1), np.int64)], 1), OCC_T)])


def three_four_five():
    return posts([(0, 0)])


def row_versus_plane():
    return posts([(0, 0), (1, -3)])


def scatter(n=200, seed=7, half=100):
    """about n obstacle columns at seeded places of a free floor of (2 half + 20)^2 cells, one layer thick; the rest of the grid is unknown"""
    r = np.random.default_rng(seed)
    c = np.unique(r.integers(-half, half, size=(n, 2)), axis=0)
    floor = box((-half - 10, -half - 10, 0), (half + 9, half + 9, 0))
    occ = np.zeros((2 * half + 20, 2 * half + 20), bool)
    occ[c[:, 0] + half + 10, c[:, 1] + half + 10] = True
    return scene([(np.concatenate([c, np.zeros((c.shape[0], 1), np.int64)], 1), OCC_T), (floor[~occ.reshape(-1)], FREE_T)])


# ---- (c) scenes in the geometry's own voxel indices: the corners, the edges, lines across the whole grid (layer k)
def _own(cells, k):
    c = np.asarray(cells, np.int64).reshape(-1, 2)
    return scene([(np.concatenate([c, np.full((c.shape[0], 1), k, np.int64)], 1), OCC_T)])


def corners(geo, k):
    N = GEOMETRIES[geo]["N"]
    lo, hi = -(N // 2), N // 2 - 1
    return _own([(lo, lo), (lo, hi), (hi, lo), (hi, hi)], k)


def edges(geo, k):
    N = GEOMETRIES[geo]["N"]
    lo, hi = -(N // 2), N // 2 - 1
    r = np.arange(lo, hi + 1)
    cells = [(lo, j) for j in r] + [(hi, j) for j in r] + [(i, lo) for i in r[1:-1]] + [(i, hi) for i in r[1:-1]]
    return _own(cells, k)


def lines(geo, k, i_line=3, j_line=-5):
    """a one-voxel wall along j at i = i_line and one along i at j = j_line: they cross every brick and every strip of the distance pass"""
    N = GEOMETRIES[geo]["N"]
    r = np.arange(-(N // 2), N // 2)
    cells = [(i_line, j) for j in r] + [(i, j_line) for i in r if i != i_line]
    return _own(cells, k)
