"""Hand-built maps for the terrain-layer tests (tests/test_nav_terrain_cpu.py, tests/test_nav_terrain_gpu.py), made with the helpers of
tests/frontier_scenes.py and nav_grid_scenes.put: each is a few bricks, the smallest shape at which one part of the pass can go wrong.  Scene coordinates
have their brick faces at multiples of 16 on every geometry (put() moves them onto a brick corner); scenes that must touch the top of the volume, the
edges of the grid or the tile borders of the window kernel are built in the geometry's own voxel indices.  The hand-worked values next to each scene
hold for THRES = 0.25 (exact in every format), where the pair (0.0, 0.5) gives r = 8 exactly."""
import numpy as np

from frontier_scenes import FREE_T, GEOMETRIES, OCC_T, scene

NAN_T, INF_T = float("nan"), float("inf")
THRES = 0.25
SUB_T = 2.0 ** -24                                      # the smallest subnormal f16

# ---- (a) columns: one feature each.  name -> ((i, j), [(k, value)]) in scene coordinates.  The brick column of i, j in 16 .. 31 holds GAP and GAPTOP
# only, so that its brick k = -16 .. -1 is absent.
COLUMNS = {
    "LK15": ((-12, -10), [(-1, OCC_T), (0, FREE_T)]),                    # a support at lk = 15, the free voxel in the brick above
    "BLOCK1": ((-10, -10), [(-8, OCC_T), (-7, FREE_T), (9, OCC_T)]),     # occupied at k + 17: blocks at clearance 17, across one brick face
    "CLEAR1": ((-8, -10), [(-8, OCC_T), (-7, FREE_T), (10, OCC_T)]),     # occupied at k + 18: does not
    "BLOCK2": ((-6, -10), [(-17, OCC_T), (-16, FREE_T), (0, OCC_T)]),    # the same across two brick faces
    "CLEAR2": ((-4, -10), [(-17, OCC_T), (-16, FREE_T), (1, OCC_T)]),
    "TWO": ((-2, -10), [(-20, OCC_T), (-19, FREE_T), (4, OCC_T), (5, FREE_T)]),      # two standable layers: pick
    "WALL": ((0, -10), [(k, OCC_T) for k in range(-8, 9)]),             # nothing to stand on: the top voxel has nothing observed above it
    "EMPTY": ((2, -10), [(-8, FREE_T), (-7, FREE_T), (-6, FREE_T)]),
    "NANUP": ((4, -10), [(-8, OCC_T), (-7, NAN_T), (-6, FREE_T)]),       # an observed NaN at k + 1: not free, not occupied
    "FREE2": ((6, -10), [(-8, OCC_T), (-7, FREE_T), (-6, FREE_T)]),      # stands with free_run = 2 as well
    "Q0": ((-12, -6), [(-8, 0.2421875), (-7, 0.5)]),                     # r = 16 * (1 / 128) / (33 / 128) = 0.48
    "Q7": ((-10, -6), [(-8, 0.0), (-7, 0.5625)]),                        # r = 4 / 0.5625 = 7.11
    "Q8": ((-8, -6), [(-8, 0.0), (-7, 0.5)]),                            # r = 8 exactly
    "Q15": ((-6, -6), [(-8, 0.0), (-7, 0.2578125)]),                     # r = 15.5
    "QCLAMP": ((-4, -6), [(-8, 0.0), (-7, 0.25)]),                       # r = 16: clamped to 15 (0.25 is not < thres: free)
    "QSUB": ((-2, -6), [(-8, SUB_T), (-7, 0.5)]),                        # r = 16 * (0.25 - 2^-24) / (0.5 - 2^-24) just below 8: 7 (8 if the subnormal were flushed)
    "QNINF": ((0, -6), [(-8, -INF_T), (-7, 0.5)]),                       # inf / inf: NaN, q = 0
    "QPINF": ((2, -6), [(-8, 0.0), (-7, INF_T)]),                        # 4 / inf = 0
    "GAP": ((20, 20), [(-18, OCC_T), (-17, FREE_T), (0, FREE_T)]),       # the absent brick lies inside the clearance, beyond free_run = 1, inside free_run = 2
    "GAPTOP": ((22, 20), [(-17, OCC_T), (0, FREE_T)]),                   # a support at lk = 15 under an absent brick: k + 1 is unknown
}
COLUMN_BAND = (-20, 8)
# (k, q) of the support (scene layers), or the col code, at THRES, band COLUMN_BAND, clearance 17, for (free_run, pick) -- worked out by hand
COLUMN_ANSWERS = {
    (1, 0): {"LK15": (-1, 8), "BLOCK1": 1, "CLEAR1": (-8, 8), "BLOCK2": 1, "CLEAR2": (-17, 8), "TWO": (-20, 8), "WALL": 1, "EMPTY": 2, "NANUP": 1, "FREE2": (-8, 8),
             "Q0": (-8, 0), "Q7": (-8, 7), "Q8": (-8, 8), "Q15": (-8, 15), "QCLAMP": (-8, 15), "QSUB": (-8, 7), "QNINF": (-8, 0), "QPINF": (-8, 0),
             "GAP": (-18, 8), "GAPTOP": 1},
    (1, 1): {"LK15": (-1, 8), "BLOCK1": 1, "CLEAR1": (-8, 8), "BLOCK2": 1, "CLEAR2": (-17, 8), "TWO": (4, 8), "WALL": 1, "EMPTY": 2, "NANUP": 1, "FREE2": (-8, 8),
             "Q0": (-8, 0), "Q7": (-8, 7), "Q8": (-8, 8), "Q15": (-8, 15), "QCLAMP": (-8, 15), "QSUB": (-8, 7), "QNINF": (-8, 0), "QPINF": (-8, 0),
             "GAP": (-18, 8), "GAPTOP": 1},
    (2, 0): {"LK15": 1, "BLOCK1": 1, "CLEAR1": 1, "BLOCK2": 1, "CLEAR2": 1, "TWO": 1, "WALL": 1, "EMPTY": 2, "NANUP": 1, "FREE2": (-8, 8),
             "Q0": 1, "Q7": 1, "Q8": 1, "Q15": 1, "QCLAMP": 1, "QSUB": 1, "QNINF": 1, "QPINF": 1, "GAP": 1, "GAPTOP": 1},
    # free_run = 0: the voxel above need not be free -- the tops of WALL, BLOCK1 (k = 9 lies above the band) and BLOCK2, NANUP and GAPTOP stand, with q = 0
    (0, 0): {"LK15": (-1, 8), "BLOCK1": 1, "CLEAR1": (-8, 8), "BLOCK2": (0, 0), "CLEAR2": (-17, 8), "TWO": (-20, 8), "WALL": (8, 0), "EMPTY": 2, "NANUP": (-8, 0),
             "FREE2": (-8, 8), "Q0": (-8, 0), "Q7": (-8, 7), "Q8": (-8, 8), "Q15": (-8, 15), "QCLAMP": (-8, 15), "QSUB": (-8, 7), "QNINF": (-8, 0), "QPINF": (-8, 0),
             "GAP": (-18, 8), "GAPTOP": (-17, 0)},
}
# the bands around CLEAR1's support at k = -8: exactly at k_min, exactly at k_max, just outside on either side -> (k, q) or the col code
EDGE_BANDS = [(-8, 8), (-20, -8), (-7, 8), (-20, -9)]
EDGE_ANSWERS = [(-8, 8), (-8, 8), 2, 2]


def _cells(parts):
    """[(i, j, k, value)] -> scene; voxels of one value share a part"""
    by = {}
    for i, j, k, v in parts:
        by.setdefault(repr(np.float16(v)), (v, []))[1].append((i, j, k))
    return scene([(np.array(c, np.int64), v) for v, c in by.values()])


def columns():
    return _cells([(ij[0], ij[1], k, v) for ij, vox in COLUMNS.values() for k, v in vox])


def top(geo):
    """in the geometry's own indices: a support 3 layers under the top of the volume (the clearance leaves the volume: unknown, allowed), and an occupied
    voxel in the top layer (k + 1 is outside: not free)"""
    t = GEOMETRIES[geo]["Nz"] // 2 - 1
    return _cells([(-20, -20, t - 3, OCC_T), (-20, -20, t - 2, FREE_T), (-18, -20, t, OCC_T), (-18, -20, t - 1, FREE_T)])


# ---- (b) surfaces: heights as integer functions of the cell, q forced by the pair (0.0, QB[q]) at THRES: r = 4 / QB[q] lies within 0.1 % of q + 0.5
QB = [np.float16(4.0 / (q + 0.5)) for q in range(16)]
assert all(int(16.0 * 0.25 / float(b)) == q and float(b) >= THRES for q, b in enumerate(QB))


def surface(heights):
    """{(i, j): height in sixteenths of a voxel} -> a scene with one occupied voxel and the free one above it per column: it stands with free_run <= 1 and
    any clearance, for the column holds nothing else"""
    parts = []
    for (i, j), h in heights.items():
        k, q = h >> 4, h & 15
        parts += [(i, j, k, OCC_T), (i, j, k + 1, float(QB[q]))]
    return _cells(parts)


PLANE_A, PLANE_B, PLANE_HALF = 1, 2, 8                   # height = 16 * (a i + b j) / 4 over -8 <= i, j <= 8


def plane_heights():
    return {(i, j): 4 * (PLANE_A * i + PLANE_B * j) for i in range(-PLANE_HALF, PLANE_HALF + 1) for j in range(-PLANE_HALF, PLANE_HALF + 1)}


def plane_slope2(s):
    """closed form: gx = 8 s * 4 a, gy = 8 s * 4 b"""
    return (32 * s * PLANE_A) ** 2 + (32 * s * PLANE_B) ** 2


def plane_step(w):
    """in the interior: 2 w * 4 * (|a| + |b|)"""
    return 8 * w * (abs(PLANE_A) + abs(PLANE_B))


CLIFF_LOW, CLIFF_HIGH = 16 * 2, 16 * 5 + 5


def cliff_heights(geo):
    """in the geometry's own indices: a cliff along i and one along j across the tile border 31 | 32 of the window kernel (unsigned cells 26 .. 37), and one
    in each of two opposite corners of the grid"""
    N = GEOMETRIES[geo]["N"]
    out = {}
    for ui in range(26, 38):
        for uj in range(26, 38):
            out[(ui - N // 2, uj - N // 2)] = CLIFF_HIGH if (ui >= 32) != (uj >= 32) else CLIFF_LOW
    for c in range(4):
        for d in range(4):
            out[(c - N // 2, d - N // 2)] = CLIFF_HIGH if c >= 1 else CLIFF_LOW
            out[(N // 2 - 1 - c, N // 2 - 1 - d)] = CLIFF_HIGH if d >= 2 else CLIFF_LOW
    return out


HOLE_HALF = 5


def hole_heights():
    """a flat 11 x 11 patch with its centre cell missing"""
    return {(i, j): 16 * 3 + 4 for i in range(-HOLE_HALF, HOLE_HALF + 1) for j in range(-HOLE_HALF, HOLE_HALF + 1) if (i, j) != (0, 0)}


# the order of the class tests (window 1, slope_base 1): cells on each side of each limit.  name -> (cell, step, nsup, slope2 or None = no valid stencil)
LIMIT_D = 5
LIMIT_CELLS = {"FLAT": ((-8, -8), 0, 9, 0),                            # the centre of a flat 3 x 3 patch
               "CORNER": ((0, -8), LIMIT_D, 9, 2 * LIMIT_D * LIMIT_D),  # ... of one whose (+1, +1) corner is LIMIT_D higher: gx = gy = LIMIT_D
               "LONE": ((8, -8), 0, 1, None),                           # a single cell
               "PAIR": ((-8, 0), LIMIT_D, 2, None)}                     # two cells LIMIT_D apart in height
LIMIT_SETS = [(65534, 0xffffffff, 1), (LIMIT_D, 2 * LIMIT_D * LIMIT_D, 1), (LIMIT_D - 1, 0xffffffff, 1), (LIMIT_D, 2 * LIMIT_D * LIMIT_D - 1, 1), (65534, 0xffffffff, 2),
              (65534, 0xffffffff, 3), (LIMIT_D - 1, 0xffffffff, 10), (LIMIT_D, 2 * LIMIT_D * LIMIT_D - 1, 10), (65534, 0xffffffff, 10), (0, 0, 0)]


def limit_heights():
    out = {}
    for (ci, cj) in (LIMIT_CELLS["FLAT"][0], LIMIT_CELLS["CORNER"][0]):
        for a in (-1, 0, 1):
            for b in (-1, 0, 1):
                out[(ci + a, cj + b)] = 0
    ci, cj = LIMIT_CELLS["CORNER"][0]
    out[(ci + 1, cj + 1)] = LIMIT_D
    out[LIMIT_CELLS["LONE"][0]] = 0
    ci, cj = LIMIT_CELLS["PAIR"][0]
    out[(ci, cj)], out[(ci + 1, cj)] = 0, LIMIT_D
    return out


def limit_classes(max_step, max_slope2, min_support):
    """the classes of the LIMIT_CELLS worked out from the definition (0 free, 1 occupied, 2 unknown), in the order of LIMIT_CELLS"""
    out = []
    for _, step, nsup, slope2 in LIMIT_CELLS.values():
        out.append(1 if step > max_step else 1 if slope2 is not None and slope2 > max_slope2 else 2 if nsup < min_support else 0)
    return out


# ---- (c) a ramp beside a cliff of the same rise, joining a floor to a platform (scene coordinates; heights in sixteenths)
RAMP_I, RAMP_J, CLIFF_J = (0, 11), (-8, -1), (0, 7)       # the ramp's cells; the cliff's strip beside it
FLOOR_I, PLATFORM_I = (-12, -1), (12, 23)
RAMP_RISE = 96                                            # 6 voxels over 12 cells: 8 sixteenths per cell, tan = 0.5, 26.6 degrees
RAMP_START, RAMP_GOAL = (-6, -4), (18, -4)


def ramp_heights():
    out = {}
    for j in range(RAMP_J[0], CLIFF_J[1] + 1):
        for i in range(FLOOR_I[0], FLOOR_I[1] + 1):
            out[(i, j)] = 0
        for i in range(PLATFORM_I[0], PLATFORM_I[1] + 1):
            out[(i, j)] = RAMP_RISE
        for i in range(RAMP_I[0], RAMP_I[1] + 1):
            out[(i, j)] = 8 * (i + 1) if j <= RAMP_J[1] else (0 if i <= 5 else RAMP_RISE)
    return out
