"""Hand-built volumes for the ESDF tests (tests/test_esdf_scenes_cpu.py, tests/test_esdf_scenes_gpu.py): each is the smallest shape that exercises one claim of
csrc/tsl_esdf.hip which a room seen from inside never does.  A scene is a dictionary of load_numpy / import_sparse arrays as in tests/frontier_scenes.py (box,
scene, place and load_pair come from there), built in brick-local coordinates around index (0, 0, 0), the corner where eight bricks meet.  Every listed voxel
is observed, the unlisted voxels of an allocated brick are unobserved, a brick without a listed voxel is absent.  PARAMS has each scene's gamma / max_dist
(gamma None: the voxel size), PLACED the scenes that also run through place() on SLAB and TALL.  Below that: the depth frames and the maps of the two
incremental cases."""
import numpy as np

import frontier_scenes as _fs
from frontier_scenes import GEOMETRIES as _FS_GEOMETRIES, box, load_pair, scene      # noqa: F401  (load_pair: for the tests)
from util import SMALL, lin

# exact arithmetic: N = 256, the voxel size is a power of two (exact in f16 and f32), axis steps add exactly and gamma = vs has an exact f16 neighbour below it
EXACT = dict(SMALL, voxel_scale=0.0625, map_scale=[16.0, 16.0])
GEOMETRIES = dict(_FS_GEOMETRIES, EXACT=dict(cfg=EXACT, N=256, Nz=256, o=(0, 0, 0), swap=False))
VS = 0.0625
FREE_T = 0.5
BELOW_VS = float(np.nextafter(np.float16(VS), np.float16(0)))          # 0.06246948: the largest f16 below the voxel size


def place(sc, geo):
    """frontier_scenes.place(); on EXACT the scene stays where it was built, and only the fit is asserted"""
    if geo != "EXACT":
        return _fs.place(sc, geo)
    idx = sc["indices"].astype(np.int64)
    assert (idx >= -128).all() and (idx < 128).all(), "the scene does not fit EXACT"
    return sc


def layered(parts):
    """scene() of parts that may overlap: a later part replaces the voxels it shares with an earlier one"""
    keep, seen = [], np.zeros(0, np.int64)
    for vox, v in reversed(parts):
        vox = np.asarray(vox, np.int64).reshape(-1, 3)
        key = lin(vox)
        new = ~np.isin(key, seen)
        seen = np.concatenate([seen, key[new]])
        if new.any():
            keep.append((vox[new], v))
    return scene(keep[::-1])


def shift(sc, d):
    return dict(sc, indices=(sc["indices"].astype(np.int64) + np.asarray(d, np.int64)).astype(np.int16))


def values_at(idx, val, voxels):
    """the values of an ESDF export (idx int16 [n, 3], val f32 [n]) at `voxels` [m, 3]; raises when one is not in the export"""
    key, want = lin(np.asarray(idx)), lin(np.asarray(voxels, np.int64).reshape(-1, 3))
    o = np.argsort(key)
    at = np.searchsorted(key[o], want)
    if (at >= key.size).any() or (key[o][np.minimum(at, key.size - 1)] != want).any():
        raise KeyError("a voxel is not in the export")
    return np.asarray(val, np.float32)[o][at]


# ---- 1. a value that reaches a brick through a corner, through an edge; one band voxel in the middle of 27 bricks ------------------------------------
def corner_only():
    """two fully observed bricks that meet in one corner, the band voxel in the far corner of the first: everything the second brick holds came through the
    voxel pair (-1, -1, -1) - (0, 0, 0), and no face or edge neighbour exists that could deliver it as well"""
    return layered([(box((-16, -16, -16), (-1, -1, -1)), FREE_T), (box((0, 0, 0), (15, 15, 15)), FREE_T), ([(-16, -16, -16)], 0.03)])


def edge_only():
    """the same with bricks (-1, -1, 0) and (0, 0, 0), which share the edge along z"""
    return layered([(box((-16, -16, 0), (-1, -1, 15)), FREE_T), (box((0, 0, 0), (15, 15, 15)), FREE_T), ([(-16, -16, 0)], 0.03)])


def late(kind, near=True):
    """A brick that is visited a second time because of a diagonal neighbour alone.  Q = brick (0, 0, 0) gets its first values through a face, from a band
    voxel at the far side of its +x neighbour; the brick P that touches Q in one corner (kind "corner": (-1, -1, -1)) or along one edge ("edge": (-1, -1, 0))
    holds no band voxel and is fed through a face by its -x neighbour, so it is relaxed one round later than Q's first visit, and its values -- lower near
    the corner than what came through the face -- reach Q in a visit whose only notified neighbour is P: the sweeps that enter there run behind their entry check"""
    z0 = -16 if kind == "corner" else 0
    src = (-17, -1, -1) if kind == "corner" else (-17, -1, 8)
    return layered([(box((-32, -16, z0), (-1, -1, z0 + 15)), FREE_T), (box((0, 0, 0), (31, 15, 15)), FREE_T), ([src], 0.0 if near else FREE_T), ([LATE_FAR], 0.0)])


LATE_FAR = (31, 8, 8)


def late_corner():
    return late("corner")


def late_edge():
    return late("edge")


CUBE27_LO, CUBE27_HI, CUBE27_BAND = -16, 31, (-1, -1, -1)


def cube27():
    """48^3 observed voxels, 27 whole bricks, one band voxel t = 0 in the top corner of the lowest brick (at the corner where eight bricks meet): along each axis
    through it the value is n * vs exactly"""
    return layered([(box((CUBE27_LO,) * 3, (CUBE27_HI,) * 3), FREE_T), ([CUBE27_BAND], 0.0)])


def cube27_at_volume_corner(geo="EXACT"):
    """cube27 moved so that the band voxel's brick is the brick of the volume with the lowest index on all three axes: 19 of its 26 neighbour bricks lie outside"""
    g = GEOMETRIES[geo]
    return shift(cube27(), (-(g["N"] // 2) - CUBE27_LO, -(g["N"] // 2) - CUBE27_LO, -(g["Nz"] // 2) - CUBE27_LO))


# ---- 2. a one-voxel corridor through unobserved space that crosses one brick face again and again -----------------------------------------------------
def zigzag_cells(n=64):
    """int64 [n, 3]: the corridor in order, in the layer z = 0: two cells at x = 0, two at x = -1, ..."""
    y = np.arange(n) - 32
    return np.stack([np.where((y + 32) % 4 < 2, 0, -1), y, np.zeros(n, np.int64)], 1).astype(np.int64)


def zigzag_crossings(cells):
    """how often consecutive cells lie in different bricks along x"""
    return int((np.diff(cells[:, 0] // 16) != 0).sum())


def zigzag():
    c = zigzag_cells()
    return layered([(c, FREE_T), (c[:1], 0.0)])


# ---- 3. a closed negative pocket without a band voxel of its own ---------------------------------------------------------------------------------------
POCKET = box((-2, -2, -2), (1, 1, 1))


def pocket():
    return layered([(box((-8, -8, -8), (7, 7, 7)), FREE_T), (POCKET, -FREE_T), ([(-8, -8, -8)], 0.01)])


# ---- 4. signs that alternate voxel by voxel --------------------------------------------------------------------------------------------------------------
CHECKER_POS_BAND, CHECKER_NEG_BAND = (16, 16, 16), (-1, -1, -1)          # an even voxel and an odd one, in opposite corners


def checker_signs():
    """one brick and a one-voxel shell into its 26 neighbours, +0.5 where i + j + k is even and -0.5 where it is odd: voxels of one side touch only across
    edge diagonals, so either side propagates in sqrt(2) steps alone, and every plane of every sweep holds both signs"""
    v = box((-1, -1, -1), (16, 16, 16))
    even = v.sum(1) % 2 == 0
    return layered([(v[even], FREE_T), (v[~even], -FREE_T), ([CHECKER_POS_BAND], 0.02), ([CHECKER_NEG_BAND], -0.02)])


# ---- 5. the edges of the band and of max_dist: rows along x across the brick face x = -1 | 0 ------------------------------------------------------------
def row(values, x0=-2):
    return layered([([(x0 + n, 0, 0)], float(v)) for n, v in enumerate(values)])


def row_voxels(n, x0=-2):
    return np.array([(x0 + a, 0, 0) for a in range(n)], np.int64)


BAND_ROWS = {
    # |t| < gamma is strict: t = vs is relaxed, the f16 value below it is kept
    "band_strict": dict(values=[VS, BELOW_VS, FREE_T, FREE_T], want=[BELOW_VS + VS, BELOW_VS, BELOW_VS + VS, BELOW_VS + 2 * VS]),      # 0.12496948, 0.06246948, 0.12496948, 0.18746948
    # -0.0 is a band value, leaves as -0.0 and lies on the positive side: it feeds the positive neighbour, not the negative one
    "neg_zero": dict(values=[-FREE_T, -0.0, FREE_T], want=[-5.0, -0.0, VS]),
    # value + edge < max_dist is strict (and so is candidate < value): four axis steps from a band value 0 is max_dist itself
    "maxdist_strict": dict(values=[0.0, FREE_T, FREE_T, FREE_T, FREE_T, FREE_T], want=[0.0, 0.0625, 0.125, 0.1875, 0.25, 0.25], max_dist=0.25),
    # max_dist below the voxel size: nothing is lowered
    "maxdist_below_vs": dict(values=[-FREE_T, -FREE_T, 0.0, FREE_T, FREE_T], want=[-0.01, -0.01, 0.0, 0.01, 0.01], max_dist=0.01),
    # gamma above max_dist: band voxels above max_dist keep their TSDF, and the lowering from a small band value stops at max_dist before it reaches them
    "wide_gamma": dict(values=[0.25, 1.0, 1.0, 1.0, 1.0, 1.0, 0.75, 0.75, -0.75, -1.0], want=[0.25, 0.3125, 0.375, 0.4375, 0.5, 0.5, 0.75, 0.75, -0.75, -0.5],
                       gamma=1.0, max_dist=0.5),
    # gamma above the voxel size: a band voxel that is offered less than |t| (0 + vs < 0.75) stays what it is, and its neighbours get |t| + edge from it, not
    # what it was offered + edge
    "band_relay": dict(values=[1.0, 0.0, 0.75, 1.0, 1.0], want=[VS, 0.0, 0.75, 0.75 + VS, 0.75 + 2 * VS], gamma=1.0),
}


# ---- 6. bricks farther than max_dist from every band voxel -----------------------------------------------------------------------------------------------
FAR_POS, FAR_NEG = box((48, 0, 0), (63, 15, 15)), box((-64, 0, 0), (-49, 15, 15))


def far_brick():
    """corner_only and two fully observed bricks without a band voxel, one at +0.5 and one at -0.5, two bricks away from anything: with max_dist = 1.0 (one
    brick) no value reaches them, and the wavefront of esdf_mode 1 never visits them"""
    c = corner_only()
    far = scene([(FAR_POS, FREE_T), (FAR_NEG, -FREE_T)])
    return {k: np.concatenate([c[k], far[k]]) for k in c}


# ---- 7. another submap in the same bricks ----------------------------------------------------------------------------------------------------------------
def other_submap_wall():
    """for submap 0: a band wall through both bricks of corner_only, next to its voxels on either side of the corner, and free space around it"""
    return layered([(box((-16, -16, -16), (15, 15, 15)), FREE_T), (box((-16, -16, -2), (15, 15, 1)), 0.0)])


def _rows(name):
    return lambda: row(BAND_ROWS[name]["values"])


SCENES = dict({"corner_only": corner_only, "edge_only": edge_only, "late_corner": late_corner, "late_edge": late_edge, "cube27": cube27,
               "cube27_corner": cube27_at_volume_corner, "zigzag": zigzag, "pocket": pocket, "checker_signs": checker_signs, "far_brick": far_brick},
              **{k: _rows(k) for k in BAND_ROWS})
PARAMS = dict({k: {} for k in SCENES}, pocket=dict(max_dist=2.0), far_brick=dict(max_dist=1.0),
              **{k: {p: v[p] for p in ("gamma", "max_dist") if p in v} for k, v in BAND_ROWS.items()})
ORDER = ["pocket"] + [k for k in SCENES if k != "pocket"]          # pocket first: the scenes after it reuse its bricks
PLACED = ["corner_only", "edge_only", "late_corner", "late_edge", "cube27", "zigzag", "checker_signs"]          # scenes 1, 2 and 4 on SLAB and TALL


def params(name):
    """(gamma or None, max_dist) of a scene"""
    p = PARAMS[name]
    return p.get("gamma"), p.get("max_dist", 5.0)


def placed(name, geo):
    """the scene on SLAB or TALL.  cube27 is as high as SLAB (48 voxels): it is moved down by one brick first and fills the volume from floor to ceiling, and
    so is checker_signs, whose shell would stick out of the ceiling by one voxel"""
    sc = SCENES[name]()
    if name in ("cube27", "checker_signs") and geo == "SLAB":
        sc = shift(sc, (0, 0, -16))
    return place(sc, geo)


# ---- the incremental cases --------------------------------------------------------------------------------------------------------------------------------
def ball_depth(R, T, base, centre, rad, K=None):
    """the depth image `base` (uint16 millimetres, camera pose R, T, intrinsics K: the 640 x 480 ones by default) with a ball in front of it"""
    from taichislam_amd.utils import synthetic as syn
    K = syn.K_DEPTH if K is None else np.asarray(K, np.float64).reshape(-1)
    fx, fy, cx, cy = K[0], K[4], K[2], K[5]
    h, w = base.shape
    ii, jj = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    d = np.stack([(ii - cx) / fx, (jj - cy) / fy, np.ones_like(ii)], axis=-1) @ R.T
    oc = T - centre
    a = (d * d).sum(-1); b = 2.0 * (d @ oc); c = float(oc @ oc) - rad * rad
    disc = b * b - 4 * a * c
    t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
    mm = np.where((t > 0) & np.isfinite(t), np.rint(1000.0 * t), 65535.0)
    return np.minimum(base.astype(np.float64), mm).astype(np.uint16)


BALL_WARM, BALL_MOVING, BALL_AFTER, BALL_MAX_DIST = 3, 6, 3, 0.8
BALL_ORACLE_FRAMES = (BALL_WARM + 1, BALL_WARM + BALL_MOVING + BALL_AFTER - 1)          # the second frame with the ball (the most band voxels around it), the last frame


def vanishing_ball(h=120, w=160):
    """(K, R, T, [depth]): a static camera in the sphere room; three frames of the room, six with a ball of radius 0.15 m, 1.5 m ahead, that moves 0.12 m per
    frame across the view, three of the room again -- band voxels appear in free space, move on and vanish: values around them must RISE"""
    from taichislam_amd.utils import synthetic as syn
    K = syn.scaled_intrinsics(h, w)
    R, T = syn.camera_pose(0)
    base = syn.sphere_room_depth(R, T, h, w, radius=3.0, K=K)
    fwd, right = R @ np.array([0.0, 0.0, 1.0]), R @ np.array([1.0, 0.0, 0.0])
    ball = [ball_depth(R, T, base, T + 1.5 * fwd + (0.12 * f - 0.3) * right, 0.15, K=K) for f in range(BALL_MOVING)]
    return K, R, T, [base] * BALL_WARM + ball + [base] * BALL_AFTER


EDIT_MAX_DIST = 0.5          # 12.5 voxels of SMALL: the dilation of esdf_mode 0 reaches one brick


def edit_block():
    """on SMALL: 5 x 5 x 5 whole bricks of free space, the face x = -32 a band plane"""
    return layered([(box((-32, -32, -32), (47, 47, 47)), FREE_T), (box((-32, -32, -32), (-32, 47, 47)), 0.0)])


def edit_points():
    """(R, T, xyz f32 [n, 3] in the sensor's frame): a sensor inside the block that sees a small patch of surface at x = 1.45 m, next to the face opposite
    the band plane"""
    y, z = np.meshgrid(np.linspace(-0.1, 0.1, 11), np.linspace(-0.1, 0.1, 11))
    xyz = np.stack([np.full(y.size, 0.55), y.ravel(), z.ravel()], 1).astype(np.float32)
    return np.eye(3), np.array([0.9, 0.02, 0.02]), xyz
