"""Hand-built maps for the Gauss-Newton family (align_linearize, align_points_linearize, register_linearize, register_score) at its limits, shared by
tests/test_gn_limits_cpu.py and tests/test_gn_limits_gpu.py.  A map is an index list with f16 values (and weights): DenseTSDF.load_numpy takes it on
the GPU, grid() turns it into the restatements' dense grid.  Every scene carries an expectation that does not come from the restatements: Python
sets of the listed voxels, the stored bit patterns, or a few f32 operations written out.

A  one stored value that is not finite (or 65504) inside a ramp            B  a steep checkerboard: addends beyond 2^31, sums beyond 2^53
C  one input on every gate's boundary and one a step past it               D  cells over brick seams and at the volume's walls"""
import functools
import itertools

import numpy as np

import render_view_ref as rv
from util import SLAB, SMALL, TALL

F32 = np.float32
F16 = np.float16
VS = F32(SMALL["voxel_scale"])
GEOS = dict(SMALL=dict(SMALL, max_bricks=4096), SLAB=dict(SLAB), TALL=dict(TALL))
USED, GATE, UNKNOWN, FAR, GRAD = 0, 1, 2, 3, 4
EYE, ZERO = np.eye(3), np.zeros(3)
OPEN = dict(d_min=1e-3, d_max=100.0)                      # a range gate that gates nothing of these scenes
SHIFT = np.array([0.3, 0.4, 0.6]) * float(VS)             # no rotation and this translation: source voxel i lands in the destination cell with base i
INT64_MIN = -2 ** 63


def dims(geo):
    """(N, Nz, lo int [3], hi int [3]): the voxel indices of the volume are lo .. hi - 1"""
    c = GEOS[geo]
    N, Nz = int(round(c["map_scale"][0] / c["voxel_scale"])), int(round(c["map_scale"][1] / c["voxel_scale"]))
    lo = np.array([-(N // 2), -(N // 2), -(Nz // 2)])
    return N, Nz, lo, lo + np.array([N, N, Nz])


def grid(geo, m):
    """the restatements' (val, known, lo) of a map"""
    N, Nz, _, _ = dims(geo)
    return rv.grid_from_export(m["indices"], m["TSDF"], N, Nz)


def make_map(idx, t, w=None):
    """indices int16 [n, 3], TSDF f16 [n], W_TSDF f16 [n] (1 unless given), occupy int8 [n]; t and w may be uint16 bit patterns"""
    idx = np.ascontiguousarray(np.asarray(idx).reshape(-1, 3).astype(np.int16))
    n = idx.shape[0]
    t = np.asarray(t)
    t = t.view(F16) if t.dtype == np.uint16 else t.astype(F16)
    w = np.ones(n, F16) if w is None else (np.asarray(w).view(F16) if np.asarray(w).dtype == np.uint16 else np.asarray(w).astype(F16))
    return dict(indices=idx, TSDF=np.ascontiguousarray(t.reshape(n)), W_TSDF=np.ascontiguousarray(w.reshape(n)), occupy=np.zeros(n, np.int8))


def without(m, drop):
    """the map without the voxels where `drop` (bool [n]) holds"""
    keep = ~np.asarray(drop, bool)
    return dict(indices=m["indices"][keep], TSDF=m["TSDF"][keep], W_TSDF=m["W_TSDF"][keep], occupy=m["occupy"][keep])


def union(*maps):
    return {k: np.concatenate([m[k] for m in maps]) for k in ("indices", "TSDF", "W_TSDF", "occupy")}


def box(lo, hi):
    """int [n, 3]: every voxel index of lo .. hi (inclusive, per axis)"""
    lo, hi = np.broadcast_to(lo, (3,)), np.broadcast_to(hi, (3,))
    return np.stack(np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)


def listed(m):
    return set(map(tuple, np.asarray(m["indices"], np.int64).tolist()))


def cell_known(base, voxels):
    """all 8 corners of the cell with base voxel `base` are listed (a voxel outside the volume never is)"""
    return all((base[0] + d[0], base[1] + d[1], base[2] + d[2]) in voxels for d in itertools.product((0, 1), repeat=3))


def cell_of(p):
    """the cell base of f32 coordinates: floor(p / VS) with the quotient formed in f32, as every sampler forms it"""
    return np.floor(np.asarray(p, F32) / VS).astype(np.int64)


def first_in(b):
    """the least f32 coordinate of the cell with base b: the least p with p / VS >= b in f32"""
    p = F32(b) * VS
    while p / VS >= F32(b):
        p = np.nextafter(p, F32(-np.inf))
    while p / VS < F32(b):
        p = np.nextafter(p, F32(np.inf))
    return p


def exact(b):
    """the f32 coordinate p with p / VS == b: cell b at fraction 0.  Not every integer has one (30 and 27 have none at this voxel size); the scenes
    are placed where it exists"""
    p = first_in(b)
    assert p / VS == F32(b), f"no f32 coordinate lies exactly on voxel {b}"
    return p


def last_in(b):
    """the greatest f32 coordinate of the cell with base b: the f32 below first_in(b + 1)"""
    return np.nextafter(first_in(b + 1), F32(-np.inf))


def inside(b, f=0.37):
    return (F32(b) + F32(f)) * VS


def cell_coordinates(b):
    """three coordinates in the cell with base b: fraction 0, an interior fraction, the last f32 below the next voxel"""
    return [exact(b), inside(b), last_in(b)]


def probes(bases):
    """(p f32 [n * 27, 3], base int [n * 27, 3]): 27 points in each cell, every combination of cell_coordinates per axis"""
    p, bb = [], []
    for b in np.asarray(bases).reshape(-1, 3).tolist():
        for q in itertools.product(*[cell_coordinates(b[a]) for a in range(3)]):
            p.append(q)
            bb.append(b)
    p, bb = np.array(p, F32), np.array(bb, np.int64)
    assert np.array_equal(cell_of(p), bb)
    return p, bb


def ramp(idx, origin, slope=(0.013, 0.021, 0.034), offset=-0.1):
    d = (np.asarray(idx) - np.asarray(origin)).astype(np.float64)
    return (offset + d @ np.asarray(slope)).astype(F16)


# ---- A: a stored value that is not finite -------------------------------------------------------------------------------------------------------------
# a 6^3 block of SMALL that crosses a brick face in x (voxel 47, the special one's, is the last of its brick), a ramp of -0.1 .. 0.24 with a gradient of about 1 per
# metre: with the default gates every finite sample is used.  The special voxel lies at offset (2, 3, 2): the 8 cells around it are tainted.
SPECIALS = dict(nan=0x7e00, pinf=0x7c00, ninf=0xfc00, max=0x7bff)      # f16 bit patterns: a quiet NaN, +inf, -inf, 65504
A_ORIGIN = np.array([45, -40, 10])
A_SPECIAL = A_ORIGIN + np.array([2, 3, 2])
A_CLEAN_CELLS = np.array([[0, 0, 0], [4, 4, 4], [3, 1, 0], [0, 4, 3]])
A_WEIGHT_VOXEL = A_ORIGIN + np.array([1, 1, 1])            # the source voxel that carries a NaN weight


def a_block():
    return box(A_ORIGIN, A_ORIGIN + 5)


def a_map(kind=None):
    """the block; kind: the key of SPECIALS stored at A_SPECIAL, None = the plain ramp"""
    idx = a_block()
    t = ramp(idx, A_ORIGIN).view(np.uint16).copy()
    if kind is not None:
        t[(idx == A_SPECIAL).all(1)] = SPECIALS[kind]
    return make_map(idx, t)


def a_tainted(base):
    """bool [n]: the cell with this base has A_SPECIAL among its corners"""
    d = A_SPECIAL - np.asarray(base)
    return ((d >= 0) & (d <= 1)).all(1)


@functools.lru_cache(maxsize=None)
def a_probes():
    """(p, base, tainted): 27 points in each of the 8 cells around A_SPECIAL and in 4 cells away from it"""
    around = A_SPECIAL - np.array(list(itertools.product((0, 1), repeat=3)))
    p, base = probes(np.concatenate([around, A_ORIGIN + A_CLEAN_CELLS]))
    return p, base, a_tainted(base)


A_K = np.array([250.0, 0, 31.5, 0, 250.0, 23.5, 0, 0, 1.0])
A_T = (A_ORIGIN + 2.5) * float(VS) - np.array([0.0, 0.0, 1.0])


@functools.lru_cache(maxsize=None)
def a_image():
    """uint16 [48, 64]: seen from A_T along +z with A_K, the pixels fall into the block's cells (4 mm per pixel, depths of 0.91 .. 1.09 m) and a
    few beside it"""
    d = np.random.default_rng(5).integers(910, 1090, (48, 64)).astype(np.uint16)
    d.setflags(write=False)
    return d


def image_points(depth, K, T):
    """(p f32 [h * w, 3], cell base int [h * w, 3]) of a depth image at the pose (identity, T), with the f32 expressions of the image kernel"""
    h, w = depth.shape
    fx, fy, cx, cy = (F32(K[i]) for i in (0, 4, 2, 5))
    T = np.asarray(T, np.float64).astype(F32)
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    dep = depth.ravel().astype(F32) / F32(1000.0)
    p = np.stack([(ii.ravel().astype(F32) - cx) * dep / fx + T[0], (jj.ravel().astype(F32) - cy) * dep / fy + T[1], dep + T[2]], 1).astype(F32)
    return p, cell_of(p)


def a_source(kind=None):
    """a source whose voxel i lands in the block's cell i at (identity, SHIFT): the 5^3 voxels that are cell bases, values within +-0.03.  kind: that
    special value at A_SPECIAL and a NaN weight at A_WEIGHT_VOXEL"""
    idx = box(A_ORIGIN, A_ORIGIN + 4)
    d = idx - A_ORIGIN
    t = (0.01 * ((d[:, 0] + 2 * d[:, 1] + 3 * d[:, 2]) % 7 - 3)).astype(F16).view(np.uint16).copy()
    w = np.ones(idx.shape[0], F16).view(np.uint16).copy()
    if kind is not None:
        t[(idx == A_SPECIAL).all(1)] = SPECIALS[kind]
        w[(idx == A_WEIGHT_VOXEL).all(1)] = SPECIALS["nan"]
    return make_map(idx, t, w)


# ---- B: magnitudes ------------------------------------------------------------------------------------------------------------------------------------
# SMALL, a 24^3 block at voxels 100 .. 123 with +-8 in a checkerboard: gradients of up to 400 per metre and axis at 4 .. 4.9 m from the origin.
B_LO, B_HI = 100, 123
B_GATES = dict(r_max=16.0, g_max=1024.0)
B_POINT_GATES = dict(OPEN, **B_GATES)
B_IMAGE_GATES = dict(d_min=0.3, d_max=5.0, **B_GATES)
B_K = np.array([200.0, 0, 79.5, 0, 200.0, 59.5, 0, 0, 1.0])
B_T = np.array([4.46, 4.46, 3.5])
# the 21 + 6 + 1 slots; the sign of an off-diagonal H entry and of a b entry is free, a diagonal entry and e are squares
B_DIAGONAL = [0, 6, 11, 15, 18, 20]
B_FREE_SIGN = [k for k in range(27) if k not in B_DIAGONAL]


@functools.lru_cache(maxsize=None)
def b_map():
    idx = box(B_LO, B_HI)
    return make_map(idx, np.where(idx.sum(1) % 2 == 0, 8.0, -8.0))


@functools.lru_cache(maxsize=None)
def b_points():
    """f32 [32768, 3]: uniform inside the block"""
    p = (np.random.default_rng(1).uniform(B_LO, B_HI, (32768, 3)) * float(VS)).astype(F32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def b_image():
    """uint16 [120, 160]: seen from B_T along +z with B_K, every pixel lies inside the block, 0.52 .. 1.1 m away"""
    d = np.random.default_rng(2).integers(520, 1100, (120, 160)).astype(np.uint16)
    d.setflags(write=False)
    return d


# With r_max = 16 the block cannot fill the last slot: e = s^2 <= 256 is at most 2^28 in fixed point.  Two gentle blocks around +100 and -100 (f16
# steps of 1/16 there; a gradient of some 6 per metre) under r_max = 128 do: s^2 is about 10^4, 2^33 in fixed point.
B_E_ORIGINS = (np.array([29, -30, 10]), np.array([45, -30, 10]))
B_E_GATES = dict(OPEN, r_max=128.0, g_max=8.0)


@functools.lru_cache(maxsize=None)
def b_e_map():
    idx = [box(o, o + 5) for o in B_E_ORIGINS]
    return make_map(np.concatenate(idx), np.concatenate([ramp(idx[0], B_E_ORIGINS[0], (0.0625, 0.125, 0.1875), 100.0),
                                                         ramp(idx[1], B_E_ORIGINS[1], (0.0625, 0.125, 0.1875), -102.0)]))


@functools.lru_cache(maxsize=None)
def b_e_points():
    """f32 [600, 3]: uniform inside the two blocks"""
    u = np.random.default_rng(6).uniform(0.0, 5.0, (600, 3))
    u[:300] += B_E_ORIGINS[0]
    u[300:] += B_E_ORIGINS[1]
    p = (u * float(VS)).astype(F32)
    p.setflags(write=False)
    return p


# the registration: register_check bounds max(2 L g_max, r_max + band)^2 2^20 by 2^62 / (4096 bricks of 4096 voxels) = 2^38: M <= 512.  g_max = 48
# gives 2 L g_max = 491.52, r_max + band = 500.  The destination holds uniform values of +-1.5 (gradients of some 16 per metre and axis, a few
# beyond g_max), the source 2^3 whole bricks with values of up to +-240: the residual is the source's value, far past the default band of 0.08.
B_REG_GATES = dict(w_min=0.0, band=250.0, r_max=250.0, g_max=48.0)
# |g_a g_b| <= (g_a^2 + g_b^2) / 2 <= g_max^2 / 2 = 1152 < 2048 for a != b, and g_a^2 >= 2048 needs 94 % of g_max on one axis: under M <= 512 the six
# products of two gradient components stay below 2^31; every other slot holds a moment arm (p x g, |p| about 3 m), or the residual
B_REG_SMALL_SLOTS = [0, 1, 2, 6, 7, 11]


@functools.lru_cache(maxsize=None)
def b_reg_destination():
    idx = box(63, 97)
    return make_map(idx, np.random.default_rng(4).uniform(-1.5, 1.5, idx.shape[0]))


@functools.lru_cache(maxsize=None)
def b_reg_source():
    idx = box(64, 95)
    return make_map(idx, np.random.default_rng(3).uniform(-240.0, 240.0, idx.shape[0]))


# ---- C: the gates' equalities -------------------------------------------------------------------------------------------------------------------------
# a block whose value rises by 0.03 per voxel along x only: in the cell C_CELL the gradient is (g0, 0, 0) at every fraction, and at fraction 0 the
# interpolant is the stored value itself.  Beside it a block of one constant value: a flat cell.
C_ORIGIN = np.array([40, -30, 10])
C_CELL = C_ORIGIN + np.array([3, 2, 2])
C_FLAT = np.array([60, -30, 10])


@functools.lru_cache(maxsize=None)
def c_map():
    idx, flat = box(C_ORIGIN, C_ORIGIN + 5), box(C_FLAT, C_FLAT + 2)
    return make_map(np.concatenate([idx, flat]), np.concatenate([ramp(idx, C_ORIGIN, (0.03, 0.0, 0.0), -0.06), np.full(flat.shape[0], 0.05, F16)]))


def c_stored(voxel):
    m = c_map()
    return F32(m["TSDF"][(m["indices"] == np.asarray(voxel)).all(1)][0])


def c_facts():
    """v: the stored value at C_CELL (the interpolant at fraction 0); g0: the gradient per metre along x in that cell, from the two stored values"""
    v = c_stored(C_CELL)
    g0 = (c_stored(C_CELL + np.array([1, 0, 0])) - v) / VS
    assert v > 0 and g0 > 0
    return v, g0


def c_corner_point():
    return np.array([[exact(x) for x in C_CELL]], F32)


def c_interior_point():
    return np.array([[inside(x) for x in C_CELL]], F32)


def c_flat_point():
    return np.array([[inside(x) for x in C_FLAT]], F32)


def c_range_points(d_min, d_max):
    """f32 [4, 3] on the x axis: at d_max, one f32 beyond it, at d_min, one f32 short of it -- and the squares say so"""
    lo, hi = F32(d_min), F32(d_max)
    x = np.array([hi, np.nextafter(hi, F32(np.inf)), lo, np.nextafter(lo, F32(0))], F32)
    assert x[0] * x[0] == hi * hi and x[1] * x[1] > hi * hi and x[2] * x[2] == lo * lo and x[3] * x[3] < lo * lo
    return np.stack([x, np.zeros(4, F32), np.zeros(4, F32)], 1)


def fixed(x):
    """rint(x 2^20) of one f32 as a Python integer"""
    return int(np.rint(np.float64(F32(x)) * 2.0 ** 20))


def c_huber_case():
    """(map, p f32 [1, 3], v, g): the blocks of b_e_map (values near 100: a weight one f32 below 1 shows in e = v^2 2^20) and a point at fraction 0
    of a cell, where the interpolant is the stored value v and the gradient per metre the three differences to the next voxels"""
    m = b_e_map()
    cell = B_E_ORIGINS[0] + 2
    val = lambda voxel: F32(m["TSDF"][(m["indices"] == voxel).all(1)][0])
    v = val(cell)
    g = [(val(cell + np.eye(3, dtype=np.int64)[a]) - v) / VS for a in range(3)]
    return m, np.array([[exact(x) for x in cell]], F32), v, g


C_DEPTH = np.array([[2500, 2501, 500, 499]], np.uint16)   # with d_max = 2.5 and d_min = 0.5: pass, gate, pass, gate
C_BAND, C_W_MIN = 0.0625, 2.0                              # both are f16 values


def c_reg_source():
    """8 source voxels in a row of C_CELL's neighbourhood: values +-band and one f16 step beyond, weights w_min and one f16 step below; the map and
    whether each voxel passes"""
    one = lambda x, up: np.nextafter(F16(x), F16(np.inf if up else -np.inf))
    t = [F16(C_BAND), F16(-C_BAND), one(C_BAND, True), one(-C_BAND, False), F16(0.01), F16(0.01), F16(0.01), F16(0.01)]
    w = [F16(5.0)] * 4 + [F16(C_W_MIN), one(C_W_MIN, False), one(C_W_MIN, True), F16(0.0)]
    ok = [True, True, False, False, True, False, True, False]
    idx = C_ORIGIN + np.array([[1 + (n % 4), 1 + n // 4, 2] for n in range(8)])
    return make_map(idx, np.array(t, F16), np.array(w, F16)), np.array(ok)


# ---- D: cell knownness at seams and walls -------------------------------------------------------------------------------------------------------------
SEAM_KINDS = [(), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]      # the axes on which the voxel c is the last of its brick
SEAM_GEOS = ("SMALL", "SLAB")


def seam_voxel(geo, kind):
    """c: local index 15 on the axes of `kind`, 5 on the others"""
    _, _, lo, _ = dims(geo)
    near = dict(SMALL=[47, 47, 47], SLAB=[23, 23, 7])[geo]                  # local index 15
    c = np.array([near[a] if a in kind else near[a] - 10 for a in range(3)])
    assert [int((c[a] - lo[a]) % 16) for a in range(3)] == [15 if a in kind else 5 for a in range(3)]
    return c


def brick_of(geo, idx):
    _, _, lo, _ = dims(geo)
    return (np.asarray(idx) - lo) // 16


def seam_variants(geo, kind):
    """[(name, map)]: the 4^3 block c - 1 .. c + 2 complete; without one corner of the cell [c, c + 1]^3 (the brick stays allocated); without every
    voxel of one of the bricks those corners lie in (the brick is never allocated), where the block spans more than one brick"""
    c = seam_voxel(geo, kind)
    idx = box(c - 1, c + 2)
    full = make_map(idx, ramp(idx, c - 1, (0.01, 0.02, 0.03), -0.05))
    bricks = {tuple(b) for b in brick_of(geo, idx).tolist()}
    assert len(bricks) == 2 ** len(kind)
    out = [("complete", full)]
    corners = [c + np.array(d) for d in itertools.product((0, 1), repeat=3)]
    for v in corners:
        out.append((f"corner {tuple(v - c)} not observed", without(full, (idx == v).all(1))))
    if len(bricks) > 1:
        for b in sorted({tuple(brick_of(geo, v).tolist()) for v in corners}):
            out.append((f"brick {b} not allocated", without(full, (brick_of(geo, idx) == np.array(b)).all(1))))
    return out


@functools.lru_cache(maxsize=None)
def seam_probes(geo, kind):
    """(p, base): 27 points in each of the 27 cells of the block"""
    c = seam_voxel(geo, kind)
    return probes(box(c - 1, c + 1))


def seam_source(geo, kind):
    """27 source voxels, one per cell of the block, landing in it at (identity, SHIFT)"""
    c = seam_voxel(geo, kind)
    idx = box(c - 1, c + 1)
    return make_map(idx, np.full(idx.shape[0], 0.01, F16))


def decoy(geo):
    """A whole brick of observed voxels in the first corner of the volume, far from every block of section D.  Loaded before the block it takes pool
    brick 0, the brick a cell read falls back to for a corner whose own brick is not allocated: a read that forgot the brick's absence would find an
    observed voxel there."""
    _, _, lo, _ = dims(geo)
    return make_map(box(lo, lo + 15), np.full(4096, 0.02, F16))


def expected_unknown(base, m):
    """bool [n] from the listed voxels alone: a probe is unknown exactly when one of its cell's 8 corners is not listed"""
    voxels = listed(m)
    return np.array([not cell_known(b, voxels) for b in np.asarray(base).tolist()])


WALL_OTHER = 4                                             # the block's first voxel on the axes along the wall


def wall_cases(geo):
    """[(name, map, p, base)]: at each of the six walls a 3^3 block that touches it, and probes whose coordinate across the wall runs over the cells with
    base lo - 1, lo, hi - 2, hi - 1 (and hi): exactly at lo * voxel, the f32 below it, exactly at the last voxel, the f32 below that"""
    _, _, lo, hi = dims(geo)
    out = []
    for a in range(3):
        for side in ("low", "high"):
            first = np.full(3, WALL_OTHER)
            first[a] = lo[a] if side == "low" else hi[a] - 3
            idx = box(first, first + 2)
            m = make_map(idx, ramp(idx, first, (0.01, 0.02, 0.03), -0.05))
            l, h = int(lo[a]), int(hi[a])
            if side == "low":
                across = [exact(l), last_in(l - 1), inside(l - 1), inside(l), last_in(l), first_in(l + 1)]
            else:
                across = [first_in(h - 2), inside(h - 2), last_in(h - 2), exact(h - 1), inside(h - 1), last_in(h - 1), exact(h)]
            along = [exact(WALL_OTHER), inside(WALL_OTHER), last_in(WALL_OTHER + 1)]
            p = np.array(list(itertools.product(*[across if b == a else along for b in range(3)])), F32)
            out.append((f"{geo} axis {a} {side}", m, p, cell_of(p)))
    return out


def wall_source(m):
    """one source voxel per voxel of a wall block: at (identity, SHIFT) voxel i lands in cell i, the last layer in cells with a corner outside"""
    return make_map(m["indices"], np.full(m["indices"].shape[0], 0.01, F16))


def origin_case():
    """(map, p, base): the block -2 .. 1 around the origin; coordinates -1, -0.5 (whose cell has base -1) and 0.25 on every axis"""
    idx = box(-2, 1)
    m = make_map(idx, ramp(idx, (-2, -2, -2), (0.01, 0.02, 0.03), -0.05))
    p = np.array(list(itertools.product([exact(-1), F32(-0.5) * VS, F32(0.25) * VS], repeat=3)), F32)
    assert (F32(-0.5) * VS) / VS == F32(-0.5)
    return m, p, cell_of(p)
