"""Hand-built depth frames for the conditioner's tests (tests/test_depth_condition_cpu.py, tests/test_depth_condition_gpu.py), and the box-in-front-of-a-wall
scene of the end-to-end test."""
import numpy as np

from taichislam_amd.utils import bilateral_tables, depth_tolerance
from taichislam_amd.utils import synthetic as syn

TOL = depth_tolerance()
WS, WR = bilateral_tables(4, sigma_px=1.5)
TOL_1, TOL_MAX = np.full(256, 1, np.uint16), np.full(256, 32767, np.uint16)


def constant(h, w, d=2000):
    return np.full((h, w), d, np.uint16)


def spike(h=15, w=17, y=7, x=8, base=2000, d=2600):
    f = constant(h, w, base)
    f[y, x] = d
    return f


def vertical_step(h=12, w=20, x=10, near=1500, far=3000):
    f = constant(h, w, far)
    f[:, :x] = near
    return f


def with_hole(h=13, w=13, y=6, x=6, base=2000):
    f = constant(h, w, base)
    f[y, x] = 0
    return f


def ramp(h, w, base=1000, step=3):
    """a slanted plane: `step` mm per column, half of it per row"""
    y, x = np.mgrid[0:h, 0:w]
    return (base + step * x + (step * y) // 2).astype(np.uint16)


def random_frames(n, h, w, seed=0, extremes=True):
    """piecewise-smooth surfaces with noise, steps, holes, speckle and, with `extremes`, the depths 0, 1 and 65535"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = np.zeros((n, h, w), np.uint16)
    for f in range(n):
        base = 800 + rng.integers(0, 3000) + rng.integers(-4, 5) * x + rng.integers(-4, 5) * y
        if w > 3:
            c = int(rng.integers(1, w))
            base = np.where(x >= c, base + rng.integers(200, 2000), base)
        d = np.clip(base + rng.integers(-12, 13, size=(h, w)), 1, 65535)
        r = rng.random((h, w))
        d = np.where(r < 0.04, 0, d)
        d = np.where((r >= 0.04) & (r < 0.08), rng.integers(1, 65536, size=(h, w)), d)
        out[f] = d
    if extremes:
        flat = out.reshape(-1)
        k = flat.size
        flat[0], flat[k // 2], flat[k - 1] = 65535, 1, 0
        if k > 6:
            flat[1], flat[k // 2 + 1], flat[k - 2] = 1, 0, 65535
    return out


# ---- end to end: a box in front of a wall, two columns of mid-depth pixels on the box's silhouette --------------------------------------------------------
E2E_H, E2E_W = 120, 160
E2E_WALL_MM, E2E_BOX_MM, E2E_FLY_MM = 2200, 1000, 1600
E2E_BOX_Y, E2E_BOX_Z = (-0.194, 0.4255), (-0.3147, 0.2995)          # the box face in the world, metres: the plane x = 1 between these y and z
E2E_CAMERA_Y = (0.0, 0.0, 0.0, -0.5)                                 # three frames from the origin, one from half a metre to the right


def _render(ty):
    K = syn.scaled_intrinsics(E2E_H, E2E_W)
    fx, fy, cx, cy = K[0], K[4], K[2], K[5]
    u, v = np.arange(E2E_W), np.arange(E2E_H)
    yb, zb = ty - (u - cx) / fx * (E2E_BOX_MM / 1000.0), -(v - cy) / fy * (E2E_BOX_MM / 1000.0)
    inb = ((zb >= E2E_BOX_Z[0]) & (zb <= E2E_BOX_Z[1]))[:, None] & ((yb >= E2E_BOX_Y[0]) & (yb <= E2E_BOX_Y[1]))[None, :]
    f = np.where(inb, E2E_BOX_MM, E2E_WALL_MM).astype(np.uint16)
    right = inb & ~np.roll(inb, -1, axis=1)                           # the last box pixel of each row
    for s in (1, 2):
        f[np.roll(right, s, axis=1) & ~inb] = E2E_FLY_MM
    return f


def box_wall_scene():
    """(K, R, poses, frames uint16 [4, 120, 160], probes).  Every camera looks along +x at a wall 2.2 m away; a box face 1 m away covers the middle of the
    image; the two columns right of the box's right silhouette read 1.6 m, between the two: flying pixels.  Three frames come from the origin and one from
    0.5 m to the right, from where the space behind the first three frames' flying pixels is seen to be empty.  In a map of the raw frames the voxels behind
    those flying pixels hold three surface observations against one free one and read occupied; in a map of the conditioned frames they hold the free one
    alone.  probes: float32 [., 3] world points `gap` (along the flying pixels' rays, behind them, in the empty space between box and wall), `wall`, and `box`
    (on the box face, away from the silhouette).  The gap probes stop at z = -0.16: below it the single frame from the right leaves three voxels of the
    grid untouched, and a voxel nobody observed reads occupied in this map (TSDF 0 is below the surface threshold)."""
    K = syn.scaled_intrinsics(E2E_H, E2E_W)
    R = syn.R_BODY_OPTICAL.copy()
    poses = [np.array([0.0, ty, 0.0]) for ty in E2E_CAMERA_Y]
    frames = np.stack([_render(ty) for ty in E2E_CAMERA_Y])

    def grid(xs, ys, zs):
        g = np.stack(np.meshgrid(xs, ys, zs, indexing="ij"), axis=-1).reshape(-1, 3)
        return np.ascontiguousarray(g, np.float32)
    step = 0.04
    probes = {"gap": grid(np.arange(1.64, 1.93, step), np.arange(-0.44, -0.31, step), np.arange(-0.16, 0.25, step)),
              "wall": grid(np.arange(2.20, 2.29, step), np.arange(-0.60, -0.47, step), np.arange(-0.24, 0.25, step)),
              "box": grid(np.arange(1.00, 1.09, step), np.arange(0.00, 0.31, step), np.arange(-0.20, 0.21, step))}
    return K, R, poses, frames, probes


def e2e_conditioned_ref():
    import depth_condition_ref as ref
    return ref.condition_np(box_wall_scene()[3], TOL, WS, WR)["depth"]


_E2E_COUNTS = []


def e2e_oracle_counts():
    """{"raw" | "cond": {"gap" | "wall" | "box": occupied probe points}} of the oracle's SMALL maps of the raw frames and of the restatement's conditioned
    frames; computed once"""
    if not _E2E_COUNTS:
        from oracle import BATCHED, OracleTSDF
        from util import SMALL
        K, R, poses, frames, probes = box_wall_scene()
        out = {}
        for name, fr in (("raw", frames), ("cond", e2e_conditioned_ref())):
            o = OracleTSDF(**SMALL)
            o.set_intrinsics(K)
            for f, T in zip(fr, poses):
                o.integrate_depth(R, T, f, mode=BATCHED)
            out[name] = {k: int(o.query_points(0, p).sum()) for k, p in probes.items()}
        _E2E_COUNTS.append(out)
    return _E2E_COUNTS[0]
