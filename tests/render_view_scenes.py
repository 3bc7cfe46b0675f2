"""Scenes and analytic answers shared by tests/test_render_view_cpu.py and tests/test_render_view_gpu.py."""
import numpy as np

import render_view_ref as ref
from taichislam_amd.utils import synthetic as syn
from util import SMALL, small_stream

F32 = np.float32
SPHERE_VS, SPHERE_R, SPHERE_N = 0.05, 0.8, 128           # DenseTSDF(map_scale=[6.4, 6.4], voxel_scale=0.05).init_sphere(voxels=60, radius=0.8)
ROOM_R = 3.0                                            # synthetic.sphere_room_depth
ROUND_TRIP_BOUND = 2 * 0.0216                           # metres: twice the maximum test_render_view_cpu.test_round_trip_through_the_oracle measures


def look_at(T, up=(0.0, 0.0, 1.0)):
    """camera-to-map rotation (optical convention: x right, y down, z forward) of a camera at T looking at the origin"""
    z = -np.asarray(T, np.float64)
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z], 1)


def sphere_views():
    """the three poses of the analytic-sphere checks: from (-1.3, 0, 0) looking at the centre, and two oblique poses 1.25 m out"""
    out = []
    for T in ((-1.3, 0.0, 0.0), 1.25 * np.array([0.6, 0.64, 0.48]), 1.25 * np.array([-0.36, 0.48, -0.8])):
        T = np.asarray(T, np.float64)
        out.append((look_at(T), T))
    return out


def sphere_grid():
    """what init_sphere(voxels=60, radius=0.8) loads at 0.05 m voxels: f16(|p| - 0.8), known for indices -30 .. 29"""
    r = np.arange(-30, 30, dtype=np.int16)
    idx = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    p = idx.astype(F32) * F32(SPHERE_VS)
    tsdf = (np.sqrt((p * p).sum(1)) - F32(SPHERE_R)).astype(np.float16)
    return ref.grid_from_export(idx, tsdf, SPHERE_N, SPHERE_N)


def ray_sphere(R, T, K, h, w, radius, inside):
    """float64 analytic answer per pixel of a sphere at the origin: (z-depth t [h * w] (nan: the ray misses it), outward unit normal at the
    point, |dc|).  inside: the far root (a room seen from within), else the near one."""
    K = np.asarray(K, np.float64).reshape(-1)
    vv, uu = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    dc = np.stack([(uu.ravel() - K[2]) / K[0], (vv.ravel() - K[5]) / K[4], np.ones(h * w)], 1)
    d = dc @ np.asarray(R, np.float64).reshape(3, 3).T
    T = np.asarray(T, np.float64)
    a, b, c = (d * d).sum(1), 2.0 * (d @ T), float(T @ T) - radius * radius
    with np.errstate(invalid="ignore"):
        root = np.sqrt(b * b - 4.0 * a * c)
        t = (-b + root) / (2.0 * a) if inside else (-b - root) / (2.0 * a)
    n = (T[None, :] + t[:, None] * d) / radius
    return t, n, np.linalg.norm(dc, axis=1), d


def check_sphere_view(depth, normal, status, R, T, K, h, w, vs, what):
    """the bounds and shares of the analytic-sphere check of tests/test_render_view_cpu.py; returns the measured figures"""
    t, n, ldc, d = ray_sphere(R, T, K, h, w, SPHERE_R, inside=False)
    meets = np.isfinite(t)
    cosi = np.where(meets, -(n * d).sum(1) / np.linalg.norm(d, axis=1), 0.0)          # incidence cosine
    hit = ((status.ravel() & ~np.uint8(0x40)) == 0)
    assert not (hit & ~meets).any(), f"{what}: {(hit & ~meets).sum()} pixels off the sphere hit"
    assert hit[cosi > 0.2].all(), f"{what}: {(~hit[cosi > 0.2]).sum()} pixels that meet the sphere at cosine > 0.2 did not hit"
    sel = hit & (cosi >= 0.5)
    share = sel.mean()
    err = np.abs(depth.ravel()[sel].astype(np.float64) - t[sel]) * ldc[sel] / vs
    dot = (normal.reshape(-1, 3)[sel].astype(np.float64) * n[sel]).sum(1)
    print(f"{what}: share {share:.3f}, depth error max {err.max():.4f} voxel, normal dot min {dot.min():.5f}")
    assert share >= 0.5, f"{what}: only {share:.3f} of the pixels are checked"
    assert err.max() <= 0.1, f"{what}: depth error {err.max():.4f} voxel"
    assert dot.min() >= 0.99, f"{what}: normal dot {dot.min():.5f}"
    assert (status.ravel()[sel] == 0).all()
    return share, err.max(), dot.min()


def room_scene():
    """(K, frames) of the room scene the CPU and GPU tests share: four 320 x 240 frames (at 160 x 120 the rays of recast_step 2 are further apart than a voxel at the wall)"""
    return small_stream(4, h=240, w=320)


def room_oracle(K, frames, cfg=SMALL):
    from oracle import BATCHED, OracleTSDF
    o = OracleTSDF(**cfg)
    o.set_intrinsics(K, K)
    for R, T, d in frames:
        o.integrate_depth(R, T, d, mode=BATCHED)
    return o


def oracle_grid(o, colour=False):
    e = o.export_sparse()
    return ref.grid_from_export(e["indices"], e["TSDF"], o.N, o.Nz, e["color"] if colour else None)


def default_step(vs):
    return F32(0.75) * F32(vs)


def room_views():
    """(name, R, T) of the bit-for-bit set: the pose of frame 1, a pose nobody integrated, from outside looking in, from the origin looking away"""
    R1, T1 = syn.camera_pose(1)
    R2, T2 = syn.camera_pose(2.5, orbit=0.2)
    R180, _ = syn.camera_pose(180)
    return [("frame1", R1, T1), ("unintegrated", R2, T2), ("outside", R180, np.array([3.6, 0.0, 0.0])), ("away", R180, np.zeros(3))]
