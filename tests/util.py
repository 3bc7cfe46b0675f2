"""Shared helpers for the parity tests (HIP path vs CPU oracle on identical inputs)."""
import numpy as np

from taichislam_amd.utils import synthetic as syn

C2 = dict(map_scale=[10.24, 10.24], voxel_scale=0.02, num_voxel_per_blk_axis=16, max_ray_length=5.0,
          min_ray_length=0.3, internal_voxels=10, recast_step=2, texture_enabled=False)
SMALL = dict(map_scale=[10.24, 10.24], voxel_scale=0.04, num_voxel_per_blk_axis=16, max_ray_length=5.0,
             min_ray_length=0.3, internal_voxels=10, recast_step=2, texture_enabled=False)
# volumes whose height differs from their width (the reference's node maps a flat slab: map_size_xy = 100, map_size_z = 10).  SLAB: N = 144, Nz = 48,
# 9 x 9 x 3 bricks, and N / 2 = 72, Nz / 2 = 24 are both 8 (mod 16): the brick faces lie at voxel indices 8 (mod 16) on every axis.  TALL: N = 64,
# Nz = 128, more bricks along z than along x (with tall_stream).  GSLAB: the global map two SLAB submaps are fused into, N = 256, Nz = 64.
SLAB = dict(SMALL, map_scale=[5.76, 1.92])
TALL = dict(SMALL, map_scale=[2.56, 5.12])
GSLAB = dict(SLAB, map_scale=[10.24, 2.4], is_global_map=True)


def lin(idx):
    i = idx.astype(np.int64)
    return ((i[:, 0] + 32768) << 32) | ((i[:, 1] + 32768) << 16) | (i[:, 2] + 32768)


def sort_export(e):
    o = np.argsort(lin(e["indices"]), kind="stable")
    out = {"indices": e["indices"][o], "TSDF": np.asarray(e["TSDF"])[o].view(np.uint16),
           "W_TSDF": np.asarray(e["W_TSDF"])[o].view(np.uint16), "occupy": e["occupy"][o]}
    if getattr(e.get("color", None), "size", 0):
        out["color"] = np.asarray(e["color"])[o].view(np.uint16)
    return out


def assert_export_equal(a, b, what=""):
    a, b = sort_export(a), sort_export(b)
    assert a["indices"].shape == b["indices"].shape, f"{what}: voxel count {a['indices'].shape[0]} != {b['indices'].shape[0]}"
    assert np.array_equal(a["indices"], b["indices"]), f"{what}: voxel index sets differ"
    for k in ("TSDF", "W_TSDF", "occupy"):
        bad = np.nonzero(a[k] != b[k])[0]
        assert bad.size == 0, f"{what}: {k} differs at {bad.size} voxels, first {a['indices'][bad[0]]}: {a[k][bad[0]]} vs {b[k][bad[0]]}"
    if "color" in a or "color" in b:
        assert np.array_equal(a["color"], b["color"]), f"{what}: color differs"


def sorted_rows(x, decimals=None):
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[:, None]
    o = np.lexsort(x.T[::-1])
    return x[o]


def small_stream(n, h=120, w=160, **kw):
    K = syn.scaled_intrinsics(h, w)
    frames = []
    for f in range(n):
        R, T = syn.camera_pose(f, **{k: v for k, v in kw.items() if k in ("orbit", "start_deg")})
        frames.append((R, T, syn.sphere_room_depth(R, T, h, w, radius=kw.get("radius", 3.0), K=K)))
    return K, frames


def tall_stream(n):
    """small_stream(n, radius=2.0) with every pose turned by Q (x -> z, z -> -x): the same depth images, seen by a camera that looks up the z axis of TALL"""
    Q = np.array([[0.0, 0, -1], [0, 1, 0], [1, 0, 0]])
    K, frames = small_stream(n, radius=2.0)
    return K, [(Q @ R, Q @ T, d) for R, T, d in frames]


def tilt(R, a, b):
    """R turned by a about z, then by b about x: a base pose off the lattice (with an axis-aligned one six of the seven splat weights of a fusion are exactly
    0); the tilt() of tools/gen_ref_golden.py, which keeps its own so that the generator needs nothing of this file"""
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    return R @ np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1.0]]) @ np.array([[1.0, 0, 0], [0, cb, -sb], [0, sb, cb]])


def make_pair(cfg, K, **gpu_kw):
    """(HIP DenseTSDF, OracleTSDF) with identical configuration."""
    from oracle import OracleTSDF
    from taichislam_amd.mapping import DenseTSDF
    g = DenseTSDF(**cfg, **gpu_kw)
    g.set_dep_camera_intrinsic(K)
    g.set_color_camera_intrinsic(K)
    ocfg = {k: v for k, v in cfg.items() if k not in ("max_disp_particles",)}
    o = OracleTSDF(**ocfg)
    o.set_intrinsics(K, K)
    return g, o
