"""View rendering without a GPU: the C-ABI entry points are declared, exported and bound and refuse a null handle; the numpy float32 restatement
the GPU tests compare against (tests/render_view_ref.py) finds an analytic sphere, obeys the status rules on hand-built grids, and reproduces the
analytic depth of the synthetic room from the oracle's map."""
import ctypes
import os
import re

import numpy as np
import pytest

import render_view_ref as ref
import render_view_scenes as sc
from taichislam_amd.utils import synthetic as syn
from util import SMALL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _declaration(name):
    txt = open(os.path.join(ROOT, "include", "taichislam_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/taichislam_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_render_symbols_declared_exported_bound_and_refuse_a_null_handle():
    from taichislam_amd import _lib
    L = ctypes.CDLL(_lib.library_path())
    L.tsl_last_error.restype = ctypes.c_char_p
    cfg = _lib.ViewCfg()
    cfg.h, cfg.w = 4, 4
    assert ctypes.sizeof(_lib.ViewCfg) == 96                                   # double K[9]; int32 h, w; float t_min, t_max, dt; int32 flags
    R = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    T = (ctypes.c_double * 3)(0, 0, 0)
    depth, status = np.zeros(16, np.float32), np.zeros(16, np.uint8)
    for name, nargs in (("tsl_tsdf_render_view", 8), ("tsl_tsdf_render_view_dev", 9)):
        assert len(_declaration(name)) == nargs
        assert hasattr(L, name), f"{name} is not exported by the built library"
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
        assert args[3] is ctypes.POINTER(_lib.ViewCfg) or args[3]._type_ is _lib.ViewCfg
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
        extra = (None,) if nargs == 9 else ()
        rc = fn(None, R, T, ctypes.byref(cfg), depth.ctypes.data_as(ctypes.c_void_p), None, None, status.ctypes.data_as(ctypes.c_void_p), *extra)
        assert rc == -1 and b"render_view" in L.tsl_last_error()


def test_python_call_refuses_what_no_view_can_have():
    from taichislam_amd.mapping import DenseTSDF
    from taichislam_amd.mapping.dense_tsdf import depth_to_mm, view_config
    K = syn.scaled_intrinsics(120, 160)
    bare = DenseTSDF.__new__(DenseTSDF)                                         # no handle: the refusal comes before anything touches the library
    for bad in (np.where(np.arange(9) == 0, np.nan, K), np.where(np.arange(9) == 5, np.inf, K)):
        with pytest.raises(ValueError):
            view_config(bad)
        with pytest.raises(ValueError):
            DenseTSDF.render_view(bare, np.eye(3), np.zeros(3), K=bad)
    for kw in (dict(shape=(0, 4)), dict(step=0.0), dict(step=-1.0), dict(t_max=float("nan")), dict(t_min=float("inf"))):
        with pytest.raises(ValueError):
            view_config(K, **kw)
    c = view_config(K, (120, 160), 0.1, 3.0, 0.02, skip=False)
    assert (c.h, c.w, c.flags) == (120, 160, 1) and c.t_min == F32(0.1) and c.dt == F32(0.02) and list(c.K) == list(K)
    assert view_config().flags == 0 and not any(view_config().K)
    mm = depth_to_mm(np.array([[0.0, 1.2344], [2.9996, 70.0]], np.float32))
    assert mm.dtype == np.uint16 and mm.tolist() == [[0, 1234], [3000, 65535]]
    assert np.array_equal(mm, ref.depth_to_mm(np.array([[0.0, 1.2344], [2.9996, 70.0]], np.float32)))


@pytest.mark.parametrize("step", [0.75, 0.4])
def test_restatement_finds_an_analytic_sphere(step):
    """f16(|p| - 0.8) at 0.05 m voxels, known for indices -30 .. 29, 160 x 120 views, t in [0.1, 3].  For hit pixels with an incidence cosine
    >= 0.5: |depth - analytic| * |dc| <= 0.1 voxel and normal . analytic normal >= 0.99 (trilinear and secant error of a radius-0.8 sphere at this
    voxel size are each below 1e-3 m, f16 near the surface 6e-5 m, gradient error about vs / 2r radians).  Measured with this restatement: depth
    error at worst 0.040 voxel, normal dot at worst 0.9991, checked share 0.60 - 0.69 for both steps."""
    val, known, lo = sc.sphere_grid()
    h, w = 120, 160
    K = syn.scaled_intrinsics(h, w)
    vs = F32(sc.SPHERE_VS)
    for n, (R, T) in enumerate(sc.sphere_views()):
        depth, nrm, _, st = ref.render(R, T, K, h, w, 0.1, 3.0, F32(step) * vs, vs, val, known, lo)
        sc.check_sphere_view(depth, nrm, st, R, T, K, h, w, float(vs), f"view {n}, step {step} voxel")
        assert set(np.unique(st)) <= {0, 1}


def _slab_grid(x0, N=32, vs=0.1, unknown_x=()):
    """val = x0 - x (free space towards -x, the surface the plane x = x0), every voxel known except the planes of x index `unknown_x`"""
    r = np.arange(-(N // 2), N // 2, dtype=np.int16)
    idx = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    idx = idx[~np.isin(idx[:, 0], list(unknown_x))]
    tsdf = (F32(x0) - idx[:, 0].astype(F32) * F32(vs)).astype(np.float16)
    return ref.grid_from_export(idx, tsdf, N, N)


def test_restatement_status_rules():
    vs = F32(0.1)
    Rf, _ = syn.camera_pose(0)                                                  # looks along +x
    Rb, _ = syn.camera_pose(180)                                                # looks along -x
    K = np.array([16.0, 0, 3.5, 0, 16.0, 2.5, 0, 0, 1.0])
    h, w = 6, 8
    val, known, lo = _slab_grid(0.33)
    # from the front: every pixel hits the plane at z-depth 1.33, the normal points back at the camera
    depth, nrm, _, st = ref.render(Rf, [-1.0, 0.03, 0.04], K, h, w, 0.1, 2.0, 0.07, vs, val, known, lo)
    assert (st == 0).all() and np.abs(depth - 1.33).max() < 2e-3
    assert np.abs(nrm - np.array([-1.0, 0, 0], np.float32)).max() < 1e-3
    # from behind: a back face ends the ray, depth 0, no normal
    depth, nrm, _, st = ref.render(Rb, [1.2, 0.03, 0.04], K, h, w, 0.1, 2.0, 0.07, vs, val, known, lo)
    assert (st == 2).all() and (depth == 0).all() and (nrm == 0).all()
    # an unknown gap around the crossing: the sample before it is positive, the one after it negative, and no crossing is made across it
    gval, gknown, _ = _slab_grid(0.33, unknown_x=(2, 3, 4))
    depth, _, _, st = ref.render(Rf, [-1.0, 0.03, 0.04], K, h, w, 0.1, 2.0, 0.07, vs, gval, gknown, lo)
    assert (st == 1).all() and (depth == 0).all()
    # a view that leaves the volume (and starts outside it): a miss, no exception
    depth, _, _, st = ref.render(Rb, [-1.0, 0.03, 0.04], K, h, w, 0.1, 50.0, 0.07, vs, val, known, lo)
    assert (st == 1).all()
    depth, _, _, st = ref.render(Rf, [-9.0, 0.03, 0.04], K, h, w, 0.1, 8.3, 0.07, vs, val, known, lo)
    assert (st == 1).all()
    depth, _, _, st = ref.render(Rf, [-9.0, 0.03, 0.04], K, h, w, 0.1, 12.0, 0.07, vs, val, known, lo)
    assert (st == 0).sum() > 0 and np.abs(depth[st == 0] - 9.33).max() < 2e-3   # ... and one that enters it finds the plane
    # a hit whose p* lies in a cell with an unknown corner: samples at x = 0.16 and 0.41 (cells 1 and 4) are known, p* at x = 0.29 is in cell 2,
    # whose corners include the unknown plane of x index 3
    hval, hknown, _ = _slab_grid(0.29, unknown_x=(3,))
    K1 = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0])
    depth, nrm, _, st = ref.render(Rf, [-1.0, 0.03, 0.04], K1, 1, 1, 1.16, 2.0, 0.25, vs, hval, hknown, lo)
    assert st[0, 0] == 0x40 and (nrm == 0).all() and abs(depth[0, 0] - 1.29) < 2e-3
    # non-finite coordinates are unknown samples, not errors
    depth, _, _, st = ref.render(Rf, [-1.0, 0.03, 0.04], np.array([0.0, 0, 3.5, 0, 16.0, 2.5, 0, 0, 1.0]), h, w, 0.1, 2.0, 0.07, vs, val, known, lo)
    assert (st == 1).all()


def _room_errors(depth, st, R, T, K, h, w, vs):
    t, _, _, _ = sc.ray_sphere(R, T, K, h, w, sc.ROOM_R, inside=True)
    hit = ((st.ravel() & ~np.uint8(0x40)) == 0)
    err = np.abs(depth.ravel()[hit].astype(np.float64) - t[hit]) / vs
    return hit, t, err


@pytest.mark.parametrize("step", [0.75, 0.4])
def test_restatement_over_the_oracles_map_reproduces_the_analytic_room(step):
    """Oracle map (BATCHED) of small_stream(4, h=240, w=320) in SMALL, 320 x 240 view at the pose and K of frame 1, t in [0.3, 5], against the
    analytic depth of the room's sphere before its rounding to millimetres.  The error is a property of the reference's projective TSDF.  Asserted:
    median <= 0.10, 99th percentile <= 0.50, maximum <= 1.0 voxel over hit pixels; hits >= 85 % of the pixels whose analytic depth is in range,
    and >= 50 % at camera_pose(2.5, orbit=0.2), which nobody integrated.
    Measured with this restatement (step 0.75 / 0.4 voxel): median 0.050 / 0.053, 99th percentile 0.335 / 0.337, maximum 0.448 / 0.450
    voxel, hits 92.7 % / 94.5 %; at the pose nobody integrated hits 72.2 % / 73.6 %, maximum 0.449 / 0.449 voxel."""
    K, frames = sc.room_scene()
    o = sc.room_oracle(K, frames)
    val, known, lo = sc.oracle_grid(o)
    vs = F32(SMALL["voxel_scale"])
    h, w = 240, 320
    R, T, _ = frames[1]
    depth, _, _, st = ref.render(R, T, K, h, w, 0.3, 5.0, F32(step) * vs, vs, val, known, lo)
    hit, t, err = _room_errors(depth, st, R, T, K, h, w, float(vs))
    gate = (t >= 0.3) & (t <= 5.0)
    share = (hit & gate).sum() / gate.sum()
    print(f"step {step}: median {np.median(err):.3f} p99 {np.percentile(err, 99):.3f} max {err.max():.3f} voxel, hits {share:.3f}")
    assert np.median(err) <= 0.10 and np.percentile(err, 99) <= 0.50 and err.max() <= 1.0
    assert share >= 0.85
    R2, T2 = syn.camera_pose(2.5, orbit=0.2)
    depth2, _, _, st2 = ref.render(R2, T2, K, h, w, 0.3, 5.0, F32(step) * vs, vs, val, known, lo)
    hit2, t2, err2 = _room_errors(depth2, st2, R2, T2, K, h, w, float(vs))
    share2 = hit2.mean()
    print(f"step {step}, unintegrated pose: median {np.median(err2):.3f} max {err2.max():.3f} voxel, hits {share2:.3f}")
    assert share2 >= 0.50


def round_trip_on_the_cpu():
    """render at the pose of frame 1 from the oracle's map, depth_to_mm, integrate that image alone into a fresh oracle map at the same pose,
    render again: (depth, status) of both renders"""
    K, frames = sc.room_scene()
    vs = F32(SMALL["voxel_scale"])
    h, w = 240, 320
    R, T, _ = frames[1]
    out = []
    o = sc.room_oracle(K, frames)
    for _ in range(2):
        val, known, lo = sc.oracle_grid(o)
        depth, _, _, st = ref.render(R, T, K, h, w, 0.3, 5.0, sc.default_step(vs), vs, val, known, lo)
        out.append((depth, st))
        o = sc.room_oracle(K, [(R, T, ref.depth_to_mm(depth))])
    return out


def test_round_trip_through_the_oracle():
    """The loop of the GPU round-trip test (tests/test_render_view_gpu.py), on the CPU: it fixes that test's bound.  Measured: over the pixels
    that hit both times the depths differ by 0.0031 m in the median and 0.0216 m at most (half a voxel: the second map holds one frame, quantised to
    millimetres, against four); render_view_scenes.ROUND_TRIP_BOUND is twice the maximum.  One frame at recast_step 2 leaves many voxels at the wall unobserved: only
    26.5 % of the pixels find all 8 corners of a crossing observed in the second map; the test asks for a tenth so that it cannot pass on nothing."""
    (d0, s0), (d1, s1) = round_trip_on_the_cpu()
    both = (s0 == 0) & (s1 == 0)
    diff = np.abs(d0[both].astype(np.float64) - d1[both])
    print(f"round trip: {both.mean():.3f} of the pixels hit twice, depth difference median {np.median(diff):.5f} max {diff.max():.5f} m")
    assert both.mean() >= 0.1
    assert diff.max() <= sc.ROUND_TRIP_BOUND
