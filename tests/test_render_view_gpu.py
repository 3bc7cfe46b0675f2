"""View rendering on the GPU (tsl_render.hip): bit for bit against the numpy restatement (tests/render_view_ref.py) over the oracle's map, skipping
against the plain walk, colours, an analytic sphere, the device form against the host form with frames in flight, the round trip through
depth_to_mm and the integrator, the refusals."""
import ctypes as C

import numpy as np
import pytest

import render_view_ref as ref
import render_view_scenes as sc
from taichislam_amd.utils import synthetic as syn
from util import C2, SMALL, make_pair

pytestmark = pytest.mark.gpu

F32 = np.float32
VS = F32(SMALL["voxel_scale"])
STEPS = (None, float(F32(0.4) * VS))                     # the default (0.75 voxel) and 0.4 voxel


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_equal(got, want, what):
    (d, n, c, s), (wd, wn, wc, ws) = got, want
    bad = np.argwhere((_bits(d) != _bits(wd)) | (s != ws))
    assert bad.size == 0, f"{what}: {len(bad)} pixels differ, first {bad[:4].tolist()}: depth {d[tuple(bad[0])]} / {wd[tuple(bad[0])]}, status {s[tuple(bad[0])]} / {ws[tuple(bad[0])]}"
    if n is not None and wn is not None:
        assert np.array_equal(_bits(n), _bits(wn)), f"{what}: normal differs at {(_bits(n) != _bits(wn)).any(2).sum()} pixels"
    if c is not None and wc is not None:
        assert np.array_equal(_bits(c), _bits(wc)), f"{what}: colour differs at {(_bits(c) != _bits(wc)).any(2).sum()} pixels"


def _room(texture=False):
    """(HIP map, oracle) after the four 320 x 240 frames of the room, K of those frames"""
    from oracle import BATCHED
    K, frames = sc.room_scene()
    g, o = make_pair(dict(SMALL, texture_enabled=True) if texture else SMALL, K)
    for f, (R, T, d) in enumerate(frames):
        tex = _texture(d.shape[0], d.shape[1], f) if texture else None
        g.recast_depth_to_map(R, T, d, tex)
        o.integrate_depth(R, T, d, tex, mode=BATCHED)
    return g, o, K, frames


def _texture(h, w, seed):
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([ii * 255 // (w - 1), jj * 255 // (h - 1), rng.integers(0, 256, size=(h, w))], -1).astype(np.uint8))


def _ref_view(R, T, K, h, w, step, grid, col=None):
    val, known, lo = grid
    dt = sc.default_step(VS) if step is None else F32(step)
    return ref.render(R, T, K, h, w, 0.3, 5.0, dt, VS, val, known, lo, col)


def test_views_equal_the_restatement_over_the_oracle_and_skipping_changes_nothing(hip_lib):
    """160 x 120 views of the room's map at the pose of frame 1, at a pose nobody integrated, from outside looking in (back faces) and from the
    origin looking away (misses), each with the default step and 0.4 voxel: depth, normal and status equal the restatement over the oracle's
    BATCHED map bit for bit, with and without skipping."""
    g, o, _, _ = _room()
    grid = sc.oracle_grid(o)
    h, w = 120, 160
    K = syn.scaled_intrinsics(h, w)
    seen = set()
    for name, R, T in sc.room_views():
        for step in STEPS:
            want = _ref_view(R, T, K, h, w, step, grid)
            got = g.render_view(R, T, K=K, shape=(h, w), step=step)
            assert got[2] is None and got[0].shape == (h, w) and got[1].shape == (h, w, 3) and got[3].dtype == np.uint8
            _check_equal(got, want, f"{name}, step {step}")
            _check_equal(g.render_view(R, T, K=K, shape=(h, w), step=step, skip=False), want, f"{name}, step {step}, no skipping")
            st = got[3]
            hits = ((st & ~np.uint8(0x40)) == 0).mean()
            print(f"{name}, step {step}: hits {hits:.3f}, status counts {dict(zip(*np.unique(st, return_counts=True)))}")
            seen |= set(np.unique(st).tolist())
            if name == "frame1":
                assert hits >= 0.85
            elif name == "unintegrated":
                assert hits >= 0.5
            elif name == "outside":
                assert (st == 2).all() and (got[0] == 0).all() and (got[1] == 0).all()
            else:
                assert (st == 1).all() and (got[0] == 0).all()
            # without normals the rest is the same
            d2, n2, _, s2 = g.render_view(R, T, K=K, shape=(h, w), step=step, normals=False)
            assert n2 is None and np.array_equal(_bits(d2), _bits(got[0])) and np.array_equal(s2, st)
    assert {0, 1, 2, 0x40} <= seen, seen
    # the defaults: the map's depth intrinsics (those of the 320 x 240 frames), t in [min_ray_length, max_ray_length], 0.75 voxel
    R, T = syn.camera_pose(1)
    K320 = syn.scaled_intrinsics(240, 320)
    _check_equal(g.render_view(R, T, shape=(240, 320)), g.render_view(R, T, K=K320, shape=(240, 320), t_min=0.3, t_max=5.0, step=float(sc.default_step(VS))), "defaults")


def test_skipping_changes_nothing_on_a_large_view(hip_lib):
    """640 x 480 of the C2 map (0.02 m voxels) after 20 frames of the room stream"""
    from taichislam_amd.mapping import DenseTSDF
    g = DenseTSDF(**C2)
    g.set_dep_camera_intrinsic(syn.K_DEPTH)
    for R, T, d in syn.sphere_room_stream(20):
        g.recast_depth_to_map(R, T, d, None)
    R180, _ = syn.camera_pose(180)
    for name, R, T in (("pose 10",) + syn.camera_pose(10), ("away", R180, np.zeros(3)), ("outside", R180, np.array([3.6, 0.0, 0.0]))):
        a = g.render_view(R, T)
        b = g.render_view(R, T, skip=False)
        assert a[0].shape == (480, 640)
        _check_equal(a, b, f"C2 {name}: skipping vs every sample")
        if name == "pose 10":
            assert ((a[3] & ~np.uint8(0x40)) == 0).mean() > 0.5


def test_colours_of_a_textured_map(hip_lib):
    from taichislam_amd import _lib
    g, _, _, _ = _room(texture=True)
    e = g.export_submap()
    val, known, lo, col = ref.grid_from_export(e["indices"], e["TSDF"], g.N, g.Nz, e["color"])
    h, w = 120, 160
    K = syn.scaled_intrinsics(h, w)
    for name, R, T in sc.room_views()[:2]:
        got = g.render_view(R, T, K=K, shape=(h, w))
        assert got[2] is not None                                        # colors=None: the map is textured
        want = _ref_view(R, T, K, h, w, None, (val, known, lo), col)
        _check_equal(got, want, f"textured, {name}")
        hit = got[3] == 0
        assert (got[2][hit].max(1) > 0).mean() > 0.9 and (got[2][~((got[3] & ~np.uint8(0x40)) == 0)] == 0).all()
        assert g.render_view(R, T, K=K, shape=(h, w), colors=False)[2] is None
    u, _, _, _ = _room()
    R, T = syn.camera_pose(1)
    assert u.render_view(R, T, K=K, shape=(h, w))[2] is None
    with pytest.raises(_lib.TslError, match="render_view"):
        u.render_view(R, T, K=K, shape=(h, w), colors=True)


def test_analytic_sphere(hip_lib):
    """init_sphere(voxels=60, radius=0.8) at 0.05 m voxels: the bounds and shares of tests/test_render_view_cpu.py hold on the GPU image, which
    equals the restatement over the same grid"""
    from taichislam_amd.mapping import DenseTSDF
    g = DenseTSDF(map_scale=[6.4, 6.4], voxel_scale=sc.SPHERE_VS, num_voxel_per_blk_axis=16)
    g.init_sphere(voxels=60, radius=sc.SPHERE_R)
    val, known, lo = sc.sphere_grid()
    h, w = 120, 160
    K = syn.scaled_intrinsics(h, w)
    vs = F32(sc.SPHERE_VS)
    for n, (R, T) in enumerate(sc.sphere_views()):
        for step in (0.75, 0.4):
            dt = F32(step) * vs
            got = g.render_view(R, T, K=K, shape=(h, w), t_min=0.1, t_max=3.0, step=float(dt))
            sc.check_sphere_view(got[0], got[1], got[3], R, T, K, h, w, float(vs), f"GPU view {n}, step {step} voxel")
            _check_equal(got, ref.render(R, T, K, h, w, 0.1, 3.0, dt, vs, val, known, lo), f"sphere view {n}, step {step}")


@pytest.mark.parametrize("shape", [(120, 160), (1, 1), (5, 7), (251, 333)])
def test_device_form_equals_host_form_with_work_in_flight(hip_lib, shape):
    import torch
    from taichislam_amd.mapping.dense_tsdf import depth_to_mm
    K, frames = sc.room_scene()
    g, _ = make_pair(SMALL, K)
    for R, T, d in frames[:2]:
        g.recast_depth_to_map(R, T, d, None)
    g.sync()
    Kv = syn.scaled_intrinsics(*shape) if shape[0] > 1 else np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0])
    Rv, Tv = syn.camera_pose(1)
    before = g.render_view(Rv, Tv, K=Kv, shape=shape)
    side = torch.cuda.Stream()
    for R, T, d in frames[2:]:                                    # queued frames, then the view: no sync in between
        g.recast_depth_to_map(R, T, d, None)
    with torch.cuda.stream(side):
        dev = g.render_view(Rv, Tv, K=Kv, shape=shape, device=True)
        mm_dev = depth_to_mm(dev[0])
    side.synchronize()
    assert dev[2] is None and all(x.is_cuda for x in (dev[0], dev[1], dev[3]))
    got = (dev[0].cpu().numpy(), dev[1].cpu().numpy(), None, dev[3].cpu().numpy())
    g.sync()
    want = g.render_view(Rv, Tv, K=Kv, shape=shape)
    _check_equal(got, want, f"device vs host, {shape}")
    assert got[0].shape == shape and ((want[3] & ~np.uint8(0x40)) == 0).any()
    if shape == (120, 160):                                     # the queued frames were integrated before the view was rendered
        assert (_bits(before[0]) != _bits(want[0])).sum() > 100
    assert np.array_equal(mm_dev.cpu().numpy().view(np.uint16), depth_to_mm(want[0]))
    dn = g.render_view(Rv, Tv, K=Kv, shape=shape, device=True, normals=False, skip=False)
    torch.cuda.synchronize()
    assert dn[1] is None and np.array_equal(_bits(dn[0].cpu().numpy()), _bits(want[0]))


def test_round_trip_through_the_integrator(hip_lib):
    """Render at the pose of frame 1, depth_to_mm, integrate that image alone into a fresh map at the same pose, render again: on the pixels that hit
    both times the depths agree within render_view_scenes.ROUND_TRIP_BOUND = 0.0432 m, twice the 0.0216 m the same loop measures on the CPU through
    the restatement and the oracle (tests/test_render_view_cpu.py::test_round_trip_through_the_oracle; 26.5 % of the pixels hit twice there)."""
    from taichislam_amd.mapping import depth_to_mm
    g, _, K, frames = _room()
    R, T, _ = frames[1]
    h, w = 240, 320
    d0, _, _, s0 = g.render_view(R, T, K=K, shape=(h, w))
    mm = depth_to_mm(d0)
    assert mm.dtype == np.uint16 and ((mm > 0) == (d0 > 0)).all()
    f, _ = make_pair(SMALL, K)
    f.recast_depth_to_map(R, T, mm, None)
    d1, _, _, s1 = f.render_view(R, T, K=K, shape=(h, w))
    both = (s0 == 0) & (s1 == 0)
    diff = np.abs(d0[both].astype(np.float64) - d1[both])
    print(f"round trip: {both.mean():.3f} of the pixels hit twice, depth difference median {np.median(diff):.5f} max {diff.max():.5f} m")
    assert both.mean() >= 0.1
    assert diff.max() <= sc.ROUND_TRIP_BOUND


def test_refusals_global_map_and_reset(hip_lib):
    from taichislam_amd import _lib
    from taichislam_amd.mapping import DenseTSDF
    g, _, K, frames = _room()
    R, T, _ = frames[1]
    h, w = 24, 32
    Kv = syn.scaled_intrinsics(h, w)
    depth, nrm, rgb, st = np.zeros((h, w), F32), np.zeros((h, w, 3), F32), np.zeros((h, w, 3), F32), np.zeros((h, w), np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    dp = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))

    def call(R=R, T=T, K=Kv, h=h, w=w, t_min=0.0, t_max=0.0, dt=0.0, rgb=None, dev=False):
        cfg = _lib.ViewCfg()
        cfg.K[:] = list(np.asarray(K, np.float64).reshape(-1))
        cfg.h, cfg.w, cfg.t_min, cfg.t_max, cfg.dt = h, w, t_min, t_max, dt
        Ra, Ta = np.ascontiguousarray(R, np.float64), np.ascontiguousarray(T, np.float64)
        if dev:
            return g.L.tsl_tsdf_render_view_dev(g.h, dp(Ra), dp(Ta), C.byref(cfg), None, None, None, None, None)
        return g.L.tsl_tsdf_render_view(g.h, dp(Ra), dp(Ta), C.byref(cfg), vp(depth), vp(nrm), None if rgb is None else vp(rgb), vp(st))

    def refused(**kw):
        rc = call(**kw)
        return rc == -1 and b"render_view" in g.L.tsl_last_error()

    assert call() == 0 and (st == 0).any()
    assert call(K=np.zeros(9)) == 0                                  # all zero: the map's depth intrinsics
    assert refused(rgb=rgb)                                          # an untextured map
    Rn = np.array(R, np.float64); Rn[1, 1] = np.nan
    assert refused(R=Rn) and refused(T=[0.0, np.inf, 0.0])
    assert refused(K=np.where(np.arange(9) == 4, np.nan, Kv)) and refused(K=np.where(np.arange(9) == 2, -np.inf, Kv))
    assert refused(h=0) and refused(w=-3)
    assert refused(t_min=2.0, t_max=2.0) and refused(t_min=2.0, t_max=1.0) and refused(t_min=6.0)       # 6 > the default t_max = 5
    assert refused(dt=-0.01) and refused(dt=float("nan")) and refused(t_max=float("inf"))
    assert refused(dt=1e-8)                                          # (5 - 0.3) / 1e-8 samples per ray
    assert refused(dev=True)                                         # null device buffers
    with pytest.raises(_lib.TslError, match="render_view"):
        g.render_view(Rn, T, K=Kv, shape=(h, w))
    with pytest.raises(_lib.TslError, match="render_view"):
        g.render_view(R, T, K=Kv, shape=(h, w), t_min=3.0, t_max=1.0)
    # a global map renders submap 0
    G = DenseTSDF(**dict(SMALL, is_global_map=True))
    G.set_dep_camera_intrinsic(K)
    for Rf, Tf, d in frames:
        G.recast_depth_to_map(Rf, Tf, d, None)
    e = G.export_submap()
    grid = ref.grid_from_export(e["indices"], e["TSDF"], G.N, G.Nz)
    got = G.render_view(R, T, K=Kv, shape=(h, w))
    _check_equal(got, _ref_view(R, T, Kv, h, w, None, grid), "global map")
    assert ((got[3] & ~np.uint8(0x40)) == 0).mean() > 0.5
    # after reset() every pixel is a miss
    g.reset()
    d, n, _, s = g.render_view(R, T, K=Kv, shape=(h, w))
    assert (s == 1).all() and (d == 0).all() and (n == 0).all()
