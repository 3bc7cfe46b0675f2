"""The view gain on the GPU (tsl_view_gain.hip): the records and both per-ray arrays of DenseTSDF.score_views equal the numpy restatement
(tests/view_gain_ref.py) over the oracle's export exactly, with skipping on and off -- on the hand-built scenes of tests/frontier_scenes.py on three
geometries and on the room -- plus the cut, batch independence, slot 1, ordering behind queued frames, the device form, repeatability, the edge cases and
every refusal.  tests/test_view_gain_cpu.py asserts that these inputs reach the branches they exist for; the assertions are repeated here on the result."""
import ctypes as C

import numpy as np
import pytest

import frontier_scenes as fs
import render_view_scenes as rv
import view_gain_ref as ref
import view_gain_scenes as vg
from taichislam_amd import _lib
from util import SMALL, make_pair, small_stream

pytestmark = pytest.mark.gpu

VS = vg.VS
_MAPS = {}


def _map(geo):
    """one GPU map per geometry for the whole module, reset before every use"""
    from taichislam_amd.mapping import DenseTSDF
    if geo not in _MAPS:
        _MAPS[geo] = DenseTSDF(**fs.GEOMETRIES[geo]["cfg"])
    g = _MAPS[geo]
    g.reset()
    g.active_submap_id[None] = 0
    return g


def _oracle(geo):
    from oracle import OracleTSDF
    return OracleTSDF(**fs.GEOMETRIES[geo]["cfg"])


def _loaded(geo, sc, sid=0):
    g, o = _map(geo), _oracle(geo)
    fs.load_pair(g, o, fs.place(sc, geo), sid)
    return g, o


def _both(g, R, T, what, **kw):
    """score_views with skipping on and off: the two results must be equal to each other; returns the first"""
    a = g.score_views(R, T, rays=True, skip=True, **kw)
    b = g.score_views(R, T, rays=True, skip=False, **kw)
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs between skip on and off"
    return a


def _check_scene(g, o, geo, R, T, what, **kw):
    want = vg.scene_ref(o.export_sparse(), geo, R, T, **kw)
    got = _both(g, R, T, what, **vg.fan_kwargs(geo), **kw)
    ref.assert_equal(got, want, what)
    dt = ref.default_step(VS)
    assert np.array_equal(got["unknown_volume"], ref.volume(want["records"]["vol_unknown"], dt, vg.K_FAN))
    assert np.array_equal(got["free_volume"], ref.volume(want["records"]["vol_free"], dt, vg.K_FAN))
    return got, want


@pytest.mark.parametrize("geo", ["SMALL", "SLAB", "TALL"])
@pytest.mark.parametrize("name", vg.SCENE_NAMES)
def test_scenes_equal_the_restatement(hip_lib, geo, name):
    g, o = _loaded(geo, vg.scene(name, geo))
    R, T = vg.scene_poses(name, geo)
    got, want = _check_scene(g, o, geo, R, T, f"{name} on {geo}")
    assert got["ray_unknown"].shape == (5, vg.H, vg.W) and got["n_free"].min() > 0
    assert vg.scene_ref(o.export_sparse(), geo, R[4:], T[4:])["n_outside"] > 0          # the pose outside the volume
    if name == "two_unknowns":
        assert want["n_absent"] > 0 and want["n_unobserved"] > 0
    if name == "plate":
        assert got["n_hit"].sum() > 0
    if name == "wall":
        assert vg.scene_ref(o.export_sparse(), geo, R[:1], T[:1])["n_outside"] > 0
    if name == "two_values":
        b, _ = _check_scene(g, o, geo, R, T, f"{name} on {geo}, free_thres 0.2", free_thres=0.2)
        assert b["n_hit"].sum() > got["n_hit"].sum() and b["n_free"].sum() < got["n_free"].sum()


@pytest.mark.parametrize("name", ["shell", "two_unknowns"])
@pytest.mark.parametrize("run", [0, 1, 7])
def test_unknown_run_cuts_the_rays(hip_lib, name, run):
    g, o = _loaded("SMALL", vg.scene(name, "SMALL"))
    R, T = vg.scene_poses(name, "SMALL")
    got, want = _check_scene(g, o, "SMALL", R, T, f"{name}, unknown_run {run}", unknown_run=run)
    if run:
        assert got["n_cut"].sum() > 0 and want["cut_in_absent"] > 0          # a cut inside an absent brick: the loop without gathers
        assert (got["ray_unknown"][(got["ray_status"] & 3) == ref.CUT] >= run).all()
    else:
        assert got["n_cut"].sum() == 0


_ROOM = []


def _room():
    """(GPU map, oracle, K) of the room scene: four 320 x 240 frames, built once"""
    from oracle import BATCHED
    if not _ROOM:
        K, frames = rv.room_scene()
        g, o = make_pair(SMALL, K)
        for R, T, d in frames:
            g.recast_depth_to_map(R, T, d, None)
            o.integrate_depth(R, T, d, mode=BATCHED)
        _ROOM.append((g, o, K))
    return _ROOM[0]


def _room_kwargs(K):
    return dict(K=vg.room_K(K), shape=vg.ROOM_SHAPE, stride=vg.ROOM_STRIDE)


def test_room_equals_the_restatement(hip_lib):
    g, o, K = _room()
    R, T = vg.room_poses()
    want = vg.room_ref(o.export_sparse(), o.N, o.Nz, K, R, T)
    got = _both(g, R, T, "room", **_room_kwargs(K))
    ref.assert_equal(got, want, "room")
    assert got["ray_unknown"].shape == (71, 20, 24)
    assert got["n_hit"].max() > 0 and got["n_range"].max() > 0 and got["n_frontier"].max() > 0
    Kf = ref.scaled_K(vg.room_K(K), vg.ROOM_STRIDE)
    assert np.array_equal(got["unknown_volume"], ref.volume(want["records"]["vol_unknown"], ref.default_step(VS), Kf))
    # the map's own intrinsics and no stride: K=None is the 240 x 320 camera
    one = g.score_views(R[0], T[0], shape=(20, 24), rays=True)
    ref.assert_equal(one, ref.score_export(o.export_sparse(), o.N, o.Nz, VS, R[:1], T[:1], K, 20, 24, np.float32(0.3), np.float32(5.0)), "room, the map's K")


def test_a_pose_scores_the_same_alone_and_in_any_batch(hip_lib):
    g, o, K = _room()
    R, T = vg.room_poses()
    kw = _room_kwargs(K)
    all_ = g.score_views(R, T, rays=True, **kw)
    for i in (0, 3, 37, 70):
        one = g.score_views(R[i], T[i], rays=True, **kw)
        for k in all_:
            assert np.array_equal(one[k][0], all_[k][i]), (i, k)
    back = g.score_views(R[::-1], T[::-1], rays=True, **kw)
    for k in all_:
        assert np.array_equal(back[k], all_[k][::-1]), k


def test_submap_slot_one_with_other_content_in_slot_zero(hip_lib):
    g, o = _map("SMALL"), _oracle("SMALL")
    fs.load_pair(g, o, fs.place(fs.plate(), "SMALL"), 0)
    fs.load_pair(g, o, fs.place(fs.two_unknowns(), "SMALL"), 1)
    R, T = vg.scene_poses("two_unknowns", "SMALL")
    g.active_submap_id[None] = 1
    o.set_active_submap(1)
    one, _ = _check_scene(g, o, "SMALL", R, T, "slot 1")
    g.active_submap_id[None] = 0
    o.set_active_submap(0)
    zero, _ = _check_scene(g, o, "SMALL", R, T, "slot 0")
    assert not np.array_equal(one["n_unknown"], zero["n_unknown"])


def test_scoring_runs_behind_the_queued_frames(hip_lib):
    """score_views straight after recast_depth_to_map of a fifth frame, nothing waited for: the result is the one of five frames, not of four"""
    from oracle import BATCHED
    K, frames = small_stream(5, h=240, w=320)
    g, o = make_pair(SMALL, K)
    for R, T, d in frames[:4]:
        g.recast_depth_to_map(R, T, d, None)
        o.integrate_depth(R, T, d, mode=BATCHED)
    Rp, Tp = vg.room_poses()
    Rp, Tp = Rp[:12], Tp[:12]
    kw = _room_kwargs(K)
    four = g.score_views(Rp, Tp, rays=True, **kw)
    ref.assert_equal(four, vg.room_ref(o.export_sparse(), o.N, o.Nz, K, Rp, Tp), "four frames")
    R, T, d = frames[4]
    g.recast_depth_to_map(R, T, d, None)
    five = g.score_views(Rp, Tp, rays=True, **kw)
    o.integrate_depth(R, T, d, mode=BATCHED)
    ref.assert_equal(five, vg.room_ref(o.export_sparse(), o.N, o.Nz, K, Rp, Tp), "five frames")
    assert not np.array_equal(five["ray_unknown"], four["ray_unknown"])


def test_device_form_equals_the_host_form(hip_lib):
    import torch
    g, o, K = _room()
    R, T = vg.room_poses()
    kw = _room_kwargs(K)
    host = g.score_views(R, T, rays=True, **kw)
    rec = np.zeros(R.shape[0], ref.RECORD_DTYPE)
    for k in ref.RECORD_DTYPE.names:
        rec[k] = host[k]
    for stream in (None, torch.cuda.Stream()):
        with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
            dev = g.score_views(R, T, rays=True, device=True, **kw)
            again = g.score_views(R[:5], T[:5], device=True, **kw)          # a second call straight behind the first: its pose table waits for the first's
            got = {k: v.clone() for k, v in dev.items()}
            got5 = again["records"].clone()
        torch.cuda.synchronize()
        assert all(v.is_cuda for v in got.values()) and got["records"].shape == (71, 16) and got["records"].dtype == torch.int32
        assert got["records"].cpu().numpy().tobytes() == rec.tobytes()
        assert got5.cpu().numpy().tobytes() == rec[:5].tobytes()
        assert np.array_equal(got["ray_unknown"].cpu().numpy(), host["ray_unknown"]) and np.array_equal(got["ray_status"].cpu().numpy(), host["ray_status"])
        assert "ray_unknown" not in again


def test_second_call_returns_the_same_bytes(hip_lib):
    g, o = _loaded("SMALL", fs.plate())
    R, T = vg.scene_poses("plate", "SMALL")
    a = g.score_views(R, T, rays=True, unknown_run=4, **vg.fan_kwargs("SMALL"))
    b = g.score_views(R, T, rays=True, unknown_run=4, **vg.fan_kwargs("SMALL"))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["n_unknown"].sum() > 0 and a["n_hit"].sum() > 0 and a["n_cut"].sum() > 0


def test_no_pose_and_a_reset_map(hip_lib):
    g, o = _loaded("SMALL", fs.shell())
    e = g.score_views(np.zeros((0, 3, 3)), np.zeros((0, 3)), rays=True, **vg.fan_kwargs("SMALL"))
    assert e["n_unknown"].shape == (0,) and e["unknown_volume"].shape == (0,) and e["ray_unknown"].shape == (0, vg.H, vg.W) and e["ray_status"].shape == (0, vg.H, vg.W)
    import torch
    d = g.score_views(np.zeros((0, 3, 3)), np.zeros((0, 3)), device=True, **vg.fan_kwargs("SMALL"))
    assert d["records"].shape == (0, 16) and d["records"].is_cuda
    assert hip_lib.tsl_tsdf_view_gain(g.h, None, None, 0, None, None, None, None) == 0          # n = 0 does nothing
    torch.cuda.synchronize()
    g.reset()
    R, T = vg.scene_poses("shell", "SMALL")
    empty = {"indices": np.zeros((0, 3), np.int16), "TSDF": np.zeros(0, np.float16)}
    want = vg.scene_ref(empty, "SMALL", R, T)
    got = _both(g, R, T, "reset map", **vg.fan_kwargs("SMALL"))
    ref.assert_equal(got, want, "reset map")
    assert got["n_free"].sum() == 0 and got["n_hit"].sum() == 0 and got["n_frontier"].sum() == 0 and (got["n_range"] == vg.H * vg.W).all()
    assert want["n_outside"] > 0 and want["n_unobserved"] == 0 and got["n_unknown"].sum() == want["n_absent"]      # every sample inside the volume is unknown


def test_refusals_leave_the_handle_usable(hip_lib):
    g, o = _loaded("SMALL", fs.plate())
    L = hip_lib
    R, T = vg.scene_poses("plate", "SMALL")
    n = R.shape[0]
    Rf, Tf = np.ascontiguousarray(R.reshape(n, 9)), np.ascontiguousarray(T)
    out = np.zeros(n, ref.RECORD_DTYPE)
    ru, rs = np.zeros((n, vg.H, vg.W), np.int32), np.zeros((n, vg.H, vg.W), np.uint8)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    dp = lambda a: None if a is None else a.ctypes.data_as(_lib.dp)

    def cfg(**kw):
        c = _lib.GainCfg()
        c.K[:] = vg.K_FAN.tolist()
        c.h, c.w, c.t_min, c.t_max = vg.H, vg.W, vg.T_MIN, vg.T_MAX["SMALL"]
        for k, v in kw.items():
            if k == "K":
                c.K[:] = v
            else:
                setattr(c, k, v)
        return c

    def call(c, R=Rf, T=Tf, n=n, out=out, ru=ru, rs=rs, h=g.h, dev=False):
        """the host form, or the device form (only ever with arguments it refuses: the buffers here are host memory)"""
        fn = L.tsl_tsdf_view_gain_dev if dev else L.tsl_tsdf_view_gain
        rc = fn(h, dp(R), dp(T), n, None if c is None else C.byref(c), vp(out), vp(ru), vp(rs), *([None] if dev else []))
        return rc, L.tsl_last_error().decode()

    nan, inf = float("nan"), float("inf")
    Rbad, Tbad = Rf.copy(), Tf.copy()
    Rbad[2, 4], Tbad[1, 0] = nan, inf
    Kbad = vg.K_FAN.tolist(); Kbad[2] = inf
    bad = [("null handle", dict(h=None), cfg()), ("null argument", dict(R=None), cfg()), ("null argument", dict(T=None), cfg()), ("null argument", dict(), None),
           ("null argument", dict(out=None), cfg()), ("poses", dict(n=-1), cfg()), ("poses", dict(n=65537), cfg()),
           ("pose is not finite", dict(R=Rbad), cfg()), ("pose is not finite", dict(T=Tbad), cfg()), ("intrinsic", dict(), cfg(K=Kbad)),
           ("not finite", dict(), cfg(t_min=nan)), ("not finite", dict(), cfg(t_max=inf)), ("not finite", dict(), cfg(dt=nan)), ("free_thres", dict(), cfg(free_thres=nan)),
           ("rays per side", dict(), cfg(h=0)), ("rays per side", dict(), cfg(w=4097)), ("rays per side", dict(), cfg(h=-3)),
           ("t_max must exceed", dict(), cfg(t_min=2.0, t_max=2.0)), ("t_max must exceed", dict(), cfg(t_min=2.0, t_max=1.0)), ("dt must be positive", dict(), cfg(dt=-0.01)),
           ("1024", dict(), cfg(t_max=1024.5)), ("2^24", dict(), cfg(t_max=1000.0, dt=1e-5)), ("unknown_run", dict(), cfg(unknown_run=-1)),
           ("go together", dict(ru=None), cfg()), ("go together", dict(rs=None), cfg())]
    for word, kw, c in bad:
        rc, msg = call(c, **kw)
        assert rc == -1 and "view_gain" in msg and "view_gain_dev" not in msg and word in msg, (word, rc, msg)
        rc, msg = call(c, dev=True, **kw)
        assert rc == -1 and "view_gain_dev" in msg and word in msg, (word, rc, msg)
    with pytest.raises(_lib.TslError, match="1024"):
        g.score_views(R, T, t_max=2000.0, **{k: v for k, v in vg.fan_kwargs("SMALL").items() if k != "t_max"})
    with pytest.raises(ValueError, match="score_views"):
        g.score_views(R, T[:3], **vg.fan_kwargs("SMALL"))
    rc, msg = call(cfg(), ru=None, rs=None)                                 # no per-ray output is fine
    assert rc == 0, msg
    _check_scene(g, o, "SMALL", R, T, "after the refusals")                 # the handle is still usable
