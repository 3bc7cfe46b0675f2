"""The view gain without a GPU: the numpy restatement (tests/view_gain_ref.py) against an independent scalar per-ray loop, its
volume against the integral it is the left sum of, the shell seen from inside, frontier_view_candidates, the argument checks of the Python layer, and
that the inputs of tests/test_view_gain_gpu.py reach the branches they exist for."""
import math

import numpy as np
import pytest

import frontier_scenes as fs
import render_view_scenes as rv
import view_gain_ref as ref
import view_gain_scenes as vg
from util import SMALL

F32 = np.float32
VS = vg.VS


# ---- an independent restatement: one ray at a time, a dictionary of voxels, rnd in its truncate-and-compare form ------------------------------------
def _rnd(x):
    x = F32(x)
    r = F32(np.trunc(x))
    if abs(F32(x - r)) >= F32(0.5):
        r = F32(r + F32(math.copysign(1.0, x)))
    return int(r)


def _scalar(sc, geo, R, T, K, h, w, t_min, t_max, dt, unknown_run, thres):
    g = fs.GEOMETRIES[geo]
    N, Nz = g["N"], g["Nz"]
    vox = {tuple(int(a) for a in i): float(np.float16(t)) for i, t in zip(sc["indices"], sc["TSDF"])}
    fx, fy, cx, cy = F32(K[0]), F32(K[4]), F32(K[2]), F32(K[5])
    t_min, dt, vs = F32(t_min), F32(dt), F32(VS)
    S = int(F32(F32(t_max) - t_min) / dt) + 1
    n = R.shape[0]
    rec = np.zeros(n, ref.RECORD_DTYPE)
    ru, rs = np.zeros((n, h, w), np.int32), np.zeros((n, h, w), np.uint8)
    for k in range(n):
        Rf, Tf = R[k].reshape(9).astype(F32), T[k].astype(F32)
        for v in range(h):
            for u in range(w):
                dc = (F32(F32(u) - cx) / fx, F32(F32(v) - cy) / fy, F32(1.0))
                d = [F32(F32(F32(Rf[r * 3] * dc[0]) + F32(Rf[r * 3 + 1] * dc[1])) + F32(Rf[r * 3 + 2] * dc[2])) for r in range(3)]
                st, nu, nf, wu, wf, run, prev, front = ref.RANGE, 0, 0, 0, 0, 0, None, False
                for s in range(S):
                    t = F32(t_min + F32(F32(s) * dt))
                    p = [F32(Tf[a] + F32(t * d[a])) for a in range(3)]
                    if not all(np.isfinite(x) for x in p):
                        continue
                    i = tuple(_rnd(min(max(F32(x / vs), F32(-16777216.0)), F32(16777216.0))) for x in p)
                    if not (-N // 2 <= i[0] < N // 2 and -N // 2 <= i[1] < N // 2 and -Nz // 2 <= i[2] < Nz // 2):
                        continue
                    wt = _rnd(F32(F32(t * t) * F32(1024.0)))
                    if i in vox:
                        if F32(vox[i]) < F32(thres):
                            st = ref.HIT
                            break
                        nf += 1; wf += wt; run = 0; prev = "free"
                        continue
                    if prev == "free":
                        front = True
                    prev = "unknown"
                    nu += 1; wu += wt; run += 1
                    if unknown_run > 0 and run >= unknown_run:
                        st = ref.CUT
                        break
                ru[k, v, u], rs[k, v, u] = nu, st | (ref.FRONTIER if front else 0)
                rec["n_unknown"][k] += nu; rec["n_free"][k] += nf; rec["vol_unknown"][k] += wu; rec["vol_free"][k] += wf
                rec[("n_hit", "n_range", "n_cut")[st]][k] += 1
                rec["n_frontier"][k] += front
    return rec, ru, rs


@pytest.mark.parametrize("name", ["shell", "plate", "two_unknowns"])
def test_restatement_equals_a_scalar_loop(name):
    geo, h, w = "SMALL", 4, 5
    K = np.array([3.0, 0, 2.0, 0, 3.0, 1.5, 0, 0, 1.0])
    sc = fs.place(vg.scene(name, geo), geo)
    R, T = vg.scene_poses(name, geo)
    R, T = R[:4], T[:4]
    for run in (0, 5):
        t_max = 2.0
        want = _scalar(sc, geo, R, T, K, h, w, vg.T_MIN, t_max, ref.default_step(VS), run, ref.fref.surf_thres(VS))
        got = ref.score_export(sc, 256, 256, VS, R, T, K, h, w, vg.T_MIN, t_max, unknown_run=run)
        assert got["records"].tobytes() == want[0].tobytes(), (name, run, got["records"], want[0])
        assert np.array_equal(got["ray_unknown"], want[1]) and np.array_equal(got["ray_status"], want[2])
        assert got["records"]["n_unknown"].sum() > 0 and got["records"]["n_free"].sum() > 0
        if run:
            assert got["records"]["n_cut"].sum() > 0
    if name == "plate":
        assert got["records"]["n_hit"].sum() > 0


def test_volume_is_the_left_sum_of_the_integral():
    """An empty map, the camera at the origin, every sample inside the volume: no ray hits, every sample is unknown, and per ray L * dt, L = vol_unknown / 1024,
    lies in [I - dt * (t_S^2 - t_0^2), I] (the left sum of an increasing function), I the integral of t^2 over [t_0, t_0 + S dt], give or take
    0.5 / 1024 * S * dt for the rounding of the S weights."""
    from taichislam_amd.mapping.dense_tsdf import VIEW_GAIN_DTYPE, gain_volume
    assert VIEW_GAIN_DTYPE == ref.RECORD_DTYPE
    e = {"indices": np.zeros((0, 3), np.int16), "TSDF": np.zeros(0, np.float16)}
    t0f, t1f, dtf = F32(0.3), F32(3.0), ref.default_step(VS)
    r = ref.score_export(e, 256, 256, VS, np.eye(3)[None], np.zeros((1, 3)), vg.K_FAN, vg.H, vg.W, t0f, t1f)
    S = ref.sample_count(t0f, t1f, dtf)
    rays = vg.H * vg.W
    assert r["n_outside"] == 0 and r["status"] == [0, rays, 0] and S > 50
    assert r["n_absent"] == rays * S and (r["ray_unknown"] == S).all() and (r["ray_status"] == ref.RANGE).all()
    t0, dt = float(t0f), float(dtf)
    tS = t0 + S * dt
    integral = (tS ** 3 - t0 ** 3) / 3.0
    lo, hi, tol = integral - dt * (tS * tS - t0 * t0), integral, 0.5 / 1024.0 * S * dt
    total = int(r["records"]["vol_unknown"][0])
    assert total % rays == 0                                   # every ray has the same samples
    L = total / rays / 1024.0
    print(f"L * dt = {L * dt:.6f} in [{lo:.6f}, {hi:.6f}] +- {tol:.6f}")
    assert lo - tol <= L * dt <= hi + tol
    fxfy = float(F32(vg.K_FAN[0])) * float(F32(vg.K_FAN[4]))
    vol = gain_volume(r["records"]["vol_unknown"], dtf, vg.K_FAN[0], vg.K_FAN[4])[0]
    assert vol == ref.volume(r["records"]["vol_unknown"], dtf, vg.K_FAN)[0]
    assert rays * (lo - tol) / fxfy <= vol <= rays * (hi + tol) / fxfy


def test_shell_from_its_centre():
    from taichislam_amd.mapping.dense_tsdf import gain_poses
    sc = fs.place(fs.shell(), "SMALL")
    R, T = vg.scene_poses("shell", "SMALL")
    R, T = gain_poses(R[0], T[0])
    r = vg.scene_ref(sc, "SMALL", R.reshape(1, 3, 3), T)
    rec = r["records"][0]
    assert rec["n_free"] > 0 and rec["n_frontier"] == vg.H * vg.W and rec["n_hit"] == 0 and rec["n_range"] == vg.H * vg.W
    r = vg.scene_ref(sc, "SMALL", R.reshape(1, 3, 3), T, unknown_run=3)
    assert r["records"][0]["n_cut"] == vg.H * vg.W and (r["ray_unknown"] == 3).all() and (r["ray_status"] == (ref.CUT | ref.FRONTIER)).all()


def test_frontier_view_candidates():
    from taichislam_amd.mapping import frontier_view_candidates
    fr = {"centroid": np.array([[1.0, 2.0, 0.5], [0.0, 0.0, 0.0], [-1.0, 0.5, 0.2], [0.3, 0.3, 0.3]]),
          "normal": np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.6, -0.8, 0.0], [0.0, 0.0, 1.0]])}
    R, T = frontier_view_candidates(fr, 0.7)
    assert R.shape == (3, 3, 3) and T.shape == (3, 3)              # the cluster with a zero normal is skipped
    keep = [0, 2, 3]
    for k, c in enumerate(keep):
        assert np.allclose(R[k].T @ R[k], np.eye(3), atol=1e-12) and abs(np.linalg.det(R[k]) - 1.0) < 1e-12
        assert np.allclose(R[k][:, 2], fr["normal"][c], atol=1e-12)          # the optical axis is the direction into the unknown
        assert np.allclose(T[k] + 0.7 * fr["normal"][c], fr["centroid"][c], atol=1e-12)      # standoff metres behind the centroid
    assert R[0][2, 1] < -0.99                                    # image y points down for a level camera
    R4, T4 = frontier_view_candidates(fr, 0.7, yaws=4)
    assert R4.shape == (12, 3, 3) and T4.shape == (12, 3)
    assert np.allclose(R4[0], R[0]) and np.allclose(T4[4], T[1])
    for k in range(12):
        assert np.allclose(R4[k].T @ R4[k], np.eye(3), atol=1e-12) and abs(np.linalg.det(R4[k]) - 1.0) < 1e-12
        assert np.allclose(T4[k] + 0.7 * R4[k][:, 2], fr["centroid"][keep[k // 4]], atol=1e-12)
    assert np.allclose(R4[1][:, 2], [0.0, 1.0, 0.0], atol=1e-12) and np.allclose(R4[2][:, 2], [-1.0, 0.0, 0.0], atol=1e-12)      # quarter turns about z
    empty = frontier_view_candidates({"centroid": np.zeros((0, 3)), "normal": np.zeros((0, 3))}, 1.0)
    assert empty[0].shape == (0, 3, 3) and empty[1].shape == (0, 3)
    with pytest.raises(ValueError):
        frontier_view_candidates(fr, 0.7, yaws=0)


def test_python_argument_checks():
    from taichislam_amd.mapping.dense_tsdf import gain_config, gain_intrinsics, gain_poses
    K = np.array([200.0, 0, 159.5, 0, 210.0, 119.5, 0, 0, 1])
    k = gain_intrinsics(K, 8)
    assert k[0] == 25.0 and k[4] == 26.25 and k[2] == 160.0 / 8 - 0.5 and k[5] == 120.0 / 8 - 0.5 and k[8] == 1.0
    assert np.array_equal(k, ref.scaled_K(K, 8))
    c = gain_config(K, (240, 320), 8, unknown_run=5, skip=False)
    assert (c.h, c.w, c.unknown_run, c.flags) == (30, 40, 5, 1) and c.K[0] == 25.0 and c.t_min == 0.0 and c.dt == 0.0 and c.free_thres == 0.0
    assert (gain_config(K, (20, 24), 7).h, gain_config(K, (20, 24), 7).w) == (3, 4)
    for kw in (dict(stride=0), dict(shape=(0, 4)), dict(shape=(5000, 4)), dict(t_max=float("inf")), dict(t_max=-1.0), dict(step=0.0), dict(step=float("nan")),
               dict(free_thres=-0.1), dict(unknown_run=-1), dict(t_min=float("nan")), dict(K=np.zeros(9)), dict(K=np.ones(8))):
        with pytest.raises(ValueError, match="score_views"):
            gain_config(**dict(dict(K=K), **kw))
    with pytest.raises(ValueError, match="stride"):
        gain_config(None, (20, 24), 2)
    R, T = gain_poses(np.eye(3), np.zeros(3))
    assert R.shape == (1, 9) and T.shape == (1, 3) and R.dtype == np.float64 and R.flags.c_contiguous
    R, T = gain_poses(np.zeros((0, 3, 3)), np.zeros((0, 3)))
    assert R.shape == (0, 9) and T.shape == (0, 3)
    for Rb, Tb in ((np.eye(3), np.zeros((2, 3))), (np.zeros((2, 3, 3)), np.zeros((3, 3))), (np.zeros((2, 9)), np.zeros((2, 3))),
                   (np.full((1, 3, 3), np.nan), np.zeros((1, 3))), (np.zeros((1, 3, 3)), np.full((1, 3), np.inf))):
        with pytest.raises(ValueError, match="score_views"):
            gain_poses(Rb, Tb)


# ---- the inputs of the GPU tests reach the branches they exist for --------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", ["SMALL", "SLAB", "TALL"])
def test_scene_inputs_reach_their_branches(geo):
    for name in vg.SCENE_NAMES:
        sc = fs.place(vg.scene(name, geo), geo)
        R, T = vg.scene_poses(name, geo)
        r = vg.scene_ref(sc, geo, R, T)
        rec = r["records"]
        assert (rec["n_unknown"] > 0)[[1, 3, 4] if name == "wall" else slice(None)].all() and rec["n_free"][:3].min() > 0, (geo, name, rec)      # (wall: the fan along +x sees the block, then the outside)
        assert rec["n_free"][3] > 0 and rec["n_free"][4] > 0, (geo, name, "the poses outside look in")
        assert vg.scene_ref(sc, geo, R[4:], T[4:])["n_outside"] > 0          # the pose outside the volume
        if name == "two_unknowns":
            assert r["n_absent"] > 0 and r["n_unobserved"] > 0
        if name == "plate":
            assert rec["n_hit"].sum() > 0
        if name == "wall":
            assert vg.scene_ref(sc, geo, R[:1], T[:1])["n_outside"] > 0      # from the block's centre towards the wall of the volume
        if name == "two_values":
            b = vg.scene_ref(sc, geo, R, T, free_thres=0.2)["records"]
            assert b["n_hit"].sum() > rec["n_hit"].sum() and b["n_free"].sum() < rec["n_free"].sum()
        if name in ("shell", "two_unknowns"):
            for run in (1, 7):
                c = vg.scene_ref(sc, geo, R, T, unknown_run=run)
                assert c["records"]["n_cut"].sum() > 0 and c["cut_in_absent"] > 0, (geo, name, run)


def test_room_inputs_reach_their_branches():
    K, frames = rv.room_scene()
    o = rv.room_oracle(K, frames)
    R, T = vg.room_poses()
    assert R.shape[0] == 71
    r = vg.room_ref(o.export_sparse(), o.N, o.Nz, K, R, T)
    rec = r["records"]
    assert r["ray_unknown"].shape == (71, 20, 24)
    assert rec["n_hit"].max() > 0 and rec["n_range"].max() > 0 and rec["n_frontier"].max() > 0
    assert r["n_absent"] > 0 and r["n_unobserved"] > 0
