"""k_depth_condition and k_depth_halve (csrc/tsl_depth.hip) against the numpy restatement of tests/depth_condition_ref.py: depth, status, counts and every
level byte for byte, through the host-pointer form and the device form, on frames that end inside a tile, at a tile, one pixel past it and in one row or
column; the argument errors with their outputs untouched; and the maps a DenseTSDF builds from raw and from conditioned frames against the oracle's."""
import ctypes as C

import numpy as np
import pytest

import depth_condition_ref as ref
import depth_condition_scenes as sc

pytestmark = pytest.mark.gpu

CFGS = [dict(),
        dict(radius=0, erode=0, min_support=0),
        dict(radius=4, erode=3, min_support=8, flags=1, min_valid=1),
        dict(radius=4, erode=0, d_min_mm=900, d_max_mm=4000, min_valid=4),
        dict(radius=1, erode=3, min_valid=3),
        dict(radius=3, erode=2)]
SHAPES = [(1, 1), (1, 70), (70, 1), (32, 64), (33, 65), (37, 53), (120, 160)]       # (32, 64) is exactly one tile


@pytest.fixture(scope="module")
def dc(hip_lib):
    from taichislam_amd.mapping import DepthConditioner
    return DepthConditioner(0, sc.TOL, sc.WS, sc.WR)


def _torch_in(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _np_out(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _run(dc, d, cfg, device):
    kw = dict(min_support=cfg.get("min_support", 6), erode=cfg.get("erode", 1), radius=cfg.get("radius", 2), erode_holes=bool(cfg.get("flags", 0)),
              levels=cfg.get("levels", 0), min_valid=cfg.get("min_valid", 2), status=True)
    if "d_min_mm" in cfg:
        kw.update(d_min=cfg["d_min_mm"] / 1000.0, d_max=cfg["d_max_mm"] / 1000.0)
    r = dc.condition(_torch_in(d) if device else d, **kw)
    if device:
        r = {"depth": _np_out(r["depth"]), "status": _np_out(r["status"]), "counts": _np_out(r["counts"]), "levels": [_np_out(l) for l in r["levels"]]}
    return r


def _check(dc, d, tol, cfg, what):
    want = ref.condition_np(d, tol, sc.WS, sc.WR, **cfg)
    for device in (False, True):
        got = _run(dc, d, cfg, device)
        w = f"{what} {cfg} {'device' if device else 'host'} form"
        for k in ("depth", "status", "counts"):
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, f"{w}: {k} is {got[k].dtype} {got[k].shape}"
            bad = np.argwhere(got[k] != want[k])
            assert bad.size == 0, f"{w}: {k} differs at {len(bad)} places, first {bad[0]}: {got[k][tuple(bad[0])]} != {want[k][tuple(bad[0])]}"
        assert len(got["levels"]) == len(want["levels"])
        for l, (a, b) in enumerate(zip(got["levels"], want["levels"])):
            assert a.shape == b.shape and np.array_equal(a, b), f"{w}: level {l + 1} differs"


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_plane_equals_the_restatement(dc, shape, n):
    h, w = shape
    d = sc.random_frames(n, h, w, seed=1000 * n + h + w)
    assert h * w * n < 3 or {0, 1, 65535} <= set(np.unique(d).tolist())
    levels = min(3, int(np.log2(min(h, w))))
    for cfg in CFGS:
        _check(dc, d, sc.TOL, dict(cfg, levels=levels), f"{n} x {h} x {w}")


@pytest.mark.parametrize("which", ["one", "max"])
def test_the_extreme_tolerances(hip_lib, which):
    from taichislam_amd.mapping import DepthConditioner
    tol = sc.TOL_1 if which == "one" else sc.TOL_MAX
    own = DepthConditioner(0, tol, sc.WS, sc.WR)
    d = sc.random_frames(3, 37, 53, seed=77)
    for cfg in (CFGS[0], CFGS[2], CFGS[3]):
        _check(own, d, tol, dict(cfg, levels=3), f"tol {which}")


def test_hand_built_frames_and_a_single_frame_keeps_its_shape(dc):
    for f in (sc.spike(), sc.vertical_step(), sc.with_hole(), sc.ramp(40, 70), sc.constant(33, 65)):
        for cfg in (CFGS[0], CFGS[2]):
            _check(dc, f, sc.TOL, dict(cfg, levels=2), "hand-built")
    r = dc.condition(sc.spike(), levels=1, status=True)
    assert r["depth"].shape == (15, 17) and r["status"].shape == (15, 17) and r["counts"].shape == (5,) and r["levels"][0].shape == (7, 8)
    r = dc.condition(_torch_in(sc.spike()))
    assert r["depth"].is_cuda and tuple(r["depth"].shape) == (15, 17) and r["status"] is None and r["levels"] == []


def _cfg(n, h, w, **kw):
    from taichislam_amd import _lib
    c = dict(ref.DEFAULTS, **kw)
    return _lib.DepthCfg(n, h, w, c["d_min_mm"], c["d_max_mm"], c["min_support"], c["erode"], c["radius"], c["flags"], c["levels"], c["min_valid"], 0)


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_status_counts_and_levels_left_out(dc, hip_lib):
    import torch
    d = sc.random_frames(2, 37, 53, seed=5)
    want = ref.condition_np(d, sc.TOL, sc.WS, sc.WR, levels=3)
    cfg = _cfg(2, 37, 53, levels=3)
    # host form: only out and level 2; level 1 is computed in the handle's own buffer, level 3 is not computed
    out, l2 = np.zeros_like(d), np.zeros((2, 9, 13), np.uint16)
    assert hip_lib.tsl_depth_condition(dc.h, C.byref(cfg), _vp(d), _vp(out), None, None, None, _vp(l2), None) == 0, hip_lib.tsl_last_error()
    assert np.array_equal(out, want["depth"]) and np.array_equal(l2, want["levels"][1])
    # out alone
    out2 = np.zeros_like(d)
    assert hip_lib.tsl_depth_condition(dc.h, C.byref(cfg), _vp(d), _vp(out2), None, None, None, None, None) == 0
    assert np.array_equal(out2, want["depth"])
    # device form: out, counts and level 3
    dd = _torch_in(d)
    o, c, l3 = torch.zeros_like(dd), torch.full((2, 5), -1, dtype=torch.int64, device="cuda"), torch.zeros((2, 4, 6), dtype=torch.int16, device="cuda")
    rc = hip_lib.tsl_depth_condition_dev(dc.h, C.byref(cfg), dd.data_ptr(), o.data_ptr(), None, c.data_ptr(), None, None, l3.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip_lib.tsl_last_error()
    assert np.array_equal(_np_out(o), want["depth"]) and np.array_equal(_np_out(c), want["counts"]) and np.array_equal(_np_out(l3), want["levels"][2])
    # a level pointer above cfg.levels is ignored
    cfg0 = _cfg(2, 37, 53, levels=0)
    keep = np.full((2, 18, 26), 0xabab, np.uint16)
    assert hip_lib.tsl_depth_condition(dc.h, C.byref(cfg0), _vp(d), _vp(out2), None, None, _vp(keep), None, None) == 0
    assert (keep == 0xabab).all()


BAD_CFGS = [("n", dict(), dict(n=0)), ("n", dict(), dict(n=65)), ("h", dict(), dict(h=0)), ("w", dict(), dict(w=8193)), ("n h w", dict(), dict(n=64, h=8192, w=8192)),
            ("d_min_mm", dict(d_min_mm=3000, d_max_mm=2999), {}), ("min_support", dict(min_support=9), {}), ("min_support", dict(min_support=-1), {}),
            ("erode", dict(erode=4), {}), ("erode", dict(erode=-1), {}), ("radius", dict(radius=5), {}), ("radius", dict(radius=-1), {}), ("flag", dict(flags=2), {}),
            ("levels", dict(levels=4), {}), ("levels", dict(levels=-1), {}), ("min_valid", dict(min_valid=0), {}), ("min_valid", dict(min_valid=5), {}),
            ("no pixels", dict(levels=3), {})]                                   # 6 x 9: level 3 would be 0 x 1


def test_argument_errors_leave_the_outputs_untouched(dc, hip_lib):
    import torch
    from taichislam_amd import _lib
    L = hip_lib
    n, h, w = 2, 6, 9
    d = sc.random_frames(n, h, w, seed=3)
    dd = _torch_in(d)
    stream = torch.cuda.current_stream().cuda_stream

    def fresh():
        host = [np.full((n, h, w), 0xabab, np.uint16), np.full((n, h, w), 0xab, np.uint8), np.full((n, 5), -7, np.int64), np.full((n, 3, 4), 0xabab, np.uint16)]
        dev = [torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda() for a in host]
        return host, dev

    def refused(cfg, handle=None, depth="d", out="o", where="", alias=False):
        handle = dc.h if handle is None else handle
        host, dev = fresh()
        before = [a.copy() for a in host]
        cp = None if cfg is None else C.byref(cfg)
        o_host = d if alias else host[0]
        rc = L.tsl_depth_condition(handle, cp, _vp(d) if depth else None, _vp(o_host) if out else None, _vp(host[1]), _vp(host[2]), _vp(host[3]), None, None)
        assert rc == -1 and b"tsl_depth_condition:" in L.tsl_last_error() and where.encode() in L.tsl_last_error(), (rc, L.tsl_last_error())
        o_dev = dd if alias else dev[0]
        rc = L.tsl_depth_condition_dev(handle, cp, dd.data_ptr() if depth else None, o_dev.data_ptr() if out else None, dev[1].data_ptr(), dev[2].data_ptr(),
                                       dev[3].data_ptr(), None, None, stream)
        assert rc == -1 and b"tsl_depth_condition_dev:" in L.tsl_last_error() and where.encode() in L.tsl_last_error(), (rc, L.tsl_last_error())
        torch.cuda.synchronize()
        for a, b, c in zip(before, host, dev):
            assert np.array_equal(a, b) and np.array_equal(a, _np_out(c)), "an output was written"
        assert np.array_equal(_np_out(dd), d)

    good = _cfg(n, h, w, levels=1)
    refused(good, handle=C.c_void_p(None), where="null handle")
    refused(None, where="null")
    refused(good, depth=None, where="null")
    refused(good, out=None, where="null")
    refused(good, alias=True, where="overlaps")
    for where, kw, dims in BAD_CFGS:
        c = _cfg(n, h, w, **kw)
        for k, v in dims.items():
            setattr(c, k, v)
        refused(c, where=where)
    # tables: not set, and out of range (the handle keeps the tables it had)
    bare = C.c_void_p()
    assert L.tsl_depth_create(0, C.byref(bare)) == 0
    try:
        refused(good, handle=bare, where="tables")
        bad_tol = sc.TOL.copy()
        bad_tol[17] = 0
        big_tol = sc.TOL.copy()
        big_tol[200] = 32768
        ws0 = sc.WS.copy()
        ws0[0, 0] = 0
        for tol, ws, wr in ((bad_tol, sc.WS, sc.WR), (big_tol, sc.WS, sc.WR), (sc.TOL, ws0, sc.WR), (None, sc.WS, sc.WR)):
            assert L.tsl_depth_set_tables(bare, _vp(tol), _vp(ws), _vp(wr)) == -1 and b"tsl_depth_set_tables" in L.tsl_last_error()
        refused(good, handle=bare, where="tables")
    finally:
        L.tsl_depth_destroy(bare)
    with pytest.raises(_lib.TslError):
        dc.set_tables(tol=bad_tol)
    _check(dc, d, sc.TOL, dict(levels=1), "after the refused tables")


def test_end_to_end_flying_pixels_leave_the_map(dc):
    """A box in front of a wall with flying pixels on the box's silhouette (depth_condition_scenes.box_wall_scene): the raw frames leave occupied voxels in
    the empty gap behind the flying pixels, the conditioned frames none, and wall and box face stay.  The counts equal the oracle's, whose maps
    tests/test_depth_condition_cpu.py checks."""
    from taichislam_amd.mapping import DenseTSDF
    from util import SMALL
    K, R, poses, frames, probes = sc.box_wall_scene()
    want = sc.e2e_oracle_counts()
    assert want["raw"]["gap"] > 0 and want["cond"]["gap"] == 0 and min(want[m][k] for m in ("raw", "cond") for k in ("wall", "box")) > 0
    raw = _torch_in(frames)
    cond = dc.condition(raw)["depth"]                               # one launch for the four frames, on the device
    assert np.array_equal(_np_out(cond), sc.e2e_conditioned_ref())
    for name, fr in (("raw", raw), ("cond", cond)):
        m = DenseTSDF(**SMALL, device=0)
        m.set_dep_camera_intrinsic(K)
        for f, T in zip(fr, poses):
            m.recast_depth_to_map(R, T, f, None)                    # a device tensor each: nothing leaves the device between conditioning and integration
        got = {k: int(np.asarray(m.is_pos_occupy(p)).sum()) for k, p in probes.items()}
        assert got == want[name], f"{name}: {got} != {want[name]}"
