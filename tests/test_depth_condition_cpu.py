"""The depth conditioning's definition, without a GPU: the two restatements of tests/depth_condition_ref.py against each other and against what the
definition promises on hand-built frames (tests/depth_condition_scenes.py), the helpers of taichislam_amd.utils, the bound symbols, and the oracle's maps of
the end-to-end scene that tests/test_depth_condition_gpu.py compares the HIP maps with."""
import os
import re

import numpy as np
import pytest

import depth_condition_ref as ref
import depth_condition_scenes as sc
from taichislam_amd.utils import bilateral_tables, depth_tolerance, halved_intrinsics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEPT, HOLE, RANGE, SPARSE, EDGE = range(5)


def _same(a, b, what):
    for k in ("depth", "status", "counts"):
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs"
    assert len(a["levels"]) == len(b["levels"])
    for l, (x, y) in enumerate(zip(a["levels"], b["levels"])):
        assert x.shape == y.shape and np.array_equal(x, y), f"{what}: level {l + 1} differs"


CONFIGS = [dict(), dict(radius=4, erode=3, flags=1, min_valid=1), dict(min_support=8, radius=0, erode=0), dict(min_support=0, radius=1, d_min_mm=900, d_max_mm=4000),
           dict(radius=3, erode=2, min_valid=4)]


@pytest.mark.parametrize("shape", [(2, 9, 11), (1, 1, 1), (1, 1, 7), (1, 6, 1), (2, 13, 16)])
def test_the_two_restatements_agree_on_random_frames(shape):
    n, h, w = shape
    d = sc.random_frames(n, h, w, seed=h * w)
    levels = min(3, int(np.log2(min(h, w))))
    for kw in CONFIGS:
        for tol in (sc.TOL, sc.TOL_1, sc.TOL_MAX):
            _same(ref.condition_np(d, tol, sc.WS, sc.WR, levels=levels, **kw), ref.condition_loop(d, tol, sc.WS, sc.WR, levels=levels, **kw), f"{shape} {kw}")


def test_the_two_restatements_agree_on_the_hand_built_frames():
    for f in (sc.spike(), sc.vertical_step(), sc.with_hole(), sc.ramp(10, 14), sc.constant(5, 6)):
        for kw in CONFIGS:
            _same(ref.condition_np(f, sc.TOL, sc.WS, sc.WR, levels=2, **kw), ref.condition_loop(f, sc.TOL, sc.WS, sc.WR, levels=2, **kw), str(kw))


def test_a_constant_frame_comes_back_unchanged():
    rng = np.random.default_rng(5)
    f = sc.constant(9, 12, 2345)
    for radius in range(5):
        ws = rng.integers(0, 256, (5, 5)).astype(np.uint8)
        wr = rng.integers(0, 256, 17).astype(np.uint8)
        ws[0, 0], wr[0] = max(ws[0, 0], 1), max(wr[0], 1)
        tol = rng.integers(1, 32768, 256).astype(np.uint16)
        # min_support 3: a corner pixel has three neighbours, so nothing is SPARSE and the whole frame is KEPT
        r = ref.condition_np(f, tol, ws, wr, radius=radius, min_support=3, levels=2)
        assert np.array_equal(r["depth"], f) and (r["status"] == KEPT).all() and r["counts"].tolist() == [f.size, 0, 0, 0, 0]
        assert np.array_equal(r["levels"][0], sc.constant(4, 6, 2345)) and np.array_equal(r["levels"][1], sc.constant(2, 3, 2345))


@pytest.mark.parametrize("erode", [0, 1, 3])
def test_pixels_with_a_clean_neighbourhood_are_kept(erode):
    d = sc.random_frames(2, 24, 31, seed=9)
    kw = dict(erode=erode, d_min_mm=500, d_max_mm=6000)
    r = ref.condition_np(d, sc.TOL, sc.WS, sc.WR, **kw)
    m = 1 + erode
    for f in range(d.shape[0]):
        for y in range(m, d.shape[1] - m):
            for x in range(m, d.shape[2] - m):
                win = d[f, y - m:y + m + 1, x - m:x + m + 1].astype(np.int64)
                # in range and within the tightest tolerance any pixel of the window has, of the centre: every pixel of the inner window then has 8 supporters
                lo = min(int(sc.TOL[v >> 8]) for v in win.reshape(-1))
                if win.min() >= 500 and win.max() <= 6000 and (win.max() - win.min()) <= lo:
                    assert r["status"][f, y, x] == KEPT
    flat = ref.condition_np(sc.ramp(24, 31), sc.TOL, sc.WS, sc.WR, erode=erode)
    assert (flat["status"][m:-m, m:-m] == KEPT).all()                     # a slanted plane: every such window is clean


@pytest.mark.parametrize("erode", [0, 1, 2, 3])
def test_a_spike_is_sparse_and_its_ring_is_edge(erode):
    y, x = 10, 11
    f = sc.spike(21, 23, y, x)
    yy, xx = np.mgrid[0:21, 0:23]
    cheb = np.maximum(np.abs(yy - y), np.abs(xx - x))
    near = cheb <= 5                                   # clear of the image border, whose pixels lack neighbours and are SPARSE themselves
    r = ref.condition_np(f, sc.TOL, sc.WS, sc.WR, erode=erode, min_support=6)
    st = r["status"]
    assert st[y, x] == SPARSE and r["depth"][y, x] == 0
    assert (st[(cheb >= 1) & (cheb <= erode)] == EDGE).all()        # the spike's neighbours keep 7 supporters: only the spike is a seed
    assert (st[near & (cheb > erode)] == KEPT).all()
    assert (r["depth"][near & (cheb > erode)] == 2000).all() and (r["depth"][cheb <= erode] == 0).all()
    # min_support 8: the spike's 8 neighbours lack one supporter each and are SPARSE too, the ring moves out by one
    st8 = ref.condition_np(f, sc.TOL, sc.WS, sc.WR, erode=erode, min_support=8)["status"]
    assert (st8[cheb <= 1] == SPARSE).all() and (st8[(cheb >= 2) & (cheb <= 1 + erode)] == EDGE).all() and (st8[near & (cheb > 1 + erode)] == KEPT).all()


def test_a_vertical_step_gives_a_sparse_column_on_each_side():
    f = sc.vertical_step()
    st = ref.condition_np(f, sc.TOL, sc.WS, sc.WR, erode=0, min_support=6)["status"]
    assert (st[1:-1, 9] == SPARSE).all() and (st[1:-1, 10] == SPARSE).all()      # 5 supporters each
    assert (st[1:-1, 2:9] == KEPT).all() and (st[1:-1, 11:-2] == KEPT).all()
    st5 = ref.condition_np(f, sc.TOL, sc.WS, sc.WR, erode=0, min_support=5)["status"]
    assert (st5[1:-1, 1:-1] == KEPT).all()                                       # 5 supporters are enough at min_support 5


def test_a_hole_erodes_only_with_the_flag():
    f = sc.with_hole(17, 17, 8, 8)
    yy, xx = np.mgrid[0:17, 0:17]
    cheb = np.maximum(np.abs(yy - 8), np.abs(xx - 8))
    a = ref.condition_np(f, sc.TOL, sc.WS, sc.WR, erode=2, min_support=6, flags=0)
    b = ref.condition_np(f, sc.TOL, sc.WS, sc.WR, erode=2, min_support=6, flags=1)
    assert a["status"][8, 8] == HOLE and b["status"][8, 8] == HOLE and a["counts"][HOLE] == 1 and b["counts"][HOLE] == 1
    assert (a["status"][(cheb >= 1) & (cheb <= 3)] == KEPT).all()                 # 7 supporters: not SPARSE, and a hole is no seed
    assert (b["status"][(cheb >= 1) & (cheb <= 2)] == EDGE).all() and (b["status"][cheb == 3] == KEPT).all()
    assert b["counts"][EDGE] - a["counts"][EDGE] == 24


def test_the_clamp_at_1_and_65535():
    ws = np.zeros((5, 5), np.uint8)
    ws[:2, :2] = 255
    wr = np.full(17, 255, np.uint8)
    wr[0] = 1                                                    # the centre weighs little: the offset follows the neighbours
    lo = np.full((7, 7), 1, np.uint16)
    hi = np.full((7, 7), 65535, np.uint16)
    for f in (lo, hi):
        r = ref.condition_np(f, sc.TOL_MAX, ws, wr, radius=1, min_support=0, erode=0)
        assert np.array_equal(r["depth"], f)
    # a pixel pulled below 1 / above 65535 by its members cannot leave the range: with these depths the unclamped value stays inside, and the loop form agrees
    f = lo.copy()
    f[3, 3] = 3
    _same(ref.condition_np(f, sc.TOL_MAX, ws, wr, radius=1, min_support=0, erode=0), ref.condition_loop(f, sc.TOL_MAX, ws, wr, radius=1, min_support=0, erode=0), "low")
    r = ref.condition_np(f, sc.TOL_MAX, ws, wr, radius=1, min_support=0, erode=0)["depth"]
    assert r.min() >= 1 and r[3, 3] == 1                         # off = floor((2 * 8 * 255 * 255 * (-2) + den) / (2 den)) = -2
    g = hi.copy()
    g[3, 3] = 65533
    r = ref.condition_np(g, sc.TOL_MAX, ws, wr, radius=1, min_support=0, erode=0)["depth"]
    assert r.max() == 65535 and r[3, 3] == 65535


def test_the_halve_rule():
    tol = sc.TOL
    step = np.array([[1500, 3000], [1500, 3000]], np.uint16)                      # the foreground wins across a step
    assert ref.halve_np(step, tol, 2).tolist() == [[1500]]
    mixed = np.array([[1500, 1503], [1506, 3000]], np.uint16)
    assert ref.halve_np(mixed, tol, 1).tolist() == [[1503]]                       # floor((2 * 4509 + 3) / 6)
    assert ref.halve_np(np.array([[1500, 1501], [0, 0]], np.uint16), tol, 2).tolist() == [[1501]]      # floor((2 * 3001 + 2) / 4): halves round up
    one = np.array([[0, 0], [0, 2000]], np.uint16)
    assert ref.halve_np(one, tol, 1).tolist() == [[2000]] and ref.halve_np(one, tol, 2).tolist() == [[0]]
    three = np.array([[2000, 0], [2001, 2002]], np.uint16)
    assert ref.halve_np(three, tol, 3).tolist() == [[2001]] and ref.halve_np(three, tol, 4).tolist() == [[0]]
    odd = np.arange(1, 36, dtype=np.uint16).reshape(5, 7) + 1000                  # an odd last row and column are dropped
    assert ref.halve_np(odd, tol, 2).shape == (2, 3)
    assert ref.halve_np(np.full((2, 2), 65535, np.uint16), sc.TOL_MAX, 4).tolist() == [[65535]]


def test_halved_intrinsics_reproject_the_block_centre():
    K = np.array([384.2, 0.0, 323.5, 0.0, 380.1, 235.1, 0.0, 0.0, 1.0])
    for level in (1, 2, 3):
        Kl = halved_intrinsics(K, level)
        s = 2 ** level
        for I, J in ((0, 0), (5, 7), (30, 11)):
            # the centre of the s x s block of source pixels that halved pixel (I, J) covers, in source pixel coordinates
            u, v = s * I + (s - 1) / 2.0, s * J + (s - 1) / 2.0
            ray0 = ((u - K[2]) / K[0], (v - K[5]) / K[4])
            ray1 = ((I - Kl[2]) / Kl[0], (J - Kl[5]) / Kl[4])
            assert np.allclose(ray0, ray1, rtol=0, atol=1e-12)
    assert halved_intrinsics(K.reshape(3, 3), 1).shape == (3, 3) and np.array_equal(halved_intrinsics(K, 0), K)


def test_the_helpers_tables_meet_the_ranges():
    for args in ((), (0.001, 0.0, 0.0), (0.02, 0.01, 0.5), (0.0, 0.0, 0.0)):
        t = depth_tolerance(*args)
        assert t.dtype == np.uint16 and t.shape == (256,) and t.min() >= 1 and t.max() <= 32767
    assert depth_tolerance()[0] == 10 and depth_tolerance()[255] == np.clip(np.rint(10 + 5 * 65.4075 ** 2), 1, 32767)
    for radius in range(5):
        ws, wr = bilateral_tables(radius)
        assert ws.dtype == np.uint8 and ws.shape == (5, 5) and wr.dtype == np.uint8 and wr.shape == (17,)
        assert ws[0, 0] == 255 and wr[0] == 255 and np.array_equal(ws, ws.T)
        assert (ws[radius + 1:] == 0).all() and (np.diff(wr.astype(int)) <= 0).all()
    with pytest.raises(ValueError):
        bilateral_tables(5)


def test_the_new_symbols_are_declared_and_bound():
    from taichislam_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "taichislam_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in ("tsl_depth_create", "tsl_depth_destroy", "tsl_depth_set_tables", "tsl_depth_condition", "tsl_depth_condition_dev"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert len(_lib.SIGNATURES["tsl_depth_condition_dev"][1]) == len(_lib.SIGNATURES["tsl_depth_condition"][1]) + 1
    import ctypes as C
    assert C.sizeof(_lib.DepthCfg) == 48
    from taichislam_amd.mapping import DepthConditioner  # noqa: F401
    # argument errors come before any device work: a null handle is refused by name
    cfg = _lib.DepthCfg(1, 4, 4, 1, 65535, 6, 1, 2, 0, 0, 2, 0)
    assert L.tsl_depth_condition(None, C.byref(cfg), None, None, None, None, None, None, None) == -1 and b"tsl_depth_condition" in L.tsl_last_error()
    assert L.tsl_depth_set_tables(None, None, None, None) == -1 and b"tsl_depth_set_tables" in L.tsl_last_error()
    L.tsl_depth_destroy(None)


def test_the_oracle_maps_of_the_end_to_end_scene():
    """What tests/test_depth_condition_gpu.py holds the HIP maps to: in the oracle's map of the raw frames the flying pixels leave occupied voxels in the
    empty gap between box and wall, in its map of the conditioned frames (the restatement's output) none; wall and box face are occupied in both."""
    c = sc.e2e_oracle_counts()
    assert c["raw"]["gap"] > 0 and c["cond"]["gap"] == 0
    for k in ("wall", "box"):
        assert c["raw"][k] > 0 and c["cond"][k] > 0
