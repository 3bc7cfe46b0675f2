"""Evict / snapshot / restore of TSDF bricks on the GPU (tsl_evict.hip) against the numpy restatement tests/evict_ref.py and the map's independent view,
export_submap() sorted by voxel.  Hand-built maps are loaded one brick per load_numpy call, so that the pool index of a brick is its place in the load order.
Every assertion on map content is an equality of bytes or integers."""
import ctypes as C

import numpy as np
import pytest

import evict_ref as er
from taichislam_amd import _lib
from util import SLAB, TALL, assert_export_equal, make_pair, tall_stream

pytestmark = pytest.mark.gpu

GEO = {"TALL": (TALL, 64, 128), "SLAB": (SLAB, 144, 48)}
VS = TALL["voxel_scale"]
PLANES = ("keys", "tw", "obs", "occ")


def mk(geo="TALL", max_bricks=64, **kw):
    from taichislam_amd.mapping import DenseTSDF
    cfg, N, Nz = GEO[geo]
    g = DenseTSDF(**dict(cfg, **kw), max_bricks=max_bricks)
    assert (g.N, g.Nz) == (N, Nz)
    return g


def brick_scene(key, geo="TALL", nvox=3, seed=0):
    """a few voxels of brick `key` with values that name the brick and the voxel"""
    _, N, Nz = GEO[geo]
    s, lo, _ = er.brick_range([key], N, Nz)
    rng = np.random.default_rng(1000 * seed + key)
    loc = np.sort(rng.choice(4096, nvox, replace=False))
    idx = lo[0] + np.stack([loc >> 8, (loc >> 4) & 15, loc & 15], -1)
    n = np.arange(nvox)
    return {"sid": int(s[0]), "indices": idx.astype(np.int16), "TSDF": (((key % 97) * 8 + n % 8 + 1) / 1024.0).astype(np.float16),
            "W_TSDF": (1 + (key + n) % 13).astype(np.float16), "occupy": ((key + n) % 5 - 2).astype(np.int8), "color": rng.random((nvox, 3)).astype(np.float16)}


def load(g, keys, geo="TALL", **kw):
    """one load_numpy call per brick, in the order given -> {key: scene}"""
    out = {}
    for k in keys:
        sc = brick_scene(int(k), geo, **kw)
        g.load_numpy(sc["sid"], sc["indices"], sc["TSDF"], sc["W_TSDF"], sc["occupy"], sc["color"] if g.enable_texture else None)
        out[int(k)] = sc
    return out


def expected_export(scenes, keys, sid, textured=False):
    """the export_submap() of slot sid that holds the scenes of `keys`"""
    ks = [k for k in keys if scenes[k]["sid"] == sid]
    cat = lambda f, shape, dt: np.concatenate([scenes[k][f] for k in ks]) if ks else np.zeros(shape, dt)
    e = {"indices": cat("indices", (0, 3), np.int16), "TSDF": cat("TSDF", 0, np.float16), "W_TSDF": cat("W_TSDF", 0, np.float16), "occupy": cat("occupy", 0, np.int8)}
    if textured:
        e["color"] = cat("color", (0, 3), np.float16)
    return e


def check_export(g, scenes, keys, sids=(0,), what=""):
    for s in sids:
        g.active_submap_id[None] = s
        assert_export_equal(g.export_submap(), expected_export(scenes, keys, s, g.enable_texture), f"{what} slot {s}")
    g.active_submap_id[None] = 0


def expected_planes(scenes, keys, geo="TALL", textured=False):
    """the payload of the bricks `keys`: ascending keys, the loaded values at their local index, zero elsewhere"""
    _, N, Nz = GEO[geo]
    keys = sorted(keys)
    n = len(keys)
    p = {"keys": np.array(keys, np.int32).reshape(n), "tw": np.zeros((n, 4096), np.uint32), "obs": np.zeros((n, 4096), np.int8), "occ": np.zeros((n, 4096), np.int8)}
    if textured:
        p["col"] = np.zeros((n, 4096, 4), np.uint16)
    for r, k in enumerate(keys):
        sc = scenes[k]
        l = er.local_index(sc["indices"], N, Nz)
        assert np.array_equal(er.key_of_voxel(sc["indices"], sc["sid"], N, Nz), np.full(l.shape, k))
        p["tw"][r, l] = sc["TSDF"].view(np.uint16).astype(np.uint32) | (sc["W_TSDF"].view(np.uint16).astype(np.uint32) << 16)
        p["obs"][r, l] = 1
        p["occ"][r, l] = sc["occupy"]
        if textured:
            p["col"][r, l, :3] = sc["color"].view(np.uint16)
    return p


def assert_planes_equal(a, b, what=""):
    names = PLANES + (("col",) if "col" in a or "col" in b else ())
    for k in names:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, f"{what}: {k} {a[k].dtype} {a[k].shape} vs {b[k].dtype} {b[k].shape}"
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


def payload_to_export(p, geo="TALL"):
    """the observed voxels of a payload as an export dict"""
    _, N, Nz = GEO[geo]
    _, lo, _ = er.brick_range(p["keys"], N, Nz)
    r, l = np.nonzero(p["obs"] > 0)
    idx = lo[r] + np.stack([l >> 8, (l >> 4) & 15, l & 15], -1)
    tw = p["tw"][r, l]
    return {"indices": idx.astype(np.int16), "TSDF": (tw & 0xffff).astype(np.uint16).view(np.float16), "W_TSDF": (tw >> 16).astype(np.uint16).view(np.float16),
            "occupy": p["occ"][r, l]}


def to_host(p):
    """a device payload as numpy arrays (the unsigned planes through the signed view of the same width)"""
    import torch
    want = {"keys": np.int32, "tw": np.uint32, "obs": np.int8, "occ": np.int8, "col": np.uint16}
    out = dict(p)
    for k, dt in want.items():
        if k in p:
            t = p[k]
            t = t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int16) if t.element_size() == 2 else t
            out[k] = t.cpu().numpy().view(dt)
    return out


KEYS12 = [77, 5, 130, 41, 9, 300, 64, 18, 255, 2, 190, 101]          # three slots of 128 bricks each, in no order

LAYOUTS = {"below": [0, 1, 2], "above": [9, 10, 11], "interleaved": [1, 4, 7, 10], "single": [5], "everything": list(range(12)), "nothing": []}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_pool_layouts(hip_lib, layout):
    g = mk()
    scenes = load(g, KEYS12)
    before = g.brick_keys()
    assert before.tolist() == KEYS12 and g.bricks_in_use() == 12
    sel = np.zeros(12, bool)
    sel[LAYOUTS[layout]] = True
    want_owner, moves, want_keys = er.plan(before, sel)
    ev = g.evict(keys=before[sel])
    st = ev["stats"]
    assert (st["selected"], st["missing"], st["moved"], st["bricks_before"], st["bricks_after"]) == (int(sel.sum()), 0, len(moves), 12, len(want_owner))
    assert layout != "above" or st["moved"] == 0
    assert g.brick_keys().tolist() == want_owner.tolist() and g.bricks_in_use() == len(want_owner)
    assert ev["keys"].tolist() == want_keys.tolist() and (np.diff(ev["keys"]) > 0).all()
    assert_planes_equal(ev, expected_planes(scenes, before[sel].tolist()), layout)
    check_export(g, scenes, want_owner.tolist(), (0, 1, 2), layout)
    # the table follows the moves: a snapshot by key finds every kept brick, and its bytes are the loaded ones
    assert_planes_equal(g.snapshot_bricks(), expected_planes(scenes, want_owner.tolist()), layout + " remainder")


BOX_BRICKS = {0: [(0, 0, 0), (1, 0, 0), (1, 1, 3), (2, 2, 4), (3, 3, 7)], 1: [(1, 0, 0), (2, 1, 1)], 2: [(0, 0, 0)]}


def box_keys(geo="TALL"):
    _, N, Nz = GEO[geo]
    return [int(er.make_key(s, *b, N, Nz)) for s in sorted(BOX_BRICKS) for b in BOX_BRICKS[s]]


# the border between bricks 0 and 1 of the x axis of TALL lies between voxels -17 and -16; the boxes end on it and one voxel either side of it
@pytest.mark.parametrize("rule", ["keep_box", "clear_box"])
@pytest.mark.parametrize("face", [-18, -17, -16, -15])
def test_box_rules_at_a_brick_border(hip_lib, rule, face):
    _, N, Nz = GEO["TALL"]
    g = mk()
    order = box_keys()
    order = order[3:] + order[:3]
    scenes = load(g, order)
    before = g.brick_keys()
    boxes = [((-32, -32, -64), (face, 31, 63)), ((face, -32, -64), (31, 31, 63)), ((face, -20, -64), (face + 17, -3, -49))]
    for lo, hi in boxes:
        for sid in (0, 1, 2, -1):
            want = er.select_box(before, rule, lo, hi, sid, N, Nz)
            snap = g.snapshot_bricks(**{rule: (lo, hi)}, sid=sid)
            assert snap["keys"].tolist() == sorted(before[want].tolist()), (rule, lo, hi, sid)
            assert snap["stats"]["selected"] == int(want.sum()) and snap["stats"]["bricks_after"] == len(order)
            # metres and voxels give the same selection: faces on the voxel centres, and a quarter of a voxel outside them
            for pad in (0.0, 0.25):
                m = g.snapshot_bricks(**{rule: ((np.array(lo) - pad) * VS, (np.array(hi) + pad) * VS)}, sid=sid, metres=True, payload=False)
                assert m["stats"]["selected"] == int(want.sum()), (rule, lo, hi, sid, pad)
    assert g.brick_keys().tolist() == before.tolist()                   # snapshots release nothing
    # a brick the box cuts through stays under both rules: the third box cuts brick (1, 0, 0) at every face: it ends inside the brick's y range
    lo, hi = boxes[2]
    want = er.select_box(before, rule, lo, hi, -1, N, Nz)
    cut = er.make_key(0, 1, 0, 0, N, Nz)
    assert not want[before.tolist().index(int(cut))]
    ev = g.evict(**{rule: (lo, hi)}, sid=-1)
    want_owner, _, want_keys = er.plan(before, want)
    assert ev["keys"].tolist() == want_keys.tolist() and g.brick_keys().tolist() == want_owner.tolist()
    check_export(g, scenes, want_owner.tolist(), (0, 1, 2), f"{rule} {face}")
    # sid=None is the active submap
    g.active_submap_id[None] = 1
    rest = g.brick_keys()
    ev = g.evict(clear_box=((-32, -32, -64), (31, 31, 63)))
    assert ev["keys"].tolist() == sorted(k for k in rest.tolist() if k // 128 == 1)
    assert sorted(g.brick_keys().tolist()) == sorted(k for k in rest.tolist() if k // 128 != 1)


def test_box_rules_on_a_global_map_and_on_slab(hip_lib):
    _, N, Nz = GEO["SLAB"]
    g = mk("SLAB", is_global_map=True)
    keys = [int(er.make_key(0, *b, N, Nz)) for b in [(4, 4, 1), (0, 0, 0), (8, 8, 2), (4, 5, 1), (3, 4, 0)]]
    scenes = load(g, keys, "SLAB")
    before = g.brick_keys()
    assert before.tolist() == keys
    lo, hi = (-8, -8, -8), (7, 23, 7)          # bricks (4, 4, 1) and (4, 5, 1) whole: the faces of SLAB's bricks lie at 8 mod 16
    want = er.select_box(before, "clear_box", lo, hi, 0, N, Nz)
    assert want.tolist() == [True, False, False, True, False]
    for sid in (None, 0, -1):
        assert g.snapshot_bricks(clear_box=(lo, hi), sid=sid)["keys"].tolist() == sorted(before[want].tolist())
    assert g.snapshot_bricks(clear_box=(lo, (7, 22, 7)))["keys"].tolist() == [keys[0]]
    ev = g.evict(keep_box=(lo, hi))
    want_owner, _, want_keys = er.plan(before, ~want)
    assert ev["keys"].tolist() == want_keys.tolist() and g.brick_keys().tolist() == want_owner.tolist()
    check_export(g, scenes, want_owner.tolist(), (0,), "global SLAB")
    assert_planes_equal(ev, expected_planes(scenes, want_keys.tolist(), "SLAB"), "global SLAB")


def test_recycled_slots_are_clean(hip_lib):
    g = mk(max_bricks=8)
    keys = [3, 40, 17, 90, 64, 5, 111, 28]
    scenes = load(g, keys, nvox=700)
    assert g.bricks_in_use() == 8
    with pytest.raises(_lib.TslError, match="capacity"):               # today's behaviour: the pool is full
        load(g, [99])
    assert g.bricks_in_use() == 8
    ev = g.evict(keys=[40, 64, 3])
    assert ev["stats"]["bricks_after"] == 5
    assert_planes_equal(ev, expected_planes(scenes, [40, 64, 3]), "evicted")
    new = load(g, [99, 100, 7], nvox=1, seed=1)
    g.sync()
    assert g.bricks_in_use() == 8
    kept = [k for k in keys if k not in (40, 64, 3)]
    scenes.update(new)
    check_export(g, scenes, kept + [99, 100, 7], (0,), "recycled")
    assert_planes_equal(g.snapshot_bricks(keys=[99, 100, 7]), expected_planes(new, [99, 100, 7]), "the recycled slots")
    assert_planes_equal(g.snapshot_bricks(), expected_planes(scenes, kept + [99, 100, 7]), "the whole pool")


@pytest.mark.parametrize("textured", [False, True])
def test_round_trip(hip_lib, textured):
    g = mk(texture_enabled=textured)
    scenes = load(g, KEYS12, nvox=40)
    before = g.snapshot_bricks()
    assert_planes_equal(before, expected_planes(scenes, KEYS12, textured=textured), "snapshot")
    active = []
    for s in (0, 1, 2):
        g.active_submap_id[None] = s
        active.append(g.count_active())
    assert active == [40 * sum(1 for k in KEYS12 if k // 128 == s) for s in (0, 1, 2)]
    ev = g.evict(keys=[130, 5, 255, 101, 2])
    assert g.bricks_in_use() == 7 and ("col" in ev) == textured
    st = g.restore_bricks(ev)
    assert (st["restored"], st["skipped"], st["bricks_before"], st["bricks_after"]) == (5, 0, 7, 12)
    assert_planes_equal(g.snapshot_bricks(), before, "after evict + restore")
    for s in (0, 1, 2):
        g.active_submap_id[None] = s
        assert g.count_active() == active[s]
    check_export(g, scenes, KEYS12, (0, 1, 2), "round trip")
    # the payload survives the wire format as it is
    from taichislam_amd.mapping import wire
    buf, _ = wire.pack(ev)
    assert_planes_equal(wire.unpack(buf), ev, "wire")
    # ... and goes into one slot of another handle of the same geometry: the bricks of slots 0 and 1 that do not share a brick id
    h = mk(texture_enabled=textured)
    one = g.snapshot_bricks(keys=[5, 130 + 128, 101])
    assert one["stats"]["missing"] == 1
    st = h.restore_bricks(one, sid=2)
    assert st["restored"] == 2 and sorted(h.brick_keys().tolist()) == [256 + 5, 256 + 101]


def test_conflicts(hip_lib):
    g = mk()
    keys = [12, 70, 33, 8, 51, 27]
    scenes = load(g, keys)
    ev = g.evict(keys=[33, 8])
    again = load(g, [33], nvox=1, seed=2)                                # brick 33 exists again
    st = g.restore_bricks(ev)
    assert (st["restored"], st["skipped"], st["bricks_after"]) == (1, 1, 6)
    assert_planes_equal(g.snapshot_bricks(keys=[33]), expected_planes(again, [33]), "skip keeps the newer brick")
    assert_planes_equal(g.snapshot_bricks(keys=[8]), expected_planes(scenes, [8]), "the other row went in")
    st = g.restore_bricks(ev, on_conflict="overwrite")
    assert (st["restored"], st["skipped"], st["bricks_after"]) == (2, 0, 6)
    assert_planes_equal(g.snapshot_bricks(), expected_planes(scenes, keys), "overwrite puts the payload back")
    check_export(g, scenes, keys, (0,), "overwrite")


def test_capacity(hip_lib):
    g = mk(max_bricks=8)
    scenes = load(g, [12, 70, 33, 8, 51, 27])
    ev = g.evict(keys=[12, 33, 27])
    scenes.update(load(g, [100, 101, 102, 103], seed=3))
    before = g.snapshot_bricks()
    order = g.brick_keys()
    assert g.bricks_in_use() == 7
    with pytest.raises(_lib.TslError, match="do not fit"):             # 7 + 3 > 8: all or nothing
        g.restore_bricks(ev)
    assert g.brick_keys().tolist() == order.tolist()
    assert_planes_equal(g.snapshot_bricks(), before, "a refused restore changes nothing")
    g.sync()
    # an eviction whose payload buffers are too small changes nothing and reports the count
    cfg = _lib.EvictCfg()
    cfg.rule, cfg.sid, cfg.release = _lib.EVICT_KEYS, -1, 1
    kin = np.array([70, 8, 100], np.int32)
    bufs = [np.zeros(2, np.int32), np.zeros((2, 4096), np.uint32), np.zeros((2, 4096), np.int8), np.zeros((2, 4096), np.int8)]
    st = _lib.EvictStats()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = hip_lib.tsl_tsdf_evict(g.h, C.byref(cfg), vp(kin), 3, *[vp(b) for b in bufs], None, 2, C.byref(st))
    assert rc == -3 and st.selected == 3
    assert g.brick_keys().tolist() == order.tolist()
    assert_planes_equal(g.snapshot_bricks(), before, "a refused eviction changes nothing")
    # all planes null: release = 0 only counts, release = 1 discards without a copy
    cfg.release = 0
    assert hip_lib.tsl_tsdf_evict(g.h, C.byref(cfg), vp(kin), 3, None, None, None, None, None, 0, C.byref(st)) == 0 and st.selected == 3 and st.bricks_after == 7
    cfg.release = 1
    assert hip_lib.tsl_tsdf_evict(g.h, C.byref(cfg), vp(kin), 3, None, None, None, None, None, 0, C.byref(st)) == 0 and st.selected == 3 and st.bricks_after == 4
    check_export(g, scenes, [k for k in order.tolist() if k not in (70, 8, 100)], (0,), "discarded")
    assert g.evict(clear_box=((-32, -32, -64), (31, 31, 63)), payload=False)["stats"]["bricks_after"] == 0 and g.bricks_in_use() == 0


def test_load_order_independence(hip_lib):
    a, b = mk(), mk()
    keys = [77, 5, 41, 9, 64, 18, 2, 101, 55]
    load(a, keys)
    load(b, keys[::-1][3:] + keys[::-1][:3])
    assert a.brick_keys().tolist() != b.brick_keys().tolist()
    box = ((-32, -32, -64), (-1, 31, 15))
    ea, eb = a.evict(keep_box=box), b.evict(keep_box=box)
    assert ea["stats"]["selected"] == eb["stats"]["selected"] > 0 and ea["stats"]["bricks_after"] > 0
    assert_planes_equal(ea, eb, "payloads of two load orders")
    assert_planes_equal(a.snapshot_bricks(), b.snapshot_bricks(), "remainders of two load orders")


def _split(o_export, evicted_keys, geo="TALL"):
    _, N, Nz = GEO[geo]
    k = er.key_of_voxel(o_export["indices"], 0, N, Nz)
    out = np.isin(k, evicted_keys)
    pick = lambda m: {f: np.asarray(o_export[f])[m] for f in ("indices", "TSDF", "W_TSDF", "occupy")}
    return pick(out), pick(~out)


@pytest.mark.parametrize("semantics", [0, 1])
def test_behind_queued_frames_and_going_on(hip_lib, semantics):
    from oracle import BATCHED, FAITHFUL
    _, N, Nz = GEO["TALL"]
    K, frames = tall_stream(6)
    mode = FAITHFUL if semantics else BATCHED
    g, o = make_pair(TALL, K, max_bricks=128)
    g.set_option("semantics", semantics)
    for R, T, d in frames[:3]:
        g.recast_depth_to_map(R, T, d, None)                            # queued: no sync() before the eviction
        o.integrate_depth(R, T, d, mode=mode)
    box = ((-32, -32, 16), (31, 31, 63))                                 # the layers below 16 go: the bricks around the sensor, the first the pool handed out
    ev = g.evict(keep_box=box)
    rest = g.snapshot_bricks()
    assert ev["stats"]["selected"] > 0 and rest["keys"].shape[0] > 0
    assert ev["stats"]["selected"] + rest["keys"].shape[0] == ev["stats"]["bricks_before"]
    _, lo, hi = er.brick_range(ev["keys"], N, Nz)
    assert (hi[:, 2] < 16).all()
    want_out, want_in = _split(o.export_sparse(), ev["keys"])
    assert_export_equal(payload_to_export(ev), want_out, "the payload is the oracle's map of the evicted bricks")
    assert_export_equal(g.export_submap(), want_in, "the remainder is the oracle's map of the other bricks")
    assert_export_equal(payload_to_export(rest), want_in, "and so is its snapshot")
    # both go on: the evicted map, and a fresh handle that received the remainder
    h, _ = make_pair(TALL, K, max_bricks=128)
    h.set_option("semantics", semantics)
    assert h.restore_bricks(rest)["restored"] == rest["keys"].shape[0]
    for R, T, d in frames[3:]:
        g.recast_depth_to_map(R, T, d, None)
        h.recast_depth_to_map(R, T, d, None)
    assert_planes_equal(g.snapshot_bricks(), h.snapshot_bricks(), "three more frames on both")
    g.sync(); h.sync()


def _downstream(g):
    from taichislam_amd.mapping import MarchingCubeMesher
    out = {}
    g.update_esdf(max_dist=1.0)
    i, j, k = np.meshgrid(np.arange(-30, 30, 3), np.arange(-30, 30, 3), np.arange(14, 62, 3), indexing="ij")
    xyz = (np.stack([i, j, k], -1).reshape(-1, 3) * VS + 0.01).astype(np.float32)
    for interp in (False, True):
        d, gr, st = g.query_esdf(xyz, interpolate=interp)
        out[f"esdf{int(interp)}"] = d.tobytes() + (gr.tobytes() if gr is not None else b"") + st.tobytes()
        assert (st == 0).any()
    m = MarchingCubeMesher(g, max_triangles=400000)
    m.generate_indexed_mesh()
    mesh = m.get_indexed_mesh()
    assert mesh["num_triangles"] > 0
    for f in ("vertices", "normals", "edges", "triangles"):
        out["mesh_" + f] = mesh[f].tobytes()
    fr = g.extract_frontiers()
    assert fr["indices"].shape[0] > 0
    for f in ("indices", "mask", "cluster", "clusters"):
        out["frontier_" + f] = fr[f].tobytes()
    nav = g.nav_grid(bands=[(0, 20), (21, 60)], radius=0.4)
    assert (nav["cls"] != 2).any()
    out["nav_cls"], out["nav_d2"] = nav["cls"].tobytes(), nav["d2"].tobytes()
    return out


@pytest.mark.parametrize("esdf_mode", [0, 1])
def test_nothing_stale_downstream(hip_lib, esdf_mode):
    K, frames = tall_stream(3)
    g, _ = make_pair(TALL, K, max_bricks=128)
    g.set_option("esdf_mode", esdf_mode)
    for R, T, d in frames:
        g.recast_depth_to_map(R, T, d, None)
    g.update_esdf(max_dist=1.0)
    xyz = np.array([[0.0, 0.0, 1.0]], np.float32)
    g.query_esdf(xyz, refresh=False)
    # an empty selection leaves the ESDF valid
    assert g.evict(keys=[])["stats"]["selected"] == 0
    assert g.evict(clear_box=((200, 200, 200), (300, 300, 300)), sid=-1)["stats"]["selected"] == 0
    g.query_esdf(xyz, refresh=False)
    ev = g.evict(keep_box=((-32, -32, 16), (31, 31, 63)))
    assert ev["stats"]["selected"] > 0 and ev["stats"]["moved"] > 0 and ev["stats"]["bricks_after"] > 0
    with pytest.raises(_lib.TslError, match="no ESDF update since"):
        g.query_esdf(xyz, refresh=False)
    h, _ = make_pair(TALL, K, max_bricks=128)
    h.set_option("esdf_mode", esdf_mode)
    h.restore_bricks(g.snapshot_bricks())
    with pytest.raises(_lib.TslError, match="no ESDF update since"):
        h.query_esdf(xyz, refresh=False)
    a, b = _downstream(g), _downstream(h)
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert a[k] == b[k], f"{k} differs between the evicted map and a fresh map of the remainder (esdf_mode {esdf_mode})"


def test_keys_rule(hip_lib):
    g = mk()
    scenes = load(g, KEYS12)
    before = g.brick_keys()
    snap = g.snapshot_bricks()
    with pytest.raises(_lib.TslError, match="outside"):
        g.evict(keys=[5, 3 * 128 * 1024])                               # max_submap_num = 1024 slots of 128 bricks
    with pytest.raises(_lib.TslError, match="outside"):
        g.evict(keys=[5, -1])
    assert g.brick_keys().tolist() == before.tolist()
    assert_planes_equal(g.snapshot_bricks(), snap, "a refused key list changes nothing")
    ask = [300, 5, 5, 300, 6, 6, 1000, 41, 5]
    sel, missing = er.select_keys(before, ask)
    assert missing == 2 and sel.sum() == 3
    ev = g.evict(keys=ask)
    assert (ev["stats"]["selected"], ev["stats"]["missing"]) == (3, 2)
    want_owner, _, want_keys = er.plan(before, sel)
    assert ev["keys"].tolist() == want_keys.tolist() == [5, 41, 300] and g.brick_keys().tolist() == want_owner.tolist()
    assert_planes_equal(ev, expected_planes(scenes, [5, 41, 300]), "keys rule")
    ev = g.evict(keys=np.array([5, 41], np.int64))                      # gone already
    assert (ev["stats"]["selected"], ev["stats"]["missing"], ev["keys"].shape) == (0, 2, (0,))


@pytest.mark.parametrize("textured", [False, True])
def test_device_form(hip_lib, textured):
    import torch
    a, b = mk(texture_enabled=textured), mk(texture_enabled=textured)
    scenes = load(a, KEYS12, nvox=20)
    load(b, KEYS12, nvox=20)
    box = ((-32, -32, -64), (31, 31, -1))
    host = a.evict(keep_box=box, sid=-1)
    dev = b.evict(keep_box=box, sid=-1, device=True)
    assert dev["tw"].is_cuda and dev["stats"] == host["stats"] and host["stats"]["selected"] > 0
    assert_planes_equal(to_host(dev), host, "device payload")
    assert a.brick_keys().tolist() == b.brick_keys(device=True).cpu().tolist()
    c = mk(texture_enabled=textured)
    st = c.restore_bricks(dev)
    assert st["restored"] == host["stats"]["selected"]
    assert_planes_equal(c.snapshot_bricks(), host, "restored from tensors")
    assert_planes_equal(to_host(c.snapshot_bricks(device=True)), host, "device snapshot")
    dk = b.snapshot_bricks(keys=torch.tensor(a.brick_keys()[:2].tolist(), device="cuda:0"), device=True)
    assert_planes_equal(to_host(dk), a.snapshot_bricks(keys=a.brick_keys()[:2]), "device key list")


def test_refusals(hip_lib):
    g = mk()
    load(g, [5, 9])
    box = ((-32, -32, -64), (31, 31, 63))
    with pytest.raises(ValueError, match="exactly one"):
        g.evict(keep_box=box, keys=[5])
    with pytest.raises(ValueError, match="exactly one"):
        g.evict()
    with pytest.raises(ValueError, match="lo > hi"):
        g.evict(clear_box=((0, 0, 1), (5, 5, 0)))
    cfg, st = _lib.EvictCfg(), _lib.EvictStats()
    cfg.rule, cfg.sid, cfg.release = _lib.EVICT_CLEAR_BOX, -1, 1
    cfg.lo[2], cfg.hi[2] = 1, 0
    assert hip_lib.tsl_tsdf_evict(g.h, C.byref(cfg), None, 0, None, None, None, None, None, 0, C.byref(st)) == -1
    cfg.rule, cfg.hi[2] = 3, 1
    assert hip_lib.tsl_tsdf_evict(g.h, C.byref(cfg), None, 0, None, None, None, None, None, 0, C.byref(st)) == -1
    with pytest.raises(ValueError, match="on_conflict"):
        g.restore_bricks(g.snapshot_bricks(), on_conflict="merge")
    other = mk("SLAB")
    with pytest.raises(ValueError, match="the payload's N"):
        other.restore_bricks(g.snapshot_bricks())
    tex = mk(texture_enabled=True)
    with pytest.raises(ValueError, match="texture_enabled"):
        tex.restore_bricks(g.snapshot_bricks())
    bad = g.snapshot_bricks()
    bad["keys"] = bad["keys"][::-1].copy()
    with pytest.raises(_lib.TslError, match="ascend"):
        g.restore_bricks(bad, on_conflict="overwrite")
    assert g.bricks_in_use() == 2
    # between merge_begin and merge_finish the global map refuses
    sub = mk()
    load(sub, [5, 9, 40])
    sub.active_submap_id[None] = 1
    G = mk(is_global_map=True)
    mask = G.merge_begin(sub)
    with pytest.raises(_lib.TslError, match="merge has begun"):
        G.evict(clear_box=box, payload=False)
    acc, cnt = G.merge_pack(mask)
    with pytest.raises(_lib.TslError, match="merge has begun"):
        G.snapshot_bricks()
    with pytest.raises(_lib.TslError, match="merge has begun"):
        G.restore_bricks(g.snapshot_bricks())
    G.merge_finish(acc, cnt)
    n = G.bricks_in_use()
    assert n > 0 and G.evict(clear_box=box)["stats"]["selected"] == n and G.bricks_in_use() == 0
