"""The free boxes and corridors without a GPU: the two restatements of tests/nav_corridor_ref.py (slab slicing and a summed-volume table) against each other
on every scene of tests/nav_corridor_scenes.py, the properties the definition promises of every box, the hand-worked scenes, the chain's invariants with
the overlap computed independently, corridor_metres on a made-up flight volume, and the four symbols in the header and the ctypes shim."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nav_corridor_ref as ref
import nav_corridor_scenes as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX_SCENES = sc.box_scenes()
CORRIDOR_SCENES = sc.corridor_scenes()


@pytest.mark.parametrize("scene", BOX_SCENES, ids=[s[0] for s in BOX_SCENES])
def test_the_two_restatements_agree_and_every_box_keeps_its_promises(scene):
    name, cost, cells, free_below, ext = scene
    a, fa = ref.boxes(cost, cells, free_below, ext)
    b, fb = ref.boxes(cost, cells, free_below, ext, how="table")
    assert a.tobytes() == b.tobytes() and fa.tobytes() == fb.tobytes(), name
    free = cost < free_below
    for c, box, f in zip(cells, a, fa):
        ref.check_box(free, c, ext, box, f)
    assert (fa == 0).any(), name                                    # a scene without a single real box tests nothing


def _slab_items(scene):
    """per kind of face the tries of a scene as the kernel divides them among lanes: {"j": [(items, moved)], "i": [(items, words, moved)], "k": [..]}"""
    _, cost, cells, free_below, ext = scene
    out = {"j": [], "i": [], "k": []}
    for c in cells:
        for axis, _, rows, words, moved in ref.tries(cost < free_below, c, ext):
            if axis == 2:
                out["j"].append((rows, moved))
            else:
                out["ik"[axis == 0]].append((rows * words, words, moved))
    return out


def test_scene_shapes_cover_the_kernel_paths():
    """what the scenes claim to reach, counted from the slabs the definition reads (ref.tries), not from the finished boxes"""
    by = {s[0]: s for s in BOX_SCENES}
    assert sorted(by[f"width {W}"][1].shape[2] for W in sc.WIDTHS) == [1, 63, 64, 65, 70]
    b65, f65 = ref.boxes(*by["width 65"][1:])
    assert ((b65[:, 2] <= 63) & (b65[:, 5] >= 64) & (f65 == 0)).any()      # a box across bit 63 / 64, and so rows of two words
    assert max(w for _, w, _ in _slab_items(by["width 65"])["i"]) == 2
    # +-j slabs of more than a wave: the planes (80 and 79 cells) and the cube (81: j closes on ext while k and i span 9)
    assert max(n for n, _ in _slab_items(by["wide plane 1 x 80 x 150, ext 127"])["j"]) == 80
    assert max(n for n, _ in _slab_items(by["tall plane 1 x 150 x 80, ext 127"])["j"]) == 79
    assert max(n for n, _ in _slab_items(by["cube 12 x 12 x 12, ext 5"])["j"]) == 81
    # +-i and +-k slabs of more than a wave of (row, word) items, moving and failing, and runs of 3, 4 and 5 words over many rows
    deep = _slab_items(by["deep slabs 70 x 70 x 70, ext 34"])
    assert max(n for n, _, _ in deep["i"]) == 134 and max(n for n, _, _ in deep["k"]) == 138
    assert sum(n > 64 and m for n, _, m in deep["i"]) > 20 and sum(n > 64 and m for n, _, m in deep["k"]) > 20 and any(n > 64 and not m for n, _, m in deep["k"])
    broad = _slab_items(by["broad slabs 200 x 20 x 260, ext 127"])
    assert max(n for n, _, _ in broad["k"]) == 100 and {w for n, w, _ in broad["k"] if n > 64} == {4, 5} and any(n > 64 and not m for n, _, m in broad["k"])
    assert {w for _, w, _ in broad["k"]} == {1, 2, 3, 4, 5}          # every run length the 255 columns of ext 127 can give
    be, fe = ref.boxes(*by["empty 5 x 7 x 9, ext 20"][1:])
    assert (be[fe == 0] == [0, 0, 0, 4, 6, 8]).all()                # the volume itself, clipped
    for axis in range(3):
        bz, fz = ref.boxes(*by[f"ext 0 on axis {axis}"][1:])
        assert (bz[fz == 0][:, axis] == bz[fz == 0][:, axis + 3]).all() and (bz[fz == 0][:, (axis + 1) % 3] != bz[fz == 0][:, (axis + 1) % 3 + 3]).any()


def test_hand_worked_l_shape():
    free = sc.l_shape() < sc.FREE_BELOW
    table = ref.BoxTable(free)
    for c, ext, want, flag in sc.L_SHAPE_CASES:
        assert ref.box_slices(free, c, ext) == (want, flag), (c, ext)
        assert table.box(c, ext) == (want, flag), (c, ext)


def test_free_below_limits():
    (_, cost, cells, _, ext), _ = sc.free_below_cases()
    b1, f1 = ref.boxes(cost, cells, 1, ext)
    for box, f in zip(b1, f1):
        if f == 0:
            assert (cost[box[0]:box[3] + 1, box[1]:box[4] + 1, box[2]:box[5] + 1] == 0).all()
    b255, f255 = ref.boxes(cost, np.array([[1, 4, 10], [1, 4, 11]]), 255, ext)
    assert f255.tolist() == [1, 0] and b255[1, 2] == 11              # 255 is never free, 254 is under free_below 255, and its box stops at the 255


def _check_chain(cost, cells, length, free_below, ext, Q, got, name):
    free = cost < free_below
    for p in range(cells.shape[0]):
        n = min(int(length[p]), cells.shape[1])
        cnt, st = int(got["count"][p]), int(got["status"][p])
        bx, sd, lk = got["boxes"][p], got["seed"][p], got["link"][p]
        assert (bx[cnt:] == -1).all() and (sd[cnt:] == -1).all() and (lk[cnt:] == ref.TAIL_LINK).all(), name
        if n <= 0:
            assert (cnt, st) == (0, 2), name
            continue
        assert 1 <= cnt <= Q and sd[0] == 0 and (np.diff(sd[:cnt]) > 0).all() and sd[cnt - 1] < n, (name, p)      # the seeds strictly increase
        assert st in (0, 1) and (st == 0 or cnt == Q), (name, p)
        covered = np.zeros(n, bool)
        last_t = 0
        for q in range(cnt):
            s = int(sd[q])
            want_box, want_flag = ref.box_slices(free, cells[p, s], ext)
            assert bx[q].tolist() == want_box, (name, p, q)
            t = s
            if want_flag == 0:
                while t + 1 < n and ref.inside(want_box, cells[p, t + 1].astype(int)):
                    t += 1
            covered[s:t + 1] = True
            last_t = t
            if q + 1 < cnt:
                assert int(sd[q + 1]) == (t if t > s else s + 1), (name, p, q)
            # the link, from the sets of cells of the two boxes
            if q == 0:
                assert lk[q] & 3 == 0
            else:
                cells_of = lambda b, f: set() if f == ref.OUTSIDE else {(k, i, j) for k in range(b[0], b[3] + 1) for i in range(b[1], b[4] + 1) for j in range(b[2], b[5] + 1)}
                pf = ref.box_slices(free, cells[p, int(sd[q - 1])], ext)[1]
                shared = cells_of(bx[q - 1].tolist(), pf) & cells_of(bx[q].tolist(), want_flag)
                assert lk[q] & 3 == (1 if shared else 2), (name, p, q)
            assert (lk[q] >> 2) == (1 if want_flag else 0), (name, p, q)
        assert covered[:last_t + 1].all(), (name, p)                 # every path cell up to the last seed's t lies in an emitted box
        assert (st == 0) == (last_t == n - 1), (name, p)


@pytest.mark.parametrize("scene", CORRIDOR_SCENES, ids=[s[0] for s in CORRIDOR_SCENES])
def test_chain_invariants_and_both_restatements(scene):
    name, cost, cells, length, free_below, ext, Q = scene
    a = ref.corridor(cost, cells, length, free_below, ext, Q)
    b = ref.corridor(cost, cells, length, free_below, ext, Q, how="table")
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (name, k)
    _check_chain(cost, cells, length, free_below, ext, Q, a, name)


def test_hand_worked_corridors():
    _, cost, cells, length, fb, ext, Q = sc.touch_only()
    got = ref.corridor(cost, cells, length, fb, ext, Q)
    w = sc.TOUCH_ONLY_WANT
    assert got["boxes"][0, :2].tolist() == w["boxes"] and got["seed"][0, :2].tolist() == w["seed"] and got["link"][0, :2].tolist() == w["link"]
    assert got["count"][0] == w["count"] and got["status"][0] == w["status"]
    # the blocked cell in the middle: its box is the cell, flagged; the boxes on either side stop short of it
    _, cost, cells, length, fb, ext, Q = sc.blocked_middle()
    got = ref.corridor(cost, cells, length, fb, ext, Q)
    n = int(got["count"][0])
    seeds, links = got["seed"][0, :n].tolist(), got["link"][0, :n].tolist()
    assert got["status"][0] == 0 and 6 in seeds and links[seeds.index(6)] == 2 + 4 and got["boxes"][0, seeds.index(6)].tolist() == [0, 2, 6, 0, 2, 6]
    assert all(b[5] < 6 or b[2] > 6 for b, s in zip(got["boxes"][0, :n].tolist(), seeds) if s != 6)
    # cut at max_boxes
    _, cost, cells, length, fb, ext, Q = sc.cut_at_max_boxes()
    cut = ref.corridor(cost, cells, length, fb, ext, Q)
    assert cut["count"][0] == 2 and cut["status"][0] == 1 and cut["boxes"][0].tobytes() == got["boxes"][0, :2].tobytes()
    # lengths 0 and 1, a negative length, a length above L
    _, cost, cells, length, fb, ext, Q = sc.short_paths()
    got = ref.corridor(cost, cells, length, fb, ext, Q)
    assert got["count"][:3].tolist() == [0, 1, 0] and got["status"][:3].tolist() == [2, 0, 2] and got["status"][3] in (0, 1)
    assert got["link"][4, 0] == 4 and got["boxes"][4, 0].tolist() == [-1] * 6 and got["link"][4, 1] & 3 == 2      # a start outside: no cells, nothing shared


# the six runs of nav_corridor_scenes.straight_random, recorded from the restatement when the scene was fixed: (count, status, seeds, links)
STRAIGHT_RUNS = (
    (22, 0, [0, 3, 6, 13, 14, 21, 24, 27, 30, 31, 32, 34, 39, 40, 47, 52, 54, 55, 56, 57, 61, 62], [0, 1, 1, 1, 1, 1, 1, 1, 1, 6, 2, 1, 1, 1, 1, 1, 1, 1, 6, 2, 1, 1]),
    (14, 0, [0, 1, 2, 3, 5, 8, 9, 10, 11, 12, 15, 16, 18, 19], [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]),
    (13, 0, [0, 1, 5, 6, 11, 14, 15, 20, 21, 26, 28, 29, 31], [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]),
    (16, 0, [0, 3, 4, 5, 7, 8, 9, 11, 12, 13, 14, 15, 16, 17, 18, 19], [0, 1, 1, 1, 1, 6, 2, 1, 2, 1, 1, 1, 1, 1, 1, 2]),
    (25, 0, [0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 21, 23, 24, 26, 27, 29, 31], [0, 1, 1, 1, 1, 1, 1, 1, 2, 1, 1, 6, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]),
    (11, 0, [0, 9, 15, 21, 30, 39, 47, 48, 49, 57, 63], [0, 1, 1, 1, 1, 1, 1, 6, 2, 1, 1]))


def test_straight_paths_through_the_random_volume_give_the_recorded_corridors():
    """The volume is fixed by its seed, so the answer is pinned: a change of the rule shows here even where both restatements follow it.  (The issue's
    prototype gave 18 boxes with every link 1 on a random volume of its own; that volume is not this one.)  A run over a wall gives link 6 = shares
    nothing + blocked, and the box after it link 2; the space diagonal (run 3) and the plane diagonal (run 4) also meet boxes that only touch."""
    _, cost, cells, length, fb, ext, Q = sc.straight_random()
    got = ref.corridor(cost, cells, length, fb, ext, Q)
    for p, (count, status, seeds, links) in enumerate(STRAIGHT_RUNS):
        assert (int(got["count"][p]), int(got["status"][p])) == (count, status), p
        assert got["seed"][p, :count].tolist() == seeds and got["link"][p, :count].tolist() == links, p


def test_corridor_metres_on_a_made_up_volume():
    from taichislam_amd.utils import corridor_metres
    vol = {"cost": np.zeros((4, 8, 8), np.uint8), "origin": (6, 0, 0), "stride": 4, "voxel": 0.05, "half": (16, 16, 16)}
    boxes = np.array([[0, 0, 0, 0, 0, 0], [1, 2, 3, 2, 4, 7], [-1] * 6], np.int16)
    got = corridor_metres(boxes, vol)
    assert got.shape == (3, 2, 3) and got.dtype == np.float64
    # cell 0 of the layers covers the voxels 6 - 16 .. 6 - 16 + 3, of the rows and columns -16 .. -13
    assert np.allclose(got[0], [[(-16 - 0.5) * 0.05, (-16 - 0.5) * 0.05, (-10 - 0.5) * 0.05], [(-13 + 0.5) * 0.05, (-13 + 0.5) * 0.05, (-7 + 0.5) * 0.05]], atol=1e-12)
    lo = [(2 * 4 - 16 - 0.5) * 0.05, (3 * 4 - 16 - 0.5) * 0.05, (1 * 4 + 6 - 16 - 0.5) * 0.05]
    hi = [(4 * 4 - 16 + 3 + 0.5) * 0.05, (7 * 4 - 16 + 3 + 0.5) * 0.05, (2 * 4 + 6 - 16 + 3 + 0.5) * 0.05]
    assert np.allclose(got[1], [lo, hi], atol=1e-12) and np.isnan(got[2]).all()
    # the sample of flight_volume in a corner cell lies inside: (n * stride + stride // 2 + origin - half) * voxel
    assert lo[0] < (2 * 4 + 2 - 16) * 0.05 < hi[0] and lo[2] < (1 * 4 + 2 + 6 - 16) * 0.05 < hi[2]
    two = corridor_metres(np.array([[[0, 3, 5, 0, 3, 9]]], np.int16), N=64, voxel=0.1)
    assert two.shape == (1, 1, 2, 3) and np.allclose(two[0, 0, :, :2], [[(3 - 32 - 0.5) * 0.1, (5 - 32 - 0.5) * 0.1], [(3 - 32 + 0.5) * 0.1, (9 - 32 + 0.5) * 0.1]]) and np.isnan(two[..., 2]).all()
    with pytest.raises(ValueError):
        corridor_metres(boxes)
    with pytest.raises(ValueError):
        corridor_metres(boxes[:, :5], vol)


def test_symbols_are_declared_bound_and_refuse_a_null_handle():
    from taichislam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "taichislam_hip.h")).read()
    names = ("tsl_tsdf_nav_boxes", "tsl_tsdf_nav_boxes_dev", "tsl_tsdf_nav_corridor", "tsl_tsdf_nav_corridor_dev")
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in _lib.SIGNATURES, n
    assert "#define TSL_BOX_BLOCKED 1" in hdr and "#define TSL_BOX_OUTSIDE 2" in hdr and (_lib.BOX_BLOCKED, _lib.BOX_OUTSIDE) == (ref.BLOCKED, ref.OUTSIDE)
    assert C.sizeof(_lib.NavCorridorCfg) == 32
    assert [f[0] for f in _lib.NavCorridorCfg._fields_] == ["D", "H", "W", "free_below", "ext_k", "ext_i", "ext_j", "max_boxes"]
    L = _lib.lib()
    cfg = _lib.NavCorridorCfg()
    assert L.tsl_tsdf_nav_boxes(None, C.byref(cfg), None, None, 0, None, None) == -1 and "nav_boxes: null handle" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_nav_boxes_dev(None, C.byref(cfg), None, None, 0, None, None, None) == -1 and "nav_boxes_dev: null handle" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_nav_corridor(None, C.byref(cfg), None, None, None, 0, 1, None, None, None, None, None) == -1
    assert "nav_corridor: null handle" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_nav_corridor_dev(None, C.byref(cfg), None, None, None, 0, 1, None, None, None, None, None, None) == -1
    assert "nav_corridor_dev: null handle" in L.tsl_last_error().decode()
