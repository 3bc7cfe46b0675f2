"""The scenes of tests/gn_limit_scenes.py against the numpy restatements alone: what the restatements give on them equals the expectation each scene
carries (listed voxels, stored bit patterns, a few f32 operations written out), and the scenes meet the conditions that make them worth running on the
GPU (addends beyond 2^31, sums beyond 2^53, inputs exactly on a gate).  tests/test_gn_limits_gpu.py compares the kernels with the same restatements."""
import numpy as np
import pytest

import gn_limit_scenes as gs
import register_ref as rr
import register_search_ref as rsr
import track_points_ref as tpr
import track_ref as tr

F32 = np.float32
VS = gs.VS
NOT_FINITE = ("nan", "pinf", "ninf")


def _defaults(**kw):
    return rr.defaults(VS, gs.SMALL["internal_voxels"], gs.SMALL["voxel_scale"], **kw)


def _counts(sums):
    return dict(zip(("n_used", "n_gate", "n_unknown", "n_far", "n_grad"), (int(v) for v in sums[tr.I_USED:])))


def _score(src, grid, gates, **kw):
    """register_search_ref.score of the one pose (identity, SHIFT) as a list e, n_used, n_unknown, n_far, n_grad"""
    sc = rsr.score(src, gs.EYE[None], gs.SHIFT[None], 1, VS, grid, **gates, **kw)
    return [int(sc[f][0]) for f in rsr.FIELDS]


def test_fix_refuses_what_is_not_finite():
    assert tr.fix(F32(1.5)) == 3 << 19 and tr.fix(np.array([-2.0 ** 20], F32))[0] == -2 ** 40
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(AssertionError):
            tr.fix(np.array([0.0, bad], F32))


@pytest.mark.parametrize("kind", list(gs.SPECIALS))
def test_a_stored_value_that_is_not_finite_reaches_no_product(kind):
    p, base, tainted = gs.a_probes()
    m = gs.a_map(kind)
    grid = gs.grid("SMALL", m)
    assert tainted.sum() == 8 * 27 and (~tainted).sum() == 4 * 27 and not gs.expected_unknown(base, m).any()
    for stride in (1, 2):
        sums, bucket, s = tpr.linearize_points(p, gs.EYE, gs.ZERO, stride, VS, grid, **gs.OPEN)
        tn = tainted[::stride]
        assert sums[tr.I_USED:].sum() == tpr.visited(p.shape[0], stride) and (sums != gs.INT64_MIN).all()
        assert (bucket[~tn] == gs.USED).all() and np.isfinite(s[~tn]).all()
        if kind in NOT_FINITE:                             # 0 * inf is a NaN: every interpolant of a tainted cell is a NaN or an inf, and far
            assert (bucket[tn] == gs.FAR).all() and not np.isfinite(s[tn]).any() and np.isnan(s[tn]).sum() >= 27 // stride
            assert sums[tr.I_USED] == (~tn).sum() and sums[tr.I_FAR] == tn.sum()
        else:
            # 65504 is a value like any other.  Of the 27 probes of a tainted cell 8 give it a weight of 0.37 or more on every axis, at least
            # 0.05 in all: those are far; where its weight is exactly 0 in the value and in the gradient the sample is used
            assert np.isfinite(s).all() and (bucket[tn] != gs.UNKNOWN).all()
            assert stride != 1 or ((bucket[tn] == gs.FAR).sum() >= 64 and (bucket[tn] == gs.USED).sum() >= 1)
    # the image: every pixel in a tainted cell is far, every pixel whose cell is not wholly listed is unknown
    ip, ibase = gs.image_points(gs.a_image(), gs.A_K, gs.A_T)
    it, iu = gs.a_tainted(ibase), gs.expected_unknown(ibase, m)
    assert it.sum() > 100 and iu.sum() > 100 and (~it & ~iu).sum() > 1000      # 8 of the 6.4 x 4.8 x 4.5 cells the image spans are tainted
    sums = tr.linearize(gs.a_image(), gs.EYE, gs.A_T, gs.A_K, 1, VS, grid)
    assert sums[tr.I_USED:].sum() == ip.shape[0] and (sums != gs.INT64_MIN).all() and sums[tr.I_UNKNOWN] == iu.sum() and sums[tr.I_GATE] == 0
    if kind in NOT_FINITE:
        assert sums[tr.I_FAR] == it.sum() and sums[tr.I_USED] == (~it & ~iu).sum()
    # the registration with the value in the destination: the 8 source voxels that land in tainted cells are far
    src = rr.source(gs.a_source())
    sums = rr.linearize(src, gs.EYE, gs.SHIFT, 1, VS, grid, **_defaults())
    assert sums[tr.I_USED:].sum() == 125 and (sums != gs.INT64_MIN).all()
    if kind in NOT_FINITE:
        assert _counts(sums) == dict(n_used=117, n_gate=0, n_unknown=0, n_far=8, n_grad=0)
    assert _score(src, grid, _defaults()) == [int(sums[i]) for i in (tr.I_E, tr.I_USED, tr.I_UNKNOWN, tr.I_FAR, tr.I_GRAD)]
    # ... and in the source, beside a NaN weight: both voxels are gated, whatever the value (an inf and 65504 lie beyond the band, a NaN nowhere)
    clean = gs.grid("SMALL", gs.a_map())
    src = rr.source(gs.a_source(kind))
    sums = rr.linearize(src, gs.EYE, gs.SHIFT, 1, VS, clean, **_defaults())
    assert _counts(sums) == dict(n_used=123, n_gate=2, n_unknown=0, n_far=0, n_grad=0) and (sums != gs.INT64_MIN).all()
    assert rsr.gate(src, 1, **_defaults())["n_gate"] == 2
    assert _score(src, clean, _defaults()) == [int(sums[i]) for i in (tr.I_E, tr.I_USED, tr.I_UNKNOWN, tr.I_FAR, tr.I_GRAD)]


def _magnitudes(sums, addends):
    """the addends as [n, 28]; checks that the int64 sums are the sums of Python integers: nothing wrapped"""
    A = np.stack(addends, 1)
    assert [sum(int(x) for x in A[:, k]) for k in range(28)] == [int(v) for v in sums[:28]]
    return A


def test_b_the_block_fills_the_wide_branch_and_passes_2_53():
    grid = gs.grid("SMALL", gs.b_map())
    p = gs.b_points()
    add = []
    sums, bucket, _ = tpr.linearize_points(p, gs.EYE, gs.ZERO, 1, VS, grid, addends=add, **gs.B_POINT_GATES)
    A = _magnitudes(sums, add)
    assert sums[tr.I_USED] == 32768 and (bucket == gs.USED).all()
    big = np.abs(A) >= 2 ** 31
    assert big[:, :27].any(0).all(), f"slots without an addend of 2^31: {np.nonzero(~big.any(0))[0].tolist()}"
    for k in gs.B_FREE_SIGN:
        assert (A[:, k] >= 2 ** 31).any() and (A[:, k] <= -2 ** 31).any(), f"slot {k} lacks a wide addend of one sign"
    assert (np.abs(sums[:28]) > 2 ** 53).sum() >= 1
    # the premise of the refusal: M = 2 L g_max, every addend is at most M^2 2^20 + 1/2, and the call is admitted
    M2 = (2.0 * 5.12 * gs.B_GATES["g_max"]) ** 2
    assert np.abs(A).max() <= M2 * 2.0 ** 20 + 0.5 and M2 * 2.0 ** 20 * 32768 <= 2.0 ** 62
    # e = s^2 <= r_max^2 stays below 2^31 on this block; the two gentle blocks fill that slot
    assert np.abs(A[:, 27]).max() <= gs.B_GATES["r_max"] ** 2 * 2.0 ** 20
    add = []
    sums, bucket, s = tpr.linearize_points(gs.b_e_points(), gs.EYE, gs.ZERO, 1, VS, gs.grid("SMALL", gs.b_e_map()), addends=add, **gs.B_E_GATES)
    A = _magnitudes(sums, add)
    assert (bucket == gs.USED).all() and (s > 90).sum() == 300 and (s < -90).sum() == 300
    assert (A[:, 27] >= 2 ** 31).all()


def test_b_the_image_fills_the_wide_branch():
    grid = gs.grid("SMALL", gs.b_map())
    add = []
    sums = tr.linearize(gs.b_image(), gs.EYE, gs.B_T, gs.B_K, 1, VS, grid, addends=add, **gs.B_IMAGE_GATES)
    A = _magnitudes(sums, add)
    _, base = gs.image_points(gs.b_image(), gs.B_K, gs.B_T)
    assert base.min() >= gs.B_LO and base.max() < gs.B_HI and sums[tr.I_USED] + sums[tr.I_GRAD] == 160 * 120 and sums[tr.I_USED] > 19000
    assert (np.abs(A) >= 2 ** 31)[:, :27].any(0).all() and (np.abs(sums[:28]) > 2 ** 53).any()
    assert (2.0 * 5.12 * gs.B_GATES["g_max"]) ** 2 * 2.0 ** 20 * 160 * 120 <= 2.0 ** 62


def test_b_the_registration_fills_the_wide_branch():
    grid = gs.grid("SMALL", gs.b_reg_destination())
    src = rr.source(gs.b_reg_source())
    g = gs.B_REG_GATES
    M = max(2.0 * 5.12 * g["g_max"], g["r_max"] + g["band"])
    assert M * M * 2.0 ** 20 * 4096 * 4096 <= 2.0 ** 62      # register_check admits a pool of 4096 bricks
    assert (np.abs(src[1]) > 0.08).mean() > 0.99 and np.abs(src[1]).max() <= g["band"]
    for stride in (1, 2):
        add = []
        sums = rr.linearize(src, gs.EYE, gs.SHIFT, stride, VS, grid, addends=add, **g)
        A = _magnitudes(sums, add)
        assert sums[tr.I_USED:].sum() == rr.visited(src, stride) == 32768 // stride ** 3 and sums[tr.I_GRAD] > 0 and sums[tr.I_USED] > 30000 // stride ** 3
        assert sums[tr.I_GATE] == sums[tr.I_UNKNOWN] == sums[tr.I_FAR] == 0
        big = (np.abs(A) >= 2 ** 31).any(0)
        assert big[[k for k in range(28) if k not in gs.B_REG_SMALL_SLOTS]].all() and (np.abs(sums[:28]) >= 2 ** 32).all()
        assert np.abs(A).max() <= M * M * 2.0 ** 20 + 0.5


def test_c_the_gates_at_equality():
    grid = gs.grid("SMALL", gs.c_map())
    v, g0 = gs.c_facts()
    lin = lambda p, **kw: tpr.linearize_points(p, gs.EYE, gs.ZERO, 1, VS, grid, **dict(gs.OPEN, **kw))
    # r_max: |s| == r_max is not far
    sums, bucket, s = lin(gs.c_corner_point(), r_max=v)
    assert bucket[0] == gs.USED and s[0] == v
    assert lin(gs.c_corner_point(), r_max=np.nextafter(v, F32(0)))[1][0] == gs.FAR
    # g_max: gg == g_max^2 is used; a flat cell is grad
    assert lin(gs.c_interior_point(), g_max=g0)[1][0] == gs.USED
    assert np.nextafter(g0, F32(0)) * np.nextafter(g0, F32(0)) < g0 * g0
    assert lin(gs.c_interior_point(), g_max=np.nextafter(g0, F32(0)))[1][0] == gs.GRAD
    sums, bucket, s = lin(gs.c_flat_point())
    assert bucket[0] == gs.GRAD and s[0] == F32(np.float16(0.05))
    # the range gate: l2 == dmax2 and l2 == dmin2 pass
    assert lin(gs.c_range_points(0.7, 3.3), d_min=0.7, d_max=3.3)[1].tolist() == [gs.UNKNOWN, gs.GATE, gs.UNKNOWN, gs.GATE]
    # the depth gate: (float)d == thr_max and == thr_min pass
    sums = tr.linearize(gs.C_DEPTH, gs.EYE, gs.ZERO, gs.A_K, 1, VS, grid, d_min=0.5, d_max=2.5)
    assert _counts(sums) == dict(n_used=0, n_gate=2, n_unknown=2, n_far=0, n_grad=0)
    # the registration: w == w_min and |t| == band pass, one f16 step beyond either is gated
    m, ok = gs.c_reg_source()
    sums = rr.linearize(rr.source(m), gs.EYE, gs.SHIFT, 1, VS, grid, **_defaults(w_min=gs.C_W_MIN, band=gs.C_BAND))
    assert sums[tr.I_GATE] == (~ok).sum() == 4 and sums[tr.I_USED] == 4
    assert rsr.gate(rr.source(m), 1, **_defaults(w_min=gs.C_W_MIN, band=gs.C_BAND))["n_gate"] == 4
    # huber: |r| == huber has the weight 1, one f32 step above it the weight huber / |r|: e = (wgt r) r and b_a = (wgt g_a) r, written out
    m, p, v, g = gs.c_huber_case()
    e = {}
    for huber, wgt in ((v, F32(1.0)), (np.nextafter(v, F32(0)), np.nextafter(v, F32(0)) / v)):
        sums = tpr.linearize_points(p, gs.EYE, gs.ZERO, 1, VS, gs.grid("SMALL", m), huber=huber, **gs.B_E_GATES)[0]
        assert sums[tr.I_USED] == 1 and sums[tr.I_E] == gs.fixed((wgt * v) * v) and [int(x) for x in sums[21:24]] == [gs.fixed((wgt * ga) * v) for ga in g]
        e[float(wgt)] = int(sums[tr.I_E])
    assert len(e) == 2 and e[1.0] - min(e.values()) > 500          # a weight one f32 below 1 takes v^2 2^-24 = 2^-11 off e = v^2, 2^9 in fixed point


def _points_against_the_sets(geo, m, p, base, what):
    """the restatement's buckets of a map with a used ramp: unknown exactly where the listed voxels say so, used elsewhere"""
    sums, bucket, s = tpr.linearize_points(p, gs.EYE, gs.ZERO, 1, VS, gs.grid(geo, m), **gs.OPEN)
    unknown = gs.expected_unknown(base, m)
    assert np.array_equal(bucket == gs.UNKNOWN, unknown) and (bucket[~unknown] == gs.USED).all(), what
    return unknown


def _register_against_the_sets(geo, m, source, what):
    sums = rr.linearize(rr.source(source), gs.EYE, gs.SHIFT, 1, VS, gs.grid(geo, m), **_defaults())
    unknown = gs.expected_unknown(source["indices"], m)
    assert _counts(sums) == dict(n_used=int((~unknown).sum()), n_gate=0, n_unknown=int(unknown.sum()), n_far=0, n_grad=0), what
    return unknown


@pytest.mark.parametrize("geo", gs.SEAM_GEOS)
def test_d_cells_over_brick_seams(geo):
    n_variants = 0
    for kind in gs.SEAM_KINDS:
        p, base = gs.seam_probes(geo, kind)
        variants = gs.seam_variants(geo, kind)
        assert len(variants) == 1 + 8 + (2 ** len(kind) if kind else 0)
        for name, m in variants:
            unknown = _points_against_the_sets(geo, m, p, base, f"{geo}, seam {kind}, {name}")
            ru = _register_against_the_sets(geo, m, gs.seam_source(geo, kind), f"{geo}, seam {kind}, {name}")
            if name == "complete":
                assert not unknown.any() and not ru.any()
            else:
                assert unknown.any() and ru.any() and (name.startswith("brick") and len(kind) == 1 or not unknown.all())
            n_variants += 1
    assert n_variants == 98


@pytest.mark.parametrize("geo", list(gs.GEOS))
def test_d_cells_at_the_walls(geo):
    _, _, lo, hi = gs.dims(geo)
    for name, m, p, base in gs.wall_cases(geo):
        unknown = _points_against_the_sets(geo, m, p, base, name)
        a = int(name.split()[2])
        # across the wall: the cells with base lo - 1 and hi - 1 (and beyond) are unknown, lo and hi - 2 are not
        across = base[:, a]
        assert unknown[(across < lo[a]) | (across >= hi[a] - 1)].all() and {int(x) for x in across[~unknown]} <= {int(lo[a]), int(lo[a]) + 1, int(hi[a]) - 2}
        assert (~unknown).sum() >= 8 and unknown.sum() >= 8, name
        ru = _register_against_the_sets(geo, m, gs.wall_source(m), name)
        assert ru.sum() == 27 - 8
    m, p, base = gs.origin_case()
    unknown = _points_against_the_sets(geo, m, p, base, "the origin")
    assert not unknown.any() and (base.min(), base.max()) == (-1, 0)
