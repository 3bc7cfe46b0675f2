"""The Gauss-Newton kernels (tsl_align.hip, tsl_align_points.hip, tsl_register.hip, tsl_register_search.hip) on the hand-built maps of
tests/gn_limit_scenes.py: stored values that are not finite, addends beyond 2^31 and sums beyond 2^53, inputs exactly on every gate, cells over brick
seams and at the walls.  Every integer and every bit pattern is compared with the numpy restatements, and the buckets with the expectation the scene
carries; tests/test_gn_limits_cpu.py checks the restatements and the scenes' conditions without a GPU."""
import numpy as np
import pytest

import gn_limit_scenes as gs
import register_ref as rr
import register_search_ref as rsr
import track_points_ref as tpr
import track_ref as tr

pytestmark = pytest.mark.gpu

F32 = np.float32
VS = gs.VS
NOT_FINITE = ("nan", "pinf", "ninf")
COUNTS = ("n_used", "n_gate", "n_unknown", "n_far", "n_grad")
_MAPS = {}


def _map(geo, role="dst"):
    """one GPU map per geometry and role for the whole module, reset before every use"""
    from taichislam_amd.mapping import DenseTSDF
    if (geo, role) not in _MAPS:
        _MAPS[geo, role] = DenseTSDF(**gs.GEOS[geo])
        N, Nz, _, _ = gs.dims(geo)
        assert (_MAPS[geo, role].N, _MAPS[geo, role].Nz) == (N, Nz)
    g = _MAPS[geo, role]
    g.reset()
    g.active_submap_id[None] = 0
    return g


def _loaded(geo, m, role="dst", first=None):
    """the map of (geo, role) holding m; first: a map loaded before it, whose bricks take the first places of the pool"""
    g = _map(geo, role)
    for e in (first, m):
        if e is not None and len(e["TSDF"]):
            g.load_numpy(0, e["indices"], e["TSDF"], e["W_TSDF"], e["occupy"], None)
    return g


def _bits32(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def _defaults(**kw):
    return rr.defaults(VS, gs.SMALL["internal_voxels"], gs.SMALL["voxel_scale"], **kw)


def _points(g, grid, p, what, stride=1, huber=0.0, **gates):
    """align_points_linearize with its per-point outputs against the restatement: the 33 integers, the buckets, s as bits (a NaN as a NaN: which
    one is not specified); counts only gives the same buckets and no sums.  Returns the restatement's (sums, bucket, s)."""
    want = tpr.linearize_points(p, gs.EYE, gs.ZERO, stride, VS, grid, huber=huber, **gates)
    sums, bucket, s = want
    for counts_only in (False, True):
        got = g.align_points_linearize(p, gs.EYE, gs.ZERO, stride=stride, huber=huber, per_point=True, counts_only=counts_only, **gates)
        ref = np.where(np.arange(tr.N_SUMS) < tr.I_USED, 0, sums) if counts_only else sums
        bad = np.nonzero(got["sums"] != ref)[0]
        assert bad.size == 0, f"{what}, counts only {counts_only}: sums {bad.tolist()} differ: {got['sums'][bad]} / {ref[bad]}"
        assert got["sums"][tr.I_USED:].sum() == tpr.visited(p.shape[0], stride) == got["bucket"].size
        bad = np.nonzero(got["bucket"] != bucket)[0]
        assert bad.size == 0, f"{what}: bucket differs at {bad[:8].tolist()}: {got['bucket'][bad[:8]]} / {bucket[bad[:8]]}"
        nan = np.isnan(s)
        assert np.array_equal(np.isnan(got["s"]), nan), f"{what}: NaN in s at {np.nonzero(np.isnan(got['s']) != nan)[0][:8].tolist()}"
        bad = np.nonzero((_bits32(got["s"]) != _bits32(s)) & ~nan)[0]
        assert bad.size == 0, f"{what}: s differs at {bad[:8].tolist()}: {got['s'][bad[:8]]} / {s[bad[:8]]}"
    plain = g.align_points_linearize(p, gs.EYE, gs.ZERO, stride=stride, huber=huber, **gates)      # the kernel without the per-point stores
    assert np.array_equal(plain["sums"], sums), f"{what}: without the per-point outputs"
    return want


def _register(dst, src, source, grid, what, stride=1, huber=0.0, **gates):
    """register_linearize (with and without counts_only) and register_score (likewise) of the pose (identity, SHIFT) against the restatements; the
    score's integers equal what the linearisation counts.  Returns the restatement's 33 integers."""
    full = _defaults(huber=huber, **gates)
    sv = rr.source(source)
    want = rr.linearize(sv, gs.EYE, gs.SHIFT, stride, VS, grid, **full)
    got = dst.register_linearize(src, gs.EYE, gs.SHIFT, stride=stride, huber=huber, **gates)
    bad = np.nonzero(got["sums"] != want)[0]
    assert bad.size == 0, f"{what}: sums {bad.tolist()} differ: {got['sums'][bad]} / {want[bad]}"
    assert want[tr.I_USED:].sum() == rr.visited(sv, stride)
    co = dst.register_linearize(src, gs.EYE, gs.SHIFT, stride=stride, huber=huber, counts_only=True, **gates)
    assert np.array_equal(co["sums"][tr.I_USED:], want[tr.I_USED:]) and not co["sums"][:tr.I_USED].any(), f"{what}: counts only"
    ref = rsr.score(sv, gs.EYE[None], gs.SHIFT[None], stride, VS, grid, **full)
    for counts_only in (False, True):
        sc = dst.register_score(src, gs.EYE[None], gs.SHIFT[None], stride=stride, huber=huber, counts_only=counts_only, **gates)
        assert int(sc["e"][0]) == (0 if counts_only else int(want[tr.I_E])) and int(ref["e"][0]) == int(want[tr.I_E]), f"{what}: score e {sc['e'][0]} / {want[tr.I_E]}"
        for f in ("n_used", "n_unknown", "n_far", "n_grad"):
            assert int(sc[f][0]) == co[f] == int(ref[f][0]), f"{what}: score {f} {sc[f][0]} / {co[f]}"
        gate = rsr.gate(sv, stride, **full)
        assert {k: sc["gate"][k] for k in gate} == gate and gate["n_gate"] == want[tr.I_GATE], f"{what}: gate {sc['gate']} / {gate}"
    return want


def _counts(sums):
    return dict(zip(COUNTS, (int(v) for v in sums[tr.I_USED:])))


# ---- A: stored values that are not finite -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(gs.SPECIALS))
def test_a_points_and_image(hip_lib, kind):
    """one NaN, +inf, -inf or 65504 in a ramp, probed in the 8 cells around it at fraction 0, inside and at the last f32 of the cell: a sample whose
    interpolant is not finite is far, never used, and no sum is undefined"""
    p, base, tainted = gs.a_probes()
    m = gs.a_map(kind)
    g, grid = _loaded("SMALL", m), gs.grid("SMALL", m)
    for stride in (1, 2):
        for huber in (0.0, 0.1):
            sums, bucket, s = _points(g, grid, p, f"{kind}, stride {stride}, huber {huber}", stride=stride, huber=huber, **gs.OPEN)
            got = g.align_points_linearize(p, gs.EYE, gs.ZERO, stride=stride, huber=huber, per_point=True, **gs.OPEN)
            tn = tainted[::stride]
            assert (got["sums"] != gs.INT64_MIN).all() and (got["bucket"][~tn] == gs.USED).all()
            if kind in NOT_FINITE:
                assert (got["bucket"][tn] == gs.FAR).all() and not np.isfinite(got["s"][tn]).any() and got["n_used"] == (~tn).sum()
    # the image kernel: the pixels of a_image fall into the same cells
    _, ibase = gs.image_points(gs.a_image(), gs.A_K, gs.A_T)
    it, iu = gs.a_tainted(ibase), gs.expected_unknown(ibase, m)
    for stride in (1, 3):
        for counts_only in (False, True):
            want = tr.linearize(gs.a_image(), gs.EYE, gs.A_T, gs.A_K, stride, VS, grid)
            if counts_only:
                want[:tr.I_USED] = 0
            got = g.align_linearize(gs.a_image(), gs.EYE, gs.A_T, K=gs.A_K, stride=stride, counts_only=counts_only)
            bad = np.nonzero(got["sums"] != want)[0]
            assert bad.size == 0, f"{kind}, image, stride {stride}, counts only {counts_only}: sums {bad.tolist()} differ: {got['sums'][bad]} / {want[bad]}"
            assert got["sums"][tr.I_USED:].sum() == tr.visited(48, 64, stride)
            if kind in NOT_FINITE:
                assert got["n_far"] == it.reshape(48, 64)[::stride, ::stride].sum() and got["n_unknown"] == iu.reshape(48, 64)[::stride, ::stride].sum()


@pytest.mark.parametrize("kind", list(gs.SPECIALS))
def test_a_registration(hip_lib, kind):
    """the special value in the destination (the 8 source voxels that land in its cells are far) and in the source, beside a NaN weight (both voxels
    are gated)"""
    m = gs.a_map(kind)
    src_map = gs.a_source()
    dst, src = _loaded("SMALL", m), _loaded("SMALL", src_map, "src")
    for huber in (0.0, 0.02):
        want = _register(dst, src, src_map, gs.grid("SMALL", m), f"{kind} in the destination, huber {huber}", huber=huber)
        assert (want != gs.INT64_MIN).all()
        if kind in NOT_FINITE:
            assert _counts(want) == dict(n_used=117, n_gate=0, n_unknown=0, n_far=8, n_grad=0)
    clean, src_map = gs.a_map(), gs.a_source(kind)
    dst, src = _loaded("SMALL", clean), _loaded("SMALL", src_map, "src")
    want = _register(dst, src, src_map, gs.grid("SMALL", clean), f"{kind} in the source")
    assert _counts(want) == dict(n_used=123, n_gate=2, n_unknown=0, n_far=0, n_grad=0)


# ---- B: magnitudes ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", (1, 3))
@pytest.mark.parametrize("huber", (0.0, 4.0))
def test_b_points(hip_lib, stride, huber):
    """32768 points in the steep block: every product slot but e holds addends beyond 2^31 of both free signs, six sums exceed 2^53 at stride 1
    (tests/test_gn_limits_cpu.py asserts it); all 33 integers equal the restatement"""
    g = _loaded("SMALL", gs.b_map())
    sums, bucket, _ = _points(g, gs.grid("SMALL", gs.b_map()), gs.b_points(), f"stride {stride}, huber {huber}", stride=stride, huber=huber, **gs.B_POINT_GATES)
    assert sums[tr.I_USED] == tpr.visited(32768, stride) and (stride != 1 or (np.abs(sums[:28]) > 2 ** 53).any())
    if stride == 1:                                         # e beyond 2^31 per addend: the gentle blocks around +-100
        g = _loaded("SMALL", gs.b_e_map())
        sums, _, _ = _points(g, gs.grid("SMALL", gs.b_e_map()), gs.b_e_points(), f"the gentle blocks, huber {huber}", huber=huber, **gs.B_E_GATES)
        assert sums[tr.I_USED] == 600 and (huber != 0.0 or sums[tr.I_E] >= 600 * 2 ** 31)


def test_b_image(hip_lib):
    """a 160 x 120 image looking into the block from half a metre"""
    g, grid = _loaded("SMALL", gs.b_map()), gs.grid("SMALL", gs.b_map())
    for stride, huber in ((1, 0.0), (1, 4.0), (2, 0.0)):
        want = tr.linearize(gs.b_image(), gs.EYE, gs.B_T, gs.B_K, stride, VS, grid, huber=huber, **gs.B_IMAGE_GATES)
        got = g.align_linearize(gs.b_image(), gs.EYE, gs.B_T, K=gs.B_K, stride=stride, huber=huber, **gs.B_GATES)
        bad = np.nonzero(got["sums"] != want)[0]
        assert bad.size == 0, f"stride {stride}, huber {huber}: sums {bad.tolist()} differ: {got['sums'][bad]} / {want[bad]}"
        assert got["n_used"] > 19000 // stride ** 2 and (stride != 1 or huber or (np.abs(want[:28]) > 2 ** 53).any())


def test_b_registration(hip_lib):
    """2^3 whole source bricks with values of up to +-240 against a steep destination, band = r_max = 250, g_max = 48: the call is admitted, the
    addends reach 2^35, every sum 2^32"""
    dm, sm = gs.b_reg_destination(), gs.b_reg_source()
    dst, src, grid = _loaded("SMALL", dm), _loaded("SMALL", sm, "src"), gs.grid("SMALL", dm)
    for stride, huber in ((1, 0.0), (1, 4.0), (2, 0.0)):
        want = _register(dst, src, sm, grid, f"stride {stride}, huber {huber}", stride=stride, huber=huber, **gs.B_REG_GATES)
        assert want[tr.I_USED] > 30000 // stride ** 3 and want[tr.I_GRAD] > 0 and (huber or (np.abs(want[:28]) >= 2 ** 32).all())


# ---- C: the gates at equality -------------------------------------------------------------------------------------------------------------------------

def test_c_gates_at_equality(hip_lib):
    """one input on each gate's boundary and one a step past it; the bucket is the one the header's wording gives"""
    m = gs.c_map()
    g, grid = _loaded("SMALL", m), gs.grid("SMALL", m)
    v, g0 = gs.c_facts()
    lin = lambda p, what, **kw: _points(g, grid, p, what, **dict(gs.OPEN, **kw))
    step = lambda x: np.nextafter(F32(x), F32(0))
    assert lin(gs.c_corner_point(), "|s| == r_max", r_max=v)[1][0] == gs.USED
    assert lin(gs.c_corner_point(), "|s| above r_max", r_max=step(v))[1][0] == gs.FAR
    assert lin(gs.c_interior_point(), "gg == g_max^2", g_max=g0)[1][0] == gs.USED
    assert lin(gs.c_interior_point(), "gg above g_max^2", g_max=step(g0))[1][0] == gs.GRAD
    assert lin(gs.c_flat_point(), "a flat cell")[1][0] == gs.GRAD
    assert lin(gs.c_range_points(0.7, 3.3), "the range gate", d_min=0.7, d_max=3.3)[1].tolist() == [gs.UNKNOWN, gs.GATE, gs.UNKNOWN, gs.GATE]
    got = g.align_linearize(gs.C_DEPTH, gs.EYE, gs.ZERO, K=gs.A_K, d_min=0.5, d_max=2.5)
    assert np.array_equal(got["sums"], tr.linearize(gs.C_DEPTH, gs.EYE, gs.ZERO, gs.A_K, 1, VS, grid, d_min=0.5, d_max=2.5))
    assert {k: got[k] for k in COUNTS} == dict(n_used=0, n_gate=2, n_unknown=2, n_far=0, n_grad=0)
    sm, ok = gs.c_reg_source()
    want = _register(g, _loaded("SMALL", sm, "src"), sm, grid, "w == w_min, |t| == band", w_min=gs.C_W_MIN, band=gs.C_BAND)
    assert want[tr.I_GATE] == (~ok).sum() == 4 and want[tr.I_USED] == 4
    # huber: e and b written out from the stored values
    hm, p, v, gr = gs.c_huber_case()
    g, grid = _loaded("SMALL", hm), gs.grid("SMALL", hm)
    for huber, wgt in ((v, F32(1.0)), (step(v), step(v) / v)):
        sums = _points(g, grid, p, f"huber {huber!r}", huber=huber, **gs.B_E_GATES)[0]
        got = g.align_points_linearize(p, gs.EYE, gs.ZERO, huber=huber, **gs.B_E_GATES)
        assert got["n_used"] == 1 and got["e"] == gs.fixed((wgt * v) * v) and [int(x) for x in got["b"][:3]] == [gs.fixed((wgt * ga) * v) for ga in gr]


# ---- D: cell knownness at seams and walls -------------------------------------------------------------------------------------------------------------

def _knownness(geo, m, p, base, source, src, what):
    """a map whose known samples are all used: the kernels' buckets against the listed voxels, points and registration.  The decoy brick is loaded
    first and takes pool brick 0."""
    g = _loaded(geo, m, first=gs.decoy(geo))
    m = gs.union(gs.decoy(geo), m)
    grid = gs.grid(geo, m)
    sums, bucket, s = _points(g, grid, p, what, **gs.OPEN)
    got = g.align_points_linearize(p, gs.EYE, gs.ZERO, per_point=True, **gs.OPEN)
    unknown = gs.expected_unknown(base, m)
    assert np.array_equal(got["bucket"] == gs.UNKNOWN, unknown) and (got["bucket"][~unknown] == gs.USED).all() and not _bits32(got["s"][unknown]).any(), what
    want = _register(g, src, source, grid, what)
    ru = gs.expected_unknown(source["indices"], m)
    assert _counts(want) == dict(n_used=int((~ru).sum()), n_gate=0, n_unknown=int(ru.sum()), n_far=0, n_grad=0), what
    return unknown


@pytest.mark.parametrize("kind", gs.SEAM_KINDS, ids=lambda k: "seam-" + ("".join("xyz"[a] for a in k) or "none"))
@pytest.mark.parametrize("geo", gs.SEAM_GEOS)
def test_d_seams(hip_lib, geo, kind):
    """the cell [c, c + 1]^3 over 1, 2, 4 or 8 bricks: complete, each corner unobserved, each brick unallocated; 27 probes in each of the 27 cells"""
    p, base = gs.seam_probes(geo, kind)
    source = gs.seam_source(geo, kind)
    src = _loaded(geo, source, "src")
    for name, m in gs.seam_variants(geo, kind):
        unknown = _knownness(geo, m, p, base, source, src, f"{geo}, seam {kind}, {name}")
        assert unknown.any() == (name != "complete")


@pytest.mark.parametrize("geo", list(gs.GEOS))
def test_d_walls(hip_lib, geo):
    """cells with base lo - 1, lo, hi - 2 and hi - 1 at each of the six walls; a coordinate exactly at lo * voxel and the f32 below it; base -1"""
    for name, m, p, base in gs.wall_cases(geo):
        source = gs.wall_source(m)
        unknown = _knownness(geo, m, p, base, source, _loaded(geo, source, "src"), name)
        assert unknown.any() and not unknown.all()
    m, p, base = gs.origin_case()
    source = gs.wall_source(m)
    assert not _knownness(geo, m, p, base, source, _loaded(geo, source, "src"), f"{geo}, the origin").any()
