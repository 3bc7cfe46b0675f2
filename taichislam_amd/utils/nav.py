"""Helpers around DenseTSDF.nav_grid, nav_field and nav_field3d (DESIGN.md sections 4.15, 4.16, 4.18): cost tables for the lookup, the cost of a flight
volume's cells, the reach of frontier clusters."""
import numpy as np


def inflation_lut(voxel, radius_vox, inscribed, inflation, scale=10.0):
    """The u8 [R * R + 2] cost table of DenseTSDF.nav_grid for R = radius_vox, indexed by the squared distance d2 in voxels, after the inflation rule of
    costmap_2d / nav2, with d = sqrt(d2) * voxel in metres (float64): 254 (lethal) at d = 0, 253 (inscribed) for 0 < d <= inscribed,
    floor(252 * exp(-scale * (d - inscribed))) for inscribed < d <= inflation, 0 beyond that and for the far entry R * R + 1.  It never increases
    with d2."""
    R = int(radius_vox)
    if not 0 <= R <= 254:
        raise ValueError("inflation_lut: radius_vox must be 0 .. 254")
    voxel, inscribed, inflation, scale = float(voxel), float(inscribed), float(inflation), float(scale)
    if not (voxel > 0.0 and inscribed >= 0.0 and inflation >= inscribed and scale >= 0.0 and np.isfinite([voxel, inscribed, inflation, scale]).all()):
        raise ValueError("inflation_lut: needs voxel > 0, 0 <= inscribed <= inflation, scale >= 0, all finite")
    d = np.sqrt(np.arange(R * R + 2, dtype=np.float64)) * voxel
    lut = np.floor(252.0 * np.exp(-scale * (d - inscribed)))
    lut = np.where(d <= inscribed, 253.0, lut)
    lut = np.where(d > inflation, 0.0, lut)
    lut[0] = 254.0
    lut[R * R + 1] = 0.0
    return lut.astype(np.uint8)


def terrain_slope2(max_slope_deg, slope_base_vox):
    """The max_slope2 of DenseTSDF.nav_terrain for a slope limit in degrees at a Sobel stride of slope_base_vox cells: floor((tan(deg) * 128 * s)^2),
    at most 2^32 - 2; None = 2^32 - 1, which switches the test off."""
    if max_slope_deg is None:
        return 0xffffffff
    deg, s = float(max_slope_deg), int(slope_base_vox)
    if not 0.0 <= deg < 90.0 or not 1 <= s <= 16:
        raise ValueError("terrain_slope2: needs 0 <= max_slope_deg < 90 and a stride of 1 .. 16 cells")
    return min(0xfffffffe, int(np.floor((np.tan(np.radians(deg)) * 128.0 * s) ** 2)))


def terrain_slope_deg(slope2, slope_base_vox):
    """The slope in degrees (float64) of the `slope2` plane of DenseTSDF.nav_terrain: atan(sqrt(slope2) / (128 * s)); NaN where slope2 is 2^32 - 1 (no
    valid stencil).  Host numpy; tensors are copied."""
    a = np.asarray(slope2.cpu().numpy() if hasattr(slope2, "cpu") else slope2)
    if a.dtype == np.int32:                                      # a torch build without uint32 hands the bits over as int32
        a = a.view(np.uint32)
    a = a.astype(np.uint32)
    d =np.degrees(np.arctan(np.sqrt(a.astype(np.float64)) / (128.0 * int(slope_base_vox))))
    return np.where(a == 0xffffffff, np.nan, d)


NAV_UNREACHED = 0xffffffff


def _host(a):
    return np.asarray(a.cpu().numpy() if hasattr(a, "cpu") else a)


def _cluster_least(frontiers, f, ok, cell):
    """The shared tail of frontier_reach and frontier_reach3d: per cluster the least f[cell] over the frontier rows with ok, the first row on a tie.
    cell: one index array per axis of f, a row of frontiers["indices"] each."""
    if f.dtype == np.int32:                                      # a torch build without uint32 hands the bits over as int32
        f = f.view(np.uint32)
    cl = _host(frontiers["cluster"]).astype(np.int64).reshape(-1)
    m = len(frontiers["clusters"])
    value = np.full(m, NAV_UNREACHED, np.uint32)
    voxel = np.full(m, -1, np.int64)
    rows = np.nonzero(ok)[0]
    if rows.size:
        v = f[tuple(c[rows] for c in cell)].astype(np.int64)
        order = np.lexsort((rows, v, cl[rows]))                  # by cluster, then value, then row
        first = order[np.concatenate([[True], np.diff(cl[rows][order]) != 0])]
        hit = v[first] != NAV_UNREACHED
        value[cl[rows][first][hit]] = v[first][hit].astype(np.uint32)
        voxel[cl[rows][first][hit]] = rows[first][hit]
    return {"value": value, "voxel": voxel, "reached": value != NAV_UNREACHED}


def frontier_reach(frontiers, field_result, band, N=None, plane=0):
    """Which frontier clusters can be reached, and how cheaply: per cluster of a DenseTSDF.extract_frontiers result the least value of a DenseTSDF.nav_field
    result over the columns (i + N / 2, j + N / 2) of the cluster's voxels whose layer k lies in band = (k_min, k_max), both ends inclusive -- the band
    the field's cost plane was projected from -- and the voxel that attains it.  N: the width of the volume (default: the height of the field's planes);
    plane: the plane of the field to read.  Host numpy; tensors are copied.  Returns a dict: `value` uint32 [m] (NAV_UNREACHED for a cluster that has
    no voxel in the band or reaches nothing), `voxel` int64 [m] (the row of frontiers["indices"] that attains it, the first in the frontiers' order
    on a tie; -1 with NAV_UNREACHED), `reached` bool [m]."""
    field = _host(field_result["field"] if isinstance(field_result, dict) else field_result)
    if field.ndim == 2:
        field = field[None]
    f = field[int(plane)]
    N = int(f.shape[0] if N is None else N)
    idx = _host(frontiers["indices"]).astype(np.int64).reshape(-1, 3)
    ui, uj = idx[:, 0] + N // 2, idx[:, 1] + N // 2
    ok = (idx[:, 2] >= int(band[0])) & (idx[:, 2] <= int(band[1])) & (ui >= 0) & (ui < f.shape[0]) & (uj >= 0) & (uj < f.shape[1])
    return _cluster_least(frontiers, f, ok, (ui, uj))


# ---- 3-D: flight volumes for DenseTSDF.nav_field3d ----------------------------------------------------------------------
def flight_lut(voxel, inscribed, inflation, scale=10.0):
    """The u8 [256] cost table of DenseTSDF.flight_volume, indexed by the distance to the nearest surface in quarter voxels, q = floor(4 d / voxel)
    clipped to 0 .. 255, after the rule of inflation_lut with d = q * voxel / 4 in metres (float64), the near end of the entry's range: 254 (lethal) at
    q = 0, 253 (inscribed) for 0 < d <= inscribed, floor(252 * exp(-scale * (d - inscribed))) for inscribed < d <= inflation, 0 beyond that.  It never
    increases with q.  One sample stands for a whole cell of the volume, so `inscribed` must include half a cell diagonal on top of the vehicle's
    radius: stride * voxel * sqrt(3) / 2 -- a cell whose centre is further than that from every surface holds no surface voxel."""
    voxel, inscribed, inflation, scale = float(voxel), float(inscribed), float(inflation), float(scale)
    if not (voxel > 0.0 and inscribed >= 0.0 and inflation >= inscribed and scale >= 0.0 and np.isfinite([voxel, inscribed, inflation, scale]).all()):
        raise ValueError("flight_lut: needs voxel > 0, 0 <= inscribed <= inflation, scale >= 0, all finite")
    d = np.arange(256, dtype=np.float64) * (voxel / 4.0)
    lut = np.floor(252.0 * np.exp(-scale * (d - inscribed)))
    lut = np.where(d <= inscribed, 253.0, lut)
    lut = np.where(d > inflation, 0.0, lut)
    lut[0] = 254.0
    return lut.astype(np.uint8)


def distance_cost(dist, status, voxel, lut, cost_unknown=255, cost_outside=255):
    """The cost of a cell from the answer of DenseTSDF.query_esdf at its sample: q = clip(floor(float32(dist) * float32(4.0 / voxel)), 0, 255), the
    distance in quarter voxels, a negative distance (and a NaN) giving 0; status 0 -> lut[q] (u8 [256], flight_lut), 1 (unknown) -> cost_unknown, 2
    (outside the volume) -> cost_outside; the flag 0x80 of the status is ignored.  Pure: numpy in gives numpy out, torch tensors in give a tensor on
    their device.  Returns u8 of dist's shape."""
    k = np.float32(4.0 / float(voxel))
    if hasattr(dist, "is_cuda"):
        import torch
        t = torch.as_tensor(np.asarray(lut, np.uint8).reshape(256), device=dist.device) if not hasattr(lut, "is_cuda") else lut.to(dist.device).reshape(256)
        q = torch.nan_to_num(torch.floor(dist.float() * float(k)), nan=0.0, posinf=255.0, neginf=0.0).clamp(0.0, 255.0).long()
        s = status.to(dist.device) & 3
        c = t[q]
        c = torch.where(s == 1, torch.full_like(c, int(cost_unknown)), c)
        return torch.where(s == 2, torch.full_like(c, int(cost_outside)), c)
    d = np.asarray(dist, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.clip(np.nan_to_num(np.floor(d * k), nan=0.0, posinf=255.0, neginf=0.0), 0.0, 255.0).astype(np.int64)
    s = np.asarray(status, np.uint8) & 3
    c = np.asarray(lut, np.uint8).reshape(256)[q]
    c = np.where(s == 1, np.uint8(cost_unknown), c)
    return np.where(s == 2, np.uint8(cost_outside), c).astype(np.uint8)


def frontier_reach3d(frontiers, field_result, volume):
    """frontier_reach for a DenseTSDF.nav_field3d result: per cluster of a DenseTSDF.extract_frontiers result the least field value over the cells of the
    flight volume that hold the cluster's voxels, and the voxel that attains it.  volume: the dict of DenseTSDF.flight_volume; the voxel (i, j, k) lies
    in cell ((k + half[0] - origin[0]) // stride, (i + half[1] - origin[1]) // stride, (j + half[2] - origin[2]) // stride); voxels outside the volume
    do not count.  Host numpy; tensors are copied.  Returns the dict of frontier_reach: `value` uint32 [m] (NAV_UNREACHED for a cluster that has no voxel
    in the volume or reaches nothing), `voxel` int64 [m] (the row of frontiers["indices"] that attains it, the first in the frontiers' order on a tie;
    -1 with NAV_UNREACHED), `reached` bool [m]."""
    f = _host(field_result["field"] if isinstance(field_result, dict) else field_result)
    if f.ndim != 3:
        raise ValueError("frontier_reach3d: the field must be [D, H, W]")
    s = int(volume["stride"])
    org, half = [int(v) for v in volume["origin"]], [int(v) for v in volume["half"]]
    idx = _host(frontiers["indices"]).astype(np.int64).reshape(-1, 3)
    ck = (idx[:, 2] + half[0] - org[0]) // s
    ci = (idx[:, 0] + half[1] - org[1]) // s
    cj = (idx[:, 1] + half[2] - org[2]) // s
    ok = (ck >= 0) & (ck < f.shape[0]) & (ci >= 0) & (ci < f.shape[1]) & (cj >= 0) & (cj < f.shape[2])
    return _cluster_least(frontiers, f, ok, (ck, ci, cj))


# ---- safe corridors: the boxes of DenseTSDF.nav_boxes / nav_corridor in metres ---------------------------------------------
def corridor_metres(boxes, volume=None, N=None, voxel=None):
    """The boxes of DenseTSDF.nav_boxes / nav_corridor as metric boxes in the frame of query_esdf: float64 [..., 2, 3], the lower and the upper corner
    (x, y, z) of the union of the voxels of the box's cells.  boxes: [..., 6] = (k0, i0, j0, k1, i1, j1); a voxel of signed index n spans (n - 1/2) *
    voxel .. (n + 1/2) * voxel, its centre being where flight_volume places its samples.  volume: the dict of DenseTSDF.flight_volume -- cell n of an
    axis covers the signed voxel indices n * stride + origin - half .. + stride - 1 (layer -> z, row -> x, column -> y).  Without a volume the boxes
    are those of 2-D planes of the map (nav_grid, nav_terrain): N (the map's cells along x and y) and voxel give x and y, one voxel per cell, and z is
    NaN -- the plane's height range is the band's, which the boxes do not carry.  Rows of -1 (a seed outside, the rows past `count`) give NaN.  Host
    numpy; tensors are copied."""
    b = _host(boxes).astype(np.int64)
    if b.ndim < 1 or b.shape[-1] != 6:
        raise ValueError("corridor_metres: boxes must be [..., 6]")
    if volume is not None:
        s, vs = int(volume["stride"]), float(volume["voxel"])
        off = [int(o) - int(h) for o, h in zip(volume["origin"], volume["half"])]      # per (layer, row, col)
    else:
        if N is None or voxel is None:
            raise ValueError("corridor_metres: needs the dict of flight_volume, or N and voxel")
        s, vs = 1, float(voxel)
        off = [0, -(int(N) // 2), -(int(N) // 2)]
    out = np.empty(b.shape[:-1] + (2, 3), np.float64)
    for x, a in enumerate((1, 2, 0)):                               # x from the row, y from the column, z from the layer
        out[..., 0, x] = (b[..., a] * s + off[a] - 0.5) * vs
        out[..., 1, x] = (b[..., a + 3] * s + off[a] + s - 0.5) * vs
    if volume is None:
        out[..., 2] = np.nan
    out[(b < 0).any(-1)] = np.nan
    return out


# ---- B-spline trajectories: the samples of DenseTSDF.traj_linearize / traj_optimize, and a spline from a path --------------
def bspline_basis(sub):
    """f32 [sub + 1, 4]: the uniform cubic B-spline weights w_0 .. w_3 at u = m / sub, m = 0 .. sub, by the f32 recipe of the kernel (every product, sum
    and quotient rounded on its own): rows 0 and sub are (1, 4, 1, 0) / 6 and (0, 1, 4, 1) / 6"""
    f = np.float32
    u = (np.arange(int(sub) + 1).astype(f) / f(sub)).astype(f)
    v, u2 = f(1.0) - u, u * u
    u3 = u2 * u
    b = np.stack([(v * v) * v, (f(3.0) * u3 - f(6.0) * u2) + f(4.0), ((f(3.0) * u2 - f(3.0) * u3) + f(3.0) * u) + f(1.0), u3], 1)
    return (b / f(6.0)).astype(f)


def bspline_points(ctrl, sub, lengths=None):
    """The sample positions of uniform cubic B-splines, bit for bit those DenseTSDF.traj_linearize evaluates: f32 [n, (K - 3) * sub + 1, 3] ([S, 3] for
    one trajectory [K, 3]).  Sample j lies in span seg = min(j // sub, L - 4) at u = (j - seg * sub) / sub and is ((w0 c0 + w1 c1) + w2 c2) + w3 c3 over
    the control points seg .. seg + 3.  With lengths (integers [n], 4 .. K) a trajectory has (L - 3) * sub + 1 samples and its row is padded with its
    last sample, so that score_paths(bspline_points(ctrl, sub, lengths), clearance, lengths=(lengths - 3) * sub + 1) scores each on its own samples.
    Host numpy; tensors are copied."""
    c = _host(ctrl).astype(np.float32)
    one = c.ndim == 2
    c = c[None] if one else c
    if c.ndim != 3 or c.shape[2] != 3 or c.shape[1] < 4:
        raise ValueError("bspline_points: ctrl must be [n, K, 3] or [K, 3] with K >= 4")
    n, K = c.shape[:2]
    sub = int(sub)
    if sub < 1:
        raise ValueError("bspline_points: sub must be at least 1")
    L = np.full(n, K, np.int64) if lengths is None else _host(lengths).astype(np.int64).reshape(n)
    if n and (L.min() < 4 or L.max() > K):
        raise ValueError("bspline_points: a length outside 4 .. K")
    j = np.minimum(np.arange((K - 3) * sub + 1)[None, :], ((L - 3) * sub)[:, None])
    seg = np.minimum(j // sub, (L - 4)[:, None])
    w = bspline_basis(sub)[j - seg * sub]                           # [n, S, 4]
    rows = np.arange(n)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        p = ((w[..., 0:1] * c[rows, seg] + w[..., 1:2] * c[rows, seg + 1]) + w[..., 2:3] * c[rows, seg + 2]) + w[..., 3:4] * c[rows, seg + 3]
    p = p.astype(np.float32)
    return p[0] if one else p


def bspline_from_path(points, K):
    """K control points (float32 [K, 3], K >= 6) of a uniform cubic B-spline along a polyline: the polyline is resampled by arc length at K - 4 points,
    its ends included, and both ends are tripled, so that the spline starts and ends AT the path's ends, at rest, and fix_ends = 3 of
    DenseTSDF.traj_optimize pins them.  points: float [m, 3] metres in the frame of query_esdf, m >= 1 -- a path of DenseTSDF.nav_paths3d in metres, or
    the centres of the boxes of corridor_metres.  Repeated points are fine.  Float64 host code."""
    p = _host(points).astype(np.float64).reshape(-1, 3)
    K = int(K)
    if K < 6 or p.shape[0] < 1 or not np.isfinite(p).all():
        raise ValueError("bspline_from_path: needs K >= 6 and at least one finite point")
    s = np.concatenate([[0.0], np.cumsum(np.sqrt((np.diff(p, axis=0) ** 2).sum(1)))])
    t = np.linspace(0.0, s[-1], K - 4)
    mid = np.stack([np.interp(t, s, p[:, a]) for a in range(3)], 1)
    mid[0], mid[-1] = p[0], p[-1]
    return np.concatenate([mid[:1], mid[:1], mid, mid[-1:], mid[-1:]], 0).astype(np.float32)
