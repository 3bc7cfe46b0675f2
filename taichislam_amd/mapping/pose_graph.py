"""PoseGraph: the poses of submaps under relative-pose constraints, solved once per variant (a bit mask over the edges) in one launch, one workgroup per
variant (include/taichislam_hip.h, "pose graph"; csrc/tsl_pose_graph.hip).  It knows no map: the edges are what
SubmapMapping.register_submaps / search_submaps return, the result is what SubmapMapping.set_frame_poses takes.

A pose (R, T) takes submap coordinates to the common frame; an edge (a, b, Z, L) says that P_b^-1 P_a was measured as Z = (Rz, Tz) with the information
matrix L in twist order (v, omega), the left twist in b's frame."""
import ctypes as C

import numpy as np

from .. import _lib
from ._sides import HOST, _is_device_tensor, _vp, device_side

REPORT_DTYPE = np.dtype(_lib.PGO_REPORT_FIELDS)
STATUS_NAMES = _lib.PGO_STATUS
_SOLVER = dict(iters=20, damping=1e-6, damping_up=10.0, damping_down=10.0, damping_min=1e-12, damping_max=1e6, pcg_tol=1e-3, pcg_max=1000, min_step=1e-6,
               rel_tol=1e-9, huber=0.0)


def pack_information(L):
    """[E, 6, 6] symmetric (or [E, 21] already packed) -> the 21 upper-triangle entries per edge the library takes"""
    L = np.asarray(L, np.float64)
    if L.ndim >= 2 and L.shape[-2:] == (6, 6):
        L = np.stack([L[..., a, c] for a in range(6) for c in range(a, 6)], axis=-1)
    return np.ascontiguousarray(L.reshape(-1, 21))


def pack_measurements(Rz, Tz):
    """[E, 3, 3] and [E, 3] -> Z [E, 12]"""
    return np.ascontiguousarray(np.concatenate([np.asarray(Rz, np.float64).reshape(-1, 9), np.asarray(Tz, np.float64).reshape(-1, 3)], axis=1))


def edge_masks(rows):
    """bool [B, E] (True: the edge takes part) -> uint64 [B, ceil(E / 64)]"""
    rows = np.atleast_2d(np.asarray(rows, bool))
    B, E = rows.shape
    bits = np.zeros((B, ((E + 63) // 64) * 64), np.uint8)
    bits[:, :E] = rows
    return np.ascontiguousarray(np.packbits(bits.reshape(B, -1, 8), axis=-1, bitorder="little").reshape(B, -1)).view(np.uint64)


def _host(a, kind):
    """ij, fixed and the masks are read on the host in both forms"""
    if a is None:
        return None
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a).astype(kind, copy=False))


class PoseGraph:
    def __init__(self, max_poses, max_edges, max_variants=1, device=0):
        """capacities: at most 8192 poses, 131072 edges, 1024 variants, and max_variants * (720 max_poses + 56 max_edges) bytes under 1 GiB"""
        self.L = _lib.lib()
        self.device = int(device)
        self.max_poses, self.max_edges, self.max_variants = int(max_poses), int(max_edges), int(max_variants)
        h = C.c_void_p()
        _lib.check(self.L.tsl_pgo_create(self.device, self.max_poses, self.max_edges, self.max_variants, C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None) is not None:
                self.L.tsl_pgo_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _inputs(self, who, R, T, fixed, ij, Z, L):
        """the side of the call and its arrays: R, T, Z, L float64 on that side, ij int32 [E, 2] and fixed uint8 [N] on the host"""
        device = _is_device_tensor(R)
        if device:
            side = device_side(R.device)
            big = []
            for name, a, tail in (("R", R, 9), ("T", T, 3), ("Z", Z, 12), ("L", L, 21)):
                if not _is_device_tensor(a) or a.dtype != side._kinds["f8"] or not a.is_contiguous() or a.device.index != self.device or a.numel() % tail:
                    raise ValueError(f"PoseGraph.{who}: with R on the device, {name} must be a contiguous float64 tensor on the graph's device")
                big.append(a)
            R, T, Z, L = big
            N, E = R.numel() // 9, Z.numel() // 12
            if T.numel() != 3 * N or L.numel() != 21 * E:
                raise ValueError(f"PoseGraph.{who}: R [N, 3, 3], T [N, 3], Z [E, 12] and L [E, 21] do not agree")
        else:
            side = HOST
            R = np.ascontiguousarray(np.asarray(R, np.float64).reshape(-1, 3, 3))
            T = np.ascontiguousarray(np.asarray(T, np.float64).reshape(-1, 3))
            Z = np.ascontiguousarray(np.asarray(Z, np.float64).reshape(-1, 12))
            L = pack_information(L)
            N, E = R.shape[0], Z.shape[0]
            if T.shape[0] != N or L.shape[0] != E:
                raise ValueError(f"PoseGraph.{who}: R [N, 3, 3], T [N, 3], Z [E, 12] and L [E, 21] do not agree")
        ij = _host(ij, np.int32).reshape(-1, 2)
        fixed = None if fixed is None else _host(fixed, np.uint8).reshape(-1)
        if ij.shape[0] != E or (fixed is not None and fixed.shape[0] != N):
            raise ValueError(f"PoseGraph.{who}: ij must be [E, 2] and fixed [N]")
        return side, R, T, fixed, ij, Z, L, N, E

    def linearize(self, R, T, fixed, ij, Z, L, mask=None, huber=0.0):
        """One mask (uint64 [ceil(E / 64)] or None = every edge): {"r" [E, 6], "cost" [E] = r^T L r, "flipped" uint8 [E], "Hd" [N, 21] (the upper triangle
        of every pose's block) and "g" [N, 6]}, on the side R came from (numpy, or float64 torch tensors on the graph's device; ij, fixed and mask are
        read on the host either way).  Rows of fixed poses are 0; fixed may be None."""
        side, R, T, fixed, ij, Z, L, N, E = self._inputs("linearize", R, T, fixed, ij, Z, L)
        mask = None if mask is None else _host(mask, np.uint64).reshape(-1)
        if mask is not None and mask.shape[0] != (E + 63) // 64:
            raise ValueError("PoseGraph.linearize: mask must hold ceil(E / 64) words")
        out = {"r": side.out((E, 6), "f8"), "cost": side.out((E,), "f8"), "flipped": side.out((E,), "u1"), "Hd": side.out((N, 21), "f8"), "g": side.out((N, 6), "f8")}
        side.call(self.L.tsl_pgo_linearize, self.L.tsl_pgo_linearize_dev, self.h, N, side.ptr(R), side.ptr(T), _vp(fixed), E, _vp(ij), side.ptr(Z), side.ptr(L),
                  _vp(mask), float(huber), *(side.ptr(out[k]) for k in ("r", "cost", "flipped", "Hd", "g")))
        return out

    def solve(self, R, T, fixed, ij, Z, L, masks=None, *, iters=20, damping=1e-6, damping_up=10, damping_down=10, damping_min=1e-12, damping_max=1e6,
              pcg_tol=1e-3, pcg_max=1000, min_step=1e-6, rel_tol=1e-9, huber=0):
        """Solve the graph once per variant: masks uint64 [B, ceil(E / 64)] (edge_masks builds them), None = one variant with every edge.  Returns {"R"
        [B, N, 3, 3], "T" [B, N, 3], "r" [B, E, 6] and "edge_cost" [B, E] (r^T L r of EVERY edge at the variant's final poses, enabled or not), "report"},
        on the side R came from.  On the host "report" is a record array [B] of REPORT_DTYPE: status (STATUS_NAMES), iterations, cost, and per iteration
        it[k] = (cost_before, cost_after, max_step, damping, pcg_iters, accepted).  On the device it is the same bytes as a uint8 tensor [B, 2576],
        ordered with torch.cuda.current_stream like the rest; PoseGraph.decode reads it (and waits)."""
        side, R, T, fixed, ij, Z, L, N, E = self._inputs("solve", R, T, fixed, ij, Z, L)
        if fixed is None:
            raise ValueError("PoseGraph.solve: fixed must name at least one pose")
        W = (E + 63) // 64
        masks = None if masks is None else _host(masks, np.uint64).reshape(-1, W)
        B = 1 if masks is None else masks.shape[0]
        cfg = _lib.PgoCfg(int(iters), int(pcg_max), float(damping), float(damping_up), float(damping_down), float(damping_min), float(damping_max), float(pcg_tol),
                          float(min_step), float(rel_tol), float(huber))
        out = {"R": side.out((B, N, 3, 3), "f8"), "T": side.out((B, N, 3), "f8"), "r": side.out((B, E, 6), "f8"), "edge_cost": side.out((B, E), "f8"),
               "report": side.out((B, REPORT_DTYPE.itemsize), "u1")}
        side.call(self.L.tsl_pgo_solve, self.L.tsl_pgo_solve_dev, self.h, N, side.ptr(R), side.ptr(T), _vp(fixed), E, _vp(ij), side.ptr(Z), side.ptr(L), B, _vp(masks),
                  C.byref(cfg), *(side.ptr(out[k]) for k in ("R", "T", "r", "edge_cost", "report")))
        if side is HOST:
            out["report"] = self.decode(out["report"])
        return out

    @staticmethod
    def decode(report):
        """the report bytes [B, 2576] (numpy, or a torch tensor: copied to the host, which waits for it) as a record array [B] of REPORT_DTYPE"""
        if hasattr(report, "detach"):
            report = report.detach().cpu().numpy()
        return np.ascontiguousarray(report).view(REPORT_DTYPE).reshape(-1)

    def leave_one_out(self, R, T, fixed, ij, Z, L, edges, **solver_kw):
        """Variant 0 solves with every edge; variant 1 + k with every edge but edges[k].  Returns solve's result with "masks" (bool [1 + K, E]) and, on the
        host, "loo_cost" [K]: the cost r^T L r of edges[k] under the solution that did not see it -- a raw number to compare and rank, not a chi-square --
        and "full_cost" [K]: the same edges under the solution with every edge."""
        E = _host(ij, np.int32).reshape(-1, 2).shape[0]
        edges = np.asarray(edges, np.int64).reshape(-1)
        rows = np.ones((1 + edges.shape[0], E), bool)
        rows[1 + np.arange(edges.shape[0]), edges] = False
        out = self.solve(R, T, fixed, ij, Z, L, edge_masks(rows), **solver_kw)
        out["masks"] = rows
        if isinstance(out["edge_cost"], np.ndarray):
            out["loo_cost"] = out["edge_cost"][1 + np.arange(edges.shape[0]), edges].copy()
            out["full_cost"] = out["edge_cost"][0, edges].copy()
        return out
