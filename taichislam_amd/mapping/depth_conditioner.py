"""DepthConditioner: raw uint16 millimetre depth frames lose their flying pixels and speckle, the pixels that stay are smoothed by an integer bilateral
filter, and the result is halved into coarser levels (include/taichislam_hip.h, "depth conditioning"; csrc/tsl_depth.hip).  One launch
conditions the whole batch.  The conditioner knows no map: its output is a depth image like any other, for recast_depth_to_map, track_depth / track_rgbd
or the Octomap."""
import ctypes as C

import numpy as np

from .. import _lib
from ..utils.depth import bilateral_tables, depth_tolerance
from ._sides import HOST, _is_device_tensor, _vp, device_side

STATUS_NAMES = ("kept", "hole", "range", "sparse", "edge")


class DepthConditioner:
    def __init__(self, device=0, tol=None, ws=None, wr=None):
        """tol uint16 [256], ws uint8 [5, 5], wr uint8 [17] (set_tables); None = utils.depth_tolerance() and utils.bilateral_tables(4, sigma_px=1.5); a radius
        below 4 reads only its own corner of ws"""
        self.L = _lib.lib()
        self.device = int(device)
        h = C.c_void_p()
        _lib.check(self.L.tsl_depth_create(self.device, C.byref(h)))
        self.h = h
        self.set_tables(tol, ws, wr)

    def __del__(self):
        try:
            if getattr(self, "h", None) is not None:
                self.L.tsl_depth_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def set_tables(self, tol=None, ws=None, wr=None):
        """The tolerance per 256 mm depth bin and the two weight tables; a table left None takes its default.  The integers are the definition: every tol
        entry in 1 .. 32767 and ws[0, 0] * wr[0] > 0, or the library refuses them and keeps the tables it had."""
        d_ws, d_wr = bilateral_tables(4, sigma_px=1.5)
        tol = depth_tolerance() if tol is None else tol
        ws, wr = d_ws if ws is None else ws, d_wr if wr is None else wr
        tabs = []
        for name, a, kind, shape in (("tol", tol, np.uint16, (256,)), ("ws", ws, np.uint8, (5, 5)), ("wr", wr, np.uint8, (17,))):
            b = np.asarray(a)
            if b.shape != shape or b.dtype.kind not in "iu" or b.min() < 0 or b.max() > np.iinfo(kind).max:
                raise ValueError(f"DepthConditioner: {name} must be {shape} integers that fit {np.dtype(kind).name}")
            tabs.append(np.ascontiguousarray(b, kind))
        _lib.check(self.L.tsl_depth_set_tables(self.h, _vp(tabs[0]), _vp(tabs[1]), _vp(tabs[2])))
        self.tol, self.ws, self.wr = tabs

    def condition(self, depth, d_min=None, d_max=None, min_support=6, erode=1, radius=2, erode_holes=False, levels=0, min_valid=2, status=False):
        """depth: uint16 millimetres, [h, w] or [n, h, w] (n <= 64), a numpy array or a contiguous torch tensor on this conditioner's device (int16 = the
        same bits).  d_min / d_max in metres gate the range (None = 1 mm .. 65535 mm).  A pixel with fewer than min_support of its 8 neighbours within
        its depth's tolerance is dropped (flying pixels, speckle, both sides of a step), and so is everything within `erode` pixels of one (erode_holes:
        of a hole as well); the pixels kept are smoothed over a (2 radius + 1)^2 window of kept pixels within tolerance.  levels: how many half-resolution
        levels to build, each pixel the mean of the foreground of its 2 x 2 block, 0 with fewer than min_valid valid pixels (utils.halved_intrinsics
        gives their K).  Returns {"depth", "levels": [...], "counts": int64 [n, 5] by status (kept, hole, range, sparse, edge), "status": uint8 or None}
        on the side the input came from, a torch result ordered with torch.cuda.current_stream; a [h, w] input gives [h, w] outputs and counts [5]."""
        device = _is_device_tensor(depth)
        if device:
            side = device_side(depth.device)
            if depth.dtype not in (side._kinds["u2"], side._kinds["i2"]) or not depth.is_contiguous() or depth.device.index != self.device:
                raise ValueError("DepthConditioner.condition: a device depth must be a contiguous uint16 tensor (int16 = the same bits) on the conditioner's device")
            d = depth
        else:
            side = HOST
            d = np.ascontiguousarray(np.asarray(depth, dtype=np.uint16))
        if d.ndim not in (2, 3):
            raise ValueError("DepthConditioner.condition: depth must be [h, w] or [n, h, w]")
        single = d.ndim == 2
        n, h, w = (1,) + tuple(d.shape) if single else tuple(d.shape)
        levels = int(levels)
        if not 0 <= levels <= 3:
            raise ValueError("DepthConditioner.condition: levels must be 0 .. 3")
        lo = 1 if d_min is None else int(np.rint(1000.0 * d_min))
        hi = 65535 if d_max is None else int(np.rint(1000.0 * d_max))
        cfg = _lib.DepthCfg(n, h, w, lo, hi, int(min_support), int(erode), int(radius), 1 if erode_holes else 0, levels, int(min_valid), 0)
        lead = () if single else (n,)
        kind = "u2" if not device or d.dtype == side._kinds["u2"] else "i2"
        out = side.out(lead + (h, w), kind)
        st = side.out(lead + (h, w), "u1") if status else None
        counts = side.out(lead + (5,), "i8")
        lv = [side.out(lead + (h >> l, w >> l), kind) for l in range(1, levels + 1)]
        lp = [side.ptr(a) for a in lv] + [None] * (3 - levels)
        side.call(self.L.tsl_depth_condition, self.L.tsl_depth_condition_dev, self.h, C.byref(cfg), side.ptr(d), side.ptr(out), side.ptr(st), side.ptr(counts), *lp)
        return {"depth": out, "levels": lv, "counts": counts, "status": st}
