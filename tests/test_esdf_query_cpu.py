"""ESDF point queries without a GPU: the C-ABI entry points are declared, exported and bound; DenseTSDF.query_esdf has its keywords; the
numpy float32 restatement the GPU tests compare against (tests/esdf_query_ref.py) behaves as a trilinear interpolant should."""
import ctypes
import inspect
import math
import os
import re

import numpy as np

import esdf_query_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declaration(name):
    txt = open(os.path.join(ROOT, "include", "taichislam_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/taichislam_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_query_symbols_declared_exported_and_bound():
    from taichislam_amd import _lib
    for name, nargs in (("tsl_esdf_query_points", 8), ("tsl_esdf_query_points_dev", 9)):
        assert len(_declaration(name)) == nargs
        assert hasattr(ctypes.CDLL(_lib.library_path()), name), f"{name} is not exported by the built library"
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
        assert args[2] is ctypes.c_float and args[4] is ctypes.c_int64       # unknown_value, n


def test_query_esdf_keywords():
    from taichislam_amd.mapping import DenseTSDF
    p = inspect.signature(DenseTSDF.query_esdf).parameters
    assert list(p)[:2] == ["self", "xyz"]
    assert p["interpolate"].default is True and p["gradient"].default is None and p["refresh"].default is True
    assert math.isnan(p["unknown_value"].default)


def _ulp_close(a, b64, ulps, scale):
    """|a - b64| within `ulps` f32 ulps of `scale` (the size of the operands the interpolation combines)"""
    return np.abs(a.astype(np.float64) - b64) <= ulps * np.spacing(np.float32(scale)).astype(np.float64)


def test_restatement_returns_the_corner_at_zero_fraction():
    rng = np.random.default_rng(1)
    c = rng.uniform(-2, 2, (5000, 8)).astype(np.float32)
    c[c == 0] = 0.5
    d, g = ref.trilinear(c, np.zeros((5000, 3), np.float32), 0.04)
    assert np.array_equal(d.view(np.uint32), c[:, 0].view(np.uint32))
    # and the gradient at the corner is the forward difference of each axis
    assert np.array_equal(g[:, 0], (c[:, 4] - c[:, 0]) / np.float32(0.04))
    assert np.array_equal(g[:, 2], (c[:, 1] - c[:, 0]) / np.float32(0.04))


def test_restatement_reproduces_an_affine_field():
    rng = np.random.default_rng(2)
    vs = np.float32(0.05)
    n = 20000
    a = rng.uniform(-1, 1, (n, 3))
    d0 = rng.uniform(-1, 1, n)
    p = np.array([[cc >> 2, (cc >> 1) & 1, cc & 1] for cc in range(8)], np.float64)
    c = (d0[:, None] + (p[None] * a[:, None, :]).sum(2) * float(vs)).astype(np.float32)
    f = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    d, g = ref.trilinear(c, f, vs)
    # the corners are the affine field rounded to f32: the gradient is a's up to a few roundings of the corner differences
    assert np.abs(g - a).max() < 1e-5 / float(vs) * 8
    true = d0 + (f.astype(np.float64) * a).sum(1) * float(vs)
    assert np.abs(d - true).max() < 1e-6 * 8


def test_restatement_agrees_with_float64_trilinear():
    rng = np.random.default_rng(3)
    n = 50000
    c = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
    f = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    d, g = ref.trilinear(c, f, 1.0)
    c64, f64 = c.astype(np.float64), f.astype(np.float64)
    w = np.ones((n, 8))
    for cc in range(8):
        for ax, bit in ((0, cc >> 2), (1, (cc >> 1) & 1), (2, cc & 1)):
            w[:, cc] *= f64[:, ax] if bit else 1 - f64[:, ax]
    d64 = (w * c64).sum(1)
    assert _ulp_close(d, d64, 8, 1.0).all()
    # the gradient along x: the bilinear interpolation of the four x differences over (f1, f2)
    gx = np.zeros(n)
    for q in (0, 1):
        for r in (0, 1):
            wy = f64[:, 1] if q else 1 - f64[:, 1]
            wz = f64[:, 2] if r else 1 - f64[:, 2]
            gx += wy * wz * (c64[:, 4 | q << 1 | r] - c64[:, q << 1 | r])
    assert _ulp_close(g[:, 0], gx, 16, 2.0).all()


def test_restatement_query_status_and_nearest():
    """the grid form: status 2 outside the volume (2 wins over 1) and for non-finite input, 1 next to an unknown voxel, mode 0 = nearest voxel"""
    N, Nz, vs = 32, 32, np.float32(0.1)
    idx = np.stack(np.meshgrid(*[np.arange(-4, 4)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.int16)
    val = (idx.astype(np.float32) * vs).sum(1)
    g, k, lo = ref.grid_from_export(idx, val, N, Nz)
    pts = np.array([[0.0, 0.0, 0.0], [0.12, -0.21, 0.05], [0.34, 0.0, 0.0], [0.36, 0.0, 0.0], [1.4, 0.0, 0.0], [5.0, 0.0, 0.0],
                    [np.nan, 0.0, 0.0], [-1.55, -1.55, -1.55]], np.float32)
    d0, _, s0 = ref.query(pts, 0, vs, g, k, lo, unknown=-7.0)
    d1, g1, s1 = ref.query(pts, 1, vs, g, k, lo, unknown=-7.0)
    assert list(s0) == [0, 0, 0, 1, 1, 2, 2, 1] and list(s1) == [0, 0, 1, 1, 1, 2, 2, 1]
    assert d0[0] == 0 and d0[2] == val[(idx == [3, 0, 0]).all(1)][0]
    assert np.array_equal(d0[[3, 4, 5, 6]], np.full(4, -7.0, np.float32)) and (g1[s1 != 0] == 0).all()
    # the affine field is reproduced inside the known block
    assert abs(d1[1] - np.float32(0.12 - 0.21 + 0.05)) < 1e-6 and np.abs(g1[1] - 1.0).max() < 1e-5
