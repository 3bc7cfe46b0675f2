"""What tests/test_register_search_cpu.py and tests/test_register_search_gpu.py share: the two guesses the pose search is for, on the maps of
tests/register_scenes.py, the default lattice of DenseTSDF.register_search, the reference runs (computed once, never written) and what they measured."""
import functools
import math

import numpy as np

import register_ref as rr
import register_scenes as rs
import register_search_ref as sr
import track_scenes as ts
from util import SMALL

VOXEL = SMALL["voxel_scale"]
# the defaults of DenseTSDF.register_search: 9 x 9 x 5 translations x 13 yaw angles
WINDOW_T, STEP_T, WINDOW_R, STEP_R, STRIDE = (0.8, 0.8, 0.4), 0.2, (0.0, 0.0, math.pi / 3), math.pi / 18, 4
N_T, STEPS_T = sr.half_counts(WINDOW_T, STEP_T)
N_R, STEPS_R = sr.half_counts(WINDOW_R, STEP_R)
N_CANDIDATES = 5265
# guess = (Cg Rd, Cg (Td - c) + c + dt): D turned by `deg` about `axis` through the true centroid c, then shifted by dt
GUESSES = {"B": ((0.7, -0.6, 0.3), (0.0, 0.0, 1.0), 55.0), "C": ((-0.7, -0.7, -0.3), (0.05, 0.1, 1.0), -58.0)}
# Measured with the restatement over the oracle's maps (tests/test_register_search_cpu.py::test_search_recovers_what_the_registration_loses prints them).
# register_ref.register directly from the guess: final error, status.  The search with the defaults above, miss = r_max = 0.4: the best candidate, its
# cost, the valid candidates, the error of the best candidate and the final error after the refinement (status 0, 8 linearisations).
MEASURED_DIRECT = {"B": (3.640071, 91.971157, 1), "C": (1.940795, 38.387759, 2)}
MEASURED_BEST = {"B": (81, 14502224, 5265), "C": (5263, 10594363, 4642)}
MEASURED_BEST_ERROR = {"B": (0.150322, 0.272999), "C": (0.289669, 6.634646)}
MEASURED_FINAL = {"B": (0.000807, 0.013677, 0, 8), "C": (0.000807, 0.013677, 0, 8)}


@functools.lru_cache(maxsize=None)
def centroid():
    """the centroid of the source's voxels in the band (every observed voxel, stride 1), in source coordinates, and carried by D"""
    idx, t, w = rs.src_voxels()
    with np.errstate(invalid="ignore"):
        ok = (w >= rs.GATES["w_min"]) & ~(np.abs(t) > rs.GATES["band"])
    qb = idx[ok].sum(0).astype(np.float64) / float(ok.sum()) * VOXEL
    Rd, Td = rs.displacement()
    return qb, Rd @ qb + Td


def guess(name):
    dt, axis, deg = GUESSES[name]
    Rd, Td = rs.displacement()
    c = centroid()[1]
    Cg = ts.rotation(axis, deg)
    return Cg @ Rd, Cg @ (Td - c) + c + np.array(dt)


@functools.lru_cache(maxsize=None)
def direct_run(name):
    """register_ref.register from the guess itself"""
    return rr.register(rs.src_voxels(), *guess(name), rs.VS, rs.dst_grid(), **rs.GATES)


@functools.lru_cache(maxsize=None)
def reference_search(name):
    """register_search_ref.search from the guess with the default lattice"""
    return sr.search(rs.src_voxels(), *guess(name), rs.VS, rs.dst_grid(), VOXEL, N_T, STEPS_T, N_R, STEPS_R, stride=STRIDE, **rs.GATES)
