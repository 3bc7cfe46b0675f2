"""Helpers around DenseTSDF.nav_grid: cost tables for its lookup."""
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
