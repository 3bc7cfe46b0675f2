"""Helpers of the pose graph (mapping.PoseGraph, SubmapMapping.optimize_poses)."""
import numpy as np


def pose_information(sigma_t, sigma_r):
    """The diagonal 6 x 6 information matrix of a relative pose known to sigma_t metres and sigma_r radians per axis, in the twist order (v, omega) of
    PoseGraph and of register_submaps' info["information"]: diag(1 / sigma_t^2 x 3, 1 / sigma_r^2 x 3)."""
    sigma_t, sigma_r = float(sigma_t), float(sigma_r)
    if not (sigma_t > 0.0 and sigma_r > 0.0 and np.isfinite(sigma_t) and np.isfinite(sigma_r)):
        raise ValueError("pose_information: the sigmas must be positive and finite")
    return np.diag([1.0 / (sigma_t * sigma_t)] * 3 + [1.0 / (sigma_r * sigma_r)] * 3)
