"""Scenes, fans and poses shared by tests/test_view_gain_cpu.py and tests/test_view_gain_gpu.py: the hand-built maps of tests/frontier_scenes.py seen by
fans of 24 x 20 rays (a multiple of neither 8 nor 16: partial tiles and partial workgroups), and the room of tests/render_view_scenes.py."""
import numpy as np

import frontier_scenes as fs
import render_view_scenes as rv
import view_gain_ref as ref
from taichislam_amd.utils import synthetic as syn
from util import SMALL, tilt

VS = SMALL["voxel_scale"]
H, W = 20, 24                                              # the fan: 24 rays across, 20 down
K_FAN = np.array([14.0, 0.0, 11.5, 0.0, 14.0, 9.5, 0.0, 0.0, 1.0])      # about 80 degrees across
T_MIN = 0.05
T_MAX = {"SMALL": 6.5, "SLAB": 2.5, "TALL": 2.5}           # SMALL: the pose outside the volume is 5.5 m from the scene
SCENE_NAMES = ("shell", "plate", "two_unknowns", "two_values", "wall")


def scene(name, geo):
    return fs.wall(geo) if name == "wall" else fs.SCENES[name]()


def centre(name, geo):
    """the centre of the scene's free block in scene voxel coordinates (before place())"""
    if name == "two_unknowns":
        return np.array([7.5, 7.5, 7.5])
    if name == "wall":
        g = fs.GEOMETRIES[geo]
        top = (g["Nz"] if g["swap"] else g["N"]) // 2 - 1 - g["o"][2 if g["swap"] else 0]
        return np.array([top - 3.5, 3.5, 3.5])
    return np.array([-0.5, -0.5, -0.5])


def placed(p, geo):
    """a point in scene voxel coordinates -> metres in the map frame of the geometry: what frontier_scenes.place does to the voxels"""
    g = fs.GEOMETRIES[geo]
    p = np.asarray(p, np.float64)
    if g["swap"]:
        p = p[::-1]
    return (p + np.array(g["o"], np.float64)) * VS


def look(eye, target, up=(0.0, 0.0, 1.0)):
    """camera-to-map rotation (x right, y down, z forward) of a camera at `eye` looking at `target`; another up where the direction is along it"""
    z = np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    z /= np.linalg.norm(z)
    up = np.asarray(up, np.float64)
    if abs(z @ up) > 0.95:
        up = np.array([0.0, 1.0, 0.0])
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], 1)


OUTSIDE_EYE = {"SMALL": (-5.5, 0.03, 0.05), "SLAB": (0.3, 0.35, 1.25), "TALL": (1.6, 0.02, 0.03)}      # beyond the -x / +z / +x wall of the volume


def scene_poses(name, geo):
    """(R [5, 3, 3], T [5, 3]): at the block's centre along +x and along a diagonal, one off-lattice tilt, one outside the free region looking in, one
    outside the volume looking in.  The eye is a little off the voxel lattice."""
    c = centre(name, geo)
    off = np.array([0.33, 0.18, -0.27])
    eye = placed(c + off, geo)
    along = look(eye, placed(c + off + np.array([10.0, 0.0, 0.0]), geo))
    diag = look(eye, placed(c + off + np.array([10.0, 9.0, 7.0]), geo))
    far = placed(c + np.array([-30.3, 2.4, 1.3]), geo)
    out = placed(c + np.array([12.3, 1.3, 0.8]), geo) if name == "wall" else np.array(OUTSIDE_EYE[geo])      # wall: beyond the wall the block stands against
    Rs = [along, diag, tilt(along, 0.3, 0.2), look(far, eye), look(out, eye)]
    Ts = [eye, eye, eye, far, out]
    return np.stack(Rs), np.stack(Ts)


def fan_kwargs(geo):
    """the keywords of DenseTSDF.score_views for the scene fans"""
    return dict(K=K_FAN, shape=(H, W), t_min=T_MIN, t_max=T_MAX[geo])


def scene_ref(sc, geo, R, T, unknown_run=0, free_thres=None):
    """the restatement over a placed scene (its arrays are those of an export) or an export_sparse dictionary"""
    g = fs.GEOMETRIES[geo]
    return ref.score_export(sc, g["N"], g["Nz"], VS, R, T, K_FAN, H, W, T_MIN, T_MAX[geo], unknown_run=unknown_run, free_thres=free_thres)


# ---- the room: the four frames of render_view_scenes.room_scene(), seen by a 24 x 20 fan -- every 8th pixel of the centred 192 x 160 window of the camera
ROOM_STRIDE, ROOM_SHAPE = 8, (160, 192)


def room_K(K):
    """the 240 x 320 camera's K moved to the centred 192 x 160 window"""
    k = np.asarray(K, np.float64).reshape(-1).copy()
    k[2] -= (320 - ROOM_SHAPE[1]) / 2
    k[5] -= (240 - ROOM_SHAPE[0]) / 2
    return k


def room_poses():
    """(R [71, 3, 3], T [71, 3]): the four room_views() and 67 poses on a circle of 1 m (67 is a multiple of nothing in the launch)"""
    Rs, Ts = [], []
    for _, R, T in rv.room_views():
        Rs.append(np.asarray(R, np.float64).reshape(3, 3)); Ts.append(np.asarray(T, np.float64).reshape(3))
    for k in range(67):
        R, T = syn.camera_pose(k, orbit=1.0, deg_per_frame=360.0 / 67.0)
        Rs.append(np.asarray(R, np.float64).reshape(3, 3)); Ts.append(np.asarray(T, np.float64).reshape(3))
    return np.stack(Rs), np.stack(Ts)


def room_ref(e, N, Nz, K, R, T, cfg=SMALL, unknown_run=0):
    """the restatement of score_views(R, T, K=room_K(K), shape=ROOM_SHAPE, stride=ROOM_STRIDE) with the map's default range and step"""
    Kf = ref.scaled_K(room_K(K), ROOM_STRIDE)
    return ref.score_export(e, N, Nz, cfg["voxel_scale"], R, T, Kf, ROOM_SHAPE[0] // ROOM_STRIDE, ROOM_SHAPE[1] // ROOM_STRIDE,
                            np.float32(cfg["min_ray_length"]), np.float32(cfg["max_ray_length"]), unknown_run=unknown_run)
