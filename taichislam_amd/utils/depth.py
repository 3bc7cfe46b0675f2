"""Tables and intrinsics for mapping.DepthConditioner (include/taichislam_hip.h, "depth conditioning").  The conditioner is defined over the INTEGERS it is
given; what is here only makes convenient integers."""
import numpy as np


def depth_tolerance(a=0.010, b=0.0, c=0.005):
    """tol uint16 [256]: clip(rint(1000 (a + b z + c z^2)), 1, 32767) millimetres at the centre z (metres) of each 256 mm depth bin -- how far two
    neighbouring pixels of one surface may differ.  The quadratic term is how a stereo or structured-light sensor's noise grows with range.  The defaults
    are a starting point; they were NOT measured on any sensor: fit a, b, c to the camera in use."""
    z = (256.0 * np.arange(256, dtype=np.float64) + 127.5) / 1000.0
    return np.clip(np.rint(1000.0 * (a + b * z + c * z * z)), 1, 32767).astype(np.uint16)


def bilateral_tables(radius, sigma_px=None, sigma_rel=0.5):
    """(ws uint8 [5, 5], wr uint8 [17]): Gaussians rounded and scaled to 255, computed in float64.  ws[|dy|, |dx|] = rint(255 exp(-(dy^2 + dx^2) / (2
    sigma_px^2))) inside `radius` and 0 beyond (sigma_px None = max(radius, 1) / 2 pixels); wr[q] = rint(255 exp(-(q / 16)^2 / (2 sigma_rel^2))), q / 16
    being the depth difference as a fraction of the tolerance.  These are convenience tables: the integers passed to the conditioner are the definition,
    and any other integers in range are as valid."""
    radius = int(radius)
    if not 0 <= radius <= 4:
        raise ValueError("bilateral_tables: radius must be 0 .. 4")
    s = float(max(radius, 1)) / 2.0 if sigma_px is None else float(sigma_px)
    if not (s > 0 and sigma_rel > 0):
        raise ValueError("bilateral_tables: the sigmas must be positive")
    i = np.arange(5, dtype=np.float64)
    ws = np.rint(255.0 * np.exp(-(i[:, None] ** 2 + i[None, :] ** 2) / (2.0 * s * s)))
    ws[i > radius, :] = 0
    ws[:, i > radius] = 0
    q = np.arange(17, dtype=np.float64) / 16.0
    wr = np.rint(255.0 * np.exp(-q * q / (2.0 * float(sigma_rel) ** 2)))
    return ws.astype(np.uint8), wr.astype(np.uint8)


def halved_intrinsics(K, level=1):
    """K of level `level` of the conditioner's pyramid, in the shape it came in (9 values or 3 x 3).  Per level fx and fy halve and c' = (c - 0.5) / 2: a
    pixel index is its centre in this library's unprojection, and halved pixel I covers source pixels 2 I and 2 I + 1, whose common centre is 2 I + 0.5."""
    K = np.array(K, dtype=np.float64)
    k = K.reshape(-1).copy()
    for _ in range(int(level)):
        k[0], k[4] = k[0] / 2.0, k[4] / 2.0
        k[2], k[5] = (k[2] - 0.5) / 2.0, (k[5] - 0.5) / 2.0
    return k.reshape(K.shape)
