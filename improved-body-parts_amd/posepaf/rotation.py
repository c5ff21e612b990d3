"""Test-time rotation search (utils/parse_skeletons.py:214-218, :265-267, :98-100): the host half.

The reference rotates the padded input with cv2.warpAffine(img, getRotationMatrix2D(center, angle, 1), (0, 0)) and rotates
the up-sampled maps back with the matrix of -angle.  Both matrices, and the inversion warpAffine applies to them before it
samples (no WARP_INVERSE_MAP), are computed here in double precision with the same operations as OpenCV 3.4
(imgwarp.cpp): math.cos / math.sin are glibc's, and CPython rounds every product and sum separately.  The kernels receive
the six inverted doubles and do the fixed-point sampling themselves (k_preprocess_affine, k_warp_affine_f32, the warped
instance of k_accumulate_scales).

Quirk kept: the reference passes the centre as (x, y) = (H / 2, W / 2) -- height and width swapped -- so on a non-square
input the rotation is not about the image centre (reference_center)."""
from __future__ import annotations

import math

import numpy as np


def reference_center(hp: int, wp: int):
    """(cx, cy) the reference passes to getRotationMatrix2D for an input of shape (hp, wp): (hp / 2, wp / 2), swapped, as the
    Point2f OpenCV converts it to (rounded to float32, then widened again)."""
    return float(np.float32(hp / 2)), float(np.float32(wp / 2))


def rotation_matrix(center_xy, angle: float):
    """cv2.getRotationMatrix2D(center, angle, 1.0): 2x3 float64, angle in degrees, counter-clockwise as displayed."""
    cx, cy = (float(np.float32(v)) for v in center_xy)
    a = float(angle) * (math.pi / 180)
    alpha, beta = math.cos(a), math.sin(a)
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy],
                     [-beta, alpha, beta * cx + (1 - alpha) * cy]], dtype=np.float64)


def invert_affine(m):
    """The inversion cv2.warpAffine applies to M without WARP_INVERSE_MAP: -> the 6 doubles (row-major) the kernels sample with
    (dst (x, y) reads src (M0 x + M1 y + M2, M3 x + M4 y + M5))."""
    M = [float(v) for v in np.asarray(m, np.float64).reshape(6)]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11 = M[4] * D
    A22 = M[0] * D
    M[0] = A11
    M[1] *= -D
    M[3] *= -D
    M[4] = A22
    b1 = -M[0] * M[2] - M[1] * M[5]
    b2 = -M[3] * M[2] - M[4] * M[5]
    M[2] = b1
    M[5] = b2
    return np.array(M, dtype=np.float64).reshape(2, 3)


def input_and_map_inverses(hp: int, wp: int, angle: float):
    """predict's two warps of one (scale, angle) entry at padded input shape (hp, wp): -> (inverse of M, applied to the input
    image; inverse of M_rev, applied to the x4 maps of the same shape).  (None, None) for angle 0, which the reference does not
    warp at all."""
    if float(angle) == 0.0:
        return None, None
    c = reference_center(hp, wp)
    return invert_affine(rotation_matrix(c, angle)), invert_affine(rotation_matrix(c, -float(angle)))


def apply_affine(m, xy):
    """points (..., 2) [x, y] through a 2x3 matrix, float64"""
    m = np.asarray(m, np.float64).reshape(2, 3)
    xy = np.asarray(xy, np.float64)
    return np.stack([m[0, 0] * xy[..., 0] + m[0, 1] * xy[..., 1] + m[0, 2],
                     m[1, 0] * xy[..., 0] + m[1, 1] * xy[..., 1] + m[1, 2]], axis=-1)


def as_c_doubles(m_inv):
    """6 host doubles for the C ABI (None stays None)"""
    if m_inv is None:
        return None
    import ctypes as C
    return (C.c_double * 6)(*[float(v) for v in np.asarray(m_inv, np.float64).reshape(6)])
