"""Matrices for ``WarpInput``: 2 x 3 affine maps in float64 from an OUTPUT pixel index (x, y) of the network's extent to a SOURCE
position in frame pixels, sx = a00 x + a01 y + c0, sy = a10 x + a11 y + c1, pixel centres at the integers -- what
``cv2.warpAffine(..., flags=INTER_LINEAR | WARP_INVERSE_MAP)`` takes.  Host arithmetic only: nothing here touches the device."""
import numpy as np


def _matrix(m, what='matrix'):
    a = np.asarray(m, np.float64)
    if a.shape != (2, 3):
        raise ValueError('{} is a 2 x 3 affine matrix, got shape {}'.format(what, a.shape))
    return a


def invert(forward) -> np.ndarray:
    """The 2 x 3 inverse of a forward matrix -- source (x, y) to output position, what ``cv2.getAffineTransform`` and
    ``cv2.estimateAffinePartial2D`` return --: the matrix a WarpInput takes.  ValueError for a singular or non-finite one."""
    f = _matrix(forward, 'forward')
    (a, b, tx), (c, d, ty) = f
    det = a * d - b * c
    if not np.isfinite(f).all() or det == 0 or not np.isfinite(1.0 / det):
        raise ValueError('forward matrix {} is singular'.format(f.tolist()))
    ia, ib, ic, id_ = d / det, -b / det, -c / det, a / det
    return np.array([[ia, ib, -(ia * tx + ib * ty)], [ic, id_, -(ic * tx + id_ * ty)]], np.float64)


def _extents(rect_wh, dst_hw):
    (w, h), (H, W) = (float(v) for v in rect_wh), (int(v) for v in dst_hw)
    if not (w > 0 and h > 0 and H >= 1 and W >= 1):
        raise ValueError('a rectangle of (w, h) = {} onto an extent (h, w) = {}: every size is > 0'.format((w, h), (H, W)))
    return w, h, H, W


def from_roi(roi, dst_hw) -> np.ndarray:
    """The crop-and-resize of the rectangle `roi` = (x, y, w, h) onto `dst_hw` = (H, W) with half-pixel centres, as a matrix:
    a00 = w / W, c0 = x + a00 / 2 - 1/2, and likewise down the other axis.  A rectangle of the network's extent is the integer
    translation (a copy).  At other scales this is NOT bit for bit a RoiInput: its taps clamp at the rectangle's edge and its fractions
    are exact rationals; a warp reads on into the frame, pads outside it and has Q16 coefficients."""
    x, y = float(roi[0]), float(roi[1])
    w, h, H, W = _extents(roi[2:4], dst_hw)
    sx, sy = w / W, h / H
    return np.array([[sx, 0.0, x + sx / 2 - 0.5], [0.0, sy, y + sy / 2 - 0.5]], np.float64)


def rotated_rect(cx, cy, w, h, angle_deg, dst_hw) -> np.ndarray:
    """The same for the w x h rectangle centred at (cx, cy) -- pixel-edge coordinates, as from_roi's x + w / 2 -- and turned by
    `angle_deg` about its centre (positive: the rectangle's x axis turns towards the frame's +y, clockwise on the screen): an oriented
    detector's box, a plate along its own axis.  Angle 0 equals ``from_roi((cx - w / 2, cy - h / 2, w, h), dst_hw)``."""
    w, h, H, W = _extents((w, h), dst_hw)
    sx, sy = w / W, h / H
    t = np.deg2rad(float(angle_deg))
    cos, sin = (1.0, 0.0) if angle_deg == 0 else (float(np.cos(t)), float(np.sin(t)))
    # output pixel centre (x + 1/2, y + 1/2) -> rectangle coordinates about its centre -> turned -> frame, centres at the integers;
    # the turned corner first and the half step behind it, so that angle 0 is from_roi's expression term by term
    x0, y0 = float(cx) - cos * w / 2 + sin * h / 2, float(cy) - sin * w / 2 - cos * h / 2
    return np.array([[cos * sx, -sin * sy, x0 + (cos * sx / 2 - sin * sy / 2) - 0.5],
                     [sin * sx, cos * sy, y0 + (sin * sx / 2 + cos * sy / 2) - 0.5]], np.float64)


def apply(matrix, xy) -> np.ndarray:
    """Network-pixel points `xy` (..., 2) as (x, y) -- box corners, landmarks -- mapped to frame positions by `matrix`, float64."""
    m = _matrix(matrix)
    p = np.asarray(xy, np.float64)
    if p.shape[-1:] != (2,):
        raise ValueError('points are (..., 2) arrays of (x, y), got shape {}'.format(p.shape))
    return p @ m[:, :2].T + m[:, 2]
