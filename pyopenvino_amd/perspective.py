"""Matrices for ``PerspectiveInput``: 3 x 3 homographies in float64 from an OUTPUT pixel index (x, y) of the network's extent to a SOURCE
position in frame pixels, sx = (h00 x + h01 y + h02) / (h20 x + h21 y + h22), sy = (h10 x + h11 y + h12) / (the same denominator), pixel
centres at the integers -- what ``cv2.warpPerspective(..., flags=INTER_LINEAR | WARP_INVERSE_MAP)`` takes.  A homography is defined up
to a factor: H and k H are the same map for any k != 0.  Host arithmetic only: nothing here touches the device."""
import numpy as np


def _matrix(m, what='matrix'):
    a = np.asarray(m, np.float64)
    if a.shape != (3, 3):
        raise ValueError('{} is a 3 x 3 homography, got shape {}'.format(what, a.shape))
    return a


def from_affine(matrix) -> np.ndarray:
    """The 2 x 3 affine matrix of a WarpInput (pyopenvino_amd.warp) as a homography: [[A], [0, 0, 1]]."""
    a = np.asarray(matrix, np.float64)
    if a.shape != (2, 3):
        raise ValueError('matrix is a 2 x 3 affine matrix, got shape {}'.format(a.shape))
    return np.concatenate([a, [[0.0, 0.0, 1.0]]], 0)


def from_quad(corners, dst_hw) -> np.ndarray:
    """The homography that maps the corner pixel centres of an output of `dst_hw` = (H, W) -- (0, 0), (W - 1, 0), (W - 1, H - 1),
    (0, H - 1) -- onto the four frame points `corners` = [(x, y)] * 4, given in that order: top-left, top-right, bottom-right,
    bottom-left OF THE OUTPUT (what ``cv2.getPerspectiveTransform(output corners, corners)`` returns): the matrix a PerspectiveInput
    takes, with h22 = 1.  ValueError for a degenerate quadrilateral (three points on a line, or an extent of one pixel along an
    axis) or a non-finite point."""
    q = np.asarray(corners, np.float64)
    H, W = (int(v) for v in dst_hw)
    if q.shape != (4, 2):
        raise ValueError('corners are four (x, y) points, got shape {}'.format(q.shape))
    out = np.array([[0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1]], np.float64)
    # sx (h20 x + h21 y + 1) = h00 x + h01 y + h02, and the same for sy: eight equations in h00 .. h21
    system, rhs = np.zeros((8, 8)), np.zeros(8)
    for k, ((x, y), (sx, sy)) in enumerate(zip(out, q)):
        system[2 * k] = [x, y, 1, 0, 0, 0, -sx * x, -sx * y]
        system[2 * k + 1] = [0, 0, 0, x, y, 1, -sy * x, -sy * y]
        rhs[2 * k], rhs[2 * k + 1] = sx, sy
    degenerate = ValueError('corners {} onto an extent (h, w) = {}: a degenerate quadrilateral'.format(q.tolist(), (H, W)))
    if not np.isfinite(q).all() or H < 2 or W < 2:
        raise degenerate
    try:
        h = np.linalg.solve(system, rhs)
    except np.linalg.LinAlgError:
        raise degenerate from None
    m = np.append(h, 1.0).reshape(3, 3)
    # a numerically singular system solves to something: the four corners have to come back, and the map has to be invertible
    back = apply(m, out) if np.isfinite(m).all() else np.full((4, 2), np.nan)
    if not (np.abs(back - q) <= 1e-6 * (1.0 + np.abs(q))).all() or abs(np.linalg.det(m / np.abs(m).max())) < 1e-12:
        raise degenerate
    return m


def invert(forward) -> np.ndarray:
    """The inverse of a forward homography -- source (x, y) to output position, what ``cv2.getPerspectiveTransform`` and
    ``cv2.findHomography`` return --: the matrix a PerspectiveInput takes.  ValueError for a singular or non-finite one."""
    f = _matrix(forward, 'forward')
    singular = ValueError('forward matrix {} is singular'.format(f.tolist()))
    if not np.isfinite(f).all() or not f.any():
        raise singular
    g = f / np.abs(f).max()                                   # (the factor is free: a determinant that means something)
    if abs(np.linalg.det(g)) < 1e-15:
        raise singular
    inv = np.linalg.inv(g)
    if not np.isfinite(inv).all():
        raise singular
    return inv


def apply(matrix, xy) -> np.ndarray:
    """Network-pixel points `xy` (..., 2) as (x, y) -- box corners, landmarks -- mapped to frame positions by `matrix`, with the
    division, float64; NaN where the denominator is 0."""
    m = _matrix(matrix)
    p = np.asarray(xy, np.float64)
    if p.shape[-1:] != (2,):
        raise ValueError('points are (..., 2) arrays of (x, y), got shape {}'.format(p.shape))
    num = p @ m[:2, :2].T + m[:2, 2]
    den = p @ m[2, :2] + m[2, 2]
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where((den == 0)[..., None], np.nan, num / den[..., None])
