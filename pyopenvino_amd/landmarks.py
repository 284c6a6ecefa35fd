"""The rule of ``LandmarkWarps`` on the host: a landmark network's points become the (n, 7) table of a ``WarpInput`` -- for Results that
were computed or read on the host, as ``detections.compact_records`` serves a detector's.  It is the rule of pvhip_landmarks_to_warps
(include/pvhip.h states it, tests/landmark_warps_ref.py restates it in numpy), bit for bit, in plain Python floats: binary64, every
operation rounded once, in the order written, nothing contracted -- and no ``np.sum``, whose pairwise summation is another order.

Host side, once per template: `template` is (K, 2) real numbers, 2 <= K <= 32; point i is the place (x, y) landmark i shall land at, in
output pixel indices of the consumer's extent, pixel centres at the integers.
  tbx = (t_0x + t_1x + ...) / K in index order, tby likewise;  cx_i = t_ix - tbx,  cy_i = t_iy - tby;
  S = sum over i of (cx_i cx_i + cy_i cy_i), in index order, starting from term 0;
  ValueError for a value that is not finite, |t| > 2^24 or S == 0;  ``packed_template`` = (tbx, tby, S, cx_0, cy_0, ...), 2 K + 3 doubles.
Row b: `points` is fp32 (N, 2 K) as x0, y0, x1, y1, ..., normalised to the row's region on pixel-edge coordinates -- 0 the region's
left or top edge, 1 its right or bottom edge --, region b = (id, x, y, w, h).
  The row is void when b >= N, id is outside [0, m), w or h is outside [1, 2^24], or one of its 2 K values is not finite.  Else
  px_i = (float(x) + float(u_i) float(w)) - 0.5,  py_i likewise with y and h;   mx = (px_0 + px_1 + ...) / K,  my likewise;
  dx_i = px_i - mx,  dy_i = py_i - my;   A = sum of (cx_i dx_i + cy_i dy_i),  B = sum of (cx_i dy_i - cy_i dx_i), each term formed first
  and then added, in index order;   a = A / S,  b = B / S;   c0 = mx - (a tbx - b tby),  c1 = my - (b tbx + a tby).
  The matrix [[a, -b, c0], [b, a, c1]] is the least-squares similarity, without reflection, from the template's points to the landmarks'
  positions: directly the inverse map a warp takes.  It is NOT ``warp.invert(cv2.estimateAffinePartial2D(landmarks -> template))``, which
  minimises in the other space; the two agree where the fit is exact.
  Q16: rint(v 65536), ties to even, for the six values (A01 = rint(-b 65536)).  The row is void as well when one of the six is not
  finite, when one breaks ``WarpInput``'s limits (|A| <= 2^26, |C| <= 2^40), or when A00 == 0 and A10 == 0 (every point in one place).
  A valid row is (id, A00, A01, C0, A10, A11, C1), a void one (-1, 0, 0, 0, 0, 0, 0).
Host arithmetic only: nothing here touches the device."""
import math

import numpy as np

MIN_POINTS, MAX_POINTS = 2, 32
EXTENT_LIMIT = 1 << 24             # w, h of a region at most; |t| of a template value at most
LINEAR_LIMIT = 1 << 26             # WarpInput.LINEAR_LIMIT
TRANSLATION_LIMIT = 1 << 40        # WarpInput.TRANSLATION_LIMIT
VOID = (-1, 0, 0, 0, 0, 0, 0)


def _template_points(template):
    t = np.asarray(template)
    if t.ndim != 2 or t.shape[1] != 2 or not MIN_POINTS <= t.shape[0] <= MAX_POINTS:
        raise ValueError('template has shape (K, 2) -- the place (x, y) of each of {} <= K <= {} landmarks --, got {}'.format(
            MIN_POINTS, MAX_POINTS, t.shape))
    if t.dtype.kind not in 'fiu':
        raise ValueError('template holds real numbers, got dtype {}'.format(t.dtype))
    return [(float(x), float(y)) for x, y in t.astype(np.float64).tolist()]


def _packed(template):
    """(tbx, tby, S, [(cx_i, cy_i)]) of a template, in Python floats."""
    pts = _template_points(template)
    K = len(pts)
    if any(not math.isfinite(v) or abs(v) > EXTENT_LIMIT for p in pts for v in p):
        raise ValueError('template holds finite values with |t| <= 2^24, got {}'.format(pts))
    sx, sy = pts[0]
    for x, y in pts[1:]:
        sx, sy = sx + x, sy + y
    tbx, tby = sx / K, sy / K
    c = [(x - tbx, y - tby) for x, y in pts]
    S = c[0][0] * c[0][0] + c[0][1] * c[0][1]
    for cx, cy in c[1:]:
        S = S + (cx * cx + cy * cy)
    if S == 0:
        raise ValueError('template holds at least two different points, got {}'.format(pts))
    return tbx, tby, S, c


def packed_template(template) -> np.ndarray:
    """The 2 K + 3 doubles (tbx, tby, S, cx_0, cy_0, cx_1, cy_1, ...) the device takes for `template`; ValueError for a template that is
    not (K, 2) real numbers with 2 <= K <= 32, holds a value that is not finite or beyond 2^24, or whose points all coincide."""
    tbx, tby, S, c = _packed(template)
    return np.array([tbx, tby, S] + [v for p in c for v in p], np.float64)


def _matrix(tbx, tby, S, c, px, py):
    """(a, b, c0, c1) of the rule from frame-pixel positions, Python floats."""
    K = len(c)
    sx, sy = px[0], py[0]
    for i in range(1, K):
        sx, sy = sx + px[i], sy + py[i]
    mx, my = sx / K, sy / K
    A = B = 0.0
    for i in range(K):
        (cx, cy), dx, dy = c[i], px[i] - mx, py[i] - my
        ta, tb = cx * dx + cy * dy, cx * dy - cy * dx
        A, B = (ta, tb) if i == 0 else (A + ta, B + tb)
    a, b = A / S, B / S
    return a, b, mx - (a * tbx - b * tby), my - (b * tbx + a * tby)


def similarity(points_xy, template) -> np.ndarray:
    """The float64 (2, 3) matrix [[a, -b, c0], [b, a, c1]] of the rule for K landmarks `points_xy` (K, 2) given in FRAME pixels (centres at
    the integers): the least-squares similarity, without reflection, that takes each template point to its landmark -- the matrix a
    ``WarpInput`` takes.  ValueError for points of another shape than the template's or that are not finite."""
    tbx, tby, S, c = _packed(template)
    p = np.asarray(points_xy)
    if p.shape != (len(c), 2) or p.dtype.kind not in 'fiu':
        raise ValueError('points_xy holds {} points (x, y) as real numbers, one per template point; got {} {}'.format(len(c), p.dtype, p.shape))
    xy = p.astype(np.float64).tolist()
    if any(not math.isfinite(v) for q in xy for v in q):
        raise ValueError('points_xy holds finite values, got {}'.format(xy))
    a, b, c0, c1 = _matrix(tbx, tby, S, c, [float(q[0]) for q in xy], [float(q[1]) for q in xy])
    return np.array([[a, -b, c0], [b, a, c1]], np.float64)


def _row(tbx, tby, S, c, u, region, m):
    """The table row of the rule for the 2 K fp32 values `u` of one row and its region (id, x, y, w, h), or None: void."""
    i, x, y, w, h = region
    if not (0 <= i < m and 1 <= w <= EXTENT_LIMIT and 1 <= h <= EXTENT_LIMIT):
        return None
    if any(not math.isfinite(v) for v in u):
        return None
    K = len(c)
    xd, yd, wd, hd = float(x), float(y), float(w), float(h)
    px = [(xd + u[2 * k] * wd) - 0.5 for k in range(K)]
    py = [(yd + u[2 * k + 1] * hd) - 0.5 for k in range(K)]
    a, b, c0, c1 = _matrix(tbx, tby, S, c, px, py)
    q = [a * 65536.0, -b * 65536.0, c0 * 65536.0, b * 65536.0, a * 65536.0, c1 * 65536.0]
    if any(not math.isfinite(v) for v in q):
        return None
    r = [round(v) for v in q]                   # (ties to even)
    if any(abs(r[j]) > (TRANSLATION_LIMIT if j in (2, 5) else LINEAR_LIMIT) for j in range(6)):
        return None
    if r[0] == 0 and r[3] == 0:
        return None
    return (int(i),) + tuple(r)


def to_warps(points, regions, template, frame_hw, frames, rows=None):
    """(table, valid): the (rows, 7) int64 table of the rule and which of its rows are valid, (rows,) bool, for float32 `points` of
    shape (N, 2 K) or (N, 2 K, 1, 1) -- a landmark network's Result --, `regions` the integer (N, 5) table (id, x, y, w, h) its pass was
    fed, or None: the whole frame, (0 if frames == 1 else b, 0, 0, w, h) of `frame_hw` = (h, w); `frames` = m, the frame count the ids
    are checked against; `rows` = n, the batch of the consumer (default N): rows behind N are void.
    ``WarpInput(frames, warp_buffer)`` with the table in the request's ``warp_buffer`` takes valid rows as they are; a void row's id of
    -1 has to be replaced first (a WarpInput refuses it on the host; only the device writes it as quiet NaN)."""
    tbx, tby, S, c = _packed(template)
    K = len(c)
    p = np.asarray(points)
    if p.dtype != np.float32 or p.ndim not in (2, 4) or p.shape[0] < 1 or p.shape[1] != 2 * K or tuple(p.shape[2:]) not in ((), (1, 1)):
        raise ValueError('points are float32 of shape (N, {0}) or (N, {0}, 1, 1) for a template of {1} points, got {2} {3}'.format(
            2 * K, K, p.dtype.name, tuple(p.shape)))
    N = p.shape[0]
    u = p.reshape(N, 2 * K).astype(np.float64).tolist()      # (exact: every float32 is a float)
    H, W = (int(v) for v in frame_hw)
    m = int(frames)
    if regions is not None:
        t = np.asarray(regions)
        if t.shape != (N, 5) or t.dtype.kind not in 'iu':
            raise ValueError('regions is an integer table of shape {} -- one (id, x, y, w, h) per row of points --, got {} {}'.format(
                (N, 5), t.dtype, t.shape))
        table_of = t.tolist()
    n = N if rows is None else int(rows)
    table, valid = np.empty((n, 7), np.int64), np.zeros(n, bool)
    for b in range(n):
        row = None
        if b < N:
            region = table_of[b] if regions is not None else (0 if m == 1 else b, 0, 0, W, H)
            row = _row(tbx, tby, S, c, u[b], region, m)
        table[b], valid[b] = (row, True) if row is not None else (VOID, False)
    return table, valid
