"""The rule of pyopenvino_amd.LandmarkWarps (pvhip_landmarks_to_warps) in numpy: a landmark network's points become the (n, 7) table of a
WarpInput.  This is the specification; the kernel and pyopenvino_amd/landmarks.py equal it bit for bit.

All of it is binary64 -- numpy's elementwise float64 operations, over all rows at once and serially over the K points --, every
operation rounded once, in the order written; no np.sum (pairwise summation is another order).

Host side, once per template: `template` is (K, 2) real numbers, 2 <= K <= 32; point i is the place (x, y) landmark i shall land at, in
output pixel indices, pixel centres at the integers.
  tbx = (t_0x + t_1x + ...) / K in index order, tby likewise;  cx_i = t_ix - tbx,  cy_i = t_iy - tby;
  S = sum over i of (cx_i cx_i + cy_i cy_i) in index order, starting from term 0;
  refused: a value that is not finite, |t| > 2^24, S == 0;  packed = (tbx, tby, S, cx_0, cy_0, ...), 2 K + 3 doubles.
Row b: `points` is fp32 (N, 2 K) as x0, y0, x1, y1, ..., normalised to the region (id, x, y, w, h) of the row on pixel-edge coordinates
(0: the region's left or top edge, 1: its right or bottom edge).
  void      b >= N, id outside [0, m), w or h outside [1, 2^24], one of the 2 K values not finite;
  px_i = (double(x) + double(u_i) double(w)) - 0.5,  py_i likewise with y and h;   mx = (px_0 + px_1 + ...) / K,  my likewise;
  dx_i = px_i - mx,  dy_i = py_i - my;   A = sum of (cx_i dx_i + cy_i dy_i),  B = sum of (cx_i dy_i - cy_i dx_i), each term formed first and
  then added, in index order;   a = A / S,  b = B / S;   c0 = mx - (a tbx - b tby),  c1 = my - (b tbx + a tby);
  the matrix is [[a, -b, c0], [b, a, c1]]; Q16 = rint(v 65536), ties to even, A01 = rint(-b 65536);
  void too  one of the six not finite, |A| > 2^26, |C| > 2^40, A00 == 0 and A10 == 0;
  a valid row is (id, A00, A01, C0, A10, A11, C1), a void one (-1, 0, 0, 0, 0, 0, 0); count = the number of valid rows."""
import collections

import numpy as np

Fitted = collections.namedtuple('Fitted', 'count valid table')
LIMIT = 1 << 24


def packed(template):
    t = np.asarray(template, np.float64)
    assert t.ndim == 2 and t.shape[1] == 2 and 2 <= t.shape[0] <= 32
    if not np.isfinite(t).all() or (np.abs(t) > LIMIT).any():
        raise ValueError('template')
    K = t.shape[0]
    s = t[0].copy()
    for i in range(1, K):
        s = s + t[i]
    tb = s / np.float64(K)
    c = t - tb
    S = c[0, 0] * c[0, 0] + c[0, 1] * c[0, 1]
    for i in range(1, K):
        S = S + (c[i, 0] * c[i, 0] + c[i, 1] * c[i, 1])
    if S == 0:
        raise ValueError('template')
    return np.concatenate([tb, [S], c.reshape(-1)]).astype(np.float64)


def whole_frames(N, frame_hw, m):
    """The regions of rows that saw whole frames: (0 if m == 1 else b, 0, 0, w, h)."""
    H, W = frame_hw
    return np.array([(0 if m == 1 else b, 0, 0, W, H) for b in range(N)], np.int64).reshape(N, 5)


def landmark_warps(points, regions, template, frame_hw, m, n=None):
    """Fitted(count, valid (n,) bool, table (n, 7) int64) of float32 `points` (N, 2 K) [or (N, 2 K, 1, 1)] and integer `regions` (N, 5),
    or None: whole frames of `frame_hw` = (h, w); `m` frames; `n` rows of the table (default N)."""
    p = np.asarray(points)
    assert p.dtype == np.float32
    N = p.shape[0]
    p = p.reshape(N, -1)
    t = packed(template)
    K = (len(t) - 3) // 2
    assert p.shape[1] == 2 * K
    tbx, tby, S, cx, cy = t[0], t[1], t[2], t[3::2], t[4::2]
    n = N if n is None else n
    r = np.asarray(whole_frames(N, frame_hw, m) if regions is None else regions).astype(np.int64).reshape(N, 5)
    rows = min(n, N)
    u, r = p[:rows].astype(np.float64), r[:rows]
    table = np.zeros((n, 7), np.int64)
    table[:, 0] = -1
    valid = np.zeros(n, bool)
    i, x, y, w, h = r.T
    ok = (i >= 0) & (i < m) & (w >= 1) & (w <= LIMIT) & (h >= 1) & (h <= LIMIT) & np.isfinite(u).all(1)
    with np.errstate(all='ignore'):
        xd, yd, wd, hd = (v.astype(np.float64) for v in (x, y, w, h))
        px = [(xd + u[:, 2 * k] * wd) - 0.5 for k in range(K)]
        py = [(yd + u[:, 2 * k + 1] * hd) - 0.5 for k in range(K)]
        sx, sy = px[0], py[0]
        for k in range(1, K):
            sx, sy = sx + px[k], sy + py[k]
        mx, my = sx / np.float64(K), sy / np.float64(K)
        A = B = None
        for k in range(K):
            dx, dy = px[k] - mx, py[k] - my
            ta, tb = cx[k] * dx + cy[k] * dy, cx[k] * dy - cy[k] * dx
            A, B = (ta, tb) if k == 0 else (A + ta, B + tb)
        a, b = A / S, B / S
        c0, c1 = mx - (a * tbx - b * tby), my - (b * tbx + a * tby)
        q = np.stack([a * 65536.0, -b * 65536.0, c0 * 65536.0, b * 65536.0, a * 65536.0, c1 * 65536.0], 1)
        ok &= np.isfinite(q).all(1)
        q = np.rint(np.where(ok[:, None], q, 0.0))
    ok &= (np.abs(q[:, [0, 1, 3, 4]]) <= 2.0 ** 26).all(1) & (np.abs(q[:, [2, 5]]) <= 2.0 ** 40).all(1)
    ok &= ~((q[:, 0] == 0) & (q[:, 3] == 0))
    table[:rows][ok, 0] = i[ok]
    table[:rows][ok, 1:] = q[ok].astype(np.int64)
    valid[:rows] = ok
    return Fitted(int(valid.sum()), valid, table)


def points_for(matrix, template, region):
    """The normalised fp32 points (2 K,) whose frame positions are `matrix` applied to the template's points, over `region` =
    (id, x, y, w, h): exact when every value involved is a dyadic fraction of few bits."""
    m, t = np.asarray(matrix, np.float64), np.asarray(template, np.float64)
    _, x, y, w, h = region
    pos = t @ m[:, :2].T + m[:, 2]
    u = np.stack([(pos[:, 0] + 0.5 - x) / w, (pos[:, 1] + 0.5 - y) / h], 1).reshape(-1)
    assert np.array_equal(np.float32(u).astype(np.float64), u)
    return np.float32(u)
