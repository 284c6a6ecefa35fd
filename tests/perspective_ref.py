"""Projective warps (pyopenvino_amd.PerspectiveInput; pvhip_input_preprocess_perspective_f32) restated in numpy.  There is no other
implementation to compare with: this restatement of the rule IS the reference, and test_perspective_input.py checks it against facts
that do not depend on it (an affine matrix gives warp_ref's bits, a keystone with D = 2 copies every second pixel, the horizon column
is the pad, -H is H, the positions stay within a derived distance of float64 of the unquantised matrix).

`matrices[b]` maps an output pixel index (x, y) to the source position sx = (h00 x + h01 y + h02) / (h20 x + h21 y + h22),
sy = (h10 x + h11 y + h12) / (the same denominator), pixel centres at the integers (cv2.warpPerspective with WARP_INVERSE_MAP).

The table.  Row b is (id, Q00, Q01, Q02, Q10, Q11, Q12, Q20, Q21, Q22), int64: matrix b scaled by ONE power of two of its own -- the
ratio does not see it, so it is not stored.  Over an extent (hd, wd): B_r = |h_r0| (wd - 1) + |h_r1| (hd - 1) + |h_r2| for the three
rows r, B = max B_r in [2^(e-1), 2^e), Q = rint(float64(h) * 2^(51 - e)), ties to even; a non-finite entry or B == 0 is refused.  Then
|Q_r0| (wd - 1) + |Q_r1| (hd - 1) + |Q_r2| <= 2^52 for every r (the limit of a table as such): the three forms below are exact as int64
and as float64.

For output pixel (y, x):
    NX = Q00 x + Q01 y + Q02,  NY = Q10 x + Q11 y + Q12,  D = Q20 x + Q21 y + Q22      (int64)
    TX = floor(float64(NX) / float64(D) * 65536.0),  TY likewise                       (one correctly rounded division each)
    the pixel is `pad` in every channel unless D != 0 and |TX| < 2^47 and |TY| < 2^47  (NaN fails the compares); else
    SX = int64(TX),  SY = int64(TY)
and from there on warp_ref's rule word for word:
    ix = SX >> 16 (floor),  fx = float32(SX & 0xFFFF) * 2^-16 (exact);   iy, fy likewise
    P(r, c) = the pixel of frame id at (r, c) when 0 <= r < H and 0 <= c < W, else `pad` in every channel; colour frames are converted
              to uint8 B, G, R first (yuv_ref / packed_ref: the chroma of a pixel's block of the frame)
    top = fx == 0 ? P(iy, ix) : (1 - fx) P(iy, ix) + fx P(iy, ix + 1);   bot: the same on row iy + 1
    v   = fy == 0 ? top : (1 - fy) top + fy bot                          (float32, in that order)
then output channel k reads channel c-1-k under reversal, and (v - mean[k]) / std[k].  A row whose id is outside [0, m) is quiet NaN.  A
negative D is a denominator like any other."""
import math

import numpy as np

import packed_ref
import yuv_ref

FORM_LIMIT = 1 << 52
POSITION_LIMIT = 2.0 ** 47


def scale_exponent(matrix, dst_hw):
    """e of the rule above for one 3 x 3 matrix over (hd, wd): B in [2^(e-1), 2^e); ValueError for a non-finite entry or B == 0."""
    hd, wd = dst_hw
    rows = [[float(v) for v in row] for row in np.asarray(matrix, np.float64)]
    if not all(math.isfinite(v) for row in rows for v in row):
        raise ValueError('a non-finite entry')
    bound = max(abs(r[0]) * (wd - 1) + abs(r[1]) * (hd - 1) + abs(r[2]) for r in rows)
    if bound == 0 or not math.isfinite(bound):
        raise ValueError('B = {}'.format(bound))
    return math.frexp(bound)[1]


def fixed(matrices, dst_hw):
    """(n, 9) int64 (Q00 .. Q22) of (n, 3, 3) matrices over (hd, wd); ValueError naming the row."""
    m = np.asarray(matrices, np.float64)
    assert m.ndim == 3 and m.shape[1:] == (3, 3), m.shape
    out = np.empty((len(m), 9), np.int64)
    for b in range(len(m)):
        try:
            e = scale_exponent(m[b], dst_hw)
        except ValueError as err:
            raise ValueError('matrices[{}]: {}'.format(b, err)) from None
        out[b] = [int(round(math.ldexp(float(v), 51 - e))) for v in m[b].reshape(9)]       # round(): ties to even
    return out


def within_limit(q, dst_hw):
    """Every row of (n, 9) coefficients keeps its three forms <= 2^52 over (hd, wd) (Python ints)."""
    hd, wd = dst_hw
    return all(abs(row[r]) * (wd - 1) + abs(row[r + 1]) * (hd - 1) + abs(row[r + 2]) <= FORM_LIMIT
               for row in np.asarray(q).reshape(-1, 9).tolist() for r in (0, 3, 6))


def table_of(matrices, ids, dst_hw):
    """The (n, 10) int64 device table of matrices and frame ids."""
    q = fixed(matrices, dst_hw)
    return np.concatenate([np.asarray(ids, np.int64).reshape(-1, 1), q], 1)


def positions(coefficients, dst_hw):
    """(SX, SY, ok) over the extent for the nine ints of one row: int64 Q16 positions where `ok`, 0 elsewhere."""
    hd, wd = dst_hw
    q00, q01, q02, q10, q11, q12, q20, q21, q22 = (int(v) for v in coefficients)
    assert within_limit([coefficients], dst_hw)
    y, x = (g.astype(np.int64) for g in np.mgrid[0:hd, 0:wd])
    nx, ny, d = q00 * x + q01 * y + q02, q10 * x + q11 * y + q12, q20 * x + q21 * y + q22
    with np.errstate(divide='ignore', invalid='ignore'):
        tx = np.floor(nx.astype(np.float64) / d.astype(np.float64) * 65536.0)
        ty = np.floor(ny.astype(np.float64) / d.astype(np.float64) * 65536.0)
        ok = (d != 0) & (np.abs(tx) < POSITION_LIMIT) & (np.abs(ty) < POSITION_LIMIT)
    return np.where(ok, tx, 0.0).astype(np.int64), np.where(ok, ty, 0.0).astype(np.int64), ok


def images(frames, nhwc=True, color='RAW'):
    """The frames as (m, H, W, c) pixels: uint8 B, G, R for colour frames, the array's own values (uint8 or float32) else."""
    frames = np.asarray(frames)
    if color in ('NV12', 'I420'):
        return yuv_ref.to_bgr(frames, color)
    if color != 'RAW':
        return packed_ref.to_bgr(frames, color)
    return frames if nhwc else frames.transpose(0, 2, 3, 1)


def warp(frames, table, dst_hw, nhwc=True, reverse=False, mean=None, std=None, pad=0.0, color='RAW'):
    """fp32 NCHW (n, c, dst_h, dst_w) of the int64 (n, 10) `table` over `frames` in their host format."""
    img = images(frames, nhwc, color)
    m, H, W, c = img.shape
    table = np.asarray(table)
    assert table.dtype == np.int64 and table.ndim == 2 and table.shape[1] == 10, (table.dtype, table.shape)
    hd, wd = dst_hw
    pad = np.float32(pad)
    one, unit = np.float32(1), np.float32(2.0 ** -16)
    out = np.empty((len(table), c, hd, wd), np.float32)
    for b, row in enumerate(table.tolist()):
        i = row[0]
        if not 0 <= i < m:
            out[b] = np.float32(np.nan)
            continue
        sx, sy, ok = positions(row[1:], dst_hw)
        ix, iy, qx, qy = sx >> 16, sy >> 16, sx & 0xFFFF, sy & 0xFFFF
        fx, fy = qx.astype(np.float32) * unit, qy.astype(np.float32) * unit
        src = img[i]

        def P(r, col, k):
            inside = ok & (r >= 0) & (r < H) & (col >= 0) & (col < W)
            v = src[np.where(inside, r, 0), np.where(inside, col, 0), k].astype(np.float32)
            return np.where(inside, v, pad)

        for k in range(c):
            s = c - 1 - k if reverse else k
            with np.errstate(invalid='ignore', over='ignore'):
                top = np.where(qx == 0, P(iy, ix, s), (one - fx) * P(iy, ix, s) + fx * P(iy, ix + 1, s))
                bot = np.where(qx == 0, P(iy + 1, ix, s), (one - fx) * P(iy + 1, ix, s) + fx * P(iy + 1, ix + 1, s))
                v = np.where(qy == 0, top, (one - fy) * top + fy * bot)
                assert v.dtype == np.float32
                if mean is not None:
                    v = v - np.float32(mean[k])
                if std is not None:
                    v = v / np.float32(std[k])
            out[b, k] = v
    return out
