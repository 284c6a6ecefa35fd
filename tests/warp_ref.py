"""Affine warps (pyopenvino_amd.WarpInput; pvhip_input_preprocess_warp_f32) restated in numpy.  There is no other implementation to compare
with: this restatement of the rule IS the reference, and test_warp_input.py checks it against facts that do not depend on it (an integer
translation is a slice, a mirror a reversed slice, a half fraction the mean of two bytes, the pad where taps leave the frame).

Row b of the table is (id, A00, A01, C0, A10, A11, C1), int64, the coefficients in Q16.  For output pixel (y, x):
    SX = A00 x + A01 y + C0,  SY = A10 x + A11 y + C1                    (int64)
    ix = SX >> 16 (floor),  fx = float32(SX & 0xFFFF) * 2^-16 (exact);   iy, fy likewise
    P(r, c) = the pixel of frame id at (r, c) when 0 <= r < H and 0 <= c < W, else `pad` in every channel; colour frames are converted
              to uint8 B, G, R first (yuv_ref / packed_ref: the chroma of a pixel's block of the frame)
    top = fx == 0 ? P(iy, ix) : (1 - fx) P(iy, ix) + fx P(iy, ix + 1);   bot: the same on row iy + 1
    v   = fy == 0 ? top : (1 - fy) top + fy bot                          (float32, in that order)
then output channel k reads channel c-1-k under reversal, and (v - mean[k]) / std[k].  A row whose id is outside [0, m) is quiet NaN."""
import numpy as np

import packed_ref
import yuv_ref

LINEAR_LIMIT, TRANSLATION_LIMIT = 1 << 26, 1 << 40


def fixed(matrices):
    """(n, 6) int64 (A00, A01, C0, A10, A11, C1): rint(float64(v) * 65536), ties to even; ValueError beyond the limits."""
    m = np.asarray(matrices, np.float64)
    assert m.ndim == 3 and m.shape[1:] == (2, 3), m.shape
    out = np.empty((len(m), 6), np.int64)
    for b in range(len(m)):
        for j, v in enumerate(m[b].reshape(6)):
            limit = TRANSLATION_LIMIT if j in (2, 5) else LINEAR_LIMIT
            if not np.isfinite(v) or abs(np.rint(v * 65536.0)) > limit:
                raise ValueError('matrices[{}]: coefficient {} = {!r}'.format(b, j, float(v)))
            out[b, j] = int(np.rint(v * 65536.0))
    return out


def table_of(matrices, ids):
    """The (n, 7) int64 device table of matrices and frame ids."""
    q = fixed(matrices)
    return np.concatenate([np.asarray(ids, np.int64).reshape(-1, 1), q], 1)


def images(frames, nhwc=True, color='RAW'):
    """The frames as (m, H, W, c) pixels: uint8 B, G, R for colour frames, the array's own values (uint8 or float32) else."""
    frames = np.asarray(frames)
    if color in ('NV12', 'I420'):
        return yuv_ref.to_bgr(frames, color)
    if color != 'RAW':
        return packed_ref.to_bgr(frames, color)
    return frames if nhwc else frames.transpose(0, 2, 3, 1)


def warp(frames, table, dst_hw, nhwc=True, reverse=False, mean=None, std=None, pad=0.0, color='RAW'):
    """fp32 NCHW (n, c, dst_h, dst_w) of the int64 (n, 7) `table` over `frames` in their host format."""
    img = images(frames, nhwc, color)
    m, H, W, c = img.shape
    table = np.asarray(table)
    assert table.dtype == np.int64 and table.ndim == 2 and table.shape[1] == 7, (table.dtype, table.shape)
    hd, wd = dst_hw
    pad = np.float32(pad)
    one, unit = np.float32(1), np.float32(2.0 ** -16)
    out = np.empty((len(table), c, hd, wd), np.float32)
    y, x = (g.astype(np.int64) for g in np.mgrid[0:hd, 0:wd])
    for b, (i, a00, a01, c0, a10, a11, c1) in enumerate(table.tolist()):
        if not 0 <= i < m:
            out[b] = np.float32(np.nan)
            continue
        sx, sy = a00 * x + a01 * y + c0, a10 * x + a11 * y + c1
        ix, iy, qx, qy = sx >> 16, sy >> 16, sx & 0xFFFF, sy & 0xFFFF
        fx, fy = qx.astype(np.float32) * unit, qy.astype(np.float32) * unit
        src = img[i]

        def P(r, col, k):
            inside = (r >= 0) & (r < H) & (col >= 0) & (col < W)
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
