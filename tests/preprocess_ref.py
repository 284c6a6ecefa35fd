"""The input preprocessing of IENetwork.input_info[name].preprocess_info restated in numpy: what pvhip_input_preprocess_f32 computes,
bit for bit.  Bilinear resize with half-pixel centres clamped at the border and no antialiasing (cv2 INTER_LINEAR, torch interpolate
bilinear with align_corners=False), its coordinates exact in integers; then channel reversal and per-channel mean / scale, all in fp32
with every operation rounded on its own (numpy never contracts a multiply and an add)."""
import numpy as np


def taps(S, D):
    """(i0, i1, f) of every destination index along an axis of source extent S and destination extent D: the source coordinate is
    num / (2D), num = max((2d+1)S - D, 0); f is one correctly rounded fp32 division, 0 at the last source index."""
    d = np.arange(D, dtype=np.int64)
    num = np.maximum((2 * d + 1) * S - D, 0)
    i0 = np.minimum(num // (2 * D), S - 1)
    i1 = np.minimum(i0 + 1, S - 1)
    f = (num - i0 * 2 * D).astype(np.float32) / np.float32(2 * D)
    return i0, i1, np.where(i0 == S - 1, np.float32(0), f).astype(np.float32)


def resize_nhwc(x, dst_hw):
    """Bilinear resize of fp32 (n, h, w, c) to (n, dst_h, dst_w, c); equal extents return x itself (skipped, not computed)."""
    n, hs, ws, c = x.shape
    hd, wd = dst_hw
    if (hs, ws) == (hd, wd):
        return x
    y0, y1, fy = taps(hs, hd)
    x0, x1, fx = taps(ws, wd)
    one = np.float32(1)
    fx = fx[None, None, :, None]
    gx = one - fx
    fy = fy[None, :, None, None]
    gy = one - fy
    r0, r1 = x[:, y0], x[:, y1]
    with np.errstate(invalid='ignore'):           # inf * 0 and inf - inf are NaN here as on the device
        top = gx * r0[:, :, x0] + fx * r0[:, :, x1]
        bot = gx * r1[:, :, x0] + fx * r1[:, :, x1]
        return (gy * top + fy * bot).astype(np.float32)


def preprocess(src, dst_hw, nhwc=True, reverse_channels=False, mean=None, std_scale=None):
    """fp32 NCHW (n, c, dst_h, dst_w) from `src` (uint8 or float32; (n, h, w, c) if nhwc else (n, c, h, w)): resize, reversal (output
    channel k reads source channel c-1-k), then (v - mean[k]) / std_scale[k] (either may be None)."""
    x = np.asarray(src)
    x = x.astype(np.float32) if nhwc else np.ascontiguousarray(x.transpose(0, 2, 3, 1)).astype(np.float32)
    v = resize_nhwc(x, dst_hw)
    if reverse_channels:
        v = v[..., ::-1]
    v = np.ascontiguousarray(v.transpose(0, 3, 1, 2))
    if mean is not None:
        v = v - np.asarray(mean, np.float32)[None, :, None, None]
    if std_scale is not None:
        v = v / np.asarray(std_scale, np.float32)[None, :, None, None]
    return np.ascontiguousarray(v, dtype=np.float32)
