"""The conversion of IENetwork.input_info[name].preprocess_info.color_format 'YUY2' / 'UYVY' / 'BGRX' / 'RGBX' restated in numpy: what
pvhip_input_preprocess_packed_f32 does to a frame before the resize, bit for bit.

  YUY2 / UYVY (packed YUV 4:2:2): uint8 of shape (n, h, w, 2), the (h, w, 2) array cv2.cvtColor(..., COLOR_YUV2BGR_YUY2 / _UYVY) takes;
    w even, h any value >= 1.  Each row is w / 2 groups of 4 bytes: Y0 U Y1 V for YUY2, U Y0 V Y1 for UYVY.  Pixel (y, x) has luma
    Y[x & 1] of group x // 2 of row y, and that group's (U, V): chroma is not interpolated.  Each pixel goes to B, G, R by exactly the
    integer rule of tests/yuv_ref.py (BT.601 limited range over 2^20, arithmetic shifts, clamp to [0, 255]): the same function
    (yuv_ref.convert), not a second set of constants.
  BGRX / RGBX (four-byte pixels): uint8 of shape (n, h, w, 4), any h, w >= 1.  The B, G, R image is frames[..., 0:3] for BGRX and
    frames[..., 2::-1] for RGBX; byte 3 is never read into the result, whatever it holds.

The device result is preprocess_ref.preprocess(..., nhwc=True, ...) of the converted uint8 B, G, R image; batch row b of a RoiInput is the
crop of the CONVERTED frame (roi_ref semantics), so a 4:2:2 pixel keeps the chroma of its absolute column pair: rectangles may start on
odd x and have odd w."""
import numpy as np

import roi_ref
import yuv_ref
from preprocess_ref import preprocess

KINDS = {'YUY2': 0, 'UYVY': 1, 'BGRX': 2, 'RGBX': 3}          # the `kind` argument of the entries
YUV422 = ('YUY2', 'UYVY')
XRGB = ('BGRX', 'RGBX')
# byte positions inside a group of 4: (Y0, U, Y1, V)
GROUP = {'YUY2': (0, 1, 2, 3), 'UYVY': (1, 0, 3, 2)}


def bytes_per_pixel(color):
    return 2 if color in YUV422 else 4


def frame_shape(color, n, hw):
    return (n, hw[0], hw[1], bytes_per_pixel(color))


def planes(frames, color):
    """(Y (n, h, w), U (n, h, w / 2), V (n, h, w / 2)) of uint8 4:2:2 frames (n, h, w, 2)."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[3] == 2 and frames.shape[2] % 2 == 0, frames.shape
    n, h, w, _ = frames.shape
    g = frames.reshape(n, h, w // 2, 4)
    y0, u, y1, v = (g[..., k] for k in GROUP[color])
    return np.stack([y0, y1], -1).reshape(n, h, w), u, v


def frames_of(y, u, v, color):
    """uint8 4:2:2 frames (n, h, w, 2) of the planes Y (n, h, w), U and V (n, h, w / 2)."""
    n, h, w = y.shape
    assert w % 2 == 0 and u.shape == v.shape == (n, h, w // 2)
    g = np.empty((n, h, w // 2, 4), np.uint8)
    for k, p in zip(GROUP[color], (y[..., 0::2], u, y[..., 1::2], v)):
        g[..., k] = p
    return g.reshape(n, h, w, 2)


def to_bgr(frames, color):
    """uint8 (n, h, w, 3) B, G, R image of uint8 frames (n, h, w, 2) (YUY2, UYVY) or (n, h, w, 4) (BGRX, RGBX)."""
    frames = np.asarray(frames)
    if color in YUV422:
        y, u, v = planes(frames, color)
        return yuv_ref.convert(y, u.repeat(2, 2), v.repeat(2, 2))
    assert color in XRGB, color
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[3] == 4, frames.shape
    return np.ascontiguousarray(frames[..., 0:3] if color == 'BGRX' else frames[..., 2::-1])


def planes_from_bgr(bgr):
    """(Y, U, V) of a uint8 (n, h, w, 3) B, G, R image (w even) as a 4:2:2 encoder makes them: BT.601 limited range in float64, the
    chroma of a column pair the mean of its two pixels.  (Test material only: frames whose conversion back mostly does not saturate.)"""
    x = np.asarray(bgr).astype(np.float64)
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    y = 16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255
    u = 128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255
    v = 128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255
    n, h, w = y.shape
    sub = lambda c: c.reshape(n, h, w // 2, 2).mean(3)  # noqa: E731
    q = lambda c: np.clip(np.rint(c), 0, 255).astype(np.uint8)  # noqa: E731
    return q(y), q(sub(u)), q(sub(v))


def frames_from_bgr(bgr, color, x=None):
    """Frames of `color` that convert (back) to `bgr`: 4:2:2 frames encoded forward (planes_from_bgr; approximately back), X frames
    exactly, with byte 3 = `x` (an array or a value; default 255)."""
    bgr = np.asarray(bgr)
    if color in YUV422:
        return frames_of(*planes_from_bgr(bgr), color)
    out = np.empty(bgr.shape[:3] + (4,), np.uint8)
    out[..., 0:3] = bgr if color == 'BGRX' else bgr[..., ::-1]
    out[..., 3] = 255 if x is None else x
    return out


def preprocess_packed(frames, color, dst_hw, reverse_channels=False, mean=None, std_scale=None):
    """fp32 NCHW (n, 3, dst_h, dst_w): what the plain entry gives."""
    return preprocess(to_bgr(frames, color), dst_hw, nhwc=True, reverse_channels=reverse_channels, mean=mean, std_scale=std_scale)


def preprocess_rois(frames, color, rois, dst_hw, reverse_channels=False, mean=None, std_scale=None):
    """fp32 NCHW (n, 3, dst_h, dst_w): row b = preprocess(crop rois[b] of the converted frames): what the ROI entry gives."""
    return roi_ref.preprocess_rois(to_bgr(frames, color), rois, dst_hw, nhwc=True, reverse_channels=reverse_channels, mean=mean,
                                   std_scale=std_scale)
