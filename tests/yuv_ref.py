"""The colour conversion of IENetwork.input_info[name].preprocess_info.color_format 'NV12' / 'I420' restated in numpy: what
pvhip_input_preprocess_yuv_f32 does to a frame before the resize, bit for bit.  A frame is uint8 of 3 h / 2 rows of w bytes (h, w even):
rows 0..h-1 the Y plane; then NV12's h / 2 rows of w / 2 interleaved (U, V) pairs, or I420's U plane (h / 2 x w / 2 bytes, contiguous)
followed at once by its V plane.  Pixel (y, x) takes the (U, V) of its 2 x 2 block, [y // 2, x // 2] (nearest, no interpolation), and

    t = max(Y - 16, 0) * 1220542 + (1 << 19)
    R = (t + 1673527 * (V - 128)) >> 20
    G = (t -  852492 * (V - 128) - 409993 * (U - 128)) >> 20
    B = (t + 2116026 * (U - 128)) >> 20

in 32-bit integers with arithmetic shifts, each clamped to [0, 255]: BT.601 limited range, 1.164 / 1.596 / 0.813 / 0.391 / 2.018 over
2^20.  The device result is preprocess_ref.preprocess of the converted B, G, R image."""
import numpy as np

CY, CRV, CGV, CGU, CBU = 1220542, 1673527, 852492, 409993, 2116026
SHIFT = 20


def convert(y, u, v):
    """uint8 (..., 3) B, G, R of luma and chroma arrays of one shape (any integer type)."""
    y, u, v = (np.asarray(a).astype(np.int32) for a in (y, u, v))
    t = np.maximum(y - 16, 0) * np.int32(CY) + np.int32(1 << (SHIFT - 1))
    u, v = u - 128, v - 128
    b = (t + np.int32(CBU) * u) >> SHIFT
    g = (t - np.int32(CGV) * v - np.int32(CGU) * u) >> SHIFT
    r = (t + np.int32(CRV) * v) >> SHIFT
    assert b.dtype == g.dtype == r.dtype == np.int32
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def planes(frames, color_format):
    """(Y (n, h, w), U (n, h/2, w/2), V (n, h/2, w/2)) of uint8 frames (n, 3 h / 2, w)."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 3 and frames.shape[1] % 3 == 0 and frames.shape[2] % 2 == 0, frames.shape
    n, rows, w = frames.shape
    h = rows // 3 * 2
    flat = frames.reshape(n, rows * w)
    y, chroma = flat[:, :h * w].reshape(n, h, w), flat[:, h * w:]
    if color_format == 'NV12':
        uv = chroma.reshape(n, h // 2, w // 2, 2)
        return y, uv[..., 0], uv[..., 1]
    assert color_format == 'I420', color_format
    q = (h // 2) * (w // 2)
    return y, chroma[:, :q].reshape(n, h // 2, w // 2), chroma[:, q:].reshape(n, h // 2, w // 2)


def frames_of(y, u, v, color_format):
    """uint8 frames (n, 3 h / 2, w) of the planes Y (n, h, w), U and V (n, h/2, w/2)."""
    n, h, w = y.shape
    assert h % 2 == 0 and w % 2 == 0 and u.shape == v.shape == (n, h // 2, w // 2)
    if color_format == 'NV12':
        chroma = np.stack([u, v], -1)
    else:
        assert color_format == 'I420', color_format
        chroma = np.stack([u, v], 1)
    return np.concatenate([y.reshape(n, -1), chroma.reshape(n, -1)], 1).astype(np.uint8).reshape(n, h // 2 * 3, w)


def to_bgr(frames, color_format):
    """uint8 (n, h, w, 3) B, G, R image of uint8 frames (n, 3 h / 2, w)."""
    y, u, v = planes(frames, color_format)
    return convert(y, u.repeat(2, 1).repeat(2, 2), v.repeat(2, 1).repeat(2, 2))


def planes_from_bgr(bgr):
    """(Y, U, V) of a uint8 (n, h, w, 3) B, G, R image, as an encoder makes them: BT.601 limited range in float64, the chroma of a 2 x 2
    block the mean of its four pixels.  (Test material only: frames whose conversion back mostly does not saturate.)"""
    x = np.asarray(bgr).astype(np.float64)
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    y = 16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255
    u = 128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255
    v = 128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255
    n, h, w = y.shape
    sub = lambda c: c.reshape(n, h // 2, 2, w // 2, 2).mean((2, 4))  # noqa: E731
    q = lambda c: np.clip(np.rint(c), 0, 255).astype(np.uint8)  # noqa: E731
    return q(y), q(sub(u)), q(sub(v))
