"""The colour rule of IENetwork.input_info[name].preprocess_info.color_standard / color_range restated in numpy: what the
pvhip_input_preprocess_*_color_f32 entries do to a YUV pixel before the resize, bit for bit.  One integer expression for all six
combinations, in 32-bit ints with arithmetic shifts, parameterised by (yoff, CY, CRV, CGV, CGU, CBU):

    y = max(Y - yoff, 0);  u = U - 128;  v = V - 128;  t = y * CY + (1 << 19)
    B = (t + CBU * u) >> 20;  G = (t - CGV * v - CGU * u) >> 20;  R = (t + CRV * v) >> 20        each clamped to [0, 255]

RULES[('BT601', 'LIMITED')] is the constants of tests/yuv_ref.py (cv2's three-decimal coefficients); every other row is
rint(x * 2^20) of the exact coefficients (``exact``).  Which chroma a pixel takes does not change: a 4:2:0 pixel that of its 2 x 2 block,
a 4:2:2 pixel that of its column pair (yuv_ref / packed_ref lay the frames out).  The device result is preprocess_ref / roi_ref /
letterbox_ref / warp_ref of the converted uint8 B, G, R image ``to_bgr`` gives, handed to them as a 'RAW' U8 NHWC image."""
import numpy as np

import packed_ref
import yuv_ref

STANDARDS = ('BT601', 'BT709', 'BT2020')                      # the `matrix` argument of the entries: the index
RANGES = ('LIMITED', 'FULL')                                  # the `full_range` argument: the index
KR_KB = {'BT601': (0.299, 0.114), 'BT709': (0.2126, 0.0722), 'BT2020': (0.2627, 0.0593)}
SHIFT = 20

# (yoff, CY, CRV, CGV, CGU, CBU)
RULES = {
    ('BT601', 'LIMITED'): (16, 1220542, 1673527, 852492, 409993, 2116026),
    ('BT601', 'FULL'): (0, 1048576, 1470104, 748826, 360853, 1858077),
    ('BT709', 'LIMITED'): (16, 1220945, 1879825, 558796, 223607, 2215014),
    ('BT709', 'FULL'): (0, 1048576, 1651297, 490864, 196424, 1945738),
    ('BT2020', 'LIMITED'): (16, 1220945, 1760217, 682019, 196426, 2245811),
    ('BT2020', 'FULL'): (0, 1048576, 1546230, 599107, 172546, 1972791),
}
NEW_RULES = [k for k in RULES if k != ('BT601', 'LIMITED')]


def codes(standard, range_):
    """(matrix, full_range) as the entries take them."""
    return STANDARDS.index(standard), RANGES.index(range_)


def exact(standard, range_):
    """(yoff, cy, crv, cgv, cgu, cbu) in float64: the matrix of the standard, luma scaled by 255/219 and chroma by 255/224 for LIMITED."""
    kr, kb = KR_KB[standard]
    kg = 1.0 - kr - kb
    ys, cs = (255.0 / 219.0, 255.0 / 224.0) if range_ == 'LIMITED' else (1.0, 1.0)
    return (16 if range_ == 'LIMITED' else 0, ys, 2 * (1 - kr) * cs, 2 * kr * (1 - kr) / kg * cs, 2 * kb * (1 - kb) / kg * cs, 2 * (1 - kb) * cs)


def convert(y, u, v, standard='BT601', range_='LIMITED'):
    """uint8 (..., 3) B, G, R of luma and chroma arrays of one shape (any integer type)."""
    yoff, cy, crv, cgv, cgu, cbu = (np.int32(c) for c in RULES[(standard, range_)])
    y, u, v = (np.asarray(a).astype(np.int32) for a in (y, u, v))
    t = np.maximum(y - yoff, 0) * cy + np.int32(1 << (SHIFT - 1))
    u, v = u - 128, v - 128
    b = (t + cbu * u) >> SHIFT
    g = (t - cgv * v - cgu * u) >> SHIFT
    r = (t + crv * v) >> SHIFT
    assert b.dtype == g.dtype == r.dtype == np.int32
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def to_bgr(frames, color, standard='BT601', range_='LIMITED'):
    """uint8 (n, h, w, 3) B, G, R image of uint8 frames: (n, 3 h / 2, w) for 'NV12' / 'I420', (n, h, w, 2) for 'YUY2' / 'UYVY'."""
    if color in ('NV12', 'I420'):
        y, u, v = yuv_ref.planes(frames, color)
        return convert(y, u.repeat(2, 1).repeat(2, 2), v.repeat(2, 1).repeat(2, 2), standard, range_)
    assert color in packed_ref.YUV422, color
    y, u, v = packed_ref.planes(frames, color)
    return convert(y, u.repeat(2, 2), v.repeat(2, 2), standard, range_)
