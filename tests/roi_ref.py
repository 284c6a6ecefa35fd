"""Regions of interest (pyopenvino_amd.RoiInput; pvhip_input_preprocess_roi_f32 / _yuv_roi_f32) restated in numpy: batch row b is the
rectangle rois[b] = (id, x, y, w, h) -- the order of OpenVINO's ROI struct -- of frame id, CROPPED and then put through
preprocess_ref.preprocess like an image of its own.  So the bilinear taps clamp at the edge of the rectangle, not of the frame; a
rectangle of exactly the destination's extent is copied, not interpolated (resize_nhwc skips equal extents); and a YUV rectangle is the
crop of the converted frame, so a pixel keeps the chroma of its absolute 2 x 2 block whatever the parity of the rectangle's origin."""
import numpy as np

import yuv_ref
from preprocess_ref import preprocess


def valid(rois, n, m, frame_hw):
    """The table is an integer (n, 5) array of rectangles inside one of m frames of extent frame_hw."""
    t = np.asarray(rois)
    if t.shape != (n, 5) or t.dtype.kind not in 'iu':
        return False
    i, x, y, w, h = t.astype(np.int64).T
    H, W = frame_hw
    return bool(((i >= 0) & (i < m) & (x >= 0) & (y >= 0) & (w >= 1) & (h >= 1) & (x + w <= W) & (y + h <= H)).all())


def crop(frames, roi, nhwc=True, color='RAW'):
    """The rectangle `roi` of `frames` as an image (1, h, w, c) / (1, c, h, w); YUV frames (m, 3 H / 2, W): of the converted B, G, R one."""
    i, x, y, w, h = (int(v) for v in roi)
    if color != 'RAW':
        return yuv_ref.to_bgr(np.asarray(frames)[i:i + 1], color)[:, y:y + h, x:x + w, :]
    frames = np.asarray(frames)
    return frames[i:i + 1, y:y + h, x:x + w, :] if nhwc else frames[i:i + 1, :, y:y + h, x:x + w]


def preprocess_rois(frames, rois, dst_hw, nhwc=True, reverse_channels=False, mean=None, std_scale=None, color='RAW'):
    """fp32 NCHW (n, c, dst_h, dst_w): row b = preprocess(crop of rois[b]).  `frames`: (m, H, W, c) if nhwc else (m, c, H, W), uint8 or
    float32; for color 'NV12' / 'I420' uint8 (m, 3 H / 2, W), converted to B, G, R first (an NHWC image)."""
    frames = np.asarray(frames)
    yuv = color != 'RAW'
    H, W = (frames.shape[1] // 3 * 2, frames.shape[2]) if yuv else (frames.shape[1:3] if nhwc else frames.shape[2:4])
    rois = np.asarray(rois)
    assert valid(rois, len(rois), frames.shape[0], (H, W)), rois
    rows = [preprocess(crop(frames, r, nhwc, color), dst_hw, nhwc=nhwc or yuv, reverse_channels=reverse_channels, mean=mean,
                       std_scale=std_scale)[0] for r in rois]
    return np.ascontiguousarray(np.stack(rows, 0), dtype=np.float32)
