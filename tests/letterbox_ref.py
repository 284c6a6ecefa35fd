"""The aspect-preserving fit of host inputs (preprocess_info.resize_fit 'LETTERBOX' / 'TOP_LEFT'; pvhip_input_preprocess_fit_f32 / _yuv_fit_f32 /
_packed_fit_f32) and the boxes mapped back (pvhip_detections_compact_fit / pvhip_detections_to_rois_fit) restated in numpy.  This is the
specification; the kernels equal it bit for bit and word for word.

Geometry, integers only: a source (or ROI rectangle) of (hs, ws) onto a destination of (hd, wd) is fitted into
  wide, ws hd >= hs wd:  iw = wd, ih = min(max((2 hs wd + ws) // (2 ws), 1), hd)        (the short side rounded half up)
  else:                  ih = hd, iw = min(max((2 ws hd + hs) // (2 hs), 1), wd)
  'LETTERBOX': dx = (wd - iw) // 2, dy = (hd - ih) // 2;  'TOP_LEFT': dx = dy = 0.
The image: inside [dy, dy + ih) x [dx, dx + iw) exactly what preprocess_ref / roi_ref / yuv_ref / packed_ref give for the same source onto
(ih, iw) -- so a source of exactly (ih, iw) is copied --; outside, the interpolated value is pad_value, which goes through the same
(v - mean[c]) / std_scale[c].  An invalid rectangle of a table is quiet NaN over the whole image.
The boxes: with fit = (Hn, Wn, dx, dy, iw, ih) a record's corner is u = (xmin float32(Wn) - float32(dx)) / float32(iw) (ymin: Hn, dy, ih), three
float32 roundings, and the rectangle is detected_rois_ref's with u in the place of the corner; the finite check is on the record's own
corners."""
import numpy as np

import packed_ref
import yuv_ref
from detected_rois_ref import Detected, _edge
from detections_ref import Compacted, label_of
from preprocess_ref import preprocess

FITS = ('LETTERBOX', 'TOP_LEFT')


def geometry(src_hw, dst_hw, fit):
    """(dx, dy, iw, ih) in Python ints."""
    (hs, ws), (hd, wd) = (int(v) for v in src_hw), (int(v) for v in dst_hw)
    assert fit in FITS and min(hs, ws, hd, wd) >= 1
    if ws * hd >= hs * wd:
        iw, ih = wd, min(max((2 * hs * wd + ws) // (2 * ws), 1), hd)
    else:
        ih, iw = hd, min(max((2 * ws * hd + hs) // (2 * hs), 1), wd)
    return ((wd - iw) // 2, (hd - ih) // 2, iw, ih) if fit == 'LETTERBOX' else (0, 0, iw, ih)


def to_image(frames, color='RAW'):
    """The (n, h, w, 3) uint8 B, G, R image of YUV 4:2:0 or 4-byte-unit frames; 'RAW' frames are the image."""
    if color == 'RAW':
        return np.asarray(frames)
    return yuv_ref.to_bgr(np.asarray(frames), color) if color in ('NV12', 'I420') else packed_ref.to_bgr(np.asarray(frames), color)


def fit_images(src, dst_hw, fit, pad_value=0.0, nhwc=True, reverse_channels=False, mean=None, std_scale=None):
    """fp32 NCHW (n, c, hd, wd) of `src` (uint8 or float32; (n, h, w, c) if nhwc else (n, c, h, w)): preprocess() onto (ih, iw), placed at
    (dy, dx), the rest the pad through the same mean / scale."""
    x = np.asarray(src)
    n, c = x.shape[0], x.shape[3 if nhwc else 1]
    hs, ws = x.shape[1:3] if nhwc else x.shape[2:4]
    dx, dy, iw, ih = geometry((hs, ws), dst_hw, fit)
    v = np.full((1, c, 1, 1), np.float32(pad_value), np.float32)
    if mean is not None:
        v = v - np.asarray(mean, np.float32)[None, :, None, None]
    if std_scale is not None:
        v = v / np.asarray(std_scale, np.float32)[None, :, None, None]
    out = np.empty((n, c) + tuple(dst_hw), np.float32)
    out[...] = v
    out[:, :, dy:dy + ih, dx:dx + iw] = preprocess(x, (ih, iw), nhwc=nhwc, reverse_channels=reverse_channels, mean=mean, std_scale=std_scale)
    return out


def fit_frames(frames, dst_hw, fit, pad_value=0.0, nhwc=True, color='RAW', **pre):
    """fit_images of frames in any declared format (`color` other than 'RAW': converted to a U8 NHWC B, G, R image first)."""
    return fit_images(to_image(frames, color), dst_hw, fit, pad_value, nhwc or color != 'RAW', **pre)


def fit_rois(frames, rois, dst_hw, fit, pad_value=0.0, nhwc=True, color='RAW', **pre):
    """fp32 NCHW (n, c, hd, wd): row b = fit_images(the crop rois[b] = (id, x, y, w, h) of the converted frame id); a row whose rectangle does
    not lie inside one of the frames is quiet NaN."""
    image = to_image(frames, color)
    nhwc = nhwc or color != 'RAW'
    m, c = image.shape[0], image.shape[3 if nhwc else 1]
    H, W = image.shape[1:3] if nhwc else image.shape[2:4]
    rows = []
    for i, x, y, w, h in np.asarray(rois).astype(np.int64).tolist():
        if not (0 <= i < m and x >= 0 and y >= 0 and w >= 1 and h >= 1 and x + w <= W and y + h <= H):
            rows.append(np.full((c,) + tuple(dst_hw), np.nan, np.float32))
            continue
        crop = image[i:i + 1, y:y + h, x:x + w, :] if nhwc else image[i:i + 1, :, y:y + h, x:x + w]
        rows.append(fit_images(crop, dst_hw, fit, pad_value, nhwc, **pre)[0])
    return np.ascontiguousarray(np.stack(rows, 0), dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------ the boxes mapped back
def unfit(v, extent, offset, inner):
    """u = (v float32(extent) - float32(offset)) / float32(inner): three float32 roundings."""
    with np.errstate(over='ignore'):
        return (np.float32(v) * np.float32(extent) - np.float32(offset)) / np.float32(inner)


def _survivors(records, images, extent, fit, min_confidence, labels, min_size):
    """(b, p, x0, y0, w, h) of every record that passes the screen, in (image, position) order; fit None: detected_rois_ref's rule."""
    rec = np.asarray(records)
    assert rec.dtype == np.float32 and rec.shape[-1] == 7
    rec = rec.reshape(-1, 7)
    assert rec.shape[0] % images == 0
    P, (H, W) = rec.shape[0] // images, extent
    conf = np.float32(min_confidence)
    wanted = None if labels is None else [np.float32(l) for l in labels]
    for b in range(images):
        for p in range(P):
            rank, label, score, xmin, ymin, xmax, ymax = rec[b * P + p]
            if not rank >= 0:
                break
            if not score >= conf or not np.isfinite([xmin, ymin, xmax, ymax]).all():
                continue
            if wanted is not None and not any(label == l for l in wanted):
                continue
            if fit is not None:
                Hn, Wn, dx, dy, iw, ih = fit
                xmin, xmax = unfit(xmin, Wn, dx, iw), unfit(xmax, Wn, dx, iw)
                ymin, ymax = unfit(ymin, Hn, dy, ih), unfit(ymax, Hn, dy, ih)
            x0, y0 = _edge(xmin, W, False), _edge(ymin, H, False)
            w, h = _edge(xmax, W, True) - x0, _edge(ymax, H, True) - y0
            if w < min_size[1] or h < min_size[0]:
                continue
            yield b, p, x0, y0, w, h


def compact_fit(records, images, extent, fit, min_confidence=0.5, labels=None, min_size=(1, 1), max_per_image=None):
    """detections_ref.compact over frames of `extent` = (H, W) for a detector whose input was fitted with `fit` = (Hn, Wn, dx, dy, iw, ih)."""
    rec = np.asarray(records).reshape(-1, 7)
    P, bits = rec.shape[0] // images, rec.view(np.uint32)
    cap = P if max_per_image is None else max_per_image
    counts, selected, table = np.zeros(images, np.int32), np.zeros(images, np.int32), []
    for b, p, x0, y0, w, h in _survivors(rec, images, extent, fit, min_confidence, labels, min_size):
        if selected[b] < cap:
            table.append(np.array([b, x0, y0, w, h, label_of(rec[b * P + p, 1]), 0, b * P + p], np.int64).astype(np.int32).view(np.uint32))
            table[-1][6] = bits[b * P + p, 2]
            counts[b] += 1
        selected[b] += 1
    return Compacted(counts, selected, np.array(table, np.uint32).reshape(-1, 8))


def detected_rois_fit(records, n, images, extent, fit, min_confidence=0.5, labels=None, min_size=(1, 1)):
    """detected_rois_ref.detected_rois for a detector whose input was fitted with `fit`."""
    P = np.asarray(records).reshape(-1, 7).shape[0] // images
    rois = np.zeros((n, 5), np.int32)
    rois[:, 0] = -1
    record_of = np.full(n, -1, np.int32)
    selected = 0
    for b, p, x0, y0, w, h in _survivors(records, images, extent, fit, min_confidence, labels, min_size):
        if selected < n:
            rois[selected] = (b, x0, y0, w, h)
            record_of[selected] = b * P + p
        selected += 1
    return Detected(min(selected, n), selected, rois, record_of)
