"""The rule of pyopenvino_amd.DetectedRois (pvhip_detections_to_rois) in plain numpy: DetectionOutput records become the (n, 5) table of
a RoiInput.  This is the specification; the kernel equals it integer for integer.

A record is [rank, label, score, xmin, ymin, xmax, ymax] with normalised corners; image b is rows [b P, (b + 1) P) of the R = N P rows.
  live      the list of an image ends at its first record whose column 0 is not >= 0 (DetectionOutput's -1 terminator; NaN too): that
            record and everything behind it is ignored;
  selected  live, score >= float32(min_confidence) (false for NaN), four finite corners, and `labels` is None or label == float32(l) for a
            listed l;
  rectangle in float32, never contracted: x0 = floor(min(max(xmin W, 0), W)), x1 = ceil(min(max(xmax W, 0), W)), y0 / y1 alike with H;
            dropped when x1 - x0 < min_size[1] or y1 - y0 < min_size[0];
  order     survivors keep (image, position); survivor k < n is row k = (b, x0, y0, w, h) with records[k] = b P + p; rows >= count =
            min(selected, n) are (-1, 0, 0, 0, 0) with records[k] = -1; `selected` counts every survivor."""
import collections

import numpy as np

Detected = collections.namedtuple('Detected', 'count selected rois records')


def _edge(v, extent, up):
    """floor (ceil for `up`) of the float32 product v * extent clamped to [0, extent], as an int."""
    e = np.float32(extent)
    with np.errstate(over='ignore'):
        t = np.minimum(np.maximum(np.float32(v) * e, np.float32(0)), e)
    return int(np.ceil(t) if up else np.floor(t))


def detected_rois(records, n, images, extent, min_confidence=0.5, labels=None, min_size=(1, 1)):
    """Detected(count, selected, rois (n, 5) int32, records (n,) int32) of float32 `records` of shape (1, 1, R, 7) or (R, 7) that belong
    to `images` images of `extent` = (H, W)."""
    rec = np.asarray(records)
    assert rec.dtype == np.float32 and rec.shape[-1] == 7
    rec = rec.reshape(-1, 7)
    assert rec.shape[0] % images == 0
    P, (H, W) = rec.shape[0] // images, extent
    conf = np.float32(min_confidence)
    wanted = None if labels is None else [np.float32(l) for l in labels]
    rois = np.zeros((n, 5), np.int32)
    rois[:, 0] = -1
    record_of = np.full(n, -1, np.int32)
    selected = 0
    for b in range(images):
        for p in range(P):
            rank, label, score, xmin, ymin, xmax, ymax = rec[b * P + p]
            if not rank >= 0:
                break
            if not score >= conf or not np.isfinite([xmin, ymin, xmax, ymax]).all():
                continue
            if wanted is not None and not any(label == l for l in wanted):
                continue
            x0, y0 = _edge(xmin, W, False), _edge(ymin, H, False)
            w, h = _edge(xmax, W, True) - x0, _edge(ymax, H, True) - y0
            if w < min_size[1] or h < min_size[0]:
                continue
            if selected < n:
                rois[selected] = (b, x0, y0, w, h)
                record_of[selected] = b * P + p
            selected += 1
    return Detected(min(selected, n), selected, rois, record_of)


def padded(rois, pad=(0, 0, 0, 1, 1)):
    """`rois` with every row (-1, 0, 0, 0, 0) replaced by the valid rectangle `pad`: what a RoiInput is fed for the same rows < count."""
    out = np.array(rois, np.int32, copy=True)
    out[out[:, 0] < 0] = pad
    return out
