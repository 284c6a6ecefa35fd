"""The rule of ``infer(..., detections=...)`` (pvhip_detections_compact) in plain numpy, record by record: DetectionOutput records become
one flat table of the detections a caller wants.  This is the specification; the kernel equals it word for word.

A record is [rank, label, score, xmin, ymin, xmax, ymax] with normalised corners; image b is rows [b P, (b + 1) P) of the R = N P rows.
  live      the list of an image ends at its first record whose column 0 is not >= 0 (DetectionOutput's -1 terminator; NaN too): that
            record and everything behind it is ignored;
  selected  live, score >= float32(min_confidence) (false for NaN), four finite corners, and `labels` is None or label == float32(l) for a
            listed l;
  rectangle in float32, never contracted: x0 = floor(min(max(xmin W, 0), W)), x1 = ceil(min(max(xmax W, 0), W)), y0 / y1 alike with H;
            dropped when x1 - x0 < min_size[1] or y1 - y0 < min_size[0]
(so far tests/detected_rois_ref.py, whose `_edge` is used here);
  cap       image b keeps its first counts[b] = min(selected[b], max_per_image) survivors in position order;
  table     kept survivors in (image, position) order, no gap between images; total = sum(counts);
  row       (b, x0, y0, w, h, label, score bits, record): label = int32 of column 1, truncated, when it is finite and in [-2^31, 2^31),
            else -1; the score keeps its bits; record = b P + p."""
import collections
import math

import numpy as np

from detected_rois_ref import _edge

Compacted = collections.namedtuple('Compacted', 'counts selected table')


def label_of(v) -> int:
    v = float(v)
    return int(v) if math.isfinite(v) and -2.0 ** 31 <= v < 2.0 ** 31 else -1


def compact(records, images, extent, min_confidence=0.5, labels=None, min_size=(1, 1), max_per_image=None):
    """Compacted(counts (N,) int32, selected (N,) int32, table (total, 8) uint32 -- the kernel's rows as 32-bit words, negative ints in two's
    complement --) of float32 `records` of shape (1, 1, R, 7) or (R, 7) that belong to `images` images of `extent` = (H, W)."""
    rec = np.asarray(records)
    assert rec.dtype == np.float32 and rec.shape[-1] == 7
    rec = rec.reshape(-1, 7)
    assert rec.shape[0] % images == 0
    P, (H, W) = rec.shape[0] // images, extent
    cap = P if max_per_image is None else max_per_image
    assert cap >= 1
    conf = np.float32(min_confidence)
    wanted = None if labels is None else [np.float32(l) for l in labels]
    bits = rec.view(np.uint32)
    counts, selected, table = np.zeros(images, np.int32), np.zeros(images, np.int32), []
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
            if selected[b] < cap:
                table.append(np.array([b, x0, y0, w, h, label_of(label), 0, b * P + p], np.int64).astype(np.int32).view(np.uint32))
                table[-1][6] = bits[b * P + p, 2]
                counts[b] += 1
            selected[b] += 1
    return Compacted(counts, selected, np.array(table, np.uint32).reshape(-1, 8))


def as_words(d):
    """A pyopenvino_amd.Detections as Compacted, for comparing word for word."""
    total = len(d.records)
    table = np.empty((total, 8), np.uint32)
    table[:, :5] = np.asarray(d.rois, np.int32).view(np.uint32).reshape(total, 5)
    table[:, 5] = np.asarray(d.labels, np.int32).view(np.uint32)
    table[:, 6] = np.ascontiguousarray(d.scores, np.float32).view(np.uint32)
    table[:, 7] = np.asarray(d.records, np.int32).view(np.uint32)
    return Compacted(np.asarray(d.counts), np.asarray(d.selected), table)
