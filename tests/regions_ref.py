"""The rule of ``infer(..., detections=RegionScreen(...))`` (pvhip_detections_merge_regions) in plain loops, region by region and record by
record: the DetectionOutput records of n regions of m frames -- regions of any aspect, each placed in the detector's (Hn, Wn) input by an
aspect-preserving fit -- become one table of frame detections.  This is the specification; the kernel equals it word for word.

Region b = (f, x, y, w, h) is row b of the (n, 5) table: a RoiInput's, or the one a DetectedRois made, whose rows behind `count` are
(-1, 0, 0, 0, 0).  A record is [rank, label, score, xmin, ymin, xmax, ymax]; batch row b is rows [b P, (b + 1) P).
  1. candidates   region b contributes nothing if f is outside [0, m), or w or h is outside [1, 2^24].  Otherwise its geometry, in Python
                  ints (the rule that placed its pixels in the input):
                    wide, w Hn >= h Wn:  iw = Wn, ih = min(max((2 h Wn + w) // (2 w), 1), Hn)      (the short side rounded half up)
                    else:                ih = Hn, iw = min(max((2 w Hn + h) // (2 h), 1), Wn)
                    'LETTERBOX': dx = (Wn - iw) // 2, dy = (Hn - ih) // 2;  'TOP_LEFT': dx = dy = 0.
                  A record is live in front of the region's first row whose rank is not >= 0; it is a candidate when score >=
                  float32(min_confidence), its own four corners are finite, its label is listed (labels None: any), and its rectangle
                  over (h, w) is at least min_size.  The rectangle: each corner is mapped back, u = (v float32(N) - float32(d)) / float32(i)
                  with (N, d, i) = (Wn, dx, iw) for an x and (Hn, dy, ih) for a y -- three float32 roundings --, then x0 = floor(min(max(u
                  float32(w), 0), w)), x1 = ceil(the same of xmax), y0 / y1 alike with h.  So a box in the padding clamps to the region's
                  edge and one wholly in the padding has no extent and is dropped.  'STRETCH' maps nothing: u = v, tiles_ref's rule.
                  The frame rectangle is (x + x0, y + y0, w, h), int32 sums which wrap.  A region keeps its first max_per_region
                  candidates in position order; selected[f] counts the kept candidates of frame f's regions.
  2. - 4.         order, suppression, cap and table: tests/tiles_ref.py's, with its comparison (tiles_ref.overlaps)."""
import numpy as np

from detections_ref import Compacted, label_of
from tiles_ref import MAX_CANDIDATES, MAX_EXTENT, overlaps

FITS = ('STRETCH', 'LETTERBOX', 'TOP_LEFT')


def geometry(h, w, Hn, Wn, fit):
    """(dx, dy, iw, ih) of a region of (h, w) in an input of (Hn, Wn): Python ints."""
    h, w, Hn, Wn = int(h), int(w), int(Hn), int(Wn)
    if w * Hn >= h * Wn:
        iw, ih = Wn, min(max((2 * h * Wn + w) // (2 * w), 1), Hn)
    else:
        ih, iw = Hn, min(max((2 * w * Hn + h) // (2 * h), 1), Wn)
    return ((Wn - iw) // 2, (Hn - ih) // 2, iw, ih) if fit == 'LETTERBOX' else (0, 0, iw, ih)


def _back(v, N, d, i):
    with np.errstate(over='ignore'):
        return (np.float32(v) * np.float32(N) - np.float32(d)) / np.float32(i)


def _clamped(u, extent, up):
    """floor (ceil for `up`) of the float32 product u * extent clamped to [0, extent], as a Python int."""
    e = np.float32(extent)
    with np.errstate(over='ignore'):
        t = min(max(np.float32(u) * e, np.float32(0)), e)
    return int(np.ceil(t)) if up else int(np.floor(t))


def _int32(v):
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def candidates(records, regions, frames, net_hw, fit, min_confidence=0.5, labels=None, min_size=(1, 1), max_per_region=None):
    """Step 1: [(f, x0, y0, w, h, label, score bits, record)] of all regions in record order, as Python ints."""
    assert fit in FITS
    rec = np.asarray(records)
    assert rec.dtype == np.float32 and rec.shape[-1] == 7
    rec = rec.reshape(-1, 7)
    regions = np.asarray(regions)
    n = regions.shape[0]
    assert regions.shape == (n, 5) and rec.shape[0] % n == 0
    P = rec.shape[0] // n
    cap = min(P, MAX_CANDIDATES // n) if max_per_region is None else max_per_region
    assert cap >= 1
    conf = np.float32(min_confidence)
    bits = rec.view(np.uint32)
    out = []
    for b in range(n):
        f, x, y, w, h = (int(v) for v in regions[b])
        if f < 0 or f >= frames or w < 1 or w > MAX_EXTENT or h < 1 or h > MAX_EXTENT:
            continue
        if fit != 'STRETCH':
            Hn, Wn = net_hw
            dx, dy, iw, ih = geometry(h, w, Hn, Wn, fit)
        taken = 0
        for p in range(P):
            r = b * P + p
            rank, label, score, xmin, ymin, xmax, ymax = rec[r]
            if not rank >= 0:
                break
            if not score >= conf:
                continue
            if not all(np.isfinite(c) for c in (xmin, ymin, xmax, ymax)):
                continue
            if labels is not None and not any(label == np.float32(l) for l in labels):
                continue
            if fit != 'STRETCH':
                xmin, xmax = _back(xmin, Wn, dx, iw), _back(xmax, Wn, dx, iw)
                ymin, ymax = _back(ymin, Hn, dy, ih), _back(ymax, Hn, dy, ih)
            x0, y0 = _clamped(xmin, w, False), _clamped(ymin, h, False)
            bw, bh = _clamped(xmax, w, True) - x0, _clamped(ymax, h, True) - y0
            if bw < min_size[1] or bh < min_size[0]:
                continue
            if taken < cap:
                out.append((f, _int32(x + x0), _int32(y + y0), bw, bh, label_of(label), int(bits[r, 2]), r))
                taken += 1
    return out


def merge(records, regions, frames, net_hw=None, fit='STRETCH', min_confidence=0.5, labels=None, min_size=(1, 1), max_per_region=None,
          overlap='IOU', threshold=0.45, per_label=True, max_per_frame=None):
    """Compacted(counts (m,) int32, selected (m,) int32, table (total, 8) uint32) of float32 `records` of shape (1, 1, R, 7) or (R, 7)
    that belong to the n regions `regions` (an integer (n, 5) table) of `frames` = m frames."""
    assert overlap in ('IOU', 'IOS')
    cand = candidates(records, regions, frames, net_hw, fit, min_confidence, labels, min_size, max_per_region)
    counts, selected, table = np.zeros(frames, np.int32), np.zeros(frames, np.int32), []
    for f in range(frames):
        mine = [c for c in cand if c[0] == f]
        selected[f] = len(mine)
        # (the score as a float, -0.0 == 0.0; sorted() is stable and `mine` is in record order)
        mine = sorted(mine, key=lambda c: -float(np.array(c[6], np.uint32).view(np.float32)))
        kept, boxes, kept_labels = [], np.zeros((len(mine), 4), np.int64), np.zeros(len(mine), np.int64)
        for c in mine:
            k = len(kept)
            hit = overlaps(c[1:5], boxes[:k], overlap, threshold)
            if per_label:
                hit &= kept_labels[:k] == c[5]
            if not hit.any():
                boxes[k], kept_labels[k] = c[1:5], c[5]
                kept.append(c)
        if max_per_frame is not None:
            kept = kept[:max_per_frame]
        counts[f] = len(kept)
        table += kept
    words = np.array(table, np.int64).reshape(-1, 8)
    return Compacted(counts, selected, (words & 0xFFFFFFFF).astype(np.uint32))
