"""The rule of ``infer(..., detections=TiledScreen(...))`` (pvhip_detections_merge_tiles) in plain numpy, tile by tile and candidate by
candidate: the DetectionOutput records of n tiles of m frames become one table of frame detections.  This is the specification; the
kernel equals it word for word.

A record is [rank, label, score, xmin, ymin, xmax, ymax] with normalised corners; batch row b is rows [b P, (b + 1) P) of the R = n P
rows and tile b = (f, x, y, w, h) of the (n, 5) table is the rectangle [y, y + h) x [x, x + w) of frame f it saw.
  1. candidates   tile b contributes nothing if f is outside [0, m), w < 1 or h < 1 (or w or h above 2^24, which float32 does not hold
                  exactly).  Otherwise its candidates are what tests/detections_ref.py selects over the extent (h, w) of the tile: live,
                  score >= float32(min_confidence), four finite corners, the label filter, floor / ceil of the clamped float32 products,
                  min_size.  The frame rectangle is (x + x0, y + y0, w, h) (int32 sums, which wrap): boxes clamp to the tile.  A tile
                  keeps its first max_per_tile candidates in position order; selected[f] counts the kept candidates of frame f's tiles.
  2. order        within a frame by descending score as a float, +0.0 = -0.0; ties go to the lower flat record b P + p.
  3. suppression  greedy in that order: candidate i is dropped iff an earlier candidate j that was kept overlaps it, with equal int
                  labels (the row's label word) when per_label is set.  int64 inter, a_i, a_j; den = a_i + a_j - inter ('IOU') or
                  min(a_i, a_j) ('IOS'); i overlaps j iff float64(inter) > float64(float32(threshold)) * float64(den).  Equality does not
                  suppress.
  4. cap, table   a frame keeps its first max_per_frame kept candidates: counts[f].  The table is in (frame, order of step 2) order
                  without gaps, rows (f, x0, y0, w, h, label, score bits, record) as tests/detections_ref.py makes them."""
import numpy as np

from detected_rois_ref import _edge
from detections_ref import Compacted, label_of

MAX_EXTENT = 1 << 24
MAX_CANDIDATES = 4096


def _wrapped(v) -> int:
    """The int32 an int32 sum wraps to."""
    return int(np.int64(v).astype(np.int32))


def candidates(records, tiles, frames, min_confidence=0.5, labels=None, min_size=(1, 1), max_per_tile=None):
    """Step 1: [(f, x0, y0, w, h, label, score bits, record)] of all tiles in record order, as Python ints."""
    rec = np.asarray(records)
    assert rec.dtype == np.float32 and rec.shape[-1] == 7
    rec = rec.reshape(-1, 7)
    tiles = np.asarray(tiles)
    n = tiles.shape[0]
    assert tiles.shape == (n, 5) and rec.shape[0] % n == 0
    P = rec.shape[0] // n
    cap = min(P, MAX_CANDIDATES // n) if max_per_tile is None else max_per_tile
    assert cap >= 1
    conf = np.float32(min_confidence)
    wanted = None if labels is None else [np.float32(l) for l in labels]
    bits = rec.view(np.uint32)
    out = []
    for b in range(n):
        f, x, y, w, h = (int(v) for v in tiles[b])
        if not 0 <= f < frames or not 1 <= w <= MAX_EXTENT or not 1 <= h <= MAX_EXTENT:
            continue
        taken = 0
        for p in range(P):
            rank, label, score, xmin, ymin, xmax, ymax = rec[b * P + p]
            if not rank >= 0:
                break
            if not score >= conf or not np.isfinite([xmin, ymin, xmax, ymax]).all():
                continue
            if wanted is not None and not any(label == l for l in wanted):
                continue
            x0, y0 = _edge(xmin, w, False), _edge(ymin, h, False)
            bw, bh = _edge(xmax, w, True) - x0, _edge(ymax, h, True) - y0
            if bw < min_size[1] or bh < min_size[0]:
                continue
            if taken < cap:
                out.append((f, _wrapped(x + x0), _wrapped(y + y0), bw, bh, label_of(label), int(bits[b * P + p, 2]), b * P + p))
                taken += 1
    return out


def overlaps(c, kept, overlap, threshold):
    """Step 3's comparison of the rectangle `c` = (x0, y0, w, h) with every row of the int64 (k, 4) array `kept`: (k,) bools."""
    x0, y0, w, h = (np.int64(v) for v in c)
    kx0, ky0, kw, kh = kept.T
    iw = np.minimum(x0 + w, kx0 + kw) - np.maximum(x0, kx0)
    ih = np.minimum(y0 + h, ky0 + kh) - np.maximum(y0, ky0)
    inter = np.where((iw > 0) & (ih > 0), iw * ih, np.int64(0))
    den = np.minimum(w * h, kw * kh) if overlap == 'IOS' else w * h + kw * kh - inter
    return inter.astype(np.float64) > np.float64(np.float32(threshold)) * den.astype(np.float64)


def merge(records, tiles, frames, min_confidence=0.5, labels=None, min_size=(1, 1), max_per_tile=None, overlap='IOU', threshold=0.45,
          per_label=True, max_per_frame=None):
    """Compacted(counts (m,) int32, selected (m,) int32, table (total, 8) uint32) of float32 `records` of shape (1, 1, R, 7) or (R, 7)
    that belong to the n tiles `tiles` (an integer (n, 5) table) of `frames` = m frames."""
    assert overlap in ('IOU', 'IOS')
    cand = candidates(records, tiles, frames, min_confidence, labels, min_size, max_per_tile)
    counts, selected, table = np.zeros(frames, np.int32), np.zeros(frames, np.int32), []
    for f in range(frames):
        mine = [c for c in cand if c[0] == f]
        selected[f] = len(mine)
        # (the score bits as a float: -0.0 == 0.0 there; sorted() is stable and `mine` is in record order)
        mine = sorted(mine, key=lambda c: -float(np.array(c[6], np.uint32).view(np.float32).astype(np.float64)))
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
