"""The rule of ``infer(..., segments=...)`` (pvhip_segment_labels_f32) in plain loops.  This is the specification; the kernel and
pyopenvino_amd/segments.py equal it exactly.

For pixel (y, x) of batch row r of a float32 (n, C, H, W) stack of per-class score planes, with v[c] = X[r, c, y, x]:
  1. best    c* is the first class of the pixel's C values in top_k's total order: NaN of any sign or payload first, then descending
     with +0.0 == -0.0, ties to the lower class.
  2. void    the pixel is void iff v[c*] is NaN or (min_score is given and v[c*] < float32(min_score)).  Equality keeps.
  3. label   labels[r, y, x] = c*, or 255 when void.
  4. sums    areas[r, c] is the number of pixels of row r labelled c; extents[r, c] = (x0, y0, x1, y1) is min x, min y, max x + 1 and
     max y + 1 over those pixels, (0, 0, 0, 0) where there is none."""
import collections

import numpy as np

Segments = collections.namedtuple('Segments', 'labels areas extents')
VOID = 255


def best_of(values):
    """Rule 1 on one pixel's scores given as a list of Python floats (every float32 is one exactly): (c*, v[c*])."""
    best, top = 0, values[0]
    if top != top:
        return 0, top
    for c in range(1, len(values)):
        v = values[c]
        if v != v:                      # the first NaN: before every number
            return c, v
        if v > top:                     # strictly: ties, and zeros of either sign, stay with the lower class
            best, top = c, v
    return best, top


def best(x):
    """Rule 1 for every pixel of float32 `x` (n, C, H, W): (classes (n, H, W) int, their scores (n, H, W) float32).  It depends on
    nothing of the screen: compute it once per tensor."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4 and 1 <= x.shape[1] <= 255 and x.shape[2] * x.shape[3] >= 2
    n, C, H, W = x.shape
    classes = np.zeros((n, H, W), np.int64)
    scores = np.zeros((n, H, W), np.float32)
    for r in range(n):
        columns = x[r].reshape(C, H * W).T.tolist()
        for p, values in enumerate(columns):
            classes[r, p // W, p % W], scores[r, p // W, p % W] = best_of(values)
    return classes, scores


def segments(x, min_score=None, at=None):
    """Segments(labels (n, H, W) uint8, areas (n, C) int32, extents (n, C, 4) int32) of float32 `x` (n, C, H, W); `at`: best(x), when
    the caller has it already."""
    x = np.asarray(x)
    n, C, H, W = x.shape
    classes, scores = best(x) if at is None else at
    labels = np.empty((n, H, W), np.uint8)
    areas = np.zeros((n, C), np.int32)
    lo = np.zeros((n, C, 2), np.int64)
    hi = np.zeros((n, C, 2), np.int64)
    cut = None if min_score is None else np.float32(min_score)
    for r in range(n):
        for y in range(H):
            for xx in range(W):
                c, v = int(classes[r, y, xx]), scores[r, y, xx]
                if v != v or (cut is not None and v < cut):
                    labels[r, y, xx] = VOID
                    continue
                labels[r, y, xx] = c
                if areas[r, c] == 0:
                    lo[r, c], hi[r, c] = (xx, y), (xx + 1, y + 1)
                else:
                    lo[r, c] = (min(lo[r, c, 0], xx), min(lo[r, c, 1], y))
                    hi[r, c] = (max(hi[r, c, 0], xx + 1), max(hi[r, c, 1], y + 1))
                areas[r, c] += 1
    return Segments(labels, areas, np.concatenate([lo, hi], axis=2).astype(np.int32))
