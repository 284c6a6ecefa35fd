"""The rule of ``infer(..., segments=FrameSegmentScreen(...))`` (pvhip_segment_frame_labels_f32) in plain loops, written from its text;
pyopenvino_amd is not imported.  This is the specification; the kernel and segments.frame_labels equal it exactly, no tolerance anywhere.

For frame pixel (X, Y) of batch row r of a float32 (n, C, H, W) stack of planes, L[c] = X[r, c], over frames (Fh, Fw) that stand in the
rectangle (dx, dy, iw, ih) of a network input (Hn, Wn):
  1. position  in exact integers N = (2 dx F + (2 X + 1) iw) W - F Wn and D = 2 F Wn with F = Fw; P = floor(65536 N / D), floor toward
     minus infinity; the taps P >> 16 and (P >> 16) + 1 clamped to [0, W - 1]; fx = float32(P & 65535) / 65536.  Rows alike.  (The
     position rule of frame_masks_ref.tap word for word.)
  2. value     t0 = L[c][ya][xa] + fx * (L[c][ya][xb] - L[c][ya][xa]), t1 likewise on row yb, v[c] = t0 + fy * (t1 - t0): float32, each
     operation rounded once, no fma; all four taps are always read; NaN and inf follow IEEE.
  3. best, void, label  rules 1 to 3 of segments_ref on v[c]: the first class in top_k's total order, ties to the lower class; void iff
     the best is NaN or below float32(min_score), equality keeps; 255 when void.
  4. sums      areas and extents as segments_ref, over frame pixels."""
import numpy as np

from frame_masks_ref import tap
from segments_ref import VOID, Segments, best_of


def frame_segments(x, net_hw, frame, fit, min_score=None):
    """Segments(labels (n, Fh, Fw) uint8, areas (n, C) int32, extents (n, C, 4) int32) of float32 `x` (n, C, H, W).  A frame row's
    values are numpy float32 rows: one rounding per operation, as the scalars would have."""
    n, C, H, W = x.shape
    (hn, wn), (fh, fw), (dx, dy, iw, ih) = net_hw, frame, fit
    cols = [tap(X, dx, iw, fw, W, wn) for X in range(fw)]
    xa, xb, fx = [c[0] for c in cols], [c[1] for c in cols], np.asarray([c[2] for c in cols], np.float32)
    cut = None if min_score is None else np.float32(min_score)
    labels = np.empty((n, fh, fw), np.uint8)
    areas = np.zeros((n, C), np.int32)
    extents = np.zeros((n, C, 4), np.int32)
    for r in range(n):
        for Y in range(fh):
            ya, yb, fy = tap(Y, dy, ih, fh, H, hn)
            values = []
            with np.errstate(all='ignore'):
                for c in range(C):
                    L = x[r, c]
                    t0 = L[ya, xa] + fx * (L[ya, xb] - L[ya, xa])
                    t1 = L[yb, xa] + fx * (L[yb, xb] - L[yb, xa])
                    values.append(t0 + fy * (t1 - t0))
            for X, pixel in enumerate(np.stack(values, axis=1).tolist()):
                c, v = best_of(pixel)
                if v != v or (cut is not None and v < cut):
                    labels[r, Y, X] = VOID
                    continue
                labels[r, Y, X] = c
                x0, y0, x1, y1 = extents[r, c] if areas[r, c] else (X, Y, X + 1, Y + 1)
                extents[r, c] = (min(x0, X), min(y0, Y), max(x1, X + 1), max(y1, Y + 1))
                areas[r, c] += 1
    return Segments(labels, areas, extents)
