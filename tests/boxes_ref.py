"""The rule of ``infer(..., boxes=...)`` (pvhip_dense_boxes_f32) in plain loops.  This is the specification; the kernel and
pyopenvino_amd/boxes.py equal it bit for bit.

For image r and anchor a of a float32 tensor read as 'NCA' (n, E, A) or 'NAC' (n, A, E), with channel values e[0 .. E - 1], E = 4 + O + C
(O = 1 iff objectness), the first four the box:
  1. winner  c* is the first of the C class scores e[4 + O ..] in top_k's total order: NaN of any sign or payload first, then descending
     with +0.0 == -0.0, ties to the lower class.  score = e[4 + O + c*], or, with objectness, e[4] * e[4 + O + c*] as one float32 product.
     The anchor is out iff the score is NaN or below float32(min_score); equality keeps.
  2. box     all four box numbers finite, else out.  'CXCYWH' corners in float32: xa = cx - w * 0.5, xb = cx + w * 0.5, ya and yb alike;
     'XYXY': the numbers themselves.  A corner p maps to the frame in binary64 as t = ((double)p - (double)d) * (double)F / (double)i,
     (d, i, F) = (dx, iw, frame_w) for an x corner and (dy, ih, frame_h) for a y corner.  x0 = floor(min(max(t(xa), 0), frame_w)), x1 =
     ceil(min(max(t(xb), 0), frame_w)), w = x1 - x0; y alike.  Out when w < min_w or h < min_h, and, with labels, unless c* is listed.
  3. cap     selected[r] counts the anchors still in; the K best go on: descending score with +0.0 == -0.0, ties to the lower anchor.
  4. suppression  greedy in that order: int64 areas of the frame rectangles, den the union ('IOU') or the smaller area ('IOS'), dropped
     iff an earlier kept one -- of the same c* when per_label -- overlaps it with (double)inter > (double)threshold * (double)den.
  5. table   image r keeps its first counts[r] = min(kept, max_per_image) kept candidates; rows (r, x0, y0, w, h, c*, score bits,
     r * A + a) in (image, order of 3) order without gaps; total = sum(counts)."""
import collections
import math

import numpy as np

Detections = collections.namedtuple('Detections', 'counts selected rois labels scores records')
HALF = np.float32(0.5)


def order_word(bits: int) -> int:
    """The float32 with these bits as an unsigned that orders like top_k's total order: every NaN the maximum, -0.0 folded onto +0.0."""
    mag = bits & 0x7FFFFFFF
    if mag > 0x7F800000:
        return 0xFFFFFFFF
    if mag == 0:
        return 0x80000000
    return (~bits & 0xFFFFFFFF) if bits & 0x80000000 else bits | 0x80000000


def first_class(bits) -> int:
    """Rule 1 on the bit patterns of one anchor's class scores: a strictly larger order word alone replaces."""
    best, word = 0, order_word(bits[0])
    for c in range(1, len(bits)):
        w = order_word(bits[c])
        if w > word:
            best, word = c, w
    return best


def to_frame(p, d, F, i) -> float:
    """((double)p - (double)d) * (double)F / (double)i in Python floats, which are binary64."""
    return (float(p) - float(d)) * float(F) / float(i)


def rectangle(b, box, frame, geometry):
    """(x0, y0, w, h) of four finite float32 box numbers over `frame` = (H, W) through `geometry` = (dx, dy, iw, ih)."""
    if box == 'CXCYWH':
        with np.errstate(over='ignore'):
            hw, hh = b[2] * HALF, b[3] * HALF
            xa, xb, ya, yb = b[0] - hw, b[0] + hw, b[1] - hh, b[1] + hh
    else:
        xa, ya, xb, yb = b
    (fh, fw), (dx, dy, iw, ih) = frame, geometry
    x0 = math.floor(min(max(to_frame(xa, dx, fw, iw), 0.0), float(fw)))
    x1 = math.ceil(min(max(to_frame(xb, dx, fw, iw), 0.0), float(fw)))
    y0 = math.floor(min(max(to_frame(ya, dy, fh, ih), 0.0), float(fh)))
    y1 = math.ceil(min(max(to_frame(yb, dy, fh, ih), 0.0), float(fh)))
    return x0, y0, x1 - x0, y1 - y0


def suppresses(j, i, overlap, threshold) -> bool:
    """Rule 4's comparison of the kept rectangle j with the later rectangle i, both (x0, y0, w, h) in Python ints."""
    iw = min(i[0] + i[2], j[0] + j[2]) - max(i[0], j[0])
    ih = min(i[1] + i[3], j[1] + j[3]) - max(i[1], j[1])
    inter = iw * ih if iw > 0 and ih > 0 else 0
    ai, aj = i[2] * i[3], j[2] * j[3]
    den = min(ai, aj) if overlap == 'IOS' else ai + aj - inter
    return float(inter) > float(np.float32(threshold)) * float(den)


def decode(x, layout, min_score, frame, geometry, objectness=False, box='CXCYWH', labels=None, min_size=(1, 1), max_candidates=1024,
           overlap='IOU', threshold=0.45, per_label=True, max_per_image=None) -> Detections:
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 3 and layout in ('NCA', 'NAC')
    v = np.ascontiguousarray(x.transpose(0, 2, 1) if layout == 'NCA' else x)           # (n, A, E): a copy in the rule's own order
    n, A, E = v.shape
    O = 1 if objectness else 0
    C = E - 4 - O
    assert C >= 1
    bits = v.view(np.uint32).tolist()
    low = np.float32(min_score)
    cap = max_candidates if max_per_image is None else max_per_image
    counts, selected, rows = [], [], []
    for r in range(n):
        cands = []
        for a in range(A):
            c = first_class(bits[r][a][4 + O:])
            with np.errstate(invalid='ignore', over='ignore', under='ignore'):
                score = v[r, a, 4 + O + c] * v[r, a, 4] if O else v[r, a, 4 + O + c]
            if not score >= low:
                continue
            b = [v[r, a, k] for k in range(4)]
            if not all(math.isfinite(float(q)) for q in b):
                continue
            rect = rectangle(b, box, frame, geometry)
            if rect[2] < min_size[1] or rect[3] < min_size[0]:
                continue
            if labels is not None and c not in labels:
                continue
            score_bits = int(np.asarray(score, np.float32).view(np.uint32))
            cands.append((order_word(score_bits), a, c, rect, score_bits))
        selected.append(len(cands))
        cands.sort(key=lambda q: (-q[0], q[1]))
        kept = []
        for q in cands[:max_candidates]:
            if len(kept) == cap:
                break
            if not any((not per_label or j[2] == q[2]) and suppresses(j[3], q[3], overlap, threshold) for j in kept):
                kept.append(q)
        counts.append(len(kept))
        rows += [(r,) + q[3] + (q[2], q[4], r * A + q[1]) for q in kept]
    t = np.asarray(rows, np.int64).reshape(-1, 8)
    return Detections(np.asarray(counts, np.int32), np.asarray(selected, np.int32), t[:, :5].astype(np.int32), t[:, 5].astype(np.int32),
                      t[:, 6].astype(np.uint32).view(np.float32), t[:, 7].astype(np.int32))
