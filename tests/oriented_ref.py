"""The rule of ``infer(..., boxes=OrientedBoxScreen(...))`` (pvhip_oriented_boxes_f32) in plain loops.  This is the specification; the
kernels and pyopenvino_amd/oriented.py equal it bit for bit.  Steps 1 and 2 are float32, everything behind them is Python's float: one
binary64 operation at a time.  The steps are stated in pyopenvino_amd/oriented.py; here they are code."""
import collections
from fractions import Fraction
from math import factorial

import numpy as np

OrientedDetections = collections.namedtuple('OrientedDetections', 'counts selected quads boxes labels scores records')
F = np.float32
SIN = [float(Fraction((-1) ** i, factorial(2 * i + 1))) for i in range(1, 9)]
COS = [float(Fraction((-1) ** i, factorial(2 * i))) for i in range(1, 9)]


def cos_sin(angle):
    a = float(F(angle))
    k = float(np.rint(a * 0.6366197723675814))
    r = (a - k * 1.5707963267948966) - k * 6.123233995736766e-17
    z = r * r
    S, C = SIN[7], COS[7]
    for i in range(6, -1, -1):
        S, C = SIN[i] + z * S, COS[i] + z * C
    s, c = r + r * (z * S), 1.0 + z * C
    return [(c, s), (-s, c), (-c, -s), (s, -c)][int(k) & 3]


def corners(cx, cy, w, h, angle):
    """([p0, p1, p2, p3], area) of a box whose five numbers are float32."""
    cos, sin = cos_sin(angle)
    cx, cy, w, h = float(cx), float(cy), float(w), float(h)
    ux, uy, vx, vy = (w * 0.5) * cos, (w * 0.5) * sin, -((h * 0.5) * sin), (h * 0.5) * cos
    return [(cx - ux - vx, cy - uy - vy), (cx + ux - vx, cy + uy - vy), (cx + ux + vx, cy + uy + vy), (cx - ux + vx, cy - uy + vy)], w * h


def clip(subject, clipper, number=float):
    """The polygon of `subject` clipped by the edges of `clipper` in order; `number`: float, or Fraction for exact arithmetic."""
    poly = [(number(x), number(y)) for x, y in subject]
    for e in range(4):
        (ax, ay), (bx, by) = [(number(x), number(y)) for x, y in (clipper[e], clipper[(e + 1) % 4])]
        side = [(bx - ax) * (py - ay) - (by - ay) * (px - ax) for px, py in poly]
        out = []
        for m, (px, py) in enumerate(poly):
            (qx, qy), sp, sq = poly[(m + 1) % len(poly)], side[m], side[(m + 1) % len(poly)]
            if sp >= 0:
                out.append((px, py))
            if (sp >= 0) != (sq >= 0):
                t = sp / (sp - sq)
                out.append((px + t * (qx - px), py + t * (qy - py)))
        assert len(out) <= 8
        poly = out
        if not poly:
            break
    return poly


def inter(subject, clipper, number=float):
    poly, acc = clip(subject, clipper, number), number(0)
    for m, (px, py) in enumerate(poly):
        qx, qy = poly[(m + 1) % len(poly)]
        acc = acc + (px * qy - qx * py)
    return abs(acc) * number(0.5)


def winner(scores):
    """top_k's total order: the first NaN, else the first of the largest values (+0.0 == -0.0)."""
    best = 0
    for c, v in enumerate(scores):
        if np.isnan(v):
            return c
        if v > scores[best]:
            best = c
    return best


def decode(x, layout, min_score, frame, fit, objectness=False, labels=None, min_size=(1, 1), max_candidates=1024, overlap='IOU',
           threshold=0.45, per_label=True, max_per_image=None):
    v = x.transpose(0, 2, 1) if layout == 'NCA' else x                  # (n, A, E)
    n, A, E = v.shape
    O, (fh, fw), (dx, dy, iw, ih) = int(objectness), frame, fit
    C, cap, thr = E - 5 - O, max_per_image or max_candidates, float(F(threshold))
    counts, selected, rows = np.zeros(n, np.int32), np.zeros(n, np.int32), []
    for r in range(n):
        cand = []
        for a in range(A):
            e = v[r, a]
            c = winner(e[4 + O:4 + O + C])
            with np.errstate(all='ignore'):
                score = e[4] * e[4 + O + c] if O else e[4 + O + c]
            five = e[[0, 1, 2, 3, E - 1]]
            if not score >= F(min_score) or not np.isfinite(five).all() or not abs(five[4]) <= F(8):
                continue
            if not (five[2] >= F(min_size[1]) and five[3] >= F(min_size[0])) or (labels is not None and c not in labels):
                continue
            cand.append((-float(score + F(0)), a, c, score, five))
        selected[r] = len(cand)
        cand = sorted(cand, key=lambda t: t[:2])[:max_candidates]
        kept = []                                                       # (candidate, its corners, its area)
        for t in cand:
            quad, area = corners(*t[4])
            for u, other, other_area in kept:
                if per_label and u[2] != t[2]:
                    continue
                ddx, ddy = float(t[4][0]) - float(u[4][0]), float(t[4][1]) - float(u[4][1])
                R = ((float(t[4][2]) + float(t[4][3])) + (float(u[4][2]) + float(u[4][3]))) * 0.5
                if ddx * ddx + ddy * ddy > R * R:
                    continue
                both = inter(quad, other)
                if both > thr * (min(area, other_area) if overlap == 'IOS' else area + other_area - both):
                    break
            else:
                kept.append((t, quad, area))
                if len(kept) == cap:
                    break
        counts[r] = len(kept)
        for (_, a, c, score, five), quad, _ in kept:
            q = [[F((px - float(dx)) * float(fw) / float(iw)), F((py - float(dy)) * float(fh) / float(ih))] for px, py in quad]
            rows.append((q, five, c, score, r * A + a))
    col = list(zip(*rows)) if rows else [[]] * 5
    return OrientedDetections(counts, selected, np.asarray(col[0], np.float32).reshape(-1, 4, 2), np.asarray(col[1], np.float32).reshape(-1, 5),
                              np.asarray(col[2], np.int32), np.asarray(col[3], np.float32), np.asarray(col[4], np.int32))
