"""The rule of ``infer(..., maxima=...)`` (pvhip_heatmap_maxima_f32) in plain loops.  This is the specification; the kernel and
pyopenvino_amd/maxima.py equal it bit for bit.

For the plane v[0..H)[0..W) of batch row r and channel c of a float32 (n, K, H, W) stack of heatmaps:
  1. maximum  key(q) is top_k's key of (v[q], flat index q): NaN of any sign or payload first, then descending with +0.0 == -0.0, ties
     to the lower index.  Position p is a maximum iff v[p] is not NaN and key(p) is larger than the key of each of its at most eight
     neighbours that lie inside the plane.  A plateau therefore yields only those of its pixels that have no plateau neighbour before
     them in raster order; a flat plane has one maximum, at index 0.  A NaN is never a maximum and suppresses all its neighbours.
     This differs from CenterNet's ``hmax == heat`` only on exact ties.
  2. screen   the maximum passes iff min_score is None or v[p] >= float32(min_score).  Equality keeps.
  3. per plane  the first max_per_plane passing maxima are kept, in descending key order.
  4. per row  the kept maxima of the row's K planes are ordered by descending value, ties to the lower channel, then to the lower
     position: the key of (value, c * H * W + p).  The first max_per_row are the answer.
  5. refine / space  rules 3 and 4 of tests/keypoints_ref.py word for word, applied at each answered position.
Row r's first counts[r] slots are its maxima, best first; the slots behind them are (-1, -1, quiet NaN, quiet NaN, quiet NaN)."""
import collections
import functools

import numpy as np

Maxima = collections.namedtuple('Maxima', 'counts channels positions scores points')
QUIET_NAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def before(a, b):
    """(value, index) a stands before (value, index) b in top_k's total order; the values are Python floats."""
    (va, ia), (vb, ib) = a, b
    nan_a, nan_b = va != va, vb != vb
    if nan_a or nan_b:
        return (nan_a and not nan_b) or (nan_a and nan_b and ia < ib)
    if va != vb:                        # (+0.0 == -0.0)
        return va > vb
    return ia < ib


def plane_maxima(values, H, W):
    """Rule 1 on one plane given as a flat list of Python floats: the flat indices of its maxima, in raster order."""
    found = []
    for py in range(H):
        for px in range(W):
            p = py * W + px
            v = values[p]
            if v != v:
                continue
            top = True
            for qy in range(max(0, py - 1), min(H, py + 2)):
                for qx in range(max(0, px - 1), min(W, px + 2)):
                    q = qy * W + qx
                    if q != p and not before((v, p), (values[q], q)):
                        top = False
            if top:
                found.append(p)
    return found


def found_in(x):
    """Rule 1 for every plane of float32 `x` (n, K, H, W): [[the maxima of plane (r, c), descending in key order]].  It depends on
    nothing of the screen: compute it once per tensor."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4 and x.shape[2] * x.shape[3] >= 2
    n, K, H, W = x.shape
    order = functools.cmp_to_key(lambda a, b: -1 if before(a, b) else 1)
    out = []
    for r in range(n):
        out.append([])
        for c in range(K):
            values = x[r, c].reshape(-1).tolist()
            pairs = sorted(((values[p], p) for p in plane_maxima(values, H, W)), key=order)
            out[-1].append([p for _, p in pairs])
    return out


def _quarter(before_, after):
    if after > before_:
        return np.float32(0.25)
    if after < before_:
        return np.float32(-0.25)
    return np.float32(0.0)


def maxima(x, min_score=None, max_per_plane=32, max_per_row=None, refine='QUARTER', space='NORMALISED', found=None):
    """Maxima(counts (n,) int32, channels (n, R) int32, positions (n, R) int32, scores (n, R) float32, points (n, R, 2) float32) of float32
    `x` (n, K, H, W); `found`: found_in(x), when the caller has it already."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4 and refine in ('NONE', 'QUARTER') and space in ('HEATMAP', 'NORMALISED')
    n, K, H, W = x.shape
    M = max_per_plane
    R = min(K * M, 1024) if max_per_row is None else max_per_row
    assert 1 <= M <= 256 and 1 <= R <= 1024 and K * H * W <= 2 ** 31 - 1
    found = found_in(x) if found is None else found
    order = functools.cmp_to_key(lambda a, b: -1 if before(a, b) else 1)
    counts = np.zeros(n, np.int32)
    channels = np.full((n, R), -1, np.int32)
    positions = np.full((n, R), -1, np.int32)
    scores = np.full((n, R), QUIET_NAN, np.float32)
    points = np.full((n, R, 2), QUIET_NAN, np.float32)
    for r in range(n):
        row = []
        for c in range(K):
            v = x[r, c].reshape(-1)
            passing = [p for p in found[r][c] if min_score is None or v[p] >= np.float32(min_score)]       # rule 2
            row += [(float(v[p]), c * H * W + p) for p in passing[:M]]                                      # rule 3
        row = sorted(row, key=order)[:R]                                                                    # rule 4
        counts[r] = len(row)
        for slot, (_, index) in enumerate(row):
            c, p = index // (H * W), index % (H * W)
            v = x[r, c]
            py, px = p // W, p % W
            channels[r, slot], positions[r, slot] = c, p
            scores.view(np.uint32)[r, slot] = v.view(np.uint32)[py, px]                                     # the bits, whatever they say
            ox = oy = np.float32(0.0)
            if refine == 'QUARTER':
                if 1 <= px <= W - 2:
                    ox = _quarter(v[py, px - 1], v[py, px + 1])
                if 1 <= py <= H - 2:
                    oy = _quarter(v[py - 1, px], v[py + 1, px])
            fx, fy = np.float32(px) + ox, np.float32(py) + oy
            if space == 'NORMALISED':
                fx = np.float32(np.float64(fx + np.float32(0.5)) / np.float64(W))
                fy = np.float32(np.float64(fy + np.float32(0.5)) / np.float64(H))
            points[r, slot] = (fx, fy)
    return Maxima(counts, channels, positions, scores, points)
