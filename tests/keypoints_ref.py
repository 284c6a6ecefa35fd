"""The rule of ``infer(..., keypoints=...)`` (pvhip_heatmap_peaks_f32) in plain loops.  This is the specification; the kernel and
pyopenvino_amd/keypoints.py equal it bit for bit.

For the plane v[0..H)[0..W) of batch row r and channel c of a float32 (n, K, H, W) stack of heatmaps:
  1. peak    p is the first position of the plane's H * W values in top_k's total order: NaN of any sign or payload first, then
     descending with +0.0 == -0.0, ties to the lower flat index.  py = p // W, px = p % W.  positions[r][c] = p; scores[r][c] holds the
     plane's own bits at the peak.
  2. valid   the keypoint is valid iff its score is not NaN and (min_score is None or score >= float32(min_score)).
  3. refine  'NONE': ox = oy = 0.  'QUARTER': if 1 <= px <= W - 2, with l = v[py][px - 1] and r = v[py][px + 1], ox = +0.25 if r > l,
     -0.25 if r < l, else 0 (equal values, zeros of either sign, either neighbour NaN); on the plane's first or last column ox = 0.  oy
     likewise in y with H.  fx = float32(px) + ox, fy = float32(py) + oy in fp32.
  4. space   'HEATMAP': (fx, fy).  'NORMALISED': x = float32(float64(fx + float32(0.5)) / float64(W)), y likewise with fy and H.
     points[r][c] = (x, y); a void keypoint's are two quiet NaNs 0x7FC00000.
counts[r] is the number of valid keypoints of row r."""
import collections

import numpy as np

Keypoints = collections.namedtuple('Keypoints', 'counts points scores positions')
QUIET_NAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def peak_of(values):
    """Rule 1 on one plane given as a flat list of Python floats (every float32 is one exactly)."""
    best, top = 0, values[0]
    if top != top:
        return 0
    for i in range(1, len(values)):
        v = values[i]
        if v != v:                      # the first NaN: before every number
            return i
        if v > top:                     # strictly: ties, and zeros of either sign, stay with the lower index
            best, top = i, v
    return best


def positions(x):
    """Rule 1 for every plane of float32 `x` (n, K, H, W): (n, K) int32.  It depends on nothing of the screen: compute it once per tensor."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4 and x.shape[2] * x.shape[3] >= 2
    n, K, H, W = x.shape
    return np.array([[peak_of(x[r, c].reshape(-1).tolist()) for c in range(K)] for r in range(n)], np.int32).reshape(n, K)


def _quarter(before, after):
    if after > before:
        return np.float32(0.25)
    if after < before:
        return np.float32(-0.25)
    return np.float32(0.0)


def keypoints(x, min_score=None, refine='QUARTER', space='NORMALISED', at=None):
    """Keypoints(counts (n,) int32, points (n, K, 2) float32, scores (n, K) float32, positions (n, K) int32) of float32 `x` (n, K, H, W);
    `at`: positions(x), when the caller has them already."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4 and refine in ('NONE', 'QUARTER') and space in ('HEATMAP', 'NORMALISED')
    n, K, H, W = x.shape
    at = positions(x) if at is None else at
    counts = np.zeros(n, np.int32)
    points = np.full((n, K, 2), QUIET_NAN, np.float32)
    scores = np.empty((n, K), np.float32)
    for r in range(n):
        for c in range(K):
            v = x[r, c]
            p = int(at[r, c])
            py, px = p // W, p % W
            score = v[py, px]
            scores.view(np.uint32)[r, c] = v.view(np.uint32)[py, px]        # the bits, whatever they say
            if np.isnan(score) or (min_score is not None and not score >= np.float32(min_score)):
                continue
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
            points[r, c] = (fx, fy)
            counts[r] += 1
    return Keypoints(counts, points, scores, at.astype(np.int32).reshape(n, K))
