"""The rule of ``components=`` (include/pvhip.h, pvhip_components_f32) in plain loops over Python ints: a flood fill per plane, then the
statistics.  Written from the rule's text; it does not import pyopenvino_amd.components."""
import collections
import math

import numpy as np

Components = collections.namedtuple('Components', 'counts found rois areas seeds peaks sums moments')


def _order(value: float):
    """top_k's order among numbers: descending, +0.0 == -0.0."""
    return 0.0 if value == 0 else value


def _q16(value: float) -> int:
    scaled = min(max(float(value), -32768.0), 32768.0) * 65536.0        # exact in float64
    low = math.floor(scaled)
    if scaled - low == 0.5:
        return low if low % 2 == 0 else low + 1
    return low + 1 if scaled - low > 0.5 else low


def components(x, min_score, channel=0, connectivity=8, min_area=1, max_per_image=256) -> Components:
    x = np.asarray(x, np.float32)
    n, K, H, W = x.shape
    cut = float(np.float32(min_score))
    steps = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connectivity == 8 else [])
    counts, found, rows = [], [], []
    for r in range(n):
        plane = [[float(v) for v in line] for line in x[r, channel]]
        bits = x[r, channel].view(np.uint32)
        seen = [[not (plane[y][xx] >= cut) for xx in range(W)] for y in range(H)]       # (a NaN compares false: background)
        every = []
        for y0 in range(H):
            for x0 in range(W):
                if seen[y0][x0]:
                    continue
                seen[y0][x0] = True
                stack, pixels = [(y0, x0)], []
                while stack:
                    y, xx = stack.pop()
                    pixels.append((y, xx))
                    for dy, dx in steps:
                        v, u = y + dy, xx + dx
                        if 0 <= v < H and 0 <= u < W and not seen[v][u]:
                            seen[v][u] = True
                            stack.append((v, u))
                pixels.sort()                                                             # raster order
                best = max(_order(plane[y][xx]) for y, xx in pixels)
                py, px = next((y, xx) for y, xx in pixels if _order(plane[y][xx]) == best)
                xs, ys = [xx for _, xx in pixels], [y for y, _ in pixels]
                every.append(dict(area=len(pixels), seed=y0 * W + x0, peak=int(bits[py, px]),
                                  roi=(r, min(xs), min(ys), max(xs) - min(xs) + 1, max(ys) - min(ys) + 1),
                                  sum=sum(_q16(plane[y][xx]) for y, xx in pixels),
                                  moments=(sum(xs), sum(ys), sum(v * v for v in xs), sum(y * xx for y, xx in pixels), sum(v * v for v in ys))))
        kept = sorted((c for c in every if c['area'] >= min_area), key=lambda c: (-c['area'], c['seed']))[:max_per_image]
        found.append(len(every))
        counts.append(len(kept))
        rows += kept
    peaks = np.array([c['peak'] for c in rows], np.uint32).view(np.float32)
    return Components(np.array(counts, np.int32), np.array(found, np.int32), np.array([c['roi'] for c in rows], np.int32).reshape(-1, 5),
                      np.array([c['area'] for c in rows], np.int32), np.array([c['seed'] for c in rows], np.int32), peaks,
                      np.array([c['sum'] for c in rows], np.int64), np.array([c['moments'] for c in rows], np.int64).reshape(-1, 5))
