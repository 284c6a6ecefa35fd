"""The rule of ``infer(..., maxima=..., poses=...)`` (pvhip_pose_groups_f32) in plain loops.  This is the specification; the kernels and
pyopenvino_amd/poses.py equal it bit for bit.  Every operation is one float32 operation, rounded once.

Rules 1 to 5 are stated in pyopenvino_amd/poses.py; here they are code: candidates by tests/maxima_ref.py (a plane as a row), every pair of a
limb scored sample by sample, the valid ones sorted by (score bits descending, i, j) and taken greedily, the limbs walked in order."""
import collections

import numpy as np

import maxima_ref

Poses = collections.namedtuple('Poses', 'counts joints scores points totals')
F = np.float32
QUIET_NAN = maxima_ref.QUIET_NAN


def poses(heat, pafs, skeleton, min_score=None, max_per_plane=20, refine='QUARTER', space='NORMALISED', samples=10, min_field=0.05,
          min_samples=8, max_persons=32, min_joints=3, min_mean=0.2):
    n, K, H, W = heat.shape
    M, P, S = max_per_plane, max_persons, samples
    assert heat.dtype == pafs.dtype == np.float32 and pafs.shape[0::2] == heat.shape[0::2] and pafs.shape[3] == W and M <= 32 and 2 <= S <= 16
    cand = maxima_ref.maxima(heat.reshape(n * K, 1, H, W), min_score, M, M, refine, space)          # rule 1: a plane as a row
    out = Poses(np.zeros(n, np.int32), np.full((n, P, K), -1, np.int32), np.full((n, P, K), QUIET_NAN, np.float32),
                np.full((n, P, K, 2), QUIET_NAN, np.float32), np.full((n, P), QUIET_NAN, np.float32))
    for r in range(n):
        persons = []                                            # [{joint: candidate}, total]
        for a, b, cx, cy, founds in skeleton:
            valid = []
            for i in range(cand.counts[r * K + a]):
                for j in range(cand.counts[r * K + b]):
                    pa, pb = int(cand.positions[r * K + a, i]), int(cand.positions[r * K + b, j])
                    ax, ay, dx, dy = pa % W, pa // W, pb % W - pa % W, pb // W - pa // W
                    if dx == 0 and dy == 0:
                        continue
                    length = np.sqrt(F(dx * dx + dy * dy))
                    ux, uy = F(dx) / length, F(dy) / length
                    c, total = 0, F(0)
                    for s in range(S):
                        x, y = ax + (2 * s * dx + (S - 1)) // (2 * (S - 1)), ay + (2 * s * dy + (S - 1)) // (2 * (S - 1))
                        with np.errstate(all='ignore'):
                            v = pafs[r, cx, y, x] * ux + pafs[r, cy, y, x] * uy
                        if v > F(min_field):
                            c, total = c + 1, total + v
                    if c >= min_samples:
                        valid.append((-int(np.array(total / F(c), np.float32).view(np.uint32)), i, j))
            used_a, used_b = set(), set()
            for bits, i, j in sorted(valid):                    # rule 3
                if i in used_a or j in used_b:
                    continue
                used_a.add(i)
                used_b.add(j)
                score = np.array(-bits, np.uint32).view(np.float32)[()]
                heat_a, heat_b = cand.scores[r * K + a, i], cand.scores[r * K + b, j]
                holders = [p for p in persons if p[0].get(a) == i]
                if holders:
                    if b not in holders[0][0]:
                        holders[0][0][b] = j
                        holders[0][1] = (holders[0][1] + heat_b) + score
                elif founds and len(persons) < P:
                    persons.append([{a: i, b: j}, (heat_a + heat_b) + score])
        with np.errstate(all='ignore'):
            kept = [p for p in persons if len(p[0]) >= min_joints and p[1] / F(len(p[0])) >= F(min_mean)]
        out.counts[r] = len(kept)
        for q, (slots, total) in enumerate(kept):
            out.totals[r, q] = total
            for k, c in slots.items():
                out.joints[r, q, k] = cand.positions[r * K + k, c]
                out.scores.view(np.uint32)[r, q, k] = cand.scores.view(np.uint32)[r * K + k, c]
                out.points[r, q, k] = cand.points[r * K + k, c]
    return out
