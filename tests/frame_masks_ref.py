"""The frame-mask rule of include/pvhip.h (pvhip_frame_masks_f32) again, written from its text; pyopenvino_amd/masks.py is not
imported.  Positions are Python's exact integers, values numpy float32 scalars and rows; fmaf is gallery_ref's."""
import numpy as np

from gallery_ref import fmaf


def tap(X, d, i, F, P, N):
    """Rule 2 for one frame position: (first tap, second tap, fraction)."""
    p = (((2 * d * F + (2 * X + 1) * i) * P - F * N) * 65536) // (2 * F * N)            # (// floors toward minus infinity)
    x0 = p >> 16
    return min(max(x0, 0), P - 1), min(max(x0 + 1, 0), P - 1), np.float32(p & 65535) / np.float32(65536)


def offsets(rois, frame):
    out = [0]
    for _, x, y, w, h in np.asarray(rois).tolist():
        inside = x >= 0 and w >= 1 and x + w <= frame[1] and y >= 0 and h >= 1 and y + h <= frame[0]
        out.append(out[-1] + (h * ((w + 31) // 32) if inside else 0))
    return np.asarray(out, np.int64)


def frame_masks(head, layout, tail, protos, rois, records, net_hw, frame, fit, max_words):
    """(words, offsets, made) for the rows `rois` (total, 5) with records r * A + a of `head` as `layout`."""
    n, T, hp, wp = protos.shape
    v = head.transpose(0, 2, 1) if layout == 'NCA' else head                # (n, A, E)
    (hn, wn), (fh, fw), (dx, dy, iw, ih) = net_hw, frame, fit
    assert T == tail
    at = offsets(rois, frame)
    made = max(m for m in range(len(at)) if at[m] <= max_words)
    words = np.zeros(int(at[made]), np.uint32)
    for j in range(made):
        r, x, y, w, h = (int(c) for c in rois[j])
        m = v[r, int(records[j]) - r * v.shape[1], -T:]
        if at[j + 1] == at[j] or not np.isfinite(m).all():
            continue                                                        # no words, or zeros
        with np.errstate(all='ignore'):
            L = np.zeros((hp, wp), np.float32)
            for t in range(T):
                L = fmaf(np.full((hp, wp), m[t], np.float32), protos[r, t], L)
            L[~np.isfinite(protos[r]).all(axis=0)] = np.nan
            cols = [tap(X, dx, iw, fw, wp, wn) for X in range(x, x + w)]
            xa, xb, fx = [c[0] for c in cols], [c[1] for c in cols], np.asarray([c[2] for c in cols], np.float32)
            for Y in range(y, y + h):
                ya, yb, fy = tap(Y, dy, ih, fh, hp, hn)
                t0 = L[ya, xa] + fx * (L[ya, xb] - L[ya, xa])
                t1 = L[yb, xa] + fx * (L[yb, xb] - L[yb, xa])
                on = np.flatnonzero(t0 + fy * (t1 - t0) > 0)
                base = int(at[j]) + (Y - y) * ((w + 31) // 32)
                for c in on.tolist():
                    words[base + (c >> 5)] |= np.uint32(1 << (c & 31))
    return words, at, made
