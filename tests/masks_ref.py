"""The instance-mask rule of include/pvhip.h (pvhip_instance_masks_f32) again, written from its text in plain loops;
pyopenvino_amd/masks.py is not imported.  fmaf is gallery_ref's, which test_gallery.py holds against exact rationals."""
import numpy as np

from gallery_ref import fmaf


def corners(b, box):
    b = [np.float32(v) for v in b]
    with np.errstate(all='ignore'):
        if box == 'CXCYWH':
            hw, hh = b[2] * np.float32(0.5), b[3] * np.float32(0.5)
            return b[0] - hw, b[0] + hw, b[1] - hh, b[1] + hh
    return b[0], b[2], b[1], b[3]


def masks(head, layout, box, tail, protos, images, records, net_hw, crop=True):
    """(total, W32) uint32: row j for image images[j] and record records[j] = r * A + a of `head` as `layout`; the tail: an anchor's last `tail` channels."""
    n, T, hp, wp = protos.shape
    v = head.transpose(0, 2, 1) if layout == 'NCA' else head                # (n, A, E)
    A, hw, (hn, wn) = v.shape[1], hp * wp, net_hw
    assert T == tail
    e = np.stack([v[int(r), int(record) - int(r) * A] for r, record in zip(images, records)]) if len(records) else np.zeros((0, v.shape[2]), np.float32)
    planes = protos.reshape(n, T, hw)
    L = np.zeros((len(records), hw), np.float32)
    for t in range(T):                                                      # the chain, for every detection and pixel at once
        L = fmaf(np.broadcast_to(e[:, -T + t, None], L.shape), planes[list(map(int, images)), t], L)
    void = ~np.isfinite(planes).all(axis=1)                                 # (n, hw)
    out = np.zeros((len(records), (hw + 31) // 32), np.uint32)
    for j, r in enumerate(images):
        if not np.isfinite(e[j, -T:]).all():
            continue                                                        # an empty mask
        xa, xb, ya, yb = (float(c) for c in corners(e[j, :4], box))
        for q in range(hw):
            py, px = divmod(q, wp)
            on = L[j, q] > 0 and not void[int(r), q]
            if on and crop:
                on = xa * wp <= px * wn < xb * wp and ya * hp <= py * hn < yb * hp
            if on:
                out[j, q >> 5] |= np.uint32(1 << (q & 31))
    return out
