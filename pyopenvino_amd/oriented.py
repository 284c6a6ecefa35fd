"""An oriented detector head's answer (``infer(..., boxes=OrientedBoxScreen(...))``): the rule, the argument checks and the device launch.
Heads whose graph ends in a raw tensor of per-anchor rotated boxes: YOLOv8 / v11-obb exports (n, 4 + C + 1, A), e.g. (n, 20, 21504) for
DOTA at 1024 x 1024 ('NCA'), and the rotated anchor-free heads of the same shape or its transpose ('NAC').  E = 4 + O + C + 1 channels per
anchor in the order cx, cy, w, h, [objectness], C class scores, angle: pixels of the network's 4-D Parameter, and radians about the centre
(from the x axis towards the y axis of the image).  The answer is an ``OrientedDetections``: its `quads` feed a ``PerspectiveInput``
(perspective.from_quad), its `boxes` a ``WarpInput`` (warp.rotated_rect) when the geometry is uniform.

The rule (include/pvhip.h, pvhip_oriented_boxes_f32; tests/oriented_ref.py is the same again in plain loops).  From step 3 on every
operation is one binary64 operation, rounded once, none contracted:
  1. winner and score  boxes.py's step 1 word for word: c* the first class in top_k's total order, score = e[4 + O + c*] or, with
     objectness, e[4] * e[4 + O + c*] as one float32 product; out when NaN or below float32(min_score).
  2. screen  cx, cy, w, h and the angle all finite, |angle| <= 8; w >= float32(min_size[1]) and h >= float32(min_size[0]), in network
     pixels; c* listed when `labels` is given.  selected[r] counts the anchors still in.
  3. cosine and sine  a = float64(angle); k = rint(a * 0.6366197723675814); r = (a - k * 1.5707963267948966) - k * 6.123233995736766e-17;
     z = r * r; s = r + r * (z * S(z)) with S the Horner form in z of -1/3!, +1/5!, ..., +1/17!; c = 1 + z * C(z) with C that of -1/2!,
     +1/4!, ..., +1/16!; each coefficient the correctly rounded double of the rational.  By k & 3: (cos, sin) = (c, s), (-s, c), (-c, -s),
     (s, -c).  (The device library's and numpy's own differ in the last bit, so the rule has its own.)
  4. corners  u = ((w * 0.5) * cos, (w * 0.5) * sin), v = (-((h * 0.5) * sin), (h * 0.5) * cos); p0 = ctr - u - v, p1 = ctr + u - v,
     p2 = ctr + u + v, p3 = ctr - u + v, left to right; area = float64(w) * float64(h).
  5. overlap of a later candidate i with a kept candidate j: 0 when per_label and the labels differ; 0 when dx * dx + dy * dy > R * R with
     R = ((wi + hi) + (wj + hj)) * 0.5 (a bound on the two half-diagonals without a square root: part of the rule); else the polygon of i
     clipped by the four edges (q_e, q_e+1) of j in order (Sutherland-Hodgman): side(p) = (bx - ax) * (py - ay) - (by - ay) * (px - ax),
     p inside iff side(p) >= 0; walking the polygon's edges (p, q), p is emitted when inside and, when exactly one of the two is inside,
     p + t * (q - p) with t = sp / (sp - sq) behind it; an empty polygon ends it; at most 8 vertices.  inter = |sum of (px * qy - qx * py)|
     * 0.5, summed in order from +0.  i is always the subject and j the clip: the two orders differ in the last bits.
  6. suppression  the K = max_candidates best by descending score, ties to the lower anchor, greedily: i is dropped iff an earlier kept
     j has inter > float64(threshold) * den, den = (ai + aj) - inter ('IOU') or min(ai, aj) ('IOS'); equality keeps.  An image keeps
     its first max_per_image kept ones.  All in network pixels, where the boxes are rectangles.
  7. frame   each corner coordinate goes to the frame by boxes=' map, (p - d) * F / i with the geometry boxes.geometry_of learns from the
     pass, and is then rounded to float32; not clamped (a warp pads).
Out of scope: probabilistic IoU, the 'le90' / 'oc' angle conventions (plain radians about the centre only), K above 1024, tiles and
regions, masks= on an oriented head."""
import collections
import ctypes
from fractions import Fraction
from math import factorial

import numpy as np

from . import ask, boxes, detections, device
from .boxes import LAYOUTS, AmbiguousLayout
from .tiled_detections import OVERLAPS

MAX_CANDIDATES = 1024                           # PVHIP_ORIENTED_MAX_CANDIDATES: a lane per sorted candidate
ROW_WORDS = 20                                  # PVHIP_ORIENTED_ROW_BYTES / 4
MAX_ANGLE = np.float32(8)
_SIN = [float(Fraction((-1) ** i, factorial(2 * i + 1))) for i in range(1, 9)]      # -1/3! .. +1/17!
_COS = [float(Fraction((-1) ** i, factorial(2 * i))) for i in range(1, 9)]          # -1/2! .. +1/16!

_Screen = collections.namedtuple('OrientedBoxScreen', 'min_score layout objectness frame_size labels min_size max_candidates overlap threshold '
                                                      'per_label max_per_image input')
_Answer = collections.namedtuple('OrientedDetections', 'counts selected quads boxes labels scores records')


class OrientedBoxScreen(_Screen):
    """How to read an oriented detector head's Result, and which of its boxes come back: BoxScreen's fields without `box` and `tail` --
    the channels are cx, cy, w, h, [objectness], the classes, the angle in radians --, with `max_candidates` = K <= 1024 and `min_size` =
    (h, w) compared with the box's own h and w in network pixels.  Immutable; checked when a pass is started with it (ValueError)."""
    __slots__ = ()

    def __new__(cls, min_score=0.25, layout=None, objectness=False, frame_size=None, labels=None, min_size=(1, 1), max_candidates=1024,
                overlap='IOU', threshold=0.45, per_label=True, max_per_image=None, input=None):
        frozen = [detections._frozen(v) for v in (frame_size, labels, min_size)]
        return super().__new__(cls, min_score, layout, objectness, frozen[0], frozen[1], frozen[2], max_candidates, overlap, threshold,
                               per_label, max_per_image, input)


class OrientedDetections(_Answer):
    """What an oriented head's Result started with boxes=OrientedBoxScreen(...) comes back as: `counts`, `selected` (images,) int32 as
    Detections'; `quads` (total, 4, 2) float32, the corners (x, y) in frame pixels in perspective.from_quad's order -- top-left,
    top-right, bottom-right, bottom-left of the box in its own axes --, not clamped; `boxes` (total, 5) float32, the anchor's own cx, cy,
    w, h, angle in network pixels and radians; `labels` (total,) int32; `scores` (total,) float32; `records` (total,) int32, the flat
    anchor r * A + a."""
    __slots__ = ()

    def of(self, b: int) -> tuple:
        """(quads, boxes, labels, scores, records) of image b: slices of the table."""
        images = len(self.counts)
        if not -images <= b < images:
            raise IndexError('image {} of {}'.format(b, images))
        b = b % images
        lo = int(self.counts[:b].sum())
        rows = slice(lo, lo + int(self.counts[b]))
        return self.quads[rows], self.boxes[rows], self.labels[rows], self.scores[rows], self.records[rows]


def resolved(value, what='boxes') -> OrientedBoxScreen:
    """`value`, an OrientedBoxScreen, with every value checked and in its one form, by BoxScreen's own checks; ValueError."""
    if not isinstance(value, OrientedBoxScreen):
        raise ValueError('{}: an OrientedBoxScreen, got {!r}'.format(what, value))
    if not detections._count(value.max_candidates, MAX_CANDIDATES):
        raise ValueError('{}: max_candidates of an OrientedBoxScreen is a count in 1 .. {}, got {!r}'.format(what, MAX_CANDIDATES, value.max_candidates))
    b = boxes.resolved(boxes.BoxScreen(value.min_score, value.layout, value.objectness, 'CXCYWH', *value[3:]), what)
    return OrientedBoxScreen(b.min_score, b.layout, b.objectness, *b[4:13])


def shape_of(dims, layout=None, objectness=False, batch=None):
    """(layout, n, A, C) of a tensor declared as an oriented head: boxes.shape_of with the angle as one channel behind the classes."""
    return boxes.shape_of(dims, layout, objectness, batch, 1)


# ---------------------------------------------------------------------------------------------------------------- the rule in numpy
def cos_sin(angle):
    """Step 3 on float32 angles: (cos, sin) as float64."""
    a = np.asarray(angle, np.float32).astype(np.float64)
    k = np.rint(a * 0.6366197723675814)
    r = (a - k * 1.5707963267948966) - k * 6.123233995736766e-17
    z = r * r
    S, C = np.float64(_SIN[-1]), np.float64(_COS[-1])
    for s, c in zip(_SIN[-2::-1], _COS[-2::-1]):
        S, C = s + z * S, c + z * C
    s, c = r + r * (z * S), 1.0 + z * C
    q = k.astype(np.int64) & 3
    return np.choose(q, [c, -s, -c, s]), np.choose(q, [s, c, -s, -c])


def corners(b):
    """Step 4 on (m, 5) float32 rows cx, cy, w, h, angle: ((m, 4) x, (m, 4) y, area, w + h) as float64."""
    b = np.asarray(b, np.float32).astype(np.float64).reshape(-1, 5)
    cos, sin = cos_sin(np.asarray(b[:, 4], np.float32))
    cx, cy, w, h = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    ux, uy, vx, vy = (w * 0.5) * cos, (w * 0.5) * sin, -((h * 0.5) * sin), (h * 0.5) * cos
    x = np.stack([(cx - ux) - vx, (cx + ux) - vx, (cx + ux) + vx, (cx - ux) + vx], axis=1)
    y = np.stack([(cy - uy) - vy, (cy + uy) - vy, (cy + uy) + vy, (cy - uy) + vy], axis=1)
    return x, y, w * h, w + h


def intersections(x, y, qx, qy):
    """Step 5's clip: `inter` of the m subject quadrilaterals (m, 4) x, y with the clip quadrilateral qx, qy (4,), in eight fixed vertex
    slots per subject, the slots behind a subject's count unused."""
    m = x.shape[0]
    px, py, cnt = np.zeros((m, 8)), np.zeros((m, 8)), np.full(m, 4)
    px[:, :4], py[:, :4] = x, y
    slot, rows = np.arange(8)[None, :], np.arange(m)[:, None]
    with np.errstate(all='ignore'):
        for e in range(4):
            ax, ay, bx, by = qx[e], qy[e], qx[(e + 1) & 3], qy[(e + 1) & 3]
            valid = slot < cnt[:, None]
            nxt = np.where(slot + 1 < cnt[:, None], slot + 1, 0)
            sp = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
            sq, wx, wy = sp[rows, nxt], px[rows, nxt], py[rows, nxt]
            inside, crossing = valid & (sp >= 0), valid & ((sp >= 0) != (sq >= 0))
            t = sp / (sp - sq)
            emit = np.stack([inside, crossing], axis=2).reshape(m, 16)          # p, then the crossing behind it
            ex = np.stack([px, px + t * (wx - px)], axis=2).reshape(m, 16)
            ey = np.stack([py, py + t * (wy - py)], axis=2).reshape(m, 16)
            at = np.cumsum(emit, axis=1) - 1
            emit &= at < 8
            r, c = np.nonzero(emit)
            px, py = np.zeros((m, 8)), np.zeros((m, 8))
            px[r, at[r, c]], py[r, at[r, c]] = ex[r, c], ey[r, c]
            cnt = emit.sum(axis=1)
        acc = np.zeros(m)
        nxt = np.where(slot + 1 < cnt[:, None], slot + 1, 0)
        wx, wy = px[rows, nxt], py[rows, nxt]
        for v in range(8):
            acc = np.where(v < cnt, acc + (px[:, v] * wy[:, v] - wx[:, v] * py[:, v]), acc)
    return np.abs(acc) * 0.5


def decode(x, screen, net_hw, fit=None) -> OrientedDetections:
    """The rule in numpy on a host array read as `screen.layout` (None: inferred from the shape): what a Result computed on the host (a
    foreign plugin set) gets.  `net_hw`, `fit` and frame_size None as boxes.decode's."""
    screen = resolved(screen, 'decode')
    x = np.asarray(x)
    try:
        shape = shape_of(x.shape, screen.layout, screen.objectness)
    except AmbiguousLayout as e:
        raise ValueError('decode: {}'.format(e)) from None
    if x.dtype != np.float32 or shape is None:
        raise ValueError('decode takes float32 numbers of rank 3 with E = 4 + objectness + C + 1 channels, C >= 1 and n * A * E < 2^31, got {} {}'.format(
            x.dtype, x.shape))
    if not detections._pair(tuple(net_hw), detections.MAX_EXTENT):
        raise ValueError('decode: net_hw is (Hn, Wn) with both in 1 .. 2^24, got {!r}'.format(net_hw))
    Hn, Wn = (int(v) for v in net_hw)
    dx, dy, iw, ih = (0, 0, Wn, Hn) if fit is None else boxes.checked_fit(fit)
    layout, n, A, C = shape
    fh, fw = screen.frame_size or (Hn, Wn)
    O = int(screen.objectness)
    v = x.transpose(0, 2, 1) if layout == 'NCA' else x                                   # (n, A, E)
    w, score = boxes._winners(v[:, :, 4 + O:4 + O + C])
    b = v[:, :, [0, 1, 2, 3, 4 + O + C]]
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        if O:
            score = v[:, :, 4] * score                                                       # one float32 product
        keep = (score >= np.float32(screen.min_score)) & np.isfinite(b).all(axis=2) & (np.abs(b[:, :, 4]) <= MAX_ANGLE)
        keep &= (b[:, :, 2] >= np.float32(screen.min_size[1])) & (b[:, :, 3] >= np.float32(screen.min_size[0]))
    if screen.labels is not None:
        keep &= np.isin(w, np.asarray(screen.labels, np.int64))
    K, cap, threshold = screen.max_candidates, screen.max_per_image, np.float64(screen.threshold)
    counts, selected, rows = np.zeros(n, np.int32), keep.sum(axis=1).astype(np.int32), []
    for r in range(n):
        at = np.flatnonzero(keep[r])
        order = at[np.lexsort((at, -(score[r, at] + np.float32(0))))][:K]                    # (+ 0: -0.0 becomes +0.0; lexsort is stable)
        qx, qy, area, ext = corners(b[r, order])
        cx, cy, lab = b[r, order, 0].astype(np.float64), b[r, order, 1].astype(np.float64), w[r, order]
        gone, kept = np.zeros(len(order), bool), []
        for j in range(len(order)):                                                          # 6. greedy; j is kept, the later ones are i
            if gone[j]:
                continue
            kept.append(j)
            if len(kept) == cap:
                break
            i = j + 1 + np.flatnonzero(~gone[j + 1:])
            if screen.per_label:
                i = i[lab[i] == lab[j]]
            ddx, ddy, R = cx[i] - cx[j], cy[i] - cy[j], (ext[i] + ext[j]) * 0.5
            i = i[~(ddx * ddx + ddy * ddy > R * R)]
            inter = intersections(qx[i], qy[i], qx[j], qy[j])
            den = np.minimum(area[i], area[j]) if screen.overlap == 'IOS' else (area[i] + area[j]) - inter
            gone[i[inter > threshold * den]] = True
        kept = np.asarray(kept, np.int64)
        counts[r] = len(kept)
        quad = np.stack([(qx[kept] - np.float64(dx)) * np.float64(fw) / np.float64(iw),
                         (qy[kept] - np.float64(dy)) * np.float64(fh) / np.float64(ih)], axis=2).astype(np.float32)
        rows.append((quad, b[r, order[kept]], lab[kept], score[r, order[kept]], r * A + order[kept]))
    quads, five, labels, scores, records = (np.concatenate(col) for col in zip(*rows))
    return OrientedDetections(counts, selected, quads.reshape(-1, 4, 2), five.reshape(-1, 5).astype(np.float32), labels.astype(np.int32),
                              scores.astype(np.float32), records.astype(np.int32))


# ---------------------------------------------------------------------------------------------------------------- the argument
SHAPE = 'rank 3 with the batch n = {} first, E = 4 + objectness + C + 1 channels (the angle last), C >= 1 and n * A * E < 2^31'


def _fits(port, screen, batch):
    try:
        return port['precision'] == 'FP32' and shape_of(port['dims'], screen.layout, screen.objectness, batch) is not None
    except AmbiguousLayout:
        return False


def _none_fits(ports, screen, batch):
    return 'boxes: no FP32 Result of {}{} (the Results: {})'.format(
        SHAPE.format(batch), ' whose layout can be inferred' if screen.layout is None else ' as {!r}'.format(screen.layout),
        {name: tuple(port['dims']) for name, port in ports.items()})


def _checked(ienet, value, sharded: bool) -> dict:
    """boxes.checked for an OrientedBoxScreen or a dict of them."""
    batch = int(ienet.batch_size)
    ports, wanted = ask.named(ienet, 'boxes', value, sharded, _fits, _none_fits, resolved)
    for name, screen in wanted.items():
        what = 'boxes: Result {!r}'.format(name)
        try:
            shape = shape_of(ports[name]['dims'], screen.layout, screen.objectness, batch)
        except AmbiguousLayout as e:
            raise ValueError('{}: {}'.format(what, str(e).replace('BoxScreen', 'OrientedBoxScreen'))) from None
        expected = SHAPE + (' as {!r}'.format(screen.layout) if screen.layout is not None else '')
        layout = ask.declared('boxes', name, ports[name], shape, expected, batch)[0]
        wanted[name] = screen._replace(layout=layout, input=boxes.checked_input(ienet, screen, what))
    return wanted


def checked(ienet, value, sharded: bool) -> dict:
    """{Result name: resolved BoxScreen or OrientedBoxScreen} of the `boxes` argument of infer() / start_async(): the screen's type picks
    the kind, Result by Result in a dict; everything else is boxes.checked's, refusals included."""
    if isinstance(value, OrientedBoxScreen):
        return _checked(ienet, value, sharded)
    if not isinstance(value, dict) or not any(isinstance(v, OrientedBoxScreen) for v in value.values()):
        return boxes.checked(ienet, value, sharded)
    mine = _checked(ienet, {name: v for name, v in value.items() if isinstance(v, OrientedBoxScreen)}, sharded)
    plain = {name: v for name, v in value.items() if name not in mine}
    theirs = boxes.checked(ienet, plain, sharded) if plain else {}
    return {name: mine[name] if name in mine else theirs[name] for name in value}


# ---------------------------------------------------------------------------------------------------------------- the device
def scratch_bytes(n: int, A: int, per_image: int) -> int:
    """PVHIP_ORIENTED_SCRATCH_BYTES: the (n, A) 8-byte keys, the (n, A) int32 winners, then at the next 16-byte boundary the staging rows."""
    return ((12 * n * A + 15) & ~15) + 4 * ROW_WORDS * n * per_image


class Blocks:
    """The blocks of one (Result name, screen without min_score and frame_size): the header and the rows of twenty words that
    pvhip_oriented_boxes_f32 writes, their page-locked twins, the labels on the device, and `scratch` between the entry's three
    launches.  read_back copies the header, 4 (2 n + 1) bytes, then exactly 80 total bytes."""
    __slots__ = ('n', 'A', 'screen', 'header', 'rows', 'labels', 'header_host', 'rows_host', 'scratch')
    ENTRY = 'pvhip_oriented_boxes_f32'

    def __init__(self, n: int, A: int, screen: OrientedBoxScreen):
        self.n, self.A, self.screen = n, A, screen
        capacity = n * screen.max_per_image
        self.header = device.DeviceTensor.empty((2 * n + 1,), np.int32)
        self.rows = device.DeviceTensor.empty((capacity, ROW_WORDS), np.int32)
        self.header_host = device.host_empty((2 * n + 1,), np.int32)
        self.rows_host = device.host_empty((capacity, ROW_WORDS), np.int32)
        self.labels = None if screen.labels is None else device.DeviceTensor.from_numpy(np.asarray(screen.labels + (0,), np.int32))
        self.scratch = device.DeviceTensor.empty((scratch_bytes(n, A, screen.max_per_image) // 4,), np.int32)

    def launch(self, result, min_score, frame_size, fit):
        """One call (three launches) on the current stream, behind whatever wrote `result` there, over frames of `frame_size` that stand
        in the rectangle `fit` = (dx, dy, iw, ih) of the network's input."""
        s = self.screen
        layout, n, A, C = shape_of(result.shape, s.layout, s.objectness)
        assert (n, A) == (self.n, self.A) and result.dtype == np.float32
        device.call(self.ENTRY, device.ptr(result), n, A, C, LAYOUTS[layout], int(s.objectness), min_score, device.ptr(self.labels),
                    0 if s.labels is None else len(s.labels), frame_size[0], frame_size[1], fit[0], fit[1], fit[2], fit[3], s.min_size[0],
                    s.min_size[1], s.max_candidates, OVERLAPS[s.overlap], s.threshold, int(s.per_label), s.max_per_image,
                    ctypes.c_void_p(self.scratch.ptr), ctypes.c_void_p(self.header.ptr), ctypes.c_void_p(self.rows.ptr))

    def read_back(self) -> OrientedDetections:
        """The answer, copied on the current stream, which has drained: the header, then the rows it counts; the arrays are the caller's."""
        n = self.n
        device.call('pvhip_memcpy_d2h', ctypes.c_void_p(self.header_host.ctypes.data), ctypes.c_void_p(self.header.ptr), self.header_host.nbytes)
        total = int(self.header_host[2 * n])
        if not 0 <= total <= self.rows_host.shape[0]:
            raise device.PvhipError('{} left total = {} of at most {} rows'.format(self.ENTRY, total, self.rows_host.shape[0]))
        if total:
            device.call('pvhip_memcpy_d2h', ctypes.c_void_p(self.rows_host.ctypes.data), ctypes.c_void_p(self.rows.ptr), 4 * ROW_WORDS * total)
        t = self.rows_host[:total]              # (image, label, score bits, record, cx, cy, w, h, angle, eight corner numbers, 0, 0, 0)
        return OrientedDetections(self.header_host[:n].copy(), self.header_host[n:2 * n].copy(), t[:, 9:17].copy().view(np.float32).reshape(-1, 4, 2),
                                  t[:, 4:9].copy().view(np.float32), t[:, 1].copy(), t[:, 2].copy().view(np.float32), t[:, 3].copy())


class Ask(ask.Ask, collections.namedtuple('Ask', 'screen net_hw format frame_size fit')):
    """A Result asked for with boxes= and an OrientedBoxScreen, resolved: boxes.Ask's fields and its way of learning the pass's geometry."""
    __slots__ = ()
    KEYWORD = 'boxes'
    bound, key, launch_with = boxes.Ask.bound, boxes.Ask.key, boxes.Ask.launch_with

    def blocks_for(self, value):
        _, n, A, _ = shape_of(value.shape, self.screen.layout, self.screen.objectness)
        return Blocks(n, A, self.screen._replace(min_score=None, frame_size=None))

    def on_host(self, value):
        return decode(value, self.screen._replace(frame_size=self.frame_size), self.net_hw, self.fit)
