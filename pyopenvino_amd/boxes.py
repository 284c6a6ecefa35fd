"""A dense detector head's answer (``infer(..., boxes=...)``): the rule, the argument checks and the device launch.
Heads whose graph ends in a raw tensor of per-anchor boxes and class scores, decoded and suppressed outside the graph: YOLOv8 / v11
exports (n, 4 + C, A), e.g. (n, 84, 8400) ('NCA'); YOLOv5 / v7 exports (n, A, 5 + C) with an objectness column, e.g. (n, 25200, 85)
('NAC'); YOLOX, NanoDet-style and anchor-free heads of the same two shapes.  E = 4 + O + C channels per anchor (O = 1 iff `objectness`), the
first four the box, in pixels of the network's single 4-D Parameter (Hn, Wn).  The answer is detections.py's ``Detections``: its `rois`
feed a ``RoiInput``.

The rule (include/pvhip.h, pvhip_dense_boxes_f32; tests/boxes_ref.py is the same again in plain loops), for image r and anchor a with
channel values e[0 .. E - 1]:
  1. winner  c* is the first of the C class scores e[4 + O ..] in top_k's total order: NaN of any sign or payload first, then descending
     with +0.0 == -0.0, ties to the lower class.  score = e[4 + O + c*], or, with objectness, e[4] * e[4 + O + c*] as one float32
     product.  The anchor is out iff the score is NaN or below float32(min_score); equality keeps.  Any NaN among an anchor's class
     scores drops it: the quiet-NaN rows behind `count` of a DetectedRois or LandmarkWarps pass have counts = selected = 0.  On numbers
     in [0, 1] this is YOLOv5's obj * cls > conf with argmax and YOLOv8's cls.max() > conf.
  2. box     all four box numbers finite, else the anchor is out.  'CXCYWH' corners in float32: xa = cx - w * 0.5, xb = cx + w * 0.5,
     ya and yb alike; 'XYXY': the numbers themselves.  With (dx, dy, iw, ih) the geometry of the pass a corner p maps to the frame in
     binary64 as t = ((double)p - (double)d) * (double)F / (double)i, three operations each rounded once, (d, i, F) = (dx, iw, frame_w)
     for an x corner and (dy, ih, frame_h) for a y corner.  The geometry is the identity (0, 0, Wn, Hn) unless the input declares a
     resize_fit and the pass was fed host frames: then it is InputFormat.fit_geometry(extent of the frames), and frame_size None means
     that extent.  x0 = floor(min(max(t(xa), 0), frame_w)), x1 = ceil(min(max(t(xb), 0), frame_w)), w = x1 - x0; y alike.  Out when
     w < min_size[1] or h < min_size[0] (an inverted box is), and, with `labels`, unless c* is listed.  Binary64 on purpose, unlike
     DetectionScreen's float32 rule, whose inputs are normalised: with the identity geometry and frames of the network's extent
     p * F / F is p itself, so a box on integer pixel edges comes back on those edges.
  3. cap     selected[r] counts the anchors still in; the K = max_candidates best go on: descending score with +0.0 == -0.0, ties to
     the lower anchor.
  4. suppression  greedy in that order by TiledScreen's rule word for word (tiled_detections.py): int64 areas of the frame rectangles,
     den the union ('IOU') or the smaller area ('IOS'), dropped iff an earlier kept one -- of the same c* when per_label -- overlaps
     it with float64(inter) > float64(threshold) * float64(den); equality keeps.
  5. table   image r keeps its first counts[r] = min(kept, max_per_image) kept candidates; rows (r, x0, y0, w, h, c*, score bits,
     r * A + a) in (image, order of 3) order without gaps; total = sum(counts).
Where this differs from Ultralytics' post-processing: suppression runs on the integer frame rectangles, not on float network boxes; an
anchor has one class, its best, and never yields several candidates (no multi_label); class-aware suppression is by equality of the labels,
not by offsetting the coordinates per class.  Out of scope: several Results of one detector merged (v3 / v4 per-scale grids with anchors
and sigmoid / exp decoding, RegionYolo), multi-label candidates, normalised box units, rotated boxes, mask coefficients and keypoint
channels, FP16 Results, K above 4096, merging across tiles or regions, a RoiInput feed on a fitted input."""
import collections
import ctypes

import numpy as np

from . import ask, detections, device
from .detections import Detections
from .tiled_detections import OVERLAPS, _overlap

MAX_CANDIDATES = 4096                           # PVHIP_BOXES_MAX_CANDIDATES
LAYOUTS = {'NCA': 0, 'NAC': 1}                  # PVHIP_BOXES_LAYOUT_*
BOXES = {'CXCYWH': 0, 'XYXY': 1}                # PVHIP_BOXES_*
FORM_NONE, FORM_PLANES, FORM_ROWS_TEAM, FORM_ROWS_WAVE = 0, 1, 2, 3      # PVHIP_BOXES_FORM_*

_Screen = collections.namedtuple('BoxScreen', 'min_score layout objectness box frame_size labels min_size max_candidates overlap threshold '
                                              'per_label max_per_image input')


class BoxScreen(_Screen):
    """How to read a dense detector head's Result, and which of its boxes come back: anchors whose score is at least `min_score`;
    `layout` 'NCA' (n, E, A), 'NAC' (n, A, E) or None, which takes the longer of the two axes for the anchors; `objectness`: a fifth
    column multiplies the class score; `box` 'CXCYWH' or 'XYXY', in pixels of the network's input; rectangles over frames of `frame_size`
    = (H, W) (None: the network's extent, or that of the host frames a fitted input was fed); `labels`: None (any) or at most 64 class
    indices; rectangles of at least `min_size` = (h, w); the `max_candidates` = K <= 4096 best per image are suppressed greedily by
    `overlap` 'IOU' or 'IOS' above `threshold`, among equal classes when `per_label`; at most `max_per_image` (None: K) per image;
    `input` names the 4-D Parameter when the network has several.  Immutable; checked when a pass is started with it (ValueError)."""
    __slots__ = ()

    def __new__(cls, min_score=0.25, layout=None, objectness=False, box='CXCYWH', frame_size=None, labels=None, min_size=(1, 1),
                max_candidates=1024, overlap='IOU', threshold=0.45, per_label=True, max_per_image=None, input=None):
        frozen = [detections._frozen(v) for v in (frame_size, labels, min_size)]
        return super().__new__(cls, min_score, layout, objectness, box, frozen[0], frozen[1], frozen[2], max_candidates, overlap, threshold,
                               per_label, max_per_image, input)


class AmbiguousLayout(ValueError):
    """dims[1] == dims[2]: 'NCA' and 'NAC' fit alike."""


def resolved(value, what='boxes') -> BoxScreen:
    """`value` -- a BoxScreen, a real number (its min_score) or True (the default screen) -- with every value checked and in its one form
    (layout and frame_size may still be None: they depend on the Result and on the pass; `input` is the caller's: checked() knows the
    network); ValueError."""
    if value is True:
        value = BoxScreen()
    elif not isinstance(value, (bool, BoxScreen)) and isinstance(value, (int, float, np.integer, np.floating)):
        value = BoxScreen(value)
    if not isinstance(value, BoxScreen):
        raise ValueError('{}: a BoxScreen, a min_score or True, got {!r}'.format(what, value))
    min_score, layout, objectness, box, frame, labels, size, cand, overlap, threshold, per_label, cap, name = value
    if min_score is None:
        raise ValueError('{}: min_score is a finite real (of float32), got None'.format(what))
    min_score = ask.checked_min_score(min_score, what)
    if layout is not None and not (isinstance(layout, str) and layout in LAYOUTS):
        raise ValueError('{}: layout {!r} is not None or one of {}'.format(what, layout, sorted(LAYOUTS)))
    if not isinstance(objectness, (bool, np.bool_)):
        raise ValueError('{}: objectness is a bool, got {!r}'.format(what, objectness))
    if not isinstance(box, str) or box not in BOXES:
        raise ValueError('{}: box is \'CXCYWH\' or \'XYXY\', got {!r}'.format(what, box))
    if frame is not None and not detections._pair(frame, detections.MAX_EXTENT):
        raise ValueError('{}: frame_size is None or (H, W) with both in 1 .. 2^24, got {!r}'.format(what, frame))
    if labels is not None:
        if not isinstance(labels, tuple) or len(labels) > detections.MAX_LABELS or not all(
                not isinstance(l, bool) and isinstance(l, (int, np.integer)) and -2 ** 31 <= l < 2 ** 31 for l in labels):
            raise ValueError('{}: labels is None or at most {} ints, got {!r}'.format(what, detections.MAX_LABELS, labels))
        labels = tuple(int(l) for l in labels)
    if not detections._pair(size, detections._INT32_MAX):
        raise ValueError('{}: min_size is (h, w) with both >= 1, got {!r}'.format(what, size))
    if not detections._count(cand, MAX_CANDIDATES):
        raise ValueError('{}: max_candidates is a count in 1 .. {}, got {!r}'.format(what, MAX_CANDIDATES, cand))
    if not isinstance(overlap, str) or overlap not in OVERLAPS:
        raise ValueError('{}: overlap is \'IOU\' or \'IOS\', got {!r}'.format(what, overlap))
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or not 0 <= threshold <= 1:
        raise ValueError('{}: threshold {!r} is not a finite number in [0, 1]'.format(what, threshold))
    if not isinstance(per_label, (bool, np.bool_)):
        raise ValueError('{}: per_label is a bool, got {!r}'.format(what, per_label))
    if cap is None:
        cap = cand
    if not detections._count(cap, int(cand)):
        raise ValueError('{}: max_per_image is None or a count in 1 .. max_candidates = {}, got {!r}'.format(what, cand, cap))
    return BoxScreen(min_score, layout, bool(objectness), box, None if frame is None else (int(frame[0]), int(frame[1])), labels,
                     (int(size[0]), int(size[1])), int(cand), overlap, float(np.float32(threshold)), bool(per_label), int(cap), name)


def shape_of(dims, layout=None, objectness=False, batch=None):
    """(layout, n, A, C) of a tensor declared as a dense head -- rank 3, E = 4 + O + C channels with C >= 1, A >= 1, n * A * E < 2^31, n
    the batch (when given) --, else None.  `layout` None infers it: 'NCA' when dims[1] < dims[2], 'NAC' when dims[1] > dims[2];
    AmbiguousLayout, a ValueError, when they are equal."""
    dims = tuple(int(d) for d in dims)
    if len(dims) != 3:
        return None
    if layout is None:
        if dims[1] == dims[2]:
            raise AmbiguousLayout('shape {} reads as \'NCA\' and as \'NAC\': say which with BoxScreen(layout=...)'.format(dims))
        layout = 'NCA' if dims[1] < dims[2] else 'NAC'
    n, A, E = (dims[0], dims[2], dims[1]) if layout == 'NCA' else dims
    C = E - 4 - int(bool(objectness))
    if n < 1 or A < 1 or C < 1 or n * A * E >= 1 << 31 or (batch is not None and n != int(batch)):
        return None
    return layout, n, A, C


def _winners(v):
    """(class, score) of rule 1's first step on (..., C) scores: the first NaN where there is one, else the first of the largest values
    (argmax takes +0.0 == -0.0 and the lower class)."""
    nan = np.isnan(v)
    w = np.where(nan.any(axis=-1), nan.argmax(axis=-1), np.where(nan, -np.inf, v).argmax(axis=-1))
    return w, np.take_along_axis(v, w[..., None], axis=-1)[..., 0]


def decode(x, screen, net_hw, fit=None) -> Detections:
    """The rule in numpy on a host array read as `screen.layout` (None: inferred from the shape): what a Result computed on the host (a
    foreign plugin set) gets.  `net_hw` = (Hn, Wn), the extent of the network's input; `fit`: None (the identity) or (dx, dy, iw, ih),
    the rectangle of that input the frames were fitted into; frame_size None: the network's extent."""
    screen = resolved(screen, 'decode')
    x = np.asarray(x)
    try:
        shape = shape_of(x.shape, screen.layout, screen.objectness)
    except AmbiguousLayout as e:
        raise ValueError('decode: {}'.format(e)) from None
    if x.dtype != np.float32 or shape is None:
        raise ValueError('decode takes float32 numbers of rank 3 with E = 4 + objectness + C channels, C >= 1 and n * A * E < 2^31, got {} {}'.format(
            x.dtype, x.shape))
    if not detections._pair(tuple(net_hw), detections.MAX_EXTENT):
        raise ValueError('decode: net_hw is (Hn, Wn) with both in 1 .. 2^24, got {!r}'.format(net_hw))
    Hn, Wn = (int(v) for v in net_hw)
    dx, dy, iw, ih = (0, 0, Wn, Hn) if fit is None else checked_fit(fit)
    layout, n, A, C = shape
    fh, fw = screen.frame_size or (Hn, Wn)
    O = int(screen.objectness)
    v = x.transpose(0, 2, 1) if layout == 'NCA' else x                                   # (n, A, E)
    w, score = _winners(v[:, :, 4 + O:])
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        if O:
            score = v[:, :, 4] * score                                                       # one float32 product
        keep = score >= np.float32(screen.min_score)                                         # (false for NaN)
        b = v[:, :, :4]
        keep &= np.isfinite(b).all(axis=2)
        b = np.where(keep[:, :, None], b, np.float32(0))
        if screen.box == 'CXCYWH':
            hw, hh = b[:, :, 2] * np.float32(0.5), b[:, :, 3] * np.float32(0.5)
            xa, xb, ya, yb = b[:, :, 0] - hw, b[:, :, 0] + hw, b[:, :, 1] - hh, b[:, :, 1] + hh
        else:
            xa, ya, xb, yb = (b[:, :, i] for i in range(4))

        def edge(p, d, F, i, rounded):
            t = (p.astype(np.float64) - np.float64(d)) * np.float64(F) / np.float64(i)
            return rounded(np.minimum(np.maximum(t, 0.0), np.float64(F))).astype(np.int64)

        x0, y0 = edge(xa, dx, fw, iw, np.floor), edge(ya, dy, fh, ih, np.floor)
        bw, bh = edge(xb, dx, fw, iw, np.ceil) - x0, edge(yb, dy, fh, ih, np.ceil) - y0
    keep &= (bw >= screen.min_size[1]) & (bh >= screen.min_size[0])
    if screen.labels is not None:
        keep &= np.isin(w, np.asarray(screen.labels, np.int64))
    K, cap, counts, selected, rows = screen.max_candidates, screen.max_per_image, np.zeros(n, np.int32), keep.sum(axis=1).astype(np.int32), []
    bits = score.view(np.uint32)
    for r in range(n):
        at = np.flatnonzero(keep[r])
        order = at[np.lexsort((at, -(score[r, at] + np.float32(0))))][:K]                    # (+ 0: -0.0 becomes +0.0; lexsort is stable)
        rect = np.stack([x0[r, order], y0[r, order], bw[r, order], bh[r, order]], axis=1).astype(np.int64)
        gone, kept = np.zeros(len(order), bool), []
        for i in range(len(order)):                                                          # 4. greedy, 5. the first `cap` kept
            if gone[i]:
                continue
            kept.append(order[i])
            if len(kept) == cap:
                break
            hit = _overlap(rect[i], rect[i + 1:], screen.overlap, screen.threshold)
            if screen.per_label:
                hit &= w[r, order[i + 1:]] == w[r, order[i]]
            gone[i + 1:] |= hit
        kept = np.asarray(kept, np.int64)
        counts[r] = len(kept)
        rows.append(np.stack([np.full(len(kept), r, np.int64), x0[r, kept], y0[r, kept], bw[r, kept], bh[r, kept], w[r, kept],
                              bits[r, kept].astype(np.int64), r * A + kept], axis=1))
    t = np.concatenate(rows).reshape(-1, 8)
    return Detections(counts, selected, t[:, :5].astype(np.int32), t[:, 5].astype(np.int32),
                      t[:, 6].astype(np.uint32).view(np.float32), t[:, 7].astype(np.int32))


def checked_fit(fit, what='decode'):
    """`fit` as four ints (dx, dy, iw, ih), dx, dy in 0 .. 2^24 and iw, ih in 1 .. 2^24; ValueError."""
    try:
        g = tuple(fit)
        ok = len(g) == 4 and all(not isinstance(v, bool) and isinstance(v, (int, np.integer)) for v in g)
    except TypeError:
        ok = False
    if ok:
        g = tuple(int(v) for v in g)
        ok = 0 <= g[0] <= detections.MAX_EXTENT and 0 <= g[1] <= detections.MAX_EXTENT and 1 <= g[2] <= detections.MAX_EXTENT \
            and 1 <= g[3] <= detections.MAX_EXTENT
    if not ok:
        raise ValueError('{}: fit is (dx, dy, iw, ih), a rectangle of the network\'s input, got {!r}'.format(what, fit))
    return g


SHAPE = 'rank 3 with the batch n = {} first, E = 4 + objectness + C channels, C >= 1 and n * A * E < 2^31'


def _fits(port, screen, batch):
    try:
        return port['precision'] == 'FP32' and shape_of(port['dims'], screen.layout, screen.objectness, batch) is not None
    except AmbiguousLayout:
        return False


def _none_fits(ports, screen, batch):
    return 'boxes: no FP32 Result of {}{} (the Results: {})'.format(
        SHAPE.format(batch), ' whose layout can be inferred' if screen.layout is None else ' as {!r}'.format(screen.layout),
        {name: tuple(port['dims']) for name, port in ports.items()})


def checked_input(ienet, screen, what='boxes') -> str:
    """The name of the 4-D Parameter whose extent the box numbers stand in: `screen.input`, or the network's only one; ValueError."""
    names = [name for nid, name in ienet.find_node_by_type('Parameter') if len(ienet.G.nodes[nid]['data']['shape']) == 4]
    if screen.input is None:
        if len(names) != 1:
            raise ValueError('{}: the network has {} 4-D Parameters ({}): input= names the one whose pixels the boxes stand in'.format(
                what, len(names), sorted(names)))
        return names[0]
    if not isinstance(screen.input, str) or screen.input not in names:
        raise ValueError('{}: input {!r} is no 4-D Parameter of the network (it has {})'.format(what, screen.input, sorted(names)))
    return screen.input


def extent_of(ienet, name) -> tuple:
    """(Hn, Wn) of the 4-D Parameter `name` as declared."""
    shape = next(ienet.G.nodes[nid]['data']['shape'] for nid, n in ienet.find_node_by_type('Parameter') if n == name)
    return int(shape[2]), int(shape[3])


def checked(ienet, boxes, sharded: bool) -> dict:
    """{Result name: resolved BoxScreen, layout filled in and `input` named} of the `boxes` argument of infer() / start_async() -- a
    BoxScreen, a min_score or True for every FP32 Result that shape_of takes with the screen's layout (None: where it can be inferred)
    and objectness, or {Result name: any of these} --, {} for None.  Everything is looked up in the network as it was read: no device is
    needed, nothing is allocated.  ValueError ('boxes: ...'): an unknown name, a value of another type or out of range, no such Result
    for an unnamed form, a sharded batch, a Result of another rank, shape or precision, a named Result whose layout is ambiguous, no 4-D
    Parameter or several without input=."""
    if boxes is None:
        return {}
    batch = int(ienet.batch_size)
    ports, wanted = ask.named(ienet, 'boxes', boxes, sharded, _fits, _none_fits, resolved)
    for name, screen in wanted.items():
        what = 'boxes: Result {!r}'.format(name)
        try:
            shape = shape_of(ports[name]['dims'], screen.layout, screen.objectness, batch)
        except AmbiguousLayout as e:
            raise ValueError('{}: {}'.format(what, e)) from None
        expected = SHAPE + (' as {!r}'.format(screen.layout) if screen.layout is not None else '')
        layout = ask.declared('boxes', name, ports[name], shape, expected, batch)[0]
        wanted[name] = screen._replace(layout=layout, input=checked_input(ienet, screen, what))
    return wanted


def scratch_bytes(n: int, A: int, per_image: int) -> int:
    """PVHIP_BOXES_SCRATCH_BYTES: the (n, A) 8-byte keys, the (n, A) int32 winners, then at the next 16-byte boundary the staging rows."""
    return ((12 * n * A + 15) & ~15) + 32 * n * per_image


class Blocks(detections.TableBlocks):
    """The blocks of one (Result name, screen without min_score and frame_size): the header and rows pvhip_dense_boxes_f32 writes with
    their page-locked twins, the labels on the device, and `scratch`, the keys, winners and staging rows between the entry's three
    launches, which stay on the device.  read_back is TableBlocks': the header, 4 (2 n + 1) bytes, then exactly 32 total bytes."""
    __slots__ = ('n', 'A', 'scratch')
    ENTRY = 'pvhip_dense_boxes_f32'

    def __init__(self, n: int, A: int, screen: BoxScreen):
        super().__init__(n, n * screen.max_per_image, screen)
        self.n, self.A = n, A
        self.scratch = device.DeviceTensor.empty((scratch_bytes(n, A, screen.max_per_image) // 4,), np.int32)

    def launch(self, result, min_score, frame_size, fit):
        """One call (three launches) on the current stream, behind whatever wrote `result` there, over frames of `frame_size` that stand
        in the rectangle `fit` = (dx, dy, iw, ih) of the network's input."""
        s = self.screen
        layout, n, A, C = shape_of(result.shape, s.layout, s.objectness)
        assert (n, A) == (self.n, self.A) and result.dtype == np.float32
        device.call(self.ENTRY, device.ptr(result), n, A, C, LAYOUTS[layout], int(s.objectness), BOXES[s.box], min_score, device.ptr(self.labels),
                    0 if s.labels is None else len(s.labels), frame_size[0], frame_size[1], fit[0], fit[1], fit[2], fit[3], s.min_size[0],
                    s.min_size[1], s.max_candidates, OVERLAPS[s.overlap], s.threshold, int(s.per_label), s.max_per_image,
                    ctypes.c_void_p(self.scratch.ptr), ctypes.c_void_p(self.header.ptr), ctypes.c_void_p(self.rows.ptr))


class Ask(ask.Ask, collections.namedtuple('Ask', 'screen net_hw format frame_size fit')):
    """A Result asked for with boxes=, its screen resolved: `net_hw` the extent of the screen's input; `format` that input's InputFormat
    when it declares a fit, else None; `frame_size` and `fit` = (dx, dy, iw, ih), the geometry of the pass, known once its inputs are staged
    (bound): the identity over the screen's frame_size or the network's extent, or, for a fitted input fed host frames, the rectangle those
    frames were fitted into, over the screen's frame_size or theirs."""
    __slots__ = ()
    KEYWORD = 'boxes'

    def bound(self, inputs, slots):
        name = self.screen.input
        extent = slots[name].fed if self.format is not None and name in slots else None
        if extent is None:                      # nothing was fitted: a device tensor at the network's own extent, or a stretched input
            return self._replace(frame_size=self.screen.frame_size or self.net_hw, fit=(0, 0, self.net_hw[1], self.net_hw[0]))
        frame = self.screen.frame_size or (int(extent[0]), int(extent[1]))
        if not detections._pair(frame, detections.MAX_EXTENT):
            raise ValueError('boxes: frames of {} are more than 2^24 wide or high'.format(tuple(extent)))
        return self._replace(frame_size=frame, fit=tuple(int(v) for v in self.format.fit_geometry(extent)))

    def key(self, name):
        """(name, the screen without min_score and frame_size).  min_score, the frame extent and the geometry go with the launch: the blocks
        serve every one of them.  max_per_image sizes the rows, the labels are uploaded once with the blocks, and the other fields, which
        neither size nor fill a block, stay in the key because the blocks' launch reads them from their own screen."""
        return (name, self.screen._replace(min_score=None, frame_size=None))

    def blocks_for(self, value):
        _, n, A, _ = shape_of(value.shape, self.screen.layout, self.screen.objectness)
        return Blocks(n, A, self.screen._replace(min_score=None, frame_size=None))

    def launch_with(self):
        return (self.screen.min_score, self.frame_size, self.fit)

    def on_host(self, value):
        return decode(value, self.screen._replace(frame_size=self.frame_size), self.net_hw, self.fit)
