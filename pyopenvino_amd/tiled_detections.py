"""A tiled detector's answer (``infer({input: RoiInput(frames, tiles)}, detections=TiledScreen(...))``): the rule, the argument checks and
the device launch.  The batch rows of the pass are tiles of m frames; what comes back is one ``Detections`` over FRAMES.

The rule (include/pvhip.h, pvhip_detections_merge_tiles; tests/tiles_ref.py is the same again).  Records are [rank, label, score, xmin,
ymin, xmax, ymax]; batch row b is rows [b P, (b + 1) P); tile b = (f, x, y, w, h) is row b of the RoiInput's (n, 5) table.
  1. candidates   tile b contributes nothing if f is outside [0, m), w < 1 or h < 1 (or w or h above 2^24).  Otherwise its candidates are
                  exactly what detections.py's rule selects over frames of (h, w), the tile's extent: live, score >= float32(
                  min_confidence), four finite corners, the label filter, floor / ceil of the clamped float32 products, min_size.  The
                  frame rectangle is (x + x0, y + y0, w, h) (int32 sums): boxes clamp to the tile, because the detector saw nothing
                  else.  A tile keeps its first max_per_tile candidates in position order; selected[f] is the number of kept candidates
                  of all tiles of frame f.
  2. order        within a frame by descending score as a float, +0.0 = -0.0 (no NaN passes the screen); ties go to the lower flat
                  record: top_k.py's order.
  3. suppression  greedy in that order: candidate i is dropped iff an earlier candidate j that was kept overlaps it, with equal int
                  labels (the row's label word) when per_label is set.  int64 inter, a_i, a_j; den = a_i + a_j - inter for 'IOU', den =
                  min(a_i, a_j) for 'IOS'; i overlaps j iff float64(inter) > float64(float32(threshold)) * float64(den): one IEEE float64
                  product and one comparison, every area exact.  Equality does not suppress.
  4. cap, table   a frame keeps its first max_per_frame kept candidates: counts[f].  The table is in (frame, order of step 2) order
                  without gaps; rows (f, x0, y0, w, h, label, score bits, record) as detections.py's; record = b P + p, so the tile of a
                  detection is record // P.

A detector over REGIONS (``detections=RegionScreen(...)``, pvhip_detections_merge_regions; tests/regions_ref.py): the batch rows are regions
of any aspect -- a RoiInput's table, or the table a DetectedRois made on the device, whose rows behind `count` are (-1, 0, 0, 0, 0) and
contribute nothing --, placed in the (Hn, Wn) input by the input's declared resize_fit.  Step 1 alone differs: with g =
input_format.fit_geometry((h, w), (Hn, Wn), fit), the integer rule that placed the region's pixels, region b's candidates are what
detections.py's `fitted` rule selects over frames of (h, w) with (Hn, Wn, *g): every corner mapped back by (v N - d) / i in float32, three
roundings, the finite check on the record's own corners; a box in the padding clamps to the region's edge, one wholly in it is dropped.
'STRETCH' maps nothing: TiledScreen's answer bit for bit.  Steps 2 to 4 are unchanged.
ValueError before anything is staged or launched, besides detections.py's: the screen's input fed anything but a RoiInput (a RegionScreen's:
or a DetectedRois), more than 4096 candidates, a Result that `top_k` names as well, a TiledScreen over an input that declares a fit."""
import collections
import ctypes

import numpy as np

from . import ask, detections, device
from .detections import Detections
from .input_format import RESIZE_FITS, DetectedRois, RoiInput, fit_geometry

MAX_CANDIDATES = 4096                # n * max_per_tile: what one workgroup sorts in LDS
OVERLAPS = {'IOU': 0, 'IOS': 1}      # PVHIP_OVERLAP_IOU / _IOS

_Tiled = collections.namedtuple('TiledScreen', 'min_confidence labels min_size max_per_tile overlap threshold per_label max_per_frame input')
_Region = collections.namedtuple('RegionScreen', 'min_confidence labels min_size max_per_region overlap threshold per_label max_per_frame input')


class TiledScreen(_Tiled):
    """Wherever a ``DetectionScreen`` is accepted, for a pass whose 4-D input (`input` names it when the network has several) is fed a
    ``RoiInput(frames, tiles)``: the batch rows are tiles of the m frames, and the Result comes back as a ``Detections`` over frames --
    `counts` and `selected` of shape (m,), `rois[:, 0]` the frame and the rectangle in frame pixels, `records` the flat row of the Result
    (its tile is records // P).  Candidates: score >= `min_confidence`, `labels` (None: any, or at most 64 ints), rectangles of at least
    `min_size` = (h, w) clamped to their tile, the first `max_per_tile` of a tile (None: min(P, 4096 // n); n * max_per_tile <= 4096).
    Within a frame they are taken by descending score and dropped when an earlier kept one -- of the same label when `per_label` --
    overlaps them by more than `threshold`: `overlap` = 'IOU' (intersection over union) or 'IOS' (over the smaller area).  At most
    `max_per_frame` per frame (None: all).  Immutable; the values are checked when a pass is started with it (ValueError)."""
    __slots__ = ()
    ROWS = 'tiles'                      # what a batch row is called where a value is refused

    def __new__(cls, min_confidence=0.5, labels=None, min_size=(1, 1), max_per_tile=None, overlap='IOU', threshold=0.45, per_label=True,
                max_per_frame=None, input=None):
        frozen = [detections._frozen(v) for v in (labels, min_size)]
        return super().__new__(cls, min_confidence, frozen[0], frozen[1], max_per_tile, overlap, threshold, per_label, max_per_frame, input)

    def resolved_in(self, ienet, per_tile: int, what='') -> 'TiledScreen':
        """What detections.checked() makes of this screen for a Result of `ienet` with P = `per_tile`: resolved, with its `input` named."""
        return resolved(self, int(ienet.batch_size), per_tile, what)._replace(input=checked_input(ienet, self, what))


class RegionScreen(_Region):
    """Wherever a ``DetectionScreen`` is accepted, for a pass whose 4-D input (`input` names it when the network has several) is fed a
    ``RoiInput(frames, regions)`` or a ``DetectedRois(frames, detector, ...)``: the batch rows are regions of the m frames, of any aspect,
    and the input may declare ``resize_fit`` 'STRETCH', 'LETTERBOX' or 'TOP_LEFT' -- every region's boxes are mapped back through the
    geometry its own pixels were placed with.  The Result comes back as a ``Detections`` over frames as a ``TiledScreen``'s does: `counts`
    and `selected` of shape (m,), `rois[:, 0]` the frame and the rectangle in frame pixels, `records` the flat row of the Result (its
    region is records // P; for a DetectedRois, ``request.detected_rois(name).records[records // P]`` is the first-stage record).  The
    values are a TiledScreen's, with `max_per_region` (None: min(P, 4096 // n); n * max_per_region <= 4096) in the place of max_per_tile.
    Immutable; the values are checked when a pass is started with it (ValueError)."""
    __slots__ = ()
    ROWS = 'regions'

    def __new__(cls, min_confidence=0.5, labels=None, min_size=(1, 1), max_per_region=None, overlap='IOU', threshold=0.45, per_label=True,
                max_per_frame=None, input=None):
        frozen = [detections._frozen(v) for v in (labels, min_size)]
        return super().__new__(cls, min_confidence, frozen[0], frozen[1], max_per_region, overlap, threshold, per_label, max_per_frame, input)

    resolved_in = TiledScreen.resolved_in


def resolved(screen, tiles: int, per_tile: int, what=''):
    """`screen`, a TiledScreen or a RegionScreen, with every value checked and in its one form for n = `tiles` batch rows of P = `per_tile`
    records -- max_per_tile (max_per_region) and max_per_frame filled in --, so that equal screens are equal keys; `input` stays as it is
    (checked() knows the network).  ValueError."""
    conf, labels, size, cap, overlap, threshold, per_label, frame_cap, name = screen
    n, P = int(tiles), int(per_tile)
    rows, cap_name = screen.ROWS, screen._fields[3]
    # (the plain screen's checks and forms of what the two share, over a placeholder frame)
    conf, _, labels, size, _ = detections.resolved(detections.DetectionScreen(conf, (1, 1), labels, size, None), P, None, what)
    if not isinstance(overlap, str) or overlap not in OVERLAPS:
        raise ValueError('detections: {}overlap is \'IOU\' or \'IOS\', got {!r}'.format(what, overlap))
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or not 0 <= threshold <= 1:
        raise ValueError('detections: {}threshold {!r} is not a finite number in [0, 1]'.format(what, threshold))
    if not isinstance(per_label, (bool, np.bool_)):
        raise ValueError('detections: {}per_label is a bool, got {!r}'.format(what, per_label))
    for key, v in ((cap_name, cap), ('max_per_frame', frame_cap)):
        if v is not None and not detections._count(v):
            raise ValueError('detections: {}{} is None or a count >= 1, got {!r}'.format(what, key, v))
    if n > MAX_CANDIDATES:
        raise ValueError('detections: {}{} {} are more than the {} candidates one pass merges'.format(what, n, rows, MAX_CANDIDATES))
    cap = min(P, MAX_CANDIDATES // n) if cap is None else min(int(cap), P)
    if n * cap > MAX_CANDIDATES:
        raise ValueError('detections: {}{} {} x {} {} is more than {} candidates: lower {} to {} or less'.format(
            what, n, rows, cap_name, cap, MAX_CANDIDATES, cap_name, MAX_CANDIDATES // n))
    frame_cap = n * cap if frame_cap is None else min(int(frame_cap), n * cap)
    return type(screen)(conf, labels, size, cap, overlap, float(threshold), bool(per_label), frame_cap, name)


def checked_input(ienet, screen, what='') -> str:
    """The name of the 4-D Parameter whose feed carries the table of tiles or regions: `screen.input`, or the network's only one;
    ValueError."""
    names = [name for nid, name in ienet.find_node_by_type('Parameter') if len(ienet.G.nodes[nid]['data']['shape']) == 4]
    if screen.input is None:
        if len(names) != 1:
            raise ValueError('detections: {}the network has {} 4-D Parameters ({}): input= names the one fed the {}'.format(
                what, len(names), sorted(names), screen.ROWS))
        return names[0]
    if not isinstance(screen.input, str) or screen.input not in names:
        raise ValueError('detections: {}input {!r} is no 4-D Parameter of the network (it has {})'.format(what, screen.input, sorted(names)))
    return screen.input


def checked_top_k(top_k, detections):
    """No Result is named with a TiledScreen or a RegionScreen and in `top_k` as well (said here, in front of top_k's own checks, which refuse a
    detector's Result for its shape); ValueError."""
    if isinstance(top_k, dict) and isinstance(detections, dict):
        both = sorted(name for name, screen in detections.items() if isinstance(screen, (TiledScreen, RegionScreen)) and name in top_k)
        if both:
            raise ValueError('detections: Result {!r} is asked for with top_k as well'.format(both[0]))


def checked_feed(inputs: dict, screens: dict):
    """Every tiled screen's input is fed a RoiInput -- nothing else carries a tile table -- and every region screen's a RoiInput or a
    DetectedRois, whose table is made on the device; ValueError before anything is staged."""
    for name, screen in screens.items():
        fed = inputs.get(screen.input) if isinstance(inputs, dict) else None
        if isinstance(screen, RegionScreen):
            if not isinstance(fed, (RoiInput, DetectedRois)):
                raise ValueError('detections: Result {!r}: a RegionScreen needs input {!r} fed a RoiInput or a DetectedRois (frames and a '
                                 'table of regions), got {}'.format(name, screen.input, type(fed).__name__))
        elif not isinstance(fed, RoiInput):
            raise ValueError('detections: Result {!r}: a TiledScreen needs input {!r} fed a RoiInput (frames, tiles), got {}'.format(
                name, screen.input, type(fed).__name__))


def _overlap(box, others, kind: str, threshold: float):
    """Step 3's comparison of one int64 (x0, y0, w, h) with the rows of `others`."""
    iw = np.minimum(box[0] + box[2], others[:, 0] + others[:, 2]) - np.maximum(box[0], others[:, 0])
    ih = np.minimum(box[1] + box[3], others[:, 1] + others[:, 3]) - np.maximum(box[1], others[:, 1])
    inter = np.where((iw > 0) & (ih > 0), iw * ih, 0)
    area, areas = box[2] * box[3], others[:, 2] * others[:, 3]
    den = np.minimum(area, areas) if kind == 'IOS' else area + areas - inter
    return inter.astype(np.float64) > np.float64(np.float32(threshold)) * den.astype(np.float64)


def merge_tiles(records, rois, frames: int, screen) -> Detections:
    """The rule in numpy on a host array of float32 records, (1, 1, R, 7) or (R, 7), of the n tiles `rois` (an integer (n, 5) table, row
    b = (f, x, y, w, h)) of `frames` = m frames: what a Result computed on the host gets.  `screen`: a TiledScreen, or a min_confidence."""
    return _merge(records, rois, frames, screen if isinstance(screen, TiledScreen) else TiledScreen(min_confidence=screen))


def merge_regions(records, regions, frames: int, screen, net_hw=None, fit='STRETCH') -> Detections:
    """The RegionScreen rule in numpy: merge_tiles for the n regions `regions` of any aspect, each placed in a detector input of `net_hw` =
    (Hn, Wn) by `fit` = 'STRETCH' (nothing is mapped, `net_hw` is not needed), 'LETTERBOX' or 'TOP_LEFT'.  `screen`: a RegionScreen, or a
    min_confidence."""
    if not isinstance(fit, str) or fit not in RESIZE_FITS:
        raise ValueError('detections: fit is one of {}, got {!r}'.format(sorted(RESIZE_FITS), fit))
    if fit != 'STRETCH':
        net_hw = detections._frozen(net_hw)
        if not detections._pair(net_hw, detections.MAX_EXTENT):
            raise ValueError('detections: net_hw is (Hn, Wn) with both in 1 .. 2^24, got {!r}'.format(net_hw))
        net_hw = (int(net_hw[0]), int(net_hw[1]))
    return _merge(records, regions, frames, screen if isinstance(screen, RegionScreen) else RegionScreen(min_confidence=screen),
                  None if fit == 'STRETCH' else (net_hw, fit))


def _merge(records, rois, frames, screen, placed=None) -> Detections:
    """The rule of both screens; `placed`: None, or ((Hn, Wn), fit) of regions fitted into the detector's input."""
    rec, t = detections.records_checked(records), np.asarray(rois)
    if t.ndim != 2 or t.shape[1] != 5 or t.shape[0] < 1 or t.dtype.kind not in 'iu' or rec.shape[0] % t.shape[0]:
        raise ValueError('detections: an integer (n, 5) table of {} with n dividing the {} records, got {} {}'.format(
            screen.ROWS, rec.shape[0], t.dtype, t.shape))
    if not detections._count(frames):
        raise ValueError('detections: {!r} frames'.format(frames))
    t = t.astype(np.int64)
    n, m = t.shape[0], int(frames)
    P = rec.shape[0] // n
    conf, labels, min_size, cap, kind, threshold, per_label, frame_cap, _ = resolved(screen, n, P)
    # 1. candidates: the plain screen over each tile's own extent
    f, x, y, w, h = t.T
    tile_ok = (f >= 0) & (f < m) & (w >= 1) & (w <= detections.MAX_EXTENT) & (h >= 1) & (h <= detections.MAX_EXTENT)
    fh, fw = np.repeat(np.where(tile_ok, h, 1), P).astype(np.float32), np.repeat(np.where(tile_ok, w, 1), P).astype(np.float32)
    geometry = None
    if placed is not None:             # one geometry per region, in Python ints; a region that takes nothing gets a harmless one
        (Hn, Wn), how = placed
        g = np.array([fit_geometry((int(h[b]), int(w[b])), (Hn, Wn), how) if tile_ok[b] else (0, 0, 1, 1) for b in range(n)], np.int64)
        geometry = (Hn, Wn) + tuple(np.repeat(g[:, k], P) for k in range(4))
    keep, x0, y0, bw, bh, label = detections.screened(rec, n, conf, labels, min_size, fh, fw, ~tile_ok, geometry)
    cand = np.flatnonzero((keep & (np.cumsum(keep, axis=1) <= cap)).ravel())
    tile = cand // P
    boxes = np.stack([(x[tile] + x0[cand]).astype(np.int32), (y[tile] + y0[cand]).astype(np.int32), bw[cand], bh[cand]], axis=1).astype(np.int64)
    label = label[cand]
    score = rec[cand, 2]
    counts, selected, rows = np.zeros(m, np.int32), np.zeros(m, np.int32), []
    for frame in range(m):
        mine = np.flatnonzero(f[tile] == frame)
        selected[frame] = len(mine)
        # 2. order (`mine` is in record order and the sort is stable; -0.0 and 0.0 compare equal)
        mine = mine[np.argsort(-score[mine].astype(np.float64), kind='stable')]
        # 3. suppression
        gone = np.zeros(len(mine), bool)
        for i in range(len(mine)):
            if gone[i]:
                continue
            rows.append(mine[i])
            counts[frame] += 1
            if counts[frame] == frame_cap:                     # 4. cap
                break
            later = mine[i + 1:]
            hit = _overlap(boxes[mine[i]], boxes[later], kind, threshold)
            if per_label:
                hit &= label[later] == label[mine[i]]
            gone[i + 1:] |= hit
    rows = np.asarray(rows, np.int64)
    kept = cand[rows]
    table = np.concatenate([f[tile[rows]][:, None], boxes[rows]], axis=1).astype(np.int32).reshape(-1, 5)
    return Detections(counts, selected, table, label[rows].astype(np.int32), score[rows].copy(), kept.astype(np.int32))


class Blocks(detections.TableBlocks):
    """The blocks of one (Result name, resolved screen, m): what pvhip_detections_merge_tiles writes, and its candidate scratch."""
    __slots__ = ('tiles', 'per_tile', 'frames', 'scratch')
    ENTRY = 'pvhip_detections_merge_tiles'

    def __init__(self, tiles: int, per_tile: int, frames: int, screen):
        slots = tiles * screen[3]               # max_per_tile, or a RegionScreen's max_per_region
        super().__init__(frames, min(slots, frames * screen.max_per_frame), screen)
        self.tiles, self.per_tile, self.frames = tiles, per_tile, frames
        self.scratch = device.DeviceTensor.empty((9 * slots + tiles,), np.int32)

    def launch(self, result, table, *placed):
        """The entry's three launches on the current stream, behind whatever wrote `result` and uploaded `table` (the slot's (n, 5)
        device table) there; `placed`: what RegionBlocks' entry takes besides, (Hn, Wn, fit code)."""
        s = self.screen
        assert result.dtype == np.float32 and int(np.prod(result.shape)) == 7 * self.tiles * self.per_tile
        assert table.dtype == np.int32 and tuple(table.shape) == (self.tiles, 5)
        device.call(self.ENTRY, device.ptr(result), device.ptr(table), self.tiles, self.per_tile, self.frames,
                    s.min_confidence, device.ptr(self.labels), 0 if s.labels is None else len(s.labels), s.min_size[0], s.min_size[1],
                    s[3], OVERLAPS[s.overlap], s.threshold, int(s.per_label), s.max_per_frame, *placed, ctypes.c_void_p(self.scratch.ptr),
                    ctypes.c_void_p(self.header.ptr), ctypes.c_void_p(self.rows.ptr))


class RegionBlocks(Blocks):
    """The blocks of one (Result name, resolved RegionScreen, m): what pvhip_detections_merge_regions writes, and its candidate scratch."""
    __slots__ = ()
    ENTRY = 'pvhip_detections_merge_regions'


class Ask(ask.Ask, collections.namedtuple('Ask', 'screen tiles frames slot')):
    """A Result asked for with a resolved TiledScreen over n = `tiles` batch rows; `frames` = m and `slot`, the staged input's with the
    tile table page-locked and on the device, are known once the pass's inputs are staged."""
    __slots__ = ()
    KEYWORD = 'detections'
    BLOCKS = Blocks

    def bound(self, inputs, slots):
        return self._replace(frames=int(np.shape(inputs[self.screen.input].frames)[0]), slot=slots[self.screen.input])

    def key(self, name):
        return (name, self.screen, self.frames)

    def blocks_for(self, value):
        return self.BLOCKS(self.tiles, value.shape[-2] // self.tiles, self.frames, self.screen)

    def launch_with(self):
        return (self.slot.tables['roi'].device,)

    def on_host(self, value):
        return merge_tiles(value, self.slot.tables['roi'].host, self.frames, self.screen)


class RegionAsk(ask.Ask, collections.namedtuple('RegionAsk', 'screen tiles frames slot net_hw fit table_of detected')):
    """A Result asked for with a resolved RegionScreen over n = `tiles` batch rows: Ask, with `net_hw` = (Hn, Wn) and `fit`, the declared
    resize_fit, of the screen's input (its InputFormat's) and `table_of`, a function of no arguments that reads the table of a DetectedRois
    back after the pass (host_inputs.detected_rois); `detected`, known once bound: the pass was fed a DetectedRois, whose table only the
    device knows."""
    __slots__ = ()
    KEYWORD = 'detections'
    BLOCKS = RegionBlocks
    key, blocks_for = Ask.key, Ask.blocks_for

    def bound(self, inputs, slots):
        fed = inputs[self.screen.input]
        return self._replace(frames=int(np.shape(fed.frames)[0]), slot=slots[self.screen.input], detected=isinstance(fed, DetectedRois))

    def launch_with(self):
        return (self.slot.tables['roi'].device, self.net_hw[0], self.net_hw[1], RESIZE_FITS[self.fit])

    def on_host(self, value):
        table = self.table_of().rois if self.detected else self.slot.tables['roi'].host
        return merge_regions(value, table, self.frames, self.screen, self.net_hw, self.fit)
