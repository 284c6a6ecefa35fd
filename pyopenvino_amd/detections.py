"""A detector's answer (``infer(..., detections=screen)``): the rule, the argument checks and the device launch.

The rule (include/pvhip.h, pvhip_detections_compact; tests/detections_ref.py is the same again).  Records are [rank, label, score, xmin,
ymin, xmax, ymax] with normalised corners; image b is rows [b P, (b + 1) P) of the R = images P rows.
  live      an image's list ends at its first row whose column 0 is not >= 0 (DetectionOutput's -1 terminator; NaN too): that row and
            everything behind it is ignored;
  selected  live, score >= float32(min_confidence) (false for NaN), four finite corners, and `labels` is None or label == float32(l) for
            a listed l (at most 64; [] selects nothing);
  rectangle over frames of (H, W), in float32, never contracted: x0 = floor(min(max(xmin W, 0), W)), x1 = ceil(min(max(xmax W, 0), W)),
            y0 / y1 alike with H; dropped when x1 - x0 < min_size[1] or y1 - y0 < min_size[0]
-- so far exactly DetectedRois' rule (pvhip_detections_to_rois, tests/detected_rois_ref.py) --;
  fitted    a detector whose input declares a fit (preprocess_info.resize_fit) saw the frame in the rectangle [dy, dy + ih) x [dx, dx + iw)
            of its (Hn, Wn) input: with `fit` = (Hn, Wn, dx, dy, iw, ih) every corner is mapped back first, in float32, three roundings,
            u = (xmin float32(Wn) - float32(dx)) / float32(iw) (ymin: Hn, dy, ih), and the rectangle is that of u; the finite check is on the
            record's own corners.  A box in the padding clamps to the frame's edge, one wholly in it has extent 0 and is dropped
            (pvhip_detections_compact_fit, pvhip_detections_to_rois_fit; tests/letterbox_ref.py);
  cap       image b keeps its first counts[b] = min(selected[b], max_per_image) survivors in position order: its best scores, because
            an image's records stand in descending score order;
  table     the kept survivors of all images in (image, position) order, no gap between images; total = sum(counts);
  row       (b, x0, y0, w, h, label, score bits, record): label = int32 of column 1 (truncated) when that is finite and in
            [-2^31, 2^31), else -1; the score's bits are the record's own; record = b P + p.
The Result itself stays on the device, where a ``DetectedRois`` of another request reads it as before.  Over a fitted input `frame_size`
None means the extent of the frames the pass was fed; that input fed a ``RoiInput`` / ``DetectedRois`` in the same pass (a geometry per row)
is a ValueError, as is a TiledScreen over it (answers.py)."""
import collections
import ctypes

import numpy as np

from . import ask, device

MAX_LABELS = 64
MAX_EXTENT = 1 << 24                 # a frame extent is exact as float32
_INT32_MAX = int(np.iinfo(np.int32).max)

_Detections = collections.namedtuple('Detections', 'counts selected rois labels scores records')
_Screen = collections.namedtuple('DetectionScreen', 'min_confidence frame_size labels min_size max_per_image')


class Detections(_Detections):
    """What a detector's Result started with detections=... comes back as: `counts` and `selected` (images,) int32 -- the rows image b
    has in the table, and the records of it that passed the screen (more when the cap cut them) --; `rois` (total, 5) int32 in RoiInput's
    (id, x, y, w, h) order, id = the image; `labels` (total,) int32; `scores` (total,) float32; `records` (total,) int32, the flat row of
    the Result each came from.  total = counts.sum(); image b is rows [counts[:b].sum(), counts[:b + 1].sum())."""
    __slots__ = ()

    def of(self, b: int) -> tuple:
        """(rois, labels, scores, records) of image b: slices of the table."""
        images = len(self.counts)
        if not -images <= b < images:
            raise IndexError('image {} of {}'.format(b, images))
        b = b % images
        lo = int(self.counts[:b].sum())
        rows = slice(lo, lo + int(self.counts[b]))
        return self.rois[rows], self.labels[rows], self.scores[rows], self.records[rows]


class DetectionScreen(_Screen):
    """Which of a detector's records come back, and over which frames: score >= `min_confidence`; rectangles over frames of `frame_size`
    = (H, W) (None: the extent of the network's single 4-D Parameter as declared); `labels`: None (any) or at most 64 ints; rectangles
    of at least `min_size` = (h, w); at most `max_per_image` per image (None: all).  Immutable; the values are checked when a pass is
    started with it (ValueError)."""
    __slots__ = ()

    def __new__(cls, min_confidence=0.5, frame_size=None, labels=None, min_size=(1, 1), max_per_image=None):
        frozen = [_frozen(v) for v in (frame_size, labels, min_size)]
        return super().__new__(cls, min_confidence, frozen[0], frozen[1], frozen[2], max_per_image)


def _frozen(v):
    """A list, range or 1-D array as a tuple, so that a screen is a key; anything else as it is, for resolved() to judge."""
    if isinstance(v, np.ndarray):
        return tuple(v.tolist()) if v.ndim == 1 else v
    return tuple(v) if isinstance(v, (list, range)) else v


def _count(v, hi=_INT32_MAX):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer)) and 1 <= v <= hi


def _pair(v, hi):
    return isinstance(v, tuple) and len(v) == 2 and all(_count(e, hi) for e in v)


def resolved(screen, per_image: int, extent=None, what='') -> DetectionScreen:
    """`screen` (a DetectionScreen, or a number: its min_confidence) with every value checked and in its one form -- a float, tuples of
    ints, frame_size filled in from `extent`, max_per_image from `per_image` = P --, so that equal screens are equal keys; ValueError."""
    if not isinstance(screen, DetectionScreen):
        screen = DetectionScreen(min_confidence=screen)
    conf, frame, labels, size, cap = screen
    if isinstance(conf, bool) or not isinstance(conf, (int, float, np.integer, np.floating)) or not np.isfinite(conf):
        raise ValueError('detections: {}min_confidence {!r} is not a finite number'.format(what, conf))
    if labels is not None:
        if not isinstance(labels, tuple) or len(labels) > MAX_LABELS or not all(
                not isinstance(l, bool) and isinstance(l, (int, np.integer)) and -_INT32_MAX - 1 <= l <= _INT32_MAX for l in labels):
            raise ValueError('detections: {}labels is None or at most {} ints, got {!r}'.format(what, MAX_LABELS, labels))
        labels = tuple(int(l) for l in labels)
    if not _pair(size, _INT32_MAX):
        raise ValueError('detections: {}min_size is (h, w) with both >= 1, got {!r}'.format(what, size))
    if frame is None:
        frame = extent
        if frame is None:
            raise ValueError('detections: {}frame_size is needed: the network has no single 4-D Parameter to take it from'.format(what))
    if not _pair(frame, MAX_EXTENT):
        raise ValueError('detections: {}frame_size is (H, W) with both in 1 .. 2^24, got {!r}'.format(what, frame))
    if cap is None:
        cap = per_image
    if not _count(cap):
        raise ValueError('detections: {}max_per_image is None or a count >= 1, got {!r}'.format(what, cap))
    return DetectionScreen(float(conf), (int(frame[0]), int(frame[1])), labels, (int(size[0]), int(size[1])), min(int(cap), int(per_image)))


def records_checked(records) -> np.ndarray:
    """`records` as an (R, 7) array, if they are float32 records of shape (1, 1, R, 7) or (R, 7) with R >= 1; ValueError."""
    rec = np.asarray(records)
    if rec.dtype != np.float32 or rec.ndim not in (2, 4) or rec.shape[-1] != 7 or tuple(rec.shape[:-2]) not in ((), (1, 1)) or rec.shape[-2] < 1:
        raise ValueError('detections: float32 records of shape (1, 1, R, 7) or (R, 7), got {} {}'.format(rec.dtype, rec.shape))
    return rec.reshape(-1, 7)


def checked_fit(fit, what='fit'):
    """`fit` as six ints (Hn, Wn, dx, dy, iw, ih) -- a rectangle of at least 1 x 1 inside an input of at most 2^24 x 2^24 --, or None;
    ValueError."""
    if fit is None:
        return None
    try:
        g = tuple(fit)
        ok = len(g) == 6 and all(not isinstance(v, bool) and isinstance(v, (int, np.integer)) for v in g)
    except TypeError:
        ok = False
    if ok:
        Hn, Wn, dx, dy, iw, ih = g = tuple(int(v) for v in g)
        ok = 1 <= Hn <= MAX_EXTENT and 1 <= Wn <= MAX_EXTENT and iw >= 1 and ih >= 1 and dx >= 0 and dy >= 0 and dx + iw <= Wn and dy + ih <= Hn
    if not ok:
        raise ValueError('detections: {} is (Hn, Wn, dx, dy, iw, ih), a rectangle inside the detector\'s input, got {!r}'.format(what, fit))
    return g


def screened(rec, groups: int, conf, labels, min_size, height, width, empty=None, fit=None) -> tuple:
    """The rule's `live`, `selected` and `rectangle` on (N P, 7) records of N = `groups` lists, over frames of (`height`, `width`) -- two
    numbers, or float32 arrays with one extent per record --; `empty`: (N,) bool, the lists that take nothing; `fit`: the six ints of a
    fitted detector input, whose corners are mapped back first.  (keep, x0, y0, w, h, label):
    the (N, P) mask of the survivors before any cap, their rectangles as int64 and the rows' label words, one entry per record."""
    N, P = groups, rec.shape[0] // groups
    dead = ~(rec[:, 0] >= 0).reshape(N, P)
    end = np.where(dead.any(axis=1), dead.argmax(axis=1), P)
    live = np.arange(P)[None, :] < end[:, None]
    if empty is not None:
        live &= ~empty[:, None]
    keep = live.ravel() & (rec[:, 2] >= np.float32(conf)) & np.isfinite(rec[:, 3:7]).all(axis=1)
    if labels is not None:
        keep &= np.isin(rec[:, 1], np.asarray(labels, np.int64).astype(np.float32))
    corners = np.where(keep[:, None], rec[:, 3:7], np.float32(0))
    if fit is not None:
        Hn, Wn, dx, dy, iw, ih = fit
        with np.errstate(over='ignore'):
            corners = np.stack([(corners[:, k] * np.float32(N_) - np.float32(d)) / np.float32(i)
                                for k, (N_, d, i) in enumerate(((Wn, dx, iw), (Hn, dy, ih), (Wn, dx, iw), (Hn, dy, ih)))], axis=1)

    def edge(v, extent, rounded):
        e = np.float32(extent)
        with np.errstate(over='ignore', invalid='ignore'):
            return rounded(np.minimum(np.maximum(v * e, np.float32(0)), e)).astype(np.int64)

    x0, y0 = edge(corners[:, 0], width, np.floor), edge(corners[:, 1], height, np.floor)
    w, h = edge(corners[:, 2], width, np.ceil) - x0, edge(corners[:, 3], height, np.ceil) - y0
    keep &= (w >= min_size[1]) & (h >= min_size[0])
    label = rec[:, 1]
    whole = np.isfinite(label) & (label >= np.float32(-2.0 ** 31)) & (label < np.float32(2.0 ** 31))
    with np.errstate(invalid='ignore'):
        label = np.where(whole, np.where(whole, label, np.float32(0)).astype(np.int32), np.int32(-1)).astype(np.int32)
    return keep.reshape(N, P), x0, y0, w, h, label


def compact_records(records, images: int, screen, fit=None) -> Detections:
    """The rule in numpy on a host array of float32 records, (1, 1, R, 7) or (R, 7), of `images` images: what a Result computed on the
    host (a foreign plugin set) gets.  `screen`: a DetectionScreen with a frame_size (there is no network here to take it from); `fit`:
    None, or (Hn, Wn, dx, dy, iw, ih) of a fitted detector input."""
    rec = records_checked(records)
    fit = checked_fit(fit)
    if not _count(images) or rec.shape[0] % images:
        raise ValueError('detections: {} records do not divide into {!r} images'.format(rec.shape[0], images))
    N, P = int(images), rec.shape[0] // int(images)
    conf, (H, W), labels, min_size, cap = resolved(screen, P)
    keep, x0, y0, w, h, label = screened(rec, N, conf, labels, min_size, H, W, fit=fit)
    selected = keep.sum(axis=1).astype(np.int32)
    kept = np.flatnonzero((keep & (np.cumsum(keep, axis=1) <= cap)).ravel())
    rois = np.stack([kept // P, x0[kept], y0[kept], w[kept], h[kept]], axis=1).astype(np.int32).reshape(-1, 5)
    return Detections(np.minimum(selected, cap).astype(np.int32), selected, rois, label[kept], rec[kept, 2].copy(), kept.astype(np.int32))


def records_of(port, batch: int):
    """P, the records per image, of a Result whose input port is declared (1, 1, R, 7) with R a multiple of `batch`; None for any other
    shape."""
    dims = tuple(int(d) for d in port['dims'])
    if len(dims) != 4 or dims[:2] != (1, 1) or dims[3] != 7 or dims[2] < 1 or dims[2] % batch:
        return None
    return dims[2] // batch


def _declared_extent(ienet):
    """(H, W) of the network's single 4-D Parameter as declared, or None."""
    shapes = [tuple(int(d) for d in ienet.G.nodes[nid]['data']['shape']) for nid, _ in ienet.find_node_by_type('Parameter')]
    shapes = [s for s in shapes if len(s) == 4]
    return (shapes[0][2], shapes[0][3]) if len(shapes) == 1 else None


def _fits(port, screen, batch):
    return records_of(port, batch) is not None and port['precision'] == 'FP32'


def _none_fits(ports, screen, batch):
    described = ', '.join('{!r} {} {}'.format(name, port['precision'], tuple(port['dims'])) for name, port in sorted(ports.items()))
    return 'detections: the network has no FP32 Result of shape (1, 1, R, 7) with R a multiple of the batch {} (it has {})'.format(batch, described)


def checked(ienet, detections, sharded: bool) -> dict:
    """{Result name: resolved DetectionScreen} of the `detections` argument of infer() / start_async() -- a DetectionScreen or a
    min_confidence for every detector Result (FP32, declared (1, 1, R, 7) with R a multiple of the batch), or {Result name: either} --,
    {} for None; a ``TiledScreen`` or a ``RegionScreen`` in the place of a DetectionScreen resolves to one with its `input` named.
    Everything is looked up in the network as it was read: no device is needed, nothing is allocated.  ValueError ('detections: ...'): an
    unknown name, no such Result for an unnamed form, a sharded batch, a Result of another shape or precision, a value of the screen out
    of range."""
    if detections is None:
        return {}
    batch = int(ienet.batch_size)
    ports, wanted = ask.named(ienet, 'detections', detections, sharded, _fits, _none_fits)
    out = {}
    for name, screen in wanted.items():
        per_image = ask.declared('detections', name, ports[name], records_of(ports[name], batch), '(1, 1, R, 7) with R a multiple of the batch {}', batch)
        if batch * per_image >= (1 << 31) // 7:
            raise ValueError('detections: Result {!r} has too many records ({} x {})'.format(name, batch, per_image))
        what = 'Result {!r}: '.format(name)
        if hasattr(screen, 'resolved_in'):                    # a TiledScreen: the batch rows are tiles of frames, tiled_detections.py's rule
            out[name] = screen.resolved_in(ienet, per_image, what)
        else:
            out[name] = resolved(screen, per_image, _declared_extent(ienet), what)
    return out


class TableBlocks:
    """What a request keeps for one table-shaped answer over `groups` images or frames: the device header (counts, selected, total) and
    rows that `ENTRY` writes, the labels on the device (uploaded once, here), and the page-locked host twins of header and rows that
    wait() reads back into: the header, 4 (2 groups + 1) bytes, then exactly 32 total bytes."""
    __slots__ = ('groups', 'screen', 'header', 'rows', 'labels', 'header_host', 'rows_host')
    ENTRY = None

    def __init__(self, groups: int, capacity: int, screen):
        self.groups, self.screen = groups, screen
        self.header = device.DeviceTensor.empty((2 * groups + 1,), np.int32)
        self.rows = device.DeviceTensor.empty((capacity, 8), np.int32)
        self.header_host = device.host_empty((2 * groups + 1,), np.int32)
        self.rows_host = device.host_empty((capacity, 8), np.int32)
        # ([]: a device pointer with no label behind it, which selects nothing; None: NULL, any label)
        self.labels = None if screen.labels is None else device.DeviceTensor.from_numpy(np.asarray(screen.labels + (0,), np.int32))

    def read_back(self) -> Detections:
        """The answer, copied on the current stream, which has drained: the header, then the rows it counts; the arrays are the
        caller's own."""
        n = self.groups
        device.call('pvhip_memcpy_d2h', ctypes.c_void_p(self.header_host.ctypes.data), ctypes.c_void_p(self.header.ptr), self.header_host.nbytes)
        total = int(self.header_host[2 * n])
        if not 0 <= total <= self.rows_host.shape[0]:
            raise device.PvhipError('{} left total = {} of at most {} rows'.format(self.ENTRY, total, self.rows_host.shape[0]))
        if total:
            device.call('pvhip_memcpy_d2h', ctypes.c_void_p(self.rows_host.ctypes.data), ctypes.c_void_p(self.rows.ptr), 32 * total)
        t = self.rows_host[:total]                             # the kernel's rows (id, x, y, w, h, label, score bits, record)
        return Detections(self.header_host[:n].copy(), self.header_host[n:2 * n].copy(), t[:, :5].copy(), t[:, 5].copy(),
                          t[:, 6].copy().view(np.float32), t[:, 7].copy())


class Blocks(TableBlocks):
    """The blocks of one (Result name, resolved screen): what pvhip_detections_compact writes."""
    __slots__ = ('images', 'per_image')
    ENTRY = 'pvhip_detections_compact'

    def __init__(self, images: int, per_image: int, screen: DetectionScreen):
        super().__init__(images, images * min(per_image, screen.max_per_image), screen)
        self.images, self.per_image = images, per_image

    def launch(self, result, frame_size=None, fit=None):
        """The entry's two launches on the current stream, behind whatever wrote `result` there; `fit`: the six ints of a fitted
        detector input (pvhip_detections_compact_fit), over frames of `frame_size` (default: the screen's)."""
        s = self.screen
        frame = s.frame_size if frame_size is None else frame_size
        assert result.dtype == np.float32 and int(np.prod(result.shape)) == 7 * self.images * self.per_image
        device.call(self.ENTRY + ('_fit' if fit is not None else ''), device.ptr(result), self.images, self.per_image, frame[0], frame[1],
                    s.min_confidence, device.ptr(self.labels), 0 if s.labels is None else len(s.labels), s.min_size[0], s.min_size[1],
                    s.max_per_image, ctypes.c_void_p(self.header.ptr), ctypes.c_void_p(self.rows.ptr), *(fit or ()))


class Ask(ask.Ask, collections.namedtuple('Ask', 'screen images')):
    """A Result of `images` images asked for with a resolved DetectionScreen."""
    __slots__ = ()
    KEYWORD = 'detections'

    def key(self, name):
        return (name, self.screen)

    def blocks_for(self, value):
        return Blocks(self.images, value.shape[-2] // self.images, self.screen)

    def on_host(self, value):
        return compact_records(value, self.images, self.screen)


class FittedAsk(ask.Ask, collections.namedtuple('FittedAsk', 'screen images input format explicit fit')):
    """The Ask of a detector whose 4-D Parameter `input`, of InputFormat `format`, declares a fit: `fit` = (Hn, Wn, dx, dy, iw, ih) is known
    once the pass's inputs are staged (bound), from the extent of the frames that pass was fed, and frame_size -- unless the caller gave
    one (`explicit`) -- is that extent."""
    __slots__ = ()
    KEYWORD = 'detections'
    blocks_for = Ask.blocks_for

    def bound(self, inputs, slots):
        extent = slots[self.input].fed if self.input in slots else None
        if extent is None:                      # a device tensor at the network's own extent: nothing was fitted
            return self._replace(fit=None)
        screen = self.screen if self.explicit else self.screen._replace(frame_size=(int(extent[0]), int(extent[1])))
        if not _pair(screen.frame_size, MAX_EXTENT):
            raise ValueError('detections: frames of {} are more than 2^24 wide or high'.format(tuple(extent)))
        fmt = self.format
        return self._replace(screen=screen, fit=(int(fmt.dims[2]), int(fmt.dims[3])) + tuple(fmt.fit_geometry(extent)))

    def key(self, name):
        # (the blocks serve every frame extent: neither their size nor their labels depend on it)
        return (name, self.screen if self.fit is None else self.screen._replace(frame_size=None))

    def launch_with(self):
        return (self.screen.frame_size, self.fit)

    def on_host(self, value):
        return compact_records(value, self.images, self.screen, self.fit)
