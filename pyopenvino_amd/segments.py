"""The class map of a segmentation network's Result (``infer(..., segments=...)``): the rule, the argument checks and the device launch.
DeepLab-style heads, road and lane segmentation, sigmoid masks: a Result (n, C, H, W), one plane of scores per batch row and class.

The rule (include/pvhip.h, pvhip_segment_labels_f32; tests/segments_ref.py is the same again in plain loops), for pixel (y, x) of batch
row r, with v[c] = X[r, c, y, x]:
  1. best    c* is the first class of the pixel's C values in top_k's total order: NaN of any sign or payload first, then descending
     with +0.0 == -0.0, ties to the lower class.
  2. void    the pixel is void iff v[c*] is NaN or (min_score is given and v[c*] < float32(min_score)).  Any NaN among a pixel's C
     scores therefore voids it: the quiet-NaN rows behind `count` of a DetectedRois or LandmarkWarps pass are void all through.
     Equality keeps.
  3. label   labels[r, y, x] = c*, or 255 when void.  With C == 1 and a min_score: the thresholded mask of a sigmoid head.
  4. sums    areas[r, c] is the number of pixels of row r labelled c -- the void pixels of a row are H * W - areas[r].sum() --;
     extents[r, c] = (x0, y0, x1, y1) is min x, min y, max x + 1 and max y + 1 over those pixels, (0, 0, 0, 0) where there is none.
     Exact integers: the order in which they are accumulated does not matter.
Out of scope here: a per-pixel confidence map, softmax, NHWC or FP16 Results, more than 255 classes, contours and polygons.

FrameSegmentScreen answers the same ``Segments`` in FRAME pixels: the planes upsampled bilinearly to the frame the network was fed, the
letterbox removed, and the best class taken after the upsampling -- F.interpolate(logits, size, mode='bilinear',
align_corners=False).argmax(1), which gives smooth class borders where resizing the label map gives staircases.  The geometry
(frame_size, fit = (dx, dy, iw, ih)) of a pass is learned as boxes.Ask.bound learns it (boxes.geometry_of): the identity (0, 0, Wn, Hn)
over frame_size or (Hn, Wn) when nothing was fitted; InputFormat.fit_geometry(extent fed) over frame_size or that extent when the input
declares a resize_fit and was fed host frames.  The frame rule (include/pvhip.h, pvhip_segment_frame_labels_f32;
tests/segments_frame_ref.py is the same again in plain loops; exact, no tolerance anywhere), for frame pixel (X, Y) of batch row r, with
L[c] = X[r, c]:
  1. position  rule 2 of masks.py word for word, with (Wp, Hp) := (W, H): in exact integers N = (2 dx F + (2 X + 1) iw) W - F Wn and
     D = 2 F Wn with F = frame_w; P = floor(65536 N / D), floor toward minus infinity; the taps P >> 16 and (P >> 16) + 1 clamped to
     [0, W - 1]; fx = float32(P & 65535) / 65536.  Rows alike with (dy, ih, frame_h, H, Hn).
  2. value     for every class c: t0 = L[c][ya][xa] + fx * (L[c][ya][xb] - L[c][ya][xa]), t1 likewise on row yb, v[c] = t0 + fy *
     (t1 - t0): every operation float32, rounded once, no fma; all four taps are always read; no special cases, NaN and inf follow IEEE,
     so inf - inf next to the pixel voids it.
  3. best, void, label  rules 1 to 3 above on v[c]: the first class in top_k's total order, ties to the lower class; void iff the
     best is NaN or below float32(min_score), equality keeps; 255 when void.
  4. sums      rule 4 above over frame pixels.
Consequence: with the identity geometry and frame == network == map extent every fraction is 0 and a + 0 * (b - a) = a: on finite
planes the answer is `labels` bit for bit.  Where this differs from the usual host route: one interpolation goes straight from the map
to the frame through the letterbox (users otherwise upsample to the network's extent, cut the padding and resize again); fractions are
Q16.  Out of scope there as well: bicubic or antialiased sampling, per-row geometries (a RoiInput or DetectedRois feed on a fitted input).
H, W <= 4096; network, fit and frame extents <= 16384 (masks.MAX_FRAME_PLANE / MAX_FRAME_EXTENT: the integers of 1. stay below 2^59);
n * Fh * Fw < 2^31."""
import collections
import ctypes

import numpy as np

from . import ask, boxes, device, masks

VOID = 255                                      # PVHIP_SEGMENT_VOID
MAX_CLASSES = 255                               # PVHIP_SEGMENT_MAX_CLASSES: a label is a byte, and 255 says void
MAX_PLANE = 1 << 24                             # PVHIP_SEGMENT_MAX_PLANE: H * W at most

SegmentScreen = collections.namedtuple('SegmentScreen', 'min_score', defaults=(None,))
SegmentScreen.__doc__ = ('How to read a segmentation Result: a pixel is void (label 255) when its best score is below `min_score` (None: only '
                         'where a score is NaN).')

FrameSegmentScreen = collections.namedtuple('FrameSegmentScreen', 'min_score frame_size input', defaults=(None, None, None))
FrameSegmentScreen.__doc__ = ('How to read a segmentation Result in frame pixels: `min_score` as SegmentScreen\'s; `frame_size` = (Fh, Fw) '
                              'overrides the extent of the frames (None: the network\'s extent, or that of the host frames a fitted input '
                              'was fed); `input` names the network\'s 4-D Parameter when there are several.')
FORM_NONE, FORM_STAGED, FORM_DIRECT = 0, 1, 2   # PVHIP_SEGMENT_FRAME_FORM_*
FRAME_BAND_ROWS, FRAME_COL_CHUNK, FRAME_CLASS_CHUNK = 16, 252, 32      # PVHIP_SEGMENT_FRAME_BAND_ROWS, _COL_CHUNK, _CLASS_CHUNK

Segments = collections.namedtuple('Segments', 'labels areas extents')
Segments.__doc__ = ('What a Result started with segments= comes back as: `labels` (n, H, W) uint8 the class of every pixel, 255 where void, '
                    '`areas` (n, C) int32 pixels per row and class, `extents` (n, C, 4) int32 (x0, y0, x1, y1) of each class\'s pixels, zeros '
                    'where it has none.  With a FrameSegmentScreen all three are over frame pixels: `labels` (n, Fh, Fw).')


def resolved(value, what='segments'):
    """`value` -- a SegmentScreen, a FrameSegmentScreen, a real number (a SegmentScreen's min_score) or True (the default SegmentScreen)
    -- as a checked screen of its type (a FrameSegmentScreen's `input` is the caller's: checked() knows the network); ValueError."""
    if value is True:
        value = SegmentScreen()
    elif not isinstance(value, (bool, SegmentScreen, FrameSegmentScreen)) and isinstance(value, (int, float, np.integer, np.floating)):
        value = SegmentScreen(value)
    if not isinstance(value, (SegmentScreen, FrameSegmentScreen)):
        raise ValueError('{}: a SegmentScreen, a min_score or True (or a FrameSegmentScreen), got {!r}'.format(what, value))
    min_score = None if value.min_score is None else ask.checked_min_score(value.min_score, what)
    if isinstance(value, SegmentScreen):
        return SegmentScreen(min_score)
    frame = value.frame_size
    if frame is not None:
        frame = _extent(frame)
        if frame is None:
            raise ValueError('{}: frame_size is None or (Fh, Fw) with both in 1 .. {}, got {!r}'.format(what, masks.MAX_FRAME_EXTENT, value.frame_size))
    return FrameSegmentScreen(min_score, frame, value.input)


def _extent(pair):
    """`pair` as two ints in 1 .. 16384, else None."""
    try:
        pair = tuple(pair)
    except TypeError:
        return None
    if len(pair) != 2 or not all(not isinstance(v, bool) and isinstance(v, (int, np.integer)) and 1 <= v <= masks.MAX_FRAME_EXTENT for v in pair):
        return None
    return int(pair[0]), int(pair[1])


def checked_frame(what, n, H, W, net_hw=None, frame=None, fit=None):
    """What the frame rule asks of the extents it knows (None: not yet known); ValueError('{what}: ...')."""
    if max(H, W) > masks.MAX_FRAME_PLANE:
        raise ValueError('{}: a FrameSegmentScreen takes maps of at most 4096 x 4096, got {} x {}'.format(what, H, W))
    if net_hw is not None and (max(net_hw) > masks.MAX_FRAME_EXTENT or (fit is not None and max(fit) > masks.MAX_FRAME_EXTENT)):
        raise ValueError('{}: a FrameSegmentScreen takes a network extent of at most 16384 x 16384, got {} x {}'.format(what, *net_hw))
    if frame is not None and (max(frame) > masks.MAX_FRAME_EXTENT or n * frame[0] * frame[1] >= 1 << 31):
        raise ValueError('{}: a FrameSegmentScreen takes frames of at most 16384 x 16384 with n * Fh * Fw < 2^31, got {} of {} x {}'.format(what, n, *frame))


def maps_of(dims, batch=None):
    """(n, C, H, W) of a tensor declared as a stack of per-class score planes -- 4-D, n the batch (when given), 1 <= C <= 255,
    2 <= H * W <= 2^24 --, else None."""
    dims = tuple(int(d) for d in dims)
    if len(dims) != 4 or min(dims) < 1 or dims[1] > MAX_CLASSES or not 2 <= dims[2] * dims[3] <= MAX_PLANE \
            or (batch is not None and dims[0] != int(batch)):
        return None
    return dims


def sums(labelled, C: int):
    """Rule 4 of a (n, H, W) uint8 class map: (areas (n, C) int32, extents (n, C, 4) int32)."""
    n, H, W = labelled.shape
    areas = np.zeros((n, C), np.int32)
    extents = np.zeros((n, C, 4), np.int32)
    for r in range(n):
        areas[r] = np.bincount(labelled[r].reshape(-1), minlength=256)[:C]
        for c in np.flatnonzero(areas[r]):
            at = labelled[r] == c
            ys, xs = np.flatnonzero(at.any(axis=1)), np.flatnonzero(at.any(axis=0))
            extents[r, c] = (xs[0], ys[0], xs[-1] + 1, ys[-1] + 1)
    return areas, extents


def labels(x, screen=True) -> Segments:
    """The rule in numpy on a host array of shape (n, C, H, W): what a Result computed on the host (a foreign plugin set) gets."""
    screen = resolved(screen, 'labels')
    if not isinstance(screen, SegmentScreen):
        raise ValueError('labels: a FrameSegmentScreen is frame_labels\' to answer, got {!r}'.format(screen))
    (min_score,) = screen
    x = np.asarray(x)
    if x.dtype != np.float32 or maps_of(x.shape) is None:
        raise ValueError('labels takes float32 scores of shape (n, C, H, W) with C <= 255 and 2 <= H * W <= 2^24, got {} {}'.format(x.dtype, x.shape))
    C = x.shape[1]
    nan = np.isnan(x)
    void = nan.any(axis=1)
    # the first NaN where there is one, else the first of the largest values (argmax takes +0.0 == -0.0 and the lower class)
    best = np.where(void, nan.argmax(axis=1), np.where(nan, -np.inf, x).argmax(axis=1))
    if min_score is not None:
        with np.errstate(invalid='ignore'):
            void = void | (np.take_along_axis(x, best[:, None], axis=1)[:, 0] < np.float32(min_score))
    labelled = np.where(void, VOID, best).astype(np.uint8)
    return Segments(labelled, *sums(labelled, C))


def frame_labels(x, screen, net_hw, frame_size, fit=None) -> Segments:
    """The frame rule in numpy on a host array of shape (n, C, H, W): `net_hw` = (Hn, Wn), the extent of the network's input, over frames
    of `frame_size` = (Fh, Fw) that stand in the rectangle `fit` = (dx, dy, iw, ih) of that input (None: the identity).  `screen`: anything
    segments= takes; only its min_score is read."""
    min_score = resolved(screen, 'frame_labels').min_score
    x = np.asarray(x)
    if x.dtype != np.float32 or maps_of(x.shape) is None:
        raise ValueError('frame_labels takes float32 scores of shape (n, C, H, W) with C <= 255 and 2 <= H * W, got {} {}'.format(x.dtype, x.shape))
    n, C, H, W = x.shape
    net, frame = _extent(net_hw), _extent(frame_size)
    if net is None or frame is None:
        raise ValueError('frame_labels: net_hw and frame_size are (h, w) with both in 1 .. 16384, got {!r} and {!r}'.format(net_hw, frame_size))
    (hn, wn), (fh, fw) = net, frame
    dx, dy, iw, ih = (0, 0, wn, hn) if fit is None else boxes.checked_fit(fit, 'frame_labels')
    checked_frame('frame_labels', n, H, W, net, frame, (dx, dy, iw, ih))
    xa, xb, fx = masks.taps(0, fw, dx, iw, fw, W, wn)
    ya, yb, fy = masks.taps(0, fh, dy, ih, fh, H, hn)
    fx, fy = fx[None, :], fy[:, None]
    labelled = np.empty((n, fh, fw), np.uint8)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        for r in range(n):                      # a frame at a time: one class's (Fh, Fw) values and the running best
            best = cls = locked = None
            for c in range(C):
                top, bot = x[r, c][ya], x[r, c][yb]
                t0 = top[:, xa] + fx * (top[:, xb] - top[:, xa])
                t1 = bot[:, xa] + fx * (bot[:, xb] - bot[:, xa])
                v = t0 + fy * (t1 - t0)
                nan = np.isnan(v)
                if c == 0:
                    best, cls, locked = v, np.zeros(v.shape, np.uint8), nan
                    continue
                take = ~locked & (nan | (v > best))         # the first NaN stays; strictly larger: ties and zeros stay with the lower class
                best, cls = np.where(take, v, best), np.where(take, np.uint8(c), cls)
                locked = locked | nan
            void = locked if min_score is None else locked | (best < np.float32(min_score))
            labelled[r] = np.where(void, np.uint8(VOID), cls)
    return Segments(labelled, *sums(labelled, C))


def _fits(port, screen, batch):
    dims = maps_of(port['dims'], batch)
    return dims is not None and port['precision'] == 'FP32' and not (dims[:2] == (1, 1) and dims[3] == 7)


def _none_fits(ports, screen, batch):
    return 'segments: no FP32 Result of shape (n = {}, C <= 255, H, W) with 2 <= H * W <= 2^24 (the Results: {})'.format(
        batch, {name: tuple(port['dims']) for name, port in ports.items()})


def checked(ienet, segments, sharded: bool) -> dict:
    """{Result name: resolved SegmentScreen or FrameSegmentScreen, its `input` named} of the `segments` argument of infer() / start_async() -- a SegmentScreen, a FrameSegmentScreen, a min_score or True
    for every FP32 Result declared (n, C, H, W) with n the batch, 1 <= C <= 255, 2 <= H * W <= 2^24 and not of the detector shape
    (1, 1, R, 7), or {Result name: any of these} --, {} for None.  Everything is looked up in the network as it was read: no device is
    needed, nothing is allocated.  ValueError ('segments: ...'): an unknown name, a value of another type, min_score not a finite real of
    float32, no such Result for an unnamed form, a sharded batch, a Result of another rank, shape or precision, more than 255 classes;
    for a FrameSegmentScreen also a bad frame_size or input, a map above 4096 x 4096, a network or frame extent above 16384."""
    if segments is None:
        return {}
    batch = int(ienet.batch_size)
    ports, wanted = ask.named(ienet, 'segments', segments, sharded, _fits, _none_fits, resolved)
    for name, screen in wanted.items():
        dims = ask.declared('segments', name, ports[name], maps_of(ports[name]['dims'], batch), '(n = {}, C <= 255, H, W) with 2 <= H * W <= 2^24', batch)
        if isinstance(screen, FrameSegmentScreen):      # its input named, and what is known of the extents before a pass is fed
            what = 'segments: Result {!r}'.format(name)
            screen = wanted[name] = screen._replace(input=boxes.checked_input(ienet, screen, what))
            checked_frame(what, batch, dims[2], dims[3], boxes.extent_of(ienet, screen.input), screen.frame_size)
    return wanted


class Blocks(ask.FlatBlocks):
    """What a request keeps for one Result name: the device block pvhip_segment_labels_f32 writes -- (n, H, W) uint8 labels in
    ceil(n H W / 4) words, (n, C) int32 areas, (n, C, 4) int32 extents -- and the page-locked host block it is read back into in one
    copy of 4 ceil(n H W / 4) + 20 n C bytes.  Neither depends on min_score, which is an argument of the launch."""
    __slots__ = ('shape', 'label_words', 'extent')

    def __init__(self, n: int, C: int, H: int, W: int, extent=None):
        self.shape, self.extent = (n, C, H, W), extent or (H, W)        # extent: that of the labels
        self.label_words = (n * self.extent[0] * self.extent[1] + 3) // 4
        super().__init__(self.label_words + 5 * n * C)

    def launch(self, result, min_score):
        """One call on the current stream, behind whatever wrote `result` there."""
        n, C, H, W = maps_of(result.shape)
        assert (n, C, H, W) == self.shape and result.dtype == np.float32
        at = self.dev.ptr + 4 * self.label_words
        device.call('pvhip_segment_labels_f32', device.ptr(result), n, C, H, W, int(min_score is not None), float(min_score or 0.0),
                    ctypes.c_void_p(self.dev.ptr), ctypes.c_void_p(at), ctypes.c_void_p(at + 4 * n * C))

    def read_back(self) -> Segments:
        """The answer, copied on the current stream, which has drained; the arrays are the caller's own.  The entry leaves (W, H, 0, 0)
        for a class without pixels: zeros here."""
        host, (n, C, _, _), (H, W), lw = self.words(), self.shape, self.extent, self.label_words
        areas = host[lw:lw + n * C].reshape(n, C).copy()
        extents = host[lw + n * C:].reshape(n, C, 4).copy()
        extents[areas == 0] = 0
        return Segments(host[:lw].view(np.uint8)[:n * H * W].reshape(n, H, W).copy(), areas, extents)


class Ask(ask.Ask, collections.namedtuple('Ask', 'screen')):
    """A Result asked for with segments=, in its resolved form."""
    __slots__ = ()
    KEYWORD = 'segments'

    def key(self, name):
        """(name,).  min_score is no part of it: it goes with the launch."""
        return (name,)

    def blocks_for(self, value):
        return Blocks(*maps_of(value.shape))

    def launch_with(self):
        return (self.screen.min_score,)

    def on_host(self, value):
        return labels(value, self.screen)


class FrameBlocks(Blocks):
    """What a request keeps for one (Result name, frame extent): the device block pvhip_segment_frame_labels_f32 writes -- (n, Fh, Fw) uint8
    labels in ceil(n Fh Fw / 4) words, (n, C) int32 areas, (n, C, 4) int32 extents -- and its page-locked twin, read back in one copy of
    4 ceil(n Fh Fw / 4) + 20 n C bytes.  min_score and the fit are arguments of the launch."""
    __slots__ = ()

    def launch(self, result, min_score, net_hw, frame_size, fit):
        """One call on the current stream, behind whatever wrote `result` there."""
        n, C, H, W = maps_of(result.shape)
        assert (n, C, H, W) == self.shape and tuple(frame_size) == self.extent and result.dtype == np.float32
        at = self.dev.ptr + 4 * self.label_words
        device.call('pvhip_segment_frame_labels_f32', device.ptr(result), n, C, H, W, net_hw[0], net_hw[1], frame_size[0], frame_size[1],
                    fit[0], fit[1], fit[2], fit[3], int(min_score is not None), float(min_score or 0.0),
                    ctypes.c_void_p(self.dev.ptr), ctypes.c_void_p(at), ctypes.c_void_p(at + 4 * n * C))


class FrameAsk(ask.Ask, collections.namedtuple('FrameAsk', 'screen net_hw format frame_size fit')):
    """A Result asked for with segments=FrameSegmentScreen(...), its screen resolved: `net_hw` the extent of the screen's input; `format`
    that input's InputFormat when it declares a fit, else None; `frame_size` and `fit` = (dx, dy, iw, ih), the geometry of the pass, known
    once its inputs are staged (bound), as boxes.Ask's are.  Unlike a boxes ask's, the blocks' size depends on the frame extent: a request
    keeps one block pair per frame extent it has answered, until release_device_state()."""
    __slots__ = ()
    KEYWORD = 'segments'

    def bound(self, inputs, slots):
        frame, fit = boxes.geometry_of('segments', self.screen.input, self.screen.frame_size, self.net_hw, self.format, slots)
        if max(frame) > masks.MAX_FRAME_EXTENT:
            raise ValueError('segments: a FrameSegmentScreen takes frames of at most 16384 x 16384, got {} x {}'.format(*frame))
        return self._replace(frame_size=(int(frame[0]), int(frame[1])), fit=fit)

    def key(self, name):
        """(name, 'FRAME', Fh, Fw): the frame extent sizes the labels; min_score and the fit go with the launch."""
        return (name, 'FRAME') + tuple(self.frame_size)

    def blocks_for(self, value):
        n, C, H, W = maps_of(value.shape)
        checked_frame('segments', n, H, W, self.net_hw, self.frame_size, self.fit)
        return FrameBlocks(n, C, H, W, tuple(self.frame_size))

    def launch_with(self):
        return (self.screen.min_score, self.net_hw, self.frame_size, self.fit)

    def on_host(self, value):
        return frame_labels(value, self.screen, self.net_hw, self.frame_size, self.fit)
