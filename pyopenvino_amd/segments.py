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
     Exact integers: the order in which they are accumulated does not matter."""
import collections
import ctypes

import numpy as np

from . import ask, device

VOID = 255                                      # PVHIP_SEGMENT_VOID
MAX_CLASSES = 255                               # PVHIP_SEGMENT_MAX_CLASSES: a label is a byte, and 255 says void
MAX_PLANE = 1 << 24                             # PVHIP_SEGMENT_MAX_PLANE: H * W at most

SegmentScreen = collections.namedtuple('SegmentScreen', 'min_score', defaults=(None,))
SegmentScreen.__doc__ = ('How to read a segmentation Result: a pixel is void (label 255) when its best score is below `min_score` (None: only '
                         'where a score is NaN).')

Segments = collections.namedtuple('Segments', 'labels areas extents')
Segments.__doc__ = ('What a Result started with segments= comes back as: `labels` (n, H, W) uint8 the class of every pixel, 255 where void, '
                    '`areas` (n, C) int32 pixels per row and class, `extents` (n, C, 4) int32 (x0, y0, x1, y1) of each class\'s pixels, zeros '
                    'where it has none.')


def resolved(value, what='segments') -> SegmentScreen:
    """`value` -- a SegmentScreen, a real number (its min_score) or True (the default screen) -- as a checked SegmentScreen; ValueError."""
    if value is True:
        value = SegmentScreen()
    elif not isinstance(value, (bool, SegmentScreen)) and isinstance(value, (int, float, np.integer, np.floating)):
        value = SegmentScreen(value)
    if not isinstance(value, SegmentScreen):
        raise ValueError('{}: a SegmentScreen, a min_score or True, got {!r}'.format(what, value))
    (min_score,) = value
    return SegmentScreen(None if min_score is None else ask.checked_min_score(min_score, what))


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
    (min_score,) = resolved(screen, 'labels')
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


def _fits(port, screen, batch):
    dims = maps_of(port['dims'], batch)
    return dims is not None and port['precision'] == 'FP32' and not (dims[:2] == (1, 1) and dims[3] == 7)


def _none_fits(ports, screen, batch):
    return 'segments: no FP32 Result of shape (n = {}, C <= 255, H, W) with 2 <= H * W <= 2^24 (the Results: {})'.format(
        batch, {name: tuple(port['dims']) for name, port in ports.items()})


def checked(ienet, segments, sharded: bool) -> dict:
    """{Result name: resolved SegmentScreen} of the `segments` argument of infer() / start_async() -- a SegmentScreen, a min_score or True
    for every FP32 Result declared (n, C, H, W) with n the batch, 1 <= C <= 255, 2 <= H * W <= 2^24 and not of the detector shape
    (1, 1, R, 7), or {Result name: any of these} --, {} for None.  Everything is looked up in the network as it was read: no device is
    needed, nothing is allocated.  ValueError ('segments: ...'): an unknown name, a value of another type, min_score not a finite real of
    float32, no such Result for an unnamed form, a sharded batch, a Result of another rank, shape or precision, more than 255 classes."""
    if segments is None:
        return {}
    batch = int(ienet.batch_size)
    ports, wanted = ask.named(ienet, 'segments', segments, sharded, _fits, _none_fits, resolved)
    for name in wanted:
        ask.declared('segments', name, ports[name], maps_of(ports[name]['dims'], batch), '(n = {}, C <= 255, H, W) with 2 <= H * W <= 2^24', batch)
    return wanted


class Blocks(ask.FlatBlocks):
    """What a request keeps for one Result name: the device block pvhip_segment_labels_f32 writes -- (n, H, W) uint8 labels in
    ceil(n H W / 4) words, (n, C) int32 areas, (n, C, 4) int32 extents -- and the page-locked host block it is read back into in one
    copy of 4 ceil(n H W / 4) + 20 n C bytes.  Neither depends on min_score, which is an argument of the launch."""
    __slots__ = ('shape', 'label_words')

    def __init__(self, n: int, C: int, H: int, W: int):
        self.shape, self.label_words = (n, C, H, W), (n * H * W + 3) // 4
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
        host, (n, C, H, W), lw = self.words(), self.shape, self.label_words
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
