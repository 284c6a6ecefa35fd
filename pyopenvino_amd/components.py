"""The connected components of a probability map (``infer(..., components=...)``): the rule, the argument checks and the device launch.
Text detectors that do not regress boxes (DBNet, PixelLink-style ``text-detection-000x``, PSENet, CRAFT's region map) and blob heads
(cell and crowd localisation, defect and lane masks, any sigmoid mask whose objects are wanted one by one): a Result (n, K, H, W) of
which one plane per batch row is thresholded and its foreground grouped into objects -- what ``cv2.connectedComponentsWithStats`` does
on the host after the whole map was read back.

The rule (include/pvhip.h, pvhip_components_f32; tests/components_ref.py is the same again in plain loops; exact: every output is an
integer or the Result's own bits, no tolerance anywhere), for the plane P = X[r, channel] of batch row r:
  1. foreground  pixel p is foreground iff P[p] is not NaN and P[p] >= float32(min_score); equality keeps.  A NaN is background: the
     quiet-NaN rows behind `count` of a DetectedRois or LandmarkWarps pass have found = counts = 0.
  2. components  two foreground pixels of the same plane are joined when they are horizontal or vertical neighbours and, with
     connectivity == 8, when they are diagonal neighbours.  Neighbours are taken in (y, x), never in the flat index: column W - 1 and
     column 0 of the next row are no neighbours, nor are the last row of image r and the first of r + 1.  A component is a class of the
     transitive closure; its seed is its smallest flat index y * W + x.
  3. statistics  area; the rectangle (min x, min y, max x - min x + 1, max y - min y + 1); peak, the first of its scores in top_k's order
     among numbers (descending, +0.0 == -0.0), as the bits of the first such pixel in raster order; sum = the sum of
     llrint(clamp(float64(v), -32768, 32768) * 65536), ties to even -- an exact int64 whatever the order of addition --; the five moments
     sum x, sum y, sum x x, sum x y, sum y y over the pixel indices, int64 (modulo 2^64, which only a plane with a side above 2^19 can reach).
  4. selection   found[r] counts all components; those with area >= min_area are ranked by descending area, ties to the lower seed; the
     first max_per_image are answered, and counts[r] is their number.
Out of scope here: a label map in the answer, contours, polygons and exact minimum-area rectangles (``oriented`` gives the rectangle of
the second moments), PixelLink's link channels, components per class of a ``segments`` map, frame-space answers through a letterbox fit
(``to_frame`` scales an identity fit), a device-resident table for DetectedRois-style chaining, FP16 / NHWC Results, more than 1024
components per image."""
import collections
import ctypes

import numpy as np

from . import ask, device, maxima, segments

MAX_AREA = 1 << 24                              # PVHIP_COMPONENTS_MAX_PLANE: H * W, and so min_area, at most
MAX_PER_IMAGE = 1024                            # PVHIP_COMPONENTS_MAX_PER_IMAGE
TILE_ROWS, TILE_COLS = 32, 128                  # PVHIP_COMPONENTS_TILE_ROWS, _COLS
NO_ZERO = 0x7FFFFFFF                            # `zeros` of a component whose peak is no zero

ComponentScreen = collections.namedtuple('ComponentScreen', 'min_score channel connectivity min_area max_per_image', defaults=(0.3, 0, 8, 1, 256))
ComponentScreen.__doc__ = ('How to read a probability map: a pixel of plane `channel` (-K .. K - 1, negative from the end) is foreground when it is at '
                           'least `min_score`; foreground pixels are joined over `connectivity` (4 or 8) neighbours; of the components of at least '
                           '`min_area` (1 .. 2^24) pixels the `max_per_image` (1 .. 1024) largest of each batch row are answered.')

class Components(collections.namedtuple('Components', 'counts found rois areas seeds peaks sums moments')):
    """What a Result started with components= comes back as, flat in (image, rank) order: `counts` (n,) int32 rows per image, `found` (n,)
    int32 components per image before min_area and the cap, `rois` (total, 5) int32 (image, x, y, w, h) in map pixels (RoiInput's order),
    `areas` (total,) int32, `seeds` (total,) int32 smallest flat index y * W + x, `peaks` (total,) float32 the largest score's own bits,
    `sums` (total,) int64 Q16 sum of scores (sums / areas / 65536: the mean), `moments` (total, 5) int64 sum x, sum y, sum x x, sum x y,
    sum y y."""
    __slots__ = ()

    def of(self, r: int):
        """The rows of image r: a Components of that one image."""
        first, last = int(self.counts[:r].sum()), int(self.counts[:r + 1].sum())
        return Components(self.counts[r:r + 1], self.found[r:r + 1], *(field[first:last] for field in self[2:]))


def _checked_int(value, least, most, what, field):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not least <= int(value) <= most:
        raise ValueError('{}: {} is an int in {} .. {}, got {!r}'.format(what, field, least, most, value))
    return int(value)


def resolved(value, what='components') -> ComponentScreen:
    """`value` -- a ComponentScreen, a real number (its min_score) or True (the default screen) -- as a checked ComponentScreen (its
    channel is held against K where the Result is known: for_planes); ValueError."""
    if value is True:
        value = ComponentScreen()
    elif not isinstance(value, (bool, ComponentScreen)) and isinstance(value, (int, float, np.integer, np.floating)):
        value = ComponentScreen(value)
    if not isinstance(value, ComponentScreen):
        raise ValueError('{}: a ComponentScreen, a min_score or True, got {!r}'.format(what, value))
    min_score, channel, connectivity, min_area, most = value
    if min_score is None:
        raise ValueError('{}: min_score is a finite real (of float32), got None'.format(what))
    if isinstance(connectivity, (bool, np.bool_)) or not isinstance(connectivity, (int, np.integer)) or int(connectivity) not in (4, 8):
        raise ValueError('{}: connectivity is 4 or 8, got {!r}'.format(what, connectivity))
    return ComponentScreen(ask.checked_min_score(min_score, what), _checked_int(channel, -segments.MAX_CLASSES, segments.MAX_CLASSES - 1, what, 'channel'),
                           int(connectivity), _checked_int(min_area, 1, MAX_AREA, what, 'min_area'), _checked_int(most, 1, MAX_PER_IMAGE, what, 'max_per_image'))


def planes_of(dims, batch=None):
    """(n, K, H, W) of a tensor declared as a stack of score planes -- segments' family: 4-D, n the batch (when given), 1 <= K <= 255,
    2 <= H * W <= 2^24 -- with n * H * W < 2^31, else None."""
    dims = segments.maps_of(dims, batch)
    return dims if dims is not None and dims[0] * dims[2] * dims[3] < 1 << 31 else None


def for_planes(screen: ComponentScreen, K: int, what='components') -> ComponentScreen:
    """`screen`, resolved, for a Result of K planes: its channel counted from the front; ValueError when it is outside -K .. K - 1."""
    if not -K <= screen.channel < K:
        raise ValueError('{}: channel {} is outside {} .. {} of its K = {} planes'.format(what, screen.channel, -K, K - 1, K))
    return screen._replace(channel=screen.channel % K)


def _plane(plane, cut, eight, min_area, most):
    """Rules 1 to 4 on one (H, W) float32 plane: (found, seeds, areas, rects (x, y, w, h), peak bits, sums, moments) of the answered."""
    H, W = plane.shape
    with np.errstate(invalid='ignore'):
        fg = plane >= cut                                       # (a NaN compares false)
    edges = np.diff(np.pad(fg, ((0, 0), (1, 1))).astype(np.int8), axis=1)
    row, s = np.nonzero(edges == 1)                             # the runs, in raster order: row, first column, column behind the last
    e = np.nonzero(edges == -1)[1]
    runs = row.size
    parent = list(range(runs))
    if runs:                                                    # the runs of row y - 1 that touch run b of row y: a contiguous range
        c, S = int(eight), W + 3
        lo = np.searchsorted((row + 1) * S + e, row * S + s - c, 'right')
        hi = np.searchsorted((row + 1) * S + s, row * S + e + c, 'left')
        for b in np.flatnonzero(hi > lo):
            for a in range(lo[b], hi[b]):
                u, v = a, int(b)
                while parent[u] != u:
                    parent[u] = u = parent[parent[u]]
                while parent[v] != v:
                    parent[v] = v = parent[parent[v]]
                if u != v:
                    parent[max(u, v)] = min(u, v)              # a root is the first run of its component: the seed's
    for i in range(runs):                                       # (parents are below: one pass flattens)
        parent[i] = parent[parent[i]]
    root, comp = np.unique(np.asarray(parent, np.int64), return_inverse=True)
    found = root.size
    length = (e - s).astype(np.int64)
    y, x0, x1 = row.astype(np.int64), s.astype(np.int64), e.astype(np.int64) - 1

    def total(values):
        out = np.zeros(found, np.int64)
        np.add.at(out, comp, values)
        return out

    squares = lambda k: k * (k + 1) * (2 * k + 1) // 6          # 0 + 1 + 4 + ... + k k
    areas = total(length)
    sx = (x0 + x1) * length // 2
    moments = np.stack([total(sx), total(y * length), total(squares(x1) - squares(x0 - 1)), total(y * sx), total(y * y * length)], axis=1)
    left, top = np.full(found, W, np.int64), np.full(found, H, np.int64)
    right, bottom = np.full(found, -1, np.int64), np.full(found, -1, np.int64)
    np.minimum.at(left, comp, x0), np.minimum.at(top, comp, y), np.maximum.at(right, comp, x1), np.maximum.at(bottom, comp, y)
    seeds = (row[root] * W + s[root]).astype(np.int64) if runs else np.zeros(0, np.int64)
    # per pixel, in raster order -- the order of the runs
    of_pixel = np.repeat(comp, length)
    at = np.flatnonzero(fg.reshape(-1))
    values = plane.reshape(-1)[at]
    sums = np.zeros(found, np.int64)
    np.add.at(sums, of_pixel, np.rint(np.clip(values.astype(np.float64), -32768.0, 32768.0) * 65536.0).astype(np.int64))
    words = maxima.order_words(values)
    best = np.zeros(found, np.uint32)
    np.maximum.at(best, of_pixel, words)
    first = np.full(found, H * W, np.int64)
    np.minimum.at(first, of_pixel, np.where(words == best[of_pixel], at, H * W))
    order = np.lexsort((seeds, -areas))
    order = order[areas[order] >= min_area][:most]
    rects = np.stack([left, top, right - left + 1, bottom - top + 1], axis=1)
    peaks = plane.reshape(-1).view(np.uint32)[first[order]] if found else np.zeros(0, np.uint32)
    return found, seeds[order], areas[order], rects[order], peaks, sums[order], moments[order]


def find(x, screen=True) -> Components:
    """The rule in numpy on a host array of shape (n, K, H, W): what a Result computed on the host (a foreign plugin set) gets."""
    screen = resolved(screen, 'find')
    x = np.asarray(x)
    if x.dtype != np.float32 or planes_of(x.shape) is None:
        raise ValueError('find takes float32 scores of shape (n, K, H, W) with K <= 255, 2 <= H * W <= 2^24 and n * H * W < 2^31, got {} {}'.format(
            x.dtype, x.shape))
    n, K, H, W = x.shape
    min_score, channel, connectivity, min_area, most = for_planes(screen, K, 'find')
    x = np.ascontiguousarray(x)
    parts = [_plane(x[r, channel], np.float32(min_score), connectivity == 8, min_area, most) for r in range(n)]
    counts = np.array([p[1].size for p in parts], np.int32)
    join = lambda i, dtype: np.concatenate([p[i] for p in parts]).astype(dtype)
    rois = np.concatenate([np.repeat(np.arange(n), counts)[:, None], join(3, np.int64).reshape(-1, 4)], axis=1).astype(np.int32)
    return Components(counts, np.array([p[0] for p in parts], np.int32), rois, join(2, np.int32), join(1, np.int32),
                      join(4, np.uint32).view(np.float32), join(5, np.int64), join(6, np.int64).reshape(-1, 5))


def oriented(answer: Components) -> np.ndarray:
    """(total, 5) float64 (cx, cy, w, h, angle_deg) of every component: the centroid on pixel-edge coordinates and the rectangle of
    its second moments -- each pixel a unit square, the sides sqrt(12 lambda) along the principal axes, w the longer, the angle that of
    w's axis from +x towards +y in (-90, 90] --: the arguments of ``warp.rotated_rect``, so that a slanted text line goes to a WarpInput.
    Exact for a filled rectangle along the axes; for any other shape the rectangle with its moments, not the minimum-area one."""
    area = answer.areas.astype(np.float64)
    sx, sy, sxx, sxy, syy = (answer.moments[:, i].astype(np.float64) for i in range(5))
    mx, my = sx / area, sy / area
    cxx, cxy, cyy = sxx / area - mx * mx + 1.0 / 12.0, sxy / area - mx * my, syy / area - my * my + 1.0 / 12.0
    half, root = (cxx + cyy) / 2.0, np.sqrt(((cxx - cyy) / 2.0) ** 2 + cxy * cxy)
    angle = np.degrees(0.5 * np.arctan2(2.0 * cxy, cxx - cyy))
    return np.stack([mx + 0.5, my + 0.5, np.sqrt(12.0 * (half + root)), np.sqrt(12.0 * np.maximum(half - root, 0.0)), angle], axis=1)


def to_frame(rois, map_hw, frame_hw) -> np.ndarray:
    """`rois` (total, 5) (image, x, y, w, h) in map pixels as rectangles of frames of `frame_hw` = (Fh, Fw) that the map of `map_hw` =
    (H, W) covers whole (the identity fit only): the left and top edges floored, the right and bottom ones ceiled, in exact integers."""
    rois = np.asarray(rois, np.int64).reshape(-1, 5)
    (H, W), (Fh, Fw) = (int(v) for v in map_hw), (int(v) for v in frame_hw)
    if min(H, W, Fh, Fw) < 1:
        raise ValueError('to_frame: map_hw and frame_hw are (h, w) with both >= 1, got {!r} and {!r}'.format(map_hw, frame_hw))
    x0, y0 = rois[:, 1] * Fw // W, rois[:, 2] * Fh // H
    x1, y1 = -((rois[:, 1] + rois[:, 3]) * -Fw // W), -((rois[:, 2] + rois[:, 4]) * -Fh // H)
    return np.stack([rois[:, 0], x0, y0, x1 - x0, y1 - y0], axis=1).astype(np.int32)


def _fits(port, screen, batch):
    dims = planes_of(port['dims'], batch)
    return dims is not None and port['precision'] == 'FP32' and not (dims[:2] == (1, 1) and dims[3] == 7) and -dims[1] <= screen.channel < dims[1]


SHAPE = '(n = {}, K <= 255, H, W) with 2 <= H * W <= 2^24 and n * H * W < 2^31'


def _none_fits(ports, screen, batch):
    return 'components: no FP32 Result of shape {} with channel {} among its planes (the Results: {})'.format(
        SHAPE.format(batch), screen.channel, {name: tuple(port['dims']) for name, port in ports.items()})


def checked(ienet, components, sharded: bool) -> dict:
    """{Result name: resolved ComponentScreen, its channel counted from the front} of the `components` argument of infer() /
    start_async() -- a ComponentScreen, a min_score or True for every FP32 Result declared (n, K, H, W) with n the batch, 1 <= K <= 255,
    2 <= H * W <= 2^24, n * H * W < 2^31, not of the detector shape (1, 1, R, 7) and with the screen's channel among its planes, or
    {Result name: any of these} --, {} for None.  Everything is looked up in the network as it was read: no device is needed, nothing is
    allocated.  ValueError ('components: ...'): an unknown name, a value of another type, a field out of its range or of another type, no
    such Result for an unnamed form, a sharded batch, a Result of another rank, shape or precision, a channel outside its K."""
    if components is None:
        return {}
    batch = int(ienet.batch_size)
    ports, wanted = ask.named(ienet, 'components', components, sharded, _fits, _none_fits, resolved)
    for name in wanted:
        dims = ask.declared('components', name, ports[name], planes_of(ports[name]['dims'], batch), SHAPE, batch)
        wanted[name] = for_planes(wanted[name], dims[1], 'components: Result {!r}'.format(name))
    return wanted


class Blocks(ask.FlatBlocks):
    """What a request keeps for one (Result name, channel, connectivity, max_per_image = R): the device block pvhip_components_f32
    writes -- (n, R) int64 sums and (n, R, 5) int64 moments first, for their alignment, then (n, R, 4) int32 rectangles, (n, R) seeds,
    areas, peaks and zero signs, (n,) counts and found -- with the page-locked host block it is read back into in one copy of
    8 n + 80 n R bytes, and `scratch`, the three int32 per pixel of the union-find, which stay on the device.  None depends on min_score
    or min_area, which are arguments of the launch."""
    __slots__ = ('shape', 'channel', 'connectivity', 'R', 'scratch')

    def __init__(self, n: int, K: int, H: int, W: int, channel: int, connectivity: int, R: int):
        super().__init__(20 * n * R + 2 * n)
        self.shape, self.channel, self.connectivity, self.R = (n, K, H, W), channel, connectivity, R
        size = int(device.call('pvhip_components_scratch_bytes', n, H, W, R))
        assert size > 0, (n, H, W, R)
        self.scratch = device.DeviceTensor.empty((size // 4,), np.int32)

    def launch(self, result, min_score, min_area):
        """One call (five launches) on the current stream, behind whatever wrote `result` there."""
        n, K, H, W = planes_of(result.shape)
        assert (n, K, H, W) == self.shape and result.dtype == np.float32
        at = lambda words: ctypes.c_void_p(self.dev.ptr + 4 * words * n * self.R)
        tail = self.dev.ptr + 80 * n * self.R
        device.call('pvhip_components_f32', device.ptr(result), n, K, H, W, self.channel, self.connectivity, float(min_score), min_area, self.R,
                    ctypes.c_void_p(self.scratch.ptr), ctypes.c_void_p(tail), ctypes.c_void_p(tail + 4 * n), at(16), at(17), at(18), at(19),
                    at(12), at(0), at(2))

    def read_back(self) -> Components:
        """The answer, copied on the current stream, which has drained: the flat rows are formed here from the (n, R) block."""
        host, (n, _, _, _), R = self.words(), self.shape, self.R
        part = lambda first, words=1: host[first * n * R:(first + words) * n * R]
        counts, found = host[20 * n * R:20 * n * R + n].copy(), host[20 * n * R + n:].copy()
        image, rank = np.nonzero(np.arange(R)[None, :] < counts[:, None])
        rects = part(12, 4).reshape(n, R, 4)[image, rank].astype(np.int64)
        peaks = part(18).view(np.uint32).reshape(n, R)[image, rank]
        zeros = part(19).reshape(n, R)[image, rank]
        peaks = np.where(zeros != NO_ZERO, (zeros.astype(np.uint32) & np.uint32(1)) << np.uint32(31), peaks).astype(np.uint32)
        rois = np.stack([image, rects[:, 0], rects[:, 1], rects[:, 2] - rects[:, 0] + 1, rects[:, 3] - rects[:, 1] + 1], axis=1).astype(np.int32)
        return Components(counts, found, rois.reshape(-1, 5), part(17).reshape(n, R)[image, rank], part(16).reshape(n, R)[image, rank],
                          peaks.view(np.float32), part(0, 2).view(np.int64).reshape(n, R)[image, rank],
                          part(2, 10).view(np.int64).reshape(n, R, 5)[image, rank])


class Ask(ask.Ask, collections.namedtuple('Ask', 'screen')):
    """A Result asked for with components=, in its resolved form."""
    __slots__ = ()
    KEYWORD = 'components'

    def key(self, name):
        """(name, channel, connectivity, max_per_image).  min_score and min_area are no part of it: they go with the launch."""
        return (name, self.screen.channel, self.screen.connectivity, self.screen.max_per_image)

    def blocks_for(self, value):
        return Blocks(*planes_of(value.shape), self.screen.channel, self.screen.connectivity, self.screen.max_per_image)

    def launch_with(self):
        return (self.screen.min_score, self.screen.min_area)

    def on_host(self, value):
        return find(value, self.screen)
