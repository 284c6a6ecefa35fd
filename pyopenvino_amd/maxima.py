"""The local maxima of every plane of a heatmap network's Result (``infer(..., maxima=...)``): the rule, the argument checks and the device
launch.  Heads with several objects per plane: CenterNet-style detectors ("objects as points", one plane per class), multi-person pose
stages (OpenPose / CPM: one plane per joint, many people per plane), CenterFace, crowd and cell localisation: a Result (n, K, H, W).
``keypoints=`` answers one peak per plane; this answers the plane's local maxima, the best of each plane and then the best of each row.

The rule (include/pvhip.h, pvhip_heatmap_maxima_f32; tests/maxima_ref.py is the same again in plain loops), for the plane
v[0..H)[0..W) of batch row r and channel c:
  1. maximum  key(q) is top_k's key of (v[q], flat index q): NaN of any sign or payload first, then descending with +0.0 == -0.0, ties
     to the lower index.  Position p is a maximum iff v[p] is not NaN and key(p) is larger than the key of each of its at most eight
     neighbours that lie inside the plane.  A plateau therefore yields only those of its pixels that have no plateau neighbour before
     them in raster order; a flat plane has one maximum, at index 0.  A NaN is never a maximum and suppresses all its neighbours: the
     quiet-NaN rows behind `count` of a DetectedRois or LandmarkWarps pass have count 0.  This differs from CenterNet's
     ``hmax == heat`` (a 3 x 3 max-pool, then equality) only on exact ties: there every pixel of a plateau passes, here one per
     connected run in raster order.
  2. screen   the maximum passes iff min_score is None or v[p] >= float32(min_score).  Equality keeps.
  3. per plane  the first max_per_plane passing maxima are kept, in descending key order.
  4. per row  the kept maxima of the row's K planes are ordered by descending value, ties to the lower channel, then to the lower
     position: the key of (value, c * H * W + p), which is why K * H * W <= 2^31 - 1.  The first max_per_row are the answer.
  5. refine / space  ``keypoints``' rules 3 and 4 word for word (keypoints.py), applied at each answered position: 'QUARTER' moves the
     point a quarter pixel toward the larger of the two neighbours on each axis (none on the plane's border, none between equal
     neighbours or beside a NaN), 'NORMALISED' is float32(float64(fx + float32(0.5)) / float64(W)) on the pixel-edge convention.
Row r's first counts[r] slots are its maxima, best first; the slots behind them are (-1, -1, quiet NaN, quiet NaN, quiet NaN), as
``Matches`` pads.  'NORMALISED' `points` (n, R, 2) are what ``keypoints.to_frame`` takes unchanged."""
import collections
import ctypes

import numpy as np

from . import ask, device, keypoints
from .ask import QUIET_NAN
from .keypoints import REFINES, SPACES

MAX_PLANE = 1 << 24                             # PVHIP_MAXIMA_MAX_PLANE: H * W at most
MAX_PER_PLANE = 256                             # PVHIP_MAXIMA_MAX_PER_PLANE
MAX_PER_ROW = 1024                              # PVHIP_MAXIMA_MAX_PER_ROW
MAX_INDEX = (1 << 31) - 1                       # K * H * W at most: rule 4's index c * H * W + p is top_k's

MaximaScreen = collections.namedtuple('MaximaScreen', 'min_score max_per_plane max_per_row refine space', defaults=(None, 32, None, 'QUARTER', 'NORMALISED'))
MaximaScreen.__doc__ = ('How to read a heatmap Result with several objects per plane: a local maximum passes when it is at least `min_score` (None: any '
                        'that is not NaN); the best `max_per_plane` (1 .. 256) of each plane and then the best `max_per_row` (1 .. 1024; None: '
                        'min(K * max_per_plane, 1024)) of each batch row are answered; `refine` and `space` as in PeakScreen.')

Maxima = collections.namedtuple('Maxima', 'counts channels positions scores points')
Maxima.__doc__ = ('What a Result started with maxima= comes back as: `counts` (n,) int32 maxima per row, `channels` (n, R) int32, `positions` (n, R) '
                  'int32 flat indices py * W + px, `scores` (n, R) float32 the planes\' own bits, `points` (n, R, 2) float32 (x, y); best first, and '
                  '(-1, -1, NaN, NaN, NaN) behind the count.')


def _checked_cap(value, most, what, field):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not 1 <= int(value) <= most:
        raise ValueError('{}: {} is an int in 1 .. {}, got {!r}'.format(what, field, most, value))
    return int(value)


def resolved(value, what='maxima') -> MaximaScreen:
    """`value` -- a MaximaScreen, a real number (its min_score) or True (the default screen) -- as a checked MaximaScreen (max_per_row
    may still be None: it depends on the Result's K); ValueError."""
    if value is True:
        value = MaximaScreen()
    elif not isinstance(value, (bool, MaximaScreen)) and isinstance(value, (int, float, np.integer, np.floating)):
        value = MaximaScreen(value)
    if not isinstance(value, MaximaScreen):
        raise ValueError('{}: a MaximaScreen, a min_score or True, got {!r}'.format(what, value))
    min_score, per_plane, per_row, refine, space = value
    if not isinstance(refine, str) or refine not in REFINES:
        raise ValueError('{}: refine {!r} is not one of {}'.format(what, refine, sorted(REFINES)))
    if not isinstance(space, str) or space not in SPACES:
        raise ValueError('{}: space {!r} is not one of {}'.format(what, space, sorted(SPACES)))
    return MaximaScreen(None if min_score is None else ask.checked_min_score(min_score, what), _checked_cap(per_plane, MAX_PER_PLANE, what, 'max_per_plane'),
                        None if per_row is None else _checked_cap(per_row, MAX_PER_ROW, what, 'max_per_row'), refine, space)


def planes_of(dims, batch=None):
    """(n, K, H, W) of a tensor declared as a stack of heatmaps -- keypoints' family: 4-D, n the batch (when given), K >= 1,
    2 <= H * W <= 2^24 -- with K * H * W <= 2^31 - 1, else None."""
    dims = keypoints.planes_of(dims, batch)
    return dims if dims is not None and dims[1] * dims[2] * dims[3] <= MAX_INDEX else None


def for_planes(screen: MaximaScreen, n: int, K: int, what='maxima') -> MaximaScreen:
    """`screen`, resolved, for a Result of n rows of K planes: max_per_row filled in; ValueError when n * K * max_per_plane >= 2^31."""
    if n * K * screen.max_per_plane >= 1 << 31:
        raise ValueError('{}: n * K * max_per_plane = {} * {} * {} is not below 2^31'.format(what, n, K, screen.max_per_plane))
    return screen if screen.max_per_row is not None else screen._replace(max_per_row=min(K * screen.max_per_plane, MAX_PER_ROW))


def order_words(x):
    """The high word of top_k's key of every float32 of `x`, as uint32: order-preserving bits, -0.0 on +0.0, every NaN all ones."""
    bits = np.ascontiguousarray(x, np.float32).view(np.uint32)
    mag = bits & np.uint32(0x7FFFFFFF)
    return np.where(mag > np.uint32(0x7F800000), np.uint32(0xFFFFFFFF), np.where(mag == 0, np.uint32(0x80000000),
                    np.where(bits >> np.uint32(31) != 0, ~bits, bits | np.uint32(0x80000000)))).astype(np.uint32)


def _first_of_each(group, key, most):
    """Of items in groups `group` with distinct uint64 `key`s: the indices of the `most` largest keys of each group, by group and
    descending key."""
    order = np.lexsort((~key, group))
    g = group[order]
    starts = np.flatnonzero(np.r_[True, g[1:] != g[:-1]]) if g.size else np.zeros(0, np.int64)
    rank = np.arange(g.size) - np.repeat(starts, np.diff(np.r_[starts, g.size]))
    return order[rank < most]


def peaks_of(x, screen=True) -> Maxima:
    """The rule in numpy on a host array of shape (n, K, H, W): what a Result computed on the host (a foreign plugin set) gets."""
    screen = resolved(screen, 'peaks_of')
    x = np.asarray(x)
    if x.dtype != np.float32 or planes_of(x.shape) is None:
        raise ValueError('peaks_of takes float32 heatmaps of shape (n, K, H, W) with 2 <= H * W <= 2^24 and K * H * W <= 2^31 - 1, got {} {}'.format(
            x.dtype, x.shape))
    n, K, H, W = x.shape
    min_score, M, R, refine, space = for_planes(screen, n, K, 'peaks_of')
    x = np.ascontiguousarray(x)
    words = order_words(x)
    ring = np.zeros((n, K, H + 2, W + 2), np.uint32)             # 0 outside the plane: below every order word
    ring[:, :, 1:-1, 1:-1] = words
    across = np.maximum(np.maximum(ring[:, :, :, :-2], ring[:, :, :, 1:-1]), ring[:, :, :, 2:])       # the maximum of three along x
    # keys are distinct: above the four neighbours before p in raster order, not below the four behind it; a NaN (all ones) is never taken
    found = (words != np.uint32(0xFFFFFFFF)) & (words > across[:, :, :-2]) & (words > ring[:, :, 1:-1, :-2]) \
        & (words >= ring[:, :, 1:-1, 2:]) & (words >= across[:, :, 2:])
    if min_score is not None:
        with np.errstate(invalid='ignore'):
            found &= x >= np.float32(min_score)
    at = np.flatnonzero(found.reshape(-1))
    plane, p = at // (H * W), at % (H * W)
    high = words.reshape(-1)[at].astype(np.uint64) << np.uint64(32)
    kept = _first_of_each(plane, high | (np.uint64(0x7FFFFFFF) - p.astype(np.uint64)), M)              # rule 3
    plane, p, high = plane[kept], p[kept], high[kept]
    row, c = plane // K, plane % K
    kept = _first_of_each(row, high | (np.uint64(0x7FFFFFFF) - (c * (H * W) + p).astype(np.uint64)), R)  # rule 4
    plane, p, row, c = plane[kept], p[kept], row[kept], c[kept]
    counts = np.bincount(row, minlength=n).astype(np.int32)
    slot = np.arange(row.size) - np.repeat(np.cumsum(counts) - counts, counts)
    v = x.reshape(n * K, H * W)
    py, px = p // W, p % W
    ox = oy = np.zeros(p.size, np.float32)
    with np.errstate(invalid='ignore'):
        if refine == 'QUARTER':                                 # keypoints' rule 3
            quarter = keypoints._quarter
            ox = np.where((px >= 1) & (px <= W - 2), quarter(v[plane, np.maximum(p - 1, 0)], v[plane, np.minimum(p + 1, H * W - 1)]), np.float32(0))
            oy = np.where((py >= 1) & (py <= H - 2), quarter(v[plane, np.maximum(p - W, 0)], v[plane, np.minimum(p + W, H * W - 1)]), np.float32(0))
        fx, fy = px.astype(np.float32) + ox.astype(np.float32), py.astype(np.float32) + oy.astype(np.float32)
        if space == 'NORMALISED':                               # keypoints' rule 4
            fx = ((fx + np.float32(0.5)).astype(np.float64) / np.float64(W)).astype(np.float32)
            fy = ((fy + np.float32(0.5)).astype(np.float64) / np.float64(H)).astype(np.float32)
    out = Maxima(counts, np.full((n, R), -1, np.int32), np.full((n, R), -1, np.int32), np.full((n, R), QUIET_NAN, np.float32),
                 np.full((n, R, 2), QUIET_NAN, np.float32))
    out.channels[row, slot] = c
    out.positions[row, slot] = p
    out.scores.view(np.uint32)[row, slot] = v.view(np.uint32)[plane, p]       # the plane's own bits
    out.points[row, slot, 0] = fx
    out.points[row, slot, 1] = fy
    return out


def _fits(port, screen, batch):
    dims = planes_of(port['dims'], batch)
    return dims is not None and port['precision'] == 'FP32' and not (dims[:2] == (1, 1) and dims[3] == 7)


SHAPE = '(n = {}, K, H, W) with 2 <= H * W <= 2^24 and K * H * W <= 2^31 - 1'


def _none_fits(ports, screen, batch):
    return 'maxima: no FP32 Result of shape {} (the Results: {})'.format(SHAPE.format(batch), {name: tuple(port['dims']) for name, port in ports.items()})


def checked(ienet, maxima, sharded: bool) -> dict:
    """{Result name: resolved MaximaScreen, max_per_row filled in} of the `maxima` argument of infer() / start_async() -- a MaximaScreen, a
    min_score or True for every FP32 Result declared (n, K, H, W) with n the batch, 2 <= H * W <= 2^24, K * H * W <= 2^31 - 1 and not of
    the detector shape (1, 1, R, 7), or {Result name: any of these} --, {} for None.  Everything is looked up in the network as it was
    read: no device is needed, nothing is allocated.  ValueError ('maxima: ...'): an unknown name, a value of another type, refine or
    space unknown, min_score not a finite real of float32, max_per_plane or max_per_row not an int in its range, no such Result for an
    unnamed form, a sharded batch, a Result of another rank, shape or precision, n * K * max_per_plane >= 2^31."""
    if maxima is None:
        return {}
    batch = int(ienet.batch_size)
    ports, wanted = ask.named(ienet, 'maxima', maxima, sharded, _fits, _none_fits, resolved)
    for name in wanted:
        n, K, _, _ = ask.declared('maxima', name, ports[name], planes_of(ports[name]['dims'], batch), SHAPE, batch)
        wanted[name] = for_planes(wanted[name], n, K, 'maxima: Result {!r}'.format(name))
    return wanted


class Blocks(ask.FlatBlocks):
    """What a request keeps for one (Result name, max_per_plane, max_per_row, refine, space): the device block
    pvhip_heatmap_maxima_f32 writes -- (n,) int32 counts, (n, R) int32 channels, (n, R) int32 positions, (n, R) float32 scores,
    (n, R, 2) float32 points -- with the page-locked host block it is read back into in one copy of 4 n + 20 n R bytes, and `scratch`,
    the (n, K, M) 8-byte keys between the entry's two launches, which stay on the device.  None depends on min_score, which is an
    argument of the launch."""
    __slots__ = ('n', 'K', 'M', 'R', 'refine', 'space', 'scratch')

    def __init__(self, n: int, K: int, M: int, R: int, refine: str, space: str):
        super().__init__(n + 5 * n * R)
        self.n, self.K, self.M, self.R, self.refine, self.space = n, K, M, R, refine, space
        self.scratch = device.DeviceTensor.empty((n, K, M), np.uint64)

    def launch(self, result, min_score):
        """One call (two launches) on the current stream, behind whatever wrote `result` there."""
        n, K, H, W = planes_of(result.shape)
        assert (n, K) == (self.n, self.K) and result.dtype == np.float32
        at, R = self.dev.ptr + 4 * n, 4 * n * self.R
        device.call('pvhip_heatmap_maxima_f32', device.ptr(result), n, K, H, W, self.M, self.R, REFINES[self.refine], SPACES[self.space],
                    int(min_score is not None), float(min_score or 0.0), ctypes.c_void_p(self.scratch.ptr), ctypes.c_void_p(self.dev.ptr),
                    ctypes.c_void_p(at), ctypes.c_void_p(at + R), ctypes.c_void_p(at + 2 * R), ctypes.c_void_p(at + 3 * R))

    def read_back(self) -> Maxima:
        """The answer, copied on the current stream, which has drained; the arrays are the caller's own."""
        host, n, R = self.words(), self.n, self.R
        part = lambda i, words=1: host[n + i * n * R:n + (i + words) * n * R]
        return Maxima(host[:n].copy(), part(0).reshape(n, R).copy(), part(1).reshape(n, R).copy(),
                      part(2).view(np.float32).reshape(n, R).copy(), part(3, 2).view(np.float32).reshape(n, R, 2).copy())


class Ask(ask.Ask, collections.namedtuple('Ask', 'screen')):
    """A Result asked for with maxima=, in its resolved form."""
    __slots__ = ()
    KEYWORD = 'maxima'

    def key(self, name):
        """(name, max_per_plane, max_per_row, refine, space).  min_score is no part of it: it goes with the launch."""
        return (name, self.screen.max_per_plane, self.screen.max_per_row, self.screen.refine, self.screen.space)

    def blocks_for(self, value):
        n, K = planes_of(value.shape)[:2]
        return Blocks(n, K, self.screen.max_per_plane, self.screen.max_per_row, self.screen.refine, self.screen.space)

    def launch_with(self):
        return (self.screen.min_score,)

    def on_host(self, value):
        return peaks_of(value, self.screen)
