"""The peak of every plane of a heatmap network's Result (``infer(..., keypoints=...)``): the rule, the argument checks and the device
launch.  Landmark heads, single-person pose on a detector's crops, CPM stages, corner heads: a Result (n, K, H, W), one heatmap per batch
row and keypoint.

The rule (include/pvhip.h, pvhip_heatmap_peaks_f32; tests/keypoints_ref.py is the same again in plain loops), for the plane v[0..H)[0..W)
of batch row r and channel c:
  1. peak    p is the first position of the plane's H * W values in top_k's total order: NaN of any sign or payload first, then
     descending with +0.0 == -0.0, ties to the lower flat index.  py = p // W, px = p % W.  positions[r][c] = p; scores[r][c] holds the
     plane's own bits at the peak.
  2. valid   the keypoint is valid iff its score is not NaN and (min_score is None or score >= float32(min_score)).  The quiet-NaN rows
     behind `count` of a DetectedRois or LandmarkWarps pass are void all through: their counts are 0.
  3. refine  'NONE': ox = oy = 0.  'QUARTER': if 1 <= px <= W - 2, with l = v[py][px - 1] and r = v[py][px + 1], ox = +0.25 if r > l,
     -0.25 if r < l, else 0 (equal values, zeros of either sign, either neighbour NaN); on the plane's first or last column ox = 0.  oy
     likewise in y with H.  H == 1 or W == 1 never refines that axis.  fx = float32(px) + ox, fy = float32(py) + oy, fp32 (exact below 2^22).
  4. space   'HEATMAP': (fx, fy).  'NORMALISED', on the pixel-edge convention LandmarkWarps reads (0 the left or top edge, 1 the right or
     bottom edge): x = float32(float64(fx + float32(0.5)) / float64(W)), y likewise with fy and H: one fp32 addition, one correctly
     rounded binary64 division, one rounding to fp32.  points[r][c] = (x, y); a void keypoint's are two quiet NaNs 0x7FC00000.
counts[r] is the number of valid keypoints of row r, formed on the host.  A valid 'NORMALISED' `points` of a Result with K points per row,
reshaped (n, 2 K), is what ``landmarks.to_warps`` takes."""
import collections
import ctypes

import numpy as np

from . import ask, device
from .ask import QUIET_NAN

REFINES = {'NONE': 0, 'QUARTER': 1}             # PVHIP_PEAKS_NONE, PVHIP_PEAKS_QUARTER
SPACES = {'HEATMAP': 0, 'NORMALISED': 1}        # PVHIP_PEAKS_HEATMAP, PVHIP_PEAKS_NORMALISED
MAX_PLANE = 1 << 24                             # PVHIP_PEAKS_MAX_PLANE: H * W at most (a flat index is exact in fp32)

PeakScreen = collections.namedtuple('PeakScreen', 'min_score refine space', defaults=(None, 'QUARTER', 'NORMALISED'))
PeakScreen.__doc__ = ('How to read a heatmap Result: a keypoint is valid when its peak is at least `min_score` (None: any peak that is not NaN); '
                      '`refine` \'QUARTER\' moves the peak a quarter pixel toward its larger neighbour on each axis, \'NONE\' leaves it; `space` '
                      '\'NORMALISED\' gives points in [0, 1] of the plane on pixel-edge coordinates, \'HEATMAP\' in heatmap pixels, centres at the integers.')

Keypoints = collections.namedtuple('Keypoints', 'counts points scores positions')
Keypoints.__doc__ = ('What a Result started with keypoints= comes back as: `counts` (n,) int32 valid keypoints per row, `points` (n, K, 2) float32 '
                     '(x, y), NaN where void, `scores` (n, K) float32 the peaks\' own bits, `positions` (n, K) int32 flat indices py * W + px.')


def resolved(value, what='keypoints') -> PeakScreen:
    """`value` -- a PeakScreen, a real number (its min_score) or True (the default screen) -- as a checked PeakScreen; ValueError."""
    if value is True:
        value = PeakScreen()
    elif not isinstance(value, (bool, PeakScreen)) and isinstance(value, (int, float, np.integer, np.floating)):
        value = PeakScreen(value)
    if not isinstance(value, PeakScreen):
        raise ValueError('{}: a PeakScreen, a min_score or True, got {!r}'.format(what, value))
    min_score, refine, space = value
    if not isinstance(refine, str) or refine not in REFINES:
        raise ValueError('{}: refine {!r} is not one of {}'.format(what, refine, sorted(REFINES)))
    if not isinstance(space, str) or space not in SPACES:
        raise ValueError('{}: space {!r} is not one of {}'.format(what, space, sorted(SPACES)))
    return PeakScreen(None if min_score is None else ask.checked_min_score(min_score, what), refine, space)


def planes_of(dims, batch=None):
    """(n, K, H, W) of a tensor declared as a stack of heatmaps -- 4-D, n the batch (when given), K >= 1, 2 <= H * W <= 2^24 --, else None."""
    dims = tuple(int(d) for d in dims)
    if len(dims) != 4 or min(dims) < 1 or not 2 <= dims[2] * dims[3] <= MAX_PLANE or (batch is not None and dims[0] != int(batch)):
        return None
    return dims


def _quarter(before, after):
    return np.where(after > before, np.float32(0.25), np.where(after < before, np.float32(-0.25), np.float32(0))).astype(np.float32)


def peaks(x, screen=True) -> Keypoints:
    """The rule in numpy on a host array of shape (n, K, H, W): what a Result computed on the host (a foreign plugin set) gets."""
    min_score, refine, space = resolved(screen, 'peaks')
    x = np.asarray(x)
    if x.dtype != np.float32 or planes_of(x.shape) is None:
        raise ValueError('peaks takes float32 heatmaps of shape (n, K, H, W) with 2 <= H * W <= 2^24, got {} {}'.format(x.dtype, x.shape))
    n, K, H, W = x.shape
    v = np.ascontiguousarray(x).reshape(n * K, H * W)
    nan = np.isnan(v)
    with np.errstate(invalid='ignore'):
        # the first NaN where there is one, else the first of the largest values (argmax takes +0.0 == -0.0 and the lower index)
        p = np.where(nan.any(axis=1), nan.argmax(axis=1), np.where(nan, -np.inf, v).argmax(axis=1)).astype(np.int64)
        at = np.arange(n * K)
        score = v[at, p]
        valid = ~np.isnan(score)
        if min_score is not None:
            valid &= score >= np.float32(min_score)
        py, px = p // W, p % W
        ox = oy = np.zeros(n * K, np.float32)
        if refine == 'QUARTER':
            inner = (px >= 1) & (px <= W - 2)
            ox = np.where(inner, _quarter(v[at, np.maximum(p - 1, 0)], v[at, np.minimum(p + 1, H * W - 1)]), np.float32(0))
            inner = (py >= 1) & (py <= H - 2)
            oy = np.where(inner, _quarter(v[at, np.maximum(p - W, 0)], v[at, np.minimum(p + W, H * W - 1)]), np.float32(0))
        fx, fy = px.astype(np.float32) + ox.astype(np.float32), py.astype(np.float32) + oy.astype(np.float32)
        if space == 'NORMALISED':
            fx = ((fx + np.float32(0.5)).astype(np.float64) / np.float64(W)).astype(np.float32)
            fy = ((fy + np.float32(0.5)).astype(np.float64) / np.float64(H)).astype(np.float32)
    points = np.stack([np.where(valid, fx, QUIET_NAN), np.where(valid, fy, QUIET_NAN)], axis=1).astype(np.float32).reshape(n, K, 2)
    valid = valid.reshape(n, K)
    return Keypoints(valid.sum(axis=1).astype(np.int32), points, score.reshape(n, K).copy(), p.astype(np.int32).reshape(n, K))


def to_frame(points, regions):
    """'NORMALISED' `points` (n, K, 2) float32 through the integer (n, 5) table (id, x, y, w, h) of the regions the rows were cropped
    from: (n, K, 2) float64 in frame pixels, centres at the integers -- (float(x) + float(u) float(w)) - 0.5 in binary64, the position
    ``landmarks.to_warps`` forms from the same point --; void points stay NaN.  The `points` (n, R, 2) of a ``Maxima`` go through unchanged:
    K is whatever the second extent is, and the filler slots behind a row's count stay NaN."""
    p = np.asarray(points)
    t = np.asarray(regions)
    if p.dtype != np.float32 or p.ndim != 3 or p.shape[2] != 2:
        raise ValueError('to_frame: points are float32 of shape (n, K, 2), got {} {}'.format(p.dtype, p.shape))
    if t.shape != (p.shape[0], 5) or t.dtype.kind not in 'iu':
        raise ValueError('to_frame: regions is an integer table of shape {} -- one (id, x, y, w, h) per row --, got {} {}'.format(
            (p.shape[0], 5), t.dtype, t.shape))
    t = t.astype(np.float64)
    u = p.astype(np.float64)
    return np.stack([(t[:, None, 1] + u[:, :, 0] * t[:, None, 3]) - 0.5, (t[:, None, 2] + u[:, :, 1] * t[:, None, 4]) - 0.5], axis=2)


def _fits(port, screen, batch):
    dims = planes_of(port['dims'], batch)
    return dims is not None and port['precision'] == 'FP32' and not (dims[:2] == (1, 1) and dims[3] == 7)


def _none_fits(ports, screen, batch):
    return 'keypoints: no FP32 Result of shape (n = {}, K, H, W) with 2 <= H * W <= 2^24 (the Results: {})'.format(
        batch, {name: tuple(port['dims']) for name, port in ports.items()})


def checked(ienet, keypoints, sharded: bool) -> dict:
    """{Result name: resolved PeakScreen} of the `keypoints` argument of infer() / start_async() -- a PeakScreen, a min_score or True for
    every FP32 Result declared (n, K, H, W) with n the batch, 2 <= H * W <= 2^24 and not of the detector shape (1, 1, R, 7), or {Result
    name: any of these} --, {} for None.  Everything is looked up in the network as it was read: no device is needed, nothing is allocated.
    ValueError ('keypoints: ...'): an unknown name, a value of another type, refine or space unknown, min_score not a finite real of
    float32, no such Result for an unnamed form, a sharded batch, a Result of another rank, shape or precision."""
    if keypoints is None:
        return {}
    batch = int(ienet.batch_size)
    ports, wanted = ask.named(ienet, 'keypoints', keypoints, sharded, _fits, _none_fits, resolved)
    for name in wanted:
        ask.declared('keypoints', name, ports[name], planes_of(ports[name]['dims'], batch), '(n = {}, K, H, W) with 2 <= H * W <= 2^24', batch)
    return wanted


class Blocks(ask.FlatBlocks):
    """What a request keeps for one (Result name, refine, space): the device block pvhip_heatmap_peaks_f32 writes -- (n, K) int32
    positions, (n, K) float32 scores, (n, K, 2) float32 points -- and the page-locked host block it is read back into in one copy of
    16 n K bytes.  Neither depends on min_score, which is an argument of the launch: a caller that varies the threshold from call to call
    keeps one pair of blocks."""
    __slots__ = ('n', 'K', 'refine', 'space')

    def __init__(self, n: int, K: int, refine: str, space: str):
        super().__init__(4 * n * K)
        self.n, self.K, self.refine, self.space = n, K, refine, space

    def launch(self, result, min_score):
        """One launch on the current stream, behind whatever wrote `result` there."""
        n, K, H, W = planes_of(result.shape)
        assert (n, K) == (self.n, self.K) and result.dtype == np.float32
        at = self.dev.ptr
        device.call('pvhip_heatmap_peaks_f32', device.ptr(result), n, K, H, W, REFINES[self.refine], SPACES[self.space],
                    int(min_score is not None), float(min_score or 0.0), ctypes.c_void_p(at), ctypes.c_void_p(at + 4 * n * K),
                    ctypes.c_void_p(at + 8 * n * K))

    def read_back(self) -> Keypoints:
        """The answer, copied on the current stream, which has drained; the arrays are the caller's own.  A valid point is finite and a
        void one NaN: the counts are formed here."""
        host, n, K = self.words(), self.n, self.K
        points = host[2 * n * K:].view(np.float32).reshape(n, K, 2).copy()
        return Keypoints((~np.isnan(points[:, :, 0])).sum(axis=1).astype(np.int32), points,
                         host[n * K:2 * n * K].view(np.float32).reshape(n, K).copy(), host[:n * K].reshape(n, K).copy())


class Ask(ask.Ask, collections.namedtuple('Ask', 'screen')):
    """A Result asked for with keypoints=, in its resolved form."""
    __slots__ = ()
    KEYWORD = 'keypoints'

    def key(self, name):
        """(name, refine, space).  min_score is no part of it: it goes with the launch."""
        return (name, self.screen.refine, self.screen.space)

    def blocks_for(self, value):
        n, K = planes_of(value.shape)[:2]
        return Blocks(n, K, self.screen.refine, self.screen.space)

    def launch_with(self):
        return (self.screen.min_score,)

    def on_host(self, value):
        return peaks(value, self.screen)
