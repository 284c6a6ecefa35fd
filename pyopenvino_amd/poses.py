"""Multi-person poses from a heatmap Result and a part-affinity-field Result (``infer(..., maxima=..., poses=...)``): the rule, the
argument checks and the device launch.  Heads of the OpenPose family (OpenPose / CPM stages, lightweight-OpenPose,
`human-pose-estimation-0001`-like): one Result (n, K, H, W) of joint heatmaps, asked for with ``maxima=``, and one Result (n, 2L, H, W)
of part-affinity fields (PAFs), two planes per limb, asked for with ``poses=``.  ``maxima=`` answers the candidate joints of every
plane; this groups them into persons.

The rule (include/pvhip.h, pvhip_pose_groups_f32; tests/poses_ref.py is the same again in plain loops), for batch row r.  Every operation
is fp32 rounded once, no product is fused into a sum, division and square root are the correctly rounded ones:
  1. candidates  the candidates of joint k are the maxima of plane k that ``maxima``'s rules 1 to 3 keep (its min_score and
     max_per_plane), in that order: candidate index i = 0 ..; (px, py) is the position.  max_per_plane <= 32, so a limb has at most
     1024 pairs.
  2. scoring     limb l has joints (a, b) and PAF channels (cx, cy).  For candidate i of a and j of b: dx = bx - ax, dy = by - ay as
     ints; dx == dy == 0 is no connection.  len = sqrt(float32(dx dx + dy dy)), ux = float32(dx) / len, uy = float32(dy) / len.
     Sample s = 0 .. S - 1 stands at the pixel x = ax + floor((2 s dx + (S - 1)) / (2 (S - 1))), y alike: the nearest pixel, no
     interpolation.  v_s = paf[cx][y][x] * ux + paf[cy][y][x] * uy.  A sample passes iff v_s > float32(min_field); a NaN does not.  c is
     the number passing, sum adds the passing v_s in order of s from +0.  The connection is valid iff c >= min_samples; its score is
     sum / float32(c).
  3. matching    a limb's valid connections are ranked by descending score bits (the scores are positive: min_field >= 0), ties to the
     lower i and then the lower j.  A connection is taken iff neither its i nor its j was taken before it.
  4. assembling  limbs in skeleton order, a limb's taken connections in rank order.  For (i, j, score): the first person (lowest index)
     whose slot a holds i.  If found and its slot b is empty, slot b becomes j and total = (total + heat_b_j) + score; if its slot b is
     occupied nothing happens.  If not found, the limb's `founds` flag is true and fewer than max_persons persons exist, a new person
     is made with total = (heat_a_i + heat_b_j) + score.  A person is kept iff it has at least min_joints joints and
     total / float32(joints) >= float32(min_mean).  Kept persons stay in creation order.  A row of NaN heat has no candidates: count 0
     -- the rows behind `count` of a DetectedRois pass.
  5. skeleton    'OPENPOSE18' (K >= 18 and 2L == 38: OPENPOSE18 below) or an (L, 5) int table (a, b, cx, cy, founds), 1 <= L <= 64,
     a != b.
Row r's first counts[r] persons are its answer; the slots of a joint a person lacks and every slot behind counts[r] are
(-1, quiet NaN, two quiet NaNs), the totals behind counts[r] quiet NaNs.  `points` reshaped (n, P * K, 2) are what
``keypoints.to_frame`` takes unchanged."""
import collections
import ctypes

import numpy as np

from . import ask, device, keypoints, maxima
from .ask import QUIET_NAN
from .keypoints import REFINES, SPACES

MAX_CANDIDATES = 32                             # PVHIP_POSES_MAX_CANDIDATES: the heat ask's max_per_plane at most
MAX_LIMBS = 64                                  # PVHIP_POSES_MAX_LIMBS
MAX_PERSONS = 64                                # PVHIP_POSES_MAX_PERSONS
MAX_JOINTS = 256                                # PVHIP_POSES_MAX_JOINTS: the heat Result's K at most
MAX_SAMPLES = 16                                # PVHIP_POSES_MAX_SAMPLES

# lightweight-OpenPose's 19 limbs over OpenPose's 18 joints: the joints (a, b), the PAF channels (cx, cy); the first 17 may found a person
_PAIRS = ((1, 2), (1, 5), (2, 3), (3, 4), (5, 6), (6, 7), (1, 8), (8, 9), (9, 10), (1, 11), (11, 12), (12, 13), (1, 0), (0, 14), (14, 16),
          (0, 15), (15, 17), (2, 16), (5, 17))
_CHANNELS = ((12, 13), (20, 21), (14, 15), (16, 17), (22, 23), (24, 25), (0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (10, 11), (28, 29), (30, 31),
             (34, 35), (32, 33), (36, 37), (18, 19), (26, 27))
OPENPOSE18 = tuple((a, b, cx, cy, int(l < 17)) for l, ((a, b), (cx, cy)) in enumerate(zip(_PAIRS, _CHANNELS)))

PoseScreen = collections.namedtuple('PoseScreen', 'heat skeleton samples min_field min_samples max_persons min_joints min_mean',
                                    defaults=(None, 'OPENPOSE18', 10, 0.05, 8, 32, 3, 0.2))
PoseScreen.__doc__ = ('How to group the candidates of the heatmap Result `heat` (asked for with maxima= in the same start; None: the single one) by '
                      'this Result\'s part-affinity fields: `skeleton` \'OPENPOSE18\' or an (L, 5) int table (a, b, cx, cy, founds); a pair is '
                      'scored on `samples` (2 .. 16) pixels between its ends, of which at least `min_samples` exceed `min_field` (>= 0); at most '
                      '`max_persons` (1 .. 64) persons per row, kept with at least `min_joints` joints and a mean score of at least `min_mean`.')

Poses = collections.namedtuple('Poses', 'counts joints scores points totals')
Poses.__doc__ = ('What a Result started with poses= comes back as: `counts` (n,) int32 persons per row, `joints` (n, P, K) int32 flat positions '
                 'py * W + px of the heatmap, -1 where a person lacks the joint, `scores` (n, P, K) float32 the heatmap\'s own bits there, `points` '
                 '(n, P, K, 2) float32 (x, y) by the heat ask\'s refine and space, `totals` (n, P) float32; NaN where absent and behind the count.')


def _int_in(value, least, most, what, field):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not least <= int(value) <= most:
        raise ValueError('{}: {} is an int in {} .. {}, got {!r}'.format(what, field, least, most, value))
    return int(value)


def _real(value, what, field, least=None):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)) or not np.isfinite(value) \
            or abs(float(value)) > float(np.finfo(np.float32).max) or (least is not None and float(value) < least):
        raise ValueError('{}: {} is a finite real (of float32){}, got {!r}'.format(what, field, '' if least is None else ' >= {}'.format(least), value))
    return float(np.float32(value))


def resolved(value, what='poses') -> PoseScreen:
    """`value` -- a PoseScreen or True -- checked, a table skeleton as a tuple of (a, b, cx, cy, founds); ValueError."""
    if value is True:
        value = PoseScreen()
    if not isinstance(value, PoseScreen):
        raise ValueError('{}: a PoseScreen or True, got {!r}'.format(what, value))
    heat, skeleton, samples, min_field, min_samples, persons, min_joints, min_mean = value
    if heat is not None and not isinstance(heat, str):
        raise ValueError('{}: heat is None or the name of a Result asked for with maxima=, got {!r}'.format(what, heat))
    if not (isinstance(skeleton, str) and skeleton == 'OPENPOSE18'):
        try:
            table = np.asarray(skeleton)
            fits = table.ndim == 2 and table.shape[1] == 5 and 1 <= table.shape[0] <= MAX_LIMBS and table.dtype.kind in 'iu'
        except (TypeError, ValueError):
            fits = False
        if isinstance(skeleton, str) or not fits:
            raise ValueError('{}: skeleton is \'OPENPOSE18\' or an (L, 5) int table (a, b, cx, cy, founds) with 1 <= L <= {}, got {!r}'.format(
                what, MAX_LIMBS, skeleton))
        skeleton = tuple(tuple(int(v) for v in row) for row in table)
    samples = _int_in(samples, 2, MAX_SAMPLES, what, 'samples')
    return PoseScreen(heat, skeleton, samples, _real(min_field, what, 'min_field', 0.0), _int_in(min_samples, 1, samples, what, 'min_samples'),
                      _int_in(persons, 1, MAX_PERSONS, what, 'max_persons'), _int_in(min_joints, 1, MAX_JOINTS, what, 'min_joints'),
                      _real(min_mean, what, 'min_mean'))


def skeleton_for(screen: PoseScreen, K: int, channels: int, what='poses') -> np.ndarray:
    """The (L, 5) int32 table of a resolved screen over K joints and `channels` PAF planes; ValueError for a skeleton they do not admit."""
    if screen.min_joints > K:
        raise ValueError('{}: min_joints = {} of K = {} joints'.format(what, screen.min_joints, K))
    if screen.skeleton == 'OPENPOSE18':
        if K < 18 or channels != 38:
            raise ValueError('{}: skeleton \'OPENPOSE18\' takes K >= 18 joints and 38 field planes, got K = {} and {}'.format(what, K, channels))
        return np.array(OPENPOSE18, np.int32)
    table = np.array(screen.skeleton, np.int64)
    for l, (a, b, cx, cy, founds) in enumerate(table.tolist()):
        if not (0 <= a < K and 0 <= b < K and a != b):
            raise ValueError('{}: skeleton limb {}: joints ({}, {}) are not two different joints in 0 .. {}'.format(what, l, a, b, K - 1))
        if not (0 <= cx < channels and 0 <= cy < channels):
            raise ValueError('{}: skeleton limb {}: channels ({}, {}) are not in 0 .. {}'.format(what, l, cx, cy, channels - 1))
        if founds not in (0, 1):
            raise ValueError('{}: skeleton limb {}: founds is 0 or 1, got {}'.format(what, l, founds))
    return table.astype(np.int32)


def fields_of(dims, batch=None):
    """(n, C, H, W) of a tensor declared as part-affinity fields -- keypoints' family with 1 <= C <= 128 and below 2^31 elements --, else None."""
    dims = keypoints.planes_of(dims, batch)
    return dims if dims is not None and dims[1] <= 2 * MAX_LIMBS and int(np.prod(dims, dtype=np.int64)) < 1 << 31 else None


def _connections(fx, fy, pa, pb, W, S, min_field, min_samples):
    """Rules 2 and 3 for one limb: the taken (i, j, score) in rank order; pa, pb: the candidates' positions."""
    ax, ay, bx, by = pa % W, pa // W, pb % W, pb // W
    dx, dy = bx[None, :] - ax[:, None], by[None, :] - ay[:, None]
    with np.errstate(invalid='ignore', divide='ignore'):
        length = np.sqrt((dx * dx + dy * dy).astype(np.float32))
        ux, uy = dx.astype(np.float32) / length, dy.astype(np.float32) / length
        c, total = np.zeros(dx.shape, np.int64), np.zeros(dx.shape, np.float32)
        for s in range(S):
            x, y = ax[:, None] + (2 * s * dx + (S - 1)) // (2 * (S - 1)), ay[:, None] + (2 * s * dy + (S - 1)) // (2 * (S - 1))
            v = fx[y, x] * ux + fy[y, x] * uy
            ok = v > np.float32(min_field)
            c += ok
            total = np.where(ok, total + v, total)
        i, j = np.nonzero(c >= min_samples)
        score = (total[i, j] / c[i, j].astype(np.float32)).astype(np.float32)
    key = (score.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - (i * MAX_CANDIDATES + j).astype(np.uint64))
    taken, used_a, used_b = [], set(), set()
    for at in np.argsort(~key, kind='stable').tolist():
        if i[at] not in used_a and j[at] not in used_b:
            used_a.add(i[at])
            used_b.add(j[at])
            taken.append((int(i[at]), int(j[at]), score[at]))
    return taken


def group(heat, pafs, maxima_screen=True, screen=True) -> Poses:
    """The rule in numpy on host arrays (n, K, H, W) and (n, 2L, H, W): what Results computed on the host (a foreign plugin set) get."""
    heat_screen, screen = maxima.resolved(maxima_screen, 'group'), resolved(screen, 'group')
    heat, pafs = np.ascontiguousarray(heat), np.ascontiguousarray(pafs)
    if heat.dtype != np.float32 or pafs.dtype != np.float32 or maxima.planes_of(heat.shape) is None or fields_of(pafs.shape) is None \
            or heat.shape[:1] + heat.shape[2:] != pafs.shape[:1] + pafs.shape[2:] or heat.shape[1] > MAX_JOINTS or heat.size >= 1 << 31:
        raise ValueError('group takes float32 heatmaps (n, K, H, W), K <= 256, and fields (n, 2L, H, W), 2L <= 128, of one n, H, W with '
                         '2 <= H * W <= 2^24, each below 2^31 elements, got {} {} and {} {}'.format(heat.dtype, heat.shape, pafs.dtype, pafs.shape))
    if heat_screen.max_per_plane > MAX_CANDIDATES:
        raise ValueError('group: the heatmaps\' max_per_plane = {} is above {}'.format(heat_screen.max_per_plane, MAX_CANDIDATES))
    n, K, H, W = heat.shape
    table = skeleton_for(screen, K, pafs.shape[1], 'group')
    M, P, S = heat_screen.max_per_plane, screen.max_persons, screen.samples
    cand = maxima.peaks_of(heat.reshape(n * K, 1, H, W), heat_screen._replace(max_per_row=M))       # rule 1: a plane a row
    out = Poses(np.zeros(n, np.int32), np.full((n, P, K), -1, np.int32), np.full((n, P, K), QUIET_NAN, np.float32),
                np.full((n, P, K, 2), QUIET_NAN, np.float32), np.full((n, P), QUIET_NAN, np.float32))
    for r in range(n):
        persons = []                                            # [slots (K,), total]
        counts, positions, values = cand.counts[r * K:(r + 1) * K], cand.positions[r * K:(r + 1) * K].astype(np.int64), cand.scores[r * K:(r + 1) * K]
        for a, b, cx, cy, founds in table.tolist():
            if not counts[a] or not counts[b]:
                continue
            for i, j, score in _connections(pafs[r, cx], pafs[r, cy], positions[a, :counts[a]], positions[b, :counts[b]], W, S,
                                            screen.min_field, screen.min_samples):
                found = [p for p in persons if p[0][a] == i]
                if found:
                    if found[0][0][b] < 0:
                        found[0][0][b] = j
                        found[0][1] = (found[0][1] + values[b, j]) + score
                elif founds and len(persons) < P:
                    slots = np.full(K, -1, np.int64)
                    slots[a], slots[b] = i, j
                    persons.append([slots, (values[a, i] + values[b, j]) + score])
        with np.errstate(invalid='ignore'):
            kept = [p for p in persons if (p[0] >= 0).sum() >= screen.min_joints
                    and p[1] / np.float32((p[0] >= 0).sum()) >= np.float32(screen.min_mean)]
        out.counts[r] = len(kept)
        for q, (slots, total) in enumerate(kept):
            k = np.flatnonzero(slots >= 0)
            out.joints[r, q, k] = cand.positions[r * K + k, slots[k]]
            out.scores[r, q, k] = cand.scores[r * K + k, slots[k]]
            out.points[r, q, k] = cand.points[r * K + k, slots[k]]
            out.totals[r, q] = total
    return out


SHAPE = '(n = {}, 2L, H, W) with 2L <= 128, 2 <= H * W <= 2^24 and below 2^31 elements'


def checked(ienet, poses, heats: dict, sharded: bool) -> dict:
    """{field Result name: (resolved PoseScreen with `heat` named, its skeleton as a tuple of rows)} of the `poses` argument of infer() /
    start_async() -- a PoseScreen or True for every FP32 Result that fields_of takes and maxima= does not name, or {Result name: either}
    -- given `heats` = {Result name: resolved MaximaScreen} of the same call's maxima=.  ValueError ('poses: ...'): no maxima= in the
    call, an unknown name, a sharded batch, a field out of range, a Result of another rank, shape or precision, a heat not asked for or
    of another n, H or W, of more than 256 joints or with max_per_plane > 32, several heats and no heat=, a skeleton that K and 2L do not
    admit."""
    if not heats:
        raise ValueError('poses: the candidates these group come from maxima= in the same call, which names no Result')
    batch = int(ienet.batch_size)
    if not isinstance(poses, dict):
        screen = resolved(poses)
        ports, _ = ask.named(ienet, 'poses', {}, sharded)
        poses = {name: screen for name, port in ports.items() if name not in heats and port['precision'] == 'FP32' and fields_of(port['dims'], batch)}
        if not poses:
            raise ValueError('poses: no FP32 Result of shape {} beside those under maxima= (the Results: {})'.format(
                SHAPE.format(batch), {name: tuple(port['dims']) for name, port in ports.items()}))
    ports, wanted = ask.named(ienet, 'poses', poses, sharded, resolved=resolved)
    out = {}
    for name, screen in wanted.items():
        n, channels, H, W = ask.declared('poses', name, ports[name], fields_of(ports[name]['dims'], batch), SHAPE, batch)
        if screen.heat is None and len(heats) != 1:
            raise ValueError('poses: Result {!r}: maxima= asks for {} Results ({}): heat= names the one'.format(name, len(heats), sorted(heats)))
        heat = screen.heat if screen.heat is not None else next(iter(heats))
        if heat not in heats:
            raise ValueError('poses: Result {!r}: heat {!r} is not asked for with maxima= (which asks for {})'.format(name, heat, sorted(heats)))
        if heat == name:
            raise ValueError('poses: Result {!r} is asked for with maxima as well'.format(name))
        dims = tuple(int(d) for d in ports[heat]['dims'])
        if (dims[0], dims[2], dims[3]) != (n, H, W):
            raise ValueError('poses: Result {!r} is {} and heat {!r} is {}: not one n, H and W'.format(name, (n, channels, H, W), heat, dims))
        if dims[1] > MAX_JOINTS or n * dims[1] * H * W >= 1 << 31:
            raise ValueError('poses: heat {!r} has K = {} joints, above {}, or 2^31 elements or more'.format(heat, dims[1], MAX_JOINTS))
        if heats[heat].max_per_plane > MAX_CANDIDATES:
            raise ValueError('poses: heat {!r} is asked for with max_per_plane = {}, above {}'.format(heat, heats[heat].max_per_plane, MAX_CANDIDATES))
        table = skeleton_for(screen, dims[1], channels, 'poses: Result {!r}'.format(name))
        out[name] = (screen._replace(heat=heat), tuple(tuple(row) for row in table.tolist()))
    return out


class Blocks(ask.FlatBlocks):
    """What a request keeps for one (field Result, heat Result, max_persons, L): the device block pvhip_pose_groups_f32 writes -- (n,) int32
    counts, (n, P, K) int32 joints, (n, P, K) float32 scores, (n, P, K, 2) float32 points, (n, P) float32 totals -- with the page-locked
    host block it is read back into in one copy of 4 n + 16 n P K + 4 n P bytes, and `scratch`, the limbs' taken connections between the
    entry's two launches, which stay on the device."""
    __slots__ = ('n', 'K', 'P', 'L', 'scratch')

    def __init__(self, n: int, K: int, P: int, L: int):
        super().__init__(n + 4 * n * P * K + n * P)
        self.n, self.K, self.P, self.L = n, K, P, L
        self.scratch = device.DeviceTensor.empty((n * L * (4 * MAX_CANDIDATES + 1),), np.int32)     # PVHIP_POSES_SCRATCH_BYTES

    def launch(self, pafs, heat, candidates, heat_screen, screen, table):
        """One call (two launches) on the current stream, behind the maxima call that has just written `candidates` there."""
        n, K, H, W = maxima.planes_of(heat.shape)
        assert (n, K, len(table)) == (self.n, self.K, self.L) and heat.dtype == np.float32 and pafs.dtype == np.float32
        assert (pafs.shape[0],) + tuple(pafs.shape[2:]) == (n, H, W) and tuple(candidates.shape) == (n, K, heat_screen.max_per_plane)
        table = np.ascontiguousarray(table, np.int32)
        at, slots = self.dev.ptr + 4 * n, 4 * n * self.P * K
        device.call('pvhip_pose_groups_f32', device.ptr(heat), ctypes.c_void_p(candidates.ptr), device.ptr(pafs), n, K, H, W, heat_screen.max_per_plane,
                    int(pafs.shape[1]), table.ctypes.data_as(ctypes.c_void_p), len(table), REFINES[heat_screen.refine], SPACES[heat_screen.space],
                    screen.samples, screen.min_field, screen.min_samples, self.P, screen.min_joints, screen.min_mean, ctypes.c_void_p(self.scratch.ptr),
                    ctypes.c_void_p(self.dev.ptr), ctypes.c_void_p(at), ctypes.c_void_p(at + slots), ctypes.c_void_p(at + 2 * slots),
                    ctypes.c_void_p(at + 4 * slots))

    def read_back(self) -> Poses:
        """The answer, copied on the current stream, which has drained; the arrays are the caller's own."""
        host, n, P, K = self.words(), self.n, self.P, self.K
        s = n * P * K
        return Poses(host[:n].copy(), host[n:n + s].reshape(n, P, K).copy(), host[n + s:n + 2 * s].view(np.float32).reshape(n, P, K).copy(),
                     host[n + 2 * s:n + 4 * s].view(np.float32).reshape(n, P, K, 2).copy(), host[n + 4 * s:].view(np.float32).reshape(n, P).copy())


class Ask(ask.Ask, collections.namedtuple('Ask', 'screen table')):
    """A field Result asked for with poses=: `screen` the resolved PoseScreen with its heat named, `table` the skeleton's rows."""
    __slots__ = ()
    KEYWORD = 'poses'

    @property
    def needs(self):
        return (self.screen.heat,)

    def key(self, name):
        """(name, heat, max_persons, L): what sizes the blocks; everything else goes with the launch."""
        return (name, self.screen.heat, self.screen.max_persons, len(self.table))

    def launch(self, blocks, value, *others):
        (heat_ask, heat_value, heat_blocks), = others
        blocks = blocks or Blocks(int(value.shape[0]), int(heat_value.shape[1]), self.screen.max_persons, len(self.table))
        blocks.launch(value, heat_value, heat_blocks.scratch, heat_ask.screen, self.screen, self.table)
        return blocks

    def on_host(self, value, *others):
        (heat_ask, heat_value, _), = others
        return group(np.asarray(heat_value), value, heat_ask.screen, self.screen._replace(skeleton=self.table))
