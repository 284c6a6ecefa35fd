"""The k best enrolled embeddings for every row of an embedding network's Result (``infer(..., matches=Gallery(...))``): the rule, the
gallery and its packing, the argument checks and the device launches.

The rule (include/pvhip.h, pvhip_gallery_match_f32; tests/gallery_ref.py is the same again):
  1. norm    of a row v[0..D) of float32: s = the binary64 sum of double(v[d])^2 for d ascending, started from 0.0, one rounding per
     addition (the squares are exact in binary64); the row is void when an element is not finite or when s == 0; r = sqrt(s), correctly
     rounded binary64.
  2. gallery rows, on the host when the Gallery is made: under 'COSINE' u[g][d] = float32(double(v[d]) / r); under 'DOT' u = v, and a
     row is void only for an element that is not finite.  A void gallery row is a ValueError.
  3. chain   a[r][g] starts at +0.0f; for d = 0 .. D - 1 in order a = fmaf(x[r][d], u[g][d], a): fp32, one rounding per step,
     subnormals kept.  x is the Result's own bits, not normalised.  A chain may end at -0.0 (a negative underflow); a zero of either sign
     counts as +0.0 from here on, so zero padding behind D does not change the answer.
  4. order   per row the gallery rows are sorted by a in top_k's total order -- NaN first, then descending, +0 equal to -0, ties to the
     lower gallery index --; the first k are the candidates.  A chain of finite factors may overflow to an infinity and then stays
     there: it never holds NaN.
  5. score   under 'DOT' score = a; under 'COSINE' score = float32(double(a) / r_row), r_row from 1. on the query row.  A NaN score is
     the quiet NaN 0x7FC00000.  Slot j is kept when min_score is None or score >= min_score (a NaN is not); counts[r] is the length of
     the leading run of kept slots; the slots behind it are void: (-1, -1, the quiet NaN 0x7FC00000).
  6. a void query row -- an element that is not finite under either metric, or s == 0 under 'COSINE' -- has count 0 and every slot void
     (the quiet-NaN rows behind `count` of a DetectedRois or LandmarkWarps pass are such rows).

fmaf in numpy (Python 3.10 has no math.fma) by rounding to odd: the product of two float32 is exact in float64 (48 bits); it is added to c
in float64, TwoSum gives the exact residual, and a sum that is inexact and even in its last mantissa bit moves one ulp toward the
residual; 53 >= 2 * 24 + 2 bits, so the final .astype(float32) rounds once (tests/test_gallery.py holds it against glibc's fmaf)."""
import collections
import ctypes

import numpy as np

from . import ask, device
from .ask import QUIET_NAN
from .top_k import MAX_K, rows_of

CHUNK = 256             # PVHIP_GALLERY_CHUNK of include/pvhip.h: gallery rows per list of k keys (tests place G on both sides of it)
MAX_D = 1024
MAX_G = 1 << 24
METRICS = {'COSINE': 0, 'DOT': 1}       # PVHIP_GALLERY_COSINE, PVHIP_GALLERY_DOT

GalleryMatch = collections.namedtuple('GalleryMatch', 'gallery k min_score', defaults=(1, None))
GalleryMatch.__doc__ = ('How to match a Result against a Gallery: the `k` best gallery rows of every batch row (1 .. min(G, 64)), and of '
                        'those the leading ones whose score is at least `min_score` (None: all k).')

Matches = collections.namedtuple('Matches', 'counts indices ids scores')
Matches.__doc__ = ('What a Result started with matches= comes back as: `counts` (n,) int32, `indices` (n, k) int32 gallery rows best first, '
                   '`ids` (n, k) int32 = gallery.ids[indices], `scores` (n, k) float32; slots at or after counts[r] are (-1, -1, NaN).')


def fmaf(a, b, c):
    """fmaf of float32 arrays, elementwise and broadcasting: a * b + c with one rounding."""
    a, b, c = (np.asarray(t, np.float32).astype(np.float64) for t in (a, b, c))
    with np.errstate(over='ignore', invalid='ignore'):
        p = a * b                                       # exact
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)                     # TwoSum: p + c = s + e exactly
        odd = (s.view(np.int64) & 1) != 0
        toward = np.where(e > 0, np.inf, -np.inf)
        s = np.where(np.isfinite(s) & (e != 0) & ~odd, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def norm(v, piece=4096):
    """(s, r, finite) of the rows of a float32 (n, D) array by rule 1: s and r float64 (n,), finite bool (n,).  `piece` rows at a time,
    transposed, so that a gallery of millions of rows is walked once and every addition is one vector operation over the piece."""
    v = np.asarray(v, np.float32)
    s = np.zeros(v.shape[0], np.float64)
    finite = np.empty(v.shape[0], bool)
    with np.errstate(over='ignore', invalid='ignore'):
        for at in range(0, v.shape[0], piece):
            w = np.ascontiguousarray(v[at:at + piece].T, np.float64)
            part = np.zeros(w.shape[1], np.float64)
            for d in range(w.shape[0]):
                part = part + w[d] * w[d]
            s[at:at + piece] = part
            finite[at:at + piece] = np.isfinite(w).all(axis=0)
        return s, np.sqrt(s), finite


def pack(u):
    """The rows u (G, D) float32 in the matrix cores' operand order, flat float32: G padded to a multiple of 32 and D to a multiple of 8
    with zeros; u[g][d] stands at ((g // 32 * (Dp // 8) + d // 8) * 64 + (((d & 1) << 5) | (g & 31))) * 4 + ((d & 7) >> 1)."""
    u = np.asarray(u, np.float32)
    G, D = u.shape
    Gp, Dp = -(-G // 32) * 32, -(-D // 8) * 8
    padded = np.zeros((Gp, Dp), np.float32)
    padded[:G, :D] = u
    blocks = padded.reshape(Gp // 32, 32, Dp // 8, 4, 2)          # [block][j][group][step][half]
    return np.ascontiguousarray(blocks.transpose(0, 2, 4, 1, 3)).reshape(-1)     # [block][group][half][j][step]


def unpack(packed, G: int, D: int):
    """The rows pack() packed, (G, D) float32."""
    Gp, Dp = -(-G // 32) * 32, -(-D // 8) * 8
    blocks = np.asarray(packed, np.float32).reshape(Gp // 32, Dp // 8, 2, 32, 4)
    return np.ascontiguousarray(blocks.transpose(0, 3, 1, 4, 2).reshape(Gp, Dp)[:G, :D])


class Gallery:
    """Enrolled embeddings to match Results against: `embeddings` (G, D) real numbers, taken as float32, 1 <= G <= 2^24, 1 <= D <= 1024;
    `ids` (G,) int32, default arange(G) -- several templates may share one identity --; `metric` 'COSINE' or 'DOT'.  Made on the host
    (no device is needed): the rows are normalised by rule 2 and packed here, and uploaded once, on the first launch that needs them.
    Immutable; one Gallery may serve any number of requests and networks of the process.  ValueError for a wrong shape, a void row or an
    unknown metric."""
    __slots__ = ('size', 'dim', 'metric', 'ids', 'packed', '_dev', '__weakref__')

    def __init__(self, embeddings, ids=None, metric='COSINE'):
        if metric not in METRICS:
            raise ValueError('Gallery: metric {!r} is not one of {}'.format(metric, sorted(METRICS)))
        try:
            v = np.asarray(embeddings, dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError('Gallery: embeddings are (G, D) real numbers') from None
        if v.ndim != 2 or not 1 <= v.shape[0] <= MAX_G or not 1 <= v.shape[1] <= MAX_D:
            raise ValueError('Gallery: embeddings of shape {}: not (G, D) with 1 <= G <= 2^24 and 1 <= D <= {}'.format(v.shape, MAX_D))
        G, D = v.shape
        if ids is None:
            ids = np.arange(G, dtype=np.int32)
        else:
            given = np.asarray(ids)
            if given.shape != (G,) or given.dtype.kind not in 'iu' or (given.size and (given.min() < -2 ** 31 or given.max() >= 2 ** 31)):
                raise ValueError('Gallery: ids are (G,) = ({},) int32, got {} {}'.format(G, given.dtype, given.shape))
            ids = given.astype(np.int32)
        s, r, finite = norm(v)
        void = ~finite | (s == 0) if metric == 'COSINE' else ~finite
        if void.any():
            raise ValueError('Gallery: row {} is void ({})'.format(int(np.argmax(void)),
                                                                  'an element is not finite' if not finite[np.argmax(void)] else 'all zeros'))
        u = v
        if metric == 'COSINE':
            u = np.empty_like(v)
            for at in range(0, G, 65536):
                u[at:at + 65536] = (v[at:at + 65536].astype(np.float64) / r[at:at + 65536, None]).astype(np.float32)
        packed = pack(u)
        ids.setflags(write=False)
        packed.setflags(write=False)
        for name, value in (('size', G), ('dim', D), ('metric', metric), ('ids', ids), ('packed', packed), ('_dev', None)):
            object.__setattr__(self, name, value)

    def __setattr__(self, name, value):
        raise AttributeError('a Gallery is immutable')

    @property
    def rows(self):
        """The rows as they are matched (normalised under 'COSINE'), (G, D) float32: unpacked from the packed copy."""
        return unpack(self.packed, self.size, self.dim)

    def on_device(self):
        """The packed rows in HBM: uploaded on the first call -- and again after a device.shutdown(), which frees them --, on the current
        stream and before the call returns."""
        if self._dev is None or self._dev[0] != device._pinned_generation:
            object.__setattr__(self, '_dev', (device._pinned_generation, device.DeviceTensor.from_numpy(self.packed)))
        return self._dev[1]

    def __repr__(self):
        return 'Gallery({} x {}, {})'.format(self.size, self.dim, self.metric)


def resolved(value, what='matches') -> GalleryMatch:
    """`value` -- a Gallery or a GalleryMatch -- as a checked GalleryMatch; ValueError."""
    if isinstance(value, Gallery):
        value = GalleryMatch(value)
    if not isinstance(value, GalleryMatch) or not isinstance(value.gallery, Gallery):
        raise ValueError('{}: a Gallery or a GalleryMatch, got {!r}'.format(what, value))
    gallery, k, min_score = value
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= min(gallery.size, MAX_K):
        raise ValueError('{}: k = {!r} outside 1 .. min(G = {}, {})'.format(what, k, gallery.size, MAX_K))
    return GalleryMatch(gallery, int(k), None if min_score is None else ask.checked_min_score(min_score, what))


def match_rows(x, match) -> Matches:
    """The rule in numpy on a host array of shape (n, D) or (n, D, 1, ...): what a Result computed on the host (a foreign plugin set) gets."""
    gallery, k, min_score = resolved(match, 'match_rows')
    x = np.asarray(x)
    rows = rows_of(x.shape)
    if rows is None or x.dtype != np.float32 or rows[1] != gallery.dim:
        raise ValueError('match_rows takes float32 rows of shape (n, {0}) or (n, {0}, 1, ...), got {1} {2}'.format(gallery.dim, x.dtype, x.shape))
    n, D = rows
    x = np.ascontiguousarray(x).reshape(n, D)
    u = gallery.rows
    s, r, finite = norm(x)
    void = ~finite | (s == 0) if gallery.metric == 'COSINE' else ~finite
    counts = np.zeros(n, np.int32)
    indices = np.full((n, k), -1, np.int32)
    scores = np.full((n, k), QUIET_NAN, np.float32)
    position = np.arange(gallery.size)
    for row in np.flatnonzero(~void):
        a = np.zeros(gallery.size, np.float32)
        for d in range(D):
            a = fmaf(x[row, d], u[:, d], a)
        a[a == 0] = np.float32(0.0)
        nan = np.isnan(a)
        best = np.lexsort((position, -np.where(nan, np.float32(0), a), ~nan))[:k]
        with np.errstate(over='ignore', invalid='ignore'):
            score = (a[best].astype(np.float64) / r[row]).astype(np.float32) if gallery.metric == 'COSINE' else a[best].copy()
        score[np.isnan(score)] = QUIET_NAN
        kept = np.ones(k, bool) if min_score is None else score >= np.float32(min_score)
        count = k if kept.all() else int(np.argmin(kept))
        counts[row] = count
        indices[row, :count] = best[:count]
        scores[row, :count] = score[:count]
    return Matches(counts, indices, _ids_of(gallery, indices), scores)


def _ids_of(gallery, indices):
    return np.where(indices >= 0, gallery.ids[np.maximum(indices, 0)], np.int32(-1)).astype(np.int32)


def _fits(port, match, batch):
    rows = rows_of(port['dims'])
    return rows is not None and port['precision'] == 'FP32' and rows[1] == match.gallery.dim


def _none_fits(ports, match, batch):
    return 'matches: no FP32 Result of shape (n, {0}) or (n, {0}, 1, ...) to match against {1!r} (the Results: {2})'.format(
        match.gallery.dim, match.gallery, {name: tuple(port['dims']) for name, port in ports.items()})


def checked(ienet, matches, sharded: bool) -> dict:
    """{Result name: GalleryMatch} of the `matches` argument of infer() / start_async() -- a Gallery (k = 1, no threshold) or a
    GalleryMatch for every FP32 Result declared (n, D) or (n, D, 1, ...) with the gallery's D, or {Result name: either} --, {} for None.
    Everything is looked up in the network as it was read: no device is needed, nothing is allocated.  ValueError ('matches: ...'): an
    unknown name, a value of another type, k or min_score out of range, no such Result for an unnamed form, a sharded batch, a Result of
    another shape, precision or D."""
    if matches is None:
        return {}
    ports, wanted = ask.named(ienet, 'matches', matches, sharded, _fits, _none_fits, resolved)
    for name, match in wanted.items():
        rows = ask.declared('matches', name, ports[name], rows_of(ports[name]['dims']), '(n, D) or (n, D, 1, ...)')
        if rows[1] != match.gallery.dim:
            raise ValueError('matches: Result {!r} has D = {}, {!r} has {}'.format(name, rows[1], match.gallery, match.gallery.dim))
    return wanted


def chunks_of(G: int) -> int:
    return -(-G // CHUNK)


def scratch_bytes(n: int, G: int, k: int) -> int:
    """The scratch block of pvhip_gallery_match_f32: k 64-bit keys per (row, chunk of CHUNK gallery rows)."""
    return 8 * n * chunks_of(G) * k


class Blocks(ask.FlatBlocks):
    """What a request keeps for one (Result name, gallery, k): the scratch block, the device block pvhip_gallery_match_f32 writes
    -- (n,) int32 counts, (n, k) int32 indices, (n, k) float32 scores -- and the page-locked host block it is read back into in one copy
    of 4 n + 8 n k bytes.  None of them depends on min_score, which is an argument of the launch: a caller that varies the threshold
    from call to call keeps one set of blocks.  The scratch is the large one, scratch_bytes(n, G, k) = 8 n ceil(G / CHUNK) k bytes
    (n = 256, G = 1 M, k = 64: 512 MB; k = 5: 40 MB); the blocks hold their Gallery, and so its copy in HBM, until the request's
    release_device_state()."""
    __slots__ = ('n', 'gallery', 'k', 'scratch')

    def __init__(self, n: int, gallery: Gallery, k: int):
        super().__init__(n + 2 * n * k)
        self.n, self.gallery, self.k = n, gallery, k
        self.scratch = device.DeviceTensor.empty((scratch_bytes(n, gallery.size, k) // 8,), np.int64)

    def launch(self, result, min_score):
        """The launch pair on the current stream, behind whatever wrote `result` there (and behind the gallery's upload, the first time)."""
        n, D = rows_of(result.shape)
        gallery, k = self.gallery, self.k
        assert n == self.n and D == gallery.dim and result.dtype == np.float32
        packed = gallery.on_device()
        at = self.dev.ptr
        device.call('pvhip_gallery_match_f32', device.ptr(result), n, D, ctypes.c_void_p(packed.ptr), gallery.size, k, METRICS[gallery.metric],
                    int(min_score is not None), float(min_score or 0.0), ctypes.c_void_p(self.scratch.ptr), ctypes.c_void_p(at),
                    ctypes.c_void_p(at + 4 * n), ctypes.c_void_p(at + 4 * n + 4 * n * k), ctypes.c_void_p(0))

    def read_back(self) -> Matches:
        """The answer, copied on the current stream, which has drained; the arrays are the caller's own."""
        host, n, k = self.words(), self.n, self.k
        indices = host[n:n + n * k].reshape(n, k).copy()
        return Matches(host[:n].copy(), indices, _ids_of(self.gallery, indices), host[n + n * k:].view(np.float32).reshape(n, k).copy())


class Ask(ask.Ask, collections.namedtuple('Ask', 'match')):
    """A Result asked for with matches=, in its resolved form."""
    __slots__ = ()
    KEYWORD = 'matches'

    def key(self, name):
        """(name, id of the gallery, k): what the blocks' sizes depend on.  min_score is no part of it -- it goes with the launch --, so
        that thresholds that vary from call to call share one scratch block."""
        return (name, id(self.match.gallery), self.match.k)

    def blocks_for(self, value):
        return Blocks(rows_of(value.shape)[0], self.match.gallery, self.match.k)

    def launch_with(self):
        return (self.match.min_score,)

    def on_host(self, value):
        return match_rows(value, self.match)
