"""The k best classes of a classifier's Result (``infer(..., top_k=k)``): the rule, the argument checks and the device launch.

The rule (include/pvhip.h, pvhip_topk_rows_f32; tests/topk_ref.py is the same again): for a row x[0..C) of float32 and 1 <= k <= min(C, 64)
the answer is the first k positions of the row sorted by this total order:
  1. NaN (any sign, any payload) ranks before every number -- a poisoned row shows NaN as its first score instead of hiding it (the rows
     behind `count` of a DetectedRois pass are such rows);
  2. then by value, descending; +0.0 and -0.0 are equal;
  3. equal rank (ties, zeros of either sign, several NaNs): the lower index first.
On rows without ties or NaN this is the reference sample's ``np.argsort(row)[::-1][:k]``.  `values` are the row's own bits at `indices`."""
import collections
import ctypes

import numpy as np

from . import ask, device

MAX_K = 64

TopK = collections.namedtuple('TopK', 'indices values')
TopK.__doc__ = 'What a Result started with top_k=k comes back as: `indices` (n, k) int32 and `values` (n, k) float32, best first.'


def top_k_rows(x, k: int) -> TopK:
    """The rule in numpy on a host array of shape (n, C) or (n, C, 1, ...): what a Result computed on the host (a foreign plugin set) gets."""
    x = np.asarray(x)
    rows = rows_of(x.shape)
    if rows is None or x.dtype != np.float32:
        raise ValueError('top_k takes float32 rows of shape (n, C) or (n, C, 1, ...), got {} {}'.format(x.dtype, x.shape))
    n, C = rows
    if not 1 <= k <= min(C, MAX_K):
        raise ValueError('top_k = {} outside 1 .. min(C = {}, {})'.format(k, C, MAX_K))
    x = np.ascontiguousarray(x).reshape(n, C)
    indices = np.empty((n, k), np.int32)
    position = np.arange(C)
    for r in range(n):
        nan = np.isnan(x[r])
        indices[r] = np.lexsort((position, -np.where(nan, np.float32(0), x[r]), ~nan))[:k]
    return TopK(indices, np.take_along_axis(x, indices.astype(np.int64), axis=1))


def rows_of(dims):
    """(n, C) of a tensor declared (n, C) or (n, C, 1, ...): one row of C scores per image; None for any other shape."""
    dims = tuple(int(d) for d in dims)
    if len(dims) < 2 or dims[0] < 1 or dims[1] < 1 or any(d != 1 for d in dims[2:]):
        return None
    return dims[0], dims[1]


def checked(ienet, top_k, sharded: bool) -> dict:
    """{Result name: k} of the `top_k` argument of infer() / start_async() -- an int for every Result, or {Result name: k} --, {} for
    None.  Everything is looked up in the network as it was read: no device is needed, nothing is allocated.  ValueError ('top_k: ...'):
    an unknown name, a sharded batch, a k that is no count, a Result whose declared shape is not (n, C) or (n, C, 1, ...) or that is not
    FP32, k outside 1 .. min(C, 64)."""
    if top_k is None:
        return {}
    ports, wanted = ask.named(ienet, 'top_k', top_k, sharded)
    out = {}
    for name, k in wanted.items():
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError('top_k: Result {!r}: k is a count from 1 to {}, got {!r}'.format(name, MAX_K, k))
        rows = ask.declared('top_k', name, ports[name], rows_of(ports[name]['dims']), '(n, C) or (n, C, 1, ...)')
        if not 1 <= k <= min(rows[1], MAX_K):
            raise ValueError('top_k: Result {!r}: k = {} outside 1 .. min(C = {}, {})'.format(name, int(k), rows[1], MAX_K))
        out[name] = int(k)
    return out


class Blocks(ask.FlatBlocks):
    """What a request keeps for one (Result name, k): the device block pvhip_topk_rows_f32 writes -- (n, k) int32 indices, then (n, k)
    float32 values -- and the page-locked host block it is read back into in one copy of 8 n k bytes."""
    __slots__ = ('n', 'k')

    def __init__(self, n: int, k: int):
        super().__init__(2 * n * k)
        self.n, self.k = n, k

    def launch(self, result):
        """One launch on the current stream, behind whatever wrote `result` there."""
        n, C = rows_of(result.shape)
        assert n == self.n and result.dtype == np.float32
        device.call('pvhip_topk_rows_f32', device.ptr(result), n, C, self.k, ctypes.c_void_p(self.dev.ptr),
                    ctypes.c_void_p(self.dev.ptr + 4 * n * self.k))

    def read_back(self) -> TopK:
        """The pair, copied on the current stream, which has drained; the arrays are the caller's own."""
        pair = self.words().reshape(2, self.n, self.k)
        return TopK(pair[0].copy(), pair[1].view(np.float32).copy())


class Ask(ask.Ask, collections.namedtuple('Ask', 'k')):
    """A Result asked for with top_k=k."""
    __slots__ = ()
    KEYWORD = 'top_k'

    def key(self, name):
        return (name, self.k)

    def blocks_for(self, value):
        return Blocks(rows_of(value.shape)[0], self.k)

    def on_host(self, value):
        return top_k_rows(value, self.k)
