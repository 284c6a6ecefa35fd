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

from . import device

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
    None.  Everything is looked up in the network as it was read: no device is needed, nothing is allocated."""
    if top_k is None:
        return {}
    results = {name: ienet.G.nodes[nid] for nid, name in ienet.find_node_by_type('Result')}
    if isinstance(top_k, dict):
        unknown = [name for name in top_k if name not in results]
        if unknown:
            raise ValueError('top_k: the network has no Result named {!r} (it has {})'.format(unknown[0], sorted(results)))
        wanted = dict(top_k)
    else:
        wanted = {name: top_k for name in results}
    if wanted and sharded:
        raise ValueError('top_k: not with a batch sharded over ranks')
    out = {}
    for name, k in wanted.items():
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError('top_k: Result {!r}: k is a count from 1 to {}, got {!r}'.format(name, MAX_K, k))
        port = next(iter(results[name]['input'].values()))
        rows = rows_of(port['dims'])
        if rows is None:
            raise ValueError('top_k: Result {!r} has shape {}: not (n, C) or (n, C, 1, ...)'.format(name, tuple(port['dims'])))
        if port['precision'] != 'FP32':
            raise ValueError('top_k: Result {!r} is {}: FP32 Results only'.format(name, port['precision']))
        if not 1 <= k <= min(rows[1], MAX_K):
            raise ValueError('top_k: Result {!r}: k = {} outside 1 .. min(C = {}, {})'.format(name, int(k), rows[1], MAX_K))
        out[name] = int(k)
    return out


class Blocks:
    """What a request keeps for one (Result name, k): the device block pvhip_topk_rows_f32 writes -- (n, k) int32 indices, then (n, k)
    float32 values -- and the page-locked host block it is read back into in one copy of 8 n k bytes."""
    __slots__ = ('n', 'k', 'dev', 'host')

    def __init__(self, n: int, k: int):
        self.n, self.k = n, k
        self.dev = device.DeviceTensor.empty((2, n, k), np.int32)
        self.host = device.host_empty((2, n, k), np.int32)

    def launch(self, result):
        """One launch on the current stream, behind whatever wrote `result` there."""
        n, C = rows_of(result.shape)
        assert n == self.n and result.dtype == np.float32
        device.call('pvhip_topk_rows_f32', device.ptr(result), n, C, self.k, ctypes.c_void_p(self.dev.ptr),
                    ctypes.c_void_p(self.dev.ptr + 4 * n * self.k))

    def read_back(self) -> TopK:
        """The pair, copied on the current stream, which has drained; the arrays are the caller's own."""
        device.call('pvhip_memcpy_d2h', ctypes.c_void_p(self.host.ctypes.data), ctypes.c_void_p(self.dev.ptr), self.host.nbytes)
        return TopK(self.host[0].copy(), self.host[1].view(np.float32).copy())


class Ask(collections.namedtuple('Ask', 'k')):
    """A Result asked for with top_k=k, as answers.py drives it: the key of its blocks, the launch on the value a pass left on the
    device -- into `blocks`, or into new ones for None: they are returned --, and the rule on a host value."""
    __slots__ = ()

    def bound(self, inputs, slots):
        return self

    def key(self, name):
        return (name, self.k)

    def launch(self, blocks, value):
        blocks = blocks or Blocks(rows_of(value.shape)[0], self.k)
        blocks.launch(value)
        return blocks

    def on_host(self, value):
        return top_k_rows(value, self.k)
