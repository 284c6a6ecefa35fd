"""The rule of ``infer(..., top_k=k)`` (pvhip_topk_rows_f32) in plain numpy.  This is the specification; the kernel equals it index for
index, and its values bit for bit.

For a row x[0..C) of float32 and 1 <= k <= min(C, 64) the answer is the first k positions of the row sorted by this total order:
  1. NaN (any sign, any payload) ranks before every number;
  2. then by value, descending; +0.0 and -0.0 are equal;
  3. equal rank (ties, zeros of either sign, several NaNs): the lower index first.
`indices` is int32; `values[r, j]` holds the bits of x[r, indices[r, j]] unchanged.  On a row without ties or NaN this is
np.argsort(row)[::-1][:k], what the reference's sample computes."""
import collections

import numpy as np

TopK = collections.namedtuple('TopK', 'indices values')


def top_k_row(row, k):
    """The k positions of one row, best first."""
    row = np.asarray(row)
    assert row.dtype == np.float32 and row.ndim == 1 and 1 <= k <= min(row.shape[0], 64)
    isnan = np.isnan(row)
    return np.lexsort((np.arange(row.shape[0]), -np.where(isnan, 0, row), ~isnan))[:k]


def top_k(x, k):
    """TopK(indices (n, k) int32, values (n, k) float32) of float32 `x` of shape (n, C) or (n, C, 1, ...)."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim >= 2 and all(d == 1 for d in x.shape[2:])
    x = x.reshape(x.shape[0], x.shape[1])
    indices = np.stack([top_k_row(row, k) for row in x], 0).astype(np.int32)
    values = np.stack([row[i] for row, i in zip(x, indices)], 0)
    return TopK(indices, values)
