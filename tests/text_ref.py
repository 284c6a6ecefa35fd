"""The rule of ``infer(..., text=...)`` (pvhip_ctc_greedy_f32) in plain loops.  This is the specification; the kernel and
pyopenvino_amd/text.py equal it bit for bit.

For batch row r with scores v[t][c] of a float32 tensor read as 'TNC' (T, n, C), 'NTC' (n, T, C) or 'NCT' (n, C, T):
  1. winner  w(t) is the first class of timestep t in top_k's total order: NaN of any sign or payload first, then descending with
     +0.0 == -0.0, ties to the lower class.
  2. void    row r is void iff the winning score of any of its timesteps is NaN, that is, iff any of its T * C scores is NaN.
     A void row has length -1 and nothing but filler: the quiet-NaN rows behind `count` of a DetectedRois or LandmarkWarps pass
     are void.  An empty string (length 0) is an answer and not a void row.
  3. emit    timestep t emits iff w(t) != blank and (merge_repeated is false, or t == 0, or w(t) != w(t - 1)).  A repeat across
     a blank therefore emits twice: a, blank, a is aa.
  4. order   the emitting timesteps in ascending t fill slots 0, 1, ...: symbols = w(t), scores = the bits of v[t][w(t)],
     steps = t.
Row r's first lengths[r] slots are its string in time order; the slots behind them -- all of them in a void row -- are
(-1, quiet NaN, -1)."""
import collections

import numpy as np

Text = collections.namedtuple('Text', 'lengths symbols scores steps')
QUIET_NAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def extents(shape, layout):
    """(n, T, C) of a rank-3 shape read as `layout`."""
    a, b, c = shape
    return {'TNC': (b, a, c), 'NTC': (a, b, c), 'NCT': (a, c, b)}[layout]


def at(layout, r, t, c):
    """The index of v[t][c] of batch row r in a tensor read as `layout`."""
    return {'TNC': (t, r, c), 'NTC': (r, t, c), 'NCT': (r, c, t)}[layout]


def first_class(values):
    """Rule 1 on the scores of one timestep, a list of Python floats: the class that stands first."""
    best = 0
    for c in range(1, len(values)):
        v, b = values[c], values[best]
        if b != b:                      # a NaN already stands first: a later one does not replace it
            break
        if v != v or v > b:             # (+0.0 == -0.0: neither is larger, the lower class stays)
            best = c
    return best


def winners_of(x, layout):
    """[[w(t) for t in range(T)] for r in range(n)] and whether each (r, t) winner's score is a NaN, of a float32 array."""
    n, T, C = extents(x.shape, layout)
    with np.errstate(invalid='ignore'):                         # (a signalling NaN becomes a quiet one: a NaN either way)
        values = x.astype(np.float64).tolist()                  # exact: every float32 is a float64; -0.0 stays -0.0
    wins, nans = [], []
    for r in range(n):
        row_w, row_nan = [], []
        for t in range(T):
            scores = []
            for c in range(C):
                i, j, k = at(layout, r, t, c)
                scores.append(values[i][j][k])
            w = first_class(scores)
            row_w.append(w)
            row_nan.append(scores[w] != scores[w])
        wins.append(row_w)
        nans.append(row_nan)
    return wins, nans


def greedy(x, layout, blank=-1, merge_repeated=True, winners=None) -> Text:
    """The rule on a float32 array of rank 3 read as `layout`; `blank` in -C .. C - 1.  `winners`: winners_of(x, layout), when the caller
    has it."""
    assert x.dtype == np.float32 and x.ndim == 3
    n, T, C = extents(x.shape, layout)
    assert -C <= blank < C and C >= 2 and T >= 1
    if blank < 0:
        blank += C
    wins, nans = winners if winners is not None else winners_of(x, layout)
    out = Text(np.zeros(n, np.int32), np.full((n, T), -1, np.int32), np.full((n, T), QUIET_NAN, np.float32), np.full((n, T), -1, np.int32))
    bits, out_bits = x.view(np.uint32), out.scores.view(np.uint32)
    for r in range(n):
        if any(nans[r]):                                        # rule 2
            out.lengths[r] = -1
            continue
        slot = 0
        for t in range(T):
            w = wins[r][t]
            if w != blank and (not merge_repeated or t == 0 or w != wins[r][t - 1]):      # rule 3
                out.symbols[r, slot] = w                        # rule 4
                out_bits[r, slot] = bits[at(layout, r, t, w)]
                out.steps[r, slot] = t
                slot += 1
        out.lengths[r] = slot
    return out
