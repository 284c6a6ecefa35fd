"""The gallery-matching rule of include/pvhip.h (pvhip_gallery_match_f32) again, written from its text alone in numpy and plain loops;
pyopenvino_amd/gallery.py is not imported.  test_gallery.py holds the product against it bit for bit.

fmaf has no numpy form (and Python 3.10 no math.fma): it is restated by rounding to odd -- the product of two float32 is exact in float64
(48 bits), it is added to c in float64, TwoSum gives the exact residual, and a sum that is inexact and even in its last mantissa bit
moves one ulp toward the residual; then one .astype(float32).  fma_exact is the same value through exact rationals, for the test that
holds the restatement (and glibc's fmaf) against it."""
import collections
import fractions

import numpy as np

Matches = collections.namedtuple('Matches', 'counts indices ids scores')
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def fma_exact(a, b, c):
    """fmaf(a, b, c) of three finite float32 scalars through exact rationals: one rounding, by numpy's float32 of an exactly rounded
    float64 would round twice, so the rational is rounded to float32 here, to nearest even, by hand."""
    exact = fractions.Fraction(float(a)) * fractions.Fraction(float(b)) + fractions.Fraction(float(c))
    if exact == 0:
        return np.float32(0.0) if not (np.signbit(np.float32(a) * np.float32(b)) and np.signbit(c)) else np.float32(-0.0)
    sign, mag = (-1 if exact < 0 else 1), abs(exact)
    e = mag.numerator.bit_length() - mag.denominator.bit_length()         # 2^(e-1) <= mag < 2^(e+1)
    if fractions.Fraction(2) ** e > mag:
        e -= 1
    e = max(e, -126)                                                        # subnormals share the exponent of the smallest normal
    ulp = fractions.Fraction(2) ** (e - 23)
    q, rest = divmod(mag, ulp)
    q = int(q)
    if rest * 2 > ulp or (rest * 2 == ulp and q & 1):
        q += 1
    value = fractions.Fraction(q) * ulp
    if value >= fractions.Fraction(2) ** 128:
        return np.float32(sign * np.inf)
    return np.float32(sign * float(value))                                  # exact: value is a float32


def fmaf(a, b, c):
    """Elementwise fmaf of float32 arrays of one shape."""
    a64, b64, c64 = (np.asarray(t, np.float32).astype(np.float64) for t in (a, b, c))
    with np.errstate(all='ignore'):
        p = a64 * b64
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)
        bits = np.ascontiguousarray(s).view(np.int64)
        step = np.isfinite(s) & (err != 0) & ((bits & 1) == 0)
        # one ulp toward the residual: away from zero when the residual has the sum's sign (an inexact sum is not zero)
        bits = bits + np.where(step, np.where((err > 0) == (s > 0), 1, -1), 0)
        return bits.view(np.float64).astype(np.float32)


def norms(v):
    """Rule 1 for every row of a float32 (n, D): (s, r, some element is not finite), the sum in the order of d, one addition at a time."""
    v = np.asarray(v, np.float32)
    s = np.zeros(v.shape[0], np.float64)
    with np.errstate(all='ignore'):
        for d in range(v.shape[1]):
            w = v[:, d].astype(np.float64)
            s = s + w * w
        return s, np.sqrt(s), ~np.isfinite(v).all(axis=1)


def norm_row(v):
    """(s, r, void by a non-finite element) of one float32 row, in plain Python floats (binary64)."""
    s = 0.0
    bad = False
    for t in v:
        if not np.isfinite(t):
            bad = True
        w = float(t)
        with np.errstate(all='ignore'):
            s = float(np.float64(s) + np.float64(w) * np.float64(w))
    with np.errstate(all='ignore'):
        return s, float(np.sqrt(np.float64(s))), bad


def gallery_rows(v, metric):
    """Rule 2: the rows as they are matched; ValueError for a void row."""
    v = np.asarray(v, np.float32)
    s, r, bad = norms(v)
    if bad.any() or (metric == 'COSINE' and (s == 0.0).any()):
        raise ValueError('void gallery row')
    if metric == 'DOT':
        return v.copy()
    assert metric == 'COSINE'
    return (v.astype(np.float64) / r[:, None]).astype(np.float32)


def chains(x, u, piece=1 << 15):
    """Rule 3: a (n, G) float32 of x (n, D) and u (G, D); the gallery in pieces whose work arrays stay in cache."""
    n, D = x.shape
    G = u.shape[0]
    a = np.zeros((n, G), np.float32)
    step = max(1, piece // n)
    for g0 in range(0, G, step):
        part = a[:, g0:g0 + step]
        for d in range(D):
            part = fmaf(np.broadcast_to(x[:, d:d + 1], part.shape), np.broadcast_to(u[None, g0:g0 + step, d], part.shape), part)
        a[:, g0:g0 + step] = part
    return a


def order(a_row, k):
    """Rule 4 on one row of chain values: the first k gallery rows."""
    nan = np.isnan(a_row)
    return np.lexsort((np.arange(len(a_row)), -np.where(nan, np.float32(0), a_row), ~nan))[:k]     # (-0.0 == +0.0 as sort keys)


def live_chains(x, u):
    """The chain values match() looks at: a void row's are those of a row of zeros."""
    return chains(np.where(np.isfinite(x), x, np.float32(0)), u)


def orders(a, k):
    """Rule 4 on every row of the chain values a (n, G): (n, k)."""
    return np.stack([order(row, k) for row in a])


def match(x, u, ids, metric, k, min_score=None, a=None, best=None):
    """Rules 3 - 6 for the query rows x (n, D) float32 against the matched rows u (G, D) (gallery_rows' output) with `ids` (G,); `a`,
    `best`: live_chains(x, u) and orders(a, k) where a caller has them already."""
    x = np.asarray(x, np.float32)
    n = x.shape[0]
    a = live_chains(x, u) if a is None else a
    a = np.where(a == 0, np.float32(0.0), a)                                    # a zero of either sign counts as +0.0
    counts = np.zeros(n, np.int32)
    indices = np.full((n, k), -1, np.int32)
    out_ids = np.full((n, k), -1, np.int32)
    scores = np.full((n, k), QNAN, np.float32)
    sums, roots, bads = norms(x)
    for r in range(n):
        s, root, bad = sums[r], roots[r], bads[r]
        if bad or (metric == 'COSINE' and s == 0.0):
            continue
        for j, g in enumerate(order(a[r], k) if best is None else best[r]):
            with np.errstate(all='ignore'):
                score = a[r, g] if metric == 'DOT' else np.float32(np.float64(a[r, g]) / np.float64(root))
            if np.isnan(score):
                score = QNAN
            if min_score is not None and not score >= np.float32(min_score):
                break
            counts[r] = j + 1
            indices[r, j], out_ids[r, j], scores[r, j] = g, ids[g], score
    return Matches(counts, indices, out_ids, scores)
