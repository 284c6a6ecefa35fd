"""Gallery matching on the device (``infer(..., matches=Gallery(...))``): the rule of include/pvhip.h in its three statements (the header,
pyopenvino_amd/gallery.py, tests/gallery_ref.py), the packing, the argument checks, and pvhip_gallery_match_f32 against the rule bit for
bit."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import gallery_ref
import helpers
import test_detected_rois as det_tests
import test_roi_input as roi_tests
import test_top_k as top_k_tests
from helpers import MODELS

from pyopenvino_amd import gallery as gallery_rule
from pyopenvino_amd import Gallery, GalleryMatch, Matches

ENTRY = 'pvhip_gallery_match_f32'
C = gallery_rule.CHUNK
_net = roi_tests._net


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what=''):
    """`got` (a Matches of the product) equals `want` (the rule's): counts, indices and ids exact, scores bit for bit."""
    assert got.counts.dtype == got.indices.dtype == got.ids.dtype == np.int32 and got.scores.dtype == np.float32, what
    assert got.counts.shape == want.counts.shape and got.indices.shape == got.ids.shape == got.scores.shape == want.indices.shape, what
    assert np.array_equal(got.counts, want.counts), '{}: counts {} want {}'.format(what, got.counts.tolist(), want.counts.tolist())
    bad = np.flatnonzero((got.indices != want.indices).any(axis=1))
    assert not len(bad), '{}: row {}: indices {} want {}'.format(what, bad[0], got.indices[bad[0]].tolist(), want.indices[bad[0]].tolist())
    assert np.array_equal(got.ids, want.ids), what
    bad = np.flatnonzero((_bits(got.scores) != _bits(want.scores)).any(axis=1))
    assert not len(bad), '{}: row {}: score bits {} want {}'.format(what, bad[0], _bits(got.scores)[bad[0]].tolist(), _bits(want.scores)[bad[0]].tolist())


def _ref(x, gallery_values, ids, metric, k, min_score=None):
    return gallery_ref.match(x, gallery_ref.gallery_rows(gallery_values, metric), ids, metric, k, min_score)


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
def _double_rounding_cases():
    """(a, b, c): a * b = 1 - 2^-46 lies 2^-46 below the midpoint 2^24 + 3 of the float32 neighbours of c + a * b -- bits that the float64
    sum drops --, scaled through the exponent range, and mirrored."""
    one_up, one_down = np.float32(1 + 2.0 ** -23), np.float32(1 - 2.0 ** -23)
    cases = []
    for s in range(-90, 91, 6):
        scale = np.float32(2.0 ** s)
        for sign in (1, -1):
            cases.append((np.float32(sign) * one_up * scale, one_down, np.float32(sign) * np.float32(2.0 ** 24 + 2) * scale))
    return [np.array(t, np.float32) for t in zip(*cases)]


def test_fmaf_restatement_equals_glibc_and_exact_rationals():
    rng = np.random.default_rng(7)
    n = 120000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-40, 40, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-40, 40, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-60, 60, n)).astype(np.float32)
    c[:n // 2] = (-a[:n // 2].astype(np.float64) * b[:n // 2] * (1 + rng.standard_normal(n // 2) * 2.0 ** -20)).astype(np.float32)   # cancellation
    tiny = 40000                                                                # results in and around the subnormal range
    at = (rng.standard_normal(tiny) * 2.0 ** rng.integers(-80, -60, tiny)).astype(np.float32)
    bt = (rng.standard_normal(tiny) * 2.0 ** rng.integers(-75, -55, tiny)).astype(np.float32)
    ct = (rng.standard_normal(tiny) * 2.0 ** rng.integers(-150, -126, tiny)).astype(np.float32)
    da, db, dc = _double_rounding_cases()
    a, b, c = np.concatenate([a, at, da]), np.concatenate([b, bt, db]), np.concatenate([c, ct, dc])
    got = gallery_rule.fmaf(a, b, c)
    again = gallery_ref.fmaf(a, b, c)
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(again))
    sub = (np.abs(got) < np.float32(2.0 ** -126)) & (got != 0)
    assert sub.sum() > 1000                                                     # subnormal results are among them
    naive = (da.astype(np.float64) * db + dc).astype(np.float32)               # the float64 route rounds twice on the constructed cases
    assert (naive != got[-len(da):]).all()
    pick = np.concatenate([rng.choice(len(a), 1500, replace=False), np.flatnonzero(sub)[:300], np.arange(len(a) - len(da), len(a))])
    exact = np.array([gallery_ref.fma_exact(a[i], b[i], c[i]) for i in pick], np.float32)
    assert np.array_equal(_bits(got[pick]), _bits(exact))
    try:
        libm = ctypes.CDLL('libm.so.6')
        libm.fmaf.restype = ctypes.c_float
        libm.fmaf.argtypes = [ctypes.c_float] * 3
    except (OSError, AttributeError):
        return                                                                  # (no glibc fmaf here: the rationals above stand)
    want = np.array([libm.fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], np.float32)
    assert np.array_equal(_bits(got), _bits(want))
    # and a chain
    x = rng.standard_normal((4, 128)).astype(np.float32)
    u = rng.standard_normal((300, 128)).astype(np.float32)
    chain = gallery_ref.chains(x, u)
    for r, g in ((0, 0), (1, 17), (3, 299), (2, 150)):
        acc = 0.0
        for d in range(128):
            acc = libm.fmaf(float(x[r, d]), float(u[g, d]), acc)
        assert np.float32(acc) == chain[r, g]


def test_the_rule_on_hand_written_rows():
    eye = np.eye(8, dtype=np.float32) * np.float32(4.0)                        # an orthogonal gallery: the normalised rows are the unit vectors
    x = np.array([[0.5, 0.25, 0, 0, 0, 0, 0, 0.125], [3, 4, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, np.inf, 0, 0, 0, 0],
                  [0, 0, np.nan, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, -2, 0, 0]], np.float32)
    for rule in (lambda k, ms, metric: gallery_rule.match_rows(x, GalleryMatch(Gallery(eye, metric=metric), k, ms)),
                 lambda k, ms, metric: _ref(x, eye, np.arange(8), metric, k, ms)):
        got = rule(3, None, 'DOT')                                              # dyadic scores, exact: the chain of x with 4 e_g is 4 x[g]
        assert got.counts.tolist() == [3, 3, 3, 0, 0, 3]
        assert got.indices[0].tolist() == [0, 1, 7] and got.scores[0].tolist() == [2.0, 1.0, 0.5]
        assert got.indices[1].tolist() == [1, 0, 2] and got.scores[1].tolist() == [16.0, 12.0, 0.0]
        assert got.indices[2].tolist() == [0, 1, 2] and got.scores[2].tolist() == [0.0, 0.0, 0.0]      # all zero: not void under DOT, ties to the lower index
        assert got.indices[5].tolist() == [0, 1, 2] and got.scores[5].tolist() == [0.0, 0.0, 0.0]      # -8 at row 5 loses to the zeros
        for r in (3, 4):                                                        # each void kind voids only its own row
            assert got.indices[r].tolist() == [-1] * 3 and got.ids[r].tolist() == [-1] * 3 and (_bits(got.scores[r]) == 0x7FC00000).all()
        got = rule(2, None, 'COSINE')
        assert got.counts.tolist() == [2, 2, 0, 0, 0, 2]                        # all zero is void under COSINE
        assert got.indices[1].tolist() == [1, 0] and got.scores[1].tolist() == [np.float32(0.8), np.float32(0.6)]       # r is exactly 5
        assert got.indices[5].tolist() == [0, 1] and got.scores[5].tolist() == [0.0, 0.0]
        got = rule(3, 0.7, 'COSINE')                                            # min_score cuts the run
        assert got.counts.tolist() == [1, 1, 0, 0, 0, 0] and got.indices[1].tolist() == [1, -1, -1]
        assert _bits(got.scores[1]).tolist() == [int(_bits(np.float32(0.8))[0]), 0x7FC00000, 0x7FC00000]
    assert gallery_rule.norm(x[1:2])[1][0] == 5.0 and gallery_ref.norm_row(x[1])[:2] == (25.0, 5.0)
    # duplicated gallery rows and several templates of one identity: ties go to the lower gallery row
    rows = np.array([[1, 2, 3], [2, 4, 6], [1, 2, 3], [-1, 0, 0], [1, 2, 3]], np.float32)
    ids = np.array([7, 7, 9, 3, 7], np.int32)
    q = np.array([[1, 2, 3]], np.float32)
    for metric in ('COSINE', 'DOT'):
        got = gallery_rule.match_rows(q, GalleryMatch(Gallery(rows, ids, metric), 4))
        _same(got, _ref(q, rows, ids, metric, 4), metric)
        assert got.indices[0].tolist() == ([0, 1, 2, 4] if metric == 'COSINE' else [1, 0, 2, 4]) and got.ids[0].tolist() == [7, 7, 9, 7]
    for bad, kw in ((np.zeros((2, 3)), {}), (np.ones(3), {}), (np.ones((2, 1025)), {}), (np.ones((0, 3)), {}), ([[1, np.nan]], {}),
                    ([[1, np.inf]], {'metric': 'DOT'}), (np.ones((2, 3)), {'metric': 'L2'}), (np.ones((2, 3)), {'ids': [1, 2, 3]}),
                    (np.ones((2, 3)), {'ids': [0.5, 1.0]})):
        with pytest.raises(ValueError, match='Gallery: '):
            Gallery(bad, **kw)
    g = Gallery(np.zeros((2, 3)) + [[0, 0, 0], [1, 0, 0]], metric='DOT')        # an all-zero row is no void row under DOT
    with pytest.raises(AttributeError):
        g.metric = 'COSINE'
    with pytest.raises(ValueError):
        g.packed[0] = 1.0


def _random_case(rng, n, D, G, huge=False):
    x = rng.standard_normal((n, D)).astype(np.float32)
    v = rng.standard_normal((G, D)).astype(np.float32)
    if huge:
        x *= np.float32(2.0 ** 100)
        v *= np.float32(2.0 ** 27)
    return x, v, rng.integers(0, max(1, G // 2), G).astype(np.int32)


def test_three_restatements_agree():
    """gallery.match_rows is gallery_ref bit for bit: random rows, ties, void rows, overflowing chains, both metrics, with a threshold."""
    rng = np.random.default_rng(11)
    for n, D, G, k in ((1, 1, 1, 1), (4, 7, 40, 5), (6, 33, 70, 64), (3, 128, 300, 10)):
        for huge in (False, True):
            x, v, ids = _random_case(rng, n, D, G, huge)
            if G > 4:
                v[G - 1] = v[1]
                v[3] = v[1]
            if n > 2:
                x[1] = 0
                x[2, D // 2] = -np.inf
            for metric in ('COSINE', 'DOT'):
                gal = Gallery(v, ids, metric)
                assert np.array_equal(_bits(gal.rows), _bits(gallery_ref.gallery_rows(v, metric)))
                whole = gallery_rule.match_rows(x, GalleryMatch(gal, k))
                _same(whole, _ref(x, v, ids, metric, k), (n, D, G, k, huge, metric))
                finite = whole.scores[np.isfinite(whole.scores)]
                ms = float(np.median(finite)) if len(finite) else 0.0
                _same(gallery_rule.match_rows(x.reshape(n, D, 1, 1), GalleryMatch(gal, k, ms)), _ref(x, v, ids, metric, k, ms), (n, D, G, k, huge, metric, ms))
    x, v, ids = _random_case(rng, 2, 4, 50)                                     # an overflowed chain stays at its infinity (the product is not rounded)
    v *= np.float32(2.0 ** -20)
    v[7] = (3e38, -3e38, 0, 0)
    x[0] = (3e38, 3e38, 1, 1)
    got = gallery_rule.match_rows(x, GalleryMatch(Gallery(v, metric='DOT'), 3))
    _same(got, _ref(x, v, np.arange(50), 'DOT', 3), 'overflow')
    assert got.indices[0, 0] == 7 and got.scores[0, 0] == np.inf and got.counts[0] == 3


def test_scores_are_inside_the_derived_bound_of_the_float64_cosines():
    """|score - cos| <= gamma(D + 4) * sum |x_d| |v_d| / (|x| |v|), gamma(m) = m u / (1 - m u), u = 2^-24.  The roundings counted: one of
    every gallery element to float32 after the division by r; D of the chain (one per fmaf); one of the score to float32; and two for
    the binary64 roundings of the two r and of the two divisions, each below 2^-52 -- counted as whole u, generously."""
    rng = np.random.default_rng(13)
    for D in (8, 100, 512, 1000):
        x, v, ids = _random_case(rng, 6, D, 60)
        got = gallery_rule.match_rows(x, GalleryMatch(Gallery(v), 60))
        x64, v64 = x.astype(np.float64), v.astype(np.float64)
        nx, nv = np.sqrt((x64 * x64).sum(1)), np.sqrt((v64 * v64).sum(1))
        cos = (x64 @ v64.T) / nx[:, None] / nv[None, :]
        mass = (np.abs(x64) @ np.abs(v64).T) / nx[:, None] / nv[None, :]
        m, u = D + 4, 2.0 ** -24
        bound = m * u / (1 - m * u) * mass
        at = got.indices.astype(np.int64)
        err = np.abs(got.scores.astype(np.float64) - np.take_along_axis(cos, at, 1))
        assert (got.counts == 60).all() and (err <= np.take_along_axis(bound, at, 1)).all(), (D, float((err / np.take_along_axis(bound, at, 1)).max()))


def test_packing():
    rng = np.random.default_rng(17)
    for G in (1, 31, 32, 33, 65):
        for D in (1, 7, 8, 9, 1000):
            u = rng.standard_normal((G, D)).astype(np.float32)
            u[u == 0] = 1
            packed = gallery_rule.pack(u)
            Gp, Dp = -(-G // 32) * 32, -(-D // 8) * 8
            assert packed.dtype == np.float32 and packed.shape == (Gp * Dp,)
            assert np.array_equal(gallery_rule.unpack(packed, G, D), u)
            assert np.count_nonzero(packed) == G * D                            # the pads are zero
            for g, d in {(0, 0), (G - 1, D - 1), (G // 2, D // 2), (G - 1, 0), (0, D - 1), (min(G - 1, 32), min(D - 1, 8))}:
                lane = ((d & 1) << 5) | (g & 31)                                # the stated lane formula
                assert packed[((g // 32 * (Dp // 8) + d // 8) * 64 + lane) * 4 + ((d & 7) >> 1)] == u[g, d]


def test_argument_rules(monkeypatch):
    """Every refusal is a ValueError('matches: ...') raised before anything is staged or launched: this test runs where there is no device."""
    n = 4
    ie, net, name = _net(batch=n)
    ex = ie.load_network(net, 'GPU', num_requests=2)
    out_name = net.outputs[0]['name']
    assert tuple(net.outputs[0]['input'][0]['dims']) == (n, 1000)
    x = np.zeros((n, 3, 224, 224), np.float32)
    req = ex.requests[0]
    rng = np.random.default_rng(19)
    gal = Gallery(rng.standard_normal((70, 1000)).astype(np.float32))
    small = Gallery(rng.standard_normal((3, 1000)).astype(np.float32))
    other = Gallery(rng.standard_normal((70, 512)).astype(np.float32))
    starts = (lambda m, **kw: ex.infer({name: x}, matches=m, **kw), lambda m, **kw: req.start_async({name: x}, matches=m, **kw),
              lambda m, **kw: ex.requests[1].infer({name: x}, matches=m, **kw), lambda m, **kw: ex.start_async(1, {name: x}, matches=m, **kw),
              lambda m, **kw: req.infer({name: x}, kw.get('top_k'), kw.get('detections'), m))

    def refused(match, m, **kw):
        for start in starts:
            with pytest.raises(ValueError, match=match) as e:
                start(m, **kw)
            assert str(e.value).startswith('matches: '), str(e.value)
        for r in ex.requests:
            assert not r._in_flight and not r._asks and not r.runner.answers.blocks and not r.runner.host_inputs.slots and r.runner._pending is None
        assert gal._dev is None and small._dev is None and other._dev is None

    refused('no FP32 Result', other)                                           # no Result qualifies
    refused('no Result named', {'prob': gal})
    refused('has D = 1000', {out_name: other})
    for bad in (5, 'gallery', 0.5, [gal], (gal, 1), GalleryMatch(np.ones((3, 1000)))):
        refused('a Gallery or a GalleryMatch', bad)
        refused('a Gallery or a GalleryMatch', {out_name: bad})
    for k in (0, -1, 65, 71, 1.0, True, None):
        refused('outside 1', GalleryMatch(gal, k))
    refused('outside 1', {out_name: GalleryMatch(small, 4)})
    for ms in (np.nan, np.inf, -np.inf, 'x', True, 1e39):
        refused('min_score', GalleryMatch(gal, 1, ms))
    refused('asked for with top_k as well', gal, top_k=5)
    refused('asked for with top_k as well', {out_name: gal}, top_k={out_name: 5})
    ex.comm = types.SimpleNamespace(world=2, rank=0)
    try:
        refused('sharded', gal)
    finally:
        ex.comm = None
    ports = [r.runner.ienet.outputs[0]['input'][0] for r in ex.requests]
    for port in ports:
        port['precision'] = 'FP16'
    try:
        refused('FP32 Results only', {out_name: gal})
        refused('no FP32 Result', gal)
    finally:
        for port in ports:
            port['precision'] = 'FP32'
    ie_d, net_d, name_d = _net('ssd_mobilenet_v1_coco', 2)                     # a detector's records are no rows of embeddings
    det = ie_d.load_network(net_d, 'GPU', num_requests=1)
    det_out = net_d.outputs[0]['name']
    seven = Gallery(np.ones((2, 7), np.float32))
    for start in (lambda m, **kw: det.infer({name_d: np.zeros((2, 3, 300, 300), np.float32)}, matches=m, **kw),):
        with pytest.raises(ValueError, match=r'matches: Result .* has shape'):
            start({det_out: seven})
        with pytest.raises(ValueError, match='matches: no FP32 Result'):
            start(seven)
        with pytest.raises(ValueError, match=r'matches: Result .* has shape'):      # (no Result can pass both keywords' shape checks)
            start({det_out: seven}, detections=0.5)
    # ... so the refusal of one Result under matches and detections is reached here with gallery.checked's result stubbed: the rule of
    # Answers.checked itself, should the shape rules of the two keywords ever come to overlap
    from pyopenvino_amd import answers as answers_module
    with monkeypatch.context() as patched:
        patched.setattr(answers_module.gallery_rule, 'checked', lambda ienet, matches, sharded: {det_out: GalleryMatch(seven, 1, None)})
        with pytest.raises(ValueError, match='matches: Result {!r} is asked for with detections as well'.format(det_out)):
            det.infer({name_d: np.zeros((2, 3, 300, 300), np.float32)}, detections=0.5, matches={det_out: seven})
        assert not det.answers.blocks and det._pending is None and seven._dev is None
    # the resolved forms, and the four-positional call of Answers.checked as it was
    answers = ex.answers
    assert answers.checked({name: x}, None, None, False) == {} and answers.checked({name: x}, None, None, False, None) == {}
    assert answers.checked({name: x}, 5, None, False) == {out_name: (5,)}
    asks = answers.checked({name: x}, None, None, False, gal)
    assert set(asks) == {out_name} and asks[out_name].match == GalleryMatch(gal, 1, None) and isinstance(asks[out_name], gallery_rule.Ask)
    assert asks[out_name].key(out_name) == (out_name, id(gal), 1)
    assert gallery_rule.Ask(GalleryMatch(gal, 5, 0.25)).key(out_name) == gallery_rule.Ask(GalleryMatch(gal, 5, None)).key(out_name)     # (one scratch block for every threshold)
    assert gallery_rule.checked(net, None, False) == {} and gallery_rule.checked(net, {}, True) == {}
    assert gallery_rule.checked(net, {out_name: GalleryMatch(gal, np.int64(64), 1)}, False) == {out_name: GalleryMatch(gal, 64, 1.0)}
    with pytest.raises(ValueError, match='match_rows'):
        gallery_rule.match_rows(np.zeros((2, 999), np.float32), gal)


def test_a_host_result_gets_the_rule_in_numpy():
    """A plugin set that computes on the host (the oracle's) hands wait() host arrays: the same keyword, the same rule, no device."""
    from pyopenvino_amd import IECore, synth
    ie = IECore(plugin_package='oracle.op_plugins')
    net = ie.read_network(os.path.join(MODELS, 'mnist.xml'))
    net.set_batch(4)
    ex = ie.load_network(net, 'GPU', num_requests=2)
    name, out_name = net.inputs[0]['name'], net.outputs[0]['name']
    x = np.concatenate([synth.uniform_pixels(10 + i, (1, 1, 28, 28)) for i in range(4)], 0)
    full = np.array(ex.infer({name: x})[out_name], copy=True)
    assert full.shape == (4, 10) and full.dtype == np.float32
    rng = np.random.default_rng(23)
    v, ids = rng.standard_normal((40, 10)).astype(np.float32), rng.integers(0, 9, 40).astype(np.int32)
    for metric in ('COSINE', 'DOT'):
        gal = Gallery(v, ids, metric)
        for k, ms in ((1, None), (5, None), (40, 0.1)):
            for got in (ex.infer({name: x}, matches=GalleryMatch(gal, k, ms)), ex.requests[1].infer({name: x}, matches={out_name: GalleryMatch(gal, k, ms)})):
                assert isinstance(got[out_name], Matches)
                _same(got[out_name], _ref(full, v, ids, metric, k, ms), (metric, k, ms))
        _same(ex.infer({name: x}, matches=gal)[out_name], _ref(full, v, ids, metric, 1), 'a Gallery alone')
        assert gal._dev is None
    assert np.array_equal(ex.infer({name: x})[out_name], full)                 # and whole again without the keyword


def test_abi_declares_the_entry():
    import pyopenvino_amd
    from pyopenvino_amd import device
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert ENTRY in device.SIGNATURES and len(device.SIGNATURES[ENTRY][1]) == 14 and ENTRY not in device._NOT_STATUS
    m = re.search(r'\bint\s+' + ENTRY + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S)
    assert m and len(m.group(1).split(',')) == 14
    for text in ('a = fmaf(x[r][i], u[g][i], a)', 's = the binary64 sum of (double)v[i] * (double)v[i] for i ascending', 'r = sqrt(s), correctly rounded binary64',
                 'score = (float)((double)a / r_row)', 'ties to the lower gallery index', 'counts[r] is the length of the leading run of kept slots',
                 '(((i & 1) << 5) | (g & 31))'):
        assert text in header, text                                             # the rule is stated there
    assert re.search(r'#define\s+PVHIP_GALLERY_CHUNK\s+{}\b'.format(C), header) and C % 32 == 0
    assert re.search(r'#define\s+PVHIP_GALLERY_COSINE\s+0\b', header) and re.search(r'#define\s+PVHIP_GALLERY_DOT\s+1\b', header)
    assert gallery_rule.METRICS == {'COSINE': 0, 'DOT': 1}
    assert re.search(r'#define\s+PVHIP_ABI_VERSION\s+19\b', header)
    lib = device.load_library()
    assert hasattr(lib, ENTRY) and lib.pvhip_abi_version() == 19
    for name in ('Gallery', 'GalleryMatch', 'Matches'):
        assert name in pyopenvino_amd.__all__ and getattr(pyopenvino_amd, name) is getattr(gallery_rule, name)
    assert Matches._fields == ('counts', 'indices', 'ids', 'scores') and GalleryMatch._fields == ('gallery', 'k', 'min_score')
    makefile = open(os.path.join(helpers.REPO, 'pyopenvino_amd', 'csrc', 'Makefile')).read()
    assert 'pvhip_gallery.hip' in makefile and 'pvhip_topk_keys.h' in makefile


# ---------------------------------------------------------------------------------------------------------------- GPU
GUARD = 16                                                    # sentinel words in front of and behind each output
SENTINEL = 0x7f7f7f7f


def _device_match(hip, x, gal, k, min_score=None, offset=0):
    """The entry on `x` (n, D) -- `offset`: starting that many floats into a larger device tensor --, the outputs between sentinel words
    that must stay untouched: (Matches, r of every row)."""
    n, D = x.shape
    flat = np.concatenate([np.full(offset, 9e9, np.float32), x.ravel(), np.full(7, 9e9, np.float32)])
    src = hip.DeviceTensor.from_numpy(flat)
    sizes = (n, n * k, n * k, 2 * n)
    outs = [hip.DeviceTensor.empty((size + 2 * GUARD,), np.int32) for size in sizes]
    scratch = hip.DeviceTensor.empty((gallery_rule.scratch_bytes(n, gal.size, k) // 4 + 2 * GUARD,), np.int32)
    for t in outs + [scratch]:
        hip.call('pvhip_memset', ctypes.c_void_p(t.ptr), 0x7f, t.nbytes)
    hip.call(ENTRY, ctypes.c_void_p(src.ptr + 4 * offset), n, D, ctypes.c_void_p(gal.on_device().ptr), gal.size, k, gallery_rule.METRICS[gal.metric],
             int(min_score is not None), float(min_score or 0.0), ctypes.c_void_p(scratch.ptr + 4 * GUARD),
             *(ctypes.c_void_p(t.ptr + 4 * GUARD) for t in outs))
    counts, idx, val, norms = (np.asarray(t) for t in outs)
    for t in (counts, idx, val, norms, np.asarray(scratch)):
        assert (t[:GUARD] == SENTINEL).all() and (t[-GUARD:] == SENTINEL).all(), 'a word outside the output was written'
    assert not (idx[GUARD:-GUARD] == SENTINEL).any() and not (counts[GUARD:-GUARD] == SENTINEL).any(), 'an output was not written'
    indices = idx[GUARD:-GUARD].reshape(n, k).copy()
    ids = np.where(indices >= 0, gal.ids[np.maximum(indices, 0)], -1).astype(np.int32)
    return (Matches(counts[GUARD:-GUARD].copy(), indices, ids, val[GUARD:-GUARD].view(np.float32).reshape(n, k).copy()),
            norms[GUARD:-GUARD].copy().view(np.float64))


def _fillings(rng, n, D, G):
    """[(what, x (n, D), gallery values (G, D))]: every filling of the kernel test for one shape."""
    x, v, _ = _random_case(rng, n, D, G)
    out = [('normal', x, v), ('all equal', np.full((n, D), 0.5, np.float32), np.full((G, D), 0.25, np.float32))]
    xd, vd = x.copy(), v.copy()                               # duplicates across a 32-row block boundary and across a chunk boundary,
    for lo in (31, C - 1, 2 * C - 1):                         # as the best matches of some query row
        if lo + 1 < G:
            vd[lo + 1] = vd[lo]
            xd[lo % n] = vd[lo] * np.float32(3)
    vd[G - 1] = vd[0]
    out.append(('duplicates', xd, vd))
    xs = (x * np.float32(2.0 ** -140)).astype(np.float32)     # subnormal queries: subnormal chain values under either metric
    xs[0, :] = np.float32(2.0 ** -149)
    out.append(('subnormal', xs, v))
    vt = (v * np.float32(2.0 ** -130)).astype(np.float32)     # and a subnormal gallery (left as it is under DOT)
    vt[np.abs(vt).sum(1) == 0, 0] = np.float32(2.0 ** -149)
    out.append(('subnormal gallery', x, vt))
    out.append(('huge', (x * np.float32(2.0 ** 100)).astype(np.float32), (v * np.float32(2.0 ** 27)).astype(np.float32)))     # chains overflow under DOT
    xv = x.copy()                                             # void query rows among live ones
    xv[0 % n, D // 2] = np.nan
    if n > 1:
        xv[n - 1] = 0
    if n > 2:
        xv[n // 2, 0] = -np.inf
    if n > 40:
        xv[33:36] = np.float32(np.nan)
    out.append(('void rows', xv, v))
    return out


SHAPES = [(1, 1, 1, 1), (1, 2, 2, 2), (3, 10, 33, 5), (5, 8, 64, 64), (31, 7, 31, 31), (32, 8, 32, 32), (33, 9, 65, 64),
          (4, 128, C - 1, 5), (4, 128, C, 5), (4, 128, C + 1, 64), (2, 1000, 2 * C + 17, 10), (65, 512, C + 33, 1), (256, 16, 4099, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize('n,D,G,k', SHAPES)
def test_kernel_equals_the_rule(hip, n, D, G, k):
    rng = np.random.default_rng(n * 100003 + D * 67 + G * 7 + k)
    ids = rng.integers(0, max(1, G // 2), G).astype(np.int32)
    for what, x, v in _fillings(rng, n, D, G):
        for metric in ('COSINE', 'DOT'):
            gal = Gallery(v, ids, metric)
            u = gallery_ref.gallery_rows(v, metric)
            assert np.array_equal(_bits(gallery_rule.unpack(gal.packed, G, D)), _bits(u))
            a = gallery_ref.live_chains(x, u)                 # (once for the asks below)
            best = gallery_ref.orders(a, k)
            want = gallery_ref.match(x, u, ids, metric, k, None, a, best)
            got, norms = _device_match(hip, x, gal, k)
            _same(got, want, '{} {} {}'.format((n, D, G, k), what, metric))
            s, r, finite = gallery_rule.norm(x)
            assert np.array_equal(norms[finite].view(np.uint64), r[finite].view(np.uint64)) and np.isnan(norms[~finite]).all(), (what, metric)
            live = want.scores[np.isfinite(want.scores)]
            ms = float(np.median(live)) if len(live) else 0.0
            _same(_device_match(hip, x, gal, k, ms)[0], gallery_ref.match(x, u, ids, metric, k, ms, a, best), '{} {} {} min_score {}'.format((n, D, G, k), what, metric, ms))
            if (n, D, G, k) == (3, 10, 33, 5):                # no row starts on a 16-byte boundary
                for offset in (1, 2, 3):
                    _same(_device_match(hip, x, gal, k, None, offset)[0], want, '{} {} {} offset {}'.format((n, D, G, k), what, metric, offset))


@pytest.mark.gpu
def test_the_norm_is_correctly_rounded(hip):
    """r of the merge launch equals numpy's sqrt bit for bit: squares, the neighbours of squares, the ends of the range, random s."""
    rng = np.random.default_rng(29)
    m = 4000
    x = np.zeros((m, 2), np.float32)
    x[:, 0] = (1 + rng.random(m)) * 2.0 ** rng.integers(-70, 60, m)
    x[:1000, 1] = 0                                           # s = x0^2 exactly: r = |x0|
    x[1000:2000, 1] = x[1000:2000, 0] * np.float32(2.0 ** -26)          # s just above a square: r near a rounding boundary of x0
    x[2000:, 1] = (1 + rng.random(m - 2000)) * 2.0 ** rng.integers(-70, 60, m - 2000)
    x[0] = (3, 4)
    x[1] = (2.0 ** -149, 0)
    x[2] = (3.4028234663852886e38, 3.4028234663852886e38)
    x[3] = (2.0 ** -149, 2.0 ** -149)
    x[4] = (1, 2.0 ** -27)
    gal = Gallery(np.ones((1, 2), np.float32), metric='DOT')
    _, norms = _device_match(hip, x, gal, 1)
    s, r, finite = gallery_rule.norm(x)
    assert finite.all() and r[0] == 5.0 and np.array_equal(r[5:1000], x[5:1000, 0].astype(np.float64))
    assert np.array_equal(norms.view(np.uint64), r.view(np.uint64))
    assert np.array_equal(norms[:64].view(np.uint64), np.array([gallery_ref.norm_row(row)[1] for row in x[:64]], np.float64).view(np.uint64))


@pytest.mark.gpu
def test_entry_rejects_what_it_cannot_do(hip):
    rng = np.random.default_rng(31)
    x, v, ids = _random_case(rng, 4, 64, 100)
    gal = Gallery(v, ids)
    t = hip.DeviceTensor.from_numpy(x)
    o = hip.DeviceTensor.empty((4096,), np.int32)
    sc = hip.DeviceTensor.empty((gallery_rule.scratch_bytes(4, 100, 64) // 4,), np.int32)
    p, packed, scratch = ctypes.c_void_p(t.ptr), ctypes.c_void_p(gal.on_device().ptr), ctypes.c_void_p(sc.ptr)
    counts, indices, scores, norms = (ctypes.c_void_p(o.ptr + 4096 * i) for i in range(4))
    good = [p, 4, 64, packed, 100, 5, 0, 0, 0.0, scratch, counts, indices, scores, norms]
    hip.call(ENTRY, *good)
    good[-1] = None                                           # (the norms are optional)
    hip.call(ENTRY, *good)
    refusals = [(0, None), (3, None), (9, None), (10, None), (11, None), (12, None),                         # nulls
                (0, ctypes.c_void_p(t.ptr + 2)), (3, ctypes.c_void_p(gal.on_device().ptr + 4)), (9, ctypes.c_void_p(sc.ptr + 4)),
                (10, ctypes.c_void_p(o.ptr + 1)), (11, ctypes.c_void_p(o.ptr + 2)), (12, ctypes.c_void_p(o.ptr + 3)), (13, ctypes.c_void_p(o.ptr + 4)),
                (1, 0), (1, -1), (2, 0), (2, 1025), (4, 0), (4, (1 << 24) + 1), (5, 0), (5, 65), (5, 101), (6, 2), (6, -1), (7, 2),
                (1, 1 << 30)]
    for at, bad in refusals:
        args = list(good)
        args[at] = bad
        with pytest.raises(hip.PvhipError):
            hip.call(ENTRY, *args)
    for ms in (np.nan, np.inf):
        args = list(good)
        args[7], args[8] = 1, ms
        with pytest.raises(hip.PvhipError):
            hip.call(ENTRY, *args)
    args = list(good)
    args[4], args[5] = 3, 4                                   # k > G
    with pytest.raises(hip.PvhipError):
        hip.call(ENTRY, *args)
    hip.synchronize()
    _same(_device_match(hip, x, gal, 5)[0], _ref(x, v, ids, 'COSINE', 5), 'after the refusals')       # the device is still usable


def _mnist(batch, requests=1):
    from pyopenvino_amd import IECore
    ie = IECore(plugin_package='pyopenvino_amd.op_plugins')
    net = ie.read_network(os.path.join(MODELS, 'mnist.xml'))
    net.set_batch(batch)
    return ie.load_network(net, 'GPU', num_requests=requests), net.inputs[0]['name'], net.outputs[0]['name']


@pytest.mark.gpu
def test_public_path(hip):
    """mnist at batch 3 and GoogLeNet at batch 8 on a D = 1000 gallery: matches= is the rule on the same request's own full Result; then a
    device-resident input five times with the keyword alternating, replayed from the request's one recording from the third call on."""
    from pyopenvino_amd import synth
    rng = np.random.default_rng(37)
    ex, name, out_name = _mnist(3)
    x = np.concatenate([synth.uniform_pixels(10 + i, (1, 1, 28, 28)) for i in range(3)], 0)
    full = np.array(ex.infer({name: x})[out_name], copy=True)
    v, ids = rng.standard_normal((50, 10)).astype(np.float32), rng.integers(0, 9, 50).astype(np.int32)
    for metric in ('COSINE', 'DOT'):
        gal = Gallery(v, ids, metric)
        _same(ex.infer({name: x}, matches=gal)[out_name], _ref(full, v, ids, metric, 1), 'mnist ' + metric)
        _same(ex.requests[0].infer({name: x}, None, None, {out_name: GalleryMatch(gal, 7, 0.2)})[out_name], _ref(full, v, ids, metric, 7, 0.2), 'mnist k = 7')
    assert np.array_equal(ex.infer({name: x})[out_name], full)

    ex, name, out_name = top_k_tests._googlenet(8, 1234)
    req = ex.requests[0]
    x = synth.uniform_pixels(4242, (8, 3, 224, 224))
    full = np.array(req.infer({name: x})[out_name], copy=True)
    assert full.shape == (8, 1000) and full.dtype == np.float32
    G = 2 * C + 40
    v = (full[rng.integers(0, 8, G)] * (1 + 0.5 * rng.standard_normal((G, 1000)))).astype(np.float32)       # templates around the rows themselves
    ids = rng.integers(0, 100, G).astype(np.int32)
    gal = Gallery(v, ids)
    u = gallery_ref.gallery_rows(v, 'COSINE')
    want = {k: gallery_ref.match(full, u, ids, 'COSINE', k) for k in (1, 5, 64)}
    ms = float(want[5].scores[:, 2].min())
    _same(req.infer({name: x}, matches=GalleryMatch(gal, 5))[out_name], want[5], 'request')
    _same(ex.infer({name: x}, matches=gal)[out_name], want[1], "the network's own infer()")
    _same(ex.infer({name: x}, False, None, None, {out_name: GalleryMatch(gal, 64)})[out_name], want[64], 'k = 64')
    _same(req.infer({name: x}, matches=GalleryMatch(gal, 5, ms))[out_name], gallery_ref.match(full, u, ids, 'COSINE', 5, ms), 'min_score')
    assert np.array_equal(ex.infer({name: x})[out_name], full)               # and whole again without the keyword
    xd = hip.DeviceTensor.from_numpy(x)
    kinds = [GalleryMatch(gal, 5), None, {out_name: gal}, GalleryMatch(gal, 5), None]
    for call, kind in enumerate(kinds):
        req.start_async({name: xd}, matches=kind)
        assert (req._replayed is not None) == (call >= 2), 'call {}'.format(call)
        res = req.wait()[out_name]
        if kind is None:
            helpers.assert_bit_exact(res, full, 'call {}: whole'.format(call))
        else:
            _same(res, want[5 if isinstance(kind, GalleryMatch) else 1], 'call {}'.format(call))
    assert ex._auto_graph['captured'] and ex._graph is not None              # one recording served every kind
    assert sorted(ex.answers.blocks) == [(out_name, id(gal), 1), (out_name, id(gal), 5), (out_name, id(gal), 64)]   # (min_score shares the blocks of its k)
    ex.release_device_state()
    assert not ex.answers.blocks


@pytest.mark.gpu
def test_requests_in_flight_share_one_gallery(hip):
    """Two requests in flight at batch 4 share one Gallery with different k (and a top_k beside them): all started, then all waited for."""
    from pyopenvino_amd import synth
    import topk_ref
    B, R = 4, 2
    ex, name, out_name = top_k_tests._googlenet(B, 1234, requests=R)
    single, _, _ = top_k_tests._googlenet(B, 1234)
    rng = np.random.default_rng(41)
    v, ids = rng.standard_normal((C + 5, 1000)).astype(np.float32), rng.integers(0, 50, C + 5).astype(np.int32)
    gal = Gallery(v, ids, 'DOT')
    u = gallery_ref.gallery_rows(v, 'DOT')
    asked = [[GalleryMatch(gal, 3), GalleryMatch(gal, 9, 0.0)], [GalleryMatch(gal, 9, 0.0), None], [None, GalleryMatch(gal, 3)]]
    for step, row in enumerate(asked):
        xs = [synth.uniform_pixels(5000 + 10 * step + r, (B, 3, 224, 224)) for r in range(R)]
        fulls = [np.array(single.infer({name: x})[out_name], copy=True) for x in xs]
        for r in range(R):
            if row[r] is None:
                ex.start_async(r, {name: xs[r]}, top_k=5)
            else:
                ex.start_async(r, {name: xs[r]}, matches=row[r])
        for r in (reversed(range(R)) if step % 2 else range(R)):
            res = ex.wait(r)[out_name]
            if row[r] is None:
                top_k_tests._same(res, topk_ref.top_k(fulls[r], 5), 'step {} request {}'.format(step, r))
            else:
                _same(res, gallery_ref.match(fulls[r], u, ids, 'DOT', row[r].k, row[r].min_score), 'step {} request {}'.format(step, r))


@pytest.mark.gpu
def test_cascade_rows_behind_count_are_void(hip):
    """GoogLeNet at batch 8 fed DetectedRois(frames, a records array) with fewer survivors than rows, matches=: all eight rows equal the
    rule on the full Result of the same feed bit for bit -- the rows behind `count` are NaN rows: count 0, every slot void."""
    from pyopenvino_amd import DetectedRois
    rng = np.random.default_rng(501)
    n, m, hw, kind = 8, 2, (480, 640), 'U8-NHWC'
    frames = roi_tests._frames(rng, kind, m, hw)
    rec = det_tests._random_records(rng, m, 40, long=True)
    scores = np.sort(rec[:, 2][np.isfinite(rec[:, 2])])[::-1]
    want = None
    for conf in scores[2:40]:                                 # the highest threshold that leaves 3 .. 7 survivors
        want = det_tests.detected_rois(rec, n, m, hw, min_confidence=float(conf))
        if 3 <= want.count < n:
            break
    assert want is not None and 3 <= want.count == want.selected < n, (want.count, want.selected)
    conf = float(conf)
    ex, name, out_name = det_tests._classifier(kind, n, top_k_tests._blob(11))
    req = ex.requests[0]
    full = np.array(req.infer({name: DetectedRois(frames, rec, min_confidence=conf)})[out_name], copy=True)
    assert np.isfinite(full[:want.count]).all() and np.isnan(full[want.count:]).all()
    v, ids = rng.standard_normal((70, 1000)).astype(np.float32), rng.integers(0, 9, 70).astype(np.int32)
    got = req.infer({name: DetectedRois(frames, rec, min_confidence=conf)}, matches=GalleryMatch(Gallery(v, ids), 3))[out_name]
    _same(got, _ref(full, v, ids, 'COSINE', 3), 'cascade')
    assert (got.counts[:want.count] == 3).all() and (got.counts[want.count:] == 0).all()
    assert (got.indices[want.count:] == -1).all() and (got.ids[want.count:] == -1).all() and (_bits(got.scores[want.count:]) == 0x7FC00000).all()
    det_tests._same(req.detected_rois(name), want, 'with matches')
