"""The local maxima of heatmaps made on the device (``infer(..., maxima=...)``, pvhip_heatmap_maxima_f32): counts, channels, positions,
scores and points of an (n, K, H, W) Result by the rule of tests/maxima_ref.py, bit for bit, one entry call behind the pass and one
read-back of 4 n + 20 n R bytes.  The first tests need no GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import helpers
import maxima_ref
import test_keypoints as keypoints_tests
import test_top_k as top_k_tests

ENTRY, FORM = 'pvhip_heatmap_maxima_f32', 'pvhip_heatmap_maxima_form'
NAN, INF = np.float32(np.nan), np.float32(np.inf)
QUIET = 0x7FC00000
FORM_NONE, FORM_WAVE, FORM_BLOCK = 0, 1, 2              # PVHIP_MAXIMA_FORM_*
WAVE_PLANE = 1024                                       # kWavePlane of pvhip_maxima.hip: the last H * W of the one-wave-per-plane form
FORM_STEPS = [WAVE_PLANE]                               # the H * W behind which the form query changes its answer
KEY_CAPACITY = 2048                                     # Sizes<256>::kKeys of pvhip_maxima.hip: the keys a workgroup's buffer holds at most
WAVE_KEY_CAPACITY = 512                                 # Sizes<64>::kKeys: a wave's
WAVE_GRID, BLOCK_GRID = 8192, 8192                      # the most workgroups launch 1 starts in either form: beyond, a team takes several planes
_mnist_head, _pixels, _bits = keypoints_tests._mnist_head, keypoints_tests._pixels, keypoints_tests._bits
det_tests, roi_tests = top_k_tests.det_tests, top_k_tests.roi_tests
SHAPES = [(1, 1, 1, 2), (2, 3, 1, 7), (3, 5, 7, 9), (2, 4, 6, 2), (1, 2, 33, 31), (2, 17, 64, 48)]
CAPS = {(1, 1, 1, 2): (1, 1), (2, 3, 1, 7): (1, 2), (3, 5, 7, 9): (4, 7), (2, 4, 6, 2): (1, 3), (1, 2, 33, 31): (16, 20), (2, 17, 64, 48): (32, 100)}
UNCAPPED = (256, 1024)


def _same(got, want, what=''):
    """`got` (a Maxima of the product) equals `want` (the rule's): counts, channels and positions exact, scores and points bit for bit."""
    assert [a.dtype for a in got] == [np.int32, np.int32, np.int32, np.float32, np.float32], what
    assert [a.shape for a in got] == [a.shape for a in want], (what, [a.shape for a in got], [a.shape for a in want])
    assert np.array_equal(got.counts, want.counts), '{}: counts {} want {}'.format(what, got.counts.tolist(), want.counts.tolist())
    for field in ('channels', 'positions'):
        bad = np.argwhere(getattr(got, field) != getattr(want, field))
        assert not len(bad), '{}: slot {}: {} {} want {}'.format(what, bad[0].tolist(), field, getattr(got, field)[tuple(bad[0])], getattr(want, field)[tuple(bad[0])])
    bad = np.argwhere(_bits(got.scores) != _bits(want.scores))
    assert not len(bad), '{}: slot {}: score bits {:#x} want {:#x}'.format(what, bad[0].tolist(), _bits(got.scores)[tuple(bad[0])], _bits(want.scores)[tuple(bad[0])])
    bad = np.argwhere((_bits(got.points) != _bits(want.points)).any(axis=2))
    assert not len(bad), '{}: slot {}: point {} want {}'.format(what, bad[0].tolist(), got.points[tuple(bad[0])].tolist(), want.points[tuple(bad[0])].tolist())


def _filler_behind_the_counts(got):
    R = got.channels.shape[1]
    behind = np.arange(R)[None, :] >= got.counts[:, None]
    assert (got.channels[behind] == -1).all() and (got.positions[behind] == -1).all() and (_bits(got.scores)[behind] == QUIET).all()
    assert (_bits(got.points)[behind] == QUIET).all() and (got.channels[~behind] >= 0).all() and not np.isnan(got.points[~behind]).any()


def _lattice(shape, ascending):
    """A maximum at every even (y, x), ceil(H / 2) * ceil(W / 2) a plane, their values ascending or descending in raster order."""
    n, K, H, W = shape
    x = np.zeros(shape, np.float32)
    ys, xs = np.meshgrid(np.arange(0, H, 2), np.arange(0, W, 2), indexing='ij')
    ramp = (1 + np.arange(ys.size, dtype=np.float32)).reshape(ys.shape)
    x[:, :, ::2, ::2] = ramp if ascending else ramp[::-1, ::-1]
    return x


def _fillings(rng, shape):
    """[(what, (n, K, H, W) float32)]: every filling of the rule's tests for one shape."""
    n, K, H, W = shape
    nans = rng.standard_normal(shape).astype(np.float32)
    many = max(1, nans.size // 40)
    at = rng.choice(nans.size, size=many, replace=False)
    kinds = np.array(top_k_tests.SPECIALS[:3], np.uint32)      # quiet, negative, signalling
    nans.reshape(-1).view(np.uint32)[at] = kinds[np.arange(many) % 3] | (rng.integers(0, 1 << 16, many).astype(np.uint32) << np.uint32(3))
    row = rng.standard_normal(shape).astype(np.float32)
    row.view(np.uint32)[n // 2] = QUIET                        # one all-NaN row (n == 1: the only one)
    return [('normal', rng.standard_normal(shape).astype(np.float32)), ('four levels', (rng.integers(0, 4, shape) / 4).astype(np.float32)),
            ('signed zeros', rng.choice(np.array([0.0, -0.0, -1.0, -2.0], np.float32), shape)), ('NaNs', nans), ('NaN row', row),
            ('all equal', np.full(shape, 0.25, np.float32)), ('lattice ascending', _lattice(shape, True)), ('lattice descending', _lattice(shape, False))]


def _cases(shape):
    """[(what, x, (min_score, M, R, refine, space), the rule's answer)] of a shape: every filling with the caps off, with caps that bite
    and with a min_score, the median of the scores that pass without one.  Made once per shape and handed out unchanged."""
    if shape not in _cases.made:
        rng = np.random.default_rng(sum(d * 31 ** i for i, d in enumerate(shape)))
        made, bites = [], [False, False]
        for what, x in _fillings(rng, shape):
            found = maxima_ref.found_in(x)
            passing = np.array([x[r, c].reshape(-1)[p] for r in range(shape[0]) for c in range(shape[1]) for p in found[r][c]], np.float32)
            cut = float(np.median(passing)) if passing.size else 0.0
            M, R = CAPS[shape]
            for screen in ((None,) + UNCAPPED + ('QUARTER', 'NORMALISED'), (None, M, R, 'NONE', 'HEATMAP'), (cut, M, None, 'QUARTER', 'HEATMAP'),
                           (cut,) + UNCAPPED + ('NONE', 'NORMALISED')):
                want = maxima_ref.maxima(x, None if screen[0] is None else float(np.float32(screen[0])), *screen[1:], found=found)
                made.append(('{} {} {}'.format(shape, what, screen), x, screen, want))
                if screen[0] is None and screen[1] == M:        # conditions on the inputs: the caps have something to cut
                    bites[0] |= any(len(plane) > M for row in found for plane in row)
                    bites[1] |= any(sum(min(len(plane), M) for plane in row) > R for row in found)
            if what in ('normal', 'NaNs', 'lattice ascending', 'lattice descending') and passing.size > 1:      # and the threshold keeps some and drops some
                assert 0 < (passing >= np.float32(cut)).sum() < passing.size, (shape, what)
        assert shape[2] * shape[3] < 16 or all(bites), (shape, bites)
        _cases.made[shape] = made
    return _cases.made[shape]


_cases.made = {}


def _screen(screen):
    from pyopenvino_amd import MaximaScreen
    return MaximaScreen(*screen)


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
def test_the_rule_on_hand_written_planes():
    from pyopenvino_amd import Maxima, MaximaScreen, maxima

    def both(x, **screen):
        x = np.asarray(x, np.float32)
        x = x.reshape((1,) * (4 - x.ndim) + x.shape)
        screen = MaximaScreen(**{'refine': 'NONE', 'space': 'HEATMAP', **screen})
        want = maxima_ref.maxima(x, *screen)
        got = maxima.peaks_of(x, screen)                        # the product's own numpy form (host Results) is the same rule
        assert isinstance(got, Maxima)
        _same(got, want, str(x.tolist()))
        _filler_behind_the_counts(got)
        return want

    def found(x, **screen):
        want = both(x, **screen)
        return [(int(c), int(p)) for c, p in zip(want.channels[0, :want.counts[0]], want.positions[0, :want.counts[0]])]

    assert found(np.full((4, 5), 0.5)) == [(0, 0)]                                  # a flat plane: one maximum, at 0
    z = np.full((4, 5), 0.5, np.float32)
    z[1, 2] = NAN                                                                   # the NaN is not reported and suppresses its eight neighbours;
    assert found(z) == [(0, 0)]                                                     # every other pixel has an equal neighbour before it
    z[1, 2], z[1, 1] = 0.5, NAN
    assert found(z) == []                                                           # (index 0 is beside this one)
    z = np.zeros((4, 5), np.float32)
    z[1, 1:4] = 1
    z[2, 0] = 1
    assert found(z) == [(0, 1 * 5 + 1)]                                             # a plateau: only the pixel with no plateau neighbour before it
    assert found([[0.0, -0.0]]) == [(0, 0)] and found([[-0.0, 0.0]]) == [(0, 0)]    # zeros of either sign tie: the lower index
    assert found([[-1, -0.0, 0.0, -1]]) == [(0, 1)]
    z = np.zeros((5, 7), np.float32)
    for value, (y, x) in enumerate(((0, 0), (0, 6), (4, 0), (4, 6), (0, 3), (4, 3), (2, 0), (2, 6)), 1):     # the corners, then the edges
        z[y, x] = value
    assert found(z) == [(0, 2 * 7 + 6), (0, 2 * 7 + 0), (0, 4 * 7 + 3), (0, 3), (0, 4 * 7 + 6), (0, 4 * 7), (0, 6), (0, 0)]
    # min_score equal to a maximum's value keeps it; one ulp above drops it
    z = np.zeros((3, 7), np.float32)
    z[1, 1], z[1, 5] = 0.7, 0.9
    top = np.float32(0.7)
    assert found(z, min_score=float(top)) == [(0, 12), (0, 8)] and found(z, min_score=float(np.nextafter(top, INF))) == [(0, 12)]
    assert found(z, min_score=0.7) == [(0, 12), (0, 8)] and found(z, min_score=1.0) == [] and found(z, max_per_plane=1) == [(0, 12)]
    # two planes with equal values order by channel, then by position
    z = np.zeros((1, 2, 3, 7), np.float32)
    z[0, 1, 1, 1] = z[0, 0, 1, 5] = z[0, 0, 1, 1] = 2
    assert found(z) == [(0, 8), (0, 12), (1, 8)] and found(z, max_per_row=2) == [(0, 8), (0, 12)]
    assert found(z, max_per_plane=1, max_per_row=5) == [(0, 8), (1, 8)]
    assert found([[1.0, 2.0]]) == [(0, 1)] and found([[3.0], [2.0]]) == [(0, 0)]    # H == 1, W == 2 and W == 1
    assert found([[NAN, 1.0]]) == [] and found([[INF, 0, -INF]]) == [(0, 0)] and found([[-INF, -INF]]) == [(0, 0)]
    # the quarter-pixel rule at an answered position, both spaces
    z = np.zeros((3, 4), np.float32)
    z[1, 1], z[1, 2], z[0, 1] = 5, 1, 2
    want = both(z, refine='QUARTER')
    assert want.points[0, 0].tolist() == [1.25, 0.75]
    want = both(z, refine='QUARTER', space='NORMALISED')
    assert want.points[0, 0].tolist() == [float(np.float32(1.75 / 4)), float(np.float32(1.25 / 3))]
    # anything but float32 (n, K, H, W) with 2 <= H * W is refused
    for bad in (np.zeros((1, 1, 1, 1), np.float32), np.zeros((2, 3, 4), np.float32), np.zeros((1, 1, 2, 2), np.float64), np.zeros((1, 0, 2, 2), np.float32)):
        with pytest.raises(ValueError, match='peaks_of'):
            maxima.peaks_of(bad)
    for bad in ('x', None, False, MaximaScreen(np.nan), MaximaScreen(max_per_plane=0), MaximaScreen(max_per_row=1025), MaximaScreen(refine='HALF')):
        with pytest.raises(ValueError, match='peaks_of'):
            maxima.peaks_of(np.zeros((1, 1, 2, 2), np.float32), bad)


@pytest.mark.parametrize('shape', SHAPES)
def test_peaks_of_agrees_with_the_loops(shape):
    from pyopenvino_amd import maxima
    for what, x, screen, want in _cases(shape):
        got = maxima.peaks_of(x, _screen(screen))
        _same(got, want, what)
        _filler_behind_the_counts(got)
    x = np.random.default_rng(3).standard_normal((2, 3, 8, 5, 7)).astype(np.float32)[:, :, :, :, 2]      # not contiguous: the same answer
    _same(maxima.peaks_of(x), maxima_ref.maxima(np.ascontiguousarray(x)), 'strided')


def test_argument_rules(tmp_path, monkeypatch):
    """Every refusal is a ValueError('maxima: ...') raised before anything is staged or launched: this test runs where there is no device."""
    from pyopenvino_amd import Gallery, GalleryMatch, MaximaScreen, answers as answers_module, detections as detections_rule, maxima as rule
    n = 4
    ex, net, name, out_name = _mnist_head(tmp_path, n, requests=2)
    x = np.zeros((n, 1, 28, 28), np.float32)
    req = ex.requests[0]
    others = ('top_k', 'detections', 'matches', 'keypoints', 'segments')
    starts = (lambda s, **kw: ex.infer({name: x}, maxima=s, **kw), lambda s, **kw: req.start_async({name: x}, maxima=s, **kw),
              lambda s, **kw: ex.requests[1].infer({name: x}, maxima=s, **kw), lambda s, **kw: ex.start_async(1, {name: x}, maxima=s, **kw),
              lambda s, **kw: req.infer({name: x}, *(kw.get(k) for k in others), s),
              lambda s, **kw: req.start_async({name: x}, *(kw.get(k) for k in others), s),
              lambda s, **kw: ex.infer({name: x}, False, *(kw.get(k) for k in others), s),
              lambda s, **kw: ex.start_async(0, {name: x}, *(kw.get(k) for k in others), s))       # the keyword stands last

    def refused(match, s, network=ex, starts=starts, **kw):
        for start in starts:
            with pytest.raises(ValueError, match=match) as e:
                start(s, **kw)
            assert str(e.value).startswith('maxima: '), str(e.value)
        for r in network.requests:
            assert not r._in_flight and not r._asks and not r.runner.answers.blocks and not r.runner.host_inputs.slots and r.runner._pending is None

    refused('no Result named', {'heatmaps/nope': True})
    refused('no Result named', {out_name: True, 'nope': 0.5})
    for bad in ('QUARTER', [0.5], (0.5,), False, np.bool_(True), b'1', 1j, MaximaScreen):
        refused('a MaximaScreen, a min_score or True', bad)
        refused('a MaximaScreen, a min_score or True', {out_name: bad})
    refused('a MaximaScreen, a min_score or True', {out_name: None})
    for bad in ('HALF', 'quarter', None, 1):
        refused('refine', MaximaScreen(refine=bad))
        refused('refine', {out_name: MaximaScreen(0.5, refine=bad)})
    for bad in ('PIXELS', 'normalised', None, 0):
        refused('space', MaximaScreen(space=bad))
    for bad in (np.nan, np.inf, -np.inf, 'x', True, 1e39, -1e39, [1.0]):
        refused('min_score', MaximaScreen(bad))
        refused('min_score', {out_name: MaximaScreen(min_score=bad)})
    for bad in (np.nan, np.inf, 1e39, np.float64(-1e300)):
        refused('min_score', bad)
    for bad in (0, -1, 257, 1 << 40, 2.0, '4', None, True, np.bool_(True), np.float32(8)):
        refused('max_per_plane is an int in 1 .. 256', MaximaScreen(max_per_plane=bad))
        refused('max_per_plane is an int in 1 .. 256', {out_name: MaximaScreen(0.5, bad)})
    for bad in (0, -1, 1025, 1 << 40, 2.0, '4', True, np.bool_(False)):
        refused('max_per_row is an int in 1 .. 1024', MaximaScreen(max_per_row=bad))
        refused('max_per_row is an int in 1 .. 1024', {out_name: MaximaScreen(0.5, 4, bad)})
    ex.comm = types.SimpleNamespace(world=2, rank=0)
    try:
        refused('sharded', True)
        refused('sharded', {out_name: 0.5})
    finally:
        ex.comm = None
    ports = [r.runner.ienet.outputs[0]['input'][0] for r in ex.requests]       # (every request has its own copy of the graph)
    for port in ports:
        port['precision'] = 'FP16'
    try:
        refused('FP32 Results only', {out_name: True})
        refused('no FP32 Result', True)
    finally:
        for port in ports:
            port['precision'] = 'FP32'
    declared = [port['dims'] for port in ports]
    for dims in ((n, 32, 676), (n, 32, 26, 26, 1), (n, 32, 1, 1), (2, 32, 26, 26), (n, 32, 4097, 4096), (n, 129, 4096, 4096), (n, 1 << 30, 1, 2)):
        for port in ports:                                                     # another rank, one element, another batch, beyond 2^24, K * H * W beyond 2^31 - 1
            port['dims'] = dims
        try:
            refused('has shape .*: not \\(n = 4, K, H, W\\) with 2 <= H \\* W <= 2\\^24 and K \\* H \\* W <= 2\\^31 - 1', {out_name: True})
            refused('no FP32 Result', 0.5)
        finally:
            for port, dims in zip(ports, declared):
                port['dims'] = dims
    for port in ports:                                                         # n * K * M: 4 * 2^21 * 256 = 2^31
        port['dims'] = (n, 1 << 21, 2, 2)
    try:
        refused('n \\* K \\* max_per_plane', MaximaScreen(max_per_plane=256))
        refused('n \\* K \\* max_per_plane', {out_name: MaximaScreen(max_per_plane=256)})
        assert rule.checked(ex.requests[0].runner.ienet, MaximaScreen(max_per_plane=255), False)[out_name].max_per_row == 1024
    finally:
        for port, dims in zip(ports, declared):
            port['dims'] = dims
    # a classifier has no heatmaps, a detector's (1, 1, R, 7) records are none for the unnamed forms
    ie_c, net_c, name_c = roi_tests._net('mnist', n)
    cls = ie_c.load_network(net_c, 'GPU', num_requests=1)
    xc = np.zeros((n, 1, 28, 28), np.float32)
    cls_starts = (lambda s, **kw: cls.infer({name_c: xc}, maxima=s), lambda s, **kw: cls.requests[0].start_async({name_c: xc}, maxima=s))
    refused('no FP32 Result', True, cls, cls_starts)
    refused('has shape', {net_c.outputs[0]['name']: True}, cls, cls_starts)
    ie_d, net_d, name_d = roi_tests._net('ssd_mobilenet_v1_coco', 1)
    det = ie_d.load_network(net_d, 'GPU', num_requests=1)
    dims = tuple(net_d.outputs[0]['input'][0]['dims'])
    assert dims[:2] == (1, 1) and dims[3] == 7
    xd = np.zeros((1, 3, 300, 300), np.float32)
    refused('no FP32 Result', True, det, (lambda s, **kw: det.infer({name_d: xd}, maxima=s), lambda s, **kw: det.requests[0].start_async({name_d: xd}, maxima=s)))
    # one Result under two keywords: the later keyword speaks and names the earlier.  keypoints and segments fit the same Results; no
    # Result passes the shape rules of the other three, so their checks are stubbed to reach the rule of Answers.checked itself
    clash = 'Result {!r} is asked for with {} as well'
    for keyword in ('keypoints', 'segments'):
        for value in (True, 0.5, {out_name: True}):
            refused(clash.format(out_name, keyword), True, **{keyword: value})
            refused(clash.format(out_name, keyword), {out_name: 0.5}, **{keyword: value})
    gal = Gallery(np.ones((3, 7), np.float32))
    for keyword, module, stub, value in (('top_k', answers_module.top_k_rule, lambda ienet, top_k, sharded: {out_name: 1}, 1),
                                         ('detections', answers_module.detections_rule, lambda ienet, d, sharded: {out_name: detections_rule.DetectionScreen()}, 0.5),
                                         ('matches', answers_module.gallery_rule, lambda ienet, matches, sharded: {out_name: GalleryMatch(gal, 1, None)}, gal)):
        with monkeypatch.context() as patched:
            patched.setattr(module, 'checked', stub)
            refused(clash.format(out_name, keyword), True, **{keyword: value})
            refused(clash.format(out_name, keyword), {out_name: 0.5}, **{keyword: value})
    assert gal._dev is None
    # the resolved forms: max_per_row is filled in from the Result's K
    default = MaximaScreen(None, 32, 1024, 'QUARTER', 'NORMALISED')
    assert MaximaScreen() == (None, 32, None, 'QUARTER', 'NORMALISED')
    assert rule.checked(net, None, False) == {} and rule.checked(net, {}, True) == {} and rule.checked(net, True, False) == {out_name: default}
    assert rule.checked(net, 0.5, False) == rule.checked(net, {out_name: np.float32(0.5)}, False) == {out_name: default._replace(min_score=0.5)}
    assert rule.checked(net, 1, False) == {out_name: default._replace(min_score=1.0)} and isinstance(rule.checked(net, 1, False)[out_name].min_score, float)
    assert rule.checked(net, 0.7, False)[out_name].min_score == float(np.float32(0.7))                   # the threshold is the float32
    assert rule.checked(net, MaximaScreen(max_per_plane=np.int64(3)), False) == {out_name: default._replace(max_per_plane=3, max_per_row=96)}
    assert rule.checked(net, {out_name: MaximaScreen(np.int64(-2), 1, 7, 'NONE', 'HEATMAP')}, False) == {out_name: MaximaScreen(-2.0, 1, 7, 'NONE', 'HEATMAP')}
    assert rule.planes_of((4, 17, 64, 48)) == (4, 17, 64, 48) and rule.planes_of((4, 17, 64, 48), 2) is None and rule.planes_of((4, 17, 1, 1)) is None
    assert rule.planes_of((1, 127, 4096, 4096)) is not None and rule.planes_of((1, 128, 4096, 4096)) is None


def test_answers_checked_takes_the_new_argument_last(tmp_path):
    from pyopenvino_amd import MaximaScreen, keypoints, maxima as rule, segments
    n = 4
    ex, net, name, out_name = _mnist_head(tmp_path, n)
    x = np.zeros((n, 1, 28, 28), np.float32)
    answers = ex.answers
    assert answers.checked({name: x}, None, None, False) == {} and answers.checked({name: x}, None, None, False, None, None, None) == {}
    assert answers.checked({name: x}, None, None, False, None, None, None, None) == {} and answers.checked({name: x}, None, None, False, maxima=None) == {}
    asks = answers.checked({name: x}, None, None, False, None, None, None, 0.5)
    screen = MaximaScreen(0.5, 32, 1024, 'QUARTER', 'NORMALISED')
    assert set(asks) == {out_name} and isinstance(asks[out_name], rule.Ask) and asks[out_name].KEYWORD == 'maxima'
    assert asks[out_name] == (screen,) and asks[out_name].screen == screen      # an ask equals the plain tuple of its fields
    assert asks == answers.checked({name: x}, None, None, False, maxima={out_name: MaximaScreen(0.5)})
    assert asks[out_name].key(out_name) == (out_name, 32, 1024, 'QUARTER', 'NORMALISED') == rule.Ask(screen._replace(min_score=None)).key(out_name)
    assert rule.Ask(screen._replace(max_per_row=100)).key(out_name) != asks[out_name].key(out_name)
    assert asks[out_name].launch_with() == (0.5,) and asks[out_name].bound({name: x}, {}) is asks[out_name]
    # the six- and seven-argument calls answer as before
    kept = answers.checked({name: x}, None, None, False, None, True)
    assert set(kept) == {out_name} and isinstance(kept[out_name], keypoints.Ask)
    kept = answers.checked({name: x}, None, None, False, None, None, True)
    assert set(kept) == {out_name} and isinstance(kept[out_name], segments.Ask)
    assert not answers.blocks and not ex.host_inputs.slots and ex._pending is None


def _head_found(full):
    """found_in of the mnist head's Result, and a min_score that keeps some of its maxima and drops others."""
    found = maxima_ref.found_in(full)
    passing = np.array([full[r, c].reshape(-1)[p] for r in range(full.shape[0]) for c in range(full.shape[1]) for p in found[r][c]], np.float32)
    return found, float(np.median(passing))


def _head_want(full, found, given):
    from pyopenvino_amd import MaximaScreen
    screen = given if isinstance(given, MaximaScreen) else MaximaScreen(None if given is True else given)
    return maxima_ref.maxima(full, None if screen.min_score is None else float(np.float32(screen.min_score)), *screen[1:], found=found)


def test_a_host_result_gets_the_rule_in_numpy(tmp_path):
    """A plugin set that computes on the host (the oracle's) hands wait() host arrays: the same keyword, the same rule, no device."""
    from pyopenvino_amd import Maxima, MaximaScreen
    n = 3
    ex, net, name, out_name = _mnist_head(tmp_path, n, requests=2, package='oracle.op_plugins')
    x = _pixels(10, n)
    full = np.array(ex.infer({name: x})[out_name], copy=True)
    assert full.shape == (n, 32, 26, 26) and full.dtype == np.float32 and np.isfinite(full).all()
    found, cut = _head_found(full)
    for given in (True, cut, MaximaScreen(cut, 4, 50, 'NONE', 'HEATMAP'), MaximaScreen(None, 256, None, 'QUARTER', 'HEATMAP')):
        want = _head_want(full, found, given)
        for got in (ex.infer({name: x}, maxima=given), ex.requests[1].infer({name: x}, maxima={out_name: given})):
            assert set(got) == {out_name} and isinstance(got[out_name], Maxima)
            _same(got[out_name], want, repr(given))
    assert 0 < _head_want(full, found, cut).counts.sum() < _head_want(full, found, True).counts.sum()
    assert np.array_equal(ex.infer({name: x})[out_name], full)           # and whole again without the keyword
    with pytest.raises(ValueError, match='maxima: min_score'):
        ex.infer({name: x}, maxima=MaximaScreen(np.inf))


def test_abi_declares_the_entries():
    import pyopenvino_amd
    from pyopenvino_amd import device, keypoints, maxima
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for entry, count in ((ENTRY, 17), (FORM, 2)):
        assert entry in device.SIGNATURES and len(device.SIGNATURES[entry][1]) == count
        m = re.search(r'\bint\s+' + entry + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S)
        assert m and len(m.group(1).split(',')) == count, entry
    assert ENTRY not in device._NOT_STATUS and FORM in device._NOT_STATUS
    joined = re.sub(r'\s*\n \*\s+', ' ', header)                               # the rule is stated there (its lines joined)
    for phrase in ('NaN of any sign or payload first, then descending with +0.0 == -0.0, ties to the lower index',
                   'is a maximum iff v[p] is not NaN and key(p) is larger than the key of each of its at most eight neighbours that lie inside the plane',
                   'a flat plane has one maximum, at index 0', 'A NaN is never a maximum and suppresses all its neighbours',
                   'the maximum passes iff has_min == 0 or v[p] >= min_score', 'Equality keeps',
                   'the first max_per_plane passing maxima are kept, in descending key order',
                   'ties to the lower channel, then to the lower position: the key of (value, c * h * w + p)',
                   'rules 3 and 4 of pvhip_heatmap_peaks_f32 above, word for word',
                   'the slots behind them are (-1, -1, quiet NaN, quiet NaN, quiet NaN)'):
        assert phrase in joined, phrase
    for phrase in ('ties to the lower index', 'a flat plane has one maximum, at index 0', 'A NaN is never a maximum and suppresses all its neighbours',
                   'Equality keeps', 'in descending key order', 'ties to the lower channel, then to the lower position', 'only on exact ties',
                   '(-1, -1, quiet NaN, quiet NaN, quiet NaN)'):
        assert phrase in re.sub(r'\s*\n\s+', ' ', maxima.__doc__) and phrase in re.sub(r'\s*\n\s+', ' ', maxima_ref.__doc__), phrase
    assert '(n, R, 2)' in re.sub(r'\s*\n\s+', ' ', keypoints.to_frame.__doc__)
    for define, value in (('PVHIP_MAXIMA_MAX_PER_PLANE', maxima.MAX_PER_PLANE), ('PVHIP_MAXIMA_MAX_PER_ROW', maxima.MAX_PER_ROW),
                          ('PVHIP_MAXIMA_FORM_NONE', FORM_NONE), ('PVHIP_MAXIMA_FORM_WAVE', FORM_WAVE), ('PVHIP_MAXIMA_FORM_BLOCK', FORM_BLOCK)):
        assert re.search(r'#define\s+{}\s+{}\b'.format(define, value), header), define
    assert re.search(r'#define\s+PVHIP_MAXIMA_MAX_PLANE\s+\(1 << 24\)', header)
    assert (maxima.MAX_PLANE, maxima.MAX_PER_PLANE, maxima.MAX_PER_ROW, maxima.MAX_INDEX) == (1 << 24, 256, 1024, 2 ** 31 - 1)
    assert maxima.REFINES is keypoints.REFINES and maxima.SPACES is keypoints.SPACES            # rule 5 is keypoints' own
    assert re.search(r'#define\s+PVHIP_ABI_VERSION\s+19\b', header)
    lib = device.load_library()
    assert hasattr(lib, ENTRY) and hasattr(lib, FORM) and lib.pvhip_abi_version() == 19
    assert pyopenvino_amd.Maxima is maxima.Maxima and pyopenvino_amd.MaximaScreen is maxima.MaximaScreen
    assert 'Maxima' in pyopenvino_amd.__all__ and 'MaximaScreen' in pyopenvino_amd.__all__
    assert pyopenvino_amd.Maxima._fields == ('counts', 'channels', 'positions', 'scores', 'points')
    assert pyopenvino_amd.MaximaScreen._fields == ('min_score', 'max_per_plane', 'max_per_row', 'refine', 'space')
    assert tuple(pyopenvino_amd.MaximaScreen()) == (None, 32, None, 'QUARTER', 'NORMALISED')


def _form_steps():
    """Every H * W after which pvhip_heatmap_maxima_form changes its answer, for planes of one row (the form depends on H * W alone)."""
    from pyopenvino_amd import device
    forms = [device.call(FORM, 1, s) for s in range(2, 1 << 14)]
    return [s for s, (a, b) in zip(range(2, 1 << 14), zip(forms, forms[1:])) if a != b]


def test_the_form_query():
    """It needs no device, answers NONE for what the entry refuses, and changes where the kernel test stands and nowhere else."""
    from pyopenvino_amd import device
    form = lambda h, w: device.call(FORM, h, w)
    assert [form(1, 1), form(0, 2), form(2, -1), form(4097, 4096), form(1 << 16, 1 << 16), form(1, (1 << 24) + 1)] == [FORM_NONE] * 6
    assert _form_steps() == FORM_STEPS
    for h, w in ((1, 2), (2, 1), (32, 32), (1, 1024), (1024, 1), (26, 26)):
        assert form(h, w) == FORM_WAVE
    for h, w in ((25, 41), (1, 1025), (1025, 1), (46, 46), (128, 128), (4096, 4096), (1, 1 << 24), (1 << 24, 1)):
        assert form(h, w) == FORM_BLOCK


# ---------------------------------------------------------------------------------------------------------------- GPU
GUARD, SENTINEL = top_k_tests.GUARD, top_k_tests.SENTINEL


def _device_maxima(hip, x, screen, offset=0):
    """The entry on `x` (n, K, H, W) -- `offset`: starting that many elements into a larger device tensor --, the outputs between
    sentinel words that must stay untouched, every slot written."""
    from pyopenvino_amd import maxima
    n, K, H, W = x.shape
    min_score, M, R, refine, space = maxima.for_planes(maxima.resolved(_screen(screen)), n, K)
    if offset:
        src = hip.DeviceTensor.from_numpy(np.concatenate([np.full(offset, 9e9, np.float32), x.ravel(), np.full(7, 9e9, np.float32)]))
    else:
        src = hip.DeviceTensor.from_numpy(x)
    scratch = hip.DeviceTensor.empty((n * K * M + 2 * GUARD,), np.uint64)
    outs = [hip.DeviceTensor.empty((words + 2 * GUARD,), np.int32) for words in (n, n * R, n * R, n * R, 2 * n * R)]
    for t in outs + [scratch]:
        hip.call('pvhip_memset', ctypes.c_void_p(t.ptr), 0x7f, t.nbytes)
    hip.call(ENTRY, ctypes.c_void_p(src.ptr + 4 * offset), n, K, H, W, M, R, maxima.REFINES[refine], maxima.SPACES[space], int(min_score is not None),
             float(min_score or 0.0), ctypes.c_void_p(scratch.ptr + 8 * GUARD), *(ctypes.c_void_p(t.ptr + 4 * GUARD) for t in outs))
    keys = np.asarray(scratch)
    assert (keys[:GUARD] == 0x7f7f7f7f7f7f7f7f).all() and (keys[-GUARD:] == 0x7f7f7f7f7f7f7f7f).all(), 'a word outside the scratch was written'
    cnt, cha, pos, sco, pts = (np.asarray(t) for t in outs)
    for t in (cnt, cha, pos, sco, pts):
        assert (t[:GUARD] == SENTINEL).all() and (t[-GUARD:] == SENTINEL).all(), 'a word outside the output was written'
        assert not (t[GUARD:-GUARD] == SENTINEL).any(), 'an answer was not written'
    return maxima_ref.Maxima(cnt[GUARD:-GUARD].copy(), cha[GUARD:-GUARD].reshape(n, R).copy(), pos[GUARD:-GUARD].reshape(n, R).copy(),
                             sco[GUARD:-GUARD].view(np.float32).reshape(n, R).copy(), pts[GUARD:-GUARD].view(np.float32).reshape(n, R, 2).copy())


def _kernel_equals_the_rule(hip, shape, offsets=()):
    for what, x, screen, want in _cases(shape):
        _same(_device_maxima(hip, x, screen), want, what)
        for offset in offsets:
            _same(_device_maxima(hip, x, screen, offset), want, '{} offset {}'.format(what, offset))


def _kernel_equals_peaks_of(hip, x, screens, what):
    """Where the loops would take minutes the reference is maxima.peaks_of, which the tests above hold to them."""
    from pyopenvino_amd import maxima
    for screen in screens:
        want = maxima.peaks_of(x, _screen(screen))
        got = _device_maxima(hip, x, screen)
        _same(got, want, '{} {}'.format(what, screen))
        _filler_behind_the_counts(got)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_equals_the_rule(hip, shape):
    assert hip.call(FORM, *shape[2:]) == (FORM_WAVE if shape[2] * shape[3] <= WAVE_PLANE else FORM_BLOCK)
    _kernel_equals_the_rule(hip, shape, offsets=(1, 2, 3) if shape in ((3, 5, 7, 9), (1, 2, 33, 31)) else ())


@pytest.mark.gpu
@pytest.mark.parametrize('delta', [-1, 0, 1])
def test_kernel_equals_the_rule_at_the_form_step(hip, delta):
    """Planes of T - 1, T and T + 1 elements for the H * W = T behind which the form query changes its answer, as one row (column chunks
    of a tile, offsets 1 .. 3) and as rows of a few elements."""
    from pyopenvino_amd import maxima
    assert _form_steps() == FORM_STEPS
    for T in FORM_STEPS:
        size = T + delta
        assert hip.call(FORM, 1, size) == (FORM_WAVE if delta <= 0 else FORM_BLOCK)
        rng = np.random.default_rng(size)
        screens = ((None,) + UNCAPPED + ('QUARTER', 'NORMALISED'), (0.5, 5, 9, 'NONE', 'HEATMAP'))
        for shape in ((3, 2, 1, size), (2, 3, next(h for h in (3, 2, 5, 1) if size % h == 0), 0)):
            shape = shape[:3] + (size // shape[2],)
            assert hip.call(FORM, *shape[2:]) == hip.call(FORM, 1, size)
            for what, x in _fillings(rng, shape):
                for offset in (0, 1 + size % 3):
                    for screen in screens:
                        _same(_device_maxima(hip, x, screen, offset), maxima.peaks_of(x, _screen(screen)), '{} {} {} offset {}'.format(shape, what, screen, offset))


@pytest.mark.gpu
@pytest.mark.parametrize('ascending', [True, False])
def test_kernel_keeps_the_largest_of_more_maxima_than_its_buffer_holds(hip, ascending):
    """A lattice with more maxima a plane than the key buffer holds -- 91 x 91, the smallest such square for a workgroup: 46 * 46 = 2116
    against KEY_CAPACITY; 1 x 1023 for a wave: 512 against WAVE_KEY_CAPACITY less the 256 a cut leaves --: ascending, every later
    maximum is above the floor and the buffer is cut before every tile but the first; descending, everything behind the first cut is
    skipped.  And a 512-wide plane, ten rows a tile, one of 1200 columns, which a workgroup takes in two chunks, and a narrow one of five tiles."""
    for shape, capacity in (((2, 3, 91, 91), KEY_CAPACITY), ((3, 2, 1, 1023), WAVE_KEY_CAPACITY - 256), ((1, 2, 30, 512), 0), ((1, 1, 7, 1200), 0), ((1, 1, 5000, 3), 0)):
        x = _lattice(shape, ascending)
        side = lambda d: -(-d // 2)
        assert side(shape[2]) * side(shape[3]) > capacity and (shape[2] != shape[3] or side(shape[2] - 1) ** 2 <= capacity)
        want = _kernel_equals_peaks_of(hip, x, ((1000.5, 256, None, 'NONE', 'NORMALISED'), (None, 7, 10, 'NONE', 'HEATMAP'),
                                                (None,) + UNCAPPED + ('QUARTER', 'NORMALISED')), shape)
        assert (want.counts > 0).all()
    rng = np.random.default_rng(17)                            # dense noise on a plane of several tiles and chunks, a few NaNs in it
    x = rng.standard_normal((2, 2, 70, 530)).astype(np.float32)
    x.reshape(-1).view(np.uint32)[rng.choice(x.size, size=300, replace=False)] = QUIET
    _kernel_equals_peaks_of(hip, x, ((None,) + UNCAPPED + ('QUARTER', 'NORMALISED'), (0.0, 32, 40, 'QUARTER', 'HEATMAP')), 'noise')


@pytest.mark.gpu
def test_kernel_walks_more_planes_than_its_grid(hip):
    """More planes than launch 1 starts workgroups, in either form: the grid-stride loop takes a second trip, and the last planes' keys
    reach their rows."""
    rng = np.random.default_rng(23)
    for shape, grid, form in (((3, 3000, 1, 5), WAVE_GRID, FORM_WAVE), ((2, 4100, 25, 41), BLOCK_GRID, FORM_BLOCK)):
        assert shape[0] * shape[1] > grid and hip.call(FORM, *shape[2:]) == form
        x = rng.standard_normal(shape).astype(np.float32)
        x[:, -1] += 10                                          # the last plane of every row is answered first
        want = _kernel_equals_peaks_of(hip, x, ((None, 2, 1024, 'QUARTER', 'NORMALISED'), (1.5, 256, 50, 'NONE', 'HEATMAP')), shape)
        assert (want.channels[:, 0] == shape[1] - 1).all()


@pytest.mark.gpu
def test_entry_rejects_what_it_cannot_do(hip):
    t = hip.DeviceTensor.from_numpy(np.arange(256, dtype=np.float32))
    o = hip.DeviceTensor.empty((4096,), np.int32)
    at = lambda words: ctypes.c_void_p(o.ptr + 4 * words)
    good = [ctypes.c_void_p(t.ptr), 2, 4, 4, 8, 8, 16, 1, 1, 0, 0.0, at(0), at(1024), at(1100), at(1200), at(1300), at(1400)]
    hip.call(ENTRY, *good)
    bads = [(0, None)] + [(i, None) for i in range(11, 17)]                                # a null pointer
    bads += [(0, ctypes.c_void_p(t.ptr + 2)), (11, ctypes.c_void_p(o.ptr + 4))] + [(i, ctypes.c_void_p(o.ptr + 4802)) for i in range(12, 17)]     # off their boundaries
    bads += [(i, bad) for i in (1, 2, 3, 4) for bad in (0, -1)]                             # n, K, H, W < 1
    bads += [(5, 0), (5, -1), (5, 257), (6, 0), (6, -3), (6, 1025)]                         # M, R out of range
    bads += [(7, 2), (7, -1), (8, 2), (8, -1), (9, 2), (9, -1)]                             # refine, space unknown, has_min neither 0 nor 1
    bads += [(10, float('nan')), (10, float('inf')), (10, float('-inf'))]                   # min_score not finite
    for i, bad in bads:
        args = list(good)
        args[i] = bad
        with pytest.raises(hip.PvhipError):
            hip.call(ENTRY, *args)
        if i == 10:
            args[9] = 1
            with pytest.raises(hip.PvhipError):
                hip.call(ENTRY, *args)
    for n, K, H, W, M in ((2, 4, 1, 1, 8), (1, 1, 4097, 4096, 8), (1, 1, 1 << 16, 1 << 16, 8), (1, 128, 4096, 4096, 1), (1, 1 << 30, 1, 2, 1),
                          (4, 1 << 21, 2, 2, 256), (1 << 23, 1, 1, 2, 256)):
        args = list(good)                                      # H * W < 2, H * W > 2^24, K * H * W > 2^31 - 1, n * K * M >= 2^31
        args[1:6] = n, K, H, W, M
        with pytest.raises(hip.PvhipError):
            hip.call(ENTRY, *args)
    hip.synchronize()
    x = np.arange(256, dtype=np.float32).reshape(2, 4, 4, 8)   # the device is still usable
    x[:, :, 1, 2] += 500
    screen = (100.0, 8, 16, 'QUARTER', 'NORMALISED')
    _same(_device_maxima(hip, x, screen), maxima_ref.maxima(x, *screen), 'after the refusals')


def _on_device(hip, req, out_name):
    """The Result the request's last pass left: still a device tensor."""
    G = req.runner.ienet.G
    (value,) = [G.nodes[nid]['result'] for nid, result in req.runner.ienet.find_node_by_type('Result') if result == out_name]
    assert isinstance(value, hip.DeviceTensor)
    return np.asarray(value)


@pytest.mark.gpu
def test_public_path(hip, tmp_path):
    """The truncated mnist network at batch 3: maxima= is the rule on the request's own full Result in every form of the value, named and
    unnamed; a second call with another min_score allocates nothing; three passes on a device-resident input, the third replayed."""
    import test_answer_checks as order_tests
    from pyopenvino_amd import Maxima, MaximaScreen
    n = 3
    ex, net, name, out_name = _mnist_head(tmp_path, n, requests=2)
    req = ex.requests[0]
    x = _pixels(10, n)
    full = np.array(req.infer({name: x})[out_name], copy=True)
    assert full.shape == (n, 32, 26, 26) and full.dtype == np.float32 and np.isfinite(full).all()
    found, cut = _head_found(full)
    plain = MaximaScreen(cut, 4, 50, 'NONE', 'HEATMAP')
    for given in (True, cut, MaximaScreen(), MaximaScreen(cut), plain, {out_name: True}, {out_name: plain}):
        got = req.infer({name: x}, maxima=given)
        assert set(got) == {out_name} and isinstance(got[out_name], Maxima)
        _same(got[out_name], _head_want(full, found, given[out_name] if isinstance(given, dict) else given), repr(given))
        _filler_behind_the_counts(got[out_name])
    default = _head_want(full, found, True)
    assert default.channels.shape == (n, 1024) and 0 < _head_want(full, found, cut).counts.sum() < default.counts.sum()
    _same(ex.infer({name: x}, maxima=True)[out_name], default, 'the network\'s own infer()')
    _same(ex.requests[1].infer({name: x}, None, None, None, None, None, cut)[out_name], _head_want(full, found, cut), 'the second request, positionally')
    assert np.array_equal(ex.infer({name: x})[out_name], full)              # and whole again without the keyword
    assert sorted(ex.answers.blocks) == [(out_name, 4, 50, 'NONE', 'HEATMAP'), (out_name, 32, 1024, 'QUARTER', 'NORMALISED')]
    # another min_score: the same blocks, nothing allocated
    real_call, issued = hip.call, []
    hip.call = lambda entry, *args: (issued.append(entry), real_call(entry, *args))[1]
    try:
        got = req.infer({name: x}, maxima=cut / 2)[out_name]
    finally:
        hip.call = real_call
    _same(got, _head_want(full, found, cut / 2), 'another min_score')
    assert issued.count(ENTRY) == 1 and not set(order_tests.ALLOCATIONS) & set(issued[issued.index(ENTRY):])
    assert len(ex.answers.blocks) == 2
    # the same device-resident tensor: eager, eager, replayed; identical answers, and the Result stays on the device
    xd = hip.DeviceTensor.from_numpy(x)
    for given in (True, plain):
        other, _, _, _ = _mnist_head(tmp_path, n)
        answers = []
        for call in range(3):
            other.requests[0].start_async({name: xd}, maxima=given)
            assert (other.requests[0]._replayed is not None) == (call == 2), call
            answers.append(other.requests[0].wait()[out_name])
            _same(answers[-1], _head_want(full, found, given), '{} pass {}'.format(given, call))
            helpers.assert_bit_exact(_on_device(hip, other.requests[0], out_name), full, 'the Result behind pass {}'.format(call))
        for later in answers[1:]:
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(answers[0], later))
        other.release_device_state()
        assert not other.answers.blocks
    with pytest.raises(ValueError, match='maxima: Result .* is asked for with keypoints as well'):
        ex.infer({name: x}, keypoints=True, maxima={out_name: True})


@pytest.mark.gpu
def test_the_launch_order_behind_the_pass(hip, tmp_path):
    """What test_answer_checks pins for the other kinds: select, the entry once (its two launches are one call), one event, select;
    wait() makes exactly one copy; no pass after the first allocates -- alone and beside top_k of another Result."""
    import test_answer_checks as order_tests
    from pyopenvino_amd import IECore
    n = 2
    x = hip.DeviceTensor.from_numpy(_pixels(20, n))
    ex, _, name, out_name = _mnist_head(tmp_path, n)
    for asked in (dict(maxima=True), dict(maxima=0.25)):
        got = order_tests._same_answers(order_tests._passes(hip, ex.requests[0], {name: x}, asked, [ENTRY], [1]), out_name)
        assert got.counts.shape == (n,) and got.channels.shape == (n, 1024) and got.points.shape == (n, 1024, 2) and (got.counts > 0).all()
        ex, _, name, out_name = _mnist_head(tmp_path, n)        # (a request that has not recorded yet)
    matrix = order_tests.matrix
    ie = IECore(plugin_package='pyopenvino_amd.op_plugins')
    net = ie.read_network(matrix._two_heads(str(tmp_path)), weights=os.path.join(matrix.MODELS, 'mnist.bin'))
    net.set_batch(n)
    two = ie.load_network(net, 'GPU', num_requests=1)
    rows, maps = (out['name'] for out in sorted(net.outputs, key=lambda out: len(out['input'][0]['dims'])))
    answers = order_tests._passes(hip, two.requests[0], {net.inputs[0]['name']: x}, dict(top_k={rows: 3}, maxima={maps: True}),
                                  ['pvhip_topk_rows_f32', ENTRY], [1, 1])
    assert order_tests._same_answers(answers, rows).indices.shape == (n, 3) and order_tests._same_answers(answers, maps).positions.shape == (n, 1024)


@pytest.mark.gpu
def test_requests_in_flight(hip, tmp_path):
    """Two requests at batch 3, three steps, another input every time, the keyword cycling through True, a named MaximaScreen and None
    per request and step: all started, then all waited for; every answer is the rule (maxima.peaks_of, which the tests above hold to the
    loops) on that input's synchronous single-request Result."""
    from pyopenvino_amd import MaximaScreen, maxima
    B, R, steps = 3, 2, 3
    ex, net, name, out_name = _mnist_head(tmp_path, B, requests=R)
    single, _, _, _ = _mnist_head(tmp_path, B)
    xs = [[_pixels(3000 + 100 * step + 10 * r, B) for r in range(R)] for step in range(steps)]
    fulls = [[np.array(single.infer({name: x})[out_name], copy=True) for x in row] for row in xs]
    assert len({f.tobytes() for row in fulls for f in row}) == R * steps
    plain = MaximaScreen(0.5, 3, 40, 'NONE', 'HEATMAP')
    kinds = (True, {out_name: plain}, None)
    seen = set()
    for step in range(steps):
        asked = [(r + step) % 3 for r in range(R)]
        for r in range(R):
            ex.start_async(r, {name: xs[step][r]}, maxima=kinds[asked[r]])
        for r in (reversed(range(R)) if step % 2 else range(R)):
            res = ex.wait(r)[out_name]
            seen.add((r, asked[r]))
            if asked[r] == 2:
                helpers.assert_bit_exact(res, fulls[step][r], 'step {} request {}'.format(step, r))
            else:
                _same(res, maxima.peaks_of(fulls[step][r], plain if asked[r] else True), 'step {} request {} kind {}'.format(step, r, asked[r]))
    assert len(seen) == R * 3                                 # every request gave every kind of answer


@pytest.mark.gpu
def test_cascade_rows_behind_count_have_no_maxima(hip, tmp_path):
    """GoogLeNet's first Convolution + bias + ReLU at batch 8 as a heatmap network (8, 64, 112, 112), fed DetectedRois(frames, a records
    array) with fewer survivors than rows: the rows behind `count` are NaN rows and come back with count 0 and all-filler slots; the
    rows before it are the rule (maxima.peaks_of) on the full Result of the same feed; and detected_rois() still reads its table."""
    from pyopenvino_amd import DetectedRois, IECore, maxima
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
    ie = IECore(plugin_package=keypoints_tests.HIP)
    net = ie.read_network(keypoints_tests._heatmap_head('googlenet-v1', tmp_path), weights=top_k_tests._blob(11))
    net.set_batch(n)
    name, out_name = net.inputs[0]['name'], net.outputs[0]['name']
    det_tests._declare(net, name, kind, mean=roi_tests._mean())
    ex = ie.load_network(net, 'GPU', num_requests=1)
    req = ex.requests[0]
    full = np.array(req.infer({name: DetectedRois(frames, rec, min_confidence=conf)})[out_name], copy=True)
    assert full.shape == (n, 64, 112, 112)
    assert np.isfinite(full[:want.count]).all() and (_bits(full[want.count:]) == QUIET).all()
    got = req.infer({name: DetectedRois(frames, rec, min_confidence=conf)}, maxima=True)[out_name]
    _same(got, maxima.peaks_of(full), 'cascade')
    _filler_behind_the_counts(got)
    assert (got.counts[:want.count] > 0).all() and (got.counts[want.count:] == 0).all() and (got.channels[want.count:] == -1).all()
    det_tests._same(req.detected_rois(name), want, 'with maxima')
