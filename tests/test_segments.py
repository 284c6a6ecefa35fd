"""A segmentation network's answer made on the device (``infer(..., segments=...)``, pvhip_segment_labels_f32): the class of every pixel of
an (n, C, H, W) Result, and the area and extent of every class, by the rule of tests/segments_ref.py -- labels byte for byte, areas and
extents exactly --, one entry call behind the pass and one read-back of 4 ceil(n H W / 4) + 20 n C bytes.  The first tests need no GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import helpers
import segments_ref
import test_keypoints as keypoints_tests
import test_top_k as top_k_tests

ENTRY, FORM = 'pvhip_segment_labels_f32', 'pvhip_segment_labels_form'
NAN, INF = np.float32(np.nan), np.float32(np.inf)
QUIET = 0x7FC00000
FORM_NONE, FORM_QUADS = 0, 1                            # PVHIP_SEGMENT_FORM_*
TRIP_PIXELS = 1024                                      # kTripPixels of pvhip_segments.hip: the pixels one workgroup takes per trip
MAX_WORKGROUPS = 2048                                   # kMaxBlocks of pvhip_common.h: beyond as many trips a workgroup takes several
FORM_STEPS = []                                     # the H * W behind which the form query changes its answer: one form, no step
_mnist_head, _pixels = keypoints_tests._mnist_head, keypoints_tests._pixels
det_tests, roi_tests = top_k_tests.det_tests, top_k_tests.roi_tests
SHAPES = [(1, 1, 1, 2), (2, 3, 1, 7), (3, 5, 7, 9), (2, 4, 6, 2), (1, 255, 2, 2), (2, 21, 40, 30)]
UNSPLIT = ('all equal', 'NaN row')                      # the fillings a threshold need not split


def _same(got, want, what=''):
    """`got` (a Segments of the product) equals `want` (the rule's): labels byte for byte, areas and extents exactly."""
    assert got.labels.dtype == np.uint8 and got.areas.dtype == np.int32 and got.extents.dtype == np.int32, what
    assert got.labels.shape == want.labels.shape and got.areas.shape == want.areas.shape and got.extents.shape == want.areas.shape + (4,), what
    bad = np.argwhere(got.labels != want.labels)
    assert not len(bad), '{}: {} pixels differ, the first {}: label {} want {}'.format(what, len(bad), bad[0].tolist(), got.labels[tuple(bad[0])],
                                                                                     want.labels[tuple(bad[0])])
    bad = np.argwhere(got.areas != want.areas)
    assert not len(bad), '{}: (row, class) {}: area {} want {}'.format(what, bad[0].tolist(), got.areas[tuple(bad[0])], want.areas[tuple(bad[0])])
    bad = np.argwhere((got.extents != want.extents).any(axis=2))
    assert not len(bad), '{}: (row, class) {}: extent {} want {}'.format(what, bad[0].tolist(), got.extents[tuple(bad[0])].tolist(),
                                                                         want.extents[tuple(bad[0])].tolist())


def _threshold(scores):
    """The median of the best scores that are numbers (0 without one)."""
    finite = scores[np.isfinite(scores)]
    return float(np.median(finite)) if finite.size else 0.0


def _ref(full, min_score=None):
    return segments_ref.segments(full, None if min_score is None else float(np.float32(min_score)))


def _class_map(shape, classes):
    """Scores of `shape` whose best class at every pixel is `classes` (n, H, W): 4 .. 5 there, below 1 elsewhere."""
    n, C, H, W = shape
    rng = np.random.default_rng(C * 1000 + H * W)
    x = rng.uniform(0, 1, shape).astype(np.float32)
    np.put_along_axis(x, classes[:, None], rng.uniform(4, 5, (n, 1, H, W)).astype(np.float32), axis=1)
    return x


def _blocky(shape):
    """A few large regions: quadrants of the map, another class in each and in each row."""
    n, C, H, W = shape
    r, y, x = np.meshgrid(np.arange(n), np.arange(H), np.arange(W), indexing='ij')
    return _class_map(shape, (r + 2 * (2 * y // max(H, 1)) + (2 * x // max(W, 1))) % C)


def _salt_and_pepper(shape):
    """Every pixel another class than the pixel before it (C > 1)."""
    n, C, H, W = shape
    r, y, x = np.meshgrid(np.arange(n), np.arange(H), np.arange(W), indexing='ij')
    return _class_map(shape, (r + y * W + x) % C)


def _fillings(rng, shape):
    """[(what, (n, C, H, W) float32)]: every filling of the rule's tests for one shape.  All but the all-equal and the NaN-row one have
    a dent -- every class of pixel (0, 0) of row 0 at -8, below everything else --, so that the median of the best scores splits them."""
    n, C, H, W = shape
    quantised = (rng.integers(0, 4, shape) / 4).astype(np.float32)
    zeros = rng.choice(np.array([0.0, -0.0, -1.0, -2.0], np.float32), shape)
    zeros.reshape(n, C, -1)[:, :, 1::2] = np.minimum(zeros.reshape(n, C, -1)[:, :, 1::2], np.float32(-1))      # (every other pixel: no zero at all)
    nans = rng.standard_normal(shape).astype(np.float32)
    many = max(1, nans.size // 40)
    at = rng.choice(nans.size, size=many, replace=False)
    kinds = np.array(top_k_tests.SPECIALS[:3], np.uint32)      # quiet, negative, signalling
    nans.reshape(-1).view(np.uint32)[at] = kinds[np.arange(many) % 3] | (rng.integers(0, 1 << 16, many).astype(np.uint32) << np.uint32(3))
    row = rng.standard_normal(shape).astype(np.float32)
    row.view(np.uint32)[n // 2] = QUIET                        # one all-NaN row (n == 1: the only one)
    out = [('normal', rng.standard_normal(shape).astype(np.float32)), ('four levels', quantised), ('blocky', _blocky(shape)),
           ('salt and pepper', _salt_and_pepper(shape)), ('signed zeros', zeros), ('NaNs', nans), ('NaN row', row),
           ('all equal', np.full(shape, 0.25, np.float32))]
    for what, x in out:
        if what not in UNSPLIT:
            x[0, :, 0, 0] = -8
    return out


def _cases(shape):
    """[(what, x, min_score or None, the rule's answer)] of a shape: every filling without and with a min_score, the median of its best
    scores.  The answers are made once per shape and handed out unchanged."""
    if shape not in _cases.made:
        rng = np.random.default_rng(sum(d * 31 ** i for i, d in enumerate(shape)))
        made = []
        for what, x in _fillings(rng, shape):
            at = segments_ref.best(x)
            cut = _threshold(at[1])
            for min_score in (None, cut):
                want = segments_ref.segments(x, None if min_score is None else float(np.float32(min_score)), at)
                if min_score is not None and what not in UNSPLIT:      # a condition on the inputs: the threshold has something to do
                    assert (want.labels == 255).any() and (want.labels != 255).any(), (shape, what)
                made.append(('{} {} min_score {}'.format(shape, what, min_score), x, min_score, want))
        _cases.made[shape] = made
    return _cases.made[shape]


_cases.made = {}


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
def test_the_rule_on_hand_written_pixels():
    from pyopenvino_amd import Segments, SegmentScreen, segments

    def both(x, min_score=None):
        x = np.asarray(x, np.float32)
        want = segments_ref.segments(x, min_score)
        got = segments.labels(x, SegmentScreen(min_score))      # the product's own numpy form (host Results) is the same rule
        assert isinstance(got, Segments)
        _same(got, want, str(x.tolist()))
        return want

    def pixel(values, min_score=None):
        """The label of one pixel with these scores (beside a second pixel that is always class 0)."""
        x = np.zeros((1, len(values), 1, 2), np.float32)
        for c, value in enumerate(values):                      # (a np.uint32 is the score's bits: no conversion quiets a signalling NaN)
            if isinstance(value, np.uint32):
                x.view(np.uint32)[0, c, 0, 0] = value
            else:
                x[0, c, 0, 0] = value
        x[0, 0, 0, 1] = 1
        return int(both(x, min_score).labels[0, 0, 0])

    word = np.uint32

    assert pixel([1, 3, 3, 2]) == 1 and pixel([2, 2, 2]) == 0                      # a tie: the lower class
    assert pixel([0.0, -0.0]) == 0 and pixel([-0.0, 0.0]) == 0 and pixel([-1, -0.0, 0.0]) == 1      # zeros of either sign are equal
    for bits in (0x7FC00000, 0xFFC00001, 0x7F800123, 0xFF800001):                  # a NaN of each sign, quiet and signalling: void,
        assert pixel([word(bits), 5, 1]) == 255 and pixel([1, 5, word(bits)]) == 255      # in a lower and in a higher class than the best
        assert pixel([1, 5, word(bits)], -1e30) == 255 and pixel([word(bits)]) == 255
    assert pixel([1, INF, 3]) == 1 and pixel([INF, INF]) == 0 and pixel([-INF, -INF, -INF]) == 0 and pixel([-INF, -3e38]) == 1
    assert pixel([-INF, -INF], -3e38) == 255 and pixel([1, INF], 3e38) == 1
    # min_score equal to the best score keeps, one ulp above it voids; the threshold is the float32
    top = np.float32(0.7)
    assert pixel([0.1, top, 0.3], float(top)) == 1 and pixel([0.1, top, 0.3], float(np.nextafter(top, INF))) == 255
    assert pixel([0.1, top, 0.3], float(np.nextafter(top, -INF))) == 1 and pixel([0.1, top, 0.3], 0.7) == 1
    assert pixel([-0.0], 0.0) == 0 and pixel([0.0, -1], -0.0) == 0                  # -0.0 is not below +0.0
    # C == 1: a thresholded mask
    mask = both([[[[0.2, 0.9, 0.5], [0.5, 0.1, 0.7]]]], 0.5)
    assert mask.labels.tolist() == [[[255, 0, 0], [0, 255, 0]]] and mask.areas.tolist() == [[4]] and mask.extents.tolist() == [[[0, 0, 3, 2]]]
    assert both([[[[0.2, 0.9]]]]).labels.tolist() == [[[0, 0]]]
    # a class with no pixels, a class that is one pixel in a corner, and the void pixels counted by what is left
    x = np.zeros((2, 4, 3, 5), np.float32)
    x[:, 1] = 1
    x[0, 2, 2, 4] = 2                                                              # class 2: the last pixel of row 0
    x[1, 3, 0, 0] = 2                                                              # class 3: the first pixel of row 1
    x[1, 0, 1, 2] = NAN
    want = both(x)
    assert want.areas.tolist() == [[0, 14, 1, 0], [0, 13, 0, 1]] and int(3 * 5 - want.areas[1].sum()) == 1 and want.labels[1, 1, 2] == 255
    assert want.extents[0].tolist() == [[0, 0, 0, 0], [0, 0, 5, 3], [4, 2, 5, 3], [0, 0, 0, 0]]
    assert want.extents[1].tolist() == [[0, 0, 0, 0], [0, 0, 5, 3], [0, 0, 0, 0], [0, 0, 1, 1]]
    for corner in ((0, 0), (0, 4), (2, 0), (2, 4)):
        x = np.zeros((1, 2, 3, 5), np.float32)
        x[0, 1][corner] = 1
        want = both(x)
        assert want.areas.tolist() == [[14, 1]] and want.extents[0, 1].tolist() == [corner[1], corner[0], corner[1] + 1, corner[0] + 1]
    # anything but float32 (n, C, H, W) with C <= 255 and 2 <= H * W is refused
    for bad in (np.zeros((1, 1, 1, 1), np.float32), np.zeros((2, 3, 4), np.float32), np.zeros((1, 1, 2, 2), np.float64), np.zeros((1, 0, 2, 2), np.float32),
                np.zeros((1, 256, 1, 2), np.float32)):
        with pytest.raises(ValueError, match='labels'):
            segments.labels(bad)
    for bad in ('x', None, False, SegmentScreen(np.nan), SegmentScreen(1e39), SegmentScreen('0.5')):
        with pytest.raises(ValueError, match='labels'):
            segments.labels(np.zeros((1, 1, 2, 2), np.float32), bad)


@pytest.mark.parametrize('shape', SHAPES)
def test_labels_agrees_with_the_loops(shape):
    from pyopenvino_amd import SegmentScreen, segments
    for what, x, min_score, want in _cases(shape):
        _same(segments.labels(x, SegmentScreen(min_score)), want, what)
    x = np.random.default_rng(3).standard_normal((2, 3, 8, 5, 7)).astype(np.float32)[:, :, :, :, 2]      # not contiguous: the same answer
    _same(segments.labels(x), segments_ref.segments(np.ascontiguousarray(x)), 'strided')


def test_argument_rules(tmp_path, monkeypatch):
    """Every refusal is a ValueError('segments: ...') raised before anything is staged or launched: this test runs where there is no device."""
    from pyopenvino_amd import Gallery, GalleryMatch, SegmentScreen, answers as answers_module, detections as detections_rule, segments as rule
    n = 4
    ex, net, name, out_name = _mnist_head(tmp_path, n, requests=2)
    x = np.zeros((n, 1, 28, 28), np.float32)
    req = ex.requests[0]
    others = ('top_k', 'detections', 'matches', 'keypoints')
    starts = (lambda s, **kw: ex.infer({name: x}, segments=s, **kw), lambda s, **kw: req.start_async({name: x}, segments=s, **kw),
              lambda s, **kw: ex.requests[1].infer({name: x}, segments=s, **kw), lambda s, **kw: ex.start_async(1, {name: x}, segments=s, **kw),
              lambda s, **kw: req.infer({name: x}, *(kw.get(k) for k in others), s),
              lambda s, **kw: req.start_async({name: x}, *(kw.get(k) for k in others), s),
              lambda s, **kw: ex.infer({name: x}, False, *(kw.get(k) for k in others), s),
              lambda s, **kw: ex.start_async(0, {name: x}, *(kw.get(k) for k in others), s))       # the keyword stands last

    def refused(match, s, network=ex, starts=starts, **kw):
        for start in starts:
            with pytest.raises(ValueError, match=match) as e:
                start(s, **kw)
            assert str(e.value).startswith('segments: '), str(e.value)
        for r in network.requests:
            assert not r._in_flight and not r._asks and not r.runner.answers.blocks and not r.runner.host_inputs.slots and r.runner._pending is None

    refused('no Result named', {'heatmaps/nope': True})
    refused('no Result named', {out_name: True, 'nope': 0.5})
    for bad in ('VOID', [0.5], (0.5,), False, np.bool_(True), b'1', 1j, SegmentScreen):
        refused('a SegmentScreen, a min_score or True', bad)
        refused('a SegmentScreen, a min_score or True', {out_name: bad})
    refused('a SegmentScreen, a min_score or True', {out_name: None})
    for bad in (np.nan, np.inf, -np.inf, 'x', True, 1e39, -1e39, [1.0]):
        refused('min_score', SegmentScreen(bad))
        refused('min_score', {out_name: SegmentScreen(min_score=bad)})
    for bad in (np.nan, np.inf, 1e39, np.float64(-1e300)):
        refused('min_score', bad)
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
    for dims in ((n, 32, 676), (n, 32, 26, 26, 1), (n, 32, 1, 1), (2, 32, 26, 26), (n, 32, 4097, 4096), (n, 256, 26, 26), (n, 1000, 2, 2)):
        for port in ports:                                                     # another rank, one pixel, another batch, beyond 2^24, C > 255
            port['dims'] = dims
        try:
            refused('has shape .*: not \\(n = 4, C <= 255, H, W\\) with 2 <= H \\* W <= 2\\^24', {out_name: True})
            refused('no FP32 Result', 0.5)
        finally:
            for port, dims in zip(ports, declared):
                port['dims'] = dims
    for port in ports:                                                         # 255 classes are the most
        port['dims'] = (n, 255, 26, 26)
    try:
        assert rule.checked(ex.requests[0].runner.ienet, True, False) == {out_name: SegmentScreen(None)}
    finally:
        for port, dims in zip(ports, declared):
            port['dims'] = dims
    # a classifier has no maps, a detector's (1, 1, R, 7) records are none for the unnamed forms
    ie_c, net_c, name_c = roi_tests._net('mnist', n)
    cls = ie_c.load_network(net_c, 'GPU', num_requests=1)
    xc = np.zeros((n, 1, 28, 28), np.float32)
    cls_starts = (lambda s, **kw: cls.infer({name_c: xc}, segments=s), lambda s, **kw: cls.requests[0].start_async({name_c: xc}, segments=s))
    refused('no FP32 Result', True, cls, cls_starts)
    refused('has shape', {net_c.outputs[0]['name']: True}, cls, cls_starts)
    ie_d, net_d, name_d = roi_tests._net('ssd_mobilenet_v1_coco', 1)
    det = ie_d.load_network(net_d, 'GPU', num_requests=1)
    dims = tuple(net_d.outputs[0]['input'][0]['dims'])
    assert dims[:2] == (1, 1) and dims[3] == 7
    xd = np.zeros((1, 3, 300, 300), np.float32)
    refused('no FP32 Result', True, det, (lambda s, **kw: det.infer({name_d: xd}, segments=s), lambda s, **kw: det.requests[0].start_async({name_d: xd}, segments=s)))
    # one Result under two keywords: the later keyword speaks and names the earlier.  keypoints fits the same Results; no Result passes
    # the shape rules of the other three, so their checks are stubbed to reach the rule of Answers.checked itself
    clash = 'Result {!r} is asked for with {} as well'
    for value in (True, 0.5, {out_name: True}):
        refused(clash.format(out_name, 'keypoints'), True, keypoints=value)
        refused(clash.format(out_name, 'keypoints'), {out_name: 0.5}, keypoints=value)
    gal = Gallery(np.ones((3, 7), np.float32))
    for keyword, module, stub, value in (('top_k', answers_module.top_k_rule, lambda ienet, top_k, sharded: {out_name: 1}, 1),
                                         ('detections', answers_module.detections_rule, lambda ienet, d, sharded: {out_name: detections_rule.DetectionScreen()}, 0.5),
                                         ('matches', answers_module.gallery_rule, lambda ienet, matches, sharded: {out_name: GalleryMatch(gal, 1, None)}, gal)):
        with monkeypatch.context() as patched:
            patched.setattr(module, 'checked', stub)
            refused(clash.format(out_name, keyword), True, **{keyword: value})
            refused(clash.format(out_name, keyword), {out_name: 0.5}, **{keyword: value})
    assert gal._dev is None
    # the resolved forms
    default = SegmentScreen(None)
    assert SegmentScreen() == default
    assert rule.checked(net, None, False) == {} and rule.checked(net, {}, True) == {} and rule.checked(net, True, False) == {out_name: default}
    assert rule.checked(net, 0.5, False) == rule.checked(net, {out_name: np.float32(0.5)}, False) == {out_name: SegmentScreen(0.5)}
    assert rule.checked(net, 1, False) == {out_name: SegmentScreen(1.0)} and isinstance(rule.checked(net, 1, False)[out_name].min_score, float)
    assert rule.checked(net, 0.7, False)[out_name].min_score == float(np.float32(0.7))                   # the threshold is the float32
    assert rule.checked(net, {out_name: SegmentScreen(np.int64(-2))}, False) == {out_name: SegmentScreen(-2.0)}
    assert rule.maps_of((4, 21, 64, 48)) == (4, 21, 64, 48) and rule.maps_of((4, 21, 64, 48), 2) is None and rule.maps_of((4, 21, 1, 1)) is None
    assert rule.maps_of((4, 255, 1, 2)) == (4, 255, 1, 2) and rule.maps_of((4, 256, 1, 2)) is None and rule.maps_of((1, 1, 4096, 4096)) is not None


def test_answers_checked_takes_the_new_argument_last(tmp_path):
    from pyopenvino_amd import SegmentScreen, keypoints, segments as rule
    n = 4
    ex, net, name, out_name = _mnist_head(tmp_path, n)
    x = np.zeros((n, 1, 28, 28), np.float32)
    answers = ex.answers
    assert answers.checked({name: x}, None, None, False) == {} and answers.checked({name: x}, None, None, False, None, None) == {}
    assert answers.checked({name: x}, None, None, False, None, None, None) == {} and answers.checked({name: x}, None, None, False, segments=None) == {}
    asks = answers.checked({name: x}, None, None, False, None, None, 0.5)
    assert set(asks) == {out_name} and isinstance(asks[out_name], rule.Ask) and asks[out_name].KEYWORD == 'segments'
    assert asks[out_name] == (SegmentScreen(0.5),) and asks[out_name].screen == SegmentScreen(0.5)      # an ask equals the plain tuple of its fields
    assert asks == answers.checked({name: x}, None, None, False, segments={out_name: SegmentScreen(0.5)})
    assert asks[out_name].key(out_name) == (out_name,) == rule.Ask(SegmentScreen()).key(out_name)      # one block pair for every threshold
    assert asks[out_name].launch_with() == (0.5,) and asks[out_name].bound({name: x}, {}) is asks[out_name]
    # the five-argument calls answer as before
    kept = answers.checked({name: x}, None, None, False, None, True)
    assert set(kept) == {out_name} and isinstance(kept[out_name], keypoints.Ask)
    assert not answers.blocks and not ex.host_inputs.slots and ex._pending is None


def test_a_host_result_gets_the_rule_in_numpy(tmp_path):
    """A plugin set that computes on the host (the oracle's) hands wait() host arrays: the same keyword, the same rule, no device."""
    from pyopenvino_amd import Segments, SegmentScreen
    n = 3
    ex, net, name, out_name = _mnist_head(tmp_path, n, requests=2, package='oracle.op_plugins')
    x = _pixels(10, n)
    full = np.array(ex.infer({name: x})[out_name], copy=True)
    assert full.shape == (n, 32, 26, 26) and full.dtype == np.float32 and np.isfinite(full).all()
    at = segments_ref.best(full)
    cut = _threshold(at[1])
    for given in (True, cut, SegmentScreen(cut), SegmentScreen()):
        min_score = None if given is True else given.min_score if isinstance(given, SegmentScreen) else given
        want = segments_ref.segments(full, None if min_score is None else float(np.float32(min_score)), at)
        for got in (ex.infer({name: x}, segments=given), ex.requests[1].infer({name: x}, segments={out_name: given})):
            assert set(got) == {out_name} and isinstance(got[out_name], Segments)
            _same(got[out_name], want, repr(given))
        assert ((want.labels == 255).any() and (want.labels != 255).any()) == (min_score is not None)
    assert np.array_equal(ex.infer({name: x})[out_name], full)           # and whole again without the keyword
    with pytest.raises(ValueError, match='segments: min_score'):
        ex.infer({name: x}, segments=SegmentScreen(np.inf))


def test_abi_declares_the_entries():
    import pyopenvino_amd
    from pyopenvino_amd import device, segments
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for entry, count in ((ENTRY, 10), (FORM, 3)):
        assert entry in device.SIGNATURES and len(device.SIGNATURES[entry][1]) == count
        m = re.search(r'\bint\s+' + entry + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S)
        assert m and len(m.group(1).split(',')) == count, entry
    assert ENTRY not in device._NOT_STATUS and FORM in device._NOT_STATUS
    joined = re.sub(r'\s*\n \*\s+', ' ', header)                               # the rule is stated there (its lines joined)
    for phrase in ('NaN of any sign or payload first, then descending with +0.0 == -0.0, ties to the lower class',
                   'the pixel is void iff v[k*] is NaN or (has_min == 1 and v[k*] < min_score)', 'Equality keeps',
                   'labels[r][y][x] = k*, or PVHIP_SEGMENT_VOID (255) when void', 'areas[r][k] is the number of pixels of row r labelled k',
                   '(x0, y0, x1, y1) is min x, min y, max x + 1 and max y + 1 over those pixels',
                   'A class without pixels in a row reads (w, h, 0, 0)'):
        assert phrase in joined, phrase
    for phrase in ('ties to the lower class', 'Equality keeps', '255 when void', 'min x, min y, max x + 1 and max y + 1'):
        assert phrase in re.sub(r'\s*\n\s+', ' ', segments.__doc__) and phrase in re.sub(r'\s*\n\s+', ' ', segments_ref.__doc__), phrase
    for define, value in (('PVHIP_SEGMENT_VOID', 255), ('PVHIP_SEGMENT_MAX_CLASSES', 255), ('PVHIP_SEGMENT_FORM_NONE', FORM_NONE),
                          ('PVHIP_SEGMENT_FORM_QUADS', FORM_QUADS)):
        assert re.search(r'#define\s+{}\s+{}\b'.format(define, value), header), define
    assert re.search(r'#define\s+PVHIP_SEGMENT_MAX_PLANE\s+\(1 << 24\)', header)
    assert (segments.VOID, segments.MAX_CLASSES, segments.MAX_PLANE) == (255, 255, 1 << 24)
    assert re.search(r'#define\s+PVHIP_ABI_VERSION\s+19\b', header)
    lib = device.load_library()
    assert hasattr(lib, ENTRY) and hasattr(lib, FORM) and lib.pvhip_abi_version() == 19
    assert pyopenvino_amd.Segments is segments.Segments and pyopenvino_amd.SegmentScreen is segments.SegmentScreen
    assert 'Segments' in pyopenvino_amd.__all__ and 'SegmentScreen' in pyopenvino_amd.__all__
    assert pyopenvino_amd.Segments._fields == ('labels', 'areas', 'extents')
    assert pyopenvino_amd.SegmentScreen._fields == ('min_score',) and tuple(pyopenvino_amd.SegmentScreen()) == (None,)


def _form_steps(c):
    """Every H * W after which pvhip_segment_labels_form changes its answer, for maps of one image row and `c` classes."""
    from pyopenvino_amd import device
    forms = [device.call(FORM, c, 1, s) for s in range(2, 1 << 14)]
    return [s for s, (a, b) in zip(range(2, 1 << 14), zip(forms, forms[1:])) if a != b]


def test_the_form_query():
    """It needs no device, answers NONE for what the entry refuses, and changes nowhere else: one form serves every size and phase."""
    from pyopenvino_amd import device
    form = lambda c, h, w: device.call(FORM, c, h, w)
    assert [form(1, 1, 1), form(0, 2, 2), form(-1, 2, 2), form(256, 2, 2), form(4, 0, 5), form(4, 5, -1), form(4, 4097, 4096),
            form(4, 1 << 16, 1 << 16)] == [FORM_NONE] * 8
    assert [form(1, 1, 2), form(255, 2, 1), form(21, 513, 513), form(4, 4096, 4096), form(32, 1, 1 << 24)] == [FORM_QUADS] * 5
    for c in (1, 4, 21, 255):
        assert _form_steps(c) == FORM_STEPS                    # a threshold that appears fails here: the kernel test then wants its T - 1, T, T + 1


# ---------------------------------------------------------------------------------------------------------------- GPU
GUARD = top_k_tests.GUARD


def _device_segments(hip, x, min_score, offset=0, label_offset=0):
    """The entry on `x` (n, C, H, W) -- `offset`: starting that many elements into a larger device tensor; `label_offset`: the labels
    starting that many bytes into theirs --, the outputs between sentinel bytes that must stay untouched.  A class without pixels reads
    (W, H, 0, 0) at this level (include/pvhip.h): that is asserted here and turned into zeros, as Blocks.read_back does."""
    n, C, H, W = x.shape
    fill = 0x7F if C <= 127 else 0xFE                          # (no label of the shape is the fill, C == 255's class 254 apart)
    if offset:
        src = hip.DeviceTensor.from_numpy(np.concatenate([np.full(offset, 9e9, np.float32), x.ravel(), np.full(7, 9e9, np.float32)]))
    else:
        src = hip.DeviceTensor.from_numpy(x)
    pixels = n * H * W
    outs = [hip.DeviceTensor.empty((words + 2 * GUARD,), np.int32) for words in ((pixels + label_offset + 3) // 4, n * C, 4 * n * C)]
    for t in outs:
        hip.call('pvhip_memset', ctypes.c_void_p(t.ptr), fill, t.nbytes)
    hip.call(ENTRY, ctypes.c_void_p(src.ptr + 4 * offset), n, C, H, W, int(min_score is not None), float(min_score or 0.0),
             ctypes.c_void_p(outs[0].ptr + 4 * GUARD + label_offset), ctypes.c_void_p(outs[1].ptr + 4 * GUARD), ctypes.c_void_p(outs[2].ptr + 4 * GUARD))
    lab, are, ext = (np.asarray(t).view(np.uint8) for t in outs)
    first = 4 * GUARD + label_offset
    assert (lab[:first] == fill).all() and (lab[first + pixels:] == fill).all(), 'a byte outside the labels was written'
    for t in (are, ext):
        assert (t[:4 * GUARD] == fill).all() and (t[-4 * GUARD:] == fill).all(), 'a word outside the output was written'
    if C <= 254:
        assert not (lab[first:first + pixels] == fill).any(), 'a label was not written'
    areas = are[4 * GUARD:-4 * GUARD].view(np.int32).reshape(n, C).copy()
    extents = ext[4 * GUARD:-4 * GUARD].view(np.int32).reshape(n, C, 4).copy()
    assert (extents[areas == 0] == (W, H, 0, 0)).all(), 'a class without pixels does not read (W, H, 0, 0)'
    extents[areas == 0] = 0
    return segments_ref.Segments(lab[first:first + pixels].reshape(n, H, W).copy(), areas, extents)


def _kernel_equals_the_rule(hip, shape, offsets=()):
    for what, x, min_score, want in _cases(shape):
        cut = None if min_score is None else float(np.float32(min_score))
        _same(_device_segments(hip, x, cut), want, what)
        for offset in offsets:
            _same(_device_segments(hip, x, cut, offset=offset), want, '{} x offset {}'.format(what, offset))
            _same(_device_segments(hip, x, cut, label_offset=offset), want, '{} labels offset {}'.format(what, offset))
            _same(_device_segments(hip, x, cut, offset=offset, label_offset=4 - offset), want, '{} both offset {}'.format(what, offset))


# (2, 2, 33, 32): 1056 pixels a row, past what one workgroup takes per trip; (2, 2, 1, TRIP_PIXELS - 1 .. + 1): the seam between two
# workgroups before, on and behind the seam between two rows, and the sums of a row that come from two workgroups
GPU_SHAPES = [(1, 1, 1, 2), (2, 3, 1, 7), (3, 5, 7, 9), (2, 4, 6, 2), (1, 255, 2, 2), (2, 2, 33, 32), (2, 2, 1, TRIP_PIXELS - 1),
              (2, 2, 1, TRIP_PIXELS), (2, 2, 1, TRIP_PIXELS + 1), (4, 21, 46, 46), (2, 4, 64, 96)]


@pytest.mark.gpu
@pytest.mark.parametrize('shape', GPU_SHAPES)
def test_kernel_equals_the_rule(hip, shape):
    assert hip.call(FORM, *shape[1:]) == FORM_QUADS and FORM_STEPS == []       # (one form: no step to stand at)
    _kernel_equals_the_rule(hip, shape, offsets=(1, 2, 3) if shape == (3, 5, 7, 9) else ())


@pytest.mark.gpu
def test_kernel_equals_the_rule_past_one_trip_a_workgroup(hip):
    """Beyond MAX_WORKGROUPS trips a workgroup takes several consecutive trips and carries its table of sums from one to the next: a
    path no small map reaches.  (3, 2, 1000, 1001) is 2933 trips, two a workgroup, the seams of the batch rows inside a trip and
    inside a workgroup's two.  The loops would take minutes here: the reference is segments.labels, which the tests above hold to them."""
    from pyopenvino_amd import SegmentScreen, segments
    shape = (3, 2, 1000, 1001)
    trips = -(-shape[0] * shape[2] * shape[3] // TRIP_PIXELS)
    assert MAX_WORKGROUPS < trips <= 2 * MAX_WORKGROUPS and (shape[2] * shape[3]) % (2 * TRIP_PIXELS) not in (0, TRIP_PIXELS)
    rng = np.random.default_rng(11)
    x = _blocky(shape)
    x.reshape(-1).view(np.uint32)[rng.choice(x.size, size=500, replace=False)] = QUIET
    cut = float(np.float32(4.5))
    for min_score in (None, cut):
        want = segments.labels(x, SegmentScreen(min_score))
        assert (want.labels == 255).any() and (want.areas > 0).all()
        _same(_device_segments(hip, x, min_score), want, '{} min_score {}'.format(shape, min_score))


@pytest.mark.gpu
def test_entry_rejects_what_it_cannot_do(hip):
    t = hip.DeviceTensor.from_numpy(np.arange(256, dtype=np.float32))
    o = hip.DeviceTensor.empty((512,), np.int32)
    p, a, b, c = ctypes.c_void_p(t.ptr), ctypes.c_void_p(o.ptr), ctypes.c_void_p(o.ptr + 256), ctypes.c_void_p(o.ptr + 512)
    good = [p, 2, 4, 4, 8, 0, 0.0, a, b, c]
    hip.call(ENTRY, *good)
    bads = [(0, None), (7, None), (8, None), (9, None)]                                     # a null pointer
    bads += [(0, ctypes.c_void_p(t.ptr + 2)), (8, ctypes.c_void_p(o.ptr + 258)), (9, ctypes.c_void_p(o.ptr + 513))]      # x, areas, extents off a 4-byte boundary
    bads += [(at, bad) for at in (1, 2, 3, 4) for bad in (0, -1)]                           # n, C, H, W < 1
    bads += [(2, 256), (2, 1000)]                                                           # C > 255
    bads += [(5, 2), (5, -1)]                                                               # has_min neither 0 nor 1
    bads += [(6, float('nan')), (6, float('inf')), (6, float('-inf'))]                      # min_score not finite
    for at, bad in bads:
        args = list(good)
        args[at] = bad
        with pytest.raises(hip.PvhipError):
            hip.call(ENTRY, *args)
        if at == 6:
            args[5] = 1
            with pytest.raises(hip.PvhipError):
                hip.call(ENTRY, *args)
    for n, C, H, W in ((2, 4, 1, 1), (1, 1, 4097, 4096), (1, 1, 1 << 16, 1 << 16), (1 << 30, 1, 1, 2), (128, 1, 4096, 4096), (1 << 15, 2, 256, 256)):
        with pytest.raises(hip.PvhipError):                    # H * W < 2, H * W > 2^24, n * H * W >= 2^31
            hip.call(ENTRY, p, n, C, H, W, 0, 0.0, a, b, c)
    hip.synchronize()
    x = np.arange(256, dtype=np.float32).reshape(2, 4, 4, 8)   # the device is still usable
    x[:, 1, :, :4] += 100
    _same(_device_segments(hip, x, 130.0), segments_ref.segments(x, 130.0), 'after the refusals')


def _on_device(hip, req, out_name):
    """The Result the request's last pass left: still a device tensor."""
    G = req.runner.ienet.G
    (value,) = [G.nodes[nid]['result'] for nid, result in req.runner.ienet.find_node_by_type('Result') if result == out_name]
    assert isinstance(value, hip.DeviceTensor)
    return np.asarray(value)


@pytest.mark.gpu
def test_public_path(hip, tmp_path):
    """The truncated mnist network at batch 3: segments= is the rule on the request's own full Result for True, for a threshold and in the
    named form beside top_k on a second Result, three passes each on a device-resident input, the third replayed from the recording."""
    import test_answer_checks as order_tests
    from pyopenvino_amd import IECore, Segments, SegmentScreen, TopK
    n = 3
    ex, net, name, out_name = _mnist_head(tmp_path, n, requests=2)
    req = ex.requests[0]
    x = _pixels(10, n)
    full = np.array(req.infer({name: x})[out_name], copy=True)
    assert full.shape == (n, 32, 26, 26) and full.dtype == np.float32 and np.isfinite(full).all()
    at = segments_ref.best(full)
    cut = _threshold(at[1])
    wants = {None: segments_ref.segments(full, None, at), cut: segments_ref.segments(full, float(np.float32(cut)), at)}
    assert not (wants[None].labels == 255).any() and (wants[cut].labels == 255).any() and (wants[cut].labels != 255).any()
    assert (wants[None].areas.sum(axis=1) == 26 * 26).all()
    for given, want in ((True, wants[None]), (cut, wants[cut]), (SegmentScreen(cut), wants[cut]), ({out_name: True}, wants[None])):
        got = req.infer({name: x}, segments=given)
        assert set(got) == {out_name} and isinstance(got[out_name], Segments)
        _same(got[out_name], want, repr(given))
    _same(ex.infer({name: x}, segments=True)[out_name], wants[None], 'the network\'s own infer()')
    _same(ex.requests[1].infer({name: x}, None, None, None, None, cut)[out_name], wants[cut], 'the second request, positionally')
    assert np.array_equal(ex.infer({name: x})[out_name], full)              # and whole again without the keyword
    # the same device-resident tensor: eager, eager, replayed; identical answers, and the Result stays on the device
    xd = hip.DeviceTensor.from_numpy(x)
    for given, want in ((True, wants[None]), (cut, wants[cut])):
        other, _, _, _ = _mnist_head(tmp_path, n)
        answers = []
        for call in range(3):
            other.requests[0].start_async({name: xd}, segments=given)
            assert (other.requests[0]._replayed is not None) == (call == 2), call
            answers.append(other.requests[0].wait()[out_name])
            _same(answers[-1], want, '{} pass {}'.format(given, call))
            helpers.assert_bit_exact(_on_device(hip, other.requests[0], out_name), full, 'the Result behind pass {}'.format(call))
        for later in answers[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(answers[0], later))
        assert sorted(other.answers.blocks) == [(out_name,)]
        other.release_device_state()
        assert not other.answers.blocks
    assert sorted(ex.answers.blocks) == [(out_name,)]              # one block pair for every threshold
    # the named form beside top_k on a second Result
    matrix = order_tests.matrix
    ie = IECore(plugin_package='pyopenvino_amd.op_plugins')
    two = ie.read_network(matrix._two_heads(str(tmp_path)), weights=os.path.join(matrix.MODELS, 'mnist.bin'))
    two.set_batch(n)
    ex2 = ie.load_network(two, 'GPU', num_requests=1)
    rows, maps = (out['name'] for out in sorted(two.outputs, key=lambda out: len(out['input'][0]['dims'])))
    whole = ex2.infer({two.inputs[0]['name']: x})
    full2 = np.array(whole[maps], copy=True)
    want2 = _ref(full2, cut)
    for call in range(3):
        ex2.requests[0].start_async({two.inputs[0]['name']: xd}, top_k={rows: 3}, segments={maps: cut})
        assert (ex2.requests[0]._replayed is not None) == (call == 2), call
        got = ex2.requests[0].wait()
        assert isinstance(got[rows], TopK) and isinstance(got[maps], Segments)
        _same(got[maps], want2, 'beside top_k, pass {}'.format(call))
        assert got[rows].indices.shape == (n, 3) and np.array_equal(got[rows].indices[:, 0], np.asarray(whole[rows]).argmax(axis=1))
    with pytest.raises(ValueError, match='segments: Result .* is asked for with keypoints as well'):
        ex2.infer({two.inputs[0]['name']: x}, keypoints=True, segments={maps: True})


@pytest.mark.gpu
def test_the_launch_order_behind_the_pass(hip, tmp_path):
    """What test_answer_checks pins for the other kinds: select, the entry once (its two launches are one call), one event, select;
    wait() makes exactly one copy; no pass after the first allocates -- alone and beside top_k."""
    import test_answer_checks as order_tests
    from pyopenvino_amd import IECore
    n = 2
    x = hip.DeviceTensor.from_numpy(_pixels(20, n))
    ex, _, name, out_name = _mnist_head(tmp_path, n)
    for asked in (dict(segments=True), dict(segments=0.25)):
        got = order_tests._same_answers(order_tests._passes(hip, ex.requests[0], {name: x}, asked, [ENTRY], [1]), out_name)
        assert got.labels.shape == (n, 26, 26) and got.areas.shape == (n, 32) and got.extents.shape == (n, 32, 4)
        ex, _, name, out_name = _mnist_head(tmp_path, n)        # (a request that has not recorded yet)
    matrix = order_tests.matrix
    ie = IECore(plugin_package='pyopenvino_amd.op_plugins')
    net = ie.read_network(matrix._two_heads(str(tmp_path)), weights=os.path.join(matrix.MODELS, 'mnist.bin'))
    net.set_batch(n)
    two = ie.load_network(net, 'GPU', num_requests=1)
    rows, maps = (out['name'] for out in sorted(net.outputs, key=lambda out: len(out['input'][0]['dims'])))
    answers = order_tests._passes(hip, two.requests[0], {net.inputs[0]['name']: x}, dict(top_k={rows: 3}, segments={maps: True}),
                                  ['pvhip_topk_rows_f32', ENTRY], [1, 1])
    assert order_tests._same_answers(answers, rows).indices.shape == (n, 3) and order_tests._same_answers(answers, maps).labels.shape == (n, 26, 26)


@pytest.mark.gpu
def test_requests_in_flight(hip, tmp_path):
    """Two requests at batch 3, three steps, another input every time, the keyword cycling through True, a named threshold and None per
    request and step: all started, then all waited for; every answer is the rule on that input's synchronous single-request Result."""
    B, R, steps = 3, 2, 3
    ex, net, name, out_name = _mnist_head(tmp_path, B, requests=R)
    single, _, _, _ = _mnist_head(tmp_path, B)
    xs = [[_pixels(3000 + 100 * step + 10 * r, B) for r in range(R)] for step in range(steps)]
    fulls = [[np.array(single.infer({name: x})[out_name], copy=True) for x in row] for row in xs]
    assert len({f.tobytes() for row in fulls for f in row}) == R * steps
    kinds = (True, {out_name: 0.5}, None)
    seen = set()
    for step in range(steps):
        asked = [(r + step) % 3 for r in range(R)]
        for r in range(R):
            ex.start_async(r, {name: xs[step][r]}, segments=kinds[asked[r]])
        for r in (reversed(range(R)) if step % 2 else range(R)):
            res = ex.wait(r)[out_name]
            seen.add((r, asked[r]))
            if asked[r] == 2:
                helpers.assert_bit_exact(res, fulls[step][r], 'step {} request {}'.format(step, r))
            else:
                _same(res, _ref(fulls[step][r], 0.5 if asked[r] else None), 'step {} request {} kind {}'.format(step, r, asked[r]))
    assert len(seen) == R * 3                                 # every request gave every kind of answer


@pytest.mark.gpu
def test_cascade_rows_behind_count_are_void(hip, tmp_path):
    """GoogLeNet's first Convolution + bias + ReLU at batch 8 as a segmentation network (8, 64, 112, 112), fed DetectedRois(frames, a
    records array) with fewer survivors than rows: the rows behind `count` are NaN rows and come back all 255 with areas and extents
    zeros; the rows before it are the rule (segments.labels, which the tests above hold to the loops) on the full Result of the same
    feed; and detected_rois() still reads its table afterwards."""
    from pyopenvino_amd import DetectedRois, IECore, segments
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
    assert np.isfinite(full[:want.count]).all() and (full[want.count:].view(np.uint32) == QUIET).all()
    got = req.infer({name: DetectedRois(frames, rec, min_confidence=conf)}, segments=True)[out_name]
    _same(got, segments.labels(full), 'cascade')
    assert (got.labels[:want.count] != 255).all() and (got.areas[:want.count].sum(axis=1) == 112 * 112).all()
    assert (got.labels[want.count:] == 255).all() and not got.areas[want.count:].any() and not got.extents[want.count:].any()
    det_tests._same(req.detected_rois(name), want, 'with segments')
