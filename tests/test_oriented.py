"""``infer(..., boxes=OrientedBoxScreen(...))``: an oriented detector head decoded, screened and suppressed by rotated overlap on the device
(pvhip_oriented_boxes_f32).  tests/oriented_ref.py is the rule in plain loops; pyopenvino_amd/oriented.py (numpy) and the kernels equal
it bit for bit on all seven arrays.  The loops' answer of a case is made once and serves the host test and the device test."""
import functools
import math
import os
import types
from fractions import Fraction

import numpy as np
import pytest

import oriented_ref
import test_boxes as boxes_tests
import test_keypoints as keypoints_tests

NAN, INF, PI4, F = np.float32(np.nan), np.float32(np.inf), np.float32(np.pi / 4), np.float32(9)
ANGLES = np.array([0, PI4, -PI4, np.nextafter(PI4, F), np.nextafter(PI4, -F), -np.nextafter(PI4, F), -np.nextafter(PI4, -F),
                   3 * np.pi / 4, -2.5, 7.9], np.float32)
NET = (256, 256)


def _head(seed, n, A, C, clusters, objectness=False):
    """(n, A, E) anchors in eighths around `clusters` centres of a grid 24 apart, so that clusters never touch, boxes of one cluster nearly
    coincide and scores tie; every score is at least 0.25."""
    rng = np.random.default_rng(seed)
    cell = rng.permutation(100)[:clusters][rng.integers(0, clusters, (n, A))]
    v = np.zeros((n, A, 4 + int(objectness) + C + 1), np.float32)
    v[:, :, 0] = 16 + 24 * (cell % 10) + rng.integers(-8, 9, (n, A)) / 8
    v[:, :, 1] = 16 + 24 * (cell // 10) + rng.integers(-8, 9, (n, A)) / 8
    v[:, :, 2:4] = rng.integers(48, 113, (n, A, 2)) / 8
    v[:, :, 4:-1] = rng.integers(2, 9, (n, A, int(objectness) + C)) / 8
    v[:, :, -1] = ANGLES[rng.integers(0, len(ANGLES), (n, A))]
    return v


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x, layout, the screen's fields with `fit`, the loops' answer) of one case."""
    layout, s = 'NCA', dict(min_score=0.25)
    if name == 'planes odd':                                    # A % 4 != 0; launched one word into a buffer: image 1 at an odd 4-byte phase
        v, s = _head(1, 2, 37, 3, 6), dict(min_score=0.5, frame_size=(1080, 1920), fit=(0, 56, 256, 144))
    elif name.startswith('chunks'):                             # more than 64 kept of the 128 best; the cut below the kept count
        v, s = _head(2, 1, 300, 1, 100), dict(min_score=0.25, max_candidates=128, max_per_image=70 if name.endswith('cut') else None)
    elif name == 'worklist':                                    # the keep buffer cuts; every chunk meets kept boxes of many earlier chunks
        v = _head(3, 1, 1100, 1, 40)
    elif name == 'rows 16':
        layout, v, s = 'NAC', _head(4, 2, 50, 2, 5, True), dict(min_score=0.25, objectness=True)
    elif name == 'rows 64':                                     # E > 128
        layout, v = 'NAC', _head(5, 1, 40, 130, 4)
    else:                                                       # the screen, on one small head
        v = _head(6, 2, 45, 3, 3)
        v[1] = NAN                                              # an all-NaN batch row beside a live one
        v[0, :6, -1] = [NAN, INF, np.nextafter(np.float32(8), F), -8.5, 8, -8]       # the last two are in
        v[0, 6:11, 2] = [NAN, INF, -INF, -4, 0.5]
        v[0, 11, 0], v[0, 12, 4:7] = INF, NAN
        v[0, 13:16, 2:4] = [[6, 7], [np.nextafter(np.float32(6), -F), 7], [6, np.nextafter(np.float32(7), -F)]]
        s = {'ios': dict(overlap='IOS'), 'any label': dict(per_label=False), 'threshold 0': dict(threshold=0.0), 'threshold 1': dict(threshold=1.0),
             'labels': dict(labels=(2, 0, 9)), 'min_size': dict(min_size=(7, 6))}[name[len('screen '):]]
        s = dict(s, min_score=0.25)
    x = boxes_tests._physical(v, layout)
    x.setflags(write=False)
    fields = {k: val for k, val in s.items() if k not in ('min_score', 'frame_size', 'fit')}
    want = oriented_ref.decode(x, layout, s['min_score'], s.get('frame_size') or NET, s.get('fit') or (0, 0, NET[1], NET[0]), **fields)
    return x, layout, s, want


CASES = ['planes odd', 'chunks', 'chunks cut', 'worklist', 'rows 16', 'rows 64'] + ['screen ' + k for k in ('ios', 'any label', 'threshold 0', 'threshold 1', 'labels', 'min_size')]


def _same(got, want, what):
    for field, a, b in zip(want._fields, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, field, a.dtype, a.shape, b.dtype, b.shape)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), '{}: {} differs\n{}\n{}'.format(what, field, a[:2], b[:2])


def _expected(name, want):
    """What the case is there to exercise, seen in the loops' answer alone."""
    if name.startswith('chunks'):
        assert want.selected[0] == 300 and want.counts[0] == (70 if name.endswith('cut') else _case('chunks')[3].counts[0]) and _case('chunks')[3].counts[0] > 70
    elif name == 'worklist':
        assert want.selected[0] == 1100 and 64 < want.counts[0] < 1024
    elif name.startswith('screen'):
        free = _case('screen threshold 1')[3]
        assert want.counts[1] == 0 and want.selected[1] == 0 and 0 < want.counts[0] <= free.counts[0] == free.selected[0]
        assert not set(want.records.tolist()) & {0, 1, 2, 3, 6, 7, 8, 9, 10, 11, 12} and {4, 5} <= set(free.records.tolist())
        if name == 'screen min_size':                           # equality keeps, one step below is out
            assert 13 in want.records and not {14, 15} & set(want.records.tolist())
        elif name not in ('screen threshold 1', 'screen labels'):
            assert want.counts[0] < want.selected[0]
    else:
        assert (0 < want.counts).all() and (want.counts < want.selected).all(), (want.counts, want.selected)


def _screen(layout, s):
    from pyopenvino_amd import OrientedBoxScreen
    return OrientedBoxScreen(layout=layout, **{k: v for k, v in s.items() if k != 'fit'})


@pytest.mark.parametrize('name', CASES)
def test_decode_equals_the_loops(name):
    from pyopenvino_amd import oriented
    x, layout, s, want = _case(name)
    _expected(name, want)
    got = oriented.decode(x, _screen(layout, s), NET, s.get('fit'))
    _same(got, want, name)
    assert all(np.array_equal(a, b[:want.counts[0]]) for a, b in zip(got.of(0), want[2:]))


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_kernels_equal_the_loops(hip, name):
    """The entry as a request launches it, one word into a larger buffer for the odd phase; three calls, the same bits."""
    from pyopenvino_amd import oriented
    x, layout, s, want = _case(name)
    screen = oriented.resolved(_screen(layout, s))
    n, A = x.shape[0], x.shape[2 if layout == 'NCA' else 1]
    odd = int(name == 'planes odd')
    src = hip.DeviceTensor.from_numpy(np.concatenate([np.full(odd, 9e9, np.float32), x.ravel(), np.full(7, 9e9, np.float32)]))
    blocks = oriented.Blocks(n, A, screen._replace(min_score=None, frame_size=None))
    for call in range(3):
        blocks.launch(types.SimpleNamespace(ptr=src.ptr + 4 * odd, shape=x.shape, dtype=x.dtype), screen.min_score, s.get('frame_size') or NET,
                      s.get('fit') or (0, 0, NET[1], NET[0]))
        _same(blocks.read_back(), want, '{} call {}'.format(name, call))


def test_the_rule_s_cosine_and_sine():
    angles = np.concatenate([ANGLES, np.random.default_rng(0).uniform(-8, 8, 1000).astype(np.float32)])
    for a in angles:
        c, s = oriented_ref.cos_sin(a)
        assert abs(c - math.cos(float(a))) <= 1e-15 and abs(s - math.sin(float(a))) <= 1e-15, a
    (p, _), (q, _) = oriented_ref.corners(10, 10, 2, 2, 0), oriented_ref.corners(10, 10, 2, 2, PI4)
    assert abs(oriented_ref.inter(q, p) - 8 * (math.sqrt(2) - 1)) <= 1e-12


def test_the_clip_against_exact_arithmetic():
    rng = np.random.default_rng(1)
    for _ in range(200):
        b = np.concatenate([rng.uniform(20, 44, (2, 2)), rng.uniform(1, 20, (2, 2)), rng.choice(ANGLES, (2, 1))], axis=1).astype(np.float32)
        (p, ai), (q, aj) = oriented_ref.corners(*b[0]), oriented_ref.corners(*b[1])
        assert max(abs(c) for c in np.ravel(p + q)) < 64
        assert abs(Fraction(oriented_ref.inter(p, q)) - oriented_ref.inter(p, q, Fraction)) <= Fraction(1e-9) * Fraction(ai + aj)


@functools.lru_cache(maxsize=None)
def _upright():
    """(1, 80, 4 + 2 + 1) 'NAC' boxes on integer pixel edges with angle 0; no pair's IoU, by the loops' own clip, within 1e-6 of 0.45."""
    rng = np.random.default_rng(2)
    v = np.zeros((1, 80, 7), np.float32)
    lo, wh = rng.integers(0, 40, (80, 2)), 2 * rng.integers(2, 12, (80, 2))
    v[0, :, :2], v[0, :, 2:4], v[0, :, 4:6] = lo + wh / 2, wh, rng.integers(2, 9, (80, 2)) / 8
    quads = [oriented_ref.corners(*row[[0, 1, 2, 3, 6]]) for row in v[0]]
    for i, (p, ai) in enumerate(quads):
        for q, aj in quads[:i]:
            both = oriented_ref.inter(p, q)
            assert abs(both / (ai + aj - both) - 0.45) > 1e-6
    return v


def test_upright_boxes_keep_what_boxscreen_keeps():
    from pyopenvino_amd import BoxScreen, OrientedBoxScreen, boxes, oriented
    v = _upright()
    got = oriented.decode(v, OrientedBoxScreen(0.25, 'NAC'), (64, 64))
    plain = boxes.decode(np.ascontiguousarray(v[:, :, :6]), BoxScreen(0.25, 'NAC'), (64, 64))
    assert np.array_equal(got.records, plain.records) and 1 < got.counts[0] < got.selected[0] == plain.selected[0]
    assert np.array_equal(got.quads[:, 0], plain.rois[:, 1:3]) and np.array_equal(got.quads[:, 2] - got.quads[:, 0], plain.rois[:, 3:5])


def _bad(out_name, n):
    """(what the refusal says, the arguments[, the dims the Result is declared with for this start])."""
    from pyopenvino_amd import OrientedBoxScreen
    good = OrientedBoxScreen(layout='NCA')
    yield 'max_candidates of an OrientedBoxScreen is a count in 1 .. 1024', dict(boxes=good._replace(max_candidates=1025))
    yield 'max_per_image is None or a count in 1 .. max_candidates = 8', dict(boxes=good._replace(max_candidates=8, max_per_image=9))
    for field, bad in (('min_score', NAN), ('layout', 'ACN'), ('objectness', 1), ('frame_size', (0, 8)), ('labels', tuple(range(65))), ('min_size', (0, 1)),
                       ('overlap', 'GIOU'), ('threshold', 1.5), ('per_label', None), ('input', 'nope')):
        yield field, dict(boxes={out_name: good._replace(**{field: bad})})
    yield 'no Result named', dict(boxes={'nope': good})
    yield 'reads as \'NCA\' and as \'NAC\'', dict(boxes={out_name: OrientedBoxScreen()}), (n, 32, 32)
    yield 'has shape', dict(boxes={out_name: good}), (n, 32, 26, 26)
    yield 'asked for with text as well', dict(boxes={out_name: good}, text={out_name: True})
    yield 'masks= takes the boxes of a BoxScreen', dict(boxes={out_name: good}, masks=True)
    yield 'is fed a RoiInput', dict(boxes=good)                 # (the input is made to declare a fit below)


def test_refusals_and_the_host_route(tmp_path):
    """Every refusal is a ValueError('boxes: ...') before anything is staged; a plugin set that computes on the host gets the numpy rule;
    a BoxScreen under the same keyword keeps its own kind."""
    from pyopenvino_amd import BoxScreen, Detections, OrientedBoxScreen, OrientedDetections, RoiInput, oriented
    n = 2
    ex, net, name, out_name = boxes_tests._head(tmp_path, n, package='oracle.op_plugins')
    x, req, formats = keypoints_tests._pixels(10, n), ex.requests[0], ex.host_inputs.formats
    port = next(iter(ex.ienet.G.nodes[[nid for nid, result in ex.ienet.find_node_by_type('Result') if result == out_name][0]]['input'].values()))
    for match, kw, *dims in _bad(out_name, n):
        kept, fed, saved = port['dims'], x, dict(formats)
        port['dims'] = dims[0] if dims else kept
        if 'RoiInput' in match:
            formats[name] = types.SimpleNamespace(fitted=True, fit='LETTERBOX')
            fed = RoiInput(np.zeros((n, 28, 28, 1), np.uint8), np.array([[0, 0, 0, 20, 20]] * n, np.int32))
        try:
            with pytest.raises(ValueError, match=match) as e:
                ex.infer({name: fed}, **kw)
        finally:
            port['dims'] = kept
            formats.clear()
            formats.update(saved)
        assert str(e.value).startswith('boxes: '), str(e.value)
        assert not req._in_flight and not req._asks and not ex.answers.blocks and not ex.host_inputs.slots
    with pytest.raises(ValueError, match='boxes: not with a batch sharded'):
        oriented.checked(ex.ienet, OrientedBoxScreen(layout='NCA'), True)
    x = x * np.float32(64)                                      # (the head's numbers are small: some of its boxes are a pixel wide now)
    full = np.array(ex.infer({name: x})[out_name], copy=True)
    screen = OrientedBoxScreen(0.0, 'NCA', max_candidates=64, threshold=0.2)
    got = ex.infer({name: x}, boxes=screen)[out_name]
    assert isinstance(got, OrientedDetections) and got.counts.min() > 0
    _same(got, oriented_ref.decode(full, 'NCA', 0.0, (28, 28), (0, 0, 28, 28), max_candidates=64, threshold=0.2), 'host route')
    assert isinstance(ex.infer({name: x}, boxes={out_name: BoxScreen(0.5, 'NCA')})[out_name], Detections)


@pytest.mark.gpu
def test_letterboxed_frames_give_quads_in_frame_pixels(hip, tmp_path):
    """The head behind a U8 / NHWC input that declares 'LETTERBOX', fed host frames: the quads go through the geometry of the frames fed;
    frame_size None is their extent; eager and replayed passes answer alike."""
    from pyopenvino_amd import IECore, OrientedBoxScreen, OrientedDetections
    from pyopenvino_amd.input_format import fit_geometry
    n = 2
    boxes_tests._head(tmp_path, n)                              # writes the IR
    ie = IECore(plugin_package=keypoints_tests.HIP)
    net = ie.read_network(os.path.join(str(tmp_path), 'mnist_text_ntc.xml'), weights=os.path.join(str(tmp_path), 'mnist_text_ntc.bin'))
    net.set_batch(n)
    name, info = net.inputs[0]['name'], net.input_info[net.inputs[0]['name']]
    info.precision, info.layout = 'U8', 'NHWC'
    info.preprocess_info.resize_algorithm, info.preprocess_info.resize_fit = 'RESIZE_BILINEAR', 'LETTERBOX'
    info.preprocess_info.init(1)
    info.preprocess_info[0].std_scale = 1 / 64                  # pixels in 0 .. 16320: some of the head's boxes are a pixel wide
    info.preprocess_info.mean_variant = 'MEAN_VALUE'
    req = ie.load_network(net, 'GPU', num_requests=1).requests[0]
    frames = np.random.default_rng(8).integers(0, 256, (n, 540, 560, 1), dtype=np.uint8)
    full = np.array(req.infer({name: frames})['text'], copy=True)
    fit = fit_geometry((540, 560), (28, 28), 'LETTERBOX')
    for frame in (None, (28000, 28000)):
        want = oriented_ref.decode(full, 'NCA', 0.0, frame or (540, 560), fit, max_candidates=64, threshold=0.2)
        for call in range(3):
            got = req.infer({name: frames}, boxes=OrientedBoxScreen(0.0, 'NCA', frame_size=frame, max_candidates=64, threshold=0.2))['text']
            assert isinstance(got, OrientedDetections) and got.counts.sum() > 0
            _same(got, want, 'frame {} call {}'.format(frame, call))
    assert fit != (0, 0, 28, 28) and len(req.runner.answers.blocks) == 1
