"""``infer(..., boxes=...)``: a dense detector head's raw tensor decoded, screened and suppressed on the device (pvhip_dense_boxes_f32).
tests/boxes_ref.py is the rule in plain loops; pyopenvino_amd/boxes.py (numpy) and the kernels equal it bit for bit."""
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest

import boxes_ref
import helpers
import test_keypoints as keypoints_tests
import test_text as text_tests
import test_top_k as top_k_tests

ENTRY, FORM = 'pvhip_dense_boxes_f32', 'pvhip_dense_boxes_form'
LAYOUTS = ('NCA', 'NAC')                                # PVHIP_BOXES_LAYOUT_* 0, 1
BOXES = ('CXCYWH', 'XYXY')                              # PVHIP_BOXES_* 0, 1
OVERLAPS = ('IOU', 'IOS')                               # PVHIP_OVERLAP_* 0, 1
FORM_NONE, FORM_PLANES, FORM_ROWS_TEAM, FORM_ROWS_WAVE = 0, 1, 2, 3
NAN, INF = np.float32(np.nan), np.float32(np.inf)
NET = (64, 64)                                          # the extent the fillings' box numbers stand in

# (n, C, A): the smallest at which each mechanism can go wrong -- one anchor; a few; C around the planes form's trip of four classes; A
# around a wave and around a lane's four anchors, and beyond a workgroup's 1024; a head of real proportions.  From A = 64 on there are
# three images, the last of them empty.
SHAPES = [(1, 1, 1), (2, 3, 5), (3, 1, 64), (3, 3, 63), (3, 4, 65), (3, 5, 255), (3, 9, 256), (3, 4, 257), (3, 3, 1025), (3, 80, 2100)]
LONG = (3, 80, 2100)                                    # fewer fillings: the loops of the reference take a while on it


def _physical(v, layout):
    """The logical (n, A, E) array as a contiguous tensor of `layout`."""
    return np.ascontiguousarray(v.transpose(0, 2, 1)) if layout == 'NCA' else np.ascontiguousarray(v)


def _same(got, want, what=''):
    assert np.array_equal(got.counts, want.counts), (what, got.counts, want.counts)
    assert np.array_equal(got.selected, want.selected), (what, got.selected, want.selected)
    for field in ('rois', 'labels', 'records'):
        a, b = getattr(got, field), getattr(want, field)
        assert a.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b), (what, field, a[:8], b[:8])
    assert got.scores.dtype == np.float32 and np.array_equal(got.scores.view(np.uint32), want.scores.view(np.uint32)), (what, 'scores')
    assert got.rois.shape == (int(got.counts.sum()), 5)


def _ref(x, layout, s):
    """boxes_ref on `x` for the screen `s`, a dict of BoxScreen's fields with `frame_size` and `fit` (None: the identity over NET)."""
    s = dict(s)
    frame, fit = s.pop('frame_size', None) or NET, s.pop('fit', None) or (0, 0, NET[1], NET[0])
    return boxes_ref.decode(x, layout, s.pop('min_score', 0.25), frame, fit, **s)


def _screen(layout, s):
    from pyopenvino_amd import BoxScreen
    s = {k: v for k, v in s.items() if k != 'fit'}
    return BoxScreen(layout=layout, **s)


# ---------------------------------------------------------------------------------------------------------------- the fillings
def _boxes(rng, n, A, xyxy=False):
    """(n, A, 4) boxes of 10 .. 16 pixels around a few centres of a 64 x 64 extent, so that many of them overlap and many do not."""
    centres = rng.integers(8, 56, (6, 2)).astype(np.float32)
    c = centres[rng.integers(0, 6, (n, A))] + rng.integers(-2, 3, (n, A, 2)).astype(np.float32) * np.float32(0.75)
    wh = rng.integers(10, 17, (n, A, 2)).astype(np.float32)
    if xyxy:
        return np.concatenate([c - wh / 2, c + wh / 2], axis=2).astype(np.float32)
    return np.concatenate([c, wh], axis=2).astype(np.float32)


def _fillings(shape):
    """[(what, v (n, A, E) float32, screen fields)] for (n, C, A).  The last image of three is empty under every screen."""
    n, C, A = shape
    rng = np.random.default_rng(1000 * A + C)
    out = []

    def head(scores, obj=None, xyxy=False):
        parts = [_boxes(rng, n, A, xyxy)] + ([obj[:, :, None]] if obj is not None else []) + [scores]
        v = np.concatenate(parts, axis=2).astype(np.float32)
        if n == 3:
            v[2, :, 4:] = np.minimum(v[2, :, 4:], np.float32(0.125))                 # below every min_score used here
        return v

    peak = (rng.random((n, A, 1)) ** 0.5).astype(np.float32)                         # an anchor's best score: three quarters pass 0.25
    normal = (peak * rng.random((n, A, C)) * 0.875).astype(np.float32)
    np.put_along_axis(normal, rng.integers(0, C, (n, A, 1)), peak, axis=2)
    caps = dict(min_score=0.25, max_candidates=32, max_per_image=5) if A >= 64 else dict(min_score=0.25)
    out.append(('normal', head(normal), caps))
    obj = rng.random((n, A)).astype(np.float32)
    obj[:, ::7] = 0
    with_inf = normal.copy()
    with_inf[:, ::14, 0] = INF                                                       # 0 * inf: a NaN score; inf alone: the best score there is
    with_inf[:, 3::14, C - 1] = INF
    out.append(('objectness', head(with_inf, obj), dict(min_score=0.125, objectness=True)))
    out.append(('infinite scores', head(with_inf), dict(min_score=0.5, per_label=False)))
    levels = np.array([0.2, 0.5, 0.7, 0.9], np.float32)[rng.integers(0, 4, (n, A, C))]
    out.append(('four levels', head(levels), dict(min_score=0.5, max_candidates=48, threshold=0.3)))
    nans = normal.copy()
    kinds = np.array([0x7FC00000, 0xFFC00001, 0x7F800001], np.uint32).view(np.float32)   # quiet, negative with a payload, signalling
    where = rng.random((n, A, C)) < 0.1
    nans[where] = kinds[rng.integers(0, 3, int(where.sum()))]
    v = head(nans)
    out.append(('NaNs scattered', v, dict(min_score=0.25)))
    if shape == LONG:
        return out
    out.append(('all equal', head(np.full((n, A, C), 0.625, np.float32)), dict(min_score=0.625, max_candidates=16, overlap='IOS')))
    zeros = np.array([0.0, -0.0, -0.5], np.float32)[rng.integers(0, 3, (n, A, C))]
    vz = head(zeros)
    if n == 3:
        vz[2, :, 4:] = -1
    out.append(('signed zeros', vz, dict(min_score=-0.0, threshold=0.6)))
    v = head(normal)
    v[0] = NAN                                                                       # (a cascade's row behind `count`)
    out.append(('one image all NaN', v, dict(min_score=0.25)))
    v = head(normal)
    bad = np.array([INF, -INF, NAN, -20.0, 3e38], np.float32)
    at = rng.random((n, A)) < 0.4
    col = rng.integers(0, 4, (n, A))
    for r, a in zip(*np.nonzero(at)):
        v[r, a, col[r, a]] = bad[(r + a) % 5]                                        # non-finite numbers, negative extents, overflowing corners
    out.append(('bad boxes', v, dict(min_score=0.25)))
    v = head(normal, xyxy=True)
    v[:, 1::5, [0, 2]] = v[:, 1::5, [2, 0]]                                          # inverted
    out.append(('XYXY', v, dict(min_score=0.25, box='XYXY', min_size=(12, 11))))
    out.append(('labels', head(normal), dict(min_score=0.25, labels=(0, C - 1, 7), frame_size=(1080, 1920), fit=(0, 14, 64, 36))))
    return out


@functools.lru_cache(maxsize=None)
def _cases(shape):
    """[(what, layout, x, screen fields, the reference's answer)]: every filling in both layouts, computed once and shared by the tests.
    For A >= 64 the fixture asserts that the reference screens some anchors out and some in, suppresses some and keeps some, leaves an
    image empty and that a cap bites: a kernel that drops nothing, or everything, cannot pass."""
    n, C, A = shape
    cases = []
    for what, v, s in _fillings(shape):
        want = None
        for layout in LAYOUTS:
            x = _physical(v, layout)
            x.setflags(write=False)
            got = _ref(x, layout, s)
            if want is not None:
                _same(got, want, 'the reference on both layouts: ' + what)
            want = got
            cases.append((what, layout, x, s, want))
        if A >= 64 and what == 'normal':
            K, cap = s['max_candidates'], s['max_per_image']
            assert (want.selected > 0).any() and (want.selected[:2] < A).all(), (shape, want.selected)            # some in, some out
            assert want.selected[2] == 0 and want.counts[2] == 0, (shape, want.selected)                          # an empty image
            assert (want.selected > K).any(), (shape, want.selected)                                              # the candidates' cap bites
            free = _ref(_physical(v, 'NAC'), 'NAC', dict(s, max_per_image=None))
            assert ((free.counts > 1) & (free.counts < np.minimum(free.selected, K))).any(), (shape, free.counts)  # some suppressed, some kept
            assert (free.counts > cap).any() and (want.counts == cap).any(), (shape, free.counts)                 # the image's cap bites
    return cases


# ---------------------------------------------------------------------------------------------------------------- without a GPU
@pytest.mark.parametrize('shape', SHAPES)
def test_decode_agrees_with_the_loops(shape):
    from pyopenvino_amd import boxes
    for what, layout, x, s, want in _cases(shape):
        screen = _screen(layout, s)
        got = boxes.decode(x, screen, NET, s.get('fit'))
        _same(got, want, '{} {}'.format(what, layout))
        if shape[2] > 4 + int(s.get('objectness', False)) + shape[1]:                 # more anchors than channels: the layout is inferred
            _same(boxes.decode(x, screen._replace(layout=None), NET, s.get('fit')), want, what + ' inferred')
        for b in range(shape[0]):                                                    # of() slices the table
            rows = slice(int(got.counts[:b].sum()), int(got.counts[:b + 1].sum()))
            assert np.array_equal(got.of(b)[0], want.rois[rows]) and (got.of(b)[0][:, 0] == b).all()


def _designed():
    """(x as 'NAC' (1, 8, 6) 'XYXY' on an 8 x 8 network and frame, {what: (screen fields, the records kept)})."""
    v = np.array([[[0, 0, 2, 2, 0.9, 0.1],            # 0
                   [0, 0, 2, 1, 0.8, 0.2],            # 1: half of 0; IoU 2 / 4 = 0.5 exactly, IoS 1
                   [0, 0, 2, 2, 0.1, 0.7],            # 2: 0 again, of the other class
                   [2, 0, 4, 2, 0.6, 0.0],            # 3: touches 0, no overlap
                   [1, 1, 3, 3, 0.5, 0.0],            # 4: one pixel of 0 (IoU 1 / 7) and one of 3
                   [4, 4, 8, 8, 0.4, 0.3],            # 5: alone
                   [5, 5, 7, 7, 0.35, 0.0],           # 6: inside 5: IoU 4 / 16, IoS 1
                   [0, 0, 2, 2, 0.3, 0.0]]], np.float32)   # 7: 0 once more
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    base = dict(min_score=0.25, box='XYXY', frame_size=(8, 8), fit=(0, 0, 8, 8))
    return v, {
        'overlap equal to threshold * den keeps': (dict(base, threshold=0.5), [0, 1, 2, 3, 4, 5, 6]),
        'just above it suppresses': (dict(base, threshold=below), [0, 2, 3, 4, 5, 6]),
        'across labels': (dict(base, threshold=0.5, per_label=False), [0, 1, 3, 4, 5, 6]),
        'IOS': (dict(base, threshold=0.5, overlap='IOS'), [0, 2, 3, 4, 5]),
        'IOS across labels': (dict(base, threshold=0.5, overlap='IOS', per_label=False), [0, 3, 4, 5]),
        'threshold 0': (dict(base, threshold=0.0), [0, 2, 3, 5]),
        'threshold 1': (dict(base, threshold=1.0), [0, 1, 2, 3, 4, 5, 6, 7]),
        'max_per_image': (dict(base, threshold=1.0, max_per_image=3), [0, 1, 2]),
        'max_candidates': (dict(base, threshold=1.0, max_candidates=2), [0, 1]),
        'labels []': (dict(base, labels=()), []),
        'one label': (dict(base, threshold=1.0, labels=(1,)), [2]),
        'min_size': (dict(base, threshold=1.0, min_size=(2, 3)), [5]),
    }


def test_designed_suppression_cases_by_hand():
    from pyopenvino_amd import boxes
    v, cases = _designed()
    for what, (s, kept) in cases.items():
        for layout in LAYOUTS:
            x = _physical(v, layout)
            want = _ref(x, layout, s)
            assert want.records.tolist() == kept, (what, want.records)
            _same(boxes.decode(x, _screen(layout, s), (8, 8), s['fit']), want, what)
    want = _ref(v, 'NAC', cases['threshold 1'][0])
    assert want.rois.tolist()[4] == [0, 1, 1, 2, 2] and want.labels.tolist() == [0, 0, 1, 0, 0, 0, 0, 0] and want.selected.tolist() == [8]
    assert cases['max_candidates'][0]['max_candidates'] < want.selected[0]


def _grid(A=150, dup=60):
    """(1, A + dup, 5) 'NAC' 'CXCYWH': A anchors each in a 4 x 4 cell of its own of a 64 x 64 frame, then `dup` of them again with lower
    scores: more than 64 are kept, and the later ones are suppressed by kept ones of earlier chunks."""
    rng = np.random.default_rng(5)
    cells = rng.permutation(256)[:A]
    cells = np.concatenate([cells, cells[rng.permutation(A)[:dup]]])
    v = np.zeros((1, A + dup, 5), np.float32)
    v[0, :, 0], v[0, :, 1], v[0, :, 2:4] = 4 * (cells % 16) + 2, 4 * (cells // 16) + 2, 4
    v[0, :A, 4] = rng.permutation(A) / np.float32(A) * 0.5 + 0.5
    v[0, A:, 4] = rng.permutation(dup) / np.float32(dup) * 0.25 + 0.25
    return v


def _crowd(A=5000):
    """(1, A, 6) 'NAC': every anchor passes, 40 distinct boxes, two classes."""
    rng = np.random.default_rng(6)
    v = np.zeros((1, A, 6), np.float32)
    cell = rng.integers(0, 40, A)
    v[0, :, 0], v[0, :, 1], v[0, :, 2:4] = 8 * (cell % 8) + 4, 8 * (cell // 8) + 4, 8
    v[0, :, 4:] = rng.integers(1, 4096, (A, 2)) / np.float32(4096)                   # many ties
    return v


def _edges():
    """(1, 40, 5) 'NAC' 'XYXY' boxes on integer pixel edges of a 637 x 481 network."""
    rng = np.random.default_rng(7)
    v = np.zeros((1, 40, 5), np.float32)
    v[0, :, 0], v[0, :, 1] = rng.integers(0, 600, 40), rng.integers(0, 450, 40)
    v[0, :, 2], v[0, :, 3] = v[0, :, 0] + rng.integers(1, 37, 40), v[0, :, 1] + rng.integers(1, 31, 40)
    v[0, :, 4] = 0.5 + np.arange(40) / np.float32(128)
    return v


def test_integer_edges_come_back_on_those_edges():
    from pyopenvino_amd import BoxScreen, boxes
    v = _edges()
    got = boxes.decode(v, BoxScreen(0.25, 'NAC', box='XYXY', threshold=1.0), (481, 637))
    assert got.counts.tolist() == [40]
    want = v[0, got.records, :4].astype(np.int64)
    assert np.array_equal(got.rois[:, 1:3], want[:, :2]) and np.array_equal(got.rois[:, 1:3] + got.rois[:, 3:5], want[:, 2:])
    _same(got, boxes_ref.decode(v, 'NAC', 0.25, (481, 637), (0, 0, 637, 481), box='XYXY', threshold=1.0))
    # the float32 route p / Wn * Wn moves some of these corners across an edge: why the rule is binary64
    moved = np.floor(v[0, :, 0] / np.float32(637) * np.float32(637)) != v[0, :, 0]
    moved |= np.ceil(v[0, :, 2] / np.float32(637) * np.float32(637)) != v[0, :, 2]
    assert moved.any()


def test_layout_inference():
    from pyopenvino_amd import boxes
    assert boxes.shape_of((4, 84, 8400)) == ('NCA', 4, 8400, 80) and boxes.shape_of((4, 25200, 85), None, True, 4) == ('NAC', 4, 25200, 80)
    assert boxes.shape_of((4, 84, 8400), 'NAC') == ('NAC', 4, 84, 8396) and boxes.shape_of((4, 6, 2100), None, True) == ('NCA', 4, 2100, 1)
    assert boxes.shape_of((4, 4, 100)) is None and boxes.shape_of((4, 5, 100), None, True) is None and boxes.shape_of((4, 5, 100)) == ('NCA', 4, 100, 1)
    assert boxes.shape_of((4, 84, 8400), None, False, 5) is None and boxes.shape_of((4, 84)) is None and boxes.shape_of((4, 84, 8400, 1)) is None
    assert boxes.shape_of((1, 1 << 15, 1 << 16), 'NAC') is None and boxes.shape_of((1, (1 << 15) - 1, 1 << 16), 'NAC') is not None
    assert boxes.shape_of((4, 0, 9), 'NAC') is None
    with pytest.raises(boxes.AmbiguousLayout, match='reads as \'NCA\' and as \'NAC\''):
        boxes.shape_of((4, 84, 84))
    assert boxes.shape_of((4, 84, 84), 'NCA') == ('NCA', 4, 84, 80)
    with pytest.raises(ValueError, match='decode: shape .* reads as'):
        boxes.decode(np.zeros((1, 6, 6), np.float32), True, NET)
    for bad in (np.zeros((1, 4, 9), np.float32), np.zeros((1, 6, 9), np.float64), np.zeros((6, 9), np.float32)):
        with pytest.raises(ValueError, match='decode takes float32'):
            boxes.decode(bad, 0.5, NET)
    for bad in ((1, 2, 3), (0, 0, 0, 4), (0, 0, 4.0, 4), (-1, 0, 4, 4), 'fit'):
        with pytest.raises(ValueError, match='decode: fit is'):
            boxes.decode(np.zeros((1, 6, 9), np.float32), 0.5, NET, bad)


def _head(tmp_path, n, requests=1, package=keypoints_tests.HIP):
    """mnist's first Convolution + bias + ReLU reshaped to the rank-3 Result 'text' (n, 32, 676), the IR tests/test_text.py writes: as
    'NCA' 676 anchors of 28 classes, as 'NAC' 32 anchors of 672."""
    return text_tests._text_head(tmp_path, n, requests=requests, package=package)


def test_argument_rules(tmp_path, monkeypatch):
    """Every refusal is a ValueError('boxes: ...') raised before anything is staged or launched: this test runs where there is no device."""
    from pyopenvino_amd import BoxScreen, Gallery, GalleryMatch, RoiInput, TextScreen, answers as answers_module, boxes as rule, detections as detections_rule
    n = 4
    ex, net, name, out_name = _head(tmp_path, n, requests=2)
    x = np.zeros((n, 1, 28, 28), np.float32)
    req = ex.requests[0]
    others = ('top_k', 'detections', 'matches', 'keypoints', 'segments', 'maxima', 'text')
    starts = (lambda s, **kw: ex.infer({name: x}, boxes=s, **kw), lambda s, **kw: req.start_async({name: x}, boxes=s, **kw),
              lambda s, **kw: ex.requests[1].infer({name: x}, boxes=s, **kw), lambda s, **kw: ex.start_async(1, {name: x}, boxes=s, **kw),
              lambda s, **kw: req.infer({name: x}, *(kw.get(k) for k in others), s),
              lambda s, **kw: req.start_async({name: x}, *(kw.get(k) for k in others), s),
              lambda s, **kw: ex.infer({name: x}, False, *(kw.get(k) for k in others), s),
              lambda s, **kw: ex.start_async(0, {name: x}, *(kw.get(k) for k in others), s))       # the keyword stands last

    def refused(match, s, network=ex, starts=starts, **kw):
        for start in starts:
            with pytest.raises(ValueError, match=match) as e:
                start(s, **kw)
            assert str(e.value).startswith('boxes: '), str(e.value)
        for r in network.requests:
            assert not r._in_flight and not r._asks and not r.runner.answers.blocks and not r.runner.host_inputs.slots and r.runner._pending is None

    refused('no Result named', {'nope': True})
    refused('no Result named', {out_name: True, 'nope': BoxScreen()})
    for bad in ('NCA', [True], (True,), False, np.bool_(True), b'1', BoxScreen, None):
        refused('a BoxScreen, a min_score or True', {out_name: bad})
        if bad is not None:
            refused('a BoxScreen, a min_score or True', bad)
    for bad in (NAN, INF, 1e39, '1', None, True):
        refused('min_score is', BoxScreen(bad))
    refused('min_score is', float('nan'))
    for bad in ('ACN', 'nca', 1, b'NCA'):
        refused('layout', BoxScreen(layout=bad))
    for field, message, bads in (('objectness', 'objectness is a bool', (1, 0, None, 'yes')), ('box', 'box is \'CXCYWH\' or \'XYXY\'', ('xyxy', 'XYWH', 0, None)),
                                 ('frame_size', 'frame_size is None or \\(H, W\\)', ((0, 8), (8,), 8, (8, 8.0), (1 << 25, 8), (True, 8))),
                                 ('labels', 'labels is None or at most 64 ints', (tuple(range(65)), (0.5,), 3, (True,), (1 << 31,))),
                                 ('min_size', 'min_size is \\(h, w\\)', ((0, 1), (1,), 1, None, (1.0, 1))),
                                 ('max_candidates', 'max_candidates is a count in 1 .. 4096', (0, 4097, -1, None, 1.0, True)),
                                 ('overlap', 'overlap is \'IOU\' or \'IOS\'', ('iou', 'GIOU', 0, None)),
                                 ('threshold', 'threshold .* is not a finite number in \\[0, 1\\]', (-0.1, 1.5, NAN, None, True, '0.5')),
                                 ('per_label', 'per_label is a bool', (1, None, 'no')),
                                 ('max_per_image', 'max_per_image is None or a count in 1 .. max_candidates = 1024', (0, 1025, -3, 2.0, True)),
                                 ('input', 'input .* is no 4-D Parameter of the network', ('nope', 3, out_name))):
        for bad in bads:
            refused(message, BoxScreen(layout='NCA', **{field: bad}))
            refused(message, {out_name: BoxScreen(layout='NCA', **{field: bad})})
    refused('max_per_image is None or a count in 1 .. max_candidates = 8', BoxScreen(max_candidates=8, max_per_image=9))
    ex.comm = types.SimpleNamespace(world=2, rank=0)
    try:
        refused('sharded', True)
        refused('sharded', {out_name: BoxScreen(0.5)})
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

    def with_dims(dims):
        for port in ports:
            port['dims'] = dims

    try:
        # another rank, another batch, no class, n * A * E = 2^31
        for dims in ((n, 32), (n, 32, 26, 26), (2, 32, 676), (n, 4, 676), (n, 1 << 14, 1 << 15)):
            with_dims(dims)
            refused('has shape .*: not rank 3 with the batch n = 4 first, E = 4 \\+ objectness \\+ C channels, C >= 1 and n \\* A \\* E < 2\\^31', {out_name: True})
            refused('no FP32 Result', True)
        with_dims((n, 5, 676))                                  # one class, but none with an objectness column
        assert rule.checked(ex.requests[0].runner.ienet, True, False)[out_name].layout == 'NCA'
        refused('has shape', {out_name: BoxScreen(objectness=True)})
        refused('no FP32 Result', BoxScreen(objectness=True))
        refused('has shape .* as \'NCA\'', {out_name: BoxScreen(layout='NCA', objectness=True)})
        with_dims((n, 676, 676))
        refused('reads as \'NCA\' and as \'NAC\': say which with BoxScreen\\(layout=...\\)', {out_name: True})
        refused('no FP32 Result .* whose layout can be inferred', 0.5)
        assert rule.checked(ex.requests[0].runner.ienet, BoxScreen(layout='NAC'), False)[out_name].layout == 'NAC'
        # the shapes the issue names
        for dims, objectness, want in (((n, 84, 8400), False, 'NCA'), ((n, 25200, 85), True, 'NAC'), ((n, 6, 2100), True, 'NCA')):
            with_dims(dims)
            got = rule.checked(ex.requests[0].runner.ienet, BoxScreen(objectness=objectness), False)
            assert got == {out_name: rule.resolved(BoxScreen(objectness=objectness))._replace(layout=want, input=name)}
        # one Result under two keywords: the later keyword speaks and names the earlier.  (n, 32, 676) is 32 timesteps too; no Result
        # passes the shape rules of the other six, so their checks are stubbed
        with_dims((n, 32, 676))
        clash = 'Result {!r} is asked for with {} as well'
        for value in (True, {out_name: TextScreen(0)}):
            refused(clash.format(out_name, 'text'), True, text=value)
            refused(clash.format(out_name, 'text'), {out_name: BoxScreen(0.5)}, text=value)
        gal = Gallery(np.ones((3, 7), np.float32))
        stubs = (('top_k', answers_module.top_k_rule, lambda ienet, top_k, sharded: {out_name: 1}, 1),
                 ('detections', answers_module.detections_rule, lambda ienet, d, sharded: {out_name: detections_rule.resolved(0.5, 100, (28, 28))}, 0.5),
                 ('matches', answers_module.gallery_rule, lambda ienet, matches, sharded: {out_name: GalleryMatch(gal, 1, None)}, gal),
                 ('keypoints', answers_module.keypoints_rule, lambda ienet, v, sharded: {out_name: answers_module.keypoints_rule.resolved(True)}, True),
                 ('segments', answers_module.segments_rule, lambda ienet, v, sharded: {out_name: answers_module.segments_rule.resolved(True)}, True),
                 ('maxima', answers_module.maxima_rule, lambda ienet, v, sharded: {out_name: answers_module.maxima_rule.resolved(True)}, True))
        for keyword, module, stub, value in stubs:
            with monkeypatch.context() as patched:
                patched.setattr(module, 'checked', stub)
                refused(clash.format(out_name, keyword), True, **{keyword: value})
                refused(clash.format(out_name, keyword), {out_name: BoxScreen(0.5)}, **{keyword: value})
        assert gal._dev is None
    finally:
        for port, dims in zip(ports, declared):
            port['dims'] = dims
    # no 4-D Parameter, or several without input=
    params = [(r.runner.ienet, nid) for r in ex.requests for nid, _ in r.runner.ienet.find_node_by_type('Parameter')]
    shapes = [g.G.nodes[nid]['data']['shape'] for g, nid in params]
    try:
        for g, nid in params:
            g.G.nodes[nid]['data']['shape'] = list(shapes[0])[:3]
        refused('the network has 0 4-D Parameters', True)
        refused('the network has 0 4-D Parameters', {out_name: BoxScreen(0.5)})
    finally:
        for (g, nid), shape in zip(params, shapes):
            g.G.nodes[nid]['data']['shape'] = shape
    # a classifier has no anchors
    import test_roi_input as roi_tests
    ie_c, net_c, name_c = roi_tests._net('mnist', n)
    cls = ie_c.load_network(net_c, 'GPU', num_requests=1)
    cls_starts = (lambda s, **kw: cls.infer({name_c: x}, boxes=s), lambda s, **kw: cls.requests[0].start_async({name_c: x}, boxes=s))
    refused('no FP32 Result', True, cls, cls_starts)
    refused('has shape', {net_c.outputs[0]['name']: True}, cls, cls_starts)
    # the resolved forms
    default = rule.resolved(True)
    assert BoxScreen() == (0.25, None, False, 'CXCYWH', None, None, (1, 1), 1024, 'IOU', 0.45, True, None, None)
    assert default == rule.resolved(0.25) == rule.resolved(BoxScreen()) and default.max_per_image == 1024 and default.threshold == float(np.float32(0.45))
    assert rule.checked(net, None, False) == {} and rule.checked(net, {}, True) == {}
    assert rule.checked(net, True, False) == rule.checked(net, {out_name: 0.25}, False) == {out_name: default._replace(layout='NCA', input=name)}
    got = rule.checked(net, BoxScreen(np.float32(0.5), 'NAC', np.bool_(True), labels=[np.int64(3)], min_size=[2, 3], frame_size=np.array([9, 8]),
                                      max_candidates=np.int32(7), threshold=1, input=name), False)[out_name]
    assert got == (0.5, 'NAC', True, 'CXCYWH', (9, 8), (3,), (2, 3), 7, 'IOU', 1.0, True, 7, name)
    assert type(got.objectness) is bool and type(got.max_candidates) is int and type(got.threshold) is float and type(got.labels[0]) is int


def test_answers_checked_takes_the_new_argument_last(tmp_path):
    from pyopenvino_amd import BoxScreen, boxes as rule
    n = 4
    ex, net, name, out_name = _head(tmp_path, n)
    x = np.zeros((n, 1, 28, 28), np.float32)
    answers = ex.answers
    assert answers.checked({name: x}, None, None, False) == {} and answers.checked({name: x}, None, None, False, None, None, None, None, None) == {}
    assert answers.checked({name: x}, None, None, False, None, None, None, None, None, None) == {} and answers.checked({name: x}, None, None, False, boxes=None) == {}
    asks = answers.checked({name: x}, None, None, False, None, None, None, None, None, BoxScreen(0.5, 'NCA', max_per_image=9))
    screen = rule.resolved(BoxScreen(0.5, 'NCA', max_per_image=9))._replace(input=name)
    assert set(asks) == {out_name} and isinstance(asks[out_name], rule.Ask) and asks[out_name].KEYWORD == 'boxes'
    assert asks[out_name] == (screen, (28, 28), None, None, None)              # an ask equals the plain tuple of its fields
    assert asks == answers.checked({name: x}, None, None, False, boxes={out_name: BoxScreen(0.5, max_per_image=9)})
    # min_score and frame_size share the blocks; the fields that size or fill them do not
    key = asks[out_name].key(out_name)
    assert key == rule.Ask(screen._replace(min_score=0.75, frame_size=(9, 9)), (28, 28), None, None, None).key(out_name)
    for other in (dict(max_per_image=8), dict(labels=(1,)), dict(layout='NAC'), dict(threshold=0.5)):
        assert rule.Ask(screen._replace(**other), (28, 28), None, None, None).key(out_name) != key
    bound = asks[out_name].bound({name: x}, {})
    assert bound.frame_size == (28, 28) and bound.fit == (0, 0, 28, 28) and bound.launch_with() == (0.5, (28, 28), (0, 0, 28, 28))
    assert rule.Ask(screen._replace(frame_size=(480, 640)), (28, 28), None, None, None).bound({name: x}, {}).launch_with() == (0.5, (480, 640), (0, 0, 28, 28))
    with pytest.raises(ValueError, match='text: no FP32 Result'):               # the shorter calls answer as before
        keypoints_tests._mnist_head(tmp_path, n)[0].answers.checked({name: x}, None, None, False, None, None, None, None, True)
    assert not answers.blocks and not ex.host_inputs.slots and ex._pending is None


def test_a_host_result_gets_the_rule_in_numpy(tmp_path):
    """A plugin set that computes on the host (the oracle's) hands wait() host arrays: the same keyword, the same rule, no device."""
    from pyopenvino_amd import BoxScreen, Detections, RoiInput, boxes
    n = 3
    x = keypoints_tests._pixels(10, n)
    ex, net, name, out_name = _head(tmp_path, n, requests=2, package='oracle.op_plugins')
    full = np.array(ex.infer({name: x})[out_name], copy=True)
    assert full.shape == (n, 32, 676) and full.dtype == np.float32
    for given in (BoxScreen(0.5, 'NCA'), 0.25, BoxScreen(0.25, 'NAC', True, 'XYXY', (100, 50), threshold=0.2, per_label=False, max_per_image=5)):
        screen = boxes.resolved(given)
        want = boxes.decode(full, screen, (28, 28))
        for got in (ex.infer({name: x}, boxes=given), ex.requests[1].infer({name: x}, boxes={out_name: given})):
            assert set(got) == {out_name} and isinstance(got[out_name], Detections)
            _same(got[out_name], want, repr(given))
    assert np.array_equal(ex.infer({name: x})[out_name], full)                   # and whole again without the keyword
    kept = ex.infer({name: x}, boxes=BoxScreen(0.25, 'NCA', frame_size=(56, 56)))[out_name]
    assert kept.counts.sum() > 0
    RoiInput(np.zeros((n, 56, 56, 1), np.uint8), kept.rois)                       # the answer's rois are a RoiInput's table


def test_abi_declares_the_entries():
    from pyopenvino_amd import boxes, device
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    m = re.search(r'\b' + ENTRY + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S)
    assert m and len(m.group(1).split(',')) == 26 == len(device.SIGNATURES[ENTRY][1])
    assert len(device.SIGNATURES[FORM][1]) == 3 and FORM in device._NOT_STATUS
    for define, value in (('LAYOUT_NCA', 0), ('LAYOUT_NAC', 1), ('CXCYWH', 0), ('XYXY', 1), ('FORM_NONE', FORM_NONE), ('FORM_PLANES', FORM_PLANES),
                          ('FORM_ROWS_TEAM', FORM_ROWS_TEAM), ('FORM_ROWS_WAVE', FORM_ROWS_WAVE), ('MAX_CANDIDATES', 4096)):
        assert re.search(r'#define\s+PVHIP_BOXES_{}\s+{}\b'.format(define, value), header), define
    assert boxes.LAYOUTS == {'NCA': 0, 'NAC': 1} and boxes.BOXES == {'CXCYWH': 0, 'XYXY': 1} and boxes.MAX_CANDIDATES == 4096
    assert re.search(r'#define\s+PVHIP_ABI_VERSION\s+19\b', header)             # an addition: the version is unchanged
    assert boxes.scratch_bytes(3, 5, 2) == 192 + 192 and boxes.scratch_bytes(1, 1, 1) == 16 + 32


def _rows_switch():
    """The E up to which pvhip_dense_boxes_form answers ROWS_TEAM for 'NAC': read from the query, which needs no device."""
    from pyopenvino_amd import device
    forms = [device.call(FORM, 1, 64, e) for e in range(5, 2048)]
    steps = [e for e, (a, b) in zip(range(5, 2048), zip(forms, forms[1:])) if a != b]
    assert len(steps) == 1 and forms[0] == FORM_ROWS_TEAM and forms[-1] == FORM_ROWS_WAVE, steps
    return steps[0]


def test_the_form_query():
    from pyopenvino_amd import device
    form = lambda layout, a, e: device.call(FORM, layout, a, e)
    assert [form(-1, 64, 9), form(2, 64, 9), form(0, 0, 9), form(1, -1, 9), form(0, 64, 4), form(1, 64, 0)] == [FORM_NONE] * 6
    assert [form(0, a, e) for a in (1, 63, 8400) for e in (5, 84, 4000)] == [FORM_PLANES] * 9
    assert form(1, 25200, 85) == FORM_ROWS_TEAM and form(1, 1, 5) == FORM_ROWS_TEAM and _rows_switch() >= 85


# ---------------------------------------------------------------------------------------------------------------- GPU
GUARD, SENTINEL = top_k_tests.GUARD, top_k_tests.SENTINEL


def _device_boxes(hip, x, layout, s, offset=0, raw=False):
    """The entry on `x`, a contiguous tensor of `layout` -- `offset`: starting that many elements into a larger device tensor --, for the
    screen fields `s`; header, rows and scratch between sentinel words that must stay untouched; every header word written, and no row
    behind total."""
    from pyopenvino_amd import boxes, detections
    n, A, E = (x.shape[0], x.shape[2], x.shape[1]) if layout == 'NCA' else x.shape
    O = int(s.get('objectness', False))
    K = s.get('max_candidates', 1024)
    cap = s.get('max_per_image') or K
    frame, fit = s.get('frame_size') or NET, s.get('fit') or (0, 0, NET[1], NET[0])
    labels = s.get('labels')
    if offset:
        src = hip.DeviceTensor.from_numpy(np.concatenate([np.full(offset, 9e9, np.float32), x.ravel(), np.full(7, 9e9, np.float32)]))
    else:
        src = hip.DeviceTensor.from_numpy(x)
    words = boxes.scratch_bytes(n, A, cap) // 4
    scratch = hip.DeviceTensor.empty((words + 2 * GUARD,), np.int32)
    header = hip.DeviceTensor.empty((2 * n + 1 + 2 * GUARD,), np.int32)
    rows = hip.DeviceTensor.empty((8 * n * cap + 2 * GUARD,), np.int32)
    dev_labels = None if labels is None else hip.DeviceTensor.from_numpy(np.asarray(tuple(labels) + (0,), np.int32))
    for t in (scratch, header, rows):
        hip.call('pvhip_memset', ctypes.c_void_p(t.ptr), 0x7f, t.nbytes)
    hip.call(ENTRY, ctypes.c_void_p(src.ptr + 4 * offset), n, A, E - 4 - O, LAYOUTS.index(layout), O, BOXES.index(s.get('box', 'CXCYWH')),
             float(s.get('min_score', 0.25)), hip.ptr(dev_labels), 0 if labels is None else len(labels), frame[0], frame[1], fit[0], fit[1], fit[2], fit[3],
             s.get('min_size', (1, 1))[0], s.get('min_size', (1, 1))[1], K, OVERLAPS.index(s.get('overlap', 'IOU')), float(s.get('threshold', 0.45)),
             int(s.get('per_label', True)), cap, ctypes.c_void_p(scratch.ptr + 4 * GUARD), ctypes.c_void_p(header.ptr + 4 * GUARD),
             ctypes.c_void_p(rows.ptr + 4 * GUARD))
    sc, hd, rw = np.asarray(scratch), np.asarray(header), np.asarray(rows)
    for t, what in ((sc, 'scratch'), (hd, 'header'), (rw, 'rows')):
        assert (t[:GUARD] == SENTINEL).all() and (t[-GUARD:] == SENTINEL).all(), 'a word outside the {} was written'.format(what)
    assert not (sc[GUARD:GUARD + 3 * n * A] == SENTINEL).any(), 'a key or a winner was not written'
    hd, rw = hd[GUARD:-GUARD], rw[GUARD:-GUARD].reshape(-1, 8)
    total = int(hd[2 * n])
    assert 0 <= total == int(hd[:n].sum()) <= n * cap and (rw[total:] == SENTINEL).all() and not (hd == SENTINEL).any()
    t = rw[:total]
    got = detections.Detections(hd[:n].copy(), hd[n:2 * n].copy(), t[:, :5].copy(), t[:, 5].copy(), t[:, 6].copy().view(np.float32), t[:, 7].copy())
    return (got, hd.tobytes() + t.tobytes()) if raw else got


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_equals_the_rule(hip, shape):
    n, C, A = shape
    for what, layout, x, s, want in _cases(shape):
        E = 4 + int(s.get('objectness', False)) + C
        assert hip.call(FORM, LAYOUTS.index(layout), A, E) == (FORM_PLANES if layout == 'NCA' else FORM_ROWS_TEAM if E <= _rows_switch() else FORM_ROWS_WAVE)
        got, raw = _device_boxes(hip, x, layout, s, raw=True)
        _same(got, want, '{} {}'.format(what, layout))
        if what in ('normal', 'objectness'):
            for offset in (1, 2, 3):                            # no plane, no row starts on a 16-byte boundary
                _same(_device_boxes(hip, x, layout, s, offset), want, '{} {} offset {}'.format(what, layout, offset))
        if what in ('normal', 'four levels'):                   # three calls: the same bytes
            for again in range(2):
                assert _device_boxes(hip, x, layout, s, raw=True)[1] == raw, (what, layout, again)


def _switch_cases():
    """[(E, objectness, v (2, 70, E), screen fields, boxes.decode's answer)] for rows of E numbers on both sides of the E at which the form
    query says the 'NAC' form changes, with and without the objectness column; the last class, in the row's tail, wins now and then."""
    from pyopenvino_amd import boxes
    switch = _rows_switch()
    rng = np.random.default_rng(41)
    n, A = 2, 70
    cases = []
    for E in (switch - 1, switch, switch + 1, switch + 2):
        for objectness in (False, True):
            C = E - 4 - int(objectness)
            peak = rng.random((n, A, 1)).astype(np.float32)
            scores = (peak * rng.random((n, A, C)) * 0.875).astype(np.float32)
            np.put_along_axis(scores, np.where(rng.random((n, A, 1)) < 0.3, C - 1, rng.integers(0, C, (n, A, 1))), peak, axis=2)
            parts = [_boxes(rng, n, A)] + ([0.5 + rng.random((n, A, 1)).astype(np.float32) / 2] if objectness else []) + [scores]
            v = np.concatenate(parts, axis=2).astype(np.float32)
            s = dict(min_score=0.3, objectness=objectness, threshold=0.5)
            want = boxes.decode(v, _screen('NAC', s), NET)      # (held to the loops above)
            assert 0 < want.counts.sum() < want.selected.sum() < n * A and (want.labels == C - 1).any() and (want.labels < C - 1).any()
            cases.append((E, objectness, v, s, want))
    return switch, cases


def test_the_rows_on_both_sides_of_the_switch_against_the_loops():
    for E, objectness, v, s, want in _switch_cases()[1][::3]:
        _same(want, _ref(v, 'NAC', s), 'E {}'.format(E))


@pytest.mark.gpu
def test_kernel_on_both_sides_of_the_rows_switch(hip):
    """Rows of E numbers around the E at which the form query says the 'NAC' form changes from teams of 16 lanes to a wave per anchor,
    at every 4-byte phase."""
    switch, cases = _switch_cases()
    for E, objectness, v, s, want in cases:
        assert hip.call(FORM, 1, 70, E) == (FORM_ROWS_TEAM if E <= switch else FORM_ROWS_WAVE)
        for offset in range(4):
            _same(_device_boxes(hip, v, 'NAC', s, offset), want, 'E {} objectness {} offset {}'.format(E, objectness, offset))
        _same(_device_boxes(hip, _physical(v, 'NCA'), 'NCA', s), want, 'E {} as planes'.format(E))


@pytest.mark.gpu
def test_designed_suppression_cases(hip):
    v, cases = _designed()
    for what, (s, kept) in cases.items():
        for layout in LAYOUTS:
            x = _physical(v, layout)
            got = _device_boxes(hip, x, layout, s)
            _same(got, _ref(x, layout, s), what)
            assert got.records.tolist() == kept, what
    # 64 labels, of which two exist
    s = dict(cases['threshold 1'][0], labels=tuple(range(1, 65)))
    _same(_device_boxes(hip, v, 'NAC', s), _ref(v, 'NAC', s), '64 labels')
    # more than 64 kept in one image: the chunks of the greedy pass
    v = _grid()
    for s in (dict(min_score=0.25, max_candidates=256), dict(min_score=0.25, max_candidates=256, max_per_image=100), dict(min_score=0.25, max_candidates=130)):
        want = _ref(v, 'NAC', s)
        assert want.counts[0] == min(150, s.get('max_per_image', 150), s['max_candidates']) > 64 and want.selected[0] == 210
        for layout in LAYOUTS:
            _same(_device_boxes(hip, _physical(v, layout), layout, s), want, 'grid {}'.format(s))
    # integer edges stay, and a letterboxed 1920 x 1080 frame in a 64 x 64 extent
    v = _edges()
    s = dict(min_score=0.25, box='XYXY', threshold=1.0, frame_size=(481, 637), fit=(0, 0, 637, 481))
    got = _device_boxes(hip, v, 'NAC', s)
    _same(got, _ref(v, 'NAC', s), 'edges')
    assert np.array_equal(got.rois[:, 1:3], v[0, got.records, :2].astype(np.int32)) and got.counts.tolist() == [40]
    from pyopenvino_amd.input_format import fit_geometry
    assert fit_geometry((1080, 1920), NET, 'LETTERBOX') == (0, 14, 64, 36)
    for what, layout, x, s, want in _cases((3, 3, 63)):
        if what == 'labels':
            assert s['fit'] == (0, 14, 64, 36) and s['frame_size'] == (1080, 1920) and want.counts.sum() > 0
            assert (want.rois[:, 2] == 0).any() and (want.rois[:, 3] > 64).all()       # boxes over the upper bar clamp to row 0
            _same(_device_boxes(hip, x, layout, s), want, 'letterbox ' + layout)


@pytest.mark.gpu
def test_more_candidates_than_the_buffer_keeps(hip):
    """A = 5000 anchors that all pass, K = 1, 64 and 4096: the key buffer is cut more than once for the small K, selected shows the cap,
    and ties at the cut go to the lower anchor.  A = 9000 takes a second cut at K = 4096."""
    v = _crowd()
    for K in (1, 64, 4096):
        s = dict(min_score=0.0, max_candidates=K, threshold=0.5)
        want = _ref(v, 'NAC', s)
        assert want.selected.tolist() == [5000] and 1 <= want.counts[0] <= min(K, 80)
        for layout in LAYOUTS:
            _same(_device_boxes(hip, _physical(v, layout), layout, s), want, 'K {} {}'.format(K, layout))
    v = _crowd(9000)
    s = dict(min_score=0.0, max_candidates=4096, threshold=0.5, max_per_image=50)
    want = _ref(v, 'NAC', s)
    assert want.selected.tolist() == [9000]
    _same(_device_boxes(hip, v, 'NAC', s), want, 'A 9000')


@pytest.mark.gpu
def test_entry_rejects_what_it_cannot_do(hip):
    x = np.zeros((2, 10, 9), np.float32)
    t = hip.DeviceTensor.from_numpy(x)
    o = hip.DeviceTensor.empty((4096,), np.int32)
    lab = hip.DeviceTensor.from_numpy(np.zeros(64, np.int32))
    at = lambda words: ctypes.c_void_p(o.ptr + 4 * words)
    good = [ctypes.c_void_p(t.ptr), 2, 10, 5, 1, 0, 0, 0.25, None, 0, 64, 64, 0, 0, 64, 64, 1, 1, 8, 0, 0.5, 1, 8, at(0), at(1024), at(2048)]
    hip.call(ENTRY, *good)
    bads = [(0, None), (23, None), (24, None), (25, None)]                                  # a null pointer
    bads += [(0, ctypes.c_void_p(t.ptr + 2)), (23, at(1)), (24, ctypes.c_void_p(o.ptr + 4098)), (25, at(2049))]      # off their boundaries
    bads += [(i, bad) for i in (1, 2, 3) for bad in (0, -1)]                                # n, a, c < 1
    bads += [(4, 2), (4, -1), (5, 2), (5, -1), (6, 2), (6, -1), (7, float('nan')), (7, float('inf'))]
    bads += [(9, 1), (9, 65), (9, -1)]                                                      # labels counted but not given, too many
    bads += [(i, bad) for i in (10, 11, 14, 15) for bad in (0, -1, (1 << 24) + 1)] + [(i, bad) for i in (12, 13) for bad in (-1, (1 << 24) + 1)]
    bads += [(16, 0), (17, 0), (18, 0), (18, 4097), (22, 0), (22, 9), (19, 2), (19, -1), (20, -0.1), (20, 1.5), (20, float('nan')), (21, 2)]
    for i, bad in bads:
        args = list(good)
        args[i] = bad
        with pytest.raises(hip.PvhipError):
            hip.call(ENTRY, *args)
    for n, A, C in ((1 << 15, 1 << 12, 12), (1, 1 << 28, 4), (1 << 28, 1, 4)):             # n * a * e >= 2^31
        args = list(good)
        args[1:4] = (n, A, C)
        with pytest.raises(hip.PvhipError):
            hip.call(ENTRY, *args)
    args = list(good)                                                                        # 64 labels are taken
    args[8:10] = ctypes.c_void_p(lab.ptr), 64
    hip.call(ENTRY, *args)
    hip.synchronize()
    v, cases = _designed()                                                                   # the device is still usable
    s, kept = cases['IOS']
    assert _device_boxes(hip, v, 'NAC', s).records.tolist() == kept


def _on_device(hip, req, out_name):
    return text_tests._on_device(hip, req, out_name)


@pytest.mark.gpu
def test_public_path(hip, tmp_path):
    """mnist's first layer reshaped to (3, 32, 676): boxes= is boxes.decode of the request's own full Result -- which the tests above hold
    to the loops -- in every form of the value, named and unnamed, eager and replayed; another min_score and frame_size allocate nothing;
    the answer's rois feed a RoiInput."""
    import test_answer_checks as order_tests
    from pyopenvino_amd import BoxScreen, Detections, RoiInput, boxes
    n = 3
    x = keypoints_tests._pixels(10, n)
    ex, net, name, out_name = _head(tmp_path, n, requests=2)
    req = ex.requests[0]
    full = np.array(req.infer({name: x})[out_name], copy=True)
    assert full.shape == (n, 32, 676) and full.dtype == np.float32 and np.isfinite(full).all()
    low = float(np.quantile(full[:, 4:], 0.98))
    plain = BoxScreen(low, 'NCA', box='XYXY', threshold=0.3)
    values = [plain, BoxScreen(0.0, 'NAC', objectness=True, max_candidates=16), BoxScreen(low, frame_size=(480, 640), per_label=False, max_per_image=7), low,
              BoxScreen(0.0, 'NCA', labels=(3, 5), overlap='IOS')]
    for given in values + [{out_name: v} for v in values]:
        got = req.infer({name: x}, boxes=given)
        assert set(got) == {out_name} and isinstance(got[out_name], Detections)
        screen = boxes.resolved(given[out_name] if isinstance(given, dict) else given)
        want = boxes.decode(full, screen, (28, 28))
        _same(got[out_name], want, repr(given))
    default = boxes.decode(full, plain, (28, 28))
    assert 0 < default.counts.sum() < default.selected.sum() and len(set(default.counts.tolist())) > 1
    _same(ex.infer({name: x}, boxes=plain)[out_name], default, 'the network\'s own infer()')
    _same(ex.requests[1].infer({name: x}, None, None, None, None, None, None, None, plain)[out_name], default, 'the second request, positionally')
    assert np.array_equal(ex.infer({name: x})[out_name], full)              # and whole again without the keyword
    blocks = len(req.runner.answers.blocks)
    real_call, issued = hip.call, []
    hip.call = lambda entry, *args: (issued.append(entry), real_call(entry, *args))[1]
    try:
        other = plain._replace(min_score=low / 2, frame_size=(100, 200))
        got = req.infer({name: x}, boxes=other)[out_name]
    finally:
        hip.call = real_call
    _same(got, boxes.decode(full, other, (28, 28)), 'another min_score and frame')
    assert issued.count(ENTRY) == 1 and not set(order_tests.ALLOCATIONS) & set(issued[issued.index(ENTRY):]) and len(req.runner.answers.blocks) == blocks
    RoiInput(np.zeros((n, 100, 200, 1), np.uint8), got.rois)                 # the table a RoiInput takes
    assert got.rois.dtype == np.int32 and (got.rois[:, 0] == np.repeat(np.arange(n), got.counts)).all()
    # the same device-resident tensor: eager, eager, replayed; identical answers, and the Result stays on the device
    xd = hip.DeviceTensor.from_numpy(x)
    fresh, _, _, _ = _head(tmp_path, n)
    answers = []
    for call in range(3):
        fresh.requests[0].start_async({name: xd}, boxes=plain)
        assert (fresh.requests[0]._replayed is not None) == (call == 2), call
        answers.append(fresh.requests[0].wait()[out_name])
        _same(answers[-1], default, 'pass {}'.format(call))
        helpers.assert_bit_exact(_on_device(hip, fresh.requests[0], out_name), full, 'the Result behind pass {}'.format(call))
    for later in answers[1:]:
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(answers[0], later))
    assert len(fresh.answers.blocks) == 1
    fresh.release_device_state()
    assert not fresh.answers.blocks


@pytest.mark.gpu
def test_the_launch_order_behind_the_pass(hip, tmp_path):
    """What test_answer_checks pins for a table answer: select, the entry once (its three launches are one call), one event, select;
    wait() makes two copies, one when total is 0; the passes with and without the keyword replay one recording."""
    import test_answer_checks as order_tests
    from pyopenvino_amd import BoxScreen
    n = 2
    x = hip.DeviceTensor.from_numpy(keypoints_tests._pixels(20, n))
    for screen, copies in ((BoxScreen(0.0, 'NCA'), 2), (BoxScreen(3e38, 'NCA'), 1)):
        ex, _, name, out_name = _head(tmp_path, n)              # (a request that has not recorded yet)
        got = order_tests._same_answers(order_tests._passes(hip, ex.requests[0], {name: x}, dict(boxes=screen), [ENTRY], [copies]), out_name)
        assert (got.counts.sum() > 0) == (copies == 2) and got.counts.shape == (n,)
        req, real_call = ex.requests[0], hip.call                 # one recording serves the pass with the keyword and the pass without
        for asked in (dict(), dict(boxes=screen), dict()):
            issued = []
            hip.call = lambda entry, *args: (issued.append(entry), real_call(entry, *args))[1]
            try:
                req.start_async({name: x}, **asked)
                assert req._replayed is not None
                out = req.wait()[out_name]
            finally:
                hip.call = real_call
            assert issued.count(order_tests.REPLAY) == 1 and not [e for e in issued if 'capture' in e] and issued.count(ENTRY) == len(asked), issued
            if asked:
                order_tests._same_answers([{out_name: got}, {out_name: out}], out_name)
            else:
                assert out.shape == (n, 32, 676)


@pytest.mark.gpu
def test_a_letterboxed_host_input_gives_the_geometry_of_its_frames(hip, tmp_path):
    """The head behind a U8 / NHWC input that declares a resize and 'LETTERBOX', fed frames of another aspect: frame_size None is the
    frames' extent and the geometry is that of the frames fed, pass by pass, under an explicit frame_size too; a RoiInput on the fitted
    input is refused as detections= refuses it."""
    from pyopenvino_amd import BoxScreen, IECore, RoiInput, boxes
    from pyopenvino_amd.input_format import fit_geometry
    n = 2
    _head(tmp_path, n)                                          # writes the IR
    ie = IECore(plugin_package=keypoints_tests.HIP)
    net = ie.read_network(os.path.join(str(tmp_path), 'mnist_text_ntc.xml'), weights=os.path.join(str(tmp_path), 'mnist_text_ntc.bin'))
    net.set_batch(n)
    name, out_name = net.inputs[0]['name'], 'text'
    info = net.input_info[name]
    info.precision, info.layout = 'U8', 'NHWC'
    info.preprocess_info.resize_algorithm = 'RESIZE_BILINEAR'
    info.preprocess_info.resize_fit = 'LETTERBOX'
    info.preprocess_info.init(1)                                # pixels in 0 .. 127.5: the head's box channels are small numbers
    info.preprocess_info[0].std_scale = 2.0
    info.preprocess_info.mean_variant = 'MEAN_VALUE'
    ex = ie.load_network(net, 'GPU', num_requests=1)
    req = ex.requests[0]
    rng = np.random.default_rng(8)
    screen = BoxScreen(0.0, 'NCA', threshold=0.4, max_per_image=50)
    differs = []
    for hw in ((540, 560), (840, 810)):                         # fitted into 28 x 27 and 27 x 28 of the 28 x 28 input
        frames = rng.integers(0, 256, (n,) + hw + (1,), dtype=np.uint8)
        full = np.array(req.infer({name: frames})[out_name], copy=True)
        assert full.shape == (n, 32, 676)
        got = req.infer({name: frames}, boxes=screen)[out_name]
        fit = fit_geometry(hw, (28, 28), 'LETTERBOX')
        assert fit in ((0, 0, 28, 27), (0, 0, 27, 28))
        _same(got, boxes.decode(full, screen._replace(frame_size=hw), (28, 28), fit), 'frames of {}'.format(hw))
        assert got.counts.sum() > 0 and (got.rois[:, 1] + got.rois[:, 3] <= hw[1]).all() and (got.rois[:, 2] + got.rois[:, 4] <= hw[0]).all()
        wide = screen._replace(frame_size=(28000, 28000))       # an explicit frame_size stays, the geometry is still the frames'
        given = req.infer({name: frames}, boxes=wide)[out_name]
        _same(given, boxes.decode(full, wide, (28, 28), fit), 'an explicit frame_size')
        differs.append(not np.array_equal(given.rois, boxes.decode(full, wide, (28, 28)).rois))
    assert all(differs)                                         # the identity geometry gives other rectangles
    with pytest.raises(ValueError, match='boxes: input .* declares resize_fit LETTERBOX and is fed a RoiInput'):
        req.infer({name: RoiInput(frames, np.array([[0, 0, 0, 20, 20]] * n, np.int32))}, boxes=screen)
    assert len(req.runner.answers.blocks) == 1                  # the blocks serve every extent
