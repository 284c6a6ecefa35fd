"""``segments=FrameSegmentScreen(...)``: a segmentation Result's class map in frame pixels (pvhip_segment_frame_labels_f32).
tests/segments_frame_ref.py is the rule from its text; segments.frame_labels and the kernel equal it exactly: labels byte for byte,
areas and extents as integers.  The first tests need no GPU."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import helpers
import segments_frame_ref as ref
import test_keypoints as keypoints_tests
import test_segments as segments_tests

ENTRY, FORM = 'pvhip_segment_frame_labels_f32', 'pvhip_segment_frame_labels_form'
GUARD, _same = segments_tests.GUARD, segments_tests._same
HEADER = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
BAND_ROWS, COL_CHUNK, CLASS_CHUNK, STAGED, DIRECT = (int(re.search(r'#define\s+PVHIP_SEGMENT_FRAME_{}\s+(\d+)'.format(name), HEADER).group(1))
                                                     for name in ('BAND_ROWS', 'COL_CHUNK', 'CLASS_CHUNK', 'FORM_STAGED', 'FORM_DIRECT'))
LETTERBOX = ((40, 56), (45, 81), (0, 4, 56, 31))        # (net, frame, fit): Fw % 4 == 1, taps clamp on all four edges
CASES = {                                               # name: (map shape, (net, frame, fit), kind, the form the query reports)
    'letterbox': ((2, 3, 5, 7), LETTERBOX, 'quarters', STAGED),
    'normals': ((2, 3, 5, 7), LETTERBOX, 'normals', STAGED),
    'one class': ((2, 1, 5, 7), LETTERBOX, 'quarters', STAGED),
    'chunk seam': ((2, CLASS_CHUNK + 1, 5, 7), LETTERBOX, 'seam', STAGED),
    '255 classes': ((2, 255, 5, 7), LETTERBOX, 'seam', STAGED),
    'tile seams': ((1, 2, 4, 5), ((8, 10), (BAND_ROWS + 1, COL_CHUNK + 1), (0, 0, 10, 8)), 'quarters', STAGED),
    'downsampling': ((1, 2, 64, 96), ((64, 96), (9, 13), (0, 0, 96, 64)), 'quarters', DIRECT),
    'batch rows': ((3, 3, 4, 5), ((8, 10), (6, 7), (0, 0, 10, 8)), 'rows', STAGED),      # three tiles, one workgroup
    'identity': ((2, 5, 9, 13), ((9, 13), (9, 13), (0, 0, 13, 9)), 'quarters', STAGED),
}
MIN_SCORE = 0.25


@functools.lru_cache(maxsize=None)
def _planes(name, specials):
    """The case's planes, read-only.  'quarters': small integers / 4, |v| <= 8, so every lerp is exact and equal values across classes
    are true ties; `specials`: a few NaN, +inf, -inf and -0.0 pixels among them.  'seam': the classes on either side of the chunk
    boundary are equal and, in a corner, the best; a NaN in each.  'rows': class 2 below everything (no pixel), row 1 quiet NaNs."""
    shape, _, kind, _ = CASES[name]
    n, C, H, W = shape
    rng = np.random.default_rng(sum(shape) + len(name))
    x = rng.standard_normal(shape).astype(np.float32) if kind == 'normals' else (rng.integers(-32, 33, shape) / 4).astype(np.float32)
    if kind == 'seam':
        x[:, :, :2, :3] = np.minimum(x[:, :, :2, :3], 7)
        x[:, CLASS_CHUNK - 1, :2, :3] = 8
        x[:, CLASS_CHUNK] = x[:, CLASS_CHUNK - 1]
        x[0, CLASS_CHUNK, 4, 6] = x[1, CLASS_CHUNK - 1, 4, 0] = np.nan
    if kind == 'rows':
        x[:, 2] = -9
        x[1].view(np.uint32)[...] = 0x7FC00000
    if specials:
        flat = x.reshape(-1)
        flat[rng.choice(x.size, 8, replace=False)] = [np.nan, np.inf, -np.inf, -0.0, np.nan, np.inf, -np.inf, -0.0]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _want(name, min_score):
    net, frame, fit = CASES[name][1]
    return ref.frame_segments(_planes(name, min_score is not None), net, frame, fit, min_score)


def _runs():
    return [(name, min_score) for name in CASES for min_score in (None, MIN_SCORE) if not (name == 'one class' and min_score is None)]


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
@pytest.mark.parametrize('name, min_score', _runs())
def test_frame_labels_equals_the_loops(name, min_score):
    from pyopenvino_amd import FrameSegmentScreen, segments
    from pyopenvino_amd.input_format import fit_geometry
    net, frame, fit = CASES[name][1]
    x, want = _planes(name, min_score is not None), _want(name, min_score)
    _same(segments.frame_labels(x, FrameSegmentScreen(min_score), net, frame, fit), want, name)
    assert (want.labels != 255).any() and (min_score is None or (want.labels == 255).any())
    assert fit_geometry(LETTERBOX[1], LETTERBOX[0], 'LETTERBOX') == LETTERBOX[2]
    if name == 'identity' and min_score is None:                # fractions 0 and a + 0 * (b - a) = a: the map's own answer
        _same(segments.labels(x), want, 'identity')
    if name == 'batch rows':
        assert not want.areas[:, 2].any() and not want.extents[:, 2].any() and (want.labels[1] == 255).all() and want.areas[0].sum() > 0
    if CASES[name][2] == 'seam' and min_score is None:          # the tie across the boundary goes to the lower class; each NaN voids
        assert (want.labels[:, 0, 0] == CLASS_CHUNK - 1).all() and not want.areas[:, CLASS_CHUNK].any()
        assert want.labels[0, 44, 80] == 255 and want.labels[1, 44, 0] == 255


def test_argument_rules(tmp_path):
    """Every refusal is a ValueError('segments: ...') before anything is staged; what bound() learns; the key."""
    from pyopenvino_amd import FrameSegmentScreen, SegmentScreen, segments
    from pyopenvino_amd.input_format import fit_geometry
    n = 8
    ex, net, name, out_name = keypoints_tests._mnist_head(tmp_path, n)
    x, req = np.zeros((n, 1, 28, 28), np.float32), ex.requests[0]
    for match, value in (('no Result named', {'nope': FrameSegmentScreen()}), ('a SegmentScreen, a min_score or True', {out_name: 'FRAME'}),
                         ('a SegmentScreen, a min_score or True', FrameSegmentScreen), ('min_score', FrameSegmentScreen(np.nan)),
                         ('frame_size', FrameSegmentScreen(frame_size=(0, 5))), ('frame_size', FrameSegmentScreen(frame_size=(16385, 5))),
                         ('frame_size', FrameSegmentScreen(frame_size=7)), ('frame_size', FrameSegmentScreen(frame_size=(4.0, 5))),
                         ('no 4-D Parameter', FrameSegmentScreen(input='nope')), ('no 4-D Parameter', {out_name: FrameSegmentScreen(input=3)}),
                         ('n \\* Fh \\* Fw < 2\\^31', FrameSegmentScreen(frame_size=(16384, 16384)))):
        for start in (lambda: ex.infer({name: x}, segments=value), lambda: req.start_async({name: x}, segments=value)):
            with pytest.raises(ValueError, match=match) as e:
                start()
            assert str(e.value).startswith('segments: '), str(e.value)
    ex.comm = type('Comm', (), dict(world=2, rank=0))()
    with pytest.raises(ValueError, match='^segments: .*sharded'):
        ex.infer({name: x}, segments=FrameSegmentScreen())
    ex.comm = None
    with pytest.raises(ValueError, match='^segments: Result .* is asked for with keypoints as well'):
        ex.infer({name: x}, keypoints=True, segments=FrameSegmentScreen())
    port = req.runner.ienet.outputs[0]['input'][0]
    declared, port['dims'] = port['dims'], (n, 2, 4097, 2)
    with pytest.raises(ValueError, match='^segments: .*maps of at most 4096 x 4096'):
        req.start_async({name: x}, segments=FrameSegmentScreen())
    port['dims'] = declared
    assert not req._in_flight and not req._asks and not ex.answers.blocks and not ex.host_inputs.slots
    asks = ex.answers.checked({name: x}, None, None, False, segments=FrameSegmentScreen(0.5, (60, 90)))
    ask = asks[out_name]
    assert isinstance(ask, segments.FrameAsk) and ask == (FrameSegmentScreen(0.5, (60, 90), name), (28, 28), None, None, None) and ask.KEYWORD == 'segments'
    assert ask.bound({}, {})[3:] == ((60, 90), (0, 0, 28, 28)) and ask._replace(screen=FrameSegmentScreen()).bound({}, {})[3:] == ((28, 28), (0, 0, 28, 28))
    fmt = type('Format', (), dict(fit_geometry=lambda self, extent: fit_geometry(extent, (28, 28), 'LETTERBOX')))()
    slots = {name: type('Slot', (), dict(fed=(540, 560)))()}
    boxed = ask._replace(screen=FrameSegmentScreen(0.5, None, name), format=fmt).bound({}, slots)
    assert boxed[3:] == ((540, 560), (0, 0, 28, 27)) and ask._replace(format=fmt).bound({}, slots)[3:] == ((60, 90), (0, 0, 28, 27))
    assert boxed.key(out_name) == (out_name, 'FRAME', 540, 560) == boxed._replace(screen=FrameSegmentScreen(0.75, None, name)).key(out_name)
    assert boxed.launch_with() == (0.5, (28, 28), (540, 560), (0, 0, 28, 27))
    with pytest.raises(ValueError, match='^segments: .*at most 16384 x 16384'):
        ask._replace(screen=FrameSegmentScreen(input=name), format=fmt).bound({}, {name: type('Slot', (), dict(fed=(20000, 560)))()})
    assert isinstance(ex.answers.checked({name: x}, None, None, False, segments=0.5)[out_name], segments.Ask)
    assert segments.resolved(True) == SegmentScreen() and FrameSegmentScreen._fields == ('min_score', 'frame_size', 'input')


# ---------------------------------------------------------------------------------------------------------------- GPU
def _device(hip, x, geometry, min_score, entry=ENTRY):
    """The entry on `x` between sentinel bytes that must stay untouched: a Segments, the extents of empty classes turned to zeros."""
    n, C, H, W = x.shape
    net, (fh, fw), fit = geometry
    src, pixels = hip.DeviceTensor.from_numpy(np.ascontiguousarray(x)), n * fh * fw
    outs = [hip.DeviceTensor.empty((words + 2 * GUARD,), np.int32) for words in ((pixels + 3) // 4, n * C, 4 * n * C)]
    for t in outs:
        hip.call('pvhip_memset', ctypes.c_void_p(t.ptr), 0xFE, t.nbytes)
    to = [ctypes.c_void_p(t.ptr + 4 * GUARD) for t in outs]
    where = (H, W) if entry != ENTRY else (H, W, net[0], net[1], fh, fw) + tuple(fit)
    hip.call(entry, hip.ptr(src), n, C, *where, int(min_score is not None), float(min_score or 0.0), *to)
    lab, are, ext = (np.asarray(t).view(np.uint8) for t in outs)
    assert (lab[:4 * GUARD] == 0xFE).all() and (lab[4 * GUARD + pixels:] == 0xFE).all(), 'a byte outside the labels was written'
    assert C > 254 or not (lab[4 * GUARD:4 * GUARD + pixels] == 0xFE).any(), 'a label was not written'
    assert all((t[:4 * GUARD] == 0xFE).all() and (t[-4 * GUARD:] == 0xFE).all() for t in (are, ext))
    areas = are[4 * GUARD:-4 * GUARD].view(np.int32).reshape(n, C).copy()
    extents = ext[4 * GUARD:-4 * GUARD].view(np.int32).reshape(n, C, 4).copy()
    assert (extents[areas == 0] == (fw, fh, 0, 0)).all()
    extents[areas == 0] = 0
    return ref.Segments(lab[4 * GUARD:4 * GUARD + pixels].reshape(n, fh, fw).copy(), areas, extents)


@pytest.mark.gpu
@pytest.mark.parametrize('name, min_score', _runs())
def test_kernel_equals_the_rule(hip, name, min_score):
    """Each case in the form the query reports; three calls, the same bytes; the identity equals pvhip_segment_labels_f32."""
    shape, geometry, _, form = CASES[name]
    (hn, wn), (fh, fw), fit = geometry
    assert hip.call(FORM, *shape[1:], hn, wn, fh, fw, *fit) == form
    x, want = _planes(name, min_score is not None), _want(name, min_score)
    got = [_device(hip, x, geometry, min_score) for _ in range(3)]
    _same(got[0], want, name)
    assert all(np.array_equal(a, b) for later in got[1:] for a, b in zip(got[0], later))
    if name == 'identity' and min_score is None:
        _same(_device(hip, x, geometry, None, 'pvhip_segment_labels_f32'), got[0], 'beside pvhip_segment_labels_f32')


@pytest.mark.gpu
def test_public_path(hip, tmp_path):
    """A U8 / NHWC / RESIZE_BILINEAR / LETTERBOX input fed host frames larger than the network: the answer is frame_labels on the
    whole Result of a pass without the keyword, under the fit the frames imply; both replay one recording; a RoiInput is refused."""
    from pyopenvino_amd import FrameSegmentScreen, IECore, RoiInput, Segments, segments
    from pyopenvino_amd.input_format import fit_geometry
    n, hw = 2, (60, 90)
    ie = IECore(plugin_package=keypoints_tests.HIP)
    net = ie.read_network(keypoints_tests._heatmap_head('mnist', tmp_path), weights=os.path.join(keypoints_tests.MODELS, 'mnist.bin'))
    net.set_batch(n)
    name, out_name = net.inputs[0]['name'], net.outputs[0]['name']
    info = net.input_info[name]
    info.precision, info.layout = 'U8', 'NHWC'
    info.preprocess_info.resize_algorithm, info.preprocess_info.resize_fit = 'RESIZE_BILINEAR', 'LETTERBOX'
    req = ie.load_network(net, 'GPU', num_requests=1).requests[0]
    frames = np.random.default_rng(5).integers(0, 256, (n,) + hw + (1,), dtype=np.uint8)
    req.infer({name: frames})
    full = np.array(req.infer({name: frames})[out_name], copy=True)
    fit = fit_geometry(hw, (28, 28), 'LETTERBOX')
    cut = float(np.median(full.max(axis=1)))
    for screen in (FrameSegmentScreen(), FrameSegmentScreen(cut), FrameSegmentScreen(cut, (30, 45))):
        req.start_async({name: frames}, segments=screen)
        assert req._replayed is not None
        got = req.wait()[out_name]
        want = segments.frame_labels(full, screen, (28, 28), screen.frame_size or hw, fit)
        assert isinstance(got, Segments) and got.labels.shape == (n,) + (screen.frame_size or hw) and len(np.unique(want.labels)) > 2
        _same(got, want, repr(screen))
    req.start_async({name: frames})
    assert req._replayed is not None and np.array_equal(req.wait()[out_name], full)
    assert sorted(req.runner.answers.blocks) == [(out_name, 'FRAME', 30, 45), (out_name, 'FRAME', 60, 90)]      # a block pair per extent
    with pytest.raises(ValueError, match='segments: input .* declares resize_fit LETTERBOX and is fed a RoiInput'):
        req.infer({name: RoiInput(frames, np.array([[0, 0, 0, 20, 20]] * n, np.int32))}, segments=FrameSegmentScreen())
