"""The connected components of a probability map made on the device (``infer(..., components=...)``, pvhip_components_f32) by the rule of
tests/components_ref.py: every field exactly, no tolerance anywhere.  The first two tests need no GPU."""
import ctypes
import types

import numpy as np
import pytest

import components_ref
import test_segments as segments_tests

ENTRY = 'pvhip_components_f32'
QUIET = 0x7FC00000
_mnist_head, _pixels = segments_tests._mnist_head, segments_tests._pixels
# (shape, channel): (2, 1, 5, 7) one partial tile, W no multiple of 4, two images; (1, 3, 33, 129) an odd plane behind channel 0 -- a
# 4-byte phase -- and one row and one column past a tile; (2, 1, 64, 256) exactly 2 x 2 tiles; (1, 2, 70, 300) ragged on both seams
HOST_SHAPES = [((1, 1, 1, 2), 0), ((2, 1, 5, 7), 0), ((1, 3, 6, 9), 1), ((1, 3, 6, 9), -1)]
GPU_SHAPES = [((1, 1, 1, 2), 0), ((2, 1, 5, 7), 0), ((1, 3, 33, 129), 1), ((2, 1, 64, 256), 0), ((1, 2, 70, 300), -1)]
FILLINGS = ('background', 'foreground', 'NaN row', 'two columns', 'checkerboard', 'corner', 'serpentine', 'blobs', 'blobs of 9', 'crowd', 'signed zeros')


def _same(got, want, what=''):
    for field, a, b in zip(want._fields, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, field, a.dtype, a.shape, b.dtype, b.shape)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), '{}: {} differs\n{}\n{}'.format(what, field, a[:12], b[:12])


def _filling(what, shape, channel):
    """(x, the screen's fields) of one filling: plane `channel` of every image holds it, the other planes noise."""
    n, K, H, W = shape
    rng = np.random.default_rng(len(what) + 31 * H + W)
    x = rng.random(shape, dtype=np.float32)
    p = np.zeros((n, H, W), np.float32)
    ys, xs = np.mgrid[0:H, 0:W]
    screen = dict(min_score=0.5, channel=channel, max_per_image=64)
    if what == 'foreground':
        p[:] = 1 + rng.random((n, H, W), dtype=np.float32)
    elif what == 'NaN row':
        p[:] = 1
        p[:, H // 2].view(np.uint32)[:] = QUIET
    elif what == 'two columns':                                 # a full last column and a full first one stay two components
        p[:, :, 0] = p[:, :, -1] = 0.5                          # (equality keeps)
    elif what == 'checkerboard':                                # many components under 4, one under 8: the cap and the tie-break by seed
        p[:] = (ys + xs) % 2
        screen.update(max_per_image=16)
    elif what == 'corner':                                      # single pixels in diagonal chains through a tile corner and over each seam
        cy, cx = min(32, H - 2), min(128, W - 2)
        for y, xx in [(cy + i, cx + i) for i in range(-2, 2)] + [(cy + i, 10 - i) for i in range(-2, 2)] + [(5 + i, cx - 1 - i) for i in range(-2, 2)]:
            if 0 <= y < H and 0 <= xx < W:
                p[:, y, xx] = 1
    elif what == 'serpentine':                                  # one pixel wide, over every seam many times: long parent chains
        p[:] = (ys % 2 == 0) | ((ys % 4 == 1) & (xs == W - 1)) | ((ys % 4 == 3) & (xs == 0))
        p[1:, ::2, W // 2] = 0                                  # (the second image: every full row cut in two)
    elif what in ('blobs', 'blobs of 9'):                       # a thresholded smooth field
        coarse = rng.random((n, H // 4 + 2, W // 4 + 2), dtype=np.float32)
        p[:] = (np.kron(coarse, np.ones((4, 4), np.float32))[:, 1:H + 1, 2:W + 2] + 0.2 * rng.random((n, H, W), dtype=np.float32)).astype(np.float32)
        screen.update(min_score=float(np.median(p)), min_area=9 if what == 'blobs of 9' else 1, max_per_image=1024)
    elif what == 'crowd':                                       # small components of every area in no order, more than R = 1024 on the
        p[:] = rng.random((n, H, W)) < 0.2                      # large shapes: the selection cuts its key buffer again and again
        screen.update(max_per_image=1024)
    elif what == 'signed zeros':                                # peaks that are zeros: the sign of the first in raster order
        p[:] = np.where(rng.random((n, H, W)) < 0.6, np.where(rng.random((n, H, W)) < 0.5, np.float32(0.0), np.float32(-0.0)), np.float32(-1))
        screen.update(min_score=0.0, connectivity=4)
    x[:, channel] = p
    return x, screen


def _cases(shape, channel):
    for what in FILLINGS:
        x, screen = _filling(what, shape, channel)
        for connectivity in ((4, 8) if 'connectivity' not in screen else (screen['connectivity'],)):
            fields = dict(screen, connectivity=connectivity)
            want = components_ref.components(x, **fields)
            if shape[2] * shape[3] > 1000:                      # the fillings do what they are for
                if what == 'checkerboard':
                    assert (want.found > 16).all() if connectivity == 4 else (want.found == 1).all()
                if what == 'corner':
                    assert (want.found == (12 if connectivity == 4 else 3)).all()
                if what == 'crowd' and shape[2] * shape[3] > 16000:
                    assert (want.found > 1024).all() and (want.counts == 1024).all()
                if what == 'blobs of 9':
                    assert (0 < want.counts).all() and (want.counts < want.found).all()
            yield '{} {} {} {}'.format(shape, channel, what, connectivity), x, fields, want


@pytest.mark.parametrize('shape, channel', HOST_SHAPES)
def test_find_agrees_with_the_loops(shape, channel):
    from pyopenvino_amd import ComponentScreen, Components, components
    for what, x, fields, want in _cases(shape, channel):
        got = components.find(x, ComponentScreen(**fields))
        assert isinstance(got, Components)
        _same(got, want, what)
        for r in range(shape[0]):
            assert len(got.of(r).areas) == want.counts[r] and (got.of(r).rois[:, 0] == r).all()
    square = Components(*(np.array(v) for v in ([1], [1], [[0, 2, 3, 4, 2]], [8], [0], [1.0], [0], [[28, 28, 108, 98, 100]])))
    assert np.allclose(components.oriented(square), [[4.0, 4.0, 4.0, 2.0, 0.0]])           # a 4 x 2 rectangle at (2, 3)
    assert components.to_frame([[1, 1, 2, 3, 3]], (10, 10), (25, 15)).tolist() == [[1, 1, 5, 5, 8]]


BAD_SCREENS = [('min_score', dict(min_score=None)), ('min_score', dict(min_score=np.nan)), ('min_score', dict(min_score='x')), ('min_score', dict(min_score=1e39)),
               ('channel', dict(channel=32)), ('channel', dict(channel=-33)), ('channel', dict(channel=0.0)), ('channel', dict(channel=True)),
               ('connectivity', dict(connectivity=6)), ('connectivity', dict(connectivity='8')), ('min_area', dict(min_area=0)),
               ('min_area', dict(min_area=(1 << 24) + 1)), ('min_area', dict(min_area=2.0)), ('max_per_image', dict(max_per_image=0)),
               ('max_per_image', dict(max_per_image=1025)), ('max_per_image', dict(max_per_image=None))]


def test_argument_refusals(tmp_path):
    """Every refusal is a ValueError('components: ...') before anything is staged or launched: no device here."""
    from pyopenvino_amd import ComponentScreen, components as rule
    n = 2
    ex, net, name, out_name = _mnist_head(tmp_path, n)           # its Result: (n, 32, 26, 26) FP32
    x = np.zeros((n, 1, 28, 28), np.float32)
    req = ex.requests[0]

    def refused(match, value, **kw):
        for start in (lambda: ex.infer({name: x}, components=value, **kw), lambda: req.start_async({name: x}, components=value, **kw)):
            with pytest.raises(ValueError, match=match) as e:
                start()
            assert str(e.value).startswith('components: '), str(e.value)
        assert not req._in_flight and not req._asks and not ex.answers.blocks and not ex.host_inputs.slots and ex._pending is None

    for match, fields in BAD_SCREENS:
        refused(match, {out_name: ComponentScreen(**fields)})
        # (the unnamed form of a channel outside K: no Result admits it)
        refused('no FP32 Result' if fields.get('channel') in (32, -33) else match, ComponentScreen(**fields))
    refused('no Result named', {'nope': True})
    refused('a ComponentScreen, a min_score or True', 'x')
    refused('a ComponentScreen, a min_score or True', {out_name: False})
    refused('Result {!r} is asked for with segments as well'.format(out_name), True, segments=True)
    ex.comm = types.SimpleNamespace(world=2, rank=0)
    try:
        refused('sharded', 0.5)
    finally:
        ex.comm = None
    port = req.runner.ienet.outputs[0]['input'][0]
    for key, bad, match in (('precision', 'FP16', 'FP32 Results only'), ('dims', (n, 32, 676), 'has shape'), ('dims', (n, 256, 26, 26), 'has shape')):
        kept, port[key] = port[key], bad
        try:
            refused(match, {out_name: True})
        finally:
            port[key] = kept
    # the good forms resolve
    assert rule.checked(net, None, False) == {} and rule.checked(net, True, False) == {out_name: ComponentScreen(float(np.float32(0.3)), 0, 8, 1, 256)}
    assert rule.checked(net, 0.5, False) == rule.checked(net, {out_name: np.float32(0.5)}, False) == {out_name: ComponentScreen(0.5)}
    assert rule.checked(net, {out_name: ComponentScreen(1, -1, 4, 9, 1024)}, False) == {out_name: ComponentScreen(1.0, 31, 4, 9, 1024)}
    ask = ex.answers.checked({name: x}, None, None, False, components=0.5)[out_name]
    assert ask.KEYWORD == 'components' and ask.key(out_name) == (out_name, 0, 8, 256) and ask.launch_with() == (0.5, 1)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _device(hip, x, fields, blocks=None):
    from pyopenvino_amd import ComponentScreen, components
    screen = components.for_planes(components.resolved(ComponentScreen(**fields)), x.shape[1])
    blocks = blocks or components.Blocks(*x.shape, screen.channel, screen.connectivity, screen.max_per_image)
    blocks.launch(hip.DeviceTensor.from_numpy(x), screen.min_score, screen.min_area)
    return blocks.read_back(), blocks


@pytest.mark.gpu
@pytest.mark.parametrize('shape, channel', GPU_SHAPES)
def test_kernel_equals_the_rule(hip, shape, channel):
    for what, x, fields, want in _cases(shape, channel):
        got, blocks = _device(hip, x, fields)
        _same(got, want, what)
        first = np.array(blocks.host, copy=True)
        for again in range(2):                                  # three calls give the same bytes
            _same(_device(hip, x, fields, blocks)[0], want, what + ' again')
            assert np.array_equal(blocks.host, first), what


@pytest.mark.gpu
def test_entry_rejects_what_it_cannot_do(hip):
    x = hip.DeviceTensor.from_numpy(np.ones((2, 3, 4, 8), np.float32))
    out = hip.DeviceTensor.empty((2 * 2 + 20 * 2 * 4,), np.int32)
    scratch = hip.DeviceTensor.empty((3 * 2 * 4 * 8,), np.int32)
    hip.call('pvhip_memset', ctypes.c_void_p(out.ptr), 0x7F, out.nbytes)
    at = lambda words: ctypes.c_void_p(out.ptr + 4 * words)
    good = [ctypes.c_void_p(x.ptr), 2, 3, 4, 8, 0, 8, 0.5, 1, 4, ctypes.c_void_p(scratch.ptr), at(160), at(162), at(128), at(136), at(144), at(152), at(96), at(0), at(16)]
    assert hip.call('pvhip_components_scratch_bytes', 2, 4, 8, 4) == scratch.nbytes and hip.call('pvhip_components_scratch_bytes', 2, 1, 1, 4) == 0
    bads = [(at_, None) for at_ in (0, 10, 11, 12, 19)] + [(18, ctypes.c_void_p(out.ptr + 4)), (0, ctypes.c_void_p(x.ptr + 2))]     # NULL, off its boundary
    bads += [(1, 0), (2, 0), (2, 256), (3, 0), (4, -1), (5, 3), (5, -4), (6, 6), (6, 0), (7, float('nan')), (7, float('inf')), (8, 0), (8, (1 << 24) + 1),
             (9, 0), (9, 1025)]
    for at_, bad in bads:
        args = list(good)
        args[at_] = bad
        with pytest.raises(hip.PvhipError):
            hip.call(ENTRY, *args)
    for n, h, w in ((2, 1, 1), (1, 4097, 4096), (128, 4096, 4096)):                       # H * W < 2, > 2^24, n * H * W >= 2^31
        with pytest.raises(hip.PvhipError):
            hip.call(ENTRY, *(good[:1] + [n, 3, h, w] + good[5:]))
    hip.synchronize()
    assert (np.asarray(out).view(np.uint8) == 0x7F).all(), 'a refusal wrote to the output block'
    hip.call(ENTRY, *good)                                      # and the device is still usable
    hip.synchronize()
    assert np.asarray(out)[160:164].tolist() == [1, 1, 1, 1]    # counts, found: one component an image


@pytest.mark.gpu
def test_public_path(hip, tmp_path):
    """The truncated mnist network at batch 3: components= is components.find (held to the loops above) on the request's own full Result,
    for a threshold and in the named form; a pass with the keyword and one without replay the same recording; rois feed a RoiInput."""
    from pyopenvino_amd import Components, ComponentScreen, RoiInput, components
    n = 3
    ex, net, name, out_name = _mnist_head(tmp_path, n)
    req = ex.requests[0]
    xd = hip.DeviceTensor.from_numpy(_pixels(10, n))
    full = np.array(req.infer({name: xd})[out_name], copy=True)
    assert full.shape == (n, 32, 26, 26) and np.isfinite(full).all()
    cut = float(np.median(full[:, 0][full[:, 0] > 0]))          # (behind a ReLU: the median of what is not zero)
    named = ComponentScreen(float(np.median(full[:, -1][full[:, -1] > 0])), -1, 4, 2, 8)
    for call, given in enumerate((cut, {out_name: named}, None, cut)):
        req.start_async({name: xd}, components=given)
        assert (req._replayed is not None) == (call >= 1), call                 # (the first pass above was eager, this start's first records)
        got = req.wait()[out_name]
        if given is None:
            assert np.array_equal(np.asarray(got), full)
            continue
        want = components.find(full, named if isinstance(given, dict) else given)
        assert isinstance(got, Components) and want.found.max() > 1 and want.counts.min() > 0
        _same(got, want, repr(given))
    assert sorted(ex.answers.blocks) == [(out_name, 0, 8, 256), (out_name, 31, 4, 8)]
    frames = np.zeros((n, 26, 26, 1), np.float32)
    assert RoiInput(frames, got.rois).rois.shape == (int(got.counts.sum()), 5) and (got.rois[:, 3:] >= 1).all()
    assert np.isfinite(components.oriented(got)).all()


@pytest.mark.gpu
def test_cascade_rows_behind_count_have_no_components(hip, tmp_path):
    """test_segments' cascade: GoogLeNet's first Convolution at batch 8 fed a DetectedRois with fewer survivors than rows; the quiet-NaN rows
    behind `count` have found = counts = 0, the rows before them are the rule on the full Result of the same feed."""
    from pyopenvino_amd import DetectedRois, IECore, components
    det_tests, roi_tests, keypoints_tests, top_k_tests = segments_tests.det_tests, segments_tests.roi_tests, segments_tests.keypoints_tests, segments_tests.top_k_tests
    rng = np.random.default_rng(501)
    n, m, hw, kind = 8, 2, (480, 640), 'U8-NHWC'
    frames = roi_tests._frames(rng, kind, m, hw)
    rec = det_tests._random_records(rng, m, 40, long=True)
    for conf in np.sort(rec[:, 2][np.isfinite(rec[:, 2])])[::-1][2:40]:          # the highest threshold that leaves 3 .. 7 survivors
        want = det_tests.detected_rois(rec, n, m, hw, min_confidence=float(conf))
        if 3 <= want.count < n:
            break
    assert 3 <= want.count < n, want.count
    conf = float(conf)
    ie = IECore(plugin_package=keypoints_tests.HIP)
    net = ie.read_network(keypoints_tests._heatmap_head('googlenet-v1', tmp_path), weights=top_k_tests._blob(11))
    net.set_batch(n)
    name, out_name = net.inputs[0]['name'], net.outputs[0]['name']
    det_tests._declare(net, name, kind, mean=roi_tests._mean())
    req = ie.load_network(net, 'GPU', num_requests=1).requests[0]
    full = np.array(req.infer({name: DetectedRois(frames, rec, min_confidence=conf)})[out_name], copy=True)
    assert (full[want.count:].view(np.uint32) == QUIET).all() and np.isfinite(full[:want.count]).all()
    cut = float(np.median(full[:want.count, 0]))
    got = req.infer({name: DetectedRois(frames, rec, min_confidence=conf)}, components=cut)[out_name]
    _same(got, components.find(full, cut), 'cascade')
    assert (got.found[:want.count] > 0).all() and not got.found[want.count:].any() and not got.counts[want.count:].any()
