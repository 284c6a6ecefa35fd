"""``infer(..., boxes=BoxScreen(tail=T), masks=...)``: instance masks made on the device (pvhip_dense_boxes_tail_f32, pvhip_instance_masks_f32).
tests/masks_ref.py is the rule in plain loops; pyopenvino_amd/masks.py (numpy) and the kernel equal it word for word."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import masks_ref
import test_boxes as boxes_tests
import test_keypoints as keypoints_tests
import test_text as text_tests
import test_top_k as top_k_tests

LAYOUTS = {'NCA': 'CXCYWH', 'NAC': 'XYXY'}              # each layout with one of the two box kinds
NAN, INF = np.float32(np.nan), np.float32(np.inf)
GUARD, SENTINEL = top_k_tests.GUARD, top_k_tests.SENTINEL
A, C = 12, 3                                            # anchors per image, classes: E = 4 + C + T


def _case(T, hp, wp, counts, layout):
    """(x as `layout`, protos, images, records, net_hw): n = len(counts) images whose kept rows are hand-made, counts[r] of them, walking
    the anchors round: 0 a box on integer pixel edges, 1 subnormal chains, 2 a chain that ends at -0.0 where the planes are tiny, 3 a NaN and 4 an
    inf coefficient, 5 a box wholly outside, 6 a box over everything, the others random boxes off the edges.  Pixel 1 is tiny in every plane, pixel 0 of
    the first image holds a NaN, the last pixel of the last image an inf.  Net (2 Hp + 1, 2 Wp): an even x edge stands exactly on a pixel edge."""
    rng = np.random.default_rng(1000 * T + hp * wp)
    n, hn, wn = len(counts), 2 * hp + 1, 2 * wp
    lo = np.stack([rng.integers(-2, wn, (n, A)), rng.integers(-2, hn, (n, A))], axis=2) + np.float32(0.25)
    xyxy = np.concatenate([lo, lo + rng.integers(1, 2 * max(hp, wp) + 2, (n, A, 2)) + np.float32(0.5)], axis=2).astype(np.float32)
    xyxy[:, 0] = (2 * (wp // 4), 2, 2 * (wp // 4) + 2 * ((wp + 1) // 2), hn - 1)
    xyxy[:, 5] = (wn + 1, 0, wn + 3, hn)
    xyxy[:, 6] = (-10, -10, wn + 10, hn + 10)
    box = xyxy if LAYOUTS[layout] == 'XYXY' else np.concatenate([(xyxy[..., :2] + xyxy[..., 2:]) / 2, xyxy[..., 2:] - xyxy[..., :2]], axis=2)
    m = rng.standard_normal((n, A, T)).astype(np.float32)
    m[:, 1] *= np.float32(1e-38)
    m[:, 2] = np.float32(-1e-30)
    m[:, 3, T - 1], m[:, 4, 0] = NAN, -INF
    protos = rng.standard_normal((n, T, hp, wp)).astype(np.float32)
    protos.reshape(n, T, -1)[:, :, 1] = np.float32(1e-30)
    protos.reshape(n, T, -1)[0, T - 1, 0], protos.reshape(n, T, -1)[n - 1, 0, -1] = NAN, INF
    v = np.concatenate([box.astype(np.float32), rng.random((n, A, C)).astype(np.float32), m], axis=2)
    images = np.repeat(np.arange(n), counts)
    records = np.concatenate([r * A + (np.arange(c) + r) % A for r, c in enumerate(counts)]).astype(np.int32)
    return boxes_tests._physical(v, layout), protos, images, records, (hn, wn)


def _found(images, records):
    from pyopenvino_amd import Detections
    return Detections(None, None, np.stack([images] + [0 * images] * 4, axis=1).astype(np.int32), None, None, np.asarray(records, np.int32))


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('shape', [(32, 8, 8), (5, 3, 7), (1, 2, 1), (64, 9, 33)])
def test_rule_equals_the_loops(shape, layout):
    from pyopenvino_amd import BoxScreen, masks
    T, hp, wp = shape
    x, protos, images, records, net = _case(T, hp, wp, (13, 0, 12), layout)
    for crop in (True, False):
        want = masks_ref.masks(x, layout, LAYOUTS[layout], T, protos, images, records, net, crop)
        got = masks.make(x, protos, _found(images, records), BoxScreen(layout=layout, box=LAYOUTS[layout], tail=T), net, crop)
        assert got.shape == (hp, wp) and got.words.dtype == np.uint32 and np.array_equal(got.words, want), (crop, np.argwhere(got.words != want)[:4])
        bits = masks.unpack(got)
        assert bits.shape == (25, hp, wp) and not bits[2].reshape(-1)[1] and not bits[3].any() and not bits[4].any() and not bits[:13, 0, 0].any()
        assert (crop or hp * wp == 2 or (bits[1].any() and bits[5].any())) and not (crop and bits[5].any()) and (crop or bits.any())      # (subnormals count)


@pytest.mark.parametrize('layout', LAYOUTS)
def test_the_tail_plays_no_part_in_boxes(layout):
    from pyopenvino_amd import BoxScreen, boxes
    x, _, _, _, net = _case(5, 3, 7, (1,), layout)
    cut = np.ascontiguousarray(x[:, :4 + C] if layout == 'NCA' else x[:, :, :4 + C])
    s = BoxScreen(0.3, layout, box=LAYOUTS[layout], threshold=0.9)
    got, want = boxes.decode(x, s._replace(tail=5), net), boxes.decode(cut, s, net)
    boxes_tests._same(got, want)
    assert want.counts.sum() > 2 and boxes.shape_of(x.shape, layout, False, 1, 5)[3] == C
    with pytest.raises(ValueError, match='tail = 8 channels'):          # (no class is left)
        boxes.decode(x, s._replace(tail=8), net)


def _seg_net(tmp_path, n, package=keypoints_tests.HIP):
    """mnist's first layer with two Results: the prototypes 'heatmaps' (n, 32, 26, 26) and 'text' (n, 32, 676): as 'NAC' 32 anchors, C = 640, T = 32."""
    from pyopenvino_amd import IECore
    base = keypoints_tests._heatmap_head('mnist', tmp_path)
    xml, weights = os.path.join(str(tmp_path), 'mnist_seg.xml'), os.path.join(str(tmp_path), 'mnist_seg.bin')
    blob = text_tests._with_text_chain(base, xml, open(os.path.join(text_tests.MODELS, 'mnist.bin'), 'rb').read(), None, False, [0, 32, 676])
    with open(weights, 'wb') as f:
        f.write(blob)
    net = IECore(plugin_package=package).read_network(xml, weights=weights)
    net.set_batch(n)
    return IECore(plugin_package=package).load_network(net, 'GPU', num_requests=1), net.inputs[0]['name']


HEAD = dict(layout='NAC', box='XYXY', tail=32, threshold=1.0)


def test_refusals_and_the_host_route(tmp_path):
    """Every refusal is a ValueError('masks: ...') before anything is staged; a plugin set that computes on the host gets the numpy rule."""
    from pyopenvino_amd import BoxScreen, Masks, MaskScreen, boxes, masks
    n, head = 2, BoxScreen(0.0, **HEAD)
    ex, name = _seg_net(tmp_path, n, 'oracle.op_plugins')
    x = keypoints_tests._pixels(10, n)
    for match, kw in (('boxes= in the same call', dict(masks=True)),
                      ('asks for 0 Results with tail = 32', dict(boxes={'text': head._replace(tail=8)}, masks=True)),
                      ('head \'heatmaps\' is not asked for', dict(boxes={'text': head}, masks=MaskScreen('heatmaps'))),
                      ('head \'text\' is asked for with tail = 8', dict(boxes={'text': head._replace(tail=8)}, masks={'heatmaps': MaskScreen('text')})),
                      ('has shape \\(2, 32, 676\\): not rank 4', dict(boxes={'text': head}, masks={'text': True})),
                      ('asked for with keypoints as well', dict(boxes={'text': head}, masks=True, keypoints={'heatmaps': True})),
                      ('a MaskScreen or True', dict(boxes={'text': head}, masks=0.5)), ('crop is a bool', dict(boxes={'text': head}, masks=MaskScreen(crop=1))),
                      ('no Result named', dict(boxes={'text': head}, masks={'nope': True}))):
        with pytest.raises(ValueError, match=match) as e:
            ex.infer({name: x}, **kw)
        assert str(e.value).startswith('masks: '), str(e.value)
    with pytest.raises(ValueError, match='masks: not with a batch sharded'):
        masks.checked(ex.ienet, True, {'text': head}, True)
    h, named = boxes.resolved(head), {'heatmaps': True}
    for match, value, heads, port in (('asks for 2 Results with tail = 32 .*head= names the one', True, {'text': h, 'other': h}, {}),
                                      ('is FP16: FP32 Results only', named, {'text': h}, dict(precision='FP16')), ('no FP32 Result of rank 4', True, {'text': h}, dict(precision='FP16')),
                                      ('shape \\(3, 32, 26, 26\\): not rank 4 .* n = 2 first', named, {'text': h}, dict(dims=(3, 32, 26, 26))),
                                      ('shape \\(2, 65, 26, 26\\): not rank 4', named, {'text': h}, dict(dims=(2, 65, 26, 26))), ('shape \\(2, 0, 26, 26\\): not', named, {'text': h}, dict(dims=(2, 0, 26, 26))),
                                      ('asks for 0 Results with tail = 16', True, {'text': h}, dict(dims=(2, 16, 26, 26))), ('more than 2\\^26: lower max_per_image', True, {'text': h}, dict(dims=(2, 32, 4096, 4096)))):
        with pytest.raises(ValueError, match='^masks: .*' + match):
            _checked_with(ex, value, heads, port)
    full = ex.infer({name: x})
    got = ex.infer({name: x}, boxes={'text': head}, masks=True)
    found = boxes.decode(full['text'], head, (28, 28))
    boxes_tests._same(got['text'], found)
    assert isinstance(got['heatmaps'], Masks) and found.counts.min() > 0
    assert np.array_equal(got['heatmaps'].words, masks_ref.masks(full['text'], 'NAC', 'XYXY', 32, full['heatmaps'], found.rois[:, 0], found.records, (28, 28))) and masks.unpack(got['heatmaps']).any()


def _checked_with(ex, value, heads, fields):                             # (masks.checked with the port of 'heatmaps' declared as `fields` say)
    from pyopenvino_amd import masks
    port = next(iter(ex.ienet.G.nodes[[nid for nid, name in ex.ienet.find_node_by_type('Result') if name == 'heatmaps'][0]]['input'].values()))
    old = {k: port[k] for k in fields}
    port.update(fields)
    try:
        masks.checked(ex.ienet, value, heads, False)
    finally:
        port.update(old)


def _device_masks(hip, x, layout, T, protos, counts, records, net, crop, offset=0):
    """The entry behind a hand-written header and rows; the words between sentinels, rows from total on untouched."""
    n, hp, wp = protos.shape[0], protos.shape[2], protos.shape[3]
    w32, per, total, E = (hp * wp + 31) // 32, max(max(counts), 1), int(sum(counts)), x.shape[1] if layout == 'NCA' else x.shape[2]
    rows = np.zeros((n * per, 8), np.int32)
    rows[:total, 7] = records
    dev = [hip.DeviceTensor.from_numpy(t) for t in (x, np.concatenate([np.full(offset, 9e9, np.float32), protos.ravel()]),
                                                    np.asarray(list(counts) + [0] * n + [total], np.int32), rows)]
    words = hip.DeviceTensor.empty((n * per * w32 + 2 * GUARD,), np.int32)
    hip.call('pvhip_memset', ctypes.c_void_p(words.ptr), 0x7f, words.nbytes)
    hip.call('pvhip_instance_masks_f32', hip.ptr(dev[0]), n, A, E, list(LAYOUTS).index(layout), E - T, T, ['CXCYWH', 'XYXY'].index(LAYOUTS[layout]),
             ctypes.c_void_p(dev[1].ptr + 4 * offset), hp, wp, net[0], net[1], int(crop), per, hip.ptr(dev[2]), hip.ptr(dev[3]), ctypes.c_void_p(words.ptr + 4 * GUARD))
    w = np.asarray(words)
    assert (w[:GUARD] == SENTINEL).all() and (w[GUARD + total * w32:] == SENTINEL).all(), 'a word outside the rows below total was written'
    return w[GUARD:GUARD + total * w32].view(np.uint32).reshape(total, w32)


@pytest.mark.gpu
@pytest.mark.parametrize('T', [1, 5, 32, 64])
@pytest.mark.parametrize('plane', [(1, 31), (4, 8), (3, 11), (1, 64 * 4 + 1)])
def test_kernel_equals_the_rule(hip, plane, T):
    """Hp * Wp around a group of 32 pixels and one past 64 g; T at both ends, odd, and 32; counts around a block of 32 detections and one more
    than the staged chunk, uneven over three images; both layouts, crop on and off, each with each; crop on and off, the prototypes one float off; three calls, the same words."""
    from pyopenvino_amd import masks
    for layout, counts in itertools.product(LAYOUTS, ((33, 0, masks.STAGE + 1), (1, 32, 0))):
        x, protos, images, records, net = _case(T, plane[0], plane[1], counts, layout)
        for crop in (True, False):
            want = masks_ref.masks(x, layout, LAYOUTS[layout], T, protos, images, records, net, crop)
            for offset in (0, 1, 0):
                got = _device_masks(hip, x, layout, T, protos, counts, records, net, crop, offset)
                assert np.array_equal(got, want) and (crop or want.any()), (layout, crop, offset, np.argwhere(got != want)[:4].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize('tail', [1, 32])
def test_tail_entry_equals_decode(hip, tail):
    """The planes form and both rows forms, the length read on either side of PVHIP_BOXES_TEAM_ROW, with `tail` channels stepped over."""
    from pyopenvino_amd import BoxScreen, boxes, detections
    switch, rng, n, anchors = boxes_tests._rows_switch(), np.random.default_rng(tail), 2, 70
    for layout, read in (('NCA', 9), ('NAC', switch), ('NAC', switch + 1)):
        v = np.concatenate([boxes_tests._boxes(rng, n, anchors), rng.random((n, anchors, read - 4 + tail)).astype(np.float32)], axis=2)
        v[:, :, read:] = 9.0                                                    # a tail that would win every anchor if it were read
        x, s = boxes_tests._physical(v, layout), boxes.resolved(BoxScreen(0.5, layout, tail=tail, max_per_image=40))
        want = boxes.decode(x, s, boxes_tests.NET)
        assert hip.call(boxes_tests.FORM, boxes.LAYOUTS[layout], anchors, read) == (1 if layout == 'NCA' else 2 + (read > switch)) and 0 < want.counts.sum()
        blocks = boxes.Blocks(n, anchors, s._replace(min_score=None))
        blocks.launch(hip.DeviceTensor.from_numpy(x), s.min_score, boxes_tests.NET, (0, 0, 64, 64))
        boxes_tests._same(blocks.read_back(), want, '{} {}'.format(layout, read))
        assert (want.labels < read - 4).all() and isinstance(blocks.read_back(), detections.Detections)


@pytest.mark.gpu
def test_public_path(hip, tmp_path):
    """boxes= + masks= equal the host rule on the request's own full Results; the passes replay the recording; both Results stay on the device."""
    from pyopenvino_amd import BoxScreen, Masks, MaskScreen, boxes, masks
    n = 3
    ex, name = _seg_net(tmp_path, n)
    req, xd = ex.requests[0], hip.DeviceTensor.from_numpy(keypoints_tests._pixels(10, n))
    req.infer({name: xd})
    full = {k: np.array(v, copy=True) for k, v in req.infer({name: xd}).items()}      # (the next pass replays)
    head = BoxScreen(float(np.quantile(full['text'][:, :, 4:644].max(axis=2), 0.5)), max_per_image=20, **HEAD)
    found = boxes.decode(full['text'], head, (28, 28))
    assert 0 < found.counts.sum() < 32 * n and len(set(found.counts.tolist())) > 1
    req.infer({name: xd}, boxes={'text': head}, masks=True)                 # (behind it no whole Result of the passes above is owed a copy)
    real_call = hip.call
    for given, crop in ((True, True), ({'heatmaps': MaskScreen('text', False)}, False), (MaskScreen(), True)):
        want = masks.make(full['text'], full['heatmaps'], found, head, (28, 28), crop)
        assert np.array_equal(want.words, masks_ref.masks(full['text'], 'NAC', 'XYXY', 32, full['heatmaps'], found.rois[:, 0], found.records, (28, 28), crop))
        copied = []
        hip.call = lambda entry, *args: (copied.append(args[2]) if entry == 'pvhip_memcpy_d2h' else None, real_call(entry, *args))[1]
        try:
            req.start_async({name: xd}, boxes={'text': head}, masks=given)
            replayed = req._replayed is not None
            got = req.wait()
        finally:
            hip.call = real_call
        boxes_tests._same(got['text'], found)
        assert isinstance(got['heatmaps'], Masks) and got['heatmaps'].shape == (26, 26) and np.array_equal(got['heatmaps'].words, want.words), crop
        total = int(found.counts.sum())
        assert replayed and sorted(copied) == sorted([4 * (2 * n + 1), 32 * total, 4 * total * 22]), copied
        for k in full:
            assert np.array_equal(text_tests._on_device(hip, req, k), full[k])
    assert want.words.any() and len(req.runner.answers.blocks) == 2
