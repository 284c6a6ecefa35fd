"""``infer(..., boxes=BoxScreen(tail=T), masks=...)``: instance masks made on the device (pvhip_dense_boxes_tail_f32, pvhip_instance_masks_f32).
tests/masks_ref.py is the rule in plain loops; pyopenvino_amd/masks.py (numpy) and the kernel equal it word for word."""
import ctypes
import functools
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


def _case(T, hp, wp, counts, layout, records=None, objectness=False, net=None):
    """(x as `layout`, protos, images, records, net_hw): n = len(counts) images whose kept rows are hand-made, counts[r] of them, walking
    the anchors round: 0 a box on integer pixel edges, 1 subnormal chains, 2 a chain that ends at -0.0 where the planes are tiny, 3 a NaN and 4 an
    inf coefficient, 5 a box wholly outside, 6 a box over everything, the others random boxes off the edges.  Pixel 1 is tiny in every plane, pixel 0 of
    the first image holds a NaN, the last pixel of the last image an inf, pixel 2 an inf in plane 1 of every image.  Net (2 Hp + 1, 2 Wp): an even
    x edge stands exactly on a pixel edge.
    `records`: the rows' records r * A + a written out by hand, in the order of the images, in place of the walk; `objectness`: a fifth
    column stands between the box and the classes; `net`: (Hn, Wn) in place of (2 Hp + 1, 2 Wp)."""
    rng = np.random.default_rng(1000 * T + hp * wp)
    n, (hn, wn) = len(counts), net or (2 * hp + 1, 2 * wp)
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
    if T > 1 and hp * wp > 3:
        protos.reshape(n, T, -1)[:, 1, 2] = INF         # (plane 1: an odd t, which the other half of a wave holds; inf * m is +inf for half the anchors)
    parts = [box.astype(np.float32), rng.random((n, A, C)).astype(np.float32), m]
    if objectness:
        parts.insert(1, rng.random((n, A, 1)).astype(np.float32))
    v = np.concatenate(parts, axis=2)
    images = np.repeat(np.arange(n), counts)
    if records is None:
        records = np.concatenate([r * A + (np.arange(c) + r) % A for r, c in enumerate(counts)])
    records = np.asarray(records, np.int32)
    assert records.shape == images.shape and (records // A == images).all()           # every record inside its image
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


def _device_masks(hip, x, layout, T, protos, counts, records, net, crop, offset=0, per_image=None, head_offset=0, words_offset=0):
    """The entry behind a hand-written header and rows; the words between sentinels, rows from total on untouched.  `offset`, `head_offset`:
    the prototypes, the head start that many floats behind a 16-byte boundary; `words_offset`: the words that many words behind one;
    `per_image`: max_per_image, the largest count when None."""
    n, hp, wp = protos.shape[0], protos.shape[2], protos.shape[3]
    anchors, E = (x.shape[2], x.shape[1]) if layout == 'NCA' else x.shape[1:]
    w32, per, total = (hp * wp + 31) // 32, per_image or max(max(counts), 1), int(sum(counts))
    assert len(counts) == n and 0 <= min(counts) and max(counts) <= per and len(records) == total      # a header the entry is owed
    rows = np.zeros((n * per, 8), np.int32)
    rows[:total, 7] = records
    dev = [hip.DeviceTensor.from_numpy(t) for t in (np.concatenate([np.full(head_offset, 9e9, np.float32), x.ravel()]),
                                                    np.concatenate([np.full(offset, 9e9, np.float32), protos.ravel()]),
                                                    np.asarray(list(counts) + [0] * n + [total], np.int32), rows)]
    front = GUARD + words_offset
    words = hip.DeviceTensor.empty((n * per * w32 + front + GUARD,), np.int32)
    assert dev[0].ptr % 16 == 0 and dev[1].ptr % 16 == 0 and words.ptr % 16 == 0 and GUARD % 4 == 0
    hip.call('pvhip_memset', ctypes.c_void_p(words.ptr), 0x7f, words.nbytes)
    hip.call('pvhip_instance_masks_f32', ctypes.c_void_p(dev[0].ptr + 4 * head_offset), n, anchors, E, list(LAYOUTS).index(layout), E - T, T,
             ['CXCYWH', 'XYXY'].index(LAYOUTS[layout]), ctypes.c_void_p(dev[1].ptr + 4 * offset), hp, wp, net[0], net[1], int(crop), per,
             hip.ptr(dev[2]), hip.ptr(dev[3]), ctypes.c_void_p(words.ptr + 4 * front))
    w = np.asarray(words)
    assert (w[:front] == SENTINEL).all() and (w[front + total * w32:] == SENTINEL).all(), 'a word outside the rows below total was written'
    return w[front:front + total * w32].view(np.uint32).reshape(total, w32)


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


# ---------------------------------------------------------------------------------------------------------------- every form and seam
# The kernel has four instantiations (PAIRS = 4 / 8 / 16 / 32 for T <= 8 / 16 / 32 / 64), stages an image's detections PVHIP_MASKS_STAGE at
# a time, finds an image's first row by a sum strided over 64 lanes, and gives a workgroup 16 words = 512 pixels of a plane.  Each case
# below stands on one of those seams; the loops' answer is made once per (case, layout, crop) and serves the host test, which holds the
# numpy rule to it, and the device test.
STAGE = 128                                             # PVHIP_MASKS_STAGE
MAX_PER_IMAGE = 4096                                    # PVHIP_BOXES_MAX_CANDIDATES
VOID_FIRST, MASK_FIRST = (0, 1, 31, 32, 63, 127), (2, 33, 64, 96, 126)      # chunk positions d, below and from 32 on


def _chunk_records(count):
    """One image's records: at a position d of VOID_FIRST the even chunks hold a void detection (anchor 3, a NaN, or 4, an inf coefficient)
    and the odd chunks anchor 6, whose box is over everything; at a d of MASK_FIRST the other way round; elsewhere the walk."""
    out = []
    for i in range(count):
        chunk, d = divmod(i, STAGE)
        void_here = (chunk % 2 == 0) == (d in VOID_FIRST)
        out.append(i % A if d not in VOID_FIRST + MASK_FIRST else 3 + (d + chunk) % 2 if void_here else 6)
    return tuple(out)


SEAMS = {'forms T {}'.format(T): dict(T=T, plane=(3, 11), counts=(33, 0, 5)) for T in (7, 8, 9, 15, 16, 17, 31, 33, 63)}
SEAMS.update({'chunks {}'.format(c): dict(T=5, plane=(1, 33), counts=(c,), records=_chunk_records(c)) for c in (STAGE, 2 * STAGE, 2 * STAGE + 40)})
SEAMS['chunks {}'.format(MAX_PER_IMAGE)] = dict(T=3, plane=(1, 33), counts=(MAX_PER_IMAGE,), crops=(False,))
SEAMS['images 130'] = dict(T=2, plane=(1, 33), counts=tuple((1, 2, 0, 3)[r % 4] for r in range(130)), per_image=3)
SEAMS['room above the counts'] = dict(T=5, plane=(3, 11), counts=(3, 0, 5), per_image=7)
SEAMS.update({'plane {} x {} T {}'.format(hp, wp, T): dict(T=T, plane=(hp, wp), counts=(33, STAGE + 1))
              for hp, wp in ((23, 29), (1, 16 * 32 * 2 + 1), (17, 31)) for T in (5, 16)})
SEAMS['objectness'] = dict(T=9, plane=(3, 11), counts=(33, 0, 5), objectness=True)
SEAMS['alignment'] = dict(T=5, plane=(3, 11), counts=(33, 0, 5))


@functools.lru_cache(maxsize=None)
def _seam(name, layout):
    """_case of SEAMS[name], made once, read-only."""
    c = SEAMS[name]
    case = _case(c['T'], c['plane'][0], c['plane'][1], c['counts'], layout, c.get('records'), c.get('objectness', False), c.get('net'))
    for t in case[:4]:
        t.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def _seam_want(name, layout, crop):
    """The loops' answer for the case, made once, read-only, with what the case is there for asserted on it: a case must not go vacuous."""
    x, protos, images, records, net = _seam(name, layout)
    c = SEAMS[name]
    want = masks_ref.masks(x, layout, LAYOUTS[layout], c['T'], protos, images, records, net, crop)
    want.setflags(write=False)
    hw, count = c['plane'][0] * c['plane'][1], c['counts'][0]
    assert want.any() and want.shape == (sum(c['counts']), (hw + 31) // 32)
    assert hw % 32 == 0 or not (want[:, -1] >> np.uint32(hw % 32)).any()                  # bits at and beyond Hp * Wp are 0
    if 'records' in c:                                     # the arrangement: an empty row, bits STAGE further on, and the reverse
        pairs = [(i, i + STAGE, (i // STAGE % 2 == 0) == (i % STAGE in VOID_FIRST)) for i in range(count - STAGE) if i % STAGE in VOID_FIRST + MASK_FIRST]
        assert len(pairs) == {STAGE: 0, 2 * STAGE: 11, 2 * STAGE + 40: 17}[count]
        for i, j, void_first in pairs:
            assert want[j if void_first else i].any() and not want[i if void_first else j].any(), (name, i, j)
        for far in (False, True):                          # both ways round, below position 32 and from it on
            assert not pairs or {void_first for i, _, void_first in pairs if (i % STAGE >= 32) == far} == {False, True}
    if name.startswith('images'):
        assert STAGE == 128 and len(c['counts']) == 130 and all(c['counts'][r] > 0 for r in (63, 64, 65, 127, 128, 129)) and set(c['counts']) == {0, 1, 2, 3}
        assert len({protos[r].tobytes() for r in range(130)}) == 130                     # a row under another image's planes differs
    if name.startswith('plane') and crop:                  # the crop takes some set bits away and leaves others
        free = _seam_want(name, layout, False)
        assert not (want & ~free).any() and (free & ~want).any() and hw > 512 and ((hw + 31) // 32) % 4 != 0
    return want


def _seams():
    return [pytest.param(name, id=name.replace(' ', '_')) for name in SEAMS]


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('name', _seams())
def test_rule_equals_the_loops_at_every_seam(name, layout):
    """masks.make at every case the device tests below run, objectness column included: the numpy rule is held at the same edges."""
    from pyopenvino_amd import BoxScreen, masks
    assert masks.STAGE == STAGE and masks.boxes.MAX_CANDIDATES == MAX_PER_IMAGE
    c = SEAMS[name]
    x, protos, images, records, net = _seam(name, layout)
    screen = BoxScreen(layout=layout, box=LAYOUTS[layout], objectness=c.get('objectness', False), tail=c['T'])
    for crop in c.get('crops', (True, False)):
        got = masks.make(x, protos, _found(images, records), screen, net, crop)
        want = _seam_want(name, layout, crop)
        assert got.shape == c['plane'] and np.array_equal(got.words, want), (crop, np.argwhere(got.words != want)[:4].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize('name', _seams())
def test_kernel_at_every_seam(hip, name):
    """forms: each instantiation at its smallest, its largest and an odd T (with the four of test_kernel_equals_the_rule: <4> 1 5 7 8,
    <8> 9 15 16, <16> 17 31 32, <32> 33 63 64).  chunks: counts of exactly one, exactly two and two and a part chunks, a void detection
    and a masked one at the same chunk position in consecutive chunks, both ways round; 4096 rows of one image.  images: 130 of them,
    so the strided sum of the counts in front takes a second and a third step.  room: max_per_image above every count.  planes: two and
    three workgroups an image, the last wave partly filled.  objectness: tail_at = 5 + C.  Both layouts, crop on and off."""
    c = SEAMS[name]
    for layout in LAYOUTS:
        x, protos, images, records, net = _seam(name, layout)
        for crop in c.get('crops', (True, False)):
            want = _seam_want(name, layout, crop)
            got = _device_masks(hip, x, layout, c['T'], protos, c['counts'], records, net, crop, per_image=c.get('per_image'))
            assert np.array_equal(got, want), (layout, crop, np.argwhere(got != want)[:4].tolist())


@pytest.mark.gpu
def test_kernel_reads_and_writes_at_every_phase(hip):
    """`head` 1, 2 and 3 floats and `words` one word behind a 16-byte boundary, each with each and with the prototypes one float off."""
    for layout in LAYOUTS:
        x, protos, images, records, net = _seam('alignment', layout)
        for head_offset, words_offset, offset in itertools.product((0, 1, 2, 3), (0, 1), (0, 1)):
            crop = bool((head_offset + words_offset + offset) % 2)
            got = _device_masks(hip, x, layout, 5, protos, (33, 0, 5), records, net, crop, offset, None, head_offset, words_offset)
            want = _seam_want('alignment', layout, crop)
            assert np.array_equal(got, want), (layout, crop, head_offset, words_offset, offset, np.argwhere(got != want)[:4].tolist())


# ---------------------------------------------------------------------------------------------------------------- the crop's arithmetic
CROP_NET, CROP_PLANE = (1 << 24, (1 << 24) - 1), (5, 37)
ODD = (INF, -INF, np.float32(3e38), np.float32(-3e38), np.float32(1e-45), np.float32(-0.0), NAN)


def _beside(p, n):
    """[(corner v, pixel q, v * p - q * n)] with the differences -1, 0 and +1, v an integer below 2^24 and so exact in fp32.  p and n are
    coprime here, so v p = q n has no solution with 0 < q < p -- the 0 stands at pixel 0 -- and v p = q n + 1 and v p = q n - 1 have one
    each, at different pixels q and p - q: v is the inverse of p modulo n, or n less that."""
    v = pow(p, -1, n)
    out = [(n - v, ((n - v) * p + 1) // n, -1), (0, 0, 0), (v, (v * p - 1) // n, 1)]
    assert all(v * p - q * n == d and 0 <= v < 1 << 24 and 0 <= q < p and (q > 0 or d == 0) for v, q, d in out)
    return out


@functools.lru_cache(maxsize=None)
def _crop_case(layout):
    """(x, protos, records, named, want with crop, want without): one image, T = 1, every coefficient and plane value positive, so that
    without crop every bit is set and the crop alone decides.  Detections 3 k .. 3 k + 2, for corner k of xa, ya, xb, yb: that corner stands
    -1, 0, +1 beside a pixel's edge (_beside), the other three leave everything in -- the opposite corner one further in (an upper one)
    or out (a lower one) where that makes centre and half extent of 'CXCYWH' integers too, hence exact.  `named`: [(row, py, px, difference, lower corner)].  Then a
    detection per corner and value of ODD standing in that box number, the others as before; then one with box numbers 0 and 2 inf."""
    (hn, wn), (hp, wp) = CROP_NET, CROP_PLANE
    rng = np.random.default_rng(24)
    corners, named = [], []
    whole = [-1, 0, wn, hn]                                                               # (all four of its 'CXCYWH' numbers are integers)
    for k in range(4):
        p, n = ((wp, wn), (hp, hn))[k % 2]
        for v, q, d in _beside(p, n):
            c = list(whole)
            c[k], c[k ^ 2] = v, (n - ((n - v) & 1) if k < 2 else -(v & 1))
            named.append((len(corners), 2 if k % 2 == 0 else q, q if k % 2 == 0 else 5, d, k < 2))
            corners.append(c)
    as_box = lambda c: c if LAYOUTS[layout] == 'XYXY' else [(c[0] + c[2]) // 2, (c[1] + c[3]) // 2, c[2] - c[0], c[3] - c[1]]
    box = np.array([as_box(c) for c in corners] + [as_box(whole)] * (4 * len(ODD) + 1), np.float32)
    assert all((c[2] - c[0]) % 2 == 0 and (c[3] - c[1]) % 2 == 0 for c in corners + [whole])
    for k in range(4):
        box[len(corners) + len(ODD) * k:len(corners) + len(ODD) * (k + 1), k] = ODD
    box[-1, [0, 2]] = INF
    for j, c in enumerate(corners):                                                       # the fp32 corners are exactly those integers
        xa, xb, ya, yb = masks_ref.corners(box[j], LAYOUTS[layout])
        assert [float(xa), float(ya), float(xb), float(yb)] == [float(v) for v in c], (layout, j)
    anchors = len(box)
    v = np.concatenate([box[None], rng.random((1, anchors, C)).astype(np.float32), 0.5 + rng.random((1, anchors, 1)).astype(np.float32)], axis=2)
    protos = (0.5 + rng.random((1, 1, hp, wp))).astype(np.float32)
    x, records = boxes_tests._physical(v, layout), np.arange(anchors, dtype=np.int32)
    want = [masks_ref.masks(x, layout, LAYOUTS[layout], 1, protos, np.zeros(anchors, np.int64), records, CROP_NET, crop) for crop in (True, False)]
    for t in (x, protos, records) + tuple(want):
        t.setflags(write=False)
    bits = np.unpackbits(want[1].view(np.uint8), axis=1, bitorder='little')
    assert bits[:, :hp * wp].all() and not bits[:, hp * wp:].any()                          # without crop: every bit of the plane
    fp32_cannot_tell = []
    for row, py, px, d, lower in named:                    # the named pixel: inside a lower corner at -1 and 0, inside an upper one at +1
        q = py * wp + px
        assert bool(want[0][row, q >> 5] >> np.uint32(q & 31) & 1) == ((d <= 0) if lower else (d > 0)), (layout, row)
        (p, n), (vv, qq) = ((wp, wn), (hp, hn))[row // 3 % 2], (corners[row][row // 3], (px, py)[row // 3 % 2])
        fp32_cannot_tell.append(d != 0 and np.float32(vv) * np.float32(p) == np.float32(qq) * np.float32(n))
    for k in range(4):                                     # a triple's three masks differ
        assert len({want[0][3 * k + i].tobytes() for i in range(3)}) == 3, (layout, k)
    assert sum(fp32_cannot_tell) >= 6                       # (products rounded to fp32 are equal where the exact ones differ by one)
    assert len({w.tobytes() for w in want[0][len(corners):]}) >= 3 and not want[0][-1].any()
    return x, protos, records, named, want[0], want[1]


@pytest.mark.parametrize('layout', LAYOUTS)
def test_rule_crops_exactly(layout):
    """Products up to 2^24 * 2^24 that differ by one: masks.make agrees with the loops, whose own answer _crop_case holds to the text."""
    from pyopenvino_amd import BoxScreen, masks
    x, protos, records, _, cropped, free = _crop_case(layout)
    for crop, want in ((True, cropped), (False, free)):
        got = masks.make(x, protos, _found(np.zeros(len(records), np.int64), records), BoxScreen(layout=layout, box=LAYOUTS[layout], tail=1), CROP_NET, crop)
        assert np.array_equal(got.words, want), (crop, np.argwhere(got.words != want)[:4].tolist())


@pytest.mark.gpu
def test_kernel_crops_exactly(hip):
    """Net (2^24, 2^24 - 1) over a plane of (5, 37): corner times plane extent and pixel times net extent need 48 bits and stand one apart,
    on either side of `<=` and of `<`; a finite coefficient with an infinite, a huge, a subnormal, a -0.0 and a NaN box number."""
    for layout in LAYOUTS:
        x, protos, records, named, cropped, free = _crop_case(layout)
        for crop, want in ((True, cropped), (False, free)):
            got = _device_masks(hip, x, layout, 1, protos, (len(records),), records, CROP_NET, crop)
            assert np.array_equal(got, want), (layout, crop, np.argwhere(got != want)[:4].tolist())


# ---------------------------------------------------------------------------------------------------------------- objectness, refusals
@pytest.mark.gpu
def test_masks_behind_a_head_with_objectness(hip):
    """masks.Blocks.launch behind boxes.Blocks.launch, as a request runs them, on a head with the fifth column: tail_at = 5 + C in both
    entries.  T = 9: the second instantiation at its smallest T."""
    from pyopenvino_amd import BoxScreen, boxes, masks
    rng, n, anchors, T, plane = np.random.default_rng(9), 2, 70, 9, (6, 7)
    for layout, kind in LAYOUTS.items():
        v = np.concatenate([boxes_tests._boxes(rng, n, anchors, kind == 'XYXY'), 0.5 + rng.random((n, anchors, 1)).astype(np.float32) / 2,
                            rng.random((n, anchors, C)).astype(np.float32), rng.standard_normal((n, anchors, T)).astype(np.float32)], axis=2)
        protos = rng.standard_normal((n, T) + plane).astype(np.float32)
        x, s = boxes_tests._physical(v, layout), boxes.resolved(BoxScreen(0.4, layout, True, kind, tail=T, max_per_image=40))
        found = boxes.decode(x, s, boxes_tests.NET)
        assert 2 < found.counts.min() and found.counts.sum() < found.selected.sum() <= n * anchors
        head, xd, pd = boxes.Blocks(n, anchors, s._replace(min_score=None)), hip.DeviceTensor.from_numpy(x), hip.DeviceTensor.from_numpy(protos)
        mine = masks.Blocks(n, s.max_per_image, (T,) + plane)
        for crop in (True, False):
            head.launch(xd, s.min_score, boxes_tests.NET, (0, 0, 64, 64))
            mine.launch(pd, xd, head, s, boxes_tests.NET, crop)
            boxes_tests._same(head.read_back(), found, layout)
            got, want = mine.read_back(), masks.make(x, protos, found, s, boxes_tests.NET, crop)
            assert np.array_equal(want.words, masks_ref.masks(x, layout, kind, T, protos, found.rois[:, 0], found.records, boxes_tests.NET, crop))
            assert got.shape == plane and np.array_equal(got.words, want.words) and want.words.any(), (layout, crop)


def _entry_args(hip, n, anchors, E, T, plane, per, keep):
    """Arguments of a call the entry takes, with room behind every pointer and a header of zeros: no row, no word is owed.  `keep` holds
    the tensors."""
    w32 = (plane[0] * plane[1] + 31) // 32
    sizes = (n * anchors * E, n * T * plane[0] * plane[1], 2 * n + 1, 8 * n * per, n * per * w32)
    t = [hip.DeviceTensor.empty((size,), np.float32 if i < 2 else np.int32) for i, size in enumerate(sizes)]
    hip.call('pvhip_memset', ctypes.c_void_p(t[2].ptr), 0, t[2].nbytes)
    keep.extend(t)
    return [hip.ptr(t[0]), n, anchors, E, 1, E - T, T, 1, hip.ptr(t[1]), plane[0], plane[1], 7, 22, 1, per, hip.ptr(t[2]), hip.ptr(t[3]), hip.ptr(t[4])]


@pytest.mark.gpu
def test_entry_rejects_what_it_cannot_do(hip):
    """One good call, then one argument at a time made bad: PvhipError, and not a word written.  Every limit of the entry's paragraph in
    pvhip.h from both sides; the sides that other tests of this file stand on are named where they are left out."""
    ENTRY = 'pvhip_instance_masks_f32'
    x, protos, images, records, net = _seam('room above the counts', 'NAC')
    counts, per, T, (hp, wp), n, E = (3, 0, 5), 7, 5, (3, 11), 3, 4 + C + 5
    rows = np.zeros((n * per, 8), np.int32)
    rows[:len(records), 7] = records
    head, planes, rows = (hip.DeviceTensor.from_numpy(t) for t in (x, protos, rows))
    header = hip.DeviceTensor.from_numpy(np.asarray((0,) + counts + (0,) * n + (sum(counts),), np.int32))     # (one word in front: it starts 4 bytes off)
    words = hip.DeviceTensor.empty((n * per * 2 + 2 * GUARD,), np.int32)
    hip.call('pvhip_memset', ctypes.c_void_p(words.ptr), 0x7f, words.nbytes)
    off = lambda t, nbytes: ctypes.c_void_p(t.ptr + nbytes)
    good = [hip.ptr(head), n, A, E, 1, E - T, T, 1, hip.ptr(planes), hp, wp, net[0], net[1], 1, per, off(header, 4), hip.ptr(rows), off(words, 4 * GUARD)]
    untouched = lambda: bool((np.asarray(words) == SENTINEL).all())
    assert head.ptr % 16 == 0 and planes.ptr % 16 == 0 and header.ptr % 16 == 0 and rows.ptr % 16 == 0 and words.ptr % 16 == 0 and untouched()

    def good_call_equals_the_rule():
        hip.call(ENTRY, *good)
        want = _seam_want('room above the counts', 'NAC', True)
        got = np.asarray(words)[GUARD:-GUARD].view(np.uint32)
        assert np.array_equal(got[:want.size].reshape(want.shape), want) and (got[want.size:] == SENTINEL).all()
        hip.call('pvhip_memset', ctypes.c_void_p(words.ptr), 0x7f, words.nbytes)

    good_call_equals_the_rule()
    assert untouched()
    bads =[(i, None) for i in (0, 8, 15, 16, 17)]                                          # a null pointer
    bads += [(0, off(head, 2)), (8, off(planes, 2)), (15, off(header, 6)), (17, off(words, 4 * GUARD + 2))]      # off a 4-byte boundary
    bads += [(16, off(rows, 4)), (16, off(rows, 8)), (16, off(rows, 12))]                   # rows: on a 4-byte, off the 16-byte boundary
    bads += [(1, 0), (1, -1), (1, 65536), (2, 0), (2, -1), (3, 0), (3, E - 1), (4, -1), (4, 2), (7, -1), (7, 2), (13, -1), (13, 2)]
    bads += [(5, 3), (5, E - T + 1), (6, 0), (6, -1), (6, 65), (9, 0), (9, -1), (10, 0), (10, -1), (10, (1 << 24) + 1)]
    bads += [(i, bad) for i in (11, 12) for bad in (0, -1, (1 << 24) + 1)] + [(14, 0), (14, -1), (14, MAX_PER_IMAGE + 1)]
    several = [{9: 1, 10: 1}, {9: 4097, 10: 4096}]                                          # Hp * Wp of 1 and beyond 2^24
    several += [{1: 1, 2: 1 << 27, 3: 16}, {1: 1 << 15, 2: 1 << 12, 3: 16}]                 # n * a * e = 2^31
    at_the_limit = {1: 16, 14: MAX_PER_IMAGE, 9: 128, 10: 256}                              # 16 * 4096 * 1024 = 2^26 words: one W32, one image more
    several += [{**at_the_limit, 9: 1, 10: 32 * 1024 + 1}, {**at_the_limit, 1: 17}, {1: 1 << 12, 14: 1 << 12, 9: 1, 10: 129}]
    for bad in [{i: v} for i, v in bads] + several:
        args = list(good)
        for i, v in bad.items():
            args[i] = v
        with pytest.raises(hip.PvhipError):
            hip.call(ENTRY, *args)
        assert untouched(), bad
    # the other side of each limit, where no test above stands on it (T = 64, max_per_image = 4096 and hn = 2^24 do; `head`, `protos`
    # and `words` 4 bytes off a 16-byte boundary too): calls with room behind every pointer and a header of zeros
    keep = []
    for what, (n_, e_, plane_, per_) in (('n * max_per_image * W32 = 2^26', (16, 5, (128, 256), MAX_PER_IMAGE)),
                                         ('Hp * Wp = 2^24, hn = wn = 2^24', (1, 5, (4096, 4096), 1)), ('n * a * e = 2^31 - 1', (1, (1 << 31) - 1, (1, 2), 1))):
        args = _entry_args(hip, n_, 1, e_, 1, plane_, per_, keep)
        if what.startswith('Hp'):
            args[11:13] = 1 << 24, 1 << 24
        hip.call('pvhip_memset', ctypes.c_void_p(keep[-1].ptr), 0x7f, keep[-1].nbytes)
        hip.call(ENTRY, *args)
        got = np.asarray(keep[-1])
        assert (got == SENTINEL).all(), what                                                # no row below total = 0: no word
        del keep[:], got
    hip.call('pvhip_pool_release')
    # n = 65535 with a detection each; tail_at = 4, tail_at + tail = e, Hp * Wp = 2, hn = wn = 1, max_per_image = 1, crop 0 and 1
    rng, n = np.random.default_rng(65535), 65535
    x, protos = rng.standard_normal((n, 1, 5)).astype(np.float32), rng.standard_normal((n, 1, 1, 2)).astype(np.float32)
    x[:, 0, :4] = (0, 0, 1, 1)
    for crop in (True, False):
        want = masks_ref.masks(x, 'NAC', 'XYXY', 1, protos, np.arange(n), np.arange(n), (1, 1), crop)
        assert np.array_equal(_device_masks(hip, x, 'NAC', 1, protos, (1,) * n, np.arange(n), (1, 1), crop), want) and want.any()
    # the tail of the boxes entry: -1 and 65
    t, o = hip.DeviceTensor.from_numpy(np.zeros((2, 10, 10), np.float32)), hip.DeviceTensor.empty((4096,), np.int32)
    at = lambda i: off(o, 4 * i)
    tail_good = [hip.ptr(t), 2, 10, 5, 1, 1, 0, 0, 0.25, None, 0, 64, 64, 0, 0, 64, 64, 1, 1, 8, 0, 0.5, 1, 8, at(0), at(1024), at(2048)]
    hip.call('pvhip_dense_boxes_tail_f32', *tail_good)
    hip.synchronize()
    hip.call('pvhip_memset', ctypes.c_void_p(o.ptr), 0x7f, o.nbytes)
    for bad in (-1, 65):
        with pytest.raises(hip.PvhipError):
            hip.call('pvhip_dense_boxes_tail_f32', *(tail_good[:4] + [bad] + tail_good[5:]))
        assert (np.asarray(o) == SENTINEL).all(), bad
    good_call_equals_the_rule()                                                              # the device is still usable
