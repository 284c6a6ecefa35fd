"""A detector's answer made on the device (``infer(..., detections=...)``, pvhip_detections_compact): the records that pass the screen as
one flat table by the rule of tests/detections_ref.py, word for word, two launches behind the pass and a read-back of the header and of
exactly the rows it counts.  The first tests need no GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import detections_ref
import helpers
import test_detected_rois as det_tests
import test_roi_input as roi_tests
from detected_rois_ref import detected_rois
from helpers import GOLDEN, MODELS

ENTRY = 'pvhip_detections_compact'
NAN, INF = np.nan, np.inf
_net, _frames, _rec, END, ZERO = roi_tests._net, roi_tests._frames, det_tests._rec, det_tests.END, det_tests.ZERO
_random_records = det_tests._random_records


def _screen(extent, **opt):
    from pyopenvino_amd import DetectionScreen
    return DetectionScreen(frame_size=extent, **opt)


def _same(got, want, what=''):
    """`got` (a Detections of the product) equals `want` (a Compacted of the rule) word for word."""
    from pyopenvino_amd import Detections
    assert isinstance(got, Detections), (what, type(got))
    total = int(want.counts.sum())
    for a, shape, dtype in ((got.counts, want.counts.shape, np.int32), (got.selected, want.counts.shape, np.int32), (got.rois, (total, 5), np.int32),
                            (got.labels, (total,), np.int32), (got.scores, (total,), np.float32), (got.records, (total,), np.int32)):
        assert isinstance(a, np.ndarray) and a.shape == shape and a.dtype == dtype, (what, a.shape, a.dtype, shape, dtype)
    words = detections_ref.as_words(got)
    assert np.array_equal(words.counts, want.counts), (what, words.counts.tolist(), want.counts.tolist())
    assert np.array_equal(words.selected, want.selected), (what, words.selected.tolist(), want.selected.tolist())
    bad = np.flatnonzero((words.table != want.table).any(axis=1))
    assert not len(bad), '{}: row {}: {} want {}'.format(what, bad[0], words.table[bad[0]].tolist(), want.table[bad[0]].tolist())
    at = 0
    for b in range(len(got.counts)):                           # .of(b) are image b's slices
        rois, labels, scores, records = got.of(b)
        n = int(got.counts[b])
        assert len(rois) == len(labels) == len(scores) == len(records) == n and (rois[:, 0] == b).all()
        assert np.array_equal(records, got.records[at:at + n])
        at += n


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
def test_the_rule_on_hand_written_records():
    """Three images of six records over (100, 200) frames (the table of test_detected_rois, whose corners are binary fractions) and
    single records for the label conversion: detections_ref and the product's own numpy form agree, and the expected words are written
    out."""
    from pyopenvino_amd import detections
    H, W = 100, 200
    image0 = [_rec(0, 1, 0.9, 0.125, 0.25, 0.5, 0.625),       # plain: x 25..100, y 25..62.5 -> 63
              _rec(1, 2, 0.8, -0.5, 0.25, 1.5, 0.75),         # clamped: x 0..200, y 25..75
              _rec(2, 1, NAN, 0.1, 0.1, 0.2, 0.2),            # NaN score
              END, ZERO,                                      # the terminator in mid-image, a zero row behind it ...
              _rec(5, 1, 0.99, 0.1, 0.1, 0.9, 0.9)]           # ... and a live-looking row behind that
    image1 = [END] + [_rec(k, 1, 0.9, 0.1, 0.1, 0.9, 0.9) for k in range(1, 6)]        # a list ending at position 0
    image2 = [_rec(0, 1, 0.7, 1 / 128, 0.5, 0.125, 65 / 128),  # x 1..25, y 50..51
              _rec(1, 3, 0.7, INF, 0.1, 0.2, 0.2),            # an infinite corner
              _rec(2, 3, 0.7, 0.1, 0.1, NAN, 0.2),            # a NaN corner
              _rec(3, 3, 0.6, 1.2, 0.1, 1.5, 0.9),            # empty after clamping
              _rec(4, 7.9, 0.5, 0.25, 0.0, 0.75, 1.0),        # score == min_confidence; label 7.9 -> 7
              _rec(5, -1.0, 0.5, 0.0, 0.0, 1.0, 1.0)]         # label -1.0 -> -1
    rec = np.array(image0 + image1 + image2, np.float32)
    full = [(0, 25, 25, 75, 38, 1), (0, 0, 25, 200, 50, 2), (2, 1, 50, 24, 1, 1), (2, 50, 0, 100, 100, 7), (2, 0, 0, 200, 100, -1)]
    rows = [0, 1, 12, 16, 17]

    def both(records, images, **opt):
        want = detections_ref.compact(records, images, (H, W), **opt)
        got = detections.compact_records(records, images, _screen((H, W), **opt))
        _same(got, want, str(opt))
        return got

    def table(d):
        return [tuple(r) + (l,) for r, l in zip(d.rois.tolist(), d.labels.tolist())]

    d = both(rec, 3)
    assert d.counts.tolist() == [2, 0, 3] and d.selected.tolist() == [2, 0, 3] and table(d) == full and d.records.tolist() == rows
    assert np.array_equal(d.scores.view(np.uint32), rec[rows, 2].view(np.uint32))
    assert both(rec.reshape(1, 1, 18, 7), 3).records.tolist() == rows
    d = both(rec, 3, max_per_image=1)                          # the cap at 1: the first survivor of every image
    assert d.counts.tolist() == [1, 0, 1] and d.selected.tolist() == [2, 0, 3] and d.records.tolist() == [0, 12]
    d = both(rec, 3, max_per_image=2)
    assert d.counts.tolist() == [2, 0, 2] and d.selected.tolist() == [2, 0, 3] and d.records.tolist() == [0, 1, 12, 16]
    for cap in (3, 6, 1000):                                   # at selected and above it (above P: the same as P)
        assert both(rec, 3, max_per_image=cap).records.tolist() == rows
    assert both(rec, 3, labels=[1]).records.tolist() == [0, 12]
    assert both(rec, 3, labels=[2, 7]).records.tolist() == [1]         # 7.9 is not 7
    assert both(rec, 3, labels=[-1, 3]).records.tolist() == [17]       # label 3 has only bad corners and an empty box
    d = both(rec, 3, labels=[])
    assert d.counts.tolist() == [0, 0, 0] and d.rois.shape == (0, 5)
    assert both(rec, 3, min_confidence=0.75).records.tolist() == [0, 1]
    assert both(rec, 3, min_confidence=0.5000001).records.tolist() == [0, 1, 12]
    assert both(rec, 3, min_size=(2, 1)).records.tolist() == [0, 1, 16, 17]
    assert both(rec, 3, min_size=(39, 76), max_per_image=1).records.tolist() == [1, 16]
    one = both(rec, 1)                                         # one image of 18 records ends at its first terminator
    assert one.counts.tolist() == [2] and one.records.tolist() == [0, 1]
    cut = rec.copy()
    cut[1, 0] = NAN                                            # a NaN in column 0 ends a list like the terminator
    assert both(cut, 3).records.tolist() == [0, 12, 16, 17]
    # the label conversion
    for label, want in ((NAN, -1), (INF, -1), (-INF, -1), (3e9, -1), (-3e9, -1), (-1.0, -1), (7.9, 7), (-7.9, -7), (0.0, 0), (-0.0, 0), (90.0, 90),
                        (2147483520.0, 2147483520), (2147483648.0, -1), (-2147483648.0, -2147483648)):
        d = both(np.array([_rec(0, label, 0.9, 0.25, 0.25, 0.5, 0.5)], np.float32), 1)
        assert d.labels.tolist() == [want] and d.rois.tolist() == [[0, 50, 25, 50, 25]], (label, d.labels)
    # a dead batch
    dead = np.array([END, ZERO, _rec(0, 1, 0.99, 0.1, 0.1, 0.9, 0.9)] * 4, np.float32)
    d = both(dead, 4)
    assert d.counts.tolist() == d.selected.tolist() == [0] * 4
    assert d.rois.shape == (0, 5) and d.labels.shape == d.scores.shape == d.records.shape == (0,)
    assert all(len(part) == 0 for part in d.of(3))
    # what compact_records refuses
    for bad, images in ((np.zeros((6, 7), np.float64), 2), (np.zeros((6, 6), np.float32), 2), (np.zeros((2, 1, 6, 7), np.float32), 2),
                        (np.zeros((7, 7), np.float32), 2), (np.zeros((6, 7), np.float32), 0)):
        with pytest.raises(ValueError, match='detections: '):
            detections.compact_records(bad, images, _screen((H, W)))
    with pytest.raises(ValueError, match='frame_size'):
        detections.compact_records(rec, 3, 0.5)                # no network to take the frame size from


@pytest.mark.parametrize('images,per_image', [(1, 1), (1, 65), (7, 100), (130, 2)])
def test_consistent_with_the_cascades_table(images, per_image):
    """Without a cap the table is the one DetectedRois makes of the same records (tests/detected_rois_ref.py), for every n."""
    from pyopenvino_amd import detections
    rng = np.random.default_rng(images * 4099 + per_image)
    extent = (96, 128)
    rec = _random_records(rng, images, per_image)
    for opt in (dict(), dict(labels=[5, 0, 3], min_confidence=0.25), dict(min_size=(20, 33)), dict(min_confidence=-1.0)):
        d = detections.compact_records(rec, images, _screen(extent, **opt))
        _same(d, detections_ref.compact(rec, images, extent, **opt), str(opt))
        total = len(d.records)
        assert total == d.counts.sum() == d.selected.sum()
        for n in sorted({1, max(1, total - 1), max(1, total), total + 1, total + 70}):
            want = detected_rois(rec, n, images, extent, **opt)
            assert want.count == min(total, n) and d.selected.sum() == want.selected
            assert np.array_equal(d.rois[:want.count], want.rois[:want.count]) and np.array_equal(d.records[:want.count], want.records[:want.count])


def test_on_the_recorded_ssd_records_the_rule_is_the_samples_loop():
    from pyopenvino_amd import detections
    out = np.load(os.path.join(GOLDEN, 'ssd_full_e2e.npz'))['out']
    rec = out[0, 0]
    assert out.shape == (1, 1, 100, 7) and (rec[:, 0] >= 0).all() and 0 <= rec[:, 3:].min() and rec[:, 3:].max() <= 1
    assert abs(float(rec[:, 2].min()) - 0.6704) < 1e-4 and abs(float(rec[:, 2].max()) - 0.8179) < 1e-4
    d = detections.compact_records(out, 1, _screen((300, 300), min_confidence=0.5))
    _same(d, detections_ref.compact(out, 1, (300, 300), min_confidence=0.5))
    assert len(d.records) == 100 and d.counts.tolist() == [100]
    for k, (label, conf, xmin, ymin, xmax, ymax) in enumerate(rec[:, 1:]):          # the sample's loop, img_w = img_h = 300
        assert conf > 0.5
        assert (d.rois[k, 1], d.rois[k, 2]) == (int(xmin * 300), int(ymin * 300)), k
        assert d.rois[k, 1] + d.rois[k, 3] >= int(xmax * 300) and d.rois[k, 2] + d.rois[k, 4] >= int(ymax * 300), k
        assert d.labels[k] == int(label) and d.scores[k] == conf
    assert len(detections.compact_records(out, 1, _screen((300, 300), min_confidence=0.775)).records) == 10
    d = detections.compact_records(out, 1, _screen((300, 300), min_confidence=0.9))
    assert len(d.records) == 0 and d.counts.tolist() == [0] and d.rois.shape == (0, 5)


def test_argument_rules():
    """Every refusal is a ValueError that starts with 'detections: ', raised before anything is staged or launched: this test runs where
    there is no device."""
    from pyopenvino_amd import DetectionScreen, detections
    ie, net, name = _net('ssd_mobilenet_v1_coco', 2)
    ex = ie.load_network(net, 'GPU', num_requests=2)
    out_name = net.outputs[0]['name']
    assert tuple(net.outputs[0]['input'][0]['dims']) == (1, 1, 200, 7)
    x = np.zeros((2, 3, 300, 300), np.float32)
    req = ex.requests[0]
    starts = (lambda d: ex.infer({name: x}, detections=d), lambda d: ex.infer({name: x}, False, None, d),
              lambda d: req.start_async({name: x}, detections=d), lambda d: req.start_async({name: x}, None, d),
              lambda d: ex.requests[1].infer({name: x}, detections=d), lambda d: req.infer({name: x}, None, d),
              lambda d: ex.start_async(1, {name: x}, detections=d), lambda d: ex.start_async(0, {name: x}, None, d))

    def refused(match, d, network=ex, starts=starts):
        for start in starts:
            with pytest.raises(ValueError, match=match) as e:
                start(d)
            assert str(e.value).startswith('detections: '), str(e.value)
        for r in network.requests:
            assert not r._in_flight and not r._asks and not r.runner.answers.blocks
            assert not r.runner.host_inputs.slots and r.runner._pending is None

    def each_form(match, **opt):
        refused(match, DetectionScreen(**opt))
        refused(match, {out_name: DetectionScreen(**opt)})

    refused('no Result named', {'nope': 0.5})
    refused('no Result named', {out_name: 0.5, 'DetectionOutput': 0.5})
    for bad in (NAN, INF, -INF, '0.5', True, [0.5], (0.5, 0.5)):
        refused('min_confidence', bad)
        each_form('min_confidence', min_confidence=bad)
    refused('min_confidence', {out_name: None})
    for bad in (list(range(65)), [1.0], 'abc', [[1]], 3, [True], [2 ** 31], np.zeros((2, 2), np.int32)):
        each_form('at most 64 ints', labels=bad)
    for bad in ((0, 1), (1, 0), 1, (1, 1, 1), (1.0, 1), [1, True], 'ab'):
        each_form('min_size', min_size=bad)
    for bad in ((0, 300), (300, 0), (300, (1 << 24) + 1), (300,), 300, (300.0, 300), 'ab'):
        each_form('frame_size', frame_size=bad)
    for bad in (0, -1, 1.5, True, '3', 2 ** 31):
        each_form('max_per_image', max_per_image=bad)
    ex.comm = types.SimpleNamespace(world=2, rank=0)
    try:
        refused('sharded', 0.5)
        refused('sharded', {out_name: DetectionScreen()})
    finally:
        ex.comm = None
    # an FP16 Result (every request has its own copy of the graph)
    ports = [r.runner.ienet.outputs[0]['input'][0] for r in ex.requests]
    for port in ports:
        port['precision'] = 'FP16'
    try:
        refused('FP32 Results only', {out_name: 0.5})
        refused('no FP32 Result of shape', 0.5)
    finally:
        for port in ports:
            port['precision'] = 'FP32'
    # a Result whose records do not divide into the batch
    declared = [port['dims'] for port in ports]
    for port in ports:
        port['dims'] = (1, 1, 201, 7)
    try:
        refused(r'not \(1, 1, R, 7\)', {out_name: 0.5})
        refused('no FP32 Result of shape', DetectionScreen())
    finally:
        for port, dims in zip(ports, declared):
            port['dims'] = dims
    # a classifier's rows of scores are no records
    ie_c, net_c, name_c = _net(batch=2)
    cls = ie_c.load_network(net_c, 'GPU', num_requests=1)
    cls_out = net_c.outputs[0]['name']
    xc = np.zeros((2, 3, 224, 224), np.float32)
    cls_starts = (lambda d: cls.infer({name_c: xc}, detections=d), lambda d: cls.requests[0].start_async({name_c: xc}, detections=d),
                  lambda d: cls.start_async(0, {name_c: xc}, None, d))
    refused(r'not \(1, 1, R, 7\)', {cls_out: 0.5}, cls, cls_starts)
    refused('no FP32 Result of shape', 0.5, cls, cls_starts)
    refused('no FP32 Result of shape', DetectionScreen(), cls, cls_starts)
    # what is accepted, in its one form: equal screens are equal keys
    want = DetectionScreen(0.5, (300, 300), None, (1, 1), 100)
    assert detections.checked(net, None, False) == {} and detections.checked(net, {}, True) == {}
    assert detections.checked(net, 0.5, False) == detections.checked(net, DetectionScreen(), False) == {out_name: want}
    assert detections.checked(net, {out_name: np.float32(0.5)}, False) == {out_name: want}
    got = detections.checked(net, DetectionScreen(1, [480, 640], np.array([3, 1]), [2, 3], 1000), False)[out_name]
    assert got == DetectionScreen(1.0, (480, 640), (3, 1), (2, 3), 100) and hash(got) == hash(DetectionScreen(1.0, (480, 640), (3, 1), (2, 3), 100))
    assert detections.checked(net, DetectionScreen(labels=[], max_per_image=7), False)[out_name] == want._replace(labels=(), max_per_image=7)
    with pytest.raises(AttributeError):
        want.min_confidence = 0.1                              # immutable
    with pytest.raises(ValueError, match='^detections: .*frame_size is needed'):
        detections.resolved(0.5, 100, None)                    # no single 4-D Parameter to take the extent from
    assert detections.records_of({'dims': (1, 1, 200, 7)}, 2) == 100 and detections.records_of({'dims': (1, 1, 200, 7)}, 3) is None
    assert detections.records_of({'dims': (2, 1000)}, 2) is None and detections.records_of({'dims': (1, 2, 200, 7)}, 2) is None


def test_abi_declares_the_entry():
    import pyopenvino_amd
    from pyopenvino_amd import detections, device
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert ENTRY in device.SIGNATURES and len(device.SIGNATURES[ENTRY][1]) == 13 and ENTRY not in device._NOT_STATUS
    m = re.search(r'\bint\s+' + ENTRY + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S)
    assert m and len(m.group(1).split(',')) == 13
    comment = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int\s+' + ENTRY, header, flags=re.S).group(1)
    for phrase in ('Addition to ABI v18 (the version number is unchanged', 'min(selected[b], max_per_image)', '(b, x0, y0, w, h, label, score bits, record)',
                   'counts[images], then selected[images], then total', 'tests/detections_ref.py'):
        assert phrase in comment, phrase                       # the rule is stated there
    assert re.search(r'#define\s+PVHIP_ABI_VERSION\s+19\b', header)
    lib = device.load_library()
    assert hasattr(lib, ENTRY) and lib.pvhip_abi_version() == 19
    assert pyopenvino_amd.Detections is detections.Detections and pyopenvino_amd.DetectionScreen is detections.DetectionScreen
    assert 'Detections' in pyopenvino_amd.__all__ and 'DetectionScreen' in pyopenvino_amd.__all__
    assert pyopenvino_amd.Detections._fields == ('counts', 'selected', 'rois', 'labels', 'scores', 'records')


# ---------------------------------------------------------------------------------------------------------------- GPU
SENTINEL = 0x7f7f7f7f


def _device_compact(hip, rec, images, extent, min_confidence=0.5, labels=None, min_size=(1, 1), max_per_image=None):
    """The entry on `rec`: header and rows prefilled with 0x7f bytes, each with a guard row behind it, as a Compacted; rows >= total
    must be untouched."""
    per_image = rec.reshape(-1, 7).shape[0] // images
    cap = per_image if max_per_image is None else max_per_image
    capacity = images * min(per_image, cap)
    src = hip.DeviceTensor.from_numpy(rec)
    header = hip.DeviceTensor.empty((2 * images + 1 + 8,), np.int32)
    rows = hip.DeviceTensor.empty((capacity + 1, 8), np.int32)
    for t in (header, rows):
        hip.call('pvhip_memset', ctypes.c_void_p(t.ptr), 0x7f, t.nbytes)
    lab = hip.DeviceTensor.from_numpy(np.asarray(list(labels) + [0], np.int32)) if labels is not None else None      # ([]: no label passes)
    hip.call(ENTRY, ctypes.c_void_p(src.ptr), images, per_image, extent[0], extent[1], min_confidence,
             ctypes.c_void_p(lab.ptr) if lab is not None else None, 0 if labels is None else len(labels), min_size[0], min_size[1], cap,
             ctypes.c_void_p(header.ptr), ctypes.c_void_p(rows.ptr))
    header, rows = np.asarray(header), np.asarray(rows).view(np.uint32)
    assert (header[2 * images + 1:] == SENTINEL).all(), 'a word behind the header was written'
    counts, selected, total = header[:images].copy(), header[images:2 * images].copy(), int(header[2 * images])
    assert 0 <= total <= capacity and total == counts.sum(), (total, capacity, counts.sum())
    assert (rows[total:] == SENTINEL).all(), 'a row from total onward was written'
    return detections_ref.Compacted(counts, selected, rows[:total].copy())


def _equal(got, want, what):
    assert np.array_equal(got.counts, want.counts), (what, got.counts.tolist(), want.counts.tolist())
    assert np.array_equal(got.selected, want.selected), (what, got.selected.tolist(), want.selected.tolist())
    assert got.table.shape == want.table.shape, (what, got.table.shape, want.table.shape)
    bad = np.flatnonzero((got.table != want.table).any(axis=1))
    assert not len(bad), '{}: row {}: {} want {}'.format(what, bad[0], got.table[bad[0]].tolist(), want.table[bad[0]].tolist())


# an image around the chunk of 64 records; images not a multiple of the four waves of a workgroup; a base sum over more than 64 and more
# than 1024 images
SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (1, 200), (5, 130), (7, 100), (65, 3), (130, 2), (1030, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize('images,per_image', SHAPES)
def test_kernel_equals_the_rule(hip, images, per_image):
    rng = np.random.default_rng(images * 4099 + per_image)
    extent, P = (96, 128), per_image
    rec = _random_records(rng, images, per_image)
    if (images, per_image) == (1, 1):
        rec[0] = (0, 1, 0.9, 0.1, 0.1, 0.5, 0.5)
    odd = rec.copy()                                           # labels the conversion turns into -1 or truncates, in live rows too
    odd[::5, 1], odd[1::7, 1], odd[2::11, 1], odd[3::13, 1] = NAN, 3e9, -INF, 7.9
    options = [dict(), dict(max_per_image=1), dict(max_per_image=2), dict(max_per_image=P), dict(labels=[1]), dict(labels=[5, 0, 3], min_confidence=0.25),
               dict(labels=list(range(6, 70))), dict(labels=[]), dict(min_size=(20, 33)), dict(min_confidence=-1.0), dict(min_confidence=2.0),
               dict(min_confidence=0.25, max_per_image=2), dict(labels=[5, 0, 3], max_per_image=1, min_confidence=-1.0),
               dict(labels=[2], min_size=(3, 1), max_per_image=2)]
    assert detections_ref.compact(rec, images, extent, min_confidence=-1.0).selected.sum() >= 1
    for opt in options:
        _equal(_device_compact(hip, rec, images, extent, **opt), detections_ref.compact(rec, images, extent, **opt), str(opt))
    _equal(_device_compact(hip, rec.reshape(1, 1, -1, 7), images, (1080, 1920)), detections_ref.compact(rec, images, (1080, 1920)), '1080p')
    for opt in (dict(min_confidence=-1.0), dict(max_per_image=2)):
        _equal(_device_compact(hip, odd, images, extent, **opt), detections_ref.compact(odd, images, extent, **opt), 'odd labels {}'.format(opt))
    long = _random_records(rng, images, per_image, long=per_image > 3)      # (every list three records short of its image, where it has them)
    for opt in (dict(), dict(max_per_image=2), dict(labels=[5, 0, 3], min_confidence=0.25)):
        _equal(_device_compact(hip, long, images, extent, **opt), detections_ref.compact(long, images, extent, **opt), 'long {}'.format(opt))
    dead = _random_records(rng, images, per_image, dead=True)
    for opt in (dict(min_confidence=-1.0), dict(max_per_image=1)):
        got = _device_compact(hip, dead, images, extent, **opt)
        _equal(got, detections_ref.compact(dead, images, extent, **opt), 'every image dead {}'.format(opt))
        assert not got.counts.any() and not got.selected.any() and got.table.shape == (0, 8)


@pytest.mark.gpu
def test_entry_rejects_what_it_cannot_do(hip):
    rng = np.random.default_rng(5)
    rec = _random_records(rng, 4, 2)
    src = hip.DeviceTensor.from_numpy(rec)
    out = hip.DeviceTensor.empty((64 + 16,), np.int32)
    lab = hip.DeviceTensor.from_numpy(np.arange(64, dtype=np.int32))
    p, h, r = ctypes.c_void_p(src.ptr), ctypes.c_void_p(out.ptr + 256), ctypes.c_void_p(out.ptr)
    good = [p, 4, 2, 96, 128, 0.5, None, 0, 1, 1, 2, h, r]
    hip.call(ENTRY, *good)
    hip.call(ENTRY, *(good[:6] + [ctypes.c_void_p(lab.ptr), 64] + good[8:]))
    for k, bad in ((0, None), (11, None), (12, None), (12, ctypes.c_void_p(out.ptr + 4)), (12, ctypes.c_void_p(out.ptr + 8)), (1, 0), (1, -1), (2, 0),
                   (8, 0), (9, 0), (10, 0), (10, -1), (3, 0), (4, 0), (3, (1 << 24) + 1), (4, (1 << 24) + 1), (7, 65), (7, -1), (7, 1),
                   (2, 2 ** 31 // 7), (2, 2 ** 31 // 28 + 1)):
        args = list(good)
        args[k] = bad
        with pytest.raises(hip.PvhipError):
            hip.call(ENTRY, *args)
    with pytest.raises(hip.PvhipError):
        hip.call(ENTRY, *(good[:6] + [ctypes.c_void_p(lab.ptr), 65] + good[8:]))
    hip.synchronize()
    _equal(_device_compact(hip, rec, 4, (96, 128), min_confidence=0.25), detections_ref.compact(rec, 4, (96, 128), min_confidence=0.25),
           'after the refusals')                               # the device is still usable


_detector, _median_live_score = det_tests._detector, det_tests._median_live_score


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.gpu
def test_public_path_on_ssd_mobilenet(hip):
    """SSD-MobileNet at batch 2 on U8 / NHWC frames: detections= is the rule on the same request's own full Result, through the request and
    through the network's infer(); without the keyword the Result comes back whole; then a device-resident input five times with the
    keyword alternating, replayed from the request's one recording from the third call on."""
    from pyopenvino_amd import DetectionScreen, Detections
    rng = np.random.default_rng(91)
    m, hw = 2, (480, 640)
    frames = _frames(rng, 'U8-NHWC', m, hw)
    det, name, out_name = _detector(m)
    req = det.requests[0]
    full = np.array(req.infer({name: frames})[out_name], copy=True)
    assert full.shape == (1, 1, 200, 7) and full.dtype == np.float32
    conf = _median_live_score(full, m)
    want = detections_ref.compact(full, m, (300, 300), min_confidence=conf)
    assert 1 <= want.counts.sum() < 200
    got = req.infer({name: frames}, detections=conf)
    assert set(got) == {out_name} and isinstance(got[out_name], Detections)
    _same(got[out_name], want, 'request')
    _same(det.infer({name: frames}, detections=DetectionScreen(conf))[out_name], want, 'the network\'s own infer()')
    _same(det.infer({name: frames}, False, None, {out_name: conf})[out_name], want, 'positional')
    # labels, a cap that cuts and another frame size
    live = full[0, 0][full[0, 0, :, 0] >= 0]
    values, freq = np.unique(live[:, 1], return_counts=True)
    listed = [int(v) for v in values[np.argsort(-freq)][:3]]
    opt = dict(min_confidence=0.0, labels=listed, max_per_image=3)
    want_cut = detections_ref.compact(full, m, hw, **opt)
    print('labels {}: selected {} counts {}'.format(listed, want_cut.selected.tolist(), want_cut.counts.tolist()))
    assert want_cut.counts.sum() >= 1 and (want_cut.selected > want_cut.counts).any()
    _same(req.infer({name: frames}, detections=DetectionScreen(frame_size=hw, **opt))[out_name], want_cut, 'labels, cap, frame size')
    whole = req.infer({name: frames})[out_name]                # and whole again without the keyword
    assert isinstance(whole, np.ndarray) and np.array_equal(_bits(whole), _bits(full))
    # the same device-resident tensor five times
    x = rng.uniform(0, 255, (m, 3, 300, 300)).astype(np.float32)
    xd = hip.DeviceTensor.from_numpy(x)
    screen = DetectionScreen(conf)
    kinds = [screen, None, {out_name: 0.3}, screen, None]
    results = []
    for call, kind in enumerate(kinds):
        req.start_async({name: xd}, detections=kind)
        assert (req._replayed is not None) == (call >= 2), 'call {}'.format(call)
        results.append(req.wait()[out_name])
    assert det._auto_graph['captured'] and det._graph is not None           # one recording served every kind
    full_x = np.array(results[1], copy=True)
    assert isinstance(results[4], np.ndarray) and np.array_equal(_bits(results[4]), _bits(full_x))
    _same(results[0], detections_ref.compact(full_x, m, (300, 300), min_confidence=conf), 'call 0')
    _same(results[2], detections_ref.compact(full_x, m, (300, 300), min_confidence=0.3), 'call 2')
    _same(results[3], detections_ref.as_words(results[0]), 'call 3 vs call 0')
    # the request's own blocks, one per (name, screen)
    keys = sorted(det.answers.blocks, key=repr)
    assert len(keys) == 3 and {k[0] for k in keys} == {out_name}
    assert all(len(k) == 2 and type(k[1]) is DetectionScreen for k in keys)         # no key of another kind
    assert {(k[1].min_confidence, k[1].max_per_image, k[1].frame_size) for k in keys} == {(conf, 100, (300, 300)), (0.3, 100, (300, 300)), (0.0, 3, hw)}
    det.release_device_state()
    assert not det.answers.blocks


@pytest.mark.gpu
def test_cascade_makes_the_same_table(hip):
    """A detector's pass started with detections= leaves its full Result on the device: a GoogLeNet request fed DetectedRois(frames, the
    detector's request) makes a table equal to the first rows of the Detections of the same screen over the same frame size."""
    from pyopenvino_amd import DetectedRois, DetectionScreen, synth
    blob = synth.synth_weights(os.path.join(MODELS, 'googlenet-v1.xml'), 11)
    rng = np.random.default_rng(77)
    m, n, hw = 2, 8, (480, 640)
    frames = _frames(rng, 'U8-NHWC', m, hw)
    det, det_name, det_out = _detector(m)
    ex, name, out_name = det_tests._classifier('U8-NHWC', n, blob)
    full = np.array(det.requests[0].infer({det_name: frames})[det_out], copy=True)
    conf = _median_live_score(full, m)
    d = det.requests[0].infer({det_name: frames}, detections=DetectionScreen(conf, frame_size=hw))[det_out]
    _same(d, detections_ref.compact(full, m, hw, min_confidence=conf), 'detector')
    ex.requests[0].infer({name: DetectedRois(frames, det.requests[0], min_confidence=conf)})
    table = ex.requests[0].detected_rois(name)
    assert table.selected == d.selected.sum() and 1 <= table.count == min(n, len(d.records))
    assert np.array_equal(table.rois[:table.count], d.rois[:table.count]) and np.array_equal(table.records[:table.count], d.records[:table.count])
    # and in flight: the table is made of the Result of a pass that was started with the keyword and not waited for
    det.requests[0].start_async({det_name: frames}, detections=conf)
    ex.requests[0].start_async({name: DetectedRois(frames, det.requests[0], min_confidence=conf)})
    ex.requests[0].wait()
    _same(det.requests[0].wait()[det_out], detections_ref.compact(full, m, (300, 300), min_confidence=conf), 'in flight')
    det_tests._same(ex.requests[0].detected_rois(name), table, 'in flight')


def _decided(scores, conf):
    """The gaps between `conf` and the recorded scores on either side of it, and twice the deviation the project's bound
    (helpers.assert_close: |d| <= 1e-4 |want| + 1e-4 rms(want)) allows a score there."""
    s = scores.astype(np.float64)
    above, below = s[s >= conf].min(), s[s < conf].max()
    rms = float(np.sqrt(np.mean(s ** 2)))
    return above - conf, conf - below, 2 * helpers.REL_TOL * (above + rms), 2 * helpers.REL_TOL * (below + rms)


@pytest.mark.gpu
def test_against_the_reference(hip):
    """Batch 1 on the golden file's weights and image: 0.7886 stands between the recorded scores 0.79158 and 0.78561 by more than the
    project's bound can move either, so the answer is decided: three records, the reference's labels, its scores within the bound, its
    rectangles within a pixel."""
    from pyopenvino_amd import synth
    z = np.load(os.path.join(GOLDEN, 'ssd_full_e2e.npz'))
    golden, conf = z['out'], 0.7886
    up, down, slack_up, slack_down = _decided(golden[0, 0, :, 2], conf)
    print('gaps {:.3e} {:.3e}; twice the bound {:.3e} {:.3e}'.format(up, down, slack_up, slack_down))
    assert abs(up - (0.79158 - conf)) < 1e-5 and abs(down - (conf - 0.78561)) < 1e-5 and up > slack_up and down > slack_down
    blob = synth.synth_weights(os.path.join(MODELS, 'ssd_mobilenet_v1_coco.xml'), int(z['weight_seed']))
    ie, net, name = _net('ssd_mobilenet_v1_coco', 1, blob)
    ex = ie.load_network(net, 'GPU', num_requests=1)
    out_name = net.outputs[0]['name']
    x = synth.uniform_pixels(int(z['image_seed']), (1, 3, 300, 300))
    d = ex.requests[0].infer({name: x}, detections=conf)[out_name]
    assert d.counts.tolist() == [3] and d.selected.tolist() == [3] and d.records.tolist() == [0, 1, 2] and d.labels.tolist() == [6, 88, 88]
    assert (d.rois[:, 0] == 0).all()
    scores = golden[0, 0, :, 2].copy()                        # the three scores where they stand among the recorded ones: assert_close's rms is theirs
    scores[:3] = d.scores
    helpers.assert_close(scores, golden[0, 0, :, 2], helpers.REL_TOL, 'scores vs the reference')
    helpers.assert_close(d.scores, golden[0, 0, :3, 2], helpers.REL_TOL, 'scores vs the reference\'s three')
    want = detections_ref.compact(golden, 1, (300, 300), min_confidence=conf)
    assert want.counts.tolist() == [3]
    edges = d.rois[:, 1:].astype(np.int64)
    ref = want.table[:, 1:5].view(np.int32).astype(np.int64)
    for e in (edges, ref):
        e[:, 2:] += e[:, :2]                                   # (x0, y0, x1, y1)
    print('edges {} reference {}'.format(edges.tolist(), ref.tolist()))
    assert np.abs(edges - ref).max() <= 1


@pytest.mark.gpu
def test_two_requests_in_flight(hip):
    """Two requests at batch 2 on different frames, one with the keyword and one without, both started, then both waited for; then the
    other way round.  Each equals its own one-at-a-time answer."""
    rng = np.random.default_rng(92)
    m, hw = 2, (240, 320)
    det, name, out_name = _detector(m, requests=2)
    frames = [_frames(rng, 'U8-NHWC', m, hw) for _ in range(2)]
    fulls = [np.array(det.requests[r].infer({name: frames[r]})[out_name], copy=True) for r in range(2)]
    assert not np.array_equal(fulls[0], fulls[1])
    confs = [_median_live_score(f, m) for f in fulls]
    alone = [det.requests[r].infer({name: frames[r]}, detections=confs[r])[out_name] for r in range(2)]
    for r in range(2):
        _same(alone[r], detections_ref.compact(fulls[r], m, (300, 300), min_confidence=confs[r]), 'request {} alone'.format(r))
    for step, asked in enumerate(((True, False), (False, True), (True, True))):
        for r in range(2):
            det.start_async(r, {name: frames[r]}, detections=confs[r] if asked[r] else None)
        for r in (1, 0) if step % 2 else (0, 1):
            res = det.wait(r)[out_name]
            if asked[r]:
                _same(res, detections_ref.as_words(alone[r]), 'step {} request {}'.format(step, r))
            else:
                assert isinstance(res, np.ndarray) and np.array_equal(_bits(res), _bits(fulls[r])), 'step {} request {}'.format(step, r)
