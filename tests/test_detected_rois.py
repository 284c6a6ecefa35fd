"""A cascade's regions of interest made on the device (pyopenvino_amd.DetectedRois): DetectionOutput records become the (n, 5) table of
the ROI preprocessing launches by pvhip_detections_to_rois, integer for integer tests/detected_rois_ref.py, and a classifier request
reads a detector request's device-resident Result with no host wait.  The first tests need no GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import detected_rois_ref
import helpers
import test_roi_input as roi_tests
from detected_rois_ref import detected_rois, padded
from helpers import MODELS, assert_bit_exact

ENTRY = 'pvhip_detections_to_rois'
NAN, INF = np.nan, np.inf
_net, _declare, _frames = roi_tests._net, roi_tests._declare, roi_tests._frames


def _rec(rank, label, score, xmin, ymin, xmax, ymax):
    return [rank, label, score, xmin, ymin, xmax, ymax]


END, ZERO = _rec(-1, 0, 0, 0, 0, 0, 0), _rec(0, 0, 0, 0, 0, 0, 0)


def _same(got, want, what=''):
    assert got.count == want.count and got.selected == want.selected, (what, got.count, got.selected, want.count, want.selected)
    assert got.rois.dtype == np.int32 and got.records.dtype == np.int32
    assert np.array_equal(got.rois, want.rois), (what, got.rois.tolist(), want.rois.tolist())
    assert np.array_equal(got.records, want.records), (what, got.records.tolist(), want.records.tolist())


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
def test_the_rule_on_a_hand_written_table():
    """Three images of six records over (100, 200) frames; every expected table written out.  The corners are binary fractions, so
    the float32 products are exact and the expected integers can be read off."""
    from pyopenvino_amd import DetectedRois                   # noqa: F401 -- the rule specifies this input
    H, W = 100, 200
    image0 = [_rec(0, 1, 0.9, 0.125, 0.25, 0.5, 0.625),       # plain: x 25..100, y 25..62.5 -> 63
              _rec(1, 2, 0.8, -0.5, 0.25, 1.5, 0.75),         # xmin < 0 and xmax > 1 are clamped: x 0..200, y 25..75
              _rec(2, 1, NAN, 0.1, 0.1, 0.2, 0.2),            # NaN score
              END,                                            # the terminator in mid-image ...
              ZERO,                                           # ... then zero rows, which are ignored
              _rec(5, 1, 0.99, 0.1, 0.1, 0.9, 0.9)]           # (and whatever else lies behind it)
    image1 = [END] + [_rec(k, 1, 0.9, 0.1, 0.1, 0.9, 0.9) for k in range(1, 6)]        # an image whose first record is the terminator
    image2 = [_rec(0, 1, 0.7, 1 / 128, 0.5, 0.125, 65 / 128),  # x 1.5625..25 -> 1..25 (xmax W integral); y 50..50.78 -> 50..51: one row
              _rec(1, 3, 0.7, INF, 0.1, 0.2, 0.2),            # +inf corner
              _rec(2, 3, 0.7, 0.1, -INF, 0.2, 0.2),           # -inf corner
              _rec(3, 3, 0.7, 0.1, 0.1, NAN, 0.2),            # NaN corner
              _rec(4, 3, 0.6, 1.2, 0.1, 1.5, 0.9),            # empty after clamping: x 200..200
              _rec(5, 2, 0.5, 0.25, 0.0, 0.75, 1.0)]          # xmin W = 50 exactly; score == min_confidence
    rec = np.array(image0 + image1 + image2, np.float32)
    full = [(0, 25, 25, 75, 38), (0, 0, 25, 200, 50), (2, 1, 50, 24, 1), (2, 50, 0, 100, 100)]
    rows = [0, 1, 12, 17]
    none = (-1, 0, 0, 0, 0)

    def want(keep, n):
        table = [full[k] for k in keep][:n]
        recs = [rows[k] for k in keep][:n]
        return (min(len(keep), n), len(keep), table + [none] * (n - len(table)), recs + [-1] * (n - len(recs)))

    def got(n, **opt):
        d = detected_rois(rec, n, 3, (H, W), **opt)
        assert d.rois.dtype == np.int32 and d.records.dtype == np.int32 and d.rois.shape == (n, 5) and d.records.shape == (n,)
        return (d.count, d.selected, [tuple(r) for r in d.rois.tolist()], d.records.tolist())

    assert got(6) == want([0, 1, 2, 3], 6)
    assert got(6, min_confidence=0.5) == (4, 4, full + [none, none], rows + [-1, -1])
    assert got(4) == want([0, 1, 2, 3], 4)                    # n at selected
    assert got(3) == (3, 4, full[:3], rows[:3])               # selected > n: reported, n rows kept
    assert got(1) == (1, 4, full[:1], rows[:1])
    assert got(5, labels=[1]) == want([0, 2], 5)              # the label filter
    assert got(5, labels=[2, 7]) == want([1, 3], 5)
    assert got(5, labels=[3]) == (0, 0, [none] * 5, [-1] * 5)  # label 3 has only bad corners and an empty box
    assert got(5, labels=[]) == (0, 0, [none] * 5, [-1] * 5)
    assert got(5, min_confidence=0.75) == want([0, 1], 5)
    assert got(5, min_confidence=0.95) == (0, 0, [none] * 5, [-1] * 5)                  # selected = 0
    assert got(5, min_size=(2, 1)) == want([0, 1, 3], 5)      # min_size = (h, w): the one-row box goes
    assert got(5, min_size=(1, 25)) == want([0, 1, 3], 5)
    assert got(5, min_size=(39, 76)) == want([1, 3], 5)
    assert got(5, min_size=(38, 75)) == want([0, 1, 3], 5)
    # the same records as (1, 1, R, 7); one image of 18 records ends at its first terminator
    assert _same(detected_rois(rec.reshape(1, 1, 18, 7), 6, 3, (H, W)), detected_rois(rec, 6, 3, (H, W))) is None
    one = detected_rois(rec, 6, 1, (H, W))
    assert (one.count, one.selected, one.records.tolist()) == (2, 2, [0, 1, -1, -1, -1, -1])
    # a NaN in column 0 ends a list like the terminator
    cut = rec.copy()
    cut[1, 0] = NAN
    assert detected_rois(cut, 6, 3, (H, W)).records.tolist() == [0, 12, 17, -1, -1, -1]


def test_the_recorded_ssd_records_make_a_table_the_format_accepts():
    from pyopenvino_amd import DetectedRois                   # noqa: F401
    out = np.load(os.path.join(helpers.REPO, 'tests', 'golden', 'ssd_full_e2e.npz'))['out']
    assert out.shape == (1, 1, 100, 7) and (out[0, 0, :, 0] >= 0).all()
    n, extent = 16, (1080, 1920)
    ie, net, name = _net(batch=n)
    _declare(net, name, 'NV12')
    fmt = net.input_info[name].frozen()
    d = detected_rois(out, n, 1, extent, min_confidence=0.775)
    assert 1 <= d.count < 100 and d.count == d.selected == int((out[0, 0, :, 2] >= np.float32(0.775)).sum())
    table, largest = fmt.checked_rois(padded(d.rois), extent, 1)          # the project's own validator, after padding rows >= count
    assert np.array_equal(table[:d.count], d.rois[:d.count]) and (d.rois[d.count:] == (-1, 0, 0, 0, 0)).all()
    assert largest[0] <= 1080 and largest[1] <= 1920
    full = detected_rois(out, d.count, 1, extent, min_confidence=0.775)
    _, net_full, _ = _net(batch=d.count)
    _declare(net_full, name, 'NV12')
    assert np.array_equal(net_full.input_info[name].frozen().checked_rois(full.rois, extent, 1)[0], full.rois)      # a full table passes unchanged
    assert (out[0, 0, d.records[:d.count], 2] >= 0.775).all() and (d.records[d.count:] == -1).all()
    assert (np.diff(d.records[:d.count]) > 0).all()


def test_argument_rules():
    """Everything is refused before anything is allocated (no device here), in the style of input_format.py."""
    from pyopenvino_amd import DetectedRois
    n, hw = 4, (48, 64)
    ie, net, name = _net(batch=n)
    _declare(net, name, 'U8-NHWC')
    ex = ie.load_network(net, 'GPU', num_requests=2)
    req = ex.requests[0]
    frames = np.zeros((2, 48, 64, 3), np.uint8)
    good = np.zeros((6, 7), np.float32)

    def refused(error, match, frames=frames, detections=good, **opt):
        for start in (ex.infer, req.start_async, ex.requests[1].infer):
            with pytest.raises(error, match=match) as e:
                start({name: DetectedRois(frames, detections, **opt)})
            assert str(e.value).startswith('input {}: '.format(name)), str(e.value)

    refused(ValueError, '3 images need 3 frames, got 2', images=3)                     # m != images
    refused(ValueError, 'images need', frames=np.zeros((3, 48, 64, 3), np.uint8), images=2)
    refused(ValueError, 'do not divide', detections=np.zeros((7, 7), np.float32))       # R % images != 0
    refused(ValueError, 'do not divide', detections=np.zeros((1, 1, 5, 7), np.float32))
    for bad in (np.zeros((6, 7), np.float64), np.zeros((6, 7), np.float16), np.zeros((6, 7), np.int32), np.zeros((6, 6), np.float32),
                np.zeros((2, 1, 6, 7), np.float32), np.zeros((1, 6, 7), np.float32), np.zeros(7, np.float32), np.zeros((0, 7), np.float32),
                [[0.0] * 7] * 6):                             # (a list of Python floats is float64)
        refused(ValueError, r'float32 records of shape \(1, 1, R, 7\) or \(R, 7\)', detections=bad)
    refused(ValueError, 'at most 64 ints', labels=list(range(65)))
    for bad in ([-1], [1.0], 'abc', [[1]], 3):
        refused(ValueError, 'at most 64 ints', labels=bad)
    for bad in (0, True, -2, 1.0, 'x'):
        refused(ValueError, 'images is a count', images=bad)
    for bad in (NAN, '0.5', None, True):
        refused(ValueError, 'min_confidence', min_confidence=bad)
    for bad in ((0, 1), (1, 0), 1, (1, 1, 1), (1.0, 1), None):
        refused(ValueError, 'min_size', min_size=bad)
    refused(ValueError, 'frames of a RoiInput have shape', frames=np.zeros((2, 48, 64, 4), np.uint8))
    # a request that never ran; a request whose Result is no DetectionOutput; an unknown output
    other = ie.load_network(_net(batch=2)[1], 'GPU', num_requests=1).requests[0]
    refused(ValueError, 'no DetectionOutput', detections=other)
    refused(ValueError, 'no Result named', detections=other, output='nope')
    ie_d, net_d, _ = _net('ssd_mobilenet_v1_coco', 2)
    detector = ie_d.load_network(net_d).requests[0]
    refused(RuntimeError, 'never ran', detections=detector)
    refused(RuntimeError, 'never ran', detections=detector, output=net_d.outputs[0]['name'])
    # a sharded network
    ex.comm = types.SimpleNamespace(world=2, rank=0)
    try:
        refused(NotImplementedError, 'sharded')
    finally:
        ex.comm = None
    assert not ex.host_inputs.slots and not ex.requests[1].runner.host_inputs.slots                         # nothing was allocated
    with pytest.raises(KeyError):
        ex.infer({'no such input': DetectedRois(frames, good)})
    # resize not declared
    ie, net, name = _net(batch=n)
    _declare(net, name, 'U8-NHWC', resize=False)
    ex = ie.load_network(net)
    with pytest.raises(ValueError, match='resize_algorithm') as e:
        ex.infer({name: DetectedRois(np.zeros((2, 224, 224, 3), np.uint8), good)})
    assert str(e.value).startswith('input {}: '.format(name)) and not ex.host_inputs.slots
    with pytest.raises(RuntimeError, match='DetectedRois'):
        ex.requests[0].detected_rois(name)
    with pytest.raises(KeyError):
        ex.requests[0].detected_rois('no such input')


def test_abi_declares_the_entry():
    import pyopenvino_amd
    from pyopenvino_amd import device, input_format
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert ENTRY in device.SIGNATURES and len(device.SIGNATURES[ENTRY][1]) == 14 and ENTRY not in device._NOT_STATUS
    m = re.search(r'\b' + ENTRY + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S)
    assert m and len(m.group(1).split(',')) == 14
    assert re.search(r'#define\s+PVHIP_ABI_VERSION\s+19\b', header)
    lib = device.load_library()
    assert hasattr(lib, ENTRY) and lib.pvhip_abi_version() == 19
    assert pyopenvino_amd.DetectedRois is input_format.DetectedRois and 'DetectedRois' in pyopenvino_amd.__all__


# ---------------------------------------------------------------------------------------------------------------- GPU
def _random_records(rng, images, per_image, dead=False, long=False):
    """Seeded records with every special case of the rule injected: list ends anywhere (also at position 0, also a NaN in column 0),
    zero rows behind them, NaN scores, infinite and NaN corners, corners outside [0, 1], empty boxes, corners on pixel edges."""
    R = images * per_image
    rec = np.zeros((R, 7), np.float32)
    rec[:, 0] = np.tile(np.arange(per_image), images)
    rec[:, 1] = rng.integers(0, 6, R)
    rec[:, 2] = rng.uniform(0, 1, R)
    lo = rng.uniform(-0.2, 0.9, (R, 2))
    rec[:, 3:5] = lo
    rec[:, 5:7] = lo + rng.uniform(-0.05, 0.6, (R, 2))
    k = rng.integers(0, 16, R)
    rec[k == 0, 2] = NAN
    rec[k == 1, 3 + rng.integers(0, 4)] = INF
    rec[k == 2, 3 + rng.integers(0, 4)] = -INF
    rec[k == 3, 3 + rng.integers(0, 4)] = NAN
    on_edge = k == 4                                           # corners on pixel edges of a (H, W) = (96, 128) frame
    rec[on_edge, 3], rec[on_edge, 5] = rng.integers(0, 64, on_edge.sum()) / 128, rng.integers(64, 129, on_edge.sum()) / 128
    rec[k == 5, 5] = rec[k == 5, 3]                            # no width
    rec[k == 6, 2] = 0.5                                       # score == min_confidence
    for b in range(images):
        end = int(rng.integers(0, per_image + 1 + per_image // 3))                       # (past the image: no terminator, a full list)
        if rng.integers(0, 5) == 0:
            end = 0
        if images == 1:                                        # one long list: full, or ended one short of the chunk of 1024
            end = per_image - 1 if per_image == 1024 else per_image
        if long:                                               # every list ends three records short of its image
            end = per_image - 3
        if dead:
            end = 0
        if end < per_image:
            rec[b * per_image + end:(b + 1) * per_image] = 0
            rec[b * per_image + end, 0] = NAN if rng.integers(0, 4) == 0 else -1
            if end + 2 < per_image:                            # something live-looking behind the terminator
                rec[b * per_image + end + 2] = (0, 1, 0.99, 0.1, 0.1, 0.9, 0.9)
    return rec


def _device_table(hip, rec, n, images, extent, min_confidence=0.5, labels=None, min_size=(1, 1)):
    """The entry on `rec`: the table, record_of and counts tensors prefilled with 0x7f bytes, each with a guard row behind it."""
    per_image = rec.reshape(-1, 7).shape[0] // images
    src = hip.DeviceTensor.from_numpy(rec)
    outs = [hip.DeviceTensor.empty((rows + 1, cols), np.int32) for rows, cols in ((n, 5), (n, 1), (2, 1))]
    for t in outs:
        hip.call('pvhip_memset', ctypes.c_void_p(t.ptr), 0x7f, t.nbytes)
    lab = hip.DeviceTensor.from_numpy(np.asarray(list(labels) + [0], np.int32)) if labels is not None else None      # ([]: no label passes)
    hip.call(ENTRY, *(ctypes.c_void_p(t.ptr) for t in [src] + outs), n, images, per_image, extent[0], extent[1], min_confidence,
             ctypes.c_void_p(lab.ptr) if lab is not None else None, 0 if labels is None else len(labels), min_size[0], min_size[1])
    rois, record_of, counts = (np.asarray(t) for t in outs)
    assert (rois[n] == 0x7f7f7f7f).all() and record_of[n, 0] == 0x7f7f7f7f and counts[2, 0] == 0x7f7f7f7f     # nothing past the ends
    return detected_rois_ref.Detected(int(counts[0, 0]), int(counts[1, 0]), rois[:n].copy(), record_of[:n, 0].copy())


@pytest.mark.gpu
@pytest.mark.parametrize('images,per_image', [(1, 1), (1, 1023), (1, 1024), (1, 1025), (7, 100), (256, 3), (4100, 2)])
def test_kernel_equals_the_rule(hip, images, per_image):
    """R = 1; one image around the chunk of 1024 records; 7 x 100; 256 x 3 and 4100 x 2 (many list ends; more images than one block of
    list ends holds); every image dead; n below, at and above `selected`; with and without labels and a minimum size."""
    rng = np.random.default_rng(images * 4099 + per_image)
    extent = (96, 128)
    rec = _random_records(rng, images, per_image)
    if (images, per_image) == (1, 1):
        rec[0] = (0, 1, 0.9, 0.1, 0.1, 0.5, 0.5)
    selected = detected_rois(rec, 1, images, extent).selected
    assert selected >= 1 and (images * per_image < 100 or selected >= 10)
    for n in sorted({1, max(1, selected - 1), selected, selected + 1, selected + 70}):
        _same(_device_table(hip, rec, n, images, extent), detected_rois(rec, n, images, extent), 'n = {}'.format(n))
    for opt in (dict(labels=[1]), dict(labels=[5, 0, 3], min_confidence=0.25), dict(min_size=(20, 33)), dict(labels=list(range(6, 70))), dict(labels=[]),
                dict(min_confidence=-1.0), dict(min_confidence=2.0), dict(labels=[2], min_size=(3, 1), min_confidence=0.5)):
        n = 1 if images * per_image == 1 else 40
        _same(_device_table(hip, rec, n, images, extent, **opt), detected_rois(rec, n, images, extent, **opt), str(opt))
    _same(_device_table(hip, rec.reshape(1, 1, -1, 7), 9, images, (1080, 1920)), detected_rois(rec, 9, images, (1080, 1920)), '1080p')
    dead = _random_records(rng, images, per_image, dead=True)
    got = _device_table(hip, dead, 5, images, extent)
    _same(got, detected_rois(dead, 5, images, extent), 'every image dead')
    assert got.count == got.selected == 0 and (got.rois == (-1, 0, 0, 0, 0)).all() and (got.records == -1).all()


@pytest.mark.gpu
def test_entry_rejects_what_it_cannot_do(hip):
    t = hip.DeviceTensor.empty((64,), np.int32)
    p = ctypes.c_void_p(t.ptr)
    good = [p, p, p, p, 4, 1, 2, 96, 128, 0.5, None, 0, 1, 1]
    hip.call(ENTRY, *good)
    for k, bad in ((0, None), (1, None), (2, None), (3, None), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (7, (1 << 24) + 1), (11, 65), (11, -1),
                   (12, 0), (13, 0), (6, 2 ** 31 // 7)):
        args = list(good)
        args[k] = bad
        with pytest.raises(hip.PvhipError):
            hip.call(ENTRY, *args)
    hip.synchronize()


def _classifier(kind, n, blob, requests=1):
    ie, net, name = _net('googlenet-v1', n, blob)
    _declare(net, name, kind, mean=roi_tests._mean())
    return ie.load_network(net, 'GPU', num_requests=requests), name, net.outputs[0]['name']


def _host_route(ex, name, out_name, frames, rec, images, extent, **opt):
    """What the cascade did before: the numpy rule on the read-back records, then a RoiInput (rows >= count padded with a valid
    rectangle): (the rule's record, the Results)."""
    from pyopenvino_amd import RoiInput
    want = detected_rois(rec, ex.host_inputs.formats[name].dims[0], images, extent, **opt)
    return want, np.array(ex.infer({name: RoiInput(frames, padded(want.rois))})[out_name], copy=True)


@pytest.mark.gpu
@pytest.mark.parametrize('kind,hw', [('NV12', (480, 640)), ('NV12', (1080, 1920)), ('U8-NHWC', (480, 640)), ('U8-NHWC', (1080, 1920))])
def test_public_path_with_a_host_array_of_records(hip, kind, hw):
    """GoogLeNet at batch 8 fed DetectedRois(frames, array): rows < count are bit for bit those of RoiInput(frames, the rule's table),
    detected_rois() is the rule, and the rows behind are quiet NaN in the input tensor."""
    from pyopenvino_amd import DetectedRois, synth
    blob = synth.synth_weights(os.path.join(MODELS, 'googlenet-v1.xml'), 11)
    rng = np.random.default_rng(hw[0] + len(kind))
    n, m = 8, 2
    frames = _frames(rng, kind, m, hw)
    rec = _random_records(rng, m, 40, long=True)
    ex_ref, name, out_name = _classifier(kind, n, blob)
    ex, _, _ = _classifier(kind, n, blob)
    req = ex.requests[0]
    seen = set()
    for opt in (dict(min_confidence=0.93), dict(labels=[1, 4], min_size=(9, 9)), dict(min_confidence=0.3)):
        want, want_out = _host_route(ex_ref, name, out_name, frames, rec, m, hw, **opt)
        assert 1 <= want.count
        seen.add((want.count < n, want.selected > n))
        for feed in (rec, rec.reshape(1, 1, -1, 7)):
            got_out = req.infer({name: DetectedRois(frames, feed, **opt)})[out_name]
            got = req.detected_rois(name)
            _same(got, want, str(opt))
            assert (got.rois[got.count:] == (-1, 0, 0, 0, 0)).all()
            assert_bit_exact(got_out[:got.count], want_out[:got.count], '{} {} rows < count'.format(kind, opt))
            fixed = roi_tests._fixed(ex, name)
            assert_bit_exact(fixed[:got.count], roi_tests._fixed(ex_ref, name)[:got.count], 'input rows < count')
            assert np.isnan(fixed[got.count:]).all() and np.isfinite(fixed[:got.count]).all()
    assert (True, False) in seen and (False, True) in seen    # fewer survivors than batch rows, and more
    # the records as a DeviceTensor, the frames in the request's own buffer, and the synchronous infer() of the network
    opt = dict(min_confidence=0.93)
    want, want_out = _host_route(ex_ref, name, out_name, frames, rec, m, hw, **opt)
    buf = req.input_buffer(name, hw, frames=m)
    buf[...] = frames
    got_out = ex.infer({name: DetectedRois(buf, hip.DeviceTensor.from_numpy(rec), images=m, **opt)})[out_name]
    _same(req.detected_rois(name), want, 'DeviceTensor')
    assert_bit_exact(got_out[:want.count], want_out[:want.count], 'DeviceTensor records')
    # an input fed anything else afterwards has no table to read
    from pyopenvino_amd import RoiInput
    req.infer({name: RoiInput(frames, padded(want.rois))})
    with pytest.raises(RuntimeError, match='DetectedRois'):
        req.detected_rois(name)


def _detector(batch, requests=1):
    from pyopenvino_amd import synth
    blob = synth.synth_weights(os.path.join(MODELS, 'ssd_mobilenet_v1_coco.xml'), 1234)
    ie, net, name = _net('ssd_mobilenet_v1_coco', batch, blob)
    _declare(net, name, 'U8-NHWC', reverse=True)
    return ie.load_network(net, 'GPU', num_requests=requests), name, net.outputs[0]['name']


def _median_live_score(rec, images):
    rec = rec.reshape(-1, 7)
    image0 = rec[:rec.shape[0] // images]
    dead = np.flatnonzero(~(image0[:, 0] >= 0))
    live = image0[:dead[0] if len(dead) else len(image0)]
    assert len(live) >= 1
    return float(np.median(live[:, 2]))


@pytest.mark.gpu
def test_cascade_reads_the_detector_in_flight(hip):
    """SSD-MobileNet at batch 2, started and not waited for; GoogLeNet at batch 8 started on DetectedRois(frames, the detector's request);
    then both are waited for.  The yardstick is the host route on the same frames."""
    from pyopenvino_amd import DetectedRois, synth
    blob = synth.synth_weights(os.path.join(MODELS, 'googlenet-v1.xml'), 11)
    rng = np.random.default_rng(77)
    m, n, hw = 2, 8, (480, 640)
    frames = _frames(rng, 'U8-NHWC', m, hw)
    det, det_name, det_out = _detector(m)
    ex_ref, name, out_name = _classifier('U8-NHWC', n, blob)
    ex, _, _ = _classifier('U8-NHWC', n, blob)
    rec = np.array(det.requests[0].infer({det_name: frames})[det_out], copy=True)
    assert rec.shape[:2] == (1, 1) and rec.shape[3] == 7 and rec.shape[2] % m == 0
    conf = _median_live_score(rec, m)
    want, want_out = _host_route(ex_ref, name, out_name, frames, rec, m, hw, min_confidence=conf)
    assert want.count >= 1
    # waited for: its host Results, like an array
    req = ex.requests[0]
    got_out = req.infer({name: DetectedRois(frames, det.requests[0], min_confidence=conf)})[out_name]
    _same(req.detected_rois(name), want, 'a detector that has been waited for')
    assert_bit_exact(got_out[:want.count], want_out[:want.count], 'a detector that has been waited for')
    # in flight: no host wait between the two
    for order in ('classifier first', 'detector first'):
        det.requests[0].start_async({det_name: frames})
        req.start_async({name: DetectedRois(frames, det.requests[0], output=det_out, min_confidence=conf)})
        if order == 'classifier first':
            got_out, rec_again = req.wait()[out_name], det.requests[0].wait()[det_out]
        else:
            rec_again, got_out = det.requests[0].wait()[det_out], req.wait()[out_name]
        assert_bit_exact(rec_again, rec, 'the detector again')
        _same(req.detected_rois(name), want, order)
        assert_bit_exact(got_out[:want.count], want_out[:want.count], order)


@pytest.mark.gpu
def test_six_steps_detector_restarted_at_once(hip):
    """New frames every step; the detector is started on the next frames the moment the classifier's start_async has returned (its
    wait() is host-side bookkeeping only: the classifier is not waited for), two classifier requests alternate, and the passes are
    replayed from their recordings once made.  Every step equals its host route bit for bit: nothing overwrites the detector's Result
    before the table has been made of it, and no table is made before the detector's pass has ended."""
    from pyopenvino_amd import DetectedRois, synth
    blob = synth.synth_weights(os.path.join(MODELS, 'googlenet-v1.xml'), 11)
    rng = np.random.default_rng(78)
    m, n, hw, steps = 2, 8, (480, 640), 6
    frames = [_frames(rng, 'U8-NHWC', m, hw) for _ in range(steps)]
    det, det_name, det_out = _detector(m)
    dreq = det.requests[0]
    ex_ref, name, out_name = _classifier('U8-NHWC', n, blob)
    ex, _, _ = _classifier('U8-NHWC', n, blob, requests=2)
    wants = []
    for f in frames:                                          # the host route of every step
        rec = np.array(dreq.infer({det_name: f})[det_out], copy=True)
        conf = _median_live_score(rec, m)
        wants.append((rec, conf) + _host_route(ex_ref, name, out_name, f, rec, m, hw, min_confidence=conf))
    assert len({w[2].rois.tobytes() for w in wants}) > 1      # the steps differ
    assert dreq.runner._graph is not None                     # (the detector replays its recording by now)
    dreq.start_async({det_name: frames[0]})
    for step in range(steps):
        rec, conf, want, want_out = wants[step]
        req = ex.requests[step % 2]
        req.start_async({name: DetectedRois(frames[step], dreq, min_confidence=conf)})
        assert_bit_exact(dreq.wait()[det_out], rec, 'step {} detector'.format(step))
        if step + 1 < steps:
            dreq.start_async({det_name: frames[step + 1]})    # at once: the classifier's pass may not even have begun
            assert dreq._replayed is not None
        if step >= 4:
            assert req._replayed is not None, 'step {} was not replayed'.format(step)
        got_out = req.wait()[out_name]
        _same(req.detected_rois(name), want, 'step {}'.format(step))
        assert want.count >= 1
        assert_bit_exact(got_out[:want.count], want_out[:want.count], 'step {}'.format(step))
