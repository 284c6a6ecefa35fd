"""A detector over regions (``infer({input: RoiInput(...) or DetectedRois(...)}, detections=RegionScreen(...))``,
pvhip_detections_merge_regions): the batch rows are regions of any aspect, placed in the detector's input by the declared resize_fit, and
their records become one table of frame detections by the rule of tests/regions_ref.py, word for word -- a second-stage detector's boxes
in frame pixels without a host round trip.  The first tests need no GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import detections_ref
import helpers
import regions_ref
import test_detected_rois as det_tests
import test_detections as plain_tests
import test_roi_input as roi_tests
import test_tiled_detections as tiled_tests
import tiles_ref

ENTRY = 'pvhip_detections_merge_regions'
TILES_ENTRY = 'pvhip_detections_merge_tiles'
ARGS = 21
NAN, INF = np.nan, np.inf
MODELS = os.path.join(helpers.REPO, 'models')
_net, _frames, _rec, END = roi_tests._net, roi_tests._frames, det_tests._rec, det_tests.END
_same, _equal, _bits = plain_tests._same, plain_tests._equal, plain_tests._bits
FITTED = ('LETTERBOX', 'TOP_LEFT')
FIT_CODES = {'STRETCH': 0, 'LETTERBOX': 1, 'TOP_LEFT': 2}


def _both(rec, regions, m, net_hw, fit, **opt):
    """tests/regions_ref.py and the product's own numpy form agree word for word: the product's Detections."""
    from pyopenvino_amd import RegionScreen, tiled_detections
    want = regions_ref.merge(rec, regions, m, net_hw, fit, **opt)
    got = tiled_detections.merge_regions(rec, regions, m, RegionScreen(**opt), net_hw, fit)
    _same(got, want, '{} {}'.format(fit, opt))
    return got


def _table(d):
    return [tuple(r) + (l,) for r, l in zip(d.rois.tolist(), d.labels.tolist())]


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
REGION = np.array([(0, 100, 50, 160, 90)], np.int32)          # 16:9 in front of a 300 x 300 input
HAND = np.array([_rec(0, 1, 0.9, 0.25, 0.5, 0.5, 0.75),       # inside the picture
                 _rec(1, 2, 0.8, 0.25, 0.1, 0.5, 0.5),        # from the padding above into the picture
                 _rec(2, 3, 0.7, 0.25, 0.0, 0.5, 0.2),        # wholly in the padding above (rows 0 .. 60 of 65)
                 _rec(3, 4, 0.7, 0.25, 0.9, 0.5, 1.0),        # wholly in the padding below (rows 270 .. 300, the picture ends at 234)
                 _rec(4, 5, 0.6, 0.25, 0.5, INF, 0.75),       # a corner that is not finite
                 _rec(5, 6, 0.6, 0.0, 0.5, 1.0, NAN),
                 END,
                 _rec(7, 7, 0.99, 0.25, 0.5, 0.5, 0.75)], np.float32)       # behind the terminator


def test_the_rule_on_hand_written_records():
    """One 160 x 90 region at (100, 50) of frame 0 in a 300 x 300 input: LETTERBOX places it in rows 65 .. 234 (169 = (2 90 300 + 160)
    // 320), so y = (v 300 - 65) / 169 of the region's 90 rows and x = v of its 160 columns."""
    from pyopenvino_amd import input_format
    assert regions_ref.geometry(90, 160, 300, 300, 'LETTERBOX') == (0, 65, 300, 169) == input_format.fit_geometry((90, 160), (300, 300), 'LETTERBOX')
    d = _both(HAND, REGION, 1, (300, 300), 'LETTERBOX', threshold=1.0)
    # inside: x 40 .. 80; y0 = floor(85 / 169 * 90 = 45.27), y1 = ceil(160 / 169 * 90 = 85.2).  straddling: y0 clamps to the region's edge
    assert _table(d) == [(0, 140, 95, 40, 41, 1), (0, 140, 50, 40, 46, 2)]
    assert d.counts.tolist() == d.selected.tolist() == [2] and d.records.tolist() == [0, 1]
    assert np.array_equal(d.scores.view(np.uint32), HAND[d.records, 2].view(np.uint32))
    assert _both(HAND, REGION, 1, (300, 300), 'LETTERBOX', threshold=1.0, min_size=(42, 1)).records.tolist() == [1]
    assert _both(HAND, REGION, 1, (300, 300), 'LETTERBOX', threshold=0.01, per_label=False).records.tolist() == [0]      # one common row of 40 pixels
    assert _both(HAND, REGION, 1, (300, 300), 'LETTERBOX', labels=[2, 3]).records.tolist() == [1]
    assert _both(HAND, REGION, 1, (300, 300), 'LETTERBOX', max_per_region=1).records.tolist() == [0]
    # the region's frame is outside [0, m), it has no extent or one above 2^24: nothing
    for row in ((1, 100, 50, 160, 90), (-1, 0, 0, 0, 0), (0, 100, 50, 0, 90), (0, 100, 50, 160, -1), (0, 0, 0, 2 ** 24 + 1, 90)):
        d = _both(HAND, np.array([row], np.int32), 1, (300, 300), 'LETTERBOX')
        assert d.counts.tolist() == d.selected.tolist() == [0] and d.rois.shape == (0, 5)
    assert _both(HAND, np.array([(0, 2 ** 31 - 1, -2 ** 31, 160, 90)], np.int32), 1, (300, 300), 'LETTERBOX', threshold=1.0).rois.tolist() == [
        [0, -2 ** 31 + 39, -2 ** 31 + 45, 40, 41], [0, -2 ** 31 + 39, -2 ** 31, 40, 46]]            # the sums wrap as int32 do
    # what merge_regions refuses
    from pyopenvino_amd import RegionScreen, tiled_detections
    for bad_rec, bad_table, frames, hw, fit in ((HAND[:, :6], REGION, 1, (300, 300), 'LETTERBOX'), (HAND, REGION.astype(np.float32), 1, (300, 300), 'LETTERBOX'),
                                                (HAND, REGION, 0, (300, 300), 'LETTERBOX'), (HAND, REGION, 1, None, 'LETTERBOX'),
                                                (HAND, REGION, 1, (0, 300), 'TOP_LEFT'), (HAND, REGION, 1, (300, 2 ** 24 + 1), 'TOP_LEFT'),
                                                (HAND, REGION, 1, (300, 300), 'letterbox'), (HAND, REGION, 1, (300, 300), 1)):
        with pytest.raises(ValueError, match='^detections: '):
            tiled_detections.merge_regions(bad_rec, bad_table, frames, RegionScreen(), hw, fit)
    assert tiled_detections.merge_regions(HAND, REGION, 1, 0.75, [300, 300], 'LETTERBOX').records.tolist() == [0, 1]     # a min_confidence alone


def test_top_left_and_regions_of_other_aspects():
    from pyopenvino_amd import input_format
    # the same records under TOP_LEFT: rows 0 .. 169 hold the picture, so the box "in the padding above" is inside it
    d = _both(HAND, REGION, 1, (300, 300), 'TOP_LEFT', threshold=1.0)
    assert regions_ref.geometry(90, 160, 300, 300, 'TOP_LEFT') == (0, 0, 300, 169)
    # y0 = floor(150 / 169 * 90 = 79.9), y1 clamps to 90; floor(30 / 169 * 90 = 15.98) .. ceil(79.9); 0 .. ceil(60 / 169 * 90 = 31.95)
    assert _table(d) == [(0, 140, 129, 40, 11, 1), (0, 140, 65, 40, 65, 2), (0, 140, 50, 40, 32, 3)] and d.records.tolist() == [0, 1, 2]
    cases = (((0, 10, 20, 50, 200), (112, 0, 75, 300), (0, 0, 75, 300)),           # taller than wide: 75 = (2 50 300 + 200) // 400
             ((0, 5, 5, 1, 100), (148, 0, 3, 300), (0, 0, 3, 300)),                # one pixel wide: 3 = (2 1 300 + 100) // 200
             ((0, 7, 9, 150, 150), (0, 0, 300, 300), (0, 0, 300, 300)),            # exactly the network's aspect
             ((0, 0, 0, 1000, 1), (0, 149, 300, 1), (0, 0, 300, 1)))               # the short side rounds to 0 and is kept at 1
    rec = np.array([_rec(0, 1, 0.9, 0.0, 0.0, 1.0, 1.0), _rec(1, 1, 0.8, 0.4, 0.25, 0.6, 0.75), _rec(2, 2, 0.7, 0.45, 0.5, 0.55, 0.5),
                    _rec(3, 2, 0.6, 0.1, 0.3, 0.2, 0.6), END], np.float32)
    for row, boxed, top_left in cases:
        _, x, y, w, h = row
        for fit, g in (('LETTERBOX', boxed), ('TOP_LEFT', top_left)):
            assert regions_ref.geometry(h, w, 300, 300, fit) == g == input_format.fit_geometry((h, w), (300, 300), fit), (row, fit)
            d = _both(rec, np.array([row], np.int32), 1, (300, 300), fit, threshold=1.0)
            assert d.records[0] == 0 and d.rois[0].tolist() == [0, x, y, w, h], (row, fit)       # the whole input is the whole region
            assert ((d.rois[:, 1] >= x) & (d.rois[:, 2] >= y) & (d.rois[:, 1] + d.rois[:, 3] <= x + w) & (d.rois[:, 2] + d.rois[:, 4] <= y + h)).all()
    d = _both(rec, np.array([cases[0][0]], np.int32), 1, (300, 300), 'LETTERBOX', threshold=1.0)
    # record 1: x = (v 300 - 112) / 75 of 50 columns: floor(8 / 75 * 50 = 5.3) .. ceil(68 / 75 * 50 = 45.3); y = v of 200 rows
    assert d.rois[1].tolist() == [0, 10 + 5, 20 + 50, 41, 100] and d.records.tolist() == [0, 1]  # (records 2, 3: no height; in the padding)
    # a network that is not square, a region wider than it
    assert regions_ref.geometry(90, 160, 240, 416, 'LETTERBOX') == (0, 3, 416, 234)
    _both(rec, REGION, 1, (240, 416), 'LETTERBOX', threshold=1.0)


def _regions(rng, n, P, m, net_hw, fit, extent=(96, 128), specials=True, labels=3):
    """(records, table) of n regions of mixed aspect over m frames of `extent`: every box is drawn around one of a few centres its frame's
    regions share and written in the coordinates of the detector's input, where `fit` placed its region; the last rows of a table of three
    or more are (-1, 0, 0, 0, 0), as a DetectedRois table has them behind `count`; `specials` as test_tiled_detections._clustered."""
    H, W = extent
    R = n * P
    t = np.zeros((n, 5), np.int32)
    t[:, 0] = rng.permutation(np.arange(n) % m)
    t[:, 3], t[:, 4] = rng.integers(W // 3, W + 1, n), rng.integers(H // 3, H + 1, n)
    thin = rng.integers(0, 6, n)
    t[thin == 0, 3], t[thin == 1, 4] = rng.integers(1, 9, n)[thin == 0], rng.integers(1, 9, n)[thin == 1]
    t[:, 1], t[:, 2] = rng.integers(0, W - t[:, 3] + 1), rng.integers(0, H - t[:, 4] + 1)
    centres = rng.uniform(0.3, 0.7, (m, 4, 2)) * (W, H)
    sizes = rng.uniform(8, 30, (m, 4, 2))
    row = np.repeat(np.arange(n), P)
    frame, which = t[row, 0], rng.integers(0, 4, R)
    mid = centres[frame, which] + rng.normal(0, 1.5, (R, 2))
    half = sizes[frame, which] / 2 * rng.uniform(0.85, 1.15, (R, 2))
    Hn, Wn = net_hw
    g = np.array([regions_ref.geometry(t[b, 4], t[b, 3], Hn, Wn, fit) if fit != 'STRETCH' else (0, 0, Wn, Hn) for b in range(n)], np.float64)[row]
    rec = np.zeros((R, 7), np.float32)
    rec[:, 0] = np.tile(np.arange(P), n)
    rec[:, 1] = (which + rng.integers(0, 2, R)) % labels
    rec[:, 2] = rng.uniform(0, 1, R)
    for k, (sign, axis) in enumerate(((-1, 0), (-1, 1), (1, 0), (1, 1))):
        u = (mid[:, axis] + sign * half[:, axis] - t[row, 1 + axis]) / t[row, 3 + axis]            # in the region
        rec[:, 3 + k] = (u * g[:, 2 + axis] + g[:, axis]) / (Wn, Hn)[axis]                       # in the detector's input
    if specials and P > 1:
        k = rng.integers(0, 24, R)
        rec[k == 0, 2] = NAN
        rec[k == 1, 3 + rng.integers(0, 4)] = INF
        rec[k == 2, 3 + rng.integers(0, 4)] = -INF
        rec[k == 3, 3 + rng.integers(0, 4)] = NAN
        rec[k == 4, 5] = rec[k == 4, 3]
        rec[k == 5, 2] = 0.5
        rec[k == 6, 2] = -0.0
        rec[k == 7, 2] = 0.0
        rec[k == 8, 2] = INF
        rec[k == 9, 1] = NAN
        rec[k == 10, 3:7] = rng.uniform(0, 1, ((k == 10).sum(), 4))                               # anywhere, the padding included
        for b in range(n):
            end = int(rng.integers(0, P + 1 + P // 2))
            if end < P:
                rec[b * P + end] = END
                rec[b * P + end, 0] = NAN if rng.integers(0, 4) == 0 else -1
    if n >= 3:
        t[n - max(1, n // 8):] = (-1, 0, 0, 0, 0)
    return rec, t


def _net_hw(n):
    return (300, 300) if n % 2 else (240, 416)


CPU_SHAPES = tiled_tests.CPU_SHAPES
OPTIONS = [{('max_per_region' if k == 'max_per_tile' else k): v for k, v in opt.items()} for opt in tiled_tests.OPTIONS]


@pytest.mark.parametrize('n,P,m', CPU_SHAPES)
def test_stretch_equals_the_tiled_screen(n, P, m):
    """merge_regions(..., fit='STRETCH') is merge_tiles word for word, on test_tiled_detections' own clustered records, and both are
    tiles_ref; net_hw is not looked at."""
    from pyopenvino_amd import RegionScreen, TiledScreen, tiled_detections
    rng = np.random.default_rng(n * 4099 + P * 17 + m)
    rec, tiles = tiled_tests._clustered(rng, n, P, m)
    for opt, tiled_opt in zip(OPTIONS, tiled_tests.OPTIONS):
        tiled = tiled_detections.merge_tiles(rec, tiles, m, TiledScreen(**tiled_opt))
        for got in (tiled_detections.merge_regions(rec, tiles, m, RegionScreen(**opt)),
                    tiled_detections.merge_regions(rec, tiles, m, RegionScreen(**opt), (300, 300), 'STRETCH')):
            for a, b in zip(got, tiled):
                assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), opt
        _same(got, tiles_ref.merge(rec, tiles, m, **tiled_opt), str(opt))
        _same(got, regions_ref.merge(rec, tiles, m, None, 'STRETCH', **opt), str(opt))


@pytest.mark.parametrize('fit', FITTED)
def test_numpy_form_equals_the_rule_on_regions_of_mixed_aspect(fit):
    """merge_regions is regions_ref on clustered records over tables of mixed aspect with (-1, 0, 0, 0, 0) rows.  The reference itself must
    keep at least two candidates and suppress one on at least one case per fit."""
    busy = 0
    for n, P, m in CPU_SHAPES:
        rng = np.random.default_rng(n * 4099 + P * 17 + m + 7 * FIT_CODES[fit])
        rec, table = _regions(rng, n, P, m, _net_hw(n), fit)
        assert n < 3 or (table[-1] == (-1, 0, 0, 0, 0)).all()
        want = regions_ref.merge(rec, table, m, _net_hw(n), fit, min_confidence=0.1)
        print('{} selected {} counts {}'.format((n, P, m), want.selected.tolist(), want.counts.tolist()))
        busy += bool(want.counts.sum() >= 2 and want.selected.sum() > want.counts.sum())
        for opt in OPTIONS:
            _both(rec, table, m, _net_hw(n), fit, **opt)
    assert busy >= 1


def _ssd(fit='LETTERBOX', pad=114.0, batch=4, requests=1):
    """SSD-MobileNet as tests/test_detected_rois.py's detector -- U8 / NHWC frames, reversed channels, a resize -- with `fit` declared."""
    from pyopenvino_amd import synth
    blob = synth.synth_weights(os.path.join(MODELS, 'ssd_mobilenet_v1_coco.xml'), 1234)
    ie, net, name = _net('ssd_mobilenet_v1_coco', batch, blob)
    roi_tests._declare(net, name, 'U8-NHWC', reverse=True)
    if fit is not None:
        net.input_info[name].preprocess_info.resize_fit = fit
        net.input_info[name].preprocess_info.pad_value = pad
    return ie.load_network(net, 'GPU', num_requests=requests), name, net.outputs[0]['name']


TABLE = np.array([(0, 0, 0, 40, 24), (1, 10, 0, 20, 48), (0, 24, 8, 40, 30), (1, 0, 40, 64, 8)], np.int32)     # 4 regions of 2 (48, 64) frames


@pytest.mark.parametrize('fit', ('STRETCH',) + FITTED)
def test_argument_rules(fit):
    """Both feeds are accepted and every refusal is a ValueError that starts with 'detections: ', raised before anything is staged or
    launched, whatever fit the input declares: this test runs where there is no device."""
    from pyopenvino_amd import DetectedRois, Detections, DetectionScreen, RegionScreen, RoiInput, TiledScreen, detections, device, tiled_detections
    ex, name, out_name = _ssd(None if fit == 'STRETCH' else fit, requests=2)
    frames = np.zeros((2, 48, 64, 3), np.uint8)
    roi = RoiInput(frames, TABLE)
    detected = DetectedRois(frames, np.zeros((2, 7), np.float32))
    req = ex.requests[0]
    want = RegionScreen(0.5, None, (1, 1), 100, 'IOU', 0.45, True, 400, name)

    def idle():
        for r in ex.requests:
            assert not r._in_flight and not r._asks and not r.runner.answers.blocks
            assert not r.runner.host_inputs.slots and r.runner._pending is None

    # accepted: checked() makes a RegionAsk of either feed, with the input's extent and its declared fit
    for feed in (roi, detected):
        for screen in (RegionScreen(), {out_name: RegionScreen(input=name)}):
            asks = req.runner.answers.checked({name: feed}, None, screen, False)
            ask = asks[out_name]
            assert list(asks) == [out_name] and type(ask) is tiled_detections.RegionAsk and ask.screen == want and type(ask.screen) is RegionScreen
            assert (ask.tiles, ask.frames, ask.slot, ask.net_hw, ask.fit, ask.detected) == (4, None, None, (300, 300), fit, None)
            assert callable(ask.table_of)
    idle()

    def starts(x):
        return (lambda d: ex.infer({name: x}, detections=d), lambda d: ex.infer({name: x}, False, None, d),
                lambda d: req.start_async({name: x}, detections=d), lambda d: ex.requests[1].infer({name: x}, None, d),
                lambda d: ex.start_async(1, {name: x}, detections=d), lambda d: ex.start_async(0, {name: x}, None, d))

    # ... and every start gets as far as the device with them: the first thing a pass needs of it is a page-locked buffer
    for feed in (roi, detected):
        for start in starts(feed):
            for screen in (RegionScreen(), {out_name: RegionScreen()}):
                try:
                    start(screen)
                except ValueError as e:
                    raise AssertionError('refused: {}'.format(e))
                except Exception:                                                   # (no device here)
                    pass
                for r in ex.requests:
                    if r._in_flight:                                                # (a device: the pass ran)
                        assert isinstance(r.wait()[out_name], Detections)
                    r._asks = {}
                    r.runner.answers.release()
                    r.runner.host_inputs.release()

    def refused(match, d, x=roi, top_k=None):
        for start in starts(x) if top_k is None else (lambda d: req.start_async({name: x}, top_k, d), lambda d: ex.infer({name: x}, False, top_k, d)):
            with pytest.raises(ValueError, match=match) as e:
                start(d)
            assert str(e.value).startswith('detections: '), str(e.value)
        idle()

    def each_form(match, **opt):
        refused(match, RegionScreen(**opt))
        refused(match, {out_name: RegionScreen(**opt)})

    # the named input is fed anything but a RoiInput or a DetectedRois
    for x in (np.zeros((4, 48, 64, 3), np.uint8), np.zeros((4, 3, 300, 300), np.float32), types.SimpleNamespace(frames=frames, rois=TABLE),
              object.__new__(device.DeviceTensor)):
        refused('a RegionScreen needs input .* fed a RoiInput or a DetectedRois', RegionScreen(), x)
        refused('a RegionScreen needs input .* fed a RoiInput or a DetectedRois', {out_name: RegionScreen(input=name)}, x)
    for bad in ('nope', 3, out_name):
        each_form('no 4-D Parameter', input=bad)
    # the screen's values: a TiledScreen's
    for bad in ('iou', 'GIOU', None, 0):
        each_form("overlap is 'IOU' or 'IOS'", overlap=bad)
    for bad in (NAN, INF, -0.001, 1.001, '0.5', True, None):
        each_form('threshold', threshold=bad)
    for bad in (0, None, 'yes'):
        each_form('per_label is a bool', per_label=bad)
    for key in ('max_per_region', 'max_per_frame'):
        for bad in (0, -1, 1.5, True, 2 ** 31):
            each_form(key + ' is None or a count', **{key: bad})
    for bad in (NAN, '0.5', True):
        each_form('min_confidence', min_confidence=bad)
    for bad in (list(range(65)), [1.0], 3):
        each_form('at most 64 ints', labels=bad)
    for bad in ((0, 1), 1, (1.0, 1)):
        each_form('min_size', min_size=bad)
    with pytest.raises(TypeError):
        RegionScreen(max_per_tile=3)
    # what detections= refuses for every screen
    refused('no Result named', {'nope': RegionScreen()})
    ex.comm = types.SimpleNamespace(world=2, rank=0)
    try:
        each_form('sharded')
    finally:
        ex.comm = None
    refused('asked for with top_k as well', {out_name: RegionScreen()}, top_k={out_name: 1})
    refused('asked for with top_k as well', {out_name: RegionScreen()}, detected, top_k={out_name: 0})   # the clash, not top_k's refusal
    refused('threshold 2 is not a finite number', RegionScreen(threshold=2), np.zeros((4, 48, 64, 3), np.uint8))    # the value, not the feed
    # the candidate capacity
    assert tiled_detections.resolved(RegionScreen(), 4, 100).max_per_region == 100 and tiled_detections.resolved(RegionScreen(), 64, 100).max_per_region == 64
    assert tiled_detections.resolved(RegionScreen(max_per_region=5000), 4, 100).max_per_region == 100
    assert tiled_detections.resolved(RegionScreen(), 4096, 7).max_per_region == 1
    assert tiled_detections.resolved(RegionScreen(max_per_region=64), 64, 100).max_per_frame == 4096
    for n, P, cap in ((64, 100, 65), (4097, 1, None), (41, 100, 100)):
        with pytest.raises(ValueError, match='^detections: .*(lower max_per_region|4097 regions are more than the 4096)'):
            tiled_detections.resolved(RegionScreen(max_per_region=cap), n, P)
    # its one form: equal screens are equal keys; the pinned field list; no kin of the other screens
    assert detections.checked(ex.ienet, RegionScreen(), False) == {out_name: want}
    got = detections.checked(ex.ienet, RegionScreen(1, np.array([3, 1]), [2, 3], 1000, 'IOS', 1, np.True_, 7), False)[out_name]
    assert got == RegionScreen(1.0, (3, 1), (2, 3), 100, 'IOS', 1.0, True, 7, name) and hash(got) == hash(got._replace())
    assert isinstance(got.threshold, float) and isinstance(got.per_label, bool) and type(got) is RegionScreen
    assert RegionScreen() == RegionScreen(0.5, None, (1, 1), None, 'IOU', 0.45, True, None, None) and RegionScreen._fields == (
        'min_confidence', 'labels', 'min_size', 'max_per_region', 'overlap', 'threshold', 'per_label', 'max_per_frame', 'input')
    assert not isinstance(RegionScreen(), (TiledScreen, DetectionScreen)) and not isinstance(TiledScreen(), RegionScreen)
    with pytest.raises(AttributeError):
        want.threshold = 0.1
    # the other screens refuse what they refused: a TiledScreen a DetectedRois, and on a fitted input both screens
    refused('a TiledScreen needs input .* fed a RoiInput' if fit == 'STRETCH' else 'a TiledScreen over input .* resize_fit', TiledScreen(), detected)
    if fit != 'STRETCH':
        refused('a TiledScreen over input .* resize_fit ' + fit, TiledScreen())
        refused('declares resize_fit {} and is fed a RoiInput'.format(fit), 0.5)
        refused('declares resize_fit {} and is fed a DetectedRois'.format(fit), {out_name: DetectionScreen()}, detected)


@pytest.mark.parametrize('fit', FITTED)
def test_the_stage_on_host_values(fit):
    """checked(), bound(), launch() and read() on a Result that is a host array, as test_answers.py does it for tiles: the answer is the
    rule in numpy on the slot's page-locked table -- for a DetectedRois on the table read back --, nothing is recorded, no block is made."""
    from pyopenvino_amd import DetectedRois, RegionScreen, RoiInput, input_format, tiled_detections
    rng = np.random.default_rng(402)
    ex, name, out_name = _ssd(fit)
    answers = ex.answers
    rec = det_tests._random_records(rng, 4, 100).reshape(1, 1, 400, 7)
    opt = dict(min_confidence=0.25, labels=[5, 0, 3], threshold=0.1, per_label=False)
    frames = np.zeros((2, 48, 64, 3), np.uint8)
    want = regions_ref.merge(rec, TABLE, 2, (300, 300), fit, **opt)
    assert want.counts.sum() >= 2 and want.selected.sum() > want.counts.sum()
    behind = TABLE.copy()
    behind[3] = (-1, 0, 0, 0, 0)                               # what a DetectedRois that found three regions leaves
    read = []
    for feed, table in ((RoiInput(frames, TABLE), TABLE), (DetectedRois(frames, np.zeros((2, 7), np.float32)), behind)):
        asks = answers.checked({name: feed}, None, {out_name: RegionScreen(**opt)}, False)
        detected = isinstance(feed, DetectedRois)
        # (stage() fills the slot on a device; here by hand: a RoiInput's page-locked table, a DetectedRois' read-back)
        ex.host_inputs.slots[name] = types.SimpleNamespace(tables={'roi': types.SimpleNamespace(host=None if detected else table.copy(), device=None)})
        asks[out_name] = asks[out_name]._replace(table_of=lambda: read.append(1) or input_format.DetectedTable(3, 3, behind.copy(), np.arange(4, dtype=np.int32)))
        try:
            asks = answers.bound(asks, {name: feed})
            ask = asks[out_name]
            assert type(ask) is tiled_detections.RegionAsk and (ask.frames, ask.detected, ask.fit, ask.net_hw) == (2, detected, fit, (300, 300))
            assert ask.key(out_name) == (out_name, RegionScreen(0.25, (5, 0, 3), (1, 1), 100, 'IOU', 0.1, False, 400, name), 2)
            _same(answers.read(out_name, ask, rec), regions_ref.merge(rec, table, 2, (300, 300), fit, **opt), type(feed).__name__)
            assert len(read) == int(detected)
            answers.launch(asks, {out_name: rec})
            assert ex._pending is None and answers.blocks == {}
        finally:
            ex.host_inputs.release()


def test_abi_declares_the_entry():
    import pyopenvino_amd
    from pyopenvino_amd import device, tiled_detections
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert ENTRY in device.SIGNATURES and len(device.SIGNATURES[ENTRY][1]) == ARGS and ENTRY not in device._NOT_STATUS
    m = re.search(r'\bint\s+' + ENTRY + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S)
    assert m and len(m.group(1).split(',')) == ARGS
    names = [a.split()[-1].lstrip('*') for a in m.group(1).split(',')]
    assert names == ['records', 'regions', 'n', 'records_per_region', 'frames', 'min_confidence', 'labels', 'num_labels', 'min_h', 'min_w',
                     'max_per_region', 'overlap', 'threshold', 'per_label', 'max_per_frame', 'net_h', 'net_w', 'fit', 'scratch', 'header', 'rows']
    comment = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int\s+' + ENTRY, header, flags=re.S).group(1)
    for phrase in ('Addition to ABI v18 (the version number is unchanged', '(-1, 0, 0, 0, 0)', 'pvhip_detections_compact_fit', 'three roundings',
                   'never contracted', 'one wholly in the padding is dropped', 'bit for bit', 'tests/regions_ref.py', 'fit in {0, 1, 2}',
                   'net_h, net_w in [1, 2^24] when fit != 0'):
        assert phrase in comment, phrase                       # the rule is stated there
    assert re.search(r'#define\s+PVHIP_ABI_VERSION\s+19\b', header)
    lib = device.load_library()
    assert hasattr(lib, ENTRY) and lib.pvhip_abi_version() == 19
    assert pyopenvino_amd.RegionScreen is tiled_detections.RegionScreen and 'RegionScreen' in pyopenvino_amd.__all__
    # the launch that places the pixels and the launch that maps the boxes back share one function
    csrc = os.path.join(helpers.REPO, 'pyopenvino_amd', 'csrc')
    defined = [f for f in sorted(os.listdir(csrc)) if f.endswith(('.hip', '.h')) and re.search(r'\bFitRect\s+fit_rect\s*\(', open(os.path.join(csrc, f)).read())]
    assert defined == ['pvhip_fit_rect.h']
    for source in ('pvhip_preprocess.hip', 'pvhip_tiles.hip'):
        text = open(os.path.join(csrc, source)).read()
        assert '#include "pvhip_fit_rect.h"' in text and re.search(r'=\s*fit_rect\(', text), source


# ---------------------------------------------------------------------------------------------------------------- GPU
SENTINEL = 0x7f7f7f7f


def _device_merge(hip, rec, table, m, net_hw, fit, entry=ENTRY, min_confidence=0.5, labels=None, min_size=(1, 1), max_per_region=None,
                  overlap='IOU', threshold=0.45, per_label=True, max_per_frame=None):
    """`entry` on `rec` and `table`: header, rows and scratch prefilled with 0x7f bytes, each with guard words behind it, as a Compacted;
    nothing from `total` onward and nothing behind the scratch may be written."""
    n = table.shape[0]
    P = rec.reshape(-1, 7).shape[0] // n
    per_region = min(P, 4096 // n) if max_per_region is None else min(P, max_per_region)
    slots = n * per_region
    per_frame = slots if max_per_frame is None else min(max_per_frame, slots)
    capacity = min(slots, m * per_frame)
    src = hip.DeviceTensor.from_numpy(rec)
    dev_table = hip.DeviceTensor.from_numpy(np.ascontiguousarray(table, np.int32))
    header = hip.DeviceTensor.empty((2 * m + 1 + 8,), np.int32)
    rows = hip.DeviceTensor.empty((capacity + 1, 8), np.int32)
    scratch = hip.DeviceTensor.empty((9 * slots + n + 8,), np.int32)
    for t in (header, rows, scratch):
        hip.call('pvhip_memset', ctypes.c_void_p(t.ptr), 0x7f, t.nbytes)
    lab = hip.DeviceTensor.from_numpy(np.asarray(list(labels) + [0], np.int32)) if labels is not None else None      # ([]: no label passes)
    placed = (net_hw[0], net_hw[1], FIT_CODES[fit]) if entry == ENTRY else ()
    hip.call(entry, ctypes.c_void_p(src.ptr), ctypes.c_void_p(dev_table.ptr), n, P, m, min_confidence,
             ctypes.c_void_p(lab.ptr) if lab is not None else None, 0 if labels is None else len(labels), min_size[0], min_size[1], per_region,
             {'IOU': 0, 'IOS': 1}[overlap], threshold, int(per_label), per_frame, *placed, ctypes.c_void_p(scratch.ptr), ctypes.c_void_p(header.ptr),
             ctypes.c_void_p(rows.ptr))
    header, rows, scratch = np.asarray(header), np.asarray(rows).view(np.uint32), np.asarray(scratch)
    assert (header[2 * m + 1:] == SENTINEL).all(), 'a word behind the header was written'
    assert (scratch[9 * slots + n:] == SENTINEL).all(), 'a word behind the scratch was written'
    counts, selected, total = header[:m].copy(), header[m:2 * m].copy(), int(header[2 * m])
    assert 0 <= total <= capacity and total == counts.sum(), (total, capacity, counts.sum())
    assert (rows[total:] == SENTINEL).all(), 'a row from total onward was written'
    return detections_ref.Compacted(counts, selected, rows[:total].copy())


def _check(hip, rec, table, m, net_hw, fit, what, **opt):
    want = regions_ref.merge(rec, table, m, net_hw, fit, **opt)
    got = _device_merge(hip, rec, table, m, net_hw, fit, **opt)
    _equal(got, want, '{} {} {}'.format(what, fit, opt))
    if fit == 'STRETCH':                                       # the tiles entry's own output, word for word
        _equal(_device_merge(hip, rec, table, m, net_hw, fit, entry=TILES_ENTRY, **opt), got, '{} against the tiles entry {}'.format(what, opt))
    return want


# one record; a region around the chunk of 64 records; frames interleaved over the regions; regions not a multiple of the four waves of a
# workgroup over more frames; 4059 and exactly 4096 candidates
GPU_SHAPES = [(1, 1, 1, None), (1, 65, 1, None), (3, 65, 2, None), (130, 2, 7, None), (41, 100, 3, 99), (64, 64, 1, None)]
GPU_OPTIONS = [dict(), dict(overlap='IOS', threshold=0.3, per_label=False, min_confidence=-1.0), dict(labels=[2, 0], min_confidence=0.25),
               dict(min_size=(14, 17)), dict(max_per_region=1, max_per_frame=2, threshold=0.2), dict(threshold=1.0, min_confidence=-1.0)]


@pytest.mark.gpu
@pytest.mark.parametrize('fit', ('STRETCH',) + FITTED)
@pytest.mark.parametrize('n,P,m,per_region', GPU_SHAPES)
def test_kernel_equals_the_rule(hip, n, P, m, per_region, fit):
    rng = np.random.default_rng(n * 4099 + P * 17 + m + 29 * FIT_CODES[fit])
    net_hw = _net_hw(n)
    rec, table = _regions(rng, n, P, m, net_hw, fit)
    cap = dict() if per_region is None else dict(max_per_region=per_region)
    want = _check(hip, rec, table, m, net_hw, fit, 'clustered', min_confidence=0.1, **cap)
    print('selected {} counts {}'.format(want.selected.tolist(), want.counts.tolist()))
    if n * P >= 65:                                            # (the reference itself keeps two candidates and suppresses one)
        assert want.counts.sum() >= 2 and want.selected.sum() > want.counts.sum()
    for opt in GPU_OPTIONS:
        _check(hip, rec, table, m, net_hw, fit, 'clustered', **{**cap, **opt})
    # every record a candidate: n * per_region of them
    full, full_table = _regions(rng, n, P, m, net_hw, fit, specials=False)
    full_table[full_table[:, 0] < 0] = (0, 3, 5, 40, 24)       # (no row that takes nothing)
    full_table[:, 3:5] = np.maximum(full_table[:, 3:5], 9)
    full[:, 3:5], full[:, 5:7] = np.minimum(full[:, 3:5], 0.0), np.maximum(full[:, 5:7], 1.0)       # across the picture, wherever it was placed
    want = _check(hip, full, full_table, m, net_hw, fit, 'full', min_confidence=-1.0, **cap)
    assert want.selected.sum() == n * min(P, per_region or 4096 // n)
    _check(hip, full, full_table, m, net_hw, fit, 'full', min_confidence=-1.0, threshold=1.0, **cap)
    # regions with ids outside [0, m), regions without an extent or with one above 2^24, a row whose sums wrap
    odd = table.copy()
    odd[::3, 0], odd[1::5, 0], odd[2::7, 3], odd[3::11, 4] = -1, m, 0, -5
    odd[n // 2, 1:3] = (2 ** 31 - 1, -2 ** 31)
    if n >= 41:
        odd[7, 3], odd[8, 4] = 2 ** 24 + 1, 2 ** 24
    _check(hip, rec, odd, m, net_hw, fit, 'odd regions', min_confidence=0.1, **cap)
    # every region dead
    dead = rec.copy()
    dead[::P] = END
    got = _device_merge(hip, dead, table, m, net_hw, fit, min_confidence=-1.0, **cap)
    assert not got.counts.any() and not got.selected.any() and got.table.shape == (0, 8)


@pytest.mark.gpu
def test_entry_rejects_what_it_cannot_do(hip):
    rng = np.random.default_rng(5)
    rec, table = _regions(rng, 4, 8, 2, (300, 300), 'LETTERBOX')
    src = hip.DeviceTensor.from_numpy(rec)
    dev_table = hip.DeviceTensor.from_numpy(table)
    out = hip.DeviceTensor.empty((8 * 32 + 16,), np.int32)
    scratch = hip.DeviceTensor.empty((9 * 32 + 4 + 4,), np.int32)
    p = ctypes.c_void_p
    good = [p(src.ptr), p(dev_table.ptr), 4, 8, 2, 0.5, None, 0, 1, 1, 8, 0, 0.45, 1, 32, 300, 300, 1, p(scratch.ptr), p(out.ptr + 1024), p(out.ptr)]
    assert len(good) == ARGS
    hip.call(ENTRY, *good)
    for k, ok in ((17, 2), (15, 2 ** 24), (16, 1)):
        hip.call(ENTRY, *(good[:k] + [ok] + good[k + 1:]))
    hip.call(ENTRY, *(good[:15] + [0, -7, 0] + good[18:]))      # fit 0: net_h and net_w are not looked at
    for k, bad in ((17, 3), (17, -1), (15, 0), (15, -1), (15, 2 ** 24 + 1), (16, 0), (16, 2 ** 24 + 1),
                   # the tiles entry's own
                   (0, None), (1, None), (18, None), (19, None), (20, None), (20, p(out.ptr + 4)), (18, p(scratch.ptr + 8)), (2, 0), (3, 0), (4, 0),
                   (4, -1), (8, 0), (9, 0), (10, 0), (14, 0), (7, 65), (7, 1), (10, 1025), (2, 4097), (11, 2), (12, NAN), (12, 1.001),
                   (13, 2), (3, 2 ** 31 // 28 + 1)):
        args = list(good)
        args[k] = bad
        with pytest.raises(hip.PvhipError):
            hip.call(ENTRY, *args)
    for bad in ((0, 300, 1), (300, 0, 2), (2 ** 24 + 1, 300, 2)):
        with pytest.raises(hip.PvhipError):
            hip.call(ENTRY, *(good[:15] + list(bad) + good[18:]))
    hip.synchronize()
    _check(hip, rec, table, 2, (300, 300), 'LETTERBOX', 'after the refusals', min_confidence=0.1)      # the device is still usable


REGIONS = np.array([(0, 0, 0, 640, 360), (1, 40, 0, 300, 480), (0, 200, 100, 400, 225), (1, 320, 120, 240, 360)], np.int32)


@pytest.mark.gpu
def test_public_path_on_ssd_mobilenet(hip):
    """SSD-MobileNet at batch 4 with LETTERBOX and a pad value declared, on two U8 / NHWC (480, 640) frames and a RoiInput of four regions
    none of which is square: five starts of one request on the same RoiInput asking for nothing, a RegionScreen, a plain screen -- refused
    as it always was, nothing runs --, the RegionScreen, nothing; from the third pass on replayed from the request's one recording.  Each
    answer is the rule on the same request's own whole Result."""
    from pyopenvino_amd import DetectionScreen, Detections, RegionScreen, RoiInput
    rng = np.random.default_rng(96)
    m, n, hw = 2, 4, (480, 640)
    frames = _frames(rng, 'U8-NHWC', m, hw)
    det, name, out_name = _ssd('LETTERBOX', 114.0, n)
    req = det.requests[0]
    feed = RoiInput(frames, REGIONS)
    results, conf, passes = [], None, 0
    for call, kind in enumerate((None, 'region', 'plain', 'region', None)):
        if kind == 'plain':
            with pytest.raises(ValueError, match='^detections: .*declares resize_fit LETTERBOX and is fed a RoiInput'):
                req.start_async({name: feed}, detections=DetectionScreen(conf))
            assert not req._in_flight and not req._asks and det._pending is None
            results.append(None)
            continue
        req.start_async({name: feed}, detections=RegionScreen(conf) if kind else None)
        assert (req._replayed is not None) == (passes >= 2), 'call {}'.format(call)
        passes += 1
        results.append(req.wait()[out_name])
        if call == 0:
            full = np.array(results[0], copy=True)
            assert full.shape == (1, 1, 400, 7) and full.dtype == np.float32
            conf = det_tests._median_live_score(full, n)
    assert det._auto_graph['captured'] and det._graph is not None             # one recording served every kind
    want = regions_ref.merge(full, REGIONS, m, (300, 300), 'LETTERBOX', min_confidence=conf)
    print('conf {:.4f} selected {} counts {}'.format(conf, want.selected.tolist(), want.counts.tolist()))
    assert want.counts.sum() >= 1 and want.selected.sum() < 400
    assert isinstance(results[1], Detections)
    _same(results[1], want, 'call 1')
    _same(results[3], want, 'call 3')
    assert isinstance(results[4], np.ndarray) and np.array_equal(_bits(results[4]), _bits(full))     # whole and bit-equal without the keyword
    d = results[1]
    assert (d.records // 100 < n).all() and (REGIONS[d.records // 100, 0] == d.rois[:, 0]).all()
    x, y, w, h = REGIONS[d.records // 100, 1:].T                                # every box lies in its region
    assert ((d.rois[:, 1] >= x) & (d.rois[:, 2] >= y) & (d.rois[:, 1] + d.rois[:, 3] <= x + w) & (d.rois[:, 2] + d.rois[:, 4] <= y + h)).all()
    # the network's own infer() and the dict form; other options
    _same(det.infer({name: feed}, detections=RegionScreen(conf))[out_name], want, 'the network\'s own infer()')
    opt = dict(min_confidence=0.0, overlap='IOS', threshold=0.3, per_label=False, max_per_region=30, max_per_frame=5)
    want_cut = regions_ref.merge(full, REGIONS, m, (300, 300), 'LETTERBOX', **opt)
    _same(det.infer({name: feed}, False, None, {out_name: RegionScreen(input=name, **opt)})[out_name], want_cut, 'positional, the dict form')
    whole = req.infer({name: feed})[out_name]
    assert isinstance(whole, np.ndarray) and np.array_equal(_bits(whole), _bits(full))
    keys = sorted(det.answers.blocks, key=repr)
    assert len(keys) == 2 and all(type(k[1]) is RegionScreen and (k[0], k[2]) == (out_name, m) for k in keys)
    det.release_device_state()
    assert not det.answers.blocks


@pytest.mark.gpu
def test_two_stages_on_the_device(hip):
    """A detector at batch 2, started and not waited for; a second SSD at batch 4 with LETTERBOX declared, started on DetectedRois(frames,
    the detector's request) with detections=RegionScreen(...): after both waits its answer is the rule on its own Result and the table
    detected_rois() reads back, every box comes from a row in front of `count`, and the chain to the first-stage record holds.  The detector
    is restarted at once, on other frames: three pairs in all."""
    from pyopenvino_amd import DetectedRois, Detections, RegionScreen
    rng = np.random.default_rng(97)
    m, n, hw = 2, 4, (480, 640)
    det, det_name, det_out = det_tests._detector(m)
    second, name, out_name = _ssd('LETTERBOX', 114.0, n)
    first_req, req = det.requests[0], second.requests[0]
    sets = [_frames(rng, 'U8-NHWC', m, hw) for _ in range(2)]
    # a dry run of each set, everything read back: the first stage's records, the table, the second stage's whole Result
    dry = []
    for frames in sets:
        rec = np.array(first_req.infer({det_name: frames})[det_out], copy=True)
        scores = np.sort(rec.reshape(-1, 7)[rec.reshape(-1, 7)[:, 0] >= 0, 2])
        conf1 = float(scores[-3])                              # three regions pass: one batch row stays behind `count`
        full = np.array(req.infer({name: DetectedRois(frames, rec, images=m, min_confidence=conf1)})[out_name], copy=True)
        table = req.detected_rois(name)
        assert 1 <= table.count <= 3 and (table.rois[table.count:] == (-1, 0, 0, 0, 0)).all()
        live = full.reshape(n, 100, 7)[:table.count].reshape(-1, 7)
        dry.append((rec, conf1, full, table, float(np.median(live[live[:, 0] >= 0, 2]))))
    for step in range(3):
        frames = sets[step % 2]
        rec, conf1, full, table, conf2 = dry[step % 2]
        first_req.start_async({det_name: frames})
        req.start_async({name: DetectedRois(frames, first_req, min_confidence=conf1)}, detections=RegionScreen(conf2))
        if step < 2:                                           # restarted at once: its next pass waits until the table has been made
            first_req.wait()
            first_req.start_async({det_name: sets[(step + 1) % 2]})
        d = req.wait()[out_name]
        first_req.wait()
        got_table = req.detected_rois(name)
        det_tests._same(got_table, table, 'step {}'.format(step))
        want = regions_ref.merge(full, got_table.rois, m, (300, 300), 'LETTERBOX', min_confidence=conf2)
        print('step {} count {} selected {} counts {}'.format(step, got_table.count, want.selected.tolist(), want.counts.tolist()))
        assert isinstance(d, Detections) and want.counts.sum() >= 1
        _same(d, want, 'step {}'.format(step))
        region = d.records // 100
        assert (region < got_table.count).all()
        source = got_table.records[region]                     # the first-stage record each box came from
        assert (source >= 0).all() and (source // 100 == d.rois[:, 0]).all() and (rec.reshape(-1, 7)[source, 2] >= np.float32(conf1)).all()
    det.release_device_state()
    second.release_device_state()
