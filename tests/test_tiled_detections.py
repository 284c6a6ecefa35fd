"""A tiled detector's answer made on the device (``infer({input: RoiInput(frames, tiles)}, detections=TiledScreen(...))``,
pvhip_detections_merge_tiles): the records of all tiles become one table of frame detections by the rule of tests/tiles_ref.py, word for
word, three launches behind the pass and a read-back of the header and of exactly the rows it counts.  The first tests need no GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import detections_ref
import helpers
import test_detected_rois as det_tests
import test_detections as plain_tests
import test_roi_input as roi_tests
import tiles_ref

ENTRY = 'pvhip_detections_merge_tiles'
ARGS = 18
NAN, INF = np.nan, np.inf
_net, _frames, _rec, END, ZERO = roi_tests._net, roi_tests._frames, det_tests._rec, det_tests.END, det_tests.ZERO
_same, _equal = plain_tests._same, plain_tests._equal


def _both(rec, tiles, m, **opt):
    """tests/tiles_ref.py and the product's own numpy form agree word for word: the product's Detections."""
    from pyopenvino_amd import TiledScreen, tiled_detections
    want = tiles_ref.merge(rec, tiles, m, **opt)
    got = tiled_detections.merge_tiles(rec, tiles, m, TiledScreen(**opt))
    _same(got, want, str(opt))
    return got


def _table(d):
    return [tuple(r) + (l,) for r, l in zip(d.rois.tolist(), d.labels.tolist())]


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
def _hand_written():
    """Six tiles of 8 x 8 pixels with four records each over m = 3 frames (the corners are eighths, so every product is exact):
    tiles 0 and 1 of frame 0 overlap by half; tile 2 is frame 1's; tiles 3 and 4 have the ids -1 and m; tile 5 (frame 1) is dead; frame 2
    has no tile."""
    tiles = np.array([(0, 0, 0, 8, 8), (0, 4, 0, 8, 8), (1, 10, 20, 8, 8), (-1, 0, 0, 8, 8), (3, 0, 0, 8, 8), (1, 0, 0, 8, 8)], np.int32)
    live = _rec(0, 1, 0.99, 0.0, 0.0, 1.0, 1.0)
    rec = np.array([
        # tile 0
        _rec(0, 1, 0.9, 0.5, 0.25, 1.0, 0.75),                # an object in the overlap: frame (4, 2, 4, 4)
        _rec(1, 2, 0.7, 0.625, 0.0, 0.875, 0.25),             # a second one: frame (5, 0, 2, 2)
        _rec(2, 1, 0.3, 0.0, 0.0, 1.0, 1.0),                  # below min_confidence
        END,
        # tile 1, 4 pixels to the right
        _rec(0, 1, 0.8, 0.0, 0.25, 0.5, 0.75),                # the first object again with a lower score: frame (4, 2, 4, 4)
        _rec(1, 2, 0.7, 0.125, 0.0, 0.375, 0.25),             # the second one with an EQUAL score: the lower record wins
        _rec(2, 3, 0.6, -0.5, 0.5, 1.5, 2.0),                 # clamped to the tile: x 0..8, y 4..8 -> frame (4, 4, 8, 4)
        END,
        # tile 2 at (10, 20) of frame 1: A = 2 x 2, B = 2 x 1 inside it (inter / union = 2 / 4 exactly), C = B with another label
        _rec(0, 5, 0.9, 0.0, 0.0, 0.25, 0.25),
        _rec(1, 5, 0.8, 0.0, 0.0, 0.25, 0.125),
        _rec(2, 6, 0.75, 0.0, 0.0, 0.25, 0.125),
        END,
        live, live, live, live,                               # tile 3: frame -1
        live, live, live, live,                               # tile 4: frame m
        END, live, live, live,                                # tile 5: its list ends at position 0
    ], np.float32)
    return rec, tiles


def test_the_rule_on_hand_written_records():
    rec, tiles = _hand_written()
    m = 3
    o, o2, o3 = (0, 4, 2, 4, 4, 1), (0, 5, 0, 2, 2, 2), (0, 4, 4, 8, 4, 3)
    a, b, c = (1, 10, 20, 2, 2, 5), (1, 10, 20, 2, 1, 5), (1, 10, 20, 2, 1, 6)
    d = _both(rec, tiles, m, threshold=0.5)
    assert d.counts.tolist() == [3, 3, 0] and d.selected.tolist() == [5, 3, 0]
    assert _table(d) == [o, o2, o3, a, b, c]                  # the offset by (x, y), the clamp to the tile; inter / den == 0.5 is kept
    assert d.records.tolist() == [0, 1, 6, 8, 9, 10] and (d.records // 4).tolist() == [0, 0, 1, 2, 2, 2]
    assert np.array_equal(d.scores.view(np.uint32), rec[d.records, 2].view(np.uint32))
    assert _both(rec.reshape(1, 1, -1, 7), tiles.astype(np.int64), m, threshold=0.5).records.tolist() == [0, 1, 6, 8, 9, 10]
    d = _both(rec, tiles, m, threshold=0.49)                  # B is suppressed by A
    assert d.counts.tolist() == [3, 2, 0] and d.selected.tolist() == [5, 3, 0] and d.records.tolist() == [0, 1, 6, 8, 10]
    d = _both(rec, tiles, m, threshold=0.49, per_label=False)  # C too, across labels
    assert d.counts.tolist() == [3, 1, 0] and d.records.tolist() == [0, 1, 6, 8]
    d = _both(rec, tiles, m, overlap='IOS', threshold=1.0)    # inter / min(a, b) is 1.0 for A and B and for the copies: equality keeps
    assert d.counts.tolist() == [5, 3, 0] and d.records.tolist() == [0, 4, 1, 5, 6, 8, 9, 10]
    d = _both(rec, tiles, m, overlap='IOS', threshold=0.5)
    assert d.counts.tolist() == [3, 2, 0] and d.records.tolist() == [0, 1, 6, 8, 10]
    d = _both(rec, tiles, m, threshold=1.0)                   # nothing overlaps by more than 1: every candidate, ordered by score
    assert d.counts.tolist() == [5, 3, 0] and d.records.tolist() == [0, 4, 1, 5, 6, 8, 9, 10]
    d = _both(rec, tiles, m, threshold=0.0, per_label=False)  # any common pixel suppresses: (4, 4, 8, 4) meets the first object
    assert d.counts.tolist() == [2, 1, 0] and d.records.tolist() == [0, 1, 8]
    d = _both(rec, tiles, m, threshold=0.5, max_per_tile=1)
    assert d.counts.tolist() == [1, 1, 0] and d.selected.tolist() == [2, 1, 0] and d.records.tolist() == [0, 8]
    d = _both(rec, tiles, m, threshold=0.5, max_per_frame=1)
    assert d.counts.tolist() == [1, 1, 0] and d.selected.tolist() == [5, 3, 0] and _table(d) == [o, a]
    d = _both(rec, tiles, m, threshold=0.5, max_per_frame=2)
    assert d.counts.tolist() == [2, 2, 0] and d.selected.tolist() == [5, 3, 0] and d.records.tolist() == [0, 1, 8, 9]
    assert _both(rec, tiles, m, threshold=0.5, labels=[2, 6]).records.tolist() == [1, 10]
    assert _both(rec, tiles, m, threshold=0.5, labels=[]).records.tolist() == []
    assert _both(rec, tiles, m, threshold=0.5, min_size=(3, 1)).records.tolist() == [0, 6]
    # (record 2, the whole of tile 0, shares a quarter of its union with the first object: kept)
    assert _both(rec, tiles, m, threshold=0.5, min_confidence=0.25).records.tolist() == [0, 1, 6, 2, 8, 9, 10]
    assert _both(rec, tiles, m, threshold=0.2, min_confidence=0.25).records.tolist() == [0, 1, 6, 8, 10]
    assert _both(rec, tiles, m, threshold=0.5, min_confidence=0.25, per_label=False).selected.tolist() == [6, 3, 0]
    for f, want in ((0, [0, 1, 6]), (1, [8, 9, 10]), (2, []), (-1, [])):
        rois, labels, scores, records = _both(rec, tiles, m, threshold=0.5).of(f)
        assert records.tolist() == want and (rois[:, 0] == f % m).all()
    # more frames than any tile names; one frame fewer, so that frame 1's tiles are outside [0, m)
    assert _both(rec, tiles, 5, threshold=0.5).counts.tolist() == [3, 3, 0, 1, 0]           # (tile 4 is frame 3 now: four copies of one box)
    d = _both(rec, tiles, 1, threshold=0.5)
    assert d.counts.tolist() == [3] and d.records.tolist() == [0, 1, 6]
    # a tile without an extent, and a table that is no RoiInput's: the sums wrap as int32 do
    odd = tiles.copy()
    odd[0, 3], odd[2, 4] = 0, -8
    assert _both(rec, odd, m, threshold=0.5).records.tolist() == [4, 5, 6]
    odd = tiles.copy()
    odd[2, 1:3] = (2 ** 31 - 1, -2 ** 31)
    d = _both(rec, odd, m, threshold=0.5)
    assert d.rois[3:].tolist() == [[1, 2 ** 31 - 1, -2 ** 31, 2, 2], [1, 2 ** 31 - 1, -2 ** 31, 2, 1], [1, 2 ** 31 - 1, -2 ** 31, 2, 1]]
    # what merge_tiles refuses
    from pyopenvino_amd import TiledScreen, tiled_detections
    for bad_rec, bad_tiles, frames in ((rec.astype(np.float64), tiles, m), (rec[:, :6], tiles, m), (rec, tiles[:5], m), (rec, tiles[:, :4], m),
                                       (rec, tiles.astype(np.float32), m), (rec, tiles, 0)):
        with pytest.raises(ValueError, match='detections: '):
            tiled_detections.merge_tiles(bad_rec, bad_tiles, frames, TiledScreen())
    assert tiled_detections.merge_tiles(rec, tiles, m, 0.5).records.tolist() == [0, 1, 6, 8, 10]     # a min_confidence alone: the defaults


def _clustered(rng, n, P, m, extent=(96, 128), specials=True, labels=3, whole=False):
    """(records, tiles) of n tiles over m frames of `extent`: every box is drawn around one of a few centres its frame's tiles share and
    written in the coordinates of its tile, so the tiles of a frame report the same objects; `specials`: list ends anywhere, NaN scores,
    infinite and NaN corners, empty boxes and equal scores as well; `whole`: every tile is its whole frame."""
    H, W = extent
    R = n * P
    tiles = np.zeros((n, 5), np.int32)
    tiles[:, 0] = rng.permutation(np.arange(n) % m)
    tiles[:, 3], tiles[:, 4] = rng.integers(W // 2, W + 1, n), rng.integers(H // 2, H + 1, n)
    if whole:
        tiles[:, 3], tiles[:, 4] = W, H
    tiles[:, 1], tiles[:, 2] = rng.integers(0, W - tiles[:, 3] + 1), rng.integers(0, H - tiles[:, 4] + 1)
    centres = rng.uniform(0.3, 0.7, (m, 4, 2)) * (W, H)
    sizes = rng.uniform(8, 30, (m, 4, 2))
    tile = np.repeat(np.arange(n), P)
    frame, which = tiles[tile, 0], rng.integers(0, 4, R)
    mid = centres[frame, which] + rng.normal(0, 1.5, (R, 2))
    half = sizes[frame, which] / 2 * rng.uniform(0.85, 1.15, (R, 2))
    rec = np.zeros((R, 7), np.float32)
    rec[:, 0] = np.tile(np.arange(P), n)
    rec[:, 1] = (which + rng.integers(0, 2, R)) % labels
    rec[:, 2] = rng.uniform(0, 1, R)
    rec[:, 3] = (mid[:, 0] - half[:, 0] - tiles[tile, 1]) / tiles[tile, 3]
    rec[:, 4] = (mid[:, 1] - half[:, 1] - tiles[tile, 2]) / tiles[tile, 4]
    rec[:, 5] = (mid[:, 0] + half[:, 0] - tiles[tile, 1]) / tiles[tile, 3]
    rec[:, 6] = (mid[:, 1] + half[:, 1] - tiles[tile, 2]) / tiles[tile, 4]
    if specials and P > 1:
        k = rng.integers(0, 24, R)
        rec[k == 0, 2] = NAN
        rec[k == 1, 3 + rng.integers(0, 4)] = INF
        rec[k == 2, 3 + rng.integers(0, 4)] = -INF
        rec[k == 3, 3 + rng.integers(0, 4)] = NAN
        rec[k == 4, 5] = rec[k == 4, 3]                        # no width
        rec[k == 5, 2] = 0.5                                   # equal scores, and score == min_confidence
        rec[k == 6, 2] = -0.0
        rec[k == 7, 2] = 0.0
        rec[k == 8, 2] = INF
        rec[k == 9, 1] = NAN                                   # a label that becomes -1
        for b in range(n):
            end = int(rng.integers(0, P + 1 + P // 2))        # (past the tile: a full list)
            if end < P:
                rec[b * P + end] = END
                rec[b * P + end, 0] = NAN if rng.integers(0, 4) == 0 else -1
    return rec, tiles


CPU_SHAPES = [(1, 1, 1), (3, 65, 2), (16, 100, 1), (130, 2, 7)]


@pytest.mark.parametrize('n,P,m', CPU_SHAPES)
def test_numpy_form_equals_the_rule_on_clustered_records(n, P, m):
    """merge_tiles is tiles_ref on random clustered records.  The reference itself must suppress at least one candidate and keep at least
    two -- wherever the case has three records; (1, 1, 1) has one, which must be kept."""
    rng = np.random.default_rng(n * 4099 + P * 17 + m)
    rec, tiles = _clustered(rng, n, P, m)
    want = tiles_ref.merge(rec, tiles, m, min_confidence=0.1)
    print('selected {} counts {}'.format(want.selected.tolist(), want.counts.tolist()))
    if n * P >= 3:
        assert want.selected.sum() - want.counts.sum() >= 1 and want.counts.sum() >= 2
    else:
        assert want.selected.tolist() == want.counts.tolist() == [1]
    for opt in OPTIONS:
        _both(rec, tiles, m, **opt)


OPTIONS = [dict(min_confidence=0.1), dict(), dict(overlap='IOS'), dict(threshold=0.0), dict(threshold=1.0), dict(overlap='IOS', threshold=0.0),
           dict(overlap='IOS', threshold=1.0), dict(per_label=False), dict(per_label=False, overlap='IOS', threshold=0.3, min_confidence=-1.0),
           dict(labels=[1]), dict(labels=[2, 0], min_confidence=0.25), dict(labels=[]), dict(labels=list(range(6, 70))), dict(min_size=(14, 17)),
           dict(max_per_tile=1, min_confidence=-1.0), dict(max_per_frame=1), dict(max_per_frame=2, per_label=False),
           dict(max_per_tile=1, max_per_frame=2, threshold=0.2), dict(min_confidence=-1.0), dict(min_confidence=2.0)]


def test_consistent_with_the_plain_screen():
    """One tile per frame covering the whole frame, threshold 1.0 and no caps: the kept records are those detections_ref.compact keeps
    over the same extent, reordered by score within a frame."""
    rng = np.random.default_rng(31)
    m, P, extent = 5, 40, (96, 128)
    rec = det_tests._random_records(rng, m, P)
    tiles = roi_tests._whole(m, extent)
    for opt in (dict(), dict(labels=[5, 0, 3], min_confidence=0.25), dict(min_size=(20, 33)), dict(min_confidence=-1.0)):
        d = _both(rec, tiles, m, threshold=1.0, **opt)
        plain = detections_ref.compact(rec, m, extent, **opt)
        assert plain.counts.sum() >= 2 and np.array_equal(d.counts, plain.counts) and np.array_equal(d.selected, plain.selected)
        words = detections_ref.as_words(d).table
        at = 0
        for f in range(m):
            mine, theirs = words[at:at + d.counts[f]], plain.table[at:at + d.counts[f]]
            at += d.counts[f]
            assert np.array_equal(mine[np.argsort(mine[:, 7])], theirs)        # the same rows, word for word, in record order there
            scores = mine[:, 6].copy().view(np.float32)
            assert (np.diff(scores) <= 0).all()


def test_argument_rules():
    """Every refusal is a ValueError that starts with 'detections: ', raised before anything is staged or launched: this test runs where
    there is no device.  DetectionScreen values behave as before."""
    from pyopenvino_amd import DetectionScreen, DetectedRois, RoiInput, TiledScreen, detections, tiled_detections
    from pyopenvino_amd import device
    ie, net, name = _net('ssd_mobilenet_v1_coco', 4)
    det_tests._declare(net, name, 'U8-NHWC', reverse=True)
    ex = ie.load_network(net, 'GPU', num_requests=2)
    out_name = net.outputs[0]['name']
    assert tuple(net.outputs[0]['input'][0]['dims']) == (1, 1, 400, 7)
    frames = np.zeros((2, 48, 64, 3), np.uint8)
    roi = RoiInput(frames, np.array([(0, 0, 0, 40, 48), (1, 0, 0, 40, 48), (0, 24, 0, 40, 48), (1, 24, 0, 40, 48)], np.int32))
    req = ex.requests[0]

    def starts(x):
        return (lambda d: ex.infer({name: x}, detections=d), lambda d: ex.infer({name: x}, False, None, d),
                lambda d: req.start_async({name: x}, detections=d), lambda d: ex.requests[1].infer({name: x}, None, d),
                lambda d: ex.start_async(1, {name: x}, detections=d), lambda d: ex.start_async(0, {name: x}, None, d))

    def refused(match, d, x=roi, top_k=None):
        for start in starts(x) if top_k is None else (lambda d: req.start_async({name: x}, top_k, d), lambda d: ex.infer({name: x}, False, top_k, d)):
            with pytest.raises(ValueError, match=match) as e:
                start(d)
            assert str(e.value).startswith('detections: '), str(e.value)
        for r in ex.requests:
            assert not r._in_flight and not r._asks and not r.runner.answers.blocks
            assert not r.runner.host_inputs.slots and r.runner._pending is None

    def each_form(match, **opt):
        refused(match, TiledScreen(**opt))
        refused(match, {out_name: TiledScreen(**opt)})

    # the named input is fed anything but a RoiInput
    for x in (DetectedRois(frames, np.zeros((2, 7), np.float32)), np.zeros((4, 48, 64, 3), np.uint8), np.zeros((4, 3, 300, 300), np.float32),
              types.SimpleNamespace(frames=frames, rois=roi.rois)):
        refused('fed a RoiInput', TiledScreen(), x)
        refused('fed a RoiInput', {out_name: TiledScreen(input=name)}, x)
    tensor = object.__new__(device.DeviceTensor)              # (no device here: the type alone decides)
    refused('fed a RoiInput', TiledScreen(), tensor)
    for bad in ('nope', 3, out_name):
        each_form('no 4-D Parameter', input=bad)
    # the screen's values
    for bad in ('iou', 'GIOU', None, 0, b'IOU', ('IOU',)):
        each_form("overlap is 'IOU' or 'IOS'", overlap=bad)
    for bad in (NAN, INF, -INF, -0.001, 1.001, 2, '0.5', True, None, [0.5]):
        each_form('threshold', threshold=bad)
    for bad in (0, 1, None, 'yes', 1.0):
        each_form('per_label is a bool', per_label=bad)
    for key in ('max_per_tile', 'max_per_frame'):
        for bad in (0, -1, 1.5, True, '3', 2 ** 31):
            each_form(key + ' is None or a count', **{key: bad})
    for bad in (NAN, INF, '0.5', True, [0.5]):
        each_form('min_confidence', min_confidence=bad)
    for bad in (list(range(65)), [1.0], 'abc', 3, [True], [2 ** 31]):
        each_form('at most 64 ints', labels=bad)
    for bad in ((0, 1), (1, 0), 1, (1, 1, 1), (1.0, 1)):
        each_form('min_size', min_size=bad)
    # what detections= refuses today
    refused('no Result named', {'nope': TiledScreen()})
    ex.comm = types.SimpleNamespace(world=2, rank=0)
    try:
        refused('sharded', TiledScreen())
        refused('sharded', {out_name: TiledScreen()})
    finally:
        ex.comm = None
    ports = [r.runner.ienet.outputs[0]['input'][0] for r in ex.requests]
    for port in ports:
        port['precision'] = 'FP16'
    try:
        refused('FP32 Results only', {out_name: TiledScreen()})
        refused('no FP32 Result of shape', TiledScreen())
    finally:
        for port in ports:
            port['precision'] = 'FP32'
    declared = [port['dims'] for port in ports]
    for port in ports:
        port['dims'] = (1, 1, 401, 7)
    try:
        refused(r'not \(1, 1, R, 7\)', {out_name: TiledScreen()})
        refused('no FP32 Result of shape', TiledScreen())
    finally:
        for port, dims in zip(ports, declared):
            port['dims'] = dims
    refused('asked for with top_k as well', {out_name: TiledScreen()}, top_k={out_name: 1})
    # the candidate capacity: n * min(P, max_per_tile) <= 4096
    assert tiled_detections.resolved(TiledScreen(), 4, 100).max_per_tile == 100 and tiled_detections.resolved(TiledScreen(), 64, 100).max_per_tile == 64
    assert tiled_detections.resolved(TiledScreen(max_per_tile=5000), 4, 100).max_per_tile == 100
    assert tiled_detections.resolved(TiledScreen(), 4096, 7).max_per_tile == 1
    assert tiled_detections.resolved(TiledScreen(max_per_tile=64), 64, 100).max_per_frame == 4096
    for n, P, cap in ((64, 100, 65), (64, 100, 100), (4097, 1, None), (4097, 100, 1), (41, 100, 100)):
        with pytest.raises(ValueError, match='^detections: .*(lower max_per_tile|more than the 4096)'):
            tiled_detections.resolved(TiledScreen(max_per_tile=cap), n, P)
    big = [r.runner.ienet for r in ex.requests]
    for twin, port in zip(big, ports):
        twin.batch_size, port['dims'] = 64, (1, 1, 6400, 7)
    try:
        refused('lower max_per_tile to 64', TiledScreen(max_per_tile=65))
        refused('lower max_per_tile to 64', {out_name: TiledScreen(max_per_tile=100)})
    finally:
        for twin, port, dims in zip(big, ports, declared):
            twin.batch_size, port['dims'] = 4, dims
    # what is accepted, in its one form: equal screens are equal keys
    want = TiledScreen(0.5, None, (1, 1), 100, 'IOU', 0.45, True, 400, name)
    assert detections.checked(net, TiledScreen(), False) == {out_name: want}
    assert detections.checked(net, {out_name: TiledScreen(input=name)}, False) == {out_name: want}
    got = detections.checked(net, TiledScreen(1, np.array([3, 1]), [2, 3], 1000, 'IOS', 1, np.True_, 7), False)[out_name]
    assert got == TiledScreen(1.0, (3, 1), (2, 3), 100, 'IOS', 1.0, True, 7, name) and hash(got) == hash(got._replace())
    assert isinstance(got.threshold, float) and isinstance(got.per_label, bool)
    assert TiledScreen() == TiledScreen(0.5, None, (1, 1), None, 'IOU', 0.45, True, None, None) and TiledScreen()._fields == (
        'min_confidence', 'labels', 'min_size', 'max_per_tile', 'overlap', 'threshold', 'per_label', 'max_per_frame', 'input')
    with pytest.raises(AttributeError):
        want.threshold = 0.1                                   # immutable
    # DetectionScreen is what it was
    assert DetectionScreen._fields == ('min_confidence', 'frame_size', 'labels', 'min_size', 'max_per_image')
    plain = DetectionScreen(0.5, (300, 300), None, (1, 1), 100)
    assert detections.checked(net, 0.5, False) == detections.checked(net, DetectionScreen(), False) == {out_name: plain}
    assert detections.checked(net, None, False) == {} and not isinstance(TiledScreen(), DetectionScreen)
    with pytest.raises(ValueError, match='^detections: .*max_per_image'):
        detections.checked(net, DetectionScreen(max_per_image=0), False)


def test_abi_declares_the_entry():
    import pyopenvino_amd
    from pyopenvino_amd import device, tiled_detections
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert ENTRY in device.SIGNATURES and len(device.SIGNATURES[ENTRY][1]) == ARGS and ENTRY not in device._NOT_STATUS
    m = re.search(r'\bint\s+' + ENTRY + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S)
    assert m and len(m.group(1).split(',')) == ARGS
    comment = re.search(r'/\*((?:(?!\*/).)*)\*/\s*(?:#define[^\n]*\n)*int\s+' + ENTRY, header, flags=re.S).group(1)
    for phrase in ('Addition to ABI v18 (the version number is unchanged', '(double)inter > (double)threshold * (double)den', 'Equality does not suppress',
                   '(f, x0, y0, w, h, label, score bits, record)', 'counts[m], then selected[m], then total', 'tests/tiles_ref.py',
                   '<= 4096 (the candidate capacity)'):
        assert phrase in comment, phrase                       # the rule is stated there
    for kind, value in tiled_detections.OVERLAPS.items():
        assert re.search(r'#define\s+PVHIP_OVERLAP_{}\s+{}\b'.format(kind, value), header)
    assert re.search(r'#define\s+PVHIP_ABI_VERSION\s+19\b', header)
    lib = device.load_library()
    assert hasattr(lib, ENTRY) and lib.pvhip_abi_version() == 19
    assert pyopenvino_amd.TiledScreen is tiled_detections.TiledScreen and 'TiledScreen' in pyopenvino_amd.__all__
    makefile = open(os.path.join(helpers.REPO, 'pyopenvino_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=[^\n]*(\\\n[^\n]*)*pvhip_tiles\.hip', makefile, flags=re.M)


# ---------------------------------------------------------------------------------------------------------------- GPU
SENTINEL = 0x7f7f7f7f


def _device_merge(hip, rec, tiles, m, min_confidence=0.5, labels=None, min_size=(1, 1), max_per_tile=None, overlap='IOU', threshold=0.45,
                  per_label=True, max_per_frame=None):
    """The entry on `rec` and `tiles`: header and rows prefilled with 0x7f bytes, each with guard words behind it, as a Compacted; nothing
    from `total` onward may be written."""
    n = tiles.shape[0]
    P = rec.reshape(-1, 7).shape[0] // n
    per_tile = min(P, 4096 // n) if max_per_tile is None else min(P, max_per_tile)
    slots = n * per_tile
    per_frame = slots if max_per_frame is None else min(max_per_frame, slots)
    capacity = min(slots, m * per_frame)
    src = hip.DeviceTensor.from_numpy(rec)
    table = hip.DeviceTensor.from_numpy(np.ascontiguousarray(tiles, np.int32))
    header = hip.DeviceTensor.empty((2 * m + 1 + 8,), np.int32)
    rows = hip.DeviceTensor.empty((capacity + 1, 8), np.int32)
    scratch = hip.DeviceTensor.empty((9 * slots + n,), np.int32)
    for t in (header, rows, scratch):
        hip.call('pvhip_memset', ctypes.c_void_p(t.ptr), 0x7f, t.nbytes)
    lab = hip.DeviceTensor.from_numpy(np.asarray(list(labels) + [0], np.int32)) if labels is not None else None      # ([]: no label passes)
    hip.call(ENTRY, ctypes.c_void_p(src.ptr), ctypes.c_void_p(table.ptr), n, P, m, min_confidence,
             ctypes.c_void_p(lab.ptr) if lab is not None else None, 0 if labels is None else len(labels), min_size[0], min_size[1], per_tile,
             {'IOU': 0, 'IOS': 1}[overlap], threshold, int(per_label), per_frame, ctypes.c_void_p(scratch.ptr), ctypes.c_void_p(header.ptr),
             ctypes.c_void_p(rows.ptr))
    header, rows = np.asarray(header), np.asarray(rows).view(np.uint32)
    assert (header[2 * m + 1:] == SENTINEL).all(), 'a word behind the header was written'
    counts, selected, total = header[:m].copy(), header[m:2 * m].copy(), int(header[2 * m])
    assert 0 <= total <= capacity and total == counts.sum(), (total, capacity, counts.sum())
    assert (rows[total:] == SENTINEL).all(), 'a row from total onward was written'
    return detections_ref.Compacted(counts, selected, rows[:total].copy())


def _check(hip, rec, tiles, m, what, **opt):
    want = tiles_ref.merge(rec, tiles, m, **opt)
    _equal(_device_merge(hip, rec, tiles, m, **opt), want, '{} {}'.format(what, opt))
    return want


# one record; a tile around the chunk of 64 records; frames interleaved over the tiles; 1600 candidates of one frame (two sorted places a
# lane, 25 chunks); tiles not a multiple of the four waves of a workgroup over more frames; 4059 and exactly 4096 candidates
GPU_SHAPES = [(1, 1, 1, None), (1, 65, 1, None), (3, 65, 2, None), (16, 100, 1, None), (130, 2, 7, None), (41, 100, 3, 99), (64, 64, 1, None)]


@pytest.mark.gpu
@pytest.mark.parametrize('n,P,m,per_tile', GPU_SHAPES)
def test_kernel_equals_the_rule(hip, n, P, m, per_tile):
    rng = np.random.default_rng(n * 4099 + P * 17 + m)
    rec, tiles = _clustered(rng, n, P, m)
    if (n, P, m) == (3, 65, 2):
        tiles[:, 0] = (0, 1, 0)
    cap = dict() if per_tile is None else dict(max_per_tile=per_tile)
    want = _check(hip, rec, tiles, m, 'clustered', min_confidence=0.1, **cap)
    if n * P >= 3:
        assert want.selected.sum() - want.counts.sum() >= 1 and want.counts.sum() >= 2
    for opt in OPTIONS[1:]:
        _check(hip, rec, tiles, m, 'clustered', **{**cap, **opt})
    # every record a candidate: n * per_tile of them
    full, full_tiles = _clustered(rng, n, P, m, specials=False, whole=True)
    want = _check(hip, full, full_tiles, m, 'full', min_confidence=-1.0, **cap)
    assert want.selected.sum() == n * min(P, per_tile or 4096 // n)
    for opt in (dict(per_label=False, threshold=0.6), dict(overlap='IOS', threshold=0.9, max_per_frame=2), dict(threshold=1.0)):
        _check(hip, full, full_tiles, m, 'full', min_confidence=-1.0, **{**cap, **opt})
    # tiles with ids outside [0, m), tiles without an extent, a table whose sums wrap
    odd = tiles.copy()
    odd[::3, 0], odd[1::5, 0], odd[2::7, 3], odd[3::11, 4] = -1, m, 0, -5
    odd[n // 2, 1:3] = (2 ** 31 - 1, -2 ** 31)
    for opt in (dict(min_confidence=0.1), dict(per_label=False, max_per_frame=2)):
        _check(hip, rec, odd, m, 'odd tiles', **{**cap, **opt})
    # every tile dead
    dead = rec.copy()
    dead[::P] = END
    got = _device_merge(hip, dead, tiles, m, min_confidence=-1.0, **cap)
    _equal(got, tiles_ref.merge(dead, tiles, m, min_confidence=-1.0, **cap), 'every tile dead')
    assert not got.counts.any() and not got.selected.any() and got.table.shape == (0, 8)


@pytest.mark.gpu
def test_the_two_extremes_at_4096_candidates(hip):
    """64 tiles of 64 records over one (512, 512) frame, every record a candidate.  All boxes disjoint: everything is kept (64 chunks, each
    tested against all the kept ones before it).  All boxes identical: one is kept per label, the best score's lowest record."""
    rng = np.random.default_rng(4096)
    n, P = 64, 64
    tiles = roi_tests._whole(n, (512, 512), ids=[0] * n)
    cell = np.arange(n * P)
    rec = np.zeros((n * P, 7), np.float32)
    rec[:, 0] = np.tile(np.arange(P), n)
    rec[:, 1] = rng.integers(0, 3, n * P)
    rec[:, 2] = rng.integers(1, 200, n * P) / 256              # many equal scores
    rec[:, 3], rec[:, 4] = (cell % 64) / 64, (cell // 64) / 64
    rec[:, 5], rec[:, 6] = rec[:, 3] + 1 / 64, rec[:, 4] + 1 / 64
    for opt in (dict(threshold=0.0, per_label=False), dict(overlap='IOS')):
        want = _check(hip, rec, tiles, 1, 'disjoint', min_confidence=0.0, **opt)
        assert want.counts.tolist() == want.selected.tolist() == [4096]
    want = _check(hip, rec, tiles, 1, 'disjoint', min_confidence=0.0, max_per_frame=4095)
    assert want.counts.tolist() == [4095] and want.selected.tolist() == [4096]
    rec[:, 3:5], rec[:, 5:7] = 0.25, 0.5
    want = _check(hip, rec, tiles, 1, 'identical', min_confidence=0.0)
    assert want.counts.tolist() == [3] and want.selected.tolist() == [4096]
    for label in range(3):
        mine = np.flatnonzero(rec[:, 1] == label)
        assert int(want.table[:, 7][want.table[:, 5] == label][0]) == mine[np.argmax(rec[mine, 2])]
    want = _check(hip, rec, tiles, 1, 'identical', min_confidence=0.0, per_label=False, overlap='IOS', threshold=0.99)
    assert want.counts.tolist() == [1]
    want = _check(hip, rec, tiles, 1, 'identical', min_confidence=0.0, threshold=1.0, max_per_frame=70)       # nothing suppressed, capped
    assert want.counts.tolist() == [70]


@pytest.mark.gpu
def test_entry_rejects_what_it_cannot_do(hip):
    rng = np.random.default_rng(5)
    rec, tiles = _clustered(rng, 4, 8, 2)
    src = hip.DeviceTensor.from_numpy(rec)
    table = hip.DeviceTensor.from_numpy(tiles)
    out = hip.DeviceTensor.empty((8 * 32 + 16,), np.int32)
    scratch = hip.DeviceTensor.empty((9 * 32 + 4 + 4,), np.int32)
    lab = hip.DeviceTensor.from_numpy(np.arange(64, dtype=np.int32))
    p = ctypes.c_void_p
    good = [p(src.ptr), p(table.ptr), 4, 8, 2, 0.5, None, 0, 1, 1, 8, 0, 0.45, 1, 32, p(scratch.ptr), p(out.ptr + 1024), p(out.ptr)]
    assert len(good) == ARGS
    hip.call(ENTRY, *good)
    hip.call(ENTRY, *(good[:6] + [p(lab.ptr), 64] + good[8:]))
    for k, bad in ((0, None), (1, None), (15, None), (16, None), (17, None), (17, p(out.ptr + 4)), (17, p(out.ptr + 8)), (15, p(scratch.ptr + 4)),
                   (15, p(scratch.ptr + 8)), (2, 0), (2, -1), (3, 0), (4, 0), (4, -1), (8, 0), (9, 0), (10, 0), (10, -1), (14, 0), (14, -1),
                   (7, 65), (7, -1), (7, 1), (10, 1025), (2, 4097), (11, 2), (11, -1), (12, NAN), (12, -0.001), (12, 1.001), (12, INF),
                   (13, 2), (13, -1), (3, 2 ** 31 // 28 + 1), (3, 2 ** 31 // 7)):
        args = list(good)
        args[k] = bad
        with pytest.raises(hip.PvhipError):
            hip.call(ENTRY, *args)
    with pytest.raises(hip.PvhipError):
        hip.call(ENTRY, *(good[:6] + [p(lab.ptr), 65] + good[8:]))
    hip.synchronize()
    _check(hip, rec, tiles, 2, 'after the refusals', min_confidence=0.1)      # the device is still usable


_detector, _median_live_score, _bits = det_tests._detector, det_tests._median_live_score, plain_tests._bits
TILES = np.array([(0, 0, 0, 400, 480), (1, 0, 0, 400, 480), (0, 240, 0, 400, 480), (1, 240, 0, 400, 480)], np.int32)


@pytest.mark.gpu
def test_public_path_on_ssd_mobilenet(hip):
    """SSD-MobileNet at batch 4 on two U8 / NHWC (480, 640) frames cut into two overlapping tiles each: five passes of one request on
    the same RoiInput with the keyword alternating -- none, tiled, a plain DetectionScreen, tiled, none --, replayed from the request's
    one recording from the third on; detections=TiledScreen(...) is the rule on the same request's own full Result, through the request,
    the network's infer() and the dict form; the table it returns is a RoiInput's."""
    from pyopenvino_amd import DetectionScreen, Detections, RoiInput, TiledScreen
    rng = np.random.default_rng(93)
    m, n, hw = 2, 4, (480, 640)
    frames = _frames(rng, 'U8-NHWC', m, hw)
    det, name, out_name = _detector(n)
    req = det.requests[0]
    feed = RoiInput(frames, TILES)
    results, kinds = [], [None, 'tiled', 'plain', 'tiled', None]
    conf = None
    for call, kind in enumerate(kinds):
        req.start_async({name: feed}, detections={'tiled': TiledScreen(conf), 'plain': DetectionScreen(conf), None: None}[kind] if call else None)
        assert (req._replayed is not None) == (call >= 2), 'call {}'.format(call)
        results.append(req.wait()[out_name])
        if call == 0:
            full = np.array(results[0], copy=True)
            assert full.shape == (1, 1, 400, 7) and full.dtype == np.float32
            conf = _median_live_score(full, n)
    assert det._auto_graph['captured'] and det._graph is not None             # one recording served every kind
    want = tiles_ref.merge(full, TILES, m, min_confidence=conf)
    print('conf {:.4f} selected {} counts {}'.format(conf, want.selected.tolist(), want.counts.tolist()))
    assert want.counts.sum() >= 1 and want.selected.sum() < 400
    assert isinstance(results[1], Detections)
    _same(results[1], want, 'call 1')
    _same(results[3], want, 'call 3')
    _same(results[2], detections_ref.compact(full, n, (300, 300), min_confidence=conf), 'call 2: a plain screen sees four images')
    assert isinstance(results[4], np.ndarray) and np.array_equal(_bits(results[4]), _bits(full))     # whole and bit-equal without the keyword
    assert (results[1].records // 100 < n).all() and (TILES[results[1].records // 100, 0] == results[1].rois[:, 0]).all()
    # the network's own infer() and the dict form; other options
    _same(det.infer({name: feed}, detections=TiledScreen(conf))[out_name], want, 'the network\'s own infer()')
    _same(det.infer({name: feed}, False, None, {out_name: TiledScreen(conf, input=name)})[out_name], want, 'positional, the dict form')
    opt = dict(min_confidence=0.0, overlap='IOS', threshold=0.3, per_label=False, max_per_tile=30, max_per_frame=5)
    want_cut = tiles_ref.merge(full, TILES, m, **opt)
    print('cut: selected {} counts {}'.format(want_cut.selected.tolist(), want_cut.counts.tolist()))
    assert (want_cut.selected > want_cut.counts).any()
    _same(req.infer({name: feed}, detections=TiledScreen(**opt))[out_name], want_cut, 'IOS, caps')
    whole = req.infer({name: feed})[out_name]
    assert isinstance(whole, np.ndarray) and np.array_equal(_bits(whole), _bits(full))
    # the answer feeds a RoiInput over the same frames (a classifier's batch of n rows: padded as the cascade's host route pads)
    d = results[1]
    table = np.concatenate([d.rois, np.tile(np.array([(0, 0, 0, 1, 1)], np.int32), (n, 1))])[:n]
    checked, largest = det.host_inputs.formats[name].checked_rois(table, hw, m)
    assert np.array_equal(checked, table) and largest[0] <= hw[0] and largest[1] <= hw[1]
    # the request's own blocks, one per (name, screen, m)
    keys = sorted((k for k in det.answers.blocks if len(k) == 3), key=repr)
    assert len(keys) == 2 and {(k[0], k[2]) for k in keys} == {(out_name, m)}
    assert {(k[1].min_confidence, k[1].max_per_tile, k[1].max_per_frame, k[1].input) for k in keys} == {(conf, 100, 400, name), (0.0, 30, 5, name)}
    # (no key of another kind but call 2's plain screen)
    assert [k for k in det.answers.blocks if len(k) != 3] == [(out_name, DetectionScreen(conf, (300, 300), None, (1, 1), 100))]
    assert all(type(k[1]) is TiledScreen for k in keys)
    det.release_device_state()
    assert not det.answers.blocks


@pytest.mark.gpu
def test_two_requests_in_flight_with_different_tile_tables(hip):
    """Two requests at batch 4, each on its own frames and its own tile table, both started and then both waited for: each answer is the
    rule on its own Result and its own table."""
    from pyopenvino_amd import RoiInput, TiledScreen
    rng = np.random.default_rng(94)
    m, n, hw = 2, 4, (240, 320)
    det, name, out_name = _detector(n, requests=2)
    frames = [_frames(rng, 'U8-NHWC', m, hw) for _ in range(2)]
    tables = [np.array([(0, 0, 0, 200, 240), (0, 120, 0, 200, 240), (1, 0, 0, 200, 240), (1, 120, 0, 200, 240)], np.int32),
              np.array([(1, 0, 0, 320, 150), (0, 0, 0, 320, 150), (1, 0, 90, 320, 150), (0, 0, 90, 320, 150)], np.int32)]
    feeds = [RoiInput(frames[r], tables[r]) for r in range(2)]
    fulls = [np.array(det.requests[r].infer({name: feeds[r]})[out_name], copy=True) for r in range(2)]
    assert not np.array_equal(fulls[0], fulls[1])
    confs = [_median_live_score(f, n) for f in fulls]
    wants = [tiles_ref.merge(fulls[r], tables[r], m, min_confidence=confs[r]) for r in range(2)]
    for step, asked in enumerate(((True, True), (True, False), (False, True), (True, True))):
        for r in range(2):
            det.start_async(r, {name: feeds[r]}, detections=TiledScreen(confs[r]) if asked[r] else None)
        for r in (1, 0) if step % 2 else (0, 1):
            res = det.wait(r)[out_name]
            if asked[r]:
                _same(res, wants[r], 'step {} request {}'.format(step, r))
            else:
                assert isinstance(res, np.ndarray) and np.array_equal(_bits(res), _bits(fulls[r])), 'step {} request {}'.format(step, r)
