"""The stage behind the pass (pyopenvino_amd/answers.py): one ``Answers`` per request checks ``top_k=`` and ``detections=``, binds the
asks to the staged inputs, launches behind the pass and reads after it, whatever the kind.  The rules themselves are tested where they
are stated (test_top_k.py, test_detections.py, test_tiled_detections.py); the first tests here need no GPU."""
import types
import warnings

import numpy as np
import pytest

import detections_ref
import test_detected_rois as det_tests
import test_detections as plain_tests
import test_tiled_detections as tiled_tests
import test_top_k as top_k_tests
import tiles_ref
import topk_ref

_net, _same = tiled_tests._net, plain_tests._same
TABLE = np.array([(0, 0, 0, 40, 48), (1, 0, 0, 40, 48), (0, 24, 0, 40, 48), (1, 24, 0, 40, 48)], np.int32)     # 4 tiles of 2 (48, 64) frames


def _ssd(batch=4, requests=1):
    """The SSD IR at `batch` as test_tiled_detections.test_argument_rules loads it: (network, input name, Result name)."""
    ie, net, name = _net('ssd_mobilenet_v1_coco', batch)
    det_tests._declare(net, name, 'U8-NHWC', reverse=True)
    return ie.load_network(net, 'GPU', num_requests=requests), name, net.outputs[0]['name']


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
def test_the_stage_on_host_values():
    """checked(), bound(), launch() and read() on Results that are host arrays: the answer is the rule in numpy, nothing is recorded and
    no block is made -- there is no device here."""
    from pyopenvino_amd import DetectionScreen, RoiInput, TiledScreen, detections, tiled_detections, top_k
    rng = np.random.default_rng(401)
    ex, name, out_name = _ssd()
    answers = ex.requests[0].runner.answers
    assert answers is ex.answers and answers.checked({name: None}, None, None, False) == {}
    rec = det_tests._random_records(rng, 4, 100).reshape(1, 1, 400, 7)
    opt = dict(min_confidence=0.25, labels=[5, 0, 3])
    # a plain screen
    x = np.zeros((4, 300, 300, 3), np.uint8)
    asks = answers.checked({name: x}, None, DetectionScreen(**opt), False)
    assert list(asks) == [out_name] and type(asks[out_name]) is detections.Ask
    assert asks[out_name] == (DetectionScreen(0.25, (300, 300), (5, 0, 3), (1, 1), 100), 4)
    assert answers.bound(asks, {name: x}) == asks
    want = detections_ref.compact(rec, 4, (300, 300), **opt)
    assert want.counts.sum() >= 2
    _same(answers.read(out_name, asks[out_name], rec), want, 'plain')
    answers.launch(asks, {out_name: rec})
    assert ex._pending is None and answers.blocks == {}
    # a TiledScreen over a RoiInput of 2 frames and 4 tiles: the slot's page-locked table, which stage() fills on a device, by hand
    roi = RoiInput(np.zeros((2, 48, 64, 3), np.uint8), TABLE)
    opt = dict(opt, threshold=0.1, per_label=False)            # (so that the random boxes suppress each other)
    asks = answers.checked({name: roi}, None, {out_name: TiledScreen(**opt)}, False)
    assert type(asks[out_name]) is tiled_detections.Ask and asks[out_name].frames is None and asks[out_name].tiles == 4
    ex.host_inputs.slots[name] = types.SimpleNamespace(tables={'roi': types.SimpleNamespace(host=TABLE.copy(), device=None)})
    try:
        asks = answers.bound(asks, {name: roi})
        assert asks[out_name].frames == 2 and asks[out_name].key(out_name) == (out_name, asks[out_name].screen, 2)
        assert asks[out_name].screen == TiledScreen(0.25, (5, 0, 3), (1, 1), 100, 'IOU', 0.1, False, 400, name)
        want = tiles_ref.merge(rec, TABLE, 2, **opt)
        assert want.counts.sum() >= 2 and want.selected.sum() > want.counts.sum()
        _same(answers.read(out_name, asks[out_name], rec), want, 'tiled')
        answers.launch(asks, {out_name: rec})
        assert ex._pending is None and answers.blocks == {}
    finally:
        ex.host_inputs.release()
    # top_k on GoogLeNet's rows
    ie, net, name = top_k_tests._net(batch=4)
    ex = ie.load_network(net, 'GPU')
    out_name = net.outputs[0]['name']
    rows = rng.normal(0, 1, (4, 1000)).astype(np.float32)
    rows[1, 7], rows[2, 10:13] = np.nan, rows[2, 500]          # a NaN, a tie
    asks = ex.answers.checked({name: None}, 5, None, False)
    assert asks == {out_name: top_k.Ask(5)} and ex.answers.bound(asks, {name: None}) == asks
    top_k_tests._same(ex.answers.read(out_name, asks[out_name], rows), topk_ref.top_k(rows, 5), 'top_k')
    ex.answers.launch(asks, {out_name: rows})
    assert ex._pending is None and ex.answers.blocks == {}


def test_the_first_of_two_refusals_is_the_one_raised():
    """A call that is wrong in two ways: the checks run in one order -- the tiled screen / top_k clash, top_k's, detections', the clash of
    a Result named in both, the RoiInput feed --, through checked() and through every start."""
    from pyopenvino_amd import RoiInput, TiledScreen
    ex, name, out_name = _ssd(requests=2)
    roi = RoiInput(np.zeros((2, 48, 64, 3), np.uint8), TABLE)
    x = np.zeros((4, 300, 300, 3), np.uint8)
    req = ex.requests[0]
    # a TiledScreen for a Result that top_k names as well, with k out of range: the clash, not top_k's refusal
    # a screen value out of range, fed an ndarray in the place of a RoiInput: the screen's refusal, not the feed's
    for match, feed, top_k, screen in (('asked for with top_k as well', roi, {out_name: 0}, {out_name: TiledScreen()}),
                                       ('threshold 2 is not a finite number', x, None, TiledScreen(threshold=2)),
                                       ('threshold 2 is not a finite number', x, None, {out_name: TiledScreen(threshold=2)})):
        for start in (lambda: req.runner.answers.checked({name: feed}, top_k, screen, False), lambda: req.start_async({name: feed}, top_k, screen),
                      lambda: ex.infer({name: feed}, False, top_k, screen), lambda: ex.requests[1].infer({name: feed}, top_k, screen)):
            with pytest.raises(ValueError, match=match) as e:
                start()
            assert str(e.value).startswith('detections: ') and 'fed a RoiInput' not in str(e.value) and 'top_k: ' not in str(e.value)
        for r in ex.requests:
            assert not r._in_flight and not r._asks and not r.runner.answers.blocks and not r.runner.host_inputs.slots and r.runner._pending is None
    # each of the two alone is refused as itself
    with pytest.raises(ValueError, match='^top_k: '):
        req.start_async({name: roi}, {out_name: 0})
    with pytest.raises(ValueError, match='fed a RoiInput'):
        req.start_async({name: x}, None, TiledScreen())


def test_the_shared_screen_on_its_edges():
    """One image of three records through both numpy rules, the tiled one with one tile that is the frame, threshold 1.0 and no caps: a
    corner whose product with the extent overflows float32, labels NaN and 2^31, the terminator.  The same rectangles and label words as
    the rules written again, and no numpy warning."""
    from pyopenvino_amd import DetectionScreen, TiledScreen, detections, tiled_detections
    H, W = 1080, 1920
    rec = np.array([det_tests._rec(0, np.nan, 0.9, 0.25, 0.25, 3e38, 0.5),
                    det_tests._rec(1, 2.0 ** 31, 0.8, 0.5, 0.5, 0.75, 0.75),
                    det_tests.END], np.float32)
    tile = np.array([(0, 0, 0, W, H)], np.int32)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        plain = detections.compact_records(rec, 1, DetectionScreen(frame_size=(H, W)))
        tiled = tiled_detections.merge_tiles(rec, tile, 1, TiledScreen(threshold=1.0))
        want_plain, want_tiled = detections_ref.compact(rec, 1, (H, W)), tiles_ref.merge(rec, tile, 1, threshold=1.0)
    _same(plain, want_plain, 'plain')
    _same(tiled, want_tiled, 'tiled')
    for d in (plain, tiled):
        assert d.counts.tolist() == d.selected.tolist() == [2] and d.records.tolist() == [0, 1] and d.labels.tolist() == [-1, -1]
        assert d.rois.tolist() == [[0, 480, 270, 1440, 270], [0, 960, 540, 480, 270]]
    assert np.array_equal(detections_ref.as_words(plain).table, detections_ref.as_words(tiled).table)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_one_request_asked_for_two_kinds_then_none(hip):
    """SSD-MobileNet at batch 4 on one RoiInput of two frames cut into four tiles, whose staged tensor is the same from pass to pass:
    five passes of one request asked for a TiledScreen, a DetectionScreen, nothing, the TiledScreen, nothing -- replayed from the
    request's one recording from the third on.  Each answer is its rule on the whole Result of the passes that asked for nothing; after
    every wait() nothing is pending; the request keeps one block per kind."""
    from pyopenvino_amd import DetectionScreen, RoiInput, TiledScreen
    rng = np.random.default_rng(95)
    m, n = 2, 4
    det, name, out_name = det_tests._detector(n)
    req = det.requests[0]
    feed = RoiInput(tiled_tests._frames(rng, 'U8-NHWC', m, (480, 640)), tiled_tests.TILES)
    opt = dict(min_confidence=0.0)
    results = []
    for call, screen in enumerate((TiledScreen(**opt), DetectionScreen(**opt), None, TiledScreen(**opt), None)):
        req.start_async({name: feed}, detections=screen)
        assert (req._replayed is not None) == (call >= 2), 'call {}'.format(call)
        assert set(req._asks) == (set() if screen is None else {out_name})
        results.append(req.wait()[out_name])
        assert det._pending is None and req._asks == {} and not req._in_flight
    full = results[2]
    assert isinstance(full, np.ndarray) and full.shape == (1, 1, 400, 7)
    assert np.array_equal(tiled_tests._bits(results[4]), tiled_tests._bits(full))
    want = tiles_ref.merge(full, tiled_tests.TILES, m, **opt)
    plain = detections_ref.compact(full, n, (300, 300), **opt)
    print('tiled: selected {} counts {}; plain: counts {}'.format(want.selected.tolist(), want.counts.tolist(), plain.counts.tolist()))
    assert want.counts.sum() >= 1 and plain.counts.sum() >= 1
    _same(results[0], want, 'call 0: tiled, eager')
    _same(results[3], want, 'call 3: tiled, replayed')
    _same(results[1], plain, 'call 1: plain')
    keys = sorted(det.answers.blocks, key=repr)
    assert keys == [(out_name, DetectionScreen(0.0, (300, 300), None, (1, 1), 100)),
                    (out_name, TiledScreen(0.0, None, (1, 1), 100, 'IOU', 0.45, True, 400, name), m)]
    det.release_device_state()
    assert det.answers.blocks == {}
