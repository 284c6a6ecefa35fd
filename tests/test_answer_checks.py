"""What ``Answers.checked`` makes of its four arguments, and what a pass asked for an answer hands to the runtime.  tests/golden/
answer_checks.json holds the outcome of every call of a matrix -- the asks, or the refusal's type and full text -- as it was before the
kinds of answer were put behind one Ask protocol (tests/golden/make_answer_checks.py recorded it, and owns the matrix).  On the GPU,
one test pins the calls a start makes behind the pass and the calls of wait(), for every kind of answer, eager and replayed."""
import importlib.util
import json
import os
import re
import tempfile

import numpy as np
import pytest

import test_detected_rois as det_tests
import test_gallery as gallery_tests
import test_keypoints as keypoints_tests
import test_tiled_detections as tiled_tests

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('make_answer_checks', os.path.join(GOLDEN, 'make_answer_checks.py'))
matrix = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(matrix)
CLASSES = {'top_k.Ask', 'detections.Ask', 'detections.FittedAsk', 'tiled_detections.Ask', 'tiled_detections.RegionAsk', 'gallery.Ask', 'keypoints.Ask'}
CLASH = re.compile(r'(\w+): Result .* is asked for with (\w+) as well$')


def _recorded():
    with open(os.path.join(GOLDEN, 'answer_checks.json')) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
def test_the_fixture_holds_exactly_the_matrix():
    recorded, keys = _recorded(), [case[0] for case in matrix.cases()]
    assert len(keys) == len(set(keys)) == 1129
    assert sorted(recorded) == sorted(keys)
    assert {ask[0] for outcome in recorded.values() for ask in outcome.get('asks', {}).values()} == CLASSES
    refusals = [outcome['error'] for outcome in recorded.values() if 'error' in outcome]
    assert {kind for kind, _ in refusals} == {'ValueError'}
    clashes = {CLASH.match(text).groups() for _, text in refusals if CLASH.match(text)}
    # the later keyword speaks and names the earlier one: every pair of the four
    assert clashes == {('detections', 'top_k'), ('matches', 'top_k'), ('matches', 'detections'), ('keypoints', 'top_k'), ('keypoints', 'detections'),
                       ('keypoints', 'matches')}
    assert {text.split(':')[0] for _, text in refusals} == set(matrix.KEYWORDS)


def test_checked_gives_the_recorded_outcome_for_every_case():
    recorded = _recorded()
    with tempfile.TemporaryDirectory() as tmp:
        nets, fed = matrix.networks(tmp), matrix.feeds()
        for case in matrix.cases():
            got = json.loads(json.dumps(matrix.outcome(nets, fed, case)))
            assert got == recorded[case[0]], (case[0], got, recorded[case[0]])
        for ex, _, _ in nets.values():              # nothing was staged, allocated or left pending
            assert not ex.answers.blocks and not ex.host_inputs.slots and ex._pending is None
    assert all(gallery._dev is None for gallery in matrix.GALLERIES)


# ---------------------------------------------------------------------------------------------------------------- GPU
SELECT, RECORD, D2H, REPLAY = 'pvhip_stream_select', 'pvhip_event_record', 'pvhip_memcpy_d2h', 'pvhip_graph_launch'
# what makes blocks, events and the pool's epochs on a first use is no part of the order
ALLOCATIONS = ('pvhip_malloc', 'pvhip_host_alloc')
ASIDE = ('pvhip_malloc', 'pvhip_host_alloc', 'pvhip_event_create', 'pvhip_event_create_untimed', 'pvhip_pool_epoch_begin', 'pvhip_pool_epoch_dispatched',
         'pvhip_pool_epoch_end')


def _passes(hip, req, feed, asked, entries, copies, first_use=()):
    """Three passes of `req` on `feed` asked for `asked` = {keyword: value}, the third replayed from the request's recording in that start: behind the
    pass and the event that ends it each start selects the base stream, calls `entries` once each, records one event and selects stream 0 again -- with
    `first_use` in front of the entries in the first pass --, and wait() waits for that event and makes `copies`[i] copies on the base
    stream for the i-th answer.  The answers of the three passes, which are the same bit for bit."""
    real_call, answers = hip.call, []
    for call in range(3):
        issued = []
        hip.call = lambda entry, *args: (issued.append(entry), real_call(entry, *args))[1]
        try:
            req.start_async(feed, **asked)
            started, behind_pass = [e for e in issued if e not in ASIDE], issued[issued.index(entries[0]):]
            del issued[:]
            req_replayed = req._replayed is not None
            answers.append(req.wait())
            waited, in_wait = [e for e in issued if e not in ASIDE], list(issued)
        finally:
            hip.call = real_call
        what = (asked, 'pass', call, started[-12:], waited)
        print(what)
        assert req_replayed == (call == 2), what
        behind = [SELECT] + (list(first_use) if call == 0 else []) + list(entries) + [RECORD, SELECT]
        assert all(started.count(e) == 1 for e in entries) and started.count(REPLAY) == (call == 2), what
        if call == 2:                               # the replay (recorded in this start), its event, then the answers' own
            assert started[started.index(REPLAY):] == [REPLAY, RECORD, SELECT] + behind, what
        else:                                       # the eager pass ends with its event
            assert started[-len(behind) - 1:] == [RECORD] + behind, what
        if call:                                    # the blocks of the first pass serve the later ones: nothing is allocated behind the pass or in wait()
            assert not set(ALLOCATIONS) & set(behind_pass + in_wait), what + (behind_pass, in_wait)
        assert waited == ['pvhip_event_sync'] + [e for count in copies for e in [SELECT] + [D2H] * count + [SELECT]], what
    return answers


def _same_answers(answers, name):
    first = answers[0][name]
    for other in answers[1:]:
        for a, b in zip(first, other[name]):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    return first


@pytest.mark.gpu
def test_a_start_issues_its_answers_in_one_order(hip, tmp_path):
    """One request per kind of answer, three passes each on an input that stays on the device: mnist at batch 2 for top_k and for
    matches on a gallery of 3 rows and one of 257 (past CHUNK), mnist's first Convolution as a heatmap network for keypoints, the SSD IR
    at batch 4 on a RoiInput for a plain screen, one that selects nothing and a tiled one.  A flat answer is one launch (matches: one
    entry call) and one copy; a table one entry call and two copies, one when its total is 0."""
    from pyopenvino_amd import DetectionScreen, Gallery, RoiInput, TiledScreen, synth
    rng = np.random.default_rng(77)
    n = 2
    x = hip.DeviceTensor.from_numpy(np.concatenate([synth.uniform_pixels(20 + i, (1, 1, 28, 28)) for i in range(n)], 0))
    ex, name, out_name = gallery_tests._mnist(n)
    top = _same_answers(_passes(hip, ex.requests[0], {name: x}, dict(top_k=3), ['pvhip_topk_rows_f32'], [1]), out_name)
    assert top.indices.shape == (n, 3)
    for rows in (3, gallery_tests.C + 1):
        ex, name, out_name = gallery_tests._mnist(n)
        gal = Gallery(rng.standard_normal((rows, 10)).astype(np.float32))
        got = _same_answers(_passes(hip, ex.requests[0], {name: x}, dict(matches=gal), ['pvhip_gallery_match_f32'], [1], first_use=['pvhip_memcpy_h2d']),
                            out_name)
        assert got.counts.tolist() == [1] * n
    ex, _, name, out_name = keypoints_tests._mnist_head(tmp_path, n)
    got = _same_answers(_passes(hip, ex.requests[0], {name: x}, dict(keypoints=True), ['pvhip_heatmap_peaks_f32'], [1]), out_name)
    assert got.points.shape == (n, 32, 2)
    frames = RoiInput(tiled_tests._frames(rng, 'U8-NHWC', 2, (480, 640)), tiled_tests.TILES)
    for screen, entry, copies in ((DetectionScreen(0.0), 'pvhip_detections_compact', 2), (DetectionScreen(2.0), 'pvhip_detections_compact', 1),
                                  (TiledScreen(0.0), 'pvhip_detections_merge_tiles', 2)):
        det, name, out_name = det_tests._detector(4)
        got = _same_answers(_passes(hip, det.requests[0], {name: frames}, dict(detections=screen), [entry], [copies]), out_name)
        assert (got.counts.sum() > 0) == (copies == 2)


@pytest.mark.gpu
def test_two_kinds_behind_one_pass_share_one_selection_and_one_event(hip, tmp_path):
    """mnist at batch 2 with its first Convolution's heatmaps as a second Result, asked for top_k of the one and keypoints of the
    other in one pass: both launches stand behind one selection of the base stream and in front of one event."""
    from pyopenvino_amd import IECore, synth
    n = 2
    ie = IECore(plugin_package='pyopenvino_amd.op_plugins')
    net = ie.read_network(matrix._two_heads(str(tmp_path)), weights=os.path.join(matrix.MODELS, 'mnist.bin'))
    net.set_batch(n)
    ex = ie.load_network(net, 'GPU', num_requests=1)
    rows, maps = (out['name'] for out in sorted(net.outputs, key=lambda out: len(out['input'][0]['dims'])))
    x = hip.DeviceTensor.from_numpy(np.concatenate([synth.uniform_pixels(20 + i, (1, 1, 28, 28)) for i in range(n)], 0))
    answers = _passes(hip, ex.requests[0], {net.inputs[0]['name']: x}, dict(top_k={rows: 3}, keypoints={maps: True}),
                      ['pvhip_topk_rows_f32', 'pvhip_heatmap_peaks_f32'], [1, 1])
    assert _same_answers(answers, rows).indices.shape == (n, 3) and _same_answers(answers, maps).points.shape == (n, 32, 2)
