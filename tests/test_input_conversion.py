"""The launch a host input is converted by, and the order of the device work in front of it.  InputFormat.conversion chooses the entry and
its arguments on the host alone; tests/golden/input_conversions.json holds what HostInputs._convert issued for the same 840 cases
before the choice moved there (tests/golden/make_input_conversions.py recorded it, and owns the matrix).  On the GPU, one test pins the
calls HostInputs.stage() makes for every kind of feed, from the first upload to the conversion."""
import importlib.util
import json
import os

import numpy as np
import pytest

import test_landmark_warps as lt
import test_warp_input as wt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('make_input_conversions', os.path.join(GOLDEN, 'make_input_conversions.py'))
matrix = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(matrix)
KIND = {'images': None, 'roi': 'roi', 'detected': 'roi', 'warp': 'warp', 'perspective': 'perspective'}


def _recorded():
    with open(os.path.join(GOLDEN, 'input_conversions.json')) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_matrix():
    recorded, keys = _recorded(), [key for key, _, _, _ in matrix.cases()]
    assert len(keys) == len(set(keys)) == 840
    assert sorted(recorded) == sorted(keys)
    entries = {call[0] for call in recorded.values() if call}
    assert len(entries) == 16 and any(not call for call in recorded.values())        # every entry, and the case without a launch


def test_conversion_is_the_launch_recorded_for_every_case():
    from pyopenvino_amd.input_format import InputFormat
    recorded, none = _recorded(), 0
    for key, fields, extent, feed in matrix.cases():
        entry, args = InputFormat(**fields).conversion(extent, None if feed == 'images' else matrix.FRAMES, matrix.largest_of(extent, feed), KIND[feed])
        got = [] if entry is None else json.loads(json.dumps([entry, *args]))
        assert got == recorded[key], (key, got, recorded[key])
        assert entry is not None or args == ()
        none += entry is None
    assert none == sum(not call for call in recorded.values()) > 0
    # FP32 NCHW at the network's extent with nothing declared besides: the caller's array is the tensor
    assert recorded['f32.nchw|STRETCH|BT601|plain|32x32|images'] == []
    assert recorded['u8.nchw|STRETCH|BT601|plain|32x32|images'][0] == 'pvhip_input_to_nchw_f32'


UPLOAD = 'pvhip_memcpy_h2d_async'
# behind the uploads on the copy stream: the slot's event, the request's base stream, its wait for the event
BEHIND = ['pvhip_event_record', 'pvhip_stream_select', 'pvhip_stream_wait_event']


@pytest.mark.gpu
def test_stage_issues_its_device_work_in_one_order(hip):
    """mnist at batch 2, one request, frames of (20, 24), m = 3: the entries from the first upload of a pass up to and including its
    conversion, for every kind of feed -- frames first, then what the feed uploads beside them, the event, and on the base stream the
    launch that makes a table in front of the one that reads it."""
    from pyopenvino_amd import DetectedRois, LandmarkWarps, PerspectiveInput, RoiInput, WarpInput
    rng = np.random.default_rng(2024)
    n, m, hw = 2, 3, (20, 24)
    ex, name, _ = lt._mnist(n)
    frames = wt._frames(rng, 'U8-NCHW', m, hw, c=1)
    rois = np.array([(2, 1, 2, 9, 11), (0, 0, 0, 24, 20)], np.int32)
    records = np.array([(0, 1, 0.9, 0.1, 0.1, 0.6, 0.7), (1, 2, 0.8, 0.2, 0.0, 1.0, 0.9), (2, 1, 0.7, 0.0, 0.3, 0.5, 1.0)], np.float32)
    points = lt._points_near(rng, lt.T28, rois, hw, 28, m)
    landmarks = LandmarkWarps(frames, points, lt.T28, regions=rois)
    passes = [
        ('images', wt._frames(rng, 'U8-NCHW', n, (28, 28), c=1), 1, [], 'pvhip_input_to_nchw_f32'),
        ('RoiInput', RoiInput(frames, rois), 2, [], 'pvhip_input_preprocess_roi_f32'),
        ('WarpInput', WarpInput(frames, wt._translation(1.5, -2.0, n), [2, 0]), 2, [], 'pvhip_input_preprocess_warp_f32'),
        ('PerspectiveInput', PerspectiveInput(frames, np.array([np.eye(3)] * n), [1, 2]), 2, [], 'pvhip_input_preprocess_perspective_f32'),
        ('DetectedRois', DetectedRois(frames, records, labels=[1, 2]), 3, ['pvhip_detections_to_rois'], 'pvhip_input_preprocess_roi_f32'),
        ('LandmarkWarps', landmarks, 4, ['pvhip_landmarks_to_warps'], 'pvhip_input_preprocess_warp_f32'),
        ('LandmarkWarps again', landmarks, 3, ['pvhip_landmarks_to_warps'], 'pvhip_input_preprocess_warp_f32'),     # the template is uploaded once
    ]
    real_call = hip.call
    for what, feed, uploads, table, conversion in passes:
        issued = []
        hip.call = lambda entry, *args: (issued.append(entry), real_call(entry, *args))[1]
        try:
            ex.infer({name: feed})
        finally:
            hip.call = real_call
        assert UPLOAD in issued and conversion in issued, (what, issued)
        got = issued[issued.index(UPLOAD):issued.index(conversion) + 1]
        assert got == [UPLOAD] * uploads + BEHIND + table + [conversion], (what, got)
        assert [e for e in got if e not in BEHIND] == [UPLOAD] * uploads + table + [conversion], (what, got)
