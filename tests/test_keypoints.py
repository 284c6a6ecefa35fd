"""A heatmap network's answer made on the device (``infer(..., keypoints=...)``, pvhip_heatmap_peaks_f32): the peak of every plane of an
(n, K, H, W) Result by the rule of tests/keypoints_ref.py -- positions exact, scores and points bit for bit --, one launch behind the pass
and one read-back of 16 n K bytes.  The first tests need no GPU."""
import ctypes
import fractions
import itertools
import os
import re
import types
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import helpers
import keypoints_ref
import test_top_k as top_k_tests
from helpers import MODELS

ENTRY, FORM = 'pvhip_heatmap_peaks_f32', 'pvhip_heatmap_peaks_form'
HIP = 'pyopenvino_amd.op_plugins'
NAN, INF = np.float32(np.nan), np.float32(np.inf)
QUIET = 0x7FC00000
FORM_NONE, FORM_WAVE, FORM_BLOCK = 0, 1, 2              # PVHIP_PEAKS_FORM_*
WAVE_PLANE = 1024                                       # the last H * W of the one-wave-per-plane form
det_tests, roi_tests = top_k_tests.det_tests, top_k_tests.roi_tests
CONFIGS = list(itertools.product(('NONE', 'QUARTER'), ('HEATMAP', 'NORMALISED'), (False, True)))      # (refine, space, min_score given)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what=''):
    """`got` (a Keypoints of the product) equals `want` (the rule's): counts and positions exact, scores and points bit for bit."""
    assert got.counts.dtype == np.int32 and got.positions.dtype == np.int32 and got.scores.dtype == np.float32 and got.points.dtype == np.float32, what
    assert got.positions.shape == want.positions.shape == got.scores.shape and got.points.shape == want.points.shape == got.positions.shape + (2,), what
    bad = np.argwhere(got.positions != want.positions)
    assert not len(bad), '{}: plane {}: position {} want {}'.format(what, bad[0].tolist(), got.positions[tuple(bad[0])], want.positions[tuple(bad[0])])
    bad = np.argwhere(_bits(got.scores) != _bits(want.scores))
    assert not len(bad), '{}: plane {}: score bits {:#x} want {:#x}'.format(what, bad[0].tolist(), _bits(got.scores)[tuple(bad[0])], _bits(want.scores)[tuple(bad[0])])
    bad = np.argwhere((_bits(got.points) != _bits(want.points)).any(axis=2))
    assert not len(bad), '{}: plane {}: point {} want {}'.format(what, bad[0].tolist(), got.points[tuple(bad[0])].tolist(), want.points[tuple(bad[0])].tolist())
    assert np.array_equal(got.counts, want.counts), '{}: counts {} want {}'.format(what, got.counts.tolist(), want.counts.tolist())


def _threshold(scores):
    """A min_score that keeps some of the peaks and voids others where they differ: the median of the finite peak scores (0 without one)."""
    finite = scores[np.isfinite(scores)]
    return float(np.median(finite)) if finite.size else 0.0


def _heatmap_head(model, tmp_path):
    """`model`'s IR up to the bias Add (and the ReLU, if one follows) of its first Convolution, with a Result appended, written to
    `tmp_path` from the shipped xml (the shipped weights serve it: the offsets are the same): the path of the new xml."""
    tree = ET.parse(os.path.join(MODELS, model + '.xml'))
    layers, edges = tree.getroot().find('layers'), tree.getroot().find('edges')
    by_id = {int(layer.get('id')): layer for layer in layers}

    def consumers(i):
        return [int(e.get('to-layer')) for e in edges if int(e.get('from-layer')) == i]

    last = min(i for i, layer in by_id.items() if layer.get('type') == 'Convolution')
    (nxt,) = consumers(last)
    assert by_id[nxt].get('type') == 'Add'
    last = nxt
    nxt = consumers(last)
    if len(nxt) == 1 and by_id[nxt[0]].get('type') == 'ReLU':
        last = nxt[0]
    for e in list(edges):                                    # the layers up to `last` are a closed prefix of the list
        if int(e.get('to-layer')) > last:
            edges.remove(e)
        else:
            assert int(e.get('from-layer')) <= last
    for i, layer in by_id.items():
        if i > last:
            layers.remove(layer)
    out_port = by_id[last].find('output').find('port')
    result = ET.SubElement(layers, 'layer', {'id': str(last + 1), 'name': 'heatmaps', 'type': 'Result', 'version': 'opset1'})
    port = ET.SubElement(ET.SubElement(result, 'input'), 'port', {'id': '0', 'precision': 'FP32'})
    for dim in out_port.findall('dim'):
        ET.SubElement(port, 'dim').text = dim.text
    ET.SubElement(edges, 'edge', {'from-layer': str(last), 'from-port': out_port.get('id'), 'to-layer': str(last + 1), 'to-port': '0'})
    path = os.path.join(str(tmp_path), model + '_head.xml')
    tree.write(path)
    return path


def _mnist_head(tmp_path, batch, requests=1, package=HIP):
    """The first Convolution + bias + ReLU of mnist as a heatmap network: (the loaded network, input name, Result name); the Result is
    (batch, 32, 26, 26)."""
    from pyopenvino_amd import IECore
    ie = IECore(plugin_package=package)
    net = ie.read_network(_heatmap_head('mnist', tmp_path), weights=os.path.join(MODELS, 'mnist.bin'))
    net.set_batch(batch)
    assert tuple(int(d) for d in net.outputs[0]['input'][0]['dims']) == (batch, 32, 26, 26)
    return ie.load_network(net, 'GPU', num_requests=requests), net, net.inputs[0]['name'], net.outputs[0]['name']


def _pixels(seed, batch):
    from pyopenvino_amd import synth
    return np.concatenate([synth.uniform_pixels(seed + i, (1, 1, 28, 28)) for i in range(batch)], 0)


def _ref(full, screen=None):
    from pyopenvino_amd import PeakScreen
    screen = screen or PeakScreen()
    return keypoints_ref.keypoints(full, screen.min_score, screen.refine, screen.space)


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
def test_the_rule_on_hand_written_planes():
    from pyopenvino_amd import Keypoints, PeakScreen, keypoints

    def both(plane, min_score=None, refine='QUARTER', space='HEATMAP'):
        x = np.asarray(plane, np.float32)[None, None]
        want = keypoints_ref.keypoints(x, min_score, refine, space)
        got = keypoints.peaks(x, PeakScreen(min_score, refine, space))      # the product's own numpy form (host Results) is the same rule
        assert isinstance(got, Keypoints)
        _same(got, want, str(np.asarray(plane).tolist()))
        assert _bits(want.scores)[0, 0] == _bits(x).reshape(-1)[want.positions[0, 0]]
        return int(want.positions[0, 0]), tuple(want.points[0, 0].tolist()), int(want.counts[0])

    def spike(h, w, py, px, **around):
        v = np.zeros((h, w), np.float32)
        v[py, px] = 9
        for name, value in around.items():
            dy, dx = {'l': (0, -1), 'r': (0, 1), 'u': (-1, 0), 'd': (1, 0)}[name]
            v[py + dy, px + dx] = value
        return v

    # ties and all-equal planes: position 0, no offset
    assert both(np.full((4, 5), 2.5)) == (0, (0.0, 0.0), 1)
    assert both([[1, 3, 3], [3, 2, 3]]) == (1, (1.25, 0.0), 1)                      # ties: the lower flat index (r = 3 > l = 1; row 0: no oy)
    assert both([[0, 1, 3, 3, 0]]) == (2, (2.25, 0.0), 1)
    assert both(np.array([[0.0, -0.0], [-0.0, 0.0]])) == (0, (0.0, 0.0), 1)         # zeros of either sign are equal
    assert both(np.array([[-0.0, -1, 0.0, -1]]))[0] == 0
    # a peak in each corner and on each edge gives no offset on that axis: what stands next to it in the flat order (the end of the row
    # above, the start of the row below) is no neighbour; the neighbours that exist pull at the other axis
    for py, px in itertools.product((0, 2, 4), (0, 3, 6)):
        v = np.arange(35, dtype=np.float32).reshape(5, 7) / 8                       # every value differs: ascending, so r > l and d > u
        v[py, px] = 9
        want = (px + (0.25 if 0 < px < 6 else 0.0), py + (0.25 if 0 < py < 4 else 0.0))
        assert both(v) == (py * 7 + px, want, 1), (py, px)
        want = (px - (0.25 if 0 < px < 6 else 0.0), py - (0.25 if 0 < py < 4 else 0.0))
        v = -v
        v[py, px] = 9
        assert both(v) == (py * 7 + px, want, 1), (py, px)
    # r > l, r < l, r == l, +0 against -0
    assert both(spike(3, 5, 1, 2, l=1, r=2))[1] == (2.25, 1.0)
    assert both(spike(3, 5, 1, 2, l=2, r=1))[1] == (1.75, 1.0)
    assert both(spike(3, 5, 1, 2, l=2, r=2, u=1, d=3))[1] == (2.0, 1.25)
    assert both(spike(3, 5, 1, 2, l=2, r=2, u=3, d=1))[1] == (2.0, 0.75)
    assert both(spike(3, 5, 1, 2, l=0.0, r=-0.0, u=-0.0, d=0.0))[1] == (2.0, 1.0)
    assert both(spike(3, 5, 1, 2, l=-1, r=-2, u=-INF, d=-3e38))[1] == (1.75, 1.25)  # (negative neighbours)
    assert both(spike(3, 5, 1, 2, l=1, r=2, u=3, d=1), refine='NONE')[1] == (2.0, 1.0)
    # +inf peaks, -inf neighbours
    v = spike(3, 5, 1, 2, u=1, d=2)
    v[1, 2], v[1, 1], v[1, 3] = INF, -INF, 1
    assert both(v) == (7, (2.25, 1.25), 1)
    v[1, 3] = INF                                                                   # two +inf: the first; its right neighbour +inf > -inf
    assert both(v) == (7, (2.25, 1.25), 1)
    # a NaN anywhere in the plane wins and voids the keypoint -- so a peak with a NaN neighbour is a NaN peak --, whatever its sign or payload
    for at, word in (((2, 4), 0x7FC00000), ((1, 3), 0xFFC00001), ((0, 0), 0x7F800123), ((1, 1), 0xFF800001)):
        v = spike(3, 5, 1, 2, l=1, r=2)
        v.view(np.uint32)[at] = word
        pos, point, count = both(v)
        assert pos == at[0] * 5 + at[1] and count == 0 and np.isnan(point).all(), at
        assert both(v, -1e30, 'NONE', 'NORMALISED')[2] == 0
    v = spike(3, 5, 1, 2)
    v[1, 3], v[0, 1] = NAN, NAN
    assert both(v)[0] == 1                                                          # several NaNs: the first
    # all -inf: valid, position 0
    assert both(np.full((2, 3), -np.inf)) == (0, (0.0, 0.0), 1)
    assert both(np.full((2, 3), -np.inf), -3e38)[2] == 0
    # H == 1 and W == 1
    assert both([[1, 5, 7, 2]]) == (2, (1.75, 0.0), 1)
    assert both([[1], [5], [7], [2]]) == (2, (0.0, 1.75), 1)
    assert both([[1, 2]]) == (1, (1.0, 0.0), 1) and both([[2], [1]]) == (0, (0.0, 0.0), 1)
    # min_score equal to (kept), just above and just below the peak
    peak = np.float32(0.7)
    v = spike(3, 5, 1, 2, l=0.1, r=0.2)
    v[1, 2] = peak
    assert both(v, float(peak))[2] == 1 and both(v, float(np.nextafter(peak, INF)))[2] == 0 and both(v, float(np.nextafter(peak, -INF)))[2] == 1
    assert both(v, 0.7)[2] == 1                                                     # float32(0.7) is the threshold, not the double
    assert both(-v, -0.0)[2] == 1 and both(np.zeros((2, 2)) - 0.0, 0.0)[2] == 1      # -0.0 >= +0.0
    # the 'NORMALISED' values of a 3 x 5 plane as exact fractions
    for py, px in itertools.product(range(3), range(5)):
        for around in ({}, dict(l=1, r=2, u=2, d=1)):
            around = {k: a for k, a in around.items() if (k in 'lr' and 0 < px < 4) or (k in 'ud' and 0 < py < 2)}
            _, (x_, y_), _ = both(spike(3, 5, py, px, **around), space='NORMALISED')
            fx = fractions.Fraction(px) + (fractions.Fraction(1, 4) if 'r' in around else 0)
            fy = fractions.Fraction(py) - (fractions.Fraction(1, 4) if 'u' in around else 0)
            assert x_ == float(np.float32(float((fx + fractions.Fraction(1, 2)) / 5))), (py, px, around)      # (one rounding to double, one to fp32: the
            assert y_ == float(np.float32(float((fy + fractions.Fraction(1, 2)) / 3))), (py, px, around)      # division of two doubles that are exact)
    assert both(spike(3, 5, 1, 2), space='NORMALISED')[1] == (0.5, 0.5)
    # anything but float32 (n, K, H, W) with 2 <= H * W is refused
    for bad in (np.zeros((1, 1, 1, 1), np.float32), np.zeros((2, 3, 4), np.float32), np.zeros((1, 1, 2, 2), np.float64), np.zeros((1, 0, 2, 2), np.float32)):
        with pytest.raises(ValueError, match='peaks'):
            keypoints.peaks(bad)
    for bad in ('x', None, False, PeakScreen(refine='HALF'), PeakScreen(space='PIXELS'), PeakScreen(np.nan), PeakScreen(1e39)):
        with pytest.raises(ValueError, match='peaks'):
            keypoints.peaks(np.zeros((1, 1, 2, 2), np.float32), bad)


def _spikes(rng, shape, right, left):
    """One spike at a random position per plane over a low random floor; its neighbours that exist: `left` before it and `right`
    behind it, on both axes."""
    n, K, H, W = shape
    x = rng.uniform(0, 0.5, shape).astype(np.float32)
    for r in range(n):
        for c in range(K):
            py, px = int(rng.integers(0, H)), int(rng.integers(0, W))
            x[r, c, py, px] = 10
            for dy, dx, value in ((0, -1, left), (0, 1, right), (-1, 0, left), (1, 0, right)):
                if 0 <= py + dy < H and 0 <= px + dx < W:
                    x[r, c, py + dy, px + dx] = value
    return x


def _fillings(rng, shape):
    """[(what, (n, K, H, W) float32)]: every filling of the rule's kernel test for one shape."""
    n, K, H, W = shape
    size = H * W
    specials = np.array(top_k_tests.SPECIALS, np.uint32)
    ramp = (np.arange(size, dtype=np.float32)[None, :] + np.arange(n * K, dtype=np.float32)[:, None]).reshape(shape)     # exact: below 2^24
    mixed = rng.standard_normal((n * K, size)).astype(np.float32)
    nans = rng.standard_normal((n * K, size)).astype(np.float32)
    for i in range(n * K):
        at = rng.choice(size, size=min(size, len(specials)), replace=False)
        start = 0 if size >= len(specials) else int(rng.integers(0, len(specials)))
        mixed[i].view(np.uint32)[at] = np.roll(specials, -start)[:len(at)]
        if i % 3 != 2:                                        # (two planes of three: the third keeps a finite peak)
            many = min(size, 3)
            at = rng.choice(size, size=many, replace=False)
            nans[i].view(np.uint32)[at] = (np.uint32(0x7FC00000) | rng.integers(0, 1 << 22, many).astype(np.uint32)
                                           | (rng.integers(0, 2, many).astype(np.uint32) << np.uint32(31)))
    rows = rng.standard_normal(shape).astype(np.float32)
    rows.view(np.uint32)[n // 2:] = QUIET                      # the rows behind `count` of a cascade (n == 1: the only row)
    return [('normal', rng.standard_normal(shape).astype(np.float32)),
            ('three values', rng.integers(-1, 2, shape).astype(np.float32)),
            ('all equal', np.full(shape, 0.25, np.float32)),
            ('ascending', ramp),
            ('descending', np.ascontiguousarray(-ramp)),
            ('spike, equal neighbours', _spikes(rng, shape, 1, 1)),
            ('spike, greater right', _spikes(rng, shape, 2, 1)),
            ('spike, greater left', _spikes(rng, shape, 1, 2)),
            ('specials', mixed.reshape(shape)),
            ('NaNs', nans.reshape(shape)),
            ('NaN rows', rows)]


@pytest.mark.parametrize('shape', [(1, 1, 1, 2), (2, 3, 1, 7), (3, 5, 7, 9), (2, 4, 6, 1), (1, 2, 31, 33), (2, 2, 40, 30)])
def test_peaks_agrees_with_the_loops(shape):
    from pyopenvino_amd import PeakScreen, keypoints
    rng = np.random.default_rng(sum(d * 31 ** i for i, d in enumerate(shape)))
    for what, x in _fillings(rng, shape):
        at = keypoints_ref.positions(x)
        cut = _threshold(np.take_along_axis(x.reshape(shape[0], shape[1], -1), at[:, :, None].astype(np.int64), axis=2))
        for refine, space, given in CONFIGS:
            min_score = cut if given else None
            _same(keypoints.peaks(x, PeakScreen(min_score, refine, space)), keypoints_ref.keypoints(x, min_score, refine, space, at),
                  '{} {} {}'.format(shape, what, (refine, space, min_score)))
    x = rng.standard_normal((2, 3, 8, 5, 7)).astype(np.float32)[:, :, :, :, 2]          # not contiguous: the same answer
    _same(keypoints.peaks(x), keypoints_ref.keypoints(np.ascontiguousarray(x)), 'strided')


def _regions(rng, n, frame_hw):
    h, w = frame_hw
    table = np.empty((n, 5), np.int32)
    for b in range(n):
        rw, rh = int(rng.integers(8, w // 2)), int(rng.integers(8, h // 2))
        table[b] = (rng.integers(0, 3), rng.integers(0, w - rw), rng.integers(0, h - rh), rw, rh)
    return table


def test_to_frame_agrees_with_landmark_rows():
    """to_frame's positions are those landmarks._row forms from the same point: the expression on Python floats, value for value, and
    the similarity fitted on to_frame's positions is the table row to_warps makes from the points themselves."""
    from pyopenvino_amd import keypoints, landmarks
    rng = np.random.default_rng(77)
    n, K, frame_hw = 9, 5, (480, 640)
    x = rng.standard_normal((n, K, 23, 17)).astype(np.float32)
    x[4, 2, 3, 3] = NAN                                        # one void keypoint
    got = keypoints.peaks(x)
    regions = _regions(rng, n, frame_hw)
    frame = keypoints.to_frame(got.points, regions)
    assert frame.shape == (n, K, 2) and frame.dtype == np.float64
    for b in range(n):
        _, rx, ry, rw, rh = regions[b].tolist()
        for c in range(K):
            u, v = (float(t) for t in got.points[b, c])
            if (b, c) == (4, 2):
                assert np.isnan(frame[b, c]).all()
            else:
                assert frame[b, c].tolist() == [(float(rx) + u * float(rw)) - 0.5, (float(ry) + v * float(rh)) - 0.5]      # landmarks._row's expression
    template = rng.uniform(10, 100, (K, 2))
    table, valid = landmarks.to_warps(got.points.reshape(n, 2 * K), regions, template, frame_hw, 3)
    assert valid.tolist() == [b != 4 for b in range(n)]
    for b in np.flatnonzero(valid):
        m = landmarks.similarity(frame[b], template)
        want = [int(regions[b, 0])] + [round(float(t) * 65536.0) for t in (m[0, 0], m[0, 1], m[0, 2], m[1, 0], m[1, 1], m[1, 2])]
        assert table[b].tolist() == want, b
    for bad_points, bad_regions in ((got.points.astype(np.float64), regions), (got.points[:, :, :1], regions), (got.points, regions[:-1]),
                                    (got.points, regions.astype(np.float32))):
        with pytest.raises(ValueError, match='to_frame'):
            keypoints.to_frame(bad_points, bad_regions)


def test_a_normalised_block_goes_through_to_warps_unchanged():
    """points.reshape(n, 2 K) of a 'NORMALISED' answer is the (N, 2 K) landmark Result to_warps takes: the same table as from the
    points formed here in exact fractions, and a row with a void keypoint is a void row."""
    from pyopenvino_amd import keypoints, landmarks
    rng = np.random.default_rng(5)
    n, K, H, W, frame_hw = 6, 5, 12, 20, (300, 400)
    x = np.zeros((n, K, H, W), np.float32)
    want = np.empty((n, K, 2), np.float32)
    for b in range(n):
        for c in range(K):
            py, px = int(rng.integers(1, H - 1)), int(rng.integers(1, W - 1))
            x[b, c, py, px], x[b, c, py, px + 1], x[b, c, py - 1, px] = 3, 1, 2              # a quarter right, a quarter up
            want[b, c] = (float((fractions.Fraction(4 * px + 3, 4)) / W), float(fractions.Fraction(4 * py + 1, 4) / H))
    x[2, 1] = NAN
    got = keypoints.peaks(x, 2.5)
    assert got.counts.tolist() == [K, K, K - 1, K, K, K] and np.array_equal(_bits(np.delete(got.points, 2, 0)), _bits(np.delete(want, 2, 0)))
    block = got.points.reshape(n, 2 * K)
    regions = _regions(rng, n, frame_hw)
    template = rng.uniform(0, 111, (K, 2))
    table, valid = landmarks.to_warps(block, regions, template, frame_hw, 3)
    table_want, valid_want = landmarks.to_warps(want.reshape(n, 2 * K), regions, template, frame_hw, 3)
    assert valid.tolist() == [b != 2 for b in range(n)] and valid_want.all()
    assert np.array_equal(table[valid], table_want[valid]) and table[2].tolist() == list(landmarks.VOID)


def test_argument_rules(tmp_path, monkeypatch):
    """Every refusal is a ValueError('keypoints: ...') raised before anything is staged or launched: this test runs where there is no device."""
    from pyopenvino_amd import Gallery, GalleryMatch, PeakScreen, answers as answers_module, detections as detections_rule, keypoints as rule
    n = 4
    ex, net, name, out_name = _mnist_head(tmp_path, n, requests=2)
    x = np.zeros((n, 1, 28, 28), np.float32)
    req = ex.requests[0]
    starts = (lambda k, **kw: ex.infer({name: x}, keypoints=k, **kw), lambda k, **kw: req.start_async({name: x}, keypoints=k, **kw),
              lambda k, **kw: ex.requests[1].infer({name: x}, keypoints=k, **kw), lambda k, **kw: ex.start_async(1, {name: x}, keypoints=k, **kw),
              lambda k, **kw: req.infer({name: x}, kw.get('top_k'), kw.get('detections'), kw.get('matches'), k),
              lambda k, **kw: ex.infer({name: x}, False, kw.get('top_k'), kw.get('detections'), kw.get('matches'), k),
              lambda k, **kw: ex.start_async(0, {name: x}, kw.get('top_k'), kw.get('detections'), kw.get('matches'), k))

    def refused(match, k, network=ex, starts=starts, **kw):
        for start in starts:
            with pytest.raises(ValueError, match=match) as e:
                start(k, **kw)
            assert str(e.value).startswith('keypoints: '), str(e.value)
        for r in network.requests:
            assert not r._in_flight and not r._asks and not r.runner.answers.blocks and not r.runner.host_inputs.slots and r.runner._pending is None

    refused('no Result named', {'heatmaps/nope': True})
    refused('no Result named', {out_name: True, 'nope': 0.5})
    for bad in ('QUARTER', [0.5], (0.5,), False, np.bool_(True), b'1', 1j, PeakScreen):
        refused('a PeakScreen, a min_score or True', bad)
        refused('a PeakScreen, a min_score or True', {out_name: bad})
    refused('a PeakScreen, a min_score or True', {out_name: None})
    for bad in ('HALF', 'quarter', None, 1):
        refused('refine', PeakScreen(refine=bad))
        refused('refine', {out_name: PeakScreen(0.5, bad)})
    for bad in ('PIXELS', 'normalised', None, 0):
        refused('space', PeakScreen(space=bad))
    for bad in (np.nan, np.inf, -np.inf, 'x', True, 1e39, -1e39, [1.0]):
        refused('min_score', PeakScreen(bad))
        refused('min_score', {out_name: PeakScreen(min_score=bad)})
    for bad in (np.nan, np.inf, 1e39, np.float64(-1e300)):
        refused('min_score', bad)
    ex.comm = types.SimpleNamespace(world=2, rank=0)
    try:
        refused('sharded', True)
        refused('sharded', {out_name: 0.5})
    finally:
        ex.comm = None
    ports = [r.runner.ienet.outputs[0]['input'][0] for r in ex.requests]       # (every request has its own copy of the graph)
    for port in ports:
        port['precision'] = 'FP16'
    try:
        refused('FP32 Results only', {out_name: True})
        refused('no FP32 Result', True)
    finally:
        for port in ports:
            port['precision'] = 'FP32'
    declared = [port['dims'] for port in ports]
    for dims, named in (((n, 32, 676), 'has shape'), ((n, 32, 26, 26, 1), 'has shape'), ((n, 32, 1, 1), 'has shape'), ((2, 32, 26, 26), 'has shape'),
                        ((n, 32, 4097, 4096), 'has shape')):                     # another rank, one element, another batch, beyond 2^24
        for port in ports:
            port['dims'] = dims
        try:
            refused(named, {out_name: True})
            refused('no FP32 Result', 0.5)
        finally:
            for port, dims in zip(ports, declared):
                port['dims'] = dims
    # a classifier has no heatmaps, a detector's (1, 1, R, 7) records are none for the unnamed forms
    ie_c, net_c, name_c = roi_tests._net('mnist', n)
    cls = ie_c.load_network(net_c, 'GPU', num_requests=1)
    xc = np.zeros((n, 1, 28, 28), np.float32)
    cls_starts = (lambda k, **kw: cls.infer({name_c: xc}, keypoints=k), lambda k, **kw: cls.requests[0].start_async({name_c: xc}, keypoints=k))
    refused('no FP32 Result', True, cls, cls_starts)
    refused('has shape', {net_c.outputs[0]['name']: True}, cls, cls_starts)
    ie_d, net_d, name_d = roi_tests._net('ssd_mobilenet_v1_coco', 1)
    det = ie_d.load_network(net_d, 'GPU', num_requests=1)
    dims = tuple(net_d.outputs[0]['input'][0]['dims'])
    assert dims[:2] == (1, 1) and dims[3] == 7
    xd = np.zeros((1, 3, 300, 300), np.float32)
    refused('no FP32 Result', True, det, (lambda k, **kw: det.infer({name_d: xd}, keypoints=k), lambda k, **kw: det.requests[0].start_async({name_d: xd}, keypoints=k)))
    # one Result under two keywords.  No Result passes the shape rules of keypoints and of another keyword, so the rule of
    # Answers.checked itself is reached with the other keyword's check stubbed (gallery's with the three arguments it has always had)
    gal = Gallery(np.ones((3, 7), np.float32))
    for keyword, module, stub, value in (('top_k', answers_module.top_k_rule, lambda ienet, top_k, sharded: {out_name: 1}, 1),
                                         ('detections', answers_module.detections_rule, lambda ienet, d, sharded: {out_name: detections_rule.DetectionScreen()}, 0.5),
                                         ('matches', answers_module.gallery_rule, lambda ienet, matches, sharded: {out_name: GalleryMatch(gal, 1, None)}, gal)):
        with monkeypatch.context() as patched:
            patched.setattr(module, 'checked', stub)
            refused('Result {!r} is asked for with {} as well'.format(out_name, keyword), True, **{keyword: value})
            refused('Result {!r} is asked for with {} as well'.format(out_name, keyword), {out_name: 0.5}, **{keyword: value})
            assert set(ex.answers.checked({name: x}, *((value if keyword == k else None) for k in ('top_k', 'detections')), False,
                                          value if keyword == 'matches' else None)) == {out_name}      # (alone it is fine)
    assert gal._dev is None
    # the resolved forms
    default = PeakScreen(None, 'QUARTER', 'NORMALISED')
    assert PeakScreen() == default
    assert rule.checked(net, None, False) == {} and rule.checked(net, {}, True) == {} and rule.checked(net, True, False) == {out_name: default}
    assert rule.checked(net, 0.5, False) == rule.checked(net, {out_name: np.float32(0.5)}, False) == {out_name: default._replace(min_score=0.5)}
    assert rule.checked(net, 1, False) == {out_name: default._replace(min_score=1.0)} and isinstance(rule.checked(net, 1, False)[out_name].min_score, float)
    assert rule.checked(net, 0.7, False)[out_name].min_score == float(np.float32(0.7))                   # the threshold is the float32
    assert rule.checked(net, {out_name: PeakScreen(np.int64(-2), 'NONE', 'HEATMAP')}, False) == {out_name: PeakScreen(-2.0, 'NONE', 'HEATMAP')}
    assert rule.planes_of((4, 17, 64, 48)) == (4, 17, 64, 48) and rule.planes_of((4, 17, 64, 48), 2) is None and rule.planes_of((4, 17, 1, 1)) is None
    # the asks, and the positional calls of Answers.checked as they were
    answers = ex.answers
    assert answers.checked({name: x}, None, None, False) == {} and answers.checked({name: x}, None, None, False, None) == {}
    assert answers.checked({name: x}, None, None, False, None, None) == {} and answers.checked({name: x}, None, None, False, keypoints=None) == {}
    asks = answers.checked({name: x}, None, None, False, None, 0.5)
    assert set(asks) == {out_name} and isinstance(asks[out_name], rule.Ask) and asks[out_name].screen == default._replace(min_score=0.5)
    assert asks[out_name].key(out_name) == (out_name, 'QUARTER', 'NORMALISED')
    assert rule.Ask(default).key(out_name) == asks[out_name].key(out_name)       # (one block pair for every threshold)
    assert rule.Ask(PeakScreen(None, 'NONE', 'NORMALISED')).key(out_name) != asks[out_name].key(out_name)
    assert asks[out_name].bound({name: x}, {}) is asks[out_name]
    # on a classifier the old positional forms answer as before
    assert cls.answers.checked({name_c: xc}, 5, None, False) == {net_c.outputs[0]['name']: (5,)}
    assert cls.answers.checked({name_c: xc}, {net_c.outputs[0]['name']: 3}, None, False, None) == {net_c.outputs[0]['name']: (3,)}


def test_a_host_result_gets_the_rule_in_numpy(tmp_path):
    """A plugin set that computes on the host (the oracle's) hands wait() host arrays: the same keyword, the same rule, no device."""
    from pyopenvino_amd import Keypoints, PeakScreen
    n = 4
    ex, net, name, out_name = _mnist_head(tmp_path, n, requests=2, package='oracle.op_plugins')
    x = _pixels(10, n)
    full = np.array(ex.infer({name: x})[out_name], copy=True)
    assert full.shape == (n, 32, 26, 26) and full.dtype == np.float32 and np.isfinite(full).all()
    cut = _threshold(full.reshape(n, 32, -1).max(axis=2))
    assert (full.reshape(n, 32, -1).max(axis=2) >= np.float32(cut)).sum() not in (0, n * 32)
    for given in (True, cut, PeakScreen(cut, 'NONE', 'HEATMAP'), PeakScreen(None, 'QUARTER', 'HEATMAP')):
        screen = given if isinstance(given, PeakScreen) else PeakScreen(None if given is True else given)
        for got in (ex.infer({name: x}, keypoints=given), ex.requests[1].infer({name: x}, keypoints={out_name: given})):
            assert set(got) == {out_name} and isinstance(got[out_name], Keypoints)
            _same(got[out_name], _ref(full, screen._replace(min_score=None if screen.min_score is None else float(np.float32(screen.min_score)))), repr(given))
    got = ex.infer({name: x}, keypoints=True)[out_name]
    assert got.counts.tolist() == [32] * n and got.points.shape == (n, 32, 2) and (got.points >= 0).all() and (got.points <= 1).all()
    assert np.array_equal(ex.infer({name: x})[out_name], full)           # and whole again without the keyword
    with pytest.raises(ValueError, match='keypoints: refine'):
        ex.infer({name: x}, keypoints=PeakScreen(refine='HALF'))


def test_abi_declares_the_entries():
    import pyopenvino_amd
    from pyopenvino_amd import device, keypoints
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for entry, count in ((ENTRY, 12), (FORM, 2)):
        assert entry in device.SIGNATURES and len(device.SIGNATURES[entry][1]) == count
        m = re.search(r'\bint\s+' + entry + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S)
        assert m and len(m.group(1).split(',')) == count, entry
    assert ENTRY not in device._NOT_STATUS and FORM in device._NOT_STATUS
    for phrase in ('NaN of any sign or payload first, then descending with +0.0 == -0.0, ties to the lower flat index', 'py = p / w, px = p % w',
                   'valid iff its score is not NaN and (has_min == 0 or score >= min_score)', 'ox = +0.25f if r > l, -0.25f if r < l, else 0',
                   'x = (float)((double)(fx + 0.5f) / (double)w)', 'two quiet NaNs 0x7FC00000'):
        assert phrase in re.sub(r'\s*\n \*\s+', ' ', header), phrase        # the rule is stated there (its lines joined)
    for define, value in (('PVHIP_PEAKS_NONE', 0), ('PVHIP_PEAKS_QUARTER', 1), ('PVHIP_PEAKS_HEATMAP', 0), ('PVHIP_PEAKS_NORMALISED', 1),
                          ('PVHIP_PEAKS_FORM_NONE', FORM_NONE), ('PVHIP_PEAKS_FORM_WAVE', FORM_WAVE), ('PVHIP_PEAKS_FORM_BLOCK', FORM_BLOCK)):
        assert re.search(r'#define\s+{}\s+{}\b'.format(define, value), header), define
    assert keypoints.REFINES == {'NONE': 0, 'QUARTER': 1} and keypoints.SPACES == {'HEATMAP': 0, 'NORMALISED': 1} and keypoints.MAX_PLANE == 1 << 24
    assert re.search(r'#define\s+PVHIP_ABI_VERSION\s+19\b', header)
    lib = device.load_library()
    assert hasattr(lib, ENTRY) and hasattr(lib, FORM) and lib.pvhip_abi_version() == 19
    assert pyopenvino_amd.Keypoints is keypoints.Keypoints and pyopenvino_amd.PeakScreen is keypoints.PeakScreen
    assert 'Keypoints' in pyopenvino_amd.__all__ and 'PeakScreen' in pyopenvino_amd.__all__
    assert pyopenvino_amd.Keypoints._fields == ('counts', 'points', 'scores', 'positions')
    assert pyopenvino_amd.PeakScreen._fields == ('min_score', 'refine', 'space') and tuple(pyopenvino_amd.PeakScreen()) == (None, 'QUARTER', 'NORMALISED')
    # the form query needs no device and answers for planes the entry refuses
    form = lambda h, w: device.call(FORM, h, w)
    assert [form(1, 1), form(0, 5), form(5, -1), form(4097, 4096), form(1 << 16, 1 << 16)] == [FORM_NONE] * 5
    assert form(1, 2) == form(2, 1) == form(26, 26) == FORM_WAVE and form(4096, 4096) == form(1, 1 << 24) == form(46, 46) == form(64, 48) == FORM_BLOCK


def _form_steps():
    """Every H * W after which pvhip_heatmap_peaks_form changes its answer, for planes of one row (the form depends on H * W alone)."""
    from pyopenvino_amd import device
    forms = [device.call(FORM, 1, s) for s in range(2, 1 << 14)]
    return [s for s, (a, b) in zip(range(2, 1 << 14), zip(forms, forms[1:])) if a != b]


def test_the_form_changes_where_the_kernel_test_stands():
    from pyopenvino_amd import device
    assert _form_steps() == [WAVE_PLANE]                       # a moved threshold fails here and in the kernel test, not silently
    for h, w in ((32, 32), (1, 1024), (1024, 1), (16, 64)):
        assert device.call(FORM, h, w) == FORM_WAVE
    for h, w in ((25, 41), (1, 1025), (1025, 1), (5, 205)):
        assert device.call(FORM, h, w) == FORM_BLOCK


# ---------------------------------------------------------------------------------------------------------------- GPU
GUARD, SENTINEL = top_k_tests.GUARD, top_k_tests.SENTINEL


def _device_peaks(hip, x, min_score, refine, space, offset=0):
    """The entry on `x` (n, K, H, W) -- `offset`: starting that many elements into a larger device tensor --, the outputs between
    sentinel words that must stay untouched."""
    from pyopenvino_amd import keypoints
    n, K, H, W = x.shape
    if offset:
        src = hip.DeviceTensor.from_numpy(np.concatenate([np.full(offset, 9e9, np.float32), x.ravel(), np.full(7, 9e9, np.float32)]))
    else:
        src = hip.DeviceTensor.from_numpy(x)
    outs = [hip.DeviceTensor.empty((words * n * K + 2 * GUARD,), np.int32) for words in (1, 1, 2)]
    for t in outs:
        hip.call('pvhip_memset', ctypes.c_void_p(t.ptr), 0x7f, t.nbytes)
    hip.call(ENTRY, ctypes.c_void_p(src.ptr + 4 * offset), n, K, H, W, keypoints.REFINES[refine], keypoints.SPACES[space], int(min_score is not None),
             float(min_score or 0.0), *(ctypes.c_void_p(t.ptr + 4 * GUARD) for t in outs))
    pos, sco, pts = (np.asarray(t) for t in outs)
    for t in (pos, sco, pts):
        assert (t[:GUARD] == SENTINEL).all() and (t[-GUARD:] == SENTINEL).all(), 'a word outside the output was written'
    assert not (pos[GUARD:-GUARD] == SENTINEL).any() and not (pts[GUARD:-GUARD] == SENTINEL).any(), 'an answer was not written'
    points = pts[GUARD:-GUARD].view(np.float32).reshape(n, K, 2).copy()
    return keypoints_ref.Keypoints((~np.isnan(points[:, :, 0])).sum(axis=1).astype(np.int32), points,
                                   sco[GUARD:-GUARD].view(np.float32).reshape(n, K).copy(), pos[GUARD:-GUARD].reshape(n, K).copy())


def _kernel_equals_the_rule(hip, shape, offsets=()):
    rng = np.random.default_rng(sum(d * 31 ** i for i, d in enumerate(shape)))
    for what, x in _fillings(rng, shape):
        at = keypoints_ref.positions(x)                        # once per tensor: the screen does not move the peak
        cut = _threshold(np.take_along_axis(x.reshape(shape[0], shape[1], -1), at[:, :, None].astype(np.int64), axis=2))
        for refine, space, given in CONFIGS:
            min_score = cut if given else None
            want = keypoints_ref.keypoints(x, min_score, refine, space, at)
            _same(_device_peaks(hip, x, min_score, refine, space), want, '{} {} {}'.format(shape, what, (refine, space, min_score)))
            for offset in offsets:
                _same(_device_peaks(hip, x, min_score, refine, space, offset), want, '{} {} {} offset {}'.format(shape, what, (refine, space, min_score), offset))


# (3, 5, 7, 9): no plane after the first starts on a 16-byte boundary; (1, 2, 32, 32) and (1, 2, 25, 41) stand on the two sides of the form's step
SHAPES = [(1, 1, 1, 2), (1, 1, 2, 1), (2, 3, 1, 7), (3, 5, 7, 9), (2, 17, 8, 8), (1, 2, 31, 33), (1, 2, 32, 32), (1, 2, 25, 41), (4, 19, 46, 46),
          (2, 3, 64, 64), (1, 1, 129, 127), (8, 17, 64, 48)]


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_equals_the_rule(hip, shape):
    _kernel_equals_the_rule(hip, shape, offsets=(1, 2, 3) if shape == (3, 5, 7, 9) else ())


@pytest.mark.gpu
@pytest.mark.parametrize('delta', [-1, 0, 1])
def test_kernel_equals_the_rule_at_the_form_step(hip, delta):
    """Planes of T - 1, T and T + 1 elements for every H * W = T behind which the form query changes its answer; T is found through the
    query and asserted, so that a moved threshold fails here."""
    steps = _form_steps()
    assert steps == [WAVE_PLANE]
    for T in steps:
        size = T + delta
        assert hip.call(FORM, 1, size) == (FORM_WAVE if delta <= 0 else FORM_BLOCK)
        _kernel_equals_the_rule(hip, (3, 2, 1, size))          # (odd sizes: the planes start at every alignment)
        h = next(h for h in (3, 2, 5, 1) if size % h == 0)
        assert hip.call(FORM, h, size // h) == hip.call(FORM, 1, size)
        _kernel_equals_the_rule(hip, (2, 3, h, size // h))


@pytest.mark.gpu
def test_entry_rejects_what_it_cannot_do(hip):
    t = hip.DeviceTensor.from_numpy(np.arange(256, dtype=np.float32))
    o = hip.DeviceTensor.empty((512,), np.int32)
    p, a, b, c = ctypes.c_void_p(t.ptr), ctypes.c_void_p(o.ptr), ctypes.c_void_p(o.ptr + 256), ctypes.c_void_p(o.ptr + 512)
    good = [p, 2, 4, 4, 8, 1, 1, 0, 0.0, a, b, c]
    hip.call(ENTRY, *good)
    bads = [(0, None), (9, None), (10, None), (11, None)]                                  # a null pointer
    bads += [(at, bad) for at in (1, 2, 3, 4) for bad in (0, -1)]                           # n, K, H, W < 1
    bads += [(5, 2), (5, -1), (6, 2), (6, -1)]                                              # refine, space unknown
    bads += [(8, float('nan')), (8, float('inf')), (8, float('-inf'))]                      # min_score not finite
    for at, bad in bads:
        args = list(good)
        args[at] = bad
        with pytest.raises(hip.PvhipError):
            hip.call(ENTRY, *args)
        if at == 8:
            args[7] = 1
            with pytest.raises(hip.PvhipError):
                hip.call(ENTRY, *args)
    for n, K, H, W in ((2, 4, 1, 1), (1, 1, 4097, 4096), (1, 1, 1 << 16, 1 << 16), (1 << 16, 1 << 15, 1, 2), (1 << 30, 2, 1, 2), (2, 1 << 30, 2, 1)):
        with pytest.raises(hip.PvhipError):                    # H * W < 2, H * W > 2^24, n * K >= 2^31
            hip.call(ENTRY, p, n, K, H, W, 1, 1, 0, 0.0, a, b, c)
    hip.synchronize()
    x = np.arange(256, dtype=np.float32).reshape(2, 4, 4, 8)   # the device is still usable
    _same(_device_peaks(hip, x, 100.0, 'QUARTER', 'NORMALISED'), keypoints_ref.keypoints(x, 100.0), 'after the refusals')


@pytest.mark.gpu
def test_public_path(hip, tmp_path):
    """The truncated mnist network at batch 4 with two requests: keypoints= is the rule on the same request's own full Result in every
    form of the value; then a device-resident input five times with the keyword alternating, replayed from the request's one recording
    from the third call on."""
    from pyopenvino_amd import Keypoints, PeakScreen
    n = 4
    ex, net, name, out_name = _mnist_head(tmp_path, n, requests=2)
    req = ex.requests[0]
    x = _pixels(10, n)
    full = np.array(req.infer({name: x})[out_name], copy=True)
    assert full.shape == (n, 32, 26, 26) and full.dtype == np.float32 and np.isfinite(full).all()
    want = _ref(full)
    got = req.infer({name: x}, keypoints=True)
    assert set(got) == {out_name} and isinstance(got[out_name], Keypoints)
    _same(got[out_name], want, 'request')
    valid = ~np.isnan(got[out_name].points).any(axis=2)
    assert np.array_equal(got[out_name].counts, valid.sum(1)) and valid.all()
    _same(ex.infer({name: x}, keypoints=True)[out_name], want, 'the network\'s own infer()')
    _same(ex.requests[1].infer({name: x}, keypoints=True)[out_name], want, 'the second request')
    cut = _threshold(want.scores)
    assert (want.scores >= np.float32(cut)).sum() not in (0, want.scores.size)
    plain = PeakScreen(cut, 'NONE', 'HEATMAP')
    got = ex.infer({name: x}, keypoints={out_name: plain})[out_name]
    _same(got, _ref(full, plain._replace(min_score=float(np.float32(cut)))), 'a named PeakScreen')
    assert np.array_equal(got.counts, (want.scores >= np.float32(cut)).sum(1)) and (got.points[~np.isnan(got.points)] % 1 == 0).all()
    _same(ex.infer({name: x}, False, None, None, None, cut)[out_name], _ref(full, PeakScreen(float(np.float32(cut)))), 'a bare float')
    assert np.array_equal(ex.infer({name: x})[out_name], full)              # and whole again without the keyword
    # the same device-resident tensor five times
    xd = hip.DeviceTensor.from_numpy(x)
    kinds = [True, None, {out_name: plain}, True, None]
    first = {}
    for call, kind in enumerate(kinds):
        req.start_async({name: xd}, keypoints=kind)
        assert (req._replayed is not None) == (call >= 2), 'call {}'.format(call)
        res = req.wait()[out_name]
        if kind is None:
            assert isinstance(res, np.ndarray)
            helpers.assert_bit_exact(res, full, 'call {}: whole'.format(call))
        else:
            _same(res, want if kind is True else _ref(full, plain._replace(min_score=float(np.float32(cut)))), 'call {}: keypoints = {}'.format(call, kind))
        key = repr(kind)
        if key in first:
            if kind is None:
                helpers.assert_bit_exact(res, first[key], 'call {} vs the first of its kind'.format(call))
            else:
                _same(res, first[key], 'call {} vs the first of its kind'.format(call))
        else:
            first[key] = res if kind is not None else np.array(res, copy=True)
    assert ex._auto_graph['captured'] and ex._graph is not None              # one recording served every kind
    assert sorted(ex.answers.blocks) == [(out_name, 'NONE', 'HEATMAP'), (out_name, 'QUARTER', 'NORMALISED')]     # one per (name, refine, space): the float shared True's
    assert sorted(ex.requests[1].runner.answers.blocks) == [(out_name, 'QUARTER', 'NORMALISED')]
    ex.release_device_state()
    assert not ex.answers.blocks


@pytest.mark.gpu
def test_requests_in_flight(hip, tmp_path):
    """Two requests at batch 4, three steps, another input every time, the keyword cycling through True, a named PeakScreen and None
    per request and step: all started, then all waited for; every answer is the rule on that input's synchronous single-request Result."""
    from pyopenvino_amd import PeakScreen
    B, R, steps = 4, 2, 3
    ex, net, name, out_name = _mnist_head(tmp_path, B, requests=R)
    single, _, _, _ = _mnist_head(tmp_path, B)
    xs = [[_pixels(3000 + 100 * step + 10 * r, B) for r in range(R)] for step in range(steps)]
    fulls = [[np.array(single.infer({name: x})[out_name], copy=True) for x in row] for row in xs]
    assert len({f.tobytes() for row in fulls for f in row}) == R * steps
    plain = PeakScreen(0.5, 'NONE', 'HEATMAP')
    kinds = (True, {out_name: plain}, None)
    seen = set()
    for step in range(steps):
        asked = [(r + step) % 3 for r in range(R)]
        for r in range(R):
            ex.start_async(r, {name: xs[step][r]}, keypoints=kinds[asked[r]])
        for r in (reversed(range(R)) if step % 2 else range(R)):
            res = ex.wait(r)[out_name]
            seen.add((r, asked[r]))
            if asked[r] == 2:
                helpers.assert_bit_exact(res, fulls[step][r], 'step {} request {}'.format(step, r))
            else:
                _same(res, _ref(fulls[step][r], plain if asked[r] else None), 'step {} request {} kind {}'.format(step, r, asked[r]))
    assert len(seen) == R * 3                                 # every request gave every kind of answer


@pytest.mark.gpu
def test_cascade_rows_behind_count_are_void(hip, tmp_path):
    """GoogLeNet's first Convolution + bias + ReLU at batch 8 as a heatmap network (8, 64, 112, 112), fed DetectedRois(frames, a records
    array) with fewer survivors than rows: all eight rows equal the rule on the full Result of the same feed bit for bit -- the rows
    behind `count` are NaN rows: counts 0, points quiet NaN --, and detected_rois() still reads its table afterwards."""
    from pyopenvino_amd import DetectedRois, IECore
    rng = np.random.default_rng(501)
    n, m, hw, kind = 8, 2, (480, 640), 'U8-NHWC'
    frames = roi_tests._frames(rng, kind, m, hw)
    rec = det_tests._random_records(rng, m, 40, long=True)
    scores = np.sort(rec[:, 2][np.isfinite(rec[:, 2])])[::-1]
    want = None
    for conf in scores[2:40]:                                 # the highest threshold that leaves 3 .. 7 survivors
        want = det_tests.detected_rois(rec, n, m, hw, min_confidence=float(conf))
        if 3 <= want.count < n:
            break
    assert want is not None and 3 <= want.count == want.selected < n, (want.count, want.selected)
    conf = float(conf)
    ie = IECore(plugin_package=HIP)
    net = ie.read_network(_heatmap_head('googlenet-v1', tmp_path), weights=top_k_tests._blob(11))
    net.set_batch(n)
    name, out_name = net.inputs[0]['name'], net.outputs[0]['name']
    det_tests._declare(net, name, kind, mean=roi_tests._mean())
    ex = ie.load_network(net, 'GPU', num_requests=1)
    req = ex.requests[0]
    full = np.array(req.infer({name: DetectedRois(frames, rec, min_confidence=conf)})[out_name], copy=True)
    assert full.shape == (n, 64, 112, 112)
    det_tests._same(req.detected_rois(name), want, 'without keypoints')
    assert np.isfinite(full[:want.count]).all() and (_bits(full[want.count:]) == QUIET).all()
    got = req.infer({name: DetectedRois(frames, rec, min_confidence=conf)}, keypoints=True)[out_name]
    _same(got, _ref(full), 'cascade')
    assert (got.counts[:want.count] == 64).all() and np.isfinite(got.points[:want.count]).all()
    assert (got.counts[want.count:] == 0).all() and (_bits(got.points[want.count:]) == QUIET).all() and (got.positions[want.count:] == 0).all()
    det_tests._same(req.detected_rois(name), want, 'with keypoints')
