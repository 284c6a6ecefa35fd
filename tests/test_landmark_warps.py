"""Crops aligned by a landmark network's points, on the device (pyopenvino_amd.LandmarkWarps): the (n, 7) table of a WarpInput is fitted
by pvhip_landmarks_to_warps from another request's device-resident Result and the region table its pass was fed, bit for bit
tests/landmark_warps_ref.py and pyopenvino_amd/landmarks.py -- everything here is bit for bit, so no tolerance appears but the sanity
bound of the formula against np.linalg.lstsq.  The first tests need no GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import helpers
import landmark_warps_ref as ref
import test_warp_input as warp_tests
import warp_ref
from helpers import assert_bit_exact

ENTRY = 'pvhip_landmarks_to_warps'
VOID = (-1, 0, 0, 0, 0, 0, 0)
T5 = [(8, 8), (24, 8), (16, 16), (8, 24), (24, 24)]           # the template of the issue's check, for an extent of 32 x 32
T28 = [(8, 8), (20, 8), (14, 14), (9, 20), (19, 20)]          # five points in mnist's 28 x 28
FRAME, M_FRAMES = (480, 640), 3
_net, _declare, _frames, _fixed = warp_tests._net, warp_tests._declare, warp_tests._frames, warp_tests._fixed
# the void kinds a table of regions can hold, the ones whole frames can, and the planted row that stays valid
KINDS = ['nan', 'inf', 'id -1', 'id m', 'w 0', 'w 2^24 + 1', 'scale', 'translation', 'coincident']
WHOLE_KINDS = ['nan', 'inf', 'id m', 'scale', 'translation', 'coincident']


def _same(got, want, what=''):
    assert got.table.dtype == np.int64 and got.valid.dtype == np.bool_, what
    assert np.array_equal(got.table, want.table), (what, got.table.tolist(), want.table.tolist())
    assert np.array_equal(got.valid, want.valid) and got.count == want.count == int(want.valid.sum()), (what, got.valid, want.valid)


def _template(rng, K, extent=112):
    return T5 if K == 5 else rng.uniform(0, extent, (K, 2))


def _base(rng, N, K, m=M_FRAMES):
    """N rows of random points in [-0.2, 1.2] and regions inside one of m frames of FRAME: every row fits a modest similarity."""
    H, W = FRAME
    points = rng.uniform(-0.2, 1.2, (N, 2 * K)).astype(np.float32)
    w, h = rng.integers(20, 300, N), rng.integers(20, 300, N)
    regions = np.stack([rng.integers(0, m, N), rng.integers(0, W - 300, N), rng.integers(0, H - 300, N), w, h], 1).astype(np.int32)
    return points, regions


def _plant(points, regions, kind, b, m):
    """Row b of `points` (and `regions`, unless None: whole frames) made void in the way `kind` names, or valid with w = 2^24."""
    K = points.shape[1] // 2
    if kind == 'nan':
        points[b, (3 * b) % (2 * K)] = np.nan
    elif kind == 'inf':
        points[b, (5 * b + 1) % (2 * K)] = -np.inf if b % 2 else np.inf
    elif kind == 'id -1':
        regions[b, 0] = -1
    elif kind == 'id m':
        assert regions is None or m < 2 ** 31
        if regions is not None:
            regions[b, 0] = m
    elif kind == 'w 0':
        regions[b, 3 + b % 2] = 0
    elif kind == 'w 2^24 + 1':
        regions[b, 3 + b % 2] = (1 << 24) + 1
    elif kind == 'w 2^24':                                     # valid: the points stay within a few hundred pixels
        regions[b, 1:] = (0, 0, 1 << 24, 1 << 24)
        points[b] = np.float32(points[b] * 2.0 ** -16)
    elif kind == 'scale':                                      # the points spread over 3e5 pixels or more: |a| > 1024
        points[b] = np.float32(points[b] * 2.0 ** 14)
    elif kind == 'translation':                                # ... and lie 2^25 pixels and more from the origin: |c| > 2^24
        points[b] = np.float32(points[b] + 2.0 ** 21)
    elif kind == 'coincident':
        points[b, 0::2], points[b, 1::2] = points[b, 0], points[b, 1]
    else:
        raise AssertionError(kind)


def _planted(rng, N, K, table):
    """(points, regions or None, m, {row: kind}): the base with one row of every void kind its form can hold and the valid w = 2^24, on
    rows spread over [0, N); N == 1 holds none of them."""
    kinds = (KINDS + ['w 2^24']) if table else WHOLE_KINDS
    m = M_FRAMES if table else max(N - 2, 1)                   # whole frames: rows b >= m read no frame, the 'id m' kind
    points, regions = _base(rng, N, K)
    if not table:
        regions = None
    at = {}
    if N >= 2 * len(kinds):
        rows = [r for r in rng.permutation(N if table else m).tolist()][:len(kinds)]
        for b, kind in zip(rows, kinds):
            if kind != 'id m' or table:
                _plant(points, regions, kind, b, m)
                at[b] = kind
        if not table:
            at.update({b: 'id m' for b in range(m, N)})
    return points, regions, m, at


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
def test_dyadic_cases_come_back_exactly():
    """The issue's check and a few like it: points made from a matrix of dyadic values come back as that matrix, bit for bit, from the
    restatement and from landmarks.py -- a quarter turn at scale 2, scale 1/2, a half turn and the other quarter turn (a mirror through
    the centre, b < 0), and K = 2."""
    from pyopenvino_amd import LandmarkWarps, landmarks                 # noqa: F401 -- the rule specifies this input
    region = (0, 64, 32, 128, 64)
    cases = [(T5, [[0, -2, 100], [2, 0, 40]]), (T5, [[0.5, 0, 70.25], [0, 0.5, 40.5]]), (T5, [[-1, 0, 150], [0, -1, 90]]),
             (T5, [[0, 1.5, 80], [-1.5, 0, 88]]), ([(4, 4), (20, 12)], [[0.75, -0.25, 90], [0.25, 0.75, 50]]),
             ([(0, 0), (16, 0)], [[1, 0, 64], [0, 1, 32]])]
    for template, matrix in cases:
        u = ref.points_for(matrix, template, region)
        want = [0] + [int(v * 65536) for v in np.asarray(matrix, np.float64).reshape(-1)]
        assert all(float(v) * 65536 == int(v * 65536) for v in np.asarray(matrix, np.float64).reshape(-1))
        got = ref.landmark_warps(u[None], np.array([region]), template, FRAME, 1)
        assert got.table.tolist() == [want] and got.valid.tolist() == [True] and got.count == 1, (matrix, got.table.tolist())
        table, valid = landmarks.to_warps(u[None], np.array([region]), template, FRAME, 1)
        assert table.tolist() == [want] and valid.tolist() == [True] and table.dtype == np.int64 and valid.dtype == np.bool_
        frame_points = np.asarray(template, np.float64) @ np.asarray(matrix, np.float64)[:, :2].T + np.asarray(matrix, np.float64)[:, 2]
        assert np.array_equal(landmarks.similarity(frame_points, template), np.asarray(matrix, np.float64))
    assert ref.landmark_warps(ref.points_for(cases[0][1], T5, region)[None], np.array([region]), T5, FRAME, 1).table.tolist() == \
        [[0, 0, -131072, 6553600, 131072, 0, 2621440]]        # the issue's numbers, written out


@pytest.mark.parametrize('K', [2, 5, 32])
def test_to_warps_equals_the_restatement(K):
    from pyopenvino_amd import landmarks
    rng = np.random.default_rng(100 + K)
    template = _template(rng, K)
    assert_bit_exact(landmarks.packed_template(template).view(np.uint32), ref.packed(template).view(np.uint32), 'the packed template')
    assert landmarks.packed_template(template).shape == (2 * K + 3,)
    for N, n, table in ((40, 40, True), (40, 37, True), (40, 43, True), (40, 40, False), (1, 1, True), (1, 4, False), (7, 7, False)):
        points, regions, m, at = _planted(rng, N, K, table)
        want = ref.landmark_warps(points, regions, template, FRAME, m, n)
        for feed in (points, points.reshape(N, 2 * K, 1, 1)):
            got_table, got_valid = landmarks.to_warps(feed, regions, template, FRAME, m, rows=n)
            _same(ref.Fitted(int(got_valid.sum()), got_valid, got_table), want, (K, N, n, table))
        if N == 40:
            assert want.count >= N // 2
    one = ref.landmark_warps(*_base(rng, 6, K, 1), template, FRAME, 1)
    whole = ref.landmark_warps(_base(rng, 6, K)[0][:1], None, template, FRAME, 1)
    assert one.valid.all() and whole.table[0, 0] == 0 and whole.valid.all()


def test_similarity_is_the_least_squares_fit():
    """A sanity bound on the formula, not a device test: within 1e-9 of np.linalg.lstsq on the system [tx, -ty, 1, 0; ty, tx, 0, 1]."""
    from pyopenvino_amd import landmarks, warp
    rng = np.random.default_rng(9)
    for K in (2, 5, 32):
        template = _template(rng, K)
        t = np.asarray(template, np.float64)
        p = rng.uniform(0, 600, (K, 2))
        got = landmarks.similarity(p, template)
        rows = np.concatenate([np.stack([t[:, 0], -t[:, 1], np.ones(K), np.zeros(K)], 1), np.stack([t[:, 1], t[:, 0], np.zeros(K), np.ones(K)], 1)])
        a, b, c0, c1 = np.linalg.lstsq(rows, np.concatenate([p[:, 0], p[:, 1]]), rcond=None)[0]
        assert got.dtype == np.float64 and got.shape == (2, 3)
        assert np.abs(got - [[a, -b, c0], [b, a, c1]]).max() <= 1e-9
        exact = warp.apply(got, t)                             # an exact fit comes back
        assert np.abs(landmarks.similarity(exact, template) - got).max() <= 1e-9
    with pytest.raises(ValueError, match='one per template point'):
        landmarks.similarity(np.zeros((4, 2)), T5)
    with pytest.raises(ValueError, match='finite'):
        landmarks.similarity(np.full((5, 2), np.nan), T5)


@pytest.mark.parametrize('K', [2, 5, 32])
def test_every_void_condition_voids_exactly_its_own_row(K):
    from pyopenvino_amd import landmarks
    rng = np.random.default_rng(200 + K)
    template = _template(rng, K)
    N, m = 12, M_FRAMES
    points, regions = _base(rng, N, K)
    base = ref.landmark_warps(points, regions, template, FRAME, m)
    assert base.valid.all() and base.count == N and (base.table[:, 0] == regions[:, 0]).all()
    for kind in KINDS + ['w 2^24']:
        for b in (0, 5, N - 1):
            p, r = points.copy(), regions.copy()
            _plant(p, r, kind, b, m)
            got = ref.landmark_warps(p, r, template, FRAME, m)
            others = np.arange(N) != b
            assert np.array_equal(got.table[others], base.table[others]) and got.valid[others].all(), (kind, b)
            if kind == 'w 2^24':
                assert got.valid[b] and got.table[b, 0] == r[b, 0] and got.count == N
            else:
                assert not got.valid[b] and tuple(got.table[b]) == VOID and got.count == N - 1, (kind, b, got.table[b].tolist())
            table, valid = landmarks.to_warps(p, r, template, FRAME, m)
            _same(ref.Fitted(int(valid.sum()), valid, table), got, (kind, b))
    # the limits themselves are inside: a scale of exactly 1024 and a translation of exactly 2^24
    for matrix, region in (([[1024, 0, 0], [0, 1024, 0]], (0, 0, 0, 1 << 24, 1 << 24)),
                           ([[1, 0, 2.0 ** 24], [0, 1, -2.0 ** 24]], (0, 1 << 24, -(1 << 24), 64, 64))):
        t2 = [(0, 0), (16, 0)]
        u = ref.points_for(matrix, t2, region)                 # (exact, or it says so)
        got = ref.landmark_warps(u[None], np.array([region]), t2, FRAME, 1)
        assert got.valid.all() and got.table[0, 1:].tolist() == [int(v * 65536) for v in np.asarray(matrix, np.float64).reshape(-1)]
    # rows behind the rows of points
    got = ref.landmark_warps(points, regions, template, FRAME, m, N + 3)
    assert got.count == N and not got.valid[N:].any() and (got.table[N:] == VOID).all()
    # whole frames: m == 1 reads frame 0, else row b frame b, and rows b >= m are void
    assert ref.landmark_warps(points, None, template, FRAME, 1).table[:, 0].tolist() == [0] * N
    got = ref.landmark_warps(points, None, template, FRAME, N - 2)
    assert got.table[:, 0].tolist() == list(range(N - 2)) + [-1, -1] and got.count == N - 2


def test_template_rules():
    from pyopenvino_amd import landmarks
    for bad in (np.zeros((1, 2)), np.zeros((33, 2)), np.zeros((5, 3)), np.zeros(10), np.zeros((2, 5, 2))):
        with pytest.raises(ValueError, match=r'shape \(K, 2\)'):
            landmarks.packed_template(bad)
    for bad in (np.zeros((5, 2), bool), np.zeros((5, 2), complex), np.array([['a', 'b']] * 5)):
        with pytest.raises(ValueError, match='real numbers'):
            landmarks.packed_template(bad)
    for value in (np.nan, np.inf, -np.inf, 2.0 ** 24 + 2, -2.0 ** 25):
        t = np.array(T5, np.float64)
        t[3, 1] = value
        with pytest.raises(ValueError, match='finite values'):
            landmarks.packed_template(t)
    with pytest.raises(ValueError, match='two different points'):
        landmarks.packed_template([(3, 4)] * 5)
    edge = np.array(T5, np.float64)
    edge[0] = (2.0 ** 24, -2.0 ** 24)
    assert landmarks.packed_template(edge).shape == (13,)
    assert landmarks.packed_template(np.array(T5, np.int32)).tolist() == landmarks.packed_template(np.float32(T5)).tolist() \
        == [16.0, 16.0, 512.0, -8, -8, 8, -8, 0, 0, -8, 8, 8, 8]


def _mnist(batch, kind='U8-NCHW', requests=1, declare=True, fit=None):
    ie, net, name = _net('mnist', batch)
    if declare:
        _declare(net, name, kind, fit=fit)
    return ie.load_network(net, 'GPU', num_requests=requests), name, net.outputs[0]['name']


def test_argument_rules():
    """Everything is refused before anything is staged or launched (no device here), with the text 'input {name}: ...'."""
    from pyopenvino_amd import LandmarkWarps
    n, K = 3, 5
    ex, name, _ = _mnist(n, requests=2)
    req = ex.requests[0]
    frames = np.zeros((n, 1, 40, 36), np.uint8)
    good = np.zeros((n, 2 * K), np.float32)

    def refused(error, match, frames=frames, landmarks=good, template=T28, **opt):
        for start in (ex.infer, req.start_async, ex.requests[1].infer):
            with pytest.raises(error, match=match) as e:
                start({name: LandmarkWarps(frames, landmarks, template, **opt)})
            assert str(e.value).startswith('input {}: '.format(name)), str(e.value)

    for bad in (np.zeros((n, 10), np.float64), np.zeros((n, 10), np.float16), np.zeros((n, 10), np.int32), np.zeros(10, np.float32),
                np.zeros((n, 10, 1), np.float32), np.zeros((n, 10, 2, 1), np.float32), np.zeros((0, 10), np.float32),
                np.zeros((n, 5, 2), np.float32), [[0.0] * 10] * n):
        refused(ValueError, r'float32 points of shape \(N, 2 K\) or \(N, 2 K, 1, 1\)', landmarks=bad)
    refused(ValueError, 'the template of 5 points needs 10', landmarks=np.zeros((n, 12), np.float32))
    refused(ValueError, 'the template of 2 points needs 4', template=T28[:2])
    refused(ValueError, r'template has shape \(K, 2\)', template=T28[:1])
    refused(ValueError, 'template holds finite values', template=[(np.nan, 0)] + T28[1:])
    refused(ValueError, 'two different points', template=[(1, 1)] * 5)
    for bad in (np.zeros((n, 4), np.int32), np.zeros((n + 1, 5), np.int32), np.zeros((n, 5), np.float32), np.zeros(5, np.int32)):
        refused(ValueError, r'regions is an integer table of shape \(3, 5\)', regions=bad)
    refused(ValueError, '32-bit integers', regions=np.full((n, 5), 2 ** 31, np.int64))
    refused(ValueError, r'frame b for row b \(m == N\) or frame 0 \(m == 1\)', frames=np.zeros((2, 1, 40, 36), np.uint8))
    refused(ValueError, 'frames of a LandmarkWarps have shape', frames=np.zeros((n, 2, 40, 36), np.uint8))
    # a landmark request: an unknown output, a fitted input, an input last fed a warp, a request that never ran
    other, other_name, other_out = _mnist(n)
    source = other.requests[0]
    refused(ValueError, 'no Result named', landmarks=source, output='nope')
    refused(RuntimeError, 'never ran', landmarks=source)
    refused(RuntimeError, 'never ran', landmarks=source, output=other_out)
    source.runner.host_inputs.slots[other_name] = types.SimpleNamespace(last='warp')
    try:
        refused(ValueError, 'was last fed a WarpInput, a PerspectiveInput or a LandmarkWarps', landmarks=source)
    finally:
        del source.runner.host_inputs.slots[other_name]
    fitted, _, _ = _mnist(n, fit='LETTERBOX')
    refused(ValueError, 'declares resize_fit LETTERBOX', landmarks=fitted.requests[0])
    ie_g, net_g, _ = _net('googlenet-v1', n)
    refused(RuntimeError, 'never ran', landmarks=ie_g.load_network(net_g).requests[0])      # (no format declared there at all)
    # a sharded batch
    ex.comm = types.SimpleNamespace(world=2, rank=0)
    try:
        refused(NotImplementedError, 'sharded')
    finally:
        ex.comm = None
    assert not ex.host_inputs.slots and not ex.requests[1].runner.host_inputs.slots       # nothing was allocated
    with pytest.raises(KeyError):
        ex.infer({'no such input': LandmarkWarps(frames, good, T28)})
    with pytest.raises(KeyError):
        req.landmark_warps('no such input')
    with pytest.raises(RuntimeError, match='LandmarkWarps'):
        req.landmark_warps(name)
    # resize not declared: WarpInput's text
    plain, plain_name, _ = _mnist(n, declare=False)
    with pytest.raises(ValueError, match='a WarpInput is sampled on the device.*resize_algorithm') as e:
        plain.infer({plain_name: LandmarkWarps(np.zeros((n, 1, 28, 28), np.float32), good, T28)})
    assert str(e.value).startswith('input {}: '.format(plain_name)) and not plain.host_inputs.slots


def test_landmark_warps_is_refused_where_a_warp_input_is():
    from pyopenvino_amd import IECore, LandmarkWarps, RegionScreen, TiledScreen, synth
    blob = synth.synth_weights(os.path.join(helpers.MODELS, 'ssd_mobilenet_v1_coco.xml'), 1234)
    for fit in (None, 'LETTERBOX'):
        ie = IECore(plugin_package=warp_tests.HIP)
        net = ie.read_network(os.path.join(helpers.MODELS, 'ssd_mobilenet_v1_coco.xml'), weights=blob)
        net.set_batch(2)
        name = net.inputs[0]['name']
        _declare(net, name, 'U8-NHWC', reverse=True, fit=fit)
        ex = ie.load_network(net)
        fed = LandmarkWarps(np.zeros((2, 48, 64, 3), np.uint8), np.zeros((2, 10), np.float32), T5)
        if fit is None:
            with pytest.raises(ValueError, match='^detections: .*a TiledScreen needs input .* fed a RoiInput'):
                ex.infer({name: fed}, detections=TiledScreen())
        else:
            with pytest.raises(ValueError, match='^detections: .*declares resize_fit LETTERBOX and is fed a LandmarkWarps'):
                ex.infer({name: fed}, detections=0.5)
        with pytest.raises(ValueError, match='^detections: .*a RegionScreen needs input .* fed a RoiInput or a DetectedRois'):
            ex.infer({name: fed}, detections=RegionScreen())
        assert not ex.host_inputs.slots


def test_abi_declares_the_entry():
    import pyopenvino_amd
    from pyopenvino_amd import device, input_format
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert ENTRY in device.SIGNATURES and len(device.SIGNATURES[ENTRY][1]) == 11 and ENTRY not in device._NOT_STATUS
    m = re.search(r'\b' + ENTRY + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S)
    assert m and len(m.group(1).split(',')) == 11 and 'const double* tmpl' in m.group(1) and 'long long* table' in m.group(1)
    assert hasattr(device.load_library(), ENTRY)
    assert pyopenvino_amd.LandmarkWarps is input_format.LandmarkWarps and 'LandmarkWarps' in pyopenvino_amd.__all__
    assert input_format.LandmarkTable._fields == ('count', 'valid', 'table')


# ---------------------------------------------------------------------------------------------------------------- GPU
def _device_fit(hip, points, regions, template, n, m, frame_hw=FRAME):
    """The entry on `points`: the table and the valid block prefilled with 0x7f bytes, each with a guard row behind it."""
    N, K = points.shape[0], points.shape[1] // 2
    src = hip.DeviceTensor.from_numpy(np.ascontiguousarray(points, np.float32))
    reg = hip.DeviceTensor.from_numpy(np.ascontiguousarray(regions, np.int32)) if regions is not None else None
    tmpl = hip.DeviceTensor.from_numpy(ref.packed(template))
    table, valid = hip.DeviceTensor.empty((n + 1, 7), np.int64), hip.DeviceTensor.empty((n + 2,), np.int32)
    for t in (table, valid):
        hip.call('pvhip_memset', ctypes.c_void_p(t.ptr), 0x7f, t.nbytes)
    hip.call(ENTRY, ctypes.c_void_p(src.ptr), ctypes.c_void_p(reg.ptr) if reg is not None else None, ctypes.c_void_p(tmpl.ptr),
             ctypes.c_void_p(table.ptr), ctypes.c_void_p(valid.ptr), n, N, K, m, *frame_hw)
    t, v = np.asarray(table), np.asarray(valid)
    assert (t[n] == 0x7f7f7f7f7f7f7f7f).all() and v[n + 1] == 0x7f7f7f7f                  # nothing past the ends
    assert set(v[:n].tolist()) <= {0, 1}
    return ref.Fitted(int(v[n]), v[:n] != 0, t[:n].copy())


@pytest.mark.gpu
@pytest.mark.parametrize('table', [True, False], ids=['regions', 'whole frames'])
@pytest.mark.parametrize('K', [2, 5, 32])
def test_kernel_equals_the_rule(hip, K, table):
    """n in {1, 64, 65, 67} (one thread, a full workgroup, one and three threads of a second one) with rows in {n, n - 3, n + 3}; random
    points with one planted row of each void kind the form can hold -- a table of regions: all nine and the valid w = 2^24; whole frames
    (NULL) have no region to spoil, so there the six kinds of KINDS that remain, rows b >= m being the 'id m' kind."""
    rng = np.random.default_rng(300 + 2 * K + table)
    template = _template(rng, K)
    cases = []
    for n in (1, 64, 65, 67):
        for N in sorted({n, n - 3, n + 3}):
            if N >= 1:
                points, regions, m, at = _planted(rng, N, K, table)
                cases.append((n, N, points, regions, m, at, ref.landmark_warps(points, regions, template, FRAME, m, n)))
    # from the restatement alone: at least half the rows are valid and every void kind occurs
    seen = set()
    for n, N, points, regions, m, at, want in cases:
        assert want.count == int(want.valid.sum()) and (n == 1 or want.count >= n // 2), (n, N, want.count)
        for b, kind in at.items():
            if b < n:
                assert want.valid[b] == (kind == 'w 2^24') and (want.valid[b] or tuple(want.table[b]) == VOID), (n, N, b, kind)
                seen.add(kind)
        assert not want.valid[N:].any()
    assert seen == set(KINDS + ['w 2^24'] if table else WHOLE_KINDS), seen
    for n, N, points, regions, m, at, want in cases:
        _same(_device_fit(hip, points, regions, template, n, m), want, 'K = {}, n = {}, rows = {}'.format(K, n, N))


@pytest.mark.gpu
def test_kernel_returns_dyadic_matrices_exactly(hip):
    region = (2, 64, 32, 128, 64)
    u = ref.points_for([[0, -2, 100], [2, 0, 40]], T5, region)
    got = _device_fit(hip, u[None], np.array([region]), T5, 1, 3)
    assert got.table.tolist() == [[2, 0, -131072, 6553600, 131072, 0, 2621440]] and got.count == 1


@pytest.mark.gpu
def test_entry_rejects_what_it_cannot_do(hip):
    lib = hip.load_library()
    entry = getattr(lib, ENTRY)
    src = hip.DeviceTensor.from_numpy(np.zeros((4, 10), np.float32))
    reg = hip.DeviceTensor.from_numpy(np.tile(np.array([0, 0, 0, 8, 8], np.int32), (4, 1)))
    tmpl = hip.DeviceTensor.from_numpy(ref.packed(T5))
    table, valid = hip.DeviceTensor.from_numpy(np.full((4, 7), 7, np.int64)), hip.DeviceTensor.from_numpy(np.full(5, 7, np.int32))
    p = [ctypes.c_void_p(t.ptr) for t in (src, reg, tmpl, table, valid)]
    good = [4, 4, 5, 1, 48, 64]                                # n, rows, k, m, src_h, src_w
    for at in (0, 2, 3, 4):                                    # a NULL pointer other than regions
        args = list(p)
        args[at] = None
        assert entry(*args, *good) == -2, at
    for at, bad in ((0, 0), (0, -1), (1, 0), (2, 1), (2, 33), (2, 0), (3, 0), (4, 0), (5, 0), (4, (1 << 24) + 1), (5, (1 << 24) + 1)):
        args = list(good)
        args[at] = bad
        assert entry(*p, *args) == -2, (at, bad)               # PVHIP_EINVAL
    hip.synchronize()
    assert (np.asarray(table) == 7).all() and (np.asarray(valid) == 7).all()              # nothing was written
    assert entry(*p, *good) == 0 and entry(p[0], None, *p[2:], *good) == 0                # (and the same arguments in order are taken)
    edge = list(good)
    edge[4], edge[5] = 1 << 24, 1 << 24
    assert entry(p[0], None, *p[2:], *edge) == 0
    hip.synchronize()
    assert (np.asarray(table) == VOID).all() and np.asarray(valid).tolist() == [0, 0, 0, 0, 0]     # coincident points: every row void


def _points_near(rng, template, regions, frame_hw, dst, m):
    """Normalised fp32 points for every row: a rotated, scaled copy of the template inside the row's region, with a little noise."""
    from pyopenvino_amd import warp
    t = np.asarray(template, np.float64)
    out = []
    for b, (_, x, y, w, h) in enumerate(regions.tolist()):
        matrix = warp.rotated_rect(x + w * 0.5, y + h * 0.5, w * 0.8, h * 0.7, 25.0 - 40.0 * b, (dst, dst))
        pos = warp.apply(matrix, t) + rng.uniform(-0.7, 0.7, t.shape)
        out.append(np.stack([(pos[:, 0] + 0.5 - x) / w, (pos[:, 1] + 0.5 - y) / h], 1).reshape(-1))
    return np.float32(out)


def _through_warp_input(ex_ref, name, out_name, frames, table, hw):
    """What the cascade did before: the table through warp_buffer as a WarpInput, void rows replaced by the identity on frame 0:
    (the input tensor, the Result)."""
    from pyopenvino_amd import WarpInput
    req = ex_ref.requests[0]
    buf, tbuf = req.input_buffer(name, hw, frames=frames.shape[0]), req.warp_buffer(name)
    buf[...] = frames
    tbuf[...] = np.where((table[:, :1] < 0), np.array([[0, 65536, 0, 0, 0, 65536, 0]], np.int64), table)
    out = np.array(req.infer({name: WarpInput(buf, tbuf)})[out_name], copy=True)
    return _fixed(ex_ref, name), out


def _check_pass(ex, name, got_out, want, want_input, want_out, frames, ref_kind, dst, what, **opt):
    """The input tensor of the pass equals warp_ref over the restatement's table (void rows all NaN) and, on valid rows, the WarpInput's;
    so does the Result; landmark_warps() is the restatement."""
    fixed = _fixed(ex, name)
    v = want.valid
    assert_bit_exact(fixed[v], want_input[v], what + ': input rows of valid warps')
    assert_bit_exact(got_out[v], want_out[v], what + ': Results of valid warps')
    assert np.isnan(fixed[~v]).all() and np.isfinite(fixed[v]).all(), what
    assert_bit_exact(fixed, warp_tests._ref(ref_kind, frames, want.table, (dst, dst), **opt), what + ': the warp rule over the table')
    got = ex.requests[0].landmark_warps(name)
    assert isinstance(got.count, int)
    _same(got, want, what)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['FP32-NCHW', 'U8-NCHW'])
def test_mnist_from_arrays_of_landmarks(hip, kind):
    """mnist at batch 3 over one-channel frames of (40, 36): the points as a host array with a table of regions, as (N, 2 K, 1, 1) over
    whole frames, and as a DeviceTensor; one row void by a NaN."""
    from pyopenvino_amd import LandmarkWarps
    rng = np.random.default_rng(28 + len(kind))
    n, hw = 3, (40, 36)
    frames = _frames(rng, kind, n, hw, c=1)
    ex_ref, name, out_name = _mnist(n, kind)
    ex, _, _ = _mnist(n, kind)
    regions = np.array([(2, 4, 6, 28, 30), (0, 0, 0, 36, 40), (1, 10, 3, 20, 33)], np.int32)
    points = _points_near(rng, T28, regions, hw, 28, n)
    points[1, 3] = np.nan
    want = ref.landmark_warps(points, regions, T28, hw, n)
    assert want.valid.tolist() == [True, False, True]
    want_input, want_out = _through_warp_input(ex_ref, name, out_name, frames, want.table, hw)
    for step, feed in enumerate((points, points.reshape(n, 10, 1, 1), hip.DeviceTensor.from_numpy(points), points)):
        got_out = ex.infer({name: LandmarkWarps(frames, feed, T28, regions=regions if step != 2 else regions.astype(np.int64))})[out_name]
        _check_pass(ex, name, got_out, want, want_input, want_out, frames, kind, 28, '{} pass {}'.format(kind, step))
    # whole frames: row b reads frame b
    whole = _points_near(rng, T28, ref.whole_frames(n, hw, n), hw, 28, n)
    whole[2, 0] = np.inf
    want = ref.landmark_warps(whole, None, T28, hw, n)
    assert want.valid.tolist() == [True, True, False] and want.table[:2, 0].tolist() == [0, 1]
    want_input, want_out = _through_warp_input(ex_ref, name, out_name, frames, want.table, hw)
    got_out = ex.requests[0].infer({name: LandmarkWarps(frames, whole, np.array(T28, np.float32))})[out_name]
    _check_pass(ex, name, got_out, want, want_input, want_out, frames, kind, 28, kind + ' whole frames')
    # an input fed anything else afterwards has no table to read
    ex.infer({name: frames})
    with pytest.raises(RuntimeError, match='LandmarkWarps'):
        ex.requests[0].landmark_warps(name)


@pytest.mark.gpu
def test_googlenet_from_nv12_frames_and_arrays_of_landmarks(hip):
    from pyopenvino_amd import LandmarkWarps
    rng = np.random.default_rng(224)
    n, m, hw, kind = 2, 3, (96, 128), 'NV12'
    MEAN, STD, pad = warp_tests.MEAN, warp_tests.STD, 114.0
    frames = _frames(rng, kind, m, hw)
    template = (np.array(T28, np.float64) * 8).tolist()
    nets = []
    for _ in range(2):
        ie, net, name = _net('googlenet-v1', n)
        _declare(net, name, kind, reverse=True, mean=(MEAN, STD), pad=pad)
        nets.append(ie.load_network(net))
    ex_ref, ex = nets
    out_name = ex.ienet.outputs[0]['name']
    regions = np.array([(2, 30, 10, 70, 80), (1, 0, 0, 128, 96)], np.int32)
    points = _points_near(rng, template, regions, hw, 224, m)
    for void in (False, True):
        if void:
            regions[1, 0] = m
        want = ref.landmark_warps(points, regions, template, hw, m)
        assert want.valid.tolist() == [True, not void]
        want_input, want_out = _through_warp_input(ex_ref, name, out_name, frames, want.table, hw)
        got_out = ex.infer({name: LandmarkWarps(frames, points, template, regions=regions)})[out_name]
        _check_pass(ex, name, got_out, want, want_input, want_out, frames, kind, 224, 'googlenet NV12, void row: {}'.format(void),
                    reverse=True, mean=MEAN, std=STD, pad=pad)


def _chain_want(result, regions, frames, hw, m):
    """The restatement of one step of the chain: A's Result as five points per row over A's table (None: whole frames)."""
    want = ref.landmark_warps(np.asarray(result, np.float32), regions, T28, hw, m)
    return want, warp_ref.warp(frames, want.table, (28, 28), nhwc=False)


@pytest.mark.gpu
@pytest.mark.parametrize('fed', ['RoiInput', 'whole frames', 'DetectedRois'])
def test_chain_reads_the_landmark_request_in_flight(hip, fed):
    """Request A, mnist at batch 3, stands in for a landmark regressor: its (3, 10) softmax Result is five normalised points per row.
    A is started and not waited for; request B, a second mnist, is started on LandmarkWarps(frames, A, template); then both are waited
    for.  B's input equals the restatement computed from A's own Result, read after the wait, and the table A was fed -- a RoiInput's
    on the device, whole frames, and a DetectedRois' made on the device, whose rows behind count are void."""
    from pyopenvino_amd import DetectedRois, LandmarkWarps, RoiInput
    rng = np.random.default_rng(40 + len(fed))
    n, hw = 3, (40, 36)
    frames = _frames(rng, 'U8-NCHW', n, hw, c=1)
    a_net, a_name, a_out = _mnist(n)
    b_net, b_name, b_out = _mnist(n)
    A, B = a_net.requests[0], b_net.requests[0]
    rois = np.array([(1, 3, 5, 30, 31), (2, 0, 0, 36, 40), (0, 8, 2, 21, 37)], np.int32)
    records = np.array([[0, 1, 0.9, 0.1, 0.1, 0.9, 0.8], [-1, 0, 0, 0, 0, 0, 0], [0, 1, 0.8, 0.25, 0.2, 0.75, 0.9], [-1, 0, 0, 0, 0, 0, 0],
                        [-1, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0]], np.float32)         # images 0 and 1 hold one box each, image 2 none
    feed = {'RoiInput': lambda: RoiInput(frames, rois), 'whole frames': lambda: frames, 'DetectedRois': lambda: DetectedRois(frames, records)}[fed]
    for order in ('waited for', 'B first', 'A first', 'B first'):
        A.start_async({a_name: feed()})
        if order == 'waited for':                              # its host Results, like an array; its table still on the device
            result = A.wait()[a_out]
        B.start_async({b_name: LandmarkWarps(frames, A, T28)})
        if order == 'B first':
            got_out, result = B.wait()[b_out], A.wait()[a_out]
        elif order == 'A first':
            result, got_out = A.wait()[a_out], B.wait()[b_out]
        else:
            got_out = B.wait()[b_out]
        table = {'RoiInput': rois, 'whole frames': None, 'DetectedRois': None}[fed]
        if fed == 'DetectedRois':
            table = A.detected_rois(a_name).rois
            assert A.detected_rois(a_name).count == 2 and tuple(table[2]) == (-1, 0, 0, 0, 0)
        assert np.asarray(result).shape == (n, 10)
        want, want_input = _chain_want(result, table, frames, hw, n)
        assert want.valid.tolist() == ([True, True, False] if fed == 'DetectedRois' else [True] * 3), (order, want.table.tolist())
        _same(B.landmark_warps(b_name), want, '{}, {}'.format(fed, order))
        assert_bit_exact(_fixed(b_net, b_name), want_input, '{}, {}: B\'s input'.format(fed, order))
        assert np.isnan(_fixed(b_net, b_name)[~want.valid]).all() and np.isfinite(got_out[want.valid]).all()


@pytest.mark.gpu
def test_four_steps_landmark_request_restarted_at_once(hip):
    """New frames and a new ROI table every step; A is started on the next ones the moment B's start_async has returned (A's wait() is
    host-side bookkeeping: B is not waited for).  Every step's B input equals the restatement for that step's table: A's next stage()
    overwrites neither its table nor its Result before B's launch has read them."""
    from pyopenvino_amd import LandmarkWarps, RoiInput
    rng = np.random.default_rng(55)
    n, hw, steps = 3, (40, 36), 4
    frames = [_frames(rng, 'U8-NCHW', n, hw, c=1) for _ in range(steps)]
    rois = [np.stack([rng.permutation(n), rng.integers(0, 8, n), rng.integers(0, 8, n), rng.integers(12, 28, n), rng.integers(12, 32, n)], 1)
            .astype(np.int32) for _ in range(steps)]
    a_net, a_name, a_out = _mnist(n)
    b_net, b_name, b_out = _mnist(n, requests=2)
    A = a_net.requests[0]
    wants = []
    for f, r in zip(frames, rois):                             # the host route of every step
        result = np.array(A.infer({a_name: RoiInput(f, r)})[a_out], copy=True)
        wants.append((result,) + _chain_want(result, r, f, hw, n))
    assert len({w[1].table.tobytes() for w in wants}) == steps and all(w[1].valid.all() for w in wants)     # the steps differ
    A.start_async({a_name: RoiInput(frames[0], rois[0])})
    for step in range(steps):
        result, want, want_input = wants[step]
        B = b_net.requests[step % 2]
        B.start_async({b_name: LandmarkWarps(frames[step], A, T28)})
        assert_bit_exact(A.wait()[a_out], result, 'step {}: A'.format(step))
        if step + 1 < steps:
            A.start_async({a_name: RoiInput(frames[step + 1], rois[step + 1])})          # at once: B's pass may not even have begun
        B.wait()
        _same(B.landmark_warps(b_name), want, 'step {}'.format(step))
        assert_bit_exact(np.asarray(B.runner.host_inputs.slots[b_name].fixed), want_input, 'step {}: B\'s input'.format(step))
