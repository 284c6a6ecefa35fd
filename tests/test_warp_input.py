"""Affine warps as a network input (pyopenvino_amd.WarpInput): batch row b is frame ids[b] of m frames sampled through the 2 x 3 matrix
matrices[b] on the device in one launch (pvhip_input_preprocess_warp_f32), bit for bit tests/warp_ref.py.  The reference has no such
operation, so the restatement is first checked against facts that do not depend on it; those tests need no GPU."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import helpers
import packed_ref
import warp_ref
from helpers import MODELS, assert_bit_exact

HIP = 'pyopenvino_amd.op_plugins'
RAW = ['U8-NHWC', 'U8-NCHW', 'FP32-NHWC', 'FP32-NCHW']
YUV = ['NV12', 'I420']
PACKED = ['YUY2', 'UYVY', 'BGRX', 'RGBX']
KINDS = RAW + YUV + PACKED
BYTES = [k for k in KINDS if not k.startswith('FP32')]          # the kinds whose pixels are uint8
ENTRY = 'pvhip_input_preprocess_warp_f32'
FRAMES = [(48, 64), (6, 10)]                                  # both legal for every format
DESTS = [(13, 7), (22, 30), (16, 64)]                         # rows off 16-byte alignment and below one quad row; w % 4 != 0; aligned
IDS = [2, 0, 0, 1]
MEAN, STD = [104.0, 117.0, 123.0], [1.0, 57.5, 2.0]


def _is(kind):
    """(color, u8, nhwc) of a kind; a colour frame converts to a U8 NHWC image."""
    raw = kind in RAW
    return ('RAW' if raw else kind), (not raw or kind.startswith('U8')), (not raw or kind.endswith('NHWC'))


def _form(kind):
    """(format, how) of the entry."""
    color, u8, nhwc = _is(kind)
    if kind in YUV:
        return 1, int(kind == 'I420')
    if kind in PACKED:
        return 2, packed_ref.KINDS[kind]
    return 0, int(u8) | int(nhwc) << 1


def _frame_shape(kind, m, hw, c=3):
    h, w = hw
    if kind in YUV:
        return m, 3 * h // 2, w
    if kind in PACKED:
        return packed_ref.frame_shape(kind, m, hw)
    return (m, h, w, c) if kind.endswith('NHWC') else (m, c, h, w)


def _frames(rng, kind, m, hw, c=3, special=False, whole=False):
    """Random frames; FP32 kinds: `special` plants -0.0, inf and NaN, `whole` makes the values small whole numbers."""
    shape = _frame_shape(kind, m, hw, c)
    if not kind.startswith('FP32'):
        return rng.integers(0, 256, shape, dtype=np.uint8)
    f = (rng.integers(-300, 300, shape) if whole else rng.uniform(-300, 300, shape)).astype(np.float32)
    if special:
        flat = f.reshape(-1)
        at = rng.choice(flat.size, 3 * (flat.size // 16), replace=False).reshape(3, -1)
        flat[at[0]], flat[at[1]], flat[at[2]] = np.float32(-0.0), np.inf, np.nan
    return f


def _ref(kind, frames, table, dst_hw, **opt):
    color, _, nhwc = _is(kind)
    return warp_ref.warp(frames, table, dst_hw, nhwc, opt.get('reverse', False), opt.get('mean'), opt.get('std'), opt.get('pad', 0.0), color)


def _image(kind, frames):
    """(m, H, W, c) pixels of the frames, by the conversions of the existing references."""
    color, _, nhwc = _is(kind)
    return warp_ref.images(frames, nhwc, color)


def _translation(tx, ty, n=1):
    return np.array([[[1, 0, tx], [0, 1, ty]]] * n, np.float64)


def _table(matrices, ids):
    return warp_ref.table_of(matrices, ids)


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
@pytest.mark.parametrize('kind', KINDS)
def test_restatement_integer_translation_and_mirror_are_slices(kind):
    """An integer translation is the slice of the (converted) frame bit for bit -- fp32 frames hold -0.0, inf and NaN --, and
    A00 = -65536 the reversed slice."""
    rng = np.random.default_rng(11 + len(kind))
    hw, m = (48, 64), 3
    frames = _frames(rng, kind, m, hw, special=True)
    img = _image(kind, frames).astype(np.float32) if not kind.startswith('FP32') else _image(kind, frames)
    if kind.startswith('FP32'):
        assert np.isnan(img).any() and np.isinf(img).any() and (np.signbit(img) & (img == 0)).any()
    for (hd, wd), (tx, ty) in zip(DESTS, ((5, 3), (33, 26), (0, 31))):
        for i in range(m):
            want = img[i, ty:ty + hd, tx:tx + wd].transpose(2, 0, 1)
            got = _ref(kind, frames, _table(_translation(tx, ty), [i]), (hd, wd))
            assert_bit_exact(got[0], want, '{} translation ({}, {}) of frame {}'.format(kind, tx, ty, i))
            mirror = np.array([[[-1, 0, tx + wd - 1], [0, 1, ty]]], np.float64)
            assert warp_ref.fixed(mirror)[0, 0] == -65536
            got = _ref(kind, frames, _table(mirror, [i]), (hd, wd))
            assert_bit_exact(got[0], want[:, :, ::-1], '{} mirror of frame {}'.format(kind, i))
            got = _ref(kind, frames, _table(_translation(tx, ty), [i]), (hd, wd), reverse=True)
            assert_bit_exact(got[0], want[::-1], '{} translation, reversed channels'.format(kind))


@pytest.mark.parametrize('kind', BYTES)
def test_restatement_half_fraction_is_the_mean_of_two_bytes(kind):
    rng = np.random.default_rng(23 + len(kind))
    frames = _frames(rng, kind, 2, (48, 64))
    img = _image(kind, frames).astype(np.float32)
    (hd, wd), tx, ty = (22, 30), 7, 5
    half_x = warp_ref.table_of(_translation(tx + 0.5, ty), [1])
    assert half_x[0, 3] & 0xFFFF == 0x8000 and half_x[0, 6] & 0xFFFF == 0
    want = (img[1, ty:ty + hd, tx:tx + wd] + img[1, ty:ty + hd, tx + 1:tx + 1 + wd]) * np.float32(0.5)
    assert_bit_exact(_ref(kind, frames, half_x, (hd, wd))[0], want.transpose(2, 0, 1), kind + ' half a pixel along x')
    half_y = warp_ref.table_of(_translation(tx, ty + 0.5), [0])
    want = (img[0, ty:ty + hd, tx:tx + wd] + img[0, ty + 1:ty + 1 + hd, tx:tx + wd]) * np.float32(0.5)
    assert_bit_exact(_ref(kind, frames, half_y, (hd, wd))[0], want.transpose(2, 0, 1), kind + ' half a pixel along y')


@pytest.mark.parametrize('kind', KINDS)
def test_restatement_pads_exactly_where_taps_leave_the_frame(kind):
    """A row wholly outside is (pad - mean[k]) / std[k] everywhere; a row straddling every edge has pad taps exactly where ix, ix + 1,
    iy, iy + 1 leave the frame: it is the same warp of the frame embedded in a larger one filled with the pad."""
    rng = np.random.default_rng(37 + len(kind))
    hw, dst = (6, 10), (13, 17)
    H, W = hw
    frames = _frames(rng, kind, 2, hw, whole=True)
    img = _image(kind, frames).astype(np.float32)
    mean, std, pad = np.float32(MEAN), np.float32(STD), 114.0
    for matrix in (_translation(W, 0), _translation(0, H), _translation(-dst[1] - 1, 0), _translation(3, -dst[0] - 1),
                   _translation(W + 0.5, 2.25), np.array([[[1.7, 0.3, 40.0], [0.2, 1.1, -60.0]]])):
        got = _ref(kind, frames, _table(matrix, [1]), dst, mean=mean, std=std, pad=pad)
        for k in range(3):
            assert (got[0, k] == (np.float32(pad) - mean[k]) / std[k]).all(), (kind, matrix.tolist())
        assert (_ref(kind, frames, _table(matrix, [1]), dst) == 0).all()
    # the frame inside a border of pad: whole steps, then half steps on both axes ((p00 + p01 + p10 + p11) / 4, exact for whole values)
    B = 20
    big = np.full((H + 2 * B, W + 2 * B, 3), np.float32(pad))
    big[B:B + H, B:B + W] = img[0]
    tx, ty = -3, -2
    y0, x0 = B + ty, B + tx
    want = big[y0:y0 + dst[0], x0:x0 + dst[1]]
    assert (want[:, 0] == pad).all() and (want[0] == pad).all() and (want[-1] == pad).all() and (want[:, -1] == pad).all()
    assert_bit_exact(_ref(kind, frames, _table(_translation(tx, ty), [0]), dst, pad=pad)[0], want.transpose(2, 0, 1), kind + ' whole steps')
    quarter = (big[y0:y0 + dst[0], x0:x0 + dst[1]] + big[y0:y0 + dst[0], x0 + 1:x0 + 1 + dst[1]]) * np.float32(0.5)
    below = (big[y0 + 1:y0 + 1 + dst[0], x0:x0 + dst[1]] + big[y0 + 1:y0 + 1 + dst[0], x0 + 1:x0 + 1 + dst[1]]) * np.float32(0.5)
    want = (quarter + below) * np.float32(0.5)
    got = _ref(kind, frames, _table(_translation(tx + 0.5, ty + 0.5), [0]), dst, pad=pad)
    assert_bit_exact(got[0], want.transpose(2, 0, 1), kind + ' half steps over every edge')


def test_fixed_values_ties_and_limits():
    from pyopenvino_amd import WarpInput
    u = 1.0 / 65536
    m = np.array([[[1, 0, 3], [0, 1, 2]], [[-1, 0.5 * u, 1.5 * u], [2.5 * u, -0.5 * u, -1.5 * u]], [[1024, -1024, 2.0 ** 24], [0.3, -0.3, -2.0 ** 24]]])
    q = WarpInput.fixed(m)
    assert q.dtype == np.int64 and q.shape == (3, 6) and q.flags.c_contiguous
    assert q[0].tolist() == [65536, 0, 3 << 16, 0, 65536, 2 << 16]
    assert q[1].tolist() == [-65536, 0, 2, 2, 0, -2]           # ties to even, on both sides of zero
    assert q[2].tolist() == [1 << 26, -(1 << 26), 1 << 40, int(np.rint(0.3 * 65536)), -int(np.rint(0.3 * 65536)), -(1 << 40)]
    assert np.array_equal(q, warp_ref.fixed(m))
    for given in (m.astype(np.float32)[:1], m[:1].astype(np.int32), m[:1].tolist(), np.float16(m[:1])):
        assert WarpInput.fixed(given).tolist() == q[:1].tolist()
    assert WarpInput.fixed(np.zeros((0, 2, 3))).shape == (0, 6)
    ok = [[1, 0, 0], [0, 1, 0]]
    for j, bad in ((0, 1024 + u), (1, -1024 - u), (3, 2000.0), (4, -1e30), (2, 2.0 ** 24 + u), (5, -2.0 ** 24 - u), (2, 1e300),
                   (0, np.nan), (5, np.inf), (3, -np.inf)):
        rows = np.array([ok, ok, ok], np.float64)
        rows[1].reshape(-1)[j] = bad
        with pytest.raises(ValueError, match=r'matrices\[1\]'):
            WarpInput.fixed(rows)
        with pytest.raises(ValueError, match=r'matrices\[1\]'):
            warp_ref.fixed(rows)
    for shape in ((2, 3), (1, 3, 2), (1, 2, 4), (6,), (1, 1, 2, 3)):
        with pytest.raises(ValueError, match='shape'):
            WarpInput.fixed(np.zeros(shape))
    for dtype in (bool, complex, object, 'U3'):
        with pytest.raises(ValueError, match='real numbers'):
            WarpInput.fixed(np.zeros((1, 2, 3), dtype))


@functools.lru_cache(maxsize=None)
def _weights(model):
    from pyopenvino_amd import synth
    return None if model == 'mnist' else synth.synth_weights(os.path.join(MODELS, model + '.xml'), 7)


def _net(model='googlenet-v1', batch=1):
    from pyopenvino_amd import IECore
    ie = IECore(plugin_package=HIP)
    net = ie.read_network(os.path.join(MODELS, model + '.xml'), weights=_weights(model))
    if batch != 1:
        net.set_batch(batch)
    return ie, net, net.inputs[0]['name']


def _declare(net, name, kind, resize=True, reverse=False, mean=None, pad=None, fit=None):
    color, u8, nhwc = _is(kind)
    info = net.input_info[name]
    pre = info.preprocess_info
    if color != 'RAW':
        pre.color_format = color
    else:
        info.precision, info.layout = 'U8' if u8 else 'FP32', 'NHWC' if nhwc else 'NCHW'
    if resize:
        pre.resize_algorithm = 'RESIZE_BILINEAR'
    pre.reverse_channels = reverse
    if mean is not None:
        pre.init(len(mean[0]))
        for c in range(len(mean[0])):
            pre[c].mean_value, pre[c].std_scale = mean[0][c], mean[1][c]
        pre.mean_variant = 'MEAN_VALUE'
    if pad is not None:
        pre.pad_value = pad
    if fit is not None:
        pre.resize_fit = fit


@pytest.mark.parametrize('kind', KINDS)
def test_warp_input_argument_rules(kind):
    """The table the format makes of matrices and ids, the ids defaults, and every refusal -- by the format and by infer() with one
    text, before anything is allocated."""
    from pyopenvino_amd import WarpInput
    n, hw = 4, (48, 64)
    ie, net, name = _net(batch=n)
    _declare(net, name, kind)
    fmt = net.input_info[name].frozen()
    ex = ie.load_network(net)
    rng = np.random.default_rng(3)
    M = rng.uniform(-2, 2, (n, 2, 3))
    t = fmt.checked_matrices(WarpInput, M, IDS, 3)
    assert t.dtype == np.int64 and t.shape == (n, 7) and t.flags.c_contiguous
    assert t[:, 0].tolist() == IDS and np.array_equal(t[:, 1:], WarpInput.fixed(M)) and np.array_equal(t, warp_ref.table_of(M, IDS))
    assert fmt.checked_matrices(WarpInput, M, None, n)[:, 0].tolist() == [0, 1, 2, 3]            # m == n: row b reads frame b
    assert fmt.checked_matrices(WarpInput, M.tolist(), None, 1)[:, 0].tolist() == [0, 0, 0, 0]   # m == 1: every row reads the frame
    assert fmt.checked_matrices(WarpInput, M, np.array(IDS, np.uint8), 3)[:, 0].tolist() == IDS
    dtype = fmt.host_dtype

    def refused(match, matrices, ids, m):
        frames = np.zeros(_frame_shape(kind, m, hw), dtype)
        with pytest.raises(ValueError, match=match) as by_format:
            fmt.checked_matrices(WarpInput, matrices, ids, m)
        with pytest.raises(ValueError) as by_infer:
            ex.infer({name: WarpInput(frames, matrices, ids)})
        assert str(by_format.value) == str(by_infer.value) and str(by_infer.value).startswith('input {}: '.format(name))

    refused('without ids', M, None, 3)                        # neither m == n nor m == 1
    refused('without ids', M, None, 5)
    for ids in ([0, 1, 2, 3], [0, -1, 0, 0], np.array([0, 0, 2 ** 40, 0]), np.array([0, 0, 0, 2 ** 63], np.uint64)):
        refused(r'ids\[\d\] = .* none of 3 frames', M, ids, 3)
    for ids in ([0, 1, 2], [[0, 1, 2, 0]], [0.0, 1.0, 2.0, 0.0], [True, False, False, False], 2):
        refused('ids holds 4 integers', M, ids, 3)
    refused(r'one 2 x 3 matrix per batch row', M[:3], [0, 0, 0], 3)
    refused(r'shape \(n, 2, 3\)', M[0], IDS, 3)
    refused('real numbers', M > 0, IDS, 3)
    big = M.copy()
    big[2, 0, 1] = 1025.0
    refused(r'matrices\[2\] is beyond the limits', big, IDS, 3)
    big[2, 0, 1] = np.nan
    refused(r'matrices\[2\] is beyond the limits', big, IDS, 3)
    assert not ex.host_inputs.slots                           # nothing was allocated
    # a table already in the device's form (the warp_buffer): the same limits
    assert fmt.checked_matrix_table(WarpInput, t, 3) is t
    for column, value, match in ((1, (1 << 26) + 1, r'matrices\[2\]'), (2, -(1 << 26) - 1, r'matrices\[2\]'), (3, (1 << 40) + 1, r'matrices\[2\]'),
                                 (6, -(1 << 40) - 1, r'matrices\[2\]'), (5, np.iinfo(np.int64).min, r'matrices\[2\]'),
                                 (4, np.iinfo(np.int64).max, r'matrices\[2\]'), (0, 3, r'ids\[2\] = 3'), (0, -1, r'ids\[2\] = -1')):
        bad = t.copy()
        bad[2, column] = value
        with pytest.raises(ValueError, match='^input {}: {}'.format(name, match)):
            fmt.checked_matrix_table(WarpInput, bad, 3)
    for column, value in ((1, 1 << 26), (2, -(1 << 26)), (3, 1 << 40), (6, -(1 << 40))):     # the limits themselves are inside
        edge = t.copy()
        edge[2, column] = value
        fmt.checked_matrix_table(WarpInput, edge, 3)
    # the frames: RoiInput's checks
    ok = np.zeros(_frame_shape(kind, 3, hw), dtype)
    for shape in (ok.shape[1:], (0,) + ok.shape[1:], ok.shape + (1,)):
        with pytest.raises(ValueError, match='frames of a WarpInput') as by_infer:
            ex.infer({name: WarpInput(np.zeros(shape, dtype), M, IDS)})
        with pytest.raises(ValueError) as by_format:
            fmt.frames_extent_of(np.zeros(shape, dtype), WarpInput)
        assert str(by_format.value) == str(by_infer.value)
    with pytest.raises(KeyError):
        ex.infer({'no such input': WarpInput(ok, M, IDS)})
    with pytest.raises(KeyError):
        ex.requests[0].warp_buffer('no such input')
    assert not ex.host_inputs.slots


@pytest.mark.parametrize('kind', ['U8-NHWC', 'NV12', 'BGRX', None])
def test_warp_input_needs_a_declared_resize(kind):
    from pyopenvino_amd import WarpInput
    n, hw = 2, (224, 224)
    ie, net, name = _net(batch=n)
    if kind is not None:
        _declare(net, name, kind, resize=False)
    fmt = net.input_info[name].frozen()
    ex = ie.load_network(net)
    frames = np.zeros(_frame_shape(kind or 'FP32-NCHW', 1, hw), fmt.host_dtype)
    M = _translation(0, 0, n)
    with pytest.raises(ValueError, match='a WarpInput is sampled on the device.*resize_algorithm') as by_infer:
        ex.infer({name: WarpInput(frames, M)})
    for refused in (lambda: fmt.checked_matrices(WarpInput, M, None, 1), lambda: fmt.resize_declared(WarpInput), lambda: ex.requests[0].warp_buffer(name),
                    lambda: fmt.checked_matrix_table(WarpInput, np.zeros((n, 7), np.int64), 1)):
        with pytest.raises(ValueError) as by_format:
            refused()
        assert str(by_format.value) == str(by_infer.value)
    assert not ex.host_inputs.slots


def test_warp_input_is_refused_where_a_roi_input_is():
    """detections= on a fitted input fed a WarpInput is refused like a RoiInput there; a TiledScreen and a RegionScreen go on refusing
    anything but what they took; all before anything is staged."""
    from pyopenvino_amd import IECore, RegionScreen, TiledScreen, WarpInput, synth
    blob = synth.synth_weights(os.path.join(MODELS, 'ssd_mobilenet_v1_coco.xml'), 1234)
    for fit in (None, 'LETTERBOX'):
        ie = IECore(plugin_package=HIP)
        net = ie.read_network(os.path.join(MODELS, 'ssd_mobilenet_v1_coco.xml'), weights=blob)
        net.set_batch(2)
        name = net.inputs[0]['name']
        _declare(net, name, 'U8-NHWC', reverse=True, fit=fit)
        ex = ie.load_network(net)
        warp = WarpInput(np.zeros((2, 48, 64, 3), np.uint8), _translation(0, 0, 2))
        if fit is None:
            with pytest.raises(ValueError, match='^detections: .*a TiledScreen needs input .* fed a RoiInput'):
                ex.infer({name: warp}, detections=TiledScreen())
        else:
            with pytest.raises(ValueError, match='^detections: .*declares resize_fit LETTERBOX and is fed a WarpInput'):
                ex.infer({name: warp}, detections=0.5)
        with pytest.raises(ValueError, match='^detections: .*a RegionScreen needs input .* fed a RoiInput or a DetectedRois'):
            ex.infer({name: warp}, detections=RegionScreen())
        assert not ex.host_inputs.slots


def test_matrix_helpers():
    from pyopenvino_amd import WarpInput, warp
    rng = np.random.default_rng(5)
    for _ in range(20):
        M = rng.uniform(-3, 3, (2, 3))
        back = warp.invert(warp.invert(M))
        assert back.dtype == np.float64 and np.allclose(back, M, rtol=1e-9, atol=1e-9)
        pts = rng.uniform(-50, 50, (7, 2))
        assert np.allclose(warp.apply(warp.invert(M), warp.apply(M, pts)), pts, rtol=1e-9, atol=1e-7)
    assert np.array_equal(warp.apply([[2, 0, 1], [0, 3, -1]], [[0, 0], [1, 1]]), [[1, -1], [3, 2]])
    assert warp.apply(np.eye(2, 3), np.zeros((4, 5, 2))).shape == (4, 5, 2)
    for singular in ([[1, 2, 0], [2, 4, 1]], np.zeros((2, 3)), [[np.nan, 0, 0], [0, 1, 0]], [[np.inf, 0, 0], [0, 1, 0]]):
        with pytest.raises(ValueError, match='singular'):
            warp.invert(singular)
    for bad in (np.eye(3), np.zeros(6), np.zeros((1, 2, 3))):
        with pytest.raises(ValueError, match='2 x 3'):
            warp.invert(bad)
    # a rectangle of the network's extent is the integer translation
    hd, wd = 224, 300
    assert np.array_equal(warp.from_roi((11, 7, wd, hd), (hd, wd)), [[1, 0, 11], [0, 1, 7]])
    assert WarpInput.fixed([warp.from_roi((11, 7, wd, hd), (hd, wd))])[0].tolist() == [65536, 0, 11 << 16, 0, 65536, 7 << 16]
    # the half-pixel-centre rule: output pixel centre x + 1/2 lands at x0 + (x + 1/2) w / W, less the half pixel of the source's centres
    m = warp.from_roi((10, 20, 90, 60), (30, 30))
    assert np.array_equal(m, [[3.0, 0, 10 + 1.5 - 0.5], [0, 2.0, 20 + 1.0 - 0.5]])
    for roi in ((10, 20, 90, 60), (0.25, 1.5, 33.3, 17.1), (5, 5, 1, 1)):
        x, y, w, h = roi
        for dst in ((30, 30), (13, 7), (224, 224)):
            assert np.array_equal(warp.rotated_rect(x + w / 2, y + h / 2, w, h, 0, dst), warp.from_roi(roi, dst)), (roi, dst)
    # a quarter turn: the rectangle's x axis runs down the frame, and its corners map where the turned rectangle's lie
    q = warp.rotated_rect(50, 40, 20, 10, 90, (10, 20))
    assert np.allclose(q, [[0, -1, 50 + 5 - 0.5 - 0.5], [1, 0, 40 - 10 + 0.5 - 0.5]], atol=1e-12)
    corners = warp.apply(warp.rotated_rect(50, 40, 20, 10, 30, (10, 20)), [[-0.5, -0.5], [19.5, -0.5], [19.5, 9.5], [-0.5, 9.5]]) + 0.5
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    want = np.array([50, 40]) + np.array([[-10, -5], [10, -5], [10, 5], [-10, 5]]) @ np.array([[c, s], [-s, c]])
    assert np.allclose(corners, want, atol=1e-9)
    for bad in ((0, 0, 0, 5), (0, 0, 5, -1)):
        with pytest.raises(ValueError, match='every size'):
            warp.from_roi(bad, (8, 8))
    with pytest.raises(ValueError, match='every size'):
        warp.from_roi((0, 0, 5, 5), (0, 8))


def test_abi_declares_the_warp_entry():
    from pyopenvino_amd import device
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert ENTRY in device.SIGNATURES and len(device.SIGNATURES[ENTRY][1]) == 16 and ENTRY not in device._NOT_STATUS
    m = re.search(r'\b' + ENTRY + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S)
    assert m and len(m.group(1).split(',')) == 16 and 'const long long* table' in m.group(1) and 'float pad_value' in m.group(1)
    assert re.search(r'#define\s+PVHIP_ABI_VERSION\s+19\b', header)
    lib = device.load_library()
    assert hasattr(lib, ENTRY) and lib.pvhip_abi_version() == 19
    import pyopenvino_amd
    from pyopenvino_amd import input_format
    assert pyopenvino_amd.WarpInput is input_format.WarpInput and 'WarpInput' in pyopenvino_amd.__all__


# ---------------------------------------------------------------------------------------------------------------- GPU
def _matrix_set(hw, dst_hw):
    """Eight matrices in two tables of four rows (frames IDS): an integer translation, a mirror, a rotation by 30 degrees at scale 1.7
    about the frame's top right corner (it leaves the frame on two sides), a downscale of 3.3 with shear | a pure fractional
    translation, a row wholly outside, a negative C (SX < 0 over part of every row: floor, not truncation), a rotation by -75 degrees
    at scale 0.6."""
    from pyopenvino_amd import warp
    (H, W), (hd, wd) = hw, dst_hw
    turned = warp.rotated_rect(W - 1, 0.5, 1.7 * wd, 1.7 * hd, 30, dst_hw)
    src = warp.apply(turned, [[0, 0], [wd - 1, 0], [wd - 1, hd - 1], [0, hd - 1]])
    assert src[:, 0].max() > W and src[:, 1].min() < -1       # past the right and the top edge
    first = [[[1, 0, 3], [0, 1, 2]], [[-1, 0, W - 2], [0, 1, 1]], turned, [[3.3, 0.4, 1.25], [0.15, 3.3, 0.75]]]
    second = [[[1, 0, 2.37], [0, 1, 1.61]], [[1, 0, W + 5], [0, 1, 2]], [[1, 0, -2.75], [0, 1, -1.25]],
              warp.rotated_rect(W / 2, H / 2, 0.6 * wd, 0.6 * hd, -75, dst_hw)]
    tables = [_table(np.array(s, np.float64), IDS) for s in (first, second)]
    assert (tables[1][2, [3, 6]] < 0).all() and (tables[1][2, [3, 6]] & 0xFFFF != 0).all()
    return tables


class _Device:
    """Frames, a table, mean / std and a destination with guard floats on both sides, on the device."""

    def __init__(self, hip, frames, shift=0):
        frames = np.ascontiguousarray(frames)
        raw = np.zeros(frames.nbytes + shift, np.uint8)
        raw[shift:] = frames.view(np.uint8).reshape(-1)
        self.hip, self.tensor, self.src = hip, hip.DeviceTensor.from_numpy(raw), None
        self.src = self.tensor.ptr + shift
        self.mean, self.std = hip.DeviceTensor.from_numpy(np.float32(MEAN)), hip.DeviceTensor.from_numpy(np.float32(STD))

    def warp(self, kind, table, m, hw, dst_hw, c=3, guard=4, **opt):
        """The entry into a destination prefilled with 0x7f bytes: (the n images, the guard floats in front and behind)."""
        hip, n = self.hip, len(table)
        count = n * c * dst_hw[0] * dst_hw[1]
        whole = hip.DeviceTensor.empty((count + 2 * guard,))
        hip.call('pvhip_memset', ctypes.c_void_p(whole.ptr), 0x7f, whole.nbytes)
        t = hip.DeviceTensor.from_numpy(np.ascontiguousarray(table, np.int64))
        scaled = 'mean' in opt
        hip.call(ENTRY, ctypes.c_void_p(self.src), ctypes.c_void_p(whole.ptr + 4 * guard), ctypes.c_void_p(t.ptr), n, m, c, *hw, *dst_hw,
                 *_form(kind), int(opt.get('reverse', False)), ctypes.c_void_p(self.mean.ptr) if scaled else None,
                 ctypes.c_void_p(self.std.ptr) if scaled else None, opt.get('pad', 0.0))
        got = np.asarray(whole)
        return got[guard:guard + count].reshape((n, c) + tuple(dst_hw)), np.concatenate([got[:guard], got[guard + count:]])


OPTIONS = [dict(pad=0.0), dict(reverse=True, mean=MEAN, std=STD, pad=114.0)]


@pytest.mark.gpu
@pytest.mark.parametrize('hw', FRAMES)
@pytest.mark.parametrize('kind', KINDS)
def test_warp_kernel_bit_exact(hip, kind, hw):
    rng = np.random.default_rng(sum(hw) * 7 + len(kind) + KINDS.index(kind))
    m = 3
    frames = _frames(rng, kind, m, hw, special=kind.startswith('FP32'))
    dev = _Device(hip, frames)
    for dst_hw in DESTS:
        for table in _matrix_set(hw, dst_hw):
            for opt in OPTIONS:
                want = _ref(kind, frames, table, dst_hw, **opt)
                got, guards = dev.warp(kind, table, m, hw, dst_hw, **opt)
                for b in range(len(table)):                   # row by row: a failure names the matrix
                    assert_bit_exact(got[b], want[b], '{} {} -> {} {} row {} = {}'.format(kind, hw, dst_hw, sorted(opt), b, table[b].tolist()))
                assert (guards.view(np.uint32) == 0x7f7f7f7f).all()


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['U8-NHWC', 'YUY2', 'BGRX', 'NV12'])
def test_warp_kernel_bit_exact_from_unaligned_frames(hip, kind):
    """Frames one byte off 4-byte alignment: the packed kinds read their units byte by byte."""
    rng = np.random.default_rng(71 + len(kind))
    hw, m, dst_hw = (48, 64), 3, (22, 30)
    frames = _frames(rng, kind, m, hw)
    dev = _Device(hip, frames, shift=1)
    for table in _matrix_set(hw, dst_hw):
        got, _ = dev.warp(kind, table, m, hw, dst_hw, **OPTIONS[1])
        assert_bit_exact(got, _ref(kind, frames, table, dst_hw, **OPTIONS[1]), kind + ' one byte off alignment')


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['U8-NHWC', 'FP32-NCHW', 'I420', 'UYVY'])
def test_warp_kernel_writes_nan_for_a_row_of_no_frame(hip, kind):
    """A row with id = m (and one with id = -1) is quiet NaN in every plane, the other rows are what they were, and the guard floats
    in front of and behind `dst` keep their bits -- with `dst` on and off 16-byte alignment."""
    rng = np.random.default_rng(5 + len(kind))
    hw, m = (48, 64), 3
    frames = _frames(rng, kind, m, hw)
    dev = _Device(hip, frames)
    for dst_hw, guard in (((16, 64), 4), ((16, 64), 5), ((13, 7), 3), ((22, 30), 4)):
        table = _matrix_set(hw, dst_hw)[0]
        want = _ref(kind, frames, table, dst_hw, **OPTIONS[1])
        bad = table.copy()
        bad[1, 0], bad[3, 0] = m, -1
        got, guards = dev.warp(kind, bad, m, hw, dst_hw, guard=guard, **OPTIONS[1])
        assert np.isnan(got[1]).all() and np.isnan(got[3]).all()
        assert (got[[1, 3]].view(np.uint32) & 0x7fc00000 == 0x7fc00000).all()      # quiet
        assert_bit_exact(got[[0, 2]], want[[0, 2]], '{} rows beside the bad ones'.format(kind))
        assert_bit_exact(_ref(kind, frames, bad, dst_hw, **OPTIONS[1])[[0, 2]], want[[0, 2]], 'the restatement')
        assert len(guards) == 2 * guard and (guards.view(np.uint32) == 0x7f7f7f7f).all()


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_integer_translation_equals_the_roi_entries(hip, kind):
    """Against the code that was there before, not the restatement: for rectangles of exactly the destination's extent the warp entry
    with the integer translation gives the bits of the ROI entry of the format -- odd origins included."""
    rng = np.random.default_rng(101 + len(kind))
    hw, m = (48, 64), 3
    H, W = hw
    frames = _frames(rng, kind, m, hw, special=kind.startswith('FP32'))
    dev = _Device(hip, frames)
    mean, std = dev.mean, dev.std
    for hd, wd in DESTS:
        xs, ys = [1, 0, W - wd, (W - wd) // 2 | (1 if W - wd > 1 else 0)], [3, H - hd, 0, 5]
        rois = np.array([(IDS[b], min(xs[b], W - wd), ys[b], wd, hd) for b in range(4)], np.int32)
        table = _table(np.array([[[1, 0, x], [0, 1, y]] for _, x, y, _, _ in rois], np.float64), rois[:, 0])
        rt = hip.DeviceTensor.from_numpy(rois)
        for opt in OPTIONS:
            got, _ = dev.warp(kind, table, m, hw, (hd, wd), **opt)
            dst = hip.DeviceTensor.empty((4, 3, hd, wd))
            hip.call('pvhip_memset', ctypes.c_void_p(dst.ptr), 0x7f, dst.nbytes)
            scaled = 'mean' in opt
            where = (ctypes.c_void_p(dev.src), ctypes.c_void_p(dst.ptr), ctypes.c_void_p(rt.ptr), 4, m)
            tail = (int(opt.get('reverse', False)), ctypes.c_void_p(mean.ptr) if scaled else None, ctypes.c_void_p(std.ptr) if scaled else None)
            color, u8, nhwc = _is(kind)
            if kind in YUV:
                hip.call('pvhip_input_preprocess_yuv_roi_f32', *where, H, W, hd, wd, hd, wd, int(kind == 'I420'), *tail)
            elif kind in PACKED:
                hip.call('pvhip_input_preprocess_packed_roi_f32', *where, H, W, hd, wd, hd, wd, packed_ref.KINDS[kind], *tail)
            else:
                hip.call('pvhip_input_preprocess_roi_f32', *where, 3, H, W, hd, wd, hd, wd, int(u8), int(nhwc), *tail)
            assert_bit_exact(got, np.asarray(dst), '{} -> {} {}: rois {}'.format(kind, (hd, wd), sorted(opt), rois.tolist()))


@pytest.mark.gpu
def test_warp_entry_rejects_what_it_cannot_do(hip):
    lib = hip.load_library()
    src = hip.DeviceTensor.from_numpy(np.zeros(256, np.uint8))
    dst = hip.DeviceTensor.from_numpy(np.full(64, 7, np.float32))
    table = hip.DeviceTensor.from_numpy(_table(_translation(0, 0), [0]))
    s, d, t = ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), ctypes.c_void_p(table.ptr)
    entry = getattr(lib, ENTRY)
    good = (1, 1, 3, 4, 4, 2, 2, 0, 3, 0)                     # n, m, c, src_h, src_w, dst_h, dst_w, format, how, reverse

    def changed(**at):
        out = list(good)
        for k, v in at.items():
            out[int(k[1:])] = v
        return tuple(out)

    assert entry(s, d, None, *good, None, None, 0.0) == -2    # PVHIP_EINVAL, nothing launched: a NULL table
    for pad in (np.nan, np.inf, -np.inf):
        assert entry(s, d, t, *good, None, None, pad) == -2
    for args in (changed(_7=3), changed(_7=-1), changed(_7=1, _8=0, _2=1), changed(_7=1, _8=0, _2=4), changed(_7=2, _8=2, _2=4),
                 changed(_7=2, _8=0, _2=1),                   # format out of range; c != 3 for a colour format
                 changed(_8=4), changed(_8=-1), changed(_7=1, _8=2), changed(_7=2, _8=4),            # `how` out of range
                 changed(_7=1, _8=0, _3=3), changed(_7=1, _8=1, _4=3), changed(_7=2, _8=1, _4=3),    # odd extents of 4:2:0 and 4:2:2
                 changed(_0=0), changed(_0=70000), changed(_1=0), changed(_2=0), changed(_2=2000), changed(_3=0), changed(_4=0),
                 changed(_5=0), changed(_6=0), changed(_3=40000, _4=40000), changed(_5=40000, _6=40000)):
        assert entry(s, d, t, *args, None, None, 0.0) == -2, args
    assert entry(None, d, t, *good, None, None, 0.0) == -2
    assert entry(s, None, t, *good, None, None, 0.0) == -2
    assert entry(ctypes.c_void_p(src.ptr + 1), d, t, *changed(_8=2), None, None, 0.0) == -2          # fp32 off element alignment
    assert np.array_equal(np.asarray(dst), np.full(64, 7, np.float32))
    for args in (good, changed(_7=1, _8=0), changed(_7=1, _8=1), changed(_7=2, _8=0), changed(_7=2, _8=3), changed(_7=2, _8=2, _4=3)):
        assert entry(s, d, t, *args, None, None, 0.0) == 0, args                 # (and the same arguments in order are taken)


def _fixed(ex, name):
    return np.asarray(ex.host_inputs.slots[name].fixed).copy()


def _face_matrices(hw, dst_hw, n):
    """n rotated, scaled rectangles, the second one leaving the frame."""
    from pyopenvino_amd import warp
    H, W = hw
    return np.stack([warp.rotated_rect(W * (0.45 + 0.4 * b), H * 0.5, W * 0.7, H * 0.8, 20.0 - 50.0 * b, dst_hw) for b in range(n)], 0)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['U8-NHWC', 'NV12'])
def test_googlenet_from_warps_matches_the_restatement_fed_as_a_tensor(hip, kind):
    """infer({name: WarpInput(frames, M)}) with mean / scale declared: the Results of a network without declared formats fed
    warp_ref's tensor, bit for bit, three passes in a row (the third replays the recording)."""
    from pyopenvino_amd import WarpInput
    rng = np.random.default_rng(224 + len(kind))
    n, m, hw = 2, 3, (96, 128)
    frames = _frames(rng, kind, m, hw)
    M, ids = _face_matrices(hw, (224, 224), n), [2, 0]
    pad = 114.0
    want_input = _ref(kind, frames, _table(M, ids), (224, 224), reverse=True, mean=MEAN, std=STD, pad=pad)
    assert (want_input[1, 0] == (np.float32(pad) - np.float32(MEAN[0])) / np.float32(STD[0])).any()    # pad taps are in it
    ie, net, name = _net('googlenet-v1', n)
    out_name = net.outputs[0]['name']
    want = np.array(ie.load_network(net).infer({name: want_input})[out_name], copy=True)
    assert np.isfinite(want).all()
    ie, net, name = _net('googlenet-v1', n)
    _declare(net, name, kind, reverse=True, mean=(MEAN, STD), pad=pad)
    ex = ie.load_network(net)
    untouched = frames.copy()
    for step in range(3):
        got = ex.infer({name: WarpInput(frames, M, ids)})[out_name]
        assert_bit_exact(_fixed(ex, name), want_input, '{} input tensor, pass {}'.format(kind, step))
        assert_bit_exact(got, want, '{} WarpInput through infer(), pass {}'.format(kind, step))
    assert np.array_equal(frames, untouched)
    req = ex.requests[0]
    assert_bit_exact(req.infer({name: WarpInput(frames, M.tolist(), np.array(ids))})[out_name], want, kind + ' through a request, as lists')


@pytest.mark.gpu
def test_mnist_from_one_channel_fp32_warps(hip):
    from pyopenvino_amd import WarpInput
    rng = np.random.default_rng(28)
    n, m, hw = 2, 1, (40, 36)
    frames = _frames(rng, 'FP32-NCHW', m, hw, c=1)
    M = _face_matrices(hw, (28, 28), n)
    mean = ([0.5], [2.0])
    table = _table(M, [0, 0])
    want_input = warp_ref.warp(frames, table, (28, 28), nhwc=False, mean=mean[0], std=mean[1])
    ie, net, name = _net('mnist', n)
    out_name = net.outputs[0]['name']
    want = np.array(ie.load_network(net).infer({name: want_input})[out_name], copy=True)
    ie, net, name = _net('mnist', n)
    info = net.input_info[name]
    info.precision, info.layout = 'FP32', 'NCHW'
    pre = info.preprocess_info
    pre.resize_algorithm = 'RESIZE_BILINEAR'
    pre.init(1)
    pre[0].mean_value, pre[0].std_scale = mean[0][0], mean[1][0]
    pre.mean_variant = 'MEAN_VALUE'
    ex = ie.load_network(net)
    for step in range(3):
        got = ex.infer({name: WarpInput(frames, M)})[out_name]       # m == 1: every row reads the frame
        assert_bit_exact(_fixed(ex, name), want_input, 'mnist input tensor, pass {}'.format(step))
        assert_bit_exact(got, want, 'mnist from warps, pass {}'.format(step))


@pytest.mark.gpu
def test_warp_buffer_feeds_without_a_host_copy(hip):
    from pyopenvino_amd import WarpInput
    rng = np.random.default_rng(77)
    n, m, hw = 2, 3, (96, 128)
    frames = _frames(rng, 'NV12', m, hw)
    M, ids = _face_matrices(hw, (224, 224), n), [1, 2]
    ie, net, name = _net('googlenet-v1', n)
    out_name = net.outputs[0]['name']
    _declare(net, name, 'NV12', mean=(MEAN, STD))
    ex = ie.load_network(net, 'GPU', num_requests=2)
    want = np.array(ex.infer({name: WarpInput(frames, M, ids)})[out_name], copy=True)
    want_input = _fixed(ex, name)
    assert_bit_exact(want_input, _ref('NV12', frames, _table(M, ids), (224, 224), mean=MEAN, std=STD), 'the rule')
    req = ex.requests[1]
    buf, tbuf = req.input_buffer(name, hw, frames=m), req.warp_buffer(name)
    assert buf.shape == (m, 144, 128) and buf.dtype == np.uint8
    assert tbuf.shape == (n, 7) and tbuf.dtype == np.int64 and tbuf.flags.c_contiguous and req.warp_buffer(name) is tbuf
    assert ex.requests[0].warp_buffer(name) is not tbuf
    slot = req.runner.host_inputs.slots[name]
    assert tbuf is slot.tables['warp'].host and buf is slot.extents[(hw, m)].host
    buf[...] = frames
    tbuf[...] = _table(M, ids)
    copies = []
    real = np.copyto
    np.copyto = lambda dst, *a, **k: (copies.append(dst), real(dst, *a, **k))[1]
    try:
        got = req.infer({name: WarpInput(buf, tbuf)})[out_name]
    finally:
        np.copyto = real
    assert not any(c is buf or c is tbuf for c in copies)     # neither the frames nor the table was copied on the host
    assert_bit_exact(got, want, 'WarpInput from the request buffers')
    assert_bit_exact(np.asarray(slot.fixed), want_input, 'its input tensor')
    assert len(slot.extents) == 1
    # a table in the buffer that breaks a limit: refused before anything is staged
    launched = []
    real_call = hip.call
    for column, value, match in ((2, (1 << 26) + 1, r'matrices\[1\] is beyond the limits'), (6, -(1 << 40) - 1, r'matrices\[1\] is beyond'),
                                 (3, np.iinfo(np.int64).min, r'matrices\[1\] is beyond'),
                                 (0, m, r'ids\[1\] = 3 is none of 3 frames'), (0, -1, r'ids\[1\] = -1')):
        tbuf[...] = _table(M, ids)
        tbuf[1, column] = value
        hip.call = lambda entry, *args: (launched.append(entry), real_call(entry, *args))[1]
        try:
            with pytest.raises(ValueError, match=match):
                req.infer({name: WarpInput(buf, tbuf)})
        finally:
            hip.call = real_call
    assert not [e for e in launched if 'input' in e or 'memcpy' in e], launched
    with pytest.raises(ValueError, match='ids is None'):
        req.infer({name: WarpInput(buf, tbuf, ids)})
    tbuf[...] = _table(M, ids)
    assert_bit_exact(req.infer({name: WarpInput(buf, tbuf)})[out_name], want, 'and the good table again')
