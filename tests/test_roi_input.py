"""Regions of interest as a network input (pyopenvino_amd.RoiInput): batch row b is the rectangle rois[b] = (id, x, y, w, h) of frame id
of m frames, cropped, resized, reversed and scaled on the device in one launch (pvhip_input_preprocess_roi_f32 / _yuv_roi_f32), bit for
bit tests/roi_ref.py.  The first tests need no GPU.  (Page-locked buffers need the device: what input_buffer(..., frames=m) and
roi_buffer return is checked in a GPU test, as test_host_input.py does for input_buffer; the shapes themselves are checked without one.)"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import helpers
import roi_ref
import yuv_ref
from helpers import MODELS, assert_bit_exact
from preprocess_ref import preprocess

HIP = 'pyopenvino_amd.op_plugins'
RAW = ['U8-NHWC', 'U8-NCHW', 'FP32-NHWC', 'FP32-NCHW']
YUV = ['NV12', 'I420']
KINDS = RAW + YUV
ENTRY, ENTRY_YUV = 'pvhip_input_preprocess_roi_f32', 'pvhip_input_preprocess_yuv_roi_f32'


def _is(kind):
    """(yuv, u8, nhwc) of a kind; a YUV frame converts to a U8 NHWC image."""
    return kind in YUV, kind in YUV or kind.startswith('U8'), kind in YUV or kind.endswith('NHWC')


def _frame_shape(kind, m, hw, c=3):
    yuv, _, nhwc = _is(kind)
    h, w = hw
    return (m, 3 * h // 2, w) if yuv else ((m, h, w, c) if nhwc else (m, c, h, w))


def _frames(rng, kind, m, hw):
    yuv, u8, _ = _is(kind)
    shape = _frame_shape(kind, m, hw)
    if yuv:
        h, w = hw
        return yuv_ref.frames_of(*yuv_ref.planes_from_bgr(rng.integers(0, 256, (m, h, w, 3), dtype=np.uint8)), kind)
    return rng.integers(0, 256, shape, dtype=np.uint8) if u8 else rng.uniform(-300, 300, shape).astype(np.float32)


def _ref(kind, frames, rois, dst_hw, **opt):
    yuv, _, nhwc = _is(kind)
    return roi_ref.preprocess_rois(frames, rois, dst_hw, nhwc, opt.get('reverse', False), opt.get('mean'), opt.get('std'),
                                   color=kind if yuv else 'RAW')


@functools.lru_cache(maxsize=None)
def _weights(model):
    from pyopenvino_amd import synth
    return None if model == 'mnist' else synth.synth_weights(os.path.join(MODELS, model + '.xml'), 7)


def _net(model='googlenet-v1', batch=1, blob=None):
    from pyopenvino_amd import IECore
    ie = IECore(plugin_package=HIP)
    net = ie.read_network(os.path.join(MODELS, model + '.xml'), weights=blob if blob is not None else _weights(model))
    if batch != 1:
        net.set_batch(batch)
    return ie, net, net.inputs[0]['name']


def _declare(net, name, kind, resize=True, reverse=False, mean=None):
    yuv, u8, nhwc = _is(kind)
    info = net.input_info[name]
    pre = info.preprocess_info
    if yuv:
        pre.color_format = kind
    else:
        info.precision, info.layout = 'U8' if u8 else 'FP32', 'NHWC' if nhwc else 'NCHW'
    if resize:
        pre.resize_algorithm = 'RESIZE_BILINEAR'
    pre.reverse_channels = reverse
    if mean is not None:
        pre.init(3)
        for c in range(3):
            pre[c].mean_value, pre[c].std_scale = mean[0][c], mean[1][c]
        pre.mean_variant = 'MEAN_VALUE'


def _whole(n, hw, ids=None):
    h, w = hw
    return np.array([[b if ids is None else ids[b], 0, 0, w, h] for b in range(n)], np.int32)


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
@pytest.mark.parametrize('kind', KINDS)
def test_restatement_whole_frames_are_the_plain_preprocessing(kind):
    yuv, _, nhwc = _is(kind)
    rng = np.random.default_rng(len(kind))
    mean, std = [104.0, 117.0, 123.0], [1.0, 57.5, 2.0]
    for hw, dst in (((48, 64), (22, 30)), ((22, 30), (22, 30)), ((6, 10), (13, 7))):
        frames = _frames(rng, kind, 4, hw)
        image = yuv_ref.to_bgr(frames, kind) if yuv else frames
        for opt in (dict(), dict(reverse=True, mean=mean, std=std)):
            want = preprocess(image, dst, nhwc=nhwc, reverse_channels=opt.get('reverse', False), mean=opt.get('mean'), std_scale=opt.get('std'))
            assert_bit_exact(_ref(kind, frames, _whole(4, hw), dst, **opt), want, '{} {} -> {}'.format(kind, hw, dst))
            order = [3, 0, 0, 2]                              # any row of any frame, a frame twice, a frame never
            assert_bit_exact(_ref(kind, frames, _whole(4, hw, order), dst, **opt), want[order], '{} reordered'.format(kind))


@pytest.mark.parametrize('kind', KINDS)
def test_restatement_sees_nothing_outside_the_rectangle(kind):
    yuv, _, nhwc = _is(kind)
    rng = np.random.default_rng(7 + len(kind))
    H, W = 48, 64
    frames = _frames(rng, kind, 2, (H, W))
    # even and odd origins and sizes; for YUV the overwritten chroma stays clear of the 2 x 2 blocks the rectangle touches
    for roi in ((1, 10, 8, 20, 14), (1, 11, 9, 21, 13), (0, 0, 0, 5, 7), (0, W - 9, H - 7, 9, 7), (1, 31, 17, 1, 1)):
        i, x, y, w, h = roi
        table = np.array([roi], np.int64)
        want = _ref(kind, frames, table, (15, 19), reverse=True)
        other = _frames(rng, kind, 2, (H, W))
        if yuv:
            yp, up, vp = (p.copy() for p in yuv_ref.planes(frames, kind))
            yo, uo, vo = yuv_ref.planes(other, kind)
            keep = np.zeros((2, H, W), bool)
            keep[i, y:y + h, x:x + w] = True
            keep_c = np.zeros((2, H // 2, W // 2), bool)
            keep_c[i, y // 2:(y + h - 1) // 2 + 1, x // 2:(x + w - 1) // 2 + 1] = True
            changed = yuv_ref.frames_of(np.where(keep, yp, yo), np.where(keep_c, up, uo), np.where(keep_c, vp, vo), kind)
        else:
            changed = other
            if nhwc:
                changed[i, y:y + h, x:x + w, :] = frames[i, y:y + h, x:x + w, :]
            else:
                changed[i, :, y:y + h, x:x + w] = frames[i, :, y:y + h, x:x + w]
        assert not np.array_equal(changed, frames)
        assert_bit_exact(_ref(kind, changed, table, (15, 19), reverse=True), want, '{} {}'.format(kind, roi))


@pytest.mark.parametrize('color', YUV)
def test_restatement_odd_yuv_rectangle_is_the_crop_of_the_converted_image(color):
    rng = np.random.default_rng(420)
    frames = _frames(rng, color, 3, (38, 42))
    bgr = yuv_ref.to_bgr(frames, color)
    y, u, v = yuv_ref.planes(frames, color)
    for roi in ((2, 1, 1, 37, 35), (0, 5, 3, 7, 9), (1, 41, 37, 1, 1), (1, 3, 0, 2, 38)):
        i, x0, y0, w, h = roi
        got = roi_ref.crop(frames, roi, color=color)
        assert np.array_equal(got, bgr[i:i + 1, y0:y0 + h, x0:x0 + w])
        # the first pixel takes the chroma of its absolute block (y0 // 2, x0 // 2), whatever the parity of the origin
        assert got[0, 0, 0].tolist() == yuv_ref.convert(y[i, y0, x0], u[i, y0 // 2, x0 // 2], v[i, y0 // 2, x0 // 2]).tolist()
        for dst in ((h, w), (11, 13)):
            want = preprocess(bgr[i:i + 1, y0:y0 + h, x0:x0 + w], dst, reverse_channels=True)
            assert_bit_exact(roi_ref.preprocess_rois(frames, [roi], dst, reverse_channels=True, color=color), want, '{} {}'.format(color, roi))


def test_restatement_copies_a_rectangle_of_the_destination_extent():
    """Equal extents are skipped, not computed: an inf stays one pixel wide, where interpolation with weight 0 would make NaNs of its
    neighbours -- as it does when only one axis is equal."""
    frames = np.zeros((1, 12, 12, 1), np.float32)
    frames[0, 5, 6, 0] = np.inf
    same = roi_ref.preprocess_rois(frames, [(0, 2, 1, 8, 9)], (9, 8))
    assert np.isinf(same).sum() == 1 and same[0, 0, 4, 4] == np.inf and not np.isnan(same).any()
    one_axis = roi_ref.preprocess_rois(frames, [(0, 2, 1, 8, 9)], (9, 4))
    assert np.isnan(one_axis).any()


@pytest.mark.parametrize('kind', KINDS)
def test_roi_shape_and_table_rules(kind):
    """Frames of any count m in the declared format, and tables: what the format accepts, and every bad table and frames array refused
    with one text by the format and by infer(), before anything reaches the device."""
    from pyopenvino_amd import RoiInput
    yuv, u8, nhwc = _is(kind)
    n, H, W = 2, 48, 64
    ie, net, name = _net(batch=n)
    _declare(net, name, kind)
    info = net.input_info[name]
    fmt = info.frozen()
    dtype = np.dtype(np.uint8 if u8 else np.float32)
    for m in (1, 3, n, n + 5):
        shape = _frame_shape(kind, m, (H, W))
        assert fmt.host_shape((H, W), frames=m) == shape and fmt.host_dtype == dtype
        assert info.host_format((H, W), frames=m) == (shape, dtype)
        assert fmt.frames_extent_of(np.empty(shape, dtype)) == ((H, W), m)
        assert fmt.checked_frames(m) == m
    assert fmt.host_shape((H, W)) == _frame_shape(kind, n, (H, W)) == fmt.host_shape((H, W), frames=None)     # frames=None: as before
    for bad in (0, -1, 2.0, True, None, '3'):
        with pytest.raises(ValueError, match='m >= 1 frames'):
            fmt.checked_frames(bad)
    # a valid table, in any integer type: the int32 table and its largest (h, w)
    good = [[2, 1, 3, 5, 44], [0, 0, 0, W, H]] if not yuv else [[2, 1, 3, 5, 45], [0, 0, 0, W, H]]
    for table in (good, np.array(good, np.int64), np.array(good, np.uint8), np.array(good, np.int32)[:, ::1]):
        t, largest = fmt.checked_rois(table, (H, W), 3)
        assert t.dtype == np.int32 and t.shape == (n, 5) and t.flags.c_contiguous and t.tolist() == good and largest == (H, W)
    assert fmt.checked_rois([[0, 63, 47, 1, 1], [0, 3, 3, 7, 2]], (H, W), 1)[1] == (2, 7)
    ex = ie.load_network(net)
    m = 3
    frames = np.zeros(_frame_shape(kind, m, (H, W)), dtype)
    ok = [0, 0, 0, W, H]
    bad_tables = [np.zeros((n, 4), np.int32), np.zeros((n + 1, 5), np.int32), np.zeros(5, np.int32), np.zeros((1, n, 5), np.int32),
                  np.array([ok, ok], np.float32), np.array([ok, ok], np.float64), np.array([ok, ok]) > 0,
                  [ok, [m, 0, 0, W, H]], [[-1, 0, 0, W, H], ok],                          # id == m, id < 0
                  [ok, [0, -1, 0, 4, 4]], [ok, [0, 0, -1, 4, 4]],                         # a negative origin
                  [[0, 3, 3, 0, 4], ok], [ok, [0, 3, 3, 4, 0]], [ok, [0, 3, 3, -4, 4]],   # no size
                  [ok, [0, 1, 0, W, H]], [ok, [0, 0, 1, W, H]],                           # one pixel past the right, the bottom edge
                  [ok, [0, W, 0, 1, 1]], [[0, 0, H, 1, 1], ok],
                  np.array([ok, [0, 0, 0, 2 ** 40, 1]], np.int64), np.array([ok, [0, 2 ** 63, 0, 1, 1]], np.uint64)]
    for table in bad_tables:
        with pytest.raises(ValueError) as by_format:
            fmt.checked_rois(table, (H, W), m)
        with pytest.raises(ValueError) as by_infer:
            ex.infer({name: RoiInput(frames, table)})
        assert str(by_format.value) == str(by_infer.value), table
        assert str(by_format.value).startswith('input {}: '.format(name)), str(by_format.value)
        assert 'rois' in str(by_format.value)
    assert not ex.host_inputs.slots                           # nothing was allocated
    # frames of other shapes: none, no batch axis, another layout / channel count, (YUV) a row count that is no 3 h / 2, an odd extent
    if yuv:
        bad_frames = [(0, 72, 64), (72, 64), (3, 48, 64, 3), (3, 73, 64), (3, 72, 63), (3, 0, 64)]
    else:
        bad_frames = [_frame_shape(kind, 0, (H, W)), _frame_shape(kind, 3, (H, W))[1:], _frame_shape(kind, 3, (H, W), c=4), (3, 72, 64),
                      _frame_shape(kind, 3, (0, W))]
    for shape in bad_frames:
        with pytest.raises(ValueError) as by_format:
            fmt.frames_extent_of(np.empty(shape, dtype))
        with pytest.raises(ValueError) as by_infer:
            ex.infer({name: RoiInput(np.empty(shape, dtype), np.array([ok, ok], np.int32))})
        assert str(by_format.value) == str(by_infer.value), shape
        assert str(by_format.value).startswith('input {}: '.format(name)), str(by_format.value)
    for frames_arg in (0, -3, 1.5, True):                     # refused before a buffer is allocated
        with pytest.raises(ValueError, match='m >= 1 frames'):
            ex.requests[0].input_buffer(name, (H, W), frames=frames_arg)
    if yuv:
        with pytest.raises(ValueError, match='even height and width'):
            ex.requests[0].input_buffer(name, (47, 64), frames=3)
    with pytest.raises(KeyError):
        ex.infer({'no such input': RoiInput(frames, np.array([ok, ok], np.int32))})
    with pytest.raises(KeyError):
        ex.requests[0].roi_buffer('no such input')
    assert not ex.host_inputs.slots


@pytest.mark.parametrize('kind', KINDS + [None])
def test_roi_input_needs_a_declared_resize(kind):
    """Without RESIZE_BILINEAR -- declared otherwise, or never declared at all -- a RoiInput is refused, naming what to declare."""
    from pyopenvino_amd import RoiInput
    n, H, W = 2, 224, 224
    ie, net, name = _net(batch=n)
    if kind is not None:
        _declare(net, name, kind, resize=False)
    fmt = net.input_info[name].frozen()
    ex = ie.load_network(net)
    shape = _frame_shape(kind or 'FP32-NCHW', 1, (H, W))
    frames = np.zeros(shape, fmt.host_dtype)
    table = _whole(n, (H, W), [0, 0])
    with pytest.raises(ValueError, match='resize_algorithm') as by_infer:
        ex.infer({name: RoiInput(frames, table)})
    assert str(by_infer.value).startswith('input {}: '.format(name))
    for refused in (lambda: fmt.checked_rois(table, (H, W), 1), lambda: fmt.frames_extent_of(frames), lambda: fmt.checked_frames(1),
                    lambda: ex.requests[0].input_buffer(name, (H, W), frames=1), lambda: ex.requests[0].roi_buffer(name),
                    lambda: net.input_info[name].host_format((H, W), frames=1)):
        with pytest.raises(ValueError, match='resize_algorithm') as by_format:
            refused()
        assert str(by_format.value) == str(by_infer.value)
    assert not ex.host_inputs.slots


def test_abi_declares_the_roi_entries():
    from pyopenvino_amd import device
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for entry, count in ((ENTRY, 17), (ENTRY_YUV, 15)):
        assert entry in device.SIGNATURES and len(device.SIGNATURES[entry][1]) == count
        m = re.search(r'\b' + entry + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S)
        assert m and len(m.group(1).split(',')) == count, entry
        assert entry not in device._NOT_STATUS                # a status, like every launch
    assert re.search(r'#define\s+PVHIP_ABI_VERSION\s+19\b', header)
    lib = device.load_library()
    assert hasattr(lib, ENTRY) and hasattr(lib, ENTRY_YUV) and lib.pvhip_abi_version() == 19
    import pyopenvino_amd
    from pyopenvino_amd import input_format
    assert pyopenvino_amd.RoiInput is input_format.RoiInput and 'RoiInput' in pyopenvino_amd.__all__


# ---------------------------------------------------------------------------------------------------------------- GPU
class _Source:
    """Frames on the device, `shift` bytes off 16-byte alignment, with `margin` whole frames of allocation on both sides."""

    def __init__(self, hip, frames, shift=0, margin=0):
        frames = np.ascontiguousarray(frames)
        self.shape, self.frame_bytes = frames.shape, frames.nbytes // frames.shape[0]
        raw = np.zeros(frames.nbytes + shift + 2 * margin * self.frame_bytes, np.uint8)
        first = shift + margin * self.frame_bytes
        raw[first:first + frames.nbytes] = frames.view(np.uint8).reshape(-1)
        self.tensor = hip.DeviceTensor.from_numpy(raw)
        self.ptr = self.tensor.ptr + first


def _roi_args(kind, src, n, m, dst_hw, largest, reverse):
    """(entry, the integer arguments between the pointers and mean / std)."""
    yuv, u8, nhwc = _is(kind)
    shape = src.shape
    if yuv:
        return ENTRY_YUV, (n, m, shape[1] // 3 * 2, shape[2], dst_hw[0], dst_hw[1], largest[0], largest[1], int(kind == 'I420'), int(reverse))
    c, hs, ws = (shape[3], shape[1], shape[2]) if nhwc else shape[1:]
    return ENTRY, (n, m, c, hs, ws, dst_hw[0], dst_hw[1], largest[0], largest[1], int(u8), int(nhwc), int(reverse))


def _device_rois(hip, kind, src, rois, dst_hw, m=None, largest=None, reverse=False, mean=None, std=None):
    """The ROI entry of `kind` on the _Source `src` into a destination prefilled with 0x7f bytes."""
    rois = np.ascontiguousarray(rois, np.int32)
    n = rois.shape[0]
    m = src.shape[0] if m is None else m
    largest = (int(rois[:, 4].max()), int(rois[:, 3].max())) if largest is None else largest
    table = hip.DeviceTensor.from_numpy(rois)
    dst = hip.DeviceTensor.empty((n, 3) + tuple(dst_hw))
    hip.call('pvhip_memset', ctypes.c_void_p(dst.ptr), 0x7f, dst.nbytes)
    mt = hip.DeviceTensor.from_numpy(np.asarray(mean, np.float32)) if mean is not None else None
    st = hip.DeviceTensor.from_numpy(np.asarray(std, np.float32)) if std is not None else None
    entry, ints = _roi_args(kind, src, n, m, dst_hw, largest, reverse)
    hip.call(entry, ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), ctypes.c_void_p(table.ptr), *ints,
             ctypes.c_void_p(mt.ptr) if mt is not None else None, ctypes.c_void_p(st.ptr) if st is not None else None)
    return np.asarray(dst)


def _table(hw, dst_hw):
    """16 rectangles over frames 0 and 1 of three (frame 2 is read by no row), each case there by construction.  The rows:
     0 a whole frame                          1 one pixel                            2 exactly the destination's extent, odd origin
     3 the destination's width only           4 the destination's height only        5 the top left corner (top and left edges)
     6 the right edge                         7 the bottom edge                      8 the bottom right corner, odd sizes
     9 odd origin, odd sizes                 10 an upscale of more than 4x          11 the largest downscale the frame allows (row 0 is
    12 row 9's rectangle again                  13 the left edge, top to bottom         one too; more than 4x: test_roi_kernel_large_frame)
    14 three rows, edge to edge              15 the last pixel of the frame"""
    H, W = hw
    hd, wd = dst_hw
    t = [(0, 0, 0, W, H), (1, 5, 7, 1, 1), (1, 3, 5, wd, hd), (0, 10, 21, wd, hd // 2 + 1), (0, 11, 20, wd - 17, hd), (1, 0, 0, 101, 77),
         (1, W - 99, 50, 99, 120), (0, 40, H - 55, 200, 55), (1, W - 33, H - 41, 33, 41), (0, 13, 17, 151, 133), (1, 101, 203, 31, 29),
         (1, 1, 1, W - 1, H - 1), (0, 13, 17, 151, 133), (0, 0, 0, 57, H), (1, 0, 100, W, 3), (0, W - 1, H - 1, 1, 1)]
    t = np.array(t, np.int32)
    assert roi_ref.valid(t, 16, 3, hw) and 2 not in t[:, 0]
    assert hd / t[10, 4] > 4 and wd / t[10, 3] > 4 and (t[2, 3:] == (wd, hd)).all()
    return t


def _poison(kind, frames, roi):
    """An inf and a NaN inside rectangle `roi` of fp32 frames (in place)."""
    i, x, y, w, h = (int(v) for v in roi)
    if kind.endswith('NHWC'):
        frames[i, y + h // 3, x + w // 2, 0], frames[i, y + h // 2, x + w // 3, 1] = np.inf, np.nan
    else:
        frames[i, 0, y + h // 3, x + w // 2], frames[i, 1, y + h // 2, x + w // 3] = np.inf, np.nan


def _options(rng):
    mean = rng.uniform(0, 255, 3).astype(np.float32)
    std = rng.uniform(0.5, 80, 3).astype(np.float32)
    return [dict(), dict(reverse=True, mean=mean, std=std), dict(reverse=True), dict(mean=mean), dict(std=std)]


def _check_kernel(hip, kind, frames, table, dst_hw, options, shifts, what):
    fp32 = kind.startswith('FP32')
    wants = [_ref(kind, frames, table, dst_hw, **opt) for opt in options]
    for shift in shifts:
        shift = 4 * shift if fp32 else shift                  # (fp32 sources are element-aligned: byte offsets 0, 4, 8, 12)
        src = _Source(hip, frames, shift)
        for opt, want in zip(options, wants):
            got = _device_rois(hip, kind, src, table, dst_hw, **opt)
            for b in range(len(table)):                       # row by row: a failure names the rectangle
                assert_bit_exact(got[b], want[b], '{} {} {} source offset {} row {} = {}'.format(kind, what, sorted(opt), shift, b, table[b].tolist()))


@pytest.mark.gpu
@pytest.mark.parametrize('src_hw,dst_hw', [((480, 640), (224, 224)), ((482, 642), (300, 300))])
@pytest.mark.parametrize('kind', KINDS)
def test_roi_kernel_bit_exact(hip, kind, src_hw, dst_hw):
    """Every format, option set and source offset over the 16 rectangles of _table.  Source offsets are bytes 0..3 for uint8 sources and
    0, 4, 8, 12 for fp32 ones (the entry refuses an fp32 source off element alignment).  These frames cannot hold a rectangle that is
    downscaled by more than 4x to these extents (640 / 224 = 2.9): the table takes the largest they hold, and
    test_roi_kernel_large_frame adds (960, 1280) frames for the rest."""
    rng = np.random.default_rng(sum(src_hw) * 31 + sum(dst_hw) * 3 + len(kind))
    frames = _frames(rng, kind, 3, src_hw)
    table = _table(src_hw, dst_hw)
    if kind.startswith('FP32'):
        _poison(kind, frames, table[2])
        copied = _ref(kind, frames, table[2:3], dst_hw)
        assert np.isinf(copied).sum() == 1 and np.isnan(copied).sum() == 1        # copied: neither spreads
    _check_kernel(hip, kind, frames, table, dst_hw, _options(rng), (0, 1, 2, 3), '{} -> {}'.format(src_hw, dst_hw))


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_roi_kernel_large_frame(hip, kind):
    """(960, 1280) frames to 224 x 224: rectangles that are downscaled by more than 4x on both axes, which the (480, 640) frames cannot
    hold, beside an upscale of more than 4x and a copy."""
    rng = np.random.default_rng(960 + len(kind))
    hw, dst_hw = (960, 1280), (224, 224)
    frames = _frames(rng, kind, 2, hw)
    table = np.array([(0, 0, 0, 1280, 960), (1, 1, 3, 1001, 921), (0, 279, 39, 1001, 921), (1, 700, 500, 31, 29), (1, 1055, 735, 224, 224),
                      (0, 1, 3, 1001, 921)], np.int32)
    assert (table[:3, 3] > 4 * 224).all() and (table[:3, 4] > 4 * 224).all()
    if kind.startswith('FP32'):
        _poison(kind, frames, table[4])
    _check_kernel(hip, kind, frames, table, dst_hw, _options(rng), (0, 1, 2, 3), '{} -> {}'.format(hw, dst_hw))


# Two source rows of one 14000-wide rectangle exceed the kernel's 48 KiB of LDS, so the output rows are split into column tiles that
# start at tx0 > 0 inside a crop, on even and on odd source columns; (3, 14000) -> (3, 14000) is the copy in column tiles.
@pytest.mark.gpu
@pytest.mark.parametrize('dst_hw', [(2, 224), (3, 14000)])
@pytest.mark.parametrize('kind', KINDS)
def test_roi_kernel_bit_exact_in_column_tiles(hip, kind, dst_hw):
    rng = np.random.default_rng(30000 + dst_hw[1] + len(kind))
    frames = _frames(rng, kind, 1, (4, 30000))
    table = np.array([(0, 1000, 0, 14000, 4), (0, 1001, 1, 14000, 3), (0, 16000, 0, 14000, 4), (0, 15999, 1, 14000, 2)], np.int32)
    if kind.startswith('FP32'):
        _poison(kind, frames, table[1])
    options = _options(rng)
    _check_kernel(hip, kind, frames, table, dst_hw, [options[1], options[0]], (0, 3), '(4, 30000) -> {}'.format(dst_hw))


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['U8-NHWC', 'U8-NCHW', 'NV12', 'I420'])
def test_whole_frame_table_matches_the_existing_entry_at_batch_256(hip, kind):
    """(256, 480, 640) frames -> 224 x 224 with rois[b] = (b, 0, 0, 640, 480): the bits of the entry without a table, device to device."""
    yuv, u8, nhwc = _is(kind)
    rng = np.random.default_rng(256 + len(kind))
    n, hw, dst_hw = 256, (480, 640), (224, 224)
    frames = rng.integers(0, 256, _frame_shape(kind, n, hw), dtype=np.uint8)
    src = _Source(hip, frames)
    mean, std = [104.0, 117.0, 123.0], [1.0, 57.5, 2.0]
    mt, st = hip.DeviceTensor.from_numpy(np.asarray(mean, np.float32)), hip.DeviceTensor.from_numpy(np.asarray(std, np.float32))
    for opt in (dict(), dict(reverse=True, mean=mean, std=std)):
        got = _device_rois(hip, kind, src, _whole(n, hw), dst_hw, **opt)
        dst = hip.DeviceTensor.empty((n, 3) + dst_hw)
        hip.call('pvhip_memset', ctypes.c_void_p(dst.ptr), 0x7f, dst.nbytes)
        tail = (int(bool(opt)), ctypes.c_void_p(mt.ptr) if opt else None, ctypes.c_void_p(st.ptr) if opt else None)
        if yuv:
            hip.call('pvhip_input_preprocess_yuv_f32', ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), n, *hw, *dst_hw, int(kind == 'I420'), *tail)
        else:
            hip.call('pvhip_input_preprocess_f32', ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), n, 3, *hw, *dst_hw, 1, int(nhwc), *tail)
        want = np.asarray(dst)
        assert not np.isnan(want).any()
        assert_bit_exact(got, want, '{} whole-frame table, {}'.format(kind, sorted(opt)))
        del dst, got, want


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_roi_kernel_writes_nan_for_an_invalid_rectangle(hip, kind):
    """The table is device data: a row whose rectangle is not inside a frame, or exceeds the stated maxima, comes back all quiet NaN and
    its neighbours exact.  The source has a margin of a whole frame on both sides, and no rectangle here leaves that allocation."""
    rng = np.random.default_rng(99 + len(kind))
    m, hw, dst_hw = 3, (48, 64), (20, 28)
    H, W = hw
    frames = _frames(rng, kind, m, hw)
    src = _Source(hip, frames, margin=1)
    good = [(0, 3, 5, 30, 20), (2, 1, 1, 40, 30), (1, 0, 0, W, H)]
    largest = (30, 40)                                        # the stated maxima: the whole frame (row 8) exceeds them
    bad = [(1, 0, 0, 41, 30), (1, 0, 0, 40, 31), (0, 4, 4, 0, 5), (0, 4, 4, 5, 0), (m, 3, 5, 30, 20), (-1, 3, 5, 30, 20), (1, W - 29, 5, 30, 20),
           (1, 3, H - 19, 30, 20), (1, -1, 5, 30, 20), (1, 3, -1, 30, 20), (1, 3, 5, -30, 20), (1, 0, 0, W, H)]
    table = np.array([good[0], bad[0], bad[1], good[1], bad[2], bad[3], bad[4], good[0], bad[5], bad[6], bad[7], good[1], bad[8], bad[9],
                      bad[10], bad[11], good[1]], np.int32)
    valid_rows = [b for b in range(len(table)) if tuple(table[b]) in good[:2]]
    assert len(valid_rows) == 5
    want = _ref(kind, frames, table[valid_rows], dst_hw, reverse=True)
    got = _device_rois(hip, kind, src, table, dst_hw, m=m, largest=largest, reverse=True)
    for b in range(len(table)):
        if b in valid_rows:
            assert_bit_exact(got[b], want[valid_rows.index(b)], '{} row {} beside invalid ones'.format(kind, b))
        else:
            assert np.isnan(got[b]).all(), '{} row {} = {} is not all NaN'.format(kind, b, table[b].tolist())
    # with the frame as the stated maximum the whole frame is valid again
    got = _device_rois(hip, kind, src, np.array([good[2], bad[6]], np.int32), dst_hw, m=m, largest=hw)
    assert_bit_exact(got[0], _ref(kind, frames, [good[2]], dst_hw)[0], kind + ' whole frame')
    assert np.isnan(got[1]).all()


@pytest.mark.gpu
def test_roi_kernels_reject_what_they_cannot_do(hip):
    lib = hip.load_library()
    src = hip.DeviceTensor.from_numpy(np.zeros(256, np.uint8))
    dst = hip.DeviceTensor.from_numpy(np.full(64, 7, np.float32))
    rois = hip.DeviceTensor.from_numpy(np.array([[0, 0, 0, 2, 2]], np.int32))
    s, d, r = ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), ctypes.c_void_p(rois.ptr)
    raw, yuv = getattr(lib, ENTRY), getattr(lib, ENTRY_YUV)
    good_raw = (1, 1, 3, 4, 4, 2, 2, 2, 2, 1, 1, 0)           # n, m, c, src_h, src_w, dst_h, dst_w, max_roi_h, max_roi_w, u8, nhwc, reverse
    good_yuv = (1, 1, 4, 4, 2, 2, 2, 2, 0, 0)                 # n, m, src_h, src_w, dst_h, dst_w, max_roi_h, max_roi_w, planar, reverse

    def changed(args, **at):
        out = list(args)
        for k, v in at.items():
            out[int(k[1:])] = v
        return tuple(out)

    # m < 1, max_roi_* < 1 or above the frame, and what the entries without a table refuse: n, c, empty extents, an image past 2^31
    for args in ([changed(good_raw, _1=0), changed(good_raw, _1=-1), changed(good_raw, _7=0), changed(good_raw, _8=0), changed(good_raw, _7=5),
                  changed(good_raw, _8=5), changed(good_raw, _7=-1), changed(good_raw, _0=0), changed(good_raw, _0=70000), changed(good_raw, _2=0),
                  changed(good_raw, _2=2000), changed(good_raw, _3=0), changed(good_raw, _4=0), changed(good_raw, _5=0), changed(good_raw, _6=0),
                  changed(good_raw, _3=40000, _4=40000, _7=2, _8=2), changed(good_raw, _5=40000, _6=40000)]):
        assert raw(s, d, r, *args, None, None) == -2, args    # PVHIP_EINVAL, nothing launched
    for args in ([changed(good_yuv, _1=0), changed(good_yuv, _6=0), changed(good_yuv, _7=0), changed(good_yuv, _6=5), changed(good_yuv, _7=5),
                  changed(good_yuv, _0=0), changed(good_yuv, _0=70000), changed(good_yuv, _2=3), changed(good_yuv, _3=3), changed(good_yuv, _2=0),
                  changed(good_yuv, _4=0), changed(good_yuv, _5=0), changed(good_yuv, _8=2), changed(good_yuv, _8=-1),
                  changed(good_yuv, _2=40000, _3=40000), changed(good_yuv, _4=40000, _5=40000)]):
        assert yuv(s, d, r, *args, None, None) == -2, args
    for fn, args in ((raw, good_raw), (yuv, good_yuv)):
        assert fn(None, d, r, *args, None, None) == -2
        assert fn(s, None, r, *args, None, None) == -2
        assert fn(s, d, None, *args, None, None) == -2
    f32 = changed(good_raw, _9=0)
    assert raw(ctypes.c_void_p(src.ptr + 1), d, r, *f32, None, None) == -2       # an fp32 source off element alignment
    assert np.array_equal(np.asarray(dst), np.full(64, 7, np.float32))
    assert raw(s, d, r, *good_raw, None, None) == 0           # (and the same arguments in order are taken)
    assert yuv(s, d, r, *good_yuv, None, None) == 0


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_roi_buffers_shape_and_dtype(hip, kind):
    yuv, u8, nhwc = _is(kind)
    n, hw = 4, (48, 64)
    ie, net, name = _net(batch=n)
    _declare(net, name, kind)
    ex = ie.load_network(net, 'GPU', num_requests=2)
    dtype = np.dtype(np.uint8 if u8 else np.float32)
    req = ex.requests[0]
    plain = req.input_buffer(name, hw)
    assert plain.shape == _frame_shape(kind, n, hw) and req.input_buffer(name, hw, frames=None) is plain       # frames=None: as before
    for m in (1, 3, n, n + 5):
        buf = req.input_buffer(name, hw, frames=m)
        assert buf.shape == _frame_shape(kind, m, hw) and buf.dtype == dtype and buf.flags.c_contiguous
        assert req.input_buffer(name, hw, frames=m) is buf and buf is not plain          # (frames=n is not the plain buffer either)
    table = req.roi_buffer(name)
    assert table.shape == (n, 5) and table.dtype == np.int32 and req.roi_buffer(name) is table
    assert ex.requests[1].roi_buffer(name) is not table
    assert ex.requests[1].input_buffer(name, hw, frames=3) is not req.input_buffer(name, hw, frames=3)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_frames_buffer_without_its_table_is_an_array_like_any_other(hip, kind):
    """The frames buffer of a RoiInput handed to infer() as it is (the RoiInput forgotten): with m != n it is refused with the text the
    format gives for any array of that shape, and nothing is launched -- it is never taken for n images; with m == n it is n images."""
    n, hw = 4, (48, 64)
    ie, net, name = _net(batch=n)
    _declare(net, name, kind)
    fmt = net.input_info[name].frozen()
    ex = ie.load_network(net)
    req = ex.requests[0]
    launched = []
    real_call = hip.call
    for m in (1, 3, n + 5):
        buf = req.input_buffer(name, hw, frames=m)
        buf[...] = 0
        with pytest.raises(ValueError) as by_format:
            fmt.extent_of(np.empty(buf.shape, buf.dtype))
        hip.call = lambda entry, *args: (launched.append(entry), real_call(entry, *args))[1]
        try:
            for infer in (ex.infer, req.infer):
                with pytest.raises(ValueError) as by_infer:
                    infer({name: buf})
                assert str(by_infer.value) == str(by_format.value) and str(by_infer.value).startswith('input {}: '.format(name))
        finally:
            hip.call = real_call
    assert not [e for e in launched if 'input' in e or 'memcpy' in e], launched      # neither an upload nor a conversion
    assert set(ex.host_inputs.slots[name].extents) == {(hw, 1), (hw, 3), (hw, n + 5)}  # and no plain staging was made
    rng = np.random.default_rng(5)
    frames = _frames(rng, kind, n, hw)
    buf = req.input_buffer(name, hw, frames=n)
    buf[...] = frames
    ex.infer({name: buf})                                     # n frames: n images, through the plain staging of that extent
    assert_bit_exact(_fixed(ex, name), _ref(kind, frames, _whole(n, hw), (224, 224)), kind + ' frames buffer of n frames as n images')
    assert hw in ex.host_inputs.slots[name].extents


def _mean():
    return [104.0, 117.0, 123.0], [1.0, 57.5, 2.0]


def _fixed(ex, name):
    return np.asarray(ex.host_inputs.slots[name].fixed).copy()


@pytest.mark.gpu
def test_googlenet_from_nv12_rectangles_matches_the_host_crops(hip):
    """Three (480, 640) NV12 frames and 8 rectangles of one size (odd origins, an odd size) through infer({name: RoiInput}): the Results
    of the same network declared U8 / NHWC + resize fed the 8 crops of the converted frames; the same from the request's own buffers;
    and rectangles of eight sizes against the restatement and against per-rectangle passes of the U8 / NHWC network."""
    from pyopenvino_amd import RoiInput, synth
    blob = synth.synth_weights(os.path.join(MODELS, 'googlenet-v1.xml'), 11)
    rng = np.random.default_rng(2021)
    n, hw = 8, (480, 640)
    frames = _frames(rng, 'NV12', 3, hw)
    bgr = yuv_ref.to_bgr(frames, 'NV12')
    w, h = 201, 150
    table = np.array([(b % 3, 1 + 53 * b, 3 + 41 * b, w, h) for b in range(n)], np.int32)
    table[7] = (2, 640 - w, 480 - h, w, h)
    assert roi_ref.valid(table, n, 3, hw)
    crops = np.stack([bgr[i, y:y + h, x:x + w] for i, x, y, _, _ in table], 0)
    mean = _mean()
    ie, net, name = _net('googlenet-v1', n, blob)
    out_name = net.outputs[0]['name']
    _declare(net, name, 'U8-NHWC', mean=mean)
    ex_bgr = ie.load_network(net)
    want = np.array(ex_bgr.infer({name: crops})[out_name], copy=True)
    want_input = _fixed(ex_bgr, name)
    assert np.isfinite(want).all()
    assert_bit_exact(want_input, roi_ref.preprocess_rois(frames, table, (224, 224), mean=mean[0], std_scale=mean[1], color='NV12'),
                     'the U8 / NHWC input tensor of the host crops')
    ie, net, name = _net('googlenet-v1', n, blob)
    _declare(net, name, 'NV12', mean=mean)
    ex = ie.load_network(net)
    untouched = frames.copy()
    got = ex.infer({name: RoiInput(frames, table)})[out_name]
    assert np.array_equal(frames, untouched)
    assert_bit_exact(_fixed(ex, name), want_input, 'input tensor of the RoiInput')
    assert_bit_exact(got, want, 'RoiInput through infer()')
    assert_bit_exact(ex.infer({name: RoiInput(frames, table.astype(np.int64).tolist())})[out_name], want, 'the table as a list')
    # from the request's own buffers: no host copy, the same Results
    req = ex.requests[0]
    buf, tbuf = req.input_buffer(name, hw, frames=3), req.roi_buffer(name)
    assert buf.shape == (3, 720, 640) and buf.dtype == np.uint8 and tbuf.shape == (n, 5) and tbuf.dtype == np.int32
    assert buf is ex.host_inputs.slots[name].extents[(hw, 3)].host
    buf[...] = frames
    tbuf[...] = table
    assert_bit_exact(req.infer({name: RoiInput(buf, tbuf)})[out_name], want, 'RoiInput from the request buffers')
    assert len(ex.host_inputs.slots[name].extents) == 1
    # whole frames in the plain form still go their own way on the same network, and the fixed tensor keeps its address
    address = ex.host_inputs.slots[name].fixed.ptr
    ex.infer({name: np.concatenate([frames, frames, frames[:2]], 0)})
    assert_bit_exact(_fixed(ex, name), preprocess(np.concatenate([bgr, bgr, bgr[:2]], 0), (224, 224), mean=mean[0], std_scale=mean[1]), 'plain frames')
    # rectangles of eight sizes
    sizes = np.array([(0, 0, 0, 640, 480), (1, 5, 7, 1, 1), (2, 3, 5, 224, 224), (0, 11, 21, 224, 99), (1, 601, 441, 39, 39), (2, 101, 203, 31, 29),
                      (1, 1, 1, 639, 479), (0, 13, 17, 151, 133)], np.int32)
    got = ex.infer({name: RoiInput(frames, sizes)})[out_name]
    assert ex.host_inputs.slots[name].fixed.ptr == address
    got_input = _fixed(ex, name)
    assert_bit_exact(got_input, roi_ref.preprocess_rois(frames, sizes, (224, 224), mean=mean[0], std_scale=mean[1], color='NV12'), 'eight sizes')
    for b, (i, x, y, w_, h_) in enumerate(sizes):             # the device's own resize of each host crop, a pass per rectangle
        ex_bgr.infer({name: np.repeat(bgr[i:i + 1, y:y + h_, x:x + w_], n, 0)})
        assert_bit_exact(got_input[b], _fixed(ex_bgr, name)[b], 'rectangle {} against the U8 / NHWC path'.format(b))
    assert np.isfinite(got).all()


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['I420', 'U8-NHWC'])
def test_ssd_from_rectangles_with_reversed_channels(hip, kind):
    from pyopenvino_amd import RoiInput, synth
    blob = synth.synth_weights(os.path.join(MODELS, 'ssd_mobilenet_v1_coco.xml'), 1234)
    rng = np.random.default_rng(301)
    n, hw = 2, (480, 640)
    frames = _frames(rng, kind, 3, hw)
    image = yuv_ref.to_bgr(frames, kind) if kind in YUV else frames
    table = np.array([(2, 33, 17, 333, 301), (0, 640 - 333, 480 - 301, 333, 301)], np.int32)
    crops = np.stack([image[i, y:y + h, x:x + w] for i, x, y, w, h in table], 0)
    ie, net, name = _net('ssd_mobilenet_v1_coco', n, blob)
    out_name = net.outputs[0]['name']
    _declare(net, name, 'U8-NHWC', reverse=True)
    ex_bgr = ie.load_network(net)
    want = np.array(ex_bgr.infer({name: crops})[out_name], copy=True)
    want_input = _fixed(ex_bgr, name)
    ie, net, name = _net('ssd_mobilenet_v1_coco', n, blob)
    _declare(net, name, kind, reverse=True)
    ex = ie.load_network(net)
    got = ex.infer({name: RoiInput(frames, table)})[out_name]
    assert_bit_exact(_fixed(ex, name), want_input, 'SSD input tensor from {} rectangles'.format(kind))
    assert_bit_exact(got, want, 'SSD from {} rectangles as R, G, B'.format(kind))


@pytest.mark.gpu
def test_six_requests_in_flight_new_frames_and_tables_every_step(hip):
    """Six requests, new NV12 frames and a new table for every request on every step, the frame count alternating between 1 and 4 per
    request: every Result equals, bit for bit, the eager Result of the same network fed that RoiInput one request at a time, and after
    the warm-up passes every request replays its recording whatever the frames and the table."""
    from pyopenvino_amd import RoiInput, synth
    blob = synth.synth_weights(os.path.join(MODELS, 'googlenet-v1.xml'), 5)
    B, R, hw = 64, 6, (480, 640)
    rng = np.random.default_rng(66)
    counts = [1, 4]

    def table(m):
        w, h = rng.integers(32, 400, B), rng.integers(32, 400, B)
        return np.stack([rng.integers(0, m, B), rng.integers(0, 640 - w + 1), rng.integers(0, 480 - h + 1), w, h], 1).astype(np.int32)

    sources = [(_frames(rng, 'NV12', counts[k % 2], hw), table(counts[k % 2])) for k in range(4)]
    assert all(roi_ref.valid(t, B, f.shape[0], hw) for f, t in sources)
    mean = ([104.0, 117.0, 123.0], [1.0, 1.0, 1.0])

    def loaded(requests):
        ie, net, name = _net('googlenet-v1', B, blob)
        _declare(net, name, 'NV12', mean=mean)
        return ie.load_network(net, 'GPU', num_requests=requests), name, net.outputs[0]['name']

    want = []
    for f, t in sources:                                      # the first pass of a newly loaded network: dispatched eagerly, nothing recorded yet
        ex_ref, name, out_name = loaded(1)
        want.append(np.array(ex_ref.infer({name: RoiInput(f, t)})[out_name], copy=True))
        assert ex_ref._graph is None
        ex_ref.release_device_state()
        del ex_ref
    assert all(np.isfinite(w_).all() for w_ in want) and not np.array_equal(want[0], want[2])

    ex, _, _ = loaded(R)
    steps = 6
    for step in range(steps):
        order = [(r * 5 + step) % R for r in range(R)]
        fed = {}
        for r in order:
            k = (r + step) % 4                                # frame count (r + step) % 2: alternates per request, and new frames every step
            req = ex.requests[r]
            f, t = sources[k]
            if r % 2:                                         # half the requests from their own page-locked buffers, half from pageable arrays
                buf, tbuf = req.input_buffer(name, hw, frames=counts[k % 2]), req.roi_buffer(name)
                np.copyto(buf, f)
                np.copyto(tbuf, t)
                feed = RoiInput(buf, tbuf)
            else:
                feed = RoiInput(f, t)
            ex.start_async(r, {name: feed})
            fed[r] = k
            if step >= 3:
                assert req._replayed is not None, 'step {} request {} was not replayed'.format(step, r)
        for r in reversed(order):
            got = ex.wait(r)[out_name]
            assert np.array_equal(got, want[fed[r]]), 'step {} request {} (source {})'.format(step, r, fed[r])
    for req in ex.requests:
        extents = req.runner.host_inputs.slots[name].extents
        assert set(extents) == {(hw, 1), (hw, 4)} and len(extents) <= ex.MAX_SOURCE_EXTENTS
