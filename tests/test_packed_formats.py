"""Packed host inputs (IENetwork.input_info[name].preprocess_info.color_format 'YUY2' / 'UYVY' / 'BGRX' / 'RGBX'): a camera's packed
YUV 4:2:2 frames, uint8 of shape (n, h, w, 2), and a screen capture's four-byte pixels, uint8 of shape (n, h, w, 4), converted to B, G,
R on the device in the launch that crops, resizes, reverses and scales them (pvhip_input_preprocess_packed_f32 / _packed_roi_f32), bit
for bit tests/packed_ref.py followed by tests/preprocess_ref.py.  The first tests need no GPU."""
import ctypes
import dataclasses
import functools
import os
import re

import numpy as np
import pytest

import helpers
import packed_ref
import roi_ref
import yuv_ref
from detected_rois_ref import detected_rois, padded
from helpers import MODELS, assert_bit_exact
from packed_ref import KINDS, XRGB, YUV422
from preprocess_ref import preprocess

HIP = 'pyopenvino_amd.op_plugins'
FORMATS = ['YUY2', 'UYVY', 'BGRX', 'RGBX']
ENTRY, ENTRY_ROI = 'pvhip_input_preprocess_packed_f32', 'pvhip_input_preprocess_packed_roi_f32'
U8 = np.dtype(np.uint8)


@functools.lru_cache(maxsize=None)
def _weights(model, seed=7):
    """mnist ships its weights; the other IRs get seeded synthetic ones."""
    from pyopenvino_amd import synth
    return None if model == 'mnist' else synth.synth_weights(os.path.join(MODELS, model + '.xml'), seed)


def _net(model='googlenet-v1', batch=1, blob=None):
    from pyopenvino_amd import IECore
    ie = IECore(plugin_package=HIP)
    net = ie.read_network(os.path.join(MODELS, model + '.xml'), weights=blob if blob is not None else _weights(model))
    if batch != 1:
        net.set_batch(batch)
    return ie, net, net.inputs[0]['name']


def _reshaped(shape):
    """mnist with its Parameter declared to have `shape` (nothing is inferred: only what load_network checks of the input is used)."""
    ie, net, name = _net('mnist')
    nid = next(n for n in net.G.nodes if net.G.nodes[n]['name'] == name)
    net.G.nodes[nid]['data']['shape'] = shape
    return ie, net, name


def _declare(net, name, color, resize=True, reverse=False, mean=None):
    """`color` 'RAW' declares the U8 / NHWC input the converted frames are fed to."""
    info = net.input_info[name]
    pre = info.preprocess_info
    if color == 'RAW':
        info.precision, info.layout = 'U8', 'NHWC'
    pre.color_format = color
    if resize:
        pre.resize_algorithm = 'RESIZE_BILINEAR'
    pre.reverse_channels = reverse
    if mean is not None:
        pre.init(3)
        for c in range(3):
            pre[c].mean_value, pre[c].std_scale = mean[0][c], mean[1][c]
        pre.mean_variant = 'MEAN_VALUE'


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
def test_setter_takes_the_four_names_in_any_case_and_declares():
    for color in FORMATS:
        for spelled in (color, color.lower(), color.capitalize()):
            _, net, name = _net()
            info = net.input_info[name]
            assert not info.declared
            info.preprocess_info.color_format = spelled
            assert info.preprocess_info.color_format == color and info.declared
            assert (info.precision, info.layout) == ('FP32', 'NCHW')      # what was never set reads as before
    from pyopenvino_amd.input_format import PreProcessInfo
    assert PreProcessInfo.COLOR_FORMATS == ('RAW', 'NV12', 'I420') + tuple(FORMATS)


def test_setter_is_refused_after_load_and_on_other_parameters():
    ie, net, name = _net('mnist')
    pre = net.input_info[name].preprocess_info
    ie.load_network(net)
    for color in FORMATS:
        with pytest.raises(ValueError, match='between read_network and load_network'):
            pre.color_format = color
    assert pre.color_format == 'RAW'
    for change in (dict(element_type='i32'), dict(shape=(1, 784))):    # not f32; not 4-D
        _, net, name = _net('mnist')
        nid = next(n for n in net.G.nodes if net.G.nodes[n]['name'] == name)
        pre = net.input_info[name].preprocess_info
        net.G.nodes[nid]['data'].update(change)
        for color in FORMATS:
            with pytest.raises(NotImplementedError):
                pre.color_format = color
        assert pre.color_format == 'RAW' and not net.input_info[name].declared


@pytest.mark.parametrize('color', FORMATS)
def test_frozen_carries_the_kind(color):
    _, net, name = _net()
    info = net.input_info[name]
    pre = info.preprocess_info
    pre.color_format = color
    pre.reverse_channels = True
    pre.init(3)
    pre[1].mean_value = 117
    pre.mean_variant = 'MEAN_VALUE'
    fmt = info.frozen()
    assert (fmt.color, fmt.packed, fmt.packed_kind, fmt.yuv, fmt.u8, fmt.resize, fmt.reverse) == (color, True, KINDS[color], False, True, False, True)
    assert fmt.packed_bytes == packed_ref.bytes_per_pixel(color)
    assert fmt.mean.tolist() == [0, 117, 0] and fmt.std.tolist() == [1, 1, 1]
    assert fmt.host_dtype == U8
    assert fmt.needs_preprocess((224, 224)) and fmt.needs_convert((224, 224))
    with pytest.raises(dataclasses.FrozenInstanceError):
        fmt.color = 'RAW'
    assert info.preprocessing()[:2] == (False, True)
    for other, yuv in (('RAW', False), ('NV12', True), ('I420', True)):           # the formats there were keep what they had
        pre.color_format = other
        assert (info.frozen().yuv, info.frozen().packed) == (yuv, False)


@pytest.mark.parametrize('resize', [False, True])
@pytest.mark.parametrize('color', FORMATS)
def test_packed_shape_rules(color, resize):
    """host_format, InputFormat.host_shape / extent_of / checked_extent and input_buffer at the network's extent and at others; an odd
    width is refused for 4:2:2 and an odd height is not; arrays of other shapes are refused with one text by the format and by infer(),
    before anything reaches the device."""
    ie, net, name = _net(batch=2)
    info = net.input_info[name]
    info.preprocess_info.color_format = color
    info.layout = 'NHWC'                                      # not consulted
    if resize:
        info.preprocess_info.resize_algorithm = 'RESIZE_BILINEAR'
    fmt = info.frozen()
    bpp = packed_ref.bytes_per_pixel(color)
    assert info.host_format() == info.host_format((224, 224)) == ((2, 224, 224, bpp), U8)
    assert fmt.host_shape() == (2, 224, 224, bpp) and fmt.checked_extent() == (224, 224)
    assert fmt.extent_of(np.empty((2, 224, 224, bpp), np.uint8)) == (224, 224)
    assert fmt.host_shape((37, 42), frames=5) == (5, 37, 42, bpp)
    other = [(480, 640), (481, 642), (1, 2), (37, 42)] + ([(3, 5), (20, 31)] if color in XRGB else [])     # odd heights are legal
    for h, w in other:
        if resize:
            assert info.host_format((h, w)) == ((2, h, w, bpp), U8)
            assert fmt.host_shape((h, w)) == (2, h, w, bpp) and fmt.checked_extent((h, w)) == (h, w)
            assert info.source_extent((h, w)) == (h, w)
            assert fmt.extent_of(np.empty((2, h, w, bpp), np.uint8)) == (h, w)
            assert fmt.frames_extent_of(np.empty((5, h, w, bpp), np.uint8)) == ((h, w), 5)
        else:
            for refused in (info.host_format, fmt.checked_extent):
                with pytest.raises(ValueError, match='no resize is declared'):
                    refused((h, w))
    odd = [(224, 223), (480, 641), (1, 1), (37, 41)]
    for extent in odd:
        for refused in (info.host_format, fmt.checked_extent, info.source_extent):
            if color in YUV422:
                with pytest.raises(ValueError, match='even width'):
                    refused(extent)
            elif resize:
                assert refused(extent) in (extent, ((2,) + extent + (4,), U8))
    ex = ie.load_network(net)
    if color in YUV422:
        for extent in odd[1:]:
            with pytest.raises(ValueError, match='even width'):
                ex.requests[0].input_buffer(name, extent)
            if resize:
                with pytest.raises(ValueError, match='even width'):
                    ex.requests[0].input_buffer(name, extent, frames=3)
    if not resize:
        with pytest.raises(ValueError, match='no resize is declared'):
            ex.requests[0].input_buffer(name, (480, 640))
    # wrong batch, the other family's unit, a B, G, R image, an NV12 frame, no batch, no unit axis, (4:2:2) an odd width, no rows,
    # (no resize) another extent
    bad = [(3, 224, 224, bpp), (2, 224, 224, 6 - bpp), (2, 224, 224, 3), (2, 336, 224), (224, 224, bpp), (2, 224, 224 * bpp), (2, 0, 224, bpp)]
    bad += [(2, 224, 223, bpp)] if color in YUV422 or not resize else []
    bad += [] if resize else [(2, 480, 640, bpp)]
    for shape in bad:
        with pytest.raises(ValueError) as by_format:
            fmt.extent_of(np.empty(shape, np.uint8))
        with pytest.raises(ValueError) as by_infer:           # refused before anything reaches the device
            ex.infer({name: np.empty(shape, np.uint8)})
        assert str(by_format.value) == str(by_infer.value), shape
        assert str(by_format.value).startswith('input {}: '.format(name)), str(by_format.value)
    if resize:                                                # the frames of a RoiInput: the same rules with any count m
        from pyopenvino_amd import RoiInput
        table = np.array([[0, 0, 0, 2, 2]] * 2, np.int32)
        bad_frames = [(0, 48, 64, bpp), (48, 64, bpp), (3, 48, 64, 6 - bpp), (3, 48, 64, 3), (3, 72, 64), (3, 0, 64, bpp)]
        bad_frames += [(3, 48, 63, bpp)] if color in YUV422 else []
        for shape in bad_frames:
            with pytest.raises(ValueError) as by_format:
                fmt.frames_extent_of(np.empty(shape, np.uint8))
            with pytest.raises(ValueError) as by_infer:
                ex.infer({name: RoiInput(np.empty(shape, np.uint8), table)})
            assert str(by_format.value) == str(by_infer.value), shape
            assert str(by_format.value).startswith('input {}: '.format(name)), str(by_format.value)
    assert not ex.host_inputs.slots                           # nothing was allocated


@pytest.mark.parametrize('color', FORMATS)
def test_channel_count_extent_and_precision_are_checked_at_load(color):
    ie, net, name = _net('mnist')                             # one channel
    net.input_info[name].preprocess_info.color_format = color
    with pytest.raises(ValueError, match='3 channels'):
        ie.load_network(net)
    ie, net, name = _reshaped((1, 4, 28, 28))
    net.input_info[name].preprocess_info.color_format = color
    with pytest.raises(ValueError, match='3 channels'):
        ie.load_network(net)
    ie, net, name = _reshaped((1, 3, 27, 28))                 # an odd height is legal for every kind
    net.input_info[name].preprocess_info.color_format = color
    assert net.input_info[name].host_format() == ((1, 27, 28, packed_ref.bytes_per_pixel(color)), U8)
    ie.load_network(net)
    ie, net, name = _reshaped((1, 3, 28, 27))                 # the frames have the network's extent: 4:2:2 needs an even width
    net.input_info[name].preprocess_info.color_format = color
    if color in YUV422:
        with pytest.raises(ValueError, match='even width'):
            ie.load_network(net)
        with pytest.raises(ValueError, match='even width'):
            net.input_info[name].host_format()
        net.input_info[name].preprocess_info.resize_algorithm = 'RESIZE_BILINEAR'     # sources of any even width: nothing to refuse
        assert net.input_info[name].host_format((31, 40)) == ((1, 31, 40, 2), U8)
        ie.load_network(net)
    else:
        assert net.input_info[name].host_format() == ((1, 28, 27, 4), U8)
        ie.load_network(net)
    for precision, refused in (('FP32', True), ('fp32', True), ('U8', False), (None, False)):
        ie, net, name = _net()
        info = net.input_info[name]
        if precision is not None:
            info.precision = precision
        info.preprocess_info.color_format = color
        if refused:
            with pytest.raises(ValueError, match='precision FP32'):
                ie.load_network(net)
            info.preprocess_info.color_format = 'RAW'         # FP32 with RAW stays what it was
            assert info.host_format() == ((1, 3, 224, 224), np.dtype(np.float32))
        else:
            assert info.host_format() == ((1, 224, 224, packed_ref.bytes_per_pixel(color)), U8)


def test_restatement_yuy2_and_uyvy_of_the_same_planes_give_the_same_image():
    rng = np.random.default_rng(422)
    for h, w in ((1, 2), (3, 2), (7, 10), (37, 42), (480, 640)):
        y = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
        u, v = rng.integers(0, 256, (2, 2, h, w // 2), dtype=np.uint8)
        images = []
        for color in YUV422:
            frames = packed_ref.frames_of(y, u, v, color)
            assert frames.shape == (2, h, w, 2) and frames.dtype == np.uint8 and frames.flags.c_contiguous
            for got, want in zip(packed_ref.planes(frames, color), (y, u, v)):
                assert np.array_equal(got, want)
            images.append(packed_ref.to_bgr(frames, color))
        assert images[0].shape == (2, h, w, 3) and np.array_equal(images[0], images[1])
        # pixel (y, x) takes luma Y[x & 1] and the chroma of group x // 2 of its own row
        for yy, xx in ((h - 1, w - 1), (h - 1, w - 2), (0, 0), (h // 2, 1)):
            assert images[0][1, yy, xx].tolist() == yuv_ref.convert(y[1, yy, xx], u[1, yy, xx // 2], v[1, yy, xx // 2]).tolist()
    yuy2, uyvy = (packed_ref.frames_of(y, u, v, c).reshape(2, h, w // 2, 4) for c in YUV422)
    assert np.array_equal(yuy2[..., 0], y[..., 0::2]) and np.array_equal(yuy2[..., 1], u) and np.array_equal(yuy2[..., 3], v)
    assert np.array_equal(uyvy[..., 0], u) and np.array_equal(uyvy[..., 1], y[..., 0::2]) and np.array_equal(uyvy[..., 3], y[..., 1::2])


def _packed_of_nv12(nv12, color):
    """The 4:2:2 frames of an NV12 frame's planes with every chroma row doubled."""
    y, u, v = yuv_ref.planes(nv12, 'NV12')
    return packed_ref.frames_of(y, u.repeat(2, 1), v.repeat(2, 1), color)


def test_restatement_doubled_chroma_rows_give_the_nv12_image():
    rng = np.random.default_rng(420)
    for h, w in ((2, 2), (6, 10), (38, 42)):
        nv12 = rng.integers(0, 256, (2, 3 * h // 2, w), dtype=np.uint8)
        for color in YUV422:
            assert np.array_equal(packed_ref.to_bgr(_packed_of_nv12(nv12, color), color), yuv_ref.to_bgr(nv12, 'NV12'))


def test_restatement_is_the_rule_of_yuv_ref_within_one_of_the_float64_matrix():
    """The conversion is yuv_ref.convert itself, and over a sweep of byte triples (every 3rd Y, every U and V in steps of 5, and the
    corners) each channel is within 1 of the rounded float64 value of the BT.601 matrix."""
    import inspect
    assert 'yuv_ref.convert(' in inspect.getsource(packed_ref.to_bgr) and not hasattr(packed_ref, 'CY')
    k = [c / 2.0 ** 20 for c in (yuv_ref.CY, yuv_ref.CRV, yuv_ref.CGV, yuv_ref.CGU, yuv_ref.CBU)]
    ys = np.unique(np.concatenate([np.arange(0, 256, 3), [15, 16, 17, 234, 235, 236, 255]]))
    cs = np.unique(np.concatenate([np.arange(0, 256, 5), [127, 128, 129, 254, 255]]))
    y, u, v = (a.reshape(-1) for a in np.meshgrid(ys, cs, cs, indexing='ij'))
    y = y.reshape(1, 1, -1).astype(np.uint8)                  # one row of len(y) pixels: pixel x of 4:2:2 needs the chroma of its pair,
    worst = 0.0
    for color in YUV422:                                      # so every triple is laid out as a pair with the same luma twice
        frames = packed_ref.frames_of(y.repeat(2, 2), u.reshape(1, 1, -1).astype(np.uint8), v.reshape(1, 1, -1).astype(np.uint8), color)
        got = packed_ref.to_bgr(frames, color)[0, 0, 0::2].astype(np.float64)
        assert np.array_equal(got, packed_ref.to_bgr(frames, color)[0, 0, 1::2])
        yl, uf, vf = k[0] * np.maximum(y.reshape(-1) - 16.0, 0), u - 128.0, v - 128.0
        want = np.stack([yl + k[4] * uf, yl - k[2] * vf - k[3] * uf, yl + k[1] * vf], -1)
        worst = max(worst, float(np.abs(got - np.rint(np.clip(want, 0, 255))).max()))
    assert worst <= 1.0, worst


def test_restatement_bgrx_and_rgbx_and_byte_3():
    rng = np.random.default_rng(4)
    for h, w in ((1, 1), (3, 5), (37, 42)):
        bgr = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
        x = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
        bgrx, rgbx = packed_ref.frames_from_bgr(bgr, 'BGRX', x), packed_ref.frames_from_bgr(bgr, 'RGBX', x)
        assert bgrx.shape == rgbx.shape == (2, h, w, 4)
        assert np.array_equal(bgrx[..., 0], rgbx[..., 2]) and np.array_equal(bgrx[..., 2], rgbx[..., 0]) and np.array_equal(bgrx[..., 1], rgbx[..., 1])
        assert np.array_equal(packed_ref.to_bgr(bgrx, 'BGRX'), bgr) and np.array_equal(packed_ref.to_bgr(rgbx, 'RGBX'), bgr)
        assert np.array_equal(packed_ref.to_bgr(bgrx, 'BGRX'), bgrx[..., 0:3]) and np.array_equal(packed_ref.to_bgr(rgbx, 'RGBX'), rgbx[..., 2::-1])
        for color, frames in (('BGRX', bgrx), ('RGBX', rgbx)):                    # changing only byte 3 changes nothing
            changed = frames.copy()
            changed[..., 3] = ~changed[..., 3]
            assert not np.array_equal(changed, frames)
            assert np.array_equal(packed_ref.to_bgr(changed, color), bgr)
            assert_bit_exact(packed_ref.preprocess_packed(changed, color, (5, 7), reverse_channels=True),
                             preprocess(bgr, (5, 7), reverse_channels=True), color)


def _frames(rng, n, hw, color, kind):
    """n frames of extent hw: 'bytes' uniform random bytes (4:2:2: 40 % of the converted values saturate: the clamp), 'encoded' random
    B, G, R images converted forward with the chroma averaged over each column pair (mostly unsaturated arithmetic; X kinds: the image
    itself with a random byte 3)."""
    h, w = hw
    if kind == 'bytes':
        return rng.integers(0, 256, packed_ref.frame_shape(color, n, hw), dtype=np.uint8)
    return packed_ref.frames_from_bgr(rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8), color, rng.integers(0, 256, (n, h, w), dtype=np.uint8))


def test_test_material_saturates_as_stated():
    """Encoded 4:2:2 frames convert back with 0.97 of the values strictly inside (0, 255), random bytes with 0.60; the GPU tests assert
    >= 0.5 for the encoded frames they use."""
    rng = np.random.default_rng(601)
    inside = lambda x: float(((x > 0) & (x < 255)).mean())  # noqa: E731
    for color in YUV422:
        enc = inside(packed_ref.to_bgr(_frames(rng, 2, (48, 64), color, 'encoded'), color))
        raw = inside(packed_ref.to_bgr(_frames(rng, 2, (48, 64), color, 'bytes'), color))
        assert enc >= 0.9 and 0.5 <= raw <= 0.7, (enc, raw)
    flat = np.full((1, 3, 4, 3), (40, 120, 200), np.uint8)    # a flat image comes back within the rounding of Y, U, V
    back = packed_ref.to_bgr(packed_ref.frames_from_bgr(flat, 'UYVY'), 'UYVY')
    assert np.abs(back.astype(int) - flat.astype(int)).max() <= 2


def test_restatement_rectangle_is_the_crop_of_the_converted_image():
    rng = np.random.default_rng(37)
    for color in FORMATS:
        frames = _frames(rng, 3, (37, 42), color, 'encoded')
        bgr = packed_ref.to_bgr(frames, color)
        for roi in ((2, 1, 1, 41, 35), (0, 5, 3, 7, 9), (1, 41, 36, 1, 1), (1, 3, 0, 2, 37)):
            i, x0, y0, w, h = roi
            for dst in ((h, w), (11, 13)):
                want = preprocess(bgr[i:i + 1, y0:y0 + h, x0:x0 + w], dst, reverse_channels=True)
                assert_bit_exact(packed_ref.preprocess_rois(frames, color, [roi], dst, reverse_channels=True), want, '{} {}'.format(color, roi))


def test_abi_declares_the_packed_entries():
    from pyopenvino_amd import device
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for entry, count in ((ENTRY, 11), (ENTRY_ROI, 15)):
        assert entry in device.SIGNATURES and len(device.SIGNATURES[entry][1]) == count
        m = re.search(r'\b' + entry + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S)
        assert m and len(m.group(1).split(',')) == count, entry
        assert entry not in device._NOT_STATUS                # a status, like every launch
    assert re.search(r'#define\s+PVHIP_ABI_VERSION\s+19\b', header)
    lib = device.load_library()
    assert hasattr(lib, ENTRY) and hasattr(lib, ENTRY_ROI) and lib.pvhip_abi_version() == 19


# ---------------------------------------------------------------------------------------------------------------- GPU
class _Source:
    """Frames on the device, `shift` bytes off 16-byte alignment, with `margin` whole frames of allocation on both sides."""

    def __init__(self, hip, frames, shift=0, margin=0):
        frames = np.ascontiguousarray(frames)
        self.shape, self.frame_bytes = frames.shape, frames.nbytes // frames.shape[0]
        raw = np.zeros(frames.nbytes + shift + 2 * margin * self.frame_bytes, np.uint8)
        first = shift + margin * self.frame_bytes
        raw[first:first + frames.nbytes] = frames.reshape(-1)
        self.tensor = hip.DeviceTensor.from_numpy(raw)
        self.ptr = self.tensor.ptr + first


def _pre_args(hip, reverse, mean, std):
    m = hip.DeviceTensor.from_numpy(np.asarray(mean, np.float32)) if mean is not None else None
    s = hip.DeviceTensor.from_numpy(np.asarray(std, np.float32)) if std is not None else None
    return (int(reverse), ctypes.c_void_p(m.ptr) if m is not None else None, ctypes.c_void_p(s.ptr) if s is not None else None), (m, s)


def _device_packed(hip, src, dst_hw, color, reverse=False, mean=None, std=None):
    """pvhip_input_preprocess_packed_f32 on the _Source `src` into a destination prefilled with 0x7f bytes."""
    n, h, w, _ = src.shape
    dst = hip.DeviceTensor.empty((n, 3) + tuple(dst_hw))
    hip.call('pvhip_memset', ctypes.c_void_p(dst.ptr), 0x7f, dst.nbytes)
    pre, keep = _pre_args(hip, reverse, mean, std)
    hip.call(ENTRY, ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), n, h, w, dst_hw[0], dst_hw[1], KINDS[color], *pre)
    return np.asarray(dst)


def _device_rois(hip, src, rois, dst_hw, color, m=None, largest=None, reverse=False, mean=None, std=None):
    """The ROI entry on the _Source `src` into a destination prefilled with 0x7f bytes."""
    rois = np.ascontiguousarray(rois, np.int32)
    n = rois.shape[0]
    m = src.shape[0] if m is None else m
    largest = (int(rois[:, 4].max()), int(rois[:, 3].max())) if largest is None else largest
    table = hip.DeviceTensor.from_numpy(rois)
    dst = hip.DeviceTensor.empty((n, 3) + tuple(dst_hw))
    hip.call('pvhip_memset', ctypes.c_void_p(dst.ptr), 0x7f, dst.nbytes)
    pre, keep = _pre_args(hip, reverse, mean, std)
    hip.call(ENTRY_ROI, ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), ctypes.c_void_p(table.ptr), n, m, src.shape[1], src.shape[2],
             dst_hw[0], dst_hw[1], largest[0], largest[1], KINDS[color], *pre)
    return np.asarray(dst)


def _options(rng):
    mean = rng.uniform(0, 255, 3).astype(np.float32)
    std = rng.uniform(0.5, 80, 3).astype(np.float32)
    return [dict(), dict(reverse=True, mean=mean, std=std), dict(reverse=True), dict(mean=mean), dict(std=std)]


def _check_kernel(hip, rng, n, src_hw, dst_hw, color, options, shifts):
    for kind in ('bytes', 'encoded') if color in YUV422 else ('bytes',):
        frames = _frames(rng, n, src_hw, color, kind)
        bgr = packed_ref.to_bgr(frames, color)
        if kind == 'encoded':                                 # the unsaturated arithmetic is really exercised
            inside = float(((bgr > 0) & (bgr < 255)).mean())
            print('{} {}: {:.2f} of the converted values inside (0, 255)'.format(color, src_hw, inside))
            assert inside >= 0.5, '{} {}: {:.2f} of the converted values inside (0, 255)'.format(color, src_hw, inside)
        wants = [preprocess(bgr, dst_hw, nhwc=True, reverse_channels=opt.get('reverse', False), mean=opt.get('mean'), std_scale=opt.get('std'))
                 for opt in options]
        for shift in shifts:
            src = _Source(hip, frames, shift)
            for opt, want in zip(options, wants):
                what = '{} {} frames {} -> {} {} source offset {}'.format(color, kind, src_hw, dst_hw, sorted(opt), shift)
                assert_bit_exact(_device_packed(hip, src, dst_hw, color, **opt), want, what)


KERNEL_SHAPES = [((480, 640), (224, 224)), ((481, 642), (300, 300)), ((1, 2), (5, 3)), ((2, 2), (224, 224)), ((37, 42), (13, 1)),
                 ((20, 30), (20, 30))]
X_SHAPES = [((3, 5), (4, 7)), ((20, 31), (20, 31))]           # odd widths; a destination width that is no multiple of 4: scalar stores
CASES = [(c, s, d) for c in FORMATS for s, d in KERNEL_SHAPES] + [(c, s, d) for c in XRGB for s, d in X_SHAPES]


@pytest.mark.gpu
@pytest.mark.parametrize('color,src_hw,dst_hw', CASES)
def test_packed_kernel_bit_exact(hip, color, src_hw, dst_hw):
    rng = np.random.default_rng(sum(src_hw) * 31 + sum(dst_hw) * 3 + KINDS[color])
    _check_kernel(hip, rng, 2, src_hw, dst_hw, color, _options(rng), (0, 1, 2, 3))


# Rows whose sources exceed the kernel's 48 KiB of LDS (2 rows of 14000 4:2:2 pixels or of 7000 X pixels: 56 KB), so the output rows are
# split into column tiles that start at tx0 > 0, on even and on odd source columns.
COLUMN_TILES = [(c, s, d) for c in YUV422 for s, d in (((2, 14000), (2, 224)), ((3, 14002), (5, 227)), ((2, 30000), (2, 30000)))] + \
               [(c, s, d) for c in XRGB for s, d in (((2, 7000), (2, 224)), ((3, 7001), (5, 227)), ((2, 15000), (2, 15000)))]


@pytest.mark.gpu
@pytest.mark.parametrize('color,src_hw,dst_hw', COLUMN_TILES)
def test_packed_kernel_bit_exact_in_column_tiles(hip, color, src_hw, dst_hw):
    rng = np.random.default_rng(src_hw[1] + dst_hw[1] + KINDS[color])
    options = _options(rng)
    _check_kernel(hip, rng, 2, src_hw, dst_hw, color, [options[1], options[0]], (0, 3))


@pytest.mark.gpu
@pytest.mark.parametrize('src_hw,dst_hw', [((480, 640), (224, 224)), ((4, 14000), (2, 224))])
def test_yuy2_of_an_nv12_frame_matches_the_nv12_kernel(hip, src_hw, dst_hw):
    """Witness by the merged kernel: a YUY2 frame packed from an NV12 frame with doubled chroma rows gives, through the new entry, bit
    for bit what pvhip_input_preprocess_yuv_f32 gives for the NV12 frame -- device against device."""
    rng = np.random.default_rng(src_hw[1])
    h, w = src_hw
    nv12 = yuv_ref.frames_of(*yuv_ref.planes_from_bgr(rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)), 'NV12')
    mean, std = [104.0, 117.0, 123.0], [1.0, 57.5, 2.0]
    src = hip.DeviceTensor.from_numpy(nv12)
    for opt in (dict(), dict(reverse=True, mean=mean, std=std)):
        dst = hip.DeviceTensor.empty((2, 3) + dst_hw)
        hip.call('pvhip_memset', ctypes.c_void_p(dst.ptr), 0x7f, dst.nbytes)
        pre, keep = _pre_args(hip, opt.get('reverse', False), opt.get('mean'), opt.get('std'))
        hip.call('pvhip_input_preprocess_yuv_f32', ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), 2, h, w, *dst_hw, 0, *pre)
        want = np.asarray(dst)
        assert not np.isnan(want).any()
        got = _device_packed(hip, _Source(hip, _packed_of_nv12(nv12, 'YUY2')), dst_hw, 'YUY2', **opt)
        assert_bit_exact(got, want, 'YUY2 of an NV12 frame {} -> {} {}'.format(src_hw, dst_hw, sorted(opt)))


@pytest.mark.gpu
@pytest.mark.parametrize('color', ['UYVY', 'BGRX'])
def test_packed_kernel_bit_exact_batch256(hip, color):
    """Grid z: 256 small frames."""
    rng = np.random.default_rng(256)
    frames = _frames(rng, 256, (6, 8), color, 'encoded')
    got = _device_packed(hip, _Source(hip, frames), (5, 7), color, reverse=True)
    assert_bit_exact(got, packed_ref.preprocess_packed(frames, color, (5, 7), reverse_channels=True), '(256, 6, 8) {} -> 5 x 7'.format(color))


ROI_HW, ROI_DST = (37, 42), (13, 11)
# whole frames; 1 x 1 (the first, an odd and the last pixel); exactly the destination's extent (odd and even origin); odd x / w / y / h
# in every combination; the edges; rows 9 and 12 the same rectangle
ROI_TABLE = np.array([(0, 0, 0, 42, 37), (1, 0, 0, 1, 1), (2, 41, 36, 1, 1), (1, 5, 7, 1, 1), (1, 3, 5, 11, 13), (0, 30, 24, 11, 13),
                      (0, 1, 1, 41, 35), (1, 2, 3, 7, 9), (1, 3, 2, 8, 10), (0, 13, 17, 15, 13), (1, 0, 0, 42, 3), (0, 39, 0, 3, 37),
                      (0, 13, 17, 15, 13), (1, 41, 0, 1, 37), (2, 0, 0, 42, 37), (0, 7, 30, 30, 7)], np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize('color', FORMATS)
def test_packed_roi_kernel_bit_exact(hip, color):
    rng = np.random.default_rng(3742 + KINDS[color])
    assert roi_ref.valid(ROI_TABLE, len(ROI_TABLE), 3, ROI_HW) and (ROI_TABLE[4, 3:] == ROI_DST[::-1]).all()
    frames = _frames(rng, 3, ROI_HW, color, 'encoded')
    options = _options(rng)
    wants = [packed_ref.preprocess_rois(frames, color, ROI_TABLE, ROI_DST, opt.get('reverse', False), opt.get('mean'), opt.get('std'))
             for opt in options]
    for shift in (0, 1, 2, 3):
        src = _Source(hip, frames, shift)
        for opt, want in zip(options, wants):
            got = _device_rois(hip, src, ROI_TABLE, ROI_DST, color, **opt)
            for b in range(len(ROI_TABLE)):                   # row by row: a failure names the rectangle
                assert_bit_exact(got[b], want[b], '{} {} source offset {} row {} = {}'.format(color, sorted(opt), shift, b, ROI_TABLE[b].tolist()))
    # a whole-frame table is the plain entry, device against device; with the frame as the stated maximum and with the table's own
    whole = np.array([(b % 3, 0, 0, ROI_HW[1], ROI_HW[0]) for b in range(5)], np.int32)
    src = _Source(hip, frames)
    for dst_hw in (ROI_DST, (224, 224), ROI_HW):
        plain = _device_packed(hip, src, dst_hw, color, **options[1])
        assert not np.isnan(plain).any()
        assert_bit_exact(_device_rois(hip, src, whole, dst_hw, color, **options[1]), plain[whole[:, 0]], '{} whole-frame table -> {}'.format(color, dst_hw))


@pytest.mark.gpu
@pytest.mark.parametrize('color', FORMATS)
def test_packed_roi_kernel_writes_nan_for_an_invalid_rectangle(hip, color):
    """The table is device data: a row whose rectangle is not inside a frame, or exceeds the stated maxima, comes back all quiet NaN and
    its neighbours exact.  The source has a margin of a whole frame on both sides, and no rectangle here leaves that allocation."""
    rng = np.random.default_rng(99 + KINDS[color])
    m, (H, W), dst_hw = 3, ROI_HW, (9, 12)
    frames = _frames(rng, m, ROI_HW, color, 'encoded')
    src = _Source(hip, frames, margin=1)
    good = [(0, 3, 5, 25, 20), (2, 1, 1, 30, 21), (1, 0, 0, W, H)]
    largest = (21, 30)                                        # the stated maxima: the whole frame exceeds them
    bad = [(1, 0, 0, 31, 21), (1, 0, 0, 30, 22), (0, 4, 4, 0, 5), (0, 4, 4, 5, 0), (m, 3, 5, 25, 20), (-1, 3, 5, 25, 20), (1, W - 24, 5, 25, 20),
           (1, 3, H - 19, 25, 20), (1, -1, 5, 25, 20), (1, 3, -1, 25, 20), (1, 3, 5, -25, 20), (1, 0, 0, W, H)]
    table = np.array([good[0], bad[0], bad[1], good[1], bad[2], bad[3], bad[4], good[0], bad[5], bad[6], bad[7], good[1], bad[8], bad[9],
                      bad[10], bad[11], good[1]], np.int32)
    valid_rows = [b for b in range(len(table)) if tuple(table[b]) in good[:2]]
    assert len(valid_rows) == 5
    want = packed_ref.preprocess_rois(frames, color, table[valid_rows], dst_hw, reverse_channels=True)
    got = _device_rois(hip, src, table, dst_hw, color, m=m, largest=largest, reverse=True)
    for b in range(len(table)):
        if b in valid_rows:
            assert_bit_exact(got[b], want[valid_rows.index(b)], '{} row {} beside invalid ones'.format(color, b))
        else:
            assert np.isnan(got[b]).all(), '{} row {} = {} is not all NaN'.format(color, b, table[b].tolist())
    # with the frame as the stated maximum the whole frame is valid again
    got = _device_rois(hip, src, np.array([good[2], bad[6]], np.int32), dst_hw, color, m=m, largest=ROI_HW)
    assert_bit_exact(got[0], packed_ref.preprocess_rois(frames, color, [good[2]], dst_hw)[0], color + ' whole frame')
    assert np.isnan(got[1]).all()


@pytest.mark.gpu
def test_packed_entries_reject_what_they_cannot_do(hip):
    lib = hip.load_library()
    src = hip.DeviceTensor.from_numpy(np.zeros(256, np.uint8))
    dst = hip.DeviceTensor.from_numpy(np.full(64, 7, np.float32))
    rois = hip.DeviceTensor.from_numpy(np.array([[0, 0, 0, 2, 2]], np.int32))
    s, d, r = ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), ctypes.c_void_p(rois.ptr)
    plain, roi = getattr(lib, ENTRY), getattr(lib, ENTRY_ROI)
    good = (1, 4, 4, 2, 2, 0)                                 # n, src_h, src_w, dst_h, dst_w, kind
    good_roi = (1, 1, 4, 4, 2, 2, 2, 2, 0)                    # n, m, src_h, src_w, dst_h, dst_w, max_roi_h, max_roi_w, kind

    def changed(args, **at):
        out = list(args)
        for k, v in at.items():
            out[int(k[1:])] = v
        return tuple(out)

    # a kind outside 0..3, an odd width with kinds 0 and 1, zero and negative sizes, n > 65535, an image of 2^31 elements or more
    for args in (changed(good, _5=-1), changed(good, _5=4), changed(good, _2=3), changed(good, _2=3, _5=1), changed(good, _2=1, _5=0),
                 changed(good, _0=0), changed(good, _0=-1), changed(good, _0=65536), changed(good, _0=70000), changed(good, _1=0), changed(good, _1=-4),
                 changed(good, _2=0), changed(good, _2=-4), changed(good, _3=0), changed(good, _4=0), changed(good, _3=-2), changed(good, _4=-2),
                 changed(good, _1=40000, _2=40000), changed(good, _1=40000, _2=40000, _5=2), changed(good, _3=40000, _4=40000)):
        assert plain(s, d, *args, 0, None, None) == -2, args  # PVHIP_EINVAL, nothing launched
    # the same, and m < 1 and the maxima outside the frame
    for args in (changed(good_roi, _8=-1), changed(good_roi, _8=4), changed(good_roi, _3=3, _7=3), changed(good_roi, _3=3, _8=1),
                 changed(good_roi, _0=0), changed(good_roi, _0=65536), changed(good_roi, _1=0), changed(good_roi, _1=-1), changed(good_roi, _2=0),
                 changed(good_roi, _3=0), changed(good_roi, _4=0), changed(good_roi, _5=0), changed(good_roi, _6=0), changed(good_roi, _7=0),
                 changed(good_roi, _6=5), changed(good_roi, _7=5), changed(good_roi, _6=-1), changed(good_roi, _2=40000, _3=40000),
                 changed(good_roi, _4=40000, _5=40000, _8=3)):
        assert roi(s, d, r, *args, 0, None, None) == -2, args
    for k in range(4):
        assert plain(None, d, *changed(good, _5=k), 0, None, None) == -2
        assert plain(s, None, *changed(good, _5=k), 0, None, None) == -2
        assert roi(None, d, r, *changed(good_roi, _8=k), 0, None, None) == -2
        assert roi(s, None, r, *changed(good_roi, _8=k), 0, None, None) == -2
        assert roi(s, d, None, *changed(good_roi, _8=k), 0, None, None) == -2
    hip.synchronize()
    assert np.array_equal(np.asarray(dst), np.full(64, 7, np.float32))
    # and the same arguments put right are taken: every kind, an odd height for 4:2:2, an odd width for the X kinds
    for k in range(4):
        assert plain(s, d, *changed(good, _5=k), 0, None, None) == 0
        assert roi(s, d, r, *changed(good_roi, _8=k), 0, None, None) == 0
        assert plain(s, d, *changed(good, _1=3, _5=k), 0, None, None) == 0
    for k in (2, 3):
        assert plain(s, d, *changed(good, _2=3, _5=k), 0, None, None) == 0
        assert roi(s, d, r, *changed(good_roi, _3=3, _7=3, _8=k), 0, None, None) == 0
    hip.synchronize()


def _mean():
    return [104.0, 117.0, 123.0], [1.0, 57.5, 2.0]


def _fixed(ex, name):
    return np.asarray(ex.host_inputs.slots[name].fixed).copy()


def _read(ir, tmp_path, batch, seed=11):
    """GoogLeNet with synthetic weights as an fp32 IR, or as an FP16 IR in either read mode: (ie, net, input name, output name)."""
    from pyopenvino_amd import IECore, synth
    xml = os.path.join(MODELS, 'googlenet-v1.xml')
    blob = _weights('googlenet-v1', seed)
    ie = IECore(plugin_package=HIP)
    if ir == 'fp32':
        net = ie.read_network(xml, weights=blob)
    else:
        xml16, blob16 = synth.fp16_ir(xml, blob, str(tmp_path))
        net = ie.read_network(xml16, weights=blob16, fp16_as_fp32=(ir == 'fp16-as-fp32'))
    net.set_batch(batch)
    return ie, net, net.inputs[0]['name'], net.outputs[0]['name']


@pytest.mark.gpu
@pytest.mark.parametrize('ir', ['fp32', 'fp16-mfma', 'fp16-as-fp32'])
@pytest.mark.parametrize('color', ['YUY2', 'BGRX'])
def test_googlenet_from_packed_frames_matches_the_converted_bgr_frames(hip, tmp_path, color, ir):
    """(2, 480, 640) frames, resize, reverse and mean / scale declared: the Results of the same network declared U8 / NHWC and fed the
    restatement's B, G, R image, through infer() and through the request's own buffer."""
    rng = np.random.default_rng(12 + KINDS[color])
    n, hw = 2, (480, 640)
    frames = _frames(rng, n, hw, color, 'encoded')
    bgr = packed_ref.to_bgr(frames, color)
    mean = _mean()
    ie, net, name, out_name = _read(ir, tmp_path, n)
    _declare(net, name, 'RAW', reverse=True, mean=mean)
    ex_bgr = ie.load_network(net)
    want = np.array(ex_bgr.infer({name: bgr})[out_name], copy=True)
    want_input = _fixed(ex_bgr, name)
    assert np.isfinite(want).all()
    assert_bit_exact(want_input, preprocess(bgr, (224, 224), reverse_channels=True, mean=mean[0], std_scale=mean[1]), 'the U8 / NHWC input tensor')
    ie, net, name, out_name = _read(ir, tmp_path, n)
    assert net.f16_mfma == (ir == 'fp16-mfma')
    _declare(net, name, color, reverse=True, mean=mean)
    ex = ie.load_network(net)
    untouched = frames.copy()
    got = ex.infer({name: frames})[out_name]
    assert np.array_equal(frames, untouched)
    assert_bit_exact(_fixed(ex, name), want_input, color + ' input tensor')
    assert_bit_exact(got, want, '{} {} through infer()'.format(color, frames.shape))
    req = ex.requests[0]
    buf = req.input_buffer(name, hw)
    assert buf.shape == frames.shape and buf.dtype == np.uint8 and req.input_buffer(name, hw) is buf
    buf[...] = frames
    assert_bit_exact(req.infer({name: buf})[out_name], want, color + ' from the request buffer')
    if ir != 'fp32':
        return
    # frames at the network's own extent, no resize declared
    small = _frames(rng, n, (224, 224), color, 'encoded')
    ie, net, name, out_name = _read(ir, tmp_path, n)
    _declare(net, name, 'RAW', resize=False)
    want = np.array(ie.load_network(net).infer({name: packed_ref.to_bgr(small, color)})[out_name], copy=True)
    ie, net, name, out_name = _read(ir, tmp_path, n)
    _declare(net, name, color, resize=False)
    assert_bit_exact(ie.load_network(net).infer({name: small})[out_name], want, color + ' at the network\'s extent')


@pytest.mark.gpu
def test_roi_input_over_uyvy_frames_matches_the_converted_frames(hip, tmp_path):
    from pyopenvino_amd import RoiInput
    rng = np.random.default_rng(2021)
    n, m, hw = 4, 3, (481, 640)
    frames = _frames(rng, m, hw, 'UYVY', 'encoded')
    bgr = packed_ref.to_bgr(frames, 'UYVY')
    table = np.array([(2, 1, 3, 201, 150), (0, 0, 0, 640, 481), (1, 333, 255, 224, 224), (1, 639, 480, 1, 1)], np.int32)
    assert roi_ref.valid(table, n, m, hw)
    mean = _mean()
    ie, net, name, out_name = _read('fp32', tmp_path, n)
    _declare(net, name, 'RAW', reverse=True, mean=mean)
    ex_bgr = ie.load_network(net)
    want = np.array(ex_bgr.infer({name: RoiInput(bgr, table)})[out_name], copy=True)
    want_input = _fixed(ex_bgr, name)
    assert np.isfinite(want).all()
    assert_bit_exact(want_input, packed_ref.preprocess_rois(frames, 'UYVY', table, (224, 224), True, mean[0], mean[1]), 'the rule')
    ie, net, name, out_name = _read('fp32', tmp_path, n)
    _declare(net, name, 'UYVY', reverse=True, mean=mean)
    ex = ie.load_network(net)
    got = ex.infer({name: RoiInput(frames, table)})[out_name]
    assert_bit_exact(_fixed(ex, name), want_input, 'input tensor of the RoiInput')
    assert_bit_exact(got, want, 'RoiInput over UYVY frames')
    req = ex.requests[0]                                      # from the request's own buffers: no host copy, the same Results
    buf, tbuf = req.input_buffer(name, hw, frames=m), req.roi_buffer(name)
    assert buf.shape == (m, 481, 640, 2) and buf.dtype == np.uint8 and tbuf.shape == (n, 5)
    buf[...] = frames
    tbuf[...] = table
    assert_bit_exact(req.infer({name: RoiInput(buf, tbuf)})[out_name], want, 'RoiInput from the request buffers')
    assert len(ex.host_inputs.slots[name].extents) == 1


@pytest.mark.gpu
def test_detected_rois_over_rgbx_frames_matches_the_raw_one(hip, tmp_path):
    """DetectedRois(frames, host records) over RGBX frames: the Results, the input tensor and detected_rois() of the RAW one over the
    converted frames; rows behind `count` are quiet NaN."""
    from pyopenvino_amd import DetectedRois
    rng = np.random.default_rng(77)
    n, m, hw = 4, 2, (240, 321)
    frames = _frames(rng, m, hw, 'RGBX', 'encoded')
    bgr = packed_ref.to_bgr(frames, 'RGBX')
    rec = np.zeros((m * 4, 7), np.float32)
    rec[0] = (0, 1, 0.9, 0.1, 0.2, 0.6, 0.9)
    rec[1] = (1, 2, 0.3, 0.0, 0.0, 1.0, 1.0)                  # below min_confidence
    rec[2] = (2, 1, 0.8, 0.503, 0.31, 0.997, 0.77)
    rec[3, 0] = -1
    rec[4] = (0, 3, 0.7, -0.1, 0.4, 0.35, 1.2)                # clamped to the frame
    rec[5, 0] = -1
    want_table = detected_rois(rec, n, m, hw)
    assert want_table.count == 3 and want_table.selected == 3
    mean = _mean()
    results = {}
    for color, source in (('RAW', bgr), ('RGBX', frames)):
        ie, net, name, out_name = _read('fp32', tmp_path, n)
        _declare(net, name, color, reverse=True, mean=mean)
        ex = ie.load_network(net)
        req = ex.requests[0]
        out = np.array(req.infer({name: DetectedRois(source, rec)})[out_name], copy=True)
        results[color] = (out, _fixed(ex, name), req.detected_rois(name))
    for got in results.values():
        table = got[2]
        assert (table.count, table.selected) == (3, 3) and np.array_equal(table.rois, want_table.rois) and np.array_equal(table.records, want_table.records)
        assert np.isnan(got[1][3:]).all() and np.isfinite(got[1][:3]).all()
    assert_bit_exact(results['RGBX'][1][:3], results['RAW'][1][:3], 'input rows < count')
    assert_bit_exact(results['RGBX'][1][:3], packed_ref.preprocess_rois(frames, 'RGBX', padded(want_table.rois)[:3], (224, 224), True, mean[0], mean[1]),
                     'the rule')
    assert_bit_exact(results['RGBX'][0][:3], results['RAW'][0][:3], 'Results of rows < count')


@pytest.mark.gpu
def test_six_requests_in_flight_two_yuy2_source_extents(hip, tmp_path):
    """Six requests, new YUY2 frames for every request on every step, the source extent alternating between 255 x 256 and 480 x 640 per
    request: every Result equals, bit for bit, the eager Result of the same network fed those frames one request at a time, and after
    the warm-up passes every request replays its recording whatever the source size."""
    B, R = 8, 6
    rng = np.random.default_rng(66)
    extents = [(255, 256), (480, 640)]
    sources = [_frames(rng, B, extents[k % 2], 'YUY2', 'encoded') for k in range(4)]
    mean = ([104.0, 117.0, 123.0], [1.0, 1.0, 1.0])

    def loaded(requests):
        ie, net, name, out_name = _read('fp32', tmp_path, B, seed=5)
        _declare(net, name, 'YUY2', mean=mean)
        return ie.load_network(net, 'GPU', num_requests=requests), name, out_name

    want = []
    for src in sources:                                       # the first pass of a newly loaded network: dispatched eagerly, nothing recorded yet
        ex_ref, name, out_name = loaded(1)
        want.append(np.array(ex_ref.infer({name: src})[out_name], copy=True))
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
            k = (r + step) % 4                                # extent (r + step) % 2: alternates per request, and new frames every step
            req = ex.requests[r]
            if r % 2:                                         # half the requests from their own page-locked buffers, half from pageable arrays
                buf = req.input_buffer(name, extents[k % 2])
                np.copyto(buf, sources[k])
                feed = buf
            else:
                feed = sources[k]
            ex.start_async(r, {name: feed})
            fed[r] = k
            if step >= 3:
                assert req._replayed is not None, 'step {} request {} was not replayed'.format(step, r)
        for r in reversed(order):
            got = ex.wait(r)[out_name]
            assert np.array_equal(got, want[fed[r]]), 'step {} request {} (source {})'.format(step, r, extents[fed[r] % 2])
    for req in ex.requests:
        assert len(req.runner.host_inputs.slots[name].extents) <= ex.MAX_SOURCE_EXTENTS
