"""YUV 4:2:0 host inputs (IENetwork.input_info[name].preprocess_info.color_format 'NV12' / 'I420'): a decoder's frames, uint8 of shape
(n, 3 h / 2, w), converted to B, G, R on the device in the launch that resizes, reverses and scales them
(pvhip_input_preprocess_yuv_f32), bit for bit tests/yuv_ref.py followed by tests/preprocess_ref.py.  The first tests need no GPU."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import helpers
import yuv_ref
from helpers import MODELS, assert_bit_exact
from preprocess_ref import preprocess

HIP = 'pyopenvino_amd.op_plugins'
FORMATS = ['NV12', 'I420']
ENTRY = 'pvhip_input_preprocess_yuv_f32'


@functools.lru_cache(maxsize=None)
def _weights(model):
    """mnist ships its weights; the other IRs get seeded synthetic ones."""
    from pyopenvino_amd import synth
    return None if model == 'mnist' else synth.synth_weights(os.path.join(MODELS, model + '.xml'), 7)


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


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
def test_color_format_defaults_case_and_declaring():
    _, net, name = _net()
    info = net.input_info[name]
    pre = info.preprocess_info
    assert pre.color_format == 'RAW' and not info.declared
    assert info.frozen().color == 'RAW' and not info.frozen().yuv
    assert info.preprocessing() == (False, False, None)
    pre.color_format = 'nv12'                                 # accepted in any case, reported upper case
    assert pre.color_format == 'NV12' and info.declared
    pre.color_format = 'i420'
    assert pre.color_format == 'I420'
    pre.color_format = 'Raw'
    assert pre.color_format == 'RAW'
    assert (info.precision, info.layout) == ('FP32', 'NCHW')
    assert info.preprocessing() == (False, False, None)       # still the 3-tuple it was
    _, net2, name2 = _net()
    net2.input_info[name2].preprocess_info.color_format = 'RAW'        # setting the default value declares the input too
    assert net2.input_info[name2].declared
    assert net2.input_info[name2].host_format() == ((1, 3, 224, 224), np.dtype(np.float32))


def test_color_format_rejects_bad_values_and_is_frozen_at_load():
    ie, net, name = _net('mnist')
    info = net.input_info[name]
    pre = info.preprocess_info
    for bad in ('YUV', 'NV21', 'BGR', '', None, 12, True):
        with pytest.raises(ValueError, match='color_format'):
            pre.color_format = bad
    assert pre.color_format == 'RAW' and not info.declared
    ie.load_network(net)
    for value in ('NV12', 'I420', 'RAW'):
        with pytest.raises(ValueError, match='between read_network and load_network'):
            pre.color_format = value
    assert pre.color_format == 'RAW'


def test_color_format_only_for_4d_f32_parameters():
    _, net, name = _net('mnist')
    nid = next(n for n in net.G.nodes if net.G.nodes[n]['name'] == name)
    pre = net.input_info[name].preprocess_info
    net.G.nodes[nid]['data']['element_type'] = 'i32'
    with pytest.raises(NotImplementedError):
        pre.color_format = 'NV12'
    assert pre.color_format == 'RAW' and not net.input_info[name].declared


@pytest.mark.parametrize('color', FORMATS)
def test_frozen_carries_the_format(color):
    import dataclasses
    _, net, name = _net()
    info = net.input_info[name]
    pre = info.preprocess_info
    pre.color_format = color
    pre.reverse_channels = True
    pre.init(3)
    pre[1].mean_value = 117
    pre.mean_variant = 'MEAN_VALUE'
    fmt = info.frozen()
    assert (fmt.color, fmt.yuv, fmt.u8, fmt.resize, fmt.reverse) == (color, True, True, False, True)
    assert fmt.mean.tolist() == [0, 117, 0] and fmt.std.tolist() == [1, 1, 1]
    assert fmt.host_dtype == np.dtype(np.uint8)
    assert fmt.needs_preprocess((224, 224)) and fmt.needs_convert((224, 224))
    with pytest.raises(dataclasses.FrozenInstanceError):
        fmt.color = 'RAW'
    assert info.preprocessing()[:2] == (False, True)


@pytest.mark.parametrize('resize', [False, True])
@pytest.mark.parametrize('color', FORMATS)
def test_yuv_shape_rules(color, resize):
    """host_format, InputFormat.host_shape / extent_of / checked_extent and input_buffer at the network's extent and at another one;
    odd extents and arrays of other shapes are refused with one text by the format and by infer(), before anything reaches the device."""
    ie, net, name = _net(batch=2)
    info = net.input_info[name]
    info.preprocess_info.color_format = color
    info.layout = 'NHWC'                                      # not consulted
    if resize:
        info.preprocess_info.resize_algorithm = 'RESIZE_BILINEAR'
    fmt = info.frozen()
    u8 = np.dtype(np.uint8)
    assert info.host_format() == info.host_format((224, 224)) == ((2, 336, 224), u8)
    assert fmt.host_shape() == (2, 336, 224) and fmt.checked_extent() == (224, 224)
    assert fmt.extent_of(np.empty((2, 336, 224), np.uint8)) == (224, 224)
    other = [(480, 640), (482, 642), (2, 2)]                  # (482 % 4 == 2: I420's U plane ends in the middle of a row)
    for h, w in other:
        if resize:
            assert info.host_format((h, w)) == ((2, 3 * h // 2, w), u8)
            assert fmt.host_shape((h, w)) == (2, 3 * h // 2, w) and fmt.checked_extent((h, w)) == (h, w)
            assert fmt.extent_of(np.empty((2, 3 * h // 2, w), np.uint8)) == (h, w)
        else:
            for refused in (info.host_format, fmt.checked_extent):
                with pytest.raises(ValueError, match='no resize is declared'):
                    refused((h, w))
    for odd in ((223, 224), (224, 223), (481, 640), (480, 641), (1, 1)):
        for refused in (info.host_format, fmt.checked_extent, info.source_extent):
            with pytest.raises(ValueError, match='even height and width'):
                refused(odd)
    ex = ie.load_network(net)
    for odd in ((481, 640), (480, 641)):
        with pytest.raises(ValueError, match='even height and width'):
            ex.requests[0].input_buffer(name, odd)
    if not resize:
        with pytest.raises(ValueError, match='no resize is declared'):
            ex.requests[0].input_buffer(name, (480, 640))
    # wrong batch, a BGR image, no batch, a row count that is no 3 h / 2, an odd width, no rows, (no resize) another extent
    bad = [(3, 336, 224), (2, 224, 224, 3), (2, 3, 224, 224), (336, 224), (2, 337, 224), (2, 336, 223), (2, 0, 224)]
    bad += [] if resize else [(2, 720, 640)]
    for shape in bad:
        with pytest.raises(ValueError) as by_format:
            fmt.extent_of(np.empty(shape, np.uint8))
        with pytest.raises(ValueError) as by_infer:           # refused before anything reaches the device
            ex.infer({name: np.empty(shape, np.uint8)})
        assert str(by_format.value) == str(by_infer.value), shape
        assert str(by_format.value).startswith('input {}: '.format(name)), str(by_format.value)


@pytest.mark.parametrize('color', FORMATS)
def test_channel_count_extent_and_precision_are_checked_at_load(color):
    ie, net, name = _net('mnist')                             # one channel
    net.input_info[name].preprocess_info.color_format = color
    with pytest.raises(ValueError, match='3 channels'):
        ie.load_network(net)
    net.input_info[name].preprocess_info.color_format = 'RAW'
    ie.load_network(net)
    ie, net, name = _reshaped((1, 4, 28, 28))
    net.input_info[name].preprocess_info.color_format = color
    with pytest.raises(ValueError, match='3 channels'):
        ie.load_network(net)
    for shape in ((1, 3, 27, 28), (1, 3, 28, 27)):            # the frames have the network's extent: it must be even
        ie, net, name = _reshaped(shape)
        net.input_info[name].preprocess_info.color_format = color
        with pytest.raises(ValueError, match='even height and width'):
            ie.load_network(net)
        with pytest.raises(ValueError, match='even height and width'):
            net.input_info[name].host_format()
        net.input_info[name].preprocess_info.resize_algorithm = 'RESIZE_BILINEAR'     # sources of any even extent: nothing to refuse
        assert net.input_info[name].host_format((30, 40)) == ((1, 45, 40), np.dtype(np.uint8))
        with pytest.raises(ValueError, match='even height and width'):
            net.input_info[name].host_format()                # (the default source extent is the network's)
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
            assert info.host_format() == ((1, 336, 224), np.dtype(np.uint8))


def test_restatement_converts_the_known_triples():
    for (y, u, v), bgr in (((235, 128, 128), (255, 255, 255)), ((16, 128, 128), (0, 0, 0)), ((126, 128, 128), (128, 128, 128)),
                           ((81, 90, 240), (0, 0, 254))):
        assert yuv_ref.convert(y, u, v).tolist() == list(bgr), (y, u, v)
    assert yuv_ref.convert(np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 3))).shape == (2, 3, 3)


def test_restatement_nv12_and_i420_of_the_same_planes_give_the_same_image():
    rng = np.random.default_rng(420)
    for h, w in ((2, 2), (6, 10), (38, 42), (480, 640)):      # (6 % 4 == 2, 38 % 4 == 2: the U plane ends in the middle of a row)
        y = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
        u, v = rng.integers(0, 256, (2, 2, h // 2, w // 2), dtype=np.uint8)
        images = []
        for color in FORMATS:
            frames = yuv_ref.frames_of(y, u, v, color)
            assert frames.shape == (2, 3 * h // 2, w) and frames.dtype == np.uint8
            assert np.array_equal(frames[:, :h], y)
            for got, want in zip(yuv_ref.planes(frames, color), (y, u, v)):
                assert np.array_equal(got, want)
            images.append(yuv_ref.to_bgr(frames, color))
        assert images[0].shape == (2, h, w, 3) and np.array_equal(images[0], images[1])
        # pixel (y, x) takes the chroma of block (y // 2, x // 2)
        yy, xx = h - 1, w - 2
        assert images[0][1, yy, xx].tolist() == yuv_ref.convert(y[1, yy, xx], u[1, yy // 2, xx // 2], v[1, yy // 2, xx // 2]).tolist()
    nv12 = yuv_ref.frames_of(y, u, v, 'NV12')
    assert np.array_equal(nv12[:, h:, 0::2], u) and np.array_equal(nv12[:, h:, 1::2], v)


def test_restatement_against_the_float64_matrix_over_all_byte_triples():
    """All 2^24 (Y, U, V): the 32-bit evaluation equals the 64-bit one (nothing overflows: every intermediate within +-5.7e8) and every
    channel is within 1 of the rounded float64 value of the BT.601 matrix with the constants over 2^20."""
    k = [c / 2.0 ** 20 for c in (yuv_ref.CY, yuv_ref.CRV, yuv_ref.CGV, yuv_ref.CGU, yuv_ref.CBU)]
    assert [round(c, 3) for c in k] == [1.164, 1.596, 0.813, 0.391, 2.018]
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    uf, vf = u - 128.0, v - 128.0
    u64, v64 = (u - 128).astype(np.int64), (v - 128).astype(np.int64)
    worst, biggest = 0.0, 0
    for y in range(256):
        got = yuv_ref.convert(np.full_like(u, y), u, v).astype(np.float64)
        yl = k[0] * max(y - 16, 0)
        want = np.stack([yl + k[4] * uf, yl - k[2] * vf - k[3] * uf, yl + k[1] * vf], -1)
        worst = max(worst, float(np.abs(got - np.rint(np.clip(want, 0, 255))).max()))
        t = max(y - 16, 0) * yuv_ref.CY + (1 << 19)
        wide = np.stack([t + yuv_ref.CBU * u64, t - yuv_ref.CGV * v64 - yuv_ref.CGU * u64, t + yuv_ref.CRV * v64], -1)
        biggest = max(biggest, int(np.abs(wide).max()), int(np.abs(yuv_ref.CGV * v64).max()))
        assert np.array_equal(got, np.clip(wide >> 20, 0, 255)), y
    assert worst <= 1.0, worst
    assert biggest <= 5.7e8 < 2 ** 31, biggest


def test_forward_converted_frames_mostly_do_not_saturate():
    rng = np.random.default_rng(601)
    bgr = rng.integers(0, 256, (2, 48, 64, 3), dtype=np.uint8)
    back = yuv_ref.to_bgr(yuv_ref.frames_of(*yuv_ref.planes_from_bgr(bgr), 'NV12'), 'NV12')
    assert ((back > 0) & (back < 255)).mean() >= 0.5
    flat = np.full((1, 4, 4, 3), (40, 120, 200), np.uint8)    # a flat image comes back within the rounding of Y, U, V
    back = yuv_ref.to_bgr(yuv_ref.frames_of(*yuv_ref.planes_from_bgr(flat), 'I420'), 'I420')
    assert np.abs(back.astype(int) - flat.astype(int)).max() <= 2


def test_abi_declares_the_yuv_entry():
    from pyopenvino_amd import device
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    assert ENTRY in device.SIGNATURES and ENTRY + '(' in header
    assert len(device.SIGNATURES[ENTRY][1]) == 11
    assert re.search(r'#define\s+PVHIP_ABI_VERSION\s+19\b', header)
    lib = device.load_library()
    assert hasattr(lib, ENTRY) and lib.pvhip_abi_version() == 19


# ---------------------------------------------------------------------------------------------------------------- GPU
def _frames(rng, n, hw, color, kind):
    """n frames of extent hw: 'bytes' uniform random bytes (85 % of triples saturate: the clamp), 'encoded' random B, G, R images
    converted forward (mostly unsaturated arithmetic)."""
    h, w = hw
    if kind == 'bytes':
        return rng.integers(0, 256, (n, 3 * h // 2, w), dtype=np.uint8)
    return yuv_ref.frames_of(*yuv_ref.planes_from_bgr(rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)), color)


def _device_yuv(hip, frames, dst_hw, color, reverse=False, mean=None, std=None, shift=0):
    """pvhip_input_preprocess_yuv_f32 on frames (n, 3 h / 2, w); shift > 0 moves the source off 16-byte alignment."""
    n, rows, w = frames.shape
    raw = np.zeros(frames.nbytes + shift, np.uint8)
    raw[shift:] = np.ascontiguousarray(frames).reshape(-1)
    src = hip.DeviceTensor.from_numpy(raw)
    dst = hip.DeviceTensor.empty((n, 3) + tuple(dst_hw))
    hip.call('pvhip_memset', ctypes.c_void_p(dst.ptr), 0x7f, dst.nbytes)
    m = hip.DeviceTensor.from_numpy(np.asarray(mean, np.float32)) if mean is not None else None
    s = hip.DeviceTensor.from_numpy(np.asarray(std, np.float32)) if std is not None else None
    hip.call(ENTRY, ctypes.c_void_p(src.ptr + shift), ctypes.c_void_p(dst.ptr), n, rows // 3 * 2, w, dst_hw[0], dst_hw[1],
             int(color == 'I420'), int(reverse), ctypes.c_void_p(m.ptr) if m is not None else None,
             ctypes.c_void_p(s.ptr) if s is not None else None)
    return np.asarray(dst)


def _check_kernel(hip, rng, n, src_hw, dst_hw, color, options, shifts):
    for kind in ('bytes', 'encoded'):
        frames = _frames(rng, n, src_hw, color, kind)
        bgr = yuv_ref.to_bgr(frames, color)
        if kind == 'encoded':                                 # the unsaturated arithmetic is really exercised
            inside = float(((bgr > 0) & (bgr < 255)).mean())
            assert inside >= 0.5, '{} {}: {:.2f} of the converted values inside (0, 255)'.format(color, src_hw, inside)
        for opt in options:
            want = preprocess(bgr, dst_hw, nhwc=True, reverse_channels=opt.get('reverse', False), mean=opt.get('mean'), std_scale=opt.get('std'))
            for shift in shifts:
                what = '{} {} frames {} -> {} {} source offset {}'.format(color, kind, src_hw, dst_hw, sorted(opt), shift)
                assert_bit_exact(_device_yuv(hip, frames, dst_hw, color, shift=shift, **opt), want, what)


KERNEL_SHAPES = [((480, 640), (224, 224)), ((482, 642), (300, 300)), ((2, 2), (5, 3)), ((2, 2), (224, 224)), ((38, 42), (13, 1)),
                 ((20, 30), (20, 30))]


@pytest.mark.gpu
@pytest.mark.parametrize('src_hw,dst_hw', KERNEL_SHAPES)
@pytest.mark.parametrize('color', FORMATS)
def test_yuv_kernel_bit_exact(hip, color, src_hw, dst_hw):
    rng = np.random.default_rng(sum(src_hw) * 31 + sum(dst_hw) * 3 + len(color))
    mean = rng.uniform(0, 255, 3).astype(np.float32)
    std = rng.uniform(0.5, 80, 3).astype(np.float32)
    options = [dict(), dict(reverse=True, mean=mean, std=std), dict(reverse=True), dict(mean=mean), dict(std=std)]
    _check_kernel(hip, rng, 2, src_hw, dst_hw, color, options, (0, 1, 2, 3))


# Rows whose sources exceed the kernel's 48 KiB of LDS (2 Y rows of 14000 bytes and the chroma under them: 56 KB), so the output rows are
# split into column tiles that start at tx0 > 0, on even and on odd source columns.
@pytest.mark.gpu
@pytest.mark.parametrize('src_hw,dst_hw', [((4, 14000), (2, 224)), ((2, 30000), (2, 30000)), ((6, 14002), (5, 227))])
@pytest.mark.parametrize('color', FORMATS)
def test_yuv_kernel_bit_exact_in_column_tiles(hip, color, src_hw, dst_hw):
    rng = np.random.default_rng(src_hw[1] + dst_hw[1])
    mean = rng.uniform(0, 255, 3).astype(np.float32)
    std = rng.uniform(0.5, 80, 3).astype(np.float32)
    _check_kernel(hip, rng, 1, src_hw, dst_hw, color, [dict(reverse=True, mean=mean, std=std), dict()], (0, 3))


@pytest.mark.gpu
@pytest.mark.parametrize('color', FORMATS)
def test_yuv_kernel_bit_exact_batch256(hip, color):
    rng = np.random.default_rng(256)
    frames = np.concatenate([_frames(rng, 32, (480, 640), color, 'encoded' if i % 2 else 'bytes') for i in range(8)], 0)
    got = _device_yuv(hip, frames, (224, 224), color)
    for i in range(0, 256, 32):
        want = preprocess(yuv_ref.to_bgr(frames[i:i + 32], color), (224, 224))
        assert_bit_exact(got[i:i + 32], want, '(256, 720, 640) {} -> 224 x 224, images {}..'.format(color, i))


@pytest.mark.gpu
def test_yuv_kernel_rejects_what_it_cannot_do(hip):
    lib = hip.load_library()
    src = hip.DeviceTensor.from_numpy(np.zeros(64, np.uint8))
    dst = hip.DeviceTensor.from_numpy(np.full(64, 7, np.float32))
    s, d = ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr)
    fn = getattr(lib, ENTRY)
    # (n, src_h, src_w, dst_h, dst_w, planar): odd extents, zero sizes, a planar flag that is neither format, an image past 2^31
    for args in ((1, 3, 4, 2, 2, 0), (1, 4, 3, 2, 2, 1), (1, 1, 1, 2, 2, 0), (0, 4, 4, 2, 2, 0), (1, 0, 4, 2, 2, 0), (1, 4, 0, 2, 2, 1),
                 (1, 4, 4, 0, 2, 0), (1, 4, 4, 2, 0, 1), (-1, 4, 4, 2, 2, 0), (70000, 4, 4, 2, 2, 0), (1, 4, 4, 2, 2, 2), (1, 4, 4, 2, 2, -1),
                 (1, 40000, 40000, 2, 2, 0), (1, 4, 4, 40000, 40000, 0)):
        assert fn(s, d, *args, 0, None, None) == -2, args     # PVHIP_EINVAL, nothing launched
    assert fn(None, d, 1, 4, 4, 2, 2, 0, 0, None, None) == -2
    assert fn(s, None, 1, 4, 4, 2, 2, 0, 0, None, None) == -2
    assert np.array_equal(np.asarray(dst), np.full(64, 7, np.float32))
    assert fn(s, d, 1, 4, 4, 2, 2, 0, 0, None, None) == 0     # (and the same arguments in order are taken)


def _declare_yuv(net, name, color, resize=True, reverse=False, mean=None):
    pre = net.input_info[name].preprocess_info
    pre.color_format = color
    if resize:
        pre.resize_algorithm = 'RESIZE_BILINEAR'
    pre.reverse_channels = reverse
    if mean is not None:
        pre.init(3)
        for c in range(3):
            pre[c].mean_value, pre[c].std_scale = mean[0][c], mean[1][c]
        pre.mean_variant = 'MEAN_VALUE'


def _declare_bgr(net, name, resize=True, reverse=False, mean=None):
    info = net.input_info[name]
    info.precision, info.layout = 'U8', 'NHWC'
    _declare_yuv(net, name, 'RAW', resize, reverse, mean)


@pytest.mark.gpu
@pytest.mark.parametrize('color', FORMATS)
def test_googlenet_from_yuv_frames_matches_the_converted_bgr_frames(hip, color):
    """(480, 640) frames, resize and mean / scale declared: the Results of the U8 / NHWC path fed the restatement's B, G, R image."""
    from pyopenvino_amd import synth
    blob = synth.synth_weights(os.path.join(MODELS, 'googlenet-v1.xml'), 11)
    rng = np.random.default_rng(12)
    frames = _frames(rng, 8, (480, 640), color, 'encoded')
    bgr = yuv_ref.to_bgr(frames, color)
    mean = ([104.0, 117.0, 123.0], [1.0, 57.5, 2.0])
    ie, net, name = _net('googlenet-v1', 8, blob)
    out_name = net.outputs[0]['name']
    _declare_bgr(net, name, mean=mean)
    ex_bgr = ie.load_network(net)
    want = np.array(ex_bgr.infer({name: bgr})[out_name], copy=True)
    want_input = np.asarray(ex_bgr.host_inputs.slots[name].fixed).copy()
    assert np.isfinite(want).all()
    assert_bit_exact(want_input, preprocess(bgr, (224, 224), mean=mean[0], std_scale=mean[1]), 'the U8 / NHWC input tensor')
    ie, net, name = _net('googlenet-v1', 8, blob)
    _declare_yuv(net, name, color, mean=mean)
    ex = ie.load_network(net)
    got = ex.infer({name: frames})[out_name]
    assert_bit_exact(np.asarray(ex.host_inputs.slots[name].fixed), want_input, color + ' input tensor')
    assert_bit_exact(got, want, color + ' (8, 720, 640) through infer()')
    req = ex.requests[0]
    buf = req.input_buffer(name, (480, 640))
    assert buf.shape == (8, 720, 640) and buf.dtype == np.uint8 and req.input_buffer(name, (480, 640)) is buf
    buf[...] = frames
    assert_bit_exact(req.infer({name: buf})[out_name], want, color + ' from the request buffer')
    # frames at the network's own extent, no resize declared
    small = _frames(rng, 8, (224, 224), color, 'encoded')
    ie, net, name = _net('googlenet-v1', 8, blob)
    _declare_bgr(net, name, resize=False)
    want = np.array(ie.load_network(net).infer({name: yuv_ref.to_bgr(small, color)})[out_name], copy=True)
    ie, net, name = _net('googlenet-v1', 8, blob)
    _declare_yuv(net, name, color, resize=False)
    assert_bit_exact(ie.load_network(net).infer({name: small})[out_name], want, color + ' at the network\'s extent')


@pytest.mark.gpu
@pytest.mark.parametrize('color', FORMATS)
def test_ssd_from_yuv_frames_with_reversed_channels(hip, color):
    from pyopenvino_amd import synth
    blob = synth.synth_weights(os.path.join(MODELS, 'ssd_mobilenet_v1_coco.xml'), 1234)
    rng = np.random.default_rng(301)
    frames = _frames(rng, 2, (480, 640), color, 'encoded')
    ie, net, name = _net('ssd_mobilenet_v1_coco', 2, blob)
    out_name = net.outputs[0]['name']
    _declare_bgr(net, name, reverse=True)
    want = np.array(ie.load_network(net).infer({name: yuv_ref.to_bgr(frames, color)})[out_name], copy=True)
    ie, net, name = _net('ssd_mobilenet_v1_coco', 2, blob)
    _declare_yuv(net, name, color, reverse=True)
    got = ie.load_network(net).infer({name: frames})[out_name]
    assert_bit_exact(got, want, 'SSD from (2, 720, 640) {} frames as R, G, B'.format(color))


@pytest.mark.gpu
def test_six_requests_in_flight_two_yuv_source_extents(hip):
    """Six requests, new NV12 frames for every request on every step, the source extent alternating between 256 x 256 and 480 x 640 per
    request: every Result equals, bit for bit, the eager Result of the same network fed those frames one request at a time, and after
    the warm-up passes every request replays its recording whatever the source size."""
    from pyopenvino_amd import synth
    blob = synth.synth_weights(os.path.join(MODELS, 'googlenet-v1.xml'), 5)
    B, R = 64, 6
    rng = np.random.default_rng(66)
    extents = [(256, 256), (480, 640)]
    sources = [_frames(rng, B, extents[k % 2], 'NV12', 'encoded') for k in range(4)]
    mean = ([104.0, 117.0, 123.0], [1.0, 1.0, 1.0])

    def loaded(requests):
        ie, net, name = _net('googlenet-v1', B, blob)
        _declare_yuv(net, name, 'NV12', mean=mean)
        return ie.load_network(net, 'GPU', num_requests=requests), name, net.outputs[0]['name']

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
