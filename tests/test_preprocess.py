"""Input preprocessing on the device (IENetwork.input_info[name].preprocess_info): bilinear resize of a source of any extent, channel
reversal and per-channel mean / scale, in one launch with the format change (pvhip_input_preprocess_f32), bit for bit the numpy
restatement tests/preprocess_ref.py.  The first tests need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import helpers
from helpers import MODELS, assert_bit_exact
from preprocess_ref import preprocess, taps

HIP = 'pyopenvino_amd.op_plugins'


def _net(model='mnist', batch=1, blob=None):
    from pyopenvino_amd import IECore
    ie = IECore(plugin_package=HIP)
    net = ie.read_network(os.path.join(MODELS, model + '.xml'), weights=blob)
    if batch != 1:
        net.set_batch(batch)
    return ie, net, net.inputs[0]['name']


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
def test_preprocess_info_defaults_and_declaring():
    _, net, name = _net()
    info = net.input_info[name]
    pre = info.preprocess_info
    assert info.preprocess_info is pre
    assert (pre.resize_algorithm, pre.mean_variant, pre.reverse_channels, len(pre)) == ('NO_RESIZE', 'NONE', False, 0)
    assert not info.declared and info.preprocessing() == (False, False, None)
    pre.resize_algorithm = 'resize_bilinear'                  # accepted in any case, reported upper case
    assert pre.resize_algorithm == 'RESIZE_BILINEAR' and info.declared
    assert (info.precision, info.layout) == ('FP32', 'NCHW')
    pre.reverse_channels = True
    pre.init(1)
    assert (pre[0].mean_value, pre[0].std_scale) == (0.0, 1.0)
    pre[0].mean_value, pre[0].std_scale = 127.5, 2
    assert info.preprocessing()[2] is None                    # MEAN_VALUE not chosen yet
    pre.mean_variant = 'mean_value'
    resize, reverse, (mean, std) = info.preprocessing()
    assert resize and reverse and mean.tolist() == [127.5] and std.tolist() == [2.0]
    assert mean.dtype == std.dtype == np.float32
    _, net2, name2 = _net()
    net2.input_info[name2].preprocess_info.reverse_channels = False    # setting the default value declares the input too
    assert net2.input_info[name2].declared


def test_preprocess_info_rejects_bad_values():
    _, net, name = _net()
    info = net.input_info[name]
    pre = info.preprocess_info
    for what, bad in (('resize_algorithm', 'RESIZE_AREA'), ('resize_algorithm', None), ('mean_variant', 'MEAN_IMAGE'), ('mean_variant', 1),
                      ('reverse_channels', 'yes'), ('reverse_channels', 1)):
        with pytest.raises(ValueError):
            setattr(pre, what, bad)
    assert not info.declared
    assert (pre.resize_algorithm, pre.mean_variant, pre.reverse_channels) == ('NO_RESIZE', 'NONE', False)
    with pytest.raises(IndexError):
        pre[0]                                                # init() first
    for bad in (0, -1, 1.5, True, '3'):
        with pytest.raises(ValueError):
            pre.init(bad)
    pre.init(2)
    with pytest.raises(ValueError, match='std_scale'):
        pre[1].std_scale = 0
    with pytest.raises(ValueError, match='std_scale'):
        pre[1].std_scale = 1e-50                              # 0 in fp32
    for bad in (float('nan'), float('inf'), 1e39, 'x', None, True):
        with pytest.raises(ValueError):
            pre[1].mean_value = bad
        with pytest.raises(ValueError):
            pre[1].std_scale = bad
    assert (pre[1].mean_value, pre[1].std_scale) == (0.0, 1.0)
    pre[1].mean_value = 0.1
    assert pre[1].mean_value == float(np.float32(0.1))        # what the device uses
    for bad in (2, -1, '0'):
        with pytest.raises(IndexError):
            pre[bad]


def test_refused_values_leave_the_input_undeclared():
    _, net, name = _net()
    info = net.input_info[name]
    pre = info.preprocess_info
    pre.init(1)
    info.declared = False                                     # (init() declares; start from an undeclared input with a channel)
    for what, bad in (('std_scale', 0), ('std_scale', 1e-50), ('std_scale', float('nan')), ('mean_value', float('inf'))):
        with pytest.raises(ValueError):
            setattr(pre[0], what, bad)
        assert not info.declared, (what, bad)
    for what, bad in (('resize_algorithm', 'RESIZE_AREA'), ('reverse_channels', 'yes')):
        with pytest.raises(ValueError):
            setattr(pre, what, bad)
        assert not info.declared, (what, bad)
    with pytest.raises(ValueError):
        pre.init(0)
    assert not info.declared and len(pre) == 1
    pre[0].std_scale = 0.5
    assert info.declared and pre[0].std_scale == 0.5


def test_preprocess_info_is_frozen_at_load_and_checks_the_channel_count():
    ie, net, name = _net()
    pre = net.input_info[name].preprocess_info
    pre.mean_variant = 'MEAN_VALUE'
    with pytest.raises(ValueError, match='channels'):
        ie.load_network(net)                                  # MEAN_VALUE without init()
    pre.init(3)                                               # mnist's input has one channel
    with pytest.raises(ValueError, match='channels'):
        ie.load_network(net)
    pre.init(1)
    pre[0].mean_value = 33
    ie.load_network(net)
    for what, value in (('resize_algorithm', 'RESIZE_BILINEAR'), ('mean_variant', 'NONE'), ('reverse_channels', True)):
        with pytest.raises(ValueError, match='between read_network and load_network'):
            setattr(pre, what, value)
    with pytest.raises(ValueError, match='between read_network and load_network'):
        pre.init(1)
    with pytest.raises(ValueError, match='between read_network and load_network'):
        pre[0].mean_value = 1
    with pytest.raises(ValueError, match='between read_network and load_network'):
        pre[0].std_scale = 2
    assert (pre.mean_variant, pre[0].mean_value, pre[0].std_scale, len(pre)) == ('MEAN_VALUE', 33.0, 1.0, 1)


def test_preprocess_info_only_for_4d_f32_parameters():
    _, net, name = _net()
    nid = next(n for n in net.G.nodes if net.G.nodes[n]['name'] == name)
    net.G.nodes[nid]['data']['element_type'] = 'i64'
    with pytest.raises(NotImplementedError):
        net.input_info[name].preprocess_info
    net.G.nodes[nid]['data']['element_type'] = 'f32'
    net.G.nodes[nid]['data']['shape'] = (1, 784)
    with pytest.raises(NotImplementedError):
        net.input_info[name].preprocess_info
    net.G.nodes[nid]['data']['shape'] = (1, 1, 28, 28)
    pre = net.input_info[name].preprocess_info
    net.G.nodes[nid]['data']['element_type'] = 'i32'         # (the object handed out before: setting through it is refused too)
    with pytest.raises(NotImplementedError):
        pre.resize_algorithm = 'RESIZE_BILINEAR'


def test_host_format_and_source_size_rules():
    ie, net, name = _net()
    info = net.input_info[name]
    assert info.host_format() == info.host_format((28, 28)) == ((1, 1, 28, 28), np.dtype(np.float32))
    with pytest.raises(ValueError, match='no resize is declared'):
        info.host_format((32, 32))
    info.precision, info.layout = 'U8', 'NHWC'
    assert info.host_format() == ((1, 28, 28, 1), np.dtype(np.uint8))
    with pytest.raises(ValueError, match='no resize is declared'):
        info.host_format((480, 640))
    info.preprocess_info.resize_algorithm = 'RESIZE_BILINEAR'
    assert info.host_format() == ((1, 28, 28, 1), np.dtype(np.uint8))
    assert info.host_format((480, 640)) == ((1, 480, 640, 1), np.dtype(np.uint8))
    assert info.host_format([1, 3]) == ((1, 1, 3, 1), np.dtype(np.uint8))
    with pytest.raises(ValueError):
        info.host_format((0, 5))
    ex = ie.load_network(net)
    # the caller's array is checked before anything reaches the device
    for bad in (np.zeros((1, 480, 640, 3), np.uint8), np.zeros((2, 480, 640, 1), np.uint8), np.zeros((480, 640, 1), np.uint8),
                np.zeros((1, 0, 640, 1), np.uint8)):
        with pytest.raises(ValueError):
            ex.infer({name: bad})
    ie2, net2, name2 = _net()
    net2.input_info[name2].precision = 'U8'
    ex2 = ie2.load_network(net2)
    with pytest.raises(ValueError, match='means shape'):
        ex2.infer({name2: np.zeros((1, 1, 32, 32), np.uint8)})
    with pytest.raises(ValueError, match='no resize is declared'):
        ex2.requests[0].input_buffer(name2, (32, 32))
    with pytest.raises(KeyError):
        ex2.requests[0].input_buffer('no such input', (32, 32))


RESTATED_SHAPES = [((480, 640), (224, 224)), ((1080, 1920), (224, 224)), ((481, 643), (300, 300)), ((7, 9), (224, 224)),
                   ((1, 1), (5, 3)), ((28, 28), (57, 31))]


@pytest.mark.parametrize('src_hw,dst_hw', RESTATED_SHAPES)
def test_restatement_matches_float64_torch_interpolate(src_hw, dst_hw):
    torch = pytest.importorskip('torch')
    rng = np.random.default_rng(sum(src_hw) * 7 + sum(dst_hw))
    x = rng.integers(0, 256, (1,) + src_hw + (3,), dtype=np.uint8)
    x.reshape(-1)[:2] = (0, 255)
    got = preprocess(x, dst_hw)
    t = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)).astype(np.float64))
    want = torch.nn.functional.interpolate(t, size=dst_hw, mode='bilinear', align_corners=False).numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - want).max()) / 255.0
    assert err <= 1e-6, '{} -> {}: {:.3e} of the value range'.format(src_hw, dst_hw, err)


def test_restatement_identity_extents_give_the_source():
    rng = np.random.default_rng(5)
    for s in (1, 2, 37, 224):
        i0, i1, f = taps(s, s)
        assert np.array_equal(i0, np.arange(s)) and np.array_equal(i1, np.minimum(np.arange(s) + 1, s - 1)) and not f.any()
    x = rng.integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)
    assert_bit_exact(preprocess(x, (5, 7)), np.ascontiguousarray(x.transpose(0, 3, 1, 2)).astype(np.float32), 'u8 nhwc')
    xf = rng.standard_normal((2, 3, 5, 7)).astype(np.float32)
    xf.reshape(-1)[:4] = (np.nan, np.inf, -np.inf, -0.0)
    got = preprocess(xf, (5, 7), nhwc=False)
    assert_bit_exact(got, xf, 'fp32 nchw with NaN / inf')
    assert np.isinf(got.reshape(-1)[1]) and np.signbit(got.reshape(-1)[3])


def test_abi_declares_the_preprocessing_entry():
    from pyopenvino_amd import device
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    name = 'pvhip_input_preprocess_f32'
    assert name in device.SIGNATURES and name + '(' in header
    assert len(device.SIGNATURES[name][1]) == 13
    assert re.search(r'#define\s+PVHIP_ABI_VERSION\s+19\b', header)
    assert hasattr(device.load_library(), name)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _f32_values(rng, shape):
    x = (rng.standard_normal(shape) * 100).astype(np.float32)
    special = np.array([np.nan, -0.0, np.inf, -np.inf, 1e-45, -3.0e38], np.float32)
    flat = x.reshape(-1)
    flat[:min(flat.size, special.size)] = special[:flat.size]
    return x


def _device_preprocess(hip, x, dst_hw, nhwc, reverse=False, mean=None, std=None, shift=0):
    """pvhip_input_preprocess_f32 on x (n, h, w, c) or (n, c, h, w); shift > 0 moves the source off 16-byte alignment."""
    n, c = x.shape[0], (x.shape[3] if nhwc else x.shape[1])
    hs, ws = x.shape[1:3] if nhwc else x.shape[2:4]
    raw = np.zeros(x.nbytes + shift, np.uint8)
    raw[shift:] = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    src = hip.DeviceTensor.from_numpy(raw)
    dst = hip.DeviceTensor.empty((n, c) + tuple(dst_hw))
    hip.call('pvhip_memset', ctypes.c_void_p(dst.ptr), 0x7f, dst.nbytes)
    m = hip.DeviceTensor.from_numpy(np.asarray(mean, np.float32)) if mean is not None else None
    s = hip.DeviceTensor.from_numpy(np.asarray(std, np.float32)) if std is not None else None
    hip.call('pvhip_input_preprocess_f32', ctypes.c_void_p(src.ptr + shift), ctypes.c_void_p(dst.ptr), n, c, hs, ws, dst_hw[0], dst_hw[1],
             int(x.dtype == np.uint8), int(nhwc), int(reverse), ctypes.c_void_p(m.ptr) if m is not None else None,
             ctypes.c_void_p(s.ptr) if s is not None else None)
    return np.asarray(dst)


KERNEL_SHAPES = [((480, 640), (224, 224)), ((481, 643), (300, 300)), ((7, 9), (224, 224)), ((28, 28), (57, 31)), ((1, 1), (5, 3)),
                 ((1, 1), (224, 224)), ((37, 41), (13, 1)), ((9, 1), (3, 1)), ((20, 30), (20, 30))]


@pytest.mark.gpu
@pytest.mark.parametrize('src_hw,dst_hw', KERNEL_SHAPES)
@pytest.mark.parametrize('c', [1, 3, 4])
def test_preprocess_kernel_bit_exact(hip, src_hw, dst_hw, c):
    rng = np.random.default_rng(sum(src_hw) * 31 + sum(dst_hw) * 3 + c)
    n = 2
    mean = rng.uniform(0, 255, c).astype(np.float32)
    std = rng.uniform(0.5, 80, c).astype(np.float32)
    x8 = rng.integers(0, 256, (n,) + src_hw + (c,), dtype=np.uint8)
    xf = _f32_values(rng, (n,) + src_hw + (c,))
    for x, shift in ((x8, 3), (xf, 4)):
        kind = 'u8' if x.dtype == np.uint8 else 'fp32'
        for nhwc in (True, False):
            src = x if nhwc else np.ascontiguousarray(x.transpose(0, 3, 1, 2))
            options = [dict(), dict(reverse=True, mean=mean, std=std), dict(reverse=True), dict(mean=mean)]
            if (src_hw, dst_hw) == ((20, 30), (20, 30)):
                options = options[1:]                         # (equal extents and nothing else: the format path, tested below)
            for opt in options:
                want = preprocess(src, dst_hw, nhwc=nhwc, reverse_channels=opt.get('reverse', False), mean=opt.get('mean'), std_scale=opt.get('std'))
                what = '{} {} {} -> {} c={} {}'.format(kind, 'nhwc' if nhwc else 'nchw', src_hw, dst_hw, c, sorted(opt))
                assert_bit_exact(_device_preprocess(hip, src, dst_hw, nhwc, **opt), want, what)
                assert_bit_exact(_device_preprocess(hip, src, dst_hw, nhwc, shift=shift, **opt), want, what + ', unaligned source')


# Shapes whose output rows the kernel splits into column tiles: the sources of one output row pair exceed its 48 KiB LDS budget (fp32
# C = 4, 1700 columns: 2 rows x 1700 x 16 bytes = 54 KB NHWC, the same over four NCHW planes; uint8 C = 4, 7000 columns: 56 KB; no
# resize but 4000 fp32 columns of 4 channels: 64 KB), so tiles start at tx0 > 0 and read their spans from xs0 > 0.
TILED_SHAPES = [((2, 1700), (3, 224), np.float32), ((8, 1700), (5, 226), np.float32), ((3, 7000), (2, 224), np.uint8),
                ((2, 4000), (2, 4000), np.float32)]


@pytest.mark.gpu
@pytest.mark.parametrize('src_hw,dst_hw,dtype', TILED_SHAPES)
def test_preprocess_kernel_bit_exact_in_column_tiles(hip, src_hw, dst_hw, dtype):
    rng = np.random.default_rng(src_hw[1] + dst_hw[1])
    c = 4
    mean = rng.uniform(0, 255, c).astype(np.float32)
    std = rng.uniform(0.5, 80, c).astype(np.float32)
    x = rng.integers(0, 256, (1,) + src_hw + (c,), dtype=np.uint8) if dtype == np.uint8 else _f32_values(rng, (1,) + src_hw + (c,))
    shift = 3 if dtype == np.uint8 else 4
    for nhwc in (True, False):
        src = x if nhwc else np.ascontiguousarray(x.transpose(0, 3, 1, 2))
        options = [dict(reverse=True, mean=mean, std=std)] + ([dict()] if src_hw != dst_hw else [])
        for opt in options:
            want = preprocess(src, dst_hw, nhwc=nhwc, reverse_channels=opt.get('reverse', False), mean=opt.get('mean'), std_scale=opt.get('std'))
            what = '{} {} {} -> {} {}'.format(np.dtype(dtype).name, 'nhwc' if nhwc else 'nchw', src_hw, dst_hw, sorted(opt))
            assert_bit_exact(_device_preprocess(hip, src, dst_hw, nhwc, **opt), want, what)
            assert_bit_exact(_device_preprocess(hip, src, dst_hw, nhwc, shift=shift, **opt), want, what + ', unaligned source')


# Shapes whose tiles are narrower than a quad: fp32, C = 1024, one output row of 8 columns.  The planner halves the tile width to a
# multiple of 4 while it exceeds 4 and then narrows it by one column at a time, until the sources of one output row of the tile fit
# 48 KiB less the 12 (tw + 1) table bytes; a tile of tw columns reads e(tw) = min((tw - 1) S / 8 (rounded up) + 2, S) source columns.
#   NHWC, S = 32: one span of e x 4096 bytes (+ 30, rounded down to 16): e(8) = 30, e(4) = 14 (57 KB), e(3) = 10 (40 KB): tw = 3
#   NHWC, S = 64: e(3) = 18 (74 KB), e(2) = 10 (40 KB): tw = 2
#   NCHW, S = 64: 1024 spans of (4 e + 30) / 16 * 16 bytes: e(4) = 26 (128 KB), e(3) = 18 (96 KB), e(2) = 10 (64 KB), e(1) = 2 (32 KB): tw = 1
# With tw < 4 the stores are scalar, and every tile but the first starts at tx0 > 0.
NARROW_SHAPES = [(True, (1, 32), (1, 8)), (True, (1, 64), (1, 8)), (False, (1, 64), (1, 8))]


@pytest.mark.gpu
@pytest.mark.parametrize('nhwc,src_hw,dst_hw', NARROW_SHAPES)
def test_preprocess_kernel_bit_exact_in_tiles_narrower_than_a_quad(hip, nhwc, src_hw, dst_hw):
    rng = np.random.default_rng(src_hw[1] + nhwc)
    c = 1024
    mean = rng.uniform(0, 255, c).astype(np.float32)
    std = rng.uniform(0.5, 80, c).astype(np.float32)
    x = _f32_values(rng, (1,) + src_hw + (c,))
    src = x if nhwc else np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    want = preprocess(src, dst_hw, nhwc=nhwc, reverse_channels=True, mean=mean, std_scale=std)
    what = 'fp32 {} {} -> {} c={}'.format('nhwc' if nhwc else 'nchw', src_hw, dst_hw, c)
    assert_bit_exact(_device_preprocess(hip, src, dst_hw, nhwc, reverse=True, mean=mean, std=std), want, what)
    assert_bit_exact(_device_preprocess(hip, src, dst_hw, nhwc, reverse=True, mean=mean, std=std, shift=4), want, what + ', unaligned source')


@pytest.mark.gpu
def test_release_device_state_frees_the_input_staging_at_once(hip):
    """The staging of every source extent (page-locked buffer, device tensor) goes back when the request's device state is released, by
    reference counting alone: nothing of it waits for the cyclic garbage collector."""
    import gc
    from pyopenvino_amd import device
    ie, net, name = _net(batch=4)
    info = net.input_info[name]
    info.precision, info.layout = 'U8', 'NHWC'
    info.preprocess_info.resize_algorithm = 'RESIZE_BILINEAR'
    ex = ie.load_network(net)
    rng = np.random.default_rng(3)
    extents = [(40, 50), (28, 28), (64, 64)]
    gc.collect()
    gc.disable()
    try:
        for h, w in extents:
            ex.infer({name: rng.integers(0, 256, (4, h, w, 1), dtype=np.uint8)})
        staged = ex.host_inputs.slots[name].extents
        assert sorted(staged) == sorted(extents)
        host_bytes = sum(s.host.nbytes for s in staged.values())
        device_bytes = sum(s.staging.nbytes for s in staged.values())
        del staged
        blocks0, bytes0 = device.host_stats()
        in_use0 = device.pool_stats()[0]
        ex.release_device_state()
        blocks1, bytes1 = device.host_stats()
        in_use1 = device.pool_stats()[0]
    finally:
        gc.enable()
    assert blocks0 - blocks1 >= len(extents) and bytes0 - bytes1 >= host_bytes, ((blocks0, bytes0), (blocks1, bytes1))
    assert in_use0 - in_use1 >= device_bytes, (in_use0, in_use1, device_bytes)


@pytest.mark.gpu
def test_preprocess_kernel_rejects_what_it_cannot_do(hip):
    lib = hip.load_library()
    src = hip.DeviceTensor.from_numpy(np.zeros(64, np.uint8))
    dst = hip.DeviceTensor.empty((64,))
    for args in ((1, 2000, 4, 4, 2, 2, 1, 1), (1, 3, 70000, 70000, 2, 2, 1, 1), (0, 3, 4, 4, 2, 2, 1, 1), (1, 3, 4, 4, 0, 2, 1, 1),
                 (1, 3, 4, 4, 2, 2, 0, 1)):
        rc = lib.pvhip_input_preprocess_f32(ctypes.c_void_p(src.ptr + (1 if args == (1, 3, 4, 4, 2, 2, 0, 1) else 0)), ctypes.c_void_p(dst.ptr),
                                            *args, 0, 0, None, None)
        assert rc == -2, args                                 # PVHIP_EINVAL, nothing launched


@pytest.mark.gpu
def test_preprocess_kernel_bit_exact_batch256(hip):
    rng = np.random.default_rng(480)
    x = rng.integers(0, 256, (256, 480, 640, 3), dtype=np.uint8)
    got = _device_preprocess(hip, x, (224, 224), True)
    for i in range(0, 256, 32):
        assert_bit_exact(got[i:i + 32], preprocess(x[i:i + 32], (224, 224)), '(256, 480, 640, 3) uint8 -> 224 x 224, images {}..'.format(i))


@pytest.mark.gpu
def test_identity_extents_with_resize_declared_give_the_format_path_bits(hip):
    """RESIZE_BILINEAR declared and a source at the network's own extent: not resized at all -- the bits of the U8 / NHWC path, FP32
    NaN / inf sources included (identity weights would turn an inf neighbour into NaN)."""
    rng = np.random.default_rng(28)
    for precision, x in (('U8', rng.integers(0, 256, (4, 28, 28, 1), dtype=np.uint8)), ('FP32', _f32_values(rng, (4, 28, 28, 1)))):
        fixed, outs = [], []
        for resize in (False, True):
            ie, net, name = _net(batch=4)
            info = net.input_info[name]
            info.precision, info.layout = precision, 'NHWC'
            if resize:
                info.preprocess_info.resize_algorithm = 'RESIZE_BILINEAR'
            ex = ie.load_network(net)
            outs.append(np.array(ex.infer({name: x})[net.outputs[0]['name']], copy=True))
            fixed.append(np.asarray(ex.host_inputs.slots[name].fixed))
        assert_bit_exact(fixed[1], fixed[0], precision + ' input tensor')
        assert_bit_exact(fixed[1], np.ascontiguousarray(x.transpose(0, 3, 1, 2)).astype(np.float32), precision + ' input tensor vs the source')
        assert_bit_exact(outs[1], outs[0], precision + ' Result')
        # the kernel entry itself, with nothing but the format to do, is the format conversion
        src = x
        assert_bit_exact(_device_preprocess(hip, src, (28, 28), True), np.ascontiguousarray(x.transpose(0, 3, 1, 2)).astype(np.float32), precision)


def _googlenet(blob, batch, requests=1, resize=False):
    _ie, net, name = _net('googlenet-v1', batch, blob)
    if resize:
        info = net.input_info[name]
        info.precision, info.layout = 'U8', 'NHWC'
        info.preprocess_info.resize_algorithm = 'RESIZE_BILINEAR'
    return net, _ie.load_network(net, 'GPU', num_requests=requests), name, net.outputs[0]['name']


@pytest.mark.gpu
def test_googlenet_resized_on_the_device_matches_the_host_preprocessed_path(hip):
    from pyopenvino_amd import synth
    blob = synth.synth_weights(os.path.join(MODELS, 'googlenet-v1.xml'), 11)
    rng = np.random.default_rng(8)
    x = rng.integers(0, 256, (8, 256, 320, 3), dtype=np.uint8)
    _, ex_f, name, out_name = _googlenet(blob, 8)
    want = np.array(ex_f.infer({name: preprocess(x, (224, 224))})[out_name], copy=True)
    assert np.isfinite(want).all()
    _, ex, name, _ = _googlenet(blob, 8, resize=True)
    assert_bit_exact(ex.infer({name: x})[out_name], want, 'RESIZE_BILINEAR (8, 256, 320, 3) through infer()')
    req = ex.requests[0]
    buf = req.input_buffer(name, (256, 320))
    assert buf.shape == (8, 256, 320, 3) and buf.dtype == np.uint8
    assert req.input_buffer(name, (256, 320)) is buf
    buf[...] = x
    assert_bit_exact(req.infer({name: buf})[out_name], want, 'RESIZE_BILINEAR from the request buffer')
    x2 = x[:, ::-1].copy()
    want2 = np.array(ex_f.infer({name: preprocess(x2, (224, 224))})[out_name], copy=True)
    buf[...] = x2
    assert_bit_exact(req.infer({name: buf})[out_name], want2, 'new images in the request buffer')


@pytest.mark.gpu
def test_ssd_bgr_frames_reversed_and_resized_on_the_device(hip):
    from pyopenvino_amd import synth
    xml = os.path.join(MODELS, 'ssd_mobilenet_v1_coco.xml')
    blob = synth.synth_weights(xml, 1234)
    rng = np.random.default_rng(300)
    bgr = rng.integers(0, 256, (2, 480, 640, 3), dtype=np.uint8)
    ie, net, name = _net('ssd_mobilenet_v1_coco', 2, blob)
    out_name = net.outputs[0]['name']
    want = np.array(ie.load_network(net).infer({name: preprocess(bgr, (300, 300), reverse_channels=True)})[out_name], copy=True)
    ie, net, name = _net('ssd_mobilenet_v1_coco', 2, blob)
    info = net.input_info[name]
    info.precision, info.layout = 'U8', 'NHWC'
    info.preprocess_info.resize_algorithm = 'RESIZE_BILINEAR'
    info.preprocess_info.reverse_channels = True
    got = ie.load_network(net).infer({name: bgr})[out_name]
    assert_bit_exact(got, want, 'SSD from (2, 480, 640, 3) BGR frames')


@pytest.mark.gpu
def test_mnist_mean_value_and_std_scale_on_the_device(hip):
    rng = np.random.default_rng(784)
    x = rng.integers(0, 256, (4, 1, 28, 28), dtype=np.uint8)
    mean, std = np.float32(33.3), np.float32(78.5)
    ie, net, name = _net(batch=4)
    out_name = net.outputs[0]['name']
    want = np.array(ie.load_network(net).infer({name: preprocess(x, (28, 28), nhwc=False, mean=[mean], std_scale=[std])})[out_name], copy=True)
    ie, net, name = _net(batch=4)
    info = net.input_info[name]
    info.precision = 'U8'
    pre = info.preprocess_info
    pre.init(1)
    pre[0].mean_value, pre[0].std_scale = float(mean), float(std)
    pre.mean_variant = 'MEAN_VALUE'
    ex = ie.load_network(net)
    assert_bit_exact(ex.infer({name: x})[out_name], want, 'mnist U8 with MEAN_VALUE')
    buf = ex.requests[0].input_buffer(name)
    buf[...] = x
    assert_bit_exact(ex.requests[0].infer({name: buf})[out_name], want, 'mnist U8 with MEAN_VALUE from the request buffer')


@pytest.mark.gpu
def test_six_requests_in_flight_two_source_extents(hip):
    """Batch 256, six requests, new source images for every request on every step, the source extent alternating between 256 x 256 and
    480 x 640 per request: every Result equals, bit for bit, the device-resident pass fed the restatement's tensors, and after the
    warm-up passes every request replays its recording whatever the source size."""
    from pyopenvino_amd import device, synth
    blob = synth.synth_weights(os.path.join(MODELS, 'googlenet-v1.xml'), 5)
    B, R = 256, 6
    rng = np.random.default_rng(6)
    sources = [rng.integers(0, 256, (B, 256, 256, 3), dtype=np.uint8), rng.integers(0, 256, (B, 480, 640, 3), dtype=np.uint8),
               rng.integers(0, 256, (B, 256, 256, 3), dtype=np.uint8), rng.integers(0, 256, (B, 480, 640, 3), dtype=np.uint8)]
    _, ex_ref, name, out_name = _googlenet(blob, B)
    want = []
    for src in sources:
        t = device.DeviceTensor.from_numpy(np.concatenate([preprocess(src[i:i + 32], (224, 224)) for i in range(0, B, 32)], 0))
        want.append(np.array(ex_ref.infer({name: t})[out_name], copy=True))
        del t
    assert all(np.isfinite(w_).all() for w_ in want) and not np.array_equal(want[0], want[2])
    ex_ref.release_device_state()
    del ex_ref

    _, ex, _, _ = _googlenet(blob, B, requests=R, resize=True)
    extents = [(256, 256), (480, 640)]
    steps = 6
    for step in range(steps):
        order = [(r * 5 + step) % R for r in range(R)]
        fed = {}
        for r in order:
            k = (r + step) % 4                                # extent (r + step) % 2: alternates per request, and new images every step
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
