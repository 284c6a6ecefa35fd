"""Host inputs in a declared format (IENetwork.input_info: U8 / NHWC), uploaded asynchronously from page-locked per-request buffers
(InferRequest.input_buffer) and converted on the device (pvhip_input_to_nchw_f32).  The first tests need no GPU."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
from helpers import GOLDEN, MODELS, assert_bit_exact, assert_close

HIP = 'pyopenvino_amd.op_plugins'


def _mnist():
    from pyopenvino_amd import IECore
    ie = IECore(plugin_package=HIP)
    return ie, ie.read_network(os.path.join(MODELS, 'mnist.xml'))


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
def test_input_info_defaults_to_fp32_nchw():
    _, net = _mnist()
    name = net.inputs[0]['name']
    assert list(net.input_info) == [name]
    info = net.input_info[name]
    assert (info.precision, info.layout, info.declared) == ('FP32', 'NCHW', False)
    assert info.dims == (1, 1, 28, 28) and info.supported()
    assert info.host_format() == ((1, 1, 28, 28), np.dtype(np.float32))
    info.precision, info.layout = 'u8', 'nhwc'            # accepted in any case, reported upper case
    assert (info.precision, info.layout, info.declared) == ('U8', 'NHWC', True)
    assert info.host_format() == ((1, 28, 28, 1), np.dtype(np.uint8))


def test_input_info_rejects_unknown_values_and_changes_after_load():
    ie, net = _mnist()
    info = net.input_info[net.inputs[0]['name']]
    for what, bad in (('precision', 'FP16'), ('precision', 'I8'), ('layout', 'NC'), ('layout', 'CHW'), ('precision', None)):
        with pytest.raises(ValueError):
            setattr(info, what, bad)
    assert (info.precision, info.layout, info.declared) == ('FP32', 'NCHW', False)
    info.precision = 'U8'
    ie.load_network(net)
    with pytest.raises(ValueError):
        info.precision = 'FP32'
    with pytest.raises(ValueError):
        info.layout = 'NHWC'
    assert (info.precision, info.layout) == ('U8', 'NCHW')


def test_input_info_outside_4d_f32_parameters_is_not_implemented():
    _, net = _mnist()
    name = net.inputs[0]['name']
    nid = next(n for n in net.G.nodes if net.G.nodes[n]['name'] == name)
    net.G.nodes[nid]['data']['element_type'] = 'i64'
    with pytest.raises(NotImplementedError):
        net.input_info[name].precision = 'U8'
    net.G.nodes[nid]['data']['element_type'] = 'f32'
    net.G.nodes[nid]['data']['shape'] = (1, 784)
    with pytest.raises(NotImplementedError):
        net.input_info[name].layout = 'NHWC'


def _shape(layout, n, c, h, w):
    return (n, h, w, c) if layout == 'NHWC' else (n, c, h, w)


@functools.lru_cache(maxsize=None)
def _weights(model):
    """mnist ships its weights; the other IRs get seeded synthetic ones."""
    from pyopenvino_amd import synth
    return None if model == 'mnist' else synth.synth_weights(os.path.join(MODELS, model + '.xml'), 7)


def _declared_net(model, precision, layout, resize):
    from pyopenvino_amd import IECore
    ie = IECore(plugin_package=HIP)
    net = ie.read_network(os.path.join(MODELS, model + '.xml'), weights=_weights(model))
    info = net.input_info[net.inputs[0]['name']]
    info.precision, info.layout = precision, layout
    if resize:
        info.preprocess_info.resize_algorithm = 'RESIZE_BILINEAR'
    return ie, net, info


def _bad_arrays(info, precision, layout, resize, other):
    """[(array of a shape the format refuses, the ValueError text infer() gives for it)]: a wrong batch, a wrong channel count and, with
    no resize declared, a wrong extent.  The texts are written out here (and were compared with what the engine raised through infer()
    before the shape checks moved into InputFormat), not taken from the code under test."""
    n, c, h, w = info.dims
    dtype = np.uint8 if precision == 'U8' else np.float32
    if resize:
        means = 'declared {} / {} with RESIZE_BILINEAR means shape {} for any h, w'.format(precision, layout, _shape(layout, n, c, 'h', 'w'))
        shapes = [_shape(layout, n + 1, c, *other), _shape(layout, n, c + 1, *other), _shape(layout, n, c, *other)[1:]]
        return [(np.empty(s, dtype), 'input {}: {}; got {}'.format(info.name, means, s)) for s in shapes]
    means = 'declared {} / {} means shape {}'.format(precision, layout, _shape(layout, n, c, h, w))
    shapes = [_shape(layout, n + 1, c, h, w), _shape(layout, n, c + 1, h, w), _shape(layout, n, c, *other)]
    return [(np.empty(s, dtype), 'input {}: {}, got {}'.format(info.name, means, s)) for s in shapes]


@pytest.mark.parametrize('resize', [False, True])
@pytest.mark.parametrize('layout', ['NCHW', 'NHWC'])
@pytest.mark.parametrize('precision', ['FP32', 'U8'])
@pytest.mark.parametrize('model,other', [('mnist', (40, 50)), ('googlenet-v1', (256, 320))])
def test_frozen_format_owns_the_shape_rules(model, other, precision, layout, resize):
    """InputFormat (InputInfo.frozen()) against InputInfo.host_format at the network's extent and at one other, and the refusals of
    arrays with a wrong batch, channel count or (no resize declared) extent, by extent_of and by infer() alike."""
    ie, net, info = _declared_net(model, precision, layout, resize)
    fmt = info.frozen()
    n, c, h, w = info.dims
    assert (fmt.name, fmt.dims, fmt.supported, fmt.declared) == (info.name, info.dims, True, True)
    assert (fmt.u8, fmt.nhwc, fmt.resize, fmt.reverse, fmt.mean, fmt.std) == (precision == 'U8', layout == 'NHWC', resize, False, None, None)
    for extent in [(h, w), other] if resize else [(h, w)]:
        shape, dtype = info.host_format(extent)
        assert shape == _shape(layout, n, c, *extent) and dtype == np.dtype(np.uint8 if precision == 'U8' else np.float32)
        assert (fmt.host_shape(extent), fmt.host_dtype) == (shape, dtype)
        assert fmt.checked_extent(extent) == extent
        assert fmt.extent_of(np.empty(shape, dtype)) == extent
        assert fmt.needs_preprocess(extent) == (extent != (h, w))
        assert fmt.needs_convert(extent) == (extent != (h, w) or precision == 'U8' or layout == 'NHWC')
    assert fmt.host_shape() == info.host_format()[0] and fmt.checked_extent() == (h, w)
    if not resize:
        for refused in (info.host_format, fmt.checked_extent):
            with pytest.raises(ValueError, match='no resize is declared'):
                refused(other)
    ex = ie.load_network(net)
    for bad, text in _bad_arrays(info, precision, layout, resize, other):
        with pytest.raises(ValueError) as by_format:
            fmt.extent_of(bad)
        with pytest.raises(ValueError) as by_infer:               # refused before anything reaches the device
            ex.infer({info.name: bad})
        assert str(by_format.value) == str(by_infer.value) == text


def test_abi_declares_the_async_upload_and_the_conversion():
    from pyopenvino_amd import device
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    for name in ('pvhip_memcpy_h2d_async', 'pvhip_input_to_nchw_f32', 'pvhip_host_stats'):
        assert name in device.SIGNATURES and name + '(' in header, name
    lib = device.load_library()
    assert lib.pvhip_abi_version() == 19
    blocks, nbytes = ctypes.c_size_t(7), ctypes.c_size_t(7)
    assert lib.pvhip_host_stats(ctypes.byref(blocks), ctypes.byref(nbytes)) == 0      # no device needed
    assert (blocks.value, nbytes.value) == (0, 0)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _convert(hip, x, u8, nhwc, shift=0):
    """pvhip_input_to_nchw_f32 on x (n, h, w, c) or (n, c, h, w); shift > 0 moves the source off 16-byte alignment."""
    n, c, h, w = (x.shape[0], x.shape[3], x.shape[1], x.shape[2]) if nhwc else x.shape
    raw = np.zeros(x.nbytes + shift, np.uint8)
    raw[shift:] = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    src = hip.DeviceTensor.from_numpy(raw)
    dst = hip.DeviceTensor.empty((n, c, h, w))
    hip.call('pvhip_memset', ctypes.c_void_p(dst.ptr), 0x7f, dst.nbytes)
    hip.call('pvhip_input_to_nchw_f32', ctypes.c_void_p(src.ptr + shift), ctypes.c_void_p(dst.ptr), n, c, h, w, int(u8), int(nhwc))
    return np.asarray(dst)


def _want(x, nhwc):
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2) if nhwc else x).astype(np.float32)


def _f32_values(rng, shape):
    x = rng.standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    special = np.array([np.nan, -0.0, np.inf, -np.inf, 1e-45, -3.0e38], np.float32)
    flat[:min(flat.size, special.size)] = special[:flat.size]
    return x


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('w', [1, 7, 224, 225])
@pytest.mark.parametrize('c', [1, 3, 4])
def test_conversion_kernel_bit_exact(hip, n, w, c):
    rng = np.random.default_rng(1000 * n + 10 * w + c)
    h = 5
    x8 = rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
    x8.reshape(-1)[:2] = (0, 255)
    assert_bit_exact(_convert(hip, x8, True, True), _want(x8, True), 'u8 nhwc')
    assert_bit_exact(_convert(hip, x8, True, True, shift=3), _want(x8, True), 'u8 nhwc, unaligned source')
    y8 = np.ascontiguousarray(x8.transpose(0, 3, 1, 2))
    assert_bit_exact(_convert(hip, y8, True, False), _want(y8, False), 'u8 nchw')
    assert_bit_exact(_convert(hip, y8, True, False, shift=5), _want(y8, False), 'u8 nchw, unaligned source')
    xf = _f32_values(rng, (n, h, w, c))
    assert_bit_exact(_convert(hip, xf, False, True), _want(xf, True), 'fp32 nhwc')
    assert_bit_exact(_convert(hip, xf, False, True, shift=4), _want(xf, True), 'fp32 nhwc, source 4 bytes off')


@pytest.mark.gpu
def test_conversion_kernel_bit_exact_batch256(hip):
    rng = np.random.default_rng(256)
    x8 = rng.integers(0, 256, (256, 224, 224, 3), dtype=np.uint8)
    assert_bit_exact(_convert(hip, x8, True, True), _want(x8, True), 'u8 nhwc (256, 224, 224, 3)')
    xf = _f32_values(rng, (16, 224, 224, 3))
    assert_bit_exact(_convert(hip, xf, False, True), _want(xf, True), 'fp32 nhwc (16, 224, 224, 3)')


@pytest.mark.gpu
def test_async_upload_refuses_pageable_memory(hip):
    n = 1 << 16
    dst = hip.DeviceTensor.from_numpy(np.full(n, 7, np.uint8))
    pageable = np.arange(n, dtype=np.uint32).astype(np.uint8)
    lib = hip.load_library()
    rc = lib.pvhip_memcpy_h2d_async(ctypes.c_void_p(dst.ptr), pageable.ctypes.data_as(ctypes.c_void_p), n)
    assert rc == -2 and b'page-locked' in lib.pvhip_last_error()              # PVHIP_EINVAL
    pinned = hip.host_empty((n,), np.uint8)
    pinned[:] = pageable
    rc = lib.pvhip_memcpy_h2d_async(ctypes.c_void_p(dst.ptr), ctypes.c_void_p(pinned.ctypes.data + 16), n)   # runs past the block
    assert rc == -2
    hip.synchronize()
    assert np.array_equal(np.asarray(dst), np.full(n, 7, np.uint8)), 'a refused copy reached the device'
    hip.call('pvhip_memcpy_h2d_async', ctypes.c_void_p(dst.ptr), ctypes.c_void_p(pinned.ctypes.data), n)
    hip.synchronize()
    assert np.array_equal(np.asarray(dst), pageable)


def _googlenet(ie_blob, batch, requests=1, u8_nhwc=False):
    from pyopenvino_amd import IECore
    ie = IECore(plugin_package=HIP)
    net = ie.read_network(os.path.join(MODELS, 'googlenet-v1.xml'), weights=ie_blob)
    net.set_batch(batch)
    name = net.inputs[0]['name']
    if u8_nhwc:
        net.input_info[name].precision = 'U8'
        net.input_info[name].layout = 'NHWC'
    return net, ie.load_network(net, 'GPU', num_requests=requests), name, net.outputs[0]['name']


def _nhwc_u8(x_nchw):
    assert np.array_equal(x_nchw, np.floor(x_nchw)) and x_nchw.min() >= 0 and x_nchw.max() <= 255
    return np.ascontiguousarray(x_nchw.transpose(0, 2, 3, 1)).astype(np.uint8)


@pytest.mark.gpu
def test_input_buffer_shape_and_dtype(hip):
    from pyopenvino_amd import synth
    blob = synth.synth_weights(os.path.join(MODELS, 'googlenet-v1.xml'), 7)
    _, ex, name, _ = _googlenet(blob, 256, requests=2, u8_nhwc=True)
    bufs = [req.input_buffer(name) for req in ex.requests]
    for b in bufs:
        assert b.shape == (256, 224, 224, 3) and b.dtype == np.uint8 and b.flags['C_CONTIGUOUS'] and b.flags['WRITEABLE']
    assert bufs[0].ctypes.data != bufs[1].ctypes.data
    assert ex.requests[0].input_buffer(name) is bufs[0]          # allocated once per request
    _, ex2, name2, _ = _googlenet(blob, 4)
    b = ex2.requests[0].input_buffer(name2)                      # an undeclared input: the default format
    assert b.shape == (4, 3, 224, 224) and b.dtype == np.float32
    with pytest.raises(KeyError):
        ex2.requests[0].input_buffer('no such input')


@pytest.mark.gpu
def test_googlenet_u8_nhwc_rows_match_the_host_path_and_the_reference(hip):
    """googlenet_rows8.npz's images (integer pixels) as U8 NHWC through the request's buffer, the pageable fallback and the synchronous
    infer(): bit for bit the Result of the same images as FP32 NCHW on the default host path, and the reference's outputs within REL_TOL."""
    from pyopenvino_amd import synth
    z = np.load(os.path.join(GOLDEN, 'googlenet_rows8.npz'))
    blob = synth.synth_weights(os.path.join(MODELS, 'googlenet-v1.xml'), int(z['weight_seed']))
    x = np.concatenate([synth.uniform_pixels(int(s), (1, 3, 224, 224)) for s in z['image_seeds']], 0)
    _, ex_f, name, out_name = _googlenet(blob, len(x))
    want = np.array(ex_f.infer({name: x})[out_name], copy=True)
    _, ex_u, name_u, _ = _googlenet(blob, len(x), u8_nhwc=True)
    req = ex_u.requests[0]
    buf = req.input_buffer(name_u)
    buf[...] = _nhwc_u8(x)
    assert_bit_exact(req.infer({name_u: buf})[out_name], want, 'U8 NHWC from the request buffer')
    assert_bit_exact(req.infer({name_u: _nhwc_u8(x)})[out_name], want, 'U8 NHWC from a pageable array')
    assert_bit_exact(ex_u.infer({name_u: _nhwc_u8(x)})[out_name], want, 'U8 NHWC through Executable_Network.infer')
    assert_close(want, z['out'], helpers.REL_TOL, 'rows 0-7 vs the reference')


@pytest.mark.gpu
def test_six_requests_in_flight_fed_new_host_images_every_step(hip):
    """Batch 256, six requests, every request new host images on every step (U8 NHWC, from the request buffers and from pageable arrays;
    FP32 NCHW from the request buffers of an undeclared network): every Result equals, bit for bit, the device-resident path's Result for
    the same images, and after the warm-up passes every request replays its recording."""
    from pyopenvino_amd import device, synth
    blob = synth.synth_weights(os.path.join(MODELS, 'googlenet-v1.xml'), 3)
    B, R, K = 256, 6, 8
    rng = np.random.default_rng(66)
    images = [rng.integers(0, 256, (B, 224, 224, 3), dtype=np.uint8) for _ in range(K)]
    _, ex_ref, name, out_name = _googlenet(blob, B)
    want = []
    for im in images:
        t = device.DeviceTensor.from_numpy(np.ascontiguousarray(im.transpose(0, 3, 1, 2)).astype(np.float32))
        want.append(np.array(ex_ref.infer({name: t})[out_name], copy=True))
        del t
    assert all(np.isfinite(w_).all() for w_ in want)
    assert not np.array_equal(want[0], want[1])
    del ex_ref

    def rounds(ex, feed, steps, what):
        for step in range(steps):
            order = [(r * 5 + step) % R for r in range(R)]
            for r in order:
                ex.start_async(r, {name: feed(r, images[(r + step) % K], step)})
                if step >= 3:
                    assert ex.requests[r]._replayed is not None, '{}: step {} request {} was not replayed'.format(what, step, r)
            for r in reversed(order):
                got = ex.wait(r)[out_name]
                assert np.array_equal(got, want[(r + step) % K]), '{}: step {} request {}'.format(what, step, r)

    _, ex, _, _ = _googlenet(blob, B, requests=R, u8_nhwc=True)
    bufs = [req.input_buffer(name) for req in ex.requests]

    def from_buffer(r, im, step):
        np.copyto(bufs[r], im)
        return bufs[r]
    rounds(ex, from_buffer, 6, 'U8 NHWC request buffers')
    rounds(ex, lambda r, im, step: im, 6, 'U8 NHWC pageable arrays')
    ex.release_device_state()
    del ex, bufs

    _, ex, _, _ = _googlenet(blob, B, requests=R)
    fbufs = [req.input_buffer(name) for req in ex.requests]

    def from_f32_buffer(r, im, step):
        np.copyto(fbufs[r], im.transpose(0, 3, 1, 2))
        return fbufs[r]
    rounds(ex, from_f32_buffer, 5, 'FP32 NCHW request buffers')


@pytest.mark.gpu
def test_pinned_pool_freed_on_shutdown():
    """In a fresh process: read-backs fill the page-locked pool, a request-style buffer adds a block; after shutdown the library holds no
    page-locked memory, the pool is empty, and an array collected afterwards brings no stale address back into it."""
    code = '''
import gc, sys
sys.path.insert(0, {repo!r})
import numpy as np
from pyopenvino_amd import device
device.init(0)
x = device.DeviceTensor.from_numpy(np.arange(4096, dtype=np.float32))
held = x.numpy()
for _ in range(3):
    a = x.numpy(); b = device.DeviceTensor.from_numpy(np.ones(70000, np.float32)).numpy(); del a, b
gc.collect()
own = device.host_empty((1000,), np.uint8)
blocks, nbytes = device.host_stats()
assert blocks >= 3 and device._pinned_free and device._pinned_total > 0, (blocks, device._pinned_free)
del x
device.shutdown()
assert device.host_stats() == (0, 0), device.host_stats()
assert device._pinned_free == {{}} and device._pinned_total == 0
del held, own
gc.collect()
assert device._pinned_free == {{}} and device._pinned_total == 0, device._pinned_free
device.init(0)
y = device.DeviceTensor.from_numpy(np.arange(10, dtype=np.float32)).numpy()
assert np.array_equal(y, np.arange(10, dtype=np.float32)) and device.host_stats()[0] == 1
device.shutdown()
print('pool OK')
'''.format(repo=helpers.REPO)
    res = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and 'pool OK' in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
