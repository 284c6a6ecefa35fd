"""HIP plugins (through the C ABI) against the reference's recorded outputs and against the oracle on
larger seeded shapes.  GPU only."""
import importlib
import os

import ctypes
import numpy as np
import pytest

import helpers
import ref64
from helpers import assert_bit_exact, assert_close, first_out, load_case

pytestmark = pytest.mark.gpu


def hip_plugin(type_):
    return importlib.import_module('pyopenvino_amd.op_plugins.' + type_)


def oracle_plugin(type_):
    return importlib.import_module('oracle.op_plugins.' + type_)


def check(node, inputs, want, what):
    got = first_out(hip_plugin(node['type']).compute(node, inputs, kernel_type='hip', debug=False))
    want = np.asarray(want)
    if want.dtype.kind == 'i':
        assert got.dtype == want.dtype and np.array_equal(got, want), what
        return 0.0
    if node['type'] == 'DetectionOutput':       # record index and class bit for bit, score / box within the tolerance
        assert got.shape == want.shape and np.array_equal(got[..., :2], want[..., :2]), what + ': record order / classes differ'
    if node['type'] in helpers.BIT_EXACT:
        assert_bit_exact(got, np.asarray(want, dtype=np.float32), what)
        return 0.0
    return assert_close(got, want, helpers.REL_TOL, what)


@pytest.mark.parametrize('path', helpers.op_case_files(), ids=lambda p: os.path.basename(p)[:-4])
def test_hip_op_matches_reference_fixture(hip, path):
    node, inputs, want = load_case(path)
    err = check(node, inputs, want, node['name'])
    # the fp32 kernels are expected far inside the stated 1e-4: flag drift early
    assert err <= 2e-5, '{}: {:.2e}'.format(node['name'], err)


def make_node(type_, ins, data=None):
    node = {'name': type_ + '_seeded', 'type': type_, 'version': 'opset1'}
    if data:
        node['data'] = dict(data)
    node['input'] = {i: {'precision': 'I64' if a.dtype == np.int64 else 'FP32', 'dims': tuple(a.shape)} for i, a in enumerate(ins)}
    node['output'] = {len(ins): {'precision': 'FP32', 'dims': ()}}
    return node


def vs_oracle(type_, ins, data=None, what=''):
    node = make_node(type_, ins, data)
    inputs = {i: a for i, a in enumerate(ins)}
    want = first_out(oracle_plugin(type_).compute(node, inputs, kernel_type='special', debug=False))
    return check(node, inputs, want, what or type_)


def rnd(seed, shape, scale=1.0, shift=0.0):
    from pyopenvino_amd import synth
    return (synth.normal(seed, 99, int(np.prod(shape))) * scale + shift).astype(np.float32).reshape(shape)


def conv_data(strides, pb, pe, auto_pad='explicit'):
    return {'strides': '{}, {}'.format(*strides), 'dilations': '1, 1', 'pads_begin': '{}, {}'.format(*pb),
            'pads_end': '{}, {}'.format(*pe), 'auto_pad': auto_pad}


def pool_data(kernel, strides, pb, pe, rounding, auto_pad='explicit'):
    return {'kernel': '{}, {}'.format(*kernel), 'strides': '{}, {}'.format(*strides), 'pads_begin': '{}, {}'.format(*pb),
            'pads_end': '{}, {}'.format(*pe), 'rounding_type': rounding, 'auto_pad': auto_pad}


# GoogLeNet / mnist / SSD layer shapes at a small batch: every tile configuration of the conv kernel
CONV_SHAPES = [
    # (x shape, w shape, strides, pads_begin, pads_end)
    ((2, 3, 224, 224), (64, 3, 7, 7), (2, 2), (3, 3), (3, 3)),     # conv1/7x7_s2
    ((3, 64, 56, 56), (64, 64, 1, 1), (1, 1), (0, 0), (0, 0)),      # conv2/3x3_reduce
    ((3, 64, 56, 56), (192, 64, 3, 3), (1, 1), (1, 1), (1, 1)),     # conv2/3x3
    ((5, 192, 28, 28), (16, 192, 1, 1), (1, 1), (0, 0), (0, 0)),    # 3a/5x5_reduce (K_out 16)
    ((5, 16, 28, 28), (32, 16, 5, 5), (1, 1), (2, 2), (2, 2)),      # 3a/5x5
    ((4, 480, 14, 14), (96, 480, 1, 1), (1, 1), (0, 0), (0, 0)),    # 4a/3x3_reduce
    ((4, 96, 14, 14), (208, 96, 3, 3), (1, 1), (1, 1), (1, 1)),     # 4a/3x3 (K_out 208)
    ((9, 832, 7, 7), (384, 832, 1, 1), (1, 1), (0, 0), (0, 0)),     # 5b/1x1
    ((9, 192, 7, 7), (384, 192, 3, 3), (1, 1), (1, 1), (1, 1)),     # 5b/3x3
    ((7, 48, 7, 7), (128, 48, 5, 5), (1, 1), (2, 2), (2, 2)),       # 5b/5x5
    ((6, 1, 28, 28), (32, 1, 3, 3), (1, 1), (0, 0), (0, 0)),        # mnist conv 1 (C=1)
    ((6, 64, 5, 5), (64, 64, 3, 3), (1, 1), (0, 0), (0, 0)),        # mnist conv 3
    ((2, 3, 300, 300), (32, 3, 3, 3), (2, 2), (0, 0), (1, 1)),      # SSD Conv2d_0 (asymmetric pad)
    ((1, 24, 14, 14), (24, 24, 1, 1), (1, 1), (0, 0), (0, 0)),      # tiny: fewer pixels than one tile
]


@pytest.mark.parametrize('xs,ws,st,pb,pe', CONV_SHAPES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_conv_model_shapes_vs_oracle(hip, xs, ws, st, pb, pe):
    fan_in = ws[1] * ws[2] * ws[3]
    x = rnd(sum(xs), xs)
    w = rnd(sum(ws) + 1, ws, (2.0 / fan_in) ** 0.5)
    vs_oracle('Convolution', [x, w], conv_data(st, pb, pe), 'conv {} * {}'.format(xs, ws))


def test_conv_7x7_stride2_first_layer(hip):
    """The 7x7 / stride 2 / 3-channel first layer (GoogLeNet conv1) on the general c-major LDS-DMA kernel: ragged extents, K below
    64, asymmetric / no padding, many images.  (Two LDS-patch kernels written for this layer -- a persistent one and one tile per
    workgroup -- measured 0.77 / 0.80 ms against 0.68 ms + 0.07 ms for the Add in front, and lost in the pass: removed.)"""
    cases = [((2, 3, 224, 224), 64, (3, 3), (3, 3)), ((1, 3, 23, 31), 40, (3, 3), (3, 3)), ((3, 3, 40, 17), 7, (0, 0), (0, 0)),
             ((5, 3, 64, 64), 64, (2, 3), (1, 0)), ((1, 3, 7, 7), 3, (0, 0), (0, 0)), ((70, 3, 30, 30), 16, (3, 3), (3, 3))]
    for xs, k, pb, pe in cases:
        x = rnd(sum(xs), xs, 50.0)
        w = rnd(k, (k, 3, 7, 7), (2.0 / 147) ** 0.5)
        err = vs_oracle('Convolution', [x, w], conv_data((2, 2), pb, pe), 'conv1-like {} k{} pads {} {}'.format(xs, k, pb, pe))
        assert err <= 2e-5, 'conv1-like {}: {:.2e}'.format(xs, err)


def test_conv_winograd_f2x2_5x5(hip, monkeypatch):
    """F(2x2, 5x5) on the F(4x4, 3x3) kernel (5x5 / stride 1 / pad 2 layers with even extents; forced here): one, odd and many
    channel stages, ragged channel blocks, fewer patches than a workgroup holds, patch rows that end inside a 32-patch block,
    fused bias + ReLU written in place into a wider tensor; against the oracle and against the direct kernel."""
    from pyopenvino_amd import device as dev
    helpers.setenv(monkeypatch, 'PVHIP_CONV_WINOGRAD5', 'force')
    cases = [((2, 4, 8, 8), 5), ((3, 20, 12, 14), 70), ((1, 16, 28, 28), 32), ((2, 32, 14, 14), 96), ((5, 8, 2, 2), 3), ((1, 12, 4, 22), 33),
             # odd extents: the last patches hang over the edge (7x7 layers)
             ((5, 32, 7, 7), 40), ((2, 8, 5, 9), 7), ((3, 12, 3, 3), 5), ((40, 8, 7, 7), 32), ((1, 4, 1, 1), 2)]
    for xs, k in cases:
        x = rnd(sum(xs), xs)
        w = rnd(k, (k, xs[1], 5, 5), (2.0 / (xs[1] * 25)) ** 0.5)
        err = vs_oracle('Convolution', [x, w], conv_data((1, 1), (2, 2), (2, 2)), 'winograd F(2x2,5x5) {} k{}'.format(xs, k))
        assert err <= 5e-5, 'winograd F(2x2,5x5) {}: {:.2e}'.format(xs, err)
    x, w, b = np.abs(rnd(1, (2, 24, 10, 6))), rnd(2, (40, 24, 5, 5), 0.1), rnd(3, (1, 40, 1, 1), 0.3)
    node = make_node('Convolution', [x, w], conv_data((1, 1), (2, 2), (2, 2)))
    wide = dev.DeviceTensor.from_numpy(np.full((2, 50, 10, 6), -1.0, dtype=np.float32))
    fused = dict(node)
    fused['_fuse_bias'], fused['_fuse_act'], fused['_out_into'] = dev.DeviceTensor.from_numpy(b), ('relu',), (wide, 7)
    hip_plugin('Convolution').compute(fused, {0: x, 1: w})
    got = np.asarray(wide)
    helpers.setenv(monkeypatch, 'PVHIP_CONV_WINOGRAD5', '0')
    direct = np.maximum(first_out(hip_plugin('Convolution').compute(dict(node), {0: x, 1: w})) + b, 0)
    assert_close(got[:, 7:47], direct, 2e-5, 'winograd F(2x2,5x5) fused vs direct')
    assert np.all(got[:, :7] == -1.0) and np.all(got[:, 47:] == -1.0)


@pytest.mark.parametrize('form', ['F(4x4,3x3)', 'F(2x2,3x3)', 'F(2x2,5x5)'])
def test_conv_winograd_stress_elementwise(hip, monkeypatch, form):
    """The Winograd forms on hostile data, element by element against the oracle (|d| <= 1e-4 |want| + 1e-4 rms(want), on top
    of the max-norm): un-centred activations 0 .. 255 (what conv2/3x3 would see without data/mean), weights with 1 % outliers
    x 50, reduction lengths 192 x 9 = 1728 and 64 x 9 = 576 (5x5: 48 x 25, 32 x 25).  The transforms' coefficients (up to 8 and
    1/24 for F(4x4,3x3)) amplify rounding; a numpy fp32 model of the three forms puts F(4x4,3x3) at ~0.25 of this bound,
    F(2x2) at ~0.02."""
    from pyopenvino_amd import synth
    if form == 'F(4x4,3x3)':
        helpers.setenv(monkeypatch, 'PVHIP_CONV_WINOGRAD4', 'force')
        k, pad, shapes = 3, 1, [((2, 192, 28, 28), 96), ((1, 64, 56, 56), 40)]
    elif form == 'F(2x2,3x3)':
        helpers.setenv(monkeypatch, 'PVHIP_CONV_WINOGRAD4', '0')
        k, pad, shapes = 3, 1, [((2, 192, 14, 14), 96), ((3, 64, 7, 7), 40)]
    else:
        helpers.setenv(monkeypatch, 'PVHIP_CONV_WINOGRAD5', 'force')
        k, pad, shapes = 5, 2, [((2, 48, 28, 28), 64), ((2, 32, 14, 14), 40)]
    from pyopenvino_amd.op_plugins import Convolution as conv
    for xs, kout in shapes:
        x = synth.uniform_pixels(sum(xs), xs)                                    # integers 0 .. 255, not centred
        w = rnd(kout, (kout, xs[1], k, k), (2.0 / (xs[1] * k * k)) ** 0.5)
        outl = synth.uniform_pixels(kout + 1, w.shape) < 2.56                    # ~1 % of the weights
        w = np.where(outl, w * 50.0, w).astype(np.float32)
        node = make_node('Convolution', [x, w], conv_data((1, 1), (pad, pad), (pad, pad)))
        assert form.replace(' ', '') in conv.kernel_kind(node)[0].replace(' ', ''), conv.kernel_kind(node)
        got = first_out(hip_plugin('Convolution').compute(dict(node), {0: x, 1: w}))
        want = first_out(oracle_plugin('Convolution').compute(dict(node), {0: x, 1: w}, kernel_type='special'))
        excess = helpers.elementwise_excess(got, want)
        err = assert_close(got, want, helpers.REL_TOL, '{} stress {}'.format(form, xs))
        print('{} {} k{}: max-norm {:.2e}, element-wise excess {:.3f}'.format(form, xs, kout, err, excess))
        assert excess <= 0.5, '{} {}: only {:.2f} x inside the element-wise bound'.format(form, xs, 1.0 / max(excess, 1e-9))


def check_alone_vs_float64(alone, x, wt, b, pd, what):
    """A batch-256 layer's output (bias + ReLU fused) against the float64 reference on the 32 sampled images (tests/ref64.py)."""
    import ref64
    idx = ref64.SAMPLE_256
    want = ref64.relu(ref64.convolution(np.asarray(x)[idx], np.asarray(wt), (1, 1), pd, pd) + np.asarray(b).astype(np.float64))
    assert_close(alone[idx], want, helpers.REL_TOL, what + ' vs float64')


def test_convolution_kernels_side_by_side_on_several_streams_at_batch_256(hip):
    """Batch 256 makes a persistent workgroup of the six-point Winograd kernel walk several tiles (the small cases above stop at
    one), and four streams make the loads slow: a register copied while a load was still on its way into it gave wrong results
    ONLY in this setting.  Every layer, launched next to the others three times over, must give the bits it gives alone."""
    from pyopenvino_amd import device as dev, synth
    from pyopenvino_amd.op_plugins import Convolution as conv
    layers = [((256, 16, 28, 28), 64, 3), ((256, 32, 28, 28), 96, 5), ((256, 16, 14, 14), 48, 5), ((256, 64, 28, 28), 96, 1)]
    jobs = []
    for i, (xs, k, ks) in enumerate(layers):
        n, c, h, w = xs
        x = dev.DeviceTensor.from_numpy(synth.normal(1 + i, 2, n * c * h * w).astype(np.float32).reshape(xs))
        wt = dev.DeviceTensor.from_numpy((synth.normal(3 + i, 4, k * c * ks * ks) * (2.0 / (c * ks * ks)) ** 0.5).astype(np.float32).reshape((k, c, ks, ks)))
        b = dev.DeviceTensor.from_numpy(synth.normal(5 + i, 6, k).astype(np.float32).reshape((1, k, 1, 1)))
        pd = (ks // 2, ks // 2)
        run = (lambda node={}, x=x, wt=wt, b=b, pd=pd: conv.launch(node, x, wt, (1, 1), pd, pd, 'explicit', bias=b, act=('relu',)))
        dev.select_stream(0)
        alone = np.asarray(run())
        check_alone_vs_float64(alone, x, wt, b, pd, 'conv {}x{} {} alone'.format(ks, ks, xs))
        jobs.append((xs, ks, run, alone))
    try:
        for rnd_ in range(2):
            outs = []
            for rep in range(3):
                for i, (xs, ks, run, alone) in enumerate(jobs):
                    dev.select_stream(i)
                    outs.append((xs, ks, alone, run()))
            for i in range(len(jobs)):
                dev.select_stream(i)
                dev.synchronize()
            dev.select_stream(0)
            for xs, ks, alone, y in outs:
                assert_bit_exact(np.asarray(y), alone, 'conv {}x{} {} next to the others'.format(ks, ks, xs))
    finally:
        dev.select_stream(0)


@pytest.mark.parametrize('tn', ['1', '2', '4'])
def test_pointwise_kernel_forms_side_by_side_on_several_streams_at_batch_256(hip, monkeypatch, tn):
    """Every instantiation of conv_pw_kernel -- 1 / 2 / 4 channel tiles per workgroup (PVHIP_PW_TN), 16-byte and dword activation
    copies (28x28 and 7x7 images) -- next to each other and to a Winograd layer on four streams, three times over: the bits each
    gives alone.  (Its weight loads were asm statements with a hand-counted wait in rounds 1-2; a register copied while a load was
    still on its way into it would show here, as it did for the Winograd kernel.)"""
    from pyopenvino_amd import device as dev, synth
    from pyopenvino_amd.op_plugins import Convolution as conv
    helpers.setenv(monkeypatch, 'PVHIP_PW_TN', tn)
    layers = [((256, 64, 28, 28), 96, 1), ((256, 192, 7, 7), 128, 1), ((256, 16, 28, 28), 64, 3), ((256, 48, 14, 14), 160, 1)]
    jobs = []
    for i, (xs, k, ks) in enumerate(layers):
        n, c, h, w = xs
        x = dev.DeviceTensor.from_numpy(synth.normal(11 + i, 2, n * c * h * w).astype(np.float32).reshape(xs))
        wt = dev.DeviceTensor.from_numpy((synth.normal(13 + i, 4, k * c * ks * ks) * (2.0 / (c * ks * ks)) ** 0.5).astype(np.float32).reshape((k, c, ks, ks)))
        b = dev.DeviceTensor.from_numpy(synth.normal(15 + i, 6, k).astype(np.float32).reshape((1, k, 1, 1)))
        pd = (ks // 2, ks // 2)
        run = (lambda node={}, x=x, wt=wt, b=b, pd=pd: conv.launch(node, x, wt, (1, 1), pd, pd, 'explicit', bias=b, act=('relu',)))
        dev.select_stream(0)
        alone = np.asarray(run())
        if ks == 1 and i == 0:      # the form asked for is the form that ran, and it is right
            want = np.maximum(np.einsum('kc,nchw->nkhw', np.asarray(wt)[:, :, 0, 0].astype(np.float64), np.asarray(x)[:2].astype(np.float64))
                              + np.asarray(b).astype(np.float64), 0)
            assert_close(alone[:2], want.astype(np.float32), helpers.REL_TOL, 'pointwise TN={}'.format(tn))
        check_alone_vs_float64(alone, x, wt, b, pd, 'conv {}x{} {} alone (PVHIP_PW_TN={})'.format(ks, ks, xs, tn))
        jobs.append((xs, ks, run, alone))
    try:
        for rnd_ in range(2):
            outs = []
            for rep in range(3):
                for i, (xs, ks, run, alone) in enumerate(jobs):
                    dev.select_stream(i)
                    outs.append((xs, ks, alone, run()))
            for i in range(len(jobs)):
                dev.select_stream(i)
                dev.synchronize()
            dev.select_stream(0)
            for xs, ks, alone, y in outs:
                assert_bit_exact(np.asarray(y), alone, 'conv {}x{} {} (PVHIP_PW_TN={}) next to the others'.format(ks, ks, xs, tn))
    finally:
        dev.select_stream(0)


def test_conv_winograd_f4x4_3x3(hip, monkeypatch):
    """F(4x4, 3x3) (the layers with extents divisible by 4 and enough patches; forced here): one, odd and many channel
    stages, ragged channel blocks, fewer patches than a workgroup holds, several images, fused bias + ReLU written in place
    into a wider tensor; against the oracle and against the direct kernel."""
    from pyopenvino_amd import device as dev
    helpers.setenv(monkeypatch, 'PVHIP_CONV_WINOGRAD4', 'force')
    cases = [((2, 4, 8, 8), 5), ((3, 20, 12, 16), 70), ((1, 64, 56, 56), 32), ((2, 96, 28, 28), 128), ((5, 8, 4, 4), 3), ((1, 12, 4, 20), 33),
             # extents that are not multiples of 4: the last patches hang over the edge (GoogLeNet's 14x14 and 7x7 layers at batch 256)
             ((3, 16, 14, 14), 40), ((5, 24, 7, 7), 33), ((2, 8, 5, 9), 7), ((1, 12, 6, 10), 3), ((2, 4, 3, 3), 5), ((40, 8, 7, 7), 32)]
    for xs, k in cases:
        x = rnd(sum(xs), xs)
        w = rnd(k, (k, xs[1], 3, 3), (2.0 / (xs[1] * 9)) ** 0.5)
        err = vs_oracle('Convolution', [x, w], conv_data((1, 1), (1, 1), (1, 1)), 'winograd F(4x4) {} k{}'.format(xs, k))
        assert err <= 5e-5, 'winograd F(4x4) {}: {:.2e}'.format(xs, err)
    x, w, b = np.abs(rnd(1, (2, 32, 12, 8))), rnd(2, (40, 32, 3, 3), 0.1), rnd(3, (1, 40, 1, 1), 0.3)
    node = make_node('Convolution', [x, w], conv_data((1, 1), (1, 1), (1, 1)))
    wide = dev.DeviceTensor.from_numpy(np.full((2, 50, 12, 8), -1.0, dtype=np.float32))
    fused = dict(node)
    fused['_fuse_bias'], fused['_fuse_act'], fused['_out_into'] = dev.DeviceTensor.from_numpy(b), ('relu',), (wide, 7)
    hip_plugin('Convolution').compute(fused, {0: x, 1: w})
    got = np.asarray(wide)
    helpers.setenv(monkeypatch, 'PVHIP_CONV_WINOGRAD', '0')
    direct = np.maximum(first_out(hip_plugin('Convolution').compute(dict(node), {0: x, 1: w})) + b, 0)
    assert_close(got[:, 7:47], direct, 2e-5, 'winograd F(4x4) fused vs direct')
    assert np.all(got[:, :7] == -1.0) and np.all(got[:, 47:] == -1.0)


@pytest.mark.parametrize('ks', [3, 5])
def test_conv_winograd_shared_v_form_has_the_bits_of_the_two_workgroup_form(hip, monkeypatch, ks):
    """conv_wino4s_kernel (round 4: two channel blocks on ONE transformed image per stage, 16 waves, LDS counters instead of barriers)
    against conv_wino4_kernel: the same arithmetic in the same order, so the same bits -- whole and ragged extents, several tiles per
    workgroup, patch blocks that end inside an image, partial last channel block, an odd number of channel blocks, fused bias + ReLU / Clamp into a wider tensor;
    and against the oracle.  Shapes the shared form does not take (a single channel block, a stage count that is not a multiple of
    four) fall back to the two-workgroup form by themselves."""
    from pyopenvino_amd import device as dev
    helpers.setenv(monkeypatch, 'PVHIP_CONV_WINOGRAD4', 'force')
    helpers.setenv(monkeypatch, 'PVHIP_CONV_WINOGRAD5', 'force')
    pad = ks // 2
    cases = [((2, 16, 8, 8), 64), ((3, 32, 12, 16), 40), ((1, 64, 56, 56), 128), ((9, 16, 28, 28), 192), ((5, 48, 14, 14), 100),
             ((40, 16, 7, 7), 64), ((3, 80, 5, 9), 33), ((600, 16, 4, 4), 64), ((2, 16, 8, 8), 32), ((2, 24, 8, 8), 64),
             ((5, 32, 14, 14), 96), ((700, 16, 4, 4), 160), ((3, 16, 12, 12), 208)]       # odd numbers of channel blocks: the last pair is one block
    for xs, k in cases:
        x = rnd(sum(xs), xs)
        w = rnd(k, (k, xs[1], ks, ks), (2.0 / (xs[1] * ks * ks)) ** 0.5)
        b = rnd(k + 1, (1, k, 1, 1), 0.3)
        node = make_node('Convolution', [x, w], conv_data((1, 1), (pad, pad), (pad, pad)))
        outs = {}
        for mode in ('0', '2'):
            helpers.setenv(monkeypatch, 'PVHIP_WINO_SHARED', mode)
            for act in (None, ('relu',), ('clamp', 0.0, 0.5)):
                wide = dev.DeviceTensor.from_numpy(np.full((xs[0], k + 9, xs[2], xs[3]), -1.0, dtype=np.float32))
                fused = dict(node)
                fused['_fuse_bias'], fused['_out_into'] = dev.DeviceTensor.from_numpy(b), (wide, 4)
                if act is not None:
                    fused['_fuse_act'] = act
                hip_plugin('Convolution').compute(fused, {0: x, 1: w})
                outs[(mode, act)] = np.asarray(wide)
        for act in (None, ('relu',), ('clamp', 0.0, 0.5)):
            helpers.assert_bit_exact(outs[('2', act)], outs[('0', act)], 'shared V vs two workgroups {} k{} {}'.format(xs, k, act))
            assert np.all(outs[('2', act)][:, :4] == -1.0) and np.all(outs[('2', act)][:, k + 4:] == -1.0)
        want = first_out(oracle_plugin('Convolution').compute(dict(node), {0: x, 1: w}, kernel_type='special')) + b
        assert_close(outs[('2', None)][:, 4:k + 4], want, 5e-5, 'shared V vs oracle {} k{}'.format(xs, k))


@pytest.mark.parametrize('kb,waves', [(None, None), ('32', 'small'), ('32', '8'), ('64', '8'), ('32', '4'), ('64', '4')])
def test_conv_winograd_3x3(hip, monkeypatch, kb, waves):
    """3x3 / stride 1 / pad 1 layers run Winograd F(2x2, 3x3) (the default): odd extents (half-empty last patches),
    one and many channel stages, ragged channel blocks, fewer patches than a workgroup holds, fused bias + activation;
    every workgroup shape (32 / 64 output channels, 8 / 4 waves, the 32 x 32 four-wave form), the library's own choice first."""
    if kb is not None:
        helpers.setenv(monkeypatch, 'PVHIP_WINO_KB', kb)
        helpers.setenv(monkeypatch, 'PVHIP_WINO_SMALL', '1' if waves == 'small' else '0')
        if waves != 'small':
            helpers.setenv(monkeypatch, 'PVHIP_WINO_WAVES', waves)
    cases = [((2, 4, 7, 7), 5), ((3, 20, 13, 11), 70), ((1, 64, 14, 14), 32), ((2, 96, 28, 28), 128), ((5, 8, 1, 1), 3),
             ((1, 12, 2, 9), 33)]
    for xs, k in cases:
        x = rnd(sum(xs), xs)
        w = rnd(k, (k, xs[1], 3, 3), (2.0 / (xs[1] * 9)) ** 0.5)
        err = vs_oracle('Convolution', [x, w], conv_data((1, 1), (1, 1), (1, 1)), 'winograd {} k{}'.format(xs, k))
        assert err <= 2e-5, 'winograd {}: {:.2e}'.format(xs, err)
    # same weights through the direct kernel: the two algorithms agree far inside the tolerance of the path
    x, w = rnd(1, (2, 32, 9, 9)), rnd(2, (40, 32, 3, 3), 0.1)
    node = make_node('Convolution', [x, w], conv_data((1, 1), (1, 1), (1, 1)))
    wino = first_out(hip_plugin('Convolution').compute(dict(node), {0: x, 1: w}))
    helpers.setenv(monkeypatch, 'PVHIP_CONV_WINOGRAD', '0')
    direct = first_out(hip_plugin('Convolution').compute(dict(node), {0: x, 1: w}))
    assert_close(wino, direct, 5e-6, 'winograd vs direct')
    assert not np.array_equal(wino, direct)          # (they are different summations)


def test_conv_seeded_random_shapes(hip):
    """80 seeded random convolutions (kernel 1..5, stride 1..2, pads 0..2 on either side, ragged channel counts,
    batch 1..5) against the oracle: every kernel family is hit (Winograd, pointwise copy, (r,s)-major and c-major
    LDS-DMA) with shapes nobody picked by hand."""
    rng = np.random.RandomState(20240611)
    families = set()
    for case in range(80):
        kh, kw = (int(rng.randint(1, 6)),) * 2 if rng.rand() < 0.7 else (int(rng.randint(1, 6)), int(rng.randint(1, 6)))
        sh = sw = int(rng.randint(1, 3))
        pb = (int(rng.randint(0, 3)), int(rng.randint(0, 3)))
        pe = (int(rng.randint(0, 3)), int(rng.randint(0, 3)))
        if rng.rand() < 0.35:
            kh = kw = 3; sh = sw = 1; pb = pe = (1, 1)                       # Winograd-eligible
        c = int(rng.choice([1, 3, 4, 7, 8, 16, 20, 32, 48]))
        k = int(rng.choice([1, 5, 16, 31, 32, 33, 64, 70, 100]))
        h, w = int(rng.randint(max(kh - pb[0] - pe[0], 1), 19)), int(rng.randint(max(kw - pb[1] - pe[1], 1), 19))
        if rng.rand() < 0.15:
            kh = kw = sh = sw = 1; pb = pe = (0, 0); c = int(rng.choice([16, 32, 48])); w = 4 * int(rng.randint(1, 5))   # pointwise copy
        if h + pb[0] + pe[0] < kh or w + pb[1] + pe[1] < kw:
            continue
        n = int(rng.randint(1, 6))
        if (h + pb[0] + pe[0] - kh) % sh or (w + pb[1] + pe[1] - kw) % sw:
            continue                                                          # the reference's im2col raises on these
        x = rnd(1000 + case, (n, c, h, w))
        wt = rnd(2000 + case, (k, c, kh, kw), (2.0 / (c * kh * kw)) ** 0.5)
        vs_oracle('Convolution', [x, wt], conv_data((sh, sw), pb, pe), 'random case {}: x{} w{} s{} pb{} pe{}'.format(
            case, x.shape, wt.shape, (sh, sw), pb, pe))
        families.add('wino' if (kh, kw, sh, sw, pb, pe) == (3, 3, 1, 1, (1, 1), (1, 1)) and c % 4 == 0 else
                     'pw' if (kh, kw, sh, sw, pb, pe) == (1, 1, 1, 1, (0, 0), (0, 0)) and c % 16 == 0 and (h * w) % 4 == 0 else
                     'rs' if c % 16 == 0 else 'c')
    assert families == {'wino', 'pw', 'rs', 'c'}, families


def test_pad2d_matches_numpy_bit_exact(hip):
    """pvhip_pad2d_f32 (the zero-padded image of Convolution.py:64-66 as a tensor, optionally with the per-channel Add in front of the
    layer folded in) against np.pad of x (+ c): asymmetric pads, ragged widths, one plane, no padding at all."""
    import ctypes
    cases = [((2, 3, 9, 11), (3, 3, 3, 3)), ((1, 1, 1, 1), (0, 2, 1, 0)), ((3, 5, 7, 4), (0, 0, 0, 0)), ((2, 3, 224, 224), (3, 3, 3, 3)),
             ((1, 4, 6, 5), (1, 0, 0, 2))]
    for xs, (pt, pl, pb, pr) in cases:
        x = rnd(sum(xs), xs, 30.0)
        add = rnd(7, (1, xs[1], 1, 1), 100.0)
        xd = hip.DeviceTensor.from_numpy(x)
        for with_add in (False, True):
            y = hip.DeviceTensor.empty((xs[0], xs[1], xs[2] + pt + pb, xs[3] + pl + pr))
            ad = hip.DeviceTensor.from_numpy(add) if with_add else None
            hip.call('pvhip_pad2d_f32', ctypes.c_void_p(xd.ptr), ctypes.c_void_p(y.ptr), xs[0], xs[1], xs[2], xs[3], pt, pl, pb, pr,
                     ctypes.c_void_p(ad.ptr if ad is not None else 0))
            want = np.pad((x + add) if with_add else x, ((0, 0), (0, 0), (pt, pb), (pl, pr)))
            assert_bit_exact(np.asarray(y), want.astype(np.float32), 'pad2d {} pads {} add={}'.format(xs, (pt, pl, pb, pr), with_add))


def test_conv_prepadded_input_is_bit_identical(hip, monkeypatch):
    """A padded layer on the c-major kernel (C % 16 != 0) runs as a padding pass + the test-free gather; PVHIP_CONV_PREPAD=0 keeps the
    window test in the gather.  Same taps, same order: the same bits -- also with the per-channel Add in front folded into the pass
    (node['_pre_add']), against Add then Convolution as two launches."""
    cases = [((2, 3, 33, 29), (20, 3, 7, 7), (2, 2), (3, 3), (3, 3)), ((3, 5, 9, 9), (70, 5, 3, 3), (1, 1), (1, 1), (1, 1)),
             ((2, 3, 30, 30), (32, 3, 3, 3), (2, 2), (0, 0), (1, 1)), ((1, 1, 12, 12), (8, 1, 5, 5), (1, 1), (2, 2), (2, 2)),
             ((70, 3, 30, 30), (16, 3, 7, 7), (2, 2), (3, 3), (3, 3))]
    from pyopenvino_amd.op_plugins import Convolution
    for xs, ws, st, pb, pe in cases:
        x, w = rnd(sum(xs), xs, 20.0), rnd(sum(ws), ws, (2.0 / (ws[1] * ws[2] * ws[3])) ** 0.5)
        c_add = rnd(11, (1, xs[1], 1, 1), 50.0)
        bias = hip.DeviceTensor.from_numpy(rnd(5, (1, ws[0], 1, 1)))
        outs = {}
        for mode in ('0', '1'):
            helpers.setenv(monkeypatch, 'PVHIP_CONV_PREPAD', mode)
            hip.reload_settings()
            node = make_node('Convolution', [x, w], conv_data(st, pb, pe))
            node['_fuse_bias'], node['_fuse_act'] = bias, ('relu',)
            outs[mode] = np.asarray(first_out(hip_plugin('Convolution').compute(node, {0: x, 1: w})))
            if mode == '1':
                oh, ow = outs[mode].shape[2:]
                assert Convolution.prepad_wanted(xs[0], xs[1], xs[2], xs[3], ws[0], ws[2], ws[3], oh, ow, st, pb, pe), (xs, ws)
                summed = first_out(hip_plugin('Add').compute(make_node('Add', [x, c_add]), {0: x, 1: c_add}))
                two = np.asarray(first_out(hip_plugin('Convolution').compute(dict(node), {0: summed, 1: w})))
                folded = dict(node)
                folded['_pre_add'] = hip.DeviceTensor.from_numpy(c_add)
                one = np.asarray(first_out(hip_plugin('Convolution').compute(folded, {0: x, 1: w})))
                assert_bit_exact(one, two, 'Add folded into the padding pass {} * {}'.format(xs, ws))
        assert_bit_exact(outs['1'], outs['0'], 'padding pass + test-free gather vs window test {} * {}'.format(xs, ws))
    monkeypatch.delenv('PVHIP_CONV_PREPAD', raising=False)
    hip.reload_settings()


def test_conv_stem_as_winograd_on_the_space_to_depth_image(hip, monkeypatch):
    """PVHIP_CONV_STEM_WINO=1 (opt-in, round 5): a 7x7 / 2 / pad 3 first convolution over three channels as Winograd F(3x3,4x4) over the twelve
    phase channels x'(c; py, px; i, j) = xpad(c, 2 i + py, 2 j + px) (pvhip_conv2d_stem_wino_f32: 0.34 of the multiplies).  Another order of
    summation, so not the bits of the general kernel: against the oracle within the path's 1e-4 in the max norm AND element by element at
    half the |d| <= 1e-4 |want| + 1e-4 rms(want) bound, as for the other Winograd forms -- whole images, bands of one tile row, partial tile
    columns and rows (112 = 37 x 3 + 1), every epilogue, the Add in front of the layer (applied to the image, not to its padding),
    un-centred pixels with outlier weights.  Without the knob, and for geometries the kernel does not take, the row-span kernel stays."""
    from pyopenvino_amd import synth
    from pyopenvino_amd.op_plugins import Convolution
    st, pb, pe = (2, 2), (3, 3), (3, 3)
    node0 = make_node('Convolution', [np.zeros((2, 3, 224, 224), np.float32), np.zeros((64, 3, 7, 7), np.float32)], conv_data(st, pb, pe))
    assert Convolution.kernel_kind(node0)[0] == 'row spans (stem)'                    # the default
    helpers.setenv(monkeypatch, 'PVHIP_CONV_STEM_WINO', '1')
    family, frac = Convolution.kernel_kind(node0)
    assert family.startswith('Winograd F(3x3,4x4)') and abs(frac - 38 * 38 * 36 * 12 / (112.0 * 112 * 147)) < 1e-9, (family, frac)
    cases = [((2, 3, 224, 224), 64, ('relu',), False), ((3, 3, 56, 56), 64, None, False), ((1, 3, 36, 24), 48, ('relu',), False),
             ((5, 3, 30, 32), 16, ('clamp', -40.0, 75.0), False), ((9, 3, 14, 8), 32, ('relu',), False), ((2, 3, 100, 224), 64, None, True)]
    for i, (xs, k, act, hostile) in enumerate(cases):
        ws = (k, 3, 7, 7)
        if hostile:
            x = synth.uniform_pixels(70 + i, xs)                                      # integers 0 .. 255, not centred
            w = rnd(50 + i, ws, (2.0 / 147.0) ** 0.5)
            w = np.where(synth.uniform_pixels(90 + i, ws) < 2.56, w * 50.0, w).astype(np.float32)      # ~1 % of the weights x 50
        else:
            x, w = rnd(40 + i, xs, 60.0), rnd(50 + i, ws, (2.0 / 147.0) ** 0.5)
        c_add = rnd(11, (1, 3, 1, 1), 50.0)
        bias = hip.DeviceTensor.from_numpy(rnd(5, (1, k, 1, 1))) if i != 1 else None
        node = make_node('Convolution', [x, w], conv_data(st, pb, pe))
        node['_fuse_bias'], node['_fuse_act'] = bias, act
        assert Convolution.kernel_kind(node)[0].startswith('Winograd F(3x3,4x4)'), (xs, k)
        for add in (None, c_add):
            n2 = dict(node)
            if add is not None:
                n2['_pre_add'] = hip.DeviceTensor.from_numpy(add)
            got = np.asarray(first_out(hip_plugin('Convolution').compute(n2, {0: x, 1: w})))
            plain = make_node('Convolution', [x, w], conv_data(st, pb, pe))
            xin = x if add is None else (x + add).astype(np.float32)
            want = np.asarray(first_out(oracle_plugin('Convolution').compute(plain, {0: xin, 1: w}, kernel_type='special')))
            if bias is not None:
                want = want + np.asarray(bias).reshape(1, k, 1, 1)
            if act is not None:
                want = np.where(want < 0, 0, want) if act[0] == 'relu' else np.clip(want, act[1], act[2])
            want = want.astype(np.float32)
            what = 'conv1 as F(3x3,4x4) {} k={} {} add={}'.format(xs, k, act, add is not None)
            assert_close(got, want, helpers.REL_TOL, what)
            excess = helpers.elementwise_excess(got, want)
            assert excess <= 0.5, '{}: only {:.2f} x inside the element-wise bound'.format(what, 1.0 / max(excess, 1e-9))
    # geometries the Winograd form does not take stay on the row-span kernel (or wherever they were)
    for xs, ws in (((2, 3, 30, 32), (40, 3, 7, 7)), ((2, 3, 31, 32), (16, 3, 7, 7)), ((2, 3, 32, 228), (16, 3, 7, 7))):
        node = make_node('Convolution', [np.zeros(xs, np.float32), np.zeros(ws, np.float32)], conv_data(st, pb, pe))
        assert not Convolution.kernel_kind(node)[0].startswith('Winograd F(3x3,4x4)'), (xs, ws)


def test_conv_stem_row_span_kernel_has_the_bits_of_the_general_kernel(hip, monkeypatch):
    """A 7x7 / 2 / pad 3 first convolution over three channels (GoogLeNet's conv1) runs from row spans of the padded image with its weights
    resident in registers (pvhip_conv2d_stem_f32 on a padded copy; pvhip_conv2d_stem_direct_f32 straight from the image: no padding pass, the
    Add in front of the layer applied in LDS; round 5); PVHIP_CONV_STEM=0 keeps it on the general LDS-DMA kernel.  All reduce over
    the taps in the reference's (c, r, s) order on the fp32 matrix cores: the same bits -- whole and ragged tiles (output rows not a
    multiple of four per image), fewer than 64 / 32 / 16 output channels, short rows, every epilogue, the Add in front folded into the
    padding pass -- and the oracle's result within the path's 1e-4."""
    from pyopenvino_amd.op_plugins import Convolution
    cases = [((2, 3, 224, 224), 64, ('relu',)), ((3, 3, 56, 56), 64, None), ((1, 3, 36, 24), 40, ('relu',)), ((5, 3, 30, 32), 7, ('clamp', -0.5, 0.75)),
             ((9, 3, 14, 8), 17, ('relu',)), ((2, 3, 100, 224), 33, None)]
    st, pb, pe = (2, 2), (3, 3), (3, 3)
    for i, (xs, k, act) in enumerate(cases):
        ws = (k, 3, 7, 7)
        x, w = rnd(40 + i, xs, 60.0), rnd(50 + i, ws, (2.0 / 147.0) ** 0.5)
        c_add = rnd(11, (1, 3, 1, 1), 50.0)
        bias = hip.DeviceTensor.from_numpy(rnd(5, (1, k, 1, 1))) if i != 1 else None
        outs = {}
        for mode, direct in (('0', '1'), ('1', '0'), ('1', '1')):       # general kernel; row spans of a padded copy; row spans of the image itself
            helpers.setenv(monkeypatch, 'PVHIP_CONV_STEM', mode)
            helpers.setenv(monkeypatch, 'PVHIP_CONV_STEM_DIRECT', direct)
            tag = mode + direct
            node = make_node('Convolution', [x, w], conv_data(st, pb, pe))
            node['_fuse_bias'], node['_fuse_act'] = bias, act
            assert (Convolution.kernel_kind(node)[0] == 'row spans (stem)') == (mode == '1'), (xs, k, Convolution.kernel_kind(node))
            outs[tag] = np.asarray(first_out(hip_plugin('Convolution').compute(node, {0: x, 1: w})))
            folded = dict(node)
            folded['_pre_add'] = hip.DeviceTensor.from_numpy(c_add)
            outs[tag + 'add'] = np.asarray(first_out(hip_plugin('Convolution').compute(folded, {0: x, 1: w})))
        for tag, what in (('10', 'row-span kernel (padded copy)'), ('11', 'row-span kernel (the image itself)')):
            assert_bit_exact(outs[tag], outs['01'], '{} vs general kernel {} k={} {}'.format(what, xs, k, act))
            assert_bit_exact(outs[tag + 'add'], outs['01add'], '{} vs general kernel, the Add in front folded in {} k={}'.format(what, xs, k))
        outs['1'] = outs['11']
        plain = make_node('Convolution', [x, w], conv_data(st, pb, pe))
        want = np.asarray(first_out(oracle_plugin('Convolution').compute(plain, {0: x, 1: w})))
        if bias is not None:
            want = want + np.asarray(bias).reshape(1, k, 1, 1)
        if act is not None:
            want = np.where(want < 0, 0, want) if act[0] == 'relu' else np.clip(want, act[1], act[2])
        assert_close(outs['1'], want.astype(np.float32), helpers.REL_TOL, 'row-span kernel vs oracle {} k={}'.format(xs, k))
    helpers.setenv(monkeypatch, 'PVHIP_CONV_STEM', None)
    helpers.setenv(monkeypatch, 'PVHIP_CONV_STEM_DIRECT', None)
    # geometries the kernel does not take stay where they were
    for xs, ws, st_, pb_ in (((2, 3, 33, 29), (20, 3, 7, 7), (2, 2), (3, 3)), ((2, 4, 32, 32), (8, 4, 7, 7), (2, 2), (3, 3)), ((2, 3, 32, 32), (96, 3, 7, 7), (2, 2), (3, 3)),
                             ((2, 3, 32, 32), (8, 3, 7, 7), (1, 1), (3, 3)), ((1, 3, 32, 480), (8, 3, 7, 7), (2, 2), (3, 3))):
        node = make_node('Convolution', [np.zeros(xs, np.float32), np.zeros(ws, np.float32)], conv_data(st_, pb_, pb_))
        assert Convolution.kernel_kind(node)[0] != 'row spans (stem)', (xs, ws)


@pytest.mark.parametrize('kernel', ['default'])
def test_conv_fused_bias_and_activation_bit_exact(hip, monkeypatch, kernel):
    """Fused epilogues (bias, then ReLU or Clamp) of both convolution kernels and of the depthwise kernel equal
    the separate Add / ReLU / Clamp launches bit for bit, on the kernels the product routes to (the predecessor kernels: tests/diag_variants.py)."""
    cases = [('Convolution', (2, 32, 9, 9), (40, 32, 3, 3)),     # (r,s)-major kernel
             ('Convolution', (2, 5, 9, 9), (70, 5, 3, 3)),       # c-major kernel
             ('GroupConvolution', (2, 24, 11, 11), (24, 1, 1, 3, 3))]
    for type_, xs, ws in cases:
        x, w = rnd(1, xs), rnd(2, ws, 0.2)
        b = rnd(3, (1, ws[0], 1, 1))
        node = make_node(type_, [x, w], conv_data((1, 1), (1, 1), (1, 1), 'same_upper' if type_ == 'GroupConvolution' else 'explicit'))
        plain = first_out(hip_plugin(type_).compute(node, {0: x, 1: w}))
        biased = first_out(hip_plugin('Add').compute(make_node('Add', [plain, b]), {0: plain, 1: b}))
        for act, ref_type, data in ((('relu',), 'ReLU', None), (('clamp', 0.0, 6.0), 'Clamp', {'min': '0', 'max': '6'})):
            want = first_out(hip_plugin(ref_type).compute(make_node(ref_type, [biased], data), {0: biased}))
            fused_node = dict(node)
            fused_node['_fuse_bias'] = hip.DeviceTensor.from_numpy(b)
            fused_node['_fuse_act'] = act
            got = first_out(hip_plugin(type_).compute(fused_node, {0: x, 1: w}))
            assert_bit_exact(got, want, '{} fused bias + {}'.format(type_, act[0]))


def test_detection_output_batch_and_ties(hip):
    """Batch rule (the reference asserts N == 1): every image of a batch gives the records of its own N=1 run,
    stacked; equal class scores pick the later class, equal box scores put the later box first (what the oracle's
    stable sorts give); no candidate at all leaves a terminator in row 0."""
    z = np.load(os.path.join(helpers.GOLDEN, 'ops', 'detout_center_size_300x21.npz'))
    node, inputs, want = load_case(os.path.join(helpers.GOLDEN, 'ops', 'detout_center_size_300x21.npz'))
    loc2 = np.concatenate([inputs[0], rnd(5, inputs[0].shape, 0.5)], 0)
    conf2 = np.concatenate([inputs[1], inputs[1][:, ::-1].copy()], 0)
    node2 = dict(node)
    node2['input'] = {0: {'precision': 'FP32', 'dims': loc2.shape}, 1: {'precision': 'FP32', 'dims': conf2.shape}, 2: node['input'][2]}
    ins2 = {0: loc2, 1: conf2, 2: inputs[2]}
    got = first_out(hip_plugin('DetectionOutput').compute(node2, ins2))
    ref = first_out(oracle_plugin('DetectionOutput').compute(node2, ins2))
    assert got.shape == (1, 1, 200, 7) and np.array_equal(got[..., :2], ref[..., :2])
    assert_close(got, ref, 1e-6, 'batch of 2')
    assert_close(got[:, :, :100], want, 1e-6, 'image 0 of the batch vs the reference N=1 record list')
    # ties: quantised scores (many equal maxima per prior and equal box scores)
    conf_q = (np.round(inputs[1] * 8) / 8).astype(np.float32)
    ins_q = {0: inputs[0], 1: conf_q, 2: inputs[2]}
    got_q = first_out(hip_plugin('DetectionOutput').compute(node, ins_q))
    ref_q = first_out(oracle_plugin('DetectionOutput').compute(node, ins_q))
    assert np.array_equal(got_q[..., :2], ref_q[..., :2])
    assert_close(got_q, ref_q, 1e-6, 'tied scores')
    # nothing above the threshold
    ins_0 = {0: inputs[0], 1: np.full_like(inputs[1], 0.1), 2: inputs[2]}
    got_0 = first_out(hip_plugin('DetectionOutput').compute(node, ins_0))
    assert got_0[0, 0, 0, 0] == -1 and not got_0[0, 0, 1:].any() and not got_0[0, 0, 0, 1:].any()


def test_conv_identity_weights_asymmetric_input(hip):
    """A = I check with asymmetric data: catches a transposed accumulator map (guide section 3)."""
    c = 40
    x = (np.arange(2 * c * 6 * 7, dtype=np.float32).reshape(2, c, 6, 7) % 251) - 100.0
    w = np.zeros((c, c, 1, 1), dtype=np.float32)
    w[np.arange(c), np.arange(c), 0, 0] = 1.0
    node = make_node('Convolution', [x, w], conv_data((1, 1), (0, 0), (0, 0)))
    got = first_out(hip_plugin('Convolution').compute(node, {0: x, 1: w}))
    assert_bit_exact(got, x, 'identity 1x1 convolution')


def test_conv_linearity_full_size_layer(hip):
    """Size-independent property at a BASELINE-size layer (batch 256): conv(a*x1 + x2) == a*conv(x1) + conv(x2)."""
    xs, ws = (256, 96, 14, 14), (208, 96, 3, 3)
    x1, x2 = rnd(11, xs), rnd(12, xs)
    w = rnd(13, ws, (2.0 / (96 * 9)) ** 0.5)
    data = conv_data((1, 1), (1, 1), (1, 1))
    run = lambda x: first_out(hip_plugin('Convolution').compute(make_node('Convolution', [x, w], data), {0: x, 1: w}))
    y1, y2, y3 = run(x1), run(x2), run(2.0 * x1 + x2)
    # three results, each within ~1e-5 of the exact sum (this layer runs F(4x4,3x3) on 16x16-padded patches: coefficients up to 8 and 1/24)
    assert_close(y3, 2.0 * y1 + y2, 5e-5, 'linearity')
    # and a corner of it against the oracle
    want = first_out(oracle_plugin('Convolution').compute(make_node('Convolution', [x1[:2], w], data), {0: x1[:2], 1: w}))
    assert_close(y1[:2], want, helpers.REL_TOL, 'first two images vs oracle')


def test_diagnostic_build_variants_in_their_own_process(hip):
    """The predecessor convolution kernels (PVHIP_CONV_KERNEL=lds|wave, every PVHIP_CONV_TILE / _WTILE), the opt-in 16-byte gather and the
    fp32-MFMA ceiling probe live in the DIAGNOSTIC build only (libpvhip_diag.so, include/pvhip_diag.h): their tests, tests/diag_variants.py,
    run in a process of their own that loads that build (PVHIP_LIBRARY) -- this process keeps the product library."""
    import subprocess
    import sys
    from pyopenvino_amd import device as dev
    assert os.path.basename(dev.LIB_PATH) == 'libpvhip.so'
    env = dict(os.environ, PVHIP_LIBRARY=dev.DIAG_LIB_PATH)
    res = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(helpers.REPO, 'tests', 'diag_variants.py'), '-q', '-x', '-p', 'no:cacheprovider'],
                         capture_output=True, text=True, timeout=900, env=env, cwd=helpers.REPO)
    print(res.stdout[-1500:])
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]


def test_conv_error_behaviour_matches_reference(hip):
    """17x17 stride 2 'same_upper' with pads (0,0)/(1,1): the reference's im2col raises ValueError
    (window exceeds the padded input, Convolution.py:68); so do we."""
    x, w = rnd(1, (1, 3, 17, 17)), rnd(2, (8, 3, 3, 3))
    node = make_node('Convolution', [x, w], conv_data((2, 2), (0, 0), (1, 1), 'same_upper'))
    with pytest.raises(ValueError):
        hip_plugin('Convolution').compute(node, {0: x, 1: w})
    with pytest.raises(AssertionError):   # dtype / dims validation, Convolution.py:154-157
        bad = make_node('Convolution', [x, w], conv_data((1, 1), (0, 0), (0, 0)))
        bad['input'][0]['dims'] = (1, 3, 16, 16)
        hip_plugin('Convolution').compute(bad, {0: x, 1: w})


@pytest.mark.parametrize('m,n,k', [(1, 10, 64), (64, 64, 576), (256, 1000, 1024), (3, 513, 100), (65, 1, 17)])
def test_matmul_vs_oracle(hip, m, n, k):
    a, b = rnd(m + n, (m, k)), rnd(k, (n, k), (2.0 / k) ** 0.5)
    vs_oracle('MatMul', [a, b], {'transpose_a': 'false', 'transpose_b': 'true'}, 'matmul {}x{}x{}'.format(m, n, k))
    vs_oracle('MatMul', [np.ascontiguousarray(a.T), np.ascontiguousarray(b.T)], {'transpose_a': 'true', 'transpose_b': 'false'},
              'matmul^T {}x{}x{}'.format(m, n, k))


POOL_CASES = [
    ((4, 64, 112, 112), (3, 3), (2, 2), (0, 0), (0, 0), 'ceil'),
    ((4, 192, 28, 28), (3, 3), (1, 1), (1, 1), (1, 1), 'ceil'),
    ((9, 832, 7, 7), (3, 3), (1, 1), (1, 1), (1, 1), 'ceil'),
    ((3, 832, 14, 14), (3, 3), (2, 2), (0, 0), (0, 0), 'ceil'),
    ((8, 32, 26, 26), (2, 2), (2, 2), (0, 0), (0, 0), 'floor'),
    ((5, 64, 11, 11), (2, 2), (2, 2), (0, 0), (0, 0), 'floor'),     # floor mode leaves the last input row/column unused (mnist)
    ((3, 7, 10, 13), (3, 3), (3, 3), (0, 0), (0, 0), 'floor'),
    ((2, 3, 11, 9), (3, 2), (2, 3), (1, 0), (0, 2), 'ceil'),
    ((1, 2, 80, 90), (3, 3), (1, 1), (1, 1), (1, 1), 'ceil'),      # plane larger than the LDS group: row bands + padding
    ((2, 3, 97, 101), (3, 3), (2, 2), (1, 1), (0, 0), 'ceil'),     # row bands, stride 2, asymmetric pad, odd width (scalar loads)
    ((1, 1, 300, 300), (5, 4), (3, 2), (2, 1), (1, 2), 'floor'),   # run-time window extent, bands
]


@pytest.mark.parametrize('xs,k,s,pb,pe,rounding', POOL_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_maxpool_vs_oracle_bit_exact(hip, xs, k, s, pb, pe, rounding):
    vs_oracle('MaxPool', [rnd(sum(xs), xs, 1.0, -0.7)], pool_data(k, s, pb, pe, rounding))


def test_pools_seeded_random_shapes(hip):
    """120 seeded random MaxPool / AvgPool configurations (window 1..4, stride 1..3, pads 0..2, floor / ceil) against
    the oracle, bit for bit for MaxPool; where the reference raises (an empty window), so must the plugin."""
    rng = np.random.RandomState(7)
    ran = 0
    for case in range(120):
        type_ = 'MaxPool' if case % 3 else 'AvgPool'
        k = (int(rng.randint(1, 5)), int(rng.randint(1, 5)))
        st = (int(rng.randint(1, 4)), int(rng.randint(1, 4)))
        pb = (int(rng.randint(0, 3)), int(rng.randint(0, 3)))
        pe = (int(rng.randint(0, 3)), int(rng.randint(0, 3)))
        xs = (int(rng.randint(1, 4)), int(rng.randint(1, 9)), int(rng.randint(1, 40)), int(rng.randint(1, 40)))
        data = pool_data(k, st, pb, pe, 'ceil' if rng.rand() < 0.5 else 'floor')
        x = rnd(3000 + case, xs, 1.0, -0.5)
        node = make_node(type_, [x], data)
        try:
            want = first_out(oracle_plugin(type_).compute(node, {0: x}, kernel_type='special'))
        except Exception as exc:                     # the reference's own failure modes (np.max of an empty slice, ...)
            with pytest.raises(type(exc)):
                hip_plugin(type_).compute(node, {0: x})
            continue
        if want.size == 0:
            continue
        check(node, {0: x}, want, '{} case {}: x{} k{} s{} pb{} pe{} {}'.format(type_, case, xs, k, st, pb, pe, data['rounding_type']))
        ran += 1
    assert ran >= 80, ran


def test_maxpool_nan_propagates(hip):
    """np.max's rule (MaxPool.py:66-69): a NaN in the window is the result.  The kernels take it from v_maximum3_f32 (IEEE 754-2019
    maximum), not from bookkeeping beside a maxNum: NaNs of either sign, in corners next to the zero padding, beside +-inf, on the
    pipelined 3x3 kernel (stride 1 and 2), the one-shot kernel (2x2, 5x5 windows) and ragged extents."""
    x = rnd(5, (1, 2, 6, 6))
    x[0, 1, 2, 3] = np.nan
    vs_oracle('MaxPool', [x], pool_data((3, 3), (1, 1), (1, 1), (1, 1), 'ceil'))
    for xs, k, st, pb, pe in [((2, 24, 28, 28), (3, 3), (1, 1), (1, 1), (1, 1)), ((2, 24, 28, 28), (3, 3), (2, 2), (0, 0), (0, 0)),
                              ((3, 5, 14, 14), (3, 3), (2, 2), (0, 0), (0, 0)), ((2, 7, 13, 9), (5, 5), (1, 1), (2, 2), (2, 2)),
                              ((1, 3, 9, 9), (2, 2), (2, 2), (0, 0), (0, 0)), ((2, 832, 7, 7), (3, 3), (1, 1), (1, 1), (1, 1))]:
        x = rnd(sum(xs), xs, 2.0)
        x[0, 0, 0, 0] = np.nan
        x[-1, -1, -1, -1] = -np.nan
        x[0, 1, xs[2] // 2, :] = np.inf
        x[0, 1, xs[2] // 2, 1] = np.nan
        x[-1, 0, :, xs[3] // 2] = -np.inf
        x[-1, 0, 0, xs[3] // 2] = -np.nan
        vs_oracle('MaxPool', [x], pool_data(k, st, pb, pe, 'ceil'))


def test_avgpool_googlenet_shape(hip):
    vs_oracle('AvgPool', [rnd(3, (6, 1024, 7, 7))], pool_data((7, 7), (1, 1), (0, 0), (0, 0), 'ceil'))


@pytest.mark.parametrize('shape', [(1,), (3,), (4,), (5, 7), (2, 3, 5, 7), (8, 64, 56, 56), (1, 1, 1, 1023), (2, 1048577)])
def test_unary_sizes_bit_exact(hip, shape):
    x = rnd(sum(shape), shape, 3.0)
    vs_oracle('ReLU', [x])
    vs_oracle('Clamp', [x], {'min': '0', 'max': '6'})
    vs_oracle('Sigmoid', [x])


def test_unary_empty_tensor(hip):
    x = np.zeros((0, 4), dtype=np.float32)
    node = make_node('ReLU', [x])
    assert first_out(hip_plugin('ReLU').compute(node, {0: x})).shape == (0, 4)


BCAST = [((4, 64, 56, 56), (1, 64, 1, 1)), ((6, 1000), (1, 1000)), ((3, 5, 7, 7), (1, 5, 1, 1)), ((2, 3, 4, 5), (1, 1, 1, 1)),
         ((2, 3, 4, 5), (2, 3, 4, 5)), ((2, 3, 4, 5), (1, 3, 1, 5)), ((7, 13), (1, 13)), ((5, 3, 7, 7), (5, 1, 1, 1)),
         ((2, 3, 4, 5), (5,)), ((3, 1, 49), (1, 1, 49))]


@pytest.mark.parametrize('a_shape,b_shape', BCAST, ids=str)
def test_add_mul_broadcast_bit_exact(hip, a_shape, b_shape):
    a, b = rnd(1, a_shape), rnd(2, b_shape)
    vs_oracle('Add', [a, b], {'auto_broadcast': 'numpy'})
    vs_oracle('Multiply', [a, b], {'auto_broadcast': 'numpy'})
    vs_oracle('Multiply', [b, a], {'auto_broadcast': 'numpy'})


def test_add_rejects_non_broadcastable(hip):
    a, b = rnd(1, (2, 3)), rnd(2, (2, 4))
    with pytest.raises(ValueError):
        hip_plugin('Add').compute(make_node('Add', [a, b]), {0: a, 1: b})


@pytest.mark.parametrize('rows,cols', [(1, 10), (64, 10), (256, 1000), (3, 2049), (2, 5000)])
def test_softmax_rows(hip, rows, cols):
    x = rnd(rows + cols, (rows, cols), 4.0)
    vs_oracle('SoftMax', [x], {'axis': '1'})
    node = make_node('SoftMax', [x], {'axis': '1'})
    got = first_out(hip_plugin('SoftMax').compute(node, {0: x}))
    assert np.allclose(got.sum(axis=1), 1.0, atol=1e-5)


def test_softmax_overflow_like_reference(hip):
    """No max shift (SoftMax.py:12): logits > 88 overflow to inf/inf = NaN in the reference; same here."""
    x = np.array([[100.0, 1.0, 2.0]], dtype=np.float32)
    vs_oracle('SoftMax', [x], {'axis': '1'})


@pytest.mark.parametrize('shape,size', [((4, 64, 56, 56), 5), ((2, 192, 28, 28), 5), ((1, 7, 5, 3), 5), ((2, 9, 4, 4), 3), ((1, 6, 3, 3), 4)])
def test_lrn_vs_oracle(hip, shape, size):
    data = {'alpha': '9.9999997473787516e-05', 'beta': '0.75', 'bias': '1', 'size': str(size)}
    vs_oracle('LRN', [rnd(sum(shape), shape, 40.0), np.array([1], dtype=np.int64)], data)


def test_lrn_generic_beta(hip):
    data = {'alpha': '0.002', 'beta': '0.6', 'bias': '1.5', 'size': '5'}
    vs_oracle('LRN', [rnd(3, (2, 10, 6, 6), 10.0), np.array([1], dtype=np.int64)], data)


@pytest.mark.parametrize('xs,ks', [((3, 192, 28, 28), (64, 96, 16)), ((2, 512, 14, 14), (160, 112, 24)), ((5, 832, 7, 7), (384, 192, 48)),
                                   ((2, 32, 5, 9), (40, 8))])
def test_sibling_convolutions_as_one_launch_are_bit_identical(hip, xs, ks):
    """The 1x1 / 3x3_reduce / 5x5_reduce arms of an inception module (same input) handed over as one call
    (node['_siblings']): every output has the bits of its own launch, including one written in place into a wider
    (Concat) tensor, and matches the oracle."""
    from pyopenvino_amd import device as dev
    plugin = hip_plugin('Convolution')
    x = rnd(11, xs)
    data = conv_data((1, 1), (0, 0), (0, 0))
    ws = [rnd(20 + i, (k, xs[1], 1, 1), (2.0 / xs[1]) ** 0.5) for i, k in enumerate(ks)]
    bs = [rnd(40 + i, (1, k, 1, 1), 0.1) for i, k in enumerate(ks)]
    nodes = [make_node('Convolution', [x, w], data) for w in ws]
    assert plugin.siblings_fusable(nodes)
    alone = []
    for node, w, b in zip(nodes, ws, bs):
        nd = dict(node)
        nd['_fuse_bias'], nd['_fuse_act'] = dev.DeviceTensor.from_numpy(b), ('relu',)
        alone.append(first_out(plugin.compute(nd, {0: x, 1: w})))
        want = np.maximum(first_out(oracle_plugin('Convolution').compute(node, {0: x, 1: w}, kernel_type='special')) + b, 0)
        assert_close(alone[-1], want, helpers.REL_TOL, 'conv {}'.format(w.shape))
    wide = dev.DeviceTensor.from_numpy(np.full((xs[0], ks[0] + 7, xs[2], xs[3]), -1.0, dtype=np.float32))
    lead = dict(nodes[0])
    lead['_fuse_bias'], lead['_fuse_act'], lead['_out_into'] = dev.DeviceTensor.from_numpy(bs[0]), ('relu',), (wide, 3)
    lead['_siblings'] = [{'node': n_, 'inputs': {0: x, 1: w}, 'bias': dev.DeviceTensor.from_numpy(b), 'into': None}
                         for n_, w, b in zip(nodes[1:], ws[1:], bs[1:])]
    plugin.compute(lead, {0: x, 1: ws[0]})
    got = [np.asarray(wide)[:, 3:3 + ks[0]]] + [np.asarray(t) for t in lead['_sibling_out']]
    for g, a, k in zip(got, alone, ks):
        assert_bit_exact(np.ascontiguousarray(g), a, 'sibling with {} channels'.format(k))
    rest = np.asarray(wide)
    assert np.all(rest[:, :3] == -1.0) and np.all(rest[:, 3 + ks[0]:] == -1.0)       # neighbours in the wider tensor untouched


def test_sibling_convolutions_decline_other_geometries(hip):
    plugin = hip_plugin('Convolution')
    x = np.zeros((1, 32, 8, 8), dtype=np.float32)
    one = lambda k, kk=1, data=None: make_node('Convolution', [x, np.zeros((k, 32, kk, kk), dtype=np.float32)], data or conv_data((1, 1), (0, 0), (0, 0)))
    assert plugin.siblings_fusable([one(8), one(40)])
    assert not plugin.siblings_fusable([one(8)])
    assert not plugin.siblings_fusable([one(8), one(8, 3)])
    assert not plugin.siblings_fusable([one(8), one(8, data=conv_data((2, 2), (0, 0), (0, 0)))])
    assert not plugin.siblings_fusable([one(8)] * 7)
    x24 = np.zeros((1, 24, 8, 8), dtype=np.float32)
    odd = [make_node('Convolution', [x24, np.zeros((8, 24, 1, 1), dtype=np.float32)], conv_data((1, 1), (0, 0), (0, 0)))] * 2
    assert not plugin.siblings_fusable(odd)                                           # 24 channels: not whole 16-row stages


@pytest.mark.parametrize('xs,k', [((3, 192, 28, 28), 32), ((2, 480, 14, 14), 64), ((2, 528, 14, 14), 128), ((1, 32, 6, 10), 40),
                                  ((5, 16, 4, 4), 7), ((1, 48, 9, 36), 100),
                                  # odd widths (round 4: single-pixel groups; GoogLeNet's 7x7 modules): tiles that span many rows and images
                                  ((40, 832, 7, 7), 128), ((3, 32, 5, 9), 100), ((7, 16, 3, 3), 65), ((2, 48, 11, 13), 128)])
def test_maxpool_then_1x1_convolution_as_one_launch_is_bit_identical(hip, monkeypatch, xs, k):
    """3x3 / stride 1 / pad 1 MaxPool -> 1x1 convolution handed over as one call (node['_fuse_pool_in']): the bits of the two
    launches (zero pad cells take part in the max, NaN wins), also with fused bias + ReLU and written in place into a wider
    tensor; within the tolerance of the oracle's MaxPool -> Convolution.  Odd widths run the single-pixel-group form, which the
    default leaves off (PVHIP_FUSE_POOLCONV=1: measured slower than the two launches on the 7x7 modules)."""
    from pyopenvino_amd import device as dev
    if xs[3] % 2:
        helpers.setenv(monkeypatch, 'PVHIP_FUSE_POOLCONV', '1')
    conv, pool = hip_plugin('Convolution'), hip_plugin('MaxPool')
    x = rnd(sum(xs), xs, 1.0, -0.4)
    if k == 40:
        x[0, 1, 2, 3] = np.nan
    w, b = rnd(k, (k, xs[1], 1, 1), (2.0 / xs[1]) ** 0.5), rnd(k + 1, (1, k, 1, 1), 0.2)
    pnode = make_node('MaxPool', [x], pool_data((3, 3), (1, 1), (1, 1), (1, 1), 'ceil'))
    pnode['output'][1]['dims'] = tuple(xs)
    cnode = make_node('Convolution', [x, w], conv_data((1, 1), (0, 0), (0, 0)))
    assert conv.pooled_fusable(cnode, pnode)
    pooled = pool.compute(pnode, {0: x})[1]
    two = dict(cnode)
    two['_fuse_bias'], two['_fuse_act'] = dev.DeviceTensor.from_numpy(b), ('relu',)
    want = first_out(conv.compute(two, {0: pooled, 1: w}))
    wide = dev.DeviceTensor.from_numpy(np.full((xs[0], k + 9, xs[2], xs[3]), -1.0, dtype=np.float32))
    one = dict(cnode)
    one['_fuse_bias'], one['_fuse_act'], one['_fuse_pool_in'], one['_out_into'] = dev.DeviceTensor.from_numpy(b), ('relu',), pnode, (wide, 4)
    conv.compute(one, {0: x, 1: w})
    got = np.asarray(wide)
    assert_bit_exact(np.ascontiguousarray(got[:, 4:4 + k]), want, 'MaxPool + 1x1 convolution {} k{}'.format(xs, k))
    assert np.all(got[:, :4] == -1.0) and np.all(got[:, 4 + k:] == -1.0)
    opool = first_out(oracle_plugin('MaxPool').compute(pnode, {0: x}, kernel_type='special'))
    oracle = np.maximum(first_out(oracle_plugin('Convolution').compute(cnode, {0: opool, 1: w}, kernel_type='special')) + b, 0)
    assert_close(np.ascontiguousarray(got[:, 4:4 + k]), oracle, helpers.REL_TOL, 'MaxPool + 1x1 convolution vs oracle')


def test_maxpool_then_convolution_declines_other_geometries(hip, monkeypatch):
    conv = hip_plugin('Convolution')
    def pair(xs, k=8, kk=1, pool=((3, 3), (1, 1), (1, 1), (1, 1))):
        x = np.zeros(xs, dtype=np.float32)
        pn = make_node('MaxPool', [x], pool_data(pool[0], pool[1], pool[2], pool[3], 'ceil'))
        pn['output'][1]['dims'] = tuple(xs)
        pad = (kk // 2, kk // 2)
        return make_node('Convolution', [x, np.zeros((k, xs[1], kk, kk), dtype=np.float32)], conv_data((1, 1), pad, pad)), pn
    assert conv.pooled_fusable(*pair((2, 32, 12, 12)))
    assert conv.pooled_fusable(*pair((2, 32, 14, 14)))                   # rows of 14: 8-byte groups
    assert not conv.pooled_fusable(*pair((2, 32, 7, 7)))                 # odd width
    assert not conv.pooled_fusable(*pair((2, 32, 7, 7), k=128))
    helpers.setenv(monkeypatch, 'PVHIP_FUSE_POOLCONV', '1')             # ... unless asked for: 65 .. 128 output channels on single-pixel groups
    assert conv.pooled_fusable(*pair((2, 32, 7, 7), k=128)) and not conv.pooled_fusable(*pair((2, 32, 7, 7)))
    helpers.setenv(monkeypatch, 'PVHIP_FUSE_POOLCONV', None)
    assert not conv.pooled_fusable(*pair((2, 24, 12, 12)))               # 24 channels: not whole 16-row stages
    assert not conv.pooled_fusable(*pair((2, 32, 12, 12), k=200))
    assert not conv.pooled_fusable(*pair((2, 32, 12, 12), kk=3))
    assert not conv.pooled_fusable(*pair((2, 32, 12, 12), pool=((3, 3), (2, 2), (1, 1), (1, 1))))
    assert not conv.pooled_fusable(*pair((2, 32, 12, 12), pool=((3, 3), (1, 1), (0, 0), (0, 0))))


LRN_POOL_CASES = [
    # (x shape, pool stride, pads_begin, pads_end, rounding)
    ((2, 192, 56, 56), (2, 2), (0, 0), (0, 0), 'ceil'),      # conv2/norm2 -> pool2/3x3_s2: four bands of 7 pooled rows, clipped last window
    ((1, 16, 9, 12), (1, 1), (1, 1), (1, 1), 'ceil'),        # stride 1, zero pad cells all round
    ((2, 8, 13, 20), (2, 2), (1, 1), (0, 0), 'floor'),       # one chunk of channels, asymmetric padding
    ((3, 16, 7, 7), (1, 1), (1, 1), (1, 1), 'ceil'),         # odd width: one pixel per lane
    ((1, 24, 30, 10), (2, 2), (0, 0), (1, 1), 'ceil'),       # width 10: one pixel per lane, several bands, bottom / right pad cells
    ((1, 8, 40, 112), (2, 2), (0, 0), (0, 0), 'ceil'),       # wide rows: bands of 3 pooled rows
]


@pytest.mark.parametrize('xs,st,pb,pe,rounding', LRN_POOL_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fused_lrn_maxpool_has_the_bits_of_the_two_launches(hip, xs, st, pb, pe, rounding):
    """LRN -> 3x3 MaxPool as one launch (node['_fuse_pool']): the oracle's LRN then MaxPool within the tolerance of
    the LRN, and bit for bit what the two HIP launches give."""
    x = rnd(sum(xs), xs, 40.0)
    x[0, 1, 2, 3] = np.nan if xs[0] == 1 and xs[1] == 16 else x[0, 1, 2, 3]
    axes = np.array([1], dtype=np.int64)
    lrn_data = {'alpha': '9.9999997473787516e-05', 'beta': '0.75', 'bias': '1', 'size': '5'}
    lrn_node = make_node('LRN', [x, axes], lrn_data)
    pool_node = make_node('MaxPool', [x], pool_data((3, 3), st, pb, pe, rounding))
    want_lrn = first_out(oracle_plugin('LRN').compute(lrn_node, {0: x, 1: axes}, kernel_type='special'))
    want = first_out(oracle_plugin('MaxPool').compute(pool_node, {0: want_lrn}, kernel_type='special'))
    pool_node['output'][1]['dims'] = tuple(want.shape)
    lrn_plugin = hip_plugin('LRN')
    assert lrn_plugin.pool_fusable(lrn_node, pool_node)
    two_a = lrn_plugin.compute(dict(lrn_node), {0: x, 1: axes})[2]
    two = first_out(hip_plugin('MaxPool').compute(pool_node, {0: two_a}))
    fused_node = dict(lrn_node)
    fused_node['_fuse_pool'] = pool_node
    got = first_out(lrn_plugin.compute(fused_node, {0: x, 1: axes}))
    assert_close(got, want, helpers.REL_TOL, 'fused LRN+MaxPool {}'.format(xs))
    assert_bit_exact(got, two, 'fused LRN+MaxPool vs two launches {}'.format(xs))
    if tuple(st) == (2, 2) and tuple(pb) == (0, 0) and tuple(pe) == (0, 0) and xs[3] % 8 == 0:
        # the barrier-free wave form (opt-in: measured no faster), where it applies: the same bits (floor rounding and NaNs included below)
        from pyopenvino_amd import device as dev
        os.environ['PVHIP_LRNPOOL_WAVE'] = '1'
        try:
            dev.reload_settings()
            for xv, rnd_mode in ((x, rounding), (np.where(rnd(5, xs) > 2.2, np.nan, x).astype(np.float32), 'floor')):
                pn = make_node('MaxPool', [xv], pool_data((3, 3), st, pb, pe, rnd_mode))
                ref_a = lrn_plugin.compute(dict(make_node('LRN', [xv, axes], lrn_data)), {0: xv, 1: axes})[2]
                ref = first_out(hip_plugin('MaxPool').compute(pn, {0: ref_a}))
                pn['output'][1]['dims'] = tuple(ref.shape)
                fn = dict(make_node('LRN', [xv, axes], lrn_data))
                fn['_fuse_pool'] = pn
                assert_bit_exact(first_out(lrn_plugin.compute(fn, {0: xv, 1: axes})), ref, 'wave form {} {}'.format(xs, rnd_mode))
        finally:
            del os.environ['PVHIP_LRNPOOL_WAVE']
            dev.reload_settings()


@pytest.mark.parametrize('xs,st,pb,pe,rounding', [((2, 64, 112, 112), (2, 2), (0, 0), (0, 0), 'ceil'),     # GoogLeNet pool1 -> norm1
                                                   ((1, 16, 13, 11), (2, 2), (0, 0), (0, 0), 'ceil'),
                                                   ((3, 8, 9, 20), (1, 1), (1, 1), (1, 1), 'floor'),
                                                   ((2, 24, 28, 28), (1, 1), (1, 1), (1, 1), 'floor'),     # several outputs per lane
                                                   ((1, 40, 7, 7), (2, 2), (0, 0), (1, 1), 'ceil')])
def test_fused_maxpool_lrn_has_the_bits_of_the_two_launches(hip, xs, st, pb, pe, rounding):
    """3x3 MaxPool -> LRN as one launch (node['_fuse_lrn']): the oracle's MaxPool then LRN within the tolerance of the LRN, and
    bit for bit what the two HIP launches give (a NaN in the input included)."""
    x = rnd(sum(xs), xs, 40.0)
    x[0, 1, 2, 3] = np.nan if xs[0] == 1 and xs[1] == 16 else x[0, 1, 2, 3]
    axes = np.array([1], dtype=np.int64)
    pool_node = make_node('MaxPool', [x], pool_data((3, 3), st, pb, pe, rounding))
    pooled = first_out(oracle_plugin('MaxPool').compute(pool_node, {0: x}, kernel_type='special'))
    lrn_data = {'alpha': '9.9999997473787516e-05', 'beta': '0.75', 'bias': '1', 'size': '5'}
    lrn_node = make_node('LRN', [pooled, axes], lrn_data)
    want = first_out(oracle_plugin('LRN').compute(lrn_node, {0: pooled, 1: axes}, kernel_type='special'))
    lrn_node['output'][2]['dims'] = tuple(want.shape)
    pool_plugin = hip_plugin('MaxPool')
    assert pool_plugin.lrn_fusable(pool_node, lrn_node)
    two_a = first_out(pool_plugin.compute(dict(pool_node), {0: x}))
    two = first_out(hip_plugin('LRN').compute(dict(lrn_node), {0: two_a, 1: axes}))
    fused_node = dict(pool_node)
    fused_node['_fuse_lrn'] = lrn_node
    got = first_out(pool_plugin.compute(fused_node, {0: x}))
    finite = np.isfinite(want)
    assert (np.isfinite(got) == finite).all()
    assert_close(np.where(finite, got, 0.0), np.where(finite, want, 0.0), helpers.REL_TOL, 'fused MaxPool+LRN {}'.format(xs))
    assert_bit_exact(got, two, 'fused MaxPool+LRN vs two launches {}'.format(xs))


@pytest.mark.parametrize('xs,st,pb,pe,rounding,k_out,act', [
    ((2, 64, 112, 112), (2, 2), (0, 0), (0, 0), 'ceil', 64, ('relu',)),      # GoogLeNet pool1/3x3_s2 -> pool1/norm1 -> conv2/3x3_reduce
    ((3, 16, 24, 20), (2, 2), (0, 0), (0, 0), 'ceil', 40, None),             # ragged band, output channels that end inside a 32-channel tile
    ((1, 24, 12, 16), (1, 1), (1, 1), (1, 1), 'floor', 8, ('clamp', -0.25, 0.5)),
    ((2, 64, 30, 28), (2, 2), (0, 0), (0, 0), 'ceil', 33, ('relu',)),
])
def test_fused_maxpool_lrn_conv1x1_has_the_bits_of_the_two_launches(hip, xs, st, pb, pe, rounding, k_out, act):
    """3x3 MaxPool -> LRN -> 1x1 convolution (+ bias, activation) as ONE launch (node['_fuse_lrn'] + node['_fuse_conv'], round 5): the
    normalised value a lane holds is its column of a k = 1 outer-product MFMA with that channel's weights.  Bit for bit what MaxPool + LRN
    followed by the pointwise convolution launch give (the same ascending-channel fma chain), and the oracle's three nodes within 1e-4."""
    x = rnd(sum(xs), xs, 40.0)
    axes = np.array([1], dtype=np.int64)
    pool_node = make_node('MaxPool', [x], pool_data((3, 3), st, pb, pe, rounding))
    pooled = first_out(oracle_plugin('MaxPool').compute(pool_node, {0: x}, kernel_type='special'))
    lrn_node = make_node('LRN', [pooled, axes], {'alpha': '9.9999997473787516e-05', 'beta': '0.75', 'bias': '1', 'size': '5'})
    normed = first_out(oracle_plugin('LRN').compute(lrn_node, {0: pooled, 1: axes}, kernel_type='special'))
    lrn_node['output'][2]['dims'] = tuple(normed.shape)
    w = rnd(7, (k_out, xs[1], 1, 1), (2.0 / xs[1]) ** 0.5)
    bias = rnd(9, (1, k_out, 1, 1))
    conv_node = make_node('Convolution', [normed, w], conv_data((1, 1), (0, 0), (0, 0)))
    want = first_out(oracle_plugin('Convolution').compute(conv_node, {0: normed, 1: w}, kernel_type='special')) + bias
    if act is not None:
        want = np.where(want < 0, 0, want) if act[0] == 'relu' else np.clip(want, act[1], act[2])
    pool_plugin = hip_plugin('MaxPool')
    assert pool_plugin.lrn_conv_fusable(pool_node, lrn_node, conv_node)
    two_node = dict(pool_node)
    two_node['_fuse_lrn'] = lrn_node
    two_a = first_out(pool_plugin.compute(two_node, {0: x}))
    cn = dict(conv_node)
    cn['_fuse_bias'], cn['_fuse_act'] = hip.DeviceTensor.from_numpy(bias), act
    two = np.asarray(first_out(hip_plugin('Convolution').compute(cn, {0: two_a, 1: w})))
    fused_node = dict(two_node)
    fused_node['_fuse_conv'] = {'node': conv_node, 'w': w, 'bias': hip.DeviceTensor.from_numpy(bias), 'act': act}
    got = np.asarray(first_out(pool_plugin.compute(fused_node, {0: x})))
    assert got.shape == want.shape
    assert_close(got, want.astype(np.float32), helpers.REL_TOL, 'fused MaxPool+LRN+1x1 {}'.format(xs))
    assert_bit_exact(got, two, 'fused MaxPool+LRN+1x1 vs two launches {}'.format(xs))
    # a NaN in the input poisons exactly what it poisons in the two launches
    x2 = x.copy()
    x2[0, 1, 2, 3] = np.nan
    two_b = np.asarray(first_out(hip_plugin('Convolution').compute(dict(cn), {0: first_out(pool_plugin.compute(dict(two_node), {0: x2})), 1: w})))
    got_b = np.asarray(first_out(pool_plugin.compute(dict(fused_node), {0: x2})))
    assert np.isnan(got_b).any() and np.array_equal(np.isnan(got_b), np.isnan(two_b))
    assert_bit_exact(np.nan_to_num(got_b), np.nan_to_num(two_b), 'fused MaxPool+LRN+1x1 vs two launches, a NaN in the input {}'.format(xs))
    # what the kernel does not cover is declined: more than 64 channels either side, a 3x3 convolution, a stride
    big = make_node('Convolution', [normed, np.zeros((96, xs[1], 1, 1), np.float32)], conv_data((1, 1), (0, 0), (0, 0)))
    assert not pool_plugin.lrn_conv_fusable(pool_node, lrn_node, big)
    k3 = make_node('Convolution', [normed, np.zeros((8, xs[1], 3, 3), np.float32)], conv_data((1, 1), (1, 1), (1, 1)))
    assert not pool_plugin.lrn_conv_fusable(pool_node, lrn_node, k3)


def test_fused_maxpool_lrn_declines_what_it_does_not_cover(hip):
    pool_plugin = hip_plugin('MaxPool')
    axes = np.array([1], dtype=np.int64)
    def pair(xs, size='5', beta='0.75', kernel=(3, 3), st=(2, 2)):
        x = np.zeros(xs, dtype=np.float32)
        pn = make_node('MaxPool', [x], pool_data(kernel, st, (0, 0), (0, 0), 'ceil'))
        oh, ow = pool_plugin.calc_output_shape(xs[2:], kernel, st, (0, 0), (0, 0), 'ceil', 'explicit')
        ln = make_node('LRN', [np.zeros((xs[0], xs[1], oh, ow), dtype=np.float32), axes], {'alpha': '1e-4', 'beta': beta, 'bias': '1', 'size': size})
        ln['output'][2]['dims'] = (xs[0], xs[1], oh, ow)
        return pn, ln
    assert pool_plugin.lrn_fusable(*pair((2, 64, 112, 112)))
    assert not pool_plugin.lrn_fusable(*pair((2, 60, 112, 112)))           # channels not a multiple of 8
    assert not pool_plugin.lrn_fusable(*pair((2, 64, 112, 112), size='3'))
    assert not pool_plugin.lrn_fusable(*pair((2, 64, 112, 112), beta='0.6'))
    assert not pool_plugin.lrn_fusable(*pair((2, 64, 112, 112), kernel=(2, 2)))


def test_fused_lrn_maxpool_declines_what_it_does_not_cover(hip):
    lrn_plugin = hip_plugin('LRN')
    axes = np.array([1], dtype=np.int64)
    def pair(xs, size='5', beta='0.75', kernel=(3, 3), st=(2, 2)):
        x = np.zeros(xs, dtype=np.float32)
        ln = make_node('LRN', [x, axes], {'alpha': '1e-4', 'beta': beta, 'bias': '1', 'size': size})
        pn = make_node('MaxPool', [x], pool_data(kernel, st, (0, 0), (0, 0), 'ceil'))
        oh, ow = hip_plugin('MaxPool').calc_output_shape(xs[2:], kernel, st, (0, 0), (0, 0), 'ceil', 'explicit')
        pn['output'][1]['dims'] = (xs[0], xs[1], oh, ow)
        return ln, pn
    assert lrn_plugin.pool_fusable(*pair((2, 64, 56, 56)))
    assert not lrn_plugin.pool_fusable(*pair((2, 60, 56, 56)))            # channels not a multiple of 8
    assert not lrn_plugin.pool_fusable(*pair((2, 64, 56, 56), size='3'))
    assert not lrn_plugin.pool_fusable(*pair((2, 64, 56, 56), beta='0.6'))
    assert not lrn_plugin.pool_fusable(*pair((2, 64, 56, 56), kernel=(2, 2)))
    assert not lrn_plugin.pool_fusable(*pair((2, 64, 56, 56), st=(3, 3)))
    assert not lrn_plugin.pool_fusable(*pair((1, 8, 5, 2000)))             # three input rows do not fit one workgroup


def test_fused_lrn_pool_query_and_launch_agree(hip):
    """pvhip_lrn_maxpool_supported / pvhip_maxpool_lrn_supported == 1 must imply that the launch does not answer EUNSUPPORTED
    (plan_fusion folds the second node away on the query's word).  Random geometries plus the one that used to disagree: a pooled
    row wider than the input row (pads of 2 at stride 1) with a tall band = more than four pooled outputs per lane."""
    import ctypes
    from pyopenvino_amd import device as dev
    rng = np.random.default_rng(5)
    cases = [(1, 8, 124, 8, 1, 2, 2, 2, 2), (1, 8, 126, 8, 1, 2, 2, 2, 2), (1, 8, 100, 10, 1, 2, 2, 2, 2)]
    for _ in range(120):
        st = int(rng.integers(1, 3))
        cases.append((int(rng.integers(1, 3)), 8 * int(rng.integers(1, 4)), int(rng.integers(1, 140)), int(rng.integers(1, 80)), st,
                      int(rng.integers(0, 3)), int(rng.integers(0, 3)), int(rng.integers(0, 3)), int(rng.integers(0, 3))))
    said_yes = 0
    for n, c, h, w, st, pt, pl, pb, pr in cases:
        oh, ow = (h + pt + pb - 3) // st + 1, (w + pl + pr - 3) // st + 1
        if oh < 1 or ow < 1:
            continue
        x = dev.DeviceTensor.from_numpy(rng.standard_normal((n, c, h, w)).astype(np.float32))
        y = dev.DeviceTensor.empty((n, c, oh, ow))
        geo = (oh, ow, 3, 3, st, st, pt, pl, pb, pr)
        if dev.call('pvhip_lrn_maxpool_supported', n, c, h, w, 5, 0.75, 1.0, *geo):
            said_yes += 1
            dev.call('pvhip_lrn_maxpool_f32', ctypes.c_void_p(x.ptr), ctypes.c_void_p(y.ptr), n, c, h, w, 5, 1e-4, 0.75, 1.0, *geo)
        if dev.call('pvhip_maxpool_lrn_supported', n, c, h, w, *geo, 5, 0.75, 1.0):
            said_yes += 1
            dev.call('pvhip_maxpool_lrn_f32', ctypes.c_void_p(x.ptr), ctypes.c_void_p(y.ptr), n, c, h, w, *geo, 5, 1e-4, 0.75, 1.0)
    dev.synchronize()
    assert said_yes > 40
    assert not dev.call('pvhip_lrn_maxpool_supported', 1, 8, 124, 8, 5, 0.75, 1.0, 126, 10, 3, 3, 1, 1, 2, 2, 2, 2)


# Rows for the instantiations of lrn_maxpool3x3_kernel / maxpool3x3_lrn_kernel <5, VEC, BETA_MODE, ST, NI> that the cases above do not
# launch.  Which one a row reaches was derived from the plan rule (plan_lrn_pool: vec = 4 where w % 4 == 0, the largest band of pooled
# rows whose input rows fit 256 lanes x vec, bands evened out, ni = ceil(band_rows * ow / 256) rounded up to 1 / 2 / 4); there is no form
# query for the fused entries, so nothing here can ask the library.
LRN_POOL_FORM_ROWS = [
    # (x shape, stride, (pt, pl, pb, pr), rounding, NaN in the input)
    ((1, 8, 41, 4), 1, (2, 2, 2, 2), 'floor', True),        # vec 4, ST 1, NI 2: 43 x 6 outputs in one band
    ((1, 8, 84, 4), 1, (2, 2, 2, 2), 'floor', False),       # vec 4, ST 1, NI 4 (ni = 3)
    ((2, 16, 27, 36), 1, (1, 1, 1, 1), 'floor', False),     # vec 4, ST 1, NI 2: two bands of 14 rows, two chunks of channels
    ((1, 8, 50, 3), 1, (2, 2, 2, 2), 'floor', False),       # vec 1, ST 1, NI 2
    ((1, 8, 252, 1), 1, (2, 2, 2, 2), 'floor', False),      # vec 1, ST 1, NI 4 (ni = 3)
    ((1, 8, 169, 4), 2, (2, 2, 2, 2), 'floor', False),      # vec 4, ST 2, NI 2
    ((1, 16, 9, 8), 2, (0, 0, 0, 0), 'ceil', False),        # vec 4, ST 2, NI 1, four outputs per lane (pool4); PVHIP_TUNE6=1: one per lane
]
# beta = 0.75 with bias = 0 is beta mode 1 (two square roots and a division instead of the log2 / exp2 pair of mode 4)
LRN_POOL_MODE1_ROWS = [
    ((1, 16, 9, 12), 1, (1, 1, 1, 1), 'ceil', False),
    ((2, 8, 13, 20), 2, (1, 1, 0, 0), 'floor', False),
]


def _pooled_extent(size, st, p0, p1, rounding):
    span = size + p0 + p1 - 3
    return (span // st if rounding == 'floor' else -(-span // st)) + 1


def _lrn_pool_launches(x, st, pads, rounding, bias):
    """(LRN then MaxPool in two launches, the same fused, MaxPool then LRN in two launches, the same fused) through the C entries."""
    from pyopenvino_amd import device as dev
    n, c, h, w = x.shape
    pt, pl, pb, pr = pads
    oh, ow = _pooled_extent(h, st, pt, pb, rounding), _pooled_extent(w, st, pl, pr, rounding)
    geo = (oh, ow, 3, 3, st, st, pt, pl, pb, pr)
    lrn = (5, 1e-4, 0.75, bias)
    p = lambda t: ctypes.c_void_p(t.ptr)
    xd, mid_l, mid_p = dev.DeviceTensor.from_numpy(x), dev.DeviceTensor.empty(x.shape), dev.DeviceTensor.empty((n, c, oh, ow))
    out = [dev.DeviceTensor.empty((n, c, oh, ow)) for _ in range(4)]
    assert dev.call('pvhip_lrn_maxpool_supported', n, c, h, w, 5, 0.75, bias, *geo)
    assert dev.call('pvhip_maxpool_lrn_supported', n, c, h, w, *geo, 5, 0.75, bias)
    dev.call('pvhip_lrn_f32', p(xd), p(mid_l), n, c, h * w, *lrn)
    dev.call('pvhip_maxpool2d_f32', p(mid_l), p(out[0]), n, c, h, w, *geo)
    dev.call('pvhip_lrn_maxpool_f32', p(xd), p(out[1]), n, c, h, w, *lrn, *geo)
    dev.call('pvhip_maxpool2d_f32', p(xd), p(mid_p), n, c, h, w, *geo)
    dev.call('pvhip_lrn_f32', p(mid_p), p(out[2]), n, c, oh * ow, *lrn)
    dev.call('pvhip_maxpool_lrn_f32', p(xd), p(out[3]), n, c, h, w, *geo, *lrn)
    dev.synchronize()
    return [np.asarray(t) for t in out]


@pytest.mark.parametrize('xs,st,pads,rounding,nan,bias', [r + (1.0,) for r in LRN_POOL_FORM_ROWS] + [r + (0.0,) for r in LRN_POOL_MODE1_ROWS],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fused_lrn_pool_instantiations_have_the_bits_of_the_two_launches(hip, xs, st, pads, rounding, nan, bias):
    """Both orders of LRN and 3x3 MaxPool as one launch, on the shapes that reach the kernel instantiations the model-shaped cases do
    not: bit for bit what the two launches give, and, where the oracle takes the padding, its two nodes within the tolerance."""
    from pyopenvino_amd import device as dev
    x = rnd(sum(xs) + st, xs, 40.0)
    x[x == 0.0] = 1.0
    if nan:
        x[0, 1, 2, 3] = np.nan
    lp_two, lp_one, pl_two, pl_one = _lrn_pool_launches(x, st, pads, rounding, bias)
    assert_bit_exact(lp_one, lp_two, 'fused LRN+MaxPool vs two launches {} {}'.format(xs, pads))
    assert_bit_exact(pl_one, pl_two, 'fused MaxPool+LRN vs two launches {} {}'.format(xs, pads))
    assert np.isnan(lp_one).any() == nan and np.isnan(pl_one).any() == nan
    if bias == 1.0 and max(pads) <= 1:
        axes = np.array([1], dtype=np.int64)
        lrn_data = {'alpha': '9.9999997473787516e-05', 'beta': '0.75', 'bias': '1', 'size': '5'}
        pool_node = make_node('MaxPool', [x], pool_data((3, 3), (st, st), pads[:2], pads[2:], rounding))
        o_lrn = first_out(oracle_plugin('LRN').compute(make_node('LRN', [x, axes], lrn_data), {0: x, 1: axes}, kernel_type='special'))
        assert_close(lp_one, first_out(oracle_plugin('MaxPool').compute(pool_node, {0: o_lrn}, kernel_type='special')), helpers.REL_TOL,
                     'fused LRN+MaxPool vs oracle {}'.format(xs))
        o_pool = first_out(oracle_plugin('MaxPool').compute(pool_node, {0: x}, kernel_type='special'))
        assert_close(pl_one, first_out(oracle_plugin('LRN').compute(make_node('LRN', [o_pool, axes], lrn_data), {0: o_pool, 1: axes},
                                                                     kernel_type='special')), helpers.REL_TOL, 'fused MaxPool+LRN vs oracle {}'.format(xs))
    if st == 2 and max(pads) == 0 and xs[3] % 4 == 0:
        os.environ['PVHIP_TUNE6'] = '1'         # the one-output-per-lane body of lrn_maxpool3x3_kernel on a shape that takes pool4 by default
        try:
            dev.reload_settings()
            assert_bit_exact(_lrn_pool_launches(x, st, pads, rounding, bias)[1], lp_two, 'fused LRN+MaxPool, one output per lane {}'.format(xs))
        finally:
            del os.environ['PVHIP_TUNE6']
            dev.reload_settings()


@pytest.mark.parametrize('xs,st,pb,pe,rounding,k_out,act', [
    ((1, 24, 12, 16), (1, 1), (1, 1), (1, 1), 'floor', 8, ('clamp', -0.25, 0.5)),       # one 32-channel tile of outputs
    ((3, 16, 24, 20), (2, 2), (0, 0), (0, 0), 'ceil', 40, None),                        # two
])
def test_fused_maxpool_lrn_conv1x1_beta_mode_1_has_the_bits_of_the_three_launches(hip, xs, st, pb, pe, rounding, k_out, act):
    """maxpool3x3_lrn_conv1x1_kernel with bias = 0 (beta mode 1): bit for bit MaxPool, LRN and the pointwise convolution launched one
    after the other (those are held to float64 in mode 1 by the LRN-*-m1 rows of test_pool_norm_forms.py)."""
    x = rnd(sum(xs), xs, 40.0)
    x[x == 0.0] = 1.0
    axes = np.array([1], dtype=np.int64)
    pool_plugin = hip_plugin('MaxPool')
    pool_node = make_node('MaxPool', [x], pool_data((3, 3), st, pb, pe, rounding))
    pooled = first_out(pool_plugin.compute(dict(pool_node), {0: x}))
    lrn_node = make_node('LRN', [pooled, axes], {'alpha': '9.9999997473787516e-05', 'beta': '0.75', 'bias': '0', 'size': '5'})
    lrn_node['output'][2]['dims'] = tuple(pooled.shape)
    normed = first_out(hip_plugin('LRN').compute(dict(lrn_node), {0: pooled, 1: axes}))
    w = rnd(7, (k_out, xs[1], 1, 1), (2.0 / xs[1]) ** 0.5)
    bias = rnd(9, (1, k_out, 1, 1))
    conv_node = make_node('Convolution', [normed, w], conv_data((1, 1), (0, 0), (0, 0)))
    assert pool_plugin.lrn_conv_fusable(pool_node, lrn_node, conv_node)
    cn = dict(conv_node)
    cn['_fuse_bias'], cn['_fuse_act'] = hip.DeviceTensor.from_numpy(bias), act
    three = np.asarray(first_out(hip_plugin('Convolution').compute(cn, {0: normed, 1: w})))
    fused_node = dict(pool_node)
    fused_node['_fuse_lrn'] = lrn_node
    fused_node['_fuse_conv'] = {'node': conv_node, 'w': w, 'bias': hip.DeviceTensor.from_numpy(bias), 'act': act}
    got = np.asarray(first_out(pool_plugin.compute(fused_node, {0: x})))
    assert np.isfinite(got).all()
    assert_bit_exact(got, three, 'fused MaxPool+LRN+1x1, beta mode 1, vs three launches {}'.format(xs))


def test_concat_inception_shapes_bit_exact(hip):
    parts = [rnd(i, (3, c, 7, 7)) for i, c in enumerate((384, 384, 128, 128))]
    vs_oracle('Concat', parts, {'axis': '1'})
    parts = [rnd(i, (2, c, 3)) for i, c in enumerate((5, 1, 7))]
    vs_oracle('Concat', parts, {'axis': '1'})
    parts = [rnd(i, (2, 3, c)) for i, c in enumerate((5, 1, 7))]
    vs_oracle('Concat', parts, {'axis': '2'})
    vs_oracle('Concat', [rnd(1, (2, 3)), rnd(2, (4, 3))], {'axis': '0'})


def test_transpose_reshape(hip):
    x = rnd(1, (8, 64, 3, 3))
    vs_oracle('Transpose', [x, np.array([0, 2, 3, 1], dtype=np.int64)])
    vs_oracle('Transpose', [rnd(2, (3, 4, 5)), np.array([2, 0, 1], dtype=np.int64)])
    vs_oracle('Reshape', [x, np.array([-1, 576], dtype=np.int64)], {'special_zero': 'false'})
    vs_oracle('Reshape', [x, np.array([0, -1], dtype=np.int64)], {'special_zero': 'true'})


@pytest.mark.parametrize('xs,st,pb,pe', [((2, 32, 150, 150), (1, 1), (1, 1), (1, 1)), ((2, 64, 150, 150), (2, 2), (0, 0), (1, 1)),
                                         ((3, 512, 19, 19), (2, 2), (1, 1), (1, 1)), ((2, 1024, 10, 10), (1, 1), (1, 1), (1, 1))])
def test_depthwise_conv_vs_oracle(hip, xs, st, pb, pe):
    w = rnd(7, (xs[1], 1, 1, 3, 3), 0.4)
    vs_oracle('GroupConvolution', [rnd(sum(xs), xs), w], conv_data(st, pb, pe, 'same_upper'))


def test_depthwise_pipelined_kernel_has_the_bits_of_the_one_shot_kernel(hip, monkeypatch):
    """dwconv3x3_cols_kernel (3x3, stride 1 / 2: persistent, LDS-DMA, weights in registers) against dwconv2d_lds_kernel
    (PVHIP_DWCONV_COLS=0): the same products in the same order -- bit for bit, with bias + ReLU / Clamp fused, on MobileNet's
    extents, odd extents, several images, asymmetric padding, and with infinities on the border (a padded tap is 0 * w, not inf * 0)."""
    from pyopenvino_amd import device as dev
    cases = [((2, 32, 150, 150), (1, 1), (1, 1), (1, 1)), ((2, 64, 150, 150), (2, 2), (0, 0), (1, 1)), ((3, 128, 75, 75), (1, 1), (1, 1), (1, 1)),
             ((2, 128, 75, 75), (2, 2), (1, 1), (1, 1)), ((3, 512, 19, 19), (2, 2), (1, 1), (1, 1)), ((2, 1024, 10, 10), (1, 1), (1, 1), (1, 1)),
             ((1, 8, 7, 13), (1, 1), (1, 1), (1, 1)), ((5, 3, 9, 9), (2, 2), (0, 0), (1, 1)), ((1, 4, 3, 3), (1, 1), (1, 1), (1, 1)),
             ((2, 16, 38, 38), (1, 1), (0, 0), (0, 0))]
    for xs, st, pb, pe in cases:
        x = rnd(sum(xs), xs, 3.0)
        x[0, 0, 0, :] = np.inf
        x[-1, -1, :, -1] = -np.inf
        w, b = rnd(7, (xs[1], 1, 1, 3, 3), 0.4), rnd(8, (1, xs[1], 1, 1))
        for act in (None, ('relu',), ('clamp', 0.0, 6.0)):
            outs = {}
            for mode in ('1', '2', '0'):                     # lanes store their outputs / through an output stage in LDS / one-shot
                helpers.setenv(monkeypatch, 'PVHIP_DWCONV_COLS', mode)
                dev.reload_settings()
                node = make_node('GroupConvolution', [x, w], conv_data(st, pb, pe, 'explicit'))
                if act is not None:
                    node['_fuse_bias'], node['_fuse_act'] = dev.DeviceTensor.from_numpy(b), act
                outs[mode] = np.asarray(first_out(hip_plugin('GroupConvolution').compute(node, {0: x, 1: w})))
            for mode in ('1', '2'):
                assert_bit_exact(outs[mode], outs['0'], 'depthwise {} stride {} pads {} {} act {} mode {}'.format(xs, st, pb, pe, act, mode))
    monkeypatch.delenv('PVHIP_DWCONV_COLS', raising=False)
    dev.reload_settings()


def test_hipgraph_capture_and_replay(hip):
    """pvhip_graph_*: a short sequence of launches captured once on the compute stream and replayed on new input
    contents gives what the eager launches give (the buffers are fixed, as a captured forward pass requires)."""
    import ctypes
    P = ctypes.c_void_p
    x = hip.DeviceTensor.from_numpy(rnd(1, (3, 8, 12, 12)))
    b = hip.DeviceTensor.from_numpy(rnd(2, (3, 8, 12, 12)))
    t, y = hip.DeviceTensor.empty(x.shape), hip.DeviceTensor.empty(x.shape)
    hip.call('pvhip_relu_f32', P(x.ptr), P(t.ptr), x.size)            # eager run first (also loads the kernels)
    hip.synchronize()
    hip.call('pvhip_graph_begin_capture')
    hip.call('pvhip_relu_f32', P(x.ptr), P(t.ptr), x.size)
    hip.call('pvhip_sigmoid_f32', P(t.ptr), P(y.ptr), x.size)
    handle = ctypes.c_void_p(0)
    hip.call('pvhip_graph_end_capture', ctypes.byref(handle))
    try:
        for seed in (3, 4):
            new = rnd(seed, x.shape)
            hip.call('pvhip_memcpy_h2d', P(x.ptr), new.ctypes.data_as(P), new.nbytes)
            hip.call('pvhip_graph_launch', handle)
            want = first_out(oracle_plugin('Sigmoid').compute(make_node('Sigmoid', [new]), {0: np.where(new < 0, 0, new).astype(np.float32)}))
            assert_close(y.numpy(), want, 1e-6, 'replay {}'.format(seed))
    finally:
        hip.call('pvhip_graph_destroy', handle)
    del b


def test_device_tensor_roundtrip_and_pool_reuse(hip):
    x = rnd(1, (5, 7, 3))
    t = hip.DeviceTensor.from_numpy(x)
    assert t.shape == x.shape and t.dtype == np.float32
    assert_bit_exact(np.asarray(t), x)
    assert_bit_exact(np.asarray(t.reshape(35, -1)), x.reshape(35, 3))
    ptr = t.ptr
    del t
    t2 = hip.DeviceTensor.empty((5, 7, 3))
    assert t2.ptr == ptr, 'a freed block of the same size is reused'


def test_read_backs_land_in_page_locked_memory_and_the_pool_reuses_it(hip, monkeypatch):
    """DeviceTensor.numpy() of up to a few MB copies into page-locked host memory (pvhip_host_alloc: one DMA instead of the runtime's staged copy
    into pageable memory); the block goes back to the pool when the array AND its views are gone, larger read-backs and PVHIP_PINNED_RESULTS=0
    use pageable memory.  The values are the tensor's either way; an array stays valid after the tensor is freed."""
    import gc
    from pyopenvino_amd import device as dev
    x = rnd(3, (256, 1000))
    t = hip.DeviceTensor.from_numpy(x)
    a = t.numpy()
    assert_bit_exact(a, x)
    assert a.flags.writeable and a.base is not None                  # a view of a pool block
    addr, size = a.ctypes.data, 1 << (x.nbytes - 1).bit_length()
    row = a[7]
    del a
    gc.collect()
    assert addr not in dev._pinned_free.get(size, []), 'a view keeps the block out of the pool'
    del row
    gc.collect()
    assert addr in dev._pinned_free.get(size, [])
    b = t.numpy()
    assert b.ctypes.data == addr, 'the pool hands the block out again'
    del t
    assert_bit_exact(b, x)
    big = hip.DeviceTensor.from_numpy(rnd(4, (3, 1024, 1024)))       # 12 MB: pageable
    assert big.numpy().base is None
    helpers.setenv(monkeypatch, 'PVHIP_PINNED_RESULTS', '0')
    assert hip.DeviceTensor.from_numpy(x).numpy().base is None


# ---------------------------------------------------------------------------------------------------------------------
# f16-MFMA kernels for FP16 IRs: fp16 operands, fp32 accumulation
FP16_TOL = 2e-2      # against the reference's OWN float16 arithmetic (it accumulates in float16: 11 significant bits per partial sum)


def f16r(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


def test_conv_f16_mfma_vs_oracle_on_rounded_operands(hip):
    """pvhip_conv2d_f16 (node['_f16_mfma']) against the oracle convolution of the SAME operands rounded to fp16: products of two
    fp16 values are exact in fp32, so only the fp32 summation order differs -- 1e-5, element by element too.  Windows 1x1 ..
    7x7, strides, asymmetric padding, channel counts that are not multiples of the 32-row stage or the 64-channel tile, several
    images, a pixel count that is not a multiple of 128; then bias + ReLU fused and written in place into a wider tensor."""
    from pyopenvino_amd import device as dev
    cases = [((2, 3, 20, 20), 32, 3, (2, 2), (0, 0), (1, 1)), ((1, 64, 14, 14), 96, 1, (1, 1), (0, 0), (0, 0)),
             ((3, 20, 13, 11), 70, 3, (1, 1), (1, 1), (1, 1)), ((2, 16, 12, 12), 40, 5, (1, 1), (2, 2), (2, 2)),
             ((1, 3, 37, 37), 64, 7, (2, 2), (3, 3), (3, 3)), ((2, 33, 9, 9), 5, 3, (1, 1), (0, 0), (0, 0))]
    for xs, k, kk, st, pb, pe in cases:
        x, w = rnd(sum(xs), xs), rnd(k, (k, xs[1], kk, kk), (2.0 / (xs[1] * kk * kk)) ** 0.5)
        node = make_node('Convolution', [x, w], conv_data(st, pb, pe))
        node['_f16_mfma'] = True
        got = first_out(hip_plugin('Convolution').compute(dict(node), {0: x, 1: w}))
        want = first_out(oracle_plugin('Convolution').compute(make_node('Convolution', [x, w], conv_data(st, pb, pe)), {0: f16r(x), 1: f16r(w)},
                                                              kernel_type='special'))
        assert_close(got, want, 1e-5, 'f16 conv {} k{} {}x{}'.format(xs, k, kk, kk))
        plain = first_out(hip_plugin('Convolution').compute(make_node('Convolution', [x, w], conv_data(st, pb, pe)), {0: x, 1: w}))
        assert not np.array_equal(got, plain), 'the fp32 kernel ran'
        assert_close(got, plain, 5e-3, 'f16 vs fp32 operands', elementwise=False)
    x, w, b = np.abs(rnd(1, (2, 24, 10, 6))), rnd(2, (40, 24, 3, 3), 0.1), rnd(3, (1, 40, 1, 1), 0.3)
    node = make_node('Convolution', [x, w], conv_data((1, 1), (1, 1), (1, 1)))
    node['_f16_mfma'] = True
    wide = dev.DeviceTensor.from_numpy(np.full((2, 50, 10, 6), -1.0, dtype=np.float32))
    fused = dict(node)
    fused['_fuse_bias'], fused['_fuse_act'], fused['_out_into'] = dev.DeviceTensor.from_numpy(b), ('relu',), (wide, 7)
    hip_plugin('Convolution').compute(fused, {0: x, 1: w})
    got = np.asarray(wide)
    unfused = first_out(hip_plugin('Convolution').compute(dict(node), {0: x, 1: w}))
    assert_bit_exact(got[:, 7:47], np.maximum(unfused + b, 0).astype(np.float32), 'f16 conv: fused epilogue')
    assert np.all(got[:, :7] == -1.0) and np.all(got[:, 47:] == -1.0)


def test_conv_f16_dma_form_vs_oracle_and_first_f16_kernel(hip, monkeypatch):
    """pvhip_conv2d_f16_dma (FP16 IRs, C % 16 == 0: the fp32 tiles of the LDS-DMA kernel, one v_mfma_f32_32x32x16_f16 per stage and
    32-channel tile) against the oracle on fp16-ROUNDED operands (1e-5: only the fp32 summation order differs) and against the first
    f16 kernel (PVHIP_CONV_F16_DMA=0: the same arithmetic in c-major order).  3x3 / 5x5 / 7x7 / 1x1 windows, strides, padding, the
    pointwise copy (H*W % 4 == 0) and the gather (odd H*W), K_out below / between / above whole tiles, a pixel count that is not a
    multiple of 128, bias + ReLU fused into a wider tensor."""
    from pyopenvino_amd import device as dev
    cases = [((2, 16, 12, 12), 40, 3, (1, 1), (1, 1), (1, 1)), ((3, 64, 14, 14), 96, 1, (1, 1), (0, 0), (0, 0)),
             ((2, 32, 7, 7), 16, 1, (1, 1), (0, 0), (0, 0)), ((1, 48, 9, 11), 208, 3, (2, 2), (1, 1), (1, 1)),
             ((2, 16, 13, 13), 33, 5, (1, 1), (2, 2), (2, 2)), ((5, 32, 6, 6), 70, 7, (1, 1), (3, 3), (3, 3)),
             ((1, 160, 7, 7), 320, 3, (1, 1), (1, 1), (1, 1)), ((2, 16, 28, 28), 32, 5, (1, 1), (2, 2), (2, 2)),
             # c-major (C % 16 != 0; round 4: GoogLeNet's conv1 as an FP16 layer): through the padding pass without a window test, with the
             # window test where the plugin does not pad (no padding at all; PVHIP_CONV_PREPAD=0 below), reductions that end inside a stage
             ((2, 3, 37, 37), 64, 7, (2, 2), (3, 3), (3, 3)), ((1, 3, 20, 20), 32, 3, (2, 2), (0, 0), (1, 1)), ((3, 20, 13, 11), 70, 3, (1, 1), (1, 1), (1, 1)),
             ((2, 33, 9, 9), 5, 3, (1, 1), (0, 0), (0, 0)), ((2, 24, 10, 6), 40, 5, (1, 1), (2, 2), (2, 2))]
    for xs, k, kk, st, pb, pe in cases:
        x, w = rnd(sum(xs), xs), rnd(k, (k, xs[1], kk, kk), (2.0 / (xs[1] * kk * kk)) ** 0.5)
        assert dev.call('pvhip_conv2d_f16_dma_supported', xs[1], kk, kk)
        outs = {}
        helpers.setenv(monkeypatch, 'PVHIP_CONV_F16_SPAN', '0')
        for mode in ('1', '0'):
            helpers.setenv(monkeypatch, 'PVHIP_CONV_F16_DMA', mode)
            dev.reload_settings()
            node = make_node('Convolution', [x, w], conv_data(st, pb, pe))
            node['_f16_mfma'] = True
            outs[mode] = np.asarray(first_out(hip_plugin('Convolution').compute(node, {0: x, 1: w})))
            assert node['_hip_f16'] == ('lds-dma' if mode == '1' else 'gather')
        want = first_out(oracle_plugin('Convolution').compute(make_node('Convolution', [x, w], conv_data(st, pb, pe)), {0: f16r(x), 1: f16r(w)},
                                                              kernel_type='special'))
        assert_close(outs['1'], want, 1e-5, 'f16 LDS-DMA form {} k{} {}x{}'.format(xs, k, kk, kk))
        assert_close(outs['1'], outs['0'], 1e-5, 'f16 LDS-DMA form vs the first f16 kernel {} k{}'.format(xs, k))
    monkeypatch.delenv('PVHIP_CONV_F16_DMA', raising=False)
    dev.reload_settings()
    assert dev.call('pvhip_conv2d_f16_dma_supported', 3, 7, 7) and not dev.call('pvhip_conv2d_f16_dma_supported', 3, 8, 8)
    helpers.setenv(monkeypatch, 'PVHIP_CONV_PREPAD', '0')          # the c-major form with its window test (no padding pass)
    dev.reload_settings()
    x, w = rnd(9, (2, 3, 21, 17)), rnd(10, (24, 3, 5, 5), 0.2)
    node = make_node('Convolution', [x, w], conv_data((2, 1), (2, 2), (1, 2)))
    node['_f16_mfma'] = True
    got = np.asarray(first_out(hip_plugin('Convolution').compute(node, {0: x, 1: w})))
    assert node['_hip_f16'] == 'lds-dma'
    want = first_out(oracle_plugin('Convolution').compute(make_node('Convolution', [x, w], conv_data((2, 1), (2, 2), (1, 2))), {0: f16r(x), 1: f16r(w)},
                                                          kernel_type='special'))
    assert_close(got, want, 1e-5, 'f16 LDS-DMA form, c-major with the window test')
    monkeypatch.delenv('PVHIP_CONV_PREPAD', raising=False)
    dev.reload_settings()
    x, w, b = np.abs(rnd(1, (2, 32, 10, 6))), rnd(2, (40, 32, 3, 3), 0.1), rnd(3, (1, 40, 1, 1), 0.3)
    node = make_node('Convolution', [x, w], conv_data((1, 1), (1, 1), (1, 1)))
    node['_f16_mfma'] = True
    wide = dev.DeviceTensor.from_numpy(np.full((2, 50, 10, 6), -1.0, dtype=np.float32))
    fused = dict(node)
    fused['_fuse_bias'], fused['_fuse_act'], fused['_out_into'] = dev.DeviceTensor.from_numpy(b), ('relu',), (wide, 7)
    hip_plugin('Convolution').compute(fused, {0: x, 1: w})
    got = np.asarray(wide)
    unfused = first_out(hip_plugin('Convolution').compute(dict(node), {0: x, 1: w}))
    assert_bit_exact(got[:, 7:47], np.maximum(unfused + b, 0).astype(np.float32), 'f16 LDS-DMA form: fused epilogue')
    assert np.all(got[:, :7] == -1.0) and np.all(got[:, 47:] == -1.0)
    monkeypatch.delenv('PVHIP_CONV_F16_SPAN', raising=False)
    dev.reload_settings()


def test_conv_f16_span_kernel_vs_oracle_and_the_other_f16_kernels(hip, monkeypatch):
    """pvhip_conv2d_f16_span (FP16 IRs: stride-1 "same" 1x1 / 3x3 / 5x5 windows, C % 16 == 0: one LDS span per channel and stage serves
    every tap and up to 256 output channels) against the oracle on fp16-ROUNDED operands (1e-5) and against the LDS-DMA form
    (PVHIP_CONV_F16_SPAN=0).  GoogLeNet's extents (56, 28, 14, 7), H*W that is not a multiple of 4 (dword copies) or of 128 (a tile's
    tail), several tiles per image, output channels below / between / above whole tiles and above one channel group (> 256), one
    and several stages, odd and even stage counts; bias + ReLU fused into a wider tensor."""
    from pyopenvino_amd import device as dev
    cases = [((2, 16, 12, 12), 40, 3), ((3, 64, 14, 14), 96, 1), ((2, 32, 7, 7), 16, 1), ((2, 48, 7, 7), 128, 5),
             ((1, 64, 56, 56), 192, 3), ((2, 96, 28, 28), 128, 3), ((2, 16, 28, 28), 32, 5), ((1, 160, 14, 14), 320, 3),
             ((2, 192, 7, 7), 384, 3), ((1, 16, 9, 5), 33, 3), ((1, 32, 14, 14), 208, 3), ((3, 16, 13, 13), 7, 5),
             ((1, 32, 20, 61), 24, 3), ((2, 16, 3, 3), 300, 3)]
    for xs, k, kk in cases:
        pad = (kk - 1) // 2
        x, w = rnd(sum(xs), xs), rnd(k, (k, xs[1], kk, kk), (2.0 / (xs[1] * kk * kk)) ** 0.5)
        assert dev.call('pvhip_conv2d_f16_span_supported', xs[1], xs[2], xs[3], kk, kk, 1, 1, pad, pad, xs[2], xs[3]), (xs, kk)
        outs = {}
        for mode in ('2', '0'):       # 2: the 1x1 layers too (by default they stay on the LDS-DMA form, which is faster there)
            helpers.setenv(monkeypatch, 'PVHIP_CONV_F16_SPAN', mode)
            dev.reload_settings()
            node = make_node('Convolution', [x, w], conv_data((1, 1), (pad, pad), (pad, pad)))
            node['_f16_mfma'] = True
            outs[mode] = np.asarray(first_out(hip_plugin('Convolution').compute(node, {0: x, 1: w})))
            assert node['_hip_f16'] == ('span' if mode == '2' else 'lds-dma')
        want = first_out(oracle_plugin('Convolution').compute(make_node('Convolution', [x, w], conv_data((1, 1), (pad, pad), (pad, pad))),
                                                              {0: f16r(x), 1: f16r(w)}, kernel_type='special'))
        assert_close(outs['2'], want, 1e-5, 'f16 span kernel {} k{} {}x{}'.format(xs, k, kk, kk))
        assert_close(outs['2'], outs['0'], 1e-5, 'f16 span kernel vs the LDS-DMA form {} k{}'.format(xs, k))
    monkeypatch.delenv('PVHIP_CONV_F16_SPAN', raising=False)
    dev.reload_settings()
    for c, h, w_, kk, st, pad, oh, ow in [(3, 8, 8, 3, 1, 1, 8, 8), (16, 8, 8, 3, 2, 1, 4, 4), (16, 8, 8, 3, 1, 0, 6, 6), (16, 8, 8, 7, 1, 3, 8, 8),
                                          (16, 8, 70, 3, 1, 1, 8, 70), (16, 8, 40, 5, 1, 2, 8, 40)]:
        assert not dev.call('pvhip_conv2d_f16_span_supported', c, h, w_, kk, kk, st, st, pad, pad, oh, ow), (c, h, w_, kk, st, pad)
    x, w, b = np.abs(rnd(1, (2, 32, 10, 6))), rnd(2, (40, 32, 3, 3), 0.1), rnd(3, (1, 40, 1, 1), 0.3)
    node = make_node('Convolution', [x, w], conv_data((1, 1), (1, 1), (1, 1)))
    node['_f16_mfma'] = True
    wide = dev.DeviceTensor.from_numpy(np.full((2, 50, 10, 6), -1.0, dtype=np.float32))
    fused = dict(node)
    fused['_fuse_bias'], fused['_fuse_act'], fused['_out_into'] = dev.DeviceTensor.from_numpy(b), ('relu',), (wide, 7)
    hip_plugin('Convolution').compute(fused, {0: x, 1: w})
    assert fused['_hip_f16'] == 'span'
    got = np.asarray(wide)
    unfused = first_out(hip_plugin('Convolution').compute(dict(node), {0: x, 1: w}))
    assert_bit_exact(got[:, 7:47], np.maximum(unfused + b, 0).astype(np.float32), 'f16 span kernel: fused epilogue')
    assert np.all(got[:, :7] == -1.0) and np.all(got[:, 47:] == -1.0)


@pytest.mark.parametrize('xs,ks', [((3, 192, 28, 28), (64, 96, 16)), ((2, 512, 14, 14), (160, 112, 24)), ((5, 832, 7, 7), (384, 192, 48))])
def test_f16_sibling_launch_and_pooled_launch_match_their_single_launches(hip, xs, ks):
    """FP16 IRs: the 1x1 convolutions of an inception module as ONE launch of the f16 LDS-DMA form (pvhip_conv2d_multi_f16_dma) and
    MaxPool + pool_proj as one launch (pvhip_conv2d_pooled_f16): the same operands rounded the same way, the same (r,s)-major order --
    1e-5 from each member's own launch and from the oracle on fp16-rounded operands (the bits may differ: another channel tile)."""
    from pyopenvino_amd import device as dev
    plugin, pool = hip_plugin('Convolution'), hip_plugin('MaxPool')
    x = rnd(11, xs)
    data = conv_data((1, 1), (0, 0), (0, 0))
    ws = [rnd(20 + i, (k, xs[1], 1, 1), (2.0 / xs[1]) ** 0.5) for i, k in enumerate(ks)]
    bs = [rnd(40 + i, (1, k, 1, 1), 0.1) for i, k in enumerate(ks)]
    nodes = [make_node('Convolution', [x, w], data) for w in ws]
    alone = []
    for node, w, b in zip(nodes, ws, bs):
        nd = dict(node)
        nd['_f16_mfma'], nd['_fuse_bias'], nd['_fuse_act'] = True, dev.DeviceTensor.from_numpy(b), ('relu',)
        alone.append(np.asarray(first_out(plugin.compute(nd, {0: x, 1: w}))))
        want = np.maximum(first_out(oracle_plugin('Convolution').compute(node, {0: f16r(x), 1: f16r(w)}, kernel_type='special')) + b, 0)
        assert_close(alone[-1], want, 1e-5, 'f16 conv {}'.format(w.shape))
    wide = dev.DeviceTensor.from_numpy(np.full((xs[0], ks[0] + 7, xs[2], xs[3]), -1.0, dtype=np.float32))
    lead = dict(nodes[0])
    lead['_f16_mfma'], lead['_fuse_bias'], lead['_fuse_act'], lead['_out_into'] = True, dev.DeviceTensor.from_numpy(bs[0]), ('relu',), (wide, 3)
    lead['_siblings'] = [{'node': n_, 'inputs': {0: x, 1: w}, 'bias': dev.DeviceTensor.from_numpy(b), 'into': None}
                         for n_, w, b in zip(nodes[1:], ws[1:], bs[1:])]
    plugin.compute(lead, {0: x, 1: ws[0]})
    assert lead['_hip_f16'] == 'lds-dma, siblings'
    got = [np.asarray(wide)[:, 3:3 + ks[0]]] + [np.asarray(t) for t in lead['_sibling_out']]
    for g, a_, k in zip(got, alone, ks):
        assert_close(np.ascontiguousarray(g), a_, 1e-5, 'f16 sibling with {} channels'.format(k))
    rest = np.asarray(wide)
    assert np.all(rest[:, :3] == -1.0) and np.all(rest[:, 3 + ks[0]:] == -1.0)
    if xs[3] % 2 == 0:                       # MaxPool + pool_proj (even widths): against MaxPool, then the f16 convolution
        k = ks[2] if ks[2] <= 128 else 64
        w, b = ws[2][:k], bs[2][:, :k]
        pnode = make_node('MaxPool', [x], pool_data((3, 3), (1, 1), (1, 1), (1, 1), 'ceil'))
        pnode['output'][1]['dims'] = tuple(xs)
        cnode = make_node('Convolution', [x, w], data)
        assert plugin.pooled_fusable(cnode, pnode)
        pooled = pool.compute(pnode, {0: x})[1]
        two = dict(cnode)
        two['_f16_mfma'], two['_fuse_bias'], two['_fuse_act'] = True, dev.DeviceTensor.from_numpy(b), ('relu',)
        want = np.asarray(first_out(plugin.compute(two, {0: pooled, 1: w})))
        one = dict(two)
        one['_fuse_pool_in'] = pnode
        got1 = np.asarray(first_out(plugin.compute(one, {0: x, 1: w})))
        assert one['_hip_f16'] == 'MaxPool + 1x1'
        assert_close(got1, want, 1e-5, 'f16 MaxPool + 1x1 {} k{}'.format(xs, k))


def test_conv_f16_c8_blocked_fp16_tensors_between_two_convolutions(hip):
    """FP16 IRs, ABI v14: the first fp16 TENSORS in HBM.  (1) dev.BlockedHalf (fp16, channels blocked by eight, pvhip_c8_f16_*): the
    round trip gives exactly the fp16 rounding of the fp32 tensor, channel counts that are not multiples of 8 or 16 included.
    (2) pvhip_conv2d_f16_c8 reads such a tensor: against the oracle on the SAME operands rounded to fp16 (1e-5: only the fp32 summation
    order differs) and against the span kernel on the dense tensor; GoogLeNet's 3x3 / 5x5 layers (56, 28, 14, 7 wide), a 1x1, rows
    that do not fill a 32-pixel block, images taller than one tile, channel counts that need zero-padded stages (24, 40), output
    channels below / between / above whole tiles and above one 128-channel group; bias + ReLU fused into a wider tensor.
    (3) the writer: a member of the f16 sibling launch with layout = 1 stores the fp16 rounding of what it stores as fp32 NCHW."""
    from pyopenvino_amd import device as dev
    for xs in [(2, 24, 5, 7), (1, 16, 3, 3), (3, 13, 4, 6), (2, 40, 14, 14)]:
        x = rnd(sum(xs), xs)
        blocked = dev.BlockedHalf.from_dense(dev.DeviceTensor.from_numpy(x))
        assert blocked.shape == xs and blocked.dtype == np.float32
        assert_bit_exact(np.asarray(blocked), f16r(x), 'c8 round trip {}'.format(xs))
    cases = [((1, 64, 56, 56), 192, 3), ((2, 96, 28, 28), 128, 3), ((2, 16, 28, 28), 32, 5), ((1, 160, 14, 14), 320, 3), ((2, 192, 7, 7), 384, 3),
             ((2, 48, 7, 7), 128, 5), ((2, 24, 14, 14), 64, 5), ((1, 32, 14, 14), 208, 3), ((3, 16, 13, 13), 7, 5), ((1, 40, 9, 5), 33, 3),
             ((1, 32, 20, 60), 24, 3), ((2, 16, 3, 3), 300, 3), ((2, 64, 14, 14), 96, 1), ((1, 16, 40, 56), 40, 5), ((5, 32, 1, 9), 16, 3)]
    for xs, k, kk in cases:
        pad = (kk - 1) // 2
        x, w = rnd(sum(xs), xs), rnd(k, (k, xs[1], kk, kk), (2.0 / (xs[1] * kk * kk)) ** 0.5)
        assert dev.call('pvhip_conv2d_f16_c8_supported', xs[1], xs[2], xs[3], kk, kk, 1, 1, pad, pad, xs[2], xs[3]), (xs, kk)
        node = make_node('Convolution', [x, w], conv_data((1, 1), (pad, pad), (pad, pad)))
        node['_f16_mfma'] = True
        blocked = dev.BlockedHalf.from_dense(dev.DeviceTensor.from_numpy(x))
        got = np.asarray(first_out(hip_plugin('Convolution').compute(node, {0: blocked, 1: w})))
        assert node['_hip_f16'] == 'c8'
        want = first_out(oracle_plugin('Convolution').compute(make_node('Convolution', [x, w], conv_data((1, 1), (pad, pad), (pad, pad))),
                                                              {0: f16r(x), 1: f16r(w)}, kernel_type='special'))
        assert_close(got, want, 1e-5, 'f16 c8 kernel {} k{} {}x{}'.format(xs, k, kk, kk))
        dense = dict(make_node('Convolution', [x, w], conv_data((1, 1), (pad, pad), (pad, pad))))
        dense['_f16_mfma'] = True
        assert_close(got, np.asarray(first_out(hip_plugin('Convolution').compute(dense, {0: x, 1: w}))), 1e-5, 'c8 vs the dense f16 kernels {}'.format(xs))
    for c, h, w_, kk, st, pad, oh, ow in [(16, 8, 8, 3, 2, 1, 4, 4), (16, 8, 8, 3, 1, 0, 6, 6), (16, 8, 8, 7, 1, 3, 8, 8), (16, 8, 63, 3, 1, 1, 8, 63),
                                          (16, 8, 61, 5, 1, 2, 8, 61)]:
        assert not dev.call('pvhip_conv2d_f16_c8_supported', c, h, w_, kk, kk, st, st, pad, pad, oh, ow), (c, h, w_, kk, st, pad)
    # a reader the kernel does not cover gets the dense tensor (the values are the same fp16 values)
    x, w = rnd(5, (1, 16, 8, 8)), rnd(6, (8, 16, 3, 3), 0.1)
    node = make_node('Convolution', [x, w], conv_data((2, 2), (1, 1), (1, 1)))
    node['_f16_mfma'] = True
    blocked = dev.BlockedHalf.from_dense(dev.DeviceTensor.from_numpy(x))
    got = np.asarray(first_out(hip_plugin('Convolution').compute(node, {0: blocked, 1: w})))
    assert node['_hip_f16'] != 'c8'
    want = first_out(oracle_plugin('Convolution').compute(make_node('Convolution', [x, w], conv_data((2, 2), (1, 1), (1, 1))), {0: f16r(x), 1: f16r(w)},
                                                          kernel_type='special'))
    assert_close(got, want, 1e-5, 'dense fallback')
    # fused epilogue, written in place into a wider tensor
    x, w, b = np.abs(rnd(1, (2, 32, 10, 6))), rnd(2, (40, 32, 3, 3), 0.1), rnd(3, (1, 40, 1, 1), 0.3)
    node = make_node('Convolution', [x, w], conv_data((1, 1), (1, 1), (1, 1)))
    node['_f16_mfma'] = True
    blocked = dev.BlockedHalf.from_dense(dev.DeviceTensor.from_numpy(x))
    wide = dev.DeviceTensor.from_numpy(np.full((2, 50, 10, 6), -1.0, dtype=np.float32))
    fused = dict(node)
    fused['_fuse_bias'], fused['_fuse_act'], fused['_out_into'] = dev.DeviceTensor.from_numpy(b), ('relu',), (wide, 7)
    hip_plugin('Convolution').compute(fused, {0: blocked, 1: w})
    assert fused['_hip_f16'] == 'c8'
    got = np.asarray(wide)
    unfused = np.asarray(first_out(hip_plugin('Convolution').compute(dict(node), {0: blocked, 1: w})))
    assert_bit_exact(got[:, 7:47], np.maximum(unfused + b, 0).astype(np.float32), 'f16 c8 kernel: fused epilogue')
    assert np.all(got[:, :7] == -1.0) and np.all(got[:, 47:] == -1.0)
    # the writer: the sibling launch with one and with several members, blocked and dense destinations side by side
    for xs, ks, c8 in [((3, 192, 28, 28), (64, 96, 16), (False, True, True)), ((2, 512, 14, 14), (160, 112, 24), (False, True, True)),
                       ((5, 832, 7, 7), (48,), (True,)), ((2, 64, 56, 56), (64,), (True,)), ((1, 32, 6, 10), (40, 8), (True, True))]:
        x = rnd(11, xs)
        data = conv_data((1, 1), (0, 0), (0, 0))
        ws = [rnd(20 + i, (k, xs[1], 1, 1), (2.0 / xs[1]) ** 0.5) for i, k in enumerate(ks)]
        bs = [rnd(40 + i, (1, k, 1, 1), 0.1) for i, k in enumerate(ks)]
        nodes = [make_node('Convolution', [x, w], data) for w in ws]
        outs = {}
        for blocked_run in (False, True):
            lead = dict(nodes[0])
            lead['_f16_mfma'], lead['_fuse_bias'], lead['_fuse_act'] = True, dev.DeviceTensor.from_numpy(bs[0]), ('relu',)
            lead['_out_c8'] = blocked_run and c8[0]
            lead['_siblings'] = [{'node': n_, 'inputs': {0: x, 1: w}, 'bias': dev.DeviceTensor.from_numpy(b), 'into': None, 'c8': blocked_run and f}
                                 for n_, w, b, f in zip(nodes[1:], ws[1:], bs[1:], c8[1:])]
            y = next(iter(hip_plugin('Convolution').compute(lead, {0: x, 1: ws[0]}).values()))
            res = [y] + list(lead.get('_sibling_out', []))
            for t, f in zip(res, c8):
                assert isinstance(t, dev.BlockedHalf) == bool(blocked_run and f)
            outs[blocked_run] = [np.asarray(t) for t in res]
        for dense_out, blocked_out, k, f in zip(outs[False], outs[True], ks, c8):
            assert dense_out.shape == blocked_out.shape == (xs[0], k, xs[2], xs[3])
            assert_bit_exact(blocked_out, f16r(dense_out) if f else dense_out, 'sibling member with {} channels, c8 {}'.format(k, f))


def test_conv_f16_c8_module_form_blocked_in_blocked_out(hip):
    """FP16 IRs, second step: pvhip_conv2d_f16_c8_multi reads AND writes fp16 blocked by eight channels.  Each output against the oracle
    on fp16-rounded operands, rounded to fp16 where the destination is blocked (2e-3: one fp16 rounding of a 1e-5-accurate value), 1e-5
    where it is fp32: (1) the 1x1 arms of a module as one launch -- a range of a blocked Concat buffer, blocked tensors of their own
    (channel counts that are not multiples of 16 or 32), an fp32 tensor beside them; (2) 3x3 / 5x5 into a blocked Concat range; (3) MaxPool
    3x3 / 1 / 1 + 1x1 (odd widths too) against the MaxPool plugin followed by the convolution; channel counts whose last stage of four
    16-channel steps is partly empty (480, 528); (4) pvhip_maxpool3x3_c8 against the MaxPool plugin: strides, ceil / floor, padding, NaN."""
    from pyopenvino_amd import device as dev
    plugin, pool = hip_plugin('Convolution'), hip_plugin('MaxPool')

    def oracle_conv(x, w, b, pad):
        node = make_node('Convolution', [x, w], conv_data((1, 1), (pad, pad), (pad, pad)))
        return np.maximum(first_out(oracle_plugin('Convolution').compute(node, {0: f16r(x), 1: f16r(w)}, kernel_type='special')) + b, 0).astype(np.float32)

    # (1) several 1x1 members
    for xs, ks in [((3, 192, 28, 28), (64, 96, 16)), ((2, 480, 14, 14), (192, 96, 16)), ((2, 528, 14, 14), (256, 160, 32)), ((5, 832, 7, 7), (384, 192, 48)),
                   ((1, 64, 56, 56), (64,)), ((2, 40, 6, 10), (24, 8, 40))]:
        x = rnd(11, xs)
        xb = dev.BlockedHalf.from_dense(dev.DeviceTensor.from_numpy(x))
        ws = [rnd(20 + i, (k, xs[1], 1, 1), (2.0 / xs[1]) ** 0.5) for i, k in enumerate(ks)]
        bs = [rnd(40 + i, (1, k, 1, 1), 0.1) for i, k in enumerate(ks)]
        ctot = -(-(ks[0] + 24) // 16) * 16
        cat = dev.BlockedHalf((xs[0], ctot, xs[2], xs[3]))
        dev.call('pvhip_memset', ctypes.c_void_p(cat.ptr), 0, cat.buf.nbytes)
        # the first member: a range of a blocked Concat buffer; the second: a blocked tensor of its own; the third: an fp32 tensor of its own
        members = [(dev.DeviceTensor.from_numpy(ws[i]), dev.DeviceTensor.from_numpy(bs[i]), (cat, 8) if i == 0 else None, i == 1) for i in range(len(ks))]
        node = {}
        outs = plugin.launch_c8_multi(node, xb, members, act=('relu',))
        assert 'c8 module' in node['_hip_f16']
        got_cat = np.asarray(cat)
        assert np.all(got_cat[:, :8] == 0) and np.all(got_cat[:, 8 + ks[0]:] == 0)
        for i, (o, w, b) in enumerate(zip(outs, ws, bs)):
            want = oracle_conv(x, w, b, 0)
            blocked_out = isinstance(o, (dev.BlockedHalf, dev.BlockedChannelSlice))
            assert blocked_out == (i < 2)
            got = np.asarray(o)
            assert got.shape == want.shape
            if blocked_out:
                assert_bit_exact(got, f16r(got), 'a blocked output holds fp16 values')
                assert_close(got, want, 2e-3, 'module form, 1x1 member {} of {} {}'.format(i, xs, ks), elementwise=False)
            else:
                assert_close(got, want, 1e-5, 'module form, fp32 member {} of {} {}'.format(i, xs, ks))
    # (2) windows into a blocked Concat range, (3) the pooled 1x1
    for xs, k, kk, pooled in [((2, 96, 28, 28), 128, 3, False), ((1, 64, 56, 56), 192, 3, False), ((2, 16, 28, 28), 32, 5, False), ((2, 24, 14, 14), 64, 5, False),
                              ((2, 192, 7, 7), 384, 3, False), ((1, 160, 14, 14), 320, 3, False), ((3, 192, 28, 28), 32, 1, True), ((2, 480, 14, 14), 64, 1, True),
                              ((2, 832, 7, 7), 128, 1, True), ((1, 48, 5, 9), 24, 1, True)]:
        pad = (kk - 1) // 2
        x = rnd(7, xs)
        xb = dev.BlockedHalf.from_dense(dev.DeviceTensor.from_numpy(x))
        w, b = rnd(k, (k, xs[1], kk, kk), (2.0 / (xs[1] * kk * kk)) ** 0.5), rnd(3, (1, k, 1, 1), 0.1)
        cat = dev.BlockedHalf((xs[0], k + 24, xs[2], xs[3])) if (k + 24) % 16 == 0 else dev.BlockedHalf((xs[0], k + 32, xs[2], xs[3]))
        dev.call('pvhip_memset', ctypes.c_void_p(cat.ptr), 0, cat.buf.nbytes)
        node = {}
        (o,) = plugin.launch_c8_multi(node, xb, [(dev.DeviceTensor.from_numpy(w), dev.DeviceTensor.from_numpy(b), (cat, 16), False)], pool=pooled, act=('relu',))
        src = f16r(x)
        if pooled:
            pnode = make_node('MaxPool', [src], pool_data((3, 3), (1, 1), (1, 1), (1, 1), 'ceil'))
            pnode['output'][1]['dims'] = tuple(xs)
            src = np.asarray(pool.compute(pnode, {0: src})[1])
        want = oracle_conv(src, w, b, pad)
        got = np.asarray(cat)
        assert np.all(got[:, :16] == 0) and np.all(got[:, 16 + k:] == 0)
        assert_close(np.ascontiguousarray(got[:, 16:16 + k]), want, 2e-3, 'module form {} k{} {}x{} pooled {}'.format(xs, k, kk, kk, pooled), elementwise=False)
        assert_bit_exact(np.asarray(o), np.ascontiguousarray(got[:, 16:16 + k]), 'the slice object')
    # (4) MaxPool on blocked tensors
    for xs, st, pb, pe, rounding in [((2, 40, 28, 28), (2, 2), (0, 0), (0, 0), 'ceil'), ((1, 16, 14, 14), (2, 2), (0, 0), (0, 0), 'ceil'), ((2, 24, 7, 7), (1, 1), (1, 1), (1, 1), 'ceil'),
                                     ((1, 8, 9, 12), (2, 3), (1, 0), (0, 2), 'floor'), ((1, 16, 6, 6), (2, 2), (1, 1), (1, 1), 'ceil')]:
        x = f16r(rnd(5, xs))
        if xs[1] == 24:
            x[0, 3, 2, 2], x[1, 5, 0, 6] = np.nan, -np.nan
        pnode = make_node('MaxPool', [x], pool_data((3, 3), st, pb, pe, rounding))
        want = np.asarray(pool.compute(dict(pnode), {0: x})[1])
        pnode['output'][1]['dims'] = want.shape
        got = pool.compute(dict(pnode), {0: dev.BlockedHalf.from_dense(dev.DeviceTensor.from_numpy(x))})[1]
        assert isinstance(got, dev.BlockedHalf) and got.shape == want.shape
        assert_bit_exact(np.asarray(got), want, 'MaxPool on a blocked tensor {} stride {} pads {} {} {}'.format(xs, st, pb, pe, rounding))


def test_f16_fragment_panel_bits(hip):
    """The 16-byte weight-fragment panel the span, c8 and c8-module kernels read (csrc/pvhip_f16_c8.h) is ref64.f16_fragments bit for bit:
    pvhip_conv2d_f16_c8_pack -- and pvhip_conv2d_f16_span_pack where C is whole 16-channel stages -- into a block of 0xFF bytes, the
    words behind the panel untouched, *_pack_elems the panel's size.  One group with a ragged second tile; two groups of tm = 3 with
    panel rows 130 .. 191 empty; C padded to 32; 33 channels in two tiles."""
    from pyopenvino_amd import device as dev
    guard = 16
    for k, c, ks in [(40, 16, 1), (130, 32, 3), (200, 24, 5), (33, 48, 3)]:
        w = rnd(k + c, (k, c, ks, ks), 0.5)
        want = ref64.f16_fragments(w)
        nm, tm = (k + 127) // 128, -(-(-(-k // 32)) // ((k + 127) // 128))
        assert want.shape == (nm, (c + 15) // 16, ks * ks, tm, 64, 8)
        wd = dev.DeviceTensor.from_numpy(w)
        for entry in ('c8', 'span') if c % 16 == 0 else ('c8',):
            elems = int(dev.call('pvhip_conv2d_f16_{}_pack_elems'.format(entry), k, c, ks, ks))
            assert elems * 2 == want.size, (entry, k, c, ks)
            block = dev.DeviceTensor.from_numpy(np.full(elems + guard, 0xFFFFFFFF, dtype=np.uint32))
            dev.call('pvhip_conv2d_f16_{}_pack'.format(entry), dev.ptr(wd), dev.ptr(block), k, c, ks, ks)
            got = np.asarray(block)
            assert np.all(got[elems:] == 0xFFFFFFFF), 'pvhip_conv2d_f16_{}_pack wrote past its panel'.format(entry)
            assert np.array_equal(got[:elems].view(np.uint16), want.reshape(-1).view(np.uint16)), \
                'pvhip_conv2d_f16_{}_pack: fragment panel of K {} C {} {}x{}'.format(entry, k, c, ks, ks)
    assert dev.call('pvhip_conv2d_f16_span_pack_elems', 200, 24, 5, 5) == 0          # (the span entries take whole stages only)


def test_f16_c8_row_tile_plan_corners(hip):
    """pvhip_conv2d_f16_c8 and pvhip_conv2d_f16_c8_multi (one fp32 destination) on the same blocked input, each against the oracle on
    fp16-rounded operands (1e-5, as test_conv_f16_c8_blocked_fp16_tensors_between_two_convolutions), where their row-tile plans differ or
    sit on a boundary: tiles that c8's cap of ten LDS rows cuts and the module form's does not; rows of w + 2 pad = 64 pixels, the widest;
    R * w = 65 and 64, the first plan of four pixel blocks and the last of two.  Rows of 65 stay unsupported."""
    from pyopenvino_amd import device as dev
    plugin = hip_plugin('Convolution')
    k = 40
    for xs, kk in [((2, 16, 20, 6), 3), ((2, 16, 20, 6), 5), ((1, 16, 9, 60), 5), ((1, 16, 3, 62), 3), ((2, 16, 5, 13), 3), ((2, 16, 4, 16), 3)]:
        pad = (kk - 1) // 2
        x, w = rnd(sum(xs), xs), rnd(k + kk, (k, xs[1], kk, kk), (2.0 / (xs[1] * kk * kk)) ** 0.5)
        assert dev.call('pvhip_conv2d_f16_c8_supported', xs[1], xs[2], xs[3], kk, kk, 1, 1, pad, pad, xs[2], xs[3]), (xs, kk)
        assert dev.call('pvhip_conv2d_f16_c8_multi_supported', xs[1], xs[2], xs[3], kk, kk, 0, 1), (xs, kk)
        want = first_out(oracle_plugin('Convolution').compute(make_node('Convolution', [x, w], conv_data((1, 1), (pad, pad), (pad, pad))),
                                                              {0: f16r(x), 1: f16r(w)}, kernel_type='special'))
        xb = dev.BlockedHalf.from_dense(dev.DeviceTensor.from_numpy(x))
        wd = dev.DeviceTensor.from_numpy(w)
        node = {}
        got = np.asarray(plugin.launch_c8(node, xb, wd))
        assert node['_hip_f16'] == 'c8'
        assert_close(got, want, 1e-5, 'pvhip_conv2d_f16_c8 {} {}x{}'.format(xs, kk, kk))
        node = {}
        (o,) = plugin.launch_c8_multi(node, xb, [(wd, None, None, False)])
        assert 'c8 module' in node['_hip_f16'] and isinstance(o, dev.DeviceTensor)
        assert_close(np.asarray(o), want, 1e-5, 'pvhip_conv2d_f16_c8_multi {} {}x{}'.format(xs, kk, kk))
    for h, w_, kk in [(8, 63, 3), (8, 61, 5)]:                                       # w + 2 pad = 65
        pad = (kk - 1) // 2
        assert not dev.call('pvhip_conv2d_f16_c8_supported', 16, h, w_, kk, kk, 1, 1, pad, pad, h, w_), (w_, kk)
        assert not dev.call('pvhip_conv2d_f16_c8_multi_supported', 16, h, w_, kk, kk, 0, 1), (w_, kk)
    assert not dev.call('pvhip_conv2d_f16_c8_multi_supported', 16, 8, 63, 1, 1, 1, 1)       # (the pooled 1x1 copies a halo of one)


def test_fp16_stem_on_blocked_tensors(hip):
    """FP16 IRs: (1) a convolution on the f16 form of the LDS-DMA kernel stores its output as fp16 blocked by eight channels
    (pvhip_conv2d_f16_dma_c8: node['_out_c8'] on a layer the 1x1 launch does not cover -- GoogLeNet's conv1, through the padding pass with
    the per-channel constant): exactly the fp16 rounding of what the same launch stores as fp32; (2) MaxPool 3x3 + LRN on a blocked tensor
    as one launch (pvhip_maxpool3x3_lrn_c8) against the fp32 launch on the same fp16 values: one fp16 rounding of the output (1e-3),
    channel counts that are not multiples of 8 or 16, strides, padding, ceil / floor, a NaN."""
    from pyopenvino_amd import device as dev
    plugin, pool = hip_plugin('Convolution'), hip_plugin('MaxPool')
    # (0) the row-span kernel (pvhip_conv2d_f16_stem: 7x7 / 2 / pad 3 over three channels, blocked output) against the oracle on fp16-rounded
    # operands: GoogLeNet's conv1 at its own size, odd and small extents (a last tile of one row, rows that do not fill a pixel block),
    # 64 / 40 / 24 output channels, with and without the folded per-channel constant
    assert not dev.call('pvhip_conv2d_f16_stem_supported', 3, 9, 252, 64, 7, 7, 2, 2, 3, 3, 5, 126)          # (a padded row of more than 256 floats)
    assert not dev.call('pvhip_conv2d_f16_stem_supported', 4, 30, 30, 64, 7, 7, 2, 2, 3, 3, 15, 15) and not dev.call('pvhip_conv2d_f16_stem_supported', 3, 30, 30, 96, 7, 7, 2, 2, 3, 3, 15, 15)
    for xs, k, add in [((2, 3, 224, 224), 64, True), ((1, 3, 37, 41), 40, False), ((3, 3, 30, 18), 24, True), ((1, 3, 9, 250), 64, False),
                       ((2, 3, 20, 24), 24, True), ((1, 3, 12, 248), 64, False)]:
        x, w, b = np.round(rnd(sum(xs), xs, 60.0)), rnd(k, (k, 3, 7, 7), (2.0 / 147) ** 0.5), rnd(3, (1, k, 1, 1), 0.2)
        mean = np.array([-104.0, -117.0, -123.0], dtype=np.float32).reshape(1, 3, 1, 1)
        node = make_node('Convolution', [x, w], conv_data((2, 2), (3, 3), (3, 3)))
        node['_f16_mfma'], node['_fuse_bias'], node['_fuse_act'], node['_out_c8'] = True, dev.DeviceTensor.from_numpy(b), ('relu',), True
        if add:
            node['_pre_add'] = dev.DeviceTensor.from_numpy(mean)
        y = next(iter(plugin.compute(node, {0: x, 1: w}).values()))
        assert isinstance(y, dev.BlockedHalf) and node['_hip_f16'] == 'row spans, blocked output', node['_hip_f16']
        xin = (x + mean).astype(np.float32) if add else x
        want = np.maximum(first_out(oracle_plugin('Convolution').compute(make_node('Convolution', [xin, w], conv_data((2, 2), (3, 3), (3, 3))),
                                                                        {0: f16r(xin), 1: f16r(w)}, kernel_type='special')) + b, 0).astype(np.float32)
        got = np.asarray(y)
        assert_bit_exact(got, f16r(got), 'a blocked output holds fp16 values')
        assert_close(got, want, 2e-3, 'row-span conv1 {} k{}'.format(xs, k), elementwise=False)
        if xs[3] % 4 == 0 and xs[3] <= 248:
            # rows of a multiple of four pixels were read straight from the image (pvhip_conv2d_f16_stem_direct, round 5: no padding pass, the Add
            # applied in LDS): the bits of the padding pass + the kernel on the padded copy
            os.environ['PVHIP_CONV_STEM_DIRECT'] = '0'
            dev.reload_settings()
            try:
                y0 = next(iter(plugin.compute(dict(node), {0: x, 1: w}).values()))
            finally:
                del os.environ['PVHIP_CONV_STEM_DIRECT']
                dev.reload_settings()
            assert_bit_exact(got, np.asarray(y0), 'row-span conv1 straight from the image vs from the padded copy {} k{}'.format(xs, k))
    for xs, k, kk, st, pb, pe in [((2, 3, 37, 37), 64, 7, (2, 2), (3, 3), (3, 3)), ((1, 20, 13, 11), 24, 3, (1, 1), (1, 1), (1, 1)), ((2, 32, 9, 9), 40, 3, (2, 2), (0, 0), (1, 1))]:
        x, w, b = rnd(sum(xs), xs), rnd(k, (k, xs[1], kk, kk), (2.0 / (xs[1] * kk * kk)) ** 0.5), rnd(3, (1, k, 1, 1), 0.2)
        outs = {}
        os.environ['PVHIP_CONV_F16_STEM'] = '0'          # (this part: the f16 form of the LDS-DMA kernel)
        dev.reload_settings()
        for blocked in (False, True):
            node = make_node('Convolution', [x, w], conv_data(st, pb, pe))
            node['_f16_mfma'], node['_fuse_bias'], node['_fuse_act'], node['_out_c8'] = True, dev.DeviceTensor.from_numpy(b), ('relu',), blocked
            if xs[1] == 3:
                node['_pre_add'] = dev.DeviceTensor.from_numpy(np.array([-104.0, -117.0, -123.0], dtype=np.float32).reshape(1, 3, 1, 1))
            y = next(iter(plugin.compute(node, {0: x, 1: w}).values()))
            assert isinstance(y, dev.BlockedHalf) == blocked, node.get('_hip_f16')
            outs[blocked] = np.asarray(y)
        assert_bit_exact(outs[True], f16r(outs[False]), 'blocked output of the f16 LDS-DMA form {} k{}'.format(xs, k))
        del os.environ['PVHIP_CONV_F16_STEM']
        dev.reload_settings()
    lrn_data = {'alpha': '9.9999997473787516e-05', 'beta': '0.75', 'bias': '1', 'size': '5'}
    axes = np.array([1], dtype=np.int64)
    for xs, st, pb, pe, rounding in [((2, 64, 112, 112), (2, 2), (0, 0), (0, 0), 'ceil'), ((1, 20, 13, 11), (2, 2), (0, 0), (0, 0), 'ceil'),
                                     ((3, 8, 9, 20), (1, 1), (1, 1), (1, 1), 'floor'), ((2, 40, 14, 14), (2, 2), (1, 0), (0, 1), 'floor')]:
        x = f16r(rnd(sum(xs), xs, 40.0))
        if xs[1] == 20:
            x[0, 5, 4, 4] = np.nan
        pnode = make_node('MaxPool', [x], pool_data((3, 3), st, pb, pe, rounding))
        pooled = np.asarray(pool.compute(dict(pnode), {0: x})[1])
        lnode = make_node('LRN', [pooled, axes], lrn_data)
        want = np.asarray(hip_plugin('LRN').compute(dict(lnode), {0: pooled, 1: axes})[2])
        fused = dict(pnode)
        fused['output'] = {1: {'precision': 'FP32', 'dims': tuple(want.shape)}}
        fused['_fuse_lrn'] = lnode
        got = pool.compute(fused, {0: dev.BlockedHalf.from_dense(dev.DeviceTensor.from_numpy(x))})[1]
        assert isinstance(got, dev.BlockedHalf) and got.shape == want.shape
        g = np.asarray(got)
        assert np.array_equal(np.isnan(g), np.isnan(want))
        assert_close(np.nan_to_num(g), np.nan_to_num(want), 1e-3, 'MaxPool + LRN on a blocked tensor {}'.format(xs), elementwise=False)
    # (3) the other order: LRN + MaxPool on a blocked tensor (pvhip_lrn_maxpool3x3_c8) against the fp32 launch on the same fp16 values
    for xs, st, pb, pe, rounding in [((2, 192, 56, 56), (2, 2), (0, 0), (0, 0), 'ceil'), ((1, 20, 13, 11), (2, 2), (0, 0), (0, 0), 'ceil'),
                                     ((3, 8, 9, 20), (1, 1), (1, 1), (1, 1), 'floor'), ((2, 40, 14, 14), (2, 2), (1, 0), (0, 1), 'floor'), ((1, 16, 40, 112), (2, 2), (0, 0), (0, 0), 'ceil')]:
        x = f16r(rnd(sum(xs), xs, 40.0))
        if xs[1] == 20:
            x[0, 5, 4, 4] = np.nan
        lnode = make_node('LRN', [x, axes], lrn_data)
        pnode = make_node('MaxPool', [x], pool_data((3, 3), st, pb, pe, rounding))
        normed = np.asarray(hip_plugin('LRN').compute(dict(lnode), {0: x, 1: axes})[2])
        want = np.asarray(pool.compute(dict(pnode), {0: normed})[1])
        pnode['output'][1]['dims'] = tuple(want.shape)
        fused = dict(lnode)
        fused['_fuse_pool'] = pnode
        got = hip_plugin('LRN').compute(fused, {0: dev.BlockedHalf.from_dense(dev.DeviceTensor.from_numpy(x)), 1: axes})[2]
        assert isinstance(got, dev.BlockedHalf) and got.shape == want.shape, (type(got), xs)
        g = np.asarray(got)
        assert np.array_equal(np.isnan(g), np.isnan(want))
        assert_close(np.nan_to_num(g), np.nan_to_num(want), 1e-3, 'LRN + MaxPool on a blocked tensor {}'.format(xs), elementwise=False)


@pytest.mark.parametrize('xs,st,pb,pe,rounding,k_out,act', [
    ((2, 64, 112, 112), (2, 2), (0, 0), (0, 0), 'ceil', 64, ('relu',)),      # GoogLeNet (FP16 IR) pool1/3x3_s2 -> pool1/norm1 -> conv2/3x3_reduce
    ((3, 20, 13, 11), (2, 2), (0, 0), (0, 0), 'ceil', 40, None),             # channels that end inside a block, output channels inside a 32-channel tile
    ((1, 24, 12, 16), (1, 1), (1, 1), (1, 1), 'floor', 8, ('relu',)),
    ((5, 48, 30, 28), (2, 2), (1, 0), (0, 1), 'floor', 33, ('relu',)),
])
def test_fused_maxpool_lrn_conv1x1_on_blocked_tensors(hip, xs, st, pb, pe, rounding, k_out, act):
    """FP16 IRs: MaxPool 3x3 -> LRN -> 1x1 convolution (+ bias, ReLU) on blocked fp16 tensors as ONE launch (pvhip_maxpool3x3_lrn_conv1x1_c8,
    round 5: the eight normalised channels a lane holds are two operands of v_mfma_f32_32x32x4_2b_f16).  Against MaxPool + LRN on the blocked
    tensor followed by the fp32 arithmetic of the convolution on ITS fp16 output (one fp16 rounding of the result: 2e-3), and the blocked output
    holds fp16 values with zeros past k_out."""
    from pyopenvino_amd import device as dev
    pool = hip_plugin('MaxPool')
    x = f16r(rnd(sum(xs), xs, 40.0))
    axes = np.array([1], dtype=np.int64)
    pnode = make_node('MaxPool', [x], pool_data((3, 3), st, pb, pe, rounding))
    pooled = np.asarray(pool.compute(dict(pnode), {0: x})[1])
    lnode = make_node('LRN', [pooled, axes], {'alpha': '9.9999997473787516e-05', 'beta': '0.75', 'bias': '1', 'size': '5'})
    lnode['output'][2]['dims'] = tuple(pooled.shape)
    w = f16r(rnd(7, (k_out, xs[1], 1, 1), (2.0 / xs[1]) ** 0.5))
    bias = rnd(9, (1, k_out, 1, 1))
    cnode = make_node('Convolution', [pooled, w], conv_data((1, 1), (0, 0), (0, 0)))
    assert pool.lrn_conv_fusable(pnode, lnode, cnode, True)
    two = dict(pnode)
    two['output'] = {1: {'precision': 'FP32', 'dims': tuple(pooled.shape)}}
    two['_fuse_lrn'] = lnode
    xb = dev.BlockedHalf.from_dense(dev.DeviceTensor.from_numpy(x))
    normed = pool.compute(dict(two), {0: xb})[1]
    assert isinstance(normed, dev.BlockedHalf)
    want = first_out(oracle_plugin('Convolution').compute(cnode, {0: np.asarray(normed), 1: w}, kernel_type='special')) + bias
    if act is not None:
        want = np.where(want < 0, 0, want)
    fused = dict(two)
    fused['_fuse_conv'] = {'node': cnode, 'w': w, 'bias': dev.DeviceTensor.from_numpy(bias), 'act': act, 'c8': True}
    got = pool.compute(fused, {0: xb})[1]
    assert isinstance(got, dev.BlockedHalf) and got.shape == want.shape
    g = np.asarray(got)
    assert_bit_exact(g, f16r(g), 'a blocked output holds fp16 values')
    assert_close(g, want.astype(np.float32), 2e-3, 'MaxPool + LRN + 1x1 on blocked tensors {}'.format(xs), elementwise=False)
    # a dense input where the plan promised a blocked one is converted, not an error
    g2 = np.asarray(pool.compute(dict(fused), {0: x})[1])
    assert_bit_exact(g2, g, 'dense input converted by the plugin')


def test_avgpool_on_a_blocked_tensor(hip):
    """AvgPool (the reference's window rule: the 7x7 pool averages the top-left 6x6) on fp16 blocked by eight channels, fp32 output holding
    fp16 VALUES (the reference's AvgPool of a float16 tensor returns float16: AvgPool.py:57-58): the fp16 rounding of what the fp32 launch
    gives on the same fp16 values (the same sequential sum, 1e-6 before the rounding)."""
    from pyopenvino_amd import device as dev
    for xs, kern, st in [((3, 1024, 7, 7), (7, 7), (1, 1)), ((2, 20, 9, 12), (3, 3), (2, 2)), ((1, 8, 5, 5), (2, 2), (1, 1))]:
        x = f16r(rnd(sum(xs), xs))
        node = make_node('AvgPool', [x], {'kernel': '{}, {}'.format(*kern), 'strides': '{}, {}'.format(*st), 'pads_begin': '0, 0', 'pads_end': '0, 0',
                                          'rounding_type': 'floor', 'auto_pad': 'valid', 'exclude-pad': 'true'})
        want = first_out(hip_plugin('AvgPool').compute(dict(node), {0: x}))
        node['output'] = {1: {'precision': 'FP32', 'dims': tuple(want.shape)}}
        got = first_out(hip_plugin('AvgPool').compute(dict(node), {0: dev.BlockedHalf.from_dense(dev.DeviceTensor.from_numpy(x))}))
        got = np.asarray(got)
        assert_bit_exact(got, f16r(got), 'AvgPool on a blocked tensor returns fp16 values')
        assert_close(got, f16r(np.asarray(want)), 1e-3, 'AvgPool on a blocked tensor {}'.format(xs), elementwise=False)      # (one fp16 ulp where the two sums round apart)


def test_conv_f16_mfma_reference_fp16_node_fixture(hip):
    """The reference's own FP16 node fixture (resources/node_args_6.pickle, replayed as test_node_sample.py:1-16 does; cropped)
    in float16 as the reference computes it: the f16-MFMA result is within fp16 tolerance of the reference's float16 output
    (which accumulates its 27 products in float16), and 1e-5 from the exact sum of the same fp16 operands."""
    z = np.load(os.path.join(helpers.GOLDEN, 'conv_node6_fp16.npz'))
    x, w, ref = z['x'].astype(np.float32), z['w'].astype(np.float32), z['out'].astype(np.float32)
    import json
    data = json.loads(str(z['data']))
    node = make_node('Convolution', [x, w], data)
    node['_f16_mfma'] = True
    got = first_out(hip_plugin('Convolution').compute(dict(node), {0: x, 1: w}))
    assert got.shape == ref.shape
    err_ref = helpers.rel_err(got, ref)
    exact = first_out(oracle_plugin('Convolution').compute(make_node('Convolution', [x, w], data), {0: x, 1: w}, kernel_type='special'))
    err_exact = assert_close(got, exact, 1e-5, 'f16 conv vs the fp32 sum of the same fp16 operands')
    print('node_args_6 in float16: {:.2e} from the reference float16 output, {:.2e} from the fp32 sum'.format(err_ref, err_exact))
    assert err_ref <= FP16_TOL, err_ref
    assert helpers.rel_err(exact, ref) <= FP16_TOL          # (what separates them is the reference's float16 accumulation)


def test_matmul_f16_mfma(hip):
    """pvhip_matmul_f16 for the four transpose combinations and ragged shapes against float64 on the fp16-rounded operands."""
    for m, n, k in ((64, 10, 64), (3, 70, 130), (256, 1000, 1024), (65, 33, 31)):
        for ta, tb in ((False, True), (False, False), (True, False), (True, True)):
            a = rnd(m + k, (k, m) if ta else (m, k))
            b = rnd(n + k, (n, k) if tb else (k, n), 0.1)
            node = make_node('MatMul', [a, b], {'transpose_a': 'true' if ta else 'false', 'transpose_b': 'true' if tb else 'false'})
            node['_f16_mfma'] = True
            got = first_out(hip_plugin('MatMul').compute(node, {0: a, 1: b}))
            A = f16r(a).astype(np.float64).T if ta else f16r(a).astype(np.float64)
            B = f16r(b).astype(np.float64).T if tb else f16r(b).astype(np.float64)
            assert_close(got, (A @ B).astype(np.float32), 1e-5, 'matmul f16 {}x{}x{} ta={} tb={}'.format(m, n, k, ta, tb))


def test_convolution_input_beyond_32bit_offsets_is_refused_loudly(hip):
    """The convolution kernels address their input with 32-bit byte offsets (out-of-range sentinel 2^31): an input of 2^29 or more
    elements is refused with PVHIP_EUNSUPPORTED before anything is launched -- an error, never a wrapped offset."""
    import ctypes
    one = ctypes.c_void_p(256)                       # never dereferenced: the size check comes first
    for entry in ('pvhip_conv2d_f32', 'pvhip_conv2d_f16'):
        with pytest.raises(hip.PvhipError, match=r'2\^29'):
            hip.call(entry, one, one, one, 2048, 64, 128, 32, 64, 3, 3, 128, 32, 1, 1, 1, 1, ctypes.c_void_p(0), 0, 0, 0, 0.0, 0.0)
    n = ctypes.create_string_buffer(256)
    hip.call('pvhip_device_name', n, 256)
    assert n.value.decode().strip()[0] not in '(', n.value      # a marketing name, or the architecture's, in front of the parenthesis


# ---------------------------------------------------------------------------------------------------------------------
# The nontemporal forms of the streaming kernels at test sizes.  PVHIP_STREAM_NT=2 takes them at any size (by default they start at
# 64 MiB moved, i.e. only on the batch-128 SSD pass); PVHIP_STREAM_WG=1 caps the grid of the runs-of-four kernels (unary_f4_kernel<Op,
# true, 4>, binary_channel4_kernel<..., true, 4>) at kNumCU x 2 = 512 workgroups, so one sweep covers 512 x 4 x 256 float4 (8 MiB) and
# the tensors below make the run loop wrap five to six times, end part-way through a sweep, and leave a float4 tail past the last whole
# run (n4 % 1024 != 0) and, for the unary kernel, a scalar tail (n % 4 != 0).
NT_UNARY = (7, 1519807)                 # n = 10638649: n % 4 = 1, n4 = 2659662 = 2597 runs of 1024 (5 sweeps + 37) + 334
NT_CH4 = (5, 37, 236, 236)              # inner % 4 == 0: binary_channel4_kernel; n4 = 2575940 = 2515 runs (4 sweeps + 467) + 580
NT_FAMILIES = ['unary', 'binary', 'maxpool', 'depthwise']


def _nt_outputs(monkeypatch, capfd, family, mode):
    """({case: (type, inputs, attributes, fused bias, output)}, the pool3 plan lines libpvhip printed) of the family's launches under
    PVHIP_STREAM_NT=mode, PVHIP_STREAM_WG=1."""
    from pyopenvino_amd import device as dev
    helpers.setenv(monkeypatch, 'PVHIP_STREAM_WG', '1')
    helpers.setenv(monkeypatch, 'PVHIP_POOL3_VERBOSE', '1')
    helpers.setenv(monkeypatch, 'PVHIP_STREAM_NT', mode)
    capfd.readouterr()
    out = {}

    def run(case, type_, ins, data=None, bias=None):
        node = make_node(type_, ins, data)
        if bias is not None:                                # depthwise with bias + Clamp 0..6 fused, as every SSD depthwise layer
            node['_fuse_bias'], node['_fuse_act'] = dev.DeviceTensor.from_numpy(bias), ('clamp', 0.0, 6.0)
        out[case] = (type_, ins, data, bias, np.asarray(first_out(hip_plugin(type_).compute(node, dict(enumerate(ins))))))

    if family == 'unary':
        x = rnd(71, NT_UNARY, 3.0)
        run('ReLU', 'ReLU', [x])
        run('Clamp', 'Clamp', [x], {'min': '0', 'max': '6'})
        run('Sigmoid', 'Sigmoid', [x])
    elif family == 'binary':
        a, a2, c = rnd(72, NT_UNARY), rnd(73, NT_UNARY), rnd(74, (1, NT_CH4[1], 1, 1))
        big = rnd(75, NT_CH4)
        bc = {'auto_broadcast': 'numpy'}
        odd, s1 = np.ascontiguousarray(big[:, :, :235, :235]), rnd(76, (1, 1, 1, 1))
        for op in ('Add', 'Multiply'):
            run(op + ' same shape', op, [a, a2], bc)                                    # binary_same_kernel<Op, true>
            run(op + ' per channel', op, [big, c], bc)                                  # binary_channel4_kernel<Op, false, true, 4>
            run(op + ' per channel, odd plane', op, [odd, c], bc)                       # inner % 4 != 0: binary_channel_kernel
            run(op + ' strided', op, [big, rnd(77, (1, NT_CH4[1], 1, NT_CH4[3]))], bc)  # binary_strided_kernel
        # Add broadcasts its second operand only (the reference's rule); Multiply the smaller one, either way round
        run('Multiply per channel, swapped', 'Multiply', [c, big], bc)                  # the broadcast operand first
        run('Add scalar', 'Add', [odd, s1], bc)                                         # SSD's preprocessing: binary_channel_kernel, C = 1
        run('Multiply scalar', 'Multiply', [s1, odd], bc)
    elif family == 'maxpool':
        for xs, st, pb, pe, rounding in (((7, 192, 56, 56), (2, 2), (0, 0), (0, 0), 'ceil'), ((9, 256, 28, 28), (1, 1), (1, 1), (1, 1), 'ceil'),
                                         ((9, 480, 28, 28), (2, 2), (0, 0), (0, 0), 'ceil'), ((5, 832, 14, 14), (1, 1), (1, 1), (1, 1), 'ceil')):
            run('MaxPool {} s{}'.format(xs, st[0]), 'MaxPool', [rnd(sum(xs), xs, 1.0, -0.3)], pool_data((3, 3), st, pb, pe, rounding))
    else:
        for xs, st, pb, pe in (((5, 32, 150, 150), (1, 1), (1, 1), (1, 1)), ((5, 64, 150, 150), (2, 2), (0, 0), (1, 1)),
                               ((7, 128, 75, 75), (2, 2), (1, 1), (1, 1)), ((9, 256, 38, 38), (2, 2), (0, 0), (1, 1)),
                               ((9, 512, 19, 19), (1, 1), (1, 1), (1, 1)), ((7, 1024, 10, 10), (1, 1), (1, 1), (1, 1))):
            x = np.clip(rnd(sum(xs), xs, 3.0, 2.0), 0, 6)
            w, b = rnd(78, (xs[1], 1, 1, 3, 3), 0.4), rnd(79, (1, xs[1], 1, 1))
            run('depthwise {} s{}'.format(xs, st[0]), 'GroupConvolution', [x, w], conv_data(st, pb, pe, 'same_upper'), bias=b)
    plans = [l_ for l_ in capfd.readouterr().err.splitlines() if l_.startswith('pool3 ')]
    return out, plans


@pytest.mark.parametrize('family', NT_FAMILIES)
def test_nontemporal_streaming_forms_at_small_sizes(hip, monkeypatch, capfd, family):
    """Every kernel that reads PVHIP_STREAM_NT, in its nontemporal form (=2) on a grid capped by PVHIP_STREAM_WG=1: the same bits as the
    plain form (=0) -- a nontemporal access must not change a value -- and the reference's values: bit for bit against the oracle for
    the ops of helpers.BIT_EXACT, ref64.check_group against float64 for Sigmoid and depthwise + bias + Clamp 0..6."""
    nt, nt_plans = _nt_outputs(monkeypatch, capfd, family, '2')
    plain, plain_plans = _nt_outputs(monkeypatch, capfd, family, '0')
    if family in ('maxpool', 'depthwise'):               # every launch on the cols kernel (its pool3 plan found), in both modes
        for case, (_, ins, _, _, _) in nt.items():
            n, c, h, w = ins[0].shape
            tag = 'pool3 planes={} {}x{}->'.format(n * c, h, w)
            for plans in (nt_plans, plain_plans):
                assert any(l_.startswith(tag) and ': ok ' in l_ for l_ in plans), (case, plans)
    assert nt.keys() == plain.keys()
    for case, (type_, ins, data, bias, got) in nt.items():
        assert_bit_exact(got, plain[case][4], case + ': nontemporal vs plain')
        if type_ == 'Sigmoid':
            ref64.check_group(got, ref64.sigmoid(ins[0]), what=case)
        elif type_ == 'GroupConvolution':
            st, pb, pe = (ref64._ints(data[k]) for k in ('strides', 'pads_begin', 'pads_end'))
            conv = ref64.group_convolution_depthwise(ins[0], ins[1], st, pb, pe, data['auto_pad'])
            ref64.check_group(got, np.clip(conv + bias, 0.0, 6.0), what=case)
        else:
            assert type_ in helpers.BIT_EXACT
            want = first_out(oracle_plugin(type_).compute(make_node(type_, ins, data), dict(enumerate(ins)), kernel_type='special'))
            assert_bit_exact(got, np.asarray(want, dtype=np.float32), case + ' vs oracle')
