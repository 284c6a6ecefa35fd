"""tests/ref64.py -- the float64 reference the layer checks (GoogLeNet at batch 256, SSD-MobileNet at batch 128) hold the kernels
against -- pinned on the CPU: against the oracle on seeded small shapes and SSD's depthwise geometries, against the reference's recorded
per-op outputs, self-tests showing that the comparison those checks use rejects subtle corruptions of a convolution's and of a depthwise
layer's output, and the groups of both plans.  CPU only."""
import os

import numpy as np
import pytest

import helpers
import ref64
from oracle import ops

PIN_TOL = 1e-5          # ref64 (float64) vs the oracle / the recorded reference (float32 arithmetic): element by element


def rnd(seed, shape, scale=1.0, shift=0.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale + shift).astype(np.float32)


def pinned(ref, want, what):
    want = np.asarray(want, dtype=np.float64)
    assert ref.dtype == np.float64, what
    assert ref.shape == want.shape, '{}: {} != {}'.format(what, ref.shape, want.shape)
    err = helpers.rel_err(ref, want)
    ex = helpers.elementwise_excess(ref, want, PIN_TOL)
    assert err <= PIN_TOL and ex <= 1.0, '{}: max-norm {:.2e}, element-wise excess {:.2f}'.format(what, err, ex)


def node(type_, data, out_dims=None):
    return {'name': type_, 'type': type_, 'data': {k: str(v) for k, v in data.items()}, 'output': {9: {'dims': out_dims}}}


CONV_CASES = [  # x shape, K, kernel, strides, pads_begin, pads_end
    ((2, 3, 17, 13), 8, (7, 7), (2, 2), (3, 3), (3, 3)),
    ((1, 5, 9, 11), 6, (3, 3), (1, 1), (1, 0), (0, 2)),          # asymmetric padding, odd extents
    ((3, 4, 7, 7), 5, (5, 5), (1, 1), (2, 2), (2, 2)),
    ((2, 16, 6, 5), 7, (1, 1), (1, 1), (0, 0), (0, 0)),
    ((1, 3, 10, 9), 4, (3, 2), (2, 3), (0, 1), (1, 0)),
]


@pytest.mark.parametrize('xs,k,ks,st,pb,pe', CONV_CASES)
def test_convolution_vs_oracle(xs, k, ks, st, pb, pe):
    x, w = rnd(1, xs), rnd(2, (k, xs[1]) + ks, 0.3)
    ref = ref64.eval_node(node('Convolution', {'strides': '{},{}'.format(*st), 'pads_begin': '{},{}'.format(*pb),
                                                'pads_end': '{},{}'.format(*pe), 'auto_pad': 'explicit'}), [x, w])
    pinned(ref, ops.convolution_special(x, w, st, pb, pe, 'explicit'), 'conv {} {}'.format(xs, ks))
    # a chunk of one image at a time gives the same numbers
    assert np.allclose(ref, ref64.convolution(x, w, st, pb, pe, chunk_bytes=1), rtol=1e-12, atol=1e-12)


POOL_CASES = [  # x shape, kernel, strides, pads_begin, pads_end, rounding
    ((2, 3, 13, 13), (3, 3), (2, 2), (0, 0), (0, 0), 'ceil'),
    ((2, 3, 12, 12), (3, 3), (2, 2), (0, 0), (0, 0), 'ceil'),
    ((1, 4, 11, 9), (3, 3), (2, 2), (0, 0), (0, 0), 'floor'),
    ((2, 5, 7, 7), (3, 3), (1, 1), (1, 1), (1, 1), 'ceil'),
    ((1, 2, 10, 7), (2, 3), (2, 1), (1, 0), (0, 2), 'floor'),
    ((1, 2, 9, 10), (3, 2), (2, 3), (0, 1), (2, 0), 'ceil'),
]


@pytest.mark.parametrize('xs,ks,st,pb,pe,rounding', POOL_CASES)
def test_pools_vs_oracle(xs, ks, st, pb, pe, rounding):
    x = rnd(3, xs, 1.0, -0.5)              # mostly negative: the zero padding wins windows at the border
    data = {'strides': '{},{}'.format(*st), 'pads_begin': '{},{}'.format(*pb), 'pads_end': '{},{}'.format(*pe),
            'kernel': '{},{}'.format(*ks), 'rounding_type': rounding, 'auto_pad': 'explicit'}
    got = ref64.eval_node(node('MaxPool', data), [x])
    want = ops.maxpool(x, st, pb, pe, ks, rounding, 'explicit')
    assert got.shape == want.shape and np.array_equal(got, want.astype(np.float64)), 'MaxPool {} {}'.format(xs, rounding)
    x = rnd(4, xs)
    got = ref64.eval_node(node('AvgPool', data), [x])
    pinned(got, ops.avgpool(x, st, pb, pe, ks, rounding, 'explicit'), 'AvgPool {} {}'.format(xs, rounding))


def test_avgpool_googlenet_global_window_is_clipped_at_h_minus_1():
    x = rnd(5, (2, 6, 7, 7))
    got = ref64.avgpool(x, (1, 1), (0, 0), (0, 0), (7, 7), 'ceil')
    assert got.shape == (2, 6, 1, 1)
    assert np.allclose(got[:, :, 0, 0], x[:, :, :6, :6].astype(np.float64).mean(axis=(2, 3)), rtol=0, atol=1e-12)
    pinned(got, ops.avgpool(x, (1, 1), (0, 0), (0, 0), (7, 7), 'ceil', 'explicit'), 'AvgPool 7x7')


@pytest.mark.parametrize('xs,size,beta', [((2, 64, 5, 7), 5, 0.75), ((1, 3, 4, 3), 5, 0.75), ((1, 9, 3, 3), 3, 0.5), ((2, 8, 1, 1), 7, 0.75)])
def test_lrn_vs_oracle(xs, size, beta):
    x = rnd(6, xs, 20.0)              # large enough that alpha * sum of squares moves the denominator
    data = {'alpha': 1e-4, 'beta': beta, 'bias': 1.0, 'size': size}
    got = ref64.eval_node(node('LRN', data), [x])
    pinned(got, ops.lrn(x, np.float32(1e-4), np.float32(beta), np.float32(1.0), size), 'LRN {} size {}'.format(xs, size))
    # alpha is NOT divided by size
    d = (1.0 + 1e-4 * (x[:, :1].astype(np.float64) ** 2 + sum(x[:, k:k + 1].astype(np.float64) ** 2 for k in range(1, min(size // 2 + 1, xs[1]))))) ** beta
    assert np.allclose(got[:, :1], x[:, :1] / d, rtol=1e-12, atol=0)


def test_eltwise_concat_matmul_softmax_vs_oracle():
    a, b, bias = rnd(7, (3, 5, 4, 3)), rnd(8, (3, 5, 4, 3)), rnd(9, (1, 5, 1, 1))
    pinned(ref64.eval_node(node('Add', {}), [a, b]), ops.add(a, b), 'Add')
    pinned(ref64.eval_node(node('Add', {}), [a, bias]), ops.add(a, bias), 'Add bias')
    assert np.array_equal(ref64.eval_node(node('ReLU', {}), [a]), ops.relu(a).astype(np.float64))
    assert np.array_equal(ref64.eval_node(node('Clamp', {'min': 0.0, 'max': 0.5}), [a]), ops.clamp(a, 0.0, 0.5).astype(np.float64))
    parts = [rnd(10, (2, 3, 5, 7)), rnd(11, (2, 1, 5, 7)), rnd(12, (2, 4, 5, 7))]
    assert np.array_equal(ref64.eval_node(node('Concat', {'axis': 1}), parts), ops.concat(parts, 1).astype(np.float64))
    x, w = rnd(13, (6, 70)), rnd(14, (33, 70), 0.1)
    for ta, tb, xx, ww in (('false', 'true', x, w), ('false', 'false', x, w.T.copy()), ('true', 'true', x.T.copy(), w), ('true', 'false', x.T.copy(), w.T.copy())):
        got = ref64.eval_node(node('MatMul', {'transpose_a': ta, 'transpose_b': tb}), [xx, ww])
        pinned(got, ops.matmul(xx, ww, ta, tb), 'MatMul {} {}'.format(ta, tb))
    logits = rnd(15, (4, 1000), 3.0)
    pinned(ref64.eval_node(node('SoftMax', {'axis': 1}), [logits]), ops.softmax_rows(logits), 'SoftMax')
    # no max shift: a row whose exp() overflows gives NaN, as in the reference
    with np.errstate(over='ignore', invalid='ignore'):
        assert np.isnan(ref64.softmax_rows(np.array([[800.0, 1.0]]))).any()


# SSD-MobileNet's depthwise layers: (x shape, strides, pads_begin, pads_end) -- stride 1 with (1,1)/(1,1), stride 2 with the (0,0)/(1,1)
# pads of same_upper on even extents and (1,1)/(1,1) on 75x75, on 150^2, 75^2, 38^2, 19^2, 10^2, 5^2 and a 1x1 plane
DW_CASES = [
    ((2, 6, 150, 150), (1, 1), (1, 1), (1, 1)),          # Conv2d_1_depthwise
    ((2, 5, 150, 150), (2, 2), (0, 0), (1, 1)),          # Conv2d_2_depthwise
    ((2, 7, 75, 75), (1, 1), (1, 1), (1, 1)),            # Conv2d_3_depthwise
    ((2, 7, 75, 75), (2, 2), (1, 1), (1, 1)),            # Conv2d_4_depthwise (odd extent: 38 = ceil(75 / 2))
    ((2, 9, 38, 38), (2, 2), (0, 0), (1, 1)),            # Conv2d_6_depthwise
    ((3, 8, 19, 19), (1, 1), (1, 1), (1, 1)),            # Conv2d_7..11_depthwise
    ((3, 8, 19, 19), (2, 2), (1, 1), (1, 1)),            # Conv2d_12_depthwise
    ((2, 16, 10, 10), (1, 1), (1, 1), (1, 1)),           # Conv2d_13_depthwise
    ((2, 16, 10, 10), (2, 2), (0, 0), (1, 1)),           # 10 -> 5 with the extra layers' pads
    ((3, 4, 5, 5), (2, 2), (1, 1), (1, 1)),              # 5 -> 3
    ((3, 4, 5, 5), (1, 1), (1, 1), (1, 1)),
    ((3, 6, 1, 1), (1, 1), (1, 1), (1, 1)),              # a 1x1 plane: only the centre tap reads the image
    ((2, 6, 2, 2), (2, 2), (0, 0), (1, 1)),              # 2 -> 1
]


def dw_data(st, pb, pe, auto_pad='same_upper'):
    return {'strides': '{},{}'.format(*st), 'pads_begin': '{},{}'.format(*pb), 'pads_end': '{},{}'.format(*pe), 'auto_pad': auto_pad,
            'dilations': '1,1'}


@pytest.mark.parametrize('xs,st,pb,pe', DW_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_group_convolution_depthwise_vs_oracle(xs, st, pb, pe):
    x, w = rnd(30, xs), rnd(31, (xs[1], 1, 1, 3, 3), 0.4)
    for auto_pad in ('same_upper', 'explicit'):
        ref = ref64.eval_node(node('GroupConvolution', dw_data(st, pb, pe, auto_pad)), [x, w])
        want = ops.group_convolution_depthwise(x, w, st, pb, pe, auto_pad)
        pinned(ref, want, 'depthwise {} stride {} pads {} {} {}'.format(xs, st, pb, pe, auto_pad))
    # the padding is where the IR says: at the end for (0,0)/(1,1) -- the first output reads no zero row or column
    if pb == (0, 0) and xs[2] >= 3:
        assert np.allclose(ref[:, :, 0, 0], (x[:, :, :3, :3].astype(np.float64) * w[None, :, 0, 0].astype(np.float64)).sum(axis=(2, 3)),
                           rtol=1e-12, atol=1e-12)


def test_group_convolution_is_not_rounded_to_fp16():
    """f16=True rounds Convolution / MatMul operands only: an FP16 IR runs depthwise on the fp32 kernel."""
    x, w = rnd(32, (2, 4, 7, 7)), rnd(33, (4, 1, 1, 3, 3), 0.4)
    n_ = node('GroupConvolution', dw_data((1, 1), (1, 1), (1, 1)))
    assert np.array_equal(ref64.eval_node(n_, [x, w], f16=True), ref64.eval_node(n_, [x, w]))
    c = node('Convolution', dw_data((1, 1), (1, 1), (1, 1)))
    wc = rnd(34, (3, 4, 3, 3), 0.4)
    assert not np.array_equal(ref64.eval_node(c, [x, wc], f16=True), ref64.eval_node(c, [x, wc]))


def test_multiply_sigmoid_transpose_vs_oracle():
    a, s_, ch = rnd(40, (3, 5, 4, 3)), rnd(41, (1, 1, 1, 1)), rnd(42, (1, 5, 1, 1))
    for x, y in ((a, s_), (s_, a), (a, ch), (ch, a), (a, rnd(43, (3, 5, 4, 3)))):
        pinned(ref64.eval_node(node('Multiply', {}), [x, y]), ops.multiply(x, y), 'Multiply {} {}'.format(x.shape, y.shape))
    x = rnd(44, (2, 1, 191, 91), 6.0)                       # SSD's conf logits: both tails of the curve
    pinned(ref64.eval_node(node('Sigmoid', {}), [x]), ops.sigmoid(x), 'Sigmoid')
    for shape, order in (((2, 12, 19, 19), (0, 2, 3, 1)), ((3, 546, 1, 1), (0, 2, 3, 1)), ((2, 5, 3, 4), (3, 1, 0, 2))):
        x = rnd(45, shape)
        got = ref64.eval_node(node('Transpose', {}), [x, np.array(order, dtype=np.int64)])
        assert np.array_equal(got, np.ascontiguousarray(x.transpose(order)).astype(np.float64)), 'Transpose {} {}'.format(shape, order)
        # the order arrives as a float64 Const when eval_group reads it from the IR
        assert np.array_equal(got, ref64.transpose(x, np.array(order, dtype=np.float64)))


REF64_TYPES = ('Convolution', 'GroupConvolution', 'MaxPool', 'AvgPool', 'LRN', 'Add', 'Multiply', 'ReLU', 'Clamp', 'Sigmoid', 'Concat',
               'Transpose', 'Reshape', 'MatMul', 'SoftMax')


def _fixtures():
    out = []
    for p in helpers.op_case_files():
        node_, _, _ = helpers.load_case(p)
        if node_['type'] in REF64_TYPES:
            out.append(p)
    return out


@pytest.mark.parametrize('path', _fixtures(), ids=lambda p: os.path.basename(p)[:-4])
def test_ref64_vs_reference_fixture(path):
    node_, inputs, want = helpers.load_case(path)
    ins = [inputs[p] for p in sorted(inputs)]
    with np.errstate(over='ignore', invalid='ignore'):
        got = ref64.eval_node(node_, ins)
    if node_['type'] in ('MaxPool', 'ReLU', 'Clamp', 'Concat', 'Transpose', 'Reshape'):
        assert np.array_equal(got.astype(np.float32), want, equal_nan=True), node_['name']
    else:
        pinned(got, want, node_['name'])


def test_the_fixture_list_covers_every_op_type():
    seen = {helpers.load_case(p)[0]['type'] for p in _fixtures()}
    assert seen == set(REF64_TYPES), seen


# ---------------------------------------------------------------------------------------------------------------------
# the comparison of the batch-256 layer checks rejects subtle errors
def _layer_3x3_c192():
    x = np.maximum(rnd(20, (3, 192, 14, 14)), 0)                    # a ReLU output, as an inception 3x3_reduce hands it over
    w = rnd(21, (64, 192, 3, 3), (2.0 / (192 * 9)) ** 0.5)
    b = rnd(22, (1, 64, 1, 1), 0.5)
    conv = ref64.convolution(x, w, (1, 1), (1, 1), (1, 1))
    return x, w, b, conv


def _corruptions():
    x, w, b, conv = _layer_3x3_c192()
    ref = conv + b
    bad = {}
    # one input channel's contribution dropped at one output pixel (image 1, channel 17, pixel (6, 9), input channel 101)
    c = ref.copy()
    c[1, 17, 6, 9] -= float((np.pad(x[1, 101].astype(np.float64), 1)[6:9, 9:12] * w[17, 101]).sum())
    bad['channel contribution dropped'] = c
    # one 32-channel block shifted by one pixel
    c = ref.copy()
    c[0, 32:64, :, 1:] = ref[0, 32:64, :, :-1]
    bad['channel block shifted'] = c
    # one image's last row zeroed
    c = ref.copy()
    c[2, :, -1, :] = 0
    bad['last row zeroed'] = c
    # the bias added twice in one channel
    c = ref.copy()
    c[:, 40] += b[0, 40, 0, 0]
    bad['bias twice'] = c
    return ref, bad


def test_clean_reference_passes_the_check():
    ref, _ = _corruptions()
    assert ref64.check_group(ref.astype(np.float32), ref) <= 0.1


@pytest.mark.parametrize('kind', ['channel contribution dropped', 'channel block shifted', 'last row zeroed', 'bias twice'])
@pytest.mark.parametrize('winograd', [False, True])
def test_check_rejects_a_subtly_wrong_layer(kind, winograd):
    ref, bad = _corruptions()
    got = bad[kind].astype(np.float32)
    assert not np.array_equal(got, ref.astype(np.float32))
    with pytest.raises(AssertionError):
        ref64.check_group(got, ref, winograd=winograd, what=kind)


def test_f16_bound_is_one_fp16_rounding():
    ref, bad = _corruptions()
    assert ref64.f16_excess(ref.astype(np.float16).astype(np.float32), ref) <= 1.0
    for kind, c in bad.items():
        assert ref64.f16_excess(c.astype(np.float16).astype(np.float32), ref) > 1.0, kind


# ---------------------------------------------------------------------------------------------------------------------
# sample(): the images a layer check compares
def test_sample_reproduces_the_constants():
    assert ref64.sample(256) == ref64.SAMPLE_256 and len(ref64.SAMPLE_256) == 32
    assert ref64.sample(128) == ref64.SAMPLE_128 and len(ref64.SAMPLE_128) == 32


def test_sample_holds_both_ends_and_never_fewer_than_twelve_images():
    for n in range(1, 300):
        for counts in ({}, {'first': 4, 'last': 8, 'between': 4}, {'first': 4, 'last': 8, 'between': 0}):
            s = ref64.sample(n, **counts)
            assert s == sorted(set(s)) and s[0] == 0 and s[-1] == n - 1, (n, counts)
            if n <= 16:
                assert s == list(range(n))
                continue
            first, last = counts.get('first', 8), counts.get('last', 8)
            assert set(range(min(first, n))) <= set(s) and set(range(n - last, n)) <= set(s)
            assert len(s) >= ref64.MIN_SAMPLE
            assert len(s) == min(n, first + last + counts.get('between', 16)), (n, counts)
        assert ref64.sample(n, first=4, last=8, between=4) == ref64.sample(n, first=4, last=8, between=4)         # seeded by n alone
    assert len(ref64.sample(255, first=4, last=8, between=4)) == 16
    for counts in ({'first': 1, 'last': 8, 'between': 2}, {'first': 4, 'last': 4, 'between': 0}, {'first': 0}, {'last': 0}):
        with pytest.raises(ValueError):
            ref64.sample(100, **counts)


# ---------------------------------------------------------------------------------------------------------------------
# groups() on the plan bench.py times (GoogLeNet fp32, batch 256, default knobs): no device needed to plan
def test_groups_of_the_batch256_plan_cover_every_node_once():
    from pyopenvino_amd import device, synth
    device.load_library()
    blob = synth.synth_weights(os.path.join(helpers.MODELS, 'googlenet-v1.xml'), 1234)
    _, net, ex = helpers.build_network('pyopenvino_amd.op_plugins', 'googlenet-v1', weights=blob, batch=256)
    G = net.G
    gs = ref64.groups(ex)
    seen = [n for g in gs for n in g['nodes']]
    assert len(seen) == len(set(seen))
    rest = {n for n in G.nodes if G.nodes[n]['type'] not in ('Const', 'Parameter', 'Result')} - set(seen)
    assert rest == set(ex._concat_direct), rest                      # only the Concats written in place are no one's group
    outs = {g['output'] for g in gs}
    for g in gs:
        assert g['output'][0] == g['nodes'][-1]
        for src in g['inputs']:
            assert src in outs or G.nodes[src[0]]['type'] == 'Parameter' or src[0] in ex._concat_direct, (g, src)
    # the placeholder ports are never an output: the stem launch's MaxPool / LRN, LRN + MaxPool's LRN, fused conv / Add ports
    placeholders = set(ex._stem_conv) | {ex._lrn_pool[p] for p in ex._stem_conv} | {l_ for l_ in ex._lrn_pool if G.nodes[l_]['type'] == 'LRN'}
    placeholders |= {c for c, f in ex._fusion.items() if f['relu'] is not None} | {f['add'] for f in ex._fusion.values() if f['relu'] is not None}
    assert not placeholders & {o[0] for o in outs}
    names = [G.nodes[g['nodes'][0]]['name'] for g in gs]
    assert names[:4] == ['data/mean', 'pool1/3x3_s2', 'conv2/3x3/WithoutBiases', 'conv2/norm26321'], names[:4]
    assert sum(len(g['convs']) for g in gs) == sum(G.nodes[n]['type'] == 'Convolution' for n in G.nodes) == 57


# ---------------------------------------------------------------------------------------------------------------------
# the comparison rejects subtly wrong depthwise layers (SSD's stride-2 form: pads (0,0)/(1,1), bias + Clamp 0..6 fused)
def _dw_layer():
    x = np.clip(rnd(50, (3, 16, 10, 10), 3.0, 2.0), 0, 6)          # a Clamp 0..6 output, as the pointwise layer before hands it over
    w = rnd(51, (16, 1, 1, 3, 3), 0.5)
    b = rnd(52, (1, 16, 1, 1), 1.0)
    return x, w, b


def _dw_out(x, w, b, pb=(0, 0), pe=(1, 1), clamp_first=False):
    conv = ref64.group_convolution_depthwise(x, w, (2, 2), pb, pe)
    return np.clip(conv, 0, 6) + b if clamp_first else np.clip(conv + b, 0, 6)


def _dw_corruptions():
    x, w, b = _dw_layer()
    ref = _dw_out(x, w, b)
    bad = {'pads at the beginning': _dw_out(x, w, b, pb=(1, 1), pe=(0, 0))}
    w2 = w.copy()
    w2[9] = w[8]
    bad['weights of the neighbouring channel'] = _dw_out(x, w2, b)
    c = ref.copy()
    c[1, :, -1, :] = 0
    bad['last output row zeroed'] = c
    bad['Clamp at 6 before the bias'] = _dw_out(x, w, b, clamp_first=True)
    # the last output column's right-hand padding tap reads the next image's first column (a tile that runs past its plane)
    conv = ref64.group_convolution_depthwise(x, w, (2, 2), (0, 0), (1, 1))
    for ky in range(3):
        oy = np.arange(5)[np.arange(5) * 2 + ky < 10]                # output rows whose tap row ky is inside the image
        conv[0, :, oy, -1] += x[1, :, oy * 2 + ky, 0] * w[:, 0, 0, ky, 2]             # (rows, channels): advanced indices first
    bad['padding tap read from the next image'] = np.clip(conv + b, 0, 6)
    return ref, bad


def test_clean_depthwise_passes_the_check():
    ref, _ = _dw_corruptions()
    assert ref64.check_group(ref.astype(np.float32), ref) <= 0.1


@pytest.mark.parametrize('kind', ['pads at the beginning', 'weights of the neighbouring channel', 'last output row zeroed',
                                  'Clamp at 6 before the bias', 'padding tap read from the next image'])
def test_check_rejects_a_subtly_wrong_depthwise_layer(kind):
    ref, bad = _dw_corruptions()
    got = bad[kind].astype(np.float32)
    assert not np.array_equal(got, ref.astype(np.float32)), kind
    with pytest.raises(AssertionError):
        ref64.check_group(got, ref, what=kind)


# ---------------------------------------------------------------------------------------------------------------------
# DetectionOutput records: a near-tie of the oracle's scores may swap ranks, anything else may not
def _records():
    rng = np.random.default_rng(60)
    want = np.zeros((100, 7), dtype=np.float32)
    want[:40, 0] = np.arange(40)
    want[:40, 1] = rng.integers(1, 91, 40)
    want[:40, 2] = np.sort(rng.uniform(0.3, 0.9, 40))[::-1]
    want[4, 2] = want[3, 2] * np.float32(1 - 3e-7)                  # a near-tie: records 3 and 4
    want[3, 1], want[4, 1] = 17, 52
    want[:40, 3:5] = rng.uniform(0, 0.5, (40, 2))
    want[:40, 5:7] = want[:40, 3:5] + rng.uniform(0.05, 0.5, (40, 2))
    want[40] = (-1, 0, 0, 0, 0, 0, 0)                                 # the terminator
    return want


def test_detection_records_compare_near_ties_as_a_set_and_reject_the_rest():
    want = _records()
    assert ref64.compare_detections(want.copy(), want, 'same') == 40
    got = want.copy()
    got[[3, 4], 1:] = got[[4, 3], 1:]                               # the tied pair in the other order: the same records
    assert ref64.compare_detections(got, want, 'tie swapped') == 40
    bad = {kind: want.copy() for kind in ('two records out of order', 'a wrong class', 'a score off by 1e-3', 'a box corner off',
                                           'a detection lost')}
    bad['two records out of order'][[9, 10], 1:] = want[[10, 9], 1:]
    bad['a wrong class'][20, 1] += 1
    bad['a score off by 1e-3'][7, 2] *= np.float32(1 + 1e-3)
    bad['a box corner off'][30, 5] += np.float32(2e-3)
    bad['a detection lost'][39:41] = want[40:42]
    for kind, c in bad.items():
        with pytest.raises(AssertionError):
            ref64.compare_detections(c, want, kind)


# ---------------------------------------------------------------------------------------------------------------------
# groups() on the SSD plan bench.py times (ssd_mobilenet_v1_coco fp32, batch 128, whole IR): no device needed to plan
def test_groups_of_the_ssd_batch128_plan_cover_every_node_once():
    """Every node belongs to exactly one group, the prior-box subgraph included: the loader folds its VALUES (PriorBoxClustered
    computes its boxes once and hands the same device tensor out on every pass) but keeps its nodes as tasks, so no node is outside a
    group.  The prior-box subgraph is exactly the part of the graph that does not depend on the image (the layer check reads it whole,
    not by image).  The 47 fused chains are groups that end at the chain's last port; no placeholder port is an output."""
    import networkx as nx
    from pyopenvino_amd import device, synth
    device.load_library()
    z = np.load(os.path.join(helpers.GOLDEN, 'ssd_full_e2e.npz'))
    blob = synth.synth_weights(os.path.join(helpers.MODELS, 'ssd_mobilenet_v1_coco.xml'), int(z['weight_seed']))
    _, net, ex = helpers.build_network('pyopenvino_amd.op_plugins', 'ssd_mobilenet_v1_coco', weights=blob, batch=128)
    G = net.G
    gs = ref64.groups(ex)
    seen = [n for g in gs for n in g['nodes']]
    assert len(seen) == len(set(seen))
    rest = {n for n in G.nodes if G.nodes[n]['type'] not in ('Const', 'Parameter', 'Result')} - set(seen)
    assert rest == set(), sorted(G.nodes[n]['name'] for n in rest)
    # the image-independent nodes: not reachable from the input once the ShapeOf edges (shape, not data) are cut
    param = next(n for n in G.nodes if G.nodes[n]['type'] == 'Parameter')
    data = nx.DiGraph([(u, v) for u, v in G.edges if G.nodes[v]['type'] != 'ShapeOf'])
    per_image = nx.descendants(data, param)
    static = sorted(G.nodes[n]['name'] for n in seen if n not in per_image)
    assert static == ref64.SSD_PRIOR_BOX_SUBGRAPH, static
    by_name = {G.nodes[n]['name']: n for n in G.nodes}
    for name in ref64.SSD_PRIOR_BOX_SUBGRAPH:                         # each a group of its own
        assert next(g for g in gs if by_name[name] in g['nodes'])['nodes'] == [by_name[name]], name
    outs = {g['output'] for g in gs}
    for g in gs:
        assert g['output'][0] == g['nodes'][-1]
        for src in g['inputs']:
            assert src in outs or src[0] == param, (g, src)
    # the fused chains: 34 Convolution + 13 GroupConvolution; Clamp 0..6 last, or the bias Add for the 12 box / class predictors
    chains = {cid: ref64._chain(ex, cid) for cid in ex._fusion}
    assert sorted(G.nodes[c]['type'] for c in chains).count('Convolution') == 34
    assert sorted(G.nodes[c]['type'] for c in chains).count('GroupConvolution') == 13 and len(chains) == 47
    by_out = {g['output']: g for g in gs}
    clamped, predictors = 0, 0
    for cid, chain in chains.items():
        last = chain[-1]
        g = by_out.get(ref64._port(G, last))
        assert g is not None and g['nodes'] == chain, G.nodes[cid]['name']
        f = ex._fusion[cid]
        if f['relu'] is not None:
            a = G.nodes[last]['data']
            assert G.nodes[last]['type'] == 'Clamp' and float(a['min']) == 0.0 and float(a['max']) == 6.0 and f['act'] == ('clamp', 0.0, 6.0)
            clamped += 1
        else:
            assert G.nodes[last]['type'] == 'Add' and last == f['add'] and 'Predictor' in G.nodes[cid]['name'], G.nodes[cid]['name']
            predictors += 1
    assert (clamped, predictors) == (35, 12)
    assert sum(len(g['convs']) for g in gs) == sum(G.nodes[n]['type'] == 'Convolution' for n in G.nodes) == 34
    # placeholder ports -- the convolution of every chain, the bias Add of a chain that goes on to a Clamp -- are never an output
    placeholders = set(chains) | {f['add'] for f in ex._fusion.values() if f['relu'] is not None}
    assert not placeholders & {o[0] for o in outs}
