"""tests/ref64.py -- the float64 reference the batch-256 layer checks hold the kernels against -- pinned on the CPU: against the oracle on
seeded small shapes, against the reference's recorded per-op outputs, and a self-test showing that the comparison those checks use
rejects subtle corruptions of a convolution's output.  CPU only."""
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


REF64_TYPES = ('Convolution', 'MaxPool', 'AvgPool', 'LRN', 'Add', 'ReLU', 'Clamp', 'Concat', 'MatMul', 'SoftMax')


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
    if node_['type'] in ('MaxPool', 'ReLU', 'Clamp', 'Concat'):
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
