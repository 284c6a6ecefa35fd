"""The SSD pass bench.py times -- ssd_mobilenet_v1_coco fp32, batch 128, whole IR (prior boxes folded, DetectionOutput on the device),
default knobs -- and the same IR as FP16, checked launch by launch against a float64 reference (tests/ref64.py) on 32 of its images
(ref64.SAMPLE_128: 0-7, 120-127 -- the last tiles of every persistent walk; 127 is the image the SSD fixture pins -- and 16 seeded
positions in between).  Each fused group is recomputed from the HIP tensors it read, so an error shows in the launch that made it.

At this batch the large-tensor forms run: every early depthwise layer on dwconv3x3_cols_kernel with nontemporal accesses (from 64 MiB
moved on), the Sigmoid over the class scores on the nontemporal runs-of-four unary kernel, and the box / class heads (K = 12, 24, 273,
546 over 19^2 .. 1^2 pixels) with pixel tiles that cross image boundaries.  The prior-box subgraph does not depend on the image: it is
read whole and held against the oracle.  DetectionOutput is held against the oracle fed the pass's own loc / conf rows and priors.
GPU only."""
import os
import time

import numpy as np
import pytest

import helpers
import ref64

pytestmark = pytest.mark.gpu

HIP = 'pyopenvino_amd.op_plugins'
B = 128
SAMPLE = ref64.SAMPLE_128
XML = os.path.join(helpers.MODELS, 'ssd_mobilenet_v1_coco.xml')

GEMM, PW = 'implicit GEMM (LDS-DMA)', 'pointwise'
# Convolution.kernel_kind of every convolution of the fp32 pass (names without FeatureExtractor/MobilenetV1/ and the node suffix).  No
# Winograd layer: every launch is held to the tight fp32 bound.
KINDS = {'MobilenetV1/Conv2d_0': GEMM}
KINDS.update({'MobilenetV1/Conv2d_{}_pointwise'.format(i): PW for i in range(1, 14)})
for _i, (_k1, _k3) in enumerate(((256, 512), (128, 256), (128, 256), (64, 128)), start=2):
    KINDS['Conv2d_13_pointwise_1_Conv2d_{}_1x1_{}'.format(_i, _k1)] = PW
    KINDS['Conv2d_13_pointwise_2_Conv2d_{}_3x3_s2_{}'.format(_i, _k3)] = GEMM
KINDS.update({'BoxPredictor_{}/{}Predictor'.format(i, h): PW for i in range(6) for h in ('BoxEncoding', 'Class')})


def conv_name(node):
    name = node['name']
    for part in ('FeatureExtractor/MobilenetV1/', '/BatchNorm/batchnorm/mul_1', '/Conv2D'):
        name = name.replace(part, '')
    return name


def static_launches(G):
    """The prior-box subgraph and DetectionOutput: the groups check_pass leaves to the caller."""
    return {n for n in G.nodes if G.nodes[n]['name'] in ref64.SSD_PRIOR_BOX_SUBGRAPH or G.nodes[n]['type'] == 'DetectionOutput'}


_PRECISION = {np.dtype(np.float32): 'FP32', np.dtype(np.int64): 'I64', np.dtype(np.int32): 'I32'}


def check_prior_boxes(net):
    """Every group of the prior-box subgraph, whole, against the oracle's op on the HIP pass's own inputs: bit for bit (ShapeOf,
    StridedSlice, PriorBoxClustered, Unsqueeze and Concat are all helpers.BIT_EXACT).  -> the priors DetectionOutput reads."""
    import importlib
    G = net.G
    by_name = {G.nodes[n]['name']: n for n in G.nodes}
    for name in ref64.SSD_PRIOR_BOX_SUBGRAPH:
        nid = by_name[name]
        node = G.nodes[nid]
        assert node['type'] in helpers.BIT_EXACT, node['type']
        ins = {}
        for p in G.pred[nid]:
            src_port, sink = G.edges[(p, nid)]['connection'][1], G.edges[(p, nid)]['connection'][3]
            data = G.nodes[p]['output'][src_port]['data']
            if node['type'] == 'ShapeOf':           # only the shape is read: the image tensor is not copied to the host for it
                data = np.empty(tuple(data.shape), dtype=np.float32)
            ins[sink] = np.asarray(data)
        onode = dict(node, input={p: dict(node['input'][p], precision=_PRECISION[ins[p].dtype], dims=tuple(ins[p].shape)) for p in ins})
        want = next(iter(importlib.import_module('oracle.op_plugins.' + node['type']).compute(onode, ins).values()))
        got = np.asarray(next(iter(node['output'].values()))['data'])
        if want.dtype.kind == 'i':
            assert got.dtype == want.dtype and np.array_equal(got, want), name
        else:
            helpers.assert_bit_exact(got, np.asarray(want, dtype=np.float32), name)
    return np.asarray(next(iter(G.nodes[by_name['ConcatPriorBoxesClustered']]['output'].values()))['data'])


def _ssd_input():
    from pyopenvino_amd import synth
    z = np.load(os.path.join(helpers.GOLDEN, 'ssd_full_e2e.npz'))
    x = synth.uniform_pixels(777, (B, 3, 300, 300))
    x[B - 1] = synth.uniform_pixels(int(z['image_seed']), (1, 3, 300, 300))[0]
    return z, x


def test_ssd_fp32_batch128_every_group_vs_float64(hip):
    from pyopenvino_amd import synth
    t0 = time.time()
    z, x = _ssd_input()
    blob = synth.synth_weights(XML, int(z['weight_seed']))
    _, net, ex = helpers.build_network(HIP, 'ssd_mobilenet_v1_coco', weights=blob, batch=B)
    got = helpers.infer_one(ex, net, x)
    G = net.G
    # image 127 against the reference's recorded detections, as test_ssd_batch128_properties has it
    assert got.shape == (1, 1, B * 100, 7) and np.isfinite(got).all()
    last = got[:, :, (B - 1) * 100:]
    assert np.array_equal(last[0, 0, :, :2], z['out'][0, 0, :, :2]), 'record order / classes differ from the reference'
    helpers.assert_close(last, z['out'], helpers.REL_TOL, 'image 127 of the batch vs reference')
    # the family of every convolution, against the table: no Winograd form anywhere
    kinds = {conv_name(G.nodes[n]): ref64.conv_family(G.nodes[n]) for n in G.nodes if G.nodes[n]['type'] == 'Convolution'}
    assert kinds == KINDS, {k: (kinds.get(k), KINDS.get(k)) for k in set(kinds) | set(KINDS) if kinds.get(k) != KINDS.get(k)}
    assert len(kinds) == 34
    priors = check_prior_boxes(net)
    helpers.assert_bit_exact(priors, z['priors'], 'prior boxes vs reference')
    worst = ref64.check_pass(net, ex, SAMPLE, skip=static_launches(G))
    counts = ref64.check_detections(net, SAMPLE)
    ref64.report(worst, 'SSD-MobileNet fp32 batch 128')
    print('  DetectionOutput: {} sampled images, {}..{} records each; {:.0f} s in all'.format(len(counts), min(counts.values()),
                                                                                           max(counts.values()), time.time() - t0))
    assert {'GroupConvolution + Add + Clamp', PW, GEMM, 'Sigmoid', 'Multiply', 'Add', 'Transpose', 'Reshape', 'Concat'} <= set(worst)


def test_ssd_fp16_batch128_every_group_vs_float64(hip, tmp_path):
    """The FP16 IR (fp16_as_fp32=False): every Convolution on the f16 matrix cores in the LDS-DMA form (tests/golden/conv_routes.json
    pins the same routes), fp16 operands and fp32 accumulation; depthwise on the fp32 kernel over weights that hold fp16 values.  Every
    group writes a dense fp32 tensor, so each launch is held against the float64 result of its inputs with the Convolution operands
    rounded to fp16 (ref64.eval_group(f16=True)), at the 1e-5 bound of the other FP16 tests' fp32 outputs."""
    from pyopenvino_amd import IECore, synth
    t0 = time.time()
    z, x = _ssd_input()
    xml16, blob16 = synth.fp16_ir(XML, synth.synth_weights(XML, int(z['weight_seed'])), str(tmp_path))
    ie = IECore(plugin_package=HIP)
    net = ie.read_network(xml16, weights=blob16, fp16_as_fp32=False)
    net.set_batch(B)
    ex = ie.load_network(net)
    got = helpers.infer_one(ex, net, x)
    assert net.f16_mfma and got.shape == (1, 1, B * 100, 7) and np.isfinite(got).all()
    G = net.G
    kinds = {conv_name(G.nodes[n]): G.nodes[n].get('_hip_f16') for n in G.nodes if G.nodes[n]['type'] == 'Convolution'}
    assert len(kinds) == 34 and set(kinds.values()) == {'lds-dma'}, kinds
    for g in ref64.groups(ex):
        assert not ref64.is_blocked(ref64.port_data(G, g['output'])), G.nodes[g['nodes'][-1]]['name']
    check_prior_boxes(net)
    worst = ref64.check_pass(net, ex, SAMPLE, f16=True, skip=static_launches(G))
    counts = ref64.check_detections(net, SAMPLE)
    ref64.report(worst, 'SSD-MobileNet FP16 IR batch 128')
    print('  DetectionOutput: {} sampled images, {}..{} records each; {:.0f} s in all'.format(len(counts), min(counts.values()),
                                                                                           max(counts.values()), time.time() - t0))
    assert {'GroupConvolution + Add + Clamp', 'f16 lds-dma', 'Sigmoid'} <= set(worst)
