"""The pass bench.py times -- GoogLeNet at batch 256, fusion on, default knobs -- checked launch by launch against a float64 reference
(tests/ref64.py) on 32 of its images: 0-7 (the rows googlenet_rows8.npz pins), 248-255 (the last tiles of every persistent walk) and 16
seeded positions in between.  Each fused group is recomputed from the HIP tensors it read, so an error shows in the launch that made it.
GPU only.

Kernel forms at batch 256 (wino4_conv's rule, pvhip_wino.hip: the shared-V form conv_wino4s_kernel for >= 28 stages of four channels, or
>= 24 on ragged extents, or 12..16 stages with >= 2048 tiles; otherwise the persistent two-workgroup form conv_wino4_kernel, whose 512
workgroups walk several tiles each):
  - conv_wino4s_kernel, whole 4x4 patches: conv2/3x3 (C=64, 4704 tiles), inception_3b/3x3 (C=128);
  - conv_wino4s_kernel, ragged (14x14 / 7x7): inception_4a..4e/3x3, inception_5a/3x3, inception_5b/3x3;
  - conv_wino4_kernel F(4x4,3x3), whole patches: inception_3a/3x3 (C=96: 24 stages, not ragged);
  - conv_wino4_kernel F(2x2,5x5), whole patches: inception_3a, 3b, 4a..4e/5x5 (4..8 stages);
  - conv_wino4_kernel F(2x2,5x5), ragged: inception_5a/5x5, inception_5b/5x5 (7x7, 4096+ patches).
F(2x2,3x3) (conv_wino_kernel) runs on no layer at this batch."""
import os

import numpy as np
import pytest

import helpers
import ref64

pytestmark = pytest.mark.gpu

HIP = 'pyopenvino_amd.op_plugins'
B = 256
SAMPLE = ref64.SAMPLE_256

WINO4S, WINO4S_RAGGED, WINO4, WINO4_RAGGED = ref64.WINO4S, ref64.WINO4S_RAGGED, ref64.WINO4, ref64.WINO4_RAGGED
F43, F25, PW = 'Winograd F(4x4,3x3)', 'Winograd F(2x2,5x5)', 'pointwise'

# Convolution.kernel_kind of every convolution of the fp32 pass, and the wino4_conv form of the six-point ones (module docstring)
KINDS = {'conv1/7x7_s2': ('row spans (stem)', None), 'conv2/3x3_reduce': (PW, None), 'conv2/3x3': (F43, WINO4S)}
for _m, _f3, _f5 in (('3a', WINO4, WINO4), ('3b', WINO4S, WINO4), ('4a', WINO4S_RAGGED, WINO4), ('4b', WINO4S_RAGGED, WINO4),
                     ('4c', WINO4S_RAGGED, WINO4), ('4d', WINO4S_RAGGED, WINO4), ('4e', WINO4S_RAGGED, WINO4),
                     ('5a', WINO4S_RAGGED, WINO4_RAGGED), ('5b', WINO4S_RAGGED, WINO4_RAGGED)):
    for _arm in ('1x1', '3x3_reduce', '5x5_reduce', 'pool_proj'):
        KINDS['inception_{}/{}'.format(_m, _arm)] = (PW, None)
    KINDS['inception_{}/3x3'.format(_m)] = (F43, _f3)
    KINDS['inception_{}/5x5'.format(_m)] = (F25, _f5)


wino4_form, conv_family, is_blocked, report = ref64.wino4_form, ref64.conv_family, ref64.is_blocked, ref64.report


def check_pass(net, ex, f16=False, only=None):
    return ref64.check_pass(net, ex, SAMPLE, f16=f16, only=only)


def _googlenet_input():
    from pyopenvino_amd import synth
    z = np.load(os.path.join(helpers.GOLDEN, 'googlenet_rows8.npz'))
    x = synth.uniform_pixels(4242, (B, 3, 224, 224))
    for i, s in enumerate(z['image_seeds']):
        x[i] = synth.uniform_pixels(int(s), (1, 3, 224, 224))[0]
    return z, x


@pytest.mark.parametrize('stem_wino', [False, True], ids=['default', 'stem_wino'])
def test_googlenet_fp32_batch256_every_group_vs_float64(hip, monkeypatch, stem_wino):
    from pyopenvino_amd import synth, device as dev
    if stem_wino:
        helpers.setenv(monkeypatch, 'PVHIP_CONV_STEM_WINO', '1')
    z, x = _googlenet_input()
    blob = synth.synth_weights(os.path.join(helpers.MODELS, 'googlenet-v1.xml'), int(z['weight_seed']))
    _, net, ex = helpers.build_network(HIP, 'googlenet-v1', weights=blob, batch=B)
    prob = helpers.infer_one(ex, net, x)
    G = net.G
    helpers.assert_close(prob[:8], z['out'], helpers.REL_TOL, 'rows 0-7 vs reference')
    # the family of every convolution, against the table
    kinds = {}
    for n in G.nodes:
        if G.nodes[n]['type'] == 'Convolution':
            name = G.nodes[n]['name'].replace('/WithoutBiases', '')
            fam = conv_family(G.nodes[n])
            kinds[name] = (fam, wino4_form(G.nodes[n]) if 'Winograd' in fam and 'stem' not in fam else None)
    want = dict(KINDS)
    if stem_wino:
        want['conv1/7x7_s2'] = ('Winograd F(3x3,4x4), space-to-depth (stem)', None)
    assert kinds == want, {k: (kinds.get(k), want.get(k)) for k in set(kinds) | set(want) if kinds.get(k) != want.get(k)}
    assert not any(f == 'Winograd F(2x2,3x3)' for f, _ in kinds.values())
    # the channel ranges the Concat-direct launches write in place: in edge order, tiling the Concat's channels, into its own tensor
    for cat, total in ex._concat_direct.items():
        buf = next(iter(G.nodes[cat]['output'].values()))['data']
        assert isinstance(buf, dev.DeviceTensor) and buf.shape[1] == total
        off = 0
        for pred in G.pred[cat]:
            cid = next(c for c, f in ex._fusion.items() if (f['relu'] if f['relu'] is not None else f['add']) == pred)
            assert ex._fusion[cid]['into'] == (cat, off)
            sl = next(iter(G.nodes[pred]['output'].values()))['data']
            assert isinstance(sl, dev.ChannelSlice) and sl.base is buf and sl.coff == off, G.nodes[cat]['name']
            off += sl.shape[1]
        assert off == total, G.nodes[cat]['name']
    worst = check_pass(net, ex, only=2 if stem_wino else None)
    report(worst, 'GoogLeNet fp32 batch 256' + (' (PVHIP_CONV_STEM_WINO=1: conv1 and the launch after it)' if stem_wino else ''))
    if stem_wino:
        assert set(n for n in worst) >= {'Winograd F(3x3,4x4), space-to-depth (stem)'}


def test_googlenet_fp16_batch256_every_group_vs_float64(hip, tmp_path):
    """The FP16 IR on blocked fp16 tensors (default knobs): each launch against the float64 result of ITS fp16 inputs, the Convolution /
    MatMul operands rounded to fp16 (f16r).  An fp16 output (a blocked tensor; the AvgPool of one) is one fp16 rounding of an
    fp32-accumulated value:
    |got - ref| <= 2**-11 |ref| + 1e-5 (|ref| + rms(ref)); an fp32 output meets the 1e-5 bound of the other f16 tests."""
    from pyopenvino_amd import IECore, device as dev, synth
    z, x = _googlenet_input()
    xml = os.path.join(helpers.MODELS, 'googlenet-v1.xml')
    xml16, blob16 = helpers.fp16_ir(xml, synth.synth_weights(xml, int(z['weight_seed'])), str(tmp_path))
    ie = IECore(plugin_package=HIP)
    net = ie.read_network(xml16, weights=blob16, fp16_as_fp32=False)
    net.set_batch(B)
    ex = ie.load_network(net)
    helpers.infer_one(ex, net, x)
    assert net.f16_mfma and len(ex._c8_concat) == 9
    G = net.G
    blocked = [g for g in ref64.groups(ex) if is_blocked(G.nodes[g['output'][0]]['output'][g['output'][1]]['data'])]
    assert len(blocked) >= 9 * 5, len(blocked)
    worst = check_pass(net, ex, f16=True)
    report(worst, 'GoogLeNet FP16 IR batch 256, blocked fp16 tensors')
    assert isinstance(next(iter(G.nodes[next(iter(ex._c8_concat))]['output'].values()))['data'], dev.BlockedHalf)
