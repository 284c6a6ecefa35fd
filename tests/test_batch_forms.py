"""Whole fused passes at the batches where libpvhip's kernel forms switch, every launch against float64 (tests/ref64.py), and the census
that says where those batches are.

CPU part (no GPU needed).  For GoogLeNet and SSD-MobileNet, FP32 and FP16 IRs, the batch of ONE loaded network is rewritten from 1 to
256; at every batch the fusion plan is rebuilt and the library is asked what each Convolution launch takes (ref64.Census: the family from
Convolution.kernel_kind, ref64.wino4_form for the six-point layers, Convolution.route).  Each sweep is reduced to its breakpoints -- the
batches where any launch's entry changes -- and compared with tests/golden/batch_forms.json, which holds per model the breakpoints, per
class (the batches from one breakpoint up to the next) the table {conv name: [family, wino4 form]}, and whether any Route depends on the
batch at all.  GPU_BATCHES, the batches the GPU part runs, must hold every breakpoint and a batch of every class (with the batch the
batch-256 / batch-128 layer tests run): a moved threshold fails here until the list follows.

    python tests/test_batch_forms.py      # rewrite tests/golden/batch_forms.json (only when a form is MEANT to change)

What the census finds (kNumCU = 256, default knobs):
  - GoogLeNet fp32 breaks at 42, 64, 112, 168 and 256.  42: conv2/3x3 goes from F(2x2,3x3) to the persistent F(4x4,3x3) form and the 28x28
    5x5 layers from implicit GEMM to F(2x2,5x5); 64: the 14x14 3x3 layers to F(4x4,3x3); 112: conv2/3x3 to the shared-V form; 168: the
    28x28 3x3 layers to F(4x4,3x3) and the 14x14 5x5 layers to F(2x2,5x5); 256: both 7x7 families.
    Below 168 inception_4b/5x5 and 4c/5x5 (C = 24) also run a padding pass in front of the implicit-GEMM kernel (Route.pad_row).
  - No route of the GoogLeNet FP16 IR, and no family or route of SSD-MobileNet in either precision, depends on the batch up to 256 (the
    32-bit-offset guards of the c8 readers and of the stem lie above it).

GPU part.  Each pass is fused with default knobs; ref64.check_pass holds every group to the bounds of the batch-256 / batch-128 layer
tests (helpers.REL_TOL and ref64.DRIFT for fp32; 1e-5 and f16_excess <= 1 for the FP16 IRs) on 16 images (ref64.sample: the first four,
the last eight, four seeded positions in between; the whole batch up to 16), and the families the launches took are held against the
golden table of the batch's class.

Which form inside its family a launch takes -- pw_conv's tn and copy, launch_igemm's and the f16 entry's tile height and kernel form,
wino_conv's workgroup shape, the shared-V / persistent kernel of the six-point layers and whether its workgroups walk -- is pinned by
pvhip_conv2d_form: tests/test_conv_forms.py asks it for every launch of these four sweeps that enters pvhip_conv2d_f32, the pointwise route
of pvhip_conv2d_multi_f32, pvhip_conv2d_f16_dma or pvhip_conv2d_multi_f16_dma, holds the answer against the launchers' frozen inequalities,
and runs a row of every class they fall in against float64; ref64.launch_forms and ref64.family hold ref64.wino4_form against the query.
Still reported by no query: the forms inside the stem entries, the span / c8 / c8-multi readers (every launch of the GoogLeNet FP16 IR
behind its stem), the MaxPool + 1x1 launches, the fp32 multi launch with PVHIP_CONV_POINTWISE=0, the diagnostic build's overrides and
ablations, and the depthwise kernels' nontemporal switch (`dw_bytes_moved` below restates it; `pw_tn` restates plan_pw's tn, and
test_conv_forms.py compares it with the query)."""
import functools
import json
import os
import sys
import tempfile
import time

import numpy as np
import pytest

if __name__ == '__main__':          # run as a script: the package root is not on the path yet (conftest.py adds it under pytest)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import helpers
import ref64
import test_batch256_layers
import test_ssd_layers
from helpers import GOLDEN, MODELS

HIP = 'pyopenvino_amd.op_plugins'
SNAPSHOT = os.path.join(GOLDEN, 'batch_forms.json')
GOOGLENET = os.path.join(MODELS, 'googlenet-v1.xml')
SSD = os.path.join(MODELS, 'ssd_mobilenet_v1_coco.xml')
CONFIGS = {'googlenet': (GOOGLENET, False), 'googlenet_fp16': (GOOGLENET, True), 'ssd': (SSD, False), 'ssd_fp16': (SSD, True)}
SWEEP = range(1, 257)

# the batches of the GPU passes below ...
GPU_BATCHES = {'googlenet': (1, 41, 42, 64, 111, 112, 168, 255), 'googlenet_fp16': (41, 255), 'ssd': (1, 37), 'ssd_fp16': (37,)}
# ... and the whole passes other modules hold against float64 in the same way (test_batch256_layers.py, test_ssd_layers.py)
ELSEWHERE = {'googlenet': (test_batch256_layers.B,), 'googlenet_fp16': (test_batch256_layers.B,),
             'ssd': (test_ssd_layers.B,), 'ssd_fp16': (test_ssd_layers.B,)}

F23, F43, F25, GEMM = 'Winograd F(2x2,3x3)', 'Winograd F(4x4,3x3)', 'Winograd F(2x2,5x5)', 'implicit GEMM (LDS-DMA)'


# ---------------------------------------------------------------------------------------------------------------------
# the census
@functools.lru_cache(maxsize=None)
def census_snapshot(name):
    model, fp16 = CONFIGS[name]
    with tempfile.TemporaryDirectory() as tmp:
        classes, routes_vary = ref64.census_classes(ref64.Census(model, fp16, tmp), SWEEP)
    return {'breakpoints': [n for n, _ in classes], 'classes': {str(n): table for n, table in classes},
            'routes_depend_on_batch': bool(routes_vary)}


def golden(name):
    with open(SNAPSHOT) as f:
        return json.load(f)[name]


def class_table(name, batch):
    """The golden table {conv name: [family, wino4 form]} of the class `batch` falls into."""
    want = golden(name)
    return want['classes'][str(max(b for b in want['breakpoints'] if b <= batch))]


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_census_matches_the_snapshot(name):
    got, want = census_snapshot(name), golden(name)
    assert got['breakpoints'] == want['breakpoints']
    assert got == want


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_gpu_batches_cover_every_class_and_every_breakpoint(name):
    """Every class holds a batch some whole pass runs, and every breakpoint -- the lower edge of every class but the first, whose edge is
    no threshold -- is one of them.  (One class only: nothing depends on the batch, and any batch covers it.)"""
    edges = census_snapshot(name)['breakpoints']
    run = sorted(set(GPU_BATCHES[name]) | set(ELSEWHERE[name]))
    assert edges[0] == 1 and all(1 <= b <= SWEEP[-1] for b in run)
    for lo, hi in zip(edges, edges[1:] + [SWEEP[-1] + 1]):
        assert any(lo <= b < hi for b in run), 'no pass runs a batch of the class {}..{}'.format(lo, hi - 1)
    missing = [b for b in edges[1:] if b not in run]
    assert not missing, 'no pass runs the breakpoints {}'.format(missing)


def test_googlenet_fp32_census_is_the_arithmetic_of_the_eligibility_rules():
    """wino4_eligible: n ceil(h/4) ceil(w/4) >= 32 kNumCU = 8192 on whole extents, >= 1024 on ragged ones; wino25_eligible: 8192 patches of
    2x2 on whole extents, 4096 on ragged ones; the shared-V form on conv2/3x3 (16 stages) from tiles_s = ceil(196 n / 32) * 3 >= 2048."""
    up = lambda a, b: -(-a // b)
    f43 = {56: up(8192, 14 * 14), 28: up(8192, 7 * 7), 14: up(1024, 4 * 4), 7: up(1024, 2 * 2)}
    f25 = {28: up(8192, 14 * 14), 14: up(8192, 7 * 7), 7: up(4096, 4 * 4)}
    shared = next(n for n in SWEEP if up(n * 196, 32) * 3 >= 2048)
    assert (f43, f25, shared) == ({56: 42, 28: 168, 14: 64, 7: 256}, {28: 42, 14: 168, 7: 256}, 112)
    assert census_snapshot('googlenet')['breakpoints'] == sorted({1, shared} | set(f43.values()) | set(f25.values()))


def test_the_gpu_batches_run_forms_that_batch_256_never_runs():
    """F(2x2,3x3), the persistent F(4x4,3x3) form on conv2/3x3 and implicit-GEMM 5x5 layers: in the tables of the GPU batches, and in none of
    batch 256."""
    seen = set()
    for b in GPU_BATCHES['googlenet']:
        for conv, (fam, form) in class_table('googlenet', b).items():
            seen.add((fam, form, conv if conv.startswith('conv2/3x3/') else '5x5' if '/5x5/' in conv else ''))
    rare = {(F23, None, ''), (F43, ref64.WINO4, 'conv2/3x3/WithoutBiases'), (GEMM, None, '5x5')}
    assert rare <= seen
    at256 = {(fam, form, conv if conv.startswith('conv2/3x3/') else '5x5' if '/5x5/' in conv else '')
             for conv, (fam, form) in class_table('googlenet', 256).items()}
    assert not rare & at256
    # batch 255: every 56, 28 and 14 wide layer on the six-point kernels, both 7x7 families fall back
    t = class_table('googlenet', 255)
    assert all(t['inception_{}/3x3/WithoutBiases'.format(m)][0] == (F23 if m[0] == '5' else F43) and
               t['inception_{}/5x5/WithoutBiases'.format(m)][0] == (GEMM if m[0] == '5' else F25)
               for m in ('3a', '3b', '4a', '4b', '4c', '4d', '4e', '5a', '5b'))


def test_fp16_routes_and_ssd_families_do_not_depend_on_the_batch():
    for name in ('googlenet_fp16', 'ssd', 'ssd_fp16'):
        want = golden(name)
        assert want['breakpoints'] == [1] and want['routes_depend_on_batch'] is False, name
    # GoogLeNet fp32: one Route field follows the family.  inception_4b/5x5 and 4c/5x5 (C = 24, no multiple of 16) pad their input in a pass
    # of its own while they run the implicit-GEMM kernel (below batch 168) and not under F(2x2,5x5); it moves with a breakpoint of the families
    assert golden('googlenet')['routes_depend_on_batch'] is True


# ---------------------------------------------------------------------------------------------------------------------
# SSD-MobileNet at batch 37: restatements of two switches no query reports
def dw_bytes_moved(node):
    """What group_conv2d's 3x3 kernel counts against the 64 MiB point of PVHIP_STREAM_NT (pvhip_pool.hip): input plus output, fp32."""
    n, c, h, w = node['input'][0]['dims']
    _, _, oh, ow = next(iter(node['output'].values()))['dims']
    return n * c * (h * w + oh * ow) * 4


def pw_tn(node):
    """pw_conv's channel tiles per workgroup (pvhip_pw.hip, default knobs, kNumCU = 256)."""
    n, _, h, w = node['input'][0]['dims']
    t = -(-node['input'][1]['dims'][0] // 32)
    grid2 = -(-(n * h * w) // 128) * ((t + 1) // 2)
    return 1 if t == 1 or grid2 < 4 * 256 or (t & 1 and grid2 < 16 * 256) else 2


def ssd_switches(batch):
    """-> ({depthwise layer: nontemporal?}, {MobilenetV1 pointwise layer: tn}) at this batch, from the port dims."""
    with tempfile.TemporaryDirectory() as tmp:
        census = ref64.Census(SSD, False, tmp)
    census.at(batch)
    G = census.net.G
    nodes = [G.nodes[n] for n in G.nodes]
    nt = {test_ssd_layers.conv_name(nd): dw_bytes_moved(nd) >= 64 << 20 for nd in nodes if nd['type'] == 'GroupConvolution'}
    tn = {test_ssd_layers.conv_name(nd): pw_tn(nd) for nd in nodes if nd['type'] == 'Convolution' and '_pointwise/' in nd['name']}
    return nt, tn


def test_ssd_batch37_mixes_the_forms_that_batches_2_and_128_run_apart():
    nt, tn = ssd_switches(37)
    assert len(nt) == 13 and len(tn) == 13
    assert sorted(k for k, v in nt.items() if v) == sorted('MobilenetV1/Conv2d_{}_depthwise/depthwise'.format(i) for i in range(1, 7))
    assert sorted(k for k, v in tn.items() if v == 2) == sorted('MobilenetV1/Conv2d_{}_pointwise'.format(i) for i in range(1, 6))
    nt, tn = ssd_switches(128)
    assert all(nt.values()) and set(tn.values()) == {2}
    nt, tn = ssd_switches(2)
    assert not any(nt.values()) and set(tn.values()) == {1}


# ---------------------------------------------------------------------------------------------------------------------
# the GPU passes
def _sample(batch):
    return ref64.sample(batch, first=4, last=8, between=4)


def check_families(net, ex, name, batch, fp16=False):
    """The plan's launches take what the golden table of the batch's class says, and the pass that just ran left exactly that on its
    nodes: the Route of every launch (an eager pass keeps it in node['_hip_route']), and for an FP16 IR the label in node['_hip_f16']."""
    G = net.G
    forms = ref64.launch_forms(net, ex, batch)
    want = class_table(name, batch)
    got = {conv: [fam, form] for conv, (fam, form, _) in forms.items()}
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    by_name = {G.nodes[n]['name']: G.nodes[n] for n in G.nodes if G.nodes[n]['type'] == 'Convolution'}
    for conv, (fam, _, route) in forms.items():
        node = by_name[conv]
        assert node.get('_hip_route') is not None and node['_hip_route'][1] == route, (conv, node.get('_hip_route'), route)
        if fp16:
            assert 'f16 ' + str(node.get('_hip_f16')) == fam, (conv, node.get('_hip_f16'), fam)
    return got


def check_concat_direct(net, ex):
    """The channel ranges the Concat-direct launches write in place: in edge order, tiling the Concat's channels, into its own tensor."""
    from pyopenvino_amd import device as dev
    G = net.G
    assert len(ex._concat_direct) == 9
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


def _googlenet_input(batch):
    """Seeded pixels; images 0-7 (as far as the batch holds them) are the ones googlenet_rows8.npz pins."""
    from pyopenvino_amd import synth
    z = np.load(os.path.join(GOLDEN, 'googlenet_rows8.npz'))
    x = synth.uniform_pixels(4242, (batch, 3, 224, 224))
    for i, s in enumerate(z['image_seeds'][:batch]):
        x[i] = synth.uniform_pixels(int(s), (1, 3, 224, 224))[0]
    return z, x


def _print_table(what, kinds):
    print('\n{}: kernel family of every Convolution launch'.format(what))
    for conv, (fam, form) in kinds.items():
        if fam != 'pointwise':
            print('  {:36s} {}{}'.format(conv.replace('/WithoutBiases', ''), fam, ' / ' + form if form else ''))


@pytest.mark.gpu
@pytest.mark.parametrize('batch', GPU_BATCHES['googlenet'])
def test_googlenet_fp32_every_group_vs_float64(hip, batch):
    from pyopenvino_amd import synth
    t0 = time.time()
    z, x = _googlenet_input(batch)
    blob = synth.synth_weights(GOOGLENET, int(z['weight_seed']))
    _, net, ex = helpers.build_network(HIP, 'googlenet-v1', weights=blob, batch=batch)
    prob = helpers.infer_one(ex, net, x)
    rows = min(batch, 8)
    helpers.assert_close(prob[:rows], z['out'][:rows], helpers.REL_TOL, 'rows 0-{} vs reference'.format(rows - 1))
    kinds = check_families(net, ex, 'googlenet', batch)
    check_concat_direct(net, ex)
    worst = ref64.check_pass(net, ex, _sample(batch))
    _print_table('GoogLeNet fp32 batch {}'.format(batch), kinds)
    ref64.report(worst, 'GoogLeNet fp32 batch {}'.format(batch))
    print('  {} sampled images; {:.0f} s in all'.format(len(_sample(batch)), time.time() - t0))
    ran = {fam.split(' / ')[0].split(' + ')[-1] for fam in worst}
    assert {fam for fam, _ in kinds.values()} <= ran, ran


@pytest.mark.gpu
@pytest.mark.parametrize('batch', GPU_BATCHES['googlenet_fp16'])
def test_googlenet_fp16_every_group_vs_float64(hip, tmp_path, batch):
    """The FP16 IR on blocked fp16 tensors (bounds: test_batch256_layers.py).  Both batches are odd: 49 n pixels of the 7x7 layers cross
    the 32- and 128-pixel tiles inside images."""
    from pyopenvino_amd import IECore, device as dev, synth
    t0 = time.time()
    z, x = _googlenet_input(batch)
    xml16, blob16 = helpers.fp16_ir(GOOGLENET, synth.synth_weights(GOOGLENET, int(z['weight_seed'])), str(tmp_path))
    ie = IECore(plugin_package=HIP)
    net = ie.read_network(xml16, weights=blob16, fp16_as_fp32=False)
    net.set_batch(batch)
    ex = ie.load_network(net)
    helpers.infer_one(ex, net, x)
    assert net.f16_mfma and len(ex._c8_concat) == 9
    G = net.G
    kinds = check_families(net, ex, 'googlenet_fp16', batch, fp16=True)
    blocked = [g for g in ref64.groups(ex) if ref64.is_blocked(ref64.port_data(G, g['output']))]
    assert len(blocked) >= 9 * 5, len(blocked)
    assert isinstance(next(iter(G.nodes[next(iter(ex._c8_concat))]['output'].values()))['data'], dev.BlockedHalf)
    worst = ref64.check_pass(net, ex, _sample(batch), f16=True)
    _print_table('GoogLeNet FP16 IR batch {}'.format(batch), kinds)
    ref64.report(worst, 'GoogLeNet FP16 IR batch {}, blocked fp16 tensors'.format(batch))
    print('  {} sampled images; {:.0f} s in all'.format(len(_sample(batch)), time.time() - t0))


def _ssd_input(batch):
    """Seeded pixels; the last image is the one ssd_full_e2e.npz pins."""
    from pyopenvino_amd import synth
    z = np.load(os.path.join(GOLDEN, 'ssd_full_e2e.npz'))
    x = synth.uniform_pixels(777, (batch, 3, 300, 300))
    x[batch - 1] = synth.uniform_pixels(int(z['image_seed']), (1, 3, 300, 300))[0]
    return z, x


@pytest.mark.gpu
@pytest.mark.parametrize('batch', GPU_BATCHES['ssd'])
def test_ssd_fp32_every_group_vs_float64(hip, batch):
    """Batch 1, and batch 37, where one pass mixes what batches 2 and 128 run apart (ssd_switches, from the shapes): the depthwise layers
    1-6 move 65..254 MiB each (input plus output; layer 6: 37 x 256 x (38^2 + 19^2) x 4 B = 65.2 MiB) and run nontemporal, layers 7-13 move
    29..52 MiB and run plain; the pointwise layers 1-5 have ceil(P/128) ceil(T/2) = 1672..6504 >= 4 kNumCU workgroups of two channel tiles
    (tn = 2), layers 6-13 (19x19: 105 x 8 = 840; 10x10: 29 x 16 = 464) run tn = 1.  Prior boxes and DetectionOutput as in test_ssd_layers.py;
    the last image against the reference's recorded detections."""
    from pyopenvino_amd import synth
    ssd = test_ssd_layers
    t0 = time.time()
    z, x = _ssd_input(batch)
    blob = synth.synth_weights(SSD, int(z['weight_seed']))
    _, net, ex = helpers.build_network(HIP, 'ssd_mobilenet_v1_coco', weights=blob, batch=batch)
    got = helpers.infer_one(ex, net, x)
    G = net.G
    assert got.shape == (1, 1, batch * 100, 7) and np.isfinite(got).all()
    last = got[:, :, (batch - 1) * 100:]
    assert np.array_equal(last[0, 0, :, :2], z['out'][0, 0, :, :2]), 'record order / classes differ from the reference'
    helpers.assert_close(last, z['out'], helpers.REL_TOL, 'the last image of the batch vs reference')
    kinds = check_families(net, ex, 'ssd', batch)
    assert len(kinds) == 34 and {ssd.conv_name({'name': k}): v[0] for k, v in kinds.items()} == ssd.KINDS
    priors = ssd.check_prior_boxes(net)
    helpers.assert_bit_exact(priors, z['priors'], 'prior boxes vs reference')
    sample = _sample(batch)
    worst = ref64.check_pass(net, ex, sample, skip=ssd.static_launches(G))
    counts = ref64.check_detections(net, sample)
    ref64.report(worst, 'SSD-MobileNet fp32 batch {}'.format(batch))
    print('  DetectionOutput: {} sampled images, {}..{} records each; {:.0f} s in all'.format(len(counts), min(counts.values()),
                                                                                           max(counts.values()), time.time() - t0))
    assert {'GroupConvolution + Add + Clamp', ssd.PW, ssd.GEMM, 'Sigmoid', 'Multiply', 'Add', 'Transpose', 'Reshape', 'Concat'} <= set(worst)


@pytest.mark.gpu
@pytest.mark.parametrize('batch', GPU_BATCHES['ssd_fp16'])
def test_ssd_fp16_every_group_vs_float64(hip, tmp_path, batch):
    """The FP16 IR at the same odd batch (bounds and routes: test_ssd_layers.py)."""
    from pyopenvino_amd import IECore, synth
    ssd = test_ssd_layers
    t0 = time.time()
    z, x = _ssd_input(batch)
    xml16, blob16 = synth.fp16_ir(SSD, synth.synth_weights(SSD, int(z['weight_seed'])), str(tmp_path))
    ie = IECore(plugin_package=HIP)
    net = ie.read_network(xml16, weights=blob16, fp16_as_fp32=False)
    net.set_batch(batch)
    ex = ie.load_network(net)
    got = helpers.infer_one(ex, net, x)
    assert net.f16_mfma and got.shape == (1, 1, batch * 100, 7) and np.isfinite(got).all()
    G = net.G
    kinds = check_families(net, ex, 'ssd_fp16', batch, fp16=True)
    assert len(kinds) == 34 and {fam for fam, _ in kinds.values()} == {'f16 lds-dma'}, kinds
    for g in ref64.groups(ex):
        assert not ref64.is_blocked(ref64.port_data(G, g['output'])), G.nodes[g['nodes'][-1]]['name']
    ssd.check_prior_boxes(net)
    sample = _sample(batch)
    worst = ref64.check_pass(net, ex, sample, f16=True, skip=ssd.static_launches(G))
    counts = ref64.check_detections(net, sample)
    ref64.report(worst, 'SSD-MobileNet FP16 IR batch {}'.format(batch))
    print('  DetectionOutput: {} sampled images, {}..{} records each; {:.0f} s in all'.format(len(counts), min(counts.values()),
                                                                                           max(counts.values()), time.time() - t0))
    assert {'GroupConvolution + Add + Clamp', 'f16 lds-dma', 'Sigmoid'} <= set(worst)


if __name__ == '__main__':
    out = {name: census_snapshot(name) for name in sorted(CONFIGS)}
    with open(SNAPSHOT, 'w') as f:
        f.write(json.dumps(out, sort_keys=True, separators=(',', ':')) + '\n')
    print('wrote', SNAPSHOT, os.path.getsize(SNAPSHOT), 'bytes')
