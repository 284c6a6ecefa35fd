"""Host-side logic and the C-ABI surface; no GPU needed (no compute entry point is called)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
from helpers import MODELS, REPO


def test_library_loads_and_exports_every_declared_symbol():
    from pyopenvino_amd import device
    header = open(os.path.join(REPO, 'include', 'pvhip.h')).read()
    declared = set(re.findall(r'\b(pvhip_[a-z0-9_]+)\s*\(', header))
    assert len(declared) >= 40
    lib = device.load_library()                       # dlopen + prototypes; AttributeError if one is missing
    for name in declared:
        assert hasattr(lib, name), name
    assert declared == set(device.SIGNATURES), declared ^ set(device.SIGNATURES)
    nm = subprocess.run(['nm', '-D', '--defined-only', device.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r' T (pvhip_[a-z0-9_]+)', nm))
    assert declared <= exported
    m = re.search(r'#define\s+PVHIP_ABI_VERSION\s+(\d+)', header)
    assert lib.pvhip_abi_version() == int(m.group(1)) >= 9
    assert isinstance(lib.pvhip_last_error(), bytes)
    # the diagnostic build exports all of that plus what include/pvhip_diag.h declares -- and the product library none of the latter
    diag_header = open(os.path.join(REPO, 'include', 'pvhip_diag.h')).read()
    diag_only = set(re.findall(r'\b(pvhip_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', diag_header, flags=re.S)))
    assert diag_only and not (diag_only & declared) and not (diag_only & exported), diag_only & exported
    if os.path.isfile(device.DIAG_LIB_PATH):
        nm = subprocess.run(['nm', '-D', '--defined-only', device.DIAG_LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert (declared | diag_only) <= set(re.findall(r' T (pvhip_[a-z0-9_]+)', nm))


def test_header_argument_counts_match_ctypes_signatures():
    from pyopenvino_amd import device
    header = open(os.path.join(REPO, 'include', 'pvhip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name, (_, argtypes) in device.SIGNATURES.items():
        m = re.search(r'\b' + name + r'\s*\(([^;]*?)\)\s*;', header, flags=re.S)
        assert m, name
        args = m.group(1).strip()
        n = 0 if args in ('', 'void') else len(args.split(','))
        assert n == len(argtypes), '{}: header has {} parameters, ctypes {}'.format(name, n, len(argtypes))


def test_no_gpu_means_loud_failure_not_fallback():
    from pyopenvino_amd import device
    if device.device_count() > 0:
        pytest.skip('a GPU is visible here')
    with pytest.raises(device.PvhipError):
        device.DeviceTensor.from_numpy(np.zeros(4, dtype=np.float32))
    import importlib
    relu = importlib.import_module('pyopenvino_amd.op_plugins.ReLU')
    node = {'name': 'r', 'type': 'ReLU', 'input': {0: {'precision': 'FP32', 'dims': (4,)}}, 'output': {1: {'precision': 'FP32', 'dims': (4,)}}}
    with pytest.raises(device.PvhipError):
        relu.compute(node, {0: np.zeros(4, dtype=np.float32)})


def test_product_never_imports_the_oracle():
    for root, _, files in os.walk(os.path.join(REPO, 'pyopenvino_amd')):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(root, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', src, flags=re.M), f
                assert 'import torch' not in src and 'from torch' not in src, f     # no torch anywhere in the product package


def test_ir_loader_and_scheduler_match_reference_structure():
    from pyopenvino_amd import IECore
    ie = IECore()
    assert {'Convolution', 'MatMul', 'MaxPool', 'Add', 'ReLU', 'SoftMax', 'Multiply', 'AvgPool', 'Concat', 'LRN',
            'GroupConvolution', 'Clamp', 'Sigmoid', 'Const', 'Parameter', 'Result', 'Reshape', 'Transpose'} <= set(ie.plugins.plugins)
    net = ie.read_network(os.path.join(MODELS, 'mnist.xml'))
    assert len(net.G.nodes) == 33 and net.inputs[0]['name'] == 'conv2d_input'
    assert net.inputs[0]['data']['shape'] == (1, 1, 28, 28)
    conv = net.G.nodes[2]
    assert conv['type'] == 'Convolution' and conv['data']['strides'] == '1, 1' and conv['input'][1]['dims'] == (32, 1, 3, 3)
    w = net.G.nodes[1]['const']
    assert w['element_info'] == 'F32' and w['data'].dtype == np.float32 and w['data'].size == 288
    ex = ie.load_network(net)
    order = ex.task_list
    assert sorted(order) == sorted(net.G.nodes)
    pos = {n: i for i, n in enumerate(order)}
    for a, b in net.G.edges:
        assert pos[a] < pos[b]
    first_non_source = next(i for i, n in enumerate(order) if net.G.nodes[n]['type'] not in ('Const', 'Parameter'))
    assert all(net.G.nodes[n]['type'] in ('Const', 'Parameter') for n in order[:first_non_source])
    # Conv -> Add(bias) -> ReLU chains are planned as single launches
    assert set(ex._fusion) == {2, 8, 14} and ex._fused_away == {4, 5, 10, 11, 16, 17} and not ex._concat_direct
    with pytest.raises(Exception):
        ie.read_network(os.path.join(MODELS, 'does_not_exist.xml'))


def test_set_batch_rewrites_only_activation_ports():
    from pyopenvino_amd import IECore
    ie = IECore()
    net = ie.read_network(os.path.join(MODELS, 'googlenet-v1.xml'), weights=bytes(28 << 20))
    net.set_batch(256)
    G = net.G
    assert net.inputs[0]['data']['shape'] == (256, 3, 224, 224)
    assert net.outputs[0]['input'][0]['dims'] == (256, 1000)
    for nid in G.nodes:
        node = G.nodes[nid]
        if node['type'] == 'Const':
            assert node['output'][0]['dims'] == tuple(node['data']['shape'])
        if node['type'] == 'Convolution':
            assert node['input'][0]['dims'][0] == 256 and node['output'][2]['dims'][0] == 256
            assert node['input'][1]['dims'][0] != 256 or node['input'][1]['dims'] == node['input'][1]['dims']
    lrn = G.nodes[10]
    assert lrn['input'][1]['dims'] == (1,)                       # axes operand untouched
    with pytest.raises(ValueError):
        net.set_batch(0)


def test_broadcast_stride_resolution():
    from pyopenvino_amd.op_plugins._broadcast import strides_for_broadcast as sb
    assert sb((1, 6, 1, 1), (2, 6, 5, 7)) == [0, 1, 0, 0]
    assert sb((1, 10), (3, 10)) == [0, 1]
    assert sb((5,), (2, 3, 4, 5)) == [0, 0, 0, 1]
    assert sb((2, 3, 4, 5), (2, 3, 4, 5)) == [60, 20, 5, 1]
    assert sb((1, 1, 1, 1), (2, 3, 4, 5)) == [0, 0, 0, 0]
    for bad in [((2, 4), (2, 3)), ((2, 3, 4), (3, 4))]:
        with pytest.raises(ValueError):
            sb(*bad)
            np.broadcast_to(np.zeros(bad[0]), bad[1])


def test_reshape_dims_and_output_extents_match_oracle():
    from oracle import ops
    from pyopenvino_amd import common_def
    from pyopenvino_amd.op_plugins.Reshape import resolve_dims
    for shape, target in [((8, 3, 3, 64), [-1, 576]), ((8, 1024, 1, 1), [0, -1]), ((1, 19, 19, 12), [0, 1083, 1, 4]), ((2, 6), [2, 3, -1])]:
        assert resolve_dims(shape, target) == ops.reshape_dims(shape, target)
    for size in (7, 14, 28, 56, 112, 224, 300, 13):
        for k, s, pb, pe in [(3, 2, 0, 0), (3, 1, 1, 1), (7, 2, 3, 3), (2, 2, 0, 0), (3, 2, 0, 1), (5, 1, 2, 2)]:
            for rounding in ('floor', 'ceil'):
                for ap in ('explicit', 'valid', 'same_upper'):
                    for pooling in (False, True):
                        assert common_def.pooled_extent(size, k, s, pb, pe, rounding, ap, pooling) == \
                            ops.out_extent(size, k, s, pb, pe, rounding, ap, pooling)


def test_synthetic_weights_are_deterministic_and_sane():
    import hashlib
    from pyopenvino_amd import synth
    xml = os.path.join(MODELS, 'googlenet-v1.xml')
    blob = synth.synth_weights(xml, 1234)
    assert len(blob) == 27994244
    assert hashlib.sha256(blob).hexdigest() == hashlib.sha256(synth.synth_weights(xml, 1234)).hexdigest()
    assert blob != synth.synth_weights(xml, 1235)
    px = synth.uniform_pixels(7, (2, 3, 8, 8))
    assert px.dtype == np.float32 and px.min() >= 0 and px.max() <= 255 and np.array_equal(px, np.floor(px))
    z = synth.normal(3, 1, 200000)
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01


def test_shard_bounds_cover_the_batch():
    from pyopenvino_amd.shard import shard_bounds
    for total in (0, 1, 7, 256, 2048, 2049):
        for world in (1, 2, 3, 8):
            spans = [shard_bounds(total, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == total
            assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        shard_bounds(4, 2, 2)


def test_bench_work_model_matches_survey_totals():
    """The algorithmic FLOP / byte model bench.py prices the roofline with."""
    import bench
    from pyopenvino_amd import IECore
    ie = IECore()
    net = ie.read_network(os.path.join(MODELS, 'googlenet-v1.xml'), weights=bytes(28 << 20))
    work = bench.collect_work(net)
    conv_flops = sum(f for nid, (f, b) in work.items() if net.G.nodes[nid]['type'] == 'Convolution')
    assert abs(conv_flops - 3.163295744e9) < 1.0                   # GFLOP per image, SURVEY 8(a) a3
    pool_bytes = sum(b for nid, (f, b) in work.items() if net.G.nodes[nid]['type'] == 'MaxPool')
    assert abs(pool_bytes / 1e6 - (11.503 + 5.670)) < 0.01
    relu_bytes = sum(b for nid, (f, b) in work.items() if net.G.nodes[nid]['type'] == 'ReLU')
    assert abs(relu_bytes / 1e6 - 2 * 12.905) < 0.01


def test_bench_dump_outputs_writes_float_arrays_within_the_cap(tmp_path, monkeypatch):
    """bench.py --dump-outputs: one DIR/<Result name>.npy per Result in float32 / float64; above the cap, the same seeded rows every time."""
    import bench
    prob = np.arange(12000, dtype=np.float32).reshape(12, 1000)
    bench.dump_outputs({'prob/sink_port_0': prob, 'count': np.arange(3, dtype=np.int64)}, str(tmp_path / 'full'))
    got = np.load(str(tmp_path / 'full' / 'prob_sink_port_0.npy'))
    assert got.dtype == np.float32 and np.array_equal(got, prob)
    assert np.load(str(tmp_path / 'full' / 'count.npy')).dtype == np.float64
    monkeypatch.setattr(bench, 'DUMP_BYTES', 4 * 4000)
    for run in ('a', 'b'):
        bench.dump_outputs({'prob': prob}, str(tmp_path / run))
    a, b = np.load(str(tmp_path / 'a' / 'prob.npy')), np.load(str(tmp_path / 'b' / 'prob.npy'))
    assert a.shape == (4, 1000) and a.nbytes <= bench.DUMP_BYTES and np.array_equal(a, b)
    assert all(any(np.array_equal(row, p) for p in prob) for row in a)


def test_plan_folds_the_mean_add_into_conv1s_padding_pass():
    """GoogLeNet: data/mean (Add of one constant per input channel) feeds only conv1, a padded layer with C = 3: the Add is not
    dispatched, conv1 reads the Parameter and its padding pass adds the constant (the FP16 form too: test_plan_of_an_fp16_ir_...).  Unfused
    plans keep the Add."""
    _, net, ex = helpers.build_network('pyopenvino_amd.op_plugins', 'googlenet-v1', weights=bytes(28 << 20), batch=2, fuse=True)
    G = net.G
    assert len(ex._pre_add) == 1
    (cid, (aid, kid, sid)), = ex._pre_add.items()
    assert G.nodes[cid]['name'].startswith('conv1/7x7_s2') and G.nodes[aid]['type'] == 'Add' and G.nodes[kid]['type'] == 'Const'
    assert G.nodes[sid]['type'] == 'Parameter' and aid in ex._fused_away
    _, _, ex2 = helpers.build_network('pyopenvino_amd.op_plugins', 'googlenet-v1', weights=bytes(28 << 20), batch=2, fuse=False)
    assert ex2._pre_add == {}


def test_plan_of_an_fp16_ir_keeps_googlenet_on_blocked_fp16_tensors(monkeypatch):
    """GoogLeNet as an FP16 IR read with fp16_as_fp32=False (no device needed: the plan asks libpvhip's _supported queries only).  Default:
    every one of the nine channel Concats gets a blocked fp16 buffer, 21 fused convolution chains hand their output over blocked (the
    eighteen 3x3_reduce / 5x5_reduce arms, conv2/3x3_reduce, and the stem's conv1 and conv2/3x3, whose readers are MaxPool + LRN and LRN +
    MaxPool on blocked tensors), nothing is converted on the way, data/mean rides in conv1's padding pass.  PVHIP_CONV_F16_C8=1: only the 19
    tensors between a 1x1 convolution and the 3x3 / 5x5 behind it; =0: none.  An FP32 IR never gets any of it."""
    import tempfile
    from pyopenvino_amd import IECore, synth
    xml = os.path.join(MODELS, 'googlenet-v1.xml')
    blob = synth.synth_weights(xml, 1234)

    def plan(mode, fp16=True):
        helpers.setenv(monkeypatch, 'PVHIP_CONV_F16_C8', mode)      # (reloads the settings: plan and plugins read device.conv_f16_c8)
        ie = IECore(plugin_package='pyopenvino_amd.op_plugins')
        if fp16:
            with tempfile.TemporaryDirectory() as tmp:
                xml16, blob16 = synth.fp16_ir(xml, blob, tmp)
                net = ie.read_network(xml16, weights=blob16, fp16_as_fp32=False)
        else:
            net = ie.read_network(xml, weights=blob)
        net.set_batch(4)
        return net, ie.load_network(net)

    net, ex = plan(None)
    G = net.G
    names = sorted(G.nodes[c]['name'].replace('/WithoutBiases', '') for c in ex._c8_out)
    assert len(ex._c8_concat) == 9 and all(G.nodes[n]['type'] == 'Concat' for n in ex._c8_concat)
    assert len(ex._c8_out) == 21 and 'conv1/7x7_s2' in names and 'conv2/3x3' in names and 'conv2/3x3_reduce' in names, names
    assert sum(n.endswith('_reduce') for n in names) == 19
    assert ex._c8_entry == set() and len(ex._pre_add) == 1
    # every member of a blocked Concat is a fused convolution chain that writes whole 8-channel blocks at an offset that is a multiple of 8
    for cat in ex._c8_concat:
        offs = [(ex._fusion[c]['into'][1], next(iter(G.nodes[c]['output'].values()))['dims'][1]) for c in ex._fusion if ex._fusion[c]['into'] is not None and ex._fusion[c]['into'][0] == cat]
        assert len(offs) == 4 and all(o % 8 == 0 and k % 8 == 0 for o, k in offs)
        assert sum(k for _, k in offs) == next(iter(G.nodes[cat]['output'].values()))['dims'][1]
    _, ex1 = plan('1')
    assert len(ex1._c8_out) == 19 and ex1._c8_concat == set() and ex1._c8_entry == set()
    _, ex0 = plan('0')
    assert ex0._c8_out == set() and ex0._c8_concat == set()
    _, ex32 = plan(None, fp16=False)
    assert ex32._c8_out == set() and ex32._c8_concat == set() and ex32._c8_entry == set()


def _googlenet_fp16_ir_with_lrn_size(tmp, size):
    """GoogLeNet as an FP16 IR whose two LRN layers take a window of `size` channels (the blocked-fp16 LRN kernels cover five only)."""
    from pyopenvino_amd import synth
    xml = os.path.join(MODELS, 'googlenet-v1.xml')
    xml16, blob16 = synth.fp16_ir(xml, synth.synth_weights(xml, 1234), tmp)
    text = open(xml16).read()
    assert text.count('size="5"') == 2
    with open(xml16, 'w') as f:
        f.write(text.replace('size="5"', 'size="{}"'.format(size)))
    return xml16, blob16


def test_plan_of_an_fp16_ir_calls_blocked_only_what_the_plugins_will_keep_blocked(monkeypatch, tmp_path):
    """The plan and the plugins decide with the SAME predicates (MaxPool.blocked_ok, LRN.blocked_ok, Convolution.c8_dma_writer_ok =
    launch()'s own route).  GoogLeNet as an FP16 IR with LRN windows of THREE channels: neither MaxPool + LRN nor LRN + MaxPool runs on a
    blocked tensor, so the stem's convolutions must not be planned with blocked outputs (conv1, conv2/3x3 stay fp32 NCHW) and the tensor
    module 3a reads is converted once (`_c8_entry`), where the default IR (windows of five) keeps everything from conv1 on blocked."""
    from pyopenvino_amd import IECore
    from pyopenvino_amd.op_plugins import LRN, MaxPool
    helpers.setenv(monkeypatch, 'PVHIP_CONV_F16_C8', None)
    xml16, blob16 = _googlenet_fp16_ir_with_lrn_size(str(tmp_path), 3)
    ie = IECore(plugin_package='pyopenvino_amd.op_plugins')
    net = ie.read_network(xml16, weights=blob16, fp16_as_fp32=False)
    net.set_batch(4)
    ex = ie.load_network(net)
    G = net.G
    names = sorted(G.nodes[c]['name'].replace('/WithoutBiases', '') for c in ex._c8_out)
    assert 'conv1/7x7_s2' not in names and 'conv2/3x3' not in names, names
    assert len(ex._c8_concat) == 9 and len(ex._c8_entry) == 1           # the modules still run blocked, behind ONE conversion
    lrns = [n for n in G.nodes if G.nodes[n]['type'] == 'LRN']
    pools = {n: G.nodes[n] for n in G.nodes if G.nodes[n]['type'] == 'MaxPool'}
    for lid in lrns:
        folded = ex._lrn_pool.get(lid)
        if folded is not None:                                          # LRN + MaxPool launch
            assert not LRN.blocked_ok(G.nodes[lid], G.nodes[folded])
    for pid, pnode in pools.items():
        if pid in ex._lrn_pool:                                         # MaxPool + LRN launch
            assert not MaxPool.blocked_ok(pnode, G.nodes[ex._lrn_pool[pid]])
    # the predicates themselves, on IR attributes
    pool1 = next(p for p in pools.values() if p['name'].startswith('pool1/3x3_s2'))
    assert MaxPool.blocked_ok(pool1) and not MaxPool.blocked_ok(pool1, {'data': {'size': '3'}}) and MaxPool.blocked_ok(pool1, {'data': {'size': '5'}})
    odd = dict(pool1, data=dict(pool1['data'], kernel='2, 2'))
    assert not MaxPool.blocked_ok(odd)


def test_stream_plan_orders_every_cross_stream_edge(monkeypatch):
    """plan_streams on GoogLeNet (fused, Concat-eliminated) and on the unfused graph: every producer a node reads from is either on the node's own stream or in its
    wait list (and records an event); the four arms of an inception module land on four different streams; a host plugin
    set gets no plan."""
    for fuse in (True, False):
        _, net, ex = helpers.build_network('pyopenvino_amd.op_plugins', 'googlenet-v1', weights=bytes(28 << 20), batch=2, fuse=fuse)
        ex.compute_streams = 4
        stream_of, waits, records = ex.plan_streams()
        G = net.G
        assert set(stream_of.values()) >= ({0, 1, 2} if fuse else {0, 1, 2, 3})      # fused siblings leave three arms per module

        folded = {p_: s for p_, s in ex._pool_conv.values()}             # MaxPools folded into the pool_proj convolutions
        assert len(ex._pool_conv) == (7 if fuse else 0)                  # the 28x28 and 14x14 modules (rows of whole 16- / 8-byte groups)
        lead_of = {n: lead for lead, sibs in ex._siblings.items() for s in sibs
                   for n in (s, ex._fusion[s]['add'], ex._fusion[s]['relu']) if n is not None}

        def writers(nid):                    # dispatched nodes whose kernels write the tensor `nid` hands on
            if nid in folded:                # a MaxPool folded into its consumer: the tensor is the MaxPool's own input
                return writers(folded[nid])
            if nid in lead_of:               # a convolution launched with its sibling
                return [lead_of[nid]]
            if nid in ex._fused_away and G.nodes[nid]['type'] == 'Concat':
                return [w for p in G.pred[nid] for w in writers(p)]
            if nid in ex._fused_away:
                return [w for p in G.pred[nid] if G.nodes[p]['type'] != 'Const' for w in writers(p)]
            return [] if G.nodes[nid]['type'] in ('Const', 'Parameter') else [nid]

        position = {t: i for i, t in enumerate(ex.task_list)}
        for task, st in stream_of.items():
            for pred in G.pred[task]:
                for w in writers(pred):
                    assert position[w] < position[task]
                    assert stream_of[w] == st or (w in waits[task] and w in records), (G.nodes[task]['name'], G.nodes[w]['name'])
        by_name = {G.nodes[n]['name']: n for n in G.nodes}
        # LRN -> MaxPool and MaxPool -> LRN pairs the fused kernels cover are one dispatched task each (conv2/norm2 -> pool2; pool1 -> norm1)
        assert ex._lrn_pool == ({by_name['conv2/norm26321']: by_name['pool2/3x3_s2'], by_name['pool1/3x3_s2']: by_name['pool1/norm16325']} if fuse else {})
        conv = lambda a: by_name['inception_3a/' + a + '/WithoutBiases']
        if fuse:     # 1x1 + 3x3_reduce + 5x5_reduce are one launch; behind it and the pool three arms run side by side
            assert ex._siblings[conv('1x1')] == [conv('3x3_reduce'), conv('5x5_reduce')] and len(ex._siblings) == 9
            assert by_name['inception_3a/pool'] not in stream_of                 # folded into pool_proj, which forks off the module's input
            assert stream_of[conv('1x1')] != stream_of[conv('pool_proj')]
            assert len({stream_of[conv('3x3')], stream_of[conv('5x5')], stream_of[conv('pool_proj')]}) == 3
            assert stream_of[conv('3x3')] == stream_of[conv('1x1')]          # the heaviest arm stays on the producer's stream
        else:
            arms = [conv(a) for a in ('1x1', '3x3_reduce', '5x5_reduce')] + [by_name['inception_3a/pool']]
            assert len({stream_of[a] for a in arms}) == 4
            assert stream_of[conv('3x3')] == stream_of[conv('3x3_reduce')]
    _, _, ex = helpers.build_network('oracle.op_plugins', 'mnist')
    assert ex.plan_streams() is None


def test_infer_requests_api_on_host_plugins():
    """load_network(num_requests=N): requests own separate graph state; with host plugins start_async simply runs
    the pass, wait() hands the result over; a request cannot be started twice without a wait."""
    from pyopenvino_amd import IECore, synth
    ie = IECore(plugin_package='oracle.op_plugins')
    net = ie.read_network(os.path.join(MODELS, 'mnist.xml'))
    net.set_batch(2)
    ex = ie.load_network(net, 'CPU', num_requests=3)
    assert len(ex.requests) == 3 and ex.requests[0].runner is ex and ex.requests[1].runner.ienet.G is not net.G
    xs = [synth.uniform_pixels(40 + i, (2, 1, 28, 28)) for i in range(3)]
    name, out_name = net.inputs[0]['name'], net.outputs[0]['name']
    want = [ex.infer({name: x})[out_name].copy() for x in xs]
    for i, x in enumerate(xs):
        ex.start_async(i, {name: x})
    with pytest.raises(RuntimeError):
        ex.start_async(1, {name: xs[1]})
    for i in (2, 0, 1):
        assert np.array_equal(ex.wait(i)[out_name], want[i])
    assert np.array_equal(ex.requests[1].infer({name: xs[0]})[out_name], want[0])


def test_device_blocks_cannot_be_copied():
    """copy.deepcopy of a graph that holds device tensors would alias their blocks (two owners, two frees)."""
    import copy
    from pyopenvino_amd import device
    blk = device._Block.__new__(device._Block)
    blk.ptr, blk.nbytes = 0, 16
    for fn in (copy.deepcopy, copy.copy):
        with pytest.raises(device.PvhipError):
            fn(blk)
    t = device.DeviceTensor(blk, (4,))
    with pytest.raises(device.PvhipError):
        copy.deepcopy({'w': t})


def test_pickle_node_args_replays_a_node_like_the_reference(tmp_path):
    """Executable_Network.pickle_node_args (reference `inference_engine.py:216, 275-278`): run_tasks dumps `(node, inputs)` of the
    chosen nodes as node_args_<id>.pickle, and the node then runs on its own the way the reference's `test_node_sample.py:1-16`
    replays `resources/node_args_6.pickle`: unpickle, `op.compute(node, inputs)`."""
    import importlib
    import pickle
    from pyopenvino_amd import synth
    _, net, ex = helpers.build_network('oracle.op_plugins', 'mnist', batch=2)
    conv_ids = [n for n in net.G.nodes if net.G.nodes[n]['type'] == 'Convolution']
    pool_ids = [n for n in net.G.nodes if net.G.nodes[n]['type'] == 'MaxPool']
    chosen = [conv_ids[1], pool_ids[0]]
    ex.pickle_node_args = list(chosen)
    ex.pickle_dir = str(tmp_path)
    x = np.concatenate([synth.uniform_pixels(40 + i, (1, 1, 28, 28)) for i in range(2)], 0)
    helpers.infer_one(ex, net, x)
    assert sorted(os.listdir(str(tmp_path))) == sorted('node_args_{}.pickle'.format(t) for t in chosen)
    for task in chosen:
        with open(os.path.join(str(tmp_path), 'node_args_{}.pickle'.format(task)), 'rb') as f:
            node, inputs = pickle.load(file=f)
        assert node['name'] == net.G.nodes[task]['name'] and not [k for k in node if isinstance(k, str) and k.startswith('_')]
        assert all(type(v) is np.ndarray for v in inputs.values())
        op = importlib.import_module('oracle.op_plugins.' + node['type'])
        res = op.compute(node, inputs, kernel_type='special')
        port = next(iter(res))
        assert np.array_equal(res[port], np.asarray(net.G.nodes[task]['output'][port]['data']))


def test_no_inline_asm_statement_loads_into_a_register(tmp_path):
    """scripts/check_asm_loads.py (part of `make` and of build()): the sources pass, and the pattern of rounds 1-2 -- a load in one
    asm statement, its s_waitcnt in another -- is what it rejects."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('check_asm_loads', os.path.join(helpers.REPO, 'scripts', 'check_asm_loads.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.main() == 0
    old = ('asm volatile("global_load_dwordx4 %0, %2, %3\\n\\tglobal_load_dwordx4 %1, %2, %3 offset:1024" \\\n'
           '             : "=&v"(a), "=&v"(b) : "v"(off), "s"(p) : "memory");')
    got = [code for _, code in mod.asm_statements(old)]
    assert len(got) == 1 and got[0].count('global_load_dwordx4') == 2
    ok = 'asm volatile("s_mov_b32 m0, %0\\n\\tbuffer_load_dwordx4 %1, %2, %3 offen lds" :: "s"(m), "v"(v), "s"(r), "s"(o) : "memory");'
    inst = [i for _, code in mod.asm_statements(ok) for i in code.split('\n')]
    assert any('lds' in i for i in inst)


def test_expected_result_hook_takes_the_references_golden_dict(capsys):
    """Executable_Network.expected_result in the reference's own format, {node name: [precision, dims, ndarray]} (it reads
    GT[name][2]: common_def.py:76, called from inference_engine.py:284-287), and as bare arrays; a node without an entry is not
    reported by run_tasks (inference_engine.py:285), compare_results itself prints 'Skipped' (common_def.py:73-75)."""
    from pyopenvino_amd import common_def, synth
    _, net, ex = helpers.build_network('oracle.op_plugins', 'mnist', batch=1)
    x = synth.uniform_pixels(77, (1, 1, 28, 28))
    helpers.infer_one(ex, net, x)
    G = net.G
    gt = {}
    for nid in G.nodes:
        node = G.nodes[nid]
        if node['type'] in ('Convolution', 'MaxPool', 'SoftMax'):
            port = next(iter(node['output'].values()))
            gt[node['name']] = [port['precision'], port['dims'], np.array(np.asarray(port['data']), copy=True)]
    assert len(gt) >= 5
    ex.expected_result = gt
    capsys.readouterr()
    helpers.infer_one(ex, net, x)
    out = capsys.readouterr().out
    assert out.count('\x1b[32m') == len(gt) and '\x1b[31m' not in out
    wrong = next(iter(gt))
    gt[wrong] = [gt[wrong][0], gt[wrong][1], gt[wrong][2] * -3.0 + 1.0]
    ex.expected_result = {k: (v if k == wrong else v[2]) for k, v in gt.items()}      # bare arrays are taken too
    helpers.infer_one(ex, net, x)
    out = capsys.readouterr().out
    assert out.count('\x1b[31m') == 1 and out.count('\x1b[32m') == len(gt) - 1 and '\x1b[31m' + wrong in out
    assert common_def.compare_results('no such node', np.zeros(3), gt) is None and 'Skipped' in capsys.readouterr().out
    # the other debug helpers of the reference's common_def (:60-67, :109-126)
    common_def.disp_result(np.arange(8, dtype=np.float32).reshape(1, 2, 2, 2))
    out = capsys.readouterr().out
    assert out.count('C=') == 2 and ' 7.000,' in out
    common_def.dump_graph(G)
    out = capsys.readouterr().out
    assert out.count('node id=') == len(G.nodes) and out.count('edge_id=') == len(G.edges)


def _runtime_lists_after(waits_issued):
    """ROCm 7.2's bookkeeping for a sequence of (waiting stream, event's stream) waits inside one capture whose origin is stream 0,
    restated independently of the engine's CaptureStreamModel from the disassembly (profiles/r04_capture.md): a non-origin waiter
    whose event stream's parent is not the waiter itself gets parent = event stream and is appended to that stream's list.
    Returns True when hipStreamEndCapture's recursive walk over the lists, started at the origin, would never end."""
    parent, lists = {}, {}
    for waiter, ev in waits_issued:
        if waiter == 0 or parent.get(ev) == waiter:
            continue
        parent[waiter] = ev
        if waiter not in lists.setdefault(ev, []):
            lists[ev].append(waiter)
    on_path = set()

    def walk(sid):
        if sid in on_path:
            return True
        on_path.add(sid)
        ring = any(walk(c) for c in lists.get(sid, []))
        on_path.discard(sid)
        return ring

    return walk(0)


def test_multi_stream_recordings_never_close_a_ring_in_the_runtimes_stream_lists():
    """VERDICT r3 item 2.  hipStreamEndCapture died (stack overflow in its recursive walk) exactly for the plans whose raw waits
    close a ring in the runtime's parallel-stream lists -- the unfused GoogLeNet on three streams and the SSD IR on four (gpurun_out
    of round 4: scripts/capture_probe.py) -- and recorded fine for the plans that do not (fused GoogLeNet, its FP16 form, the SSD IR
    on two or three streams).  The model reproduces that split from the plans alone, and with the relays through the origin that
    _dispatch_tasks issues while recording, no plan closes a ring.  Also: every forked stream is joined back into the origin
    before the capture ends, and no wait refers to an event of an earlier pass."""
    import tempfile
    from pyopenvino_amd import IECore, synth
    from pyopenvino_amd.inference_engine import CaptureStreamModel

    def network(kind):
        ie = IECore(plugin_package='pyopenvino_amd.op_plugins')
        if kind == 'mnist':
            net = ie.read_network(os.path.join(MODELS, 'mnist.xml'))
        elif kind == 'ssd':
            xml = os.path.join(MODELS, 'ssd_mobilenet_v1_coco.xml')
            net = ie.read_network(xml, weights=synth.synth_weights(xml, 1234))
        else:
            xml = os.path.join(MODELS, 'googlenet-v1.xml')
            blob = synth.synth_weights(xml, 1234)
            if kind == 'fp16':
                with tempfile.TemporaryDirectory() as tmp:
                    xml16, blob16 = synth.fp16_ir(xml, blob, tmp)
                    net = ie.read_network(xml16, weights=blob16, fp16_as_fp32=False)
            else:
                net = ie.read_network(xml, weights=blob)
        net.set_batch(8)
        ex = ie.load_network(net)
        if kind == 'unfused':
            ex.fuse_epilogues = False
            ex.plan_fusion()
        return ex

    observed = {('unfused', 3): True, ('ssd', 4): True, ('fused', 3): False, ('fp16', 3): False, ('fp16', 4): False,
                ('ssd', 2): False, ('ssd', 3): False}           # True: hipStreamEndCapture crashed on the GPU box (raw waits)
    for kind in ('mnist', 'fused', 'unfused', 'fp16', 'ssd'):
        ex = network(kind)
        for streams in (2, 3, 4):
            ex.compute_streams = streams
            ex._stream_plans = {}
            plan = ex.plan_streams()
            stream_of, waits, records = plan
            raw = [(stream_of[t], stream_of[d]) for t in ex.task_list if t in stream_of and t not in ex._fused_away for d in waits[t]]
            if (kind, streams) in observed:
                assert _runtime_lists_after(raw) == observed[(kind, streams)], (kind, streams)
            issued, model = ex.recorded_waits()
            assert [(w, e) for _, w, e, _ in issued] == raw
            as_issued = []
            for how, w, e, _ in issued:
                as_issued += [(0, e), (w, 0)] if how == 'relay' else [(w, e)]
            assert not _runtime_lists_after(as_issued) and not model.has_ring() and not ex.recording_rings(), (kind, streams)
            assert any(how == 'relay' for how, *_ in issued) == _runtime_lists_after(raw), (kind, streams)     # relays only where needed
            # every event waited for was recorded earlier in the SAME pass, by a task on another stream
            position = {t: i for i, t in enumerate(ex.task_list)}
            for t in stream_of:
                for d in waits[t]:
                    assert d in records and position[d] < position[t] and stream_of[d] != stream_of[t]
            # the pass ends with a join of every stream the plan uses on the origin (run_tasks: `joins`), so no forked stream is left open
            assert set(stream_of.values()) <= set(range(streams)) and 0 in set(stream_of.values())
    m = CaptureStreamModel()        # the smallest ring: 2 registers under 1, re-forks from the origin, then 1 waits for 2
    assert [m.wait(2, 1), m.wait(2, 0), m.wait(1, 2)] == ['plain', 'plain', 'relay'] and not m.has_ring()
    assert _runtime_lists_after([(2, 1), (2, 0), (1, 2)]) and not _runtime_lists_after([(2, 1), (1, 2)])


def test_locality_order_is_another_legal_list_schedule(monkeypatch):
    """order_for_locality (round 4): behind a module's sibling launch come MaxPool + pool_proj (same input tensor as the launch), then
    the other arms by ascending output size (5x5, 3x3).  Still a permutation of the reference's list schedule and a topological
    order of the whole graph; PVHIP_SCHEDULE_LOCALITY=0 and the unfused plan keep the reference's order."""
    _, net, ex = helpers.build_network('pyopenvino_amd.op_plugins', 'googlenet-v1', weights=bytes(28 << 20), batch=2, fuse=True)
    G = net.G
    assert sorted(ex.task_list) == sorted(ex.list_schedule) and ex.task_list != ex.list_schedule
    pos = {t: i for i, t in enumerate(ex.task_list)}
    assert all(pos[a] < pos[b] for a, b in G.edges)
    by_name = {G.nodes[n]['name']: n for n in G.nodes}
    dispatched = [G.nodes[t]['name'] for t in ex.task_list if t not in ex._fused_away and G.nodes[t]['type'] == 'Convolution']
    for mod in ('3a', '3b', '4a', '4b', '4c', '4d', '4e'):
        at = dispatched.index('inception_{}/1x1/WithoutBiases'.format(mod))
        assert dispatched[at + 1:at + 4] == ['inception_{}/{}/WithoutBiases'.format(mod, arm) for arm in ('pool_proj', '5x5', '3x3')], mod
    for mod in ('5a', '5b'):            # 7x7 modules: the MaxPool is a launch of its own and pool_proj stays behind it
        at = dispatched.index('inception_{}/1x1/WithoutBiases'.format(mod))
        assert dispatched[at + 1:at + 4] == ['inception_{}/{}/WithoutBiases'.format(mod, arm) for arm in ('5x5', '3x3', 'pool_proj')], mod
    monkeypatch.setenv('PVHIP_SCHEDULE_LOCALITY', '0')
    ex.plan_fusion()
    assert ex.task_list == ex.list_schedule
    monkeypatch.delenv('PVHIP_SCHEDULE_LOCALITY')
    ex.plan_fusion()
    assert ex.task_list != ex.list_schedule
    ex.fuse_epilogues = False
    ex.plan_fusion()
    assert ex.task_list == ex.list_schedule
