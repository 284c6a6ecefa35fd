"""The fusion plan as data (no GPU needed): for a fixed set of networks and settings, everything the planner decides -- the task
order, the fold maps, the stream plans and the waits a recording issues -- by IR node id, against tests/golden/fusion_plan.json.
A change to what is fused shows up here as a diff of ids; a refactor of the planner must leave the file as it is.

    python tests/test_fusion_plan.py      # rewrite tests/golden/fusion_plan.json (only when the plan is MEANT to change)"""
import json
import os
import sys
import tempfile

import numpy as np
import pytest

import helpers
from helpers import GOLDEN, MODELS, REPO

SNAPSHOT = os.path.join(GOLDEN, 'fusion_plan.json')
FIELDS = ('_fusion', '_fused_away', '_concat_direct', '_lrn_pool', '_siblings', '_pool_conv', '_pre_add', '_stem_conv',
          '_c8_out', '_c8_concat', '_c8_entry')
GOOGLENET = os.path.join(MODELS, 'googlenet-v1.xml')
SSD = os.path.join(MODELS, 'ssd_mobilenet_v1_coco.xml')

# name -> (model, FP16 IR, {PVHIP_* variable: value}, fuse_epilogues); 'lrn3' is GoogLeNet's FP16 IR with LRN windows of three
CONFIGS = {
    'mnist': ('mnist', False, {}, True),
    'googlenet': (GOOGLENET, False, {}, True),
    'googlenet_unfused': (GOOGLENET, False, {}, False),
    'googlenet_locality0': (GOOGLENET, False, {'PVHIP_SCHEDULE_LOCALITY': '0'}, True),
    'googlenet_siblings0': (GOOGLENET, False, {'PVHIP_FUSE_SIBLINGS': '0'}, True),
    'googlenet_poolconv0': (GOOGLENET, False, {'PVHIP_FUSE_POOLCONV': '0'}, True),
    'googlenet_stemconv0': (GOOGLENET, False, {'PVHIP_FUSE_STEM_CONV': '0'}, True),
    'googlenet_fp16_c8_0': (GOOGLENET, True, {'PVHIP_CONV_F16_C8': '0'}, True),
    'googlenet_fp16_c8_1': (GOOGLENET, True, {'PVHIP_CONV_F16_C8': '1'}, True),
    'googlenet_fp16_c8_2': (GOOGLENET, True, {'PVHIP_CONV_F16_C8': '2'}, True),
    'googlenet_fp16_lrn3': ('lrn3', True, {}, True),
    'ssd': (SSD, False, {}, True),
    'ssd_fp16': (SSD, True, {}, True),
}
_BLOBS = {}


def _plain(obj):
    """Sets sorted, tuples as lists, dict keys as strings: one canonical JSON form whatever the hash seed."""
    if isinstance(obj, dict):
        return {str(k): _plain(v) for k, v in obj.items()}
    if isinstance(obj, (set, frozenset)):
        return sorted(_plain(v) for v in obj)
    if isinstance(obj, (list, tuple)):
        return [_plain(v) for v in obj]
    return obj


def _network(model, fp16, tmp):
    from pyopenvino_amd import IECore, synth
    ie = IECore(plugin_package='pyopenvino_amd.op_plugins')
    if model == 'mnist':
        return ie, ie.read_network(os.path.join(MODELS, 'mnist.xml'))
    if model == 'lrn3':
        from test_host_logic import _googlenet_fp16_ir_with_lrn_size
        xml16, blob16 = _googlenet_fp16_ir_with_lrn_size(tmp, 3)
        return ie, ie.read_network(xml16, weights=blob16, fp16_as_fp32=False)
    if model not in _BLOBS:
        _BLOBS[model] = synth.synth_weights(model, 1234)
    if fp16:
        xml16, blob16 = synth.fp16_ir(model, _BLOBS[model], tmp)
        return ie, ie.read_network(xml16, weights=blob16, fp16_as_fp32=False)
    return ie, ie.read_network(model, weights=_BLOBS[model])


def plan_snapshot(name, monkeypatch):
    model, fp16, env, fuse = CONFIGS[name]
    for var in ('PVHIP_SCHEDULE_LOCALITY', 'PVHIP_FUSE_SIBLINGS', 'PVHIP_FUSE_POOLCONV', 'PVHIP_FUSE_STEM_CONV', 'PVHIP_CONV_F16_C8'):
        helpers.setenv(monkeypatch, var, env.get(var))
    with tempfile.TemporaryDirectory() as tmp:
        ie, net = _network(model, fp16, tmp)
        net.set_batch(8)
        ex = ie.load_network(net)
    if not fuse:
        ex.fuse_epilogues = False
        ex.plan_fusion()
    snap = {'task_list': ex.task_list, 'list_schedule': ex.list_schedule}
    snap.update({f: getattr(ex, f) for f in FIELDS})
    for n in (1, 2, 3, 4):
        ex.compute_streams = n
        snap['plan_streams_{}'.format(n)] = ex.plan_streams()
        snap['recorded_waits_{}'.format(n)] = ex.recorded_waits()[0]
    return _plain(snap)


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_fusion_plan_matches_the_snapshot(name, monkeypatch):
    with open(SNAPSHOT) as f:
        want = json.load(f)[name]
    got = plan_snapshot(name, monkeypatch)
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], (name, key)


def _norm1(G):
    return next(n for n in G.nodes if G.nodes[n]['type'] == 'LRN' and G.nodes[n]['name'].startswith('pool1/norm1'))


def test_restricted_plan_refers_only_to_its_own_nodes():
    """infer_until's plan for fp32 GoogLeNet up to pool1/norm1: MaxPool + LRN is still one launch, but the 1x1 convolution behind it, which
    the full plan folds into that launch, is not part of the sub-graph -- so no stem convolution, and no hint or port the dispatcher
    fills for a task of the sub-graph names a node outside it."""
    import networkx as nx
    from pyopenvino_amd.fusion_plan import HINT_KEYS, data_src
    _, net, ex = helpers.build_network('pyopenvino_amd.op_plugins', 'googlenet-v1', weights=bytes(28 << 20), batch=2)
    G, full = net.G, ex.plan
    target = _norm1(G)
    pool1 = data_src(G, target)
    assert full.stem_conv and pool1 in full.stem_conv and full.lrn_pool[pool1] == target
    needed = {target} | nx.ancestors(G, target)
    sub = full.restricted(needed, {target})
    assert not sub.stem_conv and not sub.siblings and not sub.pool_conv and not sub.pre_add and not sub.concat_direct
    assert sub.lrn_pool == {pool1: target} and set(sub.order) == needed

    class Tensor:                    # what a port holds: stands for the tensor of node `nid`
        def __init__(self, nid):
            self.nid = nid
    for nid in G.nodes:
        for port in G.nodes[nid].get('output', {}).values():
            port['data'] = Tensor(nid)
    of_dict = {id(G.nodes[n]): n for n in G.nodes}

    def refs(obj):
        if isinstance(obj, Tensor):
            return {obj.nid}
        if id(obj) in of_dict:
            return {of_dict[id(obj)]}
        if isinstance(obj, dict):
            return set().union(*(refs(v) for v in obj.values()))
        if isinstance(obj, (list, tuple)):
            return set().union(*(refs(v) for v in obj))
        return set()
    ex.plan = sub
    try:
        for task in sub.order:
            if task in sub.fused_away or G.nodes[task]['type'] in ('Const', 'Parameter'):
                continue
            node = G.nodes[task]
            ex._set_hints(task, node)
            hinted = refs({k: node[k] for k in HINT_KEYS if k in node})
            assert hinted <= needed, (G.nodes[task]['name'], hinted - needed)
            assert {n for _, n in sub.receivers.get(task, ())} <= needed
        assert '_fuse_lrn' in G.nodes[pool1] and '_fuse_conv' not in G.nodes[pool1]
    finally:
        ex.plan = full


@pytest.mark.gpu
def test_infer_until_a_folded_lrn_gives_the_bits_of_the_unfused_pass(hip):
    """infer_until(x, [pool1/norm1]) on fp32 GoogLeNet runs pool1 + norm1 as one launch (the full plan's stem convolution stays out): the
    tensor equals, bit for bit, the norm1 port of an eager pass that launches every node on its own; the full plan is back afterwards."""
    from pyopenvino_amd import synth
    blob = synth.synth_weights(GOOGLENET, 1234)
    x = np.concatenate([synth.uniform_pixels(500 + i, (1, 3, 224, 224)) for i in range(2)], 0)
    _, net, ex = helpers.build_network('pyopenvino_amd.op_plugins', 'googlenet-v1', weights=blob, batch=2)
    _, net_u, ex_u = helpers.build_network('pyopenvino_amd.op_plugins', 'googlenet-v1', weights=blob, batch=2, fuse=False)
    name = net.G.nodes[_norm1(net.G)]['name']
    full = ex.plan
    got = np.asarray(ex.infer_until({net.inputs[0]['name']: x}, [name])[name])
    assert ex.plan is full
    helpers.infer_one(ex_u, net_u, x)
    want = np.asarray(next(iter(net_u.G.nodes[_norm1(net_u.G)]['output'].values()))['data'])
    assert got.shape == (2, 64, 56, 56)
    helpers.assert_bit_exact(got, want, 'pool1/norm1 of infer_until vs the unfused pass')
    helpers.assert_bit_exact(helpers.infer_one(ex, net, x), helpers.infer_one(ex_u, net_u, x), 'full pass after infer_until')


if __name__ == '__main__':
    sys.path.insert(0, REPO)
    from pyopenvino_amd import device
    out = {}
    for name in sorted(CONFIGS):
        with pytest.MonkeyPatch.context() as mp:
            out[name] = plan_snapshot(name, mp)
        device.reload_settings()
    with open(SNAPSHOT, 'w') as f:
        f.write(json.dumps(out, sort_keys=True, separators=(',', ':')) + '\n')
    print('wrote', SNAPSHOT, os.path.getsize(SNAPSHOT), 'bytes')
