"""The route of every Convolution launch (Convolution.route: entry point, weight form, padding pass, input and output layout) of GoogLeNet
and SSD-MobileNet, FP32 and FP16 IRs, at batch 8 and 256, from the facts the fusion plan gives each launch, against
tests/golden/conv_routes.json (no GPU needed).  A GPU test ties compute() to the same decision: in an eager pass each launch leaves the
route it took on its node.

    python tests/test_conv_routes.py      # rewrite tests/golden/conv_routes.json (only when a route is MEANT to change)"""
import json
import os
import sys
import tempfile

import numpy as np
import pytest

import helpers
from helpers import GOLDEN, MODELS, REPO

SNAPSHOT = os.path.join(GOLDEN, 'conv_routes.json')
GOOGLENET = os.path.join(MODELS, 'googlenet-v1.xml')
SSD = os.path.join(MODELS, 'ssd_mobilenet_v1_coco.xml')
CONFIGS = {'{}{}_b{}'.format(name, '_fp16' if fp16 else '', batch): (model, fp16, batch)
           for name, model in (('googlenet', GOOGLENET), ('ssd', SSD)) for fp16 in (False, True) for batch in (8, 256)}


def _network(model, fp16, batch, tmp):
    from pyopenvino_amd import IECore, synth
    ie = IECore(plugin_package='pyopenvino_amd.op_plugins')
    blob = synth.synth_weights(model, 1234)
    if fp16:
        xml16, blob16 = synth.fp16_ir(model, blob, tmp)
        net = ie.read_network(xml16, weights=blob16, fp16_as_fp32=False)
    else:
        net = ie.read_network(model, weights=blob)
    net.set_batch(batch)
    return net, ie.load_network(net)


def _blocked_tensors(p):
    """The nodes whose output tensor the plan hands over blocked by eight channels (dev.BlockedHalf): the blocked convolution chains,
    Concat buffers and entry tensors, and the MaxPool / LRN launches that keep a blocked input blocked (their plugins' blocked_ok)."""
    from pyopenvino_amd.fusion_plan import data_src
    from pyopenvino_amd.op_plugins import LRN, MaxPool
    G = p.G
    blocked = {p.tail(c) for c in p.c8_out} | set(p.c8_concat) | set(p.c8_entry)
    for nid in p.order:
        node, folded = G.nodes[nid], p.lrn_pool.get(nid)
        if data_src(G, nid) not in blocked or nid in p.lrn_pool.values():
            continue
        if node['type'] == 'MaxPool' and MaxPool.blocked_ok(node, G.nodes[folded] if folded is not None else None):
            blocked.update([nid] + ([folded] if folded is not None else []))
        elif node['type'] == 'LRN' and folded is not None and LRN.blocked_ok(node, G.nodes[folded]):
            blocked.add(folded)
    return blocked


def launch_facts(ex):
    """{conv node id: the arguments of Convolution.route} for every Convolution launch of the plan."""
    from pyopenvino_amd import common_def
    from pyopenvino_amd.fusion_plan import data_src
    p = ex.plan
    G, blocked = p.G, _blocked_tensors(p)
    facts = {}
    for cid in p.order:
        node = G.nodes[cid]
        if node['type'] != 'Convolution' or cid in p.fused_away:
            continue
        f = p.fusion.get(cid) or {'into': None, 'act': None}
        pooled = p.pool_conv.get(cid)
        src = data_src(G, pooled[0]) if pooled is not None else data_src(G, cid)
        sibs = p.siblings.get(cid, ())
        geo = [common_def.string_to_tuple(node['data'][k]) for k in ('strides', 'pads_begin', 'pads_end')]
        facts[cid] = (tuple(node['input'][0]['dims']), tuple(node['input'][1]['dims']), *geo, node['data']['auto_pad'], p.f16,
                      src in blocked, None if f['into'] is None else 'blocked' if f['into'][0] in p.c8_concat else 'dense',
                      any(p.fusion[s]['into'] is not None and p.fusion[s]['into'][0] in p.c8_concat for s in sibs), cid in p.c8_out, len(sibs),
                      pooled is not None, cid in p.pre_add, f['act'] is not None and f['act'][0] != 'relu')
    return facts


def route_snapshot(name):
    from pyopenvino_amd.op_plugins import Convolution
    model, fp16, batch = CONFIGS[name]
    with tempfile.TemporaryDirectory() as tmp:
        net, ex = _network(model, fp16, batch, tmp)
    return {net.G.nodes[cid]['name']: list(Convolution.route(*f)) for cid, f in launch_facts(ex).items()}


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_conv_routes_match_the_snapshot(name):
    with open(SNAPSHOT) as f:
        want = json.load(f)[name]
    assert route_snapshot(name) == want


@pytest.mark.gpu
@pytest.mark.parametrize('fp16', [False, True])
def test_eager_pass_takes_the_predicted_routes(hip, fp16):
    """GoogLeNet at batch 256, one eager pass: every Convolution launch took the route Convolution.route gives for its plan facts."""
    from pyopenvino_amd import synth
    from pyopenvino_amd.op_plugins import Convolution
    with tempfile.TemporaryDirectory() as tmp:
        net, ex = _network(GOOGLENET, fp16, 256, tmp)
        x = np.concatenate([synth.uniform_pixels(700 + i, (1, 3, 224, 224)) for i in range(256)], 0)
        helpers.infer_one(ex, net, x)
    facts = launch_facts(ex)
    assert len(facts) >= 38
    for cid, f in facts.items():
        node = net.G.nodes[cid]
        assert '_hip_route' in node, node['name']
        assert node['_hip_route'][1] == Convolution.route(*f), (node['name'], node['_hip_route'][1], Convolution.route(*f))


if __name__ == '__main__':
    sys.path.insert(0, REPO)
    out = {name: route_snapshot(name) for name in sorted(CONFIGS)}
    with open(SNAPSHOT, 'w') as f:
        f.write(json.dumps(out, sort_keys=True, separators=(',', ':')) + '\n')
    print('wrote', SNAPSHOT, os.path.getsize(SNAPSHOT), 'bytes')
