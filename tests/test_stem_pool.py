"""The stem convolution's pooled second output and the LRN + 1x1 launch behind it (PVHIP_FUSE_STEM_POOL): conv1 writes the tensor of
pool1/3x3_s2 beside its own, so that the pool1 launch is pool1/norm1 + conv2/3x3_reduce only.  Everything bit for bit: the convolution's own
output against pvhip_conv2d_stem_direct_f32, the pooled one against pvhip_maxpool2d_f32 of it, LRN + 1x1 against pvhip_lrn_f32 followed by
the pointwise convolution, GoogLeNet end to end against the pass without the fold.  The plan test at the end needs no GPU."""
import itertools
import os

import numpy as np
import pytest

import helpers
from helpers import assert_bit_exact, build_network, first_out
from test_hip_ops import conv_data, hip_plugin, make_node, rnd

HIP = 'pyopenvino_amd.op_plugins'
GOOGLENET = os.path.join(helpers.MODELS, 'googlenet-v1.xml')
SENTINEL = 12345.0        # what an output holds before the launch: a block of the pool may still hold an earlier launch's (right) values


def _pooled(extent):
    return (extent - 3 + 1) // 2 + 1          # 3x3 / stride 2 / no padding / ceil


def _stem_launches(dev, x, wf, k, pre_add, bias, act):
    """(y, yp) of the pooled form and (y, MaxPool of y) of the two separate entries, as ndarrays."""
    n, _, h, w = x.shape
    oh, ow = (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1
    poh, pow_ = _pooled(oh), _pooled(ow)
    code, lo, hi = dev.act_args(act)
    xd = dev.DeviceTensor.from_numpy(x)
    full = lambda shape: dev.DeviceTensor.from_numpy(np.full(shape, SENTINEL, np.float32))     # noqa: E731
    y0, y1, p0, p1 = full((n, k, oh, ow)), full((n, k, oh, ow)), full((n, k, poh, pow_)), full((n, k, poh, pow_))
    dev.call('pvhip_conv2d_stem_direct_f32', dev.ptr(xd), dev.ptr(wf), dev.ptr(y0), n, h, w, k, oh, ow, dev.ptr(pre_add), dev.ptr(bias), code, lo, hi)
    dev.call('pvhip_maxpool2d_f32', dev.ptr(y0), dev.ptr(p0), n, k, oh, ow, poh, pow_, 3, 3, 2, 2, 0, 0, 0, 0)
    assert dev.call('pvhip_conv2d_stem_direct_pool_supported', 0, 3, h, w, k, 7, 7, 2, 2, 3, 3, oh, ow, poh, pow_)
    dev.call('pvhip_conv2d_stem_direct_pool_f32', dev.ptr(xd), dev.ptr(wf), dev.ptr(y1), dev.ptr(p1), n, h, w, k, oh, ow, poh, pow_,
             dev.ptr(pre_add), dev.ptr(bias), code, lo, hi)
    return tuple(np.asarray(t) for t in (y1, p1, y0, p0))


def _packed(dev, w):
    wd = dev.DeviceTensor.from_numpy(w)
    wf = dev.DeviceTensor.empty((int(dev.call('pvhip_conv2d_stem_f32_pack_elems', w.shape[0])),))
    dev.call('pvhip_conv2d_stem_f32_pack', dev.ptr(wd), dev.ptr(wf), w.shape[0])
    return wf


STEM_SHAPES = [((2, 3, 32, 32), 64),      # oh 16: the last window clipped
               ((1, 3, 36, 24), 40),      # oh 18: a ragged last tile and a two-row last window; pooled rows of six floats
               ((5, 3, 30, 32), 7),       # oh 15: no clipping, fewer than 16 channels
               ((3, 3, 40, 24), 33),
               ((70, 3, 32, 32), 64),     # 280 tiles on 256 CUs: ranges of one and two tiles, every boundary inside an image
               ((300, 3, 32, 32), 64),    # 1200 tiles: ranges of four and five tiles that cross image boundaries, the carry reused tile after tile
               ((512, 3, 32, 32), 64)]    # 2048 tiles: two whole images per CU, no tile past a range, the carry restarts with each image


@pytest.mark.gpu
@pytest.mark.parametrize('xs,k', STEM_SHAPES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else 'k{}'.format(v))
def test_stem_convolution_with_the_pooled_output(hip, xs, k):
    """y has the bits of pvhip_conv2d_stem_direct_f32, yp those of pvhip_maxpool2d_f32 on y: every activation, with and without bias, with
    and without the Add in front."""
    x, w = rnd(40 + k, xs, 60.0), rnd(50 + k, (k, 3, 7, 7), (2.0 / 147.0) ** 0.5)
    wf = _packed(hip, w)
    bias, add = hip.DeviceTensor.from_numpy(rnd(5, (1, k, 1, 1))), hip.DeviceTensor.from_numpy(rnd(11, (1, 3, 1, 1), 50.0))
    combos = list(itertools.product((('relu',), ('clamp', -0.5, 0.75), None), (bias, None), (add, None)))
    if xs[0] > 100:           # the many-tile walks: one full epilogue and one bare one (the epilogues are covered by the shapes above)
        combos = [combos[0], combos[-1]]
    for act, b, a in combos:
        y, yp, y_ref, yp_ref = _stem_launches(hip, x, wf, k, a, b, act)
        what = '{} k={} {} bias={} add={}'.format(xs, k, act, b is not None, a is not None)
        assert not (yp == SENTINEL).any(), what
        assert_bit_exact(y, y_ref, 'conv1 with a pooled output, y ' + what)
        assert_bit_exact(yp, yp_ref, 'conv1 with a pooled output, yp ' + what)


@pytest.mark.gpu
def test_stem_convolution_pooled_output_with_nans(hip):
    """NaNs in the image poison conv outputs in the first rows, across a tile boundary (conv rows 3 | 4) and in the last rows and columns:
    a NaN is the maximum of every window it lies in, exactly as in pvhip_maxpool2d_f32."""
    xs, k = (2, 3, 32, 32), 64
    x, w = rnd(3, xs, 60.0), rnd(4, (k, 3, 7, 7), (2.0 / 147.0) ** 0.5)
    x[0, 0, 0, 5] = x[0, 1, 8, 16] = x[1, 2, 31, 30] = x[1, 0, 15, 0] = np.nan
    y, yp, y_ref, yp_ref = _stem_launches(hip, x, _packed(hip, w), k, None, hip.DeviceTensor.from_numpy(rnd(5, (1, k, 1, 1))), ('relu',))
    nan_rows = {int(r) for r in np.argwhere(np.isnan(y_ref[0]))[:, 1]}
    assert {0, 3, 4} <= nan_rows and np.isnan(y_ref[1, :, 15, 15]).all() and np.isnan(yp_ref).any() and not np.isnan(yp_ref).all()
    assert np.array_equal(np.isnan(yp), np.isnan(yp_ref))
    assert_bit_exact(y, y_ref, 'y, NaNs in the image')
    assert_bit_exact(yp, yp_ref, 'yp, NaNs in the image')


@pytest.mark.gpu
def test_stem_pool_query_agrees_with_the_entry(hip):
    """What pvhip_conv2d_stem_direct_pool_supported declines for the shape (n = 0) the entry refuses, what it accepts the entry runs; with
    n > 0 the query also applies the size rule -- at least eight tiles of four output rows per CU -- which the entry does not."""
    k = 8
    wf = _packed(hip, rnd(2, (k, 3, 7, 7), 0.1))
    #        x shape          oh  ow  poh pow  shape ok
    cases = [((2, 3, 32, 32), 16, 16, 8, 8, True),
             ((1, 3, 36, 24), 18, 12, 9, 6, True),
             ((2, 3, 32, 32), 16, 16, 7, 8, False),     # not the pooling's row count
             ((2, 3, 32, 32), 16, 16, 8, 7, False),     # ... nor its column count
             ((2, 3, 4, 32), 2, 16, 1, 8, False),       # fewer than three conv rows
             ((2, 3, 32, 30), 16, 15, 8, 8, False)]     # rows the direct form does not take
    for xs, oh, ow, poh, pow_, want in cases:
        n, _, h, w = xs
        geo = (3, h, w, k, 7, 7, 2, 2, 3, 3, oh, ow, poh, pow_)
        assert bool(hip.call('pvhip_conv2d_stem_direct_pool_supported', 0, *geo)) == want, xs
        assert not hip.call('pvhip_conv2d_stem_direct_pool_supported', n, *geo), xs            # two images: far below the size rule
        x = hip.DeviceTensor.from_numpy(rnd(1, xs))
        y, yp = hip.DeviceTensor.empty((n, k, oh, ow)), hip.DeviceTensor.empty((n, k, max(poh, 1), max(pow_, 1)))
        args = (hip.ptr(x), hip.ptr(wf), hip.ptr(y), hip.ptr(yp), n, h, w, k, oh, ow, poh, pow_, hip.ptr(None), hip.ptr(None), 0, 0.0, 0.0)
        if want:
            hip.call('pvhip_conv2d_stem_direct_pool_f32', *args)
        else:
            with pytest.raises(hip.PvhipError):
                hip.call('pvhip_conv2d_stem_direct_pool_f32', *args)
    # the size rule: 16 conv rows = four tiles per image; 256 CUs x eight tiles = 2048 tiles = 512 images
    geo = (3, 32, 32, k, 7, 7, 2, 2, 3, 3, 16, 16, 8, 8)
    assert hip.call('pvhip_conv2d_stem_direct_pool_supported', 512, *geo) and not hip.call('pvhip_conv2d_stem_direct_pool_supported', 511, *geo)


def _lrn_conv(dev, x, w, bias, act, alpha, lrn_bias, fused):
    n, c, h, wd = x.shape
    k = w.shape[0]
    code, lo, hi = dev.act_args(act)
    xd = dev.DeviceTensor.from_numpy(x)
    if fused:
        y, wdev = dev.DeviceTensor.from_numpy(np.full((n, k, h, wd), SENTINEL, np.float32)), dev.DeviceTensor.from_numpy(w)
        dev.call('pvhip_lrn_conv1x1_f32', dev.ptr(xd), dev.ptr(wdev), dev.ptr(y), n, c, h * wd, 5, alpha, 0.75, lrn_bias, k, dev.ptr(bias), code, lo, hi)
        return np.asarray(y)
    normed = dev.DeviceTensor.empty((n, c, h, wd))
    dev.call('pvhip_lrn_f32', dev.ptr(xd), dev.ptr(normed), n, c, h * wd, 5, alpha, 0.75, lrn_bias)
    node = make_node('Convolution', [x, w], conv_data((1, 1), (0, 0), (0, 0)))
    node['_fuse_bias'], node['_fuse_act'] = bias, act
    return np.asarray(first_out(hip_plugin('Convolution').compute(node, {0: normed, 1: w})))


@pytest.mark.gpu
@pytest.mark.parametrize('xs,k,act', [((2, 64, 56, 56), 64, ('relu',)), ((3, 8, 5, 12), 7, None), ((1, 64, 7, 8), 33, ('clamp', -0.25, 0.5))],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) and isinstance(v[0], int) else str(v))
def test_lrn_conv1x1_has_the_bits_of_the_two_launches(hip, xs, k, act):
    """pvhip_lrn_conv1x1_f32 against pvhip_lrn_f32 followed by the pointwise convolution: GoogLeNet's alpha with bias 1 (beta mode 4) and
    with bias 0 (mode 1: two square roots and a division), with and without the convolution's bias, and a NaN in the input."""
    x = rnd(sum(xs), xs, 40.0)
    x[x == 0.0] = 1.0
    w = rnd(7, (k, xs[1], 1, 1), (2.0 / xs[1]) ** 0.5)
    bias = hip.DeviceTensor.from_numpy(rnd(9, (1, k, 1, 1)))
    alpha = 9.9999997473787516e-05
    for lrn_bias, b in ((1.0, bias), (0.0, bias), (1.0, None)):
        assert hip.call('pvhip_lrn_conv1x1_supported', xs[0], xs[1], xs[2] * xs[3], 5, 0.75, lrn_bias, k)
        got, two = (_lrn_conv(hip, x, w, b, act, alpha, lrn_bias, fused) for fused in (True, False))
        assert np.isfinite(got).all() and not (got == SENTINEL).any()
        assert_bit_exact(got, two, 'LRN + 1x1 vs two launches {} k={} bias {}'.format(xs, k, lrn_bias))
    x2 = x.copy()
    x2[0, 1, 2, 3] = np.nan
    got, two = (_lrn_conv(hip, x2, w, bias, act, alpha, 1.0, fused) for fused in (True, False))
    assert np.isnan(two).any() and np.array_equal(np.isnan(got), np.isnan(two))
    assert_bit_exact(got, two, 'LRN + 1x1 vs two launches, a NaN in the input {}'.format(xs))


@pytest.mark.gpu
def test_lrn_conv1x1_query_agrees_with_the_entry(hip):
    """What pvhip_lrn_conv1x1_supported declines the entry refuses, what it accepts the entry runs."""
    cases = [((1, 16, 6, 6), 5, 0.75, 1.0, 8, True), ((1, 64, 3, 5), 5, 0.75, 0.0, 64, True),
             ((1, 60, 6, 6), 5, 0.75, 1.0, 8, False),      # channels not a multiple of eight
             ((1, 72, 6, 6), 5, 0.75, 1.0, 8, False),      # more than 64 channels in
             ((1, 16, 6, 6), 5, 0.75, 1.0, 65, False),     # ... or out
             ((1, 16, 6, 6), 3, 0.75, 1.0, 8, False),      # another window
             ((1, 16, 6, 6), 5, 0.5, 1.0, 8, False)]       # another exponent
    for xs, size, beta, lrn_bias, k, want in cases:
        n, c, h, wd = xs
        assert bool(hip.call('pvhip_lrn_conv1x1_supported', n, c, h * wd, size, beta, lrn_bias, k)) == want, (xs, size, beta, k)
        x, w, y = (hip.DeviceTensor.from_numpy(rnd(1, s)) for s in (xs, (k, c, 1, 1), (n, k, h, wd)))
        args = (hip.ptr(x), hip.ptr(w), hip.ptr(y), n, c, h * wd, size, 1e-4, beta, lrn_bias, k, hip.ptr(None), 0, 0.0, 0.0)
        if want:
            hip.call('pvhip_lrn_conv1x1_f32', *args)
        else:
            with pytest.raises(hip.PvhipError):
                hip.call('pvhip_lrn_conv1x1_f32', *args)


def _ports(net):
    return {nid: np.array(p['data']) for nid in net.G.nodes for p in net.G.nodes[nid].get('output', {}).values()
            if 'data' in p and net.G.nodes[nid]['type'] not in ('Const', 'Parameter') and hasattr(p['data'], 'shape')}


@pytest.mark.gpu
def test_googlenet_with_the_pooled_stem_output_end_to_end(hip, monkeypatch):
    """GoogLeNet (synthetic weights, batch 4) with conv1 writing pool1's tensor (PVHIP_FUSE_STEM_POOL=2: four images are far below the
    size rule) and without (=0): every Result and every node port the same bits, dispatched eagerly and replayed from a recording."""
    from pyopenvino_amd import synth
    blob = synth.synth_weights(GOOGLENET, 1234)
    x = np.concatenate([synth.uniform_pixels(500 + i, (1, 3, 224, 224)) for i in range(4)], 0)
    runs = {}
    for mode in ('0', '2'):
        helpers.setenv(monkeypatch, 'PVHIP_FUSE_STEM_POOL', mode)
        _, net, ex = build_network(HIP, 'googlenet-v1', weights=blob, batch=4)
        name = net.inputs[0]['name']
        G = net.G
        if mode == '2':
            (cid, pid), = ex.plan.stem_pool.items()
            assert G.nodes[cid]['name'].startswith('conv1/7x7_s2') and G.nodes[pid]['name'].startswith('pool1/3x3_s2') and pid in ex._stem_conv
        else:
            assert not ex.plan.stem_pool
        eager = {k_: np.asarray(v) for k_, v in ex.infer({name: x}).items()}
        if mode == '2':
            handed = G.nodes[pid].get('_pooled_in')
            assert handed is not None and tuple(handed.shape) == (4, 64, 56, 56)
        eager_ports = _ports(net)
        ex.capture_graph({name: hip.DeviceTensor.from_numpy(x)})
        replayed = {k_: np.asarray(v) for k_, v in ex.infer_graph().items()}
        runs[mode] = (eager, eager_ports, replayed, _ports(net))
        ex.release_graph()
    helpers.setenv(monkeypatch, 'PVHIP_FUSE_STEM_POOL', None)
    off, on = runs['0'], runs['2']
    assert sorted(off[0]) == sorted(on[0]) and len(off[1]) > 50
    for k_ in off[0]:
        assert_bit_exact(on[0][k_], off[0][k_], 'Result {} eager'.format(k_))
        assert_bit_exact(on[2][k_], off[2][k_], 'Result {} replayed'.format(k_))
        assert_bit_exact(on[2][k_], off[0][k_], 'Result {} replayed vs eager'.format(k_))
    for which, what in ((1, 'eager'), (3, 'replayed')):
        assert sorted(on[which]) == sorted(off[which])
        for nid in off[which]:
            assert_bit_exact(on[which][nid], off[which][nid], 'port of node {} {}'.format(nid, what))


@pytest.mark.gpu
def test_recording_keeps_the_pooled_tensor_alive(hip, monkeypatch):
    """A recording holds the address of the pooled tensor conv1 handed to pool1, which lies on no port: an eager pass beside the recording drops
    the hint, and the block must not go back to the pool (pool1's own output of the same size would take it).  Capture, one eager infer() of
    another input, replay: the replay's Results are the first input's, and the eager pass's ports are untouched by the replay."""
    from pyopenvino_amd import synth
    helpers.setenv(monkeypatch, 'PVHIP_FUSE_STEM_POOL', '2')
    _, net, ex = build_network(HIP, 'googlenet-v1', weights=synth.synth_weights(GOOGLENET, 1234), batch=4)
    name = net.inputs[0]['name']
    x1, x2 = (np.concatenate([synth.uniform_pixels(s + i, (1, 3, 224, 224)) for i in range(4)], 0) for s in (500, 600))
    want1 = {k_: np.asarray(v) for k_, v in ex.infer({name: x1}).items()}
    ex.capture_graph({name: hip.DeviceTensor.from_numpy(x1)})
    (cid, pid), = ex.plan.stem_pool.items()
    handed = net.G.nodes[pid]['_pooled_in']
    assert any(t is handed for t in ex._graph['keep'])
    want2 = {k_: np.asarray(v) for k_, v in ex.infer({name: x2}).items()}          # eager: the recording was made by hand
    assert net.G.nodes[pid]['_pooled_in'] is not handed
    ports2 = _ports(net)
    held = {nid: next(iter(net.G.nodes[nid]['output'].values()))['data'] for nid in ports2}      # the eager pass's tensors themselves
    replayed = {k_: np.asarray(v) for k_, v in ex.infer_graph().items()}
    for k_ in want1:
        assert not np.array_equal(want1[k_], want2[k_])
        assert_bit_exact(replayed[k_], want1[k_], 'Result {} replayed after an eager pass'.format(k_))
    for nid, t in held.items():
        assert_bit_exact(np.array(t), ports2[nid], 'port of node {} of the eager pass, after the replay'.format(nid))
    ex.release_graph()
    helpers.setenv(monkeypatch, 'PVHIP_FUSE_STEM_POOL', None)


FIELDS = ('_fusion', '_fused_away', '_concat_direct', '_lrn_pool', '_siblings', '_pool_conv', '_pre_add', '_stem_conv', '_c8_out', '_c8_concat', '_c8_entry')


@pytest.mark.parametrize('name,mode,want', [('googlenet', '2', True), ('googlenet', '0', False), ('googlenet', None, False),
                                            ('googlenet_fp16_c8_2', '2', False), ('ssd', '2', False)])
def test_plan_field_stem_pool(monkeypatch, name, mode, want):
    """`stem_pool` = {conv1: pool1} for fp32 GoogLeNet where the switch allows it (batch 8 is below the size rule of the default), empty
    for the FP16 IR and for SSD -- and every pinned field of the plan is the committed snapshot's whatever the switch says."""
    import json
    import test_fusion_plan as tfp
    helpers.setenv(monkeypatch, 'PVHIP_FUSE_STEM_POOL', mode)
    model, fp16, env, fuse = tfp.CONFIGS[name]
    for var in ('PVHIP_SCHEDULE_LOCALITY', 'PVHIP_FUSE_SIBLINGS', 'PVHIP_FUSE_POOLCONV', 'PVHIP_FUSE_STEM_CONV', 'PVHIP_CONV_F16_C8'):
        helpers.setenv(monkeypatch, var, env.get(var))
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        ie, net = tfp._network(model, fp16, tmp)
        net.set_batch(8)
        ex = ie.load_network(net)
    G = net.G
    if want:
        (cid, pid), = ex.plan.stem_pool.items()
        assert G.nodes[cid]['name'].startswith('conv1/7x7_s2') and G.nodes[pid]['name'].startswith('pool1/3x3_s2')
        assert ex._stem_conv[pid] and ex._lrn_pool[pid] and ex._stem_pool is ex.plan.stem_pool
    else:
        assert ex.plan.stem_pool == {}
    with open(tfp.SNAPSHOT) as f:
        snap = json.load(f)[name]
    assert tfp._plain({'task_list': ex.task_list}) == {'task_list': snap['task_list']}
    for field in FIELDS:
        assert tfp._plain(getattr(ex, field)) == snap[field], (name, mode, field)


def test_plan_field_stem_pool_follows_the_size_rule(monkeypatch):
    """The default (PVHIP_FUSE_STEM_POOL=1) takes the fold where every CU walks at least eight tiles of conv1: batch 256 (28 each), not batch 64."""
    import test_fusion_plan as tfp
    import tempfile
    helpers.setenv(monkeypatch, 'PVHIP_FUSE_STEM_POOL', None)
    for batch, want in ((256, 1), (64, 0)):
        with tempfile.TemporaryDirectory() as tmp:
            ie, net = tfp._network(GOOGLENET, False, tmp)
            net.set_batch(batch)
            ex = ie.load_network(net)
        assert len(ex.plan.stem_pool) == want, batch
