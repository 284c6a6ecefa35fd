"""Float64 reference of the ops GoogLeNet and SSD-MobileNet use, the fused groups of an execution plan, and the layer-by-layer check
of a whole pass.  A helper module the tests import.

The semantics are those of the reference's 'special' path as oracle/ops.py restates them: im2col convolution,
depthwise GroupConvolution with the same padding rules, MaxPool over the zero-padded input with ceil / floor rounding, AvgPool over
the window clipped at h-1 / w-1, LRN with alpha NOT divided by size, SoftMax without a max shift, Multiply with the smaller operand
broadcast, Sigmoid as 1 / (1 + exp(-x)).  DetectionOutput has no float64 definition here: its kernels follow the reference's float32
rules, so the layer check holds it against the oracle fed the pass's own inputs (`check_detections`).  Unlike the oracle, which rounds to float32 on purpose, every intermediate here is
float64: it is the yardstick the fp32 / fp16 kernels are held against, not a restatement of the reference's rounding.

`groups(ex)` reads an Executable_Network's fusion plan and returns, for every launch, the node ids it computes, the ports that
hold its real input tensors and the one port that holds its real output.  Ports that hold only a placeholder (the convolution /
Add ports of a fused chain, the MaxPool / LRN ports folded into the stem-convolution launch, the LRN port of LRN + MaxPool) are
never named.  `eval_group` recomputes a group from its input tensors; `check_group` is the comparison the tests apply."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from oracle.ops import out_extent


# the 32 images of a batch of 256 the layer checks compare: 0-7 (the rows googlenet_rows8.npz pins), 248-255 (the last tiles of every
# persistent walk) and 16 seeded positions in between
SAMPLE_256 = sorted(set(range(8)) | set(range(248, 256)) |
                    set(int(i) for i in np.random.default_rng(256).choice(np.arange(8, 248), 16, replace=False)))
# the same for a batch of 128 (SSD-MobileNet): 0-7, 120-127 (the last tiles of every persistent walk; 127 is the image the SSD fixture
# pins) and 16 seeded positions in between
SAMPLE_128 = sorted(set(range(8)) | set(range(120, 128)) |
                    set(int(i) for i in np.random.default_rng(128).choice(np.arange(8, 120), 16, replace=False)))

MIN_SAMPLE = 12         # sample() never returns fewer images than this (or the whole batch)


def sample(n, first=8, last=8, between=16):
    """The images of a batch of n a layer check compares: the first `first` (image 0 always), the last `last` (the last tiles of every
    walk) and `between` positions in between, drawn by default_rng(n); the whole batch when n <= 16.  The defaults are the counts of
    SAMPLE_256 / SAMPLE_128, which sample(256) / sample(128) reproduce.  Whatever the counts: both ends, and at least MIN_SAMPLE images."""
    n = int(n)
    if n <= 16:
        return list(range(n))
    if first < 1 or last < 1 or between < 0:
        raise ValueError('a sample holds both ends of the batch')
    lo, hi = min(first, n), max(n - last, 0)
    gap = np.arange(lo, hi)
    mid = np.random.default_rng(n).choice(gap, min(between, len(gap)), replace=False) if len(gap) else ()
    out = sorted(set(range(lo)) | set(range(hi, n)) | set(int(i) for i in mid))
    if len(out) < MIN_SAMPLE:
        raise ValueError('{} images of a batch of {}: a sample holds at least {}'.format(len(out), n, MIN_SAMPLE))
    assert out[0] == 0 and out[-1] == n - 1
    return out


# SSD-MobileNet's prior-box subgraph: per feature map the two ShapeOf -> StridedSlice shape vectors, PriorBoxClustered (its boxes computed
# once on the host and cached on the device) and the Unsqueeze; then the Concat of the six.  Its values depend on shapes only.
SSD_PRIOR_BOX_SUBGRAPH = sorted(['PriorBoxClustered_{}{}'.format(k, s_) for k in range(6)
                                 for s_ in ('/0_port', '/ss_0_port', '/1_port', '/ss_1_port', '/naked_not_unsqueezed', '')] +
                                ['ConcatPriorBoxesClustered'])


def _ints(s):
    return tuple(int(v) for v in str(s).replace(' ', '').split(',') if v != '')


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def convolution(x, w, strides, pads_begin, pads_end, auto_pad='explicit', chunk_bytes=1 << 26):
    """im2col + one float64 GEMM per chunk of images (the column matrix of a chunk stays below `chunk_bytes`)."""
    x, w = _f64(x), _f64(w)
    n, c, h, wd = x.shape
    kn, kc, kh, kw = w.shape
    assert kc == c, 'weights for {} channels, input has {}'.format(kc, c)
    sh, sw = strides
    oh = out_extent(h, kh, sh, pads_begin[0], pads_end[0], 'floor', auto_pad, False)
    ow = out_extent(wd, kw, sw, pads_begin[1], pads_end[1], 'floor', auto_pad, False)
    xp = np.pad(x, [(0, 0), (0, 0), (pads_begin[0], pads_end[0]), (pads_begin[1], pads_end[1])])
    wm = w.reshape(kn, -1).T                                              # (c*kh*kw, kn)
    out = np.empty((n, kn, oh, ow), dtype=np.float64)
    per_image = oh * ow * c * kh * kw * 8
    step = max(1, int(chunk_bytes // max(per_image, 1)))
    for i0 in range(0, n, step):
        xs = xp[i0:i0 + step]
        m = xs.shape[0]
        win = sliding_window_view(xs, (kh, kw), axis=(2, 3))[:, :, ::sh, ::sw][:, :, :oh, :ow]       # m,c,oh,ow,kh,kw
        col = np.ascontiguousarray(win.transpose(0, 2, 3, 1, 4, 5)).reshape(m * oh * ow, c * kh * kw)
        out[i0:i0 + m] = (col @ wm).reshape(m, oh, ow, kn).transpose(0, 3, 1, 2)
    return out


def group_convolution_depthwise(x, w, strides, pads_begin, pads_end, auto_pad='explicit'):
    """Weights [G,1,1,kh,kw], G == C: one kh x kw filter per channel over the zero-padded input, with the output extent and padding
    rules of `convolution` (same_upper / same_lower keep the IR's pads; SSD's stride-2 layers pad 0 at the beginning, 1 at the end).
    Summed tap by tap, so no (n, c, oh, ow, kh, kw) window array is ever built."""
    x, w = _f64(x), _f64(w)
    n, c, h, wd = x.shape
    g, co, ci, kh, kw = w.shape
    assert co == 1 and ci == 1 and g == c, 'depthwise weights {} for {} channels'.format(w.shape, c)
    sh, sw = strides
    oh = out_extent(h, kh, sh, pads_begin[0], pads_end[0], 'floor', auto_pad, False)
    ow = out_extent(wd, kw, sw, pads_begin[1], pads_end[1], 'floor', auto_pad, False)
    xp = np.pad(x, [(0, 0), (0, 0), (pads_begin[0], pads_end[0]), (pads_begin[1], pads_end[1])])
    assert (oh - 1) * sh + kh <= xp.shape[2] and (ow - 1) * sw + kw <= xp.shape[3], 'window exceeds the padded input'
    out = np.zeros((n, c, oh, ow))
    for ky in range(kh):
        for kx in range(kw):
            out += xp[:, :, ky:ky + (oh - 1) * sh + 1:sh, kx:kx + (ow - 1) * sw + 1:sw] * w[:, 0, 0, ky, kx].reshape(1, c, 1, 1)
    return out


def maxpool(x, strides, pads_begin, pads_end, kernel, rounding_type, auto_pad='explicit'):
    """Zero padding takes part in the max; windows are clipped at the padded extent (ceil rounding can run past it)."""
    x = _f64(x)
    n, c, h, wd = x.shape
    sh, sw = strides
    kh, kw = kernel
    oh = out_extent(h, kh, sh, pads_begin[0], pads_end[0], rounding_type, auto_pad, True)
    ow = out_extent(wd, kw, sw, pads_begin[1], pads_end[1], rounding_type, auto_pad, True)
    xp = np.pad(x, [(0, 0), (0, 0), (pads_begin[0], pads_end[0]), (pads_begin[1], pads_end[1])])
    hp, wp = xp.shape[2:]
    out = np.full((n, c, oh, ow), -np.inf)
    for y in range(oh):
        y0, y1 = y * sh, min(y * sh + kh, hp)
        for xx in range(ow):
            x0, x1 = xx * sw, min(xx * sw + kw, wp)
            out[:, :, y, xx] = xp[:, :, y0:y1, x0:x1].max(axis=(2, 3))
    return out


def avgpool(x, strides, pads_begin, pads_end, kernel, rounding_type, auto_pad='explicit'):
    """No padding; the window is clipped at h-1 / w-1 (the reference's AvgPool quirk); an empty window gives NaN."""
    x = _f64(x)
    n, c, h, wd = x.shape
    sh, sw = strides
    kh, kw = kernel
    oh = out_extent(h, kh, sh, pads_begin[0], pads_end[0], rounding_type, auto_pad, True)
    ow = out_extent(wd, kw, sw, pads_begin[1], pads_end[1], rounding_type, auto_pad, True)
    out = np.empty((n, c, oh, ow))
    for y in range(oh):
        for xx in range(ow):
            patch = x[:, :, y * sh:min(h - 1, y * sh + kh), xx * sw:min(wd - 1, xx * sw + kw)]
            out[:, :, y, xx] = np.nan if patch.size == 0 else patch.mean(axis=(2, 3))
    return out


def lrn(x, alpha, beta, bias, size):
    """Across channels: window [c - size//2, c + size//2] clipped to the channel range, alpha not divided by size."""
    x = _f64(x)
    c = x.shape[1]
    half = size // 2
    sq = x * x
    acc = np.zeros_like(x)
    for k in range(c):
        acc[:, k] = sq[:, max(0, k - half):min(c, k + half + 1)].sum(axis=1)
    return x / (bias + alpha * acc) ** beta


def add(a, b):
    a, b = _f64(a), _f64(b)
    return a + np.broadcast_to(b, a.shape)


def multiply(a, b):
    """The smaller operand broadcasts to the larger (the reference's rule)."""
    a, b = _f64(a), _f64(b)
    if a.size > b.size:
        return a * np.broadcast_to(b, a.shape)
    return np.broadcast_to(a, b.shape) * b


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-_f64(x)))


def transpose(x, order):
    return np.ascontiguousarray(_f64(x).transpose(tuple(int(v) for v in np.asarray(order).ravel())))


def relu(x):
    x = _f64(x)
    return np.where(x < 0, 0.0, x)


def clamp(x, lo, hi):
    return np.clip(_f64(x), lo, hi)


def concat(parts, axis):
    return np.concatenate([_f64(p) for p in parts], axis=axis)


def matmul(a, b, transpose_a=False, transpose_b=False):
    a, b = _f64(a), _f64(b)
    return (a.T if transpose_a else a) @ (b.T if transpose_b else b)


def pad2d(x, pads_begin, pads_end, channel_add=None):
    """pvhip_pad2d_f32: the zero-padded image Convolution.py:64-66 builds; channel_add (c values) is added to every element of x on the
    way, never to the padding."""
    x = _f64(x)
    if channel_add is not None:
        x = x + _f64(channel_add).reshape(1, -1, 1, 1)
    return np.pad(x, [(0, 0), (0, 0), (pads_begin[0], pads_end[0]), (pads_begin[1], pads_end[1])])


def u8_to_f32(x):
    """The widening copy of a U8 input: every uint8 value is an fp32 (and a float64) value."""
    x = np.asarray(x)
    assert x.dtype == np.uint8
    return x.astype(np.float64)


def nhwc_to_nchw(x):
    """(n, h, w, c) uint8 or fp32 -> (n, c, h, w); values are moved, never computed on."""
    x = np.asarray(x)
    assert x.ndim == 4 and x.dtype in (np.uint8, np.float32)
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2)).astype(np.float64)


def c8_blocks(c):
    """Channel blocks of eight of a c8 tensor: whole 16-channel stages (include/pvhip.h pvhip_c8_f16_*)."""
    return (int(c) + 15) // 16 * 2


def c8_pack(x):
    """pvhip_c8_f16_from_f32 restated: (n, c, h, w) fp32 -> float16 [n][c8_blocks(c)][h * w][8], round to nearest even (numpy's
    astype(np.float16)), channels c .. 16 * ceil(c / 16) - 1 are +0."""
    x = np.asarray(x, dtype=np.float32)
    n, c, h, w = x.shape
    cb = c8_blocks(c)
    full = np.zeros((n, cb * 8, h * w), dtype=np.float16)
    with np.errstate(over='ignore'):
        full[:, :c] = x.reshape(n, c, h * w).astype(np.float16)
    return np.ascontiguousarray(full.reshape(n, cb, 8, h * w).transpose(0, 1, 3, 2))


def c8_unpack(xb, c):
    """pvhip_c8_f16_to_f32 restated: the first c channels of a c8 tensor as (n, c, h * w) fp32 (exact: every fp16 value is an fp32 value)."""
    xb = np.asarray(xb)
    assert xb.dtype == np.float16 and xb.ndim == 4 and xb.shape[3] == 8
    n, cb, hw, _ = xb.shape
    return np.ascontiguousarray(xb.transpose(0, 1, 3, 2).reshape(n, cb * 8, hw)[:, :c]).astype(np.float32)


def f16_fragments(w):
    """pvhip_conv2d_f16_c8_pack / pvhip_conv2d_f16_span_pack restated: (k, c, ks, ks) fp32 weights -> the float16 MFMA fragment panel
    [mt][cs][tap][i][lane][q] (csrc/pvhip_f16_c8.h).  Output channels come in groups of up to 128 (mt), a group in tm 32-channel tiles
    (i), the same tm for every group; the input channels in stages of 16 (cs), c padded to whole stages.  Lane `lane` of fragment
    (mt, cs, tap, i) holds, as q = 0 .. 7, output channel (mt * tm + i) * 32 + lane % 32 at input channels cs * 16 + 8 * (lane // 32) + q
    of window tap `tap`; channels past k and past c are +0."""
    w = np.asarray(w, dtype=np.float32)
    k, c, kh, kw = w.shape
    taps = kh * kw
    nm = (k + 127) // 128
    tm = -(-(-(-k // 32)) // nm)
    ncs = (c + 15) // 16
    full = np.zeros((nm * tm * 32, ncs * 16, taps), dtype=np.float16)
    with np.errstate(over='ignore'):
        full[:k, :c] = w.reshape(k, c, taps).astype(np.float16)
    # [mt][i][lane % 32][cs][lane // 32][q][tap] -> [mt][cs][tap][i][lane // 32][lane % 32][q]
    panel = full.reshape(nm, tm, 32, ncs, 2, 8, taps).transpose(0, 3, 6, 1, 4, 2, 5)
    return np.ascontiguousarray(panel).reshape(nm, ncs, taps, tm, 64, 8)


def softmax_rows(x):
    """Per leading-axis row, no max shift."""
    x = _f64(x)
    flat = x.reshape(x.shape[0] if x.ndim > 1 else 1, -1)
    e = np.exp(flat)
    return (e / e.sum(axis=1, keepdims=True)).reshape(x.shape)


# ---------------------------------------------------------------------------------------------------------------------
# one IR node, from its inputs in sink-port order (float64; f16: Convolution / MatMul operands rounded to fp16 first -- not those of a
# GroupConvolution: an FP16 IR runs depthwise on the fp32 kernel, on weights that already hold fp16 values)
def f16r(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float64)


def eval_node(node, ins, f16=False):
    t, a = node['type'], node.get('data') or {}
    if t == 'Convolution':
        x, w = (f16r(ins[0]), f16r(ins[1])) if f16 else (ins[0], ins[1])
        return convolution(x, w, _ints(a['strides']), _ints(a['pads_begin']), _ints(a['pads_end']), a['auto_pad'])
    if t == 'GroupConvolution':
        return group_convolution_depthwise(ins[0], ins[1], _ints(a['strides']), _ints(a['pads_begin']), _ints(a['pads_end']), a['auto_pad'])
    if t == 'MaxPool':
        return maxpool(ins[0], _ints(a['strides']), _ints(a['pads_begin']), _ints(a['pads_end']), _ints(a['kernel']), a['rounding_type'],
                       a['auto_pad'])
    if t == 'AvgPool':
        return avgpool(ins[0], _ints(a['strides']), _ints(a['pads_begin']), _ints(a['pads_end']), _ints(a['kernel']), a['rounding_type'],
                       a['auto_pad'])
    if t == 'LRN':
        return lrn(ins[0], float(a['alpha']), float(a['beta']), float(a['bias']), int(a['size']))
    if t == 'Add':
        return add(ins[0], ins[1])
    if t == 'Multiply':
        return multiply(ins[0], ins[1])
    if t == 'Sigmoid':
        return sigmoid(ins[0])
    if t == 'Transpose':
        return transpose(ins[0], ins[1])
    if t == 'ReLU':
        return relu(ins[0])
    if t == 'Clamp':
        return clamp(ins[0], float(a['min']), float(a['max']))
    if t == 'Concat':
        return concat(ins, int(a['axis']))
    if t == 'MatMul':
        x, w = (f16r(ins[0]), f16r(ins[1])) if f16 else (ins[0], ins[1])
        return matmul(x, w, a.get('transpose_a') == 'true', a.get('transpose_b') == 'true')
    if t == 'SoftMax':
        return softmax_rows(ins[0])
    if t == 'Reshape':                 # the batch stays the leading axis (the sampled images are a subset of it; set_batch scales it)
        dims = tuple(next(iter(node['output'].values()))['dims'])
        return _f64(ins[0]).reshape((ins[0].shape[0],) + dims[1:])
    raise NotImplementedError(t)


# ---------------------------------------------------------------------------------------------------------------------
# the fused groups of a plan
def _chain(ex, cid):
    f = ex._fusion[cid]
    return [cid] + [n for n in (f['add'], f['relu']) if n is not None]


def _port(G, nid):
    return (nid, next(iter(G.nodes[nid]['output'])))


def groups(ex):
    """[{'launch': id of the dispatched task, 'nodes': [ids in evaluation order], 'inputs': [(node id, port)], 'output': (node id, port),
    'convs': [Convolution ids]}] in schedule order, one entry per tensor a launch writes (a sibling launch gives one per member).  Channel
    Concats written in place (`_concat_direct`) are not launches: their members' outputs are ChannelSlices of the Concat's tensor."""
    G = ex.ienet.G
    out = []
    stem_of = dict(ex._stem_conv)
    for t in ex.task_list:
        node = G.nodes[t]
        if node['type'] in ('Const', 'Parameter', 'Result') or t in ex._fused_away:
            continue
        members = []
        if t in ex._fusion:
            members = [t] + list(ex._siblings.get(t, ()))
        elif t in stem_of:
            lid = ex._lrn_pool[t]
            members = [(t, lid, stem_of[t])]
        if members and not isinstance(members[0], tuple):
            for cid in members:
                nodes = []
                if cid in ex._pre_add:
                    nodes.append(ex._pre_add[cid][0])
                if cid in ex._pool_conv:
                    nodes.append(ex._pool_conv[cid][0])
                nodes += _chain(ex, cid)
                out.append(_group(G, t, nodes))
        elif members:
            pid, lid, cid = members[0]
            out.append(_group(G, t, [pid, lid] + _chain(ex, cid)))
        elif t in ex._lrn_pool:
            out.append(_group(G, t, [t, ex._lrn_pool[t]]))
        else:
            out.append(_group(G, t, [t]))
    return out


def _group(G, launch, nodes):
    inside = set(nodes)
    inputs = []
    for nid in nodes:
        for p in sorted(G.pred[nid], key=lambda p: G.edges[(p, nid)]['connection'][3]):
            src = tuple(G.edges[(p, nid)]['connection'][:2])
            if src[0] not in inside and G.nodes[src[0]]['type'] != 'Const' and src not in inputs:
                inputs.append(src)
    return {'launch': launch, 'nodes': list(nodes), 'inputs': inputs, 'output': _port(G, nodes[-1]),
            'convs': [n for n in nodes if G.nodes[n]['type'] == 'Convolution']}


def const_value(G, nid, port=0):
    """A Const's values from the IR's weight blob (not from the device copy a plugin made of them)."""
    node = G.nodes[nid]
    dt = {'f32': np.float32, 'f16': np.float16, 'i64': np.int64, 'i32': np.int32}[node['data']['element_type']]
    return _f64(np.asarray(node['const']['data']).view(dt).reshape(tuple(int(d) for d in ref64_shape(node['data']['shape']))))


def ref64_shape(shape):
    return _ints(shape) if isinstance(shape, str) else tuple(shape)


def eval_group(G, group, inputs, f16=False, consts=None):
    """The group in float64.  `inputs` = {(node id, port): array of the sampled images}; Consts are read from the graph (`consts`: a
    cache {(node id, port): float64 array} shared across groups).  f16: Convolution / MatMul operands rounded to fp16 (the f16 matrix
    cores' operands), everything else float64."""
    consts = {} if consts is None else consts
    vals = dict(inputs)
    for nid in group['nodes']:
        node = G.nodes[nid]
        ins = []
        for p in sorted(G.pred[nid], key=lambda p: G.edges[(p, nid)]['connection'][3]):
            src = tuple(G.edges[(p, nid)]['connection'][:2])
            if G.nodes[src[0]]['type'] == 'Const':
                if src not in consts:
                    consts[src] = const_value(G, *src)
                ins.append(consts[src])
            else:
                ins.append(vals[src])
        if node['type'] == 'LRN':
            ins = ins[:1]
        vals[_port(G, nid)] = eval_node(node, ins, f16)
    return vals[group['output']]


# ---------------------------------------------------------------------------------------------------------------------
# the comparison
DRIFT = 2e-5             # max-norm bound of the fp32 kernels without a Winograd transform (the per-op fixture test's)


def check_group(got, ref, winograd=False, what=''):
    """fp32 output vs the float64 reference: helpers.assert_close at REL_TOL (max-norm and element by element), and the 2e-5
    max-norm drift bound unless a Winograd transform is in the launch.  Returns the element-wise excess."""
    import helpers
    helpers.assert_close(got, ref, helpers.REL_TOL, what)
    if not winograd:
        err = helpers.rel_err(got, ref)
        assert err <= DRIFT, '{}: max-norm error {:.2e} > {:.0e}'.format(what, err, DRIFT)
    return helpers.elementwise_excess(got, ref)


def f16_excess(got, ref, slack=None):
    """max over elements of |got - ref| / (2**-11 |ref| + 1e-5 (|ref| + rms(ref)) [+ slack]): <= 1 is one fp16 rounding of an
    fp32-accumulated value.  `slack` (elementwise, >= 0): what roundings inside the launch may add (an operand the launch itself rounds
    to fp16 from a value the reference has in float64)."""
    got, ref = _f64(got), _f64(ref)
    assert got.shape == ref.shape, '{} != {}'.format(got.shape, ref.shape)
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    rms = float(np.sqrt(np.mean(ref * ref)))
    bound = 2.0 ** -11 * np.abs(ref) + 1e-5 * (np.abs(ref) + max(rms, 1e-30))
    if slack is not None:
        bound = bound + slack
    return float((np.abs(got - ref) / bound).max())


# ---------------------------------------------------------------------------------------------------------------------
# the layer-by-layer check of a whole pass (tests/test_batch256_layers.py, tests/test_ssd_layers.py)
WINO4S, WINO4S_RAGGED, WINO4, WINO4_RAGGED = 'conv_wino4s_kernel', 'conv_wino4s_kernel, ragged', 'conv_wino4_kernel', 'conv_wino4_kernel, ragged'


def wino4_form(node):
    """wino4_conv's choice for a six-point Winograd layer (pvhip_wino.hip, default settings), from the port dims."""
    n, c, h, w = node['input'][0]['dims']
    k, _, kh, _ = node['input'][1]['dims']
    m = 4 if kh == 3 else 2
    ragged = h % m != 0 or w % m != 0
    n_tb, n_kb, stages = -(-(n * -(-h // m) * -(-w // m)) // 32), -(-k // 32), c // 4
    tiles_s = n_tb * ((n_kb + 1) // 2)
    shape_ok = n_kb >= 2 and stages % 4 == 0 and stages >= 4
    pays = stages >= 28 or (stages >= 24 and ragged) or (12 <= stages <= 16 and tiles_s >= 2048)
    return (WINO4S if shape_ok and pays else WINO4) + (', ragged' if ragged else '')


# pvhip_conv2d_form (include/pvhip.h: PVHIP_CONV_FORM_*, PVHIP_IGEMM_*): the form inside the family, as the library reports it
CONV_ENTRIES = {'pvhip_conv2d_f32': 0, 'pvhip_conv2d_multi_f32': 0, 'pvhip_conv2d_f16_dma': 1, 'pvhip_conv2d_multi_f16_dma': 1}
IGEMM_KERNELS = {0: 'reg', 1: 'pw', 2: 'rs', 3: 'cvalid', 4: 'cwindow'}


def conv_form(entry, n, c, h, w, k, kh, kw, oh, ow, sh, sw, pt, pl):
    """The form string of one launch (entry 0: pvhip_conv2d_f32 / the pointwise route of pvhip_conv2d_multi_f32, 1: the f16 LDS-DMA
    entries; k: the panel width of a multi-destination launch), 'none' for an empty output.  Host-only: no device needed."""
    import ctypes
    from pyopenvino_amd import device
    f = (ctypes.c_int * 16)()
    device.call('pvhip_conv2d_form', entry, n, c, h, w, k, kh, kw, oh, ow, sh, sw, pt, pl, f)
    kind, grid = f[0], f[1]
    if kind == -1:
        return 'none'
    if kind == 1:
        return 'pw tn={} vec={} nchunk={} stagger={} grid={}'.format(f[2], f[3], f[4], f[5], grid)
    if kind == 2:
        return 'wino2 kb={} patches={} waves={} grid={}'.format(f[2], f[3], f[4], grid)
    if kind in (3, 4):
        assert f[2] == (4 if kind == 3 else 2)
        return 'wino4 m={} ragged={} shared={} order={} tiles={} grid={} walk={}'.format(f[2], f[3], f[4], f[5], f[6], grid, f[7])
    assert kind == 0, kind
    return '{} bm={} kernel={} mtiles={} grid={}'.format('f16' if entry else 'igemm', f[2], IGEMM_KERNELS[f[3]], f[4], grid)


def launch_args(G, plan, cid, r):
    """The arguments of conv_form for the launch the Route `r` gives Convolution node `cid`: the geometry the library is handed (behind
    the padding pass, if the route has one) and, for a sibling launch, the panel width.  None: an entry the query does not cover."""
    from pyopenvino_amd.op_plugins import Convolution
    if r.entry not in CONV_ENTRIES:
        return None
    g = Convolution.geometry(G.nodes[cid])
    h, w, pads, k = g.h, g.w, g.pads_begin, g.kn
    if r.pad_row:
        h, w, pads = g.h + g.pads_begin[0] + g.pads_end[0], r.pad_row, (0, 0)
    if 'multi' in r.entry:
        k = sum(-(-int(G.nodes[m]['input'][1]['dims'][0]) // 32) * 32 for m in [cid] + list(plan.siblings.get(cid, ())))
        if not CONV_ENTRIES[r.entry] and Convolution.kernel_kind(G.nodes[cid])[0] != 'pointwise':
            return None                 # the fp32 multi launch with PVHIP_CONV_POINTWISE=0
    return (CONV_ENTRIES[r.entry], g.n, g.c, h, w, k, g.kh, g.kw, g.oh, g.ow, *g.strides, *pads)


def wino4_form_of(form):
    """The restatement's name (WINO4S ...) of a queried six-point form string."""
    f = dict(v.split('=') for v in form.split()[1:])
    return (WINO4S if f['shared'] == '1' else WINO4) + (', ragged' if f['ragged'] == '1' else '')


def read_rows(t, idx):
    """The sampled images of a tensor, as fp32 (BlockedHalf: the fp32 values of its fp16 contents).  Dense device tensors are read image
    by image: only what is compared crosses to the host."""
    from pyopenvino_amd import device as dev
    import ctypes
    if isinstance(t, np.ndarray):
        return np.ascontiguousarray(t[idx], dtype=np.float32)
    if isinstance(t, (dev.ChannelSlice, dev.BlockedChannelSlice)):
        base = read_rows(t.base, idx)
        return np.ascontiguousarray(base[:, t.coff:t.coff + t.shape[1]])
    if isinstance(t, dev.BlockedHalf):
        return read_rows(t.dense(), idx)
    assert isinstance(t, dev.DeviceTensor) and t.dtype == np.float32, type(t)
    per = int(np.prod(t.shape[1:], dtype=np.int64))
    out = np.empty((len(idx),) + tuple(t.shape[1:]), dtype=np.float32)
    for j, i in enumerate(idx):
        assert 0 <= i < t.shape[0]
        dev.call('pvhip_memcpy_d2h', ctypes.c_void_p(out[j].ctypes.data), ctypes.c_void_p(t.ptr + int(i) * per * 4), per * 4)
    return out


def conv_family(node):
    from pyopenvino_amd.op_plugins import Convolution
    return Convolution.kernel_kind(node)[0]


def family(G, ex, g):
    convs = g['convs']
    if not convs:
        return ' + '.join(G.nodes[n]['type'] for n in g['nodes'])
    node = G.nodes[convs[-1]]
    f16_kind = node.get('_hip_f16') or G.nodes[g['launch']].get('_hip_f16')        # FP16 IRs: what the launch's kernel recorded
    fam = 'f16 ' + f16_kind if f16_kind else conv_family(node)
    if fam in ('Winograd F(4x4,3x3)', 'Winograd F(2x2,5x5)'):         # the six-point layers (wino4_conv); F(2x2,3x3) has one form
        fam += ' / ' + wino4_form(node)
        route = node.get('_hip_route')
        if route is not None and route[1].entry == 'pvhip_conv2d_f32':      # what the launch took, by the library's own plan
            queried = conv_form(*launch_args(G, ex.plan, convs[-1], route[1]))
            assert fam.endswith(wino4_form_of(queried)), (node['name'], queried, fam)
    lead = [G.nodes[n]['type'] for n in g['nodes'] if n not in convs and G.nodes[n]['type'] in ('MaxPool', 'LRN')]
    return ' + '.join(lead + [fam])


def is_blocked(t):
    from pyopenvino_amd import device as dev
    return isinstance(t, (dev.BlockedHalf, dev.BlockedChannelSlice))


def port_data(G, src):
    return G.nodes[src[0]]['output'][src[1]]['data']


def check_pass(net, ex, sample, f16=False, only=None, skip=()):
    """Every group of the plan (`only`: the first groups of the schedule, by count; `skip`: launch ids the caller checks itself) against
    the float64 reference on the images `sample`.  -> {family: (worst excess, layer name)}."""
    import helpers
    G = net.G
    gs = groups(ex)
    if only is not None:
        gs = gs[:only]
    consts, worst, held = {}, {}, {}
    for g in gs:
        if g['launch'] in skip:
            continue
        ins = {src: held[src] if src in held else read_rows(port_data(G, src), sample) for src in g['inputs']}
        held = ins                                       # the members of a sibling launch share it; the previous launch's inputs go
        out_t = port_data(G, g['output'])
        got = read_rows(out_t, sample)
        name = G.nodes[g['nodes'][-1]]['name']
        fam = family(G, ex, g)
        ref = eval_group(G, g, ins, f16=f16, consts=consts)
        assert got.shape == ref.shape, '{}: {} != {}'.format(name, got.shape, ref.shape)
        assert np.isfinite(got).all(), '{}: non-finite values'.format(name)
        # fp16 outputs: blocked tensors, and the AvgPool of a blocked tensor (fp32 storage holding the fp16 values the reference's float16
        # AvgPool returns; tests/test_hip_ops.py::test_avgpool_on_a_blocked_tensor)
        fp16_out = is_blocked(out_t) or (G.nodes[g['nodes'][-1]]['type'] == 'AvgPool' and
                                         any(is_blocked(port_data(G, s_)) for s_ in g['inputs']))
        if f16 and fp16_out:
            slack = None
            if g['launch'] in ex._stem_conv:
                # pool1 -> norm1 -> conv2/3x3_reduce in one launch: the normalised tensor becomes an fp16 operand inside the launch, rounded
                # from the kernel's fp32 LRN, so each operand may sit one fp16 rounding away from f16r(float64 LRN)
                slack = _operand_slack(G, g, ins)
            ex_ = f16_excess(got, ref, slack)
            assert ex_ <= 1.0, '{} ({}): an element is {:.2f} x outside one fp16 rounding'.format(name, fam, ex_)
        elif f16:
            helpers.assert_close(got, ref, 1e-5, '{} ({})'.format(name, fam))
            ex_ = helpers.elementwise_excess(got, ref)
        else:
            wino = any('Winograd' in conv_family(G.nodes[c]) for c in g['convs'])
            ex_ = check_group(got, ref, winograd=wino, what='{} ({})'.format(name, fam))
        if ex_ >= worst.get(fam, (-1.0, ''))[0]:
            worst[fam] = (ex_, name)
        del got, ref
    return worst


def _operand_slack(G, g, ins):
    """2**-11 x (|W| * |x|), x the float64 input of the group's convolution: how far one fp16 rounding of each of its operands can move
    its output."""
    cid = g['convs'][0]
    k = g['nodes'].index(cid)
    feeder = g['nodes'][k - 1]
    x = eval_group(G, dict(g, nodes=g['nodes'][:k], output=(feeder, next(iter(G.nodes[feeder]['output'])))), ins)
    wsrc = next(tuple(G.edges[(p, cid)]['connection'][:2]) for p in G.pred[cid] if G.edges[(p, cid)]['connection'][3] == 1)
    a = G.nodes[cid]['data']
    return 2.0 ** -11 * convolution(np.abs(x), np.abs(const_value(G, *wsrc)), _ints(a['strides']), _ints(a['pads_begin']), _ints(a['pads_end']))


def report(worst, what):
    print('\n{}: worst element-wise excess per kernel family (<= 1 passes)'.format(what))
    for fam, (ex_, name) in sorted(worst.items(), key=lambda kv: -kv[1][0]):
        print('  {:8.4f}  {:60s} {}'.format(ex_, fam, name))


# ---------------------------------------------------------------------------------------------------------------------
# DetectionOutput: the oracle's float32 rules, fed the pass's own loc / conf rows and priors
NEAR_TIE = 1e-6          # two oracle scores this close (relative) may swap ranks between fp32 implementations


def _tie_runs(scores):
    """[(start, stop)] of the runs of adjacent records (descending score order) whose neighbours' scores lie within NEAR_TIE."""
    runs, i0 = [], 0
    for i in range(1, len(scores) + 1):
        if i == len(scores) or abs(scores[i] - scores[i - 1]) > NEAR_TIE * max(abs(scores[i]), abs(scores[i - 1]), 1e-30):
            if i - i0 > 1:
                runs.append((i0, i))
            i0 = i
    return runs


def compare_detections(got, want, what):
    """One image's records [n, class, score, xmin, ymin, xmax, ymax] (records x 7) against the oracle's: the record index and class
    columns bit for bit, score and boxes within REL_TOL; the records of a near-tie of the oracle's scores as a set.  -> the number of
    real detections."""
    import helpers
    got, want = np.array(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, '{}: {} != {}'.format(what, got.shape, want.shape)
    assert np.array_equal(got[:, 0], want[:, 0]), '{}: record index column differs (a different number of detections)'.format(what)
    real = int(np.argmax(want[:, 0] < 0)) if (want[:, 0] < 0).any() else len(want)
    for i0, i1 in _tie_runs(want[:real, 2]):
        for rows in (got[i0:i1], want[i0:i1]):
            rows[:] = rows[np.lexsort((rows[:, 4], rows[:, 3], rows[:, 1]))]
    assert np.array_equal(got[:, 1], want[:, 1]), '{}: classes differ'.format(what)
    helpers.assert_close(got[:, 2:], want[:, 2:], helpers.REL_TOL, what + ': scores / boxes')
    return real


def check_detections(net, sample):
    """The DetectionOutput node of `net` after a pass: each sampled image's records against the oracle's DetectionOutput fed the HIP
    pass's own loc / conf rows of that image and its priors (read whole: they are not per image).  Asserts every sampled image has
    real detections.  -> {image: number of detections}."""
    from oracle.op_plugins import DetectionOutput as oracle_do
    G = net.G
    did = next(n for n in G.nodes if G.nodes[n]['type'] == 'DetectionOutput')
    node = G.nodes[did]
    srcs = [tuple(G.edges[(p, did)]['connection'][:2]) for p in sorted(G.pred[did], key=lambda p: G.edges[(p, did)]['connection'][3])]
    loc, conf = (read_rows(port_data(G, s_), sample) for s_ in srcs[:2])
    priors = np.asarray(port_data(G, srcs[2]), dtype=np.float32)
    assert priors.shape[0] == 1, priors.shape
    out = np.asarray(next(iter(node['output'].values()))['data'])
    b = len(loc)
    ins = {0: loc, 1: conf, 2: priors}
    # the oracle validates its inputs against the node's ports: declare the sampled rows (fp32, whatever precision an FP16 IR declared)
    onode = dict(node, input={p: dict(node['input'][p], precision='FP32', dims=tuple(ins[p].shape)) for p in ins})
    want = next(iter(oracle_do.compute(onode, ins).values()))
    per = want.shape[2] // b
    assert out.shape[2] % per == 0
    counts = {}
    for j, i in enumerate(sample):
        counts[i] = compare_detections(out[0, 0, i * per:(i + 1) * per], want[0, 0, j * per:(j + 1) * per], 'DetectionOutput image {}'.format(i))
        assert counts[i] > 0 and out[0, 0, i * per, 1] > 0, 'image {}: no detections, the check would be vacuous'.format(i)
    return counts


# ---------------------------------------------------------------------------------------------------------------------
# the census of kernel forms per batch (tests/test_batch_forms.py; no device needed)
def launch_forms(net, ex, n):
    """{conv name: (family, wino4 form or None, Route)} of every Convolution launch of the plan `ex` holds, at batch n.  family:
    Convolution.kernel_kind's for an fp32 IR; 'f16 ' + the Route's label for an FP16 IR (what the launch leaves in node['_hip_f16'])."""
    import test_conv_routes
    from pyopenvino_amd.op_plugins import Convolution
    G, out = net.G, {}
    for cid, facts in test_conv_routes.launch_facts(ex).items():
        node = G.nodes[cid]
        assert node['input'][0]['dims'][0] == n, node['name']
        r = Convolution.route(*facts)
        fam, form = ('f16 ' + str(r.label), None) if ex.plan.f16 else (conv_family(node), None)
        if fam in ('Winograd F(4x4,3x3)', 'Winograd F(2x2,5x5)') and r.entry == 'pvhip_conv2d_f32':
            form = wino4_form(node)
            queried = conv_form(*launch_args(G, ex.plan, cid, r))          # the restatement and the library agree
            assert wino4_form_of(queried) == form, (node['name'], queried, form)
        out[node['name']] = (fam, form, r)
    return out


def queried_forms(net, ex):
    """{conv name: pvhip_conv2d_form's answer as a string, or None for an entry it does not cover} of the plan `ex` holds."""
    import test_conv_routes
    from pyopenvino_amd.op_plugins import Convolution
    G, out = net.G, {}
    for cid, facts in test_conv_routes.launch_facts(ex).items():
        args = launch_args(G, ex.plan, cid, Convolution.route(*facts))
        out[G.nodes[cid]['name']] = None if args is None else conv_form(*args)
    return out


class Census:
    """One loaded network whose batch is rewritten in place: at(n) sets the port dims to batch n with the network's own set_batch (from a
    snapshot of the batch-1 dims), rebuilds the fusion plan and asks the library what every Convolution launch of that plan takes."""

    def __init__(self, model, fp16, tmp_dir):
        from pyopenvino_amd import IECore, synth
        ie = IECore(plugin_package='pyopenvino_amd.op_plugins')
        blob = synth.synth_weights(model, 1234)
        if fp16:
            xml16, blob16 = synth.fp16_ir(model, blob, tmp_dir)
            self.net = ie.read_network(xml16, weights=blob16, fp16_as_fp32=False)
        else:
            self.net = ie.read_network(model, weights=blob)
        assert self.net.batch_size == 1
        self.fp16 = fp16
        self.ex = ie.load_network(self.net)
        G = self.net.G
        self._dims = {(nid, side, p): tuple(d['dims']) for nid in G.nodes for side in ('input', 'output')
                      for p, d in G.nodes[nid].get(side, {}).items()}
        self._shapes = {nid: tuple(G.nodes[nid]['data']['shape']) for nid in G.nodes if G.nodes[nid]['type'] == 'Parameter'}

    def at(self, n):
        """launch_forms of the plan at batch n."""
        G = self.net.G
        for (nid, side, p), dims in self._dims.items():
            G.nodes[nid][side][p]['dims'] = dims
        for nid, shape in self._shapes.items():
            G.nodes[nid]['data']['shape'] = shape
        self.net.batch_size = 1
        self.net.set_batch(n)
        self.ex.plan_fusion()
        return launch_forms(self.net, self.ex, n)


def census_classes(census, batches):
    """The sweep reduced to its breakpoints: ([(first batch of a class, {conv name: [family, wino4 form]})], whether any Route differs
    anywhere in the sweep).  A new class starts wherever any launch's entry (family, form or Route) differs from the batch before."""
    classes, first, last, routes_vary = [], None, None, False
    for n in batches:
        now = census.at(n)
        first = now if first is None else first
        routes_vary = routes_vary or {k: e[2] for k, e in now.items()} != {k: e[2] for k, e in first.items()}
        if now != last:
            classes.append((n, {name: [e[0], e[1]] for name, e in now.items()}))
            last = now
    return classes, routes_vary
