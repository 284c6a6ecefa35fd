"""Float64 reference of the ops GoogLeNet uses, and the fused groups of an execution plan.  A helper module the tests import.

The semantics are those of the reference's 'special' path as oracle/ops.py restates them: im2col convolution,
MaxPool over the zero-padded input with ceil / floor rounding, AvgPool over the window clipped at h-1 / w-1, LRN with alpha NOT
divided by size, SoftMax without a max shift.  Unlike the oracle, which rounds to float32 on purpose, every intermediate here is
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


def softmax_rows(x):
    """Per leading-axis row, no max shift."""
    x = _f64(x)
    flat = x.reshape(x.shape[0] if x.ndim > 1 else 1, -1)
    e = np.exp(flat)
    return (e / e.sum(axis=1, keepdims=True)).reshape(x.shape)


# ---------------------------------------------------------------------------------------------------------------------
# one IR node, from its inputs in sink-port order (float64; f16: Convolution / MatMul operands rounded to fp16 first)
def f16r(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float64)


def eval_node(node, ins, f16=False):
    t, a = node['type'], node.get('data') or {}
    if t == 'Convolution':
        x, w = (f16r(ins[0]), f16r(ins[1])) if f16 else (ins[0], ins[1])
        return convolution(x, w, _ints(a['strides']), _ints(a['pads_begin']), _ints(a['pads_end']), a['auto_pad'])
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
    if t == 'Reshape':                 # the batch stays the leading axis (the sampled images are a subset of it)
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
