# Convolution -- HIP plugin (implicit GEMM on the fp32 matrix cores).
# Replaces im2col + kernel_Convolution_im2col, the 'special' kernel (reference
# op_plugins/Convolution.py:57-87): zero padding by pads_begin/pads_end, output extent by
# calc_output_shape (:21-49) with 'floor', dilation ignored exactly as :72-87 ignores it.
import ctypes
from collections import namedtuple

import numpy as np

from .. import common_def
from .. import device as dev


# The engine may hand over a Convolution -> Add(per-channel Const) -> ReLU chain as one call: node['_fuse_bias']
# (DeviceTensor of K values) and node['_fuse_act'] = ('relu',) | ('clamp', lo, hi) are then applied in the kernel epilogue; node['_out_into'] =
# (tensor, channel offset) makes the kernel write its channels straight into the output of the channel Concat
# that consumes it.
SUPPORTS_FUSED_EPILOGUE = True
# Convolutions that read the same tensor (the 1x1 / 3x3_reduce / 5x5_reduce arms of an inception module) may be handed
# over as ONE call: node['_siblings'] = [{'node', 'inputs', 'bias', 'into'}, ...] lists the others (same attributes,
# same activation); the input is then read once, by one launch whose output-channel tiles store into the tensor of the
# convolution they belong to.  The siblings' outputs are left in node['_sibling_out'], in the same order.
SUPPORTS_SIBLINGS = True
# A 3x3 / stride 1 / pad 1 MaxPool whose only consumer is a 1x1 convolution (the pool -> pool_proj arm of an inception module) may
# be handed over with the convolution: node['_fuse_pool_in'] = the MaxPool's node dict, inputs[0] = the MaxPool's own input.  The
# kernel pools while it builds its input tile; the pooled tensor is never written.
SUPPORTS_POOLED_INPUT = True
# An Add of one fp32 constant per INPUT channel whose only consumer is a convolution that pads its input in a pass of its own (a layer
# with C % 16 != 0 and padding: GoogLeNet's data/mean -> conv1) may be handed over with the convolution: node['_pre_add'] = the constant
# (1, C, 1, 1), inputs[0] = the Add's own data input.  The padding pass adds it on the way (the same fp32 add: the same bits).
SUPPORTS_PRE_ADD = True
# FP16 IRs (node['_f16_mfma']): node['_out_c8'] (a sibling: its dict's 'c8') asks for the output as dev.BlockedHalf -- fp16, channels
# blocked by eight -- for a reader that c8_reader_ok() accepts; compute() takes such an input through pvhip_conv2d_f16_c8.
SUPPORTS_C8 = True
# ... and, second step: a blocked INPUT with blocked outputs (node['_out_into'] = (dev.BlockedHalf, channel offset): the module's blocked
# Concat buffer), several members, or a MaxPool in front runs as one launch of the module form (launch_c8_multi; c8_module_member_ok()).
SUPPORTS_C8_MODULES = True


# A pass made of such nodes can be recorded into a hipGraph (Executable_Network.infer does so by itself for device-resident inputs):
# nothing in compute() synchronises with the host or reads a tensor back once the constants are cached.
GRAPH_CAPTURE_SAFE = True

def name():
    print('Convolution')


def calc_output_shape(input_dim, kernel_dim, strides, pads_begin, pads_end, rounding_type, auto_pad):
    return tuple(common_def.pooled_extent(input_dim[i], kernel_dim[i], strides[i], pads_begin[i], pads_end[i],
                                          rounding_type, auto_pad, same_means_input=False) for i in (0, 1))


# ---- the IR side: what the fusion plan asks (IR attributes and port dims; no device needed)

Geometry = namedtuple('Geometry', 'n c h w kn kh kw strides pads_begin pads_end auto_pad oh ow')
_IR_ERRORS = (KeyError, ValueError, AssertionError, IndexError, TypeError)      # what a node the plugin cannot read raises


def _geometry(x_shape, w_shape, strides, pads_begin, pads_end, auto_pad):
    n, c, h, w = (int(d) for d in x_shape)
    kn, _, kh, kw = (int(d) for d in w_shape)
    st, pb, pe = tuple(strides), tuple(pads_begin), tuple(pads_end)
    return Geometry(n, c, h, w, kn, kh, kw, st, pb, pe, auto_pad, *calc_output_shape((h, w), (kh, kw), st, pb, pe, 'floor', auto_pad))


def geometry(node: dict):
    """The Geometry of a Convolution IR node (4-D input and weights over the same channels), or None for a node it cannot read."""
    try:
        attrs, xd, wd = node['data'], node['input'][0]['dims'], node['input'][1]['dims']
        if len(xd) != 4 or len(wd) != 4 or int(wd[1]) != int(xd[1]):
            return None
        return _geometry(xd, wd, *(common_def.string_to_tuple(attrs[k]) for k in ('strides', 'pads_begin', 'pads_end')), attrs['auto_pad'])
    except _IR_ERRORS:
        return None


def _same_window(g) -> bool:          # a stride-1 "same" window: the output has the input's extent
    pad = (g.kh - 1) // 2
    return g.kh == g.kw and g.strides == (1, 1) and g.pads_begin == (pad, pad) == g.pads_end


def _pool3x3_same(pool_node: dict) -> bool:           # a 3x3 / stride 1 / pad 1 MaxPool
    pa = pool_node['data']
    return all(common_def.string_to_tuple(pa[k]) == v for k, v in (('kernel', (3, 3)), ('strides', (1, 1)), ('pads_begin', (1, 1)),
                                                                    ('pads_end', (1, 1)))) and pa['auto_pad'] == 'explicit'


def _kind(g) -> int:
    return int(dev.call('pvhip_conv2d_kernel_kind', g.n, g.c, g.h, g.w, g.kn, g.kh, g.kw, g.oh, g.ow, *g.strides, *g.pads_begin))


def _multi_ok(g, members: int) -> bool:         # the multi-destination launch (1x1, unpadded, C % 16 == 0)
    return bool(dev.call('pvhip_conv2d_multi_supported', g.c, g.kh, g.kw, *g.strides, *g.pads_begin, members))


def _c8_reader_ok(g) -> bool:
    if g.pads_begin != g.pads_end or 2 * g.n * (-(-g.c // 16) * 16) * g.h * g.w >= 2 ** 31 or g.n * g.kn * g.oh * g.ow >= 2 ** 31:
        return False       # (32-bit offsets in the kernel; the query does not know n)
    return bool(dev.call('pvhip_conv2d_f16_c8_supported', g.c, g.h, g.w, g.kh, g.kw, *g.strides, *g.pads_begin, g.oh, g.ow))


def c8_reader_ok(node: dict) -> bool:
    """True when pvhip_conv2d_f16_c8 covers this Convolution node: it may then be handed its input as fp16 blocked by eight channels
    (dev.BlockedHalf) by the 1x1 convolution in front of it."""
    g = geometry(node)
    return g is not None and _c8_reader_ok(g)


def c8_writer_ok(node: dict) -> bool:
    """True when the f16 multi-destination launch (launch_siblings with one or more members) runs this Convolution node, i.e. when it
    can store its output as dev.BlockedHalf: 1x1, stride 1, unpadded, C % 16 == 0."""
    g = geometry(node)
    return g is not None and g.pads_end == (0, 0) and g.auto_pad in ('explicit', 'valid') and _multi_ok(g, 1)


def c8_multi_ok(x_shape, kh: int, kw: int, pool: bool, n_members: int) -> bool:
    """True when pvhip_conv2d_f16_c8_multi covers a launch of n_members convolutions with this window over a blocked input of this shape."""
    n, c, h, wd = x_shape
    if 2 * int(n) * (-(-int(c) // 16) * 16) * int(h) * int(wd) >= 2 ** 31:
        return False       # (the launch addresses its input with 32-bit byte offsets; the query does not know n)
    return bool(dev.call('pvhip_conv2d_f16_c8_multi_supported', int(c), int(h), int(wd), int(kh), int(kw), 1 if pool else 0, int(n_members)))


def c8_module_member_ok(node: dict, pool_node: dict = None) -> bool:
    """True when this Convolution node can run on pvhip_conv2d_f16_c8_multi with a blocked input AND a blocked output: a stride-1 "same"
    1x1 / 3x3 / 5x5 window (a 1x1 optionally behind a 3x3 / 1 / 1 MaxPool), output channels a multiple of 8."""
    g = geometry(node)
    if g is None or not _same_window(g) or g.kn % 8 != 0 or g.auto_pad not in ('explicit', 'valid'):
        return False
    try:
        if pool_node is not None and (g.kh != 1 or not _pool3x3_same(pool_node) or tuple(pool_node['input'][0]['dims']) != (g.n, g.c, g.h, g.w)):
            return False
    except _IR_ERRORS:
        return False
    return c8_multi_ok((g.n, g.c, g.h, g.w), g.kh, g.kw, pool_node is not None, 1)


def c8_dma_writer_ok(node: dict) -> bool:
    """True when launch(..., out_c8=True) stores this Convolution node's output as dev.BlockedHalf (the route it takes there)."""
    g = geometry(node)
    return g is not None and g.oh > 0 and g.ow > 0 and \
        _dense_route((g.n, g.c, g.h, g.w), (g.kn, g.c, g.kh, g.kw), g.strides, g.pads_begin, g.pads_end, g.auto_pad, True, False, True).out == 'blocked'


def pre_add_fusable(node: dict, add_node: dict, const_node: dict, f16: bool = False) -> bool:
    """True when this layer pads its input in a pass of its own (PVHIP_CONV_PREPAD) and the Add in front of it adds one fp32 constant per
    input channel: the padding pass then does the Add."""
    g = geometry(node)
    if g is None or g.auto_pad != 'explicit':
        return False
    xd, cd = (g.n, g.c, g.h, g.w), (1, g.c, 1, 1)
    try:
        if tuple(const_node['data']['shape']) != cd or const_node['data']['element_type'] != 'f32':
            return False
        if tuple(add_node['output'][common_def.first_output_port(add_node)]['dims']) != xd or \
                not all(tuple(p_['dims']) in (xd, cd) for p_ in add_node['input'].values()):
            return False
    except _IR_ERRORS:
        return False
    return _prepad(g, f16)


def pooled_fusable(node: dict, pool_node: dict) -> bool:
    """True when libpvhip's MaxPool + 1x1 convolution kernel covers this pair."""
    g = geometry(node)
    if g is None or (g.kh, g.kw) != (1, 1) or g.strides != (1, 1) or g.pads_begin != (0, 0) or g.pads_end != (0, 0) or \
            g.auto_pad not in ('explicit', 'valid'):
        return False
    xd = (g.n, g.c, g.h, g.w)
    try:
        if not _pool3x3_same(pool_node) or tuple(pool_node['input'][0]['dims']) != xd or \
                tuple(pool_node['output'][common_def.first_output_port(pool_node)]['dims']) != xd:
            return False
    except _IR_ERRORS:
        return False
    return bool(dev.call('pvhip_conv2d_pooled_supported', g.n, g.c, g.h, g.w, g.kn))


def siblings_fusable(nodes) -> bool:
    """True when libpvhip's multi-destination launch covers these Convolution nodes."""
    if not 2 <= len(nodes) <= dev.MAX_CONV_DESTS:
        return False
    gs = [geometry(node) for node in nodes]
    if any(g is None for g in gs):
        return False
    first = gs[0]
    return all(g[:4] == first[:4] and g[7:11] == first[7:11] and g.auto_pad in ('explicit', 'valid') and g.pads_end == (0, 0) and
               _multi_ok(g, len(nodes)) for g in gs)


def kernel_kind(node: dict):
    """(family name, executed fraction) of the kernel libpvhip runs for this Convolution node."""
    g = geometry(node)
    if g is None:
        raise ValueError('{}: not a Convolution node libpvhip can read'.format(node.get('name')))
    code = _kind(g)
    family, frac = KERNEL_KINDS[code]
    m = {2: 2, 3: 4, 4: 2, 6: 3}.get(code)          # Winograd: whole m x m output patches are computed (14x14 as 16x16 under F(4x4))
    if m:
        frac *= (-(-g.oh // m) * m) * (-(-g.ow // m) * m) / float(g.oh * g.ow)
    return family, frac


# pvhip_conv2d_kernel_kind codes -> (family name, fraction of the algorithmic multiply-adds the matrix cores execute)
KERNEL_KINDS = {5: ('row spans (stem)', 148.0 / 147.0),          # four taps per MFMA step: 147 taps in 37 steps, one slot of zero weight
                6: ('Winograd F(3x3,4x4), space-to-depth (stem)', 36.0 * 4.0 / (9.0 * 49.0)),      # 36 points x 4 phases per 9 outputs x 49 taps
                0: ('implicit GEMM (LDS-DMA)', 1.0), 1: ('pointwise', 1.0), 2: ('Winograd F(2x2,3x3)', 16.0 / 36.0),
                3: ('Winograd F(4x4,3x3)', 36.0 / 144.0), 4: ('Winograd F(2x2,5x5)', 36.0 / 100.0)}




# ---- the launch route: which entry point runs a launch, decided from values alone (shapes, layouts, settings, libpvhip's queries)

# entry: the libpvhip entry point; pack: the weight form it reads (_PACKERS; 'panel ...': the members' weights in 32-channel tiles); pad_row:
# floats per row of the zero-padded image a padding pass writes first (0: none); x_in / out: the layout it reads / the leading output's
# layout ('dense' fp32 NCHW or 'blocked' dev.BlockedHalf); label: what node['_hip_f16'] says (FP16 IRs; tests and bench.py read it).
# entry None: no launch can write the blocked Concat buffer the plan gave it.
Route = namedtuple('Route', 'entry pack pad_row x_in out label')

_F16_LABELS = {'pvhip_conv2d_f16': 'gather', 'pvhip_conv2d_f16_span': 'span', 'pvhip_conv2d_f16_dma': 'lds-dma',
               'pvhip_conv2d_f16_dma_c8': 'lds-dma, blocked output', 'pvhip_conv2d_f16_stem': 'row spans, blocked output',
               'pvhip_conv2d_f16_stem_direct': 'row spans, blocked output', 'pvhip_conv2d_f16_c8': 'c8', 'pvhip_conv2d_f16_c8_multi': 'c8 module',
               'pvhip_conv2d_multi_f16_dma': 'lds-dma, siblings', 'pvhip_conv2d_pooled_f16': 'MaxPool + 1x1'}


def _label(entry, pool=False, members=1):
    label = _F16_LABELS.get(entry)
    if entry == 'pvhip_conv2d_f16_c8_multi':
        label += (', MaxPool' if pool else '') + (', {} members'.format(members) if members > 1 else '')
    return label


def _prepad(g, f16) -> bool:
    """True for a padded layer that libpvhip runs on the c-major form of the LDS-DMA kernel (C % 16 != 0, not a Winograd or pointwise
    layer): its gather tests every tap against the window unless no window leaves the tensor (PVHIP_CONV_PREPAD=0: never)."""
    if not dev.conv_prepad or g.c % 16 == 0 or not (any(g.pads_begin) or any(g.pads_end)) or g.oh <= 0 or g.ow <= 0 or g.kh * g.kw >= 64:
        return False
    if f16:         # FP16 IRs: the c-major f16 form of the LDS-DMA kernel (every such layer: there is no Winograd or pointwise form in front of it)
        return dev.conv_f16_dma and bool(dev.call('pvhip_conv2d_f16_dma_supported', g.c, g.kh, g.kw))
    # (kind 5, the row-span kernel, pads its input in a pass of its own too: the Add in front of the layer rides in that pass just the same)
    return _kind(g) in (0, 5, 6)


def prepad_wanted(n, c, h, wd, kn, kh, kw, oh, ow, strides, pads_begin, pads_end, f16=False) -> bool:
    """_prepad of this geometry: the piece of the route that pads the input in a pass of its own (tests and scripts ask it)."""
    return _prepad(Geometry(n, c, h, wd, kn, kh, kw, tuple(strides), tuple(pads_begin), tuple(pads_end), 'explicit', oh, ow), f16)


def _dense_route(x_shape, w_shape, strides, pads_begin, pads_end, auto_pad, f16=False, into=False, out_c8=False, pre_add=False, clamp=False):
    """The Route of launch(): one convolution of a dense input (into: it writes a range of an fp32 Concat buffer)."""
    g = _geometry(x_shape, w_shape, strides, pads_begin, pads_end, auto_pad)
    geo = (g.c, g.h, g.w, g.kn, g.kh, g.kw, *g.strides, *g.pads_begin, g.oh, g.ow)      # what the stem queries take
    blocked_ok = out_c8 and not into and not clamp
    if f16 and blocked_ok and dev.conv_f16_stem and g.pads_begin == g.pads_end:
        # a 7x7 / 2 convolution over three channels with a blocked fp16 output (GoogLeNet's conv1) from row spans of the padded image
        wps = int(dev.call('pvhip_conv2d_f16_stem_supported', *geo))
        # (the kernel addresses its input with 32-bit byte offsets and the query does not know n: else the LDS-DMA form takes it)
        if wps > 0 and 4 * g.n * g.c * (g.h + 2 * g.pads_begin[0]) * wps < 2 ** 31 and g.n * 64 * g.oh * g.ow < 2 ** 31:
            if dev.conv_stem_direct and dev.call('pvhip_conv2d_f16_stem_direct_supported', *geo):
                return Route('pvhip_conv2d_f16_stem_direct', 'f16_stem_direct', 0, 'dense', 'blocked', _label('pvhip_conv2d_f16_stem_direct'))
            return Route('pvhip_conv2d_f16_stem', 'f16_stem', wps, 'dense', 'blocked', _label('pvhip_conv2d_f16_stem'))
    kind = _kind(g) if not f16 and not into and g.pads_begin == g.pads_end and g.oh > 0 and g.ow > 0 else None
    if kind in (5, 6):
        # fp32: a 7x7 / 2 first convolution over three channels from row spans (weights resident in registers, no vector instruction in its
        # reduction loop), or as Winograd F(3x3,4x4) on the space-to-depth image (kind 6: 0.34 of the multiplies)
        wps = int(dev.call('pvhip_conv2d_stem_f32_supported', *geo))
        if wps > 0:
            if kind == 6:
                return Route('pvhip_conv2d_stem_wino_f32', 'stem_wino', 0, 'dense', 'dense', None)
            if dev.conv_stem_direct and dev.call('pvhip_conv2d_stem_direct_supported', *geo):
                return Route('pvhip_conv2d_stem_direct_f32', 'stem_f32', 0, 'dense', 'dense', None)
            return Route('pvhip_conv2d_stem_f32', 'stem_f32', wps, 'dense', 'dense', None)
    # The zero-padded image as a tensor of its own, convolved WITHOUT padding (the Add in front of the layer rides in that pass): the gather
    # of a layer whose channel count is not a multiple of 16 then needs no window test -- vector instructions are matrix time lost
    pad_row = g.w + g.pads_begin[1] + g.pads_end[1] if pre_add or _prepad(g, f16) else 0
    if f16 and dev.conv_f16_span >= (2 if g.kh == 1 else 1) and dev.call('pvhip_conv2d_f16_span_supported', g.c, g.h, g.w, g.kh, g.kw, *g.strides,
                                                                           *g.pads_begin, g.oh, g.ow):
        entry, pack = 'pvhip_conv2d_f16_span', 'f16_span'
    elif f16 and dev.conv_f16_dma and dev.call('pvhip_conv2d_f16_dma_supported', g.c, g.kh, g.kw):
        # FP16 IRs: the f16 form of the LDS-DMA kernel on the fp32 panel; a reader that takes fp16 blocked by eight channels gets that
        entry, pack = ('pvhip_conv2d_f16_dma_c8' if blocked_ok else 'pvhip_conv2d_f16_dma'), 'f32'
    elif f16:       # fp16 operands on the f16 matrix cores, fp32 accumulation
        entry, pack = 'pvhip_conv2d_f16', 'f16'
    else:
        entry, pack = 'pvhip_conv2d_f32', 'f32'
    return Route(entry, pack, pad_row, 'dense', 'blocked' if entry == 'pvhip_conv2d_f16_dma_c8' else 'dense', _label(entry))


def route(x_shape, w_shape, strides, pads_begin, pads_end, auto_pad='explicit', f16=False, x_blocked=False, into=None, blocked_into=False,
          out_c8=False, siblings=0, pool=False, pre_add=False, clamp=False):
    """The Route of a compute() launch.  x_blocked: the input arrives as dev.BlockedHalf; into: the leading output's destination (None: a
    tensor of its own, 'dense' / 'blocked': a range of an fp32 / a blocked Concat buffer); blocked_into: some member writes a blocked Concat
    buffer; out_c8: the leading output is wanted blocked; siblings: how many convolutions ride in the launch besides the leading one; pool:
    a 3x3 / 1 / 1 MaxPool in front; pre_add: a per-channel Add in front; clamp: the fused activation is a Clamp."""
    blocked_into = blocked_into or into == 'blocked'
    if f16 and (x_blocked or blocked_into):
        # a blocked input (a dense one is converted when the plan gave the launch a blocked Concat buffer: a producer in front of it
        # handed over a dense tensor after all, because a kernel refused its size at launch) goes to the module form -- blocked outputs,
        # several members, a MaxPool in front -- or to the reader kernel (an fp32 output); any other geometry densifies it
        g = _geometry(x_shape, w_shape, strides, pads_begin, pads_end, auto_pad)
        if _same_window(g) and (siblings or pool or out_c8 or blocked_into) and c8_multi_ok(x_shape, g.kh, g.kw, pool, 1 + siblings):
            out = 'blocked' if into == 'blocked' or (into is None and out_c8) else 'dense'
            entry = 'pvhip_conv2d_f16_c8_multi'
            return Route(entry, 'panel f16_c8', 0, 'blocked', out, _label(entry, pool, 1 + siblings))
        if not blocked_into and not siblings and not pool and int(w_shape[1]) == g.c and _c8_reader_ok(g):
            return Route('pvhip_conv2d_f16_c8', 'f16_c8', 0, 'blocked', 'dense', _label('pvhip_conv2d_f16_c8'))
    if blocked_into:
        return Route(None, None, 0, 'dense', 'blocked', None)
    dense = (x_shape, w_shape, strides, pads_begin, pads_end, auto_pad, f16, into is not None)
    if f16 and out_c8 and not siblings and dev.conv_f16_dma and \
            not (tuple(pads_end) == (0, 0) and auto_pad in ('explicit', 'valid') and
                 _multi_ok(_geometry(x_shape, w_shape, strides, pads_begin, pads_end, auto_pad), 1)):
        return _dense_route(*dense, True, pre_add, clamp)
    if f16 and (siblings or out_c8) and dev.conv_f16_dma:
        entry = 'pvhip_conv2d_multi_f16_dma'
        return Route(entry, 'panel f32', 0, 'dense', 'blocked' if into is None and out_c8 else 'dense', _label(entry))
    if pool:
        entry = 'pvhip_conv2d_pooled_f16' if f16 else 'pvhip_conv2d_pooled_f32'
        return Route(entry, 'f32', 0, 'dense', 'dense', _label(entry))
    if siblings and not f16:
        return Route('pvhip_conv2d_multi_f32', 'panel f32', 0, 'dense', 'dense', None)
    return _dense_route(*dense, False, pre_add, clamp)


# A 7x7 / 2 first convolution on the row-span kernel that reads the image itself can write a SECOND output: the 3x3 / stride 2 / unpadded / ceil MaxPool
# of its own output (after bias and activation), taken where the values already are.  node['_fuse_pool_out'] = the MaxPool's node dict asks for it;
# the pooled tensor is left in node['_pooled_out'] (None where this launch could not make it) and the engine hands it to the MaxPool task.  The
# engine asks pooled_output_fusable() first.
SUPPORTS_POOLED_OUTPUT = True


def _pooled_extent(pool_node: dict, oh: int, ow: int):
    """(poh, pow) when the node is the MaxPool the stem kernel's second output is (3x3 / stride 2 / no padding / ceil), else None."""
    from . import MaxPool
    pa = pool_node['data']
    geo = tuple(tuple(common_def.string_to_tuple(pa[k])) for k in ('kernel', 'strides', 'pads_begin', 'pads_end'))
    if geo != ((3, 3), (2, 2), (0, 0), (0, 0)) or pa['rounding_type'] != 'ceil' or pa['auto_pad'] not in ('explicit', 'valid'):
        return None
    return MaxPool.calc_output_shape((oh, ow), (3, 3), (2, 2), (0, 0), (0, 0), 'ceil', pa['auto_pad'])


def pooled_output_fusable(node: dict, pool_node: dict, by_size: bool = True, pre_add: bool = False) -> bool:
    """True when this fp32 convolution takes pvhip_conv2d_stem_direct_f32 and that kernel's pooled form covers the MaxPool behind it (IR
    attributes and port dims; no device needed).  by_size: the native size rule decides too (every CU walks enough tiles)."""
    try:
        xs, ws = tuple(int(d) for d in node['input'][0]['dims']), tuple(int(d) for d in node['input'][1]['dims'])
        if node['input'][0]['precision'] != 'FP32' or len(xs) != 4 or len(ws) != 4:
            return False
        attrs = node['data']
        strides, pads_begin, pads_end = (tuple(common_def.string_to_tuple(attrs[k])) for k in ('strides', 'pads_begin', 'pads_end'))
        r = _dense_route(xs, ws, strides, pads_begin, pads_end, attrs['auto_pad'], pre_add=pre_add)
        if r.entry != 'pvhip_conv2d_stem_direct_f32':
            return False
        g = _geometry(xs, ws, strides, pads_begin, pads_end, attrs['auto_pad'])
        pooled = _pooled_extent(pool_node, g.oh, g.ow)
        if pooled is None or tuple(int(d) for d in pool_node['input'][0]['dims']) != (g.n, g.kn, g.oh, g.ow):
            return False
        return bool(dev.call('pvhip_conv2d_stem_direct_pool_supported', g.n if by_size else 0, g.c, g.h, g.w, g.kn, g.kh, g.kw, *g.strides, *g.pads_begin,
                             g.oh, g.ow, *pooled))
    except (KeyError, ValueError, AssertionError, IndexError, TypeError):
        return False


def _route_of(node: dict, decide, *facts) -> Route:
    """decide(*facts), kept on the node (node['_hip_route'] = (key, route)) per facts and settings: asked once, not on every launch."""
    key = (dev.settings_serial, decide, facts)
    hit = node.get('_hip_route')
    if hit is None or hit[0] != key:
        hit = node['_hip_route'] = (key, decide(*facts))
    return hit[1]


# ---- weights, packed once per node

_PACKERS = {    # weight form -> (element count query, packer, how many of (k, c, kh, kw) they take); 'f32' / 'f16' bake the input extent in
    'f32': ('pvhip_conv2d_pack_elems', 'pvhip_conv2d_pack_f32', 4),
    'f16': ('pvhip_conv2d_f16_pack_elems', 'pvhip_conv2d_f16_pack', 4),
    'f16_span': ('pvhip_conv2d_f16_span_pack_elems', 'pvhip_conv2d_f16_span_pack', 4),
    'f16_c8': ('pvhip_conv2d_f16_c8_pack_elems', 'pvhip_conv2d_f16_c8_pack', 4),
    'f16_stem': ('pvhip_conv2d_f16_stem_pack_elems', 'pvhip_conv2d_f16_stem_pack', 1),
    'f16_stem_direct': ('pvhip_conv2d_f16_stem_pack_elems', 'pvhip_conv2d_f16_stem_direct_pack', 1),
    'stem_f32': ('pvhip_conv2d_stem_f32_pack_elems', 'pvhip_conv2d_stem_f32_pack', 1),
    'stem_wino': ('pvhip_conv2d_stem_wino_pack_elems', 'pvhip_conv2d_stem_wino_pack', 1),      # (a size of its own: the query takes nothing)
}
_IMAGE_READERS = ('pvhip_conv2d_f16_stem_direct', 'pvhip_conv2d_stem_direct_f32', 'pvhip_conv2d_stem_wino_f32')  # no padding pass: the Add in LDS


def _pack(form, w, shape, extent=()):
    elems, packer, ndims = _PACKERS[form]
    dims = tuple(int(d) for d in shape[:ndims])
    out = dev.DeviceTensor.empty((int(dev.call(elems, *(dims if form != 'stem_wino' else ()))),))
    dev.call(packer, dev.ptr(w), dev.ptr(out), *dims, *extent)
    return out


def _cached(node: dict, form: str, blocks: tuple, extent: tuple, build):
    """build(), kept on the node per weight form, for these weight / bias device blocks and this baked-in extent (weights are Const
    outputs: the same blocks arrive on every infer)."""
    packs = node.setdefault('_hip_packs', {})
    hit = packs.get(form)
    if hit is None or hit[0] != blocks or hit[1] != extent:
        hit = packs[form] = (blocks, extent, build())
    return hit[2]


def packed_weights(node: dict, form: str, w, extent=()) -> 'dev.DeviceTensor':
    """The weights of one convolution in the form (_PACKERS) its kernel reads."""
    return _cached(node, form, (w._block,), (w.shape,) + tuple(extent), lambda: _pack(form, w, w.shape, extent))


def panel(node: dict, form: str, ws, biases, extent=()):
    """(the members' weights laid one after the other, each padded to whole 32-channel tiles, packed in `form`; their biases laid out the
    same, or None) of a launch with several outputs, kept on the leading node."""
    def build():
        rows = [-(-w.shape[0] // 32) * 32 for w in ws]
        host_w = np.zeros((sum(rows),) + tuple(ws[0].shape[1:]), dtype=np.float32)
        host_b = np.zeros((sum(rows),), dtype=np.float32)
        row = 0
        for w, b, kp in zip(ws, biases, rows):
            host_w[row:row + w.shape[0]] = w.numpy()
            if b is not None:
                host_b[row:row + w.shape[0]] = b.numpy().reshape(-1)
            row += kp
        wpack = _pack(form, dev.DeviceTensor.from_numpy(host_w), host_w.shape, extent)
        return wpack, dev.DeviceTensor.from_numpy(host_b) if any(b is not None for b in biases) else None
    blocks = tuple(w._block for w in ws) + tuple(b._block if b is not None else None for b in biases)
    return _cached(node, 'panel ' + form, blocks, tuple(extent), build)


# ---- the launchers

def _dest(into, n, k, h, w, blocked=False):
    """(tensor the kernel stores into, first channel, its channel count (0: a tensor of its own), the output handed on) for into =
    (Concat buffer, channel offset), or None: a tensor of its own (blocked: a dev.BlockedHalf)."""
    if into is None:
        y = dev.BlockedHalf((n, k, h, w)) if blocked else dev.DeviceTensor.empty((n, k, h, w))
        return y, 0, 0, y
    target, coff = into
    assert target.shape[0] == n and tuple(target.shape[2:]) == (h, w) and coff + k <= target.shape[1]
    view = dev.BlockedChannelSlice if isinstance(target, dev.BlockedHalf) else dev.ChannelSlice
    return target, int(coff), int(target.shape[1]), view(target, coff, k)


def _check_channels(x, w):
    if w.shape[1] != x.shape[1]:
        raise ValueError('shapes {} and {} not aligned: {} (dim 1) != {} (dim 1)'.format(x.shape, w.shape, x.shape[1], w.shape[1]))


def launch(node, x, w, strides, pads_begin, pads_end, auto_pad, bias=None, act=None, into=None, f16=False, out_c8=False):
    """One convolution of a dense input (node['_pre_add']: a per-channel Add in front); out_c8: a blocked output where the route gives one."""
    r = _route_of(node, _dense_route, tuple(x.shape), tuple(w.shape), tuple(strides), tuple(pads_begin), tuple(pads_end), auto_pad, bool(f16),
                  into is not None, bool(out_c8), node.get('_pre_add') is not None, act is not None and act[0] != 'relu')
    return _launch_dense(node, r, x, w, strides, pads_begin, pads_end, auto_pad, bias, act, into)


def _launch_dense(node, r, x, w, strides, pads_begin, pads_end, auto_pad, bias, act, into):
    n, c, h, wd = x.shape
    kn, _, kh, kw = w.shape
    _check_channels(x, w)
    oh, ow = calc_output_shape((h, wd), (kh, kw), strides, pads_begin, pads_end, 'floor', auto_pad)
    hp, wp = h + pads_begin[0] + pads_end[0], wd + pads_begin[1] + pads_end[1]
    if oh > 0 and ow > 0 and ((oh - 1) * strides[0] + kh > hp or (ow - 1) * strides[1] + kw > wp):
        # the strided slice of the padded image is shorter than (oh, ow): numpy refuses the assignment (:68)
        raise ValueError('could not broadcast input array: window exceeds the padded input '
                         '({}x{} padded, kernel {}x{}, stride {}, output {}x{})'.format(hp, wp, kh, kw, strides, oh, ow))
    pre_add = node.get('_pre_add')            # plan_fusion: the per-channel Add in front of this layer rides in the padding pass
    if pre_add is not None:
        pre_add = dev.as_device(pre_add)
        assert pre_add.size == c
    if r.label:
        node['_hip_f16'] = r.label
    act_code, act_lo, act_hi = dev.act_args(act)
    stem = _PACKERS[r.pack][2] == 1         # the row-span stem kernels: the image (or its padded copy) in, no gather table
    if stem:
        wpack = packed_weights(node, r.pack, w)
    if r.pad_row:
        xp = dev.DeviceTensor.empty((n, c, hp, r.pad_row))
        dev.call('pvhip_pad2d_f32', dev.ptr(x), dev.ptr(xp), n, c, h, wd, pads_begin[0], pads_begin[1], pads_end[0], r.pad_row - wd - pads_begin[1],
                 dev.ptr(pre_add))
        x, h, wd, pads_begin = xp, hp, r.pad_row, (0, 0)
    if not stem:                            # (the gather table of the f32 / f16 panels holds the extent of the padded image)
        wpack = packed_weights(node, r.pack, w, (h, wd) if r.pack in ('f32', 'f16') else ())
    target, coff, ctotal, y = _dest(into, n, kn, oh, ow, blocked=r.out == 'blocked')
    if stem:
        image = (dev.ptr(pre_add),) if r.entry in _IMAGE_READERS else ()
        epilogue = (act_code,) if r.out == 'blocked' else (act_code, act_lo, act_hi)
        pool_node = node.get('_fuse_pool_out')
        if pool_node is not None:
            node['_pooled_out'] = None
            pooled = _pooled_extent(pool_node, oh, ow) if r.entry == 'pvhip_conv2d_stem_direct_f32' and into is None else None
            if pooled is not None and dev.call('pvhip_conv2d_stem_direct_pool_supported', 0, c, h, wd, kn, kh, kw, *strides, *pads_begin, oh, ow, *pooled):
                yp = dev.DeviceTensor.empty((n, kn, pooled[0], pooled[1]))
                dev.call('pvhip_conv2d_stem_direct_pool_f32', dev.ptr(x), dev.ptr(wpack), dev.ptr(y), dev.ptr(yp), n, h, wd, kn, oh, ow, pooled[0], pooled[1],
                         dev.ptr(pre_add), dev.ptr(bias), act_code, act_lo, act_hi)
                node['_pooled_out'] = yp
                return y
        dev.call(r.entry, dev.ptr(x), dev.ptr(wpack), dev.ptr(y), n, h, wd, kn, oh, ow, *image, dev.ptr(bias), *epilogue)
    elif r.out == 'blocked':
        dev.call(r.entry, dev.ptr(x), dev.ptr(wpack), dev.ptr(y), n, c, h, wd, kn, kh, kw, oh, ow, strides[0], strides[1], pads_begin[0],
                 pads_begin[1], dev.ptr(bias), act_code)
    else:
        dev.call(r.entry, dev.ptr(x), dev.ptr(wpack), dev.ptr(target), n, c, h, wd, kn, kh, kw, oh, ow, strides[0], strides[1], pads_begin[0],
                 pads_begin[1], dev.ptr(bias), act_code, coff, ctotal, act_lo, act_hi)
    return y


def launch_c8(node, xb, w, bias=None, act=None, into=None):
    """FP16 IRs: the convolution of a dev.BlockedHalf input (pvhip_conv2d_f16_c8); output fp32 NCHW as launch()."""
    n, c, h, wd = xb.shape
    kn, _, kh, kw = w.shape
    _check_channels(xb, w)
    wpack = packed_weights(node, 'f16_c8', w)
    act_code, act_lo, act_hi = dev.act_args(act)
    target, coff, ctotal, y = _dest(into, n, kn, h, wd)
    node['_hip_f16'] = _label('pvhip_conv2d_f16_c8')
    dev.call('pvhip_conv2d_f16_c8', dev.ptr(xb), dev.ptr(wpack), dev.ptr(target), n, c, h, wd, kn, kh, kw, dev.ptr(bias), act_code, coff, ctotal,
             act_lo, act_hi)
    return y


def launch_pooled(node, x, w, bias=None, act=None, into=None, f16=False):
    """conv1x1(maxpool3x3/s1/p1(x)) in one launch; arguments as launch()."""
    n, c, h, wd = x.shape
    kn = w.shape[0]
    if w.shape[1] != c or tuple(w.shape[2:]) != (1, 1):
        raise ValueError('the pooled-input launch is for 1x1 convolutions over the same {} channels, got {}'.format(c, w.shape))
    wpack = packed_weights(node, 'f32', w, (h, wd))
    act_code, act_lo, act_hi = dev.act_args(act)
    target, coff, ctotal, y = _dest(into, n, kn, h, wd)
    entry = 'pvhip_conv2d_pooled_f16' if f16 else 'pvhip_conv2d_pooled_f32'
    if f16:
        node['_hip_f16'] = _label(entry)
    dev.call(entry, dev.ptr(x), dev.ptr(wpack), dev.ptr(target), n, c, h, wd, kn, dev.ptr(bias), act_code, coff, ctotal, act_lo, act_hi)
    return y


def _dests(members, n, h, wd, clamp):
    """(pvhip_conv_dest array, outputs) of a launch with several outputs: members = [(weights, bias, into or None, blocked)]."""
    dests = (dev.ConvDest * len(members))()
    outs = []
    for d, (w, _, into, blocked) in zip(dests, members):
        target, coff, ctotal, y = _dest(into, n, w.shape[0], h, wd, blocked)
        layout = 1 if isinstance(target, dev.BlockedHalf) else 0
        if layout and clamp:
            raise ValueError('a blocked fp16 output takes no Clamp')
        d.y, d.k, d.channel_offset, d.channels_total, d.layout = target.ptr, w.shape[0], coff, ctotal, layout
        outs.append(y)
    return dests, outs


def launch_c8_multi(node, xb, members, pool=False, act=None):
    """FP16 IRs, the module form: members = [(weights, bias or None, into or None, blocked)] over the blocked input xb, ONE launch
    (pvhip_conv2d_f16_c8_multi).  into = (tensor, channel offset) with a dev.BlockedHalf (the module's blocked Concat buffer) or a
    DeviceTensor (an fp32 Concat buffer); without it `blocked` chooses a dev.BlockedHalf or an fp32 tensor of the member's own.
    pool: a 3x3 / 1 / 1 MaxPool of xb in front (one member).  -> list of outputs."""
    n, c, h, wd = xb.shape
    ws = [m[0] for m in members]
    kh, kw = ws[0].shape[2:]
    for w in ws:
        if w.shape[1] != c or tuple(w.shape[2:]) != (kh, kw):
            raise ValueError('the members of a launch are convolutions of the same {} channels with the same window, got {}'.format(c, w.shape))
    wpack, bias = panel(node, 'f16_c8', ws, [m[1] for m in members])
    act_code, act_lo, act_hi = dev.act_args(act)
    dests, outs = _dests(members, n, h, wd, act_code == 2)
    node['_hip_f16'] = _label('pvhip_conv2d_f16_c8_multi', pool, len(members))
    dev.call('pvhip_conv2d_f16_c8_multi', dev.ptr(xb), dev.ptr(wpack), n, c, h, wd, kh, kw, 1 if pool else 0, dev.ptr(bias), act_code, act_lo, act_hi,
             len(members), ctypes.cast(dests, ctypes.c_void_p))
    return outs


def launch_siblings(node, x, members, strides, pads_begin, act, f16=False):
    """members: [(weights, bias or None, into or None[, blocked])], the node's own convolution first.  blocked (FP16 IRs): the member's only
    reader is pvhip_conv2d_f16_c8 -- fp16, channels blocked by eight.  -> list of outputs."""
    n, c, h, wd = x.shape
    ws = [m[0] for m in members]
    for w in ws:
        if w.shape[1] != c or tuple(w.shape[2:]) != (1, 1):
            raise ValueError('sibling convolutions must be 1x1 over the same {} channels, got {}'.format(c, w.shape))
    wpack, bias = panel(node, 'f32', ws, [m[1] for m in members], (h, wd))
    act_code, act_lo, act_hi = dev.act_args(act)
    members = [(m[0], m[1], m[2], len(m) > 3 and bool(m[3])) for m in members]
    assert f16 or not any(m[3] for m in members)
    dests, outs = _dests(members, n, h, wd, act_code == 2)
    if f16:
        node['_hip_f16'] = _label('pvhip_conv2d_multi_f16_dma')
        for m in node.get('_siblings', []):
            m['node']['_hip_f16'] = node['_hip_f16']
    dev.call('pvhip_conv2d_multi_f16_dma' if f16 else 'pvhip_conv2d_multi_f32', dev.ptr(x), dev.ptr(wpack), n, c, h, wd, 1, 1, h, wd,
             strides[0], strides[1], pads_begin[0], pads_begin[1], dev.ptr(bias), act_code, act_lo, act_hi, len(members),
             ctypes.cast(dests, ctypes.c_void_p))
    return outs


def compute(node: dict, inputs: dict = None, kernel_type: str = 'hip', debug: bool = False):
    if debug:
        print(node)
    common_def.validate_inputs(node, inputs)
    attrs = node['data']
    strides, pads_begin, pads_end = (common_def.string_to_tuple(attrs[k]) for k in ('strides', 'pads_begin', 'pads_end'))   # (dilations: ignored)
    x, w = inputs[0], dev.as_device(inputs[1])
    into, sibs, act = node.get('_out_into'), node.get('_siblings') or (), node.get('_fuse_act')
    pool = node.get('_fuse_pool_in') is not None
    r = _route_of(node, route, tuple(x.shape), tuple(w.shape), strides, pads_begin, pads_end, attrs['auto_pad'], bool(node.get('_f16_mfma')),
                  isinstance(x, dev.BlockedHalf), None if into is None else 'blocked' if isinstance(into[0], dev.BlockedHalf) else 'dense',
                  any(s.get('into') is not None and isinstance(s['into'][0], dev.BlockedHalf) for s in sibs), bool(node.get('_out_c8')), len(sibs),
                  pool, node.get('_pre_add') is not None, act is not None and act[0] != 'relu')
    if r.entry is None:
        raise RuntimeError('{}: a blocked fp16 Concat buffer, but this launch cannot write it (the fusion plan promised a blocked input and '
                           'pvhip_conv2d_f16_c8_multi)'.format(node.get('name')))
    if r.x_in == 'blocked':
        x = x if isinstance(x, dev.BlockedHalf) else dev.BlockedHalf.from_dense(dev.as_device(x))
    else:
        x = dev.as_device(x)
    bias = node.get('_fuse_bias')
    if bias is not None:
        bias = dev.as_device(bias)
        assert bias.size == w.shape[0]
    if r.pack.startswith('panel'):          # several outputs: the module form or the multi-destination launch
        members = [(w, bias, into, bool(node.get('_out_c8')))]
        for sib in sibs:
            common_def.validate_inputs(sib['node'], sib['inputs'])
            sb = sib.get('bias')
            members.append((dev.as_device(sib['inputs'][1]), dev.as_device(sb) if sb is not None else None, sib.get('into'), bool(sib.get('c8'))))
        if r.entry == 'pvhip_conv2d_f16_c8_multi':
            outs = launch_c8_multi(node, x, members, pool=pool, act=act)
        else:
            outs = launch_siblings(node, x, members, strides, pads_begin, act, f16=r.entry == 'pvhip_conv2d_multi_f16_dma')
        y, node['_sibling_out'] = outs[0], outs[1:]
    elif r.entry == 'pvhip_conv2d_f16_c8':
        y = launch_c8(node, x, w, bias=bias, act=act, into=into)
    elif r.entry in ('pvhip_conv2d_pooled_f32', 'pvhip_conv2d_pooled_f16'):
        y = launch_pooled(node, x, w, bias=bias, act=act, into=into, f16=r.entry == 'pvhip_conv2d_pooled_f16')
    else:
        y = _launch_dense(node, r, x, w, strides, pads_begin, pads_end, attrs['auto_pad'], bias, act, into)
    port = common_def.first_output_port(node)
    assert common_def.type_convert_tbl[node['output'][port]['precision']] == np.float32
    return {port: y}
