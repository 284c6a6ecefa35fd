"""Every kernel form of the MatMul, elementwise and data-movement launchers against float64, one explicit row per form.

pvhip_matmul.hip, pvhip_eltwise.hip, pvhip_move.hip and pvhip_layout.hip pick a kernel, a template instantiation and a grid from the
extents, the strides and the addresses of a launch.  pvhip_matmul_form / pvhip_unary_form / pvhip_binary_form / pvhip_concat_form /
pvhip_input_to_nchw_form (host-only; they call the plan function the launcher switches on) say which form a launch takes; ROWS below
is the table: the arguments of a launch and the form CLASS the row is there for (class_of() maps a query's answer to its class).
Transpose, pad2d and the two c8 conversions have one kernel each: their rows carry names, not planner classes (FIXED_CLASSES).

CPU part (no device): the query answers the class of every row; every row has a class of its own and the table holds exactly the
classes the planners return over a seeded sweep of shapes (plus the fixed names and the EDGE_ROWS, which are pinned by name): deleting
a row fails test_table_holds_every_class_the_planners_return; the float64 references (tests/ref64.py) agree with the oracle.

GPU part: every row is launched through the C entry (the binary ops through the plugins' launcher, op_plugins/_broadcast.py) into an
output filled with NaN bytes and compared with float64:
  * ReLU, Clamp, Add, Multiply, Concat, Transpose, pad2d, the layout kernels and the c8 conversions bit for bit (helpers.BIT_EXACT:
    against the oracle's op where it has one, and against the float64 reference rounded to fp32);
  * Sigmoid and the fp32 MatMul by ref64.check_group (REL_TOL in both norms + DRIFT in the max norm);
  * the f16 MatMul by assert_close at 1e-5 against float64 on fp16-rounded operands.
The kSwap instantiations of the channel kernels are reachable through the diagnostic build's subtract only (SUB_ROWS: they run in
tests/diag_variants.py, in the diagnostic library's own process); the nontemporal forms at test sizes run in
tests/test_hip_ops.py::test_nontemporal_streaming_forms_at_small_sizes (row Unary-nt-n10638649 takes its shape; no second GPU run here).
"""
import ctypes
import functools
import itertools
import zlib

import numpy as np
import pytest

import helpers
import ref64
from helpers import assert_bit_exact, assert_close

gpu = pytest.mark.gpu

FORM_INTS = 16                                                        # PVHIP_FORM_INTS of include/pvhip.h
NT_ENV = {'PVHIP_STREAM_NT': '2', 'PVHIP_STREAM_WG': '1'}             # test_hip_ops._nt_outputs
WG1_ENV = {'PVHIP_STREAM_WG': '1'}                                    # 256 workgroups at most: a run loop wraps at 1 MiB


# --------------------------------------------------------------------------------------------------------------------- the queries
def _query(entry, *args):
    from pyopenvino_amd import device
    f = (ctypes.c_int * FORM_INTS)()
    device.call(entry, *args, f)
    return list(f)


def matmul_form(m, n, k, ta, tb, f16):
    f = _query('pvhip_matmul_form', m, n, k, int(ta), int(tb), int(f16))
    return dict(zip(('kind', 'gx', 'gy', 'splits', 'k_chunk', 'last_k', 'akf', 'bnf', 'f16'), f))


def unary_form(n):
    return dict(zip(('kind', 'nt', 'u', 'grid', 'runs', 'rem4', 'tail', 'wraps'), _query('pvhip_unary_form', n)))


def broadcast_strides(a_shape, b_shape):
    """(output shape, a strides, b strides) as op_plugins/_broadcast.py resolves numpy broadcasting."""
    from pyopenvino_amd.op_plugins._broadcast import strides_for_broadcast
    out = tuple(int(d) for d in np.broadcast_shapes(tuple(a_shape), tuple(b_shape)))
    return out, strides_for_broadcast(a_shape, out), strides_for_broadcast(b_shape, out)


def binary_form(a_shape, b_shape, commutative=True):
    from pyopenvino_amd import device
    out, a_st, b_st = broadcast_strides(a_shape, b_shape)
    f = _query('pvhip_binary_form', len(out), device.i64_array(out), device.i64_array(a_st), device.i64_array(b_st), int(commutative))
    return dict(zip(('kind', 'bcast', 'swap', 'nt', 'C', 'inner', 'grid'), f), n=int(np.prod(out, dtype=np.int64)))


def concat_form(inner, outer):
    from pyopenvino_amd import device
    return dict(zip(('kind', 'gx', 'gy'), _query('pvhip_concat_form', len(inner), device.i64_array(inner), int(outer))))


def input_form(n, c, h, w, u8, nhwc, src_align, dst_align):
    f = _query('pvhip_input_to_nchw_form', n, c, h, w, int(u8), int(nhwc), int(src_align), int(dst_align))
    return dict(zip(('kind', 'vec', 'tile', 'vl', 'vs', 'gx', 'gy'), f))


# ---------------------------------------------------------------------------------------------------------- answers -> form classes
NONE = -1
MATMUL_KINDS = {NONE: 'none', 0: 'memset', 1: 'single', 2: 'split'}
BINARY_KINDS = {0: 'same', 1: 'channel', 2: 'channel4', 3: 'strided'}
BLOCK = 256                                                           # kBlock


def matmul_class(m, n, k, ta, tb, f16):
    """none | memset | (single: full grid / short k | split: the last split full / one element / no multiple of 16 / a shorter multiple
    of 16) x how the two operands are staged x the fp16 rounding."""
    f = matmul_form(m, n, k, ta, tb, f16)
    kind = MATMUL_KINDS[f['kind']]
    if kind in ('none', 'memset'):
        return ('MatMul', kind)
    if kind == 'single':
        sub = 'single-full-grid' if f['gx'] * f['gy'] >= 512 else 'single-short-k'
        assert f['splits'] == 1 and f['last_k'] == k
    else:
        assert f['splits'] >= 2 and f['k_chunk'] % 16 == 0 and 0 < f['last_k'] <= f['k_chunk']
        assert (f['splits'] - 1) * f['k_chunk'] + f['last_k'] == k
        last = f['last_k']
        sub = 'split-last-full' if last == f['k_chunk'] else 'split-last-one' if last == 1 else 'split-last-ragged' if last % 16 else 'split-last-short16'
    return ('MatMul', sub, 'a-k-fast' if f['akf'] else 'a-m-fast', 'b-n-fast' if f['bnf'] else 'b-k-fast', 'f16' if f['f16'] else 'f32')


def unary_class(n):
    """nt | wraps | whole runs x float4 remainder x scalar tail (none / one element / several)."""
    f = unary_form(n)
    if f['kind'] == NONE:
        return ('Unary', 'none')
    assert f['u'] == (4 if f['nt'] else 1)
    if f['nt']:
        return ('Unary', 'nt', 'wraps' if f['wraps'] else 'one-sweep')
    if f['wraps']:
        return ('Unary', 'wraps')
    return ('Unary', 'runs' if f['runs'] else 'no-runs', 'rem4' if f['rem4'] else 'no-rem4', ('no-tail', 'tail-1', 'tail-2+', 'tail-2+')[n % 4])


def binary_class(a_shape, b_shape, commutative=True):
    """The kernel x which operand is broadcast (b / a; a non-commutative op then swaps) x the part of the kernel the sizes reach:
    same: no float4 at all / the two-at-a-time loop only / a trailing single iteration only / both, x the scalar tail;
    channel: scalar / inner == 1 / inner % 4 != 0 / inner % 4 == 0 (there because n % 4 != 0), x no float4 / tail / no tail;
    channel4: C on one axis or spread over several, x whole runs present or not;  strided: the rank."""
    f = binary_form(a_shape, b_shape, commutative)
    if f['kind'] == NONE:
        return ('Binary', 'none')
    kind, n = BINARY_KINDS[f['kind']], f['n']
    n4 = n // 4
    assert f['nt'] == 0, 'a nontemporal form in the table'
    who = ('both-full', 'b-broadcast', 'a-broadcast')[f['bcast']] + ('-swapped' if f['swap'] else '')
    tail = 'no-float4' if n4 == 0 else 'tail' if n % 4 else 'no-tail'
    if kind == 'same':
        stride = f['grid'] * BLOCK
        loop = 'none' if n4 == 0 else 'singles' if n4 <= stride else 'pairs+single' if n4 < 2 * stride else 'pairs'
        return ('Binary', kind, loop, 'tail' if n % 4 else 'no-tail')
    if kind == 'channel':
        sub = 'scalar' if f['C'] == 1 else 'inner=1' if f['inner'] == 1 else 'inner%4' if f['inner'] % 4 else 'inner4'
        return ('Binary', kind, who, sub, tail)
    if kind == 'channel4':
        small = a_shape if f['bcast'] == 2 else b_shape
        axes = sum(1 for d in small if d != 1)
        assert f['inner'] % 4 == 0 and n % 4 == 0
        return ('Binary', kind, who, 'one-axis' if axes <= 1 else 'axes-spread', 'runs' if n4 >= BLOCK else 'no-runs')
    return ('Binary', kind, 'rank-{}'.format(len(np.broadcast_shapes(tuple(a_shape), tuple(b_shape)))))


def concat_geometry(shapes, axis):
    """(inner per source, outer) as op_plugins/Concat.py hands them to the entry."""
    first = shapes[0]
    outer = int(np.prod(first[:axis], dtype=np.int64))
    tail = int(np.prod(first[axis + 1:], dtype=np.int64))
    return [int(s[axis]) * tail for s in shapes], outer


def concat_class(inner, outer):
    """vec4 / scalar x the first that holds of: the most sources the entry takes; a zero-length source; outer == 1; every source one
    element per step; none of these ('plain')."""
    f = concat_form(inner, outer)
    if f['kind'] == NONE:
        return ('Concat', 'none')
    assert f['gy'] == len(inner)
    sub = ('max-sources' if len(inner) == 16 else 'empty-source' if 0 in inner else 'outer=1' if outer == 1 else
           'inner=1' if max(inner) == 1 else 'plain')
    return ('Concat', 'vec4' if f['kind'] == 1 else 'scalar', sub, 'one-block' if f['gx'] == 1 else 'blocks')


def input_class(n, c, h, w, u8, nhwc, src_align, dst_align):
    """copy | u8-linear: the destination off 16 bytes / fewer than four elements / source alignment x total % 4 |
    nhwc: T x (c == 1 | 16-byte loads x 16-byte stores x (a tile of 1 or 2 pixels / one partial tile / whole tiles and a partial last
    one / whole tiles))."""
    f = input_form(n, c, h, w, u8, nhwc, src_align, dst_align)
    total, p = n * c * h * w, h * w
    if f['kind'] == 0:
        return ('Input', 'copy')
    if f['kind'] == 1:
        if dst_align:
            assert not f['vec']
            return ('Input', 'u8-linear', 'dst-offset')
        if total < 4:
            assert not f['vec']
            return ('Input', 'u8-linear', 'tiny')
        assert f['vec'] == int(src_align % 4 == 0)
        return ('Input', 'u8-linear', 'src%4={}'.format(src_align % 4), 'total%4={}'.format(total % 4))
    assert f['gx'] == -(-p // f['tile']) and f['gy'] == n
    t = 'u8' if u8 else 'f32'
    if c == 1:
        return ('Input', 'nhwc', t, 'c=1')
    sub = ('tile={}'.format(f['tile']) if f['tile'] < 4 else 'one-partial-tile' if p < f['tile'] else 'partial-last-tile' if p % f['tile'] else
           'whole-tiles')
    return ('Input', 'nhwc', t, 'VL' if f['vl'] else 'scalar-loads', 'VS' if f['vs'] else 'scalar-stores', sub)


# --------------------------------------------------------------------------------------------------------------------- the table
class Row:
    def __init__(self, id_, family, cls, env=None, edge=None, where='here', **kw):
        self.id, self.family, self.cls, self.env, self.edge, self.where, self.kw = id_, family, cls, dict(env or {}), edge, where, kw

    def __repr__(self):
        return self.id


ROWS = []

# ---- MatMul: every class with the four transpose pairs, fp32 and f16
MATMUL_SHAPES = [('single-full-grid', (1472, 1472, 17)),      # 23 x 23 tiles: no ragged tile, a ragged K chunk
                 ('single-short-k', (65, 1, 17)),             # a ragged M tile, N = 1
                 ('split-last-full', (64, 64, 576)),
                 ('split-last-one', (64, 64, 257)),           # five chunks of 64, the last holds k = 256 alone
                 ('split-last-ragged', (3, 513, 100)),        # 64 + 36
                 ('split-last-short16', (64, 64, 272))]       # 4 x 64 + 16
TT = [(0, 0), (0, 1), (1, 0), (1, 1)]
for _sub, (_m, _n, _k) in MATMUL_SHAPES:
    for _ta, _tb in TT:
        for _f16 in (0, 1):
            ROWS.append(Row('MatMul-{}-{}x{}x{}-t{}{}-{}'.format(_sub, _m, _n, _k, _ta, _tb, 'f16' if _f16 else 'f32'), 'matmul',
                            ('MatMul', _sub, 'a-m-fast' if _ta else 'a-k-fast', 'b-k-fast' if _tb else 'b-n-fast', 'f16' if _f16 else 'f32'),
                            m=_m, n=_n, k=_k, ta=_ta, tb=_tb, f16=_f16))
ROWS += [
    Row('MatMul-memset-5x70x0', 'matmul', ('MatMul', 'memset'), m=5, n=70, k=0, ta=0, tb=0, f16=0),
    Row('MatMul-empty', 'matmul', ('MatMul', 'none'), m=0, n=5, k=3, ta=0, tb=0, f16=0),          # the GPU row launches n == 0 too
    # the FC size of both IRs at batch 256: the one large row, one transpose pair per type
    Row('MatMul-fc-256x1000x1024-f32', 'matmul', ('MatMul', 'split-last-full', 'a-k-fast', 'b-k-fast', 'f32'), edge='the FC size',
        m=256, n=1000, k=1024, ta=0, tb=1, f16=0),
    Row('MatMul-fc-256x1000x1024-f16', 'matmul', ('MatMul', 'split-last-full', 'a-k-fast', 'b-k-fast', 'f16'), edge='the FC size',
        m=256, n=1000, k=1024, ta=0, tb=1, f16=1),
]
# a NaN in A and an Inf in B, in ragged tiles; SINGLE: in the ragged K chunk; SPLIT: in the last split (k = 192 .. 199 of 200)
for _f16 in (0, 1):
    ROWS += [Row('MatMul-poison-single-65x70x17-{}'.format('f16' if _f16 else 'f32'), 'matmul',
                 ('MatMul', 'single-short-k', 'a-k-fast', 'b-k-fast', 'f16' if _f16 else 'f32'), edge='NaN / Inf through the zero fill',
                 m=65, n=70, k=17, ta=0, tb=1, f16=_f16, poison=((64, 16), (3, 69))),
             Row('MatMul-poison-split-65x70x200-{}'.format('f16' if _f16 else 'f32'), 'matmul',
                 ('MatMul', 'split-last-ragged', 'a-m-fast', 'b-n-fast', 'f16' if _f16 else 'f32'), edge='NaN / Inf through the zero fill',
                 m=65, n=70, k=200, ta=1, tb=0, f16=_f16, poison=((64, 193), (198, 69)))]

# ---- unary (ReLU, Clamp 0..6 and Sigmoid on every row)
for _n, _cls in [(1, ('no-runs', 'no-rem4', 'tail-1')), (3, ('no-runs', 'no-rem4', 'tail-2+')), (4, ('no-runs', 'rem4', 'no-tail')),
                 (5, ('no-runs', 'rem4', 'tail-1')), (1023, ('no-runs', 'rem4', 'tail-2+')),                 # just below one workgroup of 256 float4
                 (1024, ('runs', 'no-rem4', 'no-tail')), (1025, ('runs', 'no-rem4', 'tail-1')), (1026, ('runs', 'no-rem4', 'tail-2+')),
                 (1028, ('runs', 'rem4', 'no-tail')), (1029, ('runs', 'rem4', 'tail-1')), (1031, ('runs', 'rem4', 'tail-2+'))]:
    ROWS.append(Row('Unary-n{}'.format(_n), 'unary', ('Unary',) + _cls, n=_n))
ROWS += [
    # PVHIP_STREAM_WG=1: 256 workgroups, 2 x 256 + 3 whole runs, 100 float4 behind them and a tail of three
    Row('Unary-wraps-n527759', 'unary', ('Unary', 'wraps'), env=WG1_ENV, n=(2 * 256 + 3) * 1024 + 400 + 3),
    # the <true, 4> instantiation at the shape of test_nontemporal_streaming_forms_at_small_sizes, which runs it
    Row('Unary-nt-n10638649', 'unary', ('Unary', 'nt', 'wraps'), env=NT_ENV, where='test_hip_ops', n=7 * 1519807),
    # PVHIP_STREAM_NT=2 on fewer than four elements: no run at all, the scalar tail still needs its workgroup
    Row('Unary-nt-n3', 'unary', ('Unary', 'nt', 'one-sweep'), env=NT_ENV, n=3),
]


# ---- binary (Add and Multiply on every row, through op_plugins/_broadcast.py); the shapes are the smallest of each class
def bi(id_, a, b, *cls, **opt):
    return Row('Binary-' + id_, 'binary', ('Binary',) + cls, a=a, b=b, **opt)


ROWS += [
    bi('same-no-float4', (3,), (3,), 'same', 'none', 'tail'),
    bi('same-singles', (4, 1, 1, 1), (4, 1, 1, 1), 'same', 'singles', 'no-tail'),
    bi('same-singles-tail', (5,), (5,), 'same', 'singles', 'tail'),
    bi('same-pairs-single', (260, 4), (260, 4), 'same', 'pairs+single', 'no-tail'),           # lane 0..3 take two float4, the others one
    bi('same-pairs-single-tail', (13, 2, 5, 3, 5), (13, 2, 5, 3, 5), 'same', 'pairs+single', 'tail'),
    bi('same-pairs', (16, 8, 2, 2, 2, 2), (16, 8, 2, 2, 2, 2), 'same', 'pairs', 'no-tail'),
    bi('same-rank0', (), (), 'same', 'none', 'tail', edge='rank 0: one element, no shape arrays'),
    bi('channel-b-inner-odd', (2, 2), (2, 1), 'channel', 'b-broadcast', 'inner%4', 'no-tail'),
    bi('channel-b-inner-odd-tail', (3, 5, 7, 7), (1, 5, 1, 1), 'channel', 'b-broadcast', 'inner%4', 'tail'),
    bi('channel-b-inner1', (2, 4), (1, 4), 'channel', 'b-broadcast', 'inner=1', 'no-tail'),
    bi('channel-b-inner1-tail', (7, 13), (1, 13), 'channel', 'b-broadcast', 'inner=1', 'tail'),
    bi('channel-b-scalar-no-float4', (1, 1, 1, 2), (1, 1, 1, 1), 'channel', 'b-broadcast', 'scalar', 'no-float4'),
    bi('channel-b-scalar', (2, 3, 4, 5), (1, 1, 1, 1), 'channel', 'b-broadcast', 'scalar', 'no-tail'),
    bi('channel-b-scalar-tail', (5,), (1,), 'channel', 'b-broadcast', 'scalar', 'tail'),
    bi('channel-a-inner-odd', (2, 1), (2, 2), 'channel', 'a-broadcast', 'inner%4', 'no-tail'),
    bi('channel-a-inner-odd-tail', (1, 5, 1, 1), (3, 5, 7, 7), 'channel', 'a-broadcast', 'inner%4', 'tail'),
    bi('channel-a-inner1', (1, 1, 2, 1), (2, 1, 2, 1), 'channel', 'a-broadcast', 'inner=1', 'no-tail'),
    bi('channel-a-inner1-tail', (13,), (7, 13), 'channel', 'a-broadcast', 'inner=1', 'tail'),
    bi('channel-a-scalar-no-float4', (1,), (2,), 'channel', 'a-broadcast', 'scalar', 'no-float4'),
    bi('channel-a-scalar', (1,), (4,), 'channel', 'a-broadcast', 'scalar', 'no-tail'),
    bi('channel-a-scalar-tail', (1,), (5,), 'channel', 'a-broadcast', 'scalar', 'tail'),
    bi('channel4-b-one-axis', (2, 4), (2, 1), 'channel4', 'b-broadcast', 'one-axis', 'no-runs'),
    bi('channel4-b-one-axis-runs', (4, 1, 4, 16, 4), (4, 1, 1, 1, 1), 'channel4', 'b-broadcast', 'one-axis', 'runs'),
    bi('channel4-b-axes-spread', (2, 3, 5, 8), (1, 3, 5, 1), 'channel4', 'b-broadcast', 'axes-spread', 'no-runs'),   # C = 15 over two axes
    bi('channel4-b-axes-spread-runs', (8, 4, 16, 2), (8, 4, 1, 1), 'channel4', 'b-broadcast', 'axes-spread', 'runs'),
    bi('channel4-a-one-axis', (1, 3, 1, 1), (2, 3, 4, 4), 'channel4', 'a-broadcast', 'one-axis', 'no-runs'),         # the broadcast operand first
    bi('channel4-a-one-axis-runs', (1, 8, 1, 1), (8, 2, 8, 2, 4), 'channel4', 'a-broadcast', 'one-axis', 'runs'),
    bi('channel4-a-axes-spread', (1, 3, 5, 1), (2, 3, 5, 8), 'channel4', 'a-broadcast', 'axes-spread', 'no-runs'),
    bi('channel4-a-axes-spread-runs', (3, 8, 1, 1, 1), (3, 8, 2, 3, 8), 'channel4', 'a-broadcast', 'axes-spread', 'runs'),
    bi('strided-rank2', (1, 2), (4, 1), 'strided', 'rank-2'),                                   # both operands broadcast
    bi('strided-rank3', (3, 2, 2), (3, 1, 2), 'strided', 'rank-3'),
    bi('strided-rank4', (2, 3, 4, 5), (1, 3, 1, 5), 'strided', 'rank-4'),
    bi('strided-rank5', (2, 3, 4, 2, 5), (2, 3, 1, 2, 5), 'strided', 'rank-5'),                  # a stride-0 axis in the middle
    bi('strided-rank6', (2, 3, 2, 2, 3, 5), (2, 3, 1, 2, 1, 5), 'strided', 'rank-6'),
]
# The kSwap instantiations (a - b with the broadcast operand first): the diagnostic build's pvhip_diag_sub_f32, run by
# tests/diag_variants.py::test_subtract_reaches_the_swapped_channel_kernels in that library's own process.
SUB_ROWS = [
    bi('swap-channel-inner-odd', (2, 1), (2, 2), 'channel', 'a-broadcast-swapped', 'inner%4', 'no-tail', where='diag_variants'),
    bi('swap-channel-inner-odd-tail', (1, 5, 1, 1), (3, 5, 7, 7), 'channel', 'a-broadcast-swapped', 'inner%4', 'tail', where='diag_variants'),
    bi('swap-channel-inner1', (1, 1, 2, 1), (2, 1, 2, 1), 'channel', 'a-broadcast-swapped', 'inner=1', 'no-tail', where='diag_variants'),
    bi('swap-channel-inner1-tail', (13,), (7, 13), 'channel', 'a-broadcast-swapped', 'inner=1', 'tail', where='diag_variants'),
    bi('swap-channel-scalar-no-float4', (1,), (2,), 'channel', 'a-broadcast-swapped', 'scalar', 'no-float4', where='diag_variants'),
    bi('swap-channel-scalar', (1,), (4,), 'channel', 'a-broadcast-swapped', 'scalar', 'no-tail', where='diag_variants'),
    bi('swap-channel-scalar-tail', (1,), (5,), 'channel', 'a-broadcast-swapped', 'scalar', 'tail', where='diag_variants'),
    bi('swap-channel4-one-axis', (1, 3, 1, 1), (2, 3, 4, 4), 'channel4', 'a-broadcast-swapped', 'one-axis', 'no-runs', where='diag_variants'),
    bi('swap-channel4-one-axis-runs', (1, 8, 1, 1), (8, 2, 8, 2, 4), 'channel4', 'a-broadcast-swapped', 'one-axis', 'runs', where='diag_variants'),
    bi('swap-channel4-axes-spread', (1, 3, 5, 1), (2, 3, 5, 8), 'channel4', 'a-broadcast-swapped', 'axes-spread', 'no-runs', where='diag_variants'),
    bi('swap-channel4-axes-spread-runs', (3, 8, 1, 1, 1), (3, 8, 2, 3, 8), 'channel4', 'a-broadcast-swapped', 'axes-spread', 'runs', where='diag_variants'),
]
for _r in SUB_ROWS:
    _r.kw['commutative'] = False
ROWS += SUB_ROWS


# ---- Concat: the sources as shapes and the axis, as the plugin takes them
def cat(id_, shapes, axis, *cls, **opt):
    return Row('Concat-' + id_, 'concat', ('Concat',) + cls, shapes=shapes, axis=axis, **opt)


ROWS += [
    cat('vec4-16-sources', [(3, 4)] * 16, 1, 'vec4', 'max-sources', 'one-block'),
    cat('vec4-16-sources-blocks', [(7, 4)] * 7 + [(7, 0), (7, 160)] + [(7, 8)] * 7, 1, 'vec4', 'max-sources', 'blocks'),
    cat('scalar-16-sources', [(2, 1)] * 15 + [(2, 3)], 1, 'scalar', 'max-sources', 'one-block'),
    cat('scalar-16-sources-blocks', [(7, 1)] * 14 + [(7, 0), (7, 70)], 1, 'scalar', 'max-sources', 'blocks'),
    cat('vec4-empty-middle-and-end', [(2, 4), (2, 0), (2, 8), (2, 0)], 1, 'vec4', 'empty-source', 'one-block'),
    cat('vec4-empty-middle-blocks', [(300, 4), (300, 0), (300, 8)], 1, 'vec4', 'empty-source', 'blocks'),
    cat('scalar-empty-middle-and-end', [(2, 3), (2, 0), (2, 5), (2, 0)], 1, 'scalar', 'empty-source', 'one-block'),
    cat('scalar-empty-middle-blocks', [(300, 1), (300, 0), (300, 2)], 1, 'scalar', 'empty-source', 'blocks'),
    cat('vec4-axis0', [(8,), (12,)], 0, 'vec4', 'outer=1', 'one-block'),
    cat('scalar-axis0', [(2, 5), (3, 5)], 0, 'scalar', 'outer=1', 'one-block'),
    cat('scalar-inner1', [(2, 1), (2, 1)], 1, 'scalar', 'inner=1', 'one-block'),
    cat('scalar-inner1-outer70000', [(70000, 1)] * 3, 1, 'scalar', 'inner=1', 'blocks'),
    cat('scalar-one-odd-source', [(2, 4, 5), (2, 3, 5), (2, 4, 5)], 1, 'scalar', 'plain', 'one-block'),       # 20, 15, 20: one inner % 4 != 0
    cat('scalar-blocks', [(7, 70), (7, 3)], 1, 'scalar', 'plain', 'blocks'),
    cat('vec4-plain', [(2, 4), (2, 4), (2, 4)], 1, 'vec4', 'plain', 'one-block'),
    cat('vec4-blocks', [(7, 160), (7, 4)], 1, 'vec4', 'plain', 'blocks'),
    cat('empty-output', [(0, 3), (0, 5)], 1, 'none'),
]


# ---- the input layouts: (n, c, h, w, u8, nhwc, source offset, destination offset) inside one allocation each
def inp(n, c, h, w, u8, nhwc, sa, da, *cls, **opt):
    return Row('Input-{}-{}x{}x{}x{}-src{}-dst{}'.format('-'.join(cls).replace('%', 'mod').replace('=', ''), n, c, h, w, sa, da), 'input',
               ('Input',) + cls, n=n, c=c, h=h, w=w, u8=u8, nhwc=nhwc, sa=sa, da=da, **opt)


ROWS += [
    inp(1, 3, 5, 7, 0, 0, 0, 0, 'copy'),
    inp(1, 1, 1, 3, 1, 0, 0, 0, 'u8-linear', 'tiny'),
    inp(2, 3, 5, 7, 1, 0, 0, 8, 'u8-linear', 'dst-offset'),
] + [inp(1, 1, 3, 5 + _t, 1, 0, _sa, 0, 'u8-linear', 'src%4={}'.format(_sa), 'total%4={}'.format((15 + 3 * _t) % 4)) for _sa in range(4) for _t in range(4)] + [
    inp(1, 1, 5, 5, 1, 1, 0, 0, 'nhwc', 'u8', 'c=1'),
    inp(1, 1, 5, 5, 0, 1, 4, 4, 'nhwc', 'f32', 'c=1'),
    inp(1, 2, 1, 8, 1, 1, 0, 0, 'nhwc', 'u8', 'VL', 'VS', 'one-partial-tile'),
    inp(1, 2, 8, 150, 1, 1, 0, 0, 'nhwc', 'u8', 'VL', 'VS', 'partial-last-tile'),
    inp(2, 3, 8, 128, 1, 1, 0, 0, 'nhwc', 'u8', 'VL', 'VS', 'whole-tiles'),
    inp(1, 8, 2, 1, 1, 1, 0, 12, 'nhwc', 'u8', 'VL', 'scalar-stores', 'one-partial-tile'),
    inp(1, 4096, 2, 3, 1, 1, 0, 0, 'nhwc', 'u8', 'VL', 'scalar-stores', 'partial-last-tile'),       # tile = 4, p = 6
    inp(1, 4096, 2, 2, 1, 1, 0, 12, 'nhwc', 'u8', 'VL', 'scalar-stores', 'whole-tiles'),
    inp(1, 2, 2, 2, 1, 1, 1, 0, 'nhwc', 'u8', 'scalar-loads', 'VS', 'one-partial-tile'),
    inp(1, 2, 8, 150, 1, 1, 2, 0, 'nhwc', 'u8', 'scalar-loads', 'VS', 'partial-last-tile'),
    inp(1, 2, 8, 128, 1, 1, 1, 0, 'nhwc', 'u8', 'scalar-loads', 'VS', 'whole-tiles'),
    inp(1, 3, 1, 1, 1, 1, 1, 8, 'nhwc', 'u8', 'scalar-loads', 'scalar-stores', 'one-partial-tile'),
    inp(1, 2, 7, 150, 1, 1, 0, 0, 'nhwc', 'u8', 'scalar-loads', 'scalar-stores', 'partial-last-tile'),  # p * c = 2100: no 16-byte spans
    inp(1, 5, 8, 128, 1, 1, 1, 4, 'nhwc', 'u8', 'scalar-loads', 'scalar-stores', 'whole-tiles'),
    inp(1, 2, 1, 4, 0, 1, 0, 0, 'nhwc', 'f32', 'VL', 'VS', 'one-partial-tile'),
    inp(1, 2, 8, 150, 0, 1, 0, 0, 'nhwc', 'f32', 'VL', 'VS', 'partial-last-tile'),
    inp(1, 2, 8, 128, 0, 1, 0, 0, 'nhwc', 'f32', 'VL', 'VS', 'whole-tiles'),
    inp(1, 2, 1, 2, 0, 1, 0, 4, 'nhwc', 'f32', 'VL', 'scalar-stores', 'one-partial-tile'),
    inp(1, 2, 7, 150, 0, 1, 0, 8, 'nhwc', 'f32', 'VL', 'scalar-stores', 'partial-last-tile'),
    inp(1, 4, 8, 128, 0, 1, 0, 4, 'nhwc', 'f32', 'VL', 'scalar-stores', 'whole-tiles'),
    inp(2, 4096, 1, 3, 0, 1, 0, 0, 'nhwc', 'f32', 'VL', 'scalar-stores', 'tile=1'),                  # one pixel fills the 16 KB tile
    inp(1, 2048, 1, 3, 0, 1, 0, 12, 'nhwc', 'f32', 'VL', 'scalar-stores', 'tile=2'),
    inp(1, 2, 2, 2, 0, 1, 4, 0, 'nhwc', 'f32', 'scalar-loads', 'VS', 'one-partial-tile'),
    inp(1, 5, 6, 150, 0, 1, 8, 0, 'nhwc', 'f32', 'scalar-loads', 'VS', 'partial-last-tile'),
    inp(1, 64, 8, 8, 0, 1, 4, 0, 'nhwc', 'f32', 'scalar-loads', 'VS', 'whole-tiles'),
    inp(1, 2, 1, 2, 0, 1, 8, 0, 'nhwc', 'f32', 'scalar-loads', 'scalar-stores', 'one-partial-tile'),
    inp(1, 2, 7, 150, 0, 1, 4, 12, 'nhwc', 'f32', 'scalar-loads', 'scalar-stores', 'partial-last-tile'),
    inp(1, 5, 4, 128, 0, 1, 4, 4, 'nhwc', 'f32', 'scalar-loads', 'scalar-stores', 'whole-tiles'),
    inp(1, 4096, 1, 2, 0, 1, 4, 12, 'nhwc', 'f32', 'scalar-loads', 'scalar-stores', 'tile=1'),
    inp(1, 1030, 1, 3, 0, 1, 4, 0, 'nhwc', 'f32', 'scalar-loads', 'scalar-stores', 'tile=2'),        # two pixels of 1030 floats: 8240 bytes
]


# ---- one kernel each, no planner: the rows carry names (FIXED_CLASSES)
def fixed(family, id_, **kw):
    return Row('{}-{}'.format(family.capitalize(), id_), family, (family.capitalize(), id_), **kw)


_P6 = (2, 3, 5, 7, 11, 13)
ROWS += [fixed('transpose', 'perm' + ''.join(map(str, p)), shape=(2, 3, 5), perm=p) for p in itertools.permutations(range(3))]
ROWS += [
    fixed('transpose', 'rank6-seed1', shape=_P6, perm=tuple(int(v) for v in np.random.RandomState(1).permutation(6))),
    fixed('transpose', 'rank6-seed2', shape=_P6, perm=tuple(int(v) for v in np.random.RandomState(2).permutation(6))),
    fixed('transpose', 'rank6-reversed', shape=_P6, perm=(5, 4, 3, 2, 1, 0)),
    fixed('transpose', 'unit-axis', shape=(3, 1, 5, 1), perm=(2, 1, 3, 0)),
    fixed('transpose', 'empty', shape=(3, 0, 5), perm=(2, 0, 1)),
    # (n, c, h, w), (top, left, bottom, right), channel_add
    fixed('pad2d', 'no-pad', xs=(2, 3, 5, 7), pads=(0, 0, 0, 0), add=False),
    fixed('pad2d', 'top', xs=(2, 3, 5, 7), pads=(2, 0, 0, 0), add=False),
    fixed('pad2d', 'left', xs=(2, 3, 5, 7), pads=(0, 3, 0, 0), add=False),
    fixed('pad2d', 'bottom', xs=(2, 3, 5, 7), pads=(0, 0, 1, 0), add=False),
    fixed('pad2d', 'right', xs=(2, 3, 5, 7), pads=(0, 0, 0, 2), add=False),
    fixed('pad2d', 'wider-than-the-image', xs=(1, 2, 2, 3), pads=(5, 7, 4, 9), add=False),
    fixed('pad2d', 'channel-add', xs=(2, 3, 5, 7), pads=(1, 2, 3, 1), add=True),
    fixed('pad2d', 'blocks', xs=(1, 2, 40, 50), pads=(1, 1, 1, 1), add=True),              # 42 x 52 outputs: three workgroups per plane
    fixed('pad2d', '65535-planes', xs=(21845, 3, 1, 1), pads=(0, 0, 0, 0), add=True),
] + [fixed('c8', 'c{}'.format(c), c=c) for c in (1, 3, 8, 15, 16, 17, 40)]

# ---- refusals: the size check precedes every use of a pointer (read in the entries), so the rows pass dummy pointers
ROWS += [
    Row('MatMul-refused-m-4194241', 'refusal', ('Refusal', 'matmul'), edge='M > 65535 * 64'),
    Row('Concat-refused-17-sources', 'refusal', ('Refusal', 'concat-plugin'), edge='more than MAX_CONCAT sources'),
    Row('Concat-refused-2^31', 'refusal', ('Refusal', 'concat-entry'), edge='2^31 elements'),
    Row('Pad2d-refused-65536-planes', 'refusal', ('Refusal', 'pad2d'), edge='n * c == 65536'),
    Row('Input-refused-c-4097', 'refusal', ('Refusal', 'input'), edge='c > 4096 for NHWC'),
]

ROW_IDS = [r.id for r in ROWS]
assert len(set(ROW_IDS)) == len(ROW_IDS)
HERE = [r for r in ROWS if r.where == 'here']                        # the rows this module launches

# rows that share their class with a plain row (or have none): pinned by name, so that deleting one fails the coverage test too
EDGE_ROWS = {'MatMul-fc-256x1000x1024-f32', 'MatMul-fc-256x1000x1024-f16', 'MatMul-poison-single-65x70x17-f32', 'MatMul-poison-single-65x70x17-f16',
             'MatMul-poison-split-65x70x200-f32', 'MatMul-poison-split-65x70x200-f16', 'Binary-same-rank0', 'MatMul-refused-m-4194241',
             'Concat-refused-17-sources', 'Concat-refused-2^31', 'Pad2d-refused-65536-planes', 'Input-refused-c-4097'}
# classes no sweep of the planners under the default settings returns: the names of the single-kernel rows, and the forms behind
# PVHIP_STREAM_NT=2 (by default from 64 MiB moved on; the binary kernels' nontemporal forms: test_nontemporal_streaming_forms_at_small_sizes)
FIXED_CLASSES = {r.cls for r in ROWS if r.family in ('transpose', 'pad2d', 'c8')} | {('Unary', 'nt', 'wraps'), ('Unary', 'nt', 'one-sweep')}


# ------------------------------------------------------------------------------------------- every class the planners can return
def _shape_pair(rng):
    """Two broadcastable shapes of rank 0..6: equal; b keeps a run of adjacent axes; b keeps any axes; b is a scalar; both broadcast."""
    rank = int(rng.randint(0, 7))
    out = [int(rng.choice([1, 2, 3, 4, 5, 8, 13, 16, 260])) for _ in range(rank)]
    while np.prod(out, dtype=np.int64) > 200000:
        out[int(rng.randint(rank))] = 2
    mode = int(rng.randint(5))
    a, b = list(out), list(out)
    if mode == 1 and rank:
        lo = int(rng.randint(rank))
        hi = int(rng.randint(lo, rank))
        b = [d if lo <= i <= hi else 1 for i, d in enumerate(out)]
    elif mode == 2:
        b = [d if rng.randint(2) else 1 for d in out]
    elif mode == 3:
        b = [1] * rank
    elif mode == 4:
        a = [d if rng.randint(4) else 1 for d in out]
        b = [d if rng.randint(2) or a[i] == 1 else 1 for i, d in enumerate(out)]
    lead = int(rng.randint(rank + 1)) if mode in (1, 3) else 0
    if all(d == 1 for d in b[:lead]):
        b = b[lead:]                                  # a broadcast operand of lower rank
    return tuple(a), tuple(b)


@functools.lru_cache(maxsize=None)
def planner_classes():
    """The classes the five planners return over a seeded sweep of launches (default settings; PVHIP_STREAM_WG=1 is not needed: the
    unary sweep reaches sizes whose run loop wraps)."""
    seen = set()
    rng = np.random.RandomState(1)
    for _ in range(4000):
        m = int(rng.choice([0, 1, rng.randint(1, 200), rng.randint(1, 3000)]))
        n = int(rng.choice([0, 1, rng.randint(1, 200), rng.randint(1, 3000)]))
        k = int(rng.choice([0, 1, rng.randint(1, 130), rng.randint(1, 1500), 64 * rng.randint(1, 20) + 1, 16 * rng.randint(1, 80)]))
        seen.add(matmul_class(m, n, k, int(rng.randint(2)), int(rng.randint(2)), int(rng.randint(2))))
    rng = np.random.RandomState(2)
    for n in list(range(0, 2100)) + [int(v) for v in rng.randint(1, 1 << 23, 300)]:            # below 2^23 elements: 64 MiB moved
        seen.add(unary_class(n))
    rng = np.random.RandomState(3)
    for _ in range(6000):
        a, b = _shape_pair(rng)
        if rng.randint(2):
            a, b = b, a
        seen.add(binary_class(a, b, True))
        seen.add(binary_class(a, b, False))
    rng = np.random.RandomState(4)
    for _ in range(4000):
        unit = int(rng.choice([1, 1, 4]))
        inner = [int(rng.choice([0, 1, 2, 3, 5, 70])) * unit for _ in range(int(rng.choice([2, 3, 5, 16])))]
        if rng.randint(3) == 0:
            inner = [min(v, 1) for v in inner]
        seen.add(concat_class(inner, int(rng.choice([0, 1, 2, 7, 300, 70000]))))
    for sa in range(4):                                # the widening copy: every source alignment x total % 4, and the other two
        for total in range(1, 12):
            seen.add(input_class(1, 1, 1, total, 1, 0, sa, 0))
            seen.add(input_class(1, 1, 1, total, 1, 0, sa, 4 * (1 + total % 3)))
    rng = np.random.RandomState(5)
    for _ in range(8000):
        u8, nhwc = int(rng.randint(2)), int(rng.randint(2))
        c = int(rng.choice([1, 2, 3, 4, 5, 8, 16, 64, 1030, 2048, 4096]))
        h, w = int(rng.randint(1, 9)), int(rng.choice([1, 2, 3, 4, 5, 8, 32, 40, 128, 150]))
        if c > 64:
            h, w = int(rng.randint(1, 3)), int(rng.randint(1, 4))
        sa = int(rng.choice([0, 1, 2, 3])) if u8 else int(rng.choice([0, 4, 8]))
        seen.add(input_class(int(rng.randint(1, 3)), c, h, w, u8, nhwc, sa, int(rng.choice([0, 0, 0, 4, 8, 12]))))
    return frozenset(seen)


# classes of the sweep that launch nothing and have no row of their own kind (their entries' early returns: the MatMul and Concat rows
# 'empty' cover two of them on the device)
NOTHING_LAUNCHED = {('Unary', 'none'), ('Binary', 'none')}


def class_of(row):
    """The class of the row's launch as the library's query answers it (host-only)."""
    kw = row.kw
    if row.family == 'matmul':
        return matmul_class(kw['m'], kw['n'], kw['k'], kw['ta'], kw['tb'], kw['f16'])
    if row.family == 'unary':
        return unary_class(kw['n'])
    if row.family == 'binary':
        return binary_class(kw['a'], kw['b'], kw.get('commutative', True))
    if row.family == 'concat':
        return concat_class(*concat_geometry(kw['shapes'], kw['axis']))
    if row.family == 'input':
        return input_class(*(kw[k] for k in ('n', 'c', 'h', 'w', 'u8', 'nhwc', 'sa', 'da')))
    return row.cls                                     # one kernel, no planner


class Env:
    """The row's PVHIP_* switches, read by the library for the length of the block."""

    def __init__(self, row, monkeypatch):
        self.row, self.monkeypatch = row, monkeypatch

    def __enter__(self):
        for name, value in self.row.env.items():
            helpers.setenv(self.monkeypatch, name, value)

    def __exit__(self, *exc):
        for name in self.row.env:
            helpers.setenv(self.monkeypatch, name, None)


# ------------------------------------------------------------------------------------------------ inputs and float64 references
UNARY_OPS = ('ReLU', 'Clamp', 'Sigmoid')
CLAMP_LO, CLAMP_HI = 0.0, 6.0
# -0.0 (kept by all three: (v < 0) is false, and np.clip keeps it), +-inf, NaN, subnormals, Clamp's bounds and their neighbours
UNARY_SPECIALS = np.array([-0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-40, 0.0, 6.0, 5.9999995, 6.0000005, -1e-45, 7.0, -7.0], dtype=np.float32)
# fp16 edges: 65520 is the tie between 65504 and 2^16 (to even: inf), 65519.996 the fp32 below it (to 65504); 2^-24 the smallest fp16
# subnormal, 2^-25 half of it (a tie: to even, 0), the fp32 above 2^-25 (to 2^-24); 3, 5, 7 x 2^-25 ties at subnormal spacing (to 2, 2, 4
# x 2^-24); 2^-14 the smallest normal and the tie below it; 1 + 2^-11 and 1 + 3 x 2^-11 ties at normal spacing (to 1 and 1 + 2^-9)
C8_SPECIALS = np.array([65520.0, 65519.996, -65520.0, 65504.0, 2.0 ** -24, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)),
                        3 * 2.0 ** -25, 5 * 2.0 ** -25, 7 * 2.0 ** -25, -0.0, np.inf, -np.inf, np.nan, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25,
                        1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(2.0 ** -25), 1e-10, 70000.0, 0.0], dtype=np.float32)


def _rng(row):
    return np.random.RandomState(zlib.crc32(row.id.encode()) & 0x7fffffff)


def _with_specials(x, specials, rotate):
    """`x` with `specials` over its first elements and three more over its last ones (the scalar tail), rotated per row."""
    flat, n_s = x.reshape(-1), len(specials)
    lead = min(flat.size, n_s)
    flat[:lead] = np.roll(specials, -rotate)[:lead]
    if flat.size > n_s + 3:
        flat[-3:] = np.roll(specials, -rotate - 5)[:3]
    return x


@functools.lru_cache(maxsize=None)
def inputs(row):
    """The row's operands (ndarrays, read-only), seeded by its name."""
    rng, kw = _rng(row), row.kw
    if row.family == 'matmul':
        m, n, k = kw['m'], kw['n'], kw['k']
        a = rng.standard_normal((k, m) if kw['ta'] else (m, k)).astype(np.float32)
        b = (rng.standard_normal((n, k) if kw['tb'] else (k, n)) * (2.0 / max(k, 1)) ** 0.5).astype(np.float32)
        if kw.get('poison'):
            (pm, pk), (qk, qn) = kw['poison']
            a[(pk, pm) if kw['ta'] else (pm, pk)] = np.nan
            b[(qn, qk) if kw['tb'] else (qk, qn)] = np.inf
        out = (a, b)
    elif row.family == 'unary':
        out = (_with_specials((rng.standard_normal(kw['n']) * 3.0).astype(np.float32), UNARY_SPECIALS, kw['n']),)
    elif row.family == 'binary':
        a, b = (rng.standard_normal(kw[k_]).astype(np.float32) for k_ in ('a', 'b'))
        for t in (a, b):
            t.reshape(-1)[0] = -0.0                     # -0.0 + -0.0 = -0.0, -0.0 * -0.0 = +0.0
        out = (a, b)
    elif row.family == 'concat':
        out = tuple(rng.standard_normal(s).astype(np.float32) for s in kw['shapes'])
    elif row.family == 'transpose':
        out = (rng.standard_normal(kw['shape']).astype(np.float32),)
    elif row.family == 'pad2d':
        x = rng.standard_normal(kw['xs']).astype(np.float32)
        x.reshape(-1)[::3] = -0.0                       # without channel_add the kernel adds -0.0: -0.0 must stay -0.0
        out = (x, (rng.standard_normal(kw['xs'][1]) * 10.0).astype(np.float32)) if kw['add'] else (x,)
    elif row.family == 'input':
        shape = (kw['n'], kw['h'], kw['w'], kw['c']) if kw['nhwc'] else (kw['n'], kw['c'], kw['h'], kw['w'])
        if kw['u8']:
            out = (rng.randint(0, 256, shape).astype(np.uint8),)
        else:
            out = (_with_specials(rng.standard_normal(shape).astype(np.float32), np.array([np.nan, -0.0, np.inf, -np.inf, 1e-45, -3.0e38], np.float32), 0),)
    elif row.family == 'c8':
        out = (_with_specials((rng.standard_normal((2, kw['c'], 3, 5)) * 100.0).astype(np.float32), C8_SPECIALS, 0),)
    else:
        raise AssertionError(row.family)
    for t in out:
        t.setflags(write=False)
    return out


def launches(row):
    """The names of the launches a row makes."""
    return {'matmul': ('MatMul',), 'unary': UNARY_OPS, 'binary': ('Subtract',) if not row.kw.get('commutative', True) else ('Add', 'Multiply'),
            'concat': ('Concat',), 'transpose': ('Transpose',), 'pad2d': ('pad2d',), 'input': ('input',), 'c8': ('c8',)}[row.family]


@functools.lru_cache(maxsize=4)
def references(row):
    """{launch: its float64 result} (tests/ref64.py), shared by the CPU and the GPU test of the row; read-only."""
    ins, kw = inputs(row), row.kw
    with np.errstate(all='ignore'):
        if row.family == 'matmul':
            a, b = (ref64.f16r(t) for t in ins) if kw['f16'] else ins
            ref = {'MatMul': ref64.matmul(a, b, bool(kw['ta']), bool(kw['tb']))}
        elif row.family == 'unary':
            ref = {'ReLU': ref64.relu(ins[0]), 'Clamp': ref64.clamp(ins[0], CLAMP_LO, CLAMP_HI), 'Sigmoid': ref64.sigmoid(ins[0])}
        elif row.family == 'binary':
            a, b = (np.asarray(t, dtype=np.float64) for t in ins)
            ref = {'Subtract': a - b} if not kw.get('commutative', True) else {'Add': a + b, 'Multiply': a * b}
        elif row.family == 'concat':
            ref = {'Concat': ref64.concat(ins, kw['axis'])}
        elif row.family == 'transpose':
            ref = {'Transpose': ref64.transpose(ins[0], kw['perm'])}
        elif row.family == 'pad2d':
            pt, pl, pb, pr = kw['pads']
            ref = {'pad2d': ref64.pad2d(ins[0], (pt, pl), (pb, pr), ins[1] if kw['add'] else None)}
        elif row.family == 'input':
            ref = {'input': ref64.nhwc_to_nchw(ins[0]) if kw['nhwc'] else ref64.u8_to_f32(ins[0]) if kw['u8'] else np.asarray(ins[0], np.float64)}
        else:
            raise AssertionError(row.family)
    for t in ref.values():
        t.setflags(write=False)
    return ref


def oracles(row):
    """{launch: the oracle's fp32 result} for the launches the oracle has an op for (oracle/ops.py; Add broadcasts its second operand
    only and Multiply the smaller one, as the reference; the layout kernels are held against numpy's own transpose and cast)."""
    from oracle import ops
    ins, kw = inputs(row), row.kw
    out = {}
    with np.errstate(all='ignore'):
        if row.family == 'matmul' and not kw['f16']:
            out['MatMul'] = ops.matmul(ins[0], ins[1], 'true' if kw['ta'] else 'false', 'true' if kw['tb'] else 'false')
        elif row.family == 'unary':
            out = {'ReLU': ops.relu(ins[0]), 'Clamp': ops.clamp(ins[0], CLAMP_LO, CLAMP_HI), 'Sigmoid': ops.sigmoid(ins[0])}
        elif row.family == 'binary' and kw.get('commutative', True):
            a, b = ins
            shape = np.broadcast_shapes(a.shape, b.shape)
            if a.shape == shape:
                out['Add'] = ops.add(a, b)
            if (a.shape if a.size > b.size else b.shape) == shape:
                out['Multiply'] = ops.multiply(a, b)
        elif row.family == 'concat':
            out['Concat'] = ops.concat(ins, kw['axis'])
        elif row.family == 'transpose':
            out['Transpose'] = np.ascontiguousarray(ins[0].transpose(kw['perm']))          # Transpose.py:9-13, materialised
        elif row.family == 'pad2d':
            pt, pl, pb, pr = kw['pads']
            x = ops.add(ins[0], ins[1].reshape(1, -1, 1, 1)) if kw['add'] else ins[0]
            out['pad2d'] = ops._pad_hw(x, (pt, pl), (pb, pr))
        elif row.family == 'input':
            x = ins[0]
            out['input'] = np.ascontiguousarray(x.transpose(0, 3, 1, 2) if kw['nhwc'] else x).astype(np.float32)
    return {k_: np.asarray(v) for k_, v in out.items()}


WORST = {}                # MatMul row -> max-norm error against float64 of its device result (printed by the GPU test)


def compare(row, name, got, what, device_result=False):
    """`got` (fp32) against the float64 reference of launch `name` by the module's rules."""
    ref = references(row)[name]
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape, '{}: {} {} for {}'.format(what, got.dtype, got.shape, ref.shape)
    if name == 'Sigmoid':
        ref64.check_group(got, ref, what=what)
    elif name == 'MatMul':
        with np.errstate(all='ignore'):
            if row.kw.get('poison'):
                (pm, _), (_, qn) = row.kw['poison']
                bad = np.zeros(ref.shape, dtype=bool)
                bad[pm, :], bad[:, qn] = True, True
                assert np.array_equal(~np.isfinite(ref), bad), what + ': the float64 result is not non-finite on exactly one row and one column'
                assert np.isnan(ref[pm]).all() and np.isinf(ref[np.arange(ref.shape[0]) != pm, qn]).all(), what
            if row.kw['f16']:
                err = assert_close(got, ref.astype(np.float32), 1e-5, what)
            else:
                ref64.check_group(got, ref, what=what)
                err = helpers.rel_err(got, ref)
        if device_result:
            WORST[row.id] = err
            print('{}: max-norm error {:.3e} against float64 (DRIFT {:.0e})'.format(what, err, ref64.DRIFT))
    else:
        assert name in helpers.BIT_EXACT or name in ('Subtract', 'pad2d', 'input'), name
        with np.errstate(all='ignore'):
            assert_bit_exact(got, ref.astype(np.float32), what)


# ---------------------------------------------------------------------------------------------------------------------- CPU part
QUERIED = [r for r in ROWS if r.family != 'refusal']


@pytest.mark.parametrize('row', QUERIED, ids=[r.id for r in QUERIED])
def test_query_answers_the_class_of_the_row(row, monkeypatch):
    with Env(row, monkeypatch):
        assert class_of(row) == row.cls


def test_table_holds_every_class_the_planners_return():
    """Exactly the planners' classes, one row each: deleting any row fails here (a plain row leaves its class without one, an edge row
    leaves EDGE_ROWS short)."""
    plain = [r for r in ROWS if r.id not in EDGE_ROWS]
    seen = {r.cls for r in plain}
    assert len(seen) == len(plain), 'two rows for one class: {}'.format(sorted((r.cls for r in plain if [q.cls for q in plain].count(r.cls) > 1), key=str))
    wanted = (planner_classes() - NOTHING_LAUNCHED) | FIXED_CLASSES
    assert seen == wanted, 'missing {}, unknown {}'.format(sorted(wanted - seen, key=str), sorted(seen - wanted, key=str))
    assert {r.id for r in ROWS if r.edge is not None} == EDGE_ROWS
    assert all(r.where in ('here', 'test_hip_ops', 'diag_variants') for r in ROWS)


def test_nontemporal_row_has_the_shape_the_streaming_test_runs():
    import test_hip_ops
    row = next(r for r in ROWS if r.where == 'test_hip_ops')
    assert row.kw['n'] == int(np.prod(test_hip_ops.NT_UNARY)) and 'unary' in test_hip_ops.NT_FAMILIES


def test_queries_refuse_what_the_entries_refuse():
    """The refusal rows on the host: the queries return what the entries return, before any pointer is looked at."""
    from pyopenvino_amd import device
    f = (ctypes.c_int * FORM_INTS)()
    with pytest.raises(device.PvhipError, match=r'\(-5\).*too large for the tile grid'):
        device.call('pvhip_matmul_form', 65535 * 64 + 1, 1, 1, 0, 0, 0, f)
    assert matmul_form(65535 * 64, 1, 1, 0, 0, 0)['gy'] == 65535
    with pytest.raises(device.PvhipError, match=r'\(-5\).*2\^31'):
        device.call('pvhip_concat_form', 2, device.i64_array([1 << 20, 1 << 20]), 1 << 10, f)
    with pytest.raises(device.PvhipError):
        device.call('pvhip_concat_form', 17, device.i64_array([4] * 17), 1, f)
    with pytest.raises(device.PvhipError, match=r'\(-2\).*c <= 4096'):
        device.call('pvhip_input_to_nchw_form', 1, 4097, 1, 1, 1, 1, 0, 0, f)
    assert input_form(1, 4097, 1, 1, 1, 0, 0, 0)['kind'] == 1                # the limit is the NHWC tile's


# The launchers' arithmetic as it stood before the plan functions were lifted out of them (frozen here): the plans must be theirs --
# launch parameters did not change.  (The binary launcher's choice is held by the rows themselves and by tests/test_hip_ops.py.)
def _old_matmul(m, n, k):
    if m * n == 0:
        return (NONE, 0, 0, 0, 0)
    if k == 0:
        return (0, 0, 0, 0, 0)
    gx, gy = (n + 63) // 64, (m + 63) // 64
    tiles, splits = gx * gy, 1
    if tiles < 2 * 256:
        splits = max(1, min((4 * 256 + tiles - 1) // tiles, (k + 63) // 64))
    k_chunk = ((k + splits - 1) // splits + 15) // 16 * 16
    splits = (k + k_chunk - 1) // k_chunk
    if splits <= 1:
        return (1, gx, gy, 1, (k + 15) // 16 * 16)
    return (2, gx, gy, splits, k_chunk)


def test_plans_are_those_of_the_previous_launchers():
    rng = np.random.RandomState(11)
    for _ in range(20000):
        m, n = (int(rng.choice([0, 1, rng.randint(1, 300), rng.randint(1, 5000)])) for _ in range(2))
        k = int(rng.choice([0, 1, rng.randint(1, 200), rng.randint(1, 3000)]))
        ta, tb = int(rng.randint(2)), int(rng.randint(2))
        f = matmul_form(m, n, k, ta, tb, 0)
        assert (f['kind'], f['gx'], f['gy'], f['splits'], f['k_chunk']) == _old_matmul(m, n, k), (m, n, k)
        if f['kind'] > 0:
            assert (f['akf'], f['bnf']) == (int(not ta or m == 1), int(not tb or k == 1)), (m, n, k, ta, tb)      # sak == 1, sbn == 1
    cap = 256 * 16                                                       # kNumCU x PVHIP_STREAM_WG
    for n in list(range(1, 3000)) + [int(v) for v in rng.randint(1, 1 << 23, 2000)]:
        f, n4 = unary_form(n), n // 4
        assert (f['nt'], f['u'], f['grid']) == (0, 1, min(max((max(n4, 1) + 255) // 256, 1), cap)), n
    for n in (1 << 23, (1 << 23) + 5, 3 << 24):                          # 64 MiB moved and more: runs of four pieces, 2 x the cap
        f = unary_form(n)
        assert (f['nt'], f['u'], f['grid']) == (1, 4, min((n // 4 + 1023) // 1024, 2 * cap)), n
    for _ in range(5000):
        inner = [int(rng.choice([0, 1, 3, 4, 8, 70, 1000])) for _ in range(int(rng.randint(1, 17)))]
        outer = int(rng.choice([0, 1, 2, 7, 300, 70000]))
        f = concat_form(inner, outer)
        if sum(inner) * outer == 0:
            assert f['kind'] == NONE
            continue
        vec4 = all(v % 4 == 0 for v in inner)
        work = max(inner) // (4 if vec4 else 1) * outer
        assert (f['kind'], f['gx'], f['gy']) == (int(vec4), min(max((work + 255) // 256, 1), 2048), len(inner)), (inner, outer)
    for _ in range(20000):
        u8, nhwc = int(rng.randint(2)), int(rng.randint(2))
        n, c = int(rng.randint(1, 4)), int(rng.choice([1, 2, 3, 4, 5, 8, 16, 64, 100, 1030, 2048, 4096]))
        h, w = int(rng.randint(1, 40)), int(rng.randint(1, 200))
        sa, da = int(rng.randint(16)) if u8 else 4 * int(rng.randint(4)), 4 * int(rng.randint(4))
        f, p, es = input_form(n, c, h, w, u8, nhwc, sa, da), h * w, 1 if u8 else 4
        total = n * c * p
        if not nhwc:
            n4 = total // 4 if u8 and sa % 4 == 0 and da == 0 else 0
            want = (1, int(n4 > 0), 0, 0, 0, ((n4 or total) + 255) // 256, 1) if u8 else (0, 0, 0, 0, 0, 0, 0)
        else:
            tile = 1024
            while tile > 1 and tile * c * es > 16384:
                tile >>= 1
            vl = sa == 0 and (p * c * es) % 16 == 0 and (tile * c * es) % 16 == 0
            want = (2, 0, tile, int(vl), int(da == 0 and p % 4 == 0 and tile % 4 == 0), (p + tile - 1) // tile, n)
        assert tuple(f[k_] for k_ in ('kind', 'vec', 'tile', 'vl', 'vs', 'gx', 'gy')) == want, (n, c, h, w, u8, nhwc, sa, da)


LIGHT = [r for r in ROWS if r.where != 'test_hip_ops' and r.family not in ('refusal', 'c8')]


@pytest.mark.parametrize('row', LIGHT, ids=[r.id for r in LIGHT])
def test_float64_reference_agrees_with_the_oracle(row):
    found = oracles(row)
    assert found or row.family in ('matmul', 'binary'), row.id          # f16 MatMul, Subtract and doubly broadcast operands: no oracle op
    for name, value in found.items():
        assert value.dtype == np.float32
        compare(row, name, value, '{} {} (oracle)'.format(row.id, name))


def _c8_pack_by_loops(x):
    """pvhip_c8_f16_from_f32 element by element (the definition ref64.c8_pack vectorises)."""
    n, c, h, w = x.shape
    out = np.zeros((n, ref64.c8_blocks(c), h * w, 8), dtype=np.float16)
    with np.errstate(over='ignore'):
        for i, ch, p in itertools.product(range(n), range(c), range(h * w)):
            out[i, ch // 8, p, ch % 8] = np.float16(x[i, ch].reshape(-1)[p])
    return out


C8_ROWS = [r for r in ROWS if r.family == 'c8']


@pytest.mark.parametrize('row', C8_ROWS, ids=[r.id for r in C8_ROWS])
def test_c8_restatement(row):
    """ref64.c8_pack against the element-by-element definition, the rounding of the edge values it leans on, and the round trip."""
    x = inputs(row)[0]
    packed = ref64.c8_pack(x)
    assert packed.shape == (2, 2 * -(-row.kw['c'] // 16), 15, 8)
    assert np.array_equal(packed.view(np.uint16), _c8_pack_by_loops(x).view(np.uint16))
    back = ref64.c8_unpack(packed, row.kw['c'])
    assert np.array_equal(ref64.c8_pack(back.reshape(x.shape)).view(np.uint16), packed.view(np.uint16))
    # round to nearest even at the fp16 edges, from exact arithmetic: a tie goes to the neighbour with an even significand
    with np.errstate(over='ignore'):
        got = C8_SPECIALS[:10].astype(np.float16).astype(np.float64)
    assert got.tolist() == [np.inf, 65504.0, -np.inf, 65504.0, 2.0 ** -24, 0.0, 2.0 ** -24, 2 * 2.0 ** -24, 2 * 2.0 ** -24, 4 * 2.0 ** -24]
    assert C8_SPECIALS[[16, 17]].astype(np.float16).astype(np.float64).tolist() == [1.0, 1 + 2.0 ** -9]
    assert float(np.float16(C8_SPECIALS[15])) == 2.0 ** -14            # the tie below the smallest normal: to the even one, the normal


# ---------------------------------------------------------------------------------------------------------------------- GPU part
def _p(t, offset=0):
    return ctypes.c_void_p((t.ptr + offset) if t is not None else 0)


def _filled(hip, shape, byte=0xFF, dtype=np.float32):
    """A device tensor whose bytes are `byte` (0xFF: NaN), so that an element the kernel leaves out shows."""
    t = hip.DeviceTensor.empty(shape, dtype)
    hip.call('pvhip_memset', _p(t), byte, max(t.nbytes, 1))
    return t


def _launch_matmul(hip, row):
    kw = row.kw
    a, b = (hip.DeviceTensor.from_numpy(t) for t in inputs(row))
    entry = 'pvhip_matmul_f16' if kw['f16'] else 'pvhip_matmul_f32'
    outs = []
    for _ in range(2 if row.cls[1].startswith('split') else 1):          # a split launch twice: the header promises the same bits
        c = _filled(hip, (kw['m'], kw['n']))
        hip.call(entry, _p(a), _p(b), _p(c), kw['m'], kw['n'], kw['k'], kw['ta'], kw['tb'])
        outs.append(np.asarray(c))
    for again in outs[1:]:
        assert np.array_equal(again.view(np.uint32), outs[0].view(np.uint32)), row.id + ': a second launch gave other bits'
    return {'MatMul': outs[0]}


def _launch_unary(hip, row):
    x = hip.DeviceTensor.from_numpy(inputs(row)[0])
    got = {}
    for op in UNARY_OPS:
        y = _filled(hip, x.shape)
        if op == 'Clamp':
            hip.call('pvhip_clamp_f32', _p(x), _p(y), x.size, CLAMP_LO, CLAMP_HI)
        else:
            hip.call('pvhip_relu_f32' if op == 'ReLU' else 'pvhip_sigmoid_f32', _p(x), _p(y), x.size)
        got[op] = np.asarray(y)
    return got


def launch_binary(hip, row, entries):
    """{launch: result} of a binary row through {launch: entry}: the strides as op_plugins/_broadcast.py resolves them."""
    a, b = (hip.DeviceTensor.from_numpy(t) for t in inputs(row))
    shape, a_st, b_st = broadcast_strides(row.kw['a'], row.kw['b'])
    got = {}
    for name, entry in entries.items():
        out = _filled(hip, shape)
        hip.call(entry, _p(a), _p(b), _p(out), len(shape), hip.i64_array(shape), hip.i64_array(a_st), hip.i64_array(b_st))
        got[name] = np.asarray(out)
    return got


def _launch_concat(hip, row):
    parts = [hip.DeviceTensor.from_numpy(t) for t in inputs(row)]
    inner, outer = concat_geometry(row.kw['shapes'], row.kw['axis'])
    out = _filled(hip, references(row)['Concat'].shape)
    srcs = (ctypes.c_void_p * len(parts))(*[t.ptr for t in parts])
    hip.call('pvhip_concat_f32', len(parts), srcs, hip.i64_array(inner), _p(out), outer)
    return {'Concat': np.asarray(out)}


def _launch_transpose(hip, row):
    x = hip.DeviceTensor.from_numpy(inputs(row)[0])
    y = _filled(hip, references(row)['Transpose'].shape)
    hip.call('pvhip_transpose_f32', _p(x), _p(y), len(x.shape), hip.i64_array(x.shape), hip.i64_array(row.kw['perm']))
    return {'Transpose': np.asarray(y)}


def _launch_pad2d(hip, row):
    ins = [hip.DeviceTensor.from_numpy(t) for t in inputs(row)]
    y = _filled(hip, references(row)['pad2d'].shape)
    hip.call('pvhip_pad2d_f32', _p(ins[0]), _p(y), *row.kw['xs'], *row.kw['pads'], _p(ins[1] if row.kw['add'] else None))
    return {'pad2d': np.asarray(y)}


GUARD = 8                 # floats around the destination of an input row: they must keep their fill


def _launch_input(hip, row):
    """The source at byte offset sa and the destination at byte offset da + 16 * GUARD / 4 inside one DeviceTensor each (the pool's blocks
    are 16-byte aligned, which the query's alignment arguments assume)."""
    kw, x = row.kw, inputs(row)[0]
    raw = np.zeros(x.nbytes + kw['sa'], np.uint8)
    raw[kw['sa']:] = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    src = hip.DeviceTensor.from_numpy(raw)
    total = x.size
    dst = _filled(hip, (total + 2 * GUARD + 4,), 0x7f)
    assert src.ptr % 16 == 0 and dst.ptr % 16 == 0
    lead = GUARD + kw['da'] // 4
    hip.call('pvhip_input_to_nchw_f32', _p(src, kw['sa']), _p(dst, 4 * lead), kw['n'], kw['c'], kw['h'], kw['w'], kw['u8'], kw['nhwc'])
    back = np.asarray(dst)
    fill = np.frombuffer(b'\x7f' * 4, np.uint32)[0]
    assert (back[:lead].view(np.uint32) == fill).all() and (back[lead + total:].view(np.uint32) == fill).all(), row.id + ': wrote outside the tensor'
    return {'input': back[lead:lead + total].reshape(kw['n'], kw['c'], kw['h'], kw['w'])}


LAUNCHERS = {'matmul': _launch_matmul, 'unary': _launch_unary, 'concat': _launch_concat, 'transpose': _launch_transpose, 'pad2d': _launch_pad2d,
             'input': _launch_input, 'binary': lambda hip, row: launch_binary(hip, row, {'Add': 'pvhip_add_f32', 'Multiply': 'pvhip_mul_f32'})}
GPU_ROWS = [r for r in HERE if r.family in LAUNCHERS]


@gpu
@pytest.mark.parametrize('row', GPU_ROWS, ids=[r.id for r in GPU_ROWS])
def test_gpu_row(hip, row, monkeypatch, capsys):
    """The row's launches on the form the table names, into NaN-filled outputs, against float64 (and the oracle, for the bit-exact ops).

    Max-norm error of the MatMul rows against float64 (f16: on fp16-rounded operands), printed per row; measured on one MI355X for the
    transpose pairs t00 / t01 / t10 / t11 (asserted at ref64.DRIFT = 2e-5 and 1e-5, never tightened to these):
      single-full-grid 1472x1472x17   f32 1.91e-7 1.61e-7 1.74e-7 1.82e-7    f16 1.57e-7 1.58e-7 1.57e-7 1.52e-7
      single-short-k 65x1x17          f32 7.22e-8 7.50e-8 6.58e-8 1.33e-7    f16 1.15e-7 1.07e-7 8.33e-8 7.10e-8
      split-last-full 64x64x576       f32 2.00e-7 2.16e-7 1.57e-7 2.62e-7    f16 1.80e-7 1.97e-7 1.91e-7 1.60e-7
      split-last-one 64x64x257        f32 1.93e-7 1.90e-7 2.02e-7 1.52e-7    f16 2.15e-7 2.17e-7 1.44e-7 1.49e-7
      split-last-ragged 3x513x100     f32 2.79e-7 1.73e-7 1.97e-7 2.01e-7    f16 2.12e-7 2.07e-7 1.88e-7 2.32e-7
      split-last-short16 64x64x272    f32 1.76e-7 1.87e-7 2.14e-7 2.07e-7    f16 1.77e-7 1.84e-7 2.81e-7 1.71e-7
      fc 256x1000x1024 (t01)          f32 2.46e-7                            f16 1.94e-7
      poison 65x70x17 / 65x70x200     f32 1.16e-7 / 2.36e-7                  f16 1.72e-7 / 1.76e-7   (over the finite elements)"""
    with Env(row, monkeypatch):
        assert class_of(row) == row.cls
        if row.id == 'MatMul-empty':
            for m, n in ((0, 5), (5, 0)):              # nothing is launched, no pointer is needed
                hip.call('pvhip_matmul_f32', None, None, None, m, n, 3, 0, 0)
            return
        if row.id == 'MatMul-memset-5x70x0':           # k == 0: zeros into an output that held NaN; no operand is read
            c = _filled(hip, (5, 70))
            hip.call('pvhip_matmul_f32', None, None, _p(c), 5, 70, 0, 0, 0)
            assert_bit_exact(np.asarray(c), np.zeros((5, 70), np.float32), row.id)
            return
        got = LAUNCHERS[row.family](hip, row)
    assert tuple(got) == launches(row)
    found = oracles(row)
    with capsys.disabled():
        for name, value in got.items():
            compare(row, name, value, '{} {}'.format(row.id, name), device_result=True)
            if name in helpers.BIT_EXACT and name in found:
                assert_bit_exact(value, found[name], '{} {} vs the oracle'.format(row.id, name))


@gpu
@pytest.mark.parametrize('row', C8_ROWS, ids=[r.id for r in C8_ROWS])
def test_gpu_c8_conversions(hip, row):
    """pvhip_c8_f16_from_f32 into a block of 0xFF bytes: every real channel holds numpy's astype(np.float16) bits (round to nearest even;
    NaN compared as NaN), every padding channel c .. 16 * ceil(c / 16) - 1 of every pixel reads +0 -- the blocked convolutions multiply
    them by zero weights, and 0 x NaN is NaN; pvhip_c8_f16_to_f32 gives every fp16 value back exactly."""
    x = inputs(row)[0]
    n, c, h, w = x.shape
    want = ref64.c8_pack(x)
    elems = int(hip.call('pvhip_c8_f16_elems', n, c, h, w))
    assert elems * 2 == want.size
    xb = _filled(hip, (elems,))
    hip.call('pvhip_c8_f16_from_f32', _p(hip.DeviceTensor.from_numpy(x)), _p(xb), n, c, h, w)
    got = np.asarray(xb).view(np.float16).reshape(want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), row.id + ': NaN pattern'
    assert np.array_equal(got.view(np.uint16)[~nan], want.view(np.uint16)[~nan]), row.id + ': fp16 bits'
    channels = got.transpose(0, 1, 3, 2).reshape(n, -1, h * w)
    assert channels.shape[1] == 16 * -(-c // 16) and (channels[:, c:].view(np.uint16) == 0).all(), row.id + ': a padding channel is not +0'
    # the way back, and the round trip of values that are fp16 values already
    y = _filled(hip, x.shape)
    hip.call('pvhip_c8_f16_to_f32', _p(xb), _p(y), n, c, h, w)
    back = ref64.c8_unpack(want, c).reshape(x.shape)
    assert_bit_exact(np.asarray(y), back, row.id + ' to_f32')
    xb2 = _filled(hip, (elems,))
    hip.call('pvhip_c8_f16_from_f32', _p(hip.DeviceTensor.from_numpy(back)), _p(xb2), n, c, h, w)
    y2 = _filled(hip, x.shape)
    hip.call('pvhip_c8_f16_to_f32', _p(xb2), _p(y2), n, c, h, w)
    assert_bit_exact(np.asarray(y2), back, row.id + ' round trip')


@gpu
def test_gpu_refusals(hip):
    """The refusal rows: sizes beyond a launcher's grid or index range are errors before anything is launched.  The pointers are never
    looked at behind the null test (matmul_impl, pvhip_concat_f32, pvhip_pad2d_f32 and pvhip_input_to_nchw_f32 check sizes first)."""
    import importlib
    one = ctypes.c_void_p(256)
    with pytest.raises(hip.PvhipError, match=r'\(-5\).*too large for the tile grid'):
        hip.call('pvhip_matmul_f32', one, one, one, 65535 * 64 + 1, 1, 1, 0, 0)
    srcs = (ctypes.c_void_p * 2)(256, 256)
    with pytest.raises(hip.PvhipError, match=r'\(-5\).*2\^31'):
        hip.call('pvhip_concat_f32', 2, srcs, hip.i64_array([1 << 20, 1 << 20]), one, 1 << 10)
    with pytest.raises(hip.PvhipError, match=r'\(-5\).*too large'):
        hip.call('pvhip_pad2d_f32', one, one, 65536, 1, 1, 1, 0, 0, 0, 0, None)
    with pytest.raises(hip.PvhipError, match=r'\(-2\).*c <= 4096'):
        hip.call('pvhip_input_to_nchw_f32', one, one, 1, 4097, 1, 1, 0, 1)
    parts = [np.zeros((1, 2), np.float32)] * (hip.MAX_CONCAT + 1)
    node = {'name': 'cat17', 'type': 'Concat', 'data': {'axis': '1'},
            'input': {i: {'precision': 'FP32', 'dims': (1, 2)} for i in range(len(parts))},
            'output': {len(parts): {'precision': 'FP32', 'dims': (1, 2 * len(parts))}}}
    with pytest.raises(NotImplementedError, match='Concat of 17 inputs'):
        importlib.import_module('pyopenvino_amd.op_plugins.Concat').compute(node, dict(enumerate(parts)))
