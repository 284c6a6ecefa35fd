"""Every kernel form of the pooling, depthwise, LRN and SoftMax launchers against float64, one explicit row per form.

pvhip_pool.hip and pvhip_norm.hip pick a kernel and a template instantiation from inequalities on LDS bytes, alignment, window size
and beta.  pvhip_maxpool2d_form / pvhip_avgpool2d_form / pvhip_dwconv2d_form / pvhip_lrn_form (host-only; they call the plan function
the launcher switches on) say which form a geometry takes; ROWS below is the table (entry, arguments, expected form).

CPU part (runs without a device): the query answers the row's form; the table holds every form the planners can return
(ALL_FORMS, with the exclusions listed beside it); the float64 reference (tests/ref64.py) cast to fp32 agrees with the oracle's fp32
op -- bit for bit for MaxPool, within ref64.DRIFT for the others.

GPU part: every row runs through the plugin and is compared with the float64 reference: MaxPool bit for bit; the others
helpers.assert_close(REL_TOL) in both norms plus ref64.DRIFT in the max norm.  Exceptions:
  * LRN rows 'zero' (bias == 0 and an all-zero pixel column, and one pixel whose square underflows in fp32): the NaN / inf pattern
    is the oracle's fp32 one (0 / 0 = NaN, x / 0 = inf where float64 does not underflow); finite elements against float64.
  * LRN rows 'large' (activations ~1e4, d ~1e5): REL_TOL only, the max-norm error is printed (test_gpu_row's docstring keeps the
    measured figures).
"""
import ctypes
import functools
import importlib
import zlib

import numpy as np
import pytest

import helpers
import ref64
from helpers import assert_bit_exact, assert_close, first_out

gpu = pytest.mark.gpu

LRN_ALPHA = 9.9999997473787516e-05


# --------------------------------------------------------------------------------------------------------------------- the table
class Row:
    def __init__(self, id_, entry, form, env=None, **kw):
        self.id, self.entry, self.form, self.env, self.kw = id_, entry, form, dict(env or {}), kw

    def __repr__(self):
        return self.id


def mp(id_, xs, k, s, pb, pe, rounding, form, env=None, special=False):
    return Row('MaxPool-' + id_, 'MaxPool', form, env, xs=xs, k=k, s=s, pb=pb, pe=pe, rounding=rounding, special=special)


def ap(id_, xs, k, s, rounding, form, empty=False):
    return Row('AvgPool-' + id_, 'AvgPool', form, None, xs=xs, k=k, s=s, pb=(0, 0), pe=(0, 0), rounding=rounding, empty=empty)


def dw(id_, xs, k, s, pb, pe, form, env=None, act=None):
    return Row('Depthwise-' + id_, 'GroupConvolution', form, env, xs=xs, k=k, s=s, pb=pb, pe=pe, act=act)


def lrn(id_, xs, size, beta, bias, form, scale=40.0, edge=None):
    return Row('LRN-' + id_, 'LRN', form, None, xs=xs, size=size, beta=beta, bias=bias, scale=scale, edge=edge)


def sm(id_, xs, form):
    return Row('SoftMax-' + id_, 'SoftMax', form, None, xs=xs)


RELU, CLAMP = ('relu',), ('clamp', 0.0, 6.0)
P0 = (0, 0)
RT = ((5, 4), (3, 2), (2, 1), (1, 2))                 # run-time window, the pads of POOL_CASES' last row
COLS0, COLS2, STAGE0 = {'PVHIP_DWCONV_COLS': '0'}, {'PVHIP_DWCONV_COLS': '2'}, {'PVHIP_POOL3_STAGE': '0'}

ROWS = [
    # ---- MaxPool.  global: (kh + sh) * wp * 4 > 60 KB.  LDS kernels <0,0> / <2,2> / <3,3> (3x3 away from stride 1 / 2): G >= 4 planes
    # with (h * w) % 4 != 0, G in 2..3 (unaligned group starts: scalar staging), one plane, bands; floor (no clip) and ceil (clip)
    mp('global', (1, 2, 12, 2000), *RT, 'floor', 'global', special=True),
    mp('rt-grouped', (2, 5, 5, 11), *RT, 'floor', 'lds G=4 bands=1 rows=2 clip=0'),
    mp('rt-grouped-clip', (2, 5, 6, 9), *RT, 'ceil', 'lds G=4 bands=1 rows=3 clip=1'),
    mp('rt-few', (2, 5, 5, 7), *RT, 'floor', 'lds G=3 bands=1 rows=2 clip=0'),
    mp('rt-few-clip', (2, 5, 6, 7), *RT, 'ceil', 'lds G=2 bands=1 rows=3 clip=1'),
    mp('rt-single', (2, 3, 22, 79), *RT, 'floor', 'lds G=1 bands=1 rows=7 clip=0'),
    mp('rt-single-clip', (2, 3, 22, 79), *RT, 'ceil', 'lds G=1 bands=1 rows=8 clip=1'),
    mp('rt-banded', (2, 3, 47, 79), *RT, 'floor', 'lds G=1 bands=2 rows=8 clip=0', special=True),
    mp('rt-banded-clip', (2, 3, 48, 79), *RT, 'ceil', 'lds G=1 bands=2 rows=9 clip=1', special=True),
    mp('2x2-grouped', (2, 5, 5, 9), (2, 2), (2, 2), (1, 0), (0, 1), 'floor', 'lds2x2 G=4 bands=1 rows=3 clip=0'),
    mp('2x2-grouped-clip', (2, 5, 5, 11), (2, 2), (2, 2), P0, P0, 'ceil', 'lds2x2 G=4 bands=1 rows=3 clip=1'),
    mp('2x2-few', (2, 5, 5, 7), (2, 2), (2, 2), P0, P0, 'floor', 'lds2x2 G=3 bands=1 rows=2 clip=0'),
    mp('2x2-few-clip', (2, 5, 5, 7), (2, 2), (2, 2), P0, P0, 'ceil', 'lds2x2 G=3 bands=1 rows=3 clip=1'),
    mp('2x2-single', (2, 3, 25, 79), (2, 2), (2, 2), (1, 0), (0, 1), 'floor', 'lds2x2 G=1 bands=1 rows=13 clip=0'),
    mp('2x2-single-clip', (2, 3, 26, 75), (2, 2), (2, 2), (1, 0), (0, 1), 'ceil', 'lds2x2 G=1 bands=1 rows=14 clip=1'),
    mp('2x2-banded', (2, 3, 51, 79), (2, 2), (2, 2), (1, 0), (0, 1), 'floor', 'lds2x2 G=1 bands=2 rows=13 clip=0', special=True),
    mp('2x2-banded-clip', (2, 3, 52, 77), (2, 2), (2, 2), (1, 0), (0, 1), 'ceil', 'lds2x2 G=1 bands=2 rows=14 clip=1', special=True),
    mp('3x3-grouped', (2, 5, 5, 9), (3, 3), (3, 3), (1, 1), P0, 'floor', 'lds3x3 G=4 bands=1 rows=2 clip=0'),
    mp('3x3-grouped-clip', (2, 5, 5, 9), (3, 3), (3, 3), (1, 1), P0, 'ceil', 'lds3x3 G=4 bands=1 rows=2 clip=1'),
    mp('3x3-few', (2, 5, 5, 7), (3, 3), (3, 3), (1, 1), P0, 'floor', 'lds3x3 G=2 bands=1 rows=2 clip=0'),
    mp('3x3-few-clip', (2, 5, 5, 7), (3, 3), (3, 3), P0, P0, 'ceil', 'lds3x3 G=3 bands=1 rows=2 clip=1'),
    mp('3x3-single', (2, 3, 25, 79), (3, 3), (3, 3), (1, 1), P0, 'floor', 'lds3x3 G=1 bands=1 rows=8 clip=0'),
    mp('3x3-single-clip', (2, 3, 25, 79), (3, 3), (3, 3), (1, 1), P0, 'ceil', 'lds3x3 G=1 bands=1 rows=9 clip=1'),
    mp('3x3-banded', (2, 3, 53, 75), (3, 3), (3, 3), (1, 1), P0, 'floor', 'lds3x3 G=1 bands=2 rows=9 clip=0', special=True),
    mp('3x3-banded-clip', (2, 3, 51, 79), (3, 3), (3, 3), (1, 1), P0, 'ceil', 'lds3x3 G=1 bands=2 rows=9 clip=1', special=True),
    mp('3x3-s1x2-banded', (2, 3, 49, 79), (3, 3), (1, 2), (1, 1), (1, 1), 'floor', 'lds3x3 G=1 bands=2 rows=25 clip=0', special=True),      # sh != sw
    mp('3x3-s2-banded-refused-by-cols', (2, 3, 96, 100), (3, 3), (2, 2), (1, 1), (1, 1), 'ceil', 'lds3x3 G=1 bands=3 rows=17 clip=1', special=True),
    # the column kernel (3x3, stride 1 / 2): whole planes and bands, outputs through the LDS stage and (PVHIP_POOL3_STAGE=0) stored by the lanes
    mp('cols-s1', (2, 5, 7, 9), (3, 3), (1, 1), (1, 1), (1, 1), 'ceil', 'cols_s1 G=10 bands=1 rows=7 S=2 stage=1 nt=0'),
    mp('cols-s2', (2, 5, 7, 9), (3, 3), (2, 2), P0, P0, 'ceil', 'cols_s2 G=10 bands=1 rows=3 S=3 stage=1 nt=0'),
    mp('cols-s1-banded', (2, 3, 80, 92), (3, 3), (1, 1), (1, 1), (1, 1), 'ceil', 'cols_s1 G=2 bands=3 rows=27 S=4 stage=1 nt=0', special=True),
    mp('cols-s2-banded', (2, 3, 97, 100), (3, 3), (2, 2), P0, P0, 'ceil', 'cols_s2 G=1 bands=2 rows=24 S=5 stage=1 nt=0', special=True),
    mp('cols-s1-direct', (2, 5, 7, 9), (3, 3), (1, 1), (1, 1), (1, 1), 'ceil', 'cols_s1 G=10 bands=1 rows=7 S=2 stage=0 nt=0', env=STAGE0),
    mp('cols-s2-direct', (2, 5, 7, 9), (3, 3), (2, 2), P0, P0, 'ceil', 'cols_s2 G=10 bands=1 rows=3 S=3 stage=0 nt=0', env=STAGE0),
    mp('cols-s1-banded-direct', (2, 3, 80, 92), (3, 3), (1, 1), (1, 1), (1, 1), 'ceil', 'cols_s1 G=2 bands=3 rows=27 S=4 stage=0 nt=0', env=STAGE0, special=True),
    mp('cols-s2-banded-direct', (2, 3, 97, 100), (3, 3), (2, 2), P0, P0, 'ceil', 'cols_s2 G=1 bands=2 rows=24 S=5 stage=0 nt=0', env=STAGE0, special=True),

    # ---- AvgPool.  global: h * w > 4096.  LDS: every group start 16-byte aligned (G >= 4 with (h * w) % 4 != 0) or not (G = 2)
    ap('global-3x3', (1, 3, 65, 67), (3, 3), (2, 2), 'floor', 'global'),
    ap('global-7x5', (1, 3, 65, 67), (7, 5), (3, 1), 'floor', 'global'),
    ap('lds-grouped', (2, 5, 7, 9), (3, 3), (2, 2), 'floor', 'lds G=4 vec=1'),
    ap('lds-grouped-4x2', (2, 5, 9, 13), (4, 2), (1, 3), 'floor', 'lds G=4 vec=1'),
    ap('lds-unaligned', (2, 5, 7, 7), (3, 3), (2, 2), 'floor', 'lds G=2 vec=0'),
    ap('lds-empty-window', (2, 3, 5, 5), (2, 2), (2, 2), 'ceil', 'lds G=2 vec=0', empty=True),

    # ---- Depthwise.  dwconv2d_lds_kernel<0,0>: 1x1, 5x5, 3x5, 7x7 windows, strides (1,1) (2,1) (3,3) (2,2); G >= 4 with odd h * w, G in
    # 1..3 with unaligned / aligned group starts, bands with unaligned / aligned starts; asymmetric pads, pads_end beyond what the windows need
    dw('1x1-grouped', (2, 5, 3, 3), (1, 1), (1, 1), P0, (0, 2), 'lds G=4 bands=1 rows=3 vec=1'),
    dw('1x1-few-unaligned', (2, 5, 3, 3), (1, 1), (1, 1), P0, (1, 0), 'lds G=2 bands=1 rows=4 vec=0'),
    dw('1x1-few-aligned', (2, 5, 4, 3), (1, 1), (1, 1), P0, (0, 2), 'lds G=3 bands=1 rows=4 vec=1'),
    dw('1x1-banded-unaligned', (2, 3, 55, 73), (1, 1), (1, 1), P0, (0, 2), 'lds G=1 bands=2 rows=28 vec=0'),
    dw('1x1-banded-aligned', (2, 3, 56, 73), (1, 1), (1, 1), P0, (0, 2), 'lds G=1 bands=2 rows=28 vec=1'),
    dw('5x5-grouped', (2, 5, 3, 5), (5, 5), (2, 1), (2, 2), (3, 2), 'lds G=4 bands=1 rows=2 vec=1'),
    dw('5x5-few-unaligned', (2, 5, 3, 3), (5, 5), (2, 1), (2, 2), (3, 2), 'lds G=2 bands=1 rows=2 vec=0'),
    dw('5x5-few-aligned', (2, 5, 4, 5), (5, 5), (2, 1), (2, 2), (3, 2), 'lds G=3 bands=1 rows=3 vec=1'),
    dw('5x5-banded-unaligned', (2, 3, 70, 71), (5, 5), (2, 1), (2, 2), (3, 2), 'lds G=1 bands=2 rows=18 vec=0'),
    dw('5x5-banded-aligned', (2, 3, 56, 65), (5, 5), (2, 1), (2, 2), (3, 2), 'lds G=1 bands=2 rows=15 vec=1'),
    dw('5x5-banded-bias-relu', (2, 3, 70, 71), (5, 5), (2, 1), (2, 2), (3, 2), 'lds G=1 bands=2 rows=18 vec=0', act=RELU),
    dw('5x5-banded-bias-clamp', (2, 3, 70, 71), (5, 5), (2, 1), (2, 2), (3, 2), 'lds G=1 bands=2 rows=18 vec=0', act=CLAMP),
    dw('3x5-grouped', (2, 5, 3, 17), (3, 5), (3, 3), (1, 2), (2, 2), 'lds G=4 bands=1 rows=2 vec=1'),
    dw('3x5-few-unaligned', (2, 5, 3, 5), (3, 5), (3, 3), (1, 2), (2, 2), 'lds G=2 bands=1 rows=2 vec=0'),
    dw('3x5-few-aligned', (2, 5, 4, 5), (3, 5), (3, 3), (1, 2), (2, 2), 'lds G=2 bands=1 rows=2 vec=1'),
    dw('3x5-banded-unaligned', (2, 3, 51, 73), (3, 5), (3, 3), (1, 2), (2, 2), 'lds G=1 bands=2 rows=9 vec=0'),
    dw('3x5-banded-aligned', (2, 3, 60, 65), (3, 5), (3, 3), (1, 2), (2, 2), 'lds G=1 bands=2 rows=11 vec=1'),
    dw('7x7-grouped', (2, 5, 3, 7), (7, 7), (2, 2), (3, 3), (4, 3), 'lds G=4 bands=1 rows=2 vec=1'),
    dw('7x7-few-unaligned', (2, 5, 3, 3), (7, 7), (2, 2), (3, 3), (4, 3), 'lds G=3 bands=1 rows=2 vec=0'),
    dw('7x7-few-aligned', (2, 5, 4, 3), (7, 7), (2, 2), (3, 3), (4, 3), 'lds G=2 bands=1 rows=3 vec=1'),
    dw('7x7-banded-unaligned', (2, 3, 46, 73), (7, 7), (2, 2), (3, 3), (4, 3), 'lds G=1 bands=2 rows=12 vec=0'),
    dw('7x7-banded-aligned', (2, 3, 48, 73), (7, 7), (2, 2), (0, 3), (3, 5), 'lds G=1 bands=2 rows=12 vec=1'),
    dw('7x7-grouped-bias-relu', (2, 5, 3, 7), (7, 7), (2, 2), (3, 3), (4, 3), 'lds G=4 bands=1 rows=2 vec=1', act=RELU),
    dw('7x7-grouped-bias-clamp', (2, 5, 3, 7), (7, 7), (2, 2), (3, 3), (4, 3), 'lds G=4 bands=1 rows=2 vec=1', act=CLAMP),
    # dwconv2d_lds_kernel<3,3> BY DEFAULT: the column planner bands a plane of odd width and is refused
    dw('3x3-s1-odd-width-banded', (2, 3, 70, 91), (3, 3), (1, 1), (1, 1), (1, 1), 'lds3x3 G=1 bands=2 rows=35 vec=0'),
    dw('3x3-s2-odd-width-banded', (2, 3, 70, 91), (3, 3), (2, 2), P0, (1, 1), 'lds3x3 G=1 bands=2 rows=18 vec=0'),
    dw('3x3-s1-150x151', (2, 3, 150, 151), (3, 3), (1, 1), (1, 1), (1, 1), 'lds3x3 G=1 bands=7 rows=22 vec=0'),
    dw('3x3-s1-odd-width-bias-relu', (2, 3, 70, 91), (3, 3), (1, 1), (1, 1), (1, 1), 'lds3x3 G=1 bands=2 rows=35 vec=0', act=RELU),
    dw('3x3-s2-odd-width-bias-clamp', (2, 3, 70, 91), (3, 3), (2, 2), P0, (1, 1), 'lds3x3 G=1 bands=2 rows=18 vec=0', act=CLAMP),
    # ... and its other staging forms with PVHIP_DWCONV_COLS=0
    dw('3x3-grouped', (2, 5, 3, 3), (3, 3), (1, 1), (1, 1), (2, 1), 'lds3x3 G=4 bands=1 rows=4 vec=1', env=COLS0),
    dw('3x3-few-unaligned', (2, 5, 3, 5), (3, 3), (1, 1), (1, 1), (2, 1), 'lds3x3 G=3 bands=1 rows=4 vec=0', env=COLS0),
    dw('3x3-few-aligned', (2, 5, 4, 3), (3, 3), (2, 2), (1, 1), (2, 1), 'lds3x3 G=3 bands=1 rows=3 vec=1', env=COLS0),
    dw('3x3-banded-aligned', (2, 3, 56, 69), (3, 3), (1, 1), (1, 1), (2, 1), 'lds3x3 G=1 bands=2 rows=29 vec=1', env=COLS0),
    # dwconv_kernel: (kh + sh) * wp * 4 > 48 KB, or band + weights beyond 64 KB of LDS (a window of 100 x 100 taps)
    dw('global-7x7', (2, 3, 9, 1400), (7, 7), (2, 2), (3, 3), (3, 3), 'global'),
    dw('global-3x3', (2, 3, 5, 3100), (3, 3), (1, 1), (1, 1), (1, 1), 'global'),
    dw('global-3x3-cols0', (2, 3, 5, 3100), (3, 3), (1, 1), (1, 1), (1, 1), 'global', env=COLS0),
    dw('global-100x100', (2, 3, 102, 100), (100, 100), (1, 1), P0, P0, 'global'),
    dw('global-7x7-bias-relu', (2, 3, 9, 1400), (7, 7), (2, 2), (3, 3), (3, 3), 'global', act=RELU),
    dw('global-7x7-bias-clamp', (2, 3, 9, 1400), (7, 7), (2, 2), (3, 3), (3, 3), 'global', act=CLAMP),
    # the column kernel: whole planes and bands, the lanes store (default) and through the output stage (PVHIP_DWCONV_COLS=2)
    dw('cols-s1', (2, 5, 7, 9), (3, 3), (1, 1), (1, 1), (1, 1), 'cols_s1 G=10 bands=1 rows=7 S=2 stage=0 nt=0'),
    dw('cols-s2', (2, 5, 7, 9), (3, 3), (2, 2), P0, (1, 1), 'cols_s2 G=10 bands=1 rows=3 S=3 stage=0 nt=0'),
    dw('cols-s1-banded', (2, 3, 120, 120), (3, 3), (1, 1), (1, 1), (1, 1), 'cols_s1 G=1 bands=3 rows=40 S=2 stage=0 nt=0'),
    dw('cols-s2-banded', (2, 3, 120, 120), (3, 3), (2, 2), P0, (1, 1), 'cols_s2 G=2 bands=5 rows=12 S=2 stage=0 nt=0'),
    dw('cols-s1-bias-relu', (2, 5, 7, 9), (3, 3), (1, 1), (1, 1), (1, 1), 'cols_s1 G=10 bands=1 rows=7 S=2 stage=0 nt=0', act=RELU),
    dw('cols-s2-bias-clamp', (2, 5, 7, 9), (3, 3), (2, 2), P0, (1, 1), 'cols_s2 G=10 bands=1 rows=3 S=3 stage=0 nt=0', act=CLAMP),
    dw('cols-s1-staged', (2, 5, 7, 9), (3, 3), (1, 1), (1, 1), (1, 1), 'cols_s1 G=10 bands=1 rows=7 S=2 stage=1 nt=0', env=COLS2),
    dw('cols-s2-staged', (2, 5, 7, 9), (3, 3), (2, 2), P0, (1, 1), 'cols_s2 G=10 bands=1 rows=3 S=3 stage=1 nt=0', env=COLS2),
    dw('cols-s1-banded-staged', (2, 3, 120, 120), (3, 3), (1, 1), (1, 1), (1, 1), 'cols_s1 G=1 bands=3 rows=40 S=2 stage=1 nt=0', env=COLS2),
    dw('cols-s2-banded-staged', (2, 3, 120, 120), (3, 3), (2, 2), P0, (1, 1), 'cols_s2 G=2 bands=5 rows=12 S=2 stage=1 nt=0', env=COLS2),
]

# ---- LRN.  lrn_window_kernel<size, vec, beta mode>: sizes 3 / 5 / 7 x planes of 16 (vec 4) and 15 (vec 1) pixels x the five modes
LRN_MODES = [('m4', 0.75, 1.0), ('m1', 0.75, 0.0), ('m2', 0.5, 1.0), ('m3', 1.0, 1.0), ('m0', 0.6, 1.0)]      # 'm<beta mode>', beta, bias
for _size in (3, 5, 7):
    for _hw in ((4, 4), (3, 5)):
        for _i, (_m, _beta, _bias) in enumerate(LRN_MODES):
            _c = 8 if (_size + _hw[0] + _i) % 2 else 24
            _form = 'window size={} vec={} bm={} loops=0'.format(_size, 4 if _hw == (4, 4) else 1, _m[1])
            ROWS.append(lrn('window-{}-{}x{}-{}'.format(_size, _hw[0], _hw[1], _m), (2, _c) + _hw, _size, _beta, _bias, _form))
for _m, _beta, _bias in LRN_MODES:
    # lrn_generic_kernel (c % 8 != 0, and an even window) in every mode
    ROWS.append(lrn('generic-' + _m, (2, 6, 3, 5), 4, _beta, _bias, 'generic bm={} loops=0'.format(_m[1])))
    # activations of ~1e4: d ~ 1e5 (mode 4's exp2(-0.75 log2 d) is documented for d up to 100)
    ROWS.append(lrn('large-' + _m, (2, 8, 4, 4), 5, _beta, _bias, 'window size=5 vec=4 bm={} loops=0'.format(_m[1]), scale=1.0e4, edge='large'))
    # bias == 0 (where the mode allows it) and an all-zero pixel column
    if _m != 'm4':
        ROWS.append(lrn('zero-' + _m, (2, 8, 3, 5), 5, _beta, 0.0, 'window size=5 vec=1 bm={} loops=0'.format(_m[1]), edge='zero'))
ROWS += [
    lrn('generic-large-m4', (2, 6, 3, 5), 4, 0.75, 1.0, 'generic bm=4 loops=0', scale=1.0e4, edge='large'),
    lrn('generic-zero-m1', (2, 6, 3, 5), 4, 0.75, 0.0, 'generic bm=1 loops=0', edge='zero'),
    lrn('generic-grid-stride', (1, 9, 250, 251), 5, 0.75, 1.0, 'generic bm=4 loops=1'),           # more than 2048 x 256 elements
    # ---- SoftMax: more rows than workgroups (2048)
    sm('2500x3', (2500, 3), 'rows blocks=2048 loops=1'),
    sm('2049x1', (2049, 1), 'rows blocks=2048 loops=1'),
]
del _size, _hw, _i, _m, _beta, _bias, _c, _form

ROW_IDS = [r.id for r in ROWS]
assert len(set(ROW_IDS)) == len(ROW_IDS)


# ----------------------------------------------------------------------------------------------------- every form the planners return
def _all_forms():
    forms = {('MaxPool', 'global'), ('AvgPool', 'global'), ('AvgPool', 'lds', 'unaligned'), ('AvgPool', 'lds', 'aligned'),
             ('GroupConvolution', 'global'), ('SoftMax', 'rows', 'loops')}
    for kind in ('lds', 'lds2x2', 'lds3x3'):
        for staging in ('grouped', 'few', 'single', 'banded'):
            for clip in ('clip', 'noclip'):
                forms.add(('MaxPool', kind, staging, clip))
    for entry in ('MaxPool', 'GroupConvolution'):
        for kind in ('cols_s1', 'cols_s2'):
            for staging in ('dense', 'banded'):
                for stage in ('staged', 'direct'):
                    forms.add((entry, kind, staging, stage))
    for kind in ('lds', 'lds3x3'):
        # (grouped, unaligned) cannot happen: G >= 4 is rounded down to a multiple of four when (h * w) % 4 != 0, or cut to the number
        # of planes -- one workgroup, which starts at the tensor
        forms |= {('GroupConvolution', kind) + f for f in (('grouped', 'aligned'), ('few', 'aligned'), ('few', 'unaligned'),
                                                           ('banded', 'aligned'), ('banded', 'unaligned'))}
    for size in (3, 5, 7):
        for vec in (1, 4):
            for bm in range(5):
                forms.add(('LRN', 'window', size, vec, bm))
    for bm in range(5):
        forms.add(('LRN', 'generic', bm))
    return forms


# Left out: the nontemporal instantiations of the column kernels (nt=1: tests/test_hip_ops.py test_nontemporal_streaming_forms_at_small_sizes),
# SoftMax's and the window / generic LRN kernels' grids below their cap (no form of their own; 'loops' and the grid-stride row are the other
# side; lrn_window_kernel loops only beyond 2048 x 256 pixel columns, the same loop statement as the generic kernel's).
ALL_FORMS = _all_forms()


def parse(form):
    head, *fields = form.split()
    return head, {k: int(v) for k, v in (f.split('=') for f in fields)}


def form_class(row, form):
    """The planner form a form string belongs to (an element of ALL_FORMS)."""
    kind, f = parse(form)
    if kind == 'global':
        return (row.entry, kind)
    if row.entry == 'SoftMax':
        return (row.entry, kind, 'loops' if f['loops'] else 'one-pass')
    if row.entry == 'LRN':
        return (row.entry, kind, f['size'], f['vec'], f['bm']) if kind == 'window' else (row.entry, kind, f['bm'])
    if row.entry == 'AvgPool':
        return (row.entry, kind, 'aligned' if f['vec'] else 'unaligned')
    assert f['nt'] == 0 if 'nt' in f else True, 'a nontemporal form in the table'
    if kind.startswith('cols'):
        return (row.entry, kind, 'banded' if f['bands'] > 1 else 'dense', 'staged' if f['stage'] else 'direct')
    if row.entry == 'MaxPool':
        staging = 'banded' if f['bands'] > 1 else 'grouped' if f['G'] >= 4 else 'few' if f['G'] >= 2 else 'single'
        return (row.entry, kind, staging, 'clip' if f['clip'] else 'noclip')
    staging = 'banded' if f['bands'] > 1 else 'grouped' if f['G'] >= 4 else 'few'
    return (row.entry, kind, staging, 'aligned' if f['vec'] else 'unaligned')


# ----------------------------------------------------------------------------------------------------------------- the form queries
MAXPOOL_KINDS = {0: 'global', 1: 'lds', 2: 'lds2x2', 3: 'lds3x3', 4: 'cols_s1', 5: 'cols_s2'}
DWCONV_KINDS = {0: 'global', 1: 'lds', 2: 'lds3x3', 3: 'cols_s1', 4: 'cols_s2'}
FORM_INTS = 16                                                        # PVHIP_FORM_* of include/pvhip.h
KIND, G, BANDS, BAND_ROWS, CLIP, VEC, STAGE, NT, S, LRN_SIZE, LRN_BM, GRID, LOOPS = range(13)


def extents(row):
    """(oh, ow) by the plugin's own rule."""
    kw = row.kw
    plugin = importlib.import_module('pyopenvino_amd.op_plugins.' + row.entry)
    if row.entry == 'GroupConvolution':
        return plugin.calc_output_shape_group_conv(kw['xs'][2:], kw['k'], kw['s'], kw['pb'], kw['pe'], 'floor', 'explicit')
    return plugin.calc_output_shape(kw['xs'][2:], kw['k'], kw['s'], kw['pb'], kw['pe'], kw['rounding'], 'explicit')


def query(row):
    """The row's form as the library reports it (host-only), in the notation of the table."""
    from pyopenvino_amd import device
    kw, f = row.kw, (ctypes.c_int * FORM_INTS)()
    if row.entry == 'SoftMax':
        device.call('pvhip_softmax_rows_form', kw['xs'][0], kw['xs'][1], f)
        assert f[KIND] == 0
        return 'rows blocks={} loops={}'.format(f[GRID], f[LOOPS])
    if row.entry == 'LRN':
        n, c, h, w = kw['xs']
        device.call('pvhip_lrn_form', n, c, h * w, kw['size'], kw['beta'], kw['bias'], f)
        if f[KIND] == 1:
            return 'window size={} vec={} bm={} loops={}'.format(f[LRN_SIZE], f[VEC], f[LRN_BM], f[LOOPS])
        return 'generic bm={} loops={}'.format(f[LRN_BM], f[LOOPS])
    (n, c, h, w), (kh, kwd), (sh, sw), (oh, ow) = kw['xs'], kw['k'], kw['s'], extents(row)
    if row.entry == 'AvgPool':
        device.call('pvhip_avgpool2d_form', n, c, h, w, oh, ow, kh, kwd, sh, sw, f)
        return 'global' if f[KIND] == 0 else 'lds G={} vec={}'.format(f[G], f[VEC])
    if row.entry == 'MaxPool':
        device.call('pvhip_maxpool2d_form', n, c, h, w, oh, ow, kh, kwd, sh, sw, kw['pb'][0], kw['pb'][1], kw['pe'][0], kw['pe'][1], f)
        kind, last = MAXPOOL_KINDS[f[KIND]], ('clip', CLIP)
    else:
        device.call('pvhip_dwconv2d_form', n, c, h, w, kh, kwd, oh, ow, sh, sw, kw['pb'][0], kw['pb'][1], f)
        kind, last = DWCONV_KINDS[f[KIND]], ('vec', VEC)
    if kind == 'global':
        return kind
    if kind.startswith('cols'):
        return '{} G={} bands={} rows={} S={} stage={} nt={}'.format(kind, f[G], f[BANDS], f[BAND_ROWS], f[S], f[STAGE], f[NT])
    return '{} G={} bands={} rows={} {}={}'.format(kind, f[G], f[BANDS], f[BAND_ROWS], last[0], f[last[1]])


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


# --------------------------------------------------------------------------------------------------- inputs, node, float64 reference
def _rng(row):
    return np.random.RandomState(zlib.crc32(row.id.encode()) & 0x7fffffff)


def _band_boundary_row(row):
    """The first input row of the second band (bands), the middle row (whole planes)."""
    kind, f = parse(row.form)
    h = row.kw['xs'][2]
    if f.get('bands', 1) > 1:
        return min(h - 1, max(0, f['rows'] * row.kw['s'][0] - row.kw['pb'][0]))
    return h // 2


@functools.lru_cache(maxsize=None)
def _inputs(row):
    """(ndarray inputs in port order, fused bias or None), seeded by the row's name; read-only."""
    rng, kw = _rng(row), row.kw
    xs = kw['xs']
    bias = None
    if row.entry == 'SoftMax':
        ins = [rng.uniform(-4.0, 4.0, xs).astype(np.float32)]
    elif row.entry == 'LRN':
        x = (rng.standard_normal(xs) * kw['scale']).astype(np.float32)
        if kw['edge'] == 'zero':
            x[0, :, 1, 2] = 0.0                         # d == 0 and x == 0 in every channel: 0 / 0
            x[1, :, 2, 1] = 0.0
            x[1, 3, 2, 1] = 1.0e-25                     # its square underflows in fp32: d == 0 for the channels whose window holds it
        ins = [x, np.array([1], dtype=np.int64)]
    else:
        x = (rng.standard_normal(xs) - (0.6 if row.entry == 'MaxPool' else 0.0)).astype(np.float32)
        if kw.get('special'):                           # NaN wins, beside +-inf, on the row where the second band begins
            r = _band_boundary_row(row)
            x[0, 0, r, 3] = np.nan
            x[0, 1, r, :] = np.inf
            x[0, 1, r, 5] = -np.nan
            x[-1, -1, r, :] = -np.inf
            x[-1, -1, max(r - 1, 0), xs[3] - 1] = np.nan
            x[-1, 0, r, xs[3] // 2] = np.inf
        ins = [x]
        if row.entry == 'GroupConvolution':
            ins.append((rng.standard_normal((xs[1], 1, 1) + tuple(kw['k'])) * 0.4).astype(np.float32))     # distinct filters per channel
            if kw['act'] is not None:
                bias = (rng.standard_normal((1, xs[1], 1, 1)) * 0.5).astype(np.float32)
    for a in ins + ([bias] if bias is not None else []):
        a.setflags(write=False)
    return ins, bias


def _pair(v):
    return '{}, {}'.format(*v)


def make_node(row):
    ins, _ = _inputs(row)
    kw = row.kw
    node = {'name': row.id, 'type': row.entry, 'version': 'opset1'}
    if row.entry == 'SoftMax':
        node['data'] = {'axis': '1'}
    elif row.entry == 'LRN':
        node['data'] = {'alpha': repr(LRN_ALPHA), 'beta': repr(kw['beta']), 'bias': repr(kw['bias']), 'size': str(kw['size'])}
    else:
        node['data'] = {'strides': _pair(kw['s']), 'pads_begin': _pair(kw['pb']), 'pads_end': _pair(kw['pe']), 'auto_pad': 'explicit'}
        if row.entry == 'GroupConvolution':
            node['data']['dilations'] = '1, 1'
        else:
            node['data'].update(kernel=_pair(kw['k']), rounding_type=kw['rounding'])
    node['input'] = {i: {'precision': 'I64' if a.dtype == np.int64 else 'FP32', 'dims': tuple(a.shape)} for i, a in enumerate(ins)}
    node['output'] = {len(ins): {'precision': 'FP32', 'dims': ()}}
    return node


@functools.lru_cache(maxsize=None)
def reference(row):
    """The float64 result of the row (tests/ref64.py), computed once and shared by the tests; read-only."""
    ins, bias = _inputs(row)
    kw = row.kw
    if row.entry == 'SoftMax':
        ref = ref64.softmax_rows(ins[0])
    elif row.entry == 'LRN':
        with np.errstate(all='ignore'):
            ref = ref64.lrn(ins[0], float(np.float32(LRN_ALPHA)), kw['beta'], kw['bias'], kw['size'])
    elif row.entry == 'MaxPool':
        ref = ref64.maxpool(ins[0], kw['s'], kw['pb'], kw['pe'], kw['k'], kw['rounding'])
    elif row.entry == 'AvgPool':
        ref = ref64.avgpool(ins[0], kw['s'], kw['pb'], kw['pe'], kw['k'], kw['rounding'])
    else:
        ref = ref64.group_convolution_depthwise(ins[0], ins[1], kw['s'], kw['pb'], kw['pe'])
        if kw['act'] is not None:
            ref = ref64.add(ref, bias)
            ref = ref64.relu(ref) if kw['act'][0] == 'relu' else ref64.clamp(ref, kw['act'][1], kw['act'][2])
    ref.setflags(write=False)
    return ref


def oracle(row):
    """The oracle's fp32 result of the row (the fused bias / activation through its own ops)."""
    from oracle import ops
    ins, bias = _inputs(row)
    with np.errstate(all='ignore'):
        out = first_out(importlib.import_module('oracle.op_plugins.' + row.entry).compute(make_node(row), dict(enumerate(ins)), kernel_type='special'))
    if bias is not None:
        act = row.kw['act']
        out = ops.add(out, bias)
        out = ops.relu(out) if act[0] == 'relu' else ops.clamp(out, np.float32(act[1]), np.float32(act[2]))
    assert out.dtype == np.float32
    return out


def compare(row, got, what, device_result=False):
    """`got` (fp32) against the float64 reference by the module's rules; returns the max-norm error.  device_result: `got` comes from the
    kernels -- the large-d LRN rows are then held to REL_TOL only and their error printed (the oracle's fp32 result keeps DRIFT there too)."""
    ref = reference(row)
    if row.entry == 'MaxPool':
        assert_bit_exact(got, ref.astype(np.float32), what)
        return 0.0
    edge = row.kw.get('edge')
    if edge == 'zero':
        want = oracle(row)
        assert np.isnan(want).any() and np.isinf(want).any(), what + ': the row holds no 0 / 0 and no x / 0'
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[np.isinf(want)], want[np.isinf(want)]), what + ': NaN / inf pattern'
        assert not (np.isnan(ref) & ~np.isnan(want)).any(), what + ': float64 has a NaN the oracle has not'
        fin = np.isfinite(want)
        got, ref = got[fin], ref[fin]
    err = assert_close(got, ref, helpers.REL_TOL, what)
    if edge == 'large' and device_result:
        print('{}: max-norm error {:.3e}'.format(what, err))
    else:
        assert err <= ref64.DRIFT, '{}: {:.2e}'.format(what, err)
    return err


# ---------------------------------------------------------------------------------------------------------------------- CPU part
@pytest.mark.parametrize('row', ROWS, ids=ROW_IDS)
def test_query_answers_the_form_of_the_row(row, monkeypatch):
    with Env(row, monkeypatch):
        assert query(row) == row.form


def test_table_holds_every_form_the_planners_return():
    seen = {form_class(row, row.form) for row in ROWS}
    assert seen == ALL_FORMS, 'missing {}, unknown {}'.format(sorted(ALL_FORMS - seen, key=str), sorted(seen - ALL_FORMS, key=str))


def test_only_the_marked_avgpool_row_has_an_empty_window():
    for row in ROWS:
        if row.entry == 'AvgPool':
            assert bool(np.isnan(reference(row)).any()) == row.kw['empty'], row.id


@pytest.mark.parametrize('row', ROWS, ids=ROW_IDS)
def test_float64_reference_agrees_with_the_oracle(row):
    compare(row, oracle(row), row.id + ' (oracle)')


# The launchers' inequalities as they stood before the plan functions were lifted out of them (frozen here, dead branches included): the
# plans must be theirs -- launch parameters did not change.  The 3x3 / stride 1 or 2 routes go through plan_pool3, which did not move.
def _old_lds_plan(planes, h, w, oh, hp, wp, kh, sh, group_bytes, band_limit, weights):
    row_bytes, plane_bytes, min_band = wp * 4, hp * wp * 4, (kh + sh) * wp * 4
    if min_band > band_limit:
        return None
    g, band_rows, n_bands = 1, oh, 1
    if plane_bytes <= group_bytes:
        g = group_bytes // plane_bytes
        while g > 4 and (planes + g - 1) // g < 8 * 256:
            g >>= 1
        if (h * w) % 4 != 0 and g >= 4:
            g &= ~3
        g = min(g, planes)
    else:
        budget = group_bytes if group_bytes > min_band else min_band
        band_rows = min(max((budget // row_bytes - kh) // sh + 1, 1), oh)
        n_bands = (oh + band_rows - 1) // band_rows
        band_rows = (oh + n_bands - 1) // n_bands
        n_bands = (oh + band_rows - 1) // band_rows
    rows_l = hp if n_bands == 1 else min((band_rows - 1) * sh + kh, hp)
    lds = (((g * rows_l * wp + 3) & ~3) + g * weights) * 4
    if lds > 64 * 1024 or n_bands > 65535:
        return None
    return g, n_bands, band_rows


def test_plans_are_those_of_the_previous_launchers():
    from pyopenvino_amd import device
    rng = np.random.RandomState(11)
    f = (ctypes.c_int * FORM_INTS)()
    checked = 0
    for _ in range(30000):
        n, c = int(rng.randint(1, 4)), int(rng.randint(1, 41))
        h = int(rng.randint(1, (41, 401, 3001)[rng.randint(3)]))
        w = int(rng.randint(1, (41, 401, 4001)[rng.randint(3)]))
        kh, kw = [(1, 1), (2, 2), (3, 3), (5, 4), (7, 7), (3, 5), (int(rng.randint(1, 121)), int(rng.randint(1, 121)))][rng.randint(7)]
        sh, sw = int(rng.randint(1, 4)), int(rng.randint(1, 4))
        pt, pl, pb, pr = (int(v) for v in rng.randint(0, 4, 4))
        oh, ow = (h + pt + pb - kh) // sh + 1 + int(rng.randint(2)), (w + pl + pr - kw) // sw + 1 + int(rng.randint(2))
        if n * c * h * w > 2e7 or oh < 1 or ow < 1 or ((kh, kw) == (3, 3) and sh == sw and sh < 3):
            continue
        hp, wp = h + pt + pb, w + pl + pr
        if (oh - 1) * sh < hp and (ow - 1) * sw < wp:
            device.call('pvhip_maxpool2d_form', n, c, h, w, oh, ow, kh, kw, sh, sw, pt, pl, pb, pr, f)
            old = _old_lds_plan(n * c, h, w, oh, hp, wp, kh, sh, 16 * 1024, 60 * 1024, 0)
            if old is None:
                want = (0, 0, 0, 0, 0)
            else:
                want = ((3 if (kh, kw) == (3, 3) else 2 if (kh, kw) == (2, 2) else 1),) + old + (int((oh - 1) * sh + kh > hp or (ow - 1) * sw + kw > wp),)
            assert (f[KIND], f[G], f[BANDS], f[BAND_ROWS], f[CLIP]) == want, ('MaxPool', n, c, h, w, oh, ow, kh, kw, sh, sw, pt, pl, pb, pr)
        device.call('pvhip_dwconv2d_form', n, c, h, w, kh, kw, oh, ow, sh, sw, pt, pl, f)
        old = _old_lds_plan(n * c, h, w, oh, max((oh - 1) * sh + kh, h + pt), max((ow - 1) * sw + kw, w + pl), kh, sh, 16 * 1024, 48 * 1024, kh * kw)
        want = (0, 0, 0, 0) if old is None else ((2 if (kh, kw) == (3, 3) else 1),) + old
        assert (f[KIND], f[G], f[BANDS], f[BAND_ROWS]) == want, ('Depthwise', n, c, h, w, kh, kw, oh, ow, sh, sw, pt, pl)
        device.call('pvhip_avgpool2d_form', n, c, h, w, oh, ow, kh, kw, sh, sw, f)
        if h * w * 4 <= 16 * 1024:
            g = 16 * 1024 // (h * w * 4)
            while g > 4 and (n * c + g - 1) // g < 8 * 256:
                g >>= 1
            if (h * w) % 4 != 0 and g >= 4:
                g &= ~3
            want = (1, min(g, n * c))
        else:
            want = (0, 0)
        assert (f[KIND], f[G]) == want, ('AvgPool', n, c, h, w)
        checked += 1
    assert checked > 15000, checked


# ---------------------------------------------------------------------------------------------------------------------- GPU part
@gpu
@pytest.mark.parametrize('row', ROWS, ids=ROW_IDS)
def test_gpu_row(hip, row, monkeypatch, capsys):
    """The row through the plugin, on the form the table names, against float64.

    Max-norm error of the large-d LRN rows against float64, measured on one MI355X (asserted at REL_TOL only, never tightened to these):
    LRN-large-m4 4.990e-07, -m1 9.252e-08, -m2 1.184e-07, -m3 9.488e-08, -m0 2.501e-07, LRN-generic-large-m4 5.325e-07."""
    from pyopenvino_amd import device
    ins, bias = _inputs(row)
    node = make_node(row)
    with Env(row, monkeypatch):
        assert query(row) == row.form
        if bias is not None:
            node['_fuse_bias'], node['_fuse_act'] = device.DeviceTensor.from_numpy(bias), row.kw['act']
        plugin = importlib.import_module('pyopenvino_amd.op_plugins.' + row.entry)
        got = np.asarray(first_out(plugin.compute(node, dict(enumerate(ins)), kernel_type='hip', debug=False)))
    with capsys.disabled():
        compare(row, got, row.id, device_result=True)
