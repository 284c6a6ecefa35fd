"""Every kernel form of the convolution launchers against float64, one explicit row per form.

pw_conv (pvhip_pw.hip), launch_igemm and the f16 LDS-DMA entry (pvhip_conv.hip), wino_conv and wino4_conv (pvhip_wino.hip) pick a kernel,
a template instantiation and a grid from inequalities on channel counts, pixel counts, alignment and kNumCU.  pvhip_conv2d_form
(host-only; it calls the plan functions the launchers switch on) says which form a geometry takes; ROWS below is the table (entry,
geometry, switches, expected form, epilogue).  The form strings are ref64.conv_form's.

CPU part (runs without a device): the query answers the row's form; the table holds every form the planners can return (ALL_FORMS,
with the exclusions listed beside it); the launchers' inequalities as they stood before the plan functions were lifted out of them,
restated here, give the query's answer on a seeded sweep and on every Convolution launch of GoogLeNet and SSD-MobileNet (FP32 and FP16
IRs, batches 1..256); every such launch falls in a class some row runs; ref64.convolution cast to fp32 agrees with the oracle.

GPU part: every row runs through the Convolution plugin under its switches, on the form the table names, and is compared with
ref64.convolution plus the epilogue in float64: fp32 rows ref64.check_group (helpers.REL_TOL in both norms plus ref64.DRIFT; the Winograd
rows without DRIFT, their element-wise excess printed), f16 rows assert_close(1e-5) against float64 on the fp16-rounded operands.

Rows compared on a sample of images (ref64.sample; both ends, at least 12 images, one of which straddles a 32-patch block): a float64
reference of the whole tensor would take more than a few seconds.  All other rows compare the whole tensor.
    wino4-m4-ragged-shared-walk-ge28    (350, 112, 7, 9) -> 250 channels
    wino4-m2-whole-shared-mid2048       (880, 48, 8, 10) -> 250 channels

Not in the table (pvhip_conv2d_form does not report them): the stem entries, the span / c8 / c8-multi readers, the MaxPool + 1x1
launches, the fp32 multi launch with PVHIP_CONV_POINTWISE=0, and the diagnostic build's overrides and ablations.
"""
import functools
import tempfile
import time
import zlib

import numpy as np
import pytest

import helpers
import ref64
import test_batch_forms
from helpers import assert_close, first_out

gpu = pytest.mark.gpu

NUM_CU = 256                                             # kNumCU of pvhip_common.h


# --------------------------------------------------------------------------------------------------------------------- the table
class Row:
    def __init__(self, id_, entry, xs, k, ks, s, pb, pe, form, env=None, epi=None, sampled=False):
        self.id, self.entry, self.xs, self.k, self.ks, self.s, self.pb, self.pe = id_, entry, xs, k, ks, s, pb, pe
        self.form, self.env, self.epi, self.sampled = form, dict(env or {}), epi, sampled
        if entry == 'f16':
            self.env.setdefault('PVHIP_CONV_F16_SPAN', '0')            # (the span kernel takes the stride-1 "same" windows first)

    def __repr__(self):
        return self.id


# epilogues: bias + ReLU, bias + Clamp, bias + ReLU written in place into a wider tensor at channel INTO_OFF (sentinels on both sides)
RELU, CLAMP, INTO = 'relu', 'clamp', 'into'
INTO_OFF, INTO_EXTRA = 3, 7
P0, P1, P2, S1, S2 = (0, 0), (1, 1), (2, 2), (1, 1), (2, 2)
K1, K3, K5, K8 = (1, 1), (3, 3), (5, 5), (8, 8)
FORCE = {'PVHIP_CONV_WINOGRAD4': 'force', 'PVHIP_CONV_WINOGRAD5': 'force'}
SHARED = dict(FORCE, PVHIP_WINO_SHARED='2')
NOPAD = {'PVHIP_CONV_PREPAD': '0'}


def pw(id_, xs, k, form, env=None, epi=None):
    return Row('pw-' + id_, 'f32', xs, k, K1, S1, P0, P0, form, env, epi)


def f32(id_, xs, k, ks, s, pad, form, env=None, epi=None):
    return Row('igemm-' + id_, 'f32', xs, k, ks, s, pad, pad, form, env, epi)


def f16(id_, xs, k, ks, pad, form, env=None, epi=None):
    return Row('f16-' + id_, 'f16', xs, k, ks, S1, pad, pad, form, env, epi)


def w2(id_, xs, k, form, env=None, epi=None):
    return Row('wino2-' + id_, 'f32', xs, k, K3, S1, P1, P1, form, env, epi)


def w4(id_, xs, k, form, env=None, epi=None, sampled=False):
    return Row('wino4-m4-' + id_, 'f32', xs, k, K3, S1, P1, P1, form, env, epi, sampled)


def w25(id_, xs, k, form, env=None, epi=None, sampled=False):
    return Row('wino4-m2-' + id_, 'f32', xs, k, K5, S1, P2, P2, form, env, epi, sampled)


def _kb(kb, small, waves):
    return {'PVHIP_WINO_KB': kb, 'PVHIP_WINO_SMALL': small, 'PVHIP_WINO_WAVES': waves}


ROWS = [
    # ---- pointwise (C = 16).  T = ceil(K / 32) channel tiles, grid2 = ceil(P / 128) ceil(T / 2).  tn = 1: T == 1; grid2 < 4 kNumCU; odd T
    # with grid2 < 16 kNumCU.  Else tn = 2; tn = 4 under PVHIP_PW_TN only.  16-byte copies where h * w is a multiple of 4.
    pw('tn1-T1-vec', (2, 16, 6, 6), 20, 'pw tn=1 vec=1 nchunk=1 stagger=0 grid=1', epi=RELU),
    pw('tn1-few-scalar', (3, 16, 5, 7), 40, 'pw tn=1 vec=0 nchunk=2 stagger=0 grid=2', epi=CLAMP),
    pw('tn1-odd-scalar', (1, 16, 255, 259), 70, 'pw tn=1 vec=0 nchunk=3 stagger=0 grid=1548'),          # grid2 = 516 x 2 = 1032 in [1024, 4096)
    pw('tn2-vec', (2, 16, 254, 258), 40, 'pw tn=2 vec=1 nchunk=1 stagger=0 grid=1024', epi=INTO),      # ceil(131064 / 128) = 1024: the threshold
    pw('tn2-scalar', (2, 16, 255, 257), 50, 'pw tn=2 vec=0 nchunk=1 stagger=0 grid=1024', epi=RELU),
    pw('tn2-odd-vec', (4, 16, 254, 258), 70, 'pw tn=2 vec=1 nchunk=2 stagger=0 grid=4096'),            # T = 3, grid2 = 2048 x 2 = 4096: the threshold
    pw('tn4-vec', (2, 16, 6, 6), 150, 'pw tn=4 vec=1 nchunk=2 stagger=0 grid=2', {'PVHIP_PW_TN': '4'}, epi=CLAMP),
    pw('tn4-scalar', (3, 16, 5, 7), 100, 'pw tn=4 vec=0 nchunk=1 stagger=0 grid=1', {'PVHIP_PW_TN': '4'}, epi=INTO),
    # a non-zero stagger: more than 8 kNumCU workgroups AND PVHIP_PW_STAGGER (its default, 0, leaves every launch unstaggered)
    pw('tn2-stagger', (3, 16, 254, 258), 100, 'pw tn=2 vec=1 nchunk=2 stagger=1 grid=3072', {'PVHIP_PW_STAGGER': '100'}),

    # ---- fp32 implicit GEMM.  bm = 64 when K % 64 is 0 or above 32, ceil(P / 128) ceil(K / 64) >= 4 kNumCU and the window is not 1x1; else 32.
    # (r,s)-major: C = 16; c-major: C = 4 / 5 / 20, through the plugin's padding pass (valid) or with PVHIP_CONV_PREPAD=0 (window test)
    f32('bm64-rs', (2, 16, 254, 254), 300, K3, S2, P1, 'igemm bm=64 kernel=rs mtiles=5 grid=1265', epi=RELU),
    f32('bm32-k-rs', (2, 16, 9, 9), 80, K3, S2, P1, 'igemm bm=32 kernel=rs mtiles=3 grid=3', epi=CLAMP),
    f32('bm32-few-rs', (3, 16, 21, 19), 60, K3, S2, P1, 'igemm bm=32 kernel=rs mtiles=2 grid=6', epi=INTO),
    f32('bm32-1x1-s2-rs', (3, 16, 21, 19), 64, K1, S2, P0, 'igemm bm=32 kernel=rs mtiles=2 grid=6'),
    f32('bm32-1x1-c20-cvalid', (3, 20, 11, 13), 64, K1, S1, P0, 'igemm bm=32 kernel=cvalid mtiles=2 grid=8'),
    f32('bm64-cvalid', (2, 4, 254, 254), 300, K3, S2, P1, 'igemm bm=64 kernel=cvalid mtiles=5 grid=1265', epi=CLAMP),
    f32('bm32-cvalid', (3, 5, 21, 19), 33, K3, S2, P1, 'igemm bm=32 kernel=cvalid mtiles=2 grid=6', epi=INTO),
    f32('bm64-cwindow', (2, 4, 254, 254), 300, K3, S2, P1, 'igemm bm=64 kernel=cwindow mtiles=5 grid=1265', NOPAD, epi=INTO),
    f32('bm32-cwindow', (3, 5, 21, 19), 33, K3, S2, P1, 'igemm bm=32 kernel=cwindow mtiles=2 grid=6', NOPAD, epi=RELU),
    # windows of 64 taps and more: the register-staged kernel
    f32('bm64-reg', (2, 1, 261, 261), 300, K8, S2, P0, 'igemm bm=64 kernel=reg mtiles=5 grid=1265', epi=RELU),
    f32('bm32-reg', (3, 3, 14, 16), 40, K8, S1, P0, 'igemm bm=32 kernel=reg mtiles=2 grid=4', epi=CLAMP),
    # the pointwise copy of the LDS-DMA kernel: in fp32 only with the pointwise kernel switched off
    f32('bm32-pw', (3, 16, 10, 6), 40, K1, S1, P0, 'igemm bm=32 kernel=pw mtiles=2 grid=4', {'PVHIP_CONV_POINTWISE': '0'}, epi=INTO),

    # ---- the f16 LDS-DMA entry: bm = 32 / 64 / 128 for K <= 32 / <= 64 / above, times the four forms of conv_igemm_dma_kernel
    f16('bm32-pw', (3, 16, 10, 6), 20, K1, P0, 'f16 bm=32 kernel=pw mtiles=1 grid=2', epi=RELU),
    f16('bm64-pw', (3, 16, 10, 6), 50, K1, P0, 'f16 bm=64 kernel=pw mtiles=1 grid=2'),
    f16('bm128-pw', (3, 16, 10, 6), 200, K1, P0, 'f16 bm=128 kernel=pw mtiles=2 grid=4', epi=INTO),
    f16('bm32-rs', (3, 16, 10, 6), 20, K3, P1, 'f16 bm=32 kernel=rs mtiles=1 grid=2', epi=CLAMP),
    f16('bm64-rs', (3, 16, 10, 6), 50, K3, P1, 'f16 bm=64 kernel=rs mtiles=1 grid=2', epi=INTO),
    f16('bm128-rs', (3, 16, 10, 6), 200, K3, P1, 'f16 bm=128 kernel=rs mtiles=2 grid=4', epi=RELU),
    f16('bm32-cvalid', (3, 20, 10, 6), 20, K3, P1, 'f16 bm=32 kernel=cvalid mtiles=1 grid=2'),
    f16('bm64-cvalid', (3, 20, 10, 6), 50, K3, P1, 'f16 bm=64 kernel=cvalid mtiles=1 grid=2', epi=RELU),
    f16('bm128-cvalid', (3, 20, 10, 6), 200, K3, P1, 'f16 bm=128 kernel=cvalid mtiles=2 grid=4', epi=CLAMP),
    f16('bm32-cwindow', (3, 20, 10, 6), 20, K3, P1, 'f16 bm=32 kernel=cwindow mtiles=1 grid=2', NOPAD, epi=INTO),
    f16('bm64-cwindow', (3, 20, 10, 6), 50, K3, P1, 'f16 bm=64 kernel=cwindow mtiles=1 grid=2', NOPAD, epi=CLAMP),
    f16('bm128-cwindow', (3, 20, 10, 6), 200, K3, P1, 'f16 bm=128 kernel=cwindow mtiles=2 grid=4', NOPAD),

    # ---- F(2x2,3x3) (C = 4): kb = 64 (eight waves) where 64-channel blocks pad K by at most 12 %, else 32 as 32 channels x 32 patches on
    # four waves; the other workgroup shapes through PVHIP_WINO_KB / _SMALL / _WAVES (test_conv_winograd_3x3's parametrisation)
    w2('kb64', (3, 4, 13, 11), 120, 'wino2 kb=64 patches=32 waves=8 grid=8', epi=RELU),
    w2('kb32-small', (3, 4, 13, 11), 40, 'wino2 kb=32 patches=32 waves=4 grid=8', epi=CLAMP),
    w2('kb32-waves8', (3, 4, 13, 11), 40, 'wino2 kb=32 patches=64 waves=8 grid=4', _kb('32', '0', '8'), epi=INTO),
    w2('kb64-waves4', (3, 4, 13, 11), 120, 'wino2 kb=64 patches=32 waves=4 grid=8', _kb('64', '0', '4')),
    w2('kb32-waves4', (3, 4, 13, 11), 40, 'wino2 kb=32 patches=64 waves=4 grid=4', _kb('32', '0', '4')),

    # ---- the six-point kernels.  Persistent (conv_wino4_kernel): a grid of at most 2 kNumCU = 512 workgroups; shared V
    # (conv_wino4s_kernel): at most kNumCU = 256.  Rows without switches cross the eligibility thresholds themselves: 32 kNumCU = 8192
    # patches on whole extents, 1024 (F(4x4,3x3)) / 4096 (F(2x2,5x5)) on ragged ones.
    w4('whole-persistent-one', (2, 4, 8, 12), 40, 'wino4 m=4 ragged=0 shared=0 order=1 tiles=2 grid=2 walk=0', FORCE, epi=RELU),
    w4('whole-persistent-walk', (9, 4, 128, 128), 50, 'wino4 m=4 ragged=0 shared=0 order=0 tiles=576 grid=512 walk=1', epi=CLAMP),
    w4('ragged-persistent-one', (64, 4, 14, 14), 50, 'wino4 m=4 ragged=1 shared=0 order=0 tiles=64 grid=64 walk=0', epi=INTO),
    w4('ragged-persistent-walk', (2100, 4, 7, 7), 50, 'wino4 m=4 ragged=1 shared=0 order=0 tiles=526 grid=512 walk=1'),
    w4('whole-shared-one', (2, 16, 8, 12), 70, 'wino4 m=4 ragged=0 shared=1 order=1 tiles=2 grid=2 walk=0', SHARED, epi=CLAMP),
    w4('whole-shared-walk', (530, 16, 8, 8), 200, 'wino4 m=4 ragged=0 shared=1 order=0 tiles=268 grid=256 walk=1', SHARED, epi=INTO),
    w4('ragged-shared-one', (3, 16, 7, 9), 70, 'wino4 m=4 ragged=1 shared=1 order=1 tiles=2 grid=2 walk=0', SHARED, epi=RELU),
    # shared V by the `pays` rule, default switches: 28 stages and more (C = 112); 24 stages on ragged extents (C = 96)
    w4('ragged-shared-walk-ge28', (350, 112, 7, 9), 250, 'wino4 m=4 ragged=1 shared=1 order=0 tiles=264 grid=256 walk=1', epi=RELU, sampled=True),
    w4('ragged-shared-ge24', (256, 96, 7, 7), 60, 'wino4 m=4 ragged=1 shared=1 order=0 tiles=32 grid=32 walk=0', epi=CLAMP),
    w25('whole-persistent-one', (2, 4, 8, 12), 40, 'wino4 m=2 ragged=0 shared=0 order=1 tiles=4 grid=4 walk=0', FORCE, epi=CLAMP),
    w25('whole-persistent-walk', (9, 4, 64, 64), 50, 'wino4 m=2 ragged=0 shared=0 order=0 tiles=576 grid=512 walk=1', epi=RELU),
    w25('ragged-persistent-one', (256, 4, 7, 7), 50, 'wino4 m=2 ragged=1 shared=0 order=0 tiles=256 grid=256 walk=0'),
    w25('ragged-persistent-walk', (530, 4, 7, 7), 50, 'wino4 m=2 ragged=1 shared=0 order=0 tiles=530 grid=512 walk=1', epi=INTO),
    w25('whole-shared-one', (2, 16, 8, 12), 70, 'wino4 m=2 ragged=0 shared=1 order=1 tiles=4 grid=4 walk=0', SHARED, epi=INTO),
    w25('whole-shared-walk', (140, 16, 8, 8), 200, 'wino4 m=2 ragged=0 shared=1 order=1 tiles=280 grid=256 walk=1', SHARED),
    w25('ragged-shared-one', (3, 16, 7, 9), 70, 'wino4 m=2 ragged=1 shared=1 order=1 tiles=4 grid=4 walk=0', SHARED, epi=CLAMP),
    w25('ragged-shared-walk', (140, 16, 7, 7), 200, 'wino4 m=2 ragged=1 shared=1 order=1 tiles=280 grid=256 walk=1', SHARED, epi=RELU),
    # ... and 12..16 stages (C = 48) with tiles_s = ceil(17600 / 32) x 4 = 2200 >= 2048
    w25('whole-shared-mid2048', (880, 48, 8, 10), 250, 'wino4 m=2 ragged=0 shared=1 order=0 tiles=2200 grid=256 walk=1', epi=CLAMP, sampled=True),
]

ROW_IDS = [r.id for r in ROWS]
assert len(set(ROW_IDS)) == len(ROW_IDS)


# ----------------------------------------------------------------------------------------------------- every form the planners return
def _all_forms():
    forms = set()
    # pointwise: plan_pw's axes are tn x copy x stagger; tn = 1 by each of its three reasons, tn = 2 with an odd T (a last chunk of one tile)
    forms |= {('pw', tn, copy) for tn in (1, 2, 4) for copy in ('vec', 'scalar')}
    forms |= {('pw', 'tn=1 because', why) for why in ('T == 1', 'few workgroups', 'odd T')}
    forms |= {('pw', 'tn=2', 'odd T'), ('pw', 'stagger', 0), ('pw', 'stagger', 1)}
    # fp32 implicit GEMM: igemm_bm x plan_tiles' kernel.  Cannot occur: (64, 'pw') -- the pointwise copy is a 1x1 window, and a 1x1 window
    # takes bm = 32 (igemm_bm's last rule); bm = 128 -- no fp32 route picks it (PVHIP_CONV_MULTI_BM and the diagnostic build's PVHIP_CONV_TILE
    # do: out of scope).
    forms |= {('igemm', bm, kernel) for bm in (32, 64) for kernel in ('rs', 'cvalid', 'cwindow', 'reg')} | {('igemm', 32, 'pw')}
    forms |= {('igemm', 'bm=32 because', why) for why in ('K % 64 in 1..32', 'few workgroups', '1x1 stride 2', '1x1 C % 16 != 0')}
    # the f16 entry: f16_bm x plan_tiles' kernel.  Cannot occur: 'reg' -- the entry refuses windows of 64 taps and more
    forms |= {('f16', bm, kernel) for bm in (32, 64, 128) for kernel in ('pw', 'rs', 'cvalid', 'cwindow')}
    # F(2x2,3x3): (kb, patches, waves); the first two with default switches.  Cannot occur: (64, 64, .) -- 64-channel blocks always take
    # 32 patches; (32, 32, 8) -- the small form has four waves
    forms |= {('wino2', 64, 32, 8), ('wino2', 32, 32, 4), ('wino2', 32, 64, 8), ('wino2', 64, 32, 4), ('wino2', 32, 64, 4)}
    # the six-point kernels: m x ragged x kernel x walk -- all sixteen occur
    forms |= {('wino4', m, extents, kernel, walk) for m in (4, 2) for extents in ('whole', 'ragged') for kernel in ('shared', 'persistent')
              for walk in ('one', 'walk')}
    forms |= {('wino4', 'shared', 'order', 0), ('wino4', 'shared', 'order', 1)}
    forms |= {('wino4', 'default switches', m, extents) for m in (4, 2) for extents in ('whole', 'ragged')}
    forms |= {('wino4', 'shared pays by', why) for why in ('stages >= 28', 'stages >= 24, ragged', '12..16 stages, tiles_s >= 2048')}
    return forms


ALL_FORMS = _all_forms()


def parse(form):
    head, *fields = form.split()
    return head, {k: (int(v) if v.lstrip('-').isdigit() else v) for k, v in (f.split('=') for f in fields)}


def form_classes(form, args, default_switches=False):
    """The elements of ALL_FORMS a launch with this form string and these library arguments (ref64.conv_form's) belongs to."""
    kind, f = parse(form)
    _, n, c, h, w, k, kh, kw, oh, ow, sh, sw, _, _ = args
    pixels = n * oh * ow
    if kind == 'pw':
        out = {('pw', f['tn'], 'vec' if f['vec'] else 'scalar'), ('pw', 'stagger', f['stagger'])}
        t = -(-k // 32)
        grid2 = -(-pixels // 128) * ((t + 1) // 2)
        if f['tn'] == 1 and default_switches:
            out.add(('pw', 'tn=1 because', 'T == 1' if t == 1 else 'few workgroups' if grid2 < 4 * NUM_CU else 'odd T'))
        if f['tn'] == 2 and t % 2:
            out.add(('pw', 'tn=2', 'odd T'))
        return out
    if kind in ('igemm', 'f16'):
        out = {(kind, f['bm'], f['kernel'])}
        if kind == 'igemm' and f['bm'] == 32:
            if 1 <= k % 64 <= 32:
                out.add(('igemm', 'bm=32 because', 'K % 64 in 1..32'))
            elif (kh, kw) == (1, 1):
                out.add(('igemm', 'bm=32 because', '1x1 C % 16 != 0' if c % 16 else '1x1 stride 2' if (sh, sw) != (1, 1) else '1x1'))
            else:
                out.add(('igemm', 'bm=32 because', 'few workgroups'))
        return out - {('igemm', 'bm=32 because', '1x1')}
    if kind == 'wino2':
        return {('wino2', f['kb'], f['patches'], f['waves'])}
    assert kind == 'wino4', form
    extents = 'ragged' if f['ragged'] else 'whole'
    out = {('wino4', f['m'], extents, 'shared' if f['shared'] else 'persistent', 'walk' if f['walk'] else 'one')}
    if default_switches:
        out.add(('wino4', 'default switches', f['m'], extents))
    if f['shared']:
        out.add(('wino4', 'shared', 'order', f['order']))
        stages = c // 4
        if default_switches:
            out.add(('wino4', 'shared pays by', 'stages >= 28' if stages >= 28 else 'stages >= 24, ragged' if stages >= 24 else
                     '12..16 stages, tiles_s >= 2048'))
    return out


# ------------------------------------------------------------------------------------------------------------------- the form query
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


def lib_args(row):
    """The arguments of ref64.conv_form for the row: the geometry the plugin hands the library (behind its padding pass, if its route has
    one).  Under the row's switches."""
    from pyopenvino_amd.op_plugins import Convolution
    ws = (row.k, row.xs[1]) + row.ks
    r = Convolution.route(row.xs, ws, row.s, row.pb, row.pe, 'explicit', row.entry == 'f16', False, 'dense' if row.epi == INTO else None,
                          False, False, 0, False, False, row.epi == CLAMP)
    assert r.entry == ('pvhip_conv2d_f16_dma' if row.entry == 'f16' else 'pvhip_conv2d_f32'), (row.id, r)
    g = Convolution._geometry(row.xs, ws, row.s, row.pb, row.pe, 'explicit')
    h, w, pads = g.h, g.w, g.pads_begin
    if r.pad_row:
        h, w, pads = g.h + row.pb[0] + row.pe[0], r.pad_row, (0, 0)
    return (ref64.CONV_ENTRIES[r.entry], g.n, g.c, h, w, g.kn, g.kh, g.kw, g.oh, g.ow, *g.strides, *pads)


def query(row):
    return ref64.conv_form(*lib_args(row))


def default_switches(row):
    return not row.env or (row.entry == 'f16' and set(row.env) == {'PVHIP_CONV_F16_SPAN'})


# --------------------------------------------------------------------------------------------------- inputs, node, float64 reference
def _rng(row):
    return np.random.RandomState(zlib.crc32(row.id.encode()) & 0x7fffffff)


@functools.lru_cache(maxsize=None)
def _inputs(row):
    """(x, weights, bias or None), seeded by the row's name; read-only."""
    rng = _rng(row)
    c = row.xs[1]
    x = rng.standard_normal(row.xs).astype(np.float32)
    w = (rng.standard_normal((row.k, c) + row.ks) * (2.0 / (c * row.ks[0] * row.ks[1])) ** 0.5).astype(np.float32)
    bias = (rng.standard_normal((1, row.k, 1, 1)) * 0.5).astype(np.float32) if row.epi else None
    for a in (x, w) + ((bias,) if bias is not None else ()):
        a.setflags(write=False)
    return x, w, bias


def images(row):
    """The images the row compares: the whole batch, or ref64.sample's for the rows marked so."""
    return ref64.sample(row.xs[0]) if row.sampled else list(range(row.xs[0]))


def make_node(row, n=None):
    xs = ((row.xs[0] if n is None else n),) + row.xs[1:]
    pair = '{}, {}'.format
    return {'name': row.id, 'type': 'Convolution', 'version': 'opset1',
            'data': {'strides': pair(*row.s), 'dilations': '1, 1', 'pads_begin': pair(*row.pb), 'pads_end': pair(*row.pe), 'auto_pad': 'explicit'},
            'input': {0: {'precision': 'FP32', 'dims': xs}, 1: {'precision': 'FP32', 'dims': (row.k, row.xs[1]) + row.ks}},
            'output': {2: {'precision': 'FP32', 'dims': ()}}}


def _operands(row):
    x, w, bias = _inputs(row)
    x = x[images(row)] if row.sampled else x
    return (ref64.f16r(x).astype(np.float32), ref64.f16r(w).astype(np.float32), bias) if row.entry == 'f16' else (x, w, bias)


def act_of(row):
    return None if row.epi is None else ('clamp', -0.25, 0.75) if row.epi == CLAMP else ('relu',)


@functools.lru_cache(maxsize=None)
def reference(row):
    """The float64 result of the row on the images it compares (f16 rows: of the fp16-rounded operands), epilogue included; read-only."""
    x, w, bias = _operands(row)
    ref = ref64.convolution(x, w, row.s, row.pb, row.pe)
    if row.epi:
        ref = ref64.add(ref, bias)
        act = act_of(row)
        ref = ref64.relu(ref) if act[0] == 'relu' else ref64.clamp(ref, act[1], act[2])
    ref.setflags(write=False)
    return ref


def oracle(row):
    """The oracle's fp32 result on the same images and operands (the fused bias / activation through its own ops)."""
    import importlib
    from oracle import ops
    x, w, bias = _operands(row)
    out = first_out(importlib.import_module('oracle.op_plugins.Convolution').compute(make_node(row, len(x)), {0: x, 1: w}, kernel_type='special'))
    if row.epi:
        act = act_of(row)
        out = ops.add(out, bias)
        out = ops.relu(out) if act[0] == 'relu' else ops.clamp(out, np.float32(act[1]), np.float32(act[2]))
    assert out.dtype == np.float32
    return out


def is_winograd(row):
    return row.id.startswith('wino')


# ---------------------------------------------------------------------------------------------------------------------- CPU part
@pytest.mark.parametrize('row', ROWS, ids=ROW_IDS)
def test_query_answers_the_form_of_the_row(row, monkeypatch):
    with Env(row, monkeypatch):
        assert query(row) == row.form


def test_table_holds_every_form_the_planners_return(monkeypatch):
    seen = set()
    for row in ROWS:
        with Env(row, monkeypatch):
            seen |= form_classes(row.form, lib_args(row), default_switches(row))
    assert seen == ALL_FORMS, 'missing {}, unknown {}'.format(sorted(ALL_FORMS - seen, key=str), sorted(seen - ALL_FORMS, key=str))


def test_rows_exercise_the_tails(monkeypatch):
    """Per family: a pixel count that is no multiple of 128, a K that ends inside a 32-channel tile and (where bm allows) inside the second
    half of a bm tile, the three epilogues; the walking rows' last round is partly filled; the sampled rows' samples hold both ends, at
    least 12 images and one that straddles a 32-patch block."""
    fams = {}
    for row in ROWS:
        with Env(row, monkeypatch):
            args = lib_args(row)
        kind, f = parse(row.form)
        fam = kind if kind != 'wino4' else 'wino4 m={}'.format(f['m'])
        facts = fams.setdefault(fam, set())
        if (args[1] * args[8] * args[9]) % 128:
            facts.add('ragged pixels')
        if row.k % 32:
            facts.add('K inside a tile')
        bm = f.get('bm', f.get('kb', 0))
        if bm >= 64 and row.k % bm > bm // 2:
            facts.add('K inside the second half')
        facts.add(row.epi)
        if f.get('walk'):
            assert f['tiles'] % f['grid'], row.id
        if row.sampled:
            idx, m = images(row), f['m']
            per = -(-row.xs[2] // m) * -(-row.xs[3] // m)
            assert idx[0] == 0 and idx[-1] == row.xs[0] - 1 and len(idx) >= 12
            assert any((i * per) // 32 != ((i + 1) * per - 1) // 32 for i in idx), row.id
    assert set(fams) == {'pw', 'igemm', 'f16', 'wino2', 'wino4 m=4', 'wino4 m=2'}
    for fam, facts in fams.items():
        want = {'ragged pixels', 'K inside a tile', RELU, CLAMP, INTO} | ({'K inside the second half'} if fam in ('igemm', 'f16', 'wino2') else set())
        assert want <= facts, (fam, want - facts)


def test_query_checks_its_arguments_like_the_entries():
    import ctypes
    from pyopenvino_amd import device
    f = (ctypes.c_int * 16)()
    lib = device.load_library()
    ok = (0, 2, 16, 8, 8, 40, 3, 3, 8, 8, 1, 1, 1, 1)
    assert lib.pvhip_conv2d_form(*ok, f) == 0 and f[0] == 2
    assert ref64.conv_form(0, 0, 16, 8, 8, 40, 3, 3, 8, 8, 1, 1, 1, 1) == 'none'                     # an empty output: nothing is launched
    assert ref64.conv_form(1, 2, 16, 8, 8, 40, 3, 3, 0, 8, 1, 1, 1, 1) == 'none'
    for bad in ((2,) + ok[1:], ok[:2] + (0,) + ok[3:], ok[:10] + (0,) + ok[11:], ok[:12] + (-1,) + ok[13:]):
        assert lib.pvhip_conv2d_form(*bad, f) == -2 and f[0] == -1, bad                              # PVHIP_EINVAL
    unsupported = [(0, 2, 16, 300, 300, 40, 256, 3, 45, 298, 1, 1, 0, 0),                            # a window outside the table encoding
                   (0, 64, 2048, 64, 64, 8, 1, 1, 64, 64, 1, 1, 0, 0),                               # 2^29 input elements
                   (0, 64, 16, 512, 512, 128, 1, 1, 512, 512, 1, 1, 0, 0),                           # 2^31 output elements
                   (1, 2, 16, 12, 12, 40, 8, 8, 5, 5, 1, 1, 0, 0)]                                   # 64 taps on the f16 entry
    for u in unsupported:
        assert lib.pvhip_conv2d_form(*u, f) == -5 and f[0] == -1, u                                  # PVHIP_EUNSUPPORTED
    assert lib.pvhip_conv2d_form(0, 63, 2048, 64, 64, 8, 1, 1, 64, 64, 1, 1, 0, 0, f) == 0           # just below 2^29


@pytest.mark.parametrize('row', ROWS, ids=ROW_IDS)
def test_float64_reference_agrees_with_the_oracle(row):
    err = assert_close(oracle(row), reference(row), helpers.REL_TOL, row.id + ' (oracle)')
    assert err <= ref64.DRIFT, '{}: {:.2e}'.format(row.id, err)


# The launchers' inequalities as they stood before the plan functions were lifted out of them (frozen here): the plans must be theirs --
# no launch parameter moved.  ref64.wino4_form and test_batch_forms.pw_tn are the two restatements the whole-pass tests already held.
def _node(n, c, h, w, k, kh, kw):
    return {'input': {0: {'dims': (n, c, h, w)}, 1: {'dims': (k, c, kh, kw)}}}


def _old_route(n, c, h, w, kh, kw, oh, ow, sh, sw, pt, pl):
    """conv_route with default switches -> 'pw' / 'wino25' / 'wino4' / 'wino2' / 'igemm'."""
    if (kh, kw, sh, sw, pt, pl) == (1, 1, 1, 1, 0, 0) and (oh, ow) == (h, w) and c % 16 == 0:
        return 'pw'
    same = (sh, sw) == (1, 1) and (oh, ow) == (h, w) and c % 4 == 0
    if (kh, kw, pt, pl) == (5, 5, 2, 2) and same:
        if n * -(-h // 2) * -(-w // 2) >= (4096 if h % 2 or w % 2 else 32 * NUM_CU):
            return 'wino25'
    if (kh, kw, pt, pl) == (3, 3, 1, 1) and same:
        if n * -(-h // 4) * -(-w // 4) >= (1024 if h % 4 or w % 4 else 32 * NUM_CU):
            return 'wino4'
        return 'wino2'
    return 'igemm'


def _old_dma_kernel(c, h, w, kh, kw, oh, ow, sh, sw, pt, pl):
    if kh * kw >= 64:
        return 'reg'
    if c % 16 == 0:
        return 'pw' if (kh, kw, sh, sw, pt, pl) == (1, 1, 1, 1, 0, 0) and (oh, ow) == (h, w) and (h * w) % 4 == 0 else 'rs'
    return 'cvalid' if pt == 0 and pl == 0 and (oh - 1) * sh + kh <= h and (ow - 1) * sw + kw <= w else 'cwindow'


def old_form(entry, n, c, h, w, k, kh, kw, oh, ow, sh, sw, pt, pl):
    """What the previous launchers launched for these arguments (default switches), in ref64.conv_form's notation."""
    pixels = n * oh * ow
    ptiles = -(-pixels // 128)
    if entry == 1:
        bm = 128 if k > 64 else 64 if k > 32 else 32
        return 'f16 bm={} kernel={} mtiles={} grid={}'.format(bm, _old_dma_kernel(c, h, w, kh, kw, oh, ow, sh, sw, pt, pl), -(-k // bm), -(-k // bm) * ptiles)
    route = _old_route(n, c, h, w, kh, kw, oh, ow, sh, sw, pt, pl)
    if route == 'pw':
        tn = test_batch_forms.pw_tn(_node(n, c, h, w, k, 1, 1))
        nchunk = -(-(-(-k // 32)) // tn)
        return 'pw tn={} vec={} nchunk={} stagger=0 grid={}'.format(tn, int((h * w) % 4 == 0), nchunk, ptiles * nchunk)
    if route == 'igemm':
        bm = 64 if k % 64 == 0 or k % 64 > 32 else 32
        if bm == 64 and ptiles * -(-k // 64) < 4 * NUM_CU:
            bm = 32
        if (kh, kw) == (1, 1):
            bm = 32
        return 'igemm bm={} kernel={} mtiles={} grid={}'.format(bm, _old_dma_kernel(c, h, w, kh, kw, oh, ow, sh, sw, pt, pl), -(-k // bm), -(-k // bm) * ptiles)
    if route == 'wino2':
        kb = 64 if -(-k // 64) * 64 * 100 <= k * 112 else 32
        return 'wino2 kb={} patches=32 waves={} grid={}'.format(kb, 8 if kb == 64 else 4, -(-(n * -(-h // 2) * -(-w // 2)) // 32) * -(-k // kb))
    m = 4 if route == 'wino4' else 2
    name = ref64.wino4_form(_node(n, c, h, w, k, kh, kw))
    n_tb, n_kb = -(-(n * -(-h // m) * -(-w // m)) // 32), -(-k // 32)
    shared = name.startswith(ref64.WINO4S)
    tiles, cap = (n_tb * ((n_kb + 1) // 2), NUM_CU) if shared else (n_tb * n_kb, 2 * NUM_CU)
    order = int(2 * n_kb * (c // 4 + 1) * 36 * 4 * 32 > n * c * h * w)
    return 'wino4 m={} ragged={} shared={} order={} tiles={} grid={} walk={}'.format(m, int(name.endswith('ragged')), int(shared), order, tiles,
                                                                                       min(tiles, cap), int(tiles > cap))


@functools.lru_cache(maxsize=None)
def model_launches():
    """{(config, conv name, ref64.conv_form arguments)} of every Convolution launch of both models, FP32 and FP16 IRs, at batches 1..256
    whose route enters one of the covered entries (sibling launches with their panel width)."""
    import test_conv_routes
    from pyopenvino_amd.op_plugins import Convolution
    out = set()
    for name, (model, fp16) in sorted(test_batch_forms.CONFIGS.items()):
        with tempfile.TemporaryDirectory() as tmp:
            census = ref64.Census(model, fp16, tmp)
        G = census.net.G
        for n in test_batch_forms.SWEEP:
            census.at(n)
            for cid, facts in test_conv_routes.launch_facts(census.ex).items():
                args = ref64.launch_args(G, census.ex.plan, cid, Convolution.route(*facts))
                if args is not None:
                    out.add((name, G.nodes[cid]['name'], args))
    return out


def test_plans_are_those_of_the_previous_launchers():
    rng = np.random.RandomState(18)
    checked, kinds = 0, set()
    for _ in range(12000):
        entry = int(rng.randint(2))
        n = int(rng.choice([1, 2, 3, 7, 40, 64, 255, 530, 2100]))
        c = int(rng.choice([1, 3, 4, 8, 16, 20, 24, 32, 48, 64, 96, 112, 160]))
        h, w = (int(v) for v in rng.choice([1, 4, 7, 8, 13, 14, 28, 56, 57, 128, 255], 2))
        k = int(rng.choice([1, 20, 32, 33, 60, 64, 70, 96, 128, 130, 200, 256, 300, 1000]))
        kh, kw = [(1, 1), (3, 3), (5, 5), (3, 3), (1, 1), (7, 7), (8, 8), (2, 5)][rng.randint(8)]
        sh, sw = [(1, 1), (1, 1), (2, 2), (2, 1)][rng.randint(4)]
        pt, pl = [((kh - 1) // 2, (kw - 1) // 2), (0, 0), (1, 2)][rng.randint(3)]
        pb, pr = [(pt, pl), (0, 0), (2, 1)][rng.randint(3)]
        oh, ow = (h + pt + pb - kh) // sh + 1, (w + pl + pr - kw) // sw + 1
        if oh < 1 or ow < 1 or n * c * h * w >= 2 ** 29 or n * k * oh * ow >= 2 ** 31 or (entry == 1 and kh * kw >= 64):
            continue
        args = (entry, n, c, h, w, k, kh, kw, oh, ow, sh, sw, pt, pl)
        got = ref64.conv_form(*args)
        assert got == old_form(*args), args
        kinds.add(got.split()[0] + (got.split()[1] if got.startswith('wino4') else ''))
        checked += 1
    assert checked > 8000 and kinds == {'pw', 'igemm', 'f16', 'wino2', 'wino4m=4', 'wino4m=2'}, (checked, kinds)
    launches = model_launches()
    assert len(launches) > 2000
    for _, _, args in launches:
        assert ref64.conv_form(*args) == old_form(*args), args


def test_models_take_only_forms_the_table_holds(monkeypatch):
    """GoogLeNet and SSD-MobileNet, FP32 and FP16 IRs, batches 1..256 (ref64.Census): every Convolution launch that enters
    pvhip_conv2d_f32, the pointwise route of pvhip_conv2d_multi_f32, pvhip_conv2d_f16_dma or pvhip_conv2d_multi_f16_dma takes a form
    of a class some row runs."""
    covered = set()
    for row in ROWS:
        with Env(row, monkeypatch):
            covered |= form_classes(row.form, lib_args(row), default_switches(row))
    launches = model_launches()
    # (the GoogLeNet FP16 IR runs its stem entry and the c8 module form only: none of its launches enters a covered entry)
    assert {name for name, _, _ in launches} == set(test_batch_forms.CONFIGS) - {'googlenet_fp16'}
    taken = {}
    for name, conv, args in launches:
        for cls in form_classes(ref64.conv_form(*args), args, True):
            taken.setdefault(cls, (name, conv, args))
    missing = {cls: where for cls, where in taken.items() if cls not in covered}
    assert not missing, missing
    # the product runs every family, both six-point kernels in both grids, and tn = 1 and 2
    assert {('pw', 1, 'vec'), ('pw', 2, 'vec'), ('igemm', 32, 'rs'), ('f16', 128, 'pw'), ('wino2', 64, 32, 8),
            ('wino4', 4, 'whole', 'shared', 'walk'), ('wino4', 4, 'ragged', 'shared', 'walk'), ('wino4', 2, 'whole', 'persistent', 'walk')} <= set(taken)


# ---------------------------------------------------------------------------------------------------------------------- GPU part
@gpu
@pytest.mark.parametrize('row', ROWS, ids=ROW_IDS)
def test_gpu_row(hip, row, monkeypatch, capsys):
    """The row through the plugin, on the form the table names, against float64."""
    import importlib
    from pyopenvino_amd import device as dev
    plugin = importlib.import_module('pyopenvino_amd.op_plugins.Convolution')
    t0 = time.time()
    x, w, bias = _inputs(row)
    node = make_node(row)
    n, k = row.xs[0], row.k
    with Env(row, monkeypatch):
        assert query(row) == row.form
        kind = parse(row.form)[0]
        if row.entry == 'f16':
            node['_f16_mfma'] = True
        else:
            want = {'pw': 'pointwise', 'igemm': 'implicit GEMM (LDS-DMA)', 'wino2': 'Winograd F(2x2,3x3)'}.get(kind)
            want = want or ('Winograd F(4x4,3x3)' if parse(row.form)[1]['m'] == 4 else 'Winograd F(2x2,5x5)')
            assert plugin.kernel_kind(node)[0] == want, (plugin.kernel_kind(node), want)
        wide = None
        if row.epi:
            node['_fuse_bias'], node['_fuse_act'] = dev.DeviceTensor.from_numpy(bias), act_of(row)
        if row.epi == INTO:
            oh, ow = plugin.calc_output_shape(row.xs[2:], row.ks, row.s, row.pb, row.pe, 'floor', 'explicit')
            wide = dev.DeviceTensor.from_numpy(np.full((n, k + INTO_EXTRA, oh, ow), -1.0, dtype=np.float32))
            node['_out_into'] = (wide, INTO_OFF)
        out = plugin.compute(node, {0: x, 1: w}, kernel_type='hip', debug=False)
        got = np.asarray(wide) if wide is not None else np.asarray(first_out(out))
        assert node['_hip_route'][1].entry == ('pvhip_conv2d_f16_dma' if row.entry == 'f16' else 'pvhip_conv2d_f32')
        if row.entry == 'f16':
            assert node['_hip_f16'] == 'lds-dma'
    if wide is not None:
        assert np.all(got[:, :INTO_OFF] == -1.0) and np.all(got[:, INTO_OFF + k:] == -1.0), row.id + ': sentinel channels written'
        got = got[:, INTO_OFF:INTO_OFF + k]
    if row.sampled:
        got = got[images(row)]
    ref = reference(row)
    with capsys.disabled():
        if row.entry == 'f16':
            assert_close(got, ref, 1e-5, row.id)
        else:
            excess = ref64.check_group(got, ref, winograd=is_winograd(row), what=row.id)
            if is_winograd(row):
                print('\n{}: element-wise excess {:.4f}, {:.1f} s'.format(row.id, excess, time.time() - t0))
