"""The matrix and range of YUV host inputs (IENetwork.input_info[name].preprocess_info.color_standard 'BT601' / 'BT709' / 'BT2020' and
color_range 'LIMITED' / 'FULL'): one integer rule with six ints per combination, applied by the kernels of every YUV feed
(pvhip_input_preprocess_yuv_color_f32 / _packed_color_f32 / _warp_color_f32), bit for bit tests/colorimetry_ref.py followed by the
references of the feed.  The first tests need no GPU."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import colorimetry_ref as cref
import helpers
import letterbox_ref
import packed_ref
import roi_ref
import warp_ref
import yuv_ref
from helpers import MODELS, assert_bit_exact
from preprocess_ref import preprocess

HIP = 'pyopenvino_amd.op_plugins'
YUV420 = ['NV12', 'I420']
YUV422 = ['YUY2', 'UYVY']
ENTRY_YUV = 'pvhip_input_preprocess_yuv_color_f32'
ENTRY_PACKED = 'pvhip_input_preprocess_packed_color_f32'
ENTRY_WARP = 'pvhip_input_preprocess_warp_color_f32'
ENTRIES = {ENTRY_YUV: 19, ENTRY_PACKED: 19, ENTRY_WARP: 18}
NEW_RULES = cref.NEW_RULES
MEAN, STD = [104.0, 117.0, 123.0], [1.0, 57.5, 2.0]
EINVAL = -2


@functools.lru_cache(maxsize=None)
def _weights(model):
    from pyopenvino_amd import synth
    return None if model == 'mnist' else synth.synth_weights(os.path.join(MODELS, model + '.xml'), 7)


def _net(model='googlenet-v1', batch=1):
    from pyopenvino_amd import IECore
    ie = IECore(plugin_package=HIP)
    net = ie.read_network(os.path.join(MODELS, model + '.xml'), weights=_weights(model))
    if batch != 1:
        net.set_batch(batch)
    return ie, net, net.inputs[0]['name']


def _declare(net, name, color, standard=None, range_=None, mean=None, pad=None):
    """`color` 'RAW' declares the U8 / NHWC input the converted frames are fed to; RESIZE_BILINEAR either way."""
    info = net.input_info[name]
    pre = info.preprocess_info
    if color == 'RAW':
        info.precision, info.layout = 'U8', 'NHWC'
    pre.color_format = color
    pre.resize_algorithm = 'RESIZE_BILINEAR'
    if standard is not None:
        pre.color_standard = standard
    if range_ is not None:
        pre.color_range = range_
    if pad is not None:
        pre.pad_value = pad
    if mean is not None:
        pre.init(3)
        for c in range(3):
            pre[c].mean_value, pre[c].std_scale = mean[0][c], mean[1][c]
        pre.mean_variant = 'MEAN_VALUE'


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
def test_standard_and_range_defaults_case_bad_values_and_declaring():
    from pyopenvino_amd.input_format import PreProcessInfo
    assert PreProcessInfo.COLOR_STANDARDS == ('BT601', 'BT709', 'BT2020') and PreProcessInfo.COLOR_RANGES == ('LIMITED', 'FULL')
    ie, net, name = _net('mnist')
    info = net.input_info[name]
    pre = info.preprocess_info
    assert (pre.color_standard, pre.color_range) == ('BT601', 'LIMITED') and not info.declared
    for bad in ('BT.709', '709', 'REC709', 'SRGB', '', None, 709, True):
        with pytest.raises(ValueError, match='color_standard'):
            pre.color_standard = bad
    for bad in ('JFIF', 'PC', 'TV', 'full range', '', None, 1, False):
        with pytest.raises(ValueError, match='color_range'):
            pre.color_range = bad
    assert (pre.color_standard, pre.color_range) == ('BT601', 'LIMITED') and not info.declared
    pre.color_standard = 'bt709'                              # accepted in any case, reported upper case
    assert pre.color_standard == 'BT709' and info.declared
    pre.color_standard = 'Bt2020'
    assert pre.color_standard == 'BT2020'
    pre.color_range = 'full'
    assert pre.color_range == 'FULL'
    pre.color_standard, pre.color_range = 'BT601', 'Limited'
    assert (pre.color_standard, pre.color_range) == ('BT601', 'LIMITED')
    for attribute, value in (('color_standard', 'BT601'), ('color_range', 'LIMITED')):      # setting the default declares the input too
        _, other, other_name = _net('mnist')
        setattr(other.input_info[other_name].preprocess_info, attribute, value)
        assert other.input_info[other_name].declared
    ie.load_network(net)
    for attribute, value in (('color_standard', 'BT709'), ('color_standard', 'BT601'), ('color_range', 'FULL')):
        with pytest.raises(ValueError, match='between read_network and load_network'):
            setattr(pre, attribute, value)
    assert (pre.color_standard, pre.color_range) == ('BT601', 'LIMITED')


def test_standard_and_range_only_for_4d_f32_parameters():
    _, net, name = _net('mnist')
    nid = next(n for n in net.G.nodes if net.G.nodes[n]['name'] == name)
    pre = net.input_info[name].preprocess_info
    net.G.nodes[nid]['data']['element_type'] = 'i32'
    with pytest.raises(NotImplementedError):
        pre.color_standard = 'BT709'
    with pytest.raises(NotImplementedError):
        pre.color_range = 'FULL'
    assert (pre.color_standard, pre.color_range) == ('BT601', 'LIMITED') and not net.input_info[name].declared


@pytest.mark.parametrize('color', ['RAW', 'BGRX', 'RGBX'])
def test_a_rule_beside_a_format_with_nothing_to_convert_is_refused_at_load(color):
    for standard, range_ in (('BT709', None), (None, 'FULL'), ('BT2020', 'FULL')):
        ie, net, name = _net()
        _declare(net, name, color, standard, range_)
        with pytest.raises(ValueError, match=r'^input {}: .*color_format {} holds nothing to convert'.format(re.escape(name), color)):
            ie.load_network(net)
    ie, net, name = _net()                                    # the defaults, set explicitly, are no rule to refuse
    _declare(net, name, color, 'BT601', 'LIMITED')
    ie.load_network(net)


@pytest.mark.parametrize('color', YUV420 + YUV422)
def test_frozen_carries_standard_and_range(color):
    import dataclasses
    from pyopenvino_amd.input_format import InputFormat
    _, net, name = _net()
    info = net.input_info[name]
    assert (info.frozen().standard, info.frozen().full_range, info.frozen().color_rule) == ('BT601', False, (0, 0))
    info.preprocess_info.color_format = color
    assert info.frozen().default_rule
    for standard, range_ in cref.RULES:
        info.preprocess_info.color_standard, info.preprocess_info.color_range = standard, range_
        fmt = info.frozen()
        assert (fmt.color, fmt.standard, fmt.full_range) == (color, standard, range_ == 'FULL')
        assert fmt.color_rule == cref.codes(standard, range_) and fmt.default_rule == ((standard, range_) == ('BT601', 'LIMITED'))
        assert all(type(v) is int for v in fmt.color_rule)
    with pytest.raises(dataclasses.FrozenInstanceError):
        fmt.standard = 'BT601'
    # the 13 positional arguments of before still make a format, of the default rule
    old = InputFormat(name, (2, 3, 224, 224), True, True, True, True, True, False, None, None, color, 'LETTERBOX', 114.0)
    assert (old.standard, old.full_range, old.color_rule, old.default_rule) == ('BT601', False, (0, 0), True)
    assert [f.name for f in dataclasses.fields(InputFormat)][-2:] == ['standard', 'full_range']


def test_the_table_is_rint_of_its_formula():
    assert set(cref.RULES) == {(s, r) for s in cref.STANDARDS for r in cref.RANGES} and len(NEW_RULES) == 5
    for standard, range_ in NEW_RULES:
        want = cref.exact(standard, range_)
        got = cref.RULES[(standard, range_)]
        assert got[0] == want[0]
        assert list(got[1:]) == [int(np.rint(x * 2.0 ** 20)) for x in want[1:]], (standard, range_)
    # the default row: cv2's three-decimal coefficients, not the formula's
    assert cref.RULES[('BT601', 'LIMITED')] == (16, yuv_ref.CY, yuv_ref.CRV, yuv_ref.CGV, yuv_ref.CGU, yuv_ref.CBU)
    assert [round(c / 2.0 ** 20, 3) for c in cref.RULES[('BT601', 'LIMITED')][1:]] == [1.164, 1.596, 0.813, 0.391, 2.018]


def test_the_header_states_the_table_of_the_reference():
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    for (standard, range_), row in cref.RULES.items():
        matrix, full = cref.codes(standard, range_)
        assert re.search(r'\*\s+{}\s+{}\s+\S.*?\s{}\s+{}\s+{}\s+{}\s+{}\s+{}\b'.format(matrix, full, *row), header), (standard, range_)


def test_the_default_rule_is_the_existing_conversion_over_all_byte_triples():
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    for y in range(256):
        assert np.array_equal(cref.convert(np.full_like(u, y), u, v, 'BT601', 'LIMITED'), yuv_ref.convert(np.full_like(u, y), u, v)), y
    assert np.array_equal(cref.convert(7, 8, 9), yuv_ref.convert(7, 8, 9))                 # (and it is the default)


@pytest.mark.parametrize('standard,range_', list(cref.RULES))
def test_rule_against_the_float64_matrix_over_all_byte_triples(standard, range_):
    """All 2^24 (Y, U, V): the 32-bit evaluation equals the 64-bit one -- every intermediate below 2^31 (below 5.8e8) -- and every channel
    is within 1 of the clamped, rounded float64 value of the exact matrix (the default row: of its own constants over 2^20, which are
    cv2's three decimals and not the exact matrix)."""
    yoff, cy, crv, cgv, cgu, cbu = cref.RULES[(standard, range_)]
    if (standard, range_) == ('BT601', 'LIMITED'):
        k = [c / 2.0 ** 20 for c in (cy, crv, cgv, cgu, cbu)]
    else:
        k = list(cref.exact(standard, range_)[1:])
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    uf, vf = u - 128.0, v - 128.0
    u64, v64 = (u - 128).astype(np.int64), (v - 128).astype(np.int64)
    worst, biggest = 0.0, 0
    for y in range(256):
        got = cref.convert(np.full_like(u, y), u, v, standard, range_)
        yl = k[0] * max(y - yoff, 0)
        want = np.stack([yl + k[4] * uf, yl - k[2] * vf - k[3] * uf, yl + k[1] * vf], -1)
        worst = max(worst, float(np.abs(got - np.rint(np.clip(want, 0, 255))).max()))
        t = max(y - yoff, 0) * cy + (1 << 19)
        wide = np.stack([t + cbu * u64, t - cgv * v64 - cgu * u64, t + crv * v64], -1)
        biggest = max(biggest, int(np.abs(wide).max()), int(np.abs(cgv * v64).max()), int(np.abs(t - cgv * v64).max()), int(t))
        assert np.array_equal(got, np.clip(wide >> 20, 0, 255)), y
    assert worst <= 1.0, worst
    assert biggest <= 5.8e8 < 2 ** 31, biggest


# One saturated green per rule, encoded with the rule's own exact matrix (rounded): (Y, U, V).
GREEN = {('BT601', 'LIMITED'): (145, 54, 34), ('BT709', 'LIMITED'): (173, 42, 26), ('BT2020', 'LIMITED'): (164, 47, 25),
         ('BT601', 'FULL'): (150, 44, 21), ('BT709', 'FULL'): (182, 30, 12), ('BT2020', 'FULL'): (173, 36, 11)}


@pytest.mark.parametrize('standard,range_', list(cref.RULES))
def test_known_triples(standard, range_):
    black, white = ((16, 235) if range_ == 'LIMITED' else (0, 255))
    assert cref.convert(black, 128, 128, standard, range_).tolist() == [0, 0, 0]
    assert cref.convert(white, 128, 128, standard, range_).tolist() == [255, 255, 255]
    # the encoding is what the formula says it is
    kr, kb = cref.KR_KB[standard]
    luma, ys, cs = (1 - kr - kb), (219.0 if range_ == 'LIMITED' else 255.0), (224.0 if range_ == 'LIMITED' else 255.0)
    encoded = (black + ys * luma, 128 + cs * (0 - luma) / (2 * (1 - kb)), 128 + cs * (0 - luma) / (2 * (1 - kr)))
    assert GREEN[(standard, range_)] == tuple(int(np.rint(x)) for x in encoded)
    right = cref.convert(*GREEN[(standard, range_)], standard, range_).astype(int)
    assert np.abs(right - [0, 255, 0]).max() <= 1, right
    # ... and what makes the attribute observable: every other standard decodes this green more than 8 levels off
    for other in cref.STANDARDS:
        if other != standard:
            wrong = cref.convert(*GREEN[(standard, range_)], other, range_).astype(int)
            assert np.abs(wrong - right).max() > 8, (other, wrong.tolist(), right.tolist())
    # ... and the range: a full-range frame's dark greys are not crushed to black
    assert cref.convert(16, 128, 128, standard, range_).tolist() == ([0, 0, 0] if range_ == 'LIMITED' else [16, 16, 16])


def test_restatement_takes_the_chroma_the_existing_references_take():
    rng = np.random.default_rng(709)
    y = rng.integers(0, 256, (2, 6, 10), dtype=np.uint8)
    u, v = rng.integers(0, 256, (2, 2, 3, 5), dtype=np.uint8)
    for color in YUV420:
        frames = yuv_ref.frames_of(y, u, v, color)
        assert np.array_equal(cref.to_bgr(frames, color), yuv_ref.to_bgr(frames, color))
        image = cref.to_bgr(frames, color, 'BT709', 'FULL')
        assert image.shape == (2, 6, 10, 3) and image[1, 5, 8].tolist() == cref.convert(y[1, 5, 8], u[1, 2, 4], v[1, 2, 4], 'BT709', 'FULL').tolist()
    u, v = rng.integers(0, 256, (2, 2, 6, 5), dtype=np.uint8)
    for color in YUV422:
        frames = packed_ref.frames_of(y, u, v, color)
        assert np.array_equal(cref.to_bgr(frames, color), packed_ref.to_bgr(frames, color))
        image = cref.to_bgr(frames, color, 'BT2020', 'LIMITED')
        assert image[0, 5, 9].tolist() == cref.convert(y[0, 5, 9], u[0, 5, 4], v[0, 5, 4], 'BT2020', 'LIMITED').tolist()


def test_abi_declares_and_exports_the_color_entries():
    from pyopenvino_amd import device
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    lib = device.load_library()
    nm = subprocess.run(['nm', '-D', '--defined-only', device.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for entry, count in ENTRIES.items():
        assert entry in device.SIGNATURES and len(device.SIGNATURES[entry][1]) == count and entry not in device._NOT_STATUS
        m = re.search(r'\b' + entry + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S)
        assert m and len(m.group(1).split(',')) == count and ' '.join(m.group(1).split()).endswith('int matrix, int full_range')
        assert hasattr(lib, entry) and re.search(r' T ' + entry + r'\b', nm)
    assert re.search(r'#define\s+PVHIP_ABI_VERSION\s+19\b', header) and lib.pvhip_abi_version() == 19


# ---------------------------------------------------------------------------------------------------------------- GPU
def _frames(rng, color, n, hw):
    """Half the frames random bytes (most triples saturate: the clamp), half forward-encoded random images (mostly they do not)."""
    h, w = hw
    shape = (n, 3 * h // 2, w) if color in YUV420 else (n, h, w, 2)
    out = rng.integers(0, 256, shape, dtype=np.uint8)
    bgr = rng.integers(0, 256, (n - n // 2, h, w, 3), dtype=np.uint8)
    if color in YUV420:
        out[n // 2:] = yuv_ref.frames_of(*yuv_ref.planes_from_bgr(bgr), color)
    else:
        out[n // 2:] = packed_ref.frames_from_bgr(bgr, color)
    return out


def _extent(color, frames):
    return (frames.shape[1] // 3 * 2, frames.shape[2]) if color in YUV420 else frames.shape[1:3]


def _how(color):
    return int(color == 'I420') if color in YUV420 else packed_ref.KINDS[color]


class _Launch:
    """The frames on the device, and launches into a destination prefilled with 0x7f bytes."""

    def __init__(self, hip, color, frames):
        self.hip, self.color, self.m, self.hw = hip, color, frames.shape[0], _extent(color, frames)
        self.src = hip.DeviceTensor.from_numpy(np.ascontiguousarray(frames))
        self.mean, self.std = hip.DeviceTensor.from_numpy(np.float32(MEAN)), hip.DeviceTensor.from_numpy(np.float32(STD))

    def _dst(self, n, dst_hw):
        dst = self.hip.DeviceTensor.empty((n, 3) + tuple(dst_hw))
        self.hip.call('pvhip_memset', ctypes.c_void_p(dst.ptr), 0x7f, dst.nbytes)
        return dst

    def _pre(self, reverse, scaled):
        return int(reverse), ctypes.c_void_p(self.mean.ptr) if scaled else None, ctypes.c_void_p(self.std.ptr) if scaled else None

    def run(self, dst_hw, rule=None, rois=None, largest=None, fit=0, pad=0.0, reverse=False, scaled=False, entry=None):
        """`rule` = (standard, range): the _color_ entry of the format; None: the existing `entry`, with the arguments it takes."""
        n = self.m if rois is None else len(rois)
        dst = self._dst(n, dst_hw)
        table = self.hip.DeviceTensor.from_numpy(np.ascontiguousarray(rois, np.int32)) if rois is not None else None
        where = (ctypes.c_void_p(self.src.ptr), ctypes.c_void_p(dst.ptr))
        tp = ctypes.c_void_p(table.ptr) if table is not None else None
        largest = largest if largest is not None else self.hw
        tail = (_how(self.color), *self._pre(reverse, scaled))
        if rule is not None:
            self.hip.call(ENTRY_YUV if self.color in YUV420 else ENTRY_PACKED, *where, tp, n, self.m, *self.hw, *dst_hw, *largest, *tail,
                          fit, pad, *cref.codes(*rule))
        elif entry.endswith('_fit_f32'):
            self.hip.call(entry, *where, tp, n, self.m, *self.hw, *dst_hw, *largest, *tail, fit, pad)
        elif entry.endswith('_roi_f32'):
            self.hip.call(entry, *where, tp, n, self.m, *self.hw, *dst_hw, *largest, *tail)
        else:
            self.hip.call(entry, *where, n, *self.hw, *dst_hw, *tail)
        return np.asarray(dst)

    def warp(self, table, dst_hw, rule=None, pad=0.0, reverse=False, scaled=False):
        n = len(table)
        dst = self._dst(n, dst_hw)
        t = self.hip.DeviceTensor.from_numpy(np.ascontiguousarray(table, np.int64))
        args = (ctypes.c_void_p(self.src.ptr), ctypes.c_void_p(dst.ptr), ctypes.c_void_p(t.ptr), n, self.m, 3, *self.hw, *dst_hw,
                1 if self.color in YUV420 else 2, _how(self.color), *self._pre(reverse, scaled), pad)
        if rule is not None:
            self.hip.call(ENTRY_WARP, *args, *cref.codes(*rule))
        else:
            self.hip.call('pvhip_input_preprocess_warp_f32', *args)
        return np.asarray(dst)


OPTIONS = [dict(), dict(reverse=True, scaled=True)]


def _pre_of(opt):
    return dict(reverse_channels=opt.get('reverse', False), mean=MEAN if opt.get('scaled') else None, std_scale=STD if opt.get('scaled') else None)


@pytest.mark.gpu
@pytest.mark.parametrize('src_hw,dst_hw', [((2, 2), (5, 3)), ((38, 42), (13, 17)), ((38, 42), (38, 42))])
@pytest.mark.parametrize('color', YUV420)
def test_yuv_color_entry_bit_exact(hip, color, src_hw, dst_hw):
    rng = np.random.default_rng(sum(src_hw) * 31 + sum(dst_hw) + len(color))
    frames = _frames(rng, color, 2, src_hw)
    dev = _Launch(hip, color, frames)
    for rule in NEW_RULES:
        bgr = cref.to_bgr(frames, color, *rule)
        assert not np.array_equal(bgr, yuv_ref.to_bgr(frames, color))
        for opt in OPTIONS:
            want = preprocess(bgr, dst_hw, nhwc=True, **_pre_of(opt))
            assert_bit_exact(dev.run(dst_hw, rule, **opt), want, '{} {} {} -> {} {}'.format(color, rule, src_hw, dst_hw, sorted(opt)))


@pytest.mark.gpu
@pytest.mark.parametrize('src_hw,dst_hw', [((3, 6), (5, 4)), ((37, 42), (13, 17))])
@pytest.mark.parametrize('color', YUV422)
def test_packed_color_entry_bit_exact(hip, color, src_hw, dst_hw):
    rng = np.random.default_rng(sum(src_hw) * 31 + sum(dst_hw) + len(color))
    frames = _frames(rng, color, 2, src_hw)
    dev = _Launch(hip, color, frames)
    for rule in NEW_RULES:
        bgr = cref.to_bgr(frames, color, *rule)
        assert not np.array_equal(bgr, packed_ref.to_bgr(frames, color))
        for opt in OPTIONS:
            want = preprocess(bgr, dst_hw, nhwc=True, **_pre_of(opt))
            assert_bit_exact(dev.run(dst_hw, rule, **opt), want, '{} {} {} -> {} {}'.format(color, rule, src_hw, dst_hw, sorted(opt)))


# m = 2 frames of (38, 42), n = 3 rows: an odd origin and odd sizes; the whole of frame 0; a frame that is not there
ROIS = np.array([(1, 5, 3, 21, 17), (0, 0, 0, 42, 38), (2, 0, 0, 5, 5)], np.int32)


def _rois_ref(bgr, rois, dst_hw, **pre):
    rows = [roi_ref.preprocess_rois(bgr, rois[b:b + 1], dst_hw, nhwc=True, **pre)[0] if roi_ref.valid(rois[b:b + 1], 1, len(bgr), bgr.shape[1:3])
            else np.full((3,) + tuple(dst_hw), np.nan, np.float32) for b in range(len(rois))]
    return np.stack(rows, 0)


@pytest.mark.gpu
@pytest.mark.parametrize('color', YUV420 + YUV422)
def test_color_entries_bit_exact_on_a_table(hip, color):
    rng = np.random.default_rng(5 + len(color) + ord(color[0]))
    frames = _frames(rng, color, 2, (38, 42))
    dev = _Launch(hip, color, frames)
    dst_hw = (13, 17)
    for rule in (('BT709', 'LIMITED'), ('BT2020', 'FULL')):
        bgr = cref.to_bgr(frames, color, *rule)
        for opt in OPTIONS:
            want = _rois_ref(bgr, ROIS, dst_hw, **_pre_of(opt))
            assert np.isnan(want[2]).all() and np.isfinite(want[:2]).all()
            got = dev.run(dst_hw, rule, rois=ROIS, largest=(38, 42), **opt)
            assert_bit_exact(got, want, '{} {} rectangles {}'.format(color, rule, sorted(opt)))
            assert (got[2].view(np.uint32) == 0x7fc00000).all()       # quiet NaN


@pytest.mark.gpu
@pytest.mark.parametrize('color', YUV420 + YUV422)
def test_color_entries_bit_exact_under_a_letterbox(hip, color):
    rng = np.random.default_rng(11 + len(color) + ord(color[0]))
    frames = _frames(rng, color, 2, (20, 54))
    dev = _Launch(hip, color, frames)
    dst_hw, pad = (16, 16), 114.0
    assert letterbox_ref.geometry((20, 54), dst_hw, 'LETTERBOX') == (0, 5, 16, 6)
    for rule in (('BT709', 'FULL'), ('BT601', 'FULL')):
        bgr = cref.to_bgr(frames, color, *rule)
        for opt in OPTIONS:
            want = letterbox_ref.fit_images(bgr, dst_hw, 'LETTERBOX', pad, nhwc=True, **_pre_of(opt))
            assert_bit_exact(dev.run(dst_hw, rule, fit=1, pad=pad, **opt), want, '{} {} letterbox {}'.format(color, rule, sorted(opt)))


@pytest.mark.gpu
@pytest.mark.parametrize('color', ['NV12', 'YUY2'])
def test_warp_color_entry_bit_exact(hip, color):
    from pyopenvino_amd import warp
    rng = np.random.default_rng(30 + len(color) + ord(color[0]))
    hw, dst_hw, pad = (38, 42), (13, 17), 114.0
    frames = _frames(rng, color, 2, hw)
    turned = warp.rotated_rect(41, 0.5, 1.7 * 17, 1.7 * 13, 30, dst_hw)          # about the top right corner: it leaves the frame
    corners = warp.apply(turned, [[0, 0], [16, 0], [16, 12], [0, 12]])
    assert corners[:, 0].max() > 42 and corners[:, 1].min() < -1
    table = warp_ref.table_of(np.array([turned, [[1, 0, 3], [0, 1, 2]]], np.float64), [1, 0])
    dev = _Launch(hip, color, frames)
    for rule in (('BT709', 'LIMITED'), ('BT2020', 'FULL')):
        bgr = cref.to_bgr(frames, color, *rule)
        for opt in OPTIONS:
            want = warp_ref.warp(bgr, table, dst_hw, True, opt.get('reverse', False), MEAN if opt.get('scaled') else None,
                                 STD if opt.get('scaled') else None, pad, 'RAW')
            got = dev.warp(table, dst_hw, rule, pad=pad, **opt)
            assert_bit_exact(got, want, '{} {} warps {}'.format(color, rule, sorted(opt)))
        plain = dev.warp(table, dst_hw, rule)                  # the integer translation is a slice of the converted frame
        assert np.array_equal(plain[1], bgr[0, 2:15, 3:20].transpose(2, 0, 1).astype(np.float32))


@pytest.mark.gpu
def test_color_entries_with_the_default_rule_give_the_bits_of_the_existing_entries(hip):
    rng = np.random.default_rng(601)
    default = ('BT601', 'LIMITED')
    table = warp_ref.table_of(np.array([[[0.9, -0.4, 7.3], [0.4, 0.9, -3.1]], [[1, 0, 3], [0, 1, 2]]], np.float64), [1, 0])
    for color, family in (('NV12', 'yuv'), ('I420', 'yuv'), ('YUY2', 'packed'), ('UYVY', 'packed')):
        dev = _Launch(hip, color, _frames(rng, color, 2, (38, 42)))
        stem = 'pvhip_input_preprocess_' + family
        for opt in OPTIONS:
            what = '{} {} '.format(color, sorted(opt))
            assert_bit_exact(dev.run((13, 17), default, **opt), dev.run((13, 17), entry=stem + '_f32', **opt), what + 'whole images')
            assert_bit_exact(dev.run((38, 42), default, **opt), dev.run((38, 42), entry=stem + '_f32', **opt), what + 'no resize')
            assert_bit_exact(dev.run((13, 17), default, rois=ROIS, largest=(38, 42), **opt),
                             dev.run((13, 17), rois=ROIS, largest=(38, 42), entry=stem + '_roi_f32', **opt), what + 'rectangles')
            for rois in (None, ROIS):
                assert_bit_exact(dev.run((16, 24), default, rois=rois, fit=1, pad=114.0, **opt),
                                 dev.run((16, 24), rois=rois, fit=1, pad=114.0, entry=stem + '_fit_f32', **opt), what + 'fitted')
            assert_bit_exact(dev.warp(table, (13, 17), default, pad=114.0, **opt), dev.warp(table, (13, 17), pad=114.0, **opt), what + 'warps')
    # four-byte pixels and raw frames take the entries too, with the only rule they admit
    bgrx = rng.integers(0, 256, (2, 9, 7, 4), dtype=np.uint8)
    src = hip.DeviceTensor.from_numpy(bgrx)
    got = []
    for entry, rule in ((ENTRY_PACKED, (0, 114.0, 0, 0)), ('pvhip_input_preprocess_packed_fit_f32', (1, 114.0))):
        dst = hip.DeviceTensor.empty((2, 3, 5, 6))
        hip.call(entry, ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), None, 2, 2, 9, 7, 5, 6, 9, 7, 2, 0, None, None, *rule)
        got.append(np.asarray(dst))
    assert_bit_exact(got[0], preprocess(bgrx[..., :3], (5, 6), nhwc=True), 'BGRX through the _color_ entry, stretched')
    assert_bit_exact(got[1], letterbox_ref.fit_images(bgrx[..., :3], (5, 6), 'LETTERBOX', 114.0), 'BGRX, fitted')
    t = hip.DeviceTensor.from_numpy(table)
    for how, image in ((3, bgrx[..., :3]), ):
        both = []
        for entry, rule in ((ENTRY_WARP, (0, 0)), ('pvhip_input_preprocess_warp_f32', ())):
            dst = hip.DeviceTensor.empty((2, 3, 5, 6))
            hip.call(entry, ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), ctypes.c_void_p(t.ptr), 2, 2, 3, 9, 7, 5, 6, 0, how, 0, None, None,
                     1.0, *rule)
            both.append(np.asarray(dst))
        assert_bit_exact(both[0], both[1], 'raw U8 NHWC warps')


@pytest.mark.gpu
def test_color_entries_reject_what_they_cannot_do(hip):
    lib = hip.load_library()
    src = hip.DeviceTensor.from_numpy(np.zeros(256, np.uint8))
    dst = hip.DeviceTensor.from_numpy(np.full(64, 7, np.float32))
    table = hip.DeviceTensor.from_numpy(np.array([[0, 65536, 0, 0, 0, 65536, 0]], np.int64))
    s, d, t = ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), ctypes.c_void_p(table.ptr)
    yuv, packed, warp = (getattr(lib, e) for e in (ENTRY_YUV, ENTRY_PACKED, ENTRY_WARP))
    sizes = (1, 1, 4, 4, 2, 2, 4, 4)                          # n, m, src, dst, largest
    pad = ctypes.c_float(0.0)
    for matrix, full in ((3, 0), (-1, 0), (0, 2), (1, -1), (3, 2)):
        assert yuv(s, d, None, *sizes, 0, 0, None, None, 0, pad, matrix, full) == EINVAL, (matrix, full)
        assert packed(s, d, None, *sizes, 0, 0, None, None, 0, pad, matrix, full) == EINVAL, (matrix, full)
        assert warp(s, d, t, 1, 1, 3, 4, 4, 2, 2, 1, 0, 0, None, None, pad, matrix, full) == EINVAL, (matrix, full)
    for kind in (2, 3):                                       # four-byte pixels hold nothing to convert
        for matrix, full in ((1, 0), (0, 1), (2, 1)):
            assert packed(s, d, None, *sizes, kind, 0, None, None, 0, pad, matrix, full) == EINVAL, (kind, matrix, full)
            assert warp(s, d, t, 1, 1, 3, 4, 4, 2, 2, 2, kind, 0, None, None, pad, matrix, full) == EINVAL, (kind, matrix, full)
    for how in range(4):                                      # nor do raw frames
        assert warp(s, d, t, 1, 1, 3, 4, 4, 2, 2, 0, how, 0, None, None, pad, 0, 1) == EINVAL, how
        assert warp(s, d, t, 1, 1, 3, 4, 4, 2, 2, 0, how, 0, None, None, pad, 2, 0) == EINVAL, how
    # the limits of the entries they generalise: a fit that is none, a pad that is not finite under a fit, odd extents, no source
    assert yuv(s, d, None, *sizes, 0, 0, None, None, 3, pad, 1, 1) == EINVAL
    assert yuv(s, d, None, *sizes, 0, 0, None, None, 1, ctypes.c_float(np.inf), 1, 1) == EINVAL
    assert yuv(s, d, None, 1, 1, 3, 4, 2, 2, 3, 4, 0, 0, None, None, 0, pad, 1, 1) == EINVAL
    assert packed(s, d, None, 1, 1, 4, 3, 2, 2, 4, 3, 0, 0, None, None, 0, pad, 1, 1) == EINVAL
    assert yuv(None, d, None, *sizes, 0, 0, None, None, 0, pad, 1, 1) == EINVAL
    assert np.array_equal(np.asarray(dst), np.full(64, 7, np.float32))           # nothing was launched
    assert yuv(s, d, None, *sizes, 0, 0, None, None, 0, pad, 1, 1) == 0          # (and the same arguments in order are taken)
    assert packed(s, d, None, *sizes, 1, 0, None, None, 1, pad, 2, 1) == 0
    assert warp(s, d, t, 1, 1, 3, 4, 4, 2, 2, 1, 1, 0, None, None, pad, 2, 0) == 0
    assert not np.array_equal(np.asarray(dst), np.full(64, 7, np.float32))


def _fixed(ex, name):
    return np.asarray(ex.host_inputs.slots[name].fixed).copy()


@pytest.mark.gpu
def test_googlenet_from_bt709_full_range_nv12_frames(hip):
    """NV12 + BT709 + FULL + RESIZE_BILINEAR on (38, 42) frames at batch 2: the Result of the same frames converted by the restatement
    on the host and fed as U8 NHWC, bit for bit; the same declaration with the standard left at its default gives another one."""
    rng = np.random.default_rng(709)
    frames = _frames(rng, 'NV12', 2, (38, 42))
    bgr = cref.to_bgr(frames, 'NV12', 'BT709', 'FULL')
    mean = (MEAN, STD)
    ie, net, name = _net('googlenet-v1', 2)
    out_name = net.outputs[0]['name']
    _declare(net, name, 'RAW', mean=mean)
    ex_bgr = ie.load_network(net)
    want = np.array(ex_bgr.infer({name: bgr})[out_name], copy=True)
    want_input = _fixed(ex_bgr, name)
    assert np.isfinite(want).all()
    assert_bit_exact(want_input, preprocess(bgr, (224, 224), mean=MEAN, std_scale=STD), 'the U8 / NHWC input tensor')

    ie, net, name = _net('googlenet-v1', 2)
    _declare(net, name, 'NV12', 'BT709', 'FULL', mean=mean)
    ex = ie.load_network(net)
    for step in range(3):                                     # (the third pass replays the recording)
        got = ex.infer({name: frames})[out_name]
        assert_bit_exact(_fixed(ex, name), want_input, 'BT709 FULL input tensor, pass {}'.format(step))
        assert_bit_exact(got, want, 'BT709 FULL (2, 57, 42) NV12 through infer(), pass {}'.format(step))
    req = ex.requests[0]
    buf = req.input_buffer(name, (38, 42))
    buf[...] = frames
    assert_bit_exact(req.infer({name: buf})[out_name], want, 'from the request buffer')

    ie, net, name = _net('googlenet-v1', 2)
    _declare(net, name, 'NV12', None, 'FULL', mean=mean)      # the standard left at its default: BT.601
    ex = ie.load_network(net)
    other = np.array(ex.infer({name: frames})[out_name], copy=True)
    other_input = _fixed(ex, name)
    assert_bit_exact(other_input, preprocess(cref.to_bgr(frames, 'NV12', 'BT601', 'FULL'), (224, 224), mean=MEAN, std_scale=STD), 'BT601 FULL')
    assert not np.array_equal(other_input, want_input) and not np.array_equal(other, want)


@pytest.mark.gpu
def test_roi_and_warp_feeds_follow_the_declared_standard(hip):
    """A RoiInput, a WarpInput and a DetectedRois pass on GoogLeNet with NV12 + BT709 (LIMITED) declared: the input tensor is the reference's of the
    converted frames, the Result that of a network without declared formats fed that tensor."""
    from pyopenvino_amd import RoiInput, WarpInput, warp
    rng = np.random.default_rng(7090)
    n, m, hw, pad = 2, 3, (38, 42), 114.0
    frames = _frames(rng, 'NV12', m, hw)
    bgr = cref.to_bgr(frames, 'NV12', 'BT709', 'LIMITED')
    assert not np.array_equal(bgr, yuv_ref.to_bgr(frames, 'NV12'))
    rois = np.array([(2, 5, 3, 21, 17), (0, 0, 0, 42, 38)], np.int32)
    M = np.stack([warp.rotated_rect(41, 0.5, 30, 26, 30, (224, 224)), warp.rotated_rect(21, 19, 20, 18, -75, (224, 224))], 0)
    ids = [1, 2]
    want_inputs = {'rois': roi_ref.preprocess_rois(bgr, rois, (224, 224), nhwc=True, mean=MEAN, std_scale=STD),
                   'warps': warp_ref.warp(bgr, warp_ref.table_of(M, ids), (224, 224), True, False, MEAN, STD, pad, 'RAW')}
    assert (want_inputs['warps'][0, 0] == (np.float32(pad) - np.float32(MEAN[0])) / np.float32(STD[0])).any()    # pad taps are in it
    ie, net, name = _net('googlenet-v1', n)
    out_name = net.outputs[0]['name']
    plain = ie.load_network(net)
    want = {k: np.array(plain.infer({name: v})[out_name], copy=True) for k, v in want_inputs.items()}
    ie, net, name = _net('googlenet-v1', n)
    _declare(net, name, 'NV12', 'BT709', mean=(MEAN, STD), pad=pad)
    ex = ie.load_network(net)
    for step in range(2):
        for what, feed in (('rois', RoiInput(frames, rois)), ('warps', WarpInput(frames, M, ids))):
            got = ex.infer({name: feed})[out_name]
            assert_bit_exact(_fixed(ex, name), want_inputs[what], 'BT709 {} input tensor, pass {}'.format(what, step))
            assert_bit_exact(got, want[what], 'BT709 {} through infer(), pass {}'.format(what, step))
    # a DetectedRois pass: the table is made on the device from records, the frames convert by the same declared rule
    from pyopenvino_amd import DetectedRois
    import detected_rois_ref
    rec = np.zeros((3 * 2, 7), np.float32)                    # two records per image; image 1 has both of the survivors
    rec[:, 0] = np.repeat(np.arange(3), 2)
    rec[:, 1], rec[:, 2] = 1, [0.1, 0.2, 0.9, 0.8, 0.3, 0.1]
    rec[:, 3:] = [(0.1, 0.1, 0.6, 0.7), (0, 0, 1, 1), (0.13, 0.07, 0.64, 0.55), (0, 0, 1, 1), (0.2, 0.2, 0.5, 0.5), (0, 0, 1, 1)]
    table = detected_rois_ref.detected_rois(rec, n, m, hw, min_confidence=0.5)
    assert table.count == n and (table.rois[:, 0] == 1).all() and table.rois[0, 1] % 2 == 1 and table.rois[0, 4] % 2 == 1      # (an odd origin, an odd height)
    want_input = roi_ref.preprocess_rois(bgr, table.rois, (224, 224), nhwc=True, mean=MEAN, std_scale=STD)
    want_out = np.array(plain.infer({name: want_input})[out_name], copy=True)
    got = ex.infer({name: DetectedRois(frames, rec, min_confidence=0.5)})[out_name]
    assert np.array_equal(ex.requests[0].detected_rois(name).rois, table.rois)
    assert_bit_exact(_fixed(ex, name), want_input, 'BT709 DetectedRois input tensor')
    assert_bit_exact(got, want_out, 'BT709 DetectedRois through infer()')
