"""Letterbox: ``preprocess_info.resize_fit`` 'LETTERBOX' / 'TOP_LEFT' -- a host input scaled by one factor into the Parameter's extent and
padded, on the device in the launch that converts it (pvhip_input_preprocess_fit_f32 / _yuv_fit_f32 / _packed_fit_f32), bit for bit
tests/letterbox_ref.py -- and a fitted detector's boxes mapped back to the frame (pvhip_detections_compact_fit, pvhip_detections_to_rois_fit,
``infer(..., detections=)``, ``DetectedRois``), word for word the same module.  The first tests need no GPU."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import detections_ref
import helpers
import letterbox_ref
import packed_ref
import test_detected_rois as det_tests
import test_detections as compact_tests
import test_roi_input as roi_tests
import yuv_ref
from detected_rois_ref import detected_rois
from helpers import MODELS, assert_bit_exact
from preprocess_ref import preprocess

NAN, INF = np.nan, np.inf
_rec, END, ZERO = det_tests._rec, det_tests.END, det_tests.ZERO
FITS = {'LETTERBOX': 1, 'TOP_LEFT': 2}
ENTRIES = ('pvhip_input_preprocess_fit_f32', 'pvhip_input_preprocess_yuv_fit_f32', 'pvhip_input_preprocess_packed_fit_f32')
RULE_ENTRIES = ('pvhip_detections_compact_fit', 'pvhip_detections_to_rois_fit')
SSD_FIT = (300, 300, 0, 65, 300, 169)                         # a (1080, 1920) frame in the SSD's 300 x 300


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
def test_geometry_examples_and_invariants():
    from pyopenvino_amd import input_format
    assert letterbox_ref.geometry((1080, 1920), (300, 300), 'LETTERBOX') == (0, 65, 300, 169)
    assert letterbox_ref.geometry((31, 9), (20, 24), 'LETTERBOX') == (9, 0, 6, 20)
    assert letterbox_ref.geometry((1, 64), (20, 24), 'LETTERBOX') == (0, 9, 24, 1)
    assert letterbox_ref.geometry((1080, 1920), (300, 300), 'TOP_LEFT') == (0, 0, 300, 169)
    destinations = [(20, 24), (19, 23), (1, 1), (1, 7), (300, 300), (224, 3)]
    sources = list(itertools.product(range(1, 40), range(1, 40))) + [(1080, 1920), (1, 2 ** 24), (2 ** 24, 1), (2 ** 24, 2 ** 24 - 1)]
    for (hd, wd), (hs, ws) in itertools.product(destinations, sources):
        dx, dy, iw, ih = g = letterbox_ref.geometry((hs, ws), (hd, wd), 'LETTERBOX')
        assert input_format.fit_geometry((hs, ws), (hd, wd), 'LETTERBOX') == g                       # the product's own form
        assert input_format.fit_geometry((hs, ws), (hd, wd), 'TOP_LEFT') == (0, 0, iw, ih) == letterbox_ref.geometry((hs, ws), (hd, wd), 'TOP_LEFT')
        assert input_format.fit_geometry((hs, ws), (hd, wd), 'STRETCH') == (0, 0, wd, hd)
        assert 1 <= iw <= wd and 1 <= ih <= hd and (iw == wd or ih == hd), ((hs, ws), (hd, wd), g)
        assert (dx, dy) == ((wd - iw) // 2, (hd - ih) // 2) and dx + iw <= wd and dy + ih <= hd
        if hs * wd == ws * hd:
            assert g == (0, 0, wd, hd)
        # the short side is the exact quotient rounded half up, unless the clamp to 1 took it
        if ws * hd >= hs * wd:
            assert iw == wd and (ih == 1 or abs(2 * ih * ws - 2 * hs * wd) <= ws)
        else:
            assert ih == hd and (iw == 1 or abs(2 * iw * hs - 2 * ws * hd) <= hs)


def _brute(x, dst_hw, fit, pad, reverse, mean, std):
    """fit_images pixel by pixel in scalars: x is (n, h, w, c) uint8 or float32."""
    n, hs, ws, c = x.shape
    hd, wd = dst_hw
    dx, dy, iw, ih = letterbox_ref.geometry((hs, ws), dst_hw, fit)
    out = np.empty((n, c, hd, wd), np.float32)
    one = np.float32(1)

    def tap(d, S, D):
        num = max((2 * d + 1) * S - D, 0)
        i0 = min(num // (2 * D), S - 1)
        f = np.float32(0) if i0 == S - 1 else np.float32(num - i0 * 2 * D) / np.float32(2 * D)
        return i0, min(i0 + 1, S - 1), f

    for b, k, y, xx in itertools.product(range(n), range(c), range(hd), range(wd)):
        sc = c - 1 - k if reverse else k
        if dy <= y < dy + ih and dx <= xx < dx + iw:
            if (hs, ws) == (ih, iw):
                v = np.float32(x[b, y - dy, xx - dx, sc])
            else:
                y0, y1, fy = tap(y - dy, hs, ih)
                x0, x1, fx = tap(xx - dx, ws, iw)
                p = lambda r, q: np.float32(x[b, r, q, sc])                                           # noqa: E731
                top = (one - fx) * p(y0, x0) + fx * p(y0, x1)
                bot = (one - fx) * p(y1, x0) + fx * p(y1, x1)
                v = (one - fy) * top + fy * bot
        else:
            v = np.float32(pad)
        if mean is not None:
            v = v - np.float32(mean[k])
        if std is not None:
            v = v / np.float32(std[k])
        out[b, k, y, xx] = v
    return out


def test_restatement_against_a_per_pixel_loop():
    rng = np.random.default_rng(5)
    mean, std = [104.0, 117.0, 123.0], [1.0, 57.5, 2.0]
    for src_hw, dst_hw in (((3, 9), (6, 7)), ((9, 3), (6, 7)), ((3, 7), (6, 7)), ((6, 7), (6, 7)), ((1, 1), (5, 4)), ((1, 11), (5, 4)), ((11, 1), (5, 4))):
        for fit, pad, opt in (('LETTERBOX', 0.0, (False, None, None)), ('TOP_LEFT', 114.0, (True, mean, std)), ('LETTERBOX', 114.0, (True, mean, None))):
            for x in (rng.integers(0, 256, (2,) + src_hw + (3,), dtype=np.uint8), rng.uniform(-300, 300, (2,) + src_hw + (3,)).astype(np.float32)):
                got = letterbox_ref.fit_images(x, dst_hw, fit, pad, True, opt[0], opt[1], opt[2])
                assert_bit_exact(got, _brute(x, dst_hw, fit, pad, *opt), '{} -> {} {} {}'.format(src_hw, dst_hw, fit, pad))
                nchw = np.ascontiguousarray(x.transpose(0, 3, 1, 2))
                assert_bit_exact(letterbox_ref.fit_images(nchw, dst_hw, fit, pad, False, opt[0], opt[1], opt[2]), got, 'NCHW')
    # a geometry that fills the destination is the existing rule; a table's rows are the crops; an invalid row is NaN
    x = rng.integers(0, 256, (2, 10, 12, 3), dtype=np.uint8)
    assert_bit_exact(letterbox_ref.fit_images(x, (20, 24), 'LETTERBOX', 114.0), preprocess(x, (20, 24)), 'fills')
    rois = [(1, 2, 3, 7, 2), (0, 0, 0, 12, 10), (2, 0, 0, 1, 1), (0, 11, 0, 2, 1)]
    got = letterbox_ref.fit_rois(x, rois, (6, 7), 'LETTERBOX', 9.0, mean=mean)
    assert_bit_exact(got[0], letterbox_ref.fit_images(x[1:2, 3:5, 2:9], (6, 7), 'LETTERBOX', 9.0, mean=mean)[0], 'row 0')
    assert np.isnan(got[2]).all() and np.isnan(got[3]).all() and np.isfinite(got[:2]).all()
    nv12 = yuv_ref.frames_of(*yuv_ref.planes_from_bgr(rng.integers(0, 256, (2, 10, 12, 3), dtype=np.uint8)), 'NV12')
    assert_bit_exact(letterbox_ref.fit_frames(nv12, (7, 6), 'TOP_LEFT', 1.0, color='NV12'),
                     letterbox_ref.fit_images(yuv_ref.to_bgr(nv12, 'NV12'), (7, 6), 'TOP_LEFT', 1.0), 'NV12')


def test_declaration_rules():
    ie, net, name = roi_tests._net(batch=2)
    info = net.input_info[name]
    pre = info.preprocess_info
    assert pre.resize_fit == 'STRETCH' and pre.pad_value == 0.0
    fmt = info.frozen()
    assert fmt.fit == 'STRETCH' and fmt.pad == 0.0 and not fmt.fitted and fmt.fit_geometry((1080, 1920)) == (0, 0, 224, 224)
    for bad in ('letter', 1, None, 'RESIZE_BILINEAR'):
        with pytest.raises(ValueError, match='resize_fit'):
            pre.resize_fit = bad
    for bad in (NAN, INF, -INF, 1e39, '114', True, None):
        with pytest.raises(ValueError, match='pad_value'):
            pre.pad_value = bad
    assert pre.resize_fit == 'STRETCH' and pre.pad_value == 0.0 and not info.declared
    pre.resize_fit = 'letterbox'
    pre.pad_value = 114
    assert pre.resize_fit == 'LETTERBOX' and pre.pad_value == 114.0 and info.declared
    with pytest.raises(ValueError, match='resize_fit LETTERBOX .*RESIZE_BILINEAR'):     # a fit without a resize
        ie.load_network(net)
    pre.resize_algorithm = 'RESIZE_BILINEAR'
    info.precision, info.layout = 'U8', 'NHWC'
    fmt = info.frozen()
    assert fmt.fitted and fmt.fit == 'LETTERBOX' and fmt.fit_code == 1 and fmt.pad == 114.0
    assert fmt.fit_geometry((1080, 1920)) == letterbox_ref.geometry((1080, 1920), (224, 224), 'LETTERBOX') == (0, 49, 224, 126)
    assert fmt.needs_preprocess((1080, 1920)) and fmt.needs_preprocess((224, 100)) and not fmt.needs_preprocess((224, 224))
    pre.resize_fit = 'TOP_LEFT'
    assert info.frozen().fit_code == 2 and info.frozen().fit_geometry((1080, 1920)) == (0, 0, 224, 126)
    ex = ie.load_network(net)
    assert ex.host_inputs.formats[name].fit == 'TOP_LEFT' and ex.host_inputs.formats[name].pad == 114.0
    with pytest.raises(ValueError, match='between read_network and load_network'):
        pre.resize_fit = 'LETTERBOX'
    with pytest.raises(ValueError, match='between read_network and load_network'):
        pre.pad_value = 0.0
    # existing constructors hold: the fields trail and default
    from pyopenvino_amd.input_format import InputFormat
    old = InputFormat(name, (2, 3, 224, 224), True, True, True, True, True, False, None, None, 'NV12')
    assert old.fit == 'STRETCH' and old.pad == 0.0 and not old.fitted


def _by_hand(rec, images, frame, fit, conf=0.5, min_size=(1, 1)):
    """The fitted rule as a float32 loop written out: [(image, x0, y0, w, h, record)]."""
    Hn, Wn, dx, dy, iw, ih = fit
    H, W = frame
    f = np.float32
    P, out = rec.shape[0] // images, []
    for b in range(images):
        for p in range(P):
            q = rec[b * P + p]
            if not q[0] >= 0:
                break
            if not q[2] >= f(conf) or not all(np.isfinite(v) for v in q[3:7]):
                continue
            with np.errstate(over='ignore'):
                u = [(q[3] * f(Wn) - f(dx)) / f(iw), (q[4] * f(Hn) - f(dy)) / f(ih), (q[5] * f(Wn) - f(dx)) / f(iw), (q[6] * f(Hn) - f(dy)) / f(ih)]
                x0 = int(np.floor(min(max(u[0] * f(W), f(0)), f(W))))
                y0 = int(np.floor(min(max(u[1] * f(H), f(0)), f(H))))
                x1 = int(np.ceil(min(max(u[2] * f(W), f(0)), f(W))))
                y1 = int(np.ceil(min(max(u[3] * f(H), f(0)), f(H))))
            if x1 - x0 >= min_size[1] and y1 - y0 >= min_size[0]:
                out.append((b, x0, y0, x1 - x0, y1 - y0, b * P + p))
    return out


def _hand_records():
    """Two images of eight records over a (1080, 1920) frame letterboxed into 300 x 300 (rows 65..234 hold the frame)."""
    image0 = [_rec(0, 1, 0.9, 0.25, 0.5, 0.5, 0.75),          # inside the frame
              _rec(1, 2, 0.8, 0.1, 0.01, 0.9, 0.2),           # wholly in the padding above: extent 0, dropped
              _rec(2, 3, 0.8, 0.1, 0.1, 0.9, 0.5),            # straddles the upper bar: clamped to row 0
              _rec(3, 3, 0.7, 0.0, 0.7, 1.0, 1.0),            # straddles the lower bar
              _rec(4, 1, 0.9, NAN, 0.3, 0.5, 0.6),            # a NaN corner
              _rec(5, 1, 0.9, 0.2, 0.3, INF, 0.6),            # an infinite corner
              _rec(6, 1, 0.9, 0.2, -INF, 0.5, 0.6),
              _rec(7, 4, 0.5, -0.5, -0.5, 1.5, 1.5)]          # larger than the input: the whole frame
    image1 = [_rec(0, 1, 0.6, 0.3, 65 / 300, 0.6, 234 / 300),  # on the inner edges
              _rec(1, 1, 0.6, 0.3, 0.9, 0.6, 0.95),           # wholly in the padding below
              _rec(2, 5, 3e38, 3e38, 0.3, 3e38, 0.6),         # finite corners whose product overflows: clamps to the right edge, no width
              END, ZERO,
              _rec(5, 1, 0.99, 0.1, 0.3, 0.9, 0.6),           # behind the terminator
              ZERO, ZERO]
    return np.array(image0 + image1, np.float32)


def test_compact_records_with_a_fit_against_a_hand_written_loop():
    from pyopenvino_amd import DetectionScreen, detections
    rec, frame = _hand_records(), (1080, 1920)
    for opt in (dict(), dict(min_confidence=0.65), dict(min_size=(300, 1)), dict(max_per_image=2)):
        screen = DetectionScreen(frame_size=frame, **opt)
        got = detections.compact_records(rec, 2, screen, fit=SSD_FIT)
        want = _by_hand(rec, 2, frame, SSD_FIT, opt.get('min_confidence', 0.5), opt.get('min_size', (1, 1)))
        cap = opt.get('max_per_image', 8)
        kept = [r for r in want if sum(1 for o in want if o[0] == r[0] and o[5] < r[5]) < cap]
        assert [tuple(r) + (k,) for r, k in zip(got.rois.tolist(), got.records.tolist())] == kept, opt
        assert got.selected.tolist() == [sum(1 for r in want if r[0] == b) for b in range(2)]
        compact_tests._same(got, letterbox_ref.compact_fit(rec, 2, frame, SSD_FIT, **opt), str(opt))
    plain = detections.compact_records(rec, 2, DetectionScreen(frame_size=frame), fit=SSD_FIT)
    assert plain.records.tolist() == [0, 2, 3, 7, 8]           # in the padding, bad corners, no width, behind the terminator: gone
    assert plain.rois.tolist()[1] == [0, 192, 0, 1536, 544] and plain.rois.tolist()[3] == [0, 0, 0, 1920, 1080]
    assert plain.rois.tolist()[4] == [1, 576, 0, 576, 1080]
    # without a fit nothing changed, and a full-extent fit maps nothing
    screen = DetectionScreen(frame_size=(300, 300))
    old = detections.compact_records(rec, 2, screen)
    compact_tests._same(old, detections_ref.compact(rec, 2, (300, 300)), 'no fit')
    compact_tests._same(detections.compact_records(rec, 2, screen, fit=None), detections_ref.compact(rec, 2, (300, 300)), 'fit=None')
    compact_tests._equal(letterbox_ref.compact_fit(rec, 2, (300, 300), None), detections_ref.compact(rec, 2, (300, 300)), 'the restatement without a fit')
    for bad in ((300, 300, 0, 65, 300), (300, 300, 0, 65, 300, 236), (300, 300, -1, 65, 300, 169), (300, 300, 0, 65, 0, 169), (300.0, 300, 0, 65, 300, 169),
                (2 ** 24 + 1, 300, 0, 65, 300, 169), 7, 'fit'):
        with pytest.raises(ValueError, match='detections: '):
            detections.compact_records(rec, 2, screen, fit=bad)


def _ssd(fit='LETTERBOX', pad=114.0, batch=2, requests=1, load=True):
    """SSD-MobileNet as tests/test_detections.py builds it -- U8 / NHWC frames, reversed channels -- with a resize and `fit`."""
    from pyopenvino_amd import synth
    blob = synth.synth_weights(os.path.join(MODELS, 'ssd_mobilenet_v1_coco.xml'), 1234)
    ie, net, name = roi_tests._net('ssd_mobilenet_v1_coco', batch, blob)
    roi_tests._declare(net, name, 'U8-NHWC', reverse=True)
    if fit is not None:
        net.input_info[name].preprocess_info.resize_fit = fit
        net.input_info[name].preprocess_info.pad_value = pad
    return (ie.load_network(net, 'GPU', num_requests=requests) if load else net), name, net.outputs[0]['name']


def test_refused_combinations_raise_before_any_device_call():
    from pyopenvino_amd import DetectedRois, RoiInput, TiledScreen
    ex, name, out_name = _ssd()
    frames = np.zeros((1, 90, 160, 3), np.uint8)
    table = np.array([[0, 0, 0, 160, 90]] * 2, np.int32)
    with pytest.raises(ValueError, match='detections: .*resize_fit LETTERBOX.*RoiInput'):
        ex.infer({name: RoiInput(frames, table)}, detections=0.5)
    with pytest.raises(ValueError, match='detections: .*resize_fit LETTERBOX.*DetectedRois'):
        ex.requests[0].start_async({name: DetectedRois(frames, np.zeros((4, 7), np.float32))}, detections={out_name: 0.5})
    with pytest.raises(ValueError, match='detections: .*TiledScreen.*resize_fit LETTERBOX'):
        ex.infer({name: RoiInput(frames, table)}, detections=TiledScreen(0.5))
    assert not ex.host_inputs.slots and not ex.answers.blocks                      # nothing was staged or allocated
    with pytest.raises(ValueError, match='detector_fit'):
        from pyopenvino_amd import detections
        detections.checked_fit((300, 300, 0, 65, 300, 300), 'input x: detector_fit')


def test_abi_declares_the_fit_entries():
    from pyopenvino_amd import device
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for entry, count in zip(ENTRIES + RULE_ENTRIES, (19, 17, 17, 19, 20)):
        assert entry in device.SIGNATURES and len(device.SIGNATURES[entry][1]) == count and entry not in device._NOT_STATUS
        m = re.search(r'\b' + entry + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S)
        assert m and len(m.group(1).split(',')) == count, entry
        comment = re.search(r'/\*((?:(?!\*/).)*)\*/\s*(?:int\s+pvhip_\w+\s*\([^;]*;\s*)*int\s+' + entry + r'\b', header, flags=re.S).group(1)
        assert 'Addition to ABI v18 (the version number is unchanged' in comment, entry
    assert re.search(r'#define\s+PVHIP_ABI_VERSION\s+19\b', header)
    lib = device.load_library()
    assert all(hasattr(lib, e) for e in ENTRIES + RULE_ENTRIES) and lib.pvhip_abi_version() == 19


# ---------------------------------------------------------------------------------------------------------------- GPU
FORMATS = ['U8-NHWC', 'FP32-NCHW', 'NV12', 'I420', 'YUY2', 'BGRX']
DESTINATIONS = [(20, 24), (19, 23)]                            # 16-byte stores; scalar stores
# bars above and below (dy = 6); bars left and right (dx = 9 or 8: quads straddle); fills the destination; one pixel; inner extent 1 both ways
SOURCES = {'any': [(9, 31), (31, 9), (10, 12), (1, 1), (1, 64), (64, 1)],
           'even': [(10, 32), (32, 10), (10, 12), (2, 2), (2, 64), (64, 2)],             # NV12 / I420
           'even width': [(9, 32), (31, 10), (10, 12), (1, 2), (1, 64), (64, 2)]}        # YUY2


def _sources(fmt):
    return SOURCES['even' if fmt in ('NV12', 'I420') else 'even width' if fmt == 'YUY2' else 'any']


def _make_frames(rng, fmt, m, hw, c=3):
    h, w = hw
    if fmt == 'U8-NHWC':
        return rng.integers(0, 256, (m, h, w, c), dtype=np.uint8)
    if fmt == 'FP32-NCHW':
        return rng.uniform(-300, 300, (m, c, h, w)).astype(np.float32)
    bgr = rng.integers(0, 256, (m, h, w, 3), dtype=np.uint8)
    if fmt in ('NV12', 'I420'):
        return yuv_ref.frames_of(*yuv_ref.planes_from_bgr(bgr), fmt)
    return packed_ref.frames_from_bgr(bgr, fmt)


def _ref_opts(fmt):
    return dict(nhwc=fmt != 'FP32-NCHW', color='RAW' if fmt in ('U8-NHWC', 'FP32-NCHW') else fmt)


def _options(rng, c=3):
    mean = rng.uniform(0, 255, c).astype(np.float32)
    std = rng.uniform(0.5, 80, c).astype(np.float32)
    return [dict(), dict(reverse_channels=True, mean=mean, std_scale=std)]


def _device_fit(hip, fmt, frames, dst_hw, fit, pad, rois=None, largest=None, entry_of=None, reverse_channels=False, mean=None, std_scale=None):
    """The fitted entry of `fmt` on `frames` (`rois`: an (n, 5) table, else whole images) into a destination prefilled with 0x7f bytes;
    entry_of: run the EXISTING entry of the format instead (whole images only)."""
    frames = np.ascontiguousarray(frames)
    m = frames.shape[0]
    if fmt == 'U8-NHWC':
        (h, w, c), how = frames.shape[1:], (1, 1)
    elif fmt == 'FP32-NCHW':
        (c, h, w), how = frames.shape[1:], (0, 0)
    elif fmt in ('NV12', 'I420'):
        (h, w, c), how = (frames.shape[1] // 3 * 2, frames.shape[2], 3), (int(fmt == 'I420'),)
    else:
        (h, w, c), how = frames.shape[1:3] + (3,), (packed_ref.KINDS[fmt],)
    src = hip.DeviceTensor.from_numpy(frames)
    table = hip.DeviceTensor.from_numpy(np.ascontiguousarray(rois, np.int32)) if rois is not None else None
    n = m if rois is None else len(rois)
    dst = hip.DeviceTensor.empty((n, c) + tuple(dst_hw))
    hip.call('pvhip_memset', ctypes.c_void_p(dst.ptr), 0x7f, dst.nbytes)
    mt = hip.DeviceTensor.from_numpy(np.asarray(mean, np.float32)) if mean is not None else None
    st = hip.DeviceTensor.from_numpy(np.asarray(std_scale, np.float32)) if std_scale is not None else None
    pre = (int(reverse_channels), ctypes.c_void_p(mt.ptr) if mt is not None else None, ctypes.c_void_p(st.ptr) if st is not None else None)
    raw = fmt in ('U8-NHWC', 'FP32-NCHW')
    if entry_of is not None:
        assert rois is None
        hip.call(entry_of, ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), n, *((c,) if raw else ()), h, w, *dst_hw, *how, *pre)
        return np.asarray(dst)
    entry = ENTRIES[0] if raw else ENTRIES[1] if fmt in ('NV12', 'I420') else ENTRIES[2]
    largest = largest if largest is not None else ((h, w) if rois is None else (int(np.asarray(rois)[:, 4].max()), int(np.asarray(rois)[:, 3].max())))
    hip.call(entry, ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), ctypes.c_void_p(table.ptr) if table is not None else None, n, m,
             *((c,) if raw else ()), h, w, *dst_hw, *largest, *how, *pre, FITS[fit], float(pad))
    return np.asarray(dst)


EXISTING = {'U8-NHWC': 'pvhip_input_preprocess_f32', 'FP32-NCHW': 'pvhip_input_preprocess_f32', 'NV12': 'pvhip_input_preprocess_yuv_f32',
            'I420': 'pvhip_input_preprocess_yuv_f32', 'YUY2': 'pvhip_input_preprocess_packed_f32', 'BGRX': 'pvhip_input_preprocess_packed_f32'}


@pytest.mark.gpu
@pytest.mark.parametrize('dst_hw', DESTINATIONS)
@pytest.mark.parametrize('fmt', FORMATS)
def test_fit_kernels_bit_exact(hip, fmt, dst_hw):
    """Every source shape, with and without reversal and mean / scale, both fits, pad 0 and 114, at n = 2."""
    rng = np.random.default_rng(FORMATS.index(fmt) * 101 + dst_hw[0])
    options = _options(rng)
    seen = set()
    for src_hw in _sources(fmt):
        frames = _make_frames(rng, fmt, 2, src_hw)
        for opt, fit, pad in itertools.product(options, FITS, (0.0, 114.0)):
            what = '{} {} -> {} {} pad {} {}'.format(fmt, src_hw, dst_hw, fit, pad, sorted(opt))
            want = letterbox_ref.fit_frames(frames, dst_hw, fit, pad, **_ref_opts(fmt), **opt)
            got = _device_fit(hip, fmt, frames, dst_hw, fit, pad, **opt)
            assert_bit_exact(got, want, what)
            dx, dy, iw, ih = letterbox_ref.geometry(src_hw, dst_hw, fit)
            seen.add((dx > 0, dy > 0, (iw, ih) == dst_hw[::-1], min(iw, ih) == 1))
            if (iw, ih) == dst_hw[::-1]:                       # fills the destination: the existing entry's bits as well
                assert_bit_exact(got, _device_fit(hip, fmt, frames, dst_hw, fit, pad, entry_of=EXISTING[fmt], **opt), what + ' vs the existing entry')
    assert {s[0] for s in seen} == {s[1] for s in seen} == {s[2] for s in seen} == {s[3] for s in seen} == {True, False}


@pytest.mark.gpu
@pytest.mark.parametrize('c', [1, 3])
def test_fit_kernel_when_a_row_exceeds_the_lds_budget(hip, c):
    """fp32 NCHW (4, 70000): one source row is 280 KB, so the output rows split into column tiles, and (c = 1: one-row tiles) tiles lie
    wholly in the padding; the inner rectangle is one row high."""
    rng = np.random.default_rng(70000 + c)
    frames = _make_frames(rng, 'FP32-NCHW', 2, (4, 70000), c)
    options = _options(rng, c)
    for dst_hw, fit, pad, opt in (((20, 24), 'LETTERBOX', 114.0, options[1]), ((19, 23), 'LETTERBOX', 0.0, options[0]), ((20, 24), 'TOP_LEFT', 114.0, options[0])):
        assert letterbox_ref.geometry((4, 70000), dst_hw, fit)[2:] == (dst_hw[1], 1)
        want = letterbox_ref.fit_frames(frames, dst_hw, fit, pad, nhwc=False, **opt)
        assert_bit_exact(_device_fit(hip, 'FP32-NCHW', frames, dst_hw, fit, pad, **opt), want, '{} {} {}'.format(dst_hw, fit, pad))


@pytest.mark.gpu
@pytest.mark.parametrize('fmt, src_hw', [('NV12', (4, 70000)), ('I420', (4, 70000)), ('YUY2', (3, 70000)), ('BGRX', (3, 20000))])
def test_fit_kernel_of_colour_frames_when_a_row_exceeds_the_lds_budget(hip, fmt, src_hw):
    """The colour sources on the same path: one source row (70 KB of luma with its chroma, 140 KB of YUY2 groups, 80 KB of four-byte
    pixels) is over the LDS budget, so the output rows split into column tiles, most of them wholly in the padding; the inner rectangle
    is one row high."""
    rng = np.random.default_rng(70000 + FORMATS.index(fmt))
    frames = _make_frames(rng, fmt, 2, src_hw)
    options = _options(rng)
    for dst_hw, fit, pad, opt in (((20, 24), 'LETTERBOX', 114.0, options[1]), ((19, 23), 'TOP_LEFT', 0.0, options[0])):
        assert letterbox_ref.geometry(src_hw, dst_hw, fit)[2:] == (dst_hw[1], 1)
        want = letterbox_ref.fit_frames(frames, dst_hw, fit, pad, **_ref_opts(fmt), **opt)
        assert_bit_exact(_device_fit(hip, fmt, frames, dst_hw, fit, pad, **opt), want, '{} {} {} {}'.format(fmt, dst_hw, fit, pad))


def _roi_table(dst_hw):
    """Over frames of (40, 48): wide; tall; exactly its own fitted (ih, iw); 1 x 48; 40 x 1; invalid (a frame that is not there)."""
    hd, wd = dst_hw
    exact = (0, 1, 2, wd, 10)
    assert letterbox_ref.geometry((10, wd), dst_hw, 'LETTERBOX')[2:] == (wd, 10)
    return np.array([(0, 2, 3, 40, 10), (1, 5, 0, 9, 31), exact, (1, 0, 7, 48, 1), (0, 47, 0, 1, 40), (2, 0, 0, 5, 5)], np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize('dst_hw', DESTINATIONS)
@pytest.mark.parametrize('fmt', FORMATS)
def test_fit_kernels_bit_exact_on_a_table(hip, fmt, dst_hw):
    """m = 2 frames of (40, 48), n = 6 rectangles, the launch sized by the table's maxima; the invalid row is NaN, padding included."""
    rng = np.random.default_rng(FORMATS.index(fmt) * 7 + dst_hw[1])
    frames = _make_frames(rng, fmt, 2, (40, 48))
    table = _roi_table(dst_hw)
    if fmt == 'FP32-NCHW':                                     # an inf inside the copied rectangle stays one pixel: copied, not interpolated
        frames[0, :, 5, 9] = INF
    for opt, fit, pad in itertools.product(_options(rng), FITS, (0.0, 114.0)):
        what = '{} -> {} {} pad {} {}'.format(fmt, dst_hw, fit, pad, sorted(opt))
        want = letterbox_ref.fit_rois(frames, table, dst_hw, fit, pad, **_ref_opts(fmt), **opt)
        got = _device_fit(hip, fmt, frames, dst_hw, fit, pad, rois=table, **opt)
        assert_bit_exact(got, want, what)
        assert np.isnan(got[5]).all() and not np.isnan(got[:5]).any(), what
        assert np.isinf(got[2]).sum() == (3 if fmt == 'FP32-NCHW' else 0)
    # sized for whole frames, as a DetectedRois launch is: the same bits
    want = letterbox_ref.fit_rois(frames, table, dst_hw, 'LETTERBOX', 114.0, **_ref_opts(fmt))
    assert_bit_exact(_device_fit(hip, fmt, frames, dst_hw, 'LETTERBOX', 114.0, rois=table, largest=(40, 48)), want, 'sized for the frame')
    # a rectangle above the maxima the launch was sized for is NaN too
    got = _device_fit(hip, fmt, frames, dst_hw, 'LETTERBOX', 114.0, rois=table, largest=(31, 40))
    assert np.isnan(got[[3, 4, 5]]).all() and not np.isnan(got[:3]).any()
    assert_bit_exact(got[:3], want[:3], 'rows within the maxima')


@pytest.mark.gpu
def test_fit_entries_reject_what_they_cannot_do(hip):
    s, d = hip.DeviceTensor.empty((1 << 12,), np.float32), hip.DeviceTensor.empty((1 << 12,), np.float32)
    s, d = ctypes.c_void_p(s.ptr), ctypes.c_void_p(d.ptr)
    # positions: (src_h, m, max_roi_h, max_roi_w); fit and pad_value are the last two
    cases = {ENTRIES[0]: ([s, d, None, 2, 2, 3, 10, 12, 20, 24, 10, 12, 1, 1, 0, None, None, 1, 114.0], (6, 4, 10, 11)),
             ENTRIES[1]: ([s, d, None, 2, 2, 10, 12, 20, 24, 10, 12, 0, 0, None, None, 2, 0.0], (5, 4, 9, 10)),
             ENTRIES[2]: ([s, d, None, 2, 2, 10, 12, 20, 24, 10, 12, 0, 0, None, None, 1, 0.0], (5, 4, 9, 10))}
    for entry, (args, (src_h, m, max_h, max_w)) in cases.items():
        hip.call(entry, *args)
        k = len(args)
        for at, bad in ((k - 2, 0), (k - 2, 3), (k - 2, -1), (k - 1, NAN), (k - 1, INF), (0, None), (1, None), (3, 0), (src_h, 0)):
            wrong = list(args)
            wrong[at] = bad
            with pytest.raises(hip.PvhipError):
                hip.call(entry, *wrong)
        with_table = list(args)
        with_table[2] = s                                      # a table: m and the maxima count
        for at, bad in ((m, 0), (max_h, 11), (max_h, 0), (max_w, 13), (max_w, 0)):
            wrong = list(with_table)
            wrong[at] = bad
            with pytest.raises(hip.PvhipError):
                hip.call(entry, *wrong)
    hip.synchronize()


def _device_compact_fit(hip, rec, images, extent, fit, min_confidence=0.5, labels=None, min_size=(1, 1), max_per_image=None):
    """pvhip_detections_compact_fit on `rec` as a Compacted; header and rows prefilled with 0x7f bytes, rows >= total untouched."""
    per_image = rec.reshape(-1, 7).shape[0] // images
    cap = per_image if max_per_image is None else max_per_image
    capacity = images * min(per_image, cap)
    src = hip.DeviceTensor.from_numpy(rec)
    header = hip.DeviceTensor.empty((2 * images + 1 + 8,), np.int32)
    rows = hip.DeviceTensor.empty((capacity + 1, 8), np.int32)
    for t in (header, rows):
        hip.call('pvhip_memset', ctypes.c_void_p(t.ptr), 0x7f, t.nbytes)
    lab = hip.DeviceTensor.from_numpy(np.asarray(list(labels) + [0], np.int32)) if labels is not None else None
    hip.call(RULE_ENTRIES[0], ctypes.c_void_p(src.ptr), images, per_image, extent[0], extent[1], min_confidence,
             ctypes.c_void_p(lab.ptr) if lab is not None else None, 0 if labels is None else len(labels), min_size[0], min_size[1], cap,
             ctypes.c_void_p(header.ptr), ctypes.c_void_p(rows.ptr), *fit)
    header, rows = np.asarray(header), np.asarray(rows).view(np.uint32)
    assert (header[2 * images + 1:] == compact_tests.SENTINEL).all()
    counts, selected, total = header[:images].copy(), header[images:2 * images].copy(), int(header[2 * images])
    assert 0 <= total <= capacity and total == counts.sum() and (rows[total:] == compact_tests.SENTINEL).all()
    return detections_ref.Compacted(counts, selected, rows[:total].copy())


def _device_table_fit(hip, rec, n, images, extent, fit, min_confidence=0.5, labels=None, min_size=(1, 1)):
    """pvhip_detections_to_rois_fit on `rec` as a Detected; every output prefilled with 0x7f bytes, with a guard row behind it."""
    per_image = rec.reshape(-1, 7).shape[0] // images
    src = hip.DeviceTensor.from_numpy(rec)
    outs = [hip.DeviceTensor.empty((rows + 1, cols), np.int32) for rows, cols in ((n, 5), (n, 1), (2, 1))]
    for t in outs:
        hip.call('pvhip_memset', ctypes.c_void_p(t.ptr), 0x7f, t.nbytes)
    lab = hip.DeviceTensor.from_numpy(np.asarray(list(labels) + [0], np.int32)) if labels is not None else None
    hip.call(RULE_ENTRIES[1], *(ctypes.c_void_p(t.ptr) for t in [src] + outs), n, images, per_image, extent[0], extent[1], min_confidence,
             ctypes.c_void_p(lab.ptr) if lab is not None else None, 0 if labels is None else len(labels), min_size[0], min_size[1], *fit)
    rois, record_of, counts = (np.asarray(t) for t in outs)
    assert (rois[n] == 0x7f7f7f7f).all() and record_of[n, 0] == 0x7f7f7f7f and counts[2, 0] == 0x7f7f7f7f
    return det_tests.detected_rois_ref.Detected(int(counts[0, 0]), int(counts[1, 0]), rois[:n].copy(), record_of[:n, 0].copy())


@pytest.mark.gpu
def test_rule_entries_equal_the_rule(hip):
    """2 images x 70 records (more than one wave step) with every special case injected, and the hand-written records, mapped back through
    (300, 300, 0, 65, 300, 169) over a (1080, 1920) frame; the same records through the entries without the fit still match the old rule."""
    rng = np.random.default_rng(169)
    frame = (1080, 1920)
    for rec, images in ((det_tests._random_records(rng, 2, 70), 2), (det_tests._random_records(rng, 2, 70, long=True), 2), (_hand_records(), 2)):
        P = rec.shape[0] // images
        assert letterbox_ref.compact_fit(rec, images, frame, SSD_FIT, min_confidence=-1.0).selected.sum() >= 3
        for opt in (dict(), dict(min_confidence=-1.0), dict(max_per_image=2), dict(labels=[1, 3], min_confidence=0.25), dict(min_size=(200, 300)), dict(labels=[])):
            _same = compact_tests._equal
            _same(_device_compact_fit(hip, rec, images, frame, SSD_FIT, **opt), letterbox_ref.compact_fit(rec, images, frame, SSD_FIT, **opt), 'fit {}'.format(opt))
            _same(compact_tests._device_compact(hip, rec, images, frame, **opt), detections_ref.compact(rec, images, frame, **opt), 'no fit {}'.format(opt))
            if 'max_per_image' in opt:
                continue
            for n in (1, 5, 2 * P):
                det_tests._same(_device_table_fit(hip, rec, n, images, frame, SSD_FIT, **opt),
                                letterbox_ref.detected_rois_fit(rec, n, images, frame, SSD_FIT, **opt), 'table fit {} n = {}'.format(opt, n))
                det_tests._same(det_tests._device_table(hip, rec, n, images, frame, **opt), detected_rois(rec, n, images, frame, **opt),
                                'table no fit {} n = {}'.format(opt, n))
        # other geometries: bars left and right; top-left; a fit that fills the input maps nothing
        for fit in ((300, 300, 66, 0, 169, 300), (300, 300, 0, 0, 300, 169), (20, 24, 9, 0, 6, 20)):
            compact_tests._equal(_device_compact_fit(hip, rec, images, (1920, 1080), fit, min_confidence=0.1),
                                 letterbox_ref.compact_fit(rec, images, (1920, 1080), fit, min_confidence=0.1), str(fit))
        compact_tests._equal(_device_compact_fit(hip, rec, images, frame, (300, 300, 0, 0, 300, 300)),
                             letterbox_ref.compact_fit(rec, images, frame, (300, 300, 0, 0, 300, 300)), 'full')
    # what the entries refuse
    t = hip.DeviceTensor.empty((256,), np.int32)
    p, h = ctypes.c_void_p(t.ptr), ctypes.c_void_p(t.ptr + 512)
    good = [p, 2, 2, 1080, 1920, 0.5, None, 0, 1, 1, 2, h, p] + list(SSD_FIT)
    hip.call(RULE_ENTRIES[0], *good)
    rois_good = [p, p, p, p, 4, 1, 2, 1080, 1920, 0.5, None, 0, 1, 1] + list(SSD_FIT)
    hip.call(RULE_ENTRIES[1], *rois_good)
    for entry, args in ((RULE_ENTRIES[0], good), (RULE_ENTRIES[1], rois_good)):
        k = len(args) - 6
        for at, bad in ((k, 0), (k, (1 << 24) + 1), (k + 1, 0), (k + 2, -1), (k + 2, 1), (k + 3, 132), (k + 4, 0), (k + 5, 0), (k + 5, 236)):
            wrong = list(args)
            wrong[at] = bad
            with pytest.raises(hip.PvhipError):
                hip.call(entry, *wrong)
    hip.synchronize()


@pytest.mark.gpu
def test_public_path_on_a_letterboxed_ssd(hip):
    """SSD-MobileNet at batch 2, U8 / NHWC + RESIZE_BILINEAR + LETTERBOX, frames of (90, 160): the Parameter tensor is the restatement,
    detections= is the numpy rule on the whole Result with the pass's geometry, a classifier fed DetectedRois(frames, the detector's
    request) gets the table of the numpy rule, and the same network without the fit passes what it passes today."""
    from pyopenvino_amd import DetectedRois, Detections, DetectionScreen, detections, synth
    rng = np.random.default_rng(160)
    m, hw, pad = 2, (90, 160), 114.0
    frames = rng.integers(0, 256, (m,) + hw + (3,), dtype=np.uint8)
    det, name, out_name = _ssd('LETTERBOX', pad)
    req = det.requests[0]
    geometry = (300, 300) + letterbox_ref.geometry(hw, (300, 300), 'LETTERBOX')
    assert geometry == (300, 300, 0, 65, 300, 169)
    full = np.array(req.infer({name: frames})[out_name], copy=True)
    assert full.shape == (1, 1, 200, 7)
    assert_bit_exact(roi_tests._fixed(det, name), letterbox_ref.fit_images(frames, (300, 300), 'LETTERBOX', pad, reverse_channels=True), 'the Parameter tensor')
    median = compact_tests._median_live_score(full, m)
    for conf in (0.5, median):
        screen = DetectionScreen(conf, frame_size=hw)
        want = detections.compact_records(full, m, screen, fit=geometry)
        got = req.infer({name: frames}, detections=conf)[out_name]
        assert isinstance(got, Detections)
        compact_tests._same(got, detections_ref.as_words(want), 'conf {}'.format(conf))
        compact_tests._same(got, letterbox_ref.compact_fit(full, m, hw, geometry, min_confidence=conf), 'the restatement, conf {}'.format(conf))
    assert got.counts.sum() >= 1 and (got.rois[:, 1] + got.rois[:, 3] <= hw[1]).all() and (got.rois[:, 2] + got.rois[:, 4] <= hw[0]).all()
    # an explicit frame_size is honoured (the boxes in pixels of a larger original), through the network's own infer() as well
    big = (1080, 1920)
    got = det.infer({name: frames}, detections=DetectionScreen(median, frame_size=big, max_per_image=3))[out_name]
    compact_tests._same(got, letterbox_ref.compact_fit(full, m, big, geometry, min_confidence=median, max_per_image=3), 'explicit frame_size')
    # other frames, another geometry (bars left and right), the same request
    tall = rng.integers(0, 256, (m, 120, 50, 3), dtype=np.uint8)
    full_tall = np.array(req.infer({name: tall})[out_name], copy=True)
    g_tall = (300, 300) + letterbox_ref.geometry((120, 50), (300, 300), 'LETTERBOX')
    assert g_tall == (300, 300, 87, 0, 125, 300)
    assert_bit_exact(roi_tests._fixed(det, name), letterbox_ref.fit_images(tall, (300, 300), 'LETTERBOX', pad, reverse_channels=True), 'tall frames')
    conf_tall = compact_tests._median_live_score(full_tall, m)
    compact_tests._same(req.infer({name: tall}, detections=conf_tall)[out_name],
                        letterbox_ref.compact_fit(full_tall, m, (120, 50), g_tall, min_confidence=conf_tall), 'tall frames')
    assert len(det.answers.blocks) == len({0.5, median, conf_tall}) + 1          # one per screen (and the capped one), none per frame extent
    # the cascade: the detector in flight on the wide frames, the classifier on DetectedRois(frames, its request)
    blob = synth.synth_weights(os.path.join(MODELS, 'googlenet-v1.xml'), 11)
    n = 8
    ex, cls_name, cls_out = det_tests._classifier('U8-NHWC', n, blob)
    want = letterbox_ref.detected_rois_fit(full, n, m, hw, geometry, min_confidence=median)
    assert want.count >= 1
    req.start_async({name: frames})
    cls = ex.requests[0]
    cls.start_async({cls_name: DetectedRois(frames, req, min_confidence=median)})
    cls.wait()
    assert_bit_exact(req.wait()[out_name], full, 'the detector again')
    det_tests._same(cls.detected_rois(cls_name), want, 'the cascade in flight')
    cls.infer({cls_name: DetectedRois(frames, req, min_confidence=median)})              # waited for: its host Results
    det_tests._same(cls.detected_rois(cls_name), want, 'the cascade, detector waited for')
    cls.infer({cls_name: DetectedRois(frames, full, min_confidence=median, detector_fit=geometry)})
    det_tests._same(cls.detected_rois(cls_name), want, 'records as an array with detector_fit')
    cls.infer({cls_name: DetectedRois(frames, full, min_confidence=median)})
    det_tests._same(cls.detected_rois(cls_name), detected_rois(full, n, m, hw, min_confidence=median), 'records as an array without it')
    # the same network without the fit: the stretch, and the rule over the declared extent
    plain, _, _ = _ssd(None)
    preq = plain.requests[0]
    full_plain = np.array(preq.infer({name: frames})[out_name], copy=True)
    assert_bit_exact(roi_tests._fixed(plain, name), preprocess(frames, (300, 300), reverse_channels=True), 'the stretch')
    conf_plain = compact_tests._median_live_score(full_plain, m)
    compact_tests._same(preq.infer({name: frames}, detections=conf_plain)[out_name], detections_ref.compact(full_plain, m, (300, 300), min_confidence=conf_plain),
                        'without the fit')
    det.release_device_state()
    plain.release_device_state()
    ex.release_device_state()


@pytest.mark.gpu
def test_public_path_of_a_fitted_classifier(hip):
    """GoogLeNet at batch 4 on NV12 frames with RESIZE_BILINEAR + TOP_LEFT and mean / scale: an array, the request's own input_buffer, a
    RoiInput and a DetectedRois all leave the restatement in the Parameter tensor."""
    from pyopenvino_amd import DetectedRois, RoiInput
    rng = np.random.default_rng(224)
    n, hw, pad = 4, (48, 80), 114.0
    mean = roi_tests._mean()
    ie, net, name = roi_tests._net('googlenet-v1', n)
    roi_tests._declare(net, name, 'NV12', mean=mean)
    net.input_info[name].preprocess_info.resize_fit = 'TOP_LEFT'
    net.input_info[name].preprocess_info.pad_value = pad
    ex = ie.load_network(net, 'GPU')
    req = ex.requests[0]
    pre = dict(mean=mean[0], std_scale=mean[1])
    frames = roi_tests._frames(rng, 'NV12', n, hw)
    want = letterbox_ref.fit_frames(frames, (224, 224), 'TOP_LEFT', pad, color='NV12', **pre)
    assert letterbox_ref.geometry(hw, (224, 224), 'TOP_LEFT') == (0, 0, 224, 134)
    req.infer({name: frames})
    assert_bit_exact(roi_tests._fixed(ex, name), want, 'an array')
    buf = req.input_buffer(name, hw)
    buf[...] = frames[::-1]
    req.infer({name: buf})
    assert_bit_exact(roi_tests._fixed(ex, name), want[::-1], 'the request\'s own buffer')
    table = np.array([(0, 3, 5, 60, 20), (1, 7, 1, 11, 45), (3, 0, 0, 80, 48), (2, 79, 47, 1, 1)], np.int32)
    req.infer({name: RoiInput(frames, table)})
    assert_bit_exact(roi_tests._fixed(ex, name), letterbox_ref.fit_rois(frames, table, (224, 224), 'TOP_LEFT', pad, color='NV12', **pre), 'a RoiInput')
    rec = det_tests._random_records(rng, n, 10, long=True)
    rule = detected_rois(rec, n, n, hw, min_confidence=0.3)
    assert 1 <= rule.count
    req.infer({name: DetectedRois(frames, rec, min_confidence=0.3)})
    det_tests._same(req.detected_rois(name), rule, 'the table')
    fixed = roi_tests._fixed(ex, name)
    assert_bit_exact(fixed[:rule.count], letterbox_ref.fit_rois(frames, rule.rois[:rule.count], (224, 224), 'TOP_LEFT', pad, color='NV12', **pre), 'a DetectedRois')
    assert np.isnan(fixed[rule.count:]).all()
    ex.release_device_state()
