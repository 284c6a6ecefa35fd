"""``masks=MaskScreen(space='FRAME')``: instance masks in frame pixels (pvhip_frame_masks_f32).  tests/frame_masks_ref.py is the rule
from its text; pyopenvino_amd/masks.py (make_frame) and the kernel equal it word for word."""
import ctypes
import fractions
import functools

import numpy as np
import pytest

import frame_masks_ref as ref
import test_boxes as boxes_tests
import test_keypoints as keypoints_tests
import test_masks as masks_tests
import test_text as text_tests

LAYOUTS, A = masks_tests.LAYOUTS, masks_tests.A
GUARD, SENTINEL = masks_tests.GUARD, masks_tests.SENTINEL
WIDTHS = (1, 31, 32, 33, 63, 64, 65, 130)
LDS_FLOATS, BAND_ROWS = 8192, 1024                      # PVHIP_FRAME_MASKS_LDS_FLOATS, PVHIP_FRAME_MASKS_BAND_ROWS
GEOMETRIES = {                                          # (net, frame, fit) of a plane (hp, wp)
    'identity': lambda hp, wp: ((2 * hp + 1, 2 * wp), (2 * hp + 1, 2 * wp), (0, 0, 2 * wp, 2 * hp + 1)),
    'letterbox': lambda hp, wp: ((64, 64), (36, 128), (0, 23, 64, 18)),           # a wide frame in a square net: dy > 0
    'smaller': lambda hp, wp: ((hp, wp), (max(hp // 2, 1), max(wp // 2, 1)), (0, 0, wp, hp)),      # taps clamp on all four edges
    'wide': lambda hp, wp: ((36, 132), (40, 140), (3, 0, 126, 36)),               # room for every width: dx > 0
    'rows': lambda hp, wp: ((hp, 132), (10, 140), (0, 0, 132, hp)),               # hp / 10 prototype rows a frame row: short bands
    'single': lambda hp, wp: ((hp, wp), (3, 2 * wp), (0, 0, wp, hp)),             # a rectangle as wide as the frame: a band is one row
}


@functools.lru_cache(maxsize=None)
def _case(T, hp, wp, geometry, layout, counts=(13, 0, 12), heights=(1, 2, 3, 7), widths=WIDTHS):
    """(x, protos, rois, records, net, frame, fit), read-only: test_masks._case's head and planes (a NaN and an inf coefficient, subnormal
    chains, void prototype pixels) under rectangles that walk `widths` and `heights` and touch each frame edge in turn; the last row of
    the first image sticks out of the frame."""
    net, frame, fit = GEOMETRIES[geometry](hp, wp)
    x, protos, images, records, _ = masks_tests._case(T, hp, wp, counts, layout, net=net)
    rng, rois = np.random.default_rng(T + hp), []
    for k, r in enumerate(images):
        w, h = min(widths[k % 8], frame[1]), min(heights[k % len(heights)], frame[0])
        at = [(0, 0), (frame[1] - w, frame[0] - h), (frame[1] - w, 0), (int(rng.integers(0, frame[1] - w + 1)), int(rng.integers(0, frame[0] - h + 1)))][k % 4]
        rois.append((r, frame[1] - w + 1 if k == counts[0] - 1 else at[0], at[1], w, h))
    out = (x, protos, np.asarray(rois, np.int32).reshape(-1, 5), records, net, frame, fit)
    for t in out[:4]:
        t.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _want(T, hp, wp, geometry, layout, max_words=1 << 24, **kw):
    x, protos, rois, records, net, frame, fit = _case(T, hp, wp, geometry, layout, **kw)
    return ref.frame_masks(x, layout, T, protos, rois, records, net, frame, fit, max_words)


def _found(rois, records):
    from pyopenvino_amd import Detections
    return Detections(None, None, rois, None, None, np.asarray(records, np.int32))


@pytest.mark.parametrize('geometry', ['identity', 'letterbox', 'smaller'])
@pytest.mark.parametrize('shape', [(1, 1, 2), (5, 3, 7), (64, 9, 33)])
def test_rule_equals_the_loops(shape, geometry):
    from pyopenvino_amd import BoxScreen, FrameMasks, masks
    T, hp, wp = shape
    for layout in LAYOUTS:
        x, protos, rois, records, net, frame, fit = _case(T, hp, wp, geometry, layout)
        words, offsets, made = _want(T, hp, wp, geometry, layout)
        got = masks.make_frame(x, protos, _found(rois, records), BoxScreen(layout=layout, box=LAYOUTS[layout], tail=T), net, frame, fit)
        assert isinstance(got, FrameMasks) and got.made == made == len(rois) and np.array_equal(got.offsets, offsets) and np.array_equal(got.rois, rois)
        assert got.words.dtype == np.uint32 and np.array_equal(got.words, words), np.flatnonzero(got.words != words)[:4]
        assert offsets[13] == offsets[12] and masks.unpack_frame(got, 12).shape == (rois[12, 4], rois[12, 3])       # the row that sticks out
        for j in range(made):
            bits, anchor = masks.unpack_frame(got, j), records[j] % A
            assert bits.shape == (rois[j, 4], rois[j, 3]) and masks.paste(got, j, frame).sum() == bits.sum() and not (anchor in (3, 4) and bits.any())
            if anchor not in (3, 4) and j != 12 and bits.size >= 64 and hp * wp > 100:     # rectangles over several prototype pixels: no constants
                assert bits.any() and not bits.all(), (layout, j)
        assert hp * wp == 2 or (0 < sum(int(w).bit_count() for w in words) < 32 * len(words) // 2), 'every mask empty, or every mask full'
        assert masks.unpack_frame(got, made) is None


def test_positions_are_exact():
    """Rule 2 against exact rationals, negative N included: the left edge of a letterbox and of an upsampled identity."""
    from pyopenvino_amd import masks
    for d, i, F, P, N in ((0, 64, 128, 33, 64), (3, 126, 140, 33, 132), (0, 7, 30, 7, 7), (23, 18, 36, 9, 64)):
        a, b, f = masks.taps(0, F, d, i, F, P, N)
        for X in (0, 1, 2, F // 2, F - 1):
            q = fractions.Fraction(((2 * d * F + (2 * X + 1) * i) * P - F * N) * 65536, 2 * F * N)
            p = q.numerator // q.denominator
            assert ref.tap(X, d, i, F, P, N) == (a[X], b[X], f[X]) == (min(max(p >> 16, 0), P - 1), min(max((p >> 16) + 1, 0), P - 1), np.float32((p & 65535) / 65536))
        assert ((2 * d * F + i) * P - F * N < 0) == (d == 0)                # (N of column 0)


def test_capacity():
    from pyopenvino_amd import BoxScreen, masks
    x, protos, rois, records, net, frame, fit = _case(5, 3, 7, 'identity', 'NAC')
    offsets, k = _want(5, 3, 7, 'identity', 'NAC')[1], 6
    assert offsets[k - 1] < offsets[k] < offsets[k + 1]
    for max_words, made in ((int(offsets[k]), k), (int(offsets[k]) - 1, k - 1)):
        got = masks.make_frame(x, protos, _found(rois, records), BoxScreen(layout='NAC', box='XYXY', tail=5), net, frame, fit, max_words)
        words = ref.frame_masks(x, 'NAC', 5, protos, rois, records, net, frame, fit, max_words)[0]
        assert got.made == made and len(got.words) == offsets[made] and np.array_equal(got.words, words) and len(got.offsets) == len(rois) + 1
        assert masks.unpack_frame(got, made) is None and masks.unpack_frame(got, made - 1) is not None


def test_refusals_and_the_host_route(tmp_path):
    from pyopenvino_amd import BoxScreen, FrameMasks, MaskScreen, boxes, masks
    n, head = 2, BoxScreen(0.0, frame_size=(56, 84), **masks_tests.HEAD)
    ex, name = masks_tests._seg_net(tmp_path, n, 'oracle.op_plugins')
    x = keypoints_tests._pixels(10, n)
    for match, screen, h in (('space is', MaskScreen(space='NET'), head), ('crop=False is not taken', MaskScreen(crop=False, space='FRAME'), head),
                             ('max_words', MaskScreen(space='FRAME', max_words=0), head), ('max_words', MaskScreen(max_words=(1 << 28) + 1), head),
                             ('max_words', MaskScreen(max_words=True), head), ('max_words', MaskScreen(max_words=1.5), head),
                             ('frames of at most 16384', MaskScreen(space='FRAME'), head._replace(frame_size=(16385, 28)))):
        with pytest.raises(ValueError, match=match) as e:
            ex.infer({name: x}, boxes={'text': h}, masks=screen)
        assert str(e.value).startswith('masks: '), str(e.value)
    h = boxes.resolved(head)._replace(input=name)
    with pytest.raises(ValueError, match='^masks: .*prototypes of at most 4096'):
        masks_tests._checked_with(ex, MaskScreen(space='FRAME'), {'text': h}, dict(dims=(2, 32, 4097, 2)))
    full = ex.infer({name: x})
    found = boxes.decode(full['text'], head, (28, 28))
    for net, frame in (((16385, 28), (56, 84)), ((28, 28), (56, 16385))):
        with pytest.raises(ValueError, match='^masks: .*at most 16384'):
            masks.make_frame(full['text'], full['heatmaps'], found, h, net, frame)
    got = ex.infer({name: x}, boxes={'text': head}, masks=MaskScreen(space='FRAME', max_words=1 << 20))
    want = masks.make_frame(full['text'], full['heatmaps'], found, h, (28, 28), (56, 84), None, 1 << 20)
    boxes_tests._same(got['text'], found)
    assert isinstance(got['heatmaps'], FrameMasks) and got['heatmaps'].made == want.made == len(found.rois) > 0 and want.words.any()
    assert all(np.array_equal(a, b) for a, b in zip(got['heatmaps'][:3], want[:3]))


# ---------------------------------------------------------------------------------------------------------------- the entry
def _device_frame(hip, case, layout, T, counts, max_words, workgroups=0, offset=0, bad=None):
    """The entry behind a hand-written header and rows: (words below used, made); sentinels in front of the words, from `used` on,
    and around header and scratch.  `offset`: the prototypes start that many floats behind a 16-byte boundary; `bad`: {argument:
    value} that the entry refuses, and then nothing is written."""
    from pyopenvino_amd import masks
    x, protos, rois, records, net, frame, fit = case
    n, per, total = len(counts), max(max(counts), 1), len(rois)
    anchors, E = (x.shape[2], x.shape[1]) if layout == 'NCA' else x.shape[1:]
    rows = np.zeros((n * per, 8), np.int32)
    rows[:total, :5], rows[:total, 7] = rois, records
    dev = [hip.DeviceTensor.from_numpy(t) for t in (x, np.concatenate([np.full(offset, 9e9, np.float32), protos.ravel()]),
                                                    np.asarray(list(counts) + [0] * n + [total], np.int32), rows)]
    sizes = (max_words, 2, masks.frame_scratch_bytes(n, per) // 4)
    out = [hip.DeviceTensor.empty((size + 2 * GUARD,), np.int32) for size in sizes]
    for t in out:
        hip.call('pvhip_memset', ctypes.c_void_p(t.ptr), 0x7f, t.nbytes)
    args = [hip.ptr(dev[0]), n, anchors, E, list(LAYOUTS).index(layout), E - T, T, ctypes.c_void_p(dev[1].ptr + 4 * offset), protos.shape[2], protos.shape[3],
            net[0], net[1], frame[0], frame[1], fit[0], fit[1], fit[2], fit[3], per, max_words, workgroups, hip.ptr(dev[2]), hip.ptr(dev[3])] + \
           [ctypes.c_void_p(out[i].ptr + 4 * GUARD) for i in (2, 1, 0)]
    if bad:
        args = [bad.get(i, v) for i, v in enumerate(args)]
        with pytest.raises(hip.PvhipError):
            hip.call('pvhip_frame_masks_f32', *args)
        assert all((np.asarray(t) == SENTINEL).all() for t in out), bad
        return None
    hip.call('pvhip_frame_masks_f32', *args)
    w, header, scratch = (np.asarray(t) for t in out)
    made, used = (int(v) for v in header[GUARD:GUARD + 2])
    assert 0 <= used <= max_words and (w[:GUARD] == SENTINEL).all() and (w[GUARD + used:] == SENTINEL).all(), 'a word outside [0, used) was written'
    assert all((t[:GUARD] == SENTINEL).all() and (t[-GUARD:] == SENTINEL).all() for t in (header, scratch))
    return w[GUARD:GUARD + used].view(np.uint32), made


def _band(case):
    """The band height of the case's tallest rectangle, from the header's constants."""
    x, protos, rois, records, net, frame, fit = case
    j = int(np.argmax(rois[:, 4] * 100000 + rois[:, 3]))               # the widest of the tallest
    first, last = (ref.tap(X, fit[0], fit[2], frame[1], protos.shape[3], net[1]) for X in (int(rois[j, 1]), int(rois[j, 1]) + int(rois[j, 3]) - 1))
    return min(BAND_ROWS, 1 + (LDS_FLOATS // (last[1] - first[0] + 1) - 2) * (frame[0] * net[0]) // (fit[3] * protos.shape[2]))


@pytest.mark.gpu
@pytest.mark.parametrize('T, hp, wp, geometry, heights', [(1, 9, 33, 'wide', (1, 2, 3, 7)), (5, 9, 33, 'wide', (1, 2, 3, 40)), (32, 9, 33, 'letterbox', (1, 2, 3, 7)),
                                                          (64, 9, 33, 'wide', (1, 2, 3, 7)), (5, 300, 33, 'rows', (1, 2, 10)), (1, 2, 4096, 'single', (2, 1, 2))])
def test_kernel_equals_the_rule(hip, T, hp, wp, geometry, heights):
    """Every width around a word and a wave in both forms, heights 1, 2 and -- the last two cases -- one more than a band holds; counts
    (33, 0, 2); both layouts; a grid of 1 and of 3 workgroups against the entry's own; the prototypes one float off; three calls, the
    same words; the capacity cut between two rows; the row outside the frame owns no words."""
    from pyopenvino_amd import masks
    counts = (33, 0, 2)
    assert [hip.call('pvhip_frame_masks_form', w) for w in (0,) + WIDTHS + (16384, 16385)] == [0, 2, 2, 2, 1, 1, 1, 1, 1, 1, 0]
    assert (LDS_FLOATS, BAND_ROWS, 0, 1, 2) == (masks.LDS_FLOATS, masks.BAND_ROWS, masks.FORM_NONE, masks.FORM_ROW, masks.FORM_PAIR)
    for layout in LAYOUTS:
        kw = dict(counts=counts, heights=heights, widths=WIDTHS[:7] + (8192,) if geometry == 'single' else WIDTHS)
        case = _case(T, hp, wp, geometry, layout, **kw)
        words, offsets, made = _want(T, hp, wp, geometry, layout, **kw)
        assert made == 35 and offsets[32] == offsets[33] and words.any() and (geometry not in ('rows', 'single') or case[2][:, 4].max() == _band(case) + 1)
        if geometry == 'single':
            assert _band(case) == 1
        for workgroups, offset in ((0, 0), (1, 1), (3, 0)):
            got, got_made = _device_frame(hip, case, layout, T, counts, len(words) + 5, workgroups, offset)
            assert got_made == made and np.array_equal(got, words), (layout, workgroups, offset, np.flatnonzero(got != words)[:4].tolist())
        cut = int(offsets[20]) - (offsets[19] < offsets[20])
        got, got_made = _device_frame(hip, case, layout, T, counts, cut)
        assert got_made == (19 if offsets[19] < offsets[20] else 20) and np.array_equal(got, words[:len(got)]) and len(got) == offsets[got_made]


@pytest.mark.gpu
def test_entry_rejects_what_it_cannot_do(hip):
    """Each range of the entry's paragraph in pvhip.h from outside: PvhipError, and not a word written; then a good call."""
    case, counts = _case(5, 9, 33, 'wide', 'NAC', counts=(3, 0, 2)), (3, 0, 2)
    words = _want(5, 9, 33, 'wide', 'NAC', counts=(3, 0, 2))[0]
    bads = [{i: None} for i in (0, 7, 21, 22, 23, 24, 25)] + [{1: 0}, {2: 0}, {3: 4}, {4: 2}, {5: 3}, {6: 0}, {6: 65}, {8: 0}, {8: 4097}, {9: 4097}, {8: 1, 9: 1}]
    bads += [{i: v} for i in (10, 11, 12, 13, 16, 17) for v in (0, 16385)] + [{i: v} for i in (14, 15) for v in (-1, 16385)]
    bads += [{18: 0}, {18: 4097}, {1: 4097, 18: 4096}, {19: 0}, {19: (1 << 28) + 1}, {20: -1}, {20: 65536}]
    for bad in bads:
        _device_frame(hip, case, 'NAC', 5, counts, len(words), bad=bad)
    got, made = _device_frame(hip, case, 'NAC', 5, counts, len(words))
    assert made == 5 and np.array_equal(got, words)


@pytest.mark.gpu
def test_public_path(hip, tmp_path):
    """boxes= + masks=MaskScreen(space='FRAME') equal make_frame on the request's own full Results; the pass replays its recording; the
    copies are the head's two, the 8-byte header and 4 * used bytes.  (The letterbox is covered at the entry: _seg_net's input declares no fit.)"""
    from pyopenvino_amd import BoxScreen, FrameMasks, MaskScreen, boxes, masks
    n = 3
    ex, name = masks_tests._seg_net(tmp_path, n)
    req, xd = ex.requests[0], hip.DeviceTensor.from_numpy(keypoints_tests._pixels(10, n))
    req.infer({name: xd})
    full = {k: np.array(v, copy=True) for k, v in req.infer({name: xd}).items()}      # (the next pass replays)
    head = BoxScreen(float(np.quantile(full['text'][:, :, 4:644].max(axis=2), 0.5)), max_per_image=20, frame_size=(56, 84), **masks_tests.HEAD)
    found = boxes.decode(full['text'], head, (28, 28))
    screen = MaskScreen(space='FRAME', max_words=1 << 16)
    want = masks.make_frame(full['text'], full['heatmaps'], found, head, (28, 28), (56, 84), None, 1 << 16)
    assert 0 < want.made == len(found.rois) and want.words.any()
    req.infer({name: xd}, boxes={'text': head}, masks=screen)
    real_call, copied = hip.call, []
    hip.call = lambda entry, *args: (copied.append(args[2]) if entry == 'pvhip_memcpy_d2h' else None, real_call(entry, *args))[1]
    try:
        req.start_async({name: xd}, boxes={'text': head}, masks=screen)
        replayed = req._replayed is not None
        got = req.wait()
    finally:
        hip.call = real_call
    boxes_tests._same(got['text'], found)
    assert isinstance(got['heatmaps'], FrameMasks) and got['heatmaps'].made == want.made and all(np.array_equal(a, b) for a, b in zip(got['heatmaps'][:3], want[:3]))
    assert replayed and sorted(copied) == sorted([4 * (2 * n + 1), 32 * len(found.rois), 8, 4 * len(want.words)]), copied
    for k in full:
        assert np.array_equal(text_tests._on_device(hip, req, k), full[k])
