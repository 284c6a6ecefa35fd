"""Projective warps as a network input (pyopenvino_amd.PerspectiveInput): batch row b is frame ids[b] of m frames sampled through the
3 x 3 homography matrices[b] on the device in one launch (pvhip_input_preprocess_perspective_f32), bit for bit tests/perspective_ref.py.
The reference has no such operation, so the restatement is first checked against facts that do not depend on it; those tests need no
GPU.  The frames, kinds and declarations are those of test_warp_input.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import colorimetry_ref as cref
import helpers
import perspective_ref as pref
import test_warp_input as wt
import warp_ref
from helpers import MODELS, assert_bit_exact

KINDS = wt.KINDS
ENTRY = 'pvhip_input_preprocess_perspective_f32'
ENTRY_COLOR = 'pvhip_input_preprocess_perspective_color_f32'
FRAMES = [(14, 18), (34, 70)]                                 # both legal for every format
DESTS = [(37, 45), (32, 64)]                                  # partial tiles and partial quads; whole ones, aligned
MEAN, STD = wt.MEAN, wt.STD
OPTIONS = [dict(pad=0.0), dict(reverse=True, mean=MEAN, std=STD, pad=114.0)]
IDENTITY = np.eye(3)
KEYSTONE = np.array([[1, 0, 0], [0, 1, 0], [1 / 8, 0, 1]], np.float64)       # D = x / 8 + 1
HORIZON = np.array([[1, 0, 0], [0, 1, 0], [-1 / 8, 0, 1]], np.float64)       # D = 1 - x / 8: zero in column 8, negative behind it


def _ref(kind, frames, table, dst_hw, **opt):
    color, _, nhwc = wt._is(kind)
    return pref.warp(frames, table, dst_hw, nhwc, opt.get('reverse', False), opt.get('mean'), opt.get('std'), opt.get('pad', 0.0), color)


def _affine_in_q16(rng, n, linear=3.0, shift=40.0):
    """n affine 2 x 3 matrices whose entries are multiples of 2^-16."""
    a = np.concatenate([rng.uniform(-linear, linear, (n, 2, 2)), rng.uniform(-shift, shift, (n, 2, 1))], 2)
    return np.rint(a * 65536.0) / 65536.0


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
def test_restatement_affine_positions_are_the_affine_forms():
    """Rows [[A], [0, 0, 1]] with entries that are multiples of 2^-16 below 2^20: TX is A00 x + A01 y + C0 in Q16 exactly."""
    from pyopenvino_amd import perspective
    rng = np.random.default_rng(1)
    dst = (37, 45)
    y, x = (g.astype(np.int64) for g in np.mgrid[0:dst[0], 0:dst[1]])
    for _ in range(200):
        q = rng.integers(-(1 << 36) + 1, 1 << 36, (2, 3))     # Q16 of values below 2^20
        row = pref.fixed([perspective.from_affine(q / 65536.0)], dst)[0]
        sx, sy, ok = pref.positions(row, dst)
        assert ok.all()
        assert np.array_equal(sx, q[0, 0] * x + q[0, 1] * y + q[0, 2]) and np.array_equal(sy, q[1, 0] * x + q[1, 1] * y + q[1, 2])


@pytest.mark.parametrize('kind', KINDS)
def test_restatement_affine_rows_equal_the_affine_restatement(kind):
    """... and the image is warp_ref's bit for bit: the two restatements share no code."""
    from pyopenvino_amd import perspective
    rng = np.random.default_rng(13 + len(kind))
    hw, m, dst = (14, 18), 3, (37, 45)
    frames = wt._frames(rng, kind, m, hw, special=True)
    A = _affine_in_q16(rng, 4)
    A[1] = [[1, 0, 3], [0, 1, 2]]
    ids = [2, 0, 1, 1]
    H = np.stack([perspective.from_affine(a) for a in A], 0)
    for opt in OPTIONS:
        want = wt._ref(kind, frames, warp_ref.table_of(A, ids), dst, **opt)
        got = _ref(kind, frames, pref.table_of(H, ids, dst), dst, **opt)
        assert_bit_exact(got, want, '{} {}'.format(kind, sorted(opt)))


@pytest.mark.parametrize('kind', KINDS)
def test_restatement_keystone_horizon_and_negation_facts(kind):
    rng = np.random.default_rng(29 + len(kind))
    hw, dst = (34, 70), (37, 45)
    frames = wt._frames(rng, kind, 2, hw, special=True)
    img = wt._image(kind, frames)
    img = img if kind.startswith('FP32') else img.astype(np.float32)
    # D = 2 in column 8 and both numerators even there for even y: output (y, 8) is src[y / 2, 4], copied
    got = _ref(kind, frames, pref.table_of([KEYSTONE], [1], dst), dst)[0]
    rows = np.arange(0, dst[0], 2)
    assert_bit_exact(got[:, rows, 8], img[1, rows // 2, 4].T, kind + ' keystone column 8')
    # the horizon: column 8 has D == 0 and is the pad in every row and channel; no other column is refused
    sx, sy, ok = pref.positions(pref.fixed([HORIZON], dst)[0], dst)
    assert not ok[:, 8].any() and ok[:, :8].all() and ok[:, 9:].all()
    mean, std, pad = np.float32(MEAN), np.float32(STD), 114.0
    got = _ref(kind, frames, pref.table_of([HORIZON], [0], dst), dst, mean=mean, std=std, pad=pad)[0]
    for k in range(3):
        assert (got[k, :, 8] == (np.float32(pad) - mean[k]) / std[k]).all()
    assert (got[:, :, [0, 4]] != got[:, :, [8]]).any()        # (the columns beside it are sampled: D = 1 and 1/2)
    # -identity is the identity: a copy where the frame covers the extent
    got = _ref(kind, frames, pref.table_of([-IDENTITY], [1], (30, 41)), (30, 41))[0]
    assert_bit_exact(got, img[1, :30, :41].transpose(2, 0, 1), kind + ' -identity')
    assert (pref.fixed([-IDENTITY], dst) == -pref.fixed([IDENTITY], dst)).all()


def test_fixed_scale_ties_and_refusals():
    from pyopenvino_amd import PerspectiveInput, perspective
    q = PerspectiveInput.fixed([IDENTITY], (37, 45))
    assert q.dtype == np.int64 and q.shape == (1, 9) and q.flags.c_contiguous
    # B = 44 in [2^5, 2^6): e = 6, the scale 2^45
    assert q[0].tolist() == [1 << 45, 0, 0, 0, 1 << 45, 0, 0, 0, 1 << 45]
    # B = 223 h00 + ... of a power of two exactly: B in [2^(e-1), 2^e) puts 2^k at e = k + 1
    assert PerspectiveInput.fixed([[[0, 0, 4], [0, 0, 0], [0, 0, 1]]], (5, 5))[0].tolist() == [0, 0, 1 << 50, 0, 0, 0, 0, 0, 1 << 48]
    # an extent of one pixel: B = max |h_r2| = 1, e = 1, the scale 2^50; halves go to the even neighbour on both sides of zero
    u = 2.0 ** -50
    ties = np.array([[[0.5 * u, 1.5 * u, 1.0], [2.5 * u, -0.5 * u, -1.5 * u], [-2.5 * u, 3.5 * u, 0.25]]])
    assert PerspectiveInput.fixed(ties, (1, 1))[0].tolist() == [0, 2, 1 << 50, 2, 0, -2, -2, 4, 1 << 48]
    rng = np.random.default_rng(2)
    M = rng.uniform(-3, 3, (40, 3, 3)) * 10.0 ** rng.integers(-12, 12, (40, 1, 1))
    M[:4] = [perspective.from_quad([[100.25, 50.5], [900.75, 80.125], [870.5, 600.25], [60.0, 640.75]], d) for d in ((224, 224), (37, 45), (2, 2), (1080, 1920))]
    for dst in ((224, 224), (37, 45), (1, 1), (1, 9), (1080, 1920)):
        q = PerspectiveInput.fixed(M, dst)
        assert np.array_equal(q, pref.fixed(M, dst)) and pref.within_limit(q, dst) and not PerspectiveInput.beyond_limits(q, dst).any()
        hd, wd = dst
        forms = np.abs(q.astype(object)).reshape(-1, 3, 3) @ np.array([wd - 1, hd - 1, 1], object)
        assert (forms.max(1) >= 1 << 50).all() and (forms.max(1) <= 1 << 52).all()          # the scale uses the room it has
    for given in (M.astype(np.float32)[:1], np.rint(M[:1]).astype(np.int32), M[:1].tolist()):
        assert PerspectiveInput.fixed(given, (37, 45)).tolist() == pref.fixed(np.asarray(given, np.float64), (37, 45)).tolist()
    assert PerspectiveInput.fixed(np.zeros((0, 3, 3)), (4, 4)).shape == (0, 9)
    for bad in (np.nan, np.inf, -np.inf):
        rows = np.stack([IDENTITY] * 3, 0)
        rows[1, 2, 0] = bad
        with pytest.raises(ValueError, match=r'matrices\[1\]'):
            PerspectiveInput.fixed(rows, (37, 45))
        with pytest.raises(ValueError, match=r'matrices\[1\]'):
            pref.fixed(rows, (37, 45))
    rows = np.stack([IDENTITY, np.zeros((3, 3)), IDENTITY], 0)
    with pytest.raises(ValueError, match=r'matrices\[1\]'):
        PerspectiveInput.fixed(rows, (37, 45))
    with pytest.raises(ValueError, match=r'matrices\[1\]'):
        pref.fixed(rows, (37, 45))
    for shape in ((3, 3), (1, 2, 3), (1, 3, 4), (9,), (1, 1, 3, 3)):
        with pytest.raises(ValueError, match='shape'):
            PerspectiveInput.fixed(np.zeros(shape), (4, 4))
    for dtype in (bool, complex, object, 'U3'):
        with pytest.raises(ValueError, match='real numbers'):
            PerspectiveInput.fixed(np.zeros((1, 3, 3), dtype), (4, 4))
    # the limit of a table as such: 2^52 itself is inside
    edge = np.array([[1 << 40, 1 << 40, (1 << 52) - (44 + 36) * (1 << 40), 0, 0, -(1 << 52), 0, 0, 1 << 52]], np.int64)
    assert not PerspectiveInput.beyond_limits(edge, (37, 45)).any()
    for column, step in ((2, 1), (5, -1), (6, 1), (1, -(1 << 50))):
        over = edge.copy()
        over[0, column] += step
        assert PerspectiveInput.beyond_limits(over, (37, 45)).all(), column
    assert PerspectiveInput.beyond_limits(np.full((1, 9), np.iinfo(np.int64).min), (1, 1)).all()


def test_positions_stay_within_the_derived_distance_of_the_unquantised_map():
    """A from_quad homography of a 1920 x 1080 frame onto 224 x 224 with fractional corners.  Each Q is within half a unit
    u = 2^-(51-e) of its h, so each form over pixel (x, y) is within E u with E = (x + y + 1) / 2, the quotient therefore within
    E u (1 + |sx|) / (|d| - E u) of sx, and the floor adds one Q16 step: the bound is derived, not measured.  The unquantised map is
    evaluated in extended precision, so its own rounding plays no part."""
    from pyopenvino_amd import PerspectiveInput, perspective
    dst = (224, 224)
    H = perspective.from_quad([[412.3, 215.7], [1507.9, 305.2], [1633.4, 873.6], [301.8, 951.1]], dst)
    q = PerspectiveInput.fixed([H], dst)[0]
    u = np.longdouble(2.0) ** -(51 - pref.scale_exponent(H, dst))
    sx, sy, ok = pref.positions(q, dst)
    assert ok.all()
    y, x = (g.astype(np.longdouble) for g in np.mgrid[0:dst[0], 0:dst[1]])
    h = H.astype(np.longdouble)
    d = h[2, 0] * x + h[2, 1] * y + h[2, 2]
    E = (x + y + 1) / 2
    assert (np.abs(d) > E * u).all()
    for got, row in ((sx, h[0]), (sy, h[1])):
        s = (row[0] * x + row[1] * y + row[2]) / d
        err = np.abs(got.astype(np.longdouble) / 65536 - s)
        bound = E * u * (1 + np.abs(s)) / (np.abs(d) - E * u) + np.longdouble(2.0) ** -16
        worst = np.unravel_index(np.argmax(err - bound), err.shape)
        print('worst pixel {}: error {:.3e}, bound {:.3e}'.format(worst, float(err[worst]), float(bound[worst])))
        assert (err <= bound).all()
    assert sx.min() >> 16 >= 290 and sx.max() >> 16 <= 1640 and sy.min() >> 16 >= 210 and sy.max() >> 16 <= 955


def test_matrix_helpers():
    from pyopenvino_amd import perspective, warp
    rng = np.random.default_rng(5)
    for dst in ((224, 224), (37, 45), (2, 3)):
        hd, wd = dst
        out = [[0, 0], [wd - 1, 0], [wd - 1, hd - 1], [0, hd - 1]]
        for corners in ([[100.25, 50.5], [900.75, 80.125], [870.5, 600.25], [60.0, 640.75]], [[5, 5], [20, 5], [20, 15], [5, 15]],
                        [[900.0, 80.0], [100.0, 50.0], [60.0, 640.0], [870.0, 600.0]]):               # (the last one mirrored)
            H = perspective.from_quad(corners, dst)
            assert H.dtype == np.float64 and H.shape == (3, 3) and H[2, 2] == 1.0
            assert np.allclose(perspective.apply(H, out), corners, rtol=1e-9, atol=0)
    # an upright rectangle is the affine map of its corners
    assert np.allclose(perspective.from_quad([[5, 7], [5 + 2 * 44, 7], [5 + 2 * 44, 7 + 3 * 36], [5, 7 + 3 * 36]], (37, 45)),
                       [[2, 0, 5], [0, 3, 7], [0, 0, 1]], atol=1e-12)
    for bad in ([[0, 0], [1, 1], [2, 2], [0, 5]], [[3, 3]] * 4, [[0, 0], [np.nan, 0], [4, 4], [0, 4]], [[0, 0], [4, 0], [4, 0], [0, 0]]):
        with pytest.raises(ValueError, match='degenerate'):
            perspective.from_quad(bad, (8, 8))
    with pytest.raises(ValueError, match='degenerate'):
        perspective.from_quad([[0, 0], [4, 0], [4, 4], [0, 4]], (1, 8))
    with pytest.raises(ValueError, match='four'):
        perspective.from_quad(np.zeros((3, 2)), (8, 8))
    for _ in range(20):
        H = perspective.from_quad(np.array([[100, 50], [900, 80], [870, 600], [60, 640]]) + rng.uniform(-30, 30, (4, 2)), (224, 224))
        pts = rng.uniform(0, 223, (7, 2))
        assert np.allclose(perspective.apply(perspective.invert(H), perspective.apply(H, pts)), pts, rtol=1e-9, atol=1e-7)
        back = perspective.invert(perspective.invert(H))
        assert back.dtype == np.float64 and np.allclose(back / back[2, 2], H, rtol=1e-9, atol=1e-9)
        A = rng.uniform(-3, 3, (2, 3))
        assert np.array_equal(perspective.from_affine(A)[:2], A) and perspective.from_affine(A)[2].tolist() == [0, 0, 1]
        assert np.array_equal(perspective.apply(perspective.from_affine(A), pts), warp.apply(A, pts))
    assert perspective.apply(IDENTITY, np.zeros((4, 5, 2))).shape == (4, 5, 2)
    got = perspective.apply(HORIZON, [[8, 3], [4, 3], [16, 3]])
    assert np.isnan(got[0]).all() and got[1].tolist() == [8, 6] and got[2].tolist() == [-16, -3]
    for singular in (np.zeros((3, 3)), [[1, 2, 0], [2, 4, 0], [0, 0, 1]], [[np.nan, 0, 0], [0, 1, 0], [0, 0, 1]], [[np.inf, 0, 0], [0, 1, 0], [0, 0, 1]]):
        with pytest.raises(ValueError, match='singular'):
            perspective.invert(singular)
    for bad in (np.eye(2, 3), np.zeros(9), np.zeros((1, 3, 3))):
        with pytest.raises(ValueError, match='3 x 3'):
            perspective.invert(bad)
        with pytest.raises(ValueError, match='3 x 3'):
            perspective.apply(bad, [[0, 0]])
    with pytest.raises(ValueError, match='2 x 3'):
        perspective.from_affine(np.eye(3))


@pytest.mark.parametrize('kind', ['U8-NHWC', 'FP32-NCHW', 'NV12', 'YUY2'])
def test_perspective_input_argument_rules(kind):
    """The table the format makes of matrices and ids, and every refusal -- by the format and by infer() with one text, before anything
    is allocated."""
    from pyopenvino_amd import PerspectiveInput
    n, hw, dst, IDS = 4, (48, 64), (224, 224), wt.IDS
    ie, net, name = wt._net(batch=n)
    wt._declare(net, name, kind)
    fmt = net.input_info[name].frozen()
    ex = ie.load_network(net)
    rng = np.random.default_rng(3)
    M = rng.uniform(-2, 2, (n, 3, 3))
    t = fmt.checked_matrices(PerspectiveInput, M, IDS, 3)
    assert t.dtype == np.int64 and t.shape == (n, 10) and t.flags.c_contiguous
    assert t[:, 0].tolist() == IDS and np.array_equal(t[:, 1:], PerspectiveInput.fixed(M, dst)) and np.array_equal(t, pref.table_of(M, IDS, dst))
    assert fmt.checked_matrices(PerspectiveInput, M, None, n)[:, 0].tolist() == [0, 1, 2, 3]
    assert fmt.checked_matrices(PerspectiveInput, M.tolist(), None, 1)[:, 0].tolist() == [0, 0, 0, 0]
    dtype = fmt.host_dtype

    def refused(match, matrices, ids, m):
        frames = np.zeros(wt._frame_shape(kind, m, hw), dtype)
        with pytest.raises(ValueError, match=match) as by_format:
            fmt.checked_matrices(PerspectiveInput, matrices, ids, m)
        with pytest.raises(ValueError) as by_infer:
            ex.infer({name: PerspectiveInput(frames, matrices, ids)})
        assert str(by_format.value) == str(by_infer.value) and str(by_infer.value).startswith('input {}: '.format(name))

    refused('without ids', M, None, 3)
    refused(r'ids\[\d\] = .* none of 3 frames', M, [0, 1, 2, 3], 3)
    refused('ids holds 4 integers', M, [0.0, 1.0, 2.0, 0.0], 3)
    refused(r'one 3 x 3 matrix per batch row', M[:3], [0, 0, 0], 3)
    refused(r'shape \(n, 3, 3\)', M[0], IDS, 3)
    refused(r'shape \(n, 3, 3\)', M[:, :2], IDS, 3)              # an affine (n, 2, 3) is none: perspective.from_affine makes one
    refused('real numbers', M > 0, IDS, 3)
    bad = M.copy()
    bad[2, 1, 1] = np.nan
    refused(r'matrices\[2\] is no homography', bad, IDS, 3)
    bad[2] = 0
    refused(r'matrices\[2\] is no homography', bad, IDS, 3)
    assert not ex.host_inputs.slots                           # nothing was allocated
    # a table already in the device's form (the perspective_buffer): the limit over the network's extent, and the ids
    assert fmt.checked_matrix_table(PerspectiveInput, t, 3) is t
    for column, value, match in ((1, 1 << 52, r'matrices\[2\] is beyond the limit'), (9, -(1 << 52) - 1, r'matrices\[2\]'),
                                 (5, np.iinfo(np.int64).min, r'matrices\[2\]'), (0, 3, r'ids\[2\] = 3'), (0, -1, r'ids\[2\] = -1')):
        over = t.copy()
        over[2, column] = value
        with pytest.raises(ValueError, match='^input {}: {}'.format(name, match)):
            fmt.checked_matrix_table(PerspectiveInput, over, 3)
    ok = np.zeros(wt._frame_shape(kind, 3, hw), dtype)
    for shape in (ok.shape[1:], (0,) + ok.shape[1:]):
        with pytest.raises(ValueError, match='frames of a PerspectiveInput') as by_infer:
            ex.infer({name: PerspectiveInput(np.zeros(shape, dtype), M, IDS)})
        with pytest.raises(ValueError) as by_format:
            fmt.frames_extent_of(np.zeros(shape, dtype), PerspectiveInput)
        assert str(by_format.value) == str(by_infer.value)
    with pytest.raises(KeyError):
        ex.infer({'no such input': PerspectiveInput(ok, M, IDS)})
    with pytest.raises(KeyError):
        ex.requests[0].perspective_buffer('no such input')
    assert not ex.host_inputs.slots
    assert repr(PerspectiveInput(ok, M)) == 'PerspectiveInput(frames={}, matrices=(4, 3, 3))'.format(ok.shape)
    assert PerspectiveInput.__slots__ == ('frames', 'matrices', 'ids')


@pytest.mark.parametrize('kind', ['U8-NHWC', 'NV12', None])
def test_perspective_input_needs_a_declared_resize(kind):
    from pyopenvino_amd import PerspectiveInput
    n, hw = 2, (224, 224)
    ie, net, name = wt._net(batch=n)
    if kind is not None:
        wt._declare(net, name, kind, resize=False)
    fmt = net.input_info[name].frozen()
    ex = ie.load_network(net)
    frames = np.zeros(wt._frame_shape(kind or 'FP32-NCHW', 1, hw), fmt.host_dtype)
    M = np.stack([IDENTITY] * n, 0)
    with pytest.raises(ValueError, match='a PerspectiveInput is sampled on the device.*resize_algorithm') as by_infer:
        ex.infer({name: PerspectiveInput(frames, M)})
    for refused in (lambda: fmt.checked_matrices(PerspectiveInput, M, None, 1), lambda: fmt.resize_declared(PerspectiveInput),
                    lambda: ex.requests[0].perspective_buffer(name), lambda: fmt.checked_matrix_table(PerspectiveInput, np.zeros((n, 10), np.int64), 1)):
        with pytest.raises(ValueError) as by_format:
            refused()
        assert str(by_format.value) == str(by_infer.value)
    assert not ex.host_inputs.slots


def test_perspective_input_is_refused_where_a_warp_input_is():
    """detections= on a fitted input fed a PerspectiveInput is refused like a WarpInput there; a TiledScreen and a RegionScreen go on
    refusing anything but what they took; all before anything is staged."""
    from pyopenvino_amd import IECore, PerspectiveInput, RegionScreen, TiledScreen, synth
    blob = synth.synth_weights(os.path.join(MODELS, 'ssd_mobilenet_v1_coco.xml'), 1234)
    for fit in (None, 'LETTERBOX'):
        ie = IECore(plugin_package=wt.HIP)
        net = ie.read_network(os.path.join(MODELS, 'ssd_mobilenet_v1_coco.xml'), weights=blob)
        net.set_batch(2)
        name = net.inputs[0]['name']
        wt._declare(net, name, 'U8-NHWC', reverse=True, fit=fit)
        ex = ie.load_network(net)
        feed = PerspectiveInput(np.zeros((2, 48, 64, 3), np.uint8), np.stack([IDENTITY] * 2, 0))
        if fit is None:
            with pytest.raises(ValueError, match='^detections: .*a TiledScreen needs input .* fed a RoiInput'):
                ex.infer({name: feed}, detections=TiledScreen())
        else:
            with pytest.raises(ValueError, match='^detections: .*declares resize_fit LETTERBOX and is fed a PerspectiveInput'):
                ex.infer({name: feed}, detections=0.5)
        with pytest.raises(ValueError, match='^detections: .*a RegionScreen needs input .* fed a RoiInput or a DetectedRois'):
            ex.infer({name: feed}, detections=RegionScreen())
        assert not ex.host_inputs.slots


def test_abi_declares_the_perspective_entries():
    from pyopenvino_amd import device
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    lib = device.load_library()
    for entry, count in ((ENTRY, 16), (ENTRY_COLOR, 18)):
        assert entry in device.SIGNATURES and len(device.SIGNATURES[entry][1]) == count and entry not in device._NOT_STATUS
        m = re.search(r'\b' + entry + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S)
        assert m and len(m.group(1).split(',')) == count and 'const long long* table' in m.group(1) and 'float pad_value' in m.group(1)
        assert hasattr(lib, entry)
    assert 'int matrix' in re.search(ENTRY_COLOR + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S).group(1)
    assert re.search(r'#define\s+PVHIP_ABI_VERSION\s+19\b', header) and lib.pvhip_abi_version() == 19
    import pyopenvino_amd
    from pyopenvino_amd import input_format
    assert pyopenvino_amd.PerspectiveInput is input_format.PerspectiveInput and 'PerspectiveInput' in pyopenvino_amd.__all__


# ---------------------------------------------------------------------------------------------------------------- GPU
def _matrices(hw, dst_hw):
    """Eight rows over m = 3 frames: an affine-equivalent row, a mild keystone, a from_quad row with fractional corners, a keystone whose
    horizon crosses the output between two pixels of one quad (D changes sign inside it), a negated matrix, a row wholly outside the
    frame, a keystone whose horizon is column 8 itself (D == 0 there), and a row whose id is no frame."""
    from pyopenvino_amd import perspective, warp
    (H, W), (hd, wd) = hw, dst_hw
    affine = perspective.from_affine(warp.rotated_rect(W / 2, H / 2, 0.8 * W, 0.9 * H, 25, dst_hw))
    mild = np.array([[W / wd, 0.05, 0.3], [0.02, H / hd, 0.2], [0.004, 0.003, 1.0]])
    quad = perspective.from_quad([[1.3, 2.6], [W - 2.2, 0.4], [W + 1.7, H - 1.9], [0.6, H - 3.1]], dst_hw)
    xh = 4 * (wd // 8) + 1.5                                  # D = 1 - x / xh: zero between the middle pixels of one quad
    horizon = np.array([[0.4 * W / wd, 0, 1], [0, 0.4 * H / hd, 1], [-1 / xh, 0, 1.0]])
    crossing = np.array([[W / wd, 0, 0], [0, H / hd, 0], [-1 / 8, 0, 1.0]])    # ... and exactly on column 8
    outside = np.array([[1, 0, W + 5.0], [0, 1, 2], [0.001, 0, 1]])
    rows = [affine, mild, quad, horizon, -quad, outside, crossing, mild]
    ids = [2, 0, 1, 0, 1, 2, 1, 3]
    table = pref.table_of(np.stack(rows, 0), ids, dst_hw)
    d = [table[3, 7] * x + table[3, 9] for x in range(wd)]
    assert min(d) < 0 < max(d) and 0 not in d and any(d[x] > 0 > d[x + 1] and x % 4 != 3 for x in range(wd - 1))
    assert table[6, 7] * 8 + table[6, 9] == 0
    return table


class _Device(wt._Device):
    def run(self, entry, kind, table, m, hw, dst_hw, c=3, guard=4, rule=(), **opt):
        """`entry` into a destination prefilled with 0x7f bytes: (the n images, the guard floats in front and behind)."""
        hip, n = self.hip, len(table)
        count = n * c * dst_hw[0] * dst_hw[1]
        whole = hip.DeviceTensor.empty((count + 2 * guard,))
        hip.call('pvhip_memset', ctypes.c_void_p(whole.ptr), 0x7f, whole.nbytes)
        t = hip.DeviceTensor.from_numpy(np.ascontiguousarray(table, np.int64))
        scaled = 'mean' in opt
        hip.call(entry, ctypes.c_void_p(self.src), ctypes.c_void_p(whole.ptr + 4 * guard), ctypes.c_void_p(t.ptr), n, m, c, *hw, *dst_hw,
                 *wt._form(kind), int(opt.get('reverse', False)), ctypes.c_void_p(self.mean.ptr) if scaled else None,
                 ctypes.c_void_p(self.std.ptr) if scaled else None, opt.get('pad', 0.0), *rule)
        got = np.asarray(whole)
        return got[guard:guard + count].reshape((n, c) + tuple(dst_hw)), np.concatenate([got[:guard], got[guard + count:]])


def _check_rows(got, want, table, m, what):
    for b in range(len(table)):                               # row by row: a failure names the matrix
        if 0 <= table[b, 0] < m:
            assert_bit_exact(got[b], want[b], '{} row {} = {}'.format(what, b, table[b].tolist()))
        else:
            assert np.isnan(want[b]).all() and (got[b].view(np.uint32) & 0x7fc00000 == 0x7fc00000).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize('hw', FRAMES)
@pytest.mark.parametrize('kind', KINDS)
def test_perspective_kernel_bit_exact(hip, kind, hw):
    rng = np.random.default_rng(sum(hw) * 7 + len(kind) + KINDS.index(kind))
    m = 3
    frames = wt._frames(rng, kind, m, hw, special=kind.startswith('FP32'))
    dev = _Device(hip, frames)
    for dst_hw in DESTS:
        table = _matrices(hw, dst_hw)
        for opt in OPTIONS:
            want = _ref(kind, frames, table, dst_hw, **opt)
            got, guards = dev.run(ENTRY, kind, table, m, hw, dst_hw, **opt)
            _check_rows(got, want, table, m, '{} {} -> {} {}'.format(kind, hw, dst_hw, sorted(opt)))
            assert (guards.view(np.uint32) == 0x7f7f7f7f).all()


@pytest.mark.gpu
@pytest.mark.parametrize('shift', [1, 3])
@pytest.mark.parametrize('kind', ['U8-NHWC', 'YUY2', 'BGRX', 'NV12'])
def test_perspective_kernel_bit_exact_from_unaligned_frames(hip, kind, shift):
    rng = np.random.default_rng(71 + len(kind) + shift)
    hw, m, dst_hw = (34, 70), 3, (37, 45)
    frames = wt._frames(rng, kind, m, hw)
    dev = _Device(hip, frames, shift=shift)
    table = _matrices(hw, dst_hw)
    got, guards = dev.run(ENTRY, kind, table, m, hw, dst_hw, **OPTIONS[1])
    _check_rows(got, _ref(kind, frames, table, dst_hw, **OPTIONS[1]), table, m, '{} {} bytes off alignment'.format(kind, shift))
    assert (guards.view(np.uint32) == 0x7f7f7f7f).all()


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_affine_rows_equal_the_warp_entry_on_the_device(hip, kind):
    """Against the code that was there before, not the restatement: a table of [[A], [0, 0, 1]] rows gives the bits of
    pvhip_input_preprocess_warp_f32 on the Q16 table of the same matrices."""
    from pyopenvino_amd import WarpInput, perspective
    rng = np.random.default_rng(103 + len(kind))
    hw, m = (34, 70), 3
    frames = wt._frames(rng, kind, m, hw, special=kind.startswith('FP32'))
    dev = _Device(hip, frames)
    for dst_hw in DESTS:
        for affine in wt._matrix_set(hw, dst_hw):
            A = affine[:, 1:].reshape(-1, 2, 3) / 65536.0       # what the table holds: multiples of 2^-16
            assert np.array_equal(WarpInput.fixed(A), affine[:, 1:])
            table = pref.table_of(np.stack([perspective.from_affine(a) for a in A], 0), affine[:, 0], dst_hw)
            for opt in OPTIONS:
                want, _ = dev.run(wt.ENTRY, kind, affine, m, hw, dst_hw, **opt)
                got, _ = dev.run(ENTRY, kind, table, m, hw, dst_hw, **opt)
                assert_bit_exact(got, want, '{} -> {} {}: {}'.format(kind, dst_hw, sorted(opt), A.tolist()))


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['NV12', 'UYVY'])
def test_perspective_color_entry(hip, kind):
    rng = np.random.default_rng(30 + len(kind))
    hw, m, dst_hw = (34, 70), 3, (37, 45)
    frames = wt._frames(rng, kind, m, hw)
    dev = _Device(hip, frames)
    table = _matrices(hw, dst_hw)
    rule = ('BT709', 'FULL')
    bgr = cref.to_bgr(frames, kind, *rule)
    assert not np.array_equal(bgr, wt._image(kind, frames))
    for opt in OPTIONS:
        want = _ref('U8-NHWC', bgr, table, dst_hw, **opt)
        got, guards = dev.run(ENTRY_COLOR, kind, table, m, hw, dst_hw, rule=cref.codes(*rule), **opt)
        _check_rows(got, want, table, m, '{} {} {}'.format(kind, rule, sorted(opt)))
        assert (guards.view(np.uint32) == 0x7f7f7f7f).all()
        plain, _ = dev.run(ENTRY, kind, table, m, hw, dst_hw, **opt)
        default, _ = dev.run(ENTRY_COLOR, kind, table, m, hw, dst_hw, rule=(0, 0), **opt)
        assert_bit_exact(default, plain, '{} (0, 0) is the plain entry {}'.format(kind, sorted(opt)))


@pytest.mark.gpu
def test_perspective_entries_reject_what_they_cannot_do(hip):
    lib = hip.load_library()
    src = hip.DeviceTensor.from_numpy(np.zeros(256, np.uint8))
    dst = hip.DeviceTensor.from_numpy(np.full(64, 7, np.float32))
    table = hip.DeviceTensor.from_numpy(pref.table_of([IDENTITY], [0], (2, 2)))
    s, d, t = ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), ctypes.c_void_p(table.ptr)
    entry, color = getattr(lib, ENTRY), getattr(lib, ENTRY_COLOR)
    good = (1, 1, 3, 4, 4, 2, 2, 0, 3, 0)                     # n, m, c, src_h, src_w, dst_h, dst_w, format, how, reverse

    def changed(**at):
        out = list(good)
        for k, v in at.items():
            out[int(k[1:])] = v
        return tuple(out)

    zero = ctypes.c_float(0.0)
    assert entry(s, d, None, *good, None, None, zero) == -2   # PVHIP_EINVAL, nothing launched: a NULL table
    for pad in (np.nan, np.inf, -np.inf):
        assert entry(s, d, t, *good, None, None, ctypes.c_float(pad)) == -2
    for args in (changed(_7=3), changed(_7=-1), changed(_7=1, _8=0, _2=1), changed(_7=1, _8=0, _2=4), changed(_7=2, _8=2, _2=4),
                 changed(_7=2, _8=0, _2=1),                   # format out of range; c != 3 for a colour format
                 changed(_8=4), changed(_8=-1), changed(_7=1, _8=2), changed(_7=2, _8=4),            # `how` out of range
                 changed(_7=1, _8=0, _3=3), changed(_7=1, _8=1, _4=3), changed(_7=2, _8=1, _4=3),    # odd extents of 4:2:0 and 4:2:2
                 changed(_0=0), changed(_0=70000), changed(_1=0), changed(_2=0), changed(_2=2000), changed(_3=0), changed(_4=0),
                 changed(_5=0), changed(_6=0), changed(_3=40000, _4=40000), changed(_5=40000, _6=40000)):
        assert entry(s, d, t, *args, None, None, zero) == -2, args
        assert color(s, d, t, *args, None, None, zero, 0, 0) == -2, args
    assert entry(None, d, t, *good, None, None, zero) == -2
    assert entry(s, None, t, *good, None, None, zero) == -2
    assert entry(ctypes.c_void_p(src.ptr + 1), d, t, *changed(_8=2), None, None, zero) == -2           # fp32 off element alignment
    for matrix, full in ((3, 0), (-1, 0), (0, 2)):
        assert color(s, d, t, *changed(_7=1, _8=0), None, None, zero, matrix, full) == -2
    assert color(s, d, t, *good, None, None, zero, 1, 0) == -2                                         # raw frames hold nothing to convert
    assert color(s, d, t, *changed(_7=2, _8=2), None, None, zero, 0, 1) == -2                          # nor do four-byte pixels
    assert np.array_equal(np.asarray(dst), np.full(64, 7, np.float32))
    for args in (good, changed(_7=1, _8=0), changed(_7=1, _8=1), changed(_7=2, _8=0), changed(_7=2, _8=3), changed(_7=2, _8=2, _4=3)):
        assert entry(s, d, t, *args, None, None, zero) == 0, args                # (and the same arguments in order are taken)
    assert color(s, d, t, *changed(_7=1, _8=1), None, None, zero, 2, 1) == 0
    assert not np.array_equal(np.asarray(dst), np.full(64, 7, np.float32))


def _plate_matrices(hw, dst_hw, n):
    """n quadrilaterals seen at an angle, the second one leaving the frame."""
    from pyopenvino_amd import perspective
    H, W = hw
    quads = [[[0.12 * W, 0.2 * H], [0.8 * W, 0.07 * H], [0.93 * W, 0.85 * H], [0.05 * W, 0.7 * H]],
             [[0.5 * W, -0.2 * H], [1.2 * W, 0.3 * H], [0.9 * W, 1.1 * H], [0.3 * W, 0.6 * H]]]
    return np.stack([perspective.from_quad(quads[b % 2], dst_hw) for b in range(n)], 0)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['U8-NHWC', 'NV12'])
def test_googlenet_from_perspectives_matches_the_restatement_fed_as_a_tensor(hip, kind):
    """infer({name: PerspectiveInput(frames, H)}) with mean / scale declared: the Results of a network without declared formats fed
    perspective_ref's tensor, bit for bit, three passes in a row (the third replays the recording)."""
    from pyopenvino_amd import PerspectiveInput
    rng = np.random.default_rng(224 + len(kind))
    n, m, hw, dst = 2, 3, (96, 128), (224, 224)
    frames = wt._frames(rng, kind, m, hw)
    M, ids = _plate_matrices(hw, dst, n), [2, 0]
    pad = 114.0
    want_input = _ref(kind, frames, pref.table_of(M, ids, dst), dst, reverse=True, mean=MEAN, std=STD, pad=pad)
    assert (want_input[1, 0] == (np.float32(pad) - np.float32(MEAN[0])) / np.float32(STD[0])).any()    # pad taps are in it
    ie, net, name = wt._net('googlenet-v1', n)
    out_name = net.outputs[0]['name']
    want = np.array(ie.load_network(net).infer({name: want_input})[out_name], copy=True)
    assert np.isfinite(want).all()
    ie, net, name = wt._net('googlenet-v1', n)
    wt._declare(net, name, kind, reverse=True, mean=(MEAN, STD), pad=pad)
    ex = ie.load_network(net)
    untouched = frames.copy()
    for step in range(3):
        got = ex.infer({name: PerspectiveInput(frames, M, ids)})[out_name]
        assert_bit_exact(wt._fixed(ex, name), want_input, '{} input tensor, pass {}'.format(kind, step))
        assert_bit_exact(got, want, '{} PerspectiveInput through infer(), pass {}'.format(kind, step))
    assert np.array_equal(frames, untouched)
    req = ex.requests[0]
    assert_bit_exact(req.infer({name: PerspectiveInput(frames, M.tolist(), np.array(ids))})[out_name], want, kind + ' through a request, as lists')


@pytest.mark.gpu
def test_mnist_from_one_channel_fp32_perspectives(hip):
    from pyopenvino_amd import PerspectiveInput
    rng = np.random.default_rng(28)
    n, m, hw, dst = 2, 1, (40, 36), (28, 28)
    frames = wt._frames(rng, 'FP32-NCHW', m, hw, c=1)
    M = _plate_matrices(hw, dst, n)
    mean = ([0.5], [2.0])
    want_input = pref.warp(frames, pref.table_of(M, [0, 0], dst), dst, nhwc=False, mean=mean[0], std=mean[1])
    ie, net, name = wt._net('mnist', n)
    out_name = net.outputs[0]['name']
    want = np.array(ie.load_network(net).infer({name: want_input})[out_name], copy=True)
    ie, net, name = wt._net('mnist', n)
    info = net.input_info[name]
    info.precision, info.layout = 'FP32', 'NCHW'
    pre = info.preprocess_info
    pre.resize_algorithm = 'RESIZE_BILINEAR'
    pre.init(1)
    pre[0].mean_value, pre[0].std_scale = mean[0][0], mean[1][0]
    pre.mean_variant = 'MEAN_VALUE'
    ex = ie.load_network(net)
    for step in range(3):
        got = ex.infer({name: PerspectiveInput(frames, M)})[out_name]       # m == 1: every row reads the frame
        assert_bit_exact(wt._fixed(ex, name), want_input, 'mnist input tensor, pass {}'.format(step))
        assert_bit_exact(got, want, 'mnist from perspectives, pass {}'.format(step))


@pytest.mark.gpu
def test_perspective_buffer_feeds_without_a_host_copy(hip):
    from pyopenvino_amd import PerspectiveInput
    rng = np.random.default_rng(77)
    n, m, hw, dst = 2, 3, (96, 128), (224, 224)
    frames = wt._frames(rng, 'NV12', m, hw)
    M, ids = _plate_matrices(hw, dst, n), [1, 2]
    ie, net, name = wt._net('googlenet-v1', n)
    out_name = net.outputs[0]['name']
    wt._declare(net, name, 'NV12', mean=(MEAN, STD))
    ex = ie.load_network(net, 'GPU', num_requests=2)
    want = np.array(ex.infer({name: PerspectiveInput(frames, M, ids)})[out_name], copy=True)
    want_input = wt._fixed(ex, name)
    assert_bit_exact(want_input, _ref('NV12', frames, pref.table_of(M, ids, dst), dst, mean=MEAN, std=STD), 'the rule')
    req = ex.requests[1]
    buf, tbuf = req.input_buffer(name, hw, frames=m), req.perspective_buffer(name)
    assert buf.shape == (m, 144, 128) and buf.dtype == np.uint8
    assert tbuf.shape == (n, 10) and tbuf.dtype == np.int64 and tbuf.flags.c_contiguous and req.perspective_buffer(name) is tbuf
    assert ex.requests[0].perspective_buffer(name) is not tbuf
    slot = req.runner.host_inputs.slots[name]
    assert tbuf is slot.tables['perspective'].host and buf is slot.extents[(hw, m)].host
    buf[...] = frames
    tbuf[...] = pref.table_of(M, ids, dst)
    copies, staged = [], []
    real, real_call = np.copyto, hip.call
    np.copyto = lambda dst, *a, **k: (copies.append(dst), real(dst, *a, **k))[1]
    hip.call = lambda entry, *args: (staged.append((entry, args)), real_call(entry, *args))[1]
    try:
        got = req.infer({name: PerspectiveInput(buf, tbuf)})[out_name]
    finally:
        np.copyto, hip.call = real, real_call
    assert not any(c is buf or c is tbuf for c in copies)     # neither the frames nor the table was copied on the host
    uploaded = [args[1].value for entry, args in staged if entry == 'pvhip_memcpy_h2d_async']
    assert buf.ctypes.data in uploaded and tbuf.ctypes.data in uploaded                # the same pointers are staged
    assert_bit_exact(got, want, 'PerspectiveInput from the request buffers')
    assert_bit_exact(np.asarray(slot.fixed), want_input, 'its input tensor')
    assert len(slot.extents) == 1
    # a table in the buffer that breaks the limit: refused before anything is staged
    launched = []
    for column, value, match in ((2, 1 << 52, r'matrices\[1\] is beyond the limit'), (9, np.iinfo(np.int64).min, r'matrices\[1\] is beyond'),
                                 (0, m, r'ids\[1\] = 3 is none of 3 frames'), (0, -1, r'ids\[1\] = -1')):
        tbuf[...] = pref.table_of(M, ids, dst)
        tbuf[1, column] = value
        hip.call = lambda entry, *args: (launched.append(entry), real_call(entry, *args))[1]
        try:
            with pytest.raises(ValueError, match=match):
                req.infer({name: PerspectiveInput(buf, tbuf)})
        finally:
            hip.call = real_call
    assert not [e for e in launched if 'input' in e or 'memcpy' in e], launched
    with pytest.raises(ValueError, match='the perspective_buffer holds .* ids is None'):
        req.infer({name: PerspectiveInput(buf, tbuf, ids)})
    tbuf[...] = pref.table_of(M, ids, dst)
    assert_bit_exact(req.infer({name: PerspectiveInput(buf, tbuf)})[out_name], want, 'and the good table again')
