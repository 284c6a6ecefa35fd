"""A classifier's answer made on the device (``infer(..., top_k=k)``, pvhip_topk_rows_f32): the k best classes of every batch row by the
rule of tests/topk_ref.py -- indices exact, values bit for bit --, one launch behind the pass and one read-back of 8 n k bytes.  The
first tests need no GPU."""
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest

import helpers
import test_detected_rois as det_tests
import test_roi_input as roi_tests
import topk_ref
from helpers import GOLDEN, MODELS

ENTRY = 'pvhip_topk_rows_f32'
NAN, INF = np.float32(np.nan), np.float32(np.inf)
_net = roi_tests._net


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what=''):
    """`got` (a TopK of the product) equals `want` (the rule's): indices exact, values bit for bit."""
    assert got.indices.dtype == np.int32 and got.values.dtype == np.float32, (what, got.indices.dtype, got.values.dtype)
    assert got.indices.shape == want.indices.shape == got.values.shape == want.values.shape, (what, got.indices.shape, want.indices.shape)
    bad = np.flatnonzero((got.indices != want.indices).any(axis=1))
    assert not len(bad), '{}: row {}: indices {} want {}'.format(what, bad[0], got.indices[bad[0]].tolist(), want.indices[bad[0]].tolist())
    bad = np.flatnonzero((_bits(got.values) != _bits(want.values)).any(axis=1))
    assert not len(bad), '{}: row {}: value bits {} want {}'.format(what, bad[0], _bits(got.values)[bad[0]].tolist(), _bits(want.values)[bad[0]].tolist())


def _f32(words):
    return np.array(words, np.uint32).view(np.float32)


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
def test_the_rule_on_hand_written_rows():
    from pyopenvino_amd import TopK, top_k

    def both(row, k):
        row = np.asarray(row, np.float32)
        want = topk_ref.top_k(row[None], k)
        got = top_k.top_k_rows(row[None], k)                   # the product's own numpy form (host Results) is the same rule
        assert isinstance(got, TopK)
        _same(got, want, str(row.tolist()))
        assert np.array_equal(_bits(want.values[0]), _bits(row[want.indices[0]]))
        return want.indices[0].tolist(), want.values[0]

    assert both([2.5] * 9, 4)[0] == [0, 1, 2, 3]                                 # all equal: 0 .. k - 1
    idx, val = both([0.0, -0.0, 0.0], 3)
    assert idx == [0, 1, 2] and _bits(val).tolist() == [0, 0x80000000, 0]         # zeros of either sign are equal; the sign bits are kept
    assert both([3.0, 1.0, 2.0, NAN], 2)[0] == [3, 0]                             # a NaN in the last position comes first
    two = _f32([0x3F800000, 0xFFC00123, 0x40000000, 0x7F800001])                  # two NaNs (one negative, one signalling): index order
    idx, val = both(two, 3)
    assert idx == [1, 3, 2] and _bits(val).tolist() == [0xFFC00123, 0x7F800001, 0x40000000]      # payloads kept
    assert both([1.0, INF, NAN, 5.0], 3)[0] == [2, 1, 3]                          # +inf comes behind NaN
    assert both([-INF, -1.0, -3.0e38, 0.0], 4)[0] == [3, 1, 2, 0]                 # -inf comes last
    assert both([1e-45, -1e-45, 0.0, -0.0], 4)[0] == [0, 2, 3, 1]                 # denormals keep their sign; the zeros tie between them
    assert both([1.0, 3.0, 3.0, 2.0, 3.0], 5)[0] == [1, 2, 4, 3, 0]               # ties: the lower index first
    assert both([7.0], 1)[0] == [0]
    # (n, C, 1, 1) is (n, C); anything else is refused
    x = np.arange(12, dtype=np.float32).reshape(2, 6, 1, 1)
    assert top_k.top_k_rows(x, 2).indices.tolist() == [[5, 4], [5, 4]]
    for bad, k in ((np.zeros((1, 1, 4, 7), np.float32), 1), (np.zeros(5, np.float32), 1), (np.zeros((2, 3), np.float64), 1),
                   (np.zeros((2, 3), np.float32), 0), (np.zeros((2, 3), np.float32), 4), (np.zeros((2, 100), np.float32), 65)):
        with pytest.raises(ValueError):
            top_k.top_k_rows(bad, k)


def _golden_rows():
    z = np.load(os.path.join(GOLDEN, 'googlenet_rows8.npz'))
    out = z['out']
    assert out.shape == (8, 1000) and out.dtype == np.float32
    return z, out


def _decided_gap(out, k):
    """The smallest gap between neighbouring scores among the first k + 1 of any row, and the largest deviation two scores of the
    project's bound (helpers.assert_close: |d| <= 1e-4 |want| + 1e-4 rms(want)) may show between them."""
    first = -np.sort(-out.astype(np.float64), axis=1)[:, :k + 1]
    gap = float((first[:, :-1] - first[:, 1:]).min())
    rms = float(np.sqrt(np.mean(out.astype(np.float64) ** 2)))
    return gap, 2 * (helpers.REL_TOL * float(first.max()) + helpers.REL_TOL * rms)


def test_on_the_recorded_googlenet_rows_the_rule_is_the_samples_argsort():
    _, out = _golden_rows()
    assert np.isfinite(out).all()
    gap, slack = _decided_gap(out, 5)
    print('smallest gap among the first six scores of a row: {:.3e}; twice the bound: {:.3e}'.format(gap, slack))
    assert gap >= 3.7e-3 and gap > slack                      # no ties among them, and the 1e-4 bound cannot reorder them
    want = topk_ref.top_k(out, 5)
    for r in range(8):
        assert np.array_equal(want.indices[r], np.argsort(out[r])[::-1][:5]), r
        assert np.array_equal(want.values[r], out[r][np.argsort(out[r])[::-1][:5]]), r


def test_argument_rules():
    """Every refusal is a ValueError raised before anything is staged or launched: this test runs where there is no device."""
    n = 4
    ie, net, name = _net(batch=n)
    ex = ie.load_network(net, 'GPU', num_requests=2)
    out_name = net.outputs[0]['name']
    assert out_name == 'prob/sink_port_0' and tuple(net.outputs[0]['input'][0]['dims']) == (n, 1000)
    x = np.zeros((n, 3, 224, 224), np.float32)
    req = ex.requests[0]
    starts = (lambda k: ex.infer({name: x}, top_k=k), lambda k: ex.infer({name: x}, False, k), lambda k: req.start_async({name: x}, top_k=k),
              lambda k: req.start_async({name: x}, k), lambda k: ex.requests[1].infer({name: x}, top_k=k), lambda k: req.infer({name: x}, k),
              lambda k: ex.start_async(1, {name: x}, top_k=k), lambda k: ex.start_async(0, {name: x}, k))

    def refused(match, k, network=ex, starts=starts):
        for start in starts:
            with pytest.raises(ValueError, match=match) as e:
                start(k)
            assert str(e.value).startswith('top_k: '), str(e.value)
        for r in network.requests:
            assert not r._in_flight and not r._asks and not r.runner.answers.blocks and not r.runner.host_inputs.slots and r.runner._pending is None

    for bad in (0, -1, 65, 1001, 2 ** 31):
        refused('outside 1', bad)
        refused('outside 1', {out_name: bad})
    for bad in (1.0, '5', True, None, [5], (1,)):
        refused('k is a count', bad if bad is not None else {out_name: None})
    refused('no Result named', {'prob': 5})                   # (a Result goes by the name infer() returns it under)
    refused('no Result named', {out_name: 5, 'nope': 1})
    ex.comm = types.SimpleNamespace(world=2, rank=0)
    try:
        refused('sharded', 5)
        refused('sharded', {out_name: 1})
    finally:
        ex.comm = None
    # an FP16 Result (every request has its own copy of the graph)
    ports = [r.runner.ienet.outputs[0]['input'][0] for r in ex.requests]
    for port in ports:
        port['precision'] = 'FP16'
    try:
        refused('FP32 Results only', 5)
    finally:
        for port in ports:
            port['precision'] = 'FP32'
    # the SSD head's records are no rows of scores
    ie_d, net_d, name_d = _net('ssd_mobilenet_v1_coco', 2)
    det = ie_d.load_network(net_d, 'GPU', num_requests=1)
    det_out = net_d.outputs[0]['name']
    dims = tuple(net_d.outputs[0]['input'][0]['dims'])
    assert dims[:2] == (1, 1) and dims[3] == 7
    xd = np.zeros((2, 3, 300, 300), np.float32)
    det_starts = (lambda k: det.infer({name_d: xd}, top_k=k), lambda k: det.requests[0].start_async({name_d: xd}, top_k=k),
                  lambda k: det.start_async(0, {name_d: xd}, top_k=k))
    refused(r'not \(n, C\) or \(n, C, 1, \.\.\.\)', 1, det, det_starts)
    refused(r'not \(n, C\) or \(n, C, 1, \.\.\.\)', {det_out: 1}, det, det_starts)
    # nothing asked for: {} and None are the call as it was (no device here: it fails further on, not with a ValueError of top_k)
    from pyopenvino_amd import top_k
    assert top_k.checked(net, None, False) == {} and top_k.checked(net, {}, True) == {} and top_k.checked(net, 5, False) == {out_name: 5}
    assert top_k.checked(net, {out_name: np.int64(64)}, False) == {out_name: 64}
    assert top_k.rows_of((8, 1000)) == (8, 1000) and top_k.rows_of((8, 1000, 1, 1)) == (8, 1000) and top_k.rows_of((1, 1, 200, 7)) is None
    assert top_k.rows_of((1000,)) is None and top_k.rows_of((8, 10, 2)) is None


def test_a_host_result_gets_the_rule_in_numpy():
    """A plugin set that computes on the host (the oracle's) hands wait() host arrays: the same keyword, the same rule, no device."""
    from pyopenvino_amd import IECore, TopK, synth
    ie = IECore(plugin_package='oracle.op_plugins')
    net = ie.read_network(os.path.join(MODELS, 'mnist.xml'))
    net.set_batch(4)
    ex = ie.load_network(net, 'GPU', num_requests=2)
    name, out_name = net.inputs[0]['name'], net.outputs[0]['name']
    x = np.concatenate([synth.uniform_pixels(10 + i, (1, 1, 28, 28)) for i in range(4)], 0)
    full = np.array(ex.infer({name: x})[out_name], copy=True)
    assert full.shape == (4, 10) and full.dtype == np.float32
    for k in (1, 3, 10):
        for got in (ex.infer({name: x}, top_k=k), ex.requests[1].infer({name: x}, top_k={out_name: k})):
            assert isinstance(got[out_name], TopK)
            _same(got[out_name], topk_ref.top_k(full, k), 'k = {}'.format(k))
    assert np.array_equal(ex.infer({name: x})[out_name], full)           # and whole again without the keyword
    with pytest.raises(ValueError, match='outside 1'):
        ex.infer({name: x}, top_k=11)


def test_abi_declares_the_entry():
    import pyopenvino_amd
    from pyopenvino_amd import device, top_k
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert ENTRY in device.SIGNATURES and len(device.SIGNATURES[ENTRY][1]) == 6 and ENTRY not in device._NOT_STATUS
    m = re.search(r'\bint\s+' + ENTRY + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S)
    assert m and len(m.group(1).split(',')) == 6
    assert 'np.lexsort((np.arange(cols), -np.where(isnan, 0, x), ~isnan))[:k]' in header          # the rule is stated there
    assert re.search(r'#define\s+PVHIP_ABI_VERSION\s+19\b', header)
    lib = device.load_library()
    assert hasattr(lib, ENTRY) and lib.pvhip_abi_version() == 19
    assert pyopenvino_amd.TopK is top_k.TopK and 'TopK' in pyopenvino_amd.__all__ and pyopenvino_amd.TopK._fields == ('indices', 'values')


# ---------------------------------------------------------------------------------------------------------------- GPU
GUARD = 16                                                    # sentinel words in front of and behind each output
SENTINEL = 0x7f7f7f7f
SPECIALS = [0x7FC00000, 0xFFC00001, 0x7F800123,               # three NaNs of different payloads: quiet, negative, signalling
            0x00000000, 0x80000000, 0x7F800000, 0xFF800000,   # +0, -0, +inf, -inf
            0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF]   # the smallest and the largest denormals of either sign


def _fillings(rng, rows, cols, k):
    """[(what, (rows, cols) float32)]: every filling of the rule's kernel test for one shape."""
    ramp = np.arange(cols, dtype=np.float32)[None, :] + np.arange(rows, dtype=np.float32)[:, None]       # exact: below 2^24
    mixed = rng.standard_normal((rows, cols)).astype(np.float32)
    nans = rng.standard_normal((rows, cols)).astype(np.float32)
    many = min(cols, k + 3)                                   # more NaNs than k wherever the row has room for them
    for r in range(rows):
        at = rng.choice(cols, size=min(cols, len(SPECIALS)), replace=False)
        start = 0 if cols >= len(SPECIALS) else int(rng.integers(0, len(SPECIALS)))
        mixed[r].view(np.uint32)[at] = np.roll(np.array(SPECIALS, np.uint32), -start)[:len(at)]
        at = rng.choice(cols, size=many, replace=False)
        nans[r].view(np.uint32)[at] = (np.uint32(0x7FC00000) | rng.integers(0, 1 << 22, many).astype(np.uint32)
                                       | (rng.integers(0, 2, many).astype(np.uint32) << np.uint32(31)))
    assert np.isnan(nans).sum(axis=1).min() == many and (cols < len(SPECIALS) or np.isnan(mixed).sum(axis=1).min() == 3)
    return [('normal', rng.standard_normal((rows, cols)).astype(np.float32)),
            ('three values', rng.integers(-1, 2, (rows, cols)).astype(np.float32)),
            ('all equal', np.full((rows, cols), 0.25, np.float32)),
            ('ascending', ramp),
            ('descending', np.ascontiguousarray(-ramp)),
            ('specials', mixed),
            ('NaNs', nans)]


def _device_top_k(hip, x, k, offset=0):
    """The entry on `x` (rows, cols) -- `offset`: starting that many elements into a larger device tensor --, the outputs between
    sentinel words that must stay untouched."""
    rows, cols = x.shape
    if offset:
        flat = np.concatenate([np.full(offset, 9e9, np.float32), x.ravel(), np.full(7, 9e9, np.float32)])
        src = hip.DeviceTensor.from_numpy(flat)
    else:
        src = hip.DeviceTensor.from_numpy(x)
    outs = [hip.DeviceTensor.empty((rows * k + 2 * GUARD,), np.int32) for _ in range(2)]
    for t in outs:
        hip.call('pvhip_memset', ctypes.c_void_p(t.ptr), 0x7f, t.nbytes)
    hip.call(ENTRY, ctypes.c_void_p(src.ptr + 4 * offset), rows, cols, k, *(ctypes.c_void_p(t.ptr + 4 * GUARD) for t in outs))
    idx, val = (np.asarray(t) for t in outs)
    for t in (idx, val):
        assert (t[:GUARD] == SENTINEL).all() and (t[-GUARD:] == SENTINEL).all(), 'a word outside the output was written'
    assert not (idx[GUARD:-GUARD] == SENTINEL).any(), 'an index was not written'
    return topk_ref.TopK(idx[GUARD:-GUARD].reshape(rows, k).copy(), val[GUARD:-GUARD].view(np.float32).reshape(rows, k).copy())


# (2, 1024, 7) and (2, 1025, 7) stand at the step from rows held in registers to rows read again in every round
SHAPES = [(1, 1, 1), (1, 2, 2), (3, 63, 5), (5, 64, 64), (4, 65, 64), (7, 1000, 5), (256, 1000, 5), (3, 1001, 10), (2, 1023, 64),
          (2, 1024, 7), (2, 1025, 7), (2, 4099, 64), (1, 70001, 33)]


@pytest.mark.gpu
@pytest.mark.parametrize('rows,cols,k', SHAPES)
def test_kernel_equals_the_rule(hip, rows, cols, k):
    rng = np.random.default_rng(rows * 100003 + cols * 67 + k)
    for what, x in _fillings(rng, rows, cols, k):
        _same(_device_top_k(hip, x, k), topk_ref.top_k(x, k), '{} {}'.format((rows, cols, k), what))
        if (rows, cols, k) == (3, 1001, 10):                  # no row starts on a 16-byte boundary
            for offset in (1, 2, 3):
                _same(_device_top_k(hip, x, k, offset), topk_ref.top_k(x, k), '{} {} offset {}'.format((rows, cols, k), what, offset))


@pytest.mark.gpu
def test_entry_rejects_what_it_cannot_do(hip):
    t = hip.DeviceTensor.from_numpy(np.arange(256, dtype=np.float32))
    o = hip.DeviceTensor.empty((512,), np.int32)
    p, q, v = ctypes.c_void_p(t.ptr), ctypes.c_void_p(o.ptr), ctypes.c_void_p(o.ptr + 1024)
    good = [p, 4, 64, 5, q, v]
    hip.call(ENTRY, *good)
    for at, bad in ((0, None), (4, None), (5, None), (1, 0), (1, -1), (2, 0), (2, -3), (3, 0), (3, -1), (3, 65)):
        args = list(good)
        args[at] = bad
        with pytest.raises(hip.PvhipError):
            hip.call(ENTRY, *args)
    for rows, cols, k in ((4, 64, 65), (4, 3, 4), (1 << 16, 1 << 15, 1), (1 << 30, 2, 1), (2, 1 << 30, 1)):
        with pytest.raises(hip.PvhipError):                   # k > 64, k > cols, rows * cols >= 2^31
            hip.call(ENTRY, p, rows, cols, k, q, v)
    hip.synchronize()
    x = np.arange(256, dtype=np.float32).reshape(4, 64)       # the device is still usable
    _same(_device_top_k(hip, x, 5), topk_ref.top_k(x, 5), 'after the refusals')


@functools.lru_cache(maxsize=None)
def _blob(seed):
    from pyopenvino_amd import synth
    return synth.synth_weights(os.path.join(MODELS, 'googlenet-v1.xml'), seed)


def _googlenet(batch, seed, requests=1):
    ie, net, name = _net('googlenet-v1', batch, _blob(seed))
    return ie.load_network(net, 'GPU', num_requests=requests), name, net.outputs[0]['name']


@pytest.mark.gpu
def test_public_path_on_googlenet(hip):
    """GoogLeNet at batch 8 on the golden file's weights and images: top_k=5 is the rule on the same request's own full Result, its
    indices are the reference's and its scores are inside the project's bound of the reference's; then a device-resident input five
    times with the keyword alternating, replayed from the request's one recording from the third call on."""
    from pyopenvino_amd import TopK, synth
    z, golden = _golden_rows()
    ex, name, out_name = _googlenet(8, int(z['weight_seed']))
    req = ex.requests[0]
    x = np.concatenate([synth.uniform_pixels(int(s), (1, 3, 224, 224)) for s in z['image_seeds']], 0)
    full = np.array(req.infer({name: x})[out_name], copy=True)
    assert full.shape == (8, 1000) and full.dtype == np.float32
    want = topk_ref.top_k(full, 5)
    got = req.infer({name: x}, top_k=5)
    assert set(got) == {out_name} and isinstance(got[out_name], TopK)
    _same(got[out_name], want, 'request')
    _same(ex.infer({name: x}, top_k=5)[out_name], want, 'the network\'s own infer()')
    _same(ex.infer({name: x}, False, {out_name: 64})[out_name], topk_ref.top_k(full, 64), 'k = 64')
    assert np.array_equal(ex.infer({name: x})[out_name], full)              # and whole again without the keyword
    # against the reference itself
    gap, slack = _decided_gap(golden, 5)
    assert gap > slack
    ref = topk_ref.top_k(golden, 5)
    assert np.array_equal(got[out_name].indices, ref.indices)
    full_at = np.take_along_axis(full, ref.indices.astype(np.int64), axis=1)
    assert np.array_equal(_bits(got[out_name].values), _bits(full_at))
    helpers.assert_close(full, golden, helpers.REL_TOL, 'the full Result vs the reference')
    scores = golden.copy()                                    # the k scores where they stand in the rows: assert_close's rms is the rows' own
    np.put_along_axis(scores, ref.indices.astype(np.int64), got[out_name].values, axis=1)
    helpers.assert_close(scores, golden, helpers.REL_TOL, 'top-5 scores vs the reference')
    helpers.assert_close(got[out_name].values, ref.values, helpers.REL_TOL, 'top-5 scores vs the reference\'s top-5')
    # the same device-resident tensor five times
    xd = hip.DeviceTensor.from_numpy(x)
    kinds = [5, None, {out_name: 1}, 5, None]
    first = {}
    for call, kind in enumerate(kinds):
        req.start_async({name: xd}, top_k=kind)
        assert (req._replayed is not None) == (call >= 2), 'call {}'.format(call)
        res = req.wait()[out_name]
        if kind is None:
            assert isinstance(res, np.ndarray)
            helpers.assert_bit_exact(res, full, 'call {}: whole'.format(call))
        else:
            k = kind if isinstance(kind, int) else kind[out_name]
            _same(res, topk_ref.top_k(full, k), 'call {}: top_k = {}'.format(call, kind))
        key = repr(kind)
        if key in first:
            if kind is None:
                helpers.assert_bit_exact(res, first[key], 'call {} vs the first of its kind'.format(call))
            else:
                _same(res, first[key], 'call {} vs the first of its kind'.format(call))
        else:
            first[key] = res if kind is not None else np.array(res, copy=True)
    assert ex._auto_graph['captured'] and ex._graph is not None              # one recording served every kind
    assert sorted(ex.answers.blocks) == [(out_name, 1), (out_name, 5), (out_name, 64)]     # the request's own blocks, one per (name, k), no other kind's
    ex.release_device_state()
    assert not ex.answers.blocks


@pytest.mark.gpu
def test_requests_in_flight(hip):
    """Three requests at batch 4, four steps, another input every time, top_k cycling through 1, 5 and None per request and step: all
    started, then all waited for; every answer is the rule on that input's synchronous single-request Result."""
    from pyopenvino_amd import synth
    B, R, steps = 4, 3, 4
    ex, name, out_name = _googlenet(B, 1234, requests=R)
    single, _, _ = _googlenet(B, 1234)
    xs = [[synth.uniform_pixels(3000 + 10 * step + r, (B, 3, 224, 224)) for r in range(R)] for step in range(steps)]
    fulls = [[np.array(single.infer({name: x})[out_name], copy=True) for x in row] for row in xs]
    assert len({f.tobytes() for row in fulls for f in row}) == R * steps
    kinds = (1, 5, None)
    seen = set()
    for step in range(steps):
        asked = [kinds[(r + step) % 3] for r in range(R)]
        for r in range(R):
            ex.start_async(r, {name: xs[step][r]}, top_k=asked[r])
        for r in (reversed(range(R)) if step % 2 else range(R)):
            res = ex.wait(r)[out_name]
            seen.add((r, asked[r]))
            if asked[r] is None:
                helpers.assert_bit_exact(res, fulls[step][r], 'step {} request {}'.format(step, r))
            else:
                _same(res, topk_ref.top_k(fulls[step][r], asked[r]), 'step {} request {} top_k = {}'.format(step, r, asked[r]))
    assert len(seen) == R * 3                                 # every request gave every kind of answer


@pytest.mark.gpu
def test_cascade_rows_behind_count_show_nan_first(hip):
    """GoogLeNet at batch 8 fed DetectedRois(frames, a records array) with fewer survivors than rows, top_k=3: all eight rows equal the
    rule on the full Result of the same feed bit for bit -- the rows behind `count` are NaN rows, whose answer is NaN at 0, 1, 2 --, and
    detected_rois() still reads its table afterwards."""
    from pyopenvino_amd import DetectedRois
    rng = np.random.default_rng(501)
    n, m, hw, kind = 8, 2, (480, 640), 'U8-NHWC'
    frames = roi_tests._frames(rng, kind, m, hw)
    rec = det_tests._random_records(rng, m, 40, long=True)
    scores = np.sort(rec[:, 2][np.isfinite(rec[:, 2])])[::-1]
    want = None
    for conf in scores[2:40]:                                 # the highest threshold that leaves 3 .. 7 survivors
        want = det_tests.detected_rois(rec, n, m, hw, min_confidence=float(conf))
        if 3 <= want.count < n:
            break
    assert want is not None and 3 <= want.count == want.selected < n, (want.count, want.selected)
    conf = float(conf)
    ex, name, out_name = det_tests._classifier(kind, n, _blob(11))
    req = ex.requests[0]
    full = np.array(req.infer({name: DetectedRois(frames, rec, min_confidence=conf)})[out_name], copy=True)
    det_tests._same(req.detected_rois(name), want, 'without top_k')
    assert np.isfinite(full[:want.count]).all() and np.isnan(full[want.count:]).all()
    got = req.infer({name: DetectedRois(frames, rec, min_confidence=conf)}, top_k=3)[out_name]
    _same(got, topk_ref.top_k(full, 3), 'cascade')
    assert (got.indices[want.count:] == (0, 1, 2)).all() and np.isnan(got.values[want.count:]).all()
    assert np.isfinite(got.values[:want.count]).all()
    det_tests._same(req.detected_rois(name), want, 'with top_k')
