"""A text recogniser's answer made on the device (``infer(..., text=...)``, pvhip_ctc_greedy_f32): the greedy CTC decoding of a (T, n, C),
(n, T, C) or (n, C, T) Result by the rule of tests/text_ref.py, bit for bit, one entry call behind the pass and one read-back of
4 n + 12 n T bytes.  The first tests need no GPU."""
import ctypes
import os
import re
import types
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import helpers
import test_keypoints as keypoints_tests
import test_top_k as top_k_tests
import text_ref
from helpers import MODELS

ENTRY, FORM = 'pvhip_ctc_greedy_f32', 'pvhip_ctc_greedy_form'
NAN = np.float32(np.nan)
QUIET = 0x7FC00000
FORM_NONE, FORM_ROWS, FORM_PLANES = 0, 1, 2             # PVHIP_TEXT_FORM_*
LAYOUTS = ('TNC', 'NTC', 'NCT')                         # PVHIP_TEXT_LAYOUT_* 0, 1, 2
MAX_STEPS = 4096                                        # PVHIP_TEXT_MAX_STEPS
FORM_STEPS = [MAX_STEPS]                                # the T behind which the form query changes its answer (to NONE), in every layout
MAX_BLOCKS = 2048                                       # PVHIP_TEXT_MAX_BLOCKS: the rows form's grid at most
ROWS_PER_BLOCK = 4                                      # a wave per (r, t) row, four waves a workgroup
_pixels, _bits = keypoints_tests._pixels, keypoints_tests._bits
det_tests, roi_tests = top_k_tests.det_tests, top_k_tests.roi_tests
SHAPES = [(1, 1, 2), (2, 3, 5), (3, 7, 37), (2, 65, 64), (1, 5, 1001), (2, 300, 3), (1, 4096, 2)]      # (n, T, C)
OFFSET_SHAPES = ((3, 7, 37), (1, 5, 1001), (2, 65, 64))
PATTERN = 'aa_abbb__c'                                  # the winners of the `runs` filling, cycled
SHIFT = 2                                               # so that the run b b b covers t = 63, 64 and the run _ _ covers t = 255, 256


def _physical(v, layout):
    """The (n, T, C) scores `v` as a contiguous tensor of `layout`."""
    return np.ascontiguousarray(v.transpose({'TNC': (1, 0, 2), 'NTC': (0, 1, 2), 'NCT': (0, 2, 1)}[layout]))


def _same(got, want, what=''):
    """`got` (a Text of the product) equals `want` (the rule's): lengths, symbols and steps exact, scores bit for bit."""
    assert [a.dtype for a in got] == [np.int32, np.int32, np.float32, np.int32], what
    assert [a.shape for a in got] == [a.shape for a in want], (what, [a.shape for a in got], [a.shape for a in want])
    assert np.array_equal(got.lengths, want.lengths), '{}: lengths {} want {}'.format(what, got.lengths.tolist(), want.lengths.tolist())
    for field in ('symbols', 'steps'):
        bad = np.argwhere(getattr(got, field) != getattr(want, field))
        assert not len(bad), '{}: slot {}: {} {} want {}'.format(what, bad[0].tolist(), field, getattr(got, field)[tuple(bad[0])], getattr(want, field)[tuple(bad[0])])
    bad = np.argwhere(_bits(got.scores) != _bits(want.scores))
    assert not len(bad), '{}: slot {}: score bits {:#x} want {:#x}'.format(what, bad[0].tolist(), _bits(got.scores)[tuple(bad[0])], _bits(want.scores)[tuple(bad[0])])


def _filler_behind_the_lengths(got):
    T = got.symbols.shape[1]
    behind = np.arange(T)[None, :] >= np.maximum(got.lengths, 0)[:, None]
    assert (got.symbols[behind] == -1).all() and (got.steps[behind] == -1).all() and (_bits(got.scores)[behind] == QUIET).all()
    assert (got.symbols[~behind] >= 0).all() and (got.steps[~behind] >= 0).all() and not np.isnan(got.scores[~behind]).any()
    assert (got.lengths >= -1).all() and all((np.diff(got.steps[r, :length]) > 0).all() for r, length in enumerate(got.lengths) if length > 0)      # in time order


def _runs(shape, blank):
    """One-hot scores of a designed winner sequence cycling a a _ a b b b _ _ c over `blank` (in 0 .. C - 1): the letters are the first
    non-blank classes, rotated by the batch row."""
    n, T, C = shape
    others = [c for c in range(C) if c != blank]
    v = np.zeros(shape, np.float32)
    for r in range(n):
        letter = {ch: others[(i + r) % len(others)] for i, ch in enumerate('abc')}
        letter['_'] = blank
        for t in range(T):
            v[r, t, letter[PATTERN[(t + SHIFT) % len(PATTERN)]]] = 1
    return v


def _fillings(rng, shape):
    """[(what, (n, T, C) float32)]: every filling of the rule's tests for one shape."""
    n, T, C = shape
    nans = rng.standard_normal(shape).astype(np.float32)
    many = max(1, nans.size // 40)
    at = rng.choice(nans.size, size=many, replace=False)
    kinds = np.array(top_k_tests.SPECIALS[:3], np.uint32)      # quiet, negative, signalling
    nans.reshape(-1).view(np.uint32)[at] = kinds[np.arange(many) % 3] | (rng.integers(0, 1 << 16, many).astype(np.uint32) << np.uint32(3))
    row = rng.standard_normal(shape).astype(np.float32)
    row.view(np.uint32)[n // 2] = QUIET                        # one all-NaN row (n == 1: the only one)
    return [('normal', rng.standard_normal(shape).astype(np.float32)), ('four levels', (rng.integers(0, 4, shape) / 4).astype(np.float32)),
            ('signed zeros', rng.choice(np.array([0.0, -0.0, -1.0, -2.0], np.float32), shape)), ('NaNs', nans), ('NaN row', row),
            ('all equal', np.full(shape, 0.25, np.float32))] + [('runs over {}'.format(b), _runs(shape, b % C)) for b in (-1, 0, C // 2)]


def _cases(shape):
    """[(what, layout, x, blank, merge_repeated, the rule's answer)] of a shape: every filling in every layout, with and without the
    merge, the blank last, first and in the middle.  Made once per shape and handed out unchanged.  For T >= 8 the inputs are held to
    what they are for: a decoder that drops nothing cannot pass."""
    if shape not in _cases.made:
        n, T, C = shape
        rng = np.random.default_rng(sum(d * 31 ** i for i, d in enumerate(shape)))
        made = []
        differ = blank_wins = some_void = some_not = full = False
        for what, v in _fillings(rng, shape):
            for layout in LAYOUTS:
                x = _physical(v, layout)
                winners = text_ref.winners_of(x, layout)
                for blank in (-1, 0, C // 2):
                    both = [text_ref.greedy(x, layout, blank, merge, winners=winners) for merge in (True, False)]
                    for merge, want in zip((True, False), both):
                        made.append(('{} {} {} blank {} merge {}'.format(shape, what, layout, blank, merge), layout, x, blank, merge, want))
                    differ |= not np.array_equal(both[0].lengths, both[1].lengths)
                    blank_wins |= any(w == blank % C for row in winners[0] for w in row)
                    some_void |= bool((both[0].lengths < 0).any())
                    some_not |= bool((both[0].lengths >= 0).any())
                    full |= bool((both[1].lengths == T).any())
            if what.startswith('runs') and T > 256:             # the merge drops a step across t = 63 / 64, the blank across 255 / 256
                w = v[0].argmax(axis=1)
                assert w[63] == w[64] != v[0, 255].argmax() == v[0, 256].argmax()
        assert T < 8 or (differ and blank_wins and some_not and full and (some_void or n == 1)), (shape, differ, blank_wins, some_void, some_not, full)
        _cases.made[shape] = made
    return _cases.made[shape]


_cases.made = {}


def _screen(layout, blank=-1, merge=True):
    from pyopenvino_amd import TextScreen
    return TextScreen(blank, merge, layout)


# ---------------------------------------------------------------------------------------------------------------- the test networks
def _with_text_chain(xml_path, out_path, blob, batch_in_ir, transposed, target):
    """The IR at `xml_path` with a Reshape to `target` (0: the batch) behind its first ReLU, a Transpose [1, 0, 2] behind that if
    `transposed`, and a Result 'text' at the end, written to `out_path`; the I64 constants stand behind `blob`: the new blob.  With
    `batch_in_ir` every activation port so far, which reads batch 1, is rewritten to that batch."""
    tree = ET.parse(xml_path)
    layers, edges = tree.getroot().find('layers'), tree.getroot().find('edges')
    by_id = {int(layer.get('id')): layer for layer in layers}
    relu = min(i for i, layer in by_id.items() if layer.get('type') == 'ReLU')
    n = batch_in_ir or 1
    if batch_in_ir:
        for i, layer in by_id.items():
            if i > relu or layer.get('type') == 'Const':
                continue
            ports = list(layer.find('output')) + [p for p in (layer.find('input') if layer.find('input') is not None else []) if p.get('id') == '0']
            for port in ports:
                port.find('dim').text = str(n)
            if layer.get('type') == 'Parameter':
                layer.find('data').set('shape', ', '.join([str(n)] + layer.find('data').get('shape').split(', ')[1:]))
    src = [int(d.text) for d in by_id[relu].find('output').find('port')]
    src_port = by_id[relu].find('output').find('port').get('id')
    shape = [n] + list(target[1:])
    assert np.prod(shape) == np.prod(src), (shape, src)
    consts, new = [np.array(target, np.int64)], max(by_id) + 1

    def layer(i, name, kind, inputs, output, precision='FP32', data=None):
        node = ET.SubElement(layers, 'layer', {'id': str(i), 'name': name, 'type': kind, 'version': 'opset1'})
        if data:
            ET.SubElement(node, 'data', data)
        if inputs:
            into = ET.SubElement(node, 'input')
            for j, (dims, prec) in enumerate(inputs):
                port = ET.SubElement(into, 'port', {'id': str(j), 'precision': prec})
                for d in dims:
                    ET.SubElement(port, 'dim').text = str(d)
        if output is not None:
            port = ET.SubElement(ET.SubElement(node, 'output'), 'port', {'id': str(len(inputs)), 'precision': precision})
            for d in output:
                ET.SubElement(port, 'dim').text = str(d)
        return node

    def edge(a, pa, b, pb):
        ET.SubElement(edges, 'edge', {'from-layer': str(a), 'from-port': str(pa), 'to-layer': str(b), 'to-port': str(pb)})

    def const(i, name, values, offset):
        layer(i, name, 'Const', [], [len(values)], 'I64', {'element_type': 'i64', 'offset': str(offset), 'shape': str(len(values)), 'size': str(8 * len(values))})

    blob = bytes(blob) + bytes(-len(blob) % 8)
    const(new, 'text/shape', target, len(blob))
    layer(new + 1, 'text/reshape', 'Reshape', [(src, 'FP32'), ([3], 'I64')], shape, data={'special_zero': 'true'})
    edge(relu, src_port, new + 1, 0)
    edge(new, 0, new + 1, 1)
    last, last_port, at = new + 1, 2, new + 2
    if transposed:
        consts.append(np.array([1, 0, 2], np.int64))
        const(at, 'text/axes', [1, 0, 2], len(blob) + 24)
        layer(at + 1, 'text/transpose', 'Transpose', [(shape, 'FP32'), ([3], 'I64')], [shape[1], shape[0], shape[2]])
        edge(last, last_port, at + 1, 0)
        edge(at, 0, at + 1, 1)
        shape, last, at = [shape[1], shape[0], shape[2]], at + 1, at + 2
    layer(at, 'text', 'Result', [(shape, 'FP32')], None)
    edge(last, last_port, at, 0)
    tree.write(out_path)
    return bytes(blob) + b''.join(c.tobytes() for c in consts)


def _text_head(tmp_path, batch, requests=1, package=keypoints_tests.HIP, transposed=False, whole=False):
    """mnist's first Convolution + bias + ReLU, a Reshape to (batch, 32, 676) and, `transposed`, a Transpose to (32, batch, 676): (the
    loaded network, the network, input name, Result name).  set_batch carries a batch on axis 0 only, so the transposed network has its
    batch written into the IR.  `whole`: the rest of mnist stays, with its classifier Result."""
    from pyopenvino_amd import IECore
    base = os.path.join(MODELS, 'mnist.xml') if whole else keypoints_tests._heatmap_head('mnist', tmp_path)
    if not whole:                                               # (without the head's own Result)
        tree = ET.parse(base)
        layers, edges = tree.getroot().find('layers'), tree.getroot().find('edges')
        (result,) = [layer for layer in layers if layer.get('type') == 'Result']
        for e in [e for e in edges if e.get('to-layer') == result.get('id')]:
            edges.remove(e)
        layers.remove(result)
        tree.write(base)
    stem = 'mnist_text_{}{}{}'.format('tnc' if transposed else 'ntc', '_whole' if whole else '', batch if transposed else '')
    xml, weights = os.path.join(str(tmp_path), stem + '.xml'), os.path.join(str(tmp_path), stem + '.bin')
    blob = _with_text_chain(base, xml, open(os.path.join(MODELS, 'mnist.bin'), 'rb').read(), batch if transposed else None, transposed, [0, 32, 676])
    with open(weights, 'wb') as f:
        f.write(blob)
    ie = IECore(plugin_package=package)
    net = ie.read_network(xml, weights=weights)
    if transposed:
        net.batch_size = batch                                  # the IR's own
    else:
        net.set_batch(batch)
    (out,) = [o for o in net.outputs if o['name'] == 'text']
    assert tuple(int(d) for d in out['input'][0]['dims']) == ((32, batch, 676) if transposed else (batch, 32, 676))
    return ie.load_network(net, 'GPU', num_requests=requests), net, net.inputs[0]['name'], 'text'


def _want(full, screen, layout):
    """text_ref on a request's own full Result for a TextScreen or True, read as `layout` where the screen names none."""
    from pyopenvino_amd import TextScreen
    screen = TextScreen() if screen is True else screen
    return text_ref.greedy(full, screen.layout or layout, screen.blank, screen.merge_repeated)


# ---------------------------------------------------------------------------------------------------------------- no GPU needed
def test_the_rule_on_hand_written_rows():
    from pyopenvino_amd import Text, TextScreen, text

    def both(v, layout='NTC', **screen):
        """`v`: (T, C) or (n, T, C) scores; the answer of the loops, which text.greedy equals, in every layout when none is named."""
        v = np.asarray(v, np.float32)
        v = v.reshape((1,) * (3 - v.ndim) + v.shape)
        for each in (LAYOUTS if layout is None else (layout,)):
            x = _physical(v, each)
            want = text_ref.greedy(x, each, screen.get('blank', -1), screen.get('merge_repeated', True))
            got = text.greedy(x, TextScreen(layout=each, **screen))
            assert isinstance(got, Text)
            _same(got, want, '{} {}'.format(v.tolist(), each))
            _filler_behind_the_lengths(got)
        return want

    def one_hot(winners, C):
        v = np.zeros((len(winners), C), np.float32)
        v[np.arange(len(winners)), winners] = 1
        return v

    def read(v, **screen):
        want = both(v, None, **screen)
        length = max(int(want.lengths[0]), 0)
        return ''.join('abcdefgh'[s] for s in want.symbols[0, :length]), want.steps[0, :length].tolist(), int(want.lengths[0])

    a, b, c, _ = 0, 1, 2, 3
    seq = [a, a, _, a, b, b, _, _, c]
    assert read(one_hot(seq, 4)) == ('aabc', [0, 3, 4, 8], 4)                       # a repeat across a blank emits twice
    assert read(one_hot(seq, 4), merge_repeated=False) == ('aaabbc', [0, 1, 3, 4, 5, 8], 6)
    assert read(one_hot([_, _, _], 4)) == ('', [], 0)                               # an empty string is an answer ...
    v = one_hot(seq, 4)
    v[5, 0] = NAN
    assert read(v) == ('', [], -1) and read(v, merge_repeated=False) == ('', [], -1)      # ... and not a void row: one NaN anywhere voids
    v = one_hot(seq, 4)
    v.view(np.uint32)[8, 3] = 0xFFC00001                                            # (a negative NaN with a payload, not the winner's class)
    assert read(v)[2] == -1
    want = both(np.stack([one_hot(seq, 4), v]))                                     # the void row beside a good one
    assert want.lengths.tolist() == [4, -1] and (want.symbols[1] == -1).all() and (_bits(want.scores)[1] == QUIET).all() and (want.steps[1] == -1).all()
    # the blank first, in the middle and last: the same winners, another class dropped
    seq = [1, 1, 0, 2, 2, 3, 3, 0]
    assert read(one_hot(seq, 4), blank=0) == ('bcd', [0, 3, 5], 3) and read(one_hot(seq, 4), blank=2) == ('bada', [0, 2, 5, 7], 4)
    assert read(one_hot(seq, 4), blank=-1) == ('baca', [0, 2, 3, 7], 4) == read(one_hot(seq, 4), blank=3) and read(one_hot(seq, 4), blank=-4) == ('bcd', [0, 3, 5], 3)
    # ties and zeros of either sign go to the lower class; the score is the winner's own bits
    assert read([[0.5, 0.5, 0.5], [0.1, 0.7, 0.7]]) == ('ab', [0, 1], 2)
    want = both([[-0.0, 0.0, -1.0], [-1.0, 0.0, -0.0]], None)
    assert want.symbols[0, :2].tolist() == [0, 1] and _bits(want.scores)[0, :2].tolist() == [0x80000000, 0]
    assert read([[-np.inf, -np.inf], [np.inf, np.inf]], blank=1, merge_repeated=False) == ('aa', [0, 1], 2)
    assert read([[NAN, 1.0]], blank=0)[2] == -1                                     # the NaN wins the timestep, whatever the blank
    # T == 1 and C == 2
    assert read([[0.0, 1.0, 0.5]]) == ('b', [0], 1) and read([[0.0, 0.5, 1.0]]) == ('', [], 0)
    assert read([[1, 0], [1, 0], [0, 1], [1, 0]]) == ('aa', [0, 3], 2) and read([[1, 0], [1, 0], [0, 1], [1, 0]], blank=0) == ('b', [2], 1)
    # strings: None for a void row, ValueError outside the alphabet
    want = both(np.stack([one_hot([a, a, _, a, b, b, _, _, c], 4), v, one_hot([_] * 9, 4)]))
    assert text.strings(want, 'xyz') == ['xxyz', None, ''] and text.strings(want, ['A', 'B', 'C', '-']) == ['AABC', None, '']
    with pytest.raises(ValueError, match='strings: row 0 holds symbol 2'):
        text.strings(want, 'xy')
    # anything but float32 of rank 3 (or 4 with a unit axis), T <= 4096, C >= 2 and a layout is refused
    for bad in (np.zeros((2, 3), np.float32), np.zeros((1, 2, 3, 4), np.float32), np.zeros((1, 2, 3), np.float64), np.zeros((1, 4097, 2), np.float32),
                np.zeros((1, 3, 1), np.float32), np.zeros((0, 3, 2), np.float32)):
        with pytest.raises(ValueError, match='greedy'):
            text.greedy(bad, TextScreen(layout='NTC'))
    for bad in ('NTC', None, False, TextScreen(), TextScreen(layout='CTN'), TextScreen(1.0, True, 'NTC'), TextScreen(True, True, 'NTC'), TextScreen(3, True, 'NTC'),
                TextScreen(-4, True, 'NTC'), TextScreen(0, 1, 'NTC')):
        with pytest.raises(ValueError, match='greedy'):
            text.greedy(np.zeros((1, 2, 3), np.float32), bad)
    same = text.greedy(np.ones((2, 5, 1, 3), np.float32), TextScreen(layout='NTC')), text.greedy(np.ones((2, 5, 3, 1), np.float32), TextScreen(layout='NTC'))
    for got in same:                                                                # a fourth axis of extent 1 is dropped
        _same(got, text_ref.greedy(np.ones((2, 5, 3), np.float32), 'NTC'), 'unit axis')


@pytest.mark.parametrize('shape', SHAPES)
def test_greedy_agrees_with_the_loops(shape):
    from pyopenvino_amd import text
    for what, layout, x, blank, merge, want in _cases(shape):
        got = text.greedy(x, _screen(layout, blank, merge))
        _same(got, want, what)
        _filler_behind_the_lengths(got)
    n, T, C = shape
    v = np.random.default_rng(3).standard_normal((n, T, C, 3)).astype(np.float32)[:, :, :, 1]        # not contiguous: the same answer
    for layout in LAYOUTS:
        x = v.transpose({'TNC': (1, 0, 2), 'NTC': (0, 1, 2), 'NCT': (0, 2, 1)}[layout])
        assert not x.flags.c_contiguous or x.size <= max(x.shape)
        _same(text.greedy(x, _screen(layout, 0)), text_ref.greedy(np.ascontiguousarray(x), layout, 0), 'strided {}'.format(layout))


def test_argument_rules(tmp_path, monkeypatch):
    """Every refusal is a ValueError('text: ...') raised before anything is staged or launched: this test runs where there is no device."""
    from pyopenvino_amd import Gallery, GalleryMatch, TextScreen, answers as answers_module, detections as detections_rule, text as rule
    n = 4
    ex, net, name, out_name = _text_head(tmp_path, n, requests=2)
    x = np.zeros((n, 1, 28, 28), np.float32)
    req = ex.requests[0]
    others = ('top_k', 'detections', 'matches', 'keypoints', 'segments', 'maxima')
    starts = (lambda s, **kw: ex.infer({name: x}, text=s, **kw), lambda s, **kw: req.start_async({name: x}, text=s, **kw),
              lambda s, **kw: ex.requests[1].infer({name: x}, text=s, **kw), lambda s, **kw: ex.start_async(1, {name: x}, text=s, **kw),
              lambda s, **kw: req.infer({name: x}, *(kw.get(k) for k in others), s),
              lambda s, **kw: req.start_async({name: x}, *(kw.get(k) for k in others), s),
              lambda s, **kw: ex.infer({name: x}, False, *(kw.get(k) for k in others), s),
              lambda s, **kw: ex.start_async(0, {name: x}, *(kw.get(k) for k in others), s))       # the keyword stands last

    def refused(match, s, network=ex, starts=starts, **kw):
        for start in starts:
            with pytest.raises(ValueError, match=match) as e:
                start(s, **kw)
            assert str(e.value).startswith('text: '), str(e.value)
        for r in network.requests:
            assert not r._in_flight and not r._asks and not r.runner.answers.blocks and not r.runner.host_inputs.slots and r.runner._pending is None

    refused('no Result named', {'text/nope': True})
    refused('no Result named', {out_name: True, 'nope': TextScreen()})
    for bad in ('NTC', [True], (True,), False, np.bool_(True), 0.5, 1, b'1', TextScreen, (-1, True, None)):
        refused('a TextScreen or True', bad)
        refused('a TextScreen or True', {out_name: bad})
    refused('a TextScreen or True', {out_name: None})
    for bad in (1.0, '1', None, True, np.bool_(False), [0]):
        refused('blank is an int', TextScreen(bad))
        refused('blank is an int', {out_name: TextScreen(blank=bad)})
    for bad in (676, -677, 1 << 40):                            # read as 'NTC': C = 676
        refused('blank is an int in -C .. C - 1 = -676 .. 675', TextScreen(bad))
        refused('blank is an int in -C .. C - 1 = -676 .. 675', {out_name: TextScreen(bad, False)})
    refused('blank is an int in -C .. C - 1 = -32 .. 31', TextScreen(32, layout='NCT'))
    for bad in (1, 0, None, 'yes', np.int64(1)):
        refused('merge_repeated is a bool', TextScreen(merge_repeated=bad))
        refused('merge_repeated is a bool', {out_name: TextScreen(0, bad)})
    for bad in ('CTN', 'ntc', 1, ('N', 'T', 'C'), b'NTC'):
        refused('layout', TextScreen(layout=bad))
        refused('layout', {out_name: TextScreen(layout=bad)})
    ex.comm = types.SimpleNamespace(world=2, rank=0)
    try:
        refused('sharded', True)
        refused('sharded', {out_name: TextScreen(0)})
    finally:
        ex.comm = None
    ports = [r.runner.ienet.outputs[0]['input'][0] for r in ex.requests]       # (every request has its own copy of the graph)
    for port in ports:
        port['precision'] = 'FP16'
    try:
        refused('FP32 Results only', {out_name: True})
        refused('no FP32 Result', True)
    finally:
        for port in ports:
            port['precision'] = 'FP32'
    declared = [port['dims'] for port in ports]

    def with_dims(dims):
        for port in ports:
            port['dims'] = dims

    try:
        # another rank, no unit axis, another batch, T beyond 4096, one class, n * T * C = 2^31
        for dims in ((n, 32), (n, 32, 26, 26), (n, 1, 1, 32, 676), (2, 32, 676), (n, 4097, 5), (4097, n, 5), (n, 32, 1), (n, 32, 1, 1), (n, 4096, 1 << 17)):
            with_dims(dims)
            refused('has shape .*: not rank 3, or 4 with an axis of extent 1, with the batch n = 4, 1 <= T <= 4096, C >= 2 and n \\* T \\* C < 2\\^31', {out_name: True})
            refused('no FP32 Result', True)
        with_dims((n, 32, 676))                                 # the batch stands first: not (T, n, C), and as (n, C, T) the time axis is too long
        refused('has shape .* as \'TNC\'', {out_name: TextScreen(layout='TNC')})
        refused('no FP32 Result .* as \'TNC\'', TextScreen(layout='TNC'))
        with_dims((n, 32, 4097))
        refused('has shape .* as \'NCT\'', {out_name: TextScreen(layout='NCT')})
        with_dims((n, n, 676))                                  # both leading axes are the batch
        refused('reads as \'TNC\' and as \'NTC\': say which with TextScreen\\(layout=...\\)', {out_name: True})
        refused('no FP32 Result .* whose layout can be inferred', True)
        for layout in LAYOUTS:
            assert rule.checked(ex.requests[0].runner.ienet, TextScreen(layout=layout), False) == {out_name: TextScreen(n - 1 if layout == 'NCT' else 675, True, layout)}
        # the shapes the issue names, with the batch where the layout wants it
        for dims, want in (((30, n, 37), ('TNC', n, 30, 37)), ((n, 26, 37), ('NTC', n, 26, 37)), ((n, 71, 1, 88), ('NTC', n, 71, 88)), ((n, 26, 37, 1), ('NTC', n, 26, 37)),
                           ((26, n, 1, 37), ('TNC', n, 26, 37)), ((n, 1, 1, 37), ('NTC', n, 1, 37)), ((n, 4096, 2), ('NTC', n, 4096, 2))):
            with_dims(dims)
            assert rule.steps_of(dims, None, n) == want
            assert rule.checked(ex.requests[0].runner.ienet, True, False) == {out_name: TextScreen(want[3] - 1, True, want[0])}
        # one Result under two keywords: the later keyword speaks and names the earlier.  (n, 32, 1, 676) is a stack of heatmaps and of
        # class maps as well as 32 timesteps; no Result passes the shape rules of the other three, so their checks are stubbed
        with_dims((n, 32, 1, 676))
        clash = 'Result {!r} is asked for with {} as well'
        for keyword in ('keypoints', 'segments', 'maxima'):
            for value in (True, 0.5, {out_name: True}):
                refused(clash.format(out_name, keyword), True, **{keyword: value})
                refused(clash.format(out_name, keyword), {out_name: TextScreen(0)}, **{keyword: value})
        gal = Gallery(np.ones((3, 7), np.float32))
        for keyword, module, stub, value in (('top_k', answers_module.top_k_rule, lambda ienet, top_k, sharded: {out_name: 1}, 1),
                                             ('detections', answers_module.detections_rule, lambda ienet, d, sharded: {out_name: detections_rule.DetectionScreen()}, 0.5),
                                             ('matches', answers_module.gallery_rule, lambda ienet, matches, sharded: {out_name: GalleryMatch(gal, 1, None)}, gal)):
            with monkeypatch.context() as patched:
                patched.setattr(module, 'checked', stub)
                refused(clash.format(out_name, keyword), True, **{keyword: value})
                refused(clash.format(out_name, keyword), {out_name: TextScreen(0)}, **{keyword: value})
        assert gal._dev is None
        # and the other way round nothing changed: the earlier keywords among themselves name each other as before
        with pytest.raises(ValueError, match='maxima: ' + clash.format(out_name, 'keypoints')):
            ex.infer({name: x}, keypoints=True, maxima=True, text=None)
        with pytest.raises(ValueError, match='segments: ' + clash.format(out_name, 'keypoints')):
            ex.infer({name: x}, keypoints=True, segments=True, text=True)
    finally:
        for port, dims in zip(ports, declared):
            port['dims'] = dims
    # a classifier has no timesteps; heatmaps (n, 32, 26, 26) have no unit axis
    ie_c, net_c, name_c = roi_tests._net('mnist', n)
    cls = ie_c.load_network(net_c, 'GPU', num_requests=1)
    cls_starts = (lambda s, **kw: cls.infer({name_c: x}, text=s), lambda s, **kw: cls.requests[0].start_async({name_c: x}, text=s))
    refused('no FP32 Result', True, cls, cls_starts)
    refused('has shape', {net_c.outputs[0]['name']: True}, cls, cls_starts)
    # the resolved forms: blank in 0 .. C - 1, the layout filled in
    assert TextScreen() == (-1, True, None) and rule.resolved(True) == TextScreen()
    assert rule.checked(net, None, False) == {} and rule.checked(net, {}, True) == {}
    assert rule.checked(net, True, False) == rule.checked(net, TextScreen(), False) == rule.checked(net, {out_name: True}, False) == {out_name: TextScreen(675, True, 'NTC')}
    assert rule.checked(net, TextScreen(0, False), False) == {out_name: TextScreen(0, False, 'NTC')}
    assert rule.checked(net, TextScreen(np.int64(-676), np.bool_(False)), False) == {out_name: TextScreen(0, False, 'NTC')}
    got = rule.checked(net, {out_name: TextScreen(np.int32(-2), layout='NCT')}, False)
    assert got == {out_name: TextScreen(30, True, 'NCT')} and type(got[out_name].blank) is int and type(got[out_name].merge_repeated) is bool
    assert rule.steps_of((n, 32, 676)) is None and rule.steps_of((n, 32, 676), 'NCT') == ('NCT', n, 676, 32) and rule.steps_of((n, 32, 676), 'TNC', n) is None
    assert rule.steps_of((7, 5, 1, 1), None, 7) is None         # axis 2 goes, C = 1 stays: refused
    assert rule.steps_of((1, 4096, 1 << 19), 'NTC') is None and rule.steps_of((1, 4096, (1 << 19) - 1), 'NTC') is not None


def test_answers_checked_takes_the_new_argument_last(tmp_path):
    from pyopenvino_amd import TextScreen, maxima, text as rule
    n = 4
    ex, net, name, out_name = _text_head(tmp_path, n)
    x = np.zeros((n, 1, 28, 28), np.float32)
    answers = ex.answers
    assert answers.checked({name: x}, None, None, False) == {} and answers.checked({name: x}, None, None, False, None, None, None, None) == {}
    assert answers.checked({name: x}, None, None, False, None, None, None, None, None) == {} and answers.checked({name: x}, None, None, False, text=None) == {}
    asks = answers.checked({name: x}, None, None, False, None, None, None, None, TextScreen(0, False))
    screen = TextScreen(0, False, 'NTC')
    assert set(asks) == {out_name} and isinstance(asks[out_name], rule.Ask) and asks[out_name].KEYWORD == 'text'
    assert asks[out_name] == (screen,) and asks[out_name].screen == screen      # an ask equals the plain tuple of its fields
    assert asks == answers.checked({name: x}, None, None, False, text={out_name: TextScreen(-676, False)})
    assert asks[out_name].key(out_name) == (out_name, 'NTC') == rule.Ask(TextScreen(5, True, 'NTC')).key(out_name)        # blank and merge share the blocks
    assert rule.Ask(screen._replace(layout='NCT')).key(out_name) != asks[out_name].key(out_name)
    assert asks[out_name].launch_with() == ('NTC', 0, False) and asks[out_name].bound({name: x}, {}) is asks[out_name]
    # the shorter calls answer as before: no Result of this network is a stack of heatmaps
    with pytest.raises(ValueError, match='maxima: no FP32 Result'):
        answers.checked({name: x}, None, None, False, None, None, None, True)
    with pytest.raises(ValueError, match='keypoints: no FP32 Result'):
        answers.checked({name: x}, None, None, False, None, True)
    hx, _, hname, hout = keypoints_tests._mnist_head(tmp_path, n)
    kept = hx.answers.checked({hname: x}, None, None, False, None, None, None, 0.5)
    assert set(kept) == {hout} and isinstance(kept[hout], maxima.Ask)
    with pytest.raises(ValueError, match='text: no FP32 Result'):
        hx.answers.checked({hname: x}, None, None, False, None, None, None, None, True)
    assert not answers.blocks and not ex.host_inputs.slots and ex._pending is None


def test_a_host_result_gets_the_rule_in_numpy(tmp_path):
    """A plugin set that computes on the host (the oracle's) hands wait() host arrays: the same keyword, the same rule, no device."""
    from pyopenvino_amd import Text, TextScreen
    n = 3
    x = _pixels(10, n)
    for transposed, layout in ((False, 'NTC'), (True, 'TNC')):
        ex, net, name, out_name = _text_head(tmp_path, n, requests=2, package='oracle.op_plugins', transposed=transposed)
        full = np.array(ex.infer({name: x})[out_name], copy=True)
        assert full.shape == ((32, n, 676) if transposed else (n, 32, 676)) and full.dtype == np.float32 and np.isfinite(full).all()
        for given in (True, TextScreen(0, False), TextScreen(100, True, layout)) + (() if transposed else (TextScreen(layout='NCT'),)):
            want = _want(full, given, layout)
            for got in (ex.infer({name: x}, text=given), ex.requests[1].infer({name: x}, text={out_name: given})):
                assert set(got) == {out_name} and isinstance(got[out_name], Text)
                _same(got[out_name], want, repr(given))
        assert (_want(full, True, layout).lengths > 0).all()
        assert np.array_equal(ex.infer({name: x})[out_name], full)           # and whole again without the keyword
        with pytest.raises(ValueError, match='text: .*blank is an int in -C .. C - 1'):
            ex.infer({name: x}, text=TextScreen(676))


def test_abi_declares_the_entries():
    import pyopenvino_amd
    from pyopenvino_amd import device, text
    header = open(os.path.join(helpers.REPO, 'include', 'pvhip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for entry, count in ((ENTRY, 12), (FORM, 3)):
        assert entry in device.SIGNATURES and len(device.SIGNATURES[entry][1]) == count
        m = re.search(r'\bint\s+' + entry + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S)
        assert m and len(m.group(1).split(',')) == count, entry
    assert ENTRY not in device._NOT_STATUS and FORM in device._NOT_STATUS
    joined = re.sub(r'\s*\n \*\s+', ' ', header)                               # the rule is stated there (its lines joined) ...
    docs = [re.sub(r'\s*\n\s+', ' ', doc) for doc in (text.__doc__, text_ref.__doc__)]      # ... and in both docstrings, in the same words
    for phrase in ('w(t) is the first class of timestep t in top_k\'s total order: NaN of any sign or payload first, then descending with +0.0 == -0.0, ties to the lower class',
                   'row r is void iff the winning score of any of its timesteps is NaN, that is, iff any of its T * C scores is NaN',
                   'A void row has length -1 and nothing but filler', 'An empty string (length 0) is an answer and not a void row',
                   'timestep t emits iff w(t) != blank and (merge_repeated is false, or t == 0, or w(t) != w(t - 1))',
                   'A repeat across a blank therefore emits twice: a, blank, a is aa',
                   'the emitting timesteps in ascending t fill slots 0, 1, ...: symbols = w(t), scores = the bits of v[t][w(t)], steps = t',
                   '(-1, quiet NaN, -1)'):
        assert phrase in joined, phrase
        for doc in docs:
            assert phrase in doc, phrase
    for define, value in (('PVHIP_TEXT_MAX_STEPS', text.MAX_STEPS), ('PVHIP_TEXT_MAX_BLOCKS', text.MAX_BLOCKS), ('PVHIP_TEXT_FORM_NONE', FORM_NONE),
                          ('PVHIP_TEXT_FORM_ROWS', FORM_ROWS), ('PVHIP_TEXT_FORM_PLANES', FORM_PLANES)) \
            + tuple(('PVHIP_TEXT_LAYOUT_' + layout, i) for i, layout in enumerate(LAYOUTS)):
        assert re.search(r'#define\s+{}\s+{}\b'.format(define, value), header), define
    assert (text.MAX_STEPS, text.MAX_BLOCKS) == (MAX_STEPS, MAX_BLOCKS) and text.LAYOUTS == {layout: i for i, layout in enumerate(LAYOUTS)}
    assert (text.FORM_NONE, text.FORM_ROWS, text.FORM_PLANES) == (FORM_NONE, FORM_ROWS, FORM_PLANES)
    assert re.search(r'#define\s+PVHIP_ABI_VERSION\s+19\b', header)
    lib = device.load_library()
    assert hasattr(lib, ENTRY) and hasattr(lib, FORM) and lib.pvhip_abi_version() == 19
    assert pyopenvino_amd.Text is text.Text and pyopenvino_amd.TextScreen is text.TextScreen and pyopenvino_amd.text is text
    assert {'Text', 'TextScreen', 'text'} <= set(pyopenvino_amd.__all__)
    assert pyopenvino_amd.Text._fields == ('lengths', 'symbols', 'scores', 'steps')
    assert pyopenvino_amd.TextScreen._fields == ('blank', 'merge_repeated', 'layout') and tuple(pyopenvino_amd.TextScreen()) == (-1, True, None)
    for attr in ('resolved', 'steps_of', 'checked', 'greedy', 'strings', 'Blocks', 'Ask'):
        assert hasattr(text, attr), attr
    assert text.Ask.KEYWORD == 'text'


def _form_steps(layout, c):
    """Every T after which pvhip_ctc_greedy_form changes its answer for `layout` and `c` classes."""
    from pyopenvino_amd import device
    forms = [device.call(FORM, layout, t, c) for t in range(1, 3 * MAX_STEPS)]
    return [t for t, (a, b) in zip(range(1, 3 * MAX_STEPS), zip(forms, forms[1:])) if a != b]


def test_the_form_query():
    """It needs no device, answers NONE for what the entry refuses, the form of the layout otherwise, and changes at T = 4096 alone,
    where the kernel test stands."""
    from pyopenvino_amd import device
    form = lambda layout, t, c: device.call(FORM, layout, t, c)
    assert [form(-1, 30, 37), form(3, 30, 37), form(0, 0, 37), form(1, -1, 37), form(2, 4097, 37), form(0, 30, 1), form(1, 30, 0), form(2, 30, -5),
            form(0, 1 << 20, 2)] == [FORM_NONE] * 9
    for layout, want in ((0, FORM_ROWS), (1, FORM_ROWS), (2, FORM_PLANES)):
        for c in (2, 37, 1 << 20):
            assert _form_steps(layout, c) == FORM_STEPS
            assert [form(layout, t, c) for t in (1, 2, 30, 256, 257, 4096)] == [want] * 6
    assert any(shape[1] == FORM_STEPS[0] for shape in SHAPES)


# ---------------------------------------------------------------------------------------------------------------- GPU
GUARD, SENTINEL = top_k_tests.GUARD, top_k_tests.SENTINEL


def _device_text(hip, x, layout, blank, merge, offset=0):
    """The entry on `x`, a contiguous tensor of `layout` -- `offset`: starting that many elements into a larger device tensor --, `blank`
    in 0 .. C - 1; the outputs and the scratch between sentinel words that must stay untouched, every answer word written."""
    n, T, C = text_ref.extents(x.shape, layout)
    if offset:
        src = hip.DeviceTensor.from_numpy(np.concatenate([np.full(offset, 9e9, np.float32), x.ravel(), np.full(7, 9e9, np.float32)]))
    else:
        src = hip.DeviceTensor.from_numpy(x)
    scratch = hip.DeviceTensor.empty((n * T + 2 * GUARD,), np.uint64)
    outs = [hip.DeviceTensor.empty((words + 2 * GUARD,), np.int32) for words in (n, n * T, n * T, n * T)]
    for t in outs + [scratch]:
        hip.call('pvhip_memset', ctypes.c_void_p(t.ptr), 0x7f, t.nbytes)
    hip.call(ENTRY, ctypes.c_void_p(src.ptr + 4 * offset), n, T, C, LAYOUTS.index(layout), blank, int(merge), ctypes.c_void_p(scratch.ptr + 8 * GUARD),
             *(ctypes.c_void_p(t.ptr + 4 * GUARD) for t in outs))
    keys = np.asarray(scratch)
    assert (keys[:GUARD] == 0x7f7f7f7f7f7f7f7f).all() and (keys[-GUARD:] == 0x7f7f7f7f7f7f7f7f).all(), 'a word outside the scratch was written'
    assert not (keys[GUARD:-GUARD] == 0x7f7f7f7f7f7f7f7f).any(), 'a key was not written'
    length, sym, sco, step = (np.asarray(t) for t in outs)
    for t in (length, sym, sco, step):
        assert (t[:GUARD] == SENTINEL).all() and (t[-GUARD:] == SENTINEL).all(), 'a word outside the output was written'
        assert not (t[GUARD:-GUARD] == SENTINEL).any(), 'an answer was not written'
    return text_ref.Text(length[GUARD:-GUARD].copy(), sym[GUARD:-GUARD].reshape(n, T).copy(), sco[GUARD:-GUARD].view(np.float32).reshape(n, T).copy(),
                         step[GUARD:-GUARD].reshape(n, T).copy())


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_equals_the_rule(hip, shape):
    n, T, C = shape
    for layout in LAYOUTS:
        assert hip.call(FORM, LAYOUTS.index(layout), T, C) == (FORM_PLANES if layout == 'NCT' else FORM_ROWS)
    for what, layout, x, blank, merge, want in _cases(shape):
        got = _device_text(hip, x, layout, blank % C, merge)
        _same(got, want, what)
        _filler_behind_the_lengths(got)
        if shape in OFFSET_SHAPES:                              # no row, no plane starts on a 16-byte boundary
            for offset in (1, 2, 3):
                _same(_device_text(hip, x, layout, blank % C, merge, offset), want, '{} offset {}'.format(what, offset))


@pytest.mark.gpu
def test_kernel_walks_more_rows_than_its_grid(hip):
    """(3, 3000, 5): 9000 (r, t) rows against the 4 * PVHIP_TEXT_MAX_BLOCKS the rows form's grid takes in one trip -- the stride loop takes
    a second --, and in 'NCT' 2250 quads of timesteps on nine workgroups (that form's grid is not capped: there is no constant to stand
    above).  The last timesteps of every row carry a string of their own.  The reference is text.greedy, which the tests above hold to
    the loops."""
    from pyopenvino_amd import text
    n, T, C = shape = (3, 3000, 5)
    assert n * T > ROWS_PER_BLOCK * MAX_BLOCKS == ROWS_PER_BLOCK * text.MAX_BLOCKS
    rng = np.random.default_rng(23)
    v = rng.standard_normal(shape).astype(np.float32)
    v[:, -3:, :] = 0
    v[:, -3, 1], v[:, -2, 4], v[:, -1, 2] = 5, 5, 5
    for layout in LAYOUTS:
        x = _physical(v, layout)
        for blank, merge in ((4, True), (0, False), (2, True)):
            want = text.greedy(x, _screen(layout, blank, merge))
            got = _device_text(hip, x, layout, blank, merge)
            _same(got, want, '{} {} {}'.format(layout, blank, merge))
            _filler_behind_the_lengths(got)
            assert (want.lengths > 1000).all() and (want.steps[np.arange(n), want.lengths - 1] >= T - 2).all()


@pytest.mark.gpu
def test_entry_rejects_what_it_cannot_do(hip):
    t = hip.DeviceTensor.from_numpy(np.arange(512, dtype=np.float32))
    o = hip.DeviceTensor.empty((4096,), np.int32)
    at = lambda words: ctypes.c_void_p(o.ptr + 4 * words)
    good = [ctypes.c_void_p(t.ptr), 2, 8, 16, 1, 15, 1, at(0), at(1024), at(1100), at(1200), at(1300)]
    hip.call(ENTRY, *good)
    bads = [(0, None)] + [(i, None) for i in range(7, 12)]                                  # a null pointer
    bads += [(0, ctypes.c_void_p(t.ptr + 2)), (7, ctypes.c_void_p(o.ptr + 4))] + [(i, ctypes.c_void_p(o.ptr + 4802)) for i in range(8, 12)]      # off their boundaries
    bads += [(i, bad) for i in (1, 2) for bad in (0, -1)] + [(3, 1), (3, 0), (3, -1), (2, 4097)]     # n, t < 1, c < 2, t > 4096
    bads += [(4, 3), (4, -1), (5, 16), (5, -1), (6, 2), (6, -1)]                            # layout unknown, blank outside 0 .. c - 1, merge neither 0 nor 1
    for i, bad in bads:
        args = list(good)
        args[i] = bad
        with pytest.raises(hip.PvhipError):
            hip.call(ENTRY, *args)
    for n, T, C in ((1 << 19, 4096, 2), (1, 4096, 1 << 19), (1 << 30, 1, 2), (2, 1, 1 << 30)):
        args = list(good)                                       # n * t * c >= 2^31
        args[1:4], args[5] = (n, T, C), 0
        with pytest.raises(hip.PvhipError):
            hip.call(ENTRY, *args)
    hip.synchronize()
    x = np.arange(256, dtype=np.float32).reshape(2, 8, 16) % 7       # the device is still usable
    for layout in LAYOUTS:
        _same(_device_text(hip, x, layout, 6, True), text_ref.greedy(x, layout, 6, True), 'after the refusals')


def _on_device(hip, req, out_name):
    """The Result the request's last pass left: still a device tensor."""
    G = req.runner.ienet.G
    (value,) = [G.nodes[nid]['result'] for nid, result in req.runner.ienet.find_node_by_type('Result') if result == out_name]
    assert isinstance(value, hip.DeviceTensor)
    return np.asarray(value)


@pytest.mark.gpu
def test_public_path(hip, tmp_path):
    """mnist's first layer reshaped to (3, 32, 676) and, in a second network, transposed to (32, 3, 676): text= is the rule on the
    request's own full Result in every form of the value, named and unnamed -- True infers 'NTC' and 'TNC', 'NCT' reads the first as 676
    timesteps of 32 classes, where ReLU's exact zeros tie --; a second call with another blank and merge allocates nothing; three passes on
    a device-resident input, the third replayed."""
    import test_answer_checks as order_tests
    from pyopenvino_amd import Text, TextScreen
    n = 3
    x = _pixels(10, n)
    for transposed, layout in ((False, 'NTC'), (True, 'TNC')):
        ex, net, name, out_name = _text_head(tmp_path, n, requests=2, transposed=transposed)
        req = ex.requests[0]
        full = np.array(req.infer({name: x})[out_name], copy=True)
        assert full.shape == ((32, n, 676) if transposed else (n, 32, 676)) and full.dtype == np.float32 and np.isfinite(full).all()
        plain = TextScreen(100, False)
        values = [True, TextScreen(), TextScreen(0), plain, TextScreen(-1, True, layout)] + ([] if transposed else [TextScreen(layout='NCT'), TextScreen(0, False, 'NCT')])
        for given in values + [{out_name: v} for v in values]:
            got = req.infer({name: x}, text=given)
            assert set(got) == {out_name} and isinstance(got[out_name], Text)
            _same(got[out_name], _want(full, given[out_name] if isinstance(given, dict) else given, layout), repr(given))
            _filler_behind_the_lengths(got[out_name])
        default = _want(full, True, layout)
        assert default.symbols.shape == (n, 32) and len(set(default.lengths.tolist())) > 1 and (default.lengths > 0).all()      # differing lengths
        assert not np.array_equal(default.lengths, _want(full, TextScreen(-1, False), layout).lengths)                          # the merge drops steps
        if not transposed:
            planes = _want(full, TextScreen(layout='NCT'), layout)
            rows = full.transpose(0, 2, 1)                      # (n, 676, 32): a timestep's best score stands in two classes somewhere
            assert planes.symbols.shape == (n, 676) and ((rows == rows.max(axis=2, keepdims=True)).sum(axis=2) > 1).any()
        _same(ex.infer({name: x}, text=True)[out_name], default, 'the network\'s own infer()')
        _same(ex.requests[1].infer({name: x}, None, None, None, None, None, None, plain)[out_name], _want(full, plain, layout), 'the second request, positionally')
        assert np.array_equal(ex.infer({name: x})[out_name], full)              # and whole again without the keyword
        assert set(req.runner.answers.blocks) == {(out_name, layout)} | (set() if transposed else {(out_name, 'NCT')})
        # another blank and merge: the same blocks, nothing allocated
        real_call, issued = hip.call, []
        hip.call = lambda entry, *args: (issued.append(entry), real_call(entry, *args))[1]
        try:
            got = req.infer({name: x}, text=TextScreen(7, False))[out_name]
        finally:
            hip.call = real_call
        _same(got, _want(full, TextScreen(7, False), layout), 'another blank')
        assert issued.count(ENTRY) == 1 and not set(order_tests.ALLOCATIONS) & set(issued[issued.index(ENTRY):])
        assert len(req.runner.answers.blocks) == (1 if transposed else 2)
        # the same device-resident tensor: eager, eager, replayed; identical answers, and the Result stays on the device
        xd = hip.DeviceTensor.from_numpy(x)
        for given in (True, plain):
            other, _, _, _ = _text_head(tmp_path, n, transposed=transposed)
            answers = []
            for call in range(3):
                other.requests[0].start_async({name: xd}, text=given)
                assert (other.requests[0]._replayed is not None) == (call == 2), call
                answers.append(other.requests[0].wait()[out_name])
                _same(answers[-1], _want(full, given, layout), '{} pass {}'.format(given, call))
                helpers.assert_bit_exact(_on_device(hip, other.requests[0], out_name), full, 'the Result behind pass {}'.format(call))
            for later in answers[1:]:
                assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(answers[0], later))
            assert len(other.answers.blocks) == 1
            other.release_device_state()
            assert not other.answers.blocks


@pytest.mark.gpu
def test_the_launch_order_behind_the_pass(hip, tmp_path):
    """What test_answer_checks pins for the other kinds: select, the entry once (its two launches are one call), one event, select;
    wait() makes exactly one copy; no pass after the first allocates -- alone and beside top_k of another Result."""
    import test_answer_checks as order_tests
    from pyopenvino_amd import TextScreen
    n = 2
    x = hip.DeviceTensor.from_numpy(_pixels(20, n))
    for asked in (dict(text=True), dict(text=TextScreen(0, False, 'NCT'))):
        ex, _, name, out_name = _text_head(tmp_path, n)         # (a request that has not recorded yet)
        got = order_tests._same_answers(order_tests._passes(hip, ex.requests[0], {name: x}, asked, [ENTRY], [1]), out_name)
        T = 676 if asked['text'] is not True else 32
        assert got.lengths.shape == (n,) and got.symbols.shape == (n, T) and got.steps.shape == (n, T) and (got.lengths > 0).all()
    two, net, name, out_name = _text_head(tmp_path, n, whole=True)
    (rows,) = [out['name'] for out in net.outputs if out['name'] != out_name]
    answers = order_tests._passes(hip, two.requests[0], {name: x}, dict(top_k={rows: 3}, text={out_name: True}), ['pvhip_topk_rows_f32', ENTRY], [1, 1])
    assert order_tests._same_answers(answers, rows).indices.shape == (n, 3) and order_tests._same_answers(answers, out_name).symbols.shape == (n, 32)


@pytest.mark.gpu
def test_requests_in_flight(hip, tmp_path):
    """Two requests at batch 3, three steps, another input every time, the keyword cycling through True, a named TextScreen and None per
    request and step: all started, then all waited for; every answer is the rule (text.greedy, which the tests above hold to the loops)
    on that input's synchronous single-request Result."""
    from pyopenvino_amd import TextScreen, text
    B, R, steps = 3, 2, 3
    ex, net, name, out_name = _text_head(tmp_path, B, requests=R)
    single, _, _, _ = _text_head(tmp_path, B)
    xs = [[_pixels(3000 + 100 * step + 10 * r, B) for r in range(R)] for step in range(steps)]
    fulls = [[np.array(single.infer({name: x})[out_name], copy=True) for x in row] for row in xs]
    assert len({f.tobytes() for row in fulls for f in row}) == R * steps
    plain = TextScreen(0, False, 'NCT')
    kinds = (True, {out_name: plain}, None)
    seen = set()
    for step in range(steps):
        asked = [(r + step) % 3 for r in range(R)]
        for r in range(R):
            ex.start_async(r, {name: xs[step][r]}, text=kinds[asked[r]])
        for r in (reversed(range(R)) if step % 2 else range(R)):
            res = ex.wait(r)[out_name]
            seen.add((r, asked[r]))
            if asked[r] == 2:
                helpers.assert_bit_exact(res, fulls[step][r], 'step {} request {}'.format(step, r))
            else:
                _same(res, text.greedy(fulls[step][r], plain if asked[r] else TextScreen(layout='NTC')), 'step {} request {} kind {}'.format(step, r, asked[r]))
    assert len(seen) == R * 3                                 # every request gave every kind of answer


@pytest.mark.gpu
def test_cascade_rows_behind_count_are_void(hip, tmp_path):
    """GoogLeNet's first Convolution + bias + ReLU at batch 8, (8, 64, 112, 112), fed DetectedRois(frames, a records array) with fewer
    survivors than rows and read with TextScreen(layout='NCT'): 112 * 112 timesteps are more than 4096, so a Reshape in the IR declares
    the Result (8, 256, 3136), the smallest split of the planes that fits.  The rows behind `count` are NaN rows and come back with
    length -1 and all filler; the rows before it are the rule (text.greedy) on the full Result of the same feed; and detected_rois()
    still reads its table."""
    from pyopenvino_amd import DetectedRois, IECore, TextScreen, text
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
    xml = os.path.join(str(tmp_path), 'googlenet_text.xml')
    blob = _with_text_chain(os.path.join(MODELS, 'googlenet-v1.xml'), xml, top_k_tests._blob(11), None, False, [0, 256, 3136])
    tree = ET.parse(xml)                                        # only the chain behind the first ReLU stays
    layers, edges = tree.getroot().find('layers'), tree.getroot().find('edges')
    by_id = {int(layer.get('id')): layer for layer in layers}
    relu = min(i for i, layer in by_id.items() if layer.get('type') == 'ReLU')
    chain = {i for i, layer in by_id.items() if layer.get('name').startswith('text')}
    assert all(int(e.get('from-layer')) <= relu for e in edges if int(e.get('to-layer')) <= relu)
    for e in [e for e in edges if not (int(e.get('to-layer')) <= relu or int(e.get('to-layer')) in chain)]:
        edges.remove(e)
    for i, layer in by_id.items():
        if i > relu and i not in chain:
            layers.remove(layer)
    tree.write(xml)
    ie = IECore(plugin_package=keypoints_tests.HIP)
    net = ie.read_network(xml, weights=blob)
    net.set_batch(n)
    name, out_name = net.inputs[0]['name'], net.outputs[0]['name']
    assert out_name == 'text' and tuple(int(d) for d in net.outputs[0]['input'][0]['dims']) == (n, 256, 3136)
    det_tests._declare(net, name, kind, mean=roi_tests._mean())
    ex = ie.load_network(net, 'GPU', num_requests=1)
    req = ex.requests[0]
    full = np.array(req.infer({name: DetectedRois(frames, rec, min_confidence=conf)})[out_name], copy=True)
    assert full.shape == (n, 256, 3136)
    assert np.isfinite(full[:want.count]).all() and (_bits(full[want.count:]) == QUIET).all()
    screen = TextScreen(0, layout='NCT')
    got = req.infer({name: DetectedRois(frames, rec, min_confidence=conf)}, text=screen)[out_name]
    _same(got, text.greedy(full, screen), 'cascade')
    _filler_behind_the_lengths(got)
    assert got.symbols.shape == (n, 3136) and (got.lengths[:want.count] > 0).all() and (got.lengths[want.count:] == -1).all()
    assert (got.symbols[want.count:] == -1).all() and (got.steps[want.count:] == -1).all() and (_bits(got.scores)[want.count:] == QUIET).all()
    det_tests._same(req.detected_rois(name), want, 'with text')
