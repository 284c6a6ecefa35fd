"""Records tests/golden/answer_checks.json: what ``Answers.checked`` made of every call of the matrix below, as it stood before the
kinds of answer were put behind one Ask protocol -- run it on the commit "Heatmap peaks on the device: infer(..., keypoints=...)"
(``python tests/golden/make_answer_checks.py``); tests/test_answer_checks.py holds checked() to what it wrote.  No device is needed: the
built library must only exist.

A case is (network, feed, the four keyword arguments, sharded, stubs); its key is those joined by '|', its value either
{'error': [exception type, full text]} or {'asks': {Result name: [ask class name, fields]}} -- a Gallery written as its repr, an
InputFormat as its input's name, callables left out.  `stubs` = {keyword: {Result name: resolved value}} replaces that kind's own
``checked`` for the call, as tests/test_keypoints.py does: no Result passes the shape rules of two kinds but an embedding's rows
(top_k and matches) and a detector's records at batch 1 (detections and keypoints), so the other clash texts are reached only so.

The networks, all at batch 4 but 'ssd1': 'googlenet' (rows of 1000), 'mnist' (rows of 10), 'ssd' (the SSD IR, U8 / NHWC frames with a
resize), 'ssd_fit' (the same with resize_fit LETTERBOX), 'ssd1' (batch 1), 'heatmap' (mnist's first Convolution + ReLU as a Result
(4, 32, 26, 26)), 'two' (mnist with those heatmaps as a second Result) and 'mnist_f16' / 'ssd_f16' / 'heatmap_f16', whose Results are
declared FP16."""
import itertools
import json
import os
import sys
import tempfile
import xml.etree.ElementTree as ET

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
MODELS = os.path.join(REPO, 'models')
KEYWORDS = ('top_k', 'detections', 'matches', 'keypoints')
N = 4
TABLE = np.array([(0, 0, 0, 40, 48), (1, 0, 0, 40, 48), (0, 24, 0, 40, 48), (1, 24, 0, 40, 48)], np.int32)     # 4 tiles of 2 (48, 64) frames
RECORDS = np.array([(0, 1, 0.9, 0.1, 0.1, 0.6, 0.7), (1, 2, 0.8, 0.2, 0.0, 1.0, 0.9)], np.float32)


def _two_heads(tmp):
    """mnist's IR with a second Result, 'heatmaps', on the ReLU behind its first Convolution: the path of the new xml."""
    tree = ET.parse(os.path.join(MODELS, 'mnist.xml'))
    layers, edges = tree.getroot().find('layers'), tree.getroot().find('edges')
    by_id = {int(layer.get('id')): layer for layer in layers}
    relu = min(i for i, layer in by_id.items() if layer.get('type') == 'ReLU')
    out_port = by_id[relu].find('output').find('port')
    new = max(by_id) + 1
    result = ET.SubElement(layers, 'layer', {'id': str(new), 'name': 'heatmaps', 'type': 'Result', 'version': 'opset1'})
    port = ET.SubElement(ET.SubElement(result, 'input'), 'port', {'id': '0', 'precision': 'FP32'})
    for dim in out_port.findall('dim'):
        ET.SubElement(port, 'dim').text = dim.text
    ET.SubElement(edges, 'edge', {'from-layer': str(relu), 'from-port': out_port.get('id'), 'to-layer': str(new), 'to-port': '0'})
    path = os.path.join(tmp, 'mnist_two_heads.xml')
    tree.write(path)
    return path


def networks(tmp):
    """{network name: (Executable_Network, input name, [Result names])}, loaded without a device; `tmp`: a directory for the cut IRs."""
    for path in (REPO, os.path.dirname(HERE)):
        if path not in sys.path:
            sys.path.insert(0, path)
    import test_keypoints
    from pyopenvino_amd import IECore, synth
    ie = IECore(plugin_package='pyopenvino_amd.op_plugins')
    blobs = {model: synth.synth_weights(os.path.join(MODELS, model + '.xml'), 7) for model in ('googlenet-v1', 'ssd_mobilenet_v1_coco')}
    mnist = os.path.join(MODELS, 'mnist.bin')

    def load(xml, weights, batch=N, frames=False, fit=None, f16=False):
        net = ie.read_network(xml if os.path.isabs(xml) else os.path.join(MODELS, xml + '.xml'), weights=weights)
        if batch != 1:
            net.set_batch(batch)
        name = net.inputs[0]['name']
        if frames:
            info = net.input_info[name]
            info.precision, info.layout = 'U8', 'NHWC'
            info.preprocess_info.resize_algorithm = 'RESIZE_BILINEAR'
            info.preprocess_info.reverse_channels = True
            if fit is not None:
                info.preprocess_info.resize_fit = fit
        ex = ie.load_network(net, 'GPU', num_requests=1)
        if f16:
            for out in ex.ienet.outputs:
                out['input'][0]['precision'] = 'FP16'
        return ex, name, [out['name'] for out in net.outputs]

    ssd = 'ssd_mobilenet_v1_coco'
    return {'googlenet': load('googlenet-v1', blobs['googlenet-v1']), 'mnist': load('mnist', mnist), 'mnist_f16': load('mnist', mnist, f16=True),
            'ssd': load(ssd, blobs[ssd], frames=True), 'ssd_fit': load(ssd, blobs[ssd], frames=True, fit='LETTERBOX'),
            'ssd1': load(ssd, blobs[ssd], batch=1, frames=True), 'ssd_f16': load(ssd, blobs[ssd], frames=True, f16=True),
            'heatmap': load(test_keypoints._heatmap_head('mnist', tmp), mnist),
            'heatmap_f16': load(test_keypoints._heatmap_head('mnist', tmp), mnist, f16=True), 'two': load(_two_heads(tmp), mnist)}


def feeds():
    """{feed name: what the network's input is fed}; 'absent' feeds nothing at all."""
    from pyopenvino_amd import DetectedRois, RoiInput, WarpInput
    frames = np.zeros((2, 48, 64, 3), np.uint8)
    return {'array': np.zeros((N, 300, 300, 3), np.uint8), 'absent': None, 'roi': RoiInput(frames, TABLE),
            'detected': DetectedRois(frames, RECORDS, images=2), 'warp': WarpInput(frames, np.array([np.eye(3)[:2]] * N), [0, 1, 0, 1])}


def _label(v):
    """A value of the matrix as a part of a key: its repr, but for numpy's scalars, whose repr differs from version to version."""
    if isinstance(v, dict):
        return '{' + ', '.join('{}: {}'.format(k, _label(e)) for k, e in v.items()) + '}'
    if isinstance(v, np.generic):
        return '{}({})'.format(type(v).__name__, v)
    if isinstance(v, tuple) and hasattr(v, '_fields'):
        return '{}({})'.format(type(v).__name__, ', '.join(_label(e) for e in v))
    return repr(v)


def cases():
    """(key, network, feed, {keyword: value}, sharded, stubs) of every case; R / E / H / D stand for the network's own Result name."""
    from pyopenvino_amd import DetectionScreen, GalleryMatch, PeakScreen, RegionScreen, TiledScreen
    out, seen = [], set()

    def case(net, feed='array', sharded=False, stubs=None, **given):
        assert set(given) <= set(KEYWORDS)
        key = '|'.join([net, feed] + ['{}={}'.format(k, _label(given[k])) for k in KEYWORDS if given.get(k) is not None]
                       + (['sharded'] if sharded else []) + (['stub ' + _label(stubs)] if stubs else []))
        if key not in seen:                 # (the lists below overlap here and there)
            seen.add(key)
            out.append((key, net, feed, given, sharded, stubs or {}))

    R, E, D, H = 'prob/sink_port_0', 'Func/StatefulPartitionedCall/output/_11:0', 'detection_boxes:0', 'heatmaps'       # googlenet's, mnist's, the SSD's and the heatmap networks' Result
    g10, g7 = GALLERIES
    # ---- nothing asked
    for net in ('googlenet', 'mnist', 'ssd', 'heatmap', 'two'):
        case(net)
        case(net, sharded=True)
        for keyword in KEYWORDS:
            case(net, **{keyword: {}})
            case(net, sharded=True, **{keyword: {}})
    # ---- top_k alone
    for k in (5, 1, 64, np.int64(3), np.int32(7), 0, 65, -1, 1001, 'x', 5.0, True, None, [5], (5,)):
        case('googlenet', top_k=k)
        case('googlenet', top_k={R: k})
    for k in (5, 10, 11, 0, 'x'):
        case('mnist', top_k=k)
        case('mnist', top_k={E: k})
    for k in (5, {R: 5}, {'nope': 5}, {R: 5, 'nope': 'x'}, {'nope': 5, 'other': 5}):
        case('googlenet', top_k=k, sharded=True)
        case('googlenet', top_k=k)
    for net, name in (('ssd', D), ('heatmap', H), ('mnist_f16', E)):       # another shape; another precision
        for k in (5, {name: 5}, {name: 'x'}, {name: 0}, {'nope': 5}):
            case(net, top_k=k)
            case(net, top_k=k, sharded=True)
    for k in (5, 33, {E: 5}, {H: 5}, {E: 5, H: 5}, {H: 5, E: 'x'}):
        case('two', top_k=k)
    # ---- detections alone
    screens = (0.5, 0, 1, np.float32(0.25), DetectionScreen(), DetectionScreen(0.25, (480, 640), [5, 0, 3], (2, 3), 7), DetectionScreen(max_per_image=1000),
               DetectionScreen(labels=[]), DetectionScreen(labels=range(64)), DetectionScreen(labels=range(65)), DetectionScreen(labels=[1.5]),
               DetectionScreen(labels=5), 'x', True, None, float('nan'), float('inf'), DetectionScreen(min_confidence='x'),
               DetectionScreen(min_size=(0, 1)), DetectionScreen(min_size=3), DetectionScreen(frame_size=(0, 5)), DetectionScreen(frame_size=(1 << 24, 1)),
               DetectionScreen(frame_size=((1 << 24) + 1, 1)), DetectionScreen(max_per_image=0), DetectionScreen(max_per_image=1.5),
               TiledScreen(), RegionScreen())
    for s in screens:
        if s is not None:
            case('ssd', detections=s)
        case('ssd', detections={D: s})
    for s in (0.5, {D: 0.5}, {'nope': 0.5}, {D: float('nan')}, {D: 0.5, 'nope': 'x'}, TiledScreen(), {D: RegionScreen()}):
        case('ssd', detections=s, sharded=True)
        case('ssd1', detections=s)
        case('ssd_f16', detections=s)
        case('ssd_fit', detections=s)
    for net, name in (('googlenet', R), ('mnist', E), ('heatmap', H), ('two', H)):
        for s in (0.5, {name: 0.5}, {name: 'x'}, {'nope': 0.5}, TiledScreen(), {name: TiledScreen()}):
            case(net, detections=s)
            case(net, detections=s, sharded=True)
    # ---- tiled and region screens, and the plain one, with each kind of feed; over a fitted input too
    tiled = (TiledScreen(), TiledScreen(0.25, [5, 0, 3], (2, 2), 10, 'IOS', 0.1, False, 20), TiledScreen(input='image_tensor'), TiledScreen(input='nope'),
             TiledScreen(input=5), TiledScreen(threshold=2), TiledScreen(overlap='iou'), TiledScreen(per_label=1), TiledScreen(max_per_tile=0),
             TiledScreen(max_per_tile=2000), TiledScreen(max_per_frame=0), TiledScreen(min_confidence='x'), TiledScreen(labels=5))
    region = tuple(RegionScreen(*s) for s in tiled)
    for net, feed in itertools.product(('ssd', 'ssd_fit'), ('array', 'absent', 'roi', 'detected', 'warp')):
        for s in (0.5, DetectionScreen(frame_size=(48, 64)), tiled[0], tiled[1], region[0], region[1]):
            case(net, feed, detections=s)
            case(net, feed, detections={D: s})
    for net, feed in itertools.product(('ssd', 'ssd_fit'), ('array', 'roi')):
        for s in tiled[2:] + region[2:]:
            case(net, feed, detections={D: s})
    # ---- matches alone
    matches = (g10, GalleryMatch(g10), GalleryMatch(g10, 3), GalleryMatch(g10, 3, 0.25), GalleryMatch(g10, np.int64(2), np.float32(0.7)), GalleryMatch(g10, 1, 1),
               GalleryMatch(g10, 0), GalleryMatch(g10, 4), GalleryMatch(g10, True), GalleryMatch(g10, 1.0), GalleryMatch(g10, 1, float('nan')),
               GalleryMatch(g10, 1, float('inf')), GalleryMatch(g10, 1, 1e39), GalleryMatch(g10, 1, True), GalleryMatch(g10, 1, 'x'), GalleryMatch('x'),
               g7, GalleryMatch(g7, 2), 'x', 5, True, None, (g10,))
    for m in matches:
        if m is not None:
            case('mnist', matches=m)
        case('mnist', matches={E: m})
    for m in (g10, {E: g10}, {'nope': g10}, {E: 'x'}, {E: GalleryMatch(g10, 0)}, 'x', g7, {E: g7}, {E: g10, 'nope': 'x'}):
        case('mnist', matches=m, sharded=True)
        case('mnist_f16', matches=m)
        case('two', matches=m)
    for net, name in (('googlenet', R), ('ssd', D), ('heatmap', H)):
        for m in (g10, {name: g10}, {name: 'x'}, {'nope': g10}, 'x'):
            case(net, matches=m)
            case(net, matches=m, sharded=True)
    case('two', matches={H: g10})
    # ---- keypoints alone
    points = (True, 0.5, 0, 1, np.float32(0.7), np.int64(-2), PeakScreen(), PeakScreen(0.5, 'NONE', 'HEATMAP'), PeakScreen(None, 'QUARTER', 'HEATMAP'),
              PeakScreen(refine='HALF'), PeakScreen(refine=None), PeakScreen(refine=1), PeakScreen(space='PIXELS'), PeakScreen(space=None),
              PeakScreen(refine='HALF', space='PIXELS'), PeakScreen(float('nan')), PeakScreen(float('inf')), PeakScreen(1e39), PeakScreen(True), PeakScreen('x'),
              PeakScreen([1.0]), float('nan'), float('inf'), 1e39, False, None, 'QUARTER', [0.5], (0.5,), b'1', 1j, PeakScreen)
    for p in points:
        if p is not None:
            case('heatmap', keypoints=p)
        case('heatmap', keypoints={H: p})
    for p in (True, {H: 0.5}, {'nope': True}, {H: 'x'}, {H: PeakScreen(refine='HALF')}, 'x', {H: True, 'nope': 'x'}):
        case('heatmap', keypoints=p, sharded=True)
        case('heatmap_f16', keypoints=p)
        case('two', keypoints=p)
    for net, name in (('googlenet', R), ('mnist', E), ('ssd', D), ('ssd1', D)):
        for p in (True, {name: True}, {name: 'x'}, {'nope': True}, 'x'):
            case(net, keypoints=p)
            case(net, keypoints=p, sharded=True)
    case('two', keypoints={E: True})
    # ---- two keywords for different Results of one network
    for k, m, p in itertools.product((None, 3, {E: 3}), (None, g10, {E: GalleryMatch(g10, 2, 0.5)}), (None, 0.5, {H: PeakScreen()})):
        case('two', top_k=k, matches=m, keypoints=p)
    # ---- every pair of keywords naming one Result, in every form that reaches a clash text
    for k, m in itertools.product((5, {E: 5}), (g10, {E: GalleryMatch(g10, 2)})):
        case('mnist', top_k=k, matches=m)
        case('two', top_k=k, matches=m, keypoints=True)
    for s, p in itertools.product((0.5, {D: DetectionScreen()}, {D: TiledScreen()}, RegionScreen()), ({D: True}, {D: PeakScreen(0.5)})):
        case('ssd1', 'array', detections=s, keypoints=p)
        case('ssd1', 'roi', detections=s, keypoints=p)
    for s, k, feed in itertools.product((TiledScreen(), RegionScreen(), DetectionScreen(), 0.5, TiledScreen(threshold=2)), (5, 0, 'x'), ('array', 'roi')):
        case('ssd', feed, top_k={D: k}, detections={D: s})      # the tiled screens speak in front of top_k's own checks
        case('ssd', feed, top_k=k, detections={D: s})
        case('ssd', feed, top_k={D: k}, detections=s)
    stubbed = {'top_k': 1, 'detections': DetectionScreen(0.5, (300, 300), None, (1, 1), 100), 'matches': GalleryMatch(g7, 1, None),
               'keypoints': PeakScreen(None, 'QUARTER', 'NORMALISED')}
    given = {'top_k': 1, 'detections': 0.5, 'matches': g7, 'keypoints': True}
    for net, name in (('heatmap', H), ('ssd', D), ('mnist', E)):
        for a, b in itertools.combinations(KEYWORDS, 2):
            case(net, stubs={a: {name: stubbed[a]}, b: {name: stubbed[b]}}, **{a: given[a], b: given[b]})
        for a, b, c in itertools.combinations(KEYWORDS, 3):
            case(net, stubs={k: {name: stubbed[k]} for k in (a, b, c)}, **{k: given[k] for k in (a, b, c)})
        case(net, stubs={k: {name: stubbed[k]} for k in KEYWORDS}, **given)
        case(net, 'roi', stubs={k: {name: stubbed[k]} for k in KEYWORDS}, **given)
    for a, b in itertools.combinations(KEYWORDS, 2):          # two Results of 'two', each under two keywords: which one is named
        case('two', stubs={a: {H: stubbed[a], E: stubbed[a]}, b: {H: stubbed[b], E: stubbed[b]}}, **{a: given[a], b: given[b]})
        case('two', stubs={a: {E: stubbed[a], H: stubbed[a]}, b: {E: stubbed[b], H: stubbed[b]}}, **{a: given[a], b: given[b]})
    # ---- every pair of keywords each wrong on its own: the first refusal
    wrong = {'top_k': (0, 'x'), 'detections': (float('nan'), DetectionScreen(min_size=0)), 'matches': ('x', GalleryMatch(g10, 0)),
             'keypoints': ('x', PeakScreen(refine='HALF'))}
    for net, name in (('mnist', E), ('ssd', D), ('heatmap', H), ('googlenet', R), ('two', H)):
        for a, b in itertools.combinations(KEYWORDS, 2):
            for i in (0, 1):
                case(net, **{a: wrong[a][i], b: wrong[b][i]})
                case(net, **{a: {name: wrong[a][i]}, b: {name: wrong[b][i]}})
                case(net, **{a: {'nope': wrong[a][i]}, b: {'nope': wrong[b][i]}})
            case(net, sharded=True, **{a: {name: wrong[a][0]}, b: {name: wrong[b][0]}})
    # a wrong keyword beside a screen that its feed refuses: the feed checks run behind top_k's, detections' and matches', in front of keypoints'
    for net, feed, s in (('ssd', 'array', TiledScreen()), ('ssd', 'array', RegionScreen()), ('ssd_fit', 'roi', TiledScreen()), ('ssd_fit', 'roi', 0.5)):
        for keyword in ('top_k', 'matches', 'keypoints'):
            for i in (0, 1):
                case(net, feed, detections=s, **{keyword: wrong[keyword][i]})
                case(net, feed, detections={D: s}, **{keyword: {D: wrong[keyword][i]}})
    return out


class _Galleries:
    """(a Gallery of 3 rows with D = 10, one of 3 rows with D = 7), made on first use: the package is imported only then."""

    def __iter__(self):
        from pyopenvino_amd import Gallery
        if not hasattr(self, 'made'):
            self.made = (Gallery(np.eye(3, 10, dtype=np.float32)), Gallery(np.ones((3, 7), np.float32), metric='DOT'))
        return iter(self.made)


GALLERIES = _Galleries()


def _plain(v):
    """A field of an ask as JSON."""
    from pyopenvino_amd import Gallery
    from pyopenvino_amd.input_format import InputFormat
    if isinstance(v, Gallery):
        return repr(v)
    if isinstance(v, InputFormat):
        return 'InputFormat({})'.format(v.name)
    if isinstance(v, tuple):
        return [_plain(e) for e in v if not callable(e)]
    if isinstance(v, np.generic):
        return v.item()
    assert v is None or isinstance(v, (bool, int, float, str)), v
    return v


def outcome(nets, fed, case) -> dict:
    """What Answers.checked makes of `case` on `nets` = networks() with `fed` = feeds()."""
    from pyopenvino_amd import answers
    _, net, feed, given, sharded, stubs = case
    ex, name, _ = nets[net]
    rules = {'top_k': answers.top_k_rule, 'detections': answers.detections_rule, 'matches': answers.gallery_rule, 'keypoints': answers.keypoints_rule}
    real = {keyword: rules[keyword].checked for keyword in stubs}
    for keyword, found in stubs.items():
        rules[keyword].checked = lambda ienet, value, sharded, found=found: dict(found)
    try:
        asks = ex.answers.checked({} if fed[feed] is None else {name: fed[feed]}, given.get('top_k'), given.get('detections'), sharded,
                                  given.get('matches'), given.get('keypoints'))
    except Exception as e:
        return {'error': [type(e).__name__, str(e)]}
    finally:
        for keyword, function in real.items():
            rules[keyword].checked = function
    return {'asks': {result: [type(ask).__module__.rsplit('.', 1)[-1] + '.' + type(ask).__name__, _plain(tuple(ask))] for result, ask in asks.items()}}


def record() -> dict:
    with tempfile.TemporaryDirectory() as tmp:
        nets, fed = networks(tmp), feeds()
        return {case[0]: outcome(nets, fed, case) for case in cases()}


if __name__ == '__main__':
    path = os.path.join(HERE, 'answer_checks.json')
    recorded = record()
    with open(path, 'w') as f:
        json.dump(recorded, f, separators=(',', ':'), sort_keys=True)
        f.write('\n')
    print(path, os.path.getsize(path), len(recorded), 'cases')
