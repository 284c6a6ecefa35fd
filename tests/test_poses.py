"""``infer(..., maxima=..., poses=...)``: persons grouped on the device from the candidates of maxima= and the part-affinity fields
(pvhip_pose_groups_f32).  tests/poses_ref.py is the rule in plain loops; pyopenvino_amd/poses.py (numpy) and the kernels equal it bit
for bit on all five arrays.  The loops' answer of a case is made once and serves the host test and the device test."""
import functools
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import poses_ref
import test_keypoints as keypoints_tests
import test_text as text_tests

NAN = np.float32(np.nan)
CHAIN = ((0, 1, 0, 1, 1), (1, 2, 2, 3, 1), (3, 2, 5, 4, 0))             # a custom skeleton: two founding limbs in a chain, one that founds nothing
PAIR = ((0, 1, 0, 1, 1),)


def _paint(shape, channels, skeleton, rows):
    from pyopenvino_amd import synth
    return synth.paint_poses(np.zeros(shape, np.float32), np.zeros(shape[:1] + (channels,) + shape[2:], np.float32), skeleton, rows)


def _stick(x, y):
    """An OPENPOSE18 person around (x, y): 18 joints on a 9 x 13 patch, no two on one pixel."""
    at = [(4, 1), (4, 3), (2, 3), (1, 6), (0, 9), (6, 3), (7, 6), (8, 9), (3, 7), (3, 10), (2, 12), (5, 7), (5, 10), (6, 12), (3, 0), (5, 0), (2, 1), (6, 1)]
    return {k: (x + dx, y + dy) for k, (dx, dy) in enumerate(at)}


def _truth():
    return [[_stick(3, 2), _stick(30, 15)], [_stick(2, 17), _stick(20, 3), _stick(45, 10)]]


def _random(seed, shape, limbs, peaks, lattice=0):
    """Random peaks (or one every `lattice` pixels); fields in eighths, the first limb's constant: pairs of one direction tie."""
    rng = np.random.default_rng(seed)
    n, K, H, W = shape
    heat = (rng.integers(0, 4, shape) / 16).astype(np.float32)
    for plane in heat.reshape(n * K, H * W):
        at = np.arange(H * W).reshape(H, W)[1::lattice, 1::lattice].ravel() if lattice else rng.choice(H * W, peaks, replace=False)
        plane[at] = (rng.integers(8, 16, at.size) / 16).astype(np.float32)
    pafs = (rng.integers(-8, 9, (n, 2 * limbs, H, W)) / 8).astype(np.float32)
    pafs[:, 0], pafs[:, 1] = 0.5, 0.25
    return heat, pafs


@functools.lru_cache(maxsize=None)
def _case(name):
    """(heat, pafs, the MaximaScreen's fields, the PoseScreen's fields, the loops' answer) of one case."""
    from pyopenvino_amd import poses
    m, s = dict(min_score=0.3, max_per_plane=20, refine='QUARTER', space='NORMALISED'), dict(skeleton='OPENPOSE18')
    if name == 'truth':                                         # two and three well-separated people
        heat, pafs = _paint((2, 19, 32, 57), 38, poses.OPENPOSE18, _truth())
    elif name == 'conflict':                                    # candidates compete, limbs cross, equal scores
        heat, pafs = _random(5, (3, 4, 8, 9), 3, 3)
        s = dict(skeleton=CHAIN, samples=5, min_field=0.0, min_samples=2, max_persons=4, min_joints=2, min_mean=0.0)
    elif name.startswith('full'):                               # 32 candidates a plane: 1024 pairs, several chunks at S = 10 and 16
        _, S, least = name.split()
        heat, pafs = _random(7, (1, 2, 24, 24), 2, 0, lattice=3)
        m.update(max_per_plane=32, refine='NONE', space='HEATMAP')
        s = dict(skeleton=((0, 1, 2, 3, 1),), samples=int(S), min_field=0.125, min_samples=int(least), max_persons=64, min_joints=2, min_mean=0.0)
    elif name.startswith('plane'):                              # both of maxima's forms; planes at an odd 4-byte phase
        H, W = (int(v) for v in name.split()[1:])
        heat, pafs = _random(H, (2, 4, H, W), 3, 6)
        s = dict(skeleton=CHAIN, samples=16, min_field=0.0, min_samples=9, max_persons=5, min_joints=2, min_mean=0.4)
    elif name.startswith('edges'):
        # row 0: joint 0 and joint 1 share pixel (2, 2) (no connection) beside three real pairs for max_persons = 2; a NaN tap on the
        # second pair's way; joint 3's candidate finds no person on the non-founding limb; limb (1, 2) twice: the second leaves slot 2 alone.
        people = [{0: (2, 2), 1: (6, 2), 2: (6, 6)}, {0: (2, 9), 1: (9, 9)}, {0: (12, 2), 1: (12, 7)}]
        skeleton = CHAIN + ((1, 2, 2, 3, 1),)
        heat, pafs = _paint((2, 4, 12, 15), 6, skeleton, [people, [{0: (1, 1), 1: (5, 5)}]])
        heat[0, 1, 2, 2], heat[0, 3, 10, 1], pafs[0, 0, 9, 5] = 0.5, 0.8, NAN
        heat[1] = NAN                                           # a whole row of NaN heat beside a live one
        s = dict(skeleton=skeleton, samples=4, min_field=0.0, min_samples=3, max_persons=2, min_joints=2, min_mean=0.0)
        if name != 'edges':                                     # min_joints and min_mean at equality: the first person's own figures
            first = _case('edges')[4]
            mean = first.totals[0, 0] / np.float32((first.joints[0, 0] >= 0).sum())
            s.update(min_joints=3, min_mean=float(mean if name == 'edges equal' else np.nextafter(mean, np.float32(9))))
    want = poses_ref.poses(heat, pafs, **{**m, **s, 'skeleton': s['skeleton'] if s['skeleton'] != 'OPENPOSE18' else poses.OPENPOSE18})
    return heat, pafs, m, s, want


CASES = ['truth', 'conflict'] + ['full {} {}'.format(S, least) for S in (2, 10, 16) for least in (1, S)] \
    + ['plane 32 32', 'plane 40 40', 'plane 33 31', 'edges', 'edges equal', 'edges above']


def _same(got, want, what):
    for field, a, b in zip(want._fields, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, field, a.dtype, a.shape, b.dtype, b.shape)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), '{}: {} differs\n{}\n{}'.format(what, field, a[:2], b[:2])


def _expected(name, want):
    if name == 'truth':                                         # each painted person is one answered person, at the painted pixels
        assert want.counts.tolist() == [2, 3]
        for r, people in enumerate(_truth()):
            for q, person in enumerate(people):
                assert want.joints[r, q, :18].tolist() == [y * 57 + x for x, y in person.values()] and want.joints[r, q, 18] == -1
    elif name.startswith('full'):
        assert want.counts[0] > 0 or not name.endswith(' 1'), want.counts
    elif name.startswith('edges'):
        assert want.counts.tolist() == ([2, 0] if name == 'edges' else [1, 0] if name == 'edges equal' else [0, 0]) and want.joints[0, :, 3].max() == -1
    else:
        assert want.counts.min() > 0, want.counts


@pytest.mark.parametrize('name', CASES)
def test_group_equals_the_loops(name):
    from pyopenvino_amd import MaximaScreen, PoseScreen, poses
    heat, pafs, m, s, want = _case(name)
    _expected(name, want)
    _same(poses.group(heat, pafs, MaximaScreen(**m), PoseScreen(**s)), want, name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_kernels_equal_the_loops(hip, name):
    """The maxima entry and the pose entry behind it, as a request launches them; three calls, the same bytes."""
    from pyopenvino_amd import MaximaScreen, PoseScreen, maxima, poses
    heat, pafs, m, s, want = _case(name)
    n, K, H, W = heat.shape
    heat_screen, screen = maxima.for_planes(maxima.resolved(MaximaScreen(**m)), n, K), poses.resolved(PoseScreen(**s))
    table = poses.skeleton_for(screen, K, pafs.shape[1])
    found = maxima.Blocks(n, K, heat_screen.max_per_plane, heat_screen.max_per_row, heat_screen.refine, heat_screen.space)
    blocks = poses.Blocks(n, K, screen.max_persons, len(table))
    dev = hip.DeviceTensor.from_numpy(heat), hip.DeviceTensor.from_numpy(pafs)
    for call in range(3):
        found.launch(dev[0], heat_screen.min_score)
        blocks.launch(dev[1], dev[0], found.scratch, heat_screen, screen, table)
        _same(blocks.read_back(), want, '{} call {}'.format(name, call))


def _net(tmp_path, n, package=keypoints_tests.HIP):
    """mnist's first layer with two Results of one shape: 'heatmaps' (n, 32, 26, 26) and, behind a Reshape, 'text' as the fields."""
    from pyopenvino_amd import IECore
    base = keypoints_tests._heatmap_head('mnist', tmp_path)
    xml, weights = os.path.join(str(tmp_path), 'mnist_poses.xml'), os.path.join(str(tmp_path), 'mnist_poses.bin')
    blob = text_tests._with_text_chain(base, xml, open(os.path.join(text_tests.MODELS, 'mnist.bin'), 'rb').read(), None, False, [0, 32, 26, 26])
    open(weights, 'wb').write(blob)
    tree = ET.parse(xml)                                        # (the chain declares its shape constant as three numbers: here it has four)
    (reshape,) = [layer for layer in tree.getroot().find('layers') if layer.get('name') == 'text/reshape']
    reshape.find('input').findall('port')[1].find('dim').text = '4'
    tree.write(xml)
    net = IECore(plugin_package=package).read_network(xml, weights=weights)
    net.set_batch(n)
    return IECore(plugin_package=package).load_network(net, 'GPU', num_requests=1), net.inputs[0]['name']


def _bad():
    from pyopenvino_amd import MaximaScreen, PoseScreen
    good, heat = PoseScreen(skeleton=CHAIN), {'heatmaps': True}
    yield 'maxima= in the same call', dict(poses=good)
    yield 'heat \'text\' is not asked for with maxima=', dict(maxima=heat, poses={'text': good._replace(heat='text')})
    yield 'max_per_plane = 33, above 32', dict(maxima={'heatmaps': MaximaScreen(max_per_plane=33)}, poses=good)
    yield 'heat= names the one', dict(maxima=True, poses={'text': good})
    yield 'asked for with maxima as well', dict(maxima=True, poses={'text': good._replace(heat='text')})
    yield 'asked for with keypoints as well', dict(maxima=heat, poses=good, keypoints={'text': True})
    yield 'no Result named', dict(maxima=heat, poses={'nope': good})
    yield 'a PoseScreen or True', dict(maxima=heat, poses=0.5)
    yield '\'OPENPOSE18\' takes K >= 18 joints and 38 field planes', dict(maxima=heat, poses=True)
    for skeleton in ('COCO', [[0, 1, 0, 1]], [[0, 1, 0, 1, 1]] * 65, [[0.5, 1, 0, 1, 1]]):
        yield 'skeleton is \'OPENPOSE18\' or an', dict(maxima=heat, poses=good._replace(skeleton=skeleton))
    for row, match in (((0, 0, 0, 1, 1), 'two different joints'), ((0, 32, 0, 1, 1), 'two different joints'), ((0, 1, 0, 32, 1), 'channels'),
                       ((0, 1, -1, 1, 1), 'channels'), ((0, 1, 0, 1, 2), 'founds is 0 or 1')):
        yield 'skeleton limb 1: .*' + match, dict(maxima=heat, poses=good._replace(skeleton=PAIR + (row,)))
    for field, values in (('samples', (1, 17, 2.0)), ('min_field', (-0.125, np.nan, '0')), ('min_samples', (0, 11, True)), ('max_persons', (0, 65)),
                          ('min_joints', (0, 33, None)), ('min_mean', (np.inf, None)), ('heat', (3,))):
        for value in values:
            yield field, dict(maxima=heat, poses={'text': good._replace(**{field: value})})


def test_refusals_and_the_host_route(tmp_path):
    """Every refusal is a ValueError('poses: ...') before anything is staged; a plugin set that computes on the host gets the numpy rule."""
    from pyopenvino_amd import MaximaScreen, PoseScreen, Poses, maxima, poses
    n, (ex, name) = 2, _net(tmp_path, 2, 'oracle.op_plugins')
    x, req = keypoints_tests._pixels(10, n), ex.requests[0]

    def refused(match, kw):
        with pytest.raises(ValueError, match=match) as e:
            ex.infer({name: x}, **kw)
        assert str(e.value).startswith('poses: '), str(e.value)
        assert not req._in_flight and not req._asks and not ex.answers.blocks and not ex.host_inputs.slots

    for match, kw in _bad():
        refused(match, kw)
    with pytest.raises(ValueError, match='poses: not with a batch sharded'):
        poses.checked(ex.ienet, PoseScreen(skeleton=CHAIN), {'heatmaps': maxima.resolved(True)}, True)
    port = next(iter(ex.ienet.G.nodes[[nid for nid, result in ex.ienet.find_node_by_type('Result') if result == 'text'][0]]['input'].values()))
    for key, bad, match in (('dims', (n, 32, 13, 52), 'not one n, H and W'), ('dims', (n, 130, 26, 26), 'has shape'), ('precision', 'FP16', 'FP32 Results only')):
        kept, port[key] = port[key], bad
        try:
            refused(match, dict(maxima={'heatmaps': True}, poses={'text': PoseScreen(skeleton=CHAIN)}))
        finally:
            port[key] = kept
    heat_screen, screen = MaximaScreen(0.1, 20), PoseScreen(skeleton=CHAIN, min_field=0.0, min_samples=5, min_joints=2, min_mean=0.0)
    full = ex.infer({name: x})
    got = ex.infer({name: x}, maxima={'heatmaps': heat_screen}, poses=screen)
    _same(got['text'], poses.group(full['heatmaps'], full['text'], heat_screen, screen), 'host route')
    assert isinstance(got['text'], Poses) and got['text'].counts.min() > 0


@pytest.mark.gpu
def test_public_path_replays(hip, tmp_path):
    """The rule on the request's own full Results; passes with and without poses= replay the recording; the heat's Maxima is unchanged."""
    from pyopenvino_amd import MaximaScreen, PoseScreen, Poses, maxima
    n, (ex, name) = 3, _net(tmp_path, 3)
    req, xd = ex.requests[0], hip.DeviceTensor.from_numpy(keypoints_tests._pixels(10, n))
    req.infer({name: xd})
    full = {k: np.array(v, copy=True) for k, v in req.infer({name: xd}).items()}      # (the next pass replays)
    heat_screen, screen = MaximaScreen(0.1, 20), PoseScreen(skeleton=CHAIN, min_field=0.0, min_samples=5, min_joints=2, min_mean=0.0)
    m = dict(zip(heat_screen._fields, maxima.resolved(heat_screen)))
    want = poses_ref.poses(full['heatmaps'], full['text'], **{k: v for k, v in {**m, **screen._asdict()}.items() if k not in ('max_per_row', 'heat')})
    for given in (screen, None, {'text': screen._replace(heat='heatmaps')}):
        req.start_async({name: xd}, maxima={'heatmaps': heat_screen}, poses=given)
        assert req._replayed is not None
        got = req.wait()
        _same(got['heatmaps'], maxima.peaks_of(full['heatmaps'], heat_screen), 'maxima beside {!r}'.format(given))
        if given is None:
            assert np.array_equal(np.asarray(got['text']), full['text'])
        else:
            assert isinstance(got['text'], Poses) and want.counts.min() > 0
            _same(got['text'], want, repr(given))
