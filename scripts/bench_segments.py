"""A segmentation network's answer made on the device (``infer(..., segments=...)``): what the launch costs and what the read-back saves.

Two steps, each a child process under its own `timeout` (the parent never opens the device; a step that fails ends the run):

  launch   pvhip_segment_labels_f32 alone on device-resident tensors -- (32, 21, 513, 513) (a DeepLab-style head; H * W is odd, so the
           planes stand at every 4-byte phase), (32, 4, 512, 896) (road segmentation) and (256, 32, 26, 26) (the first Convolution +
           bias + ReLU of models/mnist.xml) --, device time per call by hipEvents around `--launches` back-to-back calls (each is the
           initialising launch and the walk), as 4 n C H W / time in TB/s.  Each shape twice: on a `blocky` map, four large regions, so
           that a wave sees one class, and on a `salt_and_pepper` map, every pixel another class than the one before it, the worst case
           for the sums of areas and extents.  Beside them pvhip_relu_f32 on a tensor of the same size in the same process, the three
           alternating over `--rounds` rounds: the streaming rate of the box in this session; its figure is its READ rate, it writes as
           many bytes again.  The labels, areas and extents of every timed tensor are compared with the map it was made from.
  passes   models/mnist.xml cut behind its first ReLU at batch 256 on a device-resident input, request 0, synchronous:
           `segments`           infer(..., segments=True): the pass, one entry call, 4 ceil(n H W / 4) + 20 n C bytes read back;
           `read_back_argmax`   the same pass, the whole Result read back, np.argmax(axis=1).astype(np.uint8), then the bincount and
                                the extents per class in numpy (segments.sums);
           blocks of `--steps` passes alternating between the two over `--rounds` rounds, ms per pass, median of the blocks.

Prints one JSON line; --out writes it too, --md a table of it.  e.g.
    python scripts/bench_segments.py --out profiles/segments.json --md profiles/segments.md
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench_keypoints      # noqa: E402  (scripts/ is sys.path[0]: the mnist head and the commit are found as there)

SHAPES = [(32, 21, 513, 513), (32, 4, 512, 896), (256, 32, 26, 26)]
BATCH = 256
STEP_LIMIT = {'launch': 420, 'passes': 240}                   # seconds each child may take


def class_map(kind, n, C, H, W):
    """(n, H, W) classes: `blocky`, the quadrants of the map, another class in each and in each row; `salt_and_pepper`, every pixel
    another class than the pixel before it."""
    r, y, x = np.meshgrid(np.arange(n), np.arange(H), np.arange(W), indexing='ij', sparse=True)
    if kind == 'blocky':
        return ((r + 2 * (2 * y // H) + (2 * x // W)) % C).astype(np.uint8)
    return ((r + y * W + x) % C).astype(np.uint8)


def scores_of(classes, C, rng):
    """(n, C, H, W) float32 scores in [0, 1) with 4 .. 5 at every pixel's class."""
    n, H, W = classes.shape
    x = rng.random((n, C, H, W), dtype=np.float32)
    np.put_along_axis(x, classes[:, None].astype(np.int64), (4 + rng.random((n, 1, H, W), dtype=np.float32)), axis=1)
    return x


def step_launch(args):
    from pyopenvino_amd import device, segments
    device.init(0)
    rng = np.random.default_rng(2026)
    e0, e1 = device.Event(), device.Event()
    rows = []
    for n, C, H, W in SHAPES:
        nbytes, pixels = 4 * n * C * H * W, n * H * W
        label_words = (pixels + 3) // 4
        out = device.DeviceTensor.empty((label_words + 5 * n * C,), np.int32)
        at = out.ptr + 4 * label_words
        maps, xs = {}, {}
        for kind in ('blocky', 'salt_and_pepper'):
            maps[kind] = class_map(kind, n, C, H, W)
            xs[kind] = device.DeviceTensor.from_numpy(scores_of(maps[kind], C, rng))
        ys = device.DeviceTensor.empty((n, C, H, W), np.float32)

        def labels(kind):
            device.call('pvhip_segment_labels_f32', ctypes.c_void_p(xs[kind].ptr), n, C, H, W, 0, 0.0, ctypes.c_void_p(out.ptr), ctypes.c_void_p(at),
                        ctypes.c_void_p(at + 4 * n * C))

        launches = {'blocky': lambda: labels('blocky'), 'salt_and_pepper': lambda: labels('salt_and_pepper'),
                    'relu': lambda: device.call('pvhip_relu_f32', ctypes.c_void_p(xs['blocky'].ptr), ctypes.c_void_p(ys.ptr), n * C * H * W)}
        for kind in maps:                                     # what is timed gives the map it was made from
            labels(kind)
            device.synchronize()
            host = np.asarray(out)
            assert np.array_equal(host[:label_words].view(np.uint8)[:pixels].reshape(n, H, W), maps[kind]), kind
            areas, extents = segments.sums(maps[kind], C)
            got = host[label_words + n * C:].reshape(n, C, 4).copy()
            got[areas == 0] = 0
            assert np.array_equal(host[label_words:label_words + n * C].reshape(n, C), areas) and np.array_equal(got, extents), kind
        us = {kind: [] for kind in launches}
        for _ in range(args.rounds):
            for kind, launch in launches.items():
                for _ in range(args.warmup):
                    launch()
                e0.record()
                for _ in range(args.launches):
                    launch()
                e1.record()
                e1.synchronize()
                us[kind].append(e0.elapsed_ms(e1) * 1e3 / args.launches)
        row = {'shape': [n, C, H, W], 'bytes': nbytes, 'form': device.call('pvhip_segment_labels_form', C, H, W)}
        for kind, v in us.items():
            med = float(np.median(v))
            row[kind] = {'us': med, 'read_TBps': nbytes / med * 1e-6, 'us_per_round': v, 'spread_us': max(v) - min(v)}
        extra = row['salt_and_pepper']['us'] - row['blocky']['us']
        row['salt_and_pepper_minus_blocky_us'] = extra
        row['salt_and_pepper_beyond_spread'] = bool(extra > max(row['blocky']['spread_us'], row['salt_and_pepper']['spread_us']))
        rows.append(row)
        del xs, ys, out
    return {'rows': rows, 'launches_per_round': args.launches, 'device': device.device_name()}


def step_passes(args):
    from pyopenvino_amd import IECore, device, segments
    n, C, H, W = BATCH, 32, 26, 26
    with tempfile.TemporaryDirectory() as folder:
        ie = IECore()
        xml, weights = bench_keypoints.mnist_head_ir(folder)
        net = ie.read_network(xml, weights=weights)
        net.set_batch(n)
        ex = ie.load_network(net, 'GPU', num_requests=1)
        name, out_name = net.inputs[0]['name'], net.outputs[0]['name']
        x = device.DeviceTensor.from_numpy(np.random.default_rng(3).uniform(0, 1, (n, 1, 28, 28)).astype(np.float32))

        def on_device():
            return ex.infer({name: x}, segments=True)[out_name]

        def on_host():
            full = ex.infer({name: x})[out_name]
            labelled = np.argmax(full, axis=1).astype(np.uint8)
            return (labelled,) + segments.sums(labelled, C)

        got, want = on_device(), on_host()
        assert all(np.array_equal(a, b) for a, b in zip(got, want))      # (finite: the two routes agree)
        ms = {'segments': [], 'read_back_argmax': []}
        handed = {'segments': 4 * ((n * H * W + 3) // 4) + 20 * n * C, 'read_back_argmax': 4 * n * C * H * W}
        for _ in range(args.rounds):
            for kind, run in (('segments', on_device), ('read_back_argmax', on_host)):
                for _ in range(args.warmup):
                    run()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    run()
                ms[kind].append((time.perf_counter() - t0) * 1e3 / args.steps)
        med = {kind: float(np.median(v)) for kind, v in ms.items()}
        row = {'shape': [n, C, H, W], 'ms_per_pass': med, 'ms_per_pass_per_block': ms, 'bytes_read_back': handed,
               'segments_vs_read_back': med['segments'] / med['read_back_argmax'], 'replaying': ex._graph is not None}
        ex.release_device_state()
    return {'rows': [row], 'steps_per_block': args.steps, 'rounds': args.rounds}


def markdown(line):
    """The JSON line as the tables of profiles/segments.md."""
    text = ['# The class map on the device: `pvhip_segment_labels_f32`', '',
            'Written by `python scripts/bench_segments.py --out profiles/segments.json --md profiles/segments.md` on {}, {}, commit {} plus '
            'this change; `profiles/segments.json` is the same run.  Every figure is the median of {} blocks; min-max are the blocks\' own.  '
            'Not profiled with `rocprofv3`.'.format(line['device'], line['date'], line['git_head'], line['passes']['rounds']), '',
            '## The entry alone, beside ReLU on the same bytes', '',
            'Device time per call between two hipEvents around {} back-to-back calls on one device-resident tensor; `4 n C H W / time`.  A call '
            'is two launches: the block\'s initialisation and the walk.  `blocky`: four large regions, a wave sees one class; '
            '`salt_and_pepper`: every pixel another class than the one before it.  `pvhip_relu_f32` ran on a tensor of the same size in the same '
            'process, the three alternating block by block: its figure is its READ rate, and it writes as many bytes again.'.format(
                line['launch']['launches_per_round']), '',
            '| Result | bytes | map | us | min-max | TB/s | ReLU us | min-max | ReLU read TB/s | rate / ReLU read rate |', '|---|---|---|---|---|---|---|---|---|---|']
    notes = []
    for row in line['launch']['rows']:
        relu = row['relu']
        for kind in ('blocky', 'salt_and_pepper'):
            r = row[kind]
            text.append('| {} | {:.1f} MB | {} | {:.2f} | {:.2f}-{:.2f} | {:.2f} | {:.2f} | {:.2f}-{:.2f} | {:.2f} | {:.2f} |'.format(
                tuple(row['shape']), row['bytes'] / 1e6, kind, r['us'], min(r['us_per_round']), max(r['us_per_round']), r['read_TBps'], relu['us'],
                min(relu['us_per_round']), max(relu['us_per_round']), relu['read_TBps'], relu['us'] / r['us']))
        extra, spread = row['salt_and_pepper_minus_blocky_us'], max(row['blocky']['spread_us'], row['salt_and_pepper']['spread_us'])
        notes.append('{}: salt-and-pepper - blocky = {:+.2f} us ({:+.1f} %), the blocks\' own spread {:.2f} us: {}.'.format(
            tuple(row['shape']), extra, 100 * extra / row['blocky']['us'], spread,
            '**beyond the spread**' if row['salt_and_pepper_beyond_spread'] else 'within the spread'))
    text += [''] + [note + '  ' for note in notes]
    text += ['', '## The whole pass: the keyword against the route without it', '',
             '`models/mnist.xml` cut behind its first ReLU, batch 256, a device-resident input, request 0, synchronous, blocks of {} passes, the two '
             'routes alternating.  `segments`: `infer(..., segments=True)`.  `read_back_argmax`: the same pass, the whole Result read back, '
             '`np.argmax(axis=1).astype(np.uint8)`, then the bincount and the extents per class in numpy.'.format(line['passes']['steps_per_block']), '',
             '| Result | `segments` ms | min-max | bytes read back | `read_back_argmax` ms | min-max | bytes read back | ratio |', '|---|---|---|---|---|---|---|---|']
    for row in line['passes']['rows']:
        a, b = row['ms_per_pass_per_block']['segments'], row['ms_per_pass_per_block']['read_back_argmax']
        text.append('| {} | {:.3f} | {:.3f}-{:.3f} | {} | {:.2f} | {:.2f}-{:.2f} | {} | {:.3f} |'.format(
            tuple(row['shape']), row['ms_per_pass']['segments'], min(a), max(a), row['bytes_read_back']['segments'], row['ms_per_pass']['read_back_argmax'],
            min(b), max(b), row['bytes_read_back']['read_back_argmax'], row['segments_vs_read_back']))
    return '\n'.join(text) + '\n'


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=30, help='timed passes per block')
    ap.add_argument('--warmup', type=int, default=5, help='untimed passes (calls) in front of every block')
    ap.add_argument('--rounds', type=int, default=5, help='blocks per kind, the kinds alternating')
    ap.add_argument('--launches', type=int, default=50, help='timed calls per block of the launch step')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--md', default=None, help='write the tables of the line to this file')
    ap.add_argument('--head', default=None, help='git commit to report (default: git rev-parse HEAD, when the tree is a checkout)')
    ap.add_argument('--step', choices=sorted(STEP_LIMIT), default=None, help='(the child processes) run this step here and print its JSON')
    args = ap.parse_args()
    if args.step:
        print(json.dumps({'launch': step_launch, 'passes': step_passes}[args.step](args)))
        return 0
    line = {'metric': 'segments: a segmentation network\'s class map made on the device'}
    passed_on = [a for k in ('steps', 'warmup', 'rounds', 'launches') for a in ('--' + k, str(getattr(args, k)))]
    for step in ('launch', 'passes'):
        child = subprocess.run(['timeout', '-k', '10', str(STEP_LIMIT[step]), sys.executable, os.path.abspath(__file__), '--step', step] + passed_on,
                               stdout=subprocess.PIPE, text=True)
        if child.returncode != 0:
            print('bench_segments: step {} ended with status {}: nothing further is started'.format(step, child.returncode), file=sys.stderr)
            return child.returncode
        line[step] = json.loads(child.stdout.strip().splitlines()[-1])
    line.update(git_head=bench_keypoints.git_head(args.head), device=line['launch'].pop('device'), date=time.strftime('%Y-%m-%d'),
                profiled_with_rocprofv3=False)
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    if args.md:
        with open(args.md, 'w') as f:
            f.write(markdown(line))
    return 0


if __name__ == '__main__':
    sys.exit(main())
