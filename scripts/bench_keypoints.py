"""A heatmap network's answer made on the device (``infer(..., keypoints=...)``): what the launch costs and what the read-back saves.

Three Results at batch 256: (256, 17, 64, 48) (single-person pose), (256, 19, 46, 46) (a CPM stage) and (256, 32, 26, 26) (the first
Convolution + bias + ReLU of models/mnist.xml).  Two steps, each a child process under its own `timeout` (the parent never opens the
device; a step that fails ends the run):

  launch   pvhip_heatmap_peaks_f32 alone, device time per launch by hipEvents around `--launches` back-to-back launches, as
           4 n K H W / time in TB/s, beside pvhip_relu_f32 (unary_f4_kernel) on a tensor of the same size in the same run, the two
           alternating over `--rounds` rounds.  Twice: `resident`, every launch on the same tensor (22-53 MB: it stays in the 256 MiB
           Infinity Cache, as a Result the pass has just written does), and `streamed`, the launches walking over copies of the tensor
           that add up to more than 600 MB, so that every plane comes from HBM.  ReLU's figure is its READ rate, bytes read / time; it
           writes as many bytes again.
  passes   a stand-in heatmap head per shape -- Parameter (256, 3, H, W), a 3 x 3 Convolution to K channels, bias, ReLU, Result; the
           mnist one is the shipped network cut behind its first ReLU -- on a device-resident input, request 0, synchronous:
           (b) infer(..., keypoints=True), the pass, one launch and 16 n K bytes read back;
           (c) the route without the keyword: the same pass, the whole Result read back and argmax per plane in numpy
               (`full.reshape(n * K, -1).argmax(1)`, no refinement);
           blocks of `--steps` passes alternating between the two over `--rounds` rounds, ms per pass, median of the blocks.

Prints one JSON line; --out writes it too.  e.g.  python scripts/bench_keypoints.py --out profiles/keypoints.json
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time
import xml.etree.ElementTree as ET

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BATCH = 256
SHAPES = [(BATCH, 17, 64, 48), (BATCH, 19, 46, 46), (BATCH, 32, 26, 26)]
STREAM_BYTES = 600 << 20                                      # copies walked by the `streamed` launches add up to this at least
STEP_LIMIT = {'launch': 240, 'passes': 420}                   # seconds each child may take


def _port(parent, pid, dims):
    port = ET.SubElement(parent, 'port', {'id': str(pid), 'precision': 'FP32'})
    for d in dims:
        ET.SubElement(port, 'dim').text = str(d)


def _layer(layers, lid, name, kind, data=None, inputs=(), output=None):
    layer = ET.SubElement(layers, 'layer', {'id': str(lid), 'name': name, 'type': kind, 'version': 'opset1'})
    if data:
        ET.SubElement(layer, 'data', data)
    if inputs:
        node = ET.SubElement(layer, 'input')
        for pid, dims in enumerate(inputs):
            _port(node, pid, dims)
    if output is not None:
        _port(ET.SubElement(layer, 'output'), len(inputs), output)


def head_ir(folder, K, H, W, seed=7):
    """A heatmap head as an IR: Parameter (1, 3, H, W) -> Convolution 3 x 3, pad 1, K channels -> Add bias -> ReLU -> Result (1, K, H, W);
    (path of the xml, the weight blob), weights from `seed`."""
    rng = np.random.default_rng(seed)
    weights = (rng.standard_normal((K, 3, 3, 3)) * 0.2).astype(np.float32)
    bias = (rng.standard_normal((1, K, 1, 1)) * 0.1).astype(np.float32)
    net = ET.Element('net', {'name': 'heatmap_head', 'version': '10'})
    layers, edges = ET.SubElement(net, 'layers'), ET.SubElement(net, 'edges')
    x, y = (1, 3, H, W), (1, K, H, W)
    _layer(layers, 0, 'image', 'Parameter', {'element_type': 'f32', 'shape': ', '.join(map(str, x))}, output=x)
    _layer(layers, 1, 'head/weights', 'Const', {'element_type': 'f32', 'offset': '0', 'shape': ', '.join(map(str, weights.shape)),
                                                'size': str(weights.nbytes)}, output=weights.shape)
    _layer(layers, 2, 'head/conv', 'Convolution', {'auto_pad': 'explicit', 'dilations': '1, 1', 'pads_begin': '1, 1', 'pads_end': '1, 1',
                                                   'strides': '1, 1'}, inputs=(x, weights.shape), output=y)
    _layer(layers, 3, 'head/bias', 'Const', {'element_type': 'f32', 'offset': str(weights.nbytes), 'shape': ', '.join(map(str, bias.shape)),
                                             'size': str(bias.nbytes)}, output=bias.shape)
    _layer(layers, 4, 'head/add', 'Add', {'auto_broadcast': 'numpy'}, inputs=(y, bias.shape), output=y)
    _layer(layers, 5, 'head/relu', 'ReLU', inputs=(y,), output=y)
    _layer(layers, 6, 'heatmaps', 'Result', inputs=(y,))
    for a, ap, b, bp in ((0, 0, 2, 0), (1, 0, 2, 1), (2, 2, 4, 0), (3, 0, 4, 1), (4, 2, 5, 0), (5, 1, 6, 0)):
        ET.SubElement(edges, 'edge', {'from-layer': str(a), 'from-port': str(ap), 'to-layer': str(b), 'to-port': str(bp)})
    path = os.path.join(folder, 'head_{}x{}x{}.xml'.format(K, H, W))
    ET.ElementTree(net).write(path)
    return path, weights.tobytes() + bias.tobytes()


def mnist_head_ir(folder):
    """models/mnist.xml cut behind its first ReLU, a Result appended: (path of the xml, path of the shipped weights)."""
    tree = ET.parse(os.path.join(REPO, 'models', 'mnist.xml'))
    layers, edges = tree.getroot().find('layers'), tree.getroot().find('edges')
    relu = min(int(layer.get('id')) for layer in layers if layer.get('type') == 'ReLU')
    for layer in list(layers):
        if int(layer.get('id')) > relu:
            layers.remove(layer)
    for e in list(edges):
        if int(e.get('to-layer')) > relu:
            edges.remove(e)
    out = [layer for layer in layers if int(layer.get('id')) == relu][0].find('output').find('port')
    _layer(layers, relu + 1, 'heatmaps', 'Result', inputs=([d.text for d in out.findall('dim')],))
    ET.SubElement(edges, 'edge', {'from-layer': str(relu), 'from-port': out.get('id'), 'to-layer': str(relu + 1), 'to-port': '0'})
    path = os.path.join(folder, 'mnist_head.xml')
    tree.write(path)
    return path, os.path.join(REPO, 'models', 'mnist.bin')


def step_launch(args):
    from pyopenvino_amd import device, keypoints
    device.init(0)
    rng = np.random.default_rng(2026)
    e0, e1 = device.Event(), device.Event()

    def timed(launches, copies):
        """{kind: device time per launch in us, one figure per round} of `launches` = {kind: launch}, the kinds alternating;
        launch(i) works on copy i % copies."""
        us = {kind: [] for kind in launches}
        for _ in range(args.rounds):
            for kind, launch in launches.items():
                for i in range(args.warmup):
                    launch(i % copies)
                e0.record()
                for i in range(args.launches):
                    launch(i % copies)
                e1.record()
                e1.synchronize()
                us[kind].append(e0.elapsed_ms(e1) * 1e3 / args.launches)
        return us

    rows = []
    for n, K, H, W in SHAPES:
        nbytes = 4 * n * K * H * W
        copies = -(-STREAM_BYTES // nbytes)
        host = np.maximum(rng.standard_normal((n, K, H, W)).astype(np.float32), 0)
        xs = [device.DeviceTensor.from_numpy(host) for _ in range(copies)]
        ys = [device.DeviceTensor.empty((n, K, H, W), np.float32) for _ in range(2)]
        out = device.DeviceTensor.empty((4 * n * K,), np.int32)
        peaks = lambda i: device.call('pvhip_heatmap_peaks_f32', ctypes.c_void_p(xs[i].ptr), n, K, H, W, 1, 1, 0, 0.0, ctypes.c_void_p(out.ptr),  # noqa: E731
                                      ctypes.c_void_p(out.ptr + 4 * n * K), ctypes.c_void_p(out.ptr + 8 * n * K))
        relu = lambda i: device.call('pvhip_relu_f32', ctypes.c_void_p(xs[i].ptr), ctypes.c_void_p(ys[i % 2].ptr), n * K * H * W)    # noqa: E731
        row = {'shape': [n, K, H, W], 'bytes': nbytes, 'form': device.call('pvhip_heatmap_peaks_form', H, W), 'copies_streamed': copies}
        for mode, c in (('resident', 1), ('streamed', copies)):
            us = timed({'peaks': peaks, 'relu': relu}, c)
            (p_us, p_all), (r_us, r_all) = ((float(np.median(us[kind])), us[kind]) for kind in ('peaks', 'relu'))
            row[mode] = {'peaks_us': p_us, 'peaks_read_TBps': nbytes / p_us * 1e-6, 'relu_us': r_us, 'relu_read_TBps': nbytes / r_us * 1e-6,
                         'peaks_vs_relu_read_rate': r_us / p_us, 'peaks_us_per_round': p_all, 'relu_us_per_round': r_all}
        got = np.asarray(out)[:n * K].reshape(n, K)
        assert np.array_equal(got, keypoints.peaks(host).positions), 'the launch timed here does not give the rule\'s positions'
        rows.append(row)
        del xs, ys
    return {'rows': rows, 'launches_per_round': args.launches, 'device': device.device_name()}


def step_passes(args):
    from pyopenvino_amd import IECore, device
    rows = []
    with tempfile.TemporaryDirectory() as folder:
        for n, K, H, W in SHAPES:
            ie = IECore()
            if (K, H, W) == (32, 26, 26):
                xml, weights = mnist_head_ir(folder)
            else:
                xml, weights = head_ir(folder, K, H, W)
            net = ie.read_network(xml, weights=weights)
            net.set_batch(n)
            ex = ie.load_network(net, 'GPU', num_requests=1)
            name, out_name = net.inputs[0]['name'], net.outputs[0]['name']
            shape = (n, 1, 28, 28) if (K, H, W) == (32, 26, 26) else (n, 3, H, W)
            x = device.DeviceTensor.from_numpy(np.random.default_rng(3).uniform(0, 1, shape).astype(np.float32))

            def on_device():
                return ex.infer({name: x}, keypoints=True)[out_name]

            def on_host():
                full = ex.infer({name: x})[out_name]
                flat = full.reshape(n * K, -1)
                at = flat.argmax(axis=1)
                return at, flat[np.arange(n * K), at]

            got, (at, score) = on_device(), on_host()
            assert got.positions.shape == (n, K) and np.array_equal(got.positions.reshape(-1), at)       # (finite: the two routes agree)
            ms = {'keypoints': [], 'read_back_argmax': []}
            handed = {'keypoints': int(sum(a.nbytes for a in got)), 'read_back_argmax': 4 * n * K * H * W}
            for _ in range(args.rounds):
                for kind, run in (('keypoints', on_device), ('read_back_argmax', on_host)):
                    for _ in range(args.warmup):
                        run()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        run()
                    ms[kind].append((time.perf_counter() - t0) * 1e3 / args.steps)
            med = {kind: float(np.median(v)) for kind, v in ms.items()}
            rows.append({'shape': [n, K, H, W], 'ms_per_pass': med, 'ms_per_pass_per_block': ms, 'bytes_handed_back': handed,
                         'keypoints_vs_read_back': med['keypoints'] / med['read_back_argmax'], 'replaying': ex._graph is not None})
            ex.release_device_state()
    return {'rows': rows, 'condition_holds': bool(all(r['ms_per_pass']['keypoints'] < r['ms_per_pass']['read_back_argmax'] for r in rows)),
            'steps_per_block': args.steps, 'rounds': args.rounds}


def git_head(head):
    if head is None:
        try:
            head = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=REPO, capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    return head


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=30, help='timed passes per block')
    ap.add_argument('--warmup', type=int, default=5, help='untimed passes (launches) in front of every block (round)')
    ap.add_argument('--rounds', type=int, default=5, help='blocks per kind, the kinds alternating')
    ap.add_argument('--launches', type=int, default=200, help='timed launches per round of the launch step')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--head', default=None, help='git commit to report (default: git rev-parse HEAD, when the tree is a checkout)')
    ap.add_argument('--step', choices=sorted(STEP_LIMIT), default=None, help='(the child processes) run this step here and print its JSON')
    args = ap.parse_args()
    if args.step:
        print(json.dumps({'launch': step_launch, 'passes': step_passes}[args.step](args)))
        return 0
    line = {'metric': 'keypoints: a heatmap network\'s answer made on the device, batch 256'}
    passed_on = [a for k in ('steps', 'warmup', 'rounds', 'launches') for a in ('--' + k, str(getattr(args, k)))]
    for step in ('launch', 'passes'):
        child = subprocess.run(['timeout', '-k', '10', str(STEP_LIMIT[step]), sys.executable, os.path.abspath(__file__), '--step', step] + passed_on,
                               stdout=subprocess.PIPE, text=True)
        if child.returncode != 0:
            print('bench_keypoints: step {} ended with status {}: nothing further is started'.format(step, child.returncode), file=sys.stderr)
            return child.returncode
        line[step] = json.loads(child.stdout.strip().splitlines()[-1])
    line.update(git_head=git_head(args.head), device=line['launch'].pop('device'), date=time.strftime('%Y-%m-%d'), profiled_with_rocprofv3=False)
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
