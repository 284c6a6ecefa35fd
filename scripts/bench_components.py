"""The connected components of a probability map made on the device (``infer(..., components=...)``): what the call costs beside a
streaming kernel on the same bytes and beside the host route.

One step, a child process under its own `timeout` (the parent never opens the device):

  launch   pvhip_components_f32 alone on device-resident maps -- (32, 1, 640, 640) (a DBNet-style head at batch 32) and (8, 2, 736, 1280)
           (a PixelLink-style head, channel 1) --, a thresholded smooth field (blobs of some hundred pixels, min_score its median), device
           time per call (its five launches) by hipEvents around `--launches` back-to-back calls, with 8-connectivity and R = 256.  Beside
           it pvhip_segment_labels_f32 on the same bytes in the same process, the two alternating over `--rounds` rounds: a kernel that
           reads every score once and writes a byte a pixel.  The answer of image 0 of every timed map is compared with components.find.
           `host`: the whole map read back (page-locked) plus components.find on image 0 times n, the route the keyword replaces.
           Per-launch times are not split here: run the child under ``rocprofv3 --kernel-trace --stats -- python
           scripts/bench_components.py --child --shape I`` for them, one map a process (`--shape`: 0 or 1): flatten and stats have the
           same capped grid for both maps, and a trace of both cannot tell their dispatches apart.

Prints one JSON line; --out writes it too.  e.g.
    python scripts/bench_components.py --out profiles/components.json
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [((32, 1, 640, 640), 0), ((8, 2, 736, 1280), 1)]
STEP_LIMIT = 420                                              # seconds the child may take


def smooth_field(rng, shape):
    """(n, K, H, W) float32 in [0, 1.2): a coarse random field held over 16 x 16 pixels, plus noise that frays the blobs' edges."""
    n, K, H, W = shape
    coarse = rng.random((n, K, H // 16 + 1, W // 16 + 1), dtype=np.float32)
    return (np.kron(coarse, np.ones((16, 16), np.float32))[:, :, :H, :W] + 0.2 * rng.random(shape, dtype=np.float32)).astype(np.float32)


def step_launch(args):
    from pyopenvino_amd import ComponentScreen, components, device
    device.init(0)
    rng = np.random.default_rng(2026)
    e0, e1 = device.Event(), device.Event()
    rows = []
    for (n, K, H, W), channel in (SHAPES if args.shape is None else SHAPES[args.shape:args.shape + 1]):
        x = smooth_field(rng, (n, K, H, W))
        screen = ComponentScreen(float(np.median(x[:, channel])), channel, 8, 1, 256)
        xd = device.DeviceTensor.from_numpy(x)
        blocks = components.Blocks(n, K, H, W, channel, 8, 256)
        labels = device.DeviceTensor.empty(((n * H * W + 3) // 4 + 5 * n * K,), np.int32)
        at = labels.ptr + 4 * ((n * H * W + 3) // 4)
        launches = {'components': lambda: blocks.launch(xd, screen.min_score, screen.min_area),
                    'segment_labels': lambda: device.call('pvhip_segment_labels_f32', ctypes.c_void_p(xd.ptr), n, K, H, W, 1, screen.min_score,
                                                          ctypes.c_void_p(labels.ptr), ctypes.c_void_p(at), ctypes.c_void_p(at + 4 * n * K))}
        launches['components']()
        device.synchronize()
        got, want = blocks.read_back().of(0), components.find(x[:1], screen)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want)), 'the device answer is not the rule\'s'
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
        host = device.host_empty((n, K, H, W), np.float32)
        t0 = time.perf_counter()
        device.call('pvhip_memcpy_d2h', ctypes.c_void_p(host.ctypes.data), ctypes.c_void_p(xd.ptr), host.nbytes)
        device.synchronize()
        t1 = time.perf_counter()
        components.find(host[:1], screen)
        t2 = time.perf_counter()
        row = {'shape': [n, K, H, W], 'channel': channel, 'plane_bytes': 4 * n * H * W, 'scratch_bytes': 12 * n * H * W,
               'found_image_0': int(want.found[0]), 'host': {'read_back_ms': (t1 - t0) * 1e3, 'find_ms_one_image_times_n': (t2 - t1) * 1e3 * n}}
        for kind, v in us.items():
            row[kind] = {'us': float(np.median(v)), 'us_per_round': v, 'spread_us': max(v) - min(v)}
        rows.append(row)
        del xd, blocks, labels
    return {'rows': rows, 'launches_per_round': args.launches, 'device': device.device_name()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--shape', type=int, choices=range(len(SHAPES)), help='only this map (default: both)')
    ap.add_argument('--out')
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print('RESULT ' + json.dumps(step_launch(args)))
        return
    done = subprocess.run(['timeout', '-k', '10', str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), '--child', '--launches', str(args.launches),
                           '--warmup', str(args.warmup), '--rounds', str(args.rounds)] + ([] if args.shape is None else ['--shape', str(args.shape)]), stdout=subprocess.PIPE, text=True)
    if done.returncode != 0:
        sys.exit('the launch step ended with status {}'.format(done.returncode))
    line = json.dumps(json.loads([l for l in done.stdout.splitlines() if l.startswith('RESULT ')][-1][7:]))
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
