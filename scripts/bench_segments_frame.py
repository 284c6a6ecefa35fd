"""Segmentation maps in frame pixels (``segments=FrameSegmentScreen(...)``): what pvhip_segment_frame_labels_f32 costs, beside
``segments=True`` and beside the host route.

Two workloads on seeded normal scores: `deeplab`, (8, 21, 129, 129) from a 513 x 513 network onto 1920 x 1080 frames letterboxed into it,
and `cityscapes`, (8, 19, 128, 256) from a 512 x 1024 network onto 2048 x 1024 frames.  One step, a child process under its own `timeout`
(the parent never opens the device):

  launch   per workload, on a device-resident tensor, device time per call by hipEvents around `--launches` back-to-back calls,
           `--rounds` rounds, the kinds alternating: `frame`, the entry onto the frames; `identity`, the entry with frame == network == map
           extent; `segments`, pvhip_segment_labels_f32 on the same tensor, whose answer the identity call must equal byte for byte.
           The host route on the same tensor, `--host-rounds` times, host-clocked: the whole tensor read back, then
           segments.frame_labels, the exact rule in numpy; its answer must equal the entry's.

Prints one JSON line; --out writes it too.  e.g.  python scripts/bench_segments_frame.py --out profiles/segments_frame.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WORKLOADS = {'deeplab': ((8, 21, 129, 129), (513, 513), (1080, 1920), 'LETTERBOX'),       # (map, network, frame, fit)
             'cityscapes': ((8, 19, 128, 256), (512, 1024), (1024, 2048), 'STRETCH')}
HBM_TBPS = 8.0                                                # the board's peak HBM rate
STEP_LIMIT = {'launch': 900}                                  # seconds the child may take


def step_launch(args):
    from pyopenvino_amd import device, segments
    from pyopenvino_amd.input_format import fit_geometry
    device.init(0)
    out = {}
    for name, (shape, net, frame, fit_kind) in WORKLOADS.items():
        n, C, H, W = shape
        host = np.random.default_rng(2026).standard_normal(shape).astype(np.float32)
        x = device.DeviceTensor.from_numpy(host)
        fit = tuple(int(v) for v in fit_geometry(frame, net, fit_kind))
        onto, same, plain = segments.FrameBlocks(n, C, H, W, frame), segments.FrameBlocks(n, C, H, W, (H, W)), segments.Blocks(n, C, H, W)
        kinds = {'frame': lambda: onto.launch(x, None, net, frame, fit), 'identity': lambda: same.launch(x, None, (H, W), (H, W), (0, 0, W, H)),
                 'segments': lambda: plain.launch(x, None)}
        e0, e1, us = device.Event(), device.Event(), {k: [] for k in kinds}
        for _ in range(args.rounds):
            for kind, launch in kinds.items():
                for _ in range(args.warmup):
                    launch()
                e0.record()
                for _ in range(args.launches):
                    launch()
                e1.record()
                e1.synchronize()
                us[kind].append(e0.elapsed_ms(e1) * 1e3 / args.launches)
        got, at_map, want_map = onto.read_back(), same.read_back(), plain.read_back()
        assert all(np.array_equal(a, b) for a, b in zip(at_map, want_map)), 'the identity geometry does not give segments=True\'s answer'
        host_ms = []
        for _ in range(args.host_rounds):
            t0 = time.perf_counter()
            want = segments.frame_labels(np.asarray(x), True, net, frame, fit)
            host_ms.append((time.perf_counter() - t0) * 1e3)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), 'the launch timed here does not give the rule\'s answer'
        med = {k: float(np.median(t)) for k, t in us.items()}
        pixels = n * frame[0] * frame[1]
        out[name] = {'map': list(shape), 'network': list(net), 'frame': list(frame), 'fit': list(fit),
                     'form': device.call('pvhip_segment_frame_labels_form', C, H, W, net[0], net[1], frame[0], frame[1], *fit),
                     'frame_us': med['frame'], 'identity_us': med['identity'], 'segments_us': med['segments'],
                     'identity_vs_segments': med['identity'] / med['segments'], 'frame_pixels': pixels,
                     'label_store_TBps': pixels / med['frame'] * 1e-6, 'label_store_vs_hbm_peak': pixels / med['frame'] * 1e-6 / HBM_TBPS,
                     'samples_per_second': pixels * C / med['frame'] * 1e6, 'read_back_bytes': 4 * ((pixels + 3) // 4) + 20 * n * C,
                     'tensor_bytes': host.nbytes, 'host_route_ms': float(np.median(host_ms)) if host_ms else None,
                     'host_vs_device': float(np.median(host_ms)) * 1e3 / med['frame'] if host_ms else None,
                     'spread_us': {k: [float(min(t)), float(max(t))] for k, t in us.items()}, 'us_per_round': us, 'host_route_ms_per_round': host_ms}
    return {'workloads': out, 'launches_per_round': args.launches, 'rounds': args.rounds, 'device': device.device_name()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--warmup', type=int, default=3, help='untimed calls in front of every round')
    ap.add_argument('--rounds', type=int, default=5, help='rounds per kind, the kinds alternating')
    ap.add_argument('--launches', type=int, default=20, help='timed calls per round')
    ap.add_argument('--host-rounds', type=int, default=1, help='times the host route runs')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--step', choices=sorted(STEP_LIMIT), default=None, help='(the child process) run this step here and print its JSON')
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step_launch(args)))
        return 0
    passed_on = [a for k in ('warmup', 'rounds', 'launches', 'host_rounds') for a in ('--' + k.replace('_', '-'), str(getattr(args, k)))]
    child = subprocess.run(['timeout', '-k', '10', str(STEP_LIMIT['launch']), sys.executable, os.path.abspath(__file__), '--step', 'launch'] + passed_on,
                           stdout=subprocess.PIPE, text=True)
    if child.returncode != 0:
        print('bench_segments_frame: the launch step ended with status {}: nothing further is started'.format(child.returncode), file=sys.stderr)
        return child.returncode
    line = {'metric': 'segments in frame pixels: the class map of a segmentation Result made on the device', 'launch': json.loads(child.stdout.strip().splitlines()[-1]),
            'date': time.strftime('%Y-%m-%d')}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
