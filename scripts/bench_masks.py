"""Instance masks on the device (``infer(..., boxes=BoxScreen(tail=32), masks=True)``): what the masks launch costs beside the kernel
already in the tree that streams the same prototype bytes, and beside the host route.

One pair of Results at n = 32: the head (32, 116, 8400) 'NCA' (a YOLOv8-seg export at 640 x 640: 4 + 80 + 32 channels) and the prototypes
(32, 32, 160, 160).  Seeded numbers shaped like a detector's (bench_boxes.head) with about 100 kept boxes per image (95: threshold 0.81), coefficients and
prototypes standard normal.  One step, a child process under its own `timeout` (the parent never opens the device):

  launch   pvhip_instance_masks_f32 behind one pvhip_dense_boxes_tail_f32 call on device-resident tensors, device time per call by
           hipEvents around `--launches` back-to-back calls, beside pvhip_segment_labels_f32 on the prototype tensor -- the launch that
           reads the same 105 MB once --, the two alternating over `--rounds` rounds.  The yardstick is the prototype bytes over that
           launch's rate: masks_vs_beside.  The tail entry is timed the same way on its own.  The prototypes (105 MB) stay in the
           Infinity Cache between launches, as a Result the pass has just written does.
           And the host route on the same tensors, `--host-rounds` times: both tensors read back (np.asarray of the device tensors),
           boxes.decode's table taken as given, and the matrix product as its users write it -- float32 `coefficients @ prototypes`
           > 0, cropped -- host-clocked.  (masks.make, the exact rule in numpy, is far slower and checks the launch's words once.)

Prints one JSON line; --out writes it too.  e.g.  python scripts/bench_masks.py --out profiles/masks.json
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
sys.path.insert(0, os.path.join(REPO, 'scripts'))

N, C, T, ANCHORS, EXTENT, PLANE = 32, 80, 32, 8400, 640, (160, 160)
STEP_LIMIT = {'launch': 900}                                  # seconds the child may take


def step_launch(args):
    import bench_boxes
    from pyopenvino_amd import BoxScreen, boxes, device, masks
    device.init(0)
    rng = np.random.default_rng(2026)
    v = np.concatenate([bench_boxes.head(rng, N, ANCHORS, C, False, EXTENT), rng.standard_normal((N, ANCHORS, T)).astype(np.float32)], axis=2)
    head_host = np.ascontiguousarray(v.transpose(0, 2, 1))
    protos_host = rng.standard_normal((N, T) + PLANE).astype(np.float32)
    x, protos = device.DeviceTensor.from_numpy(head_host), device.DeviceTensor.from_numpy(protos_host)
    screen = boxes.resolved(BoxScreen(0.25, 'NCA', tail=T, threshold=0.81, max_per_image=128))
    head_blocks, mask_blocks = boxes.Blocks(N, ANCHORS, screen), masks.Blocks(N, screen.max_per_image, (T,) + PLANE)
    launch_boxes = lambda: head_blocks.launch(x, screen.min_score, (EXTENT, EXTENT), (0, 0, EXTENT, EXTENT))        # noqa: E731
    launch_masks = lambda: mask_blocks.launch(protos, x, head_blocks, screen, (EXTENT, EXTENT), True)               # noqa: E731
    seg_out = device.DeviceTensor.empty(((N * PLANE[0] * PLANE[1] + 3) // 4 + 5 * N * T,), np.int32)
    beside = lambda: device.call('pvhip_segment_labels_f32', ctypes.c_void_p(protos.ptr), N, T, PLANE[0], PLANE[1], 0, 0.0,  # noqa: E731
                                 ctypes.c_void_p(seg_out.ptr + 20 * N * T), ctypes.c_void_p(seg_out.ptr), ctypes.c_void_p(seg_out.ptr + 4 * N * T))
    launch_boxes()
    e0, e1, us = device.Event(), device.Event(), {'masks': [], 'beside': [], 'boxes_tail': []}
    for _ in range(args.rounds):
        for kind, launch in (('masks', launch_masks), ('beside', beside), ('boxes_tail', launch_boxes)):
            for _ in range(args.warmup):
                launch()
            e0.record()
            for _ in range(args.launches):
                launch()
            e1.record()
            e1.synchronize()
            us[kind].append(e0.elapsed_ms(e1) * 1e3 / args.launches)
    found, got = head_blocks.read_back(), mask_blocks.read_back()
    some = min(64, len(found.records))                          # (the exact rule in numpy takes 8 bytes x 10 temporaries a pixel and row)
    want = masks.make(head_host, protos_host, found._replace(rois=found.rois[:some], records=found.records[:some]), screen, (EXTENT, EXTENT))
    assert np.array_equal(got.words[:some], want.words) and got.words.any(), 'the launch timed here does not give the rule\'s words'
    host_ms, hw = [], PLANE[0] * PLANE[1]
    for _ in range(args.host_rounds):
        t0 = time.perf_counter()
        h, p = np.asarray(x), np.asarray(protos).reshape(N, T, hw)
        r = found.rois[:, 0]
        e = h[r, :, found.records - r * ANCHORS]
        bits = np.concatenate([e[r == i, 4 + C:] @ p[i] > 0 for i in range(N)]).reshape(-1, *PLANE)
        ys, xs = np.arange(PLANE[0])[None, :, None] * 4, np.arange(PLANE[1])[None, None, :] * 4
        xa, xb, ya, yb = ((e[:, i] + s * e[:, j] / 2)[:, None, None] for i, j, s in ((0, 2, -1), (0, 2, 1), (1, 3, -1), (1, 3, 1)))
        bits &= (xs >= xa) & (xs < xb) & (ys >= ya) & (ys < yb)
        np.packbits(bits.reshape(len(r), -1), axis=1, bitorder='little')
        host_ms.append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(t)) for k, t in us.items()}
    nbytes = 4 * N * T * hw
    return {'head': [N, 4 + C + T, ANCHORS], 'prototypes': [N, T] + list(PLANE), 'rows_per_image': float(found.counts.mean()), 'prototype_bytes': nbytes,
            'head_bytes': int(head_host.nbytes), 'read_back_bytes': 4 * (2 * N + 1) + int(found.counts.sum()) * (32 + 4 * got.words.shape[1]),
            'masks_us': med['masks'], 'masks_read_TBps': nbytes / med['masks'] * 1e-6, 'beside': 'pvhip_segment_labels_f32', 'beside_us': med['beside'],
            'beside_read_TBps': nbytes / med['beside'] * 1e-6, 'masks_vs_beside': med['masks'] / med['beside'], 'boxes_tail_us': med['boxes_tail'],
            'host_route_ms': float(np.median(host_ms)), 'host_vs_device': float(np.median(host_ms)) * 1e3 / (med['masks'] + med['boxes_tail']),
            'us_per_round': us, 'host_route_ms_per_round': host_ms, 'launches_per_round': args.launches, 'device': device.device_name()}


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
        print('bench_masks: the launch step ended with status {}: nothing further is started'.format(child.returncode), file=sys.stderr)
        return child.returncode
    line = {'metric': 'masks: instance masks made on the device', 'launch': json.loads(child.stdout.strip().splitlines()[-1]), 'date': time.strftime('%Y-%m-%d')}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
