"""Instance masks in frame pixels (``masks=MaskScreen(space='FRAME')``): what pvhip_frame_masks_f32 costs, per launch, per grid size,
and beside the host route.

The workload of scripts/bench_masks.py: the head (32, 116, 8400) 'NCA' and the prototypes (32, 32, 160, 160), about 95 kept boxes per
image, here over 1920 x 1080 frames letterboxed into the 640 x 640 input: fit = (0, 140, 640, 360).  One step, a child process under its
own `timeout` (the parent never opens the device):

  launch   the entry behind one pvhip_dense_boxes_tail_f32 call on device-resident tensors, device time per call by hipEvents around
           `--launches` back-to-back calls, `--rounds` rounds, for the entry's own grid and for 1, 2, 3 and 4 workgroups per compute unit.
           `plan` is the same call with max_words = 1: launch (1) in full and a launch (2) that finds no band, so call - plan is what the
           bands cost.  The words of the entry's own grid are held against masks.make_frame for the first rows.
           The host route on the same tensors, `--host-rounds` times: both tensors read back, then masks.make_frame -- the exact rule in
           numpy over each box's own window of the planes -- host-clocked.
           PVHIP_LIBRARY names another build of the library (one with another PVHIP_FRAME_MASKS_LDS_FLOATS) to time the same way.

Prints one JSON line; --out writes it too.  e.g.  python scripts/bench_frame_masks.py --out profiles/frame_masks.json
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
sys.path.insert(0, os.path.join(REPO, 'scripts'))

N, C, T, ANCHORS, EXTENT, PLANE = 32, 80, 32, 8400, 640, (160, 160)
FRAME, FIT = (1080, 1920), (0, 140, 640, 360)
CUS, GRIDS = 256, (0, 1, 2, 3, 4)                             # workgroups per compute unit; 0: the entry's own choice
HBM_TBPS = 8.0                                                # the board's peak HBM rate
PROTOTYPE_SPACE_US = 178.0                                    # profiles/masks.md: pvhip_instance_masks_f32 on this workload
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
    head_blocks = boxes.Blocks(N, ANCHORS, screen)
    blocks, cut = masks.FrameBlocks(N, screen.max_per_image, (T,) + PLANE, args.max_words), masks.FrameBlocks(N, screen.max_per_image, (T,) + PLANE, 1)
    head_blocks.launch(x, screen.min_score, FRAME, FIT)
    kinds = {'grid_{}'.format(g): (lambda g=g: blocks.launch(protos, x, head_blocks, screen, (EXTENT, EXTENT), FRAME, FIT, g * CUS)) for g in GRIDS}
    kinds['plan'] = lambda: cut.launch(protos, x, head_blocks, screen, (EXTENT, EXTENT), FRAME, FIT)
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
    kinds['grid_0']()
    found, got = head_blocks.read_back(), blocks.read_back()
    some = min(48, got.made)
    want = masks.make_frame(head_host, protos_host, found._replace(rois=found.rois[:some], records=found.records[:some]), screen, (EXTENT, EXTENT), FRAME, FIT)
    assert np.array_equal(got.words[:len(want.words)], want.words) and want.words.any(), 'the launch timed here does not give the rule\'s words'
    host_ms = []
    for _ in range(args.host_rounds):
        t0 = time.perf_counter()
        masks.make_frame(np.asarray(x), np.asarray(protos), found, screen, (EXTENT, EXTENT), FRAME, FIT, args.max_words)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(t)) for k, t in us.items()}
    call, words = med['grid_0'], len(got.words)
    return {'head': [N, 4 + C + T, ANCHORS], 'prototypes': [N, T] + list(PLANE), 'frame': list(FRAME), 'fit': list(FIT), 'rows': len(found.rois),
            'rows_per_image': float(found.counts.mean()), 'made': got.made, 'words': words, 'pixels': int((found.rois[:got.made, 3].astype(np.int64) * found.rois[:got.made, 4]).sum()),
            'read_back_bytes': 4 * (2 * N + 1) + 32 * len(found.rois) + 8 + 4 * words, 'call_us': call, 'plan_us': med['plan'], 'bands_us': call - med['plan'],
            'words_per_second': words / call * 1e6, 'write_TBps': 4 * words / call * 1e-6, 'write_vs_hbm_peak': 4 * words / call * 1e-6 / HBM_TBPS,
            'us_by_workgroups_per_cu': {k: med[k] for k in med if k.startswith('grid_')}, 'prototype_space_us': PROTOTYPE_SPACE_US, 'vs_prototype_space': call / PROTOTYPE_SPACE_US,
            'host_route_ms': float(np.median(host_ms)) if host_ms else None, 'host_vs_device': float(np.median(host_ms)) * 1e3 / call if host_ms else None,
            'library': os.environ.get('PVHIP_LIBRARY', 'libpvhip.so'), 'us_per_round': us, 'host_route_ms_per_round': host_ms, 'launches_per_round': args.launches,
            'device': device.device_name()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--warmup', type=int, default=3, help='untimed calls in front of every round')
    ap.add_argument('--rounds', type=int, default=5, help='rounds per kind, the kinds alternating')
    ap.add_argument('--launches', type=int, default=20, help='timed calls per round')
    ap.add_argument('--host-rounds', type=int, default=1, help='times the host route runs')
    ap.add_argument('--max-words', type=int, default=1 << 24, help='MaskScreen.max_words')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--step', choices=sorted(STEP_LIMIT), default=None, help='(the child process) run this step here and print its JSON')
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step_launch(args)))
        return 0
    passed_on = [a for k in ('warmup', 'rounds', 'launches', 'host_rounds', 'max_words') for a in ('--' + k.replace('_', '-'), str(getattr(args, k)))]
    child = subprocess.run(['timeout', '-k', '10', str(STEP_LIMIT['launch']), sys.executable, os.path.abspath(__file__), '--step', 'launch'] + passed_on,
                           stdout=subprocess.PIPE, text=True)
    if child.returncode != 0:
        print('bench_frame_masks: the launch step ended with status {}: nothing further is started'.format(child.returncode), file=sys.stderr)
        return child.returncode
    line = {'metric': 'frame masks: instance masks in frame pixels made on the device', 'launch': json.loads(child.stdout.strip().splitlines()[-1]),
            'date': time.strftime('%Y-%m-%d')}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
