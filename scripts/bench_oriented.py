"""An oriented detector head decoded on the device (``infer(..., boxes=OrientedBoxScreen(...))``): what the entry costs beside boxes= on a
head of the same extent without the angle, and beside the host route.

One Result at n = 32: (32, 20, 21504) 'NCA', a YOLOv8-obb export for DOTA at 1024 x 1024 (15 classes).  Seeded numbers shaped like a
detector's: class scores of a few thousandths, and on about 300 anchors per image, in clusters around 30 objects, one class raised to
0.3 .. 0.95; boxes in pixels of the 1024 x 1024 input, angles in [-pi / 2, pi / 2), those of a cluster close to one another.  Two
regimes, both at max_candidates 1024: `realistic`, min_score 0.25 (about 300 candidates per image); `full`, min_score 0, where every
anchor passes, the keep buffer cuts and 1024 candidates per image are suppressed.  One step, a child process under its own `timeout` (the
parent never opens the device):

  launch   pvhip_oriented_boxes_f32 (its three launches) on a device-resident tensor, device time per call by hipEvents around
           `--launches` back-to-back calls, beside pvhip_dense_boxes_f32 on (32, 19, 21504) -- the same anchors without the angle channel --
           the two alternating over `--rounds` rounds.  And the host route on the same tensor, once: the whole tensor read back
           (np.asarray of the device tensor) and oriented.decode, the same rule in numpy, host-clocked apart; its answer must equal the
           entry's.  `--regime` keeps one regime and `--only-oriented` drops the other kinds: what a kernel trace (rocprofv3
           --kernel-trace --stats around `--step launch`), a run of its own, is taken on.

Prints one JSON line; --out writes it too.  e.g.  python scripts/bench_oriented.py --out profiles/oriented.json
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

SHAPE, CLASSES, EXTENT = (32, 20, 21504), 15, 1024
REGIMES = {'realistic': dict(min_score=0.25, max_candidates=1024), 'full': dict(min_score=0.0, max_candidates=1024)}
STEP_LIMIT = {'launch': 900}                                  # seconds the child may take


def head(rng, n, A, C):
    """(n, A, 4 + C + 1) numbers shaped like an oriented detector's."""
    v = np.empty((n, A, 4 + C + 1), np.float32)
    objects, sizes = rng.random((n, 30, 2)) * EXTENT, 20 + rng.random((n, 30, 2)) * 180
    turn = (rng.random((n, 30)) - 0.5) * np.pi
    v[:, :, 0:2] = rng.random((n, A, 2)) * EXTENT
    v[:, :, 2:4] = 10 + rng.random((n, A, 2)) * 100
    v[:, :, 4:4 + C] = rng.random((n, A, C)) * 0.01
    v[:, :, -1] = (rng.random((n, A)) - 0.5) * np.pi
    for r in range(n):
        at = rng.permutation(A)[:300]
        which = rng.integers(0, 30, len(at))
        v[r, at, 0:2] = objects[r, which] + rng.normal(0, 4, (len(at), 2))
        v[r, at, 2:4] = sizes[r, which] * (1 + rng.normal(0, 0.05, (len(at), 2)))
        v[r, at, 4 + (which % C)] = 0.3 + rng.random(len(at)) * 0.65
        v[r, at, -1] = turn[r, which] + rng.normal(0, 0.05, len(at))
    return v


def step_launch(args):
    from pyopenvino_amd import BoxScreen, OrientedBoxScreen, boxes, device, oriented
    device.init(0)
    rng = np.random.default_rng(2026)
    e0, e1 = device.Event(), device.Event()
    n, _, A = SHAPE
    v = head(rng, n, A, CLASSES)
    x = device.DeviceTensor.from_numpy(np.ascontiguousarray(v.transpose(0, 2, 1)))
    plain = device.DeviceTensor.from_numpy(np.ascontiguousarray(v[:, :, :-1].transpose(0, 2, 1)))
    geometry = ((EXTENT, EXTENT), (0, 0, EXTENT, EXTENT))
    rows = []
    for regime, fields in REGIMES.items():
        if args.regime not in (None, regime):
            continue
        screen = oriented.resolved(OrientedBoxScreen(layout='NCA', **fields))
        blocks = oriented.Blocks(n, A, screen)
        launches = {'oriented': lambda: blocks.launch(x, screen.min_score, *geometry)}
        if not args.only_oriented:
            beside = boxes.resolved(BoxScreen(layout='NCA', **fields))
            beside_blocks = boxes.Blocks(n, A, beside)
            launches['boxes'] = lambda: beside_blocks.launch(plain, beside.min_score, *geometry)
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
        got = blocks.read_back()
        row = {'shape': list(SHAPE), 'regime': regime, 'bytes': 4 * n * A * SHAPE[1], 'min_score': screen.min_score,
               'max_candidates': screen.max_candidates, 'selected_per_image': float(got.selected.mean()), 'rows_per_image': float(got.counts.mean()),
               'read_back_bytes': 4 * (2 * n + 1) + 4 * oriented.ROW_WORDS * int(got.counts.sum())}
        for kind, t in us.items():
            row.update({kind + '_us': float(np.median(t)), kind + '_spread_us': max(t) - min(t), kind + '_us_per_round': t})
        if not args.only_oriented:
            t0 = time.perf_counter()
            whole = np.asarray(x)
            t1 = time.perf_counter()
            want = oriented.decode(whole, screen, (EXTENT, EXTENT))
            t2 = time.perf_counter()
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want)), 'the entry timed here does not give the rule\'s answer'
            row.update(host_read_back_ms=(t1 - t0) * 1e3, host_decode_ms=(t2 - t1) * 1e3, boxes_rows_per_image=float(beside_blocks.read_back().counts.mean()))
        rows.append(row)
    return {'rows': rows, 'launches_per_round': args.launches, 'device': device.device_name()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--warmup', type=int, default=3, help='untimed calls in front of every round')
    ap.add_argument('--rounds', type=int, default=5, help='rounds per kind, the kinds alternating')
    ap.add_argument('--launches', type=int, default=20, help='timed calls per round')
    ap.add_argument('--regime', choices=sorted(REGIMES), default=None, help='this regime only')
    ap.add_argument('--only-oriented', action='store_true', help='neither boxes= beside it nor the host route')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--step', choices=sorted(STEP_LIMIT), default=None, help='(the child process) run this step here and print its JSON')
    args = ap.parse_args()
    if args.step:
        print(json.dumps({'launch': step_launch}[args.step](args)))
        return 0
    passed_on = [a for k in ('warmup', 'rounds', 'launches') for a in ('--' + k, str(getattr(args, k)))]
    passed_on += (['--regime', args.regime] if args.regime else []) + (['--only-oriented'] if args.only_oriented else [])
    child = subprocess.run(['timeout', '-k', '10', str(STEP_LIMIT['launch']), sys.executable, os.path.abspath(__file__), '--step', 'launch'] + passed_on,
                           stdout=subprocess.PIPE, text=True)
    if child.returncode != 0:
        print('bench_oriented: step launch ended with status {}: nothing further is started'.format(child.returncode), file=sys.stderr)
        return child.returncode
    line = {'metric': 'boxes: an oriented detector head decoded on the device', 'launch': json.loads(child.stdout.strip().splitlines()[-1])}
    line.update(device=line['launch'].pop('device'), date=time.strftime('%Y-%m-%d'), profiled_with_rocprofv3=False)
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
