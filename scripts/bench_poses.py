"""Multi-person poses grouped on the device (``infer(..., maxima=..., poses=...)``): what the call costs beside the host route.

One step, a child process under its own `timeout` (the parent never opens the device):

  launch   pvhip_pose_groups_f32 alone (its two launches) on device-resident OPENPOSE18 heads -- heatmaps (32, 19, H, W) and fields
           (32, 38, H, W) at 32 x 57 and at 128 x 128, with about 5 and about 20 painted people an image (a peak per joint, the limb's unit
           vector in a band along each limb, noise below the thresholds) --, behind one pvhip_heatmap_maxima_f32 call that left the
           candidates: device time per call by hipEvents around `--launches` back-to-back calls, the median of `--rounds` rounds and
           their spread.  Beside it the maxima call on the same heatmaps, timed the same way.  The answer of image 0 is compared with
           poses.group.  `host`: both tensors read back (page-locked) plus poses.group on image 0 times n, the route the keyword replaces.
           The two launches are not split here: run the child under ``rocprofv3 --kernel-trace --stats -- python scripts/bench_poses.py
           --child --row I`` for them, one row a process.

Prints one JSON line; --out writes it too.  e.g.
    python scripts/bench_poses.py --out profiles/poses.json
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

ROWS = [((32, 57), 5), ((32, 57), 20), ((128, 128), 5), ((128, 128), 20)]
N = 32
STEP_LIMIT = 420                                              # seconds the child may take


def painted(rng, hw, people, skeleton):
    """Heatmaps (N, 19, H, W) and fields (N, 38, H, W): `people` persons an image, their 18 joints scattered over a box of a quarter of the plane."""
    from pyopenvino_amd import synth
    H, W = hw
    heat, pafs = (0.05 * rng.random((N, 19, H, W), dtype=np.float32)), (0.02 * rng.standard_normal((N, 38, H, W))).astype(np.float32)
    rows = []
    for r in range(N):
        rows.append([])
        for _ in range(people):
            cx, cy = rng.integers(W // 8, W - W // 8), rng.integers(H // 8, H - H // 8)
            rows[r].append({k: (int(np.clip(cx + rng.integers(-W // 8, W // 8 + 1), 1, W - 2)), int(np.clip(cy + rng.integers(-H // 8, H // 8 + 1), 1, H - 2)))
                            for k in range(18)})
    return synth.paint_poses(heat, pafs, skeleton, rows, lambda r, q, k: 0.5 + 0.5 * rng.random())


def step_launch(args):
    from pyopenvino_amd import MaximaScreen, PoseScreen, device, maxima, poses
    device.init(0)
    rng = np.random.default_rng(2026)
    e0, e1 = device.Event(), device.Event()
    rows = []
    for hw, people in (ROWS if args.row is None else ROWS[args.row:args.row + 1]):
        heat, pafs = painted(rng, hw, people, poses.OPENPOSE18)
        heat_screen, screen = maxima.for_planes(maxima.resolved(MaximaScreen(0.3, 32)), N, 19), poses.resolved(PoseScreen(max_persons=32))
        table = poses.skeleton_for(screen, 19, 38)
        hd, pd = device.DeviceTensor.from_numpy(heat), device.DeviceTensor.from_numpy(pafs)
        found = maxima.Blocks(N, 19, heat_screen.max_per_plane, heat_screen.max_per_row, heat_screen.refine, heat_screen.space)
        blocks = poses.Blocks(N, 19, screen.max_persons, len(table))
        launches = {'poses': lambda: blocks.launch(pd, hd, found.scratch, heat_screen, screen, table),
                    'maxima': lambda: found.launch(hd, heat_screen.min_score)}
        launches['maxima']()
        launches['poses']()
        device.synchronize()
        got, want = blocks.read_back(), poses.group(heat[:1], pafs[:1], heat_screen, screen)
        assert all(np.array_equal(a[:1].view(np.uint32), b.view(np.uint32)) for a, b in zip(got, want)), 'the device answer is not the rule\'s'
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
        host = device.host_empty(heat.shape, np.float32), device.host_empty(pafs.shape, np.float32)
        t0 = time.perf_counter()
        for to, src in zip(host, (hd, pd)):
            device.call('pvhip_memcpy_d2h', ctypes.c_void_p(to.ctypes.data), ctypes.c_void_p(src.ptr), to.nbytes)
        device.synchronize()
        t1 = time.perf_counter()
        poses.group(host[0][:1], host[1][:1], heat_screen, screen)
        t2 = time.perf_counter()
        row = {'plane': list(hw), 'people_painted': people, 'persons_mean': float(got.counts.mean()), 'bytes_read_back_by_the_host_route': heat.nbytes + pafs.nbytes,
               'host': {'read_back_ms': (t1 - t0) * 1e3, 'group_ms_one_image_times_n': (t2 - t1) * 1e3 * N}}
        for kind, v in us.items():
            row[kind] = {'us': float(np.median(v)), 'us_per_round': v, 'spread_us': max(v) - min(v)}
        rows.append(row)
        del hd, pd, found, blocks
    return {'rows': rows, 'n': N, 'launches_per_round': args.launches, 'device': device.device_name()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--row', type=int, choices=range(len(ROWS)), help='only this row (default: all)')
    ap.add_argument('--out')
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print('RESULT ' + json.dumps(step_launch(args)))
        return
    done = subprocess.run(['timeout', '-k', '10', str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), '--child', '--launches', str(args.launches),
                           '--warmup', str(args.warmup), '--rounds', str(args.rounds)] + ([] if args.row is None else ['--row', str(args.row)]), stdout=subprocess.PIPE, text=True)
    if done.returncode != 0:
        sys.exit('the launch step ended with status {}'.format(done.returncode))
    line = json.dumps(json.loads([l for l in done.stdout.splitlines() if l.startswith('RESULT ')][-1][7:]))
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
