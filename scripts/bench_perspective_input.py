"""Projective warps sampled on the device: what two binary64 divisions per pixel cost beside the affine launch on the same geometry.

The rows of scripts/bench_warp_input.py: m = 8 frames of 1080 x 1920, uint8 NHWC and NV12, n = 256 rows -> (256, 3, 224, 224), every row
one seeded 672 x 672 rectangle (scale 3).  One process times, the kinds alternating over `--rounds` rounds, each as `--steps` launches
between two device events after `--warmup` untimed ones:

  warp_scale3         pvhip_input_preprocess_warp_f32, warp.from_roi of the rectangles (upright; 672 = 3 x 224 makes the coefficients whole: its one-tap path)
  warp_rot30          ... the same rectangles turned by 30 degrees about their centres
  perspective_scale3  pvhip_input_preprocess_perspective_f32 on perspective.from_affine of the warp_scale3 matrices
  perspective_rot30   ... of the warp_rot30 matrices
  perspective_keystone  ... perspective.from_quad of a trapezoid in each rectangle: the top edge 0.6 of the bottom one

Prints one JSON line.  --out FILE.md writes the table in markdown.  --kernel KIND: only that kind's launches, the run to take under
rocprofv3.  PVHIP_LIBRARY names another build of the library (one that has both entries).
Run each GPU step under its own time limit, e.g.  timeout -k 10 300 python scripts/bench_perspective_input.py --out profiles/perspective_input.md
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pyopenvino_amd import PerspectiveInput, WarpInput, device, perspective, warp  # noqa: E402
from bench_preprocess_yuv import frames, git_head, timed  # noqa: E402
from bench_warp_input import DST, FORMATS, FRAME, M, N, SIDE, ptr, rectangles  # noqa: E402

CASES = ('scale3', 'rot30', 'keystone')


def tables(rng):
    """{case: (the (N, 7) int64 warp table or None, the (N, 10) int64 perspective table)} over one set of rectangles."""
    rects = rectangles(rng, SIDE)
    ids = rects[:, :1].astype(np.int64)
    affine = {'scale3': np.stack([warp.from_roi(r[1:], DST) for r in rects]),
              'rot30': np.stack([warp.rotated_rect(r[1] + SIDE / 2, r[2] + SIDE / 2, SIDE, SIDE, 30.0, DST) for r in rects])}
    homography = {case: np.stack([perspective.from_affine(a) for a in m]) for case, m in affine.items()}
    homography['keystone'] = np.stack([perspective.from_quad(
        [[x + 0.2 * SIDE, y], [x + 0.8 * SIDE, y], [x + SIDE - 1.0, y + SIDE - 1.0], [x, y + SIDE - 1.0]], DST) for _, x, y, _, _ in rects])
    return {case: (np.concatenate([ids, WarpInput.fixed(affine[case])], 1) if case in affine else None,
                   np.concatenate([ids, PerspectiveInput.fixed(homography[case], DST)], 1)) for case in CASES}


def measure(args):
    device.init(0)
    rng = np.random.default_rng(2026)
    (hs, ws), (hd, wd) = FRAME, DST
    dst = device.DeviceTensor.empty((N, 3, hd, wd))
    d = ptr(dst)
    dev = {case: tuple(None if t is None else device.DeviceTensor.from_numpy(t) for t in pair) for case, pair in tables(rng).items()}
    out = {}
    for fmt, (form, how, _) in FORMATS.items():
        src = device.DeviceTensor.from_numpy(frames(rng, M, hs, ws, 'bgr' if fmt == 'u8' else 'nv12'))
        s = ptr(src)
        launch = {}
        for case in CASES:
            for family, table in zip(('warp', 'perspective'), dev[case]):
                if table is not None:
                    launch['{}_{}_{}'.format(family, fmt, case)] = (lambda family=family, table=table: device.call(
                        'pvhip_input_preprocess_{}_f32'.format(family), s, d, ptr(table), N, M, 3, hs, ws, hd, wd, form, how, 0, None, None, 0.0))
        if args.kernel:
            launch = {k: v for k, v in launch.items() if k == args.kernel}
        us = {kind: [] for kind in launch}
        for _ in range(args.rounds):
            for kind in launch:
                us[kind].append(timed(launch[kind], args.steps, args.warmup))
        for kind, rounds in us.items():
            out[kind] = {'launch_us': float(np.median(rounds)), 'launch_us_per_round': rounds}
        del src
    return out


def markdown(line):
    rows = ['# PerspectiveInput: the perspective launch beside the affine launch', '',
            '`python scripts/bench_perspective_input.py` on {} ({}, {}): {} frames of {} x {}, {} rows -> (256, 3, 224, 224) fp32; medians of '
            '{} rounds of {} launches between device events, the kinds alternating in one process.'.format(
                line['device'], line['date'], line['git_head'], M, FRAME[0], FRAME[1], N, line['rounds'], line['launches_per_round']), '',
            '| kind | us per launch | min .. max over rounds | perspective / warp |', '|---|---|---|---|']
    for kind, v in line['kinds'].items():
        yard = line['kinds'].get(kind.replace('perspective_', 'warp_'))
        ratio = '{:.2f}'.format(v['launch_us'] / yard['launch_us']) if kind.startswith('perspective_') and yard else ''
        rows.append('| {} | {:.1f} | {:.1f} .. {:.1f} | {} |'.format(kind, v['launch_us'], min(v['launch_us_per_round']), max(v['launch_us_per_round']), ratio))
    return '\n'.join(rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=100, help='timed launches per kind and round')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5, help='rounds over the kinds (alternating, one process)')
    ap.add_argument('--kernel', default=None, help='only the launches of this kind, e.g. perspective_u8_rot30 (see above)')
    ap.add_argument('--out', default=None, help='write the markdown table to this file')
    ap.add_argument('--head', default=None, help='git commit to report (default: git rev-parse HEAD, when the tree is a checkout)')
    args = ap.parse_args()
    kinds = measure(args)
    line = {'metric': 'projective warps -> (256, 3, 224, 224) fp32 beside the affine launch on the same geometry, event-timed', 'kinds': kinds,
            'launches_per_round': args.steps, 'rounds': args.rounds, 'git_head': git_head(args.head), 'device': device.device_name(),
            'library': os.environ.get('PVHIP_LIBRARY', 'this build'), 'date': time.strftime('%Y-%m-%d'), 'profiled_with_rocprofv3': False}
    print(json.dumps(line))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(markdown(line) + '\n')


if __name__ == '__main__':
    main()
