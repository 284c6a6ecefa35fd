"""Affine warps sampled on the device: what the warp launch costs beside the ROI launch on the equivalent upright rectangles.

m = 8 frames of 1080 x 1920, uint8 NHWC and NV12, and n = 256 rows -> (256, 3, 224, 224), googlenet's input at batch 256.  Every row has
one seeded 672 x 672 rectangle (scale 3) or, for the translation, a 224 x 224 one.  One process times, the kinds alternating over
`--rounds` rounds, each as `--steps` launches between two device events after `--warmup` untimed ones:

  warp_translate   pvhip_input_preprocess_warp_f32, integer translations (a copy: one tap per pixel)
  warp_scale3      ... warp.from_roi of the 672 x 672 rectangles (upright, four taps per pixel)
  warp_rot30       ... the same rectangles turned by 30 degrees about their centres (warp.rotated_rect)
  roi_translate    pvhip_input_preprocess_roi_f32 / _yuv_roi_f32 on the 224 x 224 rectangles (its copy path)
  roi_scale3       ... on the 672 x 672 rectangles: the launch that was there before, the yardstick

The effective rate of a kind is (the bytes of its rectangles in the frames' format + the bytes of the tensor written) over its time:
one numerator for a warp and the ROI launch of the same rectangles, whatever each really fetches (a warp at scale 3 taps four of every
nine pixels of its rectangle; the ROI launch stages all of them).

Prints one JSON line.  --out FILE.md writes the table in markdown.  --compare LIB (with --compare-label): the same measurement in a
fresh child process with that build of the library (PVHIP_LIBRARY), run after this one in each of --repeat repetitions, for the tile
shape the library was not built with.  --kernel KIND: only that kind's launches, the run to take under rocprofv3.
Run each GPU step under its own time limit, e.g.  timeout -k 10 300 python scripts/bench_warp_input.py --out profiles/warp_input.md
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pyopenvino_amd import WarpInput, device, warp  # noqa: E402
from bench_preprocess_yuv import frames, git_head, timed  # noqa: E402

N, M, FRAME, DST, SIDE = 256, 8, (1080, 1920), (224, 224), 672
TILE = '32 x 32 (8 quads x 32 rows; kWarpTileW of pvhip_preprocess.hip)'
FORMATS = {'u8': (0, 3, 3.0), 'nv12': (1, 0, 1.5)}           # format: (format, how) of the warp entry, bytes per pixel
CASES = ('translate', 'scale3', 'rot30')


def ptr(t):
    return ctypes.c_void_p(t.ptr)


def rectangles(rng, side):
    """(N, 5) int32 (id, x, y, side, side): row b in frame b % M, anywhere the rectangle -- and its turn by 30 degrees -- stays inside."""
    reach = int(np.ceil(side * (np.cos(np.pi / 6) + np.sin(np.pi / 6)) / 2)) + 1       # half the bounding box of the turned square
    cx, cy = rng.integers(reach, FRAME[1] - reach + 1, N), rng.integers(reach, FRAME[0] - reach + 1, N)
    return np.stack([np.arange(N) % M, cx - side // 2, cy - side // 2, np.full(N, side), np.full(N, side)], 1).astype(np.int32)


def tables(rng):
    """{case: (the (N, 7) int64 warp table, the (N, 5) int32 table of the equivalent upright rectangles)}."""
    small, large = rectangles(rng, DST[0]), rectangles(rng, SIDE)
    matrices = {
        'translate': np.stack([warp.from_roi(r[1:], DST) for r in small]),
        'scale3': np.stack([warp.from_roi(r[1:], DST) for r in large]),
        'rot30': np.stack([warp.rotated_rect(r[1] + SIDE / 2, r[2] + SIDE / 2, SIDE, SIDE, 30.0, DST) for r in large]),
    }
    assert (WarpInput.fixed(matrices['translate']) & 0xFFFF == 0).all()
    rois = {'translate': small, 'scale3': large, 'rot30': large}
    return {case: (np.concatenate([rois[case][:, :1].astype(np.int64), WarpInput.fixed(matrices[case])], 1), rois[case]) for case in CASES}


def measure(args):
    device.init(0)
    rng = np.random.default_rng(2026)
    (hs, ws), (hd, wd) = FRAME, DST
    dst = device.DeviceTensor.empty((N, 3, hd, wd))
    d = ptr(dst)
    host = tables(rng)
    dev = {case: (device.DeviceTensor.from_numpy(w), device.DeviceTensor.from_numpy(r)) for case, (w, r) in host.items()}
    out = {}
    for fmt, (form, how, bpp) in FORMATS.items():
        src = device.DeviceTensor.from_numpy(frames(rng, M, hs, ws, 'bgr' if fmt == 'u8' else 'nv12'))
        s = ptr(src)
        launch = {}
        for case in CASES:
            wt, rt = dev[case]
            side = int(host[case][1][0, 3])
            launch['warp_{}_{}'.format(fmt, case)] = (lambda wt=wt: device.call(
                'pvhip_input_preprocess_warp_f32', s, d, ptr(wt), N, M, 3, hs, ws, hd, wd, form, how, 0, None, None, 0.0))
            if case == 'rot30':
                continue
            if fmt == 'u8':
                launch['roi_{}_{}'.format(fmt, case)] = (lambda rt=rt, side=side: device.call(
                    'pvhip_input_preprocess_roi_f32', s, d, ptr(rt), N, M, 3, hs, ws, hd, wd, side, side, 1, 1, 0, None, None))
            else:
                launch['roi_{}_{}'.format(fmt, case)] = (lambda rt=rt, side=side: device.call(
                    'pvhip_input_preprocess_yuv_roi_f32', s, d, ptr(rt), N, M, hs, ws, hd, wd, side, side, 0, 0, None, None))
        if args.kernel:
            launch = {k: v for k, v in launch.items() if k == args.kernel}
        us = {kind: [] for kind in launch}
        for _ in range(args.rounds):
            for kind in launch:
                us[kind].append(timed(launch[kind], args.steps, args.warmup))
        for kind, rounds in us.items():
            side = int(host[kind.split('_')[2]][1][0, 3])
            nbytes = int(N * side * side * bpp) + dst.nbytes
            t = float(np.median(rounds))
            out[kind] = {'launch_us': t, 'launch_us_per_round': rounds, 'bytes': nbytes, 'effective_GBs': nbytes / (t * 1e-6) / 1e9}
        del src
    return out


def markdown(line):
    rows = ['# WarpInput: the warp launch beside the ROI launch', '',
            '`python scripts/bench_warp_input.py` on {} ({}, {}): {} frames of {} x {}, {} rows -> (256, 3, 224, 224) fp32; medians of {} rounds '
            'of {} launches between device events, the kinds alternating.  Effective GB/s: the bytes of the rectangles in the '
            'frames\' format plus the tensor written, over the time -- one numerator for a warp and the ROI launch of the same '
            'rectangles.'.format(line['device'], line['date'], line['git_head'], M, FRAME[0], FRAME[1], N, line['rounds'], line['launches_per_round']),
            '', 'Tile of the warp kernel: {}.'.format(TILE), '']
    for label, runs in line['runs'].items():
        for i, run in enumerate(runs):
            rows += ['## {} (repetition {})'.format(label, i + 1), '', '| kind | us per launch | min .. max over rounds | effective GB/s | warp / roi |',
                     '|---|---|---|---|---|']
            for kind, v in run.items():
                yard = run.get(kind.replace('warp_', 'roi_').replace('rot30', 'scale3'))
                ratio = '{:.2f}'.format(v['launch_us'] / yard['launch_us']) if kind.startswith('warp_') and yard else ''
                rows.append('| {} | {:.1f} | {:.1f} .. {:.1f} | {:.0f} | {} |'.format(
                    kind, v['launch_us'], min(v['launch_us_per_round']), max(v['launch_us_per_round']), v['effective_GBs'], ratio))
            rows.append('')
    return '\n'.join(rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=100, help='timed launches per kind and round')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5, help='rounds over the kinds (alternating, one process)')
    ap.add_argument('--kernel', default=None, help='only the launches of this kind, e.g. warp_u8_scale3 (see above)')
    ap.add_argument('--compare', default=None, help='another build of libpvhip.so to measure in a child process (see above)')
    ap.add_argument('--compare-label', default='other build')
    ap.add_argument('--repeat', type=int, default=1, help='repetitions of (this build, the --compare build)')
    ap.add_argument('--out', default=None, help='write the markdown table to this file')
    ap.add_argument('--head', default=None, help='git commit to report (default: git rev-parse HEAD, when the tree is a checkout)')
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args)))
        return
    runs = {'this build': []}
    if args.compare:
        runs[args.compare_label] = []
    for _ in range(args.repeat):
        # every measurement in a fresh child process: this one never binds the device, and the builds alternate
        for label in runs:
            env = dict(os.environ)
            if label != 'this build':
                env['PVHIP_LIBRARY'] = os.path.abspath(args.compare)
            cmd = [sys.executable, os.path.abspath(__file__), '--child', '--steps', str(args.steps), '--warmup', str(args.warmup), '--rounds', str(args.rounds)]
            if args.kernel:
                cmd += ['--kernel', args.kernel]
            done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280)
            if done.returncode != 0:
                sys.exit('{} failed ({}):\n{}'.format(label, done.returncode, done.stderr[-2000:]))
            runs[label].append(json.loads(done.stdout.strip().splitlines()[-1]))
    line = {'metric': 'affine warps -> (256, 3, 224, 224) fp32 beside the ROI launch on the upright rectangles, event-timed', 'runs': runs,
            'tile': TILE, 'launches_per_round': args.steps, 'rounds': args.rounds, 'git_head': git_head(args.head),
            'device': subprocess.run([sys.executable, '-c', 'import sys; sys.path.insert(0, {!r}); from pyopenvino_amd import device; device.init(0); '
                                      'print(device.device_name())'.format(REPO)], capture_output=True, text=True, timeout=120).stdout.strip(),
            'date': time.strftime('%Y-%m-%d'), 'profiled_with_rocprofv3': False}
    print(json.dumps(line))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(markdown(line) + '\n')


if __name__ == '__main__':
    main()
