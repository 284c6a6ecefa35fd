"""Packed frames (YUY2, UYVY, BGRX, RGBX) converted on the device against B, G, R and NV12 frames of the same extent: the launch and the
upload of one request.

For each case -- batch 256, (480, 640) -> 224 x 224 (GoogLeNet) and batch 128, (480, 640) -> 300 x 300 (SSD) -- one process times, the
kinds alternating over `--rounds` rounds:

  bgr    pvhip_input_preprocess_f32 on uint8 NHWC (n, 480, 640, 3) frames: the yardstick, 3 bytes per pixel
  nv12   pvhip_input_preprocess_yuv_f32 on (n, 720, 640) frames: 1.5 bytes per pixel
  yuy2   pvhip_input_preprocess_packed_f32 on (n, 480, 640, 2) frames, kind 0: 2 bytes per pixel
  uyvy   the same entry, kind 1
  bgrx   the same entry on (n, 480, 640, 4) frames, kind 2: 4 bytes per pixel
  rgbx   the same entry, kind 3

each as `--steps` launches between two device events after `--warmup` untimed ones, and the page-locked H2D copy of each source on the
copy stream the same way.  The 4:2:2 frames are forward-converted random images (the chroma of a column pair the mean of its two pixels),
so the conversion mostly does not saturate.  Prints one JSON line (median and per-round microseconds per launch and per copy, bytes
moved, TB/s of the launch, GB/s of the copy, upload + launch per request, and each kind against `bgr` of the same run with the run's own
spread over rounds); --out writes it too.

No time is fixed in advance; the yardstick is the `bgr` launch in the same run.  `conditions` reports, per case, whether each 4:2:2 kind
is no slower than `bgr` and each X kind no slower than 1.20 x `bgr` (the ratio of the bytes an X launch moves at 224 x 224), each with a
margin of the run's spread: (max - min) / median over rounds of the two launches compared, added.

--kernel KIND: only that kind's launches of the first case, the run to take under  rocprofv3 --kernel-trace --stats.
--case K: only case K (0 or 1), so that each case can run as a step of its own.
Run each GPU step under its own time limit, e.g.  timeout -k 10 300 python scripts/bench_preprocess_packed.py --out profiles/preprocess_packed.json
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pyopenvino_amd import device  # noqa: E402
from bench_preprocess_yuv import frames as yuv_frames, git_head, timed  # noqa: E402

CASES = [(256, (480, 640), (224, 224)), (128, (480, 640), (300, 300))]
PACKED = {'yuy2': 0, 'uyvy': 1, 'bgrx': 2, 'rgbx': 3}
KINDS = ('bgr', 'nv12') + tuple(PACKED)
LIMIT = {'yuy2': 1.0, 'uyvy': 1.0, 'bgrx': 1.2, 'rgbx': 1.2}   # against the bgr launch of the same run


def frames(rng, n, h, w, kind):
    """uint8 frames of `kind` made from 16 random images, repeated."""
    if kind in ('bgr', 'nv12'):
        return yuv_frames(rng, n, h, w, kind)
    bgr = yuv_frames(rng, n, h, w, 'bgr')
    if kind in ('bgrx', 'rgbx'):
        out = np.empty((n, h, w, 4), np.uint8)
        out[..., 0:3] = bgr if kind == 'bgrx' else bgr[..., ::-1]
        out[..., 3] = 255
        return out
    b, g, r = (bgr[..., k].astype(np.float32) for k in range(3))
    sub = lambda c: c.reshape(n, h, w // 2, 2).mean(3)  # noqa: E731
    q = lambda c: np.clip(np.rint(c), 0, 255).astype(np.uint8)  # noqa: E731
    y = q(16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255)
    u = q(sub(128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255))
    v = q(sub(128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255))
    group = (y[..., 0::2], u, y[..., 1::2], v) if kind == 'yuy2' else (u, y[..., 0::2], v, y[..., 1::2])
    return np.stack(group, -1).reshape(n, h, w, 2)


def spread(per_round):
    return (max(per_round) - min(per_round)) / float(np.median(per_round))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=200, help='timed launches per kind and round (copies: a tenth of it)')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5, help='rounds over the kinds (alternating, one process)')
    ap.add_argument('--kernel', choices=KINDS, default=None, help='only the launches of this kind, first case (see above)')
    ap.add_argument('--case', type=int, choices=(0, 1), default=None, help='only this case')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--head', default=None, help='git commit to report (default: git rev-parse HEAD, when the tree is a checkout)')
    args = ap.parse_args()
    device.init(0)
    rng = np.random.default_rng(2026)
    cases, conditions = {}, {}
    chosen = CASES[:1] if args.kernel else (CASES if args.case is None else CASES[args.case:args.case + 1])
    for n, (hs, ws), (hd, wd) in chosen:
        dst = device.DeviceTensor.empty((n, 3, hd, wd))
        host, src, launch, copy = {}, {}, {}, {}
        for kind in [args.kernel] if args.kernel else KINDS:
            x = frames(rng, n, hs, ws, kind)
            host[kind] = device.host_empty(x.shape, np.uint8)
            host[kind][...] = x
            src[kind] = device.DeviceTensor.from_numpy(x)
            s, d = ctypes.c_void_p(src[kind].ptr), ctypes.c_void_p(dst.ptr)
            if kind == 'bgr':
                launch[kind] = lambda s=s, d=d: device.call('pvhip_input_preprocess_f32', s, d, n, 3, hs, ws, hd, wd, 1, 1, 0, None, None)
            elif kind == 'nv12':
                launch[kind] = lambda s=s, d=d: device.call('pvhip_input_preprocess_yuv_f32', s, d, n, hs, ws, hd, wd, 0, 0, None, None)
            else:
                launch[kind] = lambda s=s, d=d, k=PACKED[kind]: device.call('pvhip_input_preprocess_packed_f32', s, d, n, hs, ws, hd, wd,
                                                                            k, 0, None, None)
            copy[kind] = lambda s=s, h=host[kind]: device.call('pvhip_memcpy_h2d_async', s, ctypes.c_void_p(h.ctypes.data), h.nbytes)
        us = {kind: {'launch': [], 'copy': []} for kind in launch}
        for _ in range(args.rounds):
            for kind in launch:
                us[kind]['launch'].append(timed(launch[kind], args.steps, args.warmup))
            if not args.kernel:
                for kind in launch:
                    us[kind]['copy'].append(timed(copy[kind], max(1, args.steps // 10), 1, device.COPY_STREAM))
        rows = {}
        for kind in launch:
            t = float(np.median(us[kind]['launch']))
            nbytes = src[kind].nbytes + dst.nbytes
            rows[kind] = {'launch_us': t, 'launch_us_per_round': us[kind]['launch'], 'launch_spread': spread(us[kind]['launch']),
                          'bytes_in': src[kind].nbytes, 'bytes_out': dst.nbytes, 'launch_TBs': nbytes / (t * 1e-6) / 1e12}
            if not args.kernel:
                c = float(np.median(us[kind]['copy']))
                rows[kind].update(copy_us=c, copy_us_per_round=us[kind]['copy'], copy_GBs=src[kind].nbytes / (c * 1e-6) / 1e9,
                                  copy_plus_launch_us=c + t)
        name = '{}x{}x{}->{}x{}'.format(n, hs, ws, hd, wd)
        if not args.kernel:
            bgr = rows['bgr']
            conditions[name] = {}
            for kind in KINDS[1:]:
                row = rows[kind]
                row['launch_vs_bgr'] = row['launch_us'] / bgr['launch_us']
                row['bytes_vs_bgr'] = (row['bytes_in'] + row['bytes_out']) / (bgr['bytes_in'] + bgr['bytes_out'])
                row['copy_vs_bgr'] = row['copy_us'] / bgr['copy_us']
                if kind in LIMIT:
                    margin = row['launch_spread'] + bgr['launch_spread']
                    conditions[name][kind] = {'limit': LIMIT[kind], 'margin': margin, 'launch_vs_bgr': row['launch_vs_bgr'],
                                              'holds': bool(row['launch_vs_bgr'] <= LIMIT[kind] + margin)}
        cases[name] = rows
        del src, host, dst
    line = {'metric': 'one request\'s input: uint8 frames -> (n, 3, h, w) fp32, launch and page-locked upload, event-timed', 'cases': cases,
            'conditions': conditions, 'launches_per_round': args.steps, 'rounds': args.rounds, 'git_head': git_head(args.head),
            'device': device.device_name(), 'date': time.strftime('%Y-%m-%d')}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
