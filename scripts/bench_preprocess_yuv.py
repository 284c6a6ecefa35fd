"""YUV 4:2:0 frames converted on the device against B, G, R frames of the same extent: the launch and the upload of one request.

For each case -- batch 256, (480, 640) -> 224 x 224 (GoogLeNet) and batch 128, (480, 640) -> 300 x 300 (SSD) -- one process times, the
kinds alternating over `--rounds` rounds:

  bgr    pvhip_input_preprocess_f32 on uint8 NHWC (n, 480, 640, 3) frames: the yardstick, 3 bytes per pixel
  nv12   pvhip_input_preprocess_yuv_f32 on (n, 720, 640) frames, interleaved chroma: 1.5 bytes per pixel
  i420   the same entry, planar chroma

each as `--steps` launches between two device events after `--warmup` untimed ones, and the page-locked H2D copy of each source on the
copy stream the same way.  The frames are forward-converted random images (yuv_ref.planes_from_bgr's rule, restated here), so the
conversion mostly does not saturate.  Prints one JSON line (median and per-round microseconds per launch and per copy, bytes moved, TB/s
of the launch, GB/s of the copy, upload + launch per request); --out writes it too.

--standard BT709|BT2020 / --range FULL: the nv12 and i420 launches go through pvhip_input_preprocess_yuv_color_f32 with that rule (the
frames stay the same bytes: the launch reads and writes as much, only its six constants differ); the defaults, BT601 / LIMITED, time the
existing entry as every default-format pass calls it.

--kernel nv12|i420|bgr: only that kind's launches of the first case, the run to take under  rocprofv3 --kernel-trace --stats.
Run each GPU step under its own time limit, e.g.  timeout -k 10 300 python scripts/bench_preprocess_yuv.py --out profiles/preprocess_yuv.json
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

from pyopenvino_amd import device  # noqa: E402

CASES = [(256, (480, 640), (224, 224)), (128, (480, 640), (300, 300))]
KINDS = ('bgr', 'nv12', 'i420')
STANDARDS = ('BT601', 'BT709', 'BT2020')
RANGES = ('LIMITED', 'FULL')


def frames(rng, n, h, w, kind):
    """uint8 frames: (n, h, w, 3) of random images, or their BT.601 limited-range YUV 4:2:0 encoding
    (n, 3 h / 2, w) with the chroma of a 2 x 2 block the mean of its pixels."""
    bgr = np.tile(rng.integers(0, 256, (16, h, w, 3), dtype=np.uint8), ((n + 15) // 16, 1, 1, 1))[:n]     # (16 different images, repeated)
    if kind == 'bgr':
        return bgr
    b, g, r = (bgr[..., k].astype(np.float32) for k in range(3))
    sub = lambda c: c.reshape(n, h // 2, 2, w // 2, 2).mean((2, 4))  # noqa: E731
    q = lambda c: np.clip(np.rint(c), 0, 255).astype(np.uint8)  # noqa: E731
    y = q(16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255)
    u = q(sub(128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255))
    v = q(sub(128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255))
    chroma = np.stack([u, v], -1 if kind == 'nv12' else 1)
    return np.concatenate([y.reshape(n, -1), chroma.reshape(n, -1)], 1).reshape(n, 3 * h // 2, w)


def timed(launch, steps, warmup, stream=0):
    """Microseconds per call of `launch` on `stream`: device events around `steps` calls after `warmup` untimed ones."""
    device.select_stream(stream)
    for _ in range(warmup):
        launch()
    e0, e1 = device.Event(), device.Event()
    e0.record()
    for _ in range(steps):
        launch()
    e1.record()
    e1.synchronize()
    device.select_stream(0)
    return e0.elapsed_ms(e1) * 1e3 / steps


def git_head(head):
    if head is None:
        try:
            head = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=REPO, capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    return head


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=200, help='timed launches per kind and round (copies: a tenth of it)')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5, help='rounds over the kinds (alternating, one process)')
    ap.add_argument('--kernel', choices=KINDS, default=None, help='only the launches of this kind, first case (see above)')
    ap.add_argument('--standard', choices=STANDARDS, default='BT601', help='the matrix of the YUV launches (see above)')
    ap.add_argument('--range', choices=RANGES, default='LIMITED', help='the range of the YUV launches')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--head', default=None, help='git commit to report (default: git rev-parse HEAD, when the tree is a checkout)')
    args = ap.parse_args()
    device.init(0)
    rng = np.random.default_rng(2026)
    rule = (STANDARDS.index(args.standard), RANGES.index(args.range))
    cases = {}
    for n, (hs, ws), (hd, wd) in CASES[:1] if args.kernel else CASES:
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
            elif rule == (0, 0):
                launch[kind] = lambda s=s, d=d, p=int(kind == 'i420'): device.call('pvhip_input_preprocess_yuv_f32', s, d, n, hs, ws, hd, wd,
                                                                                     p, 0, None, None)
            else:
                launch[kind] = lambda s=s, d=d, p=int(kind == 'i420'): device.call('pvhip_input_preprocess_yuv_color_f32', s, d, None, n, n,
                                                                                     hs, ws, hd, wd, hs, ws, p, 0, None, None, 0, 0.0, *rule)
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
            rows[kind] = {'launch_us': t, 'launch_us_per_round': us[kind]['launch'], 'bytes_in': src[kind].nbytes, 'bytes_out': dst.nbytes,
                          'launch_TBs': nbytes / (t * 1e-6) / 1e12}
            if not args.kernel:
                c = float(np.median(us[kind]['copy']))
                rows[kind].update(copy_us=c, copy_us_per_round=us[kind]['copy'], copy_GBs=src[kind].nbytes / (c * 1e-6) / 1e9,
                                  copy_plus_launch_us=c + t)
        if not args.kernel:
            for kind in ('nv12', 'i420'):
                rows[kind]['launch_vs_bgr'] = rows[kind]['launch_us'] / rows['bgr']['launch_us']
                rows[kind]['copy_vs_bgr'] = rows[kind]['copy_us'] / rows['bgr']['copy_us']
        cases['{}x{}x{}->{}x{}'.format(n, hs, ws, hd, wd)] = rows
        del src, host, dst
    line = {'metric': 'one request\'s input: uint8 frames -> (n, 3, h, w) fp32, launch and page-locked upload, event-timed', 'cases': cases,
            'standard': args.standard, 'range': args.range, 'library': os.path.basename(device.LIB_PATH),
            'launches_per_round': args.steps, 'rounds': args.rounds, 'git_head': git_head(args.head), 'device': device.device_name(),
            'date': time.strftime('%Y-%m-%d')}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
