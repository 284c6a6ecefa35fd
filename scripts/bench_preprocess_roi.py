"""Regions of interest cropped and resized on the device: what the ROI form of the preprocessing launch costs, and what it buys a cascade.

One process times, the kinds alternating over `--rounds` rounds, each as `--steps` launches between two device events after `--warmup`
untimed ones (and page-locked H2D copies on the copy stream the same way):

  cost   (256, 480, 640) -> 224 x 224, uint8 NHWC and NV12: pvhip_input_preprocess_roi_f32 / _yuv_roi_f32 with the whole-frame table
         rois[b] = (b, 0, 0, 640, 480) against pvhip_input_preprocess_f32 / _yuv_f32 on the same frames.  The ROI form adds one 20-byte
         read and a few scalar operations per workgroup, nothing per pixel: `roi_vs_plain` is the ratio of the medians.
  buys   one (1080, 1920) NV12 frame and 256 rectangles with sides of 32..400 pixels (seeded) -> 224 x 224 through
         pvhip_input_preprocess_yuv_roi_f32 -- the launch, the bytes it moves (the rectangles' Y and chroma bytes in, the tensor out), the
         upload of the frame and the table --, beside the cascade's best without it: 256 host-made 224 x 224 uint8 NHWC crops, uploaded
         and converted by pvhip_input_to_nchw_f32.  (The host's cropping and resizing of those 256 images is not timed: it only adds.)

Prints one JSON line; --out writes it too.  --kernel roi_nv12|roi_u8|crops: only that kind's launches, the run to take under
rocprofv3 --kernel-trace --stats.
Run each GPU step under its own time limit, e.g.  timeout -k 10 300 python scripts/bench_preprocess_roi.py --out profiles/preprocess_roi.json
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
from bench_preprocess_yuv import frames, git_head, timed  # noqa: E402

N, SRC, DST = 256, (480, 640), (224, 224)
FRAME = (1080, 1920)


def ptr(t):
    return ctypes.c_void_p(t.ptr)


def whole_frames(n, hw):
    return np.array([[b, 0, 0, hw[1], hw[0]] for b in range(n)], np.int32)


def boxes(rng, n, hw):
    """n rectangles (0, x, y, w, h) with sides of 32..400 pixels anywhere in one frame of extent hw."""
    w, h = rng.integers(32, 401, n), rng.integers(32, 401, n)
    return np.stack([np.zeros(n, np.int64), rng.integers(0, hw[1] - w + 1), rng.integers(0, hw[0] - h + 1), w, h], 1).astype(np.int32)


def median_rounds(launch, rounds, steps, warmup, stream=0):
    """{kind: [us per call, one per round]}, the kinds alternating within every round."""
    us = {kind: [] for kind in launch}
    for _ in range(rounds):
        for kind in launch:
            us[kind].append(timed(launch[kind], steps, warmup, stream))
    return us


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=200, help='timed launches per kind and round (copies: a tenth of it)')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5, help='rounds over the kinds (alternating, one process)')
    ap.add_argument('--kernel', choices=('roi_nv12', 'roi_u8', 'crops'), default=None, help='only the launches of this kind (see above)')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--head', default=None, help='git commit to report (default: git rev-parse HEAD, when the tree is a checkout)')
    args = ap.parse_args()
    device.init(0)
    rng = np.random.default_rng(2026)
    (hs, ws), (hd, wd) = SRC, DST
    dst = device.DeviceTensor.empty((N, 3, hd, wd))
    d = ptr(dst)

    # ---- what the ROI form costs: whole-frame tables against the entries without a table
    table = device.DeviceTensor.from_numpy(whole_frames(N, SRC))
    src = {kind: device.DeviceTensor.from_numpy(frames(rng, N, hs, ws, kind)) for kind in ('bgr', 'nv12')}
    u8, nv = ptr(src['bgr']), ptr(src['nv12'])
    launch = {
        'u8': lambda: device.call('pvhip_input_preprocess_f32', u8, d, N, 3, hs, ws, hd, wd, 1, 1, 0, None, None),
        'roi_u8': lambda: device.call('pvhip_input_preprocess_roi_f32', u8, d, ptr(table), N, N, 3, hs, ws, hd, wd, hs, ws, 1, 1, 0, None, None),
        'nv12': lambda: device.call('pvhip_input_preprocess_yuv_f32', nv, d, N, hs, ws, hd, wd, 0, 0, None, None),
        'roi_nv12': lambda: device.call('pvhip_input_preprocess_yuv_roi_f32', nv, d, ptr(table), N, N, hs, ws, hd, wd, hs, ws, 0, 0, None, None),
    }
    cost = {}
    if args.kernel in (None, 'roi_nv12', 'roi_u8'):
        only = {k: v for k, v in launch.items() if args.kernel in (None, k)}
        us = median_rounds(only, args.rounds, args.steps, args.warmup)
        for kind, rounds in us.items():
            t = float(np.median(rounds))
            nbytes = src['bgr' if kind.endswith('u8') else 'nv12'].nbytes + dst.nbytes
            cost[kind] = {'launch_us': t, 'launch_us_per_round': rounds, 'launch_TBs': nbytes / (t * 1e-6) / 1e12}
        for kind in ('u8', 'nv12'):
            if 'roi_' + kind in cost and kind in cost:
                cost['roi_' + kind]['roi_vs_plain'] = cost['roi_' + kind]['launch_us'] / cost[kind]['launch_us']
                cost['roi_' + kind]['roi_vs_plain_per_round'] = [a / b for a, b in zip(us['roi_' + kind], us[kind])]
    del src, table

    # ---- what it buys: one 1080p NV12 frame and 256 rectangles against 256 host-made crops
    buys = {}
    if args.kernel in (None, 'crops'):
        fh, fw = FRAME
        rois = boxes(rng, N, FRAME)
        frame_host = device.host_empty((1, 3 * fh // 2, fw), np.uint8)
        frame_host[...] = frames(rng, 1, fh, fw, 'nv12')
        rois_host = device.host_empty(rois.shape, np.int32)
        rois_host[...] = rois
        crops_host = device.host_empty((N, hd, wd, 3), np.uint8)
        crops_host[...] = rng.integers(0, 256, crops_host.shape, dtype=np.uint8)
        frame, table, crops = (device.DeviceTensor.from_numpy(a) for a in (frame_host, rois_host, crops_host))
        largest = (int(rois[:, 4].max()), int(rois[:, 3].max()))

        def upload_frame():
            device.call('pvhip_memcpy_h2d_async', ptr(frame), ctypes.c_void_p(frame_host.ctypes.data), frame_host.nbytes)
            device.call('pvhip_memcpy_h2d_async', ptr(table), ctypes.c_void_p(rois_host.ctypes.data), rois_host.nbytes)

        launch = {
            'roi_nv12_1080p': lambda: device.call('pvhip_input_preprocess_yuv_roi_f32', ptr(frame), d, ptr(table), N, 1, fh, fw, hd, wd, *largest,
                                                  0, 0, None, None),
            'host_crops_u8': lambda: device.call('pvhip_input_to_nchw_f32', ptr(crops), d, N, 3, hd, wd, 1, 1),
        }
        copy = {'roi_nv12_1080p': upload_frame,
                'host_crops_u8': lambda: device.call('pvhip_memcpy_h2d_async', ptr(crops), ctypes.c_void_p(crops_host.ctypes.data), crops_host.nbytes)}
        us = median_rounds(launch, args.rounds, args.steps, args.warmup)
        us_copy = {} if args.kernel else median_rounds(copy, args.rounds, max(1, args.steps // 10), 1, device.COPY_STREAM)
        # bytes the ROI launch has to read at least: every rectangle's Y bytes and the chroma under them
        read = int(sum(int(w) * int(h) + 2 * ((x + w - 1) // 2 - x // 2 + 1) * ((y + h - 1) // 2 - y // 2 + 1) for _, x, y, w, h in rois.tolist()))
        moved = {'roi_nv12_1080p': read + dst.nbytes, 'host_crops_u8': crops.nbytes + dst.nbytes}
        uploaded = {'roi_nv12_1080p': frame_host.nbytes + rois_host.nbytes, 'host_crops_u8': crops_host.nbytes}
        for kind in launch:
            t = float(np.median(us[kind]))
            buys[kind] = {'launch_us': t, 'launch_us_per_round': us[kind], 'bytes_moved': moved[kind], 'launch_TBs': moved[kind] / (t * 1e-6) / 1e12,
                          'bytes_uploaded': uploaded[kind]}
            if kind in us_copy:
                c = float(np.median(us_copy[kind]))
                buys[kind].update(copy_us=c, copy_us_per_round=us_copy[kind], copy_GBs=uploaded[kind] / (c * 1e-6) / 1e9, copy_plus_launch_us=c + t)
        if us_copy:
            buys['upload_plus_launch_roi_vs_host_crops'] = buys['roi_nv12_1080p']['copy_plus_launch_us'] / buys['host_crops_u8']['copy_plus_launch_us']
        buys['largest_rectangle_hw'] = list(largest)

    line = {'metric': 'regions of interest -> (256, 3, 224, 224) fp32: launch and page-locked upload, event-timed',
            'cost_256x480x640->224x224_whole_frame_tables': cost, 'buys_1x1080x1920_nv12_256_rectangles->224x224': buys,
            'launches_per_round': args.steps, 'rounds': args.rounds, 'git_head': git_head(args.head), 'device': device.device_name(),
            'date': time.strftime('%Y-%m-%d'), 'profiled_with_rocprofv3': False}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
