"""One request's input with an aspect-preserving fit (preprocess_info.resize_fit = 'LETTERBOX') against the stretch of the same source, kinds
alternating over `--rounds` rounds of ONE process, the launch event-timed:

  u8       pvhip_input_preprocess_f32 on uint8 NHWC (n, 1080, 1920, 3) frames -> (n, 3, 300, 300): the stretch, the yardstick
  u8_fit   pvhip_input_preprocess_fit_f32 on the same frames, fit 1, pad 114: 169 of the 300 rows are interpolated, 131 are padding
  nv12     pvhip_input_preprocess_yuv_f32 on (n, 1620, 1920) NV12 frames -> (n, 3, 300, 300)
  nv12_fit pvhip_input_preprocess_yuv_fit_f32 on the same frames
and, with --rois, the fitted ROI forms on one (1080, 1920) frame and n = 256 rectangles with sides of 32..400 pixels -> 224 x 224, the
launch sized for the whole frame as a DetectedRois launch is:
  roi_u8 / roi_u8_fit, roi_nv12 / roi_nv12_fit   pvhip_input_preprocess_roi_f32 / _fit_f32 and the _yuv_ forms on the same table

A fitted launch reads the same source bytes as its stretch would for the rows it interpolates and fewer of them (the padding reads
nothing), so the expectation is "not slower"; the line states both times and their ratio either way.
Prints one JSON line; --out writes it too.  --kernel KIND: only that kind's launches, the run to take under  rocprofv3 --kernel-trace --stats.
Run each GPU step under its own time limit, e.g.  timeout -k 10 300 python scripts/bench_preprocess_letterbox.py --out profiles/letterbox.json
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
from pyopenvino_amd.input_format import fit_geometry  # noqa: E402

SRC, DST, ROI_DST = (1080, 1920), (300, 300), (224, 224)
KINDS = ('u8', 'u8_fit', 'nv12', 'nv12_fit')
ROI_KINDS = ('roi_u8', 'roi_u8_fit', 'roi_nv12', 'roi_nv12_fit')
PAD = 114.0


def timed(launch, steps, warmup):
    """Microseconds per call of `launch`: device events around `steps` calls after `warmup` untimed ones."""
    for _ in range(warmup):
        launch()
    e0, e1 = device.Event(), device.Event()
    e0.record()
    for _ in range(steps):
        launch()
    e1.record()
    e1.synchronize()
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
    ap.add_argument('--steps', type=int, default=200, help='timed launches per kind and round')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5, help='rounds over the kinds (alternating, one process)')
    ap.add_argument('--batch', type=int, default=16, help='1080p frames per launch')
    ap.add_argument('--rois', action='store_true', help='the ROI forms as well')
    ap.add_argument('--kernel', choices=KINDS + ROI_KINDS, default=None, help='only the launches of this kind (see above)')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--head', default=None, help='git commit to report (default: git rev-parse HEAD, when the tree is a checkout)')
    args = ap.parse_args()
    device.init(0)
    rng = np.random.default_rng(2026)
    n, (hs, ws), (hd, wd) = args.batch, SRC, DST
    ptr = lambda t: ctypes.c_void_p(t.ptr)  # noqa: E731
    u8 = device.DeviceTensor.from_numpy(rng.integers(0, 256, (n, hs, ws, 3), dtype=np.uint8))
    nv = device.DeviceTensor.from_numpy(rng.integers(0, 256, (n, hs * 3 // 2, ws), dtype=np.uint8))      # (any bytes are a frame)
    dst = device.DeviceTensor.empty((n, 3, hd, wd))
    launch = {
        'u8': lambda: device.call('pvhip_input_preprocess_f32', ptr(u8), ptr(dst), n, 3, hs, ws, hd, wd, 1, 1, 0, None, None),
        'u8_fit': lambda: device.call('pvhip_input_preprocess_fit_f32', ptr(u8), ptr(dst), None, n, n, 3, hs, ws, hd, wd, hs, ws, 1, 1, 0, None, None,
                                      1, PAD),
        'nv12': lambda: device.call('pvhip_input_preprocess_yuv_f32', ptr(nv), ptr(dst), n, hs, ws, hd, wd, 0, 0, None, None),
        'nv12_fit': lambda: device.call('pvhip_input_preprocess_yuv_fit_f32', ptr(nv), ptr(dst), None, n, n, hs, ws, hd, wd, hs, ws, 0, 0, None, None,
                                        1, PAD),
    }
    nbytes = {'u8': u8.nbytes + dst.nbytes, 'u8_fit': u8.nbytes + dst.nbytes, 'nv12': nv.nbytes + dst.nbytes, 'nv12_fit': nv.nbytes + dst.nbytes}
    if args.rois or args.kernel in ROI_KINDS:
        N, (rh, rw) = 256, ROI_DST
        w, h = rng.integers(32, 401, N), rng.integers(32, 401, N)
        table = np.stack([np.zeros(N, np.int64), rng.integers(0, ws - w + 1), rng.integers(0, hs - h + 1), w, h], 1).astype(np.int32)
        rois = device.DeviceTensor.from_numpy(table)
        rdst = device.DeviceTensor.empty((N, 3, rh, rw))
        one = (N, 1, 3, hs, ws, rh, rw, hs, ws, 1, 1, 0, None, None)
        one_yuv = (N, 1, hs, ws, rh, rw, hs, ws, 0, 0, None, None)
        launch.update({
            'roi_u8': lambda: device.call('pvhip_input_preprocess_roi_f32', ptr(u8), ptr(rdst), ptr(rois), *one),
            'roi_u8_fit': lambda: device.call('pvhip_input_preprocess_fit_f32', ptr(u8), ptr(rdst), ptr(rois), *one, 1, PAD),
            'roi_nv12': lambda: device.call('pvhip_input_preprocess_yuv_roi_f32', ptr(nv), ptr(rdst), ptr(rois), *one_yuv),
            'roi_nv12_fit': lambda: device.call('pvhip_input_preprocess_yuv_fit_f32', ptr(nv), ptr(rdst), ptr(rois), *one_yuv, 1, PAD),
        })
        nbytes.update({k: int((w * h).sum()) * (3 if 'u8' in k else 1.5) + rdst.nbytes for k in ROI_KINDS})
    kinds = [args.kernel] if args.kernel else [k for k in KINDS + ROI_KINDS if k in launch]
    us = {kind: [] for kind in kinds}
    for _ in range(args.rounds):
        for kind in kinds:
            us[kind].append(timed(launch[kind], args.steps, args.warmup))
    rows = {}
    for kind in kinds:
        t = float(np.median(us[kind]))
        rows[kind] = {'launch_us': t, 'launch_us_per_round': us[kind], 'bytes': int(nbytes[kind]), 'launch_TBs': nbytes[kind] / (t * 1e-6) / 1e12}
    for kind in kinds:
        if kind.endswith('_fit') and kind[:-4] in rows:
            rows[kind]['fit_vs_stretch'] = rows[kind]['launch_us'] / rows[kind[:-4]]['launch_us']
    dx, dy, iw, ih = fit_geometry(SRC, DST, 'LETTERBOX')
    line = {'metric': 'one request\'s input, uint8 1080p frames -> (n, 3, 300, 300) fp32: the fitted launch against the stretch, event-timed',
            'batch': n, 'geometry_dx_dy_iw_ih': [dx, dy, iw, ih], 'kinds': rows, 'launches_per_round': args.steps, 'rounds': args.rounds,
            'git_head': git_head(args.head), 'device': device.device_name(), 'date': time.strftime('%Y-%m-%d')}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
