"""A cascade's ROI table made on the device (pyopenvino_amd.DetectedRois): what it costs and what it saves.

One process, the kinds alternating over `--rounds` rounds, medians of event-timed launches (as bench_preprocess_roi.py):

  table    pvhip_detections_to_rois alone: R = 128 x 100 seeded records (lists of 20..100 live records), n = 256.
  bound    pvhip_input_preprocess_yuv_roi_f32 on one (1080, 1920) NV12 frame and 256 rectangles with sides of 32..400 pixels -> 224 x 224,
           sized for the whole frame (what a DetectedRois launch is given: the host does not know the largest rectangle) against the same
           launch sized for the table's true largest rectangle.
  cascade  detector pass end -> classifier input ready: SSD-MobileNet at batch 2 (synthetic weights) on (480, 640) U8 NHWC frames, then
           the input tensor of GoogLeNet at batch 8, between an event behind the detector's pass and one behind the classifier's staging.
           device: start_async(DetectedRois(frames, detector request)) staged while the detector is in flight; host: detector.wait(), the
           rule in vectorised numpy on the read-back records, then the staging of RoiInput(frames, table).  The classifier's pass itself
           is not run: both routes would add the same time.

Prints one JSON line; --out writes it too.
Run each GPU step under its own time limit, e.g.  timeout -k 10 300 python scripts/bench_detected_rois.py --out profiles/detected_rois.json
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

from pyopenvino_amd import DetectedRois, IECore, RoiInput, device, synth  # noqa: E402
from bench_preprocess_roi import boxes, median_rounds, ptr  # noqa: E402
from bench_preprocess_yuv import frames, git_head  # noqa: E402

MODELS = os.path.join(REPO, 'models')
FRAME, DST = (1080, 1920), (224, 224)


def records(rng, images, per_image):
    """Seeded DetectionOutput-like records: every image a list of 20..per_image live records, a terminator, zeros."""
    rec = np.zeros((images, per_image, 7), np.float32)
    rec[..., 0] = np.arange(per_image)
    rec[..., 1] = rng.integers(1, 91, (images, per_image))
    rec[..., 2] = rng.uniform(0, 1, (images, per_image))
    lo = rng.uniform(0, 0.7, (images, per_image, 2))
    rec[..., 3:5], rec[..., 5:7] = lo, lo + rng.uniform(0.02, 0.3, (images, per_image, 2))
    for b, end in enumerate(rng.integers(20, per_image + 1, images)):
        if end < per_image:
            rec[b, end:] = 0
            rec[b, end, 0] = -1
    return rec.reshape(1, 1, images * per_image, 7)


def host_table(rec, n, images, extent, conf):
    """The rule of tests/detected_rois_ref.py for labels=None and min_size (1, 1), vectorised: the padded (n, 5) table, count."""
    rec = rec.reshape(images, -1, 7)
    P, (H, W) = rec.shape[1], extent
    dead = ~(rec[..., 0] >= 0)
    live = np.arange(P)[None, :] < np.where(dead.any(1), dead.argmax(1), P)[:, None]
    f = np.float32
    x0 = np.floor(np.clip(rec[..., 3] * f(W), 0, f(W)))
    y0 = np.floor(np.clip(rec[..., 4] * f(H), 0, f(H)))
    w, h = np.ceil(np.clip(rec[..., 5] * f(W), 0, f(W))) - x0, np.ceil(np.clip(rec[..., 6] * f(H), 0, f(H))) - y0
    keep = live & (rec[..., 2] >= f(conf)) & np.isfinite(rec[..., 3:]).all(-1) & (w >= 1) & (h >= 1)
    b, p = np.nonzero(keep)
    table = np.tile(np.array([0, 0, 0, 1, 1], np.int32), (n, 1))
    k = min(n, len(b))
    table[:k] = np.stack([b, x0[b, p], y0[b, p], w[b, p], h[b, p]], 1)[:k]
    return table, k


def loaded(model, batch, seed, declare, requests=1):
    ie = IECore(plugin_package='pyopenvino_amd.op_plugins')
    net = ie.read_network(os.path.join(MODELS, model + '.xml'), weights=synth.synth_weights(os.path.join(MODELS, model + '.xml'), seed))
    net.set_batch(batch)
    name = net.inputs[0]['name']
    info = net.input_info[name]
    info.precision, info.layout = 'U8', 'NHWC'
    info.preprocess_info.resize_algorithm = 'RESIZE_BILINEAR'
    declare(info.preprocess_info)
    return ie.load_network(net, 'GPU', num_requests=requests), name, net.outputs[0]['name']


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=200, help='timed launches per kind and round')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5, help='rounds over the kinds (alternating, one process)')
    ap.add_argument('--cascade-steps', type=int, default=20, help='timed cascade steps per route and round')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--head', default=None, help='git commit to report (default: git rev-parse HEAD, when the tree is a checkout)')
    args = ap.parse_args()
    device.init(0)
    rng = np.random.default_rng(2026)
    N = 256

    # ---- the table kernel alone
    images, per_image = 128, 100
    rec = device.DeviceTensor.from_numpy(records(rng, images, per_image))
    out = device.DeviceTensor.empty((6 * N + 2,), np.int32)
    o = out.ptr
    launch = {'table': lambda: device.call('pvhip_detections_to_rois', ptr(rec), ctypes.c_void_p(o), ctypes.c_void_p(o + 20 * N),
                                           ctypes.c_void_p(o + 24 * N), N, images, per_image, *FRAME, 0.5, None, 0, 1, 1)}
    us = median_rounds(launch, args.rounds, args.steps, args.warmup)
    counts = np.asarray(out)[6 * N:].tolist()
    table = {'records': images * per_image, 'n': N, 'launch_us': float(np.median(us['table'])), 'launch_us_per_round': us['table'],
             'count': counts[0], 'selected': counts[1]}

    # ---- the ROI launch sized for the whole frame against the true largest rectangle
    fh, fw = FRAME
    rois = boxes(rng, N, FRAME)
    frame = device.DeviceTensor.from_numpy(frames(rng, 1, fh, fw, 'nv12'))
    rois_dev = device.DeviceTensor.from_numpy(rois)
    dst = device.DeviceTensor.empty((N, 3) + DST)
    largest = (int(rois[:, 4].max()), int(rois[:, 3].max()))
    roi = lambda bound: device.call('pvhip_input_preprocess_yuv_roi_f32', ptr(frame), ptr(dst), ptr(rois_dev), N, 1, fh, fw, *DST, *bound,  # noqa: E731
                                    0, 0, None, None)
    us = median_rounds({'frame_bound': lambda: roi(FRAME), 'true_bound': lambda: roi(largest)}, args.rounds, args.steps, args.warmup)
    bound = {kind: {'launch_us': float(np.median(v)), 'launch_us_per_round': v} for kind, v in us.items()}
    bound['largest_rectangle_hw'] = list(largest)
    bound['frame_vs_true'] = bound['frame_bound']['launch_us'] / bound['true_bound']['launch_us']
    bound['frame_vs_true_per_round'] = [a / b for a, b in zip(us['frame_bound'], us['true_bound'])]
    del frame, rois_dev, dst

    # ---- detector pass end -> classifier input ready
    m, n, hw = 2, 8, (480, 640)
    det, det_name, det_out = loaded('ssd_mobilenet_v1_coco', m, 1234, lambda pre: setattr(pre, 'reverse_channels', True))
    cls, name, _ = loaded('googlenet-v1', n, 11, lambda pre: None)
    dreq, runner = det.requests[0], cls.requests[0].runner
    images_u8 = rng.integers(0, 256, (m,) + hw + (3,), dtype=np.uint8)
    buf = cls.requests[0].input_buffer(name, hw, frames=m)
    buf[...] = images_u8
    for _ in range(4):                                        # the detector replays its recording from here on
        first = np.array(dreq.infer({det_name: images_u8})[det_out], copy=True)
    live = first.reshape(m, -1, 7)[0]
    live = live[:np.argmax(~(live[:, 0] >= 0))] if (~(live[:, 0] >= 0)).any() else live
    conf = float(np.median(live[:, 2]))
    e0, e1 = device.Event(), device.Event()

    def step(route):
        dreq.start_async({det_name: images_u8})
        device.select_stream(dreq.runner.stream_base)
        e0.record()
        if route == 'device':
            runner.host_inputs.stage({name: DetectedRois(buf, dreq, min_confidence=conf)}, runner.stream_base)
            device.select_stream(runner.stream_base)
            e1.record()
            dreq.wait()
        else:
            got = dreq.wait()[det_out]
            t, _ = host_table(got, n, m, hw, conf)
            runner.host_inputs.stage({name: RoiInput(buf, t)}, runner.stream_base)
            device.select_stream(runner.stream_base)
            e1.record()
        e1.synchronize()
        device.select_stream(0)
        device.synchronize()
        return e0.elapsed_ms(e1) * 1e3

    cascade = {route: [] for route in ('device', 'host')}
    for route in cascade:
        step(route)
    for _ in range(args.rounds):
        for route in cascade:
            cascade[route].append(float(np.median([step(route) for _ in range(args.cascade_steps)])))
    want, count = host_table(first, n, m, hw, conf)
    cls.requests[0].infer({name: DetectedRois(buf, first, min_confidence=conf)})
    got = cls.requests[0].detected_rois(name)
    agree = bool(got.count == count and np.array_equal(got.rois[:count], want[:count]))
    cascade = {route: {'us': float(np.median(v)), 'us_per_round': v} for route, v in cascade.items()}
    cascade.update(device_vs_host=cascade['device']['us'] / cascade['host']['us'], count=int(count), min_confidence=conf,
                   device_table_equals_host_table=agree)

    line = {'metric': 'DetectedRois: the ROI table made on the device, event-timed', 'table_128x100_records_n256': table,
            'bound_1x1080x1920_nv12_256_rectangles->224x224': bound, 'cascade_ssd_b2_480x640->googlenet_b8_input_ready': cascade,
            'launches_per_round': args.steps, 'cascade_steps_per_round': args.cascade_steps, 'rounds': args.rounds,
            'git_head': git_head(args.head), 'device': device.device_name(), 'date': time.strftime('%Y-%m-%d'), 'profiled_with_rocprofv3': False}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
