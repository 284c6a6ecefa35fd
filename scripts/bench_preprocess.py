"""Inputs preprocessed on the device against the device-resident rate: GoogLeNet fp32, batch 256, `--requests` (6) whole-batch requests in
flight, the same number of pipelined passes timed in each mode, the modes alternating over `--rounds` rounds of ONE run:

  1. resident          every request reads its own DeviceTensor (what bench.py times), the reference point
  2. u8_nhwc_buf       U8 NHWC 224 x 224 images from the requests' page-locked buffers, converted on the device (pvhip_input_to_nchw_f32)
  3. resize_256x256    U8 NHWC 256 x 256 images from the requests' buffers, resized on the device (pvhip_input_preprocess_f32)
  4. resize_480x640    U8 NHWC 480 x 640 images (camera frames), the same

Modes 2-4 run on one network declared U8 / NHWC / RESIZE_BILINEAR (a 224 x 224 source is not resized: the conversion alone).  Every pass
gets different host images: a buffer mode rewrites one image of the request's buffer before each pass, as bench_host_input.py does.
Prints one JSON line (images/s, ratio to mode 1, how many timed passes were replays, the H2D GB/s those rates imply -- images/s x bytes
per image, not a timed copy --, and the event-timed rate of a lone page-locked copy on the copy stream); --out writes it too.

--kernel: instead, time the preprocessing kernel alone (device events around --steps launches) on a (256, 480, 640, 3) and a
(256, 256, 256, 3) uint8 batch -> (256, 3, 224, 224): the run to take under  rocprofv3 --kernel-trace --stats.
Run each GPU step under its own time limit, e.g.  timeout -k 10 600 python scripts/bench_preprocess.py --out profiles/preprocess.json
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

from pyopenvino_amd import IECore, device, synth  # noqa: E402

XML = os.path.join(REPO, 'models', 'googlenet-v1.xml')
WEIGHT_SEED = 1234
HBM_PEAK = 8e12


def load(blob, batch, requests, preprocess):
    ie = IECore()
    net = ie.read_network(XML, weights=blob)
    net.set_batch(batch)
    name = net.inputs[0]['name']
    if preprocess:
        info = net.input_info[name]
        info.precision, info.layout = 'U8', 'NHWC'
        info.preprocess_info.resize_algorithm = 'RESIZE_BILINEAR'
    return ie.load_network(net, 'GPU', num_requests=requests), name


def pipelined(ex, n_req, steps, feed):
    """`steps` passes, request r = step % n_req, each started as soon as its previous pass has been waited for.  Returns how many of
    them were replays of the request's recording."""
    in_flight, replays = [], 0
    for step in range(steps):
        r = step % n_req
        if r in in_flight:
            in_flight.remove(r)
            ex.wait(r)
        ex.start_async(r, feed(r, step))
        replays += ex.requests[r]._replayed is not None
        in_flight.append(r)
    for r in in_flight:
        ex.wait(r)
    return replays


def timed(ex, n_req, steps, warmup, feed):
    """(seconds, replayed passes) of `steps` timed passes after `warmup` untimed ones."""
    pipelined(ex, n_req, warmup, feed)
    t0 = time.perf_counter()
    replays = pipelined(ex, n_req, steps, feed)
    return time.perf_counter() - t0, replays


def h2d_rate(nbytes, reps=5):
    """GB/s of pvhip_memcpy_h2d_async from page-locked memory on the copy stream (device events around `reps` copies)."""
    host = device.host_empty((nbytes,), np.uint8)
    host[:] = 1
    dst = device.DeviceTensor.empty((nbytes,), np.uint8)
    device.select_stream(device.COPY_STREAM)
    device.call('pvhip_memcpy_h2d_async', ctypes.c_void_p(dst.ptr), ctypes.c_void_p(host.ctypes.data), nbytes)
    e0, e1 = device.Event(), device.Event()
    e0.record()
    for _ in range(reps):
        device.call('pvhip_memcpy_h2d_async', ctypes.c_void_p(dst.ptr), ctypes.c_void_p(host.ctypes.data), nbytes)
    e1.record()
    e1.synchronize()
    device.select_stream(0)
    return reps * nbytes / (e0.elapsed_ms(e1) * 1e-3) / 1e9


def git_head(head):
    if head is None:
        try:
            head = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=REPO, capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    return head


def kernel_only(args):
    """Event-timed launches of pvhip_input_preprocess_f32 alone; bytes/s = (source bytes + fp32 output bytes) / kernel time."""
    B = args.batch
    rng = np.random.default_rng(7)
    dst = device.DeviceTensor.empty((B, 3, 224, 224))
    rows = {}
    for hs, ws in ((480, 640), (256, 256)):
        src = device.DeviceTensor.from_numpy(rng.integers(0, 256, (B, hs, ws, 3), dtype=np.uint8))
        launch = lambda: device.call('pvhip_input_preprocess_f32', ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), B, 3, hs, ws,  # noqa: E731
                                     224, 224, 1, 1, 0, None, None)
        for _ in range(3):
            launch()
        e0, e1 = device.Event(), device.Event()
        e0.record()
        for _ in range(args.steps):
            launch()
        e1.record()
        e1.synchronize()
        us = e0.elapsed_ms(e1) * 1e3 / args.steps
        nbytes = src.nbytes + dst.nbytes
        rows['{}x{}'.format(hs, ws)] = {'us_per_launch': us, 'bytes_in': src.nbytes, 'bytes_out': dst.nbytes,
                                        'TBs': nbytes / (us * 1e-6) / 1e12, 'frac_of_8TBs': nbytes / (us * 1e-6) / HBM_PEAK}
        del src
    line = {'metric': 'pvhip_input_preprocess_f32 uint8 NHWC batch {} -> (N, 3, 224, 224) fp32, event-timed'.format(B), 'kernels': rows,
            'launches': args.steps, 'git_head': git_head(args.head), 'device': device.device_name()}
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=60, help='timed passes per mode and round (default 60: ten per request)')
    ap.add_argument('--warmup', type=int, default=18, help='untimed passes per mode and round first (recordings are made there)')
    ap.add_argument('--rounds', type=int, default=3, help='rounds over the modes (alternating, same box)')
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--requests', type=int, default=6)
    ap.add_argument('--kernel', action='store_true', help='time the preprocessing kernel alone (see above)')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--head', default=None, help='git commit to report (default: git rev-parse HEAD, when the tree is a checkout)')
    args = ap.parse_args()
    device.init(0)
    if args.kernel:
        return kernel_only(args)
    B, R = args.batch, args.requests
    blob = synth.synth_weights(XML, WEIGHT_SEED)
    rng = np.random.default_rng(2026)
    extents = {'u8_nhwc_buf': (224, 224), 'resize_256x256': (256, 256), 'resize_480x640': (480, 640)}

    ex_res, name = load(blob, B, R, False)
    x_dev = [device.DeviceTensor.from_numpy(synth.uniform_pixels(1000 + r, (B, 3, 224, 224))) for r in range(R)]
    ex, _ = load(blob, B, R, True)
    bufs, fresh = {}, {}
    for mode, (h, w) in extents.items():
        bufs[mode] = [req.input_buffer(name, (h, w)) for req in ex.requests]
        for b in bufs[mode]:
            b[...] = rng.integers(0, 256, b.shape, dtype=np.uint8)
        fresh[mode] = rng.integers(0, 256, (R + 1, h, w, 3), dtype=np.uint8)     # one new image per pass goes into the buffers

    def feeder(mode):
        def feed(r, s):
            bufs[mode][r][s % B] = fresh[mode][s % (R + 1)]
            return {name: bufs[mode][r]}
        return feed

    times = {mode: [] for mode in ['resident'] + list(extents)}
    for _ in range(args.rounds):
        times['resident'].append(timed(ex_res, R, args.steps, args.warmup, lambda r, s: {name: x_dev[r]}))
        for mode in extents:
            times[mode].append(timed(ex, R, args.steps, args.warmup, feeder(mode)))
    out = {}
    for mode, runs in times.items():
        rates = [args.steps * B / t for t, _ in runs]
        out[mode] = {'images_per_sec': float(np.median(rates)), 'per_round': rates,
                     'timed_passes_replayed': '{} of {}'.format(sum(n for _, n in runs), args.steps * len(runs))}
    base = out['resident']['images_per_sec']
    for mode, (h, w) in extents.items():
        row = out[mode]
        row['bytes_per_image'] = h * w * 3
        row['h2d_GBs_implied'] = row['images_per_sec'] * row['bytes_per_image'] / 1e9     # demand at that rate, not a timed copy
    for row in out.values():
        row['ratio_to_resident'] = row['images_per_sec'] / base
    line = {'metric': 'googlenet-v1 fp32 batch {} images/s from host images preprocessed on the device, {} requests in flight'.format(B, R),
            'modes': out, 'pinned_h2d_GBs': h2d_rate(B * 480 * 640 * 3), 'steps_per_mode': args.steps, 'warmup_per_mode': args.warmup,
            'rounds': args.rounds, 'git_head': git_head(args.head), 'device': device.device_name()}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
