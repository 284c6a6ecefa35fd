"""Host inputs against the device-resident rate: GoogLeNet fp32, batch 256, `--requests` (6) whole-batch requests in flight, the same
number of pipelined passes timed in each mode of ONE run:

  1. resident        every request reads its own DeviceTensor (what bench.py times), the reference point
  2. fp32_nchw_buf   FP32 NCHW from the requests' page-locked buffers (InferRequest.input_buffer): async upload on the copy stream
  3. u8_nhwc_buf     U8 NHWC from the requests' buffers (IENetwork.input_info), converted on the device
  4. fp32_nchw_pageable   FP32 NCHW from pageable ndarrays: the default host path (synchronous upload, eager passes)

Every pass of modes 2-4 gets different host images: a buffer mode rewrites one image of the request's buffer before each pass (a
whole-buffer rewrite is the caller's decode work, not the upload's); the pageable mode rotates through requests + 1 arrays.
Prints one JSON line (images/s, ratio to mode 1, H2D GB/s implied, the raw page-locked H2D rate of the copy stream); --out writes it too.
Run each GPU step under its own time limit, e.g.  timeout -k 10 600 python scripts/bench_host_input.py --out profiles/host_input.json
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


def load(blob, batch, requests, u8_nhwc):
    ie = IECore()
    net = ie.read_network(XML, weights=blob)
    net.set_batch(batch)
    name = net.inputs[0]['name']
    if u8_nhwc:
        net.input_info[name].precision = 'U8'
        net.input_info[name].layout = 'NHWC'
    return ie.load_network(net, 'GPU', num_requests=requests), name, net.outputs[0]['name']


def pipelined(ex, n_req, steps, feed):
    """`steps` passes, request r = step % n_req, each started as soon as its previous pass has been waited for."""
    in_flight = []
    for step in range(steps):
        r = step % n_req
        if r in in_flight:
            in_flight.remove(r)
            ex.wait(r)
        ex.start_async(r, feed(r, step))
        in_flight.append(r)
    for r in in_flight:
        ex.wait(r)


def timed(ex, n_req, steps, warmup, feed):
    pipelined(ex, n_req, warmup, feed)
    t0 = time.perf_counter()
    pipelined(ex, n_req, steps, feed)
    return time.perf_counter() - t0


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=60, help='timed passes per mode (default 60: ten per request)')
    ap.add_argument('--warmup', type=int, default=18, help='untimed passes per mode first (recordings are made there)')
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--requests', type=int, default=6)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--head', default=None, help='git commit to report (default: git rev-parse HEAD, when the tree is a checkout)')
    args = ap.parse_args()
    device.init(0)
    B, R = args.batch, args.requests
    blob = synth.synth_weights(XML, WEIGHT_SEED)
    rng = np.random.default_rng(2026)
    fresh = rng.integers(0, 256, (R + 1, 224, 224, 3), dtype=np.uint8)     # one new image per pass goes into the buffers
    per_image_f32, per_image_u8 = 3 * 224 * 224 * 4, 3 * 224 * 224
    out = {}

    ex, name, _ = load(blob, B, R, False)
    x_dev = [device.DeviceTensor.from_numpy(synth.uniform_pixels(1000 + r, (B, 3, 224, 224))) for r in range(R)]
    dt = timed(ex, R, args.steps, args.warmup, lambda r, s: {name: x_dev[r]})
    out['resident'] = {'images_per_sec': args.steps * B / dt}
    replayed = all(req.runner.__dict__.get('_graph') is not None for req in ex.requests)
    del x_dev

    bufs = [req.input_buffer(name) for req in ex.requests]
    for r, b in enumerate(bufs):
        b[...] = synth.uniform_pixels(2000 + r, (B, 3, 224, 224))

    def feed_f32(r, s):
        bufs[r][s % B] = fresh[s % (R + 1)].transpose(2, 0, 1)
        return {name: bufs[r]}
    dt = timed(ex, R, args.steps, args.warmup, feed_f32)
    out['fp32_nchw_buf'] = {'images_per_sec': args.steps * B / dt, 'bytes_per_image': per_image_f32}
    del bufs

    pageable = [synth.uniform_pixels(3000 + k, (B, 3, 224, 224)) for k in range(R + 1)]
    dt = timed(ex, R, args.steps, args.warmup, lambda r, s: {name: pageable[(r + s) % (R + 1)]})
    out['fp32_nchw_pageable'] = {'images_per_sec': args.steps * B / dt, 'bytes_per_image': per_image_f32}
    del pageable
    ex.release_device_state()
    for req in ex.requests[1:]:
        req.runner.release_device_state()
    del ex

    ex, name, _ = load(blob, B, R, True)
    ubufs = [req.input_buffer(name) for req in ex.requests]
    for r, b in enumerate(ubufs):
        b[...] = rng.integers(0, 256, b.shape, dtype=np.uint8)

    def feed_u8(r, s):
        ubufs[r][s % B] = fresh[s % (R + 1)]
        return {name: ubufs[r]}
    dt = timed(ex, R, args.steps, args.warmup, feed_u8)
    out['u8_nhwc_buf'] = {'images_per_sec': args.steps * B / dt, 'bytes_per_image': per_image_u8}
    replayed_u8 = all(req.runner.__dict__.get('_graph') is not None for req in ex.requests)

    base = out['resident']['images_per_sec']
    for mode, row in out.items():
        row['ratio_to_resident'] = row['images_per_sec'] / base
        if 'bytes_per_image' in row:
            row['h2d_GBs'] = row['images_per_sec'] * row['bytes_per_image'] / 1e9
    head = args.head
    if head is None:
        try:
            head = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=REPO, capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    line = {'metric': 'googlenet-v1 fp32 batch {} host-input images/s, {} requests in flight'.format(B, R), 'modes': out,
            'pinned_h2d_GBs': h2d_rate(B * per_image_f32), 'steps_per_mode': args.steps, 'warmup_per_mode': args.warmup,
            'replayed_resident_and_fp32_buf': replayed, 'replayed_u8_nhwc': replayed_u8,
            'git_head': head, 'device': device.device_name()}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
