"""A cascade's warp table fitted on the device (pyopenvino_amd.LandmarkWarps): what the removed host round trip is worth.

One process, the two routes alternating over `--rounds` rounds, medians of `--steps` timed steps each:

  table    pvhip_landmarks_to_warps alone, event-timed: n = 256 rows of K = 5 points over a table of regions.
  chain    one step of landmark network -> aligned crops -> consumer.  The landmark network is mnist at batch `--batch` (its (n, 10)
           softmax Result stands in for five normalised points per row), fed a RoiInput over U8 one-channel (480, 640) frames; the
           consumer is a second mnist at the same batch over the same frames.
           device: A.start_async(...), B.start_async({name: LandmarkWarps(frames, A, template)}) while A is in flight, A.wait(), B.wait().
           host:   A.start_async(...), A.wait(), read the Result, landmarks.to_warps, the table into warp_buffer, B.start_async({name:
                   WarpInput(frames, warp_buffer)}), B.wait() -- the route a caller had before, on the same commit.
           Two times per step: `wall_us` from before A.start_async to after B.wait() on the host's clock, and `gap_us` between a device
           event behind A's pass and one behind B's pass (what the consumer adds behind the landmark pass).

Prints one JSON line; --out writes it too.
Run each GPU step under its own time limit, e.g.  timeout -k 10 300 python scripts/bench_landmark_warps.py --out profiles/landmark_warps.json
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

from pyopenvino_amd import IECore, LandmarkWarps, RoiInput, WarpInput, device, landmarks  # noqa: E402
from bench_preprocess_roi import median_rounds, ptr  # noqa: E402
from bench_preprocess_yuv import git_head  # noqa: E402

MODELS = os.path.join(REPO, 'models')
FRAME = (480, 640)
TEMPLATE = [(8, 8), (20, 8), (14, 14), (9, 20), (19, 20)]     # five points in mnist's 28 x 28
IDENTITY = np.array([0, 65536, 0, 0, 0, 65536, 0], np.int64)  # what the host route feeds for a void row


def loaded(batch):
    ie = IECore(plugin_package='pyopenvino_amd.op_plugins')
    net = ie.read_network(os.path.join(MODELS, 'mnist.xml'))
    net.set_batch(batch)
    name = net.inputs[0]['name']
    info = net.input_info[name]
    info.precision, info.layout = 'U8', 'NCHW'
    info.preprocess_info.resize_algorithm = 'RESIZE_BILINEAR'
    return ie.load_network(net, 'GPU', num_requests=1), name, net.outputs[0]['name']


def boxes(rng, n, m):
    w, h = rng.integers(32, 201, n), rng.integers(32, 201, n)
    return np.stack([np.arange(n) % m, rng.integers(0, FRAME[1] - w + 1), rng.integers(0, FRAME[0] - h + 1), w, h], 1).astype(np.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=50, help='timed chain steps per route and round')
    ap.add_argument('--launches', type=int, default=200, help='timed launches of the table kernel per round')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5, help='rounds over the routes (alternating, one process)')
    ap.add_argument('--batch', type=int, default=64, help='rows of both networks')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--head', default=None, help='git commit to report (default: git rev-parse HEAD, when the tree is a checkout)')
    args = ap.parse_args()
    device.init(0)
    rng = np.random.default_rng(2026)

    # ---- the table kernel alone
    N, K = 256, len(TEMPLATE)
    points = device.DeviceTensor.from_numpy(rng.uniform(0, 1, (N, 2 * K)).astype(np.float32))
    regions = device.DeviceTensor.from_numpy(boxes(rng, N, 4))
    tmpl = device.DeviceTensor.from_numpy(landmarks.packed_template(TEMPLATE))
    table, valid = device.DeviceTensor.empty((N, 7), np.int64), device.DeviceTensor.empty((N + 1,), np.int32)
    launch = {'table': lambda: device.call('pvhip_landmarks_to_warps', ptr(points), ptr(regions), ptr(tmpl), ptr(table), ptr(valid),
                                           N, N, K, 4, *FRAME)}
    us = median_rounds(launch, args.rounds, args.launches, args.warmup)
    kernel = {'n': N, 'k': K, 'launch_us': float(np.median(us['table'])), 'launch_us_per_round': us['table'],
              'count': int(np.asarray(valid)[N])}

    # ---- one step of the chain, both routes
    n, m = args.batch, 4
    a_net, a_name, a_out = loaded(n)
    b_net, b_name, _ = loaded(n)
    A, B = a_net.requests[0], b_net.requests[0]
    images = rng.integers(0, 256, (m, 1) + FRAME, dtype=np.uint8)
    rois = boxes(rng, n, m)
    a_buf, a_rois = A.input_buffer(a_name, FRAME, frames=m), A.roi_buffer(a_name)
    a_buf[...], a_rois[...] = images, rois
    b_buf, b_table = B.input_buffer(b_name, FRAME, frames=m), B.warp_buffer(b_name)
    b_buf[...] = images
    for _ in range(4):                                        # the landmark request replays its recording from here on (made while
        A.infer({a_name: RoiInput(a_buf, a_rois)})            # nothing else holds its Result: a recording allocates nothing new)
    e0, e1 = device.Event(), device.Event()

    replayed = {}

    def step(route):
        t0 = time.perf_counter()
        A.start_async({a_name: RoiInput(a_buf, a_rois)})
        device.select_stream(A.runner.stream_base)
        e0.record()
        replayed['landmark'] = A._replayed is not None
        if route == 'device':
            B.start_async({b_name: LandmarkWarps(b_buf, A, TEMPLATE)})
            replayed['consumer'] = B._replayed is not None
            A.wait()
        else:
            result = A.wait()[a_out]
            fitted, ok = landmarks.to_warps(np.asarray(result, np.float32), rois, TEMPLATE, FRAME, m)
            b_table[...] = np.where(ok[:, None], fitted, IDENTITY)
            B.start_async({b_name: WarpInput(b_buf, b_table)})
        device.select_stream(B.runner.stream_base)
        e1.record()
        B.wait()
        e1.synchronize()
        wall = (time.perf_counter() - t0) * 1e6
        device.select_stream(0)
        return wall, e0.elapsed_ms(e1) * 1e3

    chain = {route: {'wall_us': [], 'gap_us': []} for route in ('device', 'host')}
    for route in chain:
        for _ in range(args.warmup):                          # both requests replay their recordings from here on
            step(route)
    for _ in range(args.rounds):
        for route in chain:
            walls, gaps = zip(*(step(route) for _ in range(args.steps)))
            chain[route]['wall_us'].append(float(np.median(walls)))
            chain[route]['gap_us'].append(float(np.median(gaps)))
    # the two routes make the same table
    step('device')
    got = B.landmark_warps(b_name)
    want, ok = landmarks.to_warps(np.asarray(A.infer({a_name: RoiInput(a_buf, a_rois)})[a_out], np.float32), rois, TEMPLATE, FRAME, m)
    agree = bool(np.array_equal(got.table, want) and np.array_equal(got.valid, ok))
    chain = {route: {'wall_us': float(np.median(v['wall_us'])), 'wall_us_per_round': v['wall_us'], 'gap_us': float(np.median(v['gap_us'])),
                     'gap_us_per_round': v['gap_us']} for route, v in chain.items()}
    chain.update(device_vs_host_wall=chain['device']['wall_us'] / chain['host']['wall_us'], valid_rows=int(got.count),
                 device_table_equals_host_table=agree, passes_replayed_from_recordings=replayed)

    line = {'metric': 'LandmarkWarps: the warp table fitted on the device', 'table_n256_k5': kernel,
            'chain_mnist_b{0}_480x640->mnist_b{0}'.format(n): chain, 'launches_per_round': args.launches, 'steps_per_round': args.steps,
            'rounds': args.rounds, 'git_head': git_head(args.head), 'device': device.device_name(), 'date': time.strftime('%Y-%m-%d'),
            'profiled_with_rocprofv3': False}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
