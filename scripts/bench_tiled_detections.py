"""A tiled detector's answer made on the device (``infer(..., detections=TiledScreen(...))``): what the added launches and the read-back
cost, against what the project offered before: reading the whole Result back and merging the tiles on the host.

SSD-MobileNet fp32 at batch 128: one pass on 8 U8 / NHWC (1080, 1920) frames cut into 16 overlapping tiles each (a RoiInput), whose
(1, 1, 12800, 7) Result is put back on the device.  On that Result, over `--rounds` rounds of ONE child process under its own `timeout` (the
parent never opens the device), at min_confidence = 0.5 and at the median score of the live records:

  device   pvhip_detections_merge_tiles (three launches), then the read-back of 4 (2 m + 1) bytes and of 32 bytes per row: a host clock
           around `--calls` launch + read-back pairs, each ending in its synchronous copy; and the launches alone by hipEvents;
  host     the whole Result read back (358 400 bytes) and tiled_detections.merge_tiles on it: the same host clock;
and that both give the same table, word for word.  No threshold is fixed here: the two times are reported.

Prints one JSON line; --out writes it too.  e.g.  python scripts/bench_tiled_detections.py --out profiles/tiled_detections.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BATCH, PER_TILE, FRAMES, EXTENT, CONF = 128, 100, 8, (1080, 1920), 0.5
STEP_LIMIT = 420                                              # seconds the child may take


def tile_table():
    """16 tiles of (360, 640) per frame on a 4 x 4 grid: neighbours overlap by a third of a tile horizontally, a third vertically."""
    h, w = 360, 640
    ys, xs = np.linspace(0, EXTENT[0] - h, 4).astype(int), np.linspace(0, EXTENT[1] - w, 4).astype(int)
    return np.array([(f, x, y, w, h) for f in range(FRAMES) for y in ys for x in xs], np.int32)


def detector():
    from pyopenvino_amd import IECore, synth
    xml = os.path.join(REPO, 'models', 'ssd_mobilenet_v1_coco.xml')
    ie = IECore()
    net = ie.read_network(xml, weights=synth.synth_weights(xml, 1234))
    net.set_batch(BATCH)
    info = net.input_info[net.inputs[0]['name']]
    info.precision, info.layout = 'U8', 'NHWC'
    info.preprocess_info.resize_algorithm = 'RESIZE_BILINEAR'
    return ie.load_network(net, 'GPU', num_requests=1), net.inputs[0]['name'], net.outputs[0]['name']


def words(d):
    return np.concatenate([d.rois, d.labels[:, None], d.scores.view(np.int32)[:, None], d.records[:, None]], axis=1)


def step(args):
    from pyopenvino_amd import RoiInput, TiledScreen, device, tiled_detections
    device.init(0)
    ex, name, out_name = detector()
    rng = np.random.default_rng(9000)
    tiles = tile_table()
    assert tiles.shape == (BATCH, 5)
    feed = RoiInput(rng.integers(0, 256, (FRAMES,) + EXTENT + (3,), dtype=np.uint8), tiles)
    req = ex.requests[0]
    records = np.array(req.infer({name: feed})[out_name], copy=True)
    assert records.shape == (1, 1, BATCH * PER_TILE, 7)
    result, table = device.DeviceTensor.from_numpy(records), device.DeviceTensor.from_numpy(tiles)    # where a pass leaves them
    rec = records.reshape(-1, 7)
    median = float(np.median(rec[rec[:, 0] >= 0, 2]))
    e0, e1 = device.Event(), device.Event()
    out = {}
    for kind, conf in (('min_confidence_0.5', CONF), ('min_confidence_median', median)):
        screen = tiled_detections.resolved(TiledScreen(conf), BATCH, PER_TILE)
        blocks = tiled_detections.Blocks(BATCH, PER_TILE, FRAMES, screen)
        device_us, launch_us, host_us = [], [], []
        for _ in range(args.rounds):
            for _ in range(args.warmup):
                blocks.launch(result, table)
                got = blocks.read_back()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                blocks.launch(result, table)
                got = blocks.read_back()
            device_us.append((time.perf_counter() - t0) * 1e6 / args.calls)
            e0.record()
            for _ in range(args.calls):
                blocks.launch(result, table)
            e1.record()
            e1.synchronize()
            launch_us.append(e0.elapsed_ms(e1) * 1e3 / args.calls)
            t0 = time.perf_counter()
            for _ in range(args.host_calls):
                want = tiled_detections.merge_tiles(np.asarray(result), tiles, FRAMES, screen)
            host_us.append((time.perf_counter() - t0) * 1e6 / args.host_calls)
        same = bool(np.array_equal(got.counts, want.counts) and np.array_equal(got.selected, want.selected) and np.array_equal(words(got), words(want)))
        out[kind] = {'min_confidence': conf, 'max_per_tile': screen.max_per_tile, 'candidates': int(got.selected.sum()), 'rows': int(got.counts.sum()),
                     'same_table': same, 'device_us': float(np.median(device_us)), 'launches_alone_us': float(np.median(launch_us)),
                     'host_us': float(np.median(host_us)), 'host_over_device': float(np.median(host_us) / np.median(device_us)),
                     'device_us_per_round': device_us, 'launches_alone_us_per_round': launch_us, 'host_us_per_round': host_us,
                     'bytes_read_back': {'device': 4 * (2 * FRAMES + 1) + 32 * int(got.counts.sum()), 'host': int(records.nbytes)}}
    out.update(tiles=BATCH, frames=FRAMES, records_per_tile=PER_TILE, frame_extent=list(EXTENT), calls_per_round=args.calls,
               host_calls_per_round=args.host_calls, rounds=args.rounds, device=device.device_name())
    return out


def git_head(head):
    if head is None:
        try:
            head = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=REPO, capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    return head


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=100, help='timed launch + read-back pairs (and launches alone) per round')
    ap.add_argument('--host-calls', type=int, default=5, help='timed read-back + merge_tiles calls on the host per round')
    ap.add_argument('--warmup', type=int, default=5, help='untimed calls in front of every round')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--head', default=None, help='git commit to report (default: git rev-parse HEAD, when the tree is a checkout)')
    ap.add_argument('--step', action='store_true', help='(the child process) measure here and print the JSON')
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step(args)))
        return 0
    passed_on = [a for k in ('calls', 'host_calls', 'warmup', 'rounds') for a in ('--' + k.replace('_', '-'), str(getattr(args, k)))]
    child = subprocess.run(['timeout', '-k', '10', str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), '--step'] + passed_on,
                           stdout=subprocess.PIPE, text=True)
    if child.returncode != 0:
        print('bench_tiled_detections: the measurement ended with status {}'.format(child.returncode), file=sys.stderr)
        return child.returncode
    line = {'metric': 'tiled detections: 128 tiles of 8 frames merged on the device, SSD-MobileNet batch 128'}
    line.update(json.loads(child.stdout.strip().splitlines()[-1]))
    line.update(git_head=git_head(args.head), date=time.strftime('%Y-%m-%d'), profiled_with_rocprofv3=False)
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
