"""A detector over regions, its answer made on the device (``infer(..., detections=RegionScreen(...))``): what the launches and the
read-back cost, (a) against what the project offered before for the same pass -- the whole Result read back, for a DetectedRois the table
too, and the rule applied in numpy -- and (b) against pvhip_detections_merge_tiles on the same records and table, which is what the
per-region geometry (one integer fit per wave, twelve flops per record) is added to.

SSD-MobileNet fp32 at batch 128 with resize_fit LETTERBOX declared: one pass on 8 U8 / NHWC (1080, 1920) frames and a RoiInput of 16
regions of mixed aspect each, whose (1, 1, 12800, 7) Result is put back on the device.  On that Result, over `--rounds` rounds of ONE child
process under its own `timeout` (the parent never opens the device), at the median score of the live records:

  (a) device   pvhip_detections_merge_regions with fit 1 (three launches), then the read-back of 4 (2 m + 1) bytes and of 32 bytes per row:
               a host clock around `--calls` launch + read-back pairs, each ending in its synchronous copy;
      host     the whole Result read back (358 400 bytes) and tiled_detections.merge_regions on it: the same host clock.  For the
               'detected' feed the table is one whose last quarter is (-1, 0, 0, 0, 0), as a DetectedRois leaves it behind `count`, and
               the host route reads its 6 n + 2 ints back as well, as InferRequest.detected_rois() does;
      and that both give the same table, word for word.
  (b) the three launches alone by hipEvents, `--calls` of them between two events: the tiles entry, the regions entry with fit 1, the
      tiles entry again, in that order in every round.  The spread of the tiles entry is the difference of its two medians and the range of
      its rounds; the regions entry is set against it.  The two entries do not make the same rectangles -- fit 1 maps the corners back --,
      so the suppression in the frames launch has other work to do; the comparison is therefore made a second time at threshold 1.0,
      where nothing is suppressed and both keep every candidate: there the candidates launch is all that differs.
No threshold is fixed here: the times are reported.

Prints one JSON line; --out writes it too.  e.g.  python scripts/bench_region_screen.py --out profiles/region_screen.json
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

BATCH, PER_REGION, FRAMES, EXTENT, NET = 128, 100, 8, (1080, 1920), (300, 300)
STEP_LIMIT = 420                                              # seconds the child may take


def region_table(rng):
    """16 regions per frame, none square: wide, tall and thin ones anywhere in the frame."""
    H, W = EXTENT
    w = rng.integers(120, 961, BATCH)
    h = np.where(rng.integers(0, 2, BATCH) == 0, w * rng.integers(20, 60, BATCH) // 100, w * rng.integers(140, 300, BATCH) // 100)
    h = np.clip(h, 40, H)
    return np.stack([np.repeat(np.arange(FRAMES), BATCH // FRAMES), rng.integers(0, W - w + 1), rng.integers(0, H - h + 1), w, h], axis=1).astype(np.int32)


def detector():
    from pyopenvino_amd import IECore, synth
    xml = os.path.join(REPO, 'models', 'ssd_mobilenet_v1_coco.xml')
    ie = IECore()
    net = ie.read_network(xml, weights=synth.synth_weights(xml, 1234))
    net.set_batch(BATCH)
    info = net.input_info[net.inputs[0]['name']]
    info.precision, info.layout = 'U8', 'NHWC'
    info.preprocess_info.resize_algorithm = 'RESIZE_BILINEAR'
    info.preprocess_info.resize_fit = 'LETTERBOX'
    info.preprocess_info.pad_value = 114.0
    return ie.load_network(net, 'GPU', num_requests=1), net.inputs[0]['name'], net.outputs[0]['name']


def words(d):
    return np.concatenate([d.rois, d.labels[:, None], d.scores.view(np.int32)[:, None], d.records[:, None]], axis=1)


def same(a, b):
    return bool(np.array_equal(a.counts, b.counts) and np.array_equal(a.selected, b.selected) and np.array_equal(words(a), words(b)))


def launches_alone(e0, e1, calls, launch):
    e0.record()
    for _ in range(calls):
        launch()
    e1.record()
    e1.synchronize()
    return e0.elapsed_ms(e1) * 1e3 / calls


def step(args):
    from pyopenvino_amd import RegionScreen, RoiInput, TiledScreen, device, tiled_detections
    device.init(0)
    ex, name, out_name = detector()
    rng = np.random.default_rng(9001)
    regions = region_table(rng)
    assert regions.shape == (BATCH, 5)
    feed = RoiInput(rng.integers(0, 256, (FRAMES,) + EXTENT + (3,), dtype=np.uint8), regions)
    records = np.array(ex.requests[0].infer({name: feed})[out_name], copy=True)
    assert records.shape == (1, 1, BATCH * PER_REGION, 7)
    result = device.DeviceTensor.from_numpy(records)                            # where a pass leaves it
    rec = records.reshape(-1, 7)
    conf = float(np.median(rec[rec[:, 0] >= 0, 2]))
    screen = tiled_detections.resolved(RegionScreen(conf), BATCH, PER_REGION)
    tiled_screen = tiled_detections.resolved(TiledScreen(conf), BATCH, PER_REGION)
    placed = (NET[0], NET[1], 1)
    e0, e1 = device.Event(), device.Event()
    out = {}
    # ---- (a)
    behind = regions.copy()
    behind[3 * BATCH // 4:] = (-1, 0, 0, 0, 0)
    for kind, host_table in (('roi_input', regions), ('detected', behind)):
        block = np.zeros(6 * BATCH + 2, np.int32)                               # the slot's (n, 5) rois | record_of | (count, selected)
        block[:5 * BATCH] = host_table.ravel()
        whole = device.DeviceTensor.from_numpy(block)
        table = device.DeviceTensor(whole._block, (BATCH, 5), np.int32)
        blocks = tiled_detections.RegionBlocks(BATCH, PER_REGION, FRAMES, screen)
        device_us, host_us = [], []
        for _ in range(args.rounds):
            for _ in range(args.warmup):
                blocks.launch(result, table, *placed)
                got = blocks.read_back()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                blocks.launch(result, table, *placed)
                got = blocks.read_back()
            device_us.append((time.perf_counter() - t0) * 1e6 / args.calls)
            t0 = time.perf_counter()
            for _ in range(args.host_calls):
                t = np.asarray(whole)[:5 * BATCH].reshape(BATCH, 5) if kind == 'detected' else host_table
                want = tiled_detections.merge_regions(np.asarray(result), t, FRAMES, screen, NET, 'LETTERBOX')
            host_us.append((time.perf_counter() - t0) * 1e6 / args.host_calls)
        out[kind] = {'min_confidence': conf, 'max_per_region': screen.max_per_region, 'candidates': int(got.selected.sum()),
                     'rows': int(got.counts.sum()), 'same_table': same(got, want), 'device_us': float(np.median(device_us)),
                     'host_us': float(np.median(host_us)), 'host_over_device': float(np.median(host_us) / np.median(device_us)),
                     'device_us_per_round': device_us, 'host_us_per_round': host_us,
                     'bytes_read_back': {'device': 4 * (2 * FRAMES + 1) + 32 * int(got.counts.sum()),
                                         'host': int(records.nbytes) + (int(block.nbytes) if kind == 'detected' else 0)}}
    # ---- (b)
    table = device.DeviceTensor.from_numpy(regions)
    for kind, threshold in (('launches_alone', 0.45), ('launches_alone_nothing_suppressed', 1.0)):
        region_blocks = tiled_detections.RegionBlocks(BATCH, PER_REGION, FRAMES, screen._replace(threshold=threshold))
        tile_blocks = tiled_detections.Blocks(BATCH, PER_REGION, FRAMES, tiled_screen._replace(threshold=threshold))
        series = {'tiles_first': [], 'regions_fit1': [], 'tiles_second': []}
        launches = {'tiles_first': lambda: tile_blocks.launch(result, table), 'regions_fit1': lambda: region_blocks.launch(result, table, *placed),
                    'tiles_second': lambda: tile_blocks.launch(result, table)}
        for _ in range(args.rounds):
            for key, launch in launches.items():
                for _ in range(args.warmup):
                    launch()
                series[key].append(launches_alone(e0, e1, args.calls, launch))
        fitted, tiled = region_blocks.read_back(), tile_blocks.read_back()
        med = {key: float(np.median(v)) for key, v in series.items()}
        both = series['tiles_first'] + series['tiles_second']
        out[kind] = {
            'threshold': threshold, 'tiles_us': float(np.median(both)), 'regions_fit1_us': med['regions_fit1'],
            'regions_minus_tiles_us': med['regions_fit1'] - float(np.median(both)),
            'tiles_spread_us': {'between_its_two_medians': abs(med['tiles_first'] - med['tiles_second']), 'range_of_rounds': float(max(both) - min(both))},
            'regions_range_of_rounds_us': float(max(series['regions_fit1']) - min(series['regions_fit1'])),
            'candidates': {'tiles': int(tiled.selected.sum()), 'regions_fit1': int(fitted.selected.sum())},
            'rows': {'tiles': int(tiled.counts.sum()), 'regions_fit1': int(fitted.counts.sum())}, 'us_per_round': series}
    out.update(regions=BATCH, frames=FRAMES, records_per_region=PER_REGION, frame_extent=list(EXTENT), calls_per_round=args.calls,
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
    ap.add_argument('--host-calls', type=int, default=5, help='timed read-back + merge_regions calls on the host per round')
    ap.add_argument('--warmup', type=int, default=5, help='untimed calls in front of every round')
    ap.add_argument('--rounds', type=int, default=7)
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
        print('bench_region_screen: the measurement ended with status {}'.format(child.returncode), file=sys.stderr)
        return child.returncode
    line = {'metric': 'region screen: 128 regions of 8 frames merged on the device, SSD-MobileNet batch 128, LETTERBOX'}
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
