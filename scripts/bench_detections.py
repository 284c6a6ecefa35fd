"""A detector's answer made on the device (``infer(..., detections=...)``): what the launches cost and what the read-back saves.

SSD-MobileNet fp32, batch 128, `--requests` (2) whole-batch requests in flight, every request reading its own device-resident input,
blocks of `--steps` pipelined passes alternating between detections=None, detections=0.5 and detections=the median score of the live
records over `--rounds` rounds of ONE process.  (With the synthetic weights every record is live and scores above 0.5: 0.5 is the screen
that keeps everything, the median score the one that keeps half.)
Two steps, each a child process under its own `timeout` (the parent never opens the device; a step that fails ends the run):

  launch   on the (1, 1, 12800, 7) Result of one pass: pvhip_detections_compact alone (its two launches: one wave per image) at both
           thresholds and, as the yardstick the parallel form is measured against, pvhip_detections_to_rois on the same records with
           n = 12800 (one workgroup):
           device time per call by hipEvents around `--launches` back-to-back calls, one figure per round; and that both select the
           same number of records.
  blocks   images/s of every block, the bytes wait() handed back per request (the arrays it returned, counted), how many timed passes
           were replays, and the one condition, for either threshold: the median block with the keyword is not below the median
           detections=None block by more than the spread (max - min) between the detections=None blocks themselves.

Prints one JSON line; --out writes it too.  e.g.  python scripts/bench_detections.py --out profiles/detections.json
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

BATCH, PER_IMAGE, CONF, EXTENT = 128, 100, 0.5, (300, 300)
STEP_LIMIT = {'launch': 240, 'blocks': 480}                   # seconds each child may take


def nbytes_of(results):
    """Bytes of the host arrays a wait() returned."""
    return int(sum(sum(a.nbytes for a in v) if isinstance(v, tuple) else v.nbytes for v in results.values()))


def pipelined(ex, n_req, steps, feed, detections):
    """`steps` passes, request r = step % n_req, each started as soon as its previous pass has been waited for:
    (replayed passes, bytes handed back by the last wait())."""
    in_flight, replays, handed = [], 0, 0
    for step in range(steps):
        r = step % n_req
        if r in in_flight:
            in_flight.remove(r)
            handed = nbytes_of(ex.wait(r))
        ex.start_async(r, feed(r), detections=detections)
        replays += ex.requests[r]._replayed is not None
        in_flight.append(r)
    for r in in_flight:
        handed = nbytes_of(ex.wait(r))
    return replays, handed


def detector(requests):
    from pyopenvino_amd import IECore, synth
    xml = os.path.join(REPO, 'models', 'ssd_mobilenet_v1_coco.xml')
    ie = IECore()
    net = ie.read_network(xml, weights=synth.synth_weights(xml, 1234))
    net.set_batch(BATCH)
    return ie.load_network(net, 'GPU', num_requests=requests), net.inputs[0]['name'], net.outputs[0]['name']


def median_live_score(records):
    rec = np.asarray(records).reshape(-1, 7)
    return float(np.median(rec[rec[:, 0] >= 0, 2]))


def step_launch(args):
    from pyopenvino_amd import device, synth
    device.init(0)
    ex, name, out_name = detector(1)
    records = ex.infer({name: device.DeviceTensor.from_numpy(synth.uniform_pixels(9000, (BATCH, 3) + EXTENT))})[out_name]
    assert records.shape == (1, 1, BATCH * PER_IMAGE, 7)
    n = BATCH * PER_IMAGE
    x = device.DeviceTensor.from_numpy(records)
    header = device.DeviceTensor.empty((2 * BATCH + 1,), np.int32)
    rows = device.DeviceTensor.empty((n, 8), np.int32)
    table = device.DeviceTensor.empty((6 * n + 2,), np.int32)
    p = ctypes.c_void_p
    median = median_live_score(records)
    compact = lambda conf: device.call('pvhip_detections_compact', p(x.ptr), BATCH, PER_IMAGE, *EXTENT, conf, None, 0, 1, 1, PER_IMAGE,  # noqa: E731
                                       p(header.ptr), p(rows.ptr))
    calls = {'pvhip_detections_compact': lambda: compact(CONF), 'pvhip_detections_compact_at_the_median': lambda: compact(median),
             'pvhip_detections_to_rois': lambda: device.call('pvhip_detections_to_rois', p(x.ptr), p(table.ptr), p(table.ptr + 20 * n),
                                                             p(table.ptr + 24 * n), n, BATCH, PER_IMAGE, *EXTENT, CONF, None, 0, 1, 1)}
    e0, e1 = device.Event(), device.Event()
    us = {entry: [] for entry in calls}
    for _ in range(args.rounds):
        for entry, call in calls.items():
            for _ in range(args.warmup):
                call()
            e0.record()
            for _ in range(args.launches):
                call()
            e1.record()
            e1.synchronize()
            us[entry].append(e0.elapsed_ms(e1) * 1e3 / args.launches)
    compact(median)
    kept_at_median = int(np.asarray(header)[2 * BATCH])
    compact(CONF)
    total, selected = int(np.asarray(header)[2 * BATCH]), int(np.asarray(table)[6 * n + 1])
    live = int((np.asarray(records).reshape(BATCH, PER_IMAGE, 7)[:, :, 0] >= 0).sum())
    med = {entry: float(np.median(v)) for entry, v in us.items()}
    return {'images': BATCH, 'records_per_image': PER_IMAGE, 'min_confidence': CONF, 'live_records': live, 'rows_kept': total, 'median_score': median,
            'rows_kept_at_the_median': kept_at_median, 'rows_kept_by_the_yardstick': selected, 'same_selection': total == selected,
            'call_us': med, 'call_us_per_round': us,
            'yardstick_over_entry': med['pvhip_detections_to_rois'] / med['pvhip_detections_compact'], 'calls_per_round': args.launches,
            'device': device.device_name()}


def step_blocks(args):
    from pyopenvino_amd import device, synth
    ex, name, out_name = detector(args.requests)
    xs = [device.DeviceTensor.from_numpy(synth.uniform_pixels(9000 + r, (BATCH, 3) + EXTENT)) for r in range(args.requests)]
    feed = lambda r: {name: xs[r]}                            # noqa: E731
    median = median_live_score(ex.requests[0].infer(feed(0))[out_name])
    kinds = {'none': None, 'detections_0.5': CONF, 'detections_median': median}
    pipelined(ex, args.requests, 4 * args.requests, feed, None)            # every request records its pass
    rate, replays, handed = {kind: [] for kind in kinds}, {kind: 0 for kind in kinds}, {}
    for _ in range(args.rounds):
        for kind, detections in kinds.items():
            pipelined(ex, args.requests, args.warmup, feed, detections)
            t0 = time.perf_counter()
            n, handed[kind] = pipelined(ex, args.requests, args.steps, feed, detections)
            rate[kind].append(args.steps * BATCH / (time.perf_counter() - t0))
            replays[kind] += n
    med = {kind: float(np.median(v)) for kind, v in rate.items()}
    spread = max(rate['none']) - min(rate['none'])
    with_keyword = [kind for kind in kinds if kind != 'none']
    return {'images_per_s': med, 'images_per_s_per_block': rate, 'median_score': median,
            'detections_vs_none': {kind: med[kind] / med['none'] for kind in with_keyword}, 'spread_of_none_blocks': spread,
            'condition_holds': {kind: bool(med[kind] >= med['none'] - spread) for kind in with_keyword},
            'bytes_read_back_per_request': handed, 'replayed_passes': replays, 'timed_passes_per_kind': args.steps * args.rounds,
            'requests': args.requests, 'batch': BATCH, 'steps_per_block': args.steps, 'rounds': args.rounds}


def git_head(head):
    if head is None:
        try:
            head = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=REPO, capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    return head


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--requests', type=int, default=2)
    ap.add_argument('--steps', type=int, default=40, help='timed passes per block')
    ap.add_argument('--warmup', type=int, default=4, help='untimed passes (calls) in front of every block (round)')
    ap.add_argument('--rounds', type=int, default=5, help='blocks per kind, the kinds alternating')
    ap.add_argument('--launches', type=int, default=200, help='timed calls per round of the launch step')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--head', default=None, help='git commit to report (default: git rev-parse HEAD, when the tree is a checkout)')
    ap.add_argument('--step', choices=sorted(STEP_LIMIT), default=None, help='(the child processes) run this step here and print its JSON')
    args = ap.parse_args()
    if args.step:
        print(json.dumps({'launch': step_launch, 'blocks': step_blocks}[args.step](args)))
        return 0
    line = {'metric': 'detections: a detector\'s answer made on the device, SSD-MobileNet batch 128'}
    passed_on = [a for k in ('requests', 'steps', 'warmup', 'rounds', 'launches') for a in ('--' + k, str(getattr(args, k)))]
    for step in ('launch', 'blocks'):
        child = subprocess.run(['timeout', '-k', '10', str(STEP_LIMIT[step]), sys.executable, os.path.abspath(__file__), '--step', step] + passed_on,
                               stdout=subprocess.PIPE, text=True)
        if child.returncode != 0:
            print('bench_detections: step {} ended with status {}: nothing further is started'.format(step, child.returncode), file=sys.stderr)
            return child.returncode
        line[step] = json.loads(child.stdout.strip().splitlines()[-1])
    line.update(git_head=git_head(args.head), device=line['launch'].pop('device'), date=time.strftime('%Y-%m-%d'), profiled_with_rocprofv3=False)
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
