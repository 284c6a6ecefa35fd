"""A classifier's answer made on the device (``infer(..., top_k=k)``): what the launch costs and what the read-back saves.

GoogLeNet fp32, batch 256, `--requests` (6) whole-batch requests in flight, every request reading its own device-resident input (what
bench.py times), blocks of `--steps` pipelined passes alternating between top_k=None and top_k=5 over `--rounds` rounds of ONE process.
Two steps, each a child process under its own `timeout` (the parent never opens the device; a step that fails ends the run):

  launch   pvhip_topk_rows_f32 alone on a (256, 1000) tensor of SoftMax rows, k = 5: device time per launch by hipEvents around
           `--launches` back-to-back launches, one figure per round.
  blocks   images/s of every block, the bytes wait() handed back per request (the arrays it returned, counted), how many timed passes
           were replays, and the one condition: the median top_k=5 block is not below the median top_k=None block by more than the
           spread (max - min) between the top_k=None blocks themselves.

Prints one JSON line; --out writes it too.  e.g.  python scripts/bench_top_k.py --out profiles/top_k.json
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

BATCH, CLASSES, K = 256, 1000, 5
STEP_LIMIT = {'launch': 120, 'blocks': 480}                   # seconds each child may take


def nbytes_of(results):
    """Bytes of the host arrays a wait() returned."""
    return int(sum(sum(a.nbytes for a in v) if isinstance(v, tuple) else v.nbytes for v in results.values()))


def pipelined(ex, n_req, steps, feed, top_k):
    """`steps` passes, request r = step % n_req, each started as soon as its previous pass has been waited for:
    (replayed passes, bytes handed back by the last wait())."""
    in_flight, replays, handed = [], 0, 0
    for step in range(steps):
        r = step % n_req
        if r in in_flight:
            in_flight.remove(r)
            handed = nbytes_of(ex.wait(r))
        ex.start_async(r, feed(r), top_k=top_k)
        replays += ex.requests[r]._replayed is not None
        in_flight.append(r)
    for r in in_flight:
        handed = nbytes_of(ex.wait(r))
    return replays, handed


def step_launch(args):
    from pyopenvino_amd import device
    device.init(0)
    rng = np.random.default_rng(2026)
    logits = rng.standard_normal((BATCH, CLASSES)).astype(np.float32) * 3
    rows = np.exp(logits - logits.max(axis=1, keepdims=True))
    x = device.DeviceTensor.from_numpy((rows / rows.sum(axis=1, keepdims=True)).astype(np.float32))
    out = device.DeviceTensor.empty((2, BATCH, K), np.int32)
    launch = lambda: device.call('pvhip_topk_rows_f32', ctypes.c_void_p(x.ptr), BATCH, CLASSES, K, ctypes.c_void_p(out.ptr),  # noqa: E731
                                 ctypes.c_void_p(out.ptr + 4 * BATCH * K))
    e0, e1 = device.Event(), device.Event()
    us = []
    for _ in range(args.rounds):
        for _ in range(args.warmup):
            launch()
        e0.record()
        for _ in range(args.launches):
            launch()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_ms(e1) * 1e3 / args.launches)
    return {'rows': BATCH, 'cols': CLASSES, 'k': K, 'launch_us': float(np.median(us)), 'launch_us_per_round': us,
            'launches_per_round': args.launches, 'device': device.device_name()}


def step_blocks(args):
    from pyopenvino_amd import IECore, device, synth
    xml = os.path.join(REPO, 'models', 'googlenet-v1.xml')
    ie = IECore()
    net = ie.read_network(xml, weights=synth.synth_weights(xml, 1234))
    net.set_batch(BATCH)
    ex = ie.load_network(net, 'GPU', num_requests=args.requests)
    name = net.inputs[0]['name']
    xs = [device.DeviceTensor.from_numpy(synth.uniform_pixels(9000 + r, (BATCH, 3, 224, 224))) for r in range(args.requests)]
    feed = lambda r: {name: xs[r]}                            # noqa: E731
    kinds = {'none': None, 'top_k_5': K}
    pipelined(ex, args.requests, 4 * args.requests, feed, None)            # every request records its pass
    rate, replays, handed = {kind: [] for kind in kinds}, {kind: 0 for kind in kinds}, {}
    for _ in range(args.rounds):
        for kind, top_k in kinds.items():
            pipelined(ex, args.requests, args.warmup, feed, top_k)
            t0 = time.perf_counter()
            n, handed[kind] = pipelined(ex, args.requests, args.steps, feed, top_k)
            rate[kind].append(args.steps * BATCH / (time.perf_counter() - t0))
            replays[kind] += n
    med = {kind: float(np.median(v)) for kind, v in rate.items()}
    spread = max(rate['none']) - min(rate['none'])
    return {'images_per_s': med, 'images_per_s_per_block': rate, 'top_k_vs_none': med['top_k_5'] / med['none'],
            'spread_of_none_blocks': spread, 'condition_holds': bool(med['top_k_5'] >= med['none'] - spread),
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
    ap.add_argument('--requests', type=int, default=6)
    ap.add_argument('--steps', type=int, default=120, help='timed passes per block')
    ap.add_argument('--warmup', type=int, default=12, help='untimed passes (launches) in front of every block (round)')
    ap.add_argument('--rounds', type=int, default=5, help='blocks per kind, the kinds alternating')
    ap.add_argument('--launches', type=int, default=200, help='timed launches per round of the launch step')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--head', default=None, help='git commit to report (default: git rev-parse HEAD, when the tree is a checkout)')
    ap.add_argument('--step', choices=sorted(STEP_LIMIT), default=None, help='(the child processes) run this step here and print its JSON')
    args = ap.parse_args()
    if args.step:
        print(json.dumps({'launch': step_launch, 'blocks': step_blocks}[args.step](args)))
        return 0
    line = {'metric': 'top_k: a classifier\'s answer made on the device, GoogLeNet batch 256'}
    passed_on = [a for k in ('requests', 'steps', 'warmup', 'rounds', 'launches') for a in ('--' + k, str(getattr(args, k)))]
    for step in ('launch', 'blocks'):
        child = subprocess.run(['timeout', '-k', '10', str(STEP_LIMIT[step]), sys.executable, os.path.abspath(__file__), '--step', step] + passed_on,
                               stdout=subprocess.PIPE, text=True)
        if child.returncode != 0:
            print('bench_top_k: step {} ended with status {}: nothing further is started'.format(step, child.returncode), file=sys.stderr)
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
