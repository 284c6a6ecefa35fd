"""The greedy CTC decoding made on the device (``infer(..., text=...)``): what the entry costs beside the kernel already in the tree that
reads the same bytes, and beside the host route.

Four Results: (30, 256, 37) 'TNC' (a Latin plate or line recogniser), (186, 32, 4442) 'TNC' (a handwritten Japanese or Chinese one),
(32, 26, 37) 'NTC' and (256, 71, 1, 88) 'NCT'.  Seeded scores: normal noise, the blank (the last class) raised on seven timesteps in
ten, so that the strings are a fraction of T as a recogniser's are.  One step, a child process under its own `timeout` (the parent
never opens the device):

  launch   pvhip_ctc_greedy_f32 (its two launches; blank -1, merge_repeated) on a device-resident tensor, device time per call by
           hipEvents around `--launches` back-to-back calls, beside the kernel that reads the same bytes in the same run, the two
           alternating over `--rounds` rounds: pvhip_topk_rows_f32 at k = 1 on the (n T, C) rows for the contiguous layouts,
           pvhip_segment_labels_f32 on (n, C, 1, T) for 'NCT'; both as 4 n T C / time.  Tensors up to 256 MiB stay in the Infinity
           Cache between launches, as a Result the pass has just written does.
           And the host route on the same tensor, `--host-rounds` times: the whole tensor read back (np.asarray of the device tensor)
           and text.greedy, the same rule in numpy, host-clocked; its answer must equal the entry's.

Prints one JSON line; --out writes it too.  e.g.  python scripts/bench_text.py --out profiles/text.json
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

SHAPES = [((30, 256, 37), 'TNC'), ((186, 32, 4442), 'TNC'), ((32, 26, 37), 'NTC'), ((256, 71, 1, 88), 'NCT')]
STEP_LIMIT = {'launch': 540}                                  # seconds the child may take


def scores(rng, shape, layout):
    """Normal noise with the last class raised by 4 on seven timesteps in ten, in the tensor's own layout."""
    x = rng.standard_normal(shape).astype(np.float32)
    flat = x.reshape([d for d in shape if d != 1] if len(shape) == 4 else shape)
    v = flat.transpose({'TNC': (1, 0, 2), 'NTC': (0, 1, 2), 'NCT': (0, 2, 1)}[layout])       # a view (n, T, C)
    v[..., -1] += np.where(rng.random(v.shape[:2]) < 0.7, np.float32(4), np.float32(0))
    return x


def step_launch(args):
    from pyopenvino_amd import TextScreen, device, text
    device.init(0)
    rng = np.random.default_rng(2026)
    e0, e1 = device.Event(), device.Event()

    def timed(launches):
        us = {kind: [] for kind in launches}
        for _ in range(args.rounds):
            for kind, launch in launches.items():
                for _ in range(args.warmup):
                    launch()
                e0.record()
                for _ in range(args.launches):
                    launch()
                e1.record()
                e1.synchronize()
                us[kind].append(e0.elapsed_ms(e1) * 1e3 / args.launches)
        return us

    rows = []
    for shape, layout in SHAPES:
        _, n, T, C = text.steps_of(shape, layout)
        nbytes = 4 * n * T * C
        host = scores(rng, shape, layout)
        x = device.DeviceTensor.from_numpy(host)
        scratch = device.DeviceTensor.empty((n, T), np.uint64)
        out = device.DeviceTensor.empty((n + 3 * n * T,), np.int32)
        at = out.ptr + 4 * n
        entry = lambda: device.call('pvhip_ctc_greedy_f32', ctypes.c_void_p(x.ptr), n, T, C, text.LAYOUTS[layout], C - 1, 1,  # noqa: E731
                                    ctypes.c_void_p(scratch.ptr), ctypes.c_void_p(out.ptr), ctypes.c_void_p(at), ctypes.c_void_p(at + 4 * n * T),
                                    ctypes.c_void_p(at + 8 * n * T))
        if layout == 'NCT':
            beside = 'pvhip_segment_labels_f32'
            other_out = device.DeviceTensor.empty(((n * T + 3) // 4 + 5 * n * C,), np.int32)
            labels = other_out.ptr + 20 * n * C
            other = lambda: device.call(beside, ctypes.c_void_p(x.ptr), n, C, 1, T, 0, 0.0, ctypes.c_void_p(labels),  # noqa: E731
                                        ctypes.c_void_p(other_out.ptr), ctypes.c_void_p(other_out.ptr + 4 * n * C))
        else:
            beside = 'pvhip_topk_rows_f32'
            other_out = device.DeviceTensor.empty((2 * n * T,), np.int32)
            other = lambda: device.call(beside, ctypes.c_void_p(x.ptr), n * T, C, 1, ctypes.c_void_p(other_out.ptr),  # noqa: E731
                                        ctypes.c_void_p(other_out.ptr + 4 * n * T))
        us = timed({'text': entry, 'beside': other})
        t_us, b_us = float(np.median(us['text'])), float(np.median(us['beside']))
        words = np.asarray(out)
        host_ms = []
        for _ in range(args.host_rounds):
            t0 = time.perf_counter()
            want = text.greedy(np.asarray(x), TextScreen(-1, True, layout))
            host_ms.append((time.perf_counter() - t0) * 1e3)
        part = lambda i: words[n + i * n * T:n + (i + 1) * n * T].reshape(n, T)      # noqa: E731
        assert np.array_equal(words[:n], want.lengths) and np.array_equal(part(0), want.symbols) and np.array_equal(part(2), want.steps) \
            and np.array_equal(part(1).view(np.uint32), want.scores.view(np.uint32)), 'the entry timed here does not give the rule\'s answer'
        spread = lambda v: (max(v) - min(v)) / float(np.median(v))                   # noqa: E731
        rows.append({'shape': list(shape), 'layout': layout, 'bytes': nbytes, 'form': device.call('pvhip_ctc_greedy_form', text.LAYOUTS[layout], T, C),
                     'read_back_bytes': 4 * n + 12 * n * T, 'text_us': t_us, 'text_read_TBps': nbytes / t_us * 1e-6, 'beside': beside, 'beside_us': b_us,
                     'beside_read_TBps': nbytes / b_us * 1e-6, 'text_vs_beside': t_us / b_us, 'text_spread': spread(us['text']),
                     'beside_spread': spread(us['beside']), 'host_route_ms': float(np.median(host_ms)), 'host_vs_text': float(np.median(host_ms)) * 1e3 / t_us,
                     'mean_length': float(want.lengths.mean()), 'text_us_per_round': us['text'], 'beside_us_per_round': us['beside'],
                     'host_route_ms_per_round': host_ms})
        del x
    return {'rows': rows, 'launches_per_round': args.launches, 'device': device.device_name()}


def git_head(head):
    if head is None:
        try:
            head = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=REPO, capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    return head


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--warmup', type=int, default=5, help='untimed calls in front of every round')
    ap.add_argument('--rounds', type=int, default=5, help='rounds per kind, the kinds alternating')
    ap.add_argument('--launches', type=int, default=50, help='timed calls per round')
    ap.add_argument('--host-rounds', type=int, default=2, help='times the host route runs per tensor')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--head', default=None, help='git commit to report (default: git rev-parse HEAD, when the tree is a checkout)')
    ap.add_argument('--step', choices=sorted(STEP_LIMIT), default=None, help='(the child process) run this step here and print its JSON')
    args = ap.parse_args()
    if args.step:
        print(json.dumps({'launch': step_launch}[args.step](args)))
        return 0
    line = {'metric': 'text: the greedy CTC decoding made on the device'}
    passed_on = [a for k in ('warmup', 'rounds', 'launches', 'host_rounds') for a in ('--' + k.replace('_', '-'), str(getattr(args, k)))]
    for step in ('launch',):
        child = subprocess.run(['timeout', '-k', '10', str(STEP_LIMIT[step]), sys.executable, os.path.abspath(__file__), '--step', step] + passed_on,
                               stdout=subprocess.PIPE, text=True)
        if child.returncode != 0:
            print('bench_text: step {} ended with status {}: nothing further is started'.format(step, child.returncode), file=sys.stderr)
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
