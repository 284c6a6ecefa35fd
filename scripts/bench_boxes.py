"""A dense detector head decoded on the device (``infer(..., boxes=...)``): what the entry costs beside the kernel already in the tree
that makes the same walk over the same bytes, and beside the host route.

Three Results at n = 32: (32, 84, 8400) 'NCA' (a YOLOv8 export at 640 x 640), (32, 25200, 85) 'NAC' with objectness (YOLOv5) and the small
head (32, 6, 2100) 'NCA' with objectness (one class at 320 x 320).  Seeded numbers shaped like a detector's: class scores of a few
thousandths, and on about 300 anchors per image, in clusters around 30 objects, one class raised to 0.3 .. 0.95; boxes in pixels of a
640 x 640 input.  Two regimes: `realistic`, min_score 0.25 and max_candidates 1024 (a few hundred candidates per image); `worst`,
min_score 0 and max_candidates 4096, where every anchor passes, every key goes through the buffer and 4096 candidates are suppressed.
One step, a child process under its own `timeout` (the parent never opens the device):

  launch   pvhip_dense_boxes_f32 (its three launches) on a device-resident tensor, device time per call by hipEvents around `--launches`
           back-to-back calls, beside pvhip_segment_labels_f32 on a tensor of the same bytes read as (n, E, 1, A) -- the planes walk
           launch 1 makes --, the two alternating over `--rounds` rounds; both as 4 n A E / time.  Tensors up to 256 MiB stay in the
           Infinity Cache between launches, as a Result the pass has just written does; (32, 25200, 85) is 274 MB and does not.
           And the host route on the same tensor, `--host-rounds` times: the whole tensor read back (np.asarray of the device tensor)
           and boxes.decode, the same rule in numpy, host-clocked; its answer must equal the entry's.
           The time of each of the three launches is a kernel trace's (rocprofv3 --kernel-trace --stats around `--step launch`), a run of
           its own.

Prints one JSON line; --out writes it too.  e.g.  python scripts/bench_boxes.py --out profiles/boxes.json
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

HEADS = [((32, 84, 8400), 'NCA', False, 640), ((32, 25200, 85), 'NAC', True, 640), ((32, 6, 2100), 'NCA', True, 320)]
REGIMES = {'realistic': dict(min_score=0.25, max_candidates=1024), 'worst': dict(min_score=0.0, max_candidates=4096)}
STEP_LIMIT = {'launch': 900}                                  # seconds the child may take


def head(rng, n, A, C, objectness, extent):
    """(n, A, E) numbers shaped like a detector's."""
    v = np.empty((n, A, 4 + int(objectness) + C), np.float32)
    objects = rng.random((n, 30, 2)) * extent
    sizes = 20 + rng.random((n, 30, 2)) * 180
    v[:, :, 0:2] = rng.random((n, A, 2)) * extent
    v[:, :, 2:4] = 10 + rng.random((n, A, 2)) * 100
    first = 4 + int(objectness)
    v[:, :, first:] = rng.random((n, A, C)) * 0.01
    if objectness:
        v[:, :, 4] = 0.01 + rng.random((n, A)) * 0.05
    for r in range(n):
        at = rng.permutation(A)[:min(300, A // 4)]
        which = rng.integers(0, 30, len(at))
        v[r, at, 0:2] = objects[r, which] + rng.normal(0, 4, (len(at), 2))
        v[r, at, 2:4] = sizes[r, which] * (1 + rng.normal(0, 0.05, (len(at), 2)))
        v[r, at, first + (which % C)] = 0.3 + rng.random(len(at)) * 0.65
        if objectness:
            v[r, at, 4] = 0.9 + rng.random(len(at)) * 0.1
    return v


def step_launch(args):
    from pyopenvino_amd import BoxScreen, boxes, device
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
    for shape, layout, objectness, extent in HEADS:
        _, n, A, C = boxes.shape_of(shape, layout, objectness)
        E = 4 + int(objectness) + C
        nbytes = 4 * n * A * E
        v = head(rng, n, A, C, objectness, extent)
        host = np.ascontiguousarray(v.transpose(0, 2, 1)) if layout == 'NCA' else v
        x = device.DeviceTensor.from_numpy(host)
        planes = (n, E, 1, A)                                   # the same bytes as a stack of E planes
        seg_out = device.DeviceTensor.empty(((n * A + 3) // 4 + 5 * n * E,), np.int32)
        seg_labels = seg_out.ptr + 20 * n * E
        beside = lambda: device.call('pvhip_segment_labels_f32', ctypes.c_void_p(x.ptr), planes[0], planes[1], planes[2], planes[3], 0, 0.0,  # noqa: E731
                                     ctypes.c_void_p(seg_labels), ctypes.c_void_p(seg_out.ptr), ctypes.c_void_p(seg_out.ptr + 4 * n * E))
        for regime, fields in REGIMES.items():
            screen = boxes.resolved(BoxScreen(layout=layout, objectness=objectness, **fields))
            blocks = boxes.Blocks(n, A, screen)
            launch_with = (screen.min_score, (extent, extent), (0, 0, extent, extent))
            entry = lambda: blocks.launch(x, *launch_with)      # noqa: E731
            us = timed({'boxes': entry, 'beside': beside})
            b_us, s_us = float(np.median(us['boxes'])), float(np.median(us['beside']))
            got = blocks.read_back()
            host_ms = []
            for _ in range(args.host_rounds):
                t0 = time.perf_counter()
                want = boxes.decode(np.asarray(x), screen, (extent, extent))
                host_ms.append((time.perf_counter() - t0) * 1e3)
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want)), 'the entry timed here does not give the rule\'s answer'
            spread = lambda t: (max(t) - min(t)) / float(np.median(t))                   # noqa: E731
            rows.append({'shape': list(shape), 'layout': layout, 'objectness': objectness, 'regime': regime, 'bytes': nbytes,
                         'form': device.call('pvhip_dense_boxes_form', boxes.LAYOUTS[layout], A, E), 'min_score': screen.min_score,
                         'max_candidates': screen.max_candidates, 'selected_per_image': float(want.selected.mean()), 'rows_per_image': float(want.counts.mean()),
                         'read_back_bytes': 4 * (2 * n + 1) + 32 * int(want.counts.sum()), 'boxes_us': b_us, 'boxes_read_TBps': nbytes / b_us * 1e-6,
                         'beside': 'pvhip_segment_labels_f32', 'beside_us': s_us, 'beside_read_TBps': nbytes / s_us * 1e-6, 'boxes_vs_beside': b_us / s_us,
                         'boxes_spread': spread(us['boxes']), 'beside_spread': spread(us['beside']), 'host_route_ms': float(np.median(host_ms)),
                         'host_vs_boxes': float(np.median(host_ms)) * 1e3 / b_us, 'boxes_us_per_round': us['boxes'], 'beside_us_per_round': us['beside'],
                         'host_route_ms_per_round': host_ms})
            del blocks
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
    ap.add_argument('--warmup', type=int, default=3, help='untimed calls in front of every round')
    ap.add_argument('--rounds', type=int, default=5, help='rounds per kind, the kinds alternating')
    ap.add_argument('--launches', type=int, default=20, help='timed calls per round')
    ap.add_argument('--host-rounds', type=int, default=1, help='times the host route runs per tensor and regime')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--head', default=None, help='git commit to report (default: git rev-parse HEAD, when the tree is a checkout)')
    ap.add_argument('--step', choices=sorted(STEP_LIMIT), default=None, help='(the child process) run this step here and print its JSON')
    args = ap.parse_args()
    if args.step:
        print(json.dumps({'launch': step_launch}[args.step](args)))
        return 0
    line = {'metric': 'boxes: a dense detector head decoded on the device'}
    passed_on = [a for k in ('warmup', 'rounds', 'launches', 'host_rounds') for a in ('--' + k.replace('_', '-'), str(getattr(args, k)))]
    for step in ('launch',):
        child = subprocess.run(['timeout', '-k', '10', str(STEP_LIMIT[step]), sys.executable, os.path.abspath(__file__), '--step', step] + passed_on,
                               stdout=subprocess.PIPE, text=True)
        if child.returncode != 0:
            print('bench_boxes: step {} ended with status {}: nothing further is started'.format(step, child.returncode), file=sys.stderr)
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
