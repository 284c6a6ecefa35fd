"""The local maxima of heatmaps made on the device (``infer(..., maxima=...)``): what the entry costs beside the streaming floor and beside
the host route.

Four Results: (32, 80, 128, 128) (a CenterNet-style detector, one plane per class), (256, 19, 46, 46) (a CPM stage), (256, 19, 32, 57)
(a multi-person pose head) and (32, 1, 512, 512) (a localisation map).  Each twice: `sparse`, sigmoid-like maps -- a background of
0.01 .. 0.1 with a few Gaussian blobs a plane -- under min_score 0.3, and `dense`, normal noise without a min_score (a ninth of all
elements are maxima: the worst case for the key buffer, which is cut before most tiles).  One step, a child process under its own
`timeout` (the parent never opens the device):

  launch   pvhip_heatmap_maxima_f32 (its two launches; max_per_plane 32, max_per_row 100) on a device-resident tensor, device time
           per call by hipEvents around `--launches` back-to-back calls, beside pvhip_heatmap_peaks_f32 -- the streaming floor: one read
           of the tensor -- on the same tensor in the same run, the two alternating over `--rounds` rounds; both as 4 n K H W / time.
           Tensors up to 256 MiB stay in the Infinity Cache between launches, as a Result the pass has just written does.
           And the host route on the same tensor, `--host-rounds` times: the whole tensor read back (np.asarray of the device tensor)
           and maxima.peaks_of, the same rule in numpy with no maximum_filter, host-clocked; its answer must equal the entry's.
           `halo` is what the kernel's header comment says a plane's tiles read twice, as a fraction of the plane: the expectation for
           sparse maps is the keypoints launch times (1 + halo).

Prints one JSON line; --out writes it too.  e.g.  python scripts/bench_maxima.py --out profiles/maxima.json
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

SHAPES = [(32, 80, 128, 128), (256, 19, 46, 46), (256, 19, 32, 57), (32, 1, 512, 512)]
PER_PLANE, PER_ROW, MIN_SCORE = 32, 100, 0.3
TILE_WORDS, WAVE_PLANE, CHUNK, TILE_ROWS = 6144, 1024, 1022, 24    # of pvhip_maxima.hip (a workgroup's), for `halo`
STEP_LIMIT = {'launch': 540}                                  # seconds the child may take


def sparse_maps(rng, shape, blobs=6):
    """Sigmoid-like heatmaps: a background of 0.01 .. 0.1 and `blobs` Gaussian bumps of height 0.4 .. 1 a plane."""
    n, K, H, W = shape
    x = rng.uniform(0.01, 0.1, shape).astype(np.float32)
    ys, xs = np.mgrid[-4:5, -4:5]
    bump = np.exp(-(ys * ys + xs * xs) / 4.0).astype(np.float32)
    flat = x.reshape(n * K, H, W)
    for plane in flat:
        for _ in range(blobs):
            cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
            y0, y1, x0, x1 = max(0, cy - 4), min(H, cy + 5), max(0, cx - 4), min(W, cx + 5)
            part = bump[y0 - cy + 4:y1 - cy + 4, x0 - cx + 4:x1 - cx + 4] * np.float32(rng.uniform(0.4, 1.0))
            plane[y0:y1, x0:x1] = np.maximum(plane[y0:y1, x0:x1], part)
    return x


def halo(H, W):
    """The fraction of a plane launch 1 stages twice: one row above and below each tile inside the plane, one column beside a chunk."""
    if H * W <= WAVE_PLANE:
        return 0.0 if W <= 510 else 2.0 / 510
    if W <= CHUNK and (H + 2) * W <= TILE_WORDS:
        return 0.0
    cols = min(W, CHUNK)
    pitch = cols if W <= CHUNK else CHUNK + 2
    rows = min(H, TILE_WORDS // pitch - 2, max(TILE_ROWS, 3072 // pitch))
    tiles = -(-H // rows)
    return 2.0 * (tiles - 1) / H + (0.0 if W <= CHUNK else 2.0 / CHUNK)


def step_launch(args):
    from pyopenvino_amd import MaximaScreen, device, maxima
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
    for n, K, H, W in SHAPES:
        nbytes = 4 * n * K * H * W
        R = min(K * PER_PLANE, PER_ROW)
        scratch = device.DeviceTensor.empty((n, K, PER_PLANE), np.uint64)
        out = device.DeviceTensor.empty((n + 5 * n * R,), np.int32)
        peak_out = device.DeviceTensor.empty((4 * n * K,), np.int32)
        row = {'shape': [n, K, H, W], 'bytes': nbytes, 'form': device.call('pvhip_heatmap_maxima_form', H, W), 'halo': halo(H, W),
               'read_back_bytes': 4 * n + 20 * n * R}
        for kind, host, min_score in (('sparse', sparse_maps(rng, (n, K, H, W)), MIN_SCORE), ('dense', rng.standard_normal((n, K, H, W)).astype(np.float32), None)):
            x = device.DeviceTensor.from_numpy(host)
            at = out.ptr + 4 * n
            entry = lambda: device.call('pvhip_heatmap_maxima_f32', ctypes.c_void_p(x.ptr), n, K, H, W, PER_PLANE, R, 1, 1, int(min_score is not None),  # noqa: E731
                                        float(min_score or 0.0), ctypes.c_void_p(scratch.ptr), ctypes.c_void_p(out.ptr), ctypes.c_void_p(at),
                                        ctypes.c_void_p(at + 4 * n * R), ctypes.c_void_p(at + 8 * n * R), ctypes.c_void_p(at + 12 * n * R))
            peaks = lambda: device.call('pvhip_heatmap_peaks_f32', ctypes.c_void_p(x.ptr), n, K, H, W, 1, 1, 0, 0.0, ctypes.c_void_p(peak_out.ptr),  # noqa: E731
                                        ctypes.c_void_p(peak_out.ptr + 4 * n * K), ctypes.c_void_p(peak_out.ptr + 8 * n * K))
            us = timed({'maxima': entry, 'peaks': peaks})
            m_us, p_us = float(np.median(us['maxima'])), float(np.median(us['peaks']))
            words = np.asarray(out)
            host_ms = []
            for _ in range(args.host_rounds):
                t0 = time.perf_counter()
                want = maxima.peaks_of(np.asarray(x), MaximaScreen(min_score, PER_PLANE, R))
                host_ms.append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(words[:n], want.counts) and np.array_equal(words[n:n + n * R].reshape(n, R), want.channels) \
                and np.array_equal(words[n + n * R:n + 2 * n * R].reshape(n, R), want.positions) \
                and np.array_equal(words[n + 3 * n * R:].view(np.uint32), want.points.reshape(-1).view(np.uint32)), 'the entry timed here does not give the rule\'s answer'
            row[kind] = {'maxima_us': m_us, 'maxima_read_TBps': nbytes / m_us * 1e-6, 'peaks_us': p_us, 'peaks_read_TBps': nbytes / p_us * 1e-6,
                         'maxima_vs_peaks': m_us / p_us, 'expected_vs_peaks': 1.0 + row['halo'], 'host_route_ms': float(np.median(host_ms)),
                         'host_vs_maxima': float(np.median(host_ms)) * 1e3 / m_us, 'answered_per_row': float(want.counts.mean()),
                         'maxima_us_per_round': us['maxima'], 'peaks_us_per_round': us['peaks'], 'host_route_ms_per_round': host_ms}
            del x
        rows.append(row)
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
    line = {'metric': 'maxima: the local maxima of heatmaps made on the device'}
    passed_on = [a for k in ('warmup', 'rounds', 'launches', 'host_rounds') for a in ('--' + k.replace('_', '-'), str(getattr(args, k)))]
    for step in ('launch',):
        child = subprocess.run(['timeout', '-k', '10', str(STEP_LIMIT[step]), sys.executable, os.path.abspath(__file__), '--step', step] + passed_on,
                               stdout=subprocess.PIPE, text=True)
        if child.returncode != 0:
            print('bench_maxima: step {} ended with status {}: nothing further is started'.format(step, child.returncode), file=sys.stderr)
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
