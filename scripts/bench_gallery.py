"""Gallery matching on the device (``infer(..., matches=Gallery(...))``): what the launch pair of pvhip_gallery_match_f32 costs, against
its two bounds and against two yardsticks measured in the same run, neither of which is the code under test.

Cases: G in {1 k, 100 k, 1 M} x D in {128, 512} x n in {1, 32, 64, 256} x k in {1, 5, 64}, 'COSINE', random normal rows.  Steps, each a
child process under its own `timeout` (the parent never opens the device; a step that fails ends the run):

  ceiling  bench.py's copy ceiling of the box (a plain device-to-device copy of 822 MB), the rate the first bound is held against.
  G x D    one child per gallery: the launch pair by hipEvents around back-to-back calls (median of `--rounds` rounds), as a fraction of
           `4 G D` bytes over the copy ceiling and of `2 n G D` flops over 155 TFLOP/s; the host route as it stood before this feature
           (read the (n, D) Result back, numpy `gallery @ x.T` on the machine's threads, argpartition, sort of the k; once per (G, D, n),
           k = 5).
  torch    one child per gallery: torch.matmul + torch.topk on the same device and the same draws (rocBLAS, writes the (n, G) matrix), by
           its own events.  Where torch sees no device the child says so in its JSON, before any GPU work, and ends with status 0: the
           figure is left out.  Any other end of this child ends the run like any other step's.
  e2e      GoogLeNet batch 64 on a device-resident input, matches= a (100 k, 1000) gallery with k = 5 against the same pass with the
           full Result read back: ms per pass, median of `--rounds` blocks of `--steps` passes, the kinds alternating.

Prints one JSON line; --out writes it too.  e.g.  python scripts/bench_gallery.py --out profiles/gallery.json
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

GS, DS, NS, KS = (1000, 100000, 1000000), (128, 512), (1, 32, 64, 256), (1, 5, 64)
PEAK_F32_MATRIX_TFLOPS = 155.0
STEP_LIMIT = {'ceiling': 120, 'gallery': 420, 'torch': 240, 'e2e': 300}    # seconds each child may take


def step_ceiling(args):
    import bench
    from pyopenvino_amd import device
    device.init(0)
    return {'copy_ceiling_GBs': bench.copy_ceiling(device)['memcpy_d2d'], 'device': device.device_name()}


def _event_us(device, fn, rounds, reps, warmup=2):
    e0, e1 = device.Event(), device.Event()
    us = []
    for _ in range(rounds):
        for _ in range(warmup):
            fn()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_ms(e1) * 1e3 / reps)
    return float(np.median(us)), [min(us), max(us)]


def step_gallery(args):
    from pyopenvino_amd import Gallery, device, gallery
    device.init(0)
    G, D = args.G, args.D
    rng = np.random.default_rng(G + D)
    rows = rng.standard_normal((G, D), dtype=np.float32)
    t0 = time.perf_counter()
    gal = Gallery(rows)
    made_s = time.perf_counter() - t0
    packed = gal.on_device()
    host_rows = gal.rows                                          # what the host route multiplies with: the normalised rows
    cases = []
    for n in NS:
        x = rng.standard_normal((n, D), dtype=np.float32)
        xd = device.DeviceTensor.from_numpy(x)
        # the host route: read back, normalise the queries, matmul, argpartition, sort the k
        def host(k=5):
            q = np.asarray(xd)
            q = q / np.sqrt((q.astype(np.float64) ** 2).sum(1))[:, None].astype(np.float32)
            s = host_rows @ q.T                                   # (G, n)
            part = np.argpartition(-s, k - 1, axis=0)[:k] if k < G else np.argsort(-s, axis=0)[:k]
            top = np.take_along_axis(s, part, 0)
            order = np.argsort(-top, axis=0)
            return np.take_along_axis(part, order, 0), np.take_along_axis(top, order, 0)
        host()
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            host()
            times.append((time.perf_counter() - t0) * 1e6)
        host_us = float(np.median(times))
        for k in KS:
            out = device.DeviceTensor.empty((n + 2 * n * k,), np.int32)
            scratch = device.DeviceTensor.empty((gallery.scratch_bytes(n, G, k) // 8,), np.int64)
            at = out.ptr
            launch = lambda: device.call('pvhip_gallery_match_f32', ctypes.c_void_p(xd.ptr), n, D, ctypes.c_void_p(packed.ptr), G, k, 0, 0, 0.0,  # noqa: E731
                                         ctypes.c_void_p(scratch.ptr), ctypes.c_void_p(at), ctypes.c_void_p(at + 4 * n),
                                         ctypes.c_void_p(at + 4 * n + 4 * n * k), ctypes.c_void_p(0))
            work = 2.0 * n * G * D
            reps = int(min(200, max(3, 2e11 / work)))
            us, spread = _event_us(device, launch, args.rounds, reps)
            case = {'G': G, 'D': D, 'n': n, 'k': k, 'launch_pair_us': us, 'launch_pair_us_min_max': spread, 'launches_per_round': reps,
                    'bytes_bound_us': None, 'flops_bound_us': work / (PEAK_F32_MATRIX_TFLOPS * 1e12) * 1e6, 'host_route_us_k5': host_us}
            if args.copy_gbs:
                case['bytes_bound_us'] = 4.0 * G * D / (args.copy_gbs * 1e9) * 1e6
                case['fraction_of_bytes_bound'] = case['bytes_bound_us'] / us
            case['fraction_of_flops_bound'] = case['flops_bound_us'] / us
            cases.append(case)
    return {'cases': cases, 'gallery_made_on_host_s': made_s}


def step_torch(args):
    """torch.matmul + torch.topk on the same rows and queries (the same draws), in a process of its own that opens the device through
    torch alone."""
    import torch
    if not torch.cuda.is_available():                             # asked before any GPU work: a yardstick this box cannot give
        return {'torch': None, 'no_device': 'torch sees no device on this box'}
    G, D = args.G, args.D
    rng = np.random.default_rng(G + D)
    rows = rng.standard_normal((G, D), dtype=np.float32)
    tg = torch.from_numpy(rows).cuda()
    tg = tg / tg.norm(dim=1, keepdim=True)
    out = []
    for n in NS:
        tx = torch.from_numpy(rng.standard_normal((n, D), dtype=np.float32)).cuda()
        tx = tx / tx.norm(dim=1, keepdim=True)
        reps = int(min(200, max(3, 2e11 / (2.0 * n * G * D))))
        for k in KS:
            on_torch = lambda: torch.topk(torch.matmul(tx, tg.T), k, dim=1)     # noqa: E731
            for _ in range(2):
                on_torch()
            torch.cuda.synchronize()
            us = []
            for _ in range(args.rounds):
                s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s0.record()
                for _ in range(reps):
                    on_torch()
                s1.record()
                s1.synchronize()
                us.append(s0.elapsed_time(s1) * 1e3 / reps)
            out.append({'n': n, 'k': k, 'torch_matmul_topk_us': float(np.median(us))})
    return {'torch': out}


def step_e2e(args):
    from pyopenvino_amd import Gallery, GalleryMatch, IECore, device, synth
    xml = os.path.join(REPO, 'models', 'googlenet-v1.xml')
    ie = IECore()
    net = ie.read_network(xml, weights=synth.synth_weights(xml, 1234))
    net.set_batch(64)
    ex = ie.load_network(net, 'GPU', num_requests=1)
    name = net.inputs[0]['name']
    xd = device.DeviceTensor.from_numpy(synth.uniform_pixels(9000, (64, 3, 224, 224)))
    gal = Gallery(np.random.default_rng(5).standard_normal((100000, 1000), dtype=np.float32))
    kinds = {'whole_result': None, 'matches_k5': GalleryMatch(gal, 5)}
    req = ex.requests[0]
    for kind in list(kinds.values()) * 3:
        req.infer({name: xd}, matches=kind)
    ms = {kind: [] for kind in kinds}
    for _ in range(args.rounds):
        for kind, value in kinds.items():
            t0 = time.perf_counter()
            for _ in range(args.steps):
                req.infer({name: xd}, matches=value)
            ms[kind].append((time.perf_counter() - t0) * 1e3 / args.steps)
    return {'batch': 64, 'gallery': [100000, 1000], 'ms_per_pass': {kind: float(np.median(v)) for kind, v in ms.items()}, 'ms_per_pass_per_block': ms,
            'note': 'whole_result hands 256 000 bytes back and leaves the 6.4 GFLOP product and the argpartition to the host; matches_k5 hands back 2 816'}


def git_head(head):
    if head is None:
        try:
            head = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=REPO, capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    return head


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20, help='timed passes per block of the e2e step')
    ap.add_argument('--galleries', default=None, help='GxD,GxD,...: only these galleries (default: all six)')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--head', default=None, help='git commit to report (default: git rev-parse HEAD, when the tree is a checkout)')
    ap.add_argument('--step', choices=sorted(STEP_LIMIT), default=None, help='(the child processes) run this step here and print its JSON')
    ap.add_argument('--G', type=int, default=0)
    ap.add_argument('--D', type=int, default=0)
    ap.add_argument('--copy-gbs', type=float, default=0.0)
    args = ap.parse_args()
    if args.step:
        print(json.dumps({'ceiling': step_ceiling, 'gallery': step_gallery, 'torch': step_torch, 'e2e': step_e2e}[args.step](args)))
        return 0
    line = {'metric': 'matches: the k best gallery rows of an embedding Result made on the device', 'cases': []}
    common = ['--rounds', str(args.rounds), '--steps', str(args.steps)]

    def child(step, extra=()):
        done = subprocess.run(['timeout', '-k', '10', str(STEP_LIMIT[step]), sys.executable, os.path.abspath(__file__), '--step', step] + common + list(extra),
                              stdout=subprocess.PIPE, text=True)
        if done.returncode != 0:
            print('bench_gallery: step {} {} ended with status {}: nothing further is started'.format(step, list(extra), done.returncode), file=sys.stderr)
            return None
        return json.loads(done.stdout.strip().splitlines()[-1])

    ceiling = child('ceiling')
    if ceiling is None:
        return 1
    line.update(ceiling)
    wanted = [tuple(int(v) for v in pair.split('x')) for pair in args.galleries.split(',')] if args.galleries else [(G, D) for G in GS for D in DS]
    for G, D in wanted:
        got = child('gallery', ['--G', str(G), '--D', str(D), '--copy-gbs', str(ceiling['copy_ceiling_GBs'])])
        if got is None:
            return 1
        cases = got.pop('cases')
        on_torch = child('torch', ['--G', str(G), '--D', str(D)])
        if on_torch is None:                                           # a failed, killed or faulted child ends the run, the yardstick's too
            return 1
        if on_torch['torch'] is None:
            got['torch_matmul_topk'] = 'not measured: ' + on_torch['no_device']
        else:
            by = {(t['n'], t['k']): t['torch_matmul_topk_us'] for t in on_torch['torch']}
            for case in cases:
                case['torch_matmul_topk_us'] = by[(case['n'], case['k'])]
        line['cases'] += cases
        line.setdefault('galleries', []).append(dict(got, G=G, D=D))
    e2e = child('e2e')
    if e2e is None:
        return 1
    line.update(e2e=e2e, git_head=git_head(args.head), date=time.strftime('%Y-%m-%d'), profiled_with_rocprofv3=False)
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
