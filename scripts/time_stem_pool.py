#!/usr/bin/env python3
"""GPU-box tool: the two stem launches of GoogLeNet with and without conv1's pooled second output, alternating on one box, over a sweep of
batches (BATCHES=8,16,...): conv1 alone (pvhip_conv2d_stem_direct_f32) against conv1 writing pool1's tensor too (.._direct_pool_f32), and
MaxPool + LRN + 1x1 (pvhip_maxpool_lrn_conv1x1_f32) against LRN + 1x1 on the pooled tensor (pvhip_lrn_conv1x1_f32).  The sum of each pair is
what the size rule of pvhip_conv2d_stem_direct_pool_supported is chosen from (profiles/stem_pool.md)."""
import os, sys
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pyopenvino_amd import device as dev, synth
dev.init(0)
c, h, w, k, ks, oh, ow, ph, pw = 3, 224, 224, 64, 7, 112, 112, 56, 56
ALPHA, BETA, BIAS = 9.9999997473787516e-05, 0.75, 1.0
P = dev.ptr


def timed(run, reps=20):
    for _ in range(3):
        run()
    dev.synchronize()
    e0 = dev.Event().record()
    for _ in range(reps):
        run()
    e1 = dev.Event().record(); e1.synchronize()
    return e0.elapsed_ms(e1) / reps


print('batch tiles/CU  conv1  conv1+pool  pool+lrn+1x1  lrn+1x1   sum before  sum after   rule', flush=True)
for n in (int(b) for b in os.environ.get('BATCHES', '8,16,32,64,72,80,88,96,128,192,256').split(',')):
    x = dev.DeviceTensor.from_numpy(synth.uniform_pixels(7, (n, c, h, w)))
    wt = dev.DeviceTensor.from_numpy((synth.normal(3, 4, k * c * ks * ks) * (2.0 / (c * ks * ks)) ** 0.5).astype(np.float32).reshape((k, c, ks, ks)))
    b = dev.DeviceTensor.from_numpy(synth.normal(5, 6, k).astype(np.float32).reshape((1, k, 1, 1)))
    mean = dev.DeviceTensor.from_numpy(np.array([-104.0, -117.0, -123.0], dtype=np.float32).reshape((1, 3, 1, 1)))
    w2 = dev.DeviceTensor.from_numpy((synth.normal(8, 9, k * k) * (2.0 / k) ** 0.5).astype(np.float32).reshape((k, k, 1, 1)))
    wf = dev.DeviceTensor.empty((int(dev.call('pvhip_conv2d_stem_f32_pack_elems', k)),))
    dev.call('pvhip_conv2d_stem_f32_pack', P(wt), P(wf), k)
    y, yp, z = dev.DeviceTensor.empty((n, k, oh, ow)), dev.DeviceTensor.empty((n, k, ph, pw)), dev.DeviceTensor.empty((n, k, ph, pw))
    runs = {
        'conv1': lambda: dev.call('pvhip_conv2d_stem_direct_f32', P(x), P(wf), P(y), n, h, w, k, oh, ow, P(mean), P(b), 1, 0.0, 0.0),
        'conv1+pool': lambda: dev.call('pvhip_conv2d_stem_direct_pool_f32', P(x), P(wf), P(y), P(yp), n, h, w, k, oh, ow, ph, pw, P(mean), P(b), 1, 0.0, 0.0),
        'pool+lrn+1x1': lambda: dev.call('pvhip_maxpool_lrn_conv1x1_f32', P(y), P(w2), P(z), n, k, oh, ow, ph, pw, 3, 3, 2, 2, 0, 0, 0, 0, 5, ALPHA, BETA, BIAS, k,
                                         P(b), 1, 0.0, 0.0),
        'lrn+1x1': lambda: dev.call('pvhip_lrn_conv1x1_f32', P(yp), P(w2), P(z), n, k, ph * pw, 5, ALPHA, BETA, BIAS, k, P(b), 1, 0.0, 0.0),
    }
    best = {tag: 1e9 for tag in runs}
    for rep in range(3):                       # alternating; the best of three per launch
        for tag, run in runs.items():
            best[tag] = min(best[tag], timed(run))
    rule = dev.call('pvhip_conv2d_stem_direct_pool_supported', n, c, h, w, k, ks, ks, 2, 2, 3, 3, oh, ow, ph, pw)
    print('{:5d} {:8.2f} {:6.3f} {:10.3f} {:12.3f} {:9.3f} {:11.3f} {:10.3f} {:6d}'.format(
        n, n * 28 / 256.0, best['conv1'], best['conv1+pool'], best['pool+lrn+1x1'], best['lrn+1x1'], best['conv1'] + best['pool+lrn+1x1'],
        best['conv1+pool'] + best['lrn+1x1'], rule), flush=True)
