"""Device time of pvhip_input_to_nchw_f32 (the U8 / NHWC input conversion) at batch 256 x 224 x 224 x 3, per form, from hipEvents around
`--reps` launches; run it under `rocprofv3 --kernel-trace --stats -- python scripts/time_input_convert.py` for per-kernel statistics."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyopenvino_amd import device  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    device.init(0)
    n, c, h, w = args.batch, 3, 224, 224
    dst = device.DeviceTensor.empty((n, c, h, w))
    rows = {}
    for tag, dtype, u8, nhwc in (('u8_nhwc', np.uint8, 1, 1), ('u8_nchw', np.uint8, 1, 0), ('fp32_nhwc', np.float32, 0, 1)):
        src = device.DeviceTensor.from_numpy(np.zeros(n * c * h * w, dtype))

        def launch():
            device.call('pvhip_input_to_nchw_f32', ctypes.c_void_p(src.ptr), ctypes.c_void_p(dst.ptr), n, c, h, w, u8, nhwc)
        launch()
        e0, e1 = device.Event(), device.Event()
        e0.record()
        for _ in range(args.reps):
            launch()
        e1.record()
        e1.synchronize()
        us = e0.elapsed_ms(e1) * 1e3 / args.reps
        moved = src.nbytes + dst.nbytes
        rows[tag] = {'us': round(us, 2), 'TBs': round(moved / (us * 1e-6) / 1e12, 3), 'bytes_moved': moved}
    print(json.dumps({'batch': n, 'reps': args.reps, 'forms': rows, 'device': device.device_name()}))


if __name__ == '__main__':
    main()
