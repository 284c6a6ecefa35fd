"""Records tests/golden/input_conversions.json: the launch HostInputs._convert issued for every case of the matrix below, as it stood
before the launch choice moved into InputFormat.conversion -- run it on the commit "MatMul, elementwise, data-movement launchers: form
queries, row per form" (``python tests/golden/make_input_conversions.py``), where _convert still exists; tests/test_input_conversion.py
holds InputFormat.conversion to what it wrote.  No device is needed: host_input.device is swapped for a stand-in whose `call` appends
and whose `ptr` gives the operand's name, or 'NULL'.

The matrix, at batch 2, c = 3, network extent 32 x 32 (840 cases): ten formats, three fits, BT601 limited for every format and BT709
full for the four YUV ones, with and without reversal + mean / std, source extents (32, 32) and (20, 48), and five feeds -- whole
images, a RoiInput whose largest rectangle is (9, 11), a DetectedRois (the frame bounds its rectangles), a WarpInput and a
PerspectiveInput, over 3 frames each.  A case's key is its six coordinates joined by '|'; its value [entry, argument, ...], or [] for
no launch."""
import itertools
import json
import os
import sys
import types

import numpy as np

DIMS = (2, 3, 32, 32)
FRAMES = 3
LARGEST = (9, 11)
PAD = 114.0
# (name, u8, nhwc, color)
FORMATS = [('f32.nchw', False, False, 'RAW'), ('f32.nhwc', False, True, 'RAW'), ('u8.nchw', True, False, 'RAW'), ('u8.nhwc', True, True, 'RAW')] \
    + [(color, True, False, color) for color in ('NV12', 'I420', 'YUY2', 'UYVY', 'BGRX', 'RGBX')]
YUV = ('NV12', 'I420', 'YUY2', 'UYVY')
FITS = ('STRETCH', 'LETTERBOX', 'TOP_LEFT')
RULES = (('BT601', False), ('BT709', True))
EXTENTS = ((32, 32), (20, 48))
FEEDS = ('images', 'roi', 'detected', 'warp', 'perspective')
MEAN, STD = np.array([104.0, 117.0, 123.0], np.float32), np.array([1.0, 2.0, 4.0], np.float32)


def cases():
    """(key, InputFormat arguments, extent, feed) of every case."""
    for (name, u8, nhwc, color), fit, (standard, full), pre, extent, feed in itertools.product(FORMATS, FITS, RULES, (False, True), EXTENTS, FEEDS):
        if standard != 'BT601' and color not in YUV:
            continue
        key = '|'.join((name, fit, standard + ('.full' if full else ''), 'pre' if pre else 'plain', '{}x{}'.format(*extent), feed))
        fmt = dict(name='x', dims=DIMS, supported=True, declared=True, u8=u8, nhwc=nhwc, resize=True, reverse=pre, mean=MEAN if pre else None,
                   std=STD if pre else None, color=color, fit=fit, pad=PAD, standard=standard, full_range=full)
        yield key, fmt, extent, feed


def largest_of(extent, feed):
    """`largest` as stage() hands it on: a RoiInput's largest rectangle, the frame for a DetectedRois, None for every other feed."""
    return LARGEST if feed == 'roi' else extent if feed == 'detected' else None


def record():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from pyopenvino_amd import host_input
    from pyopenvino_amd.input_format import InputFormat
    calls = []
    host_input.device = types.SimpleNamespace(call=lambda entry, *args: calls.append([entry, *args]),
                                              ptr=lambda t: 'NULL' if t is None else t.name)
    named = lambda name, **more: types.SimpleNamespace(name=name, **more)
    out = {}
    for key, fields, extent, feed in cases():
        fmt = InputFormat(**fields)
        fixed = named('dst', shape=DIMS)
        table = named('table')
        slot = types.SimpleNamespace(fixed=fixed, mean=named('mean') if fmt.mean is not None else None,
                                     std=named('std') if fmt.std is not None else None, rois=table, warps=table, perspectives=table)
        frames = None if feed == 'images' else FRAMES
        staged = types.SimpleNamespace(staging=named('src') if frames is not None or fmt.needs_convert(extent) else fixed, extent=extent,
                                       frames=frames, preprocess=fmt.needs_preprocess(extent))
        del calls[:]
        host_input.HostInputs._convert(fmt, slot, staged, largest_of(extent, feed),
                                       'perspective' if feed == 'perspective' else feed == 'warp')
        assert len(calls) <= 1 and key not in out
        out[key] = calls[0] if calls else []
    return out


if __name__ == '__main__':
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'input_conversions.json')
    with open(path, 'w') as f:
        json.dump(record(), f, separators=(',', ':'), sort_keys=True)
        f.write('\n')
    print(path, os.path.getsize(path))
