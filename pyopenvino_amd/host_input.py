"""Host inputs of one request: arrays handed in a declared format (input_format.InputFormat) or in the request's own page-locked buffers
(InferRequest.input_buffer) become the fixed fp32 NCHW device tensor its pass reads -- asynchronous upload on the copy stream, one
conversion launch on the request's first stream, no host synchronisation."""
import collections
import ctypes

import numpy as np

from . import device


class _Staging:
    """One source extent of one input: the page-locked host array and the device tensor it is uploaded into (the slot's fixed tensor
    itself when nothing has to be converted).  It holds no reference back to its slot, so dropping it frees its memory at once."""
    __slots__ = ('host', 'staging', 'extent', 'preprocess')

    def __init__(self, fmt, extent, fixed):
        shape, dtype = fmt.host_shape(extent), fmt.host_dtype
        self.host = device.host_empty(shape, dtype)
        self.staging = device.DeviceTensor.empty(shape, dtype) if fmt.needs_convert(extent) else fixed
        self.extent, self.preprocess = extent, fmt.needs_preprocess(extent)


class _Slot:
    """What a request keeps for one input whatever the source extent: the fp32 NCHW tensor the pass reads -- the same address on every
    call, so the pass is recorded and replayed like a device-resident one whatever the source size --, the copy's event, mean / scale on
    the device (c floats each, uploaded once per request: load_network needs no device) and {extent: _Staging}, least recently fed first."""
    __slots__ = ('fixed', 'event', 'mean', 'std', 'extents')

    def __init__(self, fmt):
        self.fixed, self.event = device.DeviceTensor.empty(fmt.dims), device.Event(timed=False)
        self.mean, self.std = (None, None) if fmt.mean is None else (device.DeviceTensor.from_numpy(fmt.mean), device.DeviceTensor.from_numpy(fmt.std))
        self.extents = collections.OrderedDict()


class HostInputs:
    """The host-input state of one Executable_Network (one per request): `formats` = {input name: InputFormat}, fixed at load_network
    and shared by every request; `slots` = {input name: _Slot} of the inputs fed from the host so far."""
    MAX_SOURCE_EXTENTS = 4              # source extents (h, w) of a resized input whose buffers a request keeps at once

    def __init__(self, formats):
        self.formats, self.slots = formats, {}

    def release(self):
        """Drop every buffer and tensor; the page-locked memory goes back once the caller holds no view of it."""
        self.slots = {}

    def _staging(self, name, extent):
        """The staging of input `name` for sources of `extent`, made on first use."""
        fmt, slot = self.formats[name], self.slots.get(name)
        if slot is None:
            if not fmt.supported:
                raise NotImplementedError('input {}: page-locked input buffers exist for 4-D f32 Parameters only'.format(name))
            slot = self.slots[name] = _Slot(fmt)
        staged = slot.extents.get(extent)
        if staged is None:
            staged = slot.extents[extent] = _Staging(fmt, extent, slot.fixed)
        return staged

    def buffer(self, name, source_size=None) -> np.ndarray:
        """The page-locked array input `name` is uploaded from for sources of `source_size` (default: the network's extent)."""
        fmt = self.formats.get(name)
        if fmt is None:
            raise KeyError('no network input named {!r}'.format(name))
        return self._staging(name, fmt.checked_extent(source_size)).host

    def stage(self, inputs: dict, stream_base: int) -> dict:
        """`inputs` with every host input of a declared format, or in one of this request's own buffers, replaced by the request's fixed
        tensor: the caller's array is copied into the page-locked buffer of its extent unless it IS that buffer, the buffer is uploaded on
        the copy stream, stream `stream_base` waits for the copy's event and converts (one launch; none for FP32 NCHW at the network's
        extent): pvhip_input_preprocess_yuv_f32 for NV12 / I420 frames, pvhip_input_preprocess_f32 when a resize, channel reversal or
        mean / scale is in effect, else pvhip_input_to_nchw_f32.
        Every other input is returned unchanged (and goes the default way).  All but the MAX_SOURCE_EXTENTS most recently fed extents
        of an input are released here: the request has no pass in flight, so nothing reads those buffers any more."""
        out = dict(inputs)
        for name, arr in inputs.items():
            fmt = self.formats.get(name)
            if fmt is None or isinstance(arr, (device.DeviceTensor, device.ChannelSlice, device.BlockedHalf)):
                continue
            slot, staged = self.slots.get(name), None
            if slot is not None and isinstance(arr, np.ndarray):
                staged = next((s for s in slot.extents.values() if arr.shape == s.host.shape and arr.dtype == s.host.dtype
                               and arr.ctypes.data == s.host.ctypes.data), None)
            if staged is None:
                if not fmt.declared:
                    continue
                a = np.asarray(arr)
                staged = self._staging(name, fmt.extent_of(a))
                np.copyto(staged.host, a, casting='same_kind' if staged.host.dtype == np.float32 else 'safe')
            slot = self.slots[name]
            slot.extents.move_to_end(staged.extent)
            while len(slot.extents) > self.MAX_SOURCE_EXTENTS:
                slot.extents.popitem(last=False)
            host, fixed = staged.host, slot.fixed
            device.select_stream(device.COPY_STREAM)
            device.call('pvhip_memcpy_h2d_async', device.ptr(staged.staging), ctypes.c_void_p(host.ctypes.data), host.nbytes)
            slot.event.record()
            device.select_stream(stream_base)
            slot.event.wait()
            if fmt.yuv:
                device.call('pvhip_input_preprocess_yuv_f32', device.ptr(staged.staging), device.ptr(fixed), fixed.shape[0], *staged.extent,
                            *fixed.shape[2:], int(fmt.color == 'I420'), int(fmt.reverse), device.ptr(slot.mean), device.ptr(slot.std))
            elif staged.preprocess:
                device.call('pvhip_input_preprocess_f32', device.ptr(staged.staging), device.ptr(fixed), *fixed.shape[:2], *staged.extent,
                            *fixed.shape[2:], int(fmt.u8), int(fmt.nhwc), int(fmt.reverse), device.ptr(slot.mean), device.ptr(slot.std))
            elif staged.staging is not fixed:
                device.call('pvhip_input_to_nchw_f32', device.ptr(staged.staging), device.ptr(fixed), *fixed.shape, int(fmt.u8), int(fmt.nhwc))
            device.select_stream(0)
            out[name] = fixed
        return out
