"""Host inputs of one request: arrays handed in a declared format (input_format.InputFormat) or in the request's own page-locked buffers
(InferRequest.input_buffer) become the fixed fp32 NCHW device tensor its pass reads -- asynchronous upload on the copy stream, one
conversion launch on the request's first stream, no host synchronisation."""
import collections
import ctypes

import numpy as np

from . import device
from .input_format import RoiInput


class _Staging:
    """One source extent of one input: the page-locked host array and the device tensor it is uploaded into (the slot's fixed tensor
    itself when nothing has to be converted).  `frames` = m: the m frames of a RoiInput instead (always uploaded into a tensor of their
    own).  It holds no reference back to its slot, so dropping it frees its memory at once."""
    __slots__ = ('host', 'staging', 'extent', 'frames', 'preprocess')

    def __init__(self, fmt, extent, fixed, frames=None):
        shape, dtype = fmt.host_shape(extent, frames), fmt.host_dtype
        self.host = device.host_empty(shape, dtype)
        self.staging = device.DeviceTensor.empty(shape, dtype) if frames is not None or fmt.needs_convert(extent) else fixed
        self.extent, self.frames, self.preprocess = extent, frames, fmt.needs_preprocess(extent)

    @property
    def key(self):
        """What _Slot.extents files it under: the extent, or (extent, m) for the frames of a RoiInput."""
        return self.extent if self.frames is None else (self.extent, self.frames)


class _Slot:
    """What a request keeps for one input whatever the source extent: the fp32 NCHW tensor the pass reads -- the same address on every
    call, so the pass is recorded and replayed like a device-resident one whatever the source size --, the copy's event, mean / scale on
    the device (c floats each, uploaded once per request: load_network needs no device) and {extent: _Staging}, least recently fed first
    -- a RoiInput's frames under (extent, m) --, and the (n, 5) int32 table of a RoiInput, page-locked and on the device, once one is fed."""
    __slots__ = ('fixed', 'event', 'mean', 'std', 'extents', 'rois_host', 'rois')

    def __init__(self, fmt):
        self.fixed, self.event = device.DeviceTensor.empty(fmt.dims), device.Event(timed=False)
        self.mean, self.std = (None, None) if fmt.mean is None else (device.DeviceTensor.from_numpy(fmt.mean), device.DeviceTensor.from_numpy(fmt.std))
        self.extents = collections.OrderedDict()
        self.rois_host = self.rois = None

    def roi_table(self):
        if self.rois_host is None:
            self.rois_host = device.host_empty((self.fixed.shape[0], 5), np.int32)
            self.rois = device.DeviceTensor.empty(self.rois_host.shape, np.int32)
        return self.rois_host


class HostInputs:
    """The host-input state of one Executable_Network (one per request): `formats` = {input name: InputFormat}, fixed at load_network
    and shared by every request; `slots` = {input name: _Slot} of the inputs fed from the host so far."""
    # source extents (h, w) of a resized input -- and (extent, frame count) pairs of its RoiInputs -- whose buffers a request keeps at once
    MAX_SOURCE_EXTENTS = 4

    def __init__(self, formats):
        self.formats, self.slots = formats, {}

    def release(self):
        """Drop every buffer and tensor; the page-locked memory goes back once the caller holds no view of it."""
        self.slots = {}

    def _slot(self, name):
        fmt, slot = self.formats[name], self.slots.get(name)
        if slot is None:
            if not fmt.supported:
                raise NotImplementedError('input {}: page-locked input buffers exist for 4-D f32 Parameters only'.format(name))
            slot = self.slots[name] = _Slot(fmt)
        return slot

    def _staging(self, name, extent, frames=None):
        """The staging of input `name` for sources of `extent` (`frames` = m: for the m frames of a RoiInput), made on first use."""
        slot = self._slot(name)
        key = extent if frames is None else (extent, frames)
        staged = slot.extents.get(key)
        if staged is None:
            staged = slot.extents[key] = _Staging(self.formats[name], extent, slot.fixed, frames)
        return staged

    def _format(self, name):
        fmt = self.formats.get(name)
        if fmt is None:
            raise KeyError('no network input named {!r}'.format(name))
        return fmt

    def buffer(self, name, source_size=None, frames=None) -> np.ndarray:
        """The page-locked array input `name` is uploaded from for sources of `source_size` (default: the network's extent); `frames`
        = m: the one the m frames of a RoiInput are uploaded from."""
        fmt = self._format(name)
        if frames is not None:
            frames = fmt.checked_frames(frames)
        return self._staging(name, fmt.checked_extent(source_size), frames).host

    def roi_buffer(self, name) -> np.ndarray:
        """The page-locked (n, 5) int32 table a RoiInput of input `name` is uploaded from."""
        fmt = self._format(name)
        fmt.checked_frames(1)               # (a resize is declared)
        return self._slot(name).roi_table()

    def _stage_rois(self, name, fmt, roi):
        """The frames and the table of RoiInput `roi` in this request's page-locked buffers -- copied, unless they are those buffers --,
        everything checked before anything is allocated: (staging, (max_h, max_w))."""
        frames = roi.frames if isinstance(roi.frames, np.ndarray) else np.asarray(roi.frames)
        extent, m = fmt.frames_extent_of(frames)
        table, largest = fmt.checked_rois(roi.rois, extent, m)
        staged = self._staging(name, extent, m)
        if not (frames.dtype == staged.host.dtype and frames.flags.c_contiguous and frames.ctypes.data == staged.host.ctypes.data):
            np.copyto(staged.host, frames, casting='same_kind' if staged.host.dtype == np.float32 else 'safe')
        rois_host = self.slots[name].roi_table()
        own = (isinstance(roi.rois, np.ndarray) and roi.rois.dtype == np.int32 and roi.rois.flags.c_contiguous
               and roi.rois.ctypes.data == rois_host.ctypes.data)
        if not own:
            np.copyto(rois_host, table)
        return staged, largest

    def stage(self, inputs: dict, stream_base: int) -> dict:
        """`inputs` with every host input of a declared format, or in one of this request's own buffers, replaced by the request's fixed
        tensor: the caller's array is copied into the page-locked buffer of its extent unless it IS that buffer, the buffer is uploaded on
        the copy stream, stream `stream_base` waits for the copy's event and converts (one launch; none for FP32 NCHW at the network's
        extent): pvhip_input_preprocess_yuv_f32 for NV12 / I420 frames, pvhip_input_preprocess_f32 when a resize, channel reversal or
        mean / scale is in effect, else pvhip_input_to_nchw_f32.  A RoiInput's frames and table go the same way -- both uploaded on the
        copy stream behind the one event -- and pvhip_input_preprocess_roi_f32 / _yuv_roi_f32 writes the fixed tensor.
        Every other input is returned unchanged (and goes the default way).  All but the MAX_SOURCE_EXTENTS most recently fed extents
        of an input are released here: the request has no pass in flight, so nothing reads those buffers any more."""
        out = dict(inputs)
        for name, arr in inputs.items():
            fmt = self.formats.get(name)
            roi = isinstance(arr, RoiInput)
            if roi:
                staged, largest = self._stage_rois(name, self._format(name), arr)
            if fmt is None or isinstance(arr, (device.DeviceTensor, device.ChannelSlice, device.BlockedHalf)):
                continue
            slot = self.slots.get(name)
            staged = staged if roi else None
            if slot is not None and isinstance(arr, np.ndarray):
                # (the frames buffer of a RoiInput is none of them: handed in without its table it is an array like any other)
                staged = next((s for s in slot.extents.values() if s.frames is None and arr.shape == s.host.shape
                               and arr.dtype == s.host.dtype and arr.ctypes.data == s.host.ctypes.data), None)
            if staged is None:
                if not fmt.declared:
                    continue
                a = np.asarray(arr)
                staged = self._staging(name, fmt.extent_of(a))
                np.copyto(staged.host, a, casting='same_kind' if staged.host.dtype == np.float32 else 'safe')
            slot = self.slots[name]
            slot.extents.move_to_end(staged.key)
            while len(slot.extents) > self.MAX_SOURCE_EXTENTS:
                slot.extents.popitem(last=False)
            host, fixed = staged.host, slot.fixed
            device.select_stream(device.COPY_STREAM)
            device.call('pvhip_memcpy_h2d_async', device.ptr(staged.staging), ctypes.c_void_p(host.ctypes.data), host.nbytes)
            if roi:
                device.call('pvhip_memcpy_h2d_async', device.ptr(slot.rois), ctypes.c_void_p(slot.rois_host.ctypes.data), slot.rois_host.nbytes)
            slot.event.record()
            device.select_stream(stream_base)
            slot.event.wait()
            if roi:
                where = (device.ptr(staged.staging), device.ptr(fixed), device.ptr(slot.rois), fixed.shape[0], staged.frames)
                if fmt.yuv:
                    device.call('pvhip_input_preprocess_yuv_roi_f32', *where, *staged.extent, *fixed.shape[2:], *largest,
                                int(fmt.color == 'I420'), int(fmt.reverse), device.ptr(slot.mean), device.ptr(slot.std))
                else:
                    device.call('pvhip_input_preprocess_roi_f32', *where, fixed.shape[1], *staged.extent, *fixed.shape[2:], *largest,
                                int(fmt.u8), int(fmt.nhwc), int(fmt.reverse), device.ptr(slot.mean), device.ptr(slot.std))
            elif fmt.yuv:
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
