"""Host inputs of one request: arrays handed in a declared format (input_format.InputFormat) or in the request's own page-locked buffers
(InferRequest.input_buffer) become the fixed fp32 NCHW device tensor its pass reads -- asynchronous upload on the copy stream, one
conversion launch on the request's first stream, no host synchronisation."""
import collections
import ctypes

import numpy as np

from . import detections as detections_rule, device
from . import landmarks as landmark_rule
from .input_format import DetectedRois, DetectedTable, LandmarkTable, LandmarkWarps, PerspectiveInput, RoiInput, WarpInput


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
    -- a RoiInput's frames under (extent, m) --, and the (n, 5) int32 table of a RoiInput, page-locked and on the device, once one is fed.
    The device table is the head of one block `table` of 6 n + 2 ints, (n, 5) rois | (n,) record_of | (count, selected): what
    pvhip_detections_to_rois writes for a DetectedRois (`detected`: what that needs besides, once one is fed) and detected_rois() reads
    back in one copy.  `warps_host` / `warps`: the (n, 7) int64 table of a WarpInput, page-locked and on the device, once one is fed;
    `perspectives_host` / `perspectives`: the (n, 10) int64 table of a PerspectiveInput likewise.  The device warp table is the head of
    one block `warp_block` of 56 n + 4 (n + 1) bytes, (n, 7) int64 | (n,) valid | count: what pvhip_landmarks_to_warps writes for a
    LandmarkWarps (`landmarks`: what that needs besides, once one is fed) and landmark_warps() reads back in one copy.  `last`: what the
    input was last fed -- 'table' (a RoiInput or a DetectedRois: `rois` holds that pass's regions), 'images' (whole images), 'warp' (a
    WarpInput, a PerspectiveInput or a LandmarkWarps: no rectangle per row) or None (anything else): what a LandmarkWarps over this
    network's Result normalises its points to.  `table_readers`: events behind the launches of OTHER requests that read `rois` on the
    device (a LandmarkWarps fed from this request); stage() waits for them before anything overwrites the table."""
    __slots__ = ('fixed', 'event', 'mean', 'std', 'extents', 'rois_host', 'rois', 'table', 'detected', 'fed', 'warps_host', 'warps',
                 'perspectives_host', 'perspectives', 'warp_block', 'landmarks', 'last', 'table_readers')

    def __init__(self, fmt):
        self.fixed, self.event = device.DeviceTensor.empty(fmt.dims), device.Event(timed=False)
        self.mean, self.std = (None, None) if fmt.mean is None else (device.DeviceTensor.from_numpy(fmt.mean), device.DeviceTensor.from_numpy(fmt.std))
        self.extents = collections.OrderedDict()
        self.rois_host = self.rois = self.table = self.detected = self.warps_host = self.warps = None
        self.perspectives_host = self.perspectives = self.warp_block = self.landmarks = None
        self.last, self.table_readers = None, []
        self.fed = None                         # the extent of the whole images the last pass was staged from (what a declared fit fitted)

    def roi_table(self):
        if self.rois_host is None:
            n = self.fixed.shape[0]
            self.rois_host = device.host_empty((n, 5), np.int32)
            self.table = device.DeviceTensor.empty((6 * n + 2,), np.int32)
            self.rois = device.DeviceTensor(self.table._block, (n, 5), np.int32)
        return self.rois_host

    def warp_table(self):
        if self.warps_host is None:
            n = self.fixed.shape[0]
            self.warps_host = device.host_empty((n, 7), np.int64)
            self.warp_block = device.DeviceTensor.empty((56 * n + 4 * (n + 1),), np.uint8)
            self.warps = device.DeviceTensor(self.warp_block._block, (n, 7), np.int64)
        return self.warps_host

    def perspective_table(self):
        if self.perspectives_host is None:
            n = self.fixed.shape[0]
            self.perspectives_host = device.host_empty((n, 10), np.int64)
            self.perspectives = device.DeviceTensor.empty((n, 10), np.int64)
        return self.perspectives_host


class _Detected:
    """What a slot keeps for DetectedRois inputs: the labels, page-locked and on the device; the records of a host array, page-locked and
    on the device, for the record count last fed; the event recorded behind the launch that reads a detector's Result (the detector's
    next pass waits for it); `source`: the device tensor the last launch read, kept alive until the next pass of this input; `live`: the
    last pass of the input was a DetectedRois."""
    __slots__ = ('labels_host', 'labels', 'records_host', 'records', 'read', 'source', 'live')

    def __init__(self):
        self.labels_host = device.host_empty((DetectedRois.MAX_LABELS,), np.int32)
        self.labels = device.DeviceTensor.empty(self.labels_host.shape, np.int32)
        self.records_host = self.records = self.source = None
        self.read, self.live = device.Event(timed=False), False

    def records_for(self, rows):
        if self.records_host is None or self.records_host.shape[0] != rows:
            self.records_host = device.host_empty((rows, 7), np.float32)
            self.records = device.DeviceTensor.empty((rows, 7), np.float32)
        return self.records_host


class _Landmarks:
    """What a slot keeps for LandmarkWarps inputs: the packed template, page-locked and on the device, and the bytes of the one uploaded
    last (`packed`: a template is uploaded once); the points and the regions of host arrays, page-locked and on the device, for the row
    count last fed; the event recorded behind the launch that reads a landmark request's Result and region table (that request's next
    pass waits for it); `source` / `regions_source`: the device tensors the last launch read, kept alive until the next pass of this
    input; `live`: the last pass of the input was a LandmarkWarps."""
    __slots__ = ('template_host', 'template', 'packed', 'points_host', 'points', 'regions_host', 'regions', 'read', 'source',
                 'regions_source', 'live')

    def __init__(self):
        self.template_host = device.host_empty((2 * landmark_rule.MAX_POINTS + 3,), np.float64)
        self.template = device.DeviceTensor.empty(self.template_host.shape, np.float64)
        self.packed = self.points_host = self.points = self.regions_host = self.regions = self.source = self.regions_source = None
        self.read, self.live = device.Event(timed=False), False

    def points_for(self, rows, values):
        if self.points_host is None or self.points_host.shape != (rows, values):
            self.points_host = device.host_empty((rows, values), np.float32)
            self.points = device.DeviceTensor.empty((rows, values), np.float32)
        return self.points_host

    def regions_for(self, rows):
        if self.regions_host is None or self.regions_host.shape[0] != rows:
            self.regions_host = device.host_empty((rows, 5), np.int32)
            self.regions = device.DeviceTensor.empty((rows, 5), np.int32)
        return self.regions_host


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

    def warp_buffer(self, name) -> np.ndarray:
        """The page-locked (n, 7) int64 table a WarpInput of input `name` is uploaded from."""
        fmt = self._format(name)
        fmt.warp_declared()
        return self._slot(name).warp_table()

    def perspective_buffer(self, name) -> np.ndarray:
        """The page-locked (n, 10) int64 table a PerspectiveInput of input `name` is uploaded from."""
        fmt = self._format(name)
        fmt.perspective_declared()
        return self._slot(name).perspective_table()

    def _stage_warps(self, name, fmt, warp):
        """The frames and the table of WarpInput or PerspectiveInput `warp` in this request's page-locked buffers -- copied, unless
        they are those buffers --, everything checked before anything is allocated: the staging."""
        slot, given = self.slots.get(name), warp.matrices
        if isinstance(warp, PerspectiveInput):
            declared, checked, checked_table = fmt.perspective_declared, fmt.checked_perspectives, fmt.checked_perspective_table
            buffer, table_of, host = 'perspective', _Slot.perspective_table, slot.perspectives_host if slot is not None else None
        else:
            declared, checked, checked_table = fmt.warp_declared, fmt.checked_warps, fmt.checked_warp_table
            buffer, table_of, host = 'warp', _Slot.warp_table, slot.warps_host if slot is not None else None
        declared()
        frames = warp.frames if isinstance(warp.frames, np.ndarray) else np.asarray(warp.frames)
        extent, m = fmt.frames_extent_of(frames, type(warp).__name__)
        own = (host is not None and isinstance(given, np.ndarray) and given.dtype == np.int64
               and given.shape == host.shape and given.flags.c_contiguous and given.ctypes.data == host.ctypes.data)
        if own:
            if warp.ids is not None:
                raise ValueError('input {}: the {}_buffer holds the frame of each row in its first column: ids is None with it'.format(name, buffer))
            checked_table(given, m)
        else:
            table = checked(given, warp.ids, m)
        staged = self._staging(name, extent, m)
        if not (frames.dtype == staged.host.dtype and frames.flags.c_contiguous and frames.ctypes.data == staged.host.ctypes.data):
            np.copyto(staged.host, frames, casting='same_kind' if staged.host.dtype == np.float32 else 'safe')
        if not own:
            np.copyto(table_of(self.slots[name]), table)
        return staged

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

    @staticmethod
    def _detections_of(name, det):
        """What DetectedRois `det` reads, nothing waited for and nothing copied: (records -- a DeviceTensor or a host array --, the images
        they belong to by default or None, the runner whose pass produces them and the event behind that pass, or (None, None), the geometry
        of the detector's fitted input or None)."""
        src = det.detections
        if not (hasattr(src, 'runner') and hasattr(src, 'start_async')):         # (an InferRequest: inference_engine imports this module)
            return (src if isinstance(src, device.DeviceTensor) else np.asarray(src)), None, None, None, None
        runner = src.runner
        net = runner.ienet
        results = net.find_node_by_type('Result')
        if det.output is not None:
            results = [r for r in results if r[1] == det.output]
            if not results:
                raise ValueError('input {}: the detector has no Result named {!r}'.format(name, det.output))
        elif len(results) != 1:
            raise ValueError('input {}: the detector has {} Results: output= names the DetectionOutput one'.format(name, len(results)))
        nid = results[0][0]
        if [net.G.nodes[p]['type'] for p in net.G.pred[nid]] != ['DetectionOutput']:
            raise ValueError('input {}: Result {!r} of the detector is no DetectionOutput'.format(name, results[0][1]))
        replayed, pending = (src._replayed, runner._pending) if src._in_flight else (None, None)
        value = replayed['results'][results[0][1]] if replayed is not None else net.G.nodes[nid].get('result')
        if value is None:
            raise RuntimeError('input {}: the detector request never ran: start_async() or infer() it first'.format(name))
        fit = runner.host_inputs.detector_fit()
        if not isinstance(value, device.DeviceTensor):        # waited for: its host Results, like an array
            return np.asarray(value), net.batch_size, None, None, fit
        return value, net.batch_size, runner, (pending[1] if pending is not None else None), fit

    def detector_fit(self):
        """(Hn, Wn, dx, dy, iw, ih) of the pass this network was last fed, when its single 4-D Parameter declares a fit and was staged
        from whole images; else None: what a DetectedRois over this network's records maps their corners back with."""
        names = [name for name, fmt in self.formats.items() if len(fmt.dims) == 4]
        if len(names) != 1 or not self.formats[names[0]].fitted:
            return None
        fmt, slot = self.formats[names[0]], self.slots.get(names[0])
        if slot is None or slot.fed is None:
            return None
        return (int(fmt.dims[2]), int(fmt.dims[3])) + tuple(fmt.fit_geometry(slot.fed))

    def _stage_detected(self, name, fmt, det, sharded):
        """The frames of DetectedRois `det` in this request's page-locked buffers, its records (a host array: in the slot's page-locked
        buffer) and its options, everything checked before anything is allocated: (staging, [(device tensor, page-locked array)] to
        upload beside the frames, launch), launch() being what `stage` issues on the base stream in front of the ROI launch."""
        if sharded:
            raise NotImplementedError('input {}: DetectedRois with a batch sharded over ranks'.format(name))
        frames = det.frames if isinstance(det.frames, np.ndarray) else np.asarray(det.frames)
        extent, m = fmt.frames_extent_of(frames)
        conf, labels, (min_h, min_w) = det.checked_options(name)
        records, images, runner, done, fit = self._detections_of(name, det)
        if det.detector_fit is not None:
            fit = detections_rule.checked_fit(det.detector_fit, 'input {}: detector_fit'.format(name))
        images = det.images if det.images is not None else (images if images is not None else m)
        per_image = det.checked_records(name, records.shape, records.dtype, images, m)
        staged = self._staging(name, extent, m)
        if not (frames.dtype == staged.host.dtype and frames.flags.c_contiguous and frames.ctypes.data == staged.host.ctypes.data):
            np.copyto(staged.host, frames, casting='same_kind' if staged.host.dtype == np.float32 else 'safe')
        slot = self.slots[name]
        slot.roi_table()
        if slot.detected is None:
            slot.detected = _Detected()
        d = slot.detected
        uploads = []
        if labels is not None and len(labels):
            d.labels_host[:len(labels)] = labels
            uploads.append((d.labels, d.labels_host))
        listed = device.ptr(d.labels if labels is not None else None)       # NULL: any label
        if isinstance(records, device.DeviceTensor):
            d.source = records
        else:
            np.copyto(d.records_for(images * per_image), records.reshape(-1, 7))
            d.source = d.records
            uploads.append((d.records, d.records_host))
        n = slot.fixed.shape[0]

        def launch():
            if done is not None:
                done.wait()                                   # the detector's pass, on the device
            device.call('pvhip_detections_to_rois' + ('_fit' if fit is not None else ''), device.ptr(d.source), ctypes.c_void_p(slot.table.ptr),
                        ctypes.c_void_p(slot.table.ptr + 20 * n), ctypes.c_void_p(slot.table.ptr + 24 * n), n, images, per_image, *extent,
                        conf, listed, 0 if labels is None else len(labels), min_h, min_w, *(fit or ()))
            if runner is not None:                            # its next pass may overwrite that Result: not before this launch has read it
                runner._result_readers.append(d.read.record())

        return staged, uploads, launch

    def detected_rois(self, name, stream_base) -> DetectedTable:
        """The table the last pass of input `name` used, read back in one copy on stream `stream_base`, which has drained."""
        self._format(name)
        slot = self.slots.get(name)
        if slot is None or slot.detected is None or not slot.detected.live:
            raise RuntimeError('input {}: its last pass was not fed a DetectedRois'.format(name))
        n = slot.fixed.shape[0]
        device.select_stream(stream_base)
        t = np.asarray(slot.table)
        device.select_stream(0)
        return DetectedTable(int(t[6 * n]), int(t[6 * n + 1]), t[:5 * n].reshape(n, 5).copy(), t[5 * n:6 * n].copy())

    @staticmethod
    def _landmarks_of(name, lw):
        """What LandmarkWarps `lw` reads, nothing waited for and nothing copied: (points -- a DeviceTensor or a host array --, the runner
        whose pass produces them and the event behind that pass, or (None, None), the _Slot whose `rois` that pass was fed or None: the
        whole frame)."""
        src = lw.landmarks
        if not (hasattr(src, 'runner') and hasattr(src, 'start_async')):         # (an InferRequest: inference_engine imports this module)
            return (src if isinstance(src, device.DeviceTensor) else np.asarray(src)), None, None, None
        runner = src.runner
        net = runner.ienet
        results = net.find_node_by_type('Result')
        if lw.output is not None:
            results = [r for r in results if r[1] == lw.output]
            if not results:
                raise ValueError('input {}: the landmark network has no Result named {!r}'.format(name, lw.output))
        elif len(results) != 1:
            raise ValueError('input {}: the landmark network has {} Results: output= names the one that holds the points'.format(name, len(results)))
        nid = results[0][0]
        fed = runner.host_inputs
        names = [k for k, f in fed.formats.items() if len(f.dims) == 4]
        owner = fed.slots.get(names[0]) if len(names) == 1 else None
        if len(names) == 1 and fed.formats[names[0]].fitted:
            raise ValueError('input {}: input {!r} of the landmark network declares resize_fit {}: its points are normalised to a fitted '
                             'rectangle, not to the region'.format(name, names[0], fed.formats[names[0]].fit))
        if owner is not None and owner.last == 'warp':
            raise ValueError('input {}: input {!r} of the landmark network was last fed a WarpInput, a PerspectiveInput or a LandmarkWarps: '
                             'its rows have no rectangle the points are normalised to'.format(name, names[0]))
        replayed, pending = (src._replayed, runner._pending) if src._in_flight else (None, None)
        value = replayed['results'][results[0][1]] if replayed is not None else net.G.nodes[nid].get('result')
        if value is None:
            raise RuntimeError('input {}: the landmark request never ran: start_async() or infer() it first'.format(name))
        owner = owner if owner is not None and owner.last == 'table' else None
        if not isinstance(value, device.DeviceTensor):        # waited for: its host Results, like an array
            return np.asarray(value), runner, None, owner
        return value, runner, (pending[1] if pending is not None else None), owner

    def _stage_landmarks(self, name, fmt, lw, sharded):
        """The frames of LandmarkWarps `lw` in this request's page-locked buffers, its template, and its points and regions when they are
        host arrays, everything checked before anything is allocated: (staging, [(device tensor, page-locked array)] to upload beside the
        frames, launch), launch() being what `stage` issues on the base stream in front of the warp launch."""
        if sharded:
            raise NotImplementedError('input {}: LandmarkWarps with a batch sharded over ranks'.format(name))
        fmt.warp_declared()
        frames = lw.frames if isinstance(lw.frames, np.ndarray) else np.asarray(lw.frames)
        extent, m = fmt.frames_extent_of(frames, 'LandmarkWarps')
        packed = lw.checked_template(name)
        k = (len(packed) - 3) // 2
        points, runner, done, owner = self._landmarks_of(name, lw)
        rows = lw.checked_points(name, points.shape, points.dtype, k)
        regions = lw.checked_regions(name, rows)
        if regions is not None:
            owner = None
        elif owner is not None and owner.rois.shape[0] != rows:
            raise ValueError('input {}: the landmark pass was fed a table of {} regions, its Result holds {} rows of points: regions names '
                             'the rectangle of each row'.format(name, owner.rois.shape[0], rows))
        elif owner is None and m != 1 and m != rows:
            raise ValueError('input {}: landmarks over whole frames read frame b for row b (m == N) or frame 0 (m == 1); with {} frames for {} '
                             'rows of points, regions names the frame and the rectangle of each row'.format(name, m, rows))
        staged = self._staging(name, extent, m)
        if not (frames.dtype == staged.host.dtype and frames.flags.c_contiguous and frames.ctypes.data == staged.host.ctypes.data):
            np.copyto(staged.host, frames, casting='same_kind' if staged.host.dtype == np.float32 else 'safe')
        slot = self.slots[name]
        slot.warp_table()
        if slot.landmarks is None:
            slot.landmarks = _Landmarks()
        lm = slot.landmarks
        uploads = []
        if lm.packed != packed.tobytes():                      # a template is uploaded once
            lm.template_host[:len(packed)] = packed
            lm.packed = packed.tobytes()
            uploads.append((lm.template, lm.template_host))
        if isinstance(points, device.DeviceTensor):
            lm.source = points
        else:
            np.copyto(lm.points_for(rows, 2 * k), points.reshape(rows, 2 * k))
            lm.source = lm.points
            uploads.append((lm.points, lm.points_host))
        if regions is not None:
            np.copyto(lm.regions_for(rows), regions)
            lm.regions_source = lm.regions
            uploads.append((lm.regions, lm.regions_host))
        else:
            lm.regions_source = owner.rois if owner is not None else None       # NULL: the whole frame
        n = slot.fixed.shape[0]

        def launch():
            if done is not None:
                done.wait()                                   # the landmark pass, on the device
            device.call('pvhip_landmarks_to_warps', device.ptr(lm.source), device.ptr(lm.regions_source), device.ptr(lm.template),
                        device.ptr(slot.warps), ctypes.c_void_p(slot.warp_block.ptr + 56 * n), n, rows, k, m, *extent)
            if (runner is not None and isinstance(points, device.DeviceTensor)) or owner is not None:
                read = lm.read.record()
                if runner is not None and isinstance(points, device.DeviceTensor):
                    runner._result_readers.append(read)       # its next pass may overwrite that Result: not before this launch has read it
                if owner is not None and read not in owner.table_readers:       # (one event per consumer slot, recorded again each pass)
                    owner.table_readers.append(read)          # nor may its next stage() overwrite that table

        return staged, uploads, launch

    def landmark_warps(self, name, stream_base) -> LandmarkTable:
        """The table the last pass of input `name` used, read back in one copy on stream `stream_base`, which has drained."""
        self._format(name)
        slot = self.slots.get(name)
        if slot is None or slot.landmarks is None or not slot.landmarks.live:
            raise RuntimeError('input {}: its last pass was not fed a LandmarkWarps'.format(name))
        n = slot.fixed.shape[0]
        device.select_stream(stream_base)
        raw = np.asarray(slot.warp_block)
        device.select_stream(0)
        valid = raw[56 * n:].view(np.int32)
        return LandmarkTable(int(valid[n]), valid[:n] != 0, raw[:56 * n].view(np.int64).reshape(n, 7).copy())

    def _find_or_copy(self, name, fmt, arr):
        """The staging host array `arr` is fed through: the one whose page-locked buffer `arr` is, else -- for a declared format -- the
        one of its extent with `arr` copied into it; None: the input goes the default way."""
        slot = self.slots.get(name)
        if slot is not None and isinstance(arr, np.ndarray):
            # (the frames buffer of a RoiInput is none of them: handed in without its table it is an array like any other)
            for s in slot.extents.values():
                if s.frames is None and arr.shape == s.host.shape and arr.dtype == s.host.dtype and arr.ctypes.data == s.host.ctypes.data:
                    return s
        if not fmt.declared:
            return None
        a = np.asarray(arr)
        staged = self._staging(name, fmt.extent_of(a))
        np.copyto(staged.host, a, casting='same_kind' if staged.host.dtype == np.float32 else 'safe')
        return staged

    @staticmethod
    def _convert(fmt, slot, staged, largest, warped=False):
        """The one launch that makes `slot.fixed` of what `staged` uploaded (none for FP32 NCHW at the network's extent):
        pvhip_input_preprocess_yuv_f32 for NV12 / I420 frames, pvhip_input_preprocess_packed_f32 for YUY2 / UYVY / BGRX / RGBX frames,
        pvhip_input_preprocess_f32 when a resize, channel reversal or mean / scale is in effect, else pvhip_input_to_nchw_f32;
        `largest` = (max_h, max_w) of a RoiInput's table: the _roi_f32 forms.  A declared fit: the _fit_f32 forms of the three, with
        the table or NULL.  `warped`: the frames of a WarpInput: pvhip_input_preprocess_warp_f32 for every format, whatever fit is
        declared; `warped` = 'perspective': those of a PerspectiveInput, pvhip_input_preprocess_perspective_f32 with the same arguments
        and the (n, 10) table.  A format whose colour rule is not BT.601 limited range (``InputFormat.default_rule``) takes the _color_f32 form of
        its launch, whichever of these it is, with the rule behind the same arguments; every other format exactly the entries above."""
        fixed = slot.fixed
        src, dst = device.ptr(staged.staging), device.ptr(fixed)
        n, c, dst_hw = fixed.shape[0], fixed.shape[1], fixed.shape[2:]
        how = (int(fmt.color == 'I420'),) if fmt.yuv else (fmt.packed_kind,) if fmt.packed else (int(fmt.u8), int(fmt.nhwc))
        pre = (int(fmt.reverse), device.ptr(slot.mean), device.ptr(slot.std))
        if warped:
            form = (1, how[0]) if fmt.yuv else (2, how[0]) if fmt.packed else (0, how[0] | how[1] << 1)
            family, table = ('perspective', slot.perspectives) if warped == 'perspective' else ('warp', slot.warps)
            entry, rule = (family + '_f32', ()) if fmt.default_rule else (family + '_color_f32', fmt.color_rule)
            device.call('pvhip_input_preprocess_' + entry, src, dst, device.ptr(table), n, staged.frames, c, *staged.extent, *dst_hw, *form,
                        *pre, fmt.pad, *rule)
        elif not fmt.default_rule:
            # (load_network admits another rule for YUV formats only) one entry per family: the table or NULL, the fit or 0
            roi = largest is not None
            device.call('pvhip_input_preprocess_yuv_color_f32' if fmt.yuv else 'pvhip_input_preprocess_packed_color_f32', src, dst,
                        device.ptr(slot.rois if roi else None), n, staged.frames if roi else n, *staged.extent, *dst_hw,
                        *(largest if roi else staged.extent), *how, *pre, fmt.fit_code, fmt.pad, *fmt.color_rule)
        elif fmt.fitted and (largest is not None or fmt.yuv or fmt.packed or staged.preprocess):
            where = (src, dst, device.ptr(slot.rois if largest is not None else None), n, staged.frames if largest is not None else n)
            sizes = (*staged.extent, *dst_hw, *(largest if largest is not None else staged.extent))
            tail = (*how, *pre, fmt.fit_code, fmt.pad)
            if fmt.yuv:
                device.call('pvhip_input_preprocess_yuv_fit_f32', *where, *sizes, *tail)
            elif fmt.packed:
                device.call('pvhip_input_preprocess_packed_fit_f32', *where, *sizes, *tail)
            else:
                device.call('pvhip_input_preprocess_fit_f32', *where, c, *sizes, *tail)
        elif largest is not None:
            where = (src, dst, device.ptr(slot.rois), n, staged.frames)
            if fmt.yuv:
                device.call('pvhip_input_preprocess_yuv_roi_f32', *where, *staged.extent, *dst_hw, *largest, *how, *pre)
            elif fmt.packed:
                device.call('pvhip_input_preprocess_packed_roi_f32', *where, *staged.extent, *dst_hw, *largest, *how, *pre)
            else:
                device.call('pvhip_input_preprocess_roi_f32', *where, c, *staged.extent, *dst_hw, *largest, *how, *pre)
        elif fmt.yuv:
            device.call('pvhip_input_preprocess_yuv_f32', src, dst, n, *staged.extent, *dst_hw, *how, *pre)
        elif fmt.packed:
            device.call('pvhip_input_preprocess_packed_f32', src, dst, n, *staged.extent, *dst_hw, *how, *pre)
        elif staged.preprocess:
            device.call('pvhip_input_preprocess_f32', src, dst, n, c, *staged.extent, *dst_hw, *how, *pre)
        elif staged.staging is not fixed:
            device.call('pvhip_input_to_nchw_f32', src, dst, *fixed.shape, *how)

    def stage(self, inputs: dict, stream_base: int, sharded: bool = False) -> dict:
        """`inputs` with every host input of a declared format, or in one of this request's own buffers, replaced by the request's fixed
        tensor: the caller's array is copied into the page-locked buffer of its extent unless it IS that buffer, the buffer is uploaded on
        the copy stream, stream `stream_base` waits for the copy's event and converts (_convert: one launch at the most).  A RoiInput's
        frames and table go the same way, both uploaded on the copy stream behind the one event, and so do a WarpInput's and a PerspectiveInput's.  A DetectedRois' frames too -- with its
        labels, and its records when they are a host array --; its table is made by pvhip_detections_to_rois on `stream_base`, behind the
        detector's pass when the records are the Result of a request in flight, and the ROI launch is sized for whole frames: the host
        never sees the table (`sharded`: the batch is sharded over ranks, which a DetectedRois refuses).  A LandmarkWarps' frames likewise
        -- with its template, once, and its points and regions when they are host arrays --; its table is fitted by
        pvhip_landmarks_to_warps on `stream_base`, behind the landmark pass when the points are the Result of a request in flight, and the
        warp launch reads it unchanged.  That launch may read ANOTHER request's region table: it leaves an event in that slot's
        `table_readers`, and the copy stream and `stream_base` wait for those before this call uploads or makes a table for the slot.
        Every other input is returned unchanged (and goes the default way).  All but the MAX_SOURCE_EXTENTS most recently fed extents
        of an input are released here: the request has no pass in flight, so nothing reads those buffers any more."""
        out = dict(inputs)
        for name, arr in inputs.items():
            fmt, largest, uploads, make_table, make_warps = self.formats.get(name), None, (), None, None
            warped = 'perspective' if isinstance(arr, PerspectiveInput) else isinstance(arr, WarpInput)
            if warped:
                staged = self._stage_warps(name, self._format(name), arr)
                slot = self.slots[name]
                uploads = ((slot.perspectives, slot.perspectives_host) if warped == 'perspective' else (slot.warps, slot.warps_host),)
            elif isinstance(arr, RoiInput):
                staged, largest = self._stage_rois(name, self._format(name), arr)
                uploads = ((self.slots[name].rois, self.slots[name].rois_host),)
            elif isinstance(arr, DetectedRois):
                staged, uploads, make_table = self._stage_detected(name, self._format(name), arr, sharded)
                largest = staged.extent                       # the host does not know the largest rectangle: the frame bounds it
            elif isinstance(arr, LandmarkWarps):
                staged, uploads, make_warps = self._stage_landmarks(name, self._format(name), arr, sharded)
                warped = True
            elif fmt is None or isinstance(arr, (device.DeviceTensor, device.ChannelSlice, device.BlockedHalf)):
                if name in self.slots:
                    self.slots[name].fed = self.slots[name].last = None
                continue
            else:
                staged = self._find_or_copy(name, fmt, arr)
                if staged is None:
                    if name in self.slots:
                        self.slots[name].last = None
                    continue
            slot = self.slots[name]
            slot.fed = staged.extent if largest is None and not warped else None
            slot.last = 'warp' if warped else 'table' if largest is not None else 'images'
            if slot.table_readers:                            # launches of other requests still read `rois`: nothing overwrites it before them
                readers, slot.table_readers = slot.table_readers, []
                for stream in (device.COPY_STREAM, stream_base):
                    device.select_stream(stream)
                    for event in readers:
                        event.wait()
            slot.extents.move_to_end(staged.key)
            while len(slot.extents) > self.MAX_SOURCE_EXTENTS:
                slot.extents.popitem(last=False)
            device.select_stream(device.COPY_STREAM)
            device.call('pvhip_memcpy_h2d_async', device.ptr(staged.staging), ctypes.c_void_p(staged.host.ctypes.data), staged.host.nbytes)
            for dst, host in uploads:
                device.call('pvhip_memcpy_h2d_async', device.ptr(dst), ctypes.c_void_p(host.ctypes.data), host.nbytes)
            slot.event.record()
            device.select_stream(stream_base)
            slot.event.wait()
            if slot.detected is not None:
                slot.detected.live = make_table is not None
                if make_table is None:
                    slot.detected.source = None
            if slot.landmarks is not None:
                slot.landmarks.live = make_warps is not None
                if make_warps is None:
                    slot.landmarks.source = slot.landmarks.regions_source = None
            if make_table is not None:
                make_table()
            if make_warps is not None:
                make_warps()
            self._convert(fmt, slot, staged, largest, warped)
            device.select_stream(0)
            out[name] = slot.fixed
        return out
