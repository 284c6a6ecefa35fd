"""Host inputs of one request: arrays handed in a declared format (input_format.InputFormat) or in the request's own page-locked buffers
(InferRequest.input_buffer), and the frames of a FrameFeed with its table, become the fixed fp32 NCHW device tensor its pass reads --
asynchronous upload on the copy stream, one conversion launch on the request's first stream (InputFormat.conversion chooses it), no
host synchronisation."""
import collections
import ctypes

import numpy as np

from . import detections as detections_rule, device
from . import landmarks as landmark_rule
from .input_format import DetectedRois, DetectedTable, FrameFeed, LandmarkTable, LandmarkWarps, PerspectiveInput, RoiInput, WarpInput

NULL = ctypes.c_void_p(0)


def _is_array(a, host) -> bool:
    """`a` is the page-locked array `host` -- the object itself, or a view of all of it --: nothing has to be copied."""
    return a is host or (isinstance(a, np.ndarray) and a.dtype == host.dtype and a.shape == host.shape and a.flags.c_contiguous
                         and a.ctypes.data == host.ctypes.data)


class _Pair:
    """A page-locked array `host` and the device tensor `device` of its shape and dtype it is uploaded into.  `block`: the longer device
    block that tensor is the head of -- what a table-making launch writes behind the table and a read-back takes in one copy --, given
    as its (shape, dtype); else the tensor itself."""
    __slots__ = ('host', 'device', 'block')

    def __init__(self, shape, dtype, block=None):
        self.host = device.host_empty(shape, dtype)
        self.block = device.DeviceTensor.empty(*(block or (shape, dtype)))
        self.device = self.block if block is None else device.DeviceTensor(self.block._block, shape, dtype)

    @classmethod
    def of_shape(cls, pair, shape, dtype):
        """`pair` when it has `shape`, else a new one: what is fed with another row count every pass keeps its buffers while it can."""
        return pair if pair is not None and pair.host.shape == shape else cls(shape, dtype)

    def holds(self, a) -> bool:
        return _is_array(a, self.host)

    @property
    def upload(self):
        return self.device, self.host


# the table of a slot by FrameFeed.KIND, (columns, dtype, the block behind it for n rows or None): 'roi' (n, 5) rois | (n,) record_of |
# (count, selected), what pvhip_detections_to_rois writes for a DetectedRois; 'warp' (n, 7) int64 | (n,) valid | count, what
# pvhip_landmarks_to_warps writes for a LandmarkWarps
TABLES = {'roi': (5, np.int32, lambda n: ((6 * n + 2,), np.int32)), 'warp': (7, np.int64, lambda n: ((56 * n + 4 * (n + 1),), np.uint8)),
          'perspective': (10, np.int64, None)}


class _Staging:
    """One source extent of one input: the page-locked host array and the device tensor it is uploaded into (the slot's fixed tensor
    itself when nothing has to be converted).  `frames` = m: the m frames of a FrameFeed instead (always uploaded into a tensor of their
    own).  It holds no reference back to its slot, so dropping it frees its memory at once."""
    __slots__ = ('host', 'staging', 'extent', 'frames')

    def __init__(self, fmt, extent, fixed, frames=None):
        shape, dtype = fmt.host_shape(extent, frames), fmt.host_dtype
        self.host = device.host_empty(shape, dtype)
        self.staging = device.DeviceTensor.empty(shape, dtype) if frames is not None or fmt.needs_convert(extent) else fixed
        self.extent, self.frames = extent, frames

    @property
    def key(self):
        """What _Slot.extents files it under: the extent, or (extent, m) for the frames of a FrameFeed."""
        return self.extent if self.frames is None else (self.extent, self.frames)

    def copy_in(self, a):
        """The caller's images or frames `a`, checked, in the page-locked array -- copied unless they are that array."""
        if not _is_array(a, self.host):
            np.copyto(self.host, a, casting='same_kind' if self.host.dtype == np.float32 else 'safe')
        return self


class _Slot:
    """What a request keeps for one input whatever the source extent: the fp32 NCHW tensor the pass reads -- the same address on every
    call, so the pass is recorded and replayed like a device-resident one whatever the source size --, the copy's event, mean / scale on
    the device (c floats each, uploaded once per request: load_network needs no device), `extents` = {extent: _Staging}, least recently
    fed first -- a FrameFeed's frames under (extent, m) --, `tables` = {FrameFeed.KIND: _Pair}, the table of each kind once one is fed
    (TABLES), and `producers` = {DetectedRois: _Detected, LandmarkWarps: _Landmarks}, what a feed whose table a launch makes needs besides.
    `fed`: the extent of the whole images the last pass was staged from (what a declared fit fitted), else None.  `last`: what the
    input was last fed -- 'table' (a feed of rectangles: tables['roi'] holds that pass's regions), 'images' (whole images), 'warp' (a
    sampled feed: no rectangle per row) or None (anything else): what a LandmarkWarps over this network's Result normalises its points
    to.  `table_readers`: events behind the launches of OTHER requests that read tables['roi'] on the device (a LandmarkWarps fed from
    this request); stage() waits for them before anything overwrites the table."""
    __slots__ = ('fixed', 'event', 'mean', 'std', 'extents', 'tables', 'producers', 'fed', 'last', 'table_readers')

    def __init__(self, fmt):
        self.fixed, self.event = device.DeviceTensor.empty(fmt.dims), device.Event(timed=False)
        self.mean, self.std = (None, None) if fmt.mean is None else (device.DeviceTensor.from_numpy(fmt.mean), device.DeviceTensor.from_numpy(fmt.std))
        self.extents, self.tables, self.producers = collections.OrderedDict(), {}, {}
        self.fed, self.last, self.table_readers = None, None, []

    def table(self, kind) -> _Pair:
        pair = self.tables.get(kind)
        if pair is None:
            n, (columns, dtype, block) = self.fixed.shape[0], TABLES[kind]
            pair = self.tables[kind] = _Pair((n, columns), dtype, block and block(n))
        return pair

    def producer(self, made):
        found = self.producers.get(made.FEED)
        if found is None:
            found = self.producers[made.FEED] = made()
        return found


class _Producer:
    """What a slot keeps for a feed whose table is made on the device from another request's Result or from arrays: the event recorded
    behind the launch that reads that Result (the request's next pass waits for it); `sources`: the device tensors the last launch
    read, kept alive until the next pass of this input; `live`: the last pass of the input was such a feed."""
    __slots__ = ('read', 'sources', 'live')

    def __init__(self):
        self.read, self.sources, self.live = device.Event(timed=False), (), False


class _Detected(_Producer):
    """DetectedRois: the labels, and the records of a host array for the record count last fed."""
    __slots__ = ('labels', 'records')
    FEED = DetectedRois

    def __init__(self):
        super().__init__()
        self.labels, self.records = _Pair((DetectedRois.MAX_LABELS,), np.int32), None


class _Landmarks(_Producer):
    """LandmarkWarps: the packed template and the bytes of the one uploaded last (`packed`: a template is uploaded once), and the points
    and the regions of host arrays for the row count last fed."""
    __slots__ = ('template', 'packed', 'points', 'regions')
    FEED = LandmarkWarps

    def __init__(self):
        super().__init__()
        self.template, self.packed = _Pair((2 * landmark_rule.MAX_POINTS + 3,), np.float64), None
        self.points = self.regions = None


# what a stager hands stage(): the _Staging of the frames, the _Pair.upload's beside them, the launch to issue on the base stream in
# front of the conversion or None, `largest` and `kind` as InputFormat.conversion takes them
_Staged = collections.namedtuple('_Staged', 'staging uploads launch largest kind')


class HostInputs:
    """The host-input state of one Executable_Network (one per request): `formats` = {input name: InputFormat}, fixed at load_network
    and shared by every request; `slots` = {input name: _Slot} of the inputs fed from the host so far."""
    # source extents (h, w) of a resized input -- and (extent, frame count) pairs of its FrameFeeds -- whose buffers a request keeps at once
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
        """The staging of input `name` for sources of `extent` (`frames` = m: for the m frames of a FrameFeed), made on first use."""
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
        = m: the one the m frames of a FrameFeed are uploaded from."""
        fmt = self._format(name)
        if frames is not None:
            frames = fmt.checked_frames(frames)
        return self._staging(name, fmt.checked_extent(source_size), frames).host

    def _table_buffer(self, name, feed) -> np.ndarray:
        self._format(name).resize_declared(feed)
        return self._slot(name).table(feed.KIND).host

    def roi_buffer(self, name) -> np.ndarray:
        """The page-locked (n, 5) int32 table a RoiInput of input `name` is uploaded from."""
        return self._table_buffer(name, RoiInput)

    def warp_buffer(self, name) -> np.ndarray:
        """The page-locked (n, 7) int64 table a WarpInput of input `name` is uploaded from."""
        return self._table_buffer(name, WarpInput)

    def perspective_buffer(self, name) -> np.ndarray:
        """The page-locked (n, 10) int64 table a PerspectiveInput of input `name` is uploaded from."""
        return self._table_buffer(name, PerspectiveInput)

    def _stage_matrices(self, name, fmt, warp, sharded):
        """The frames and the table of WarpInput or PerspectiveInput `warp` in this request's page-locked buffers -- copied, unless
        they are those buffers --, everything checked before anything is allocated."""
        feed, slot, given = type(warp), self.slots.get(name), warp.matrices
        fmt.resize_declared(feed)
        frames = np.asarray(warp.frames)
        extent, m = fmt.frames_extent_of(frames, feed)
        pair = slot.tables.get(feed.KIND) if slot is not None else None
        own = pair is not None and pair.holds(given)
        if own:
            if warp.ids is not None:
                raise ValueError('input {}: the {}_buffer holds the frame of each row in its first column: ids is None with it'.format(name, feed.BUFFER))
            fmt.checked_matrix_table(feed, given, m)
        else:
            table = fmt.checked_matrices(feed, given, warp.ids, m)
        staged = self._staging(name, extent, m).copy_in(frames)
        pair = self.slots[name].table(feed.KIND)
        if not own:
            np.copyto(pair.host, table)
        return _Staged(staged, (pair.upload,), None, None, feed.KIND)

    def _stage_rois(self, name, fmt, roi, sharded):
        """The frames and the table of RoiInput `roi` in this request's page-locked buffers -- copied, unless they are those buffers --,
        everything checked before anything is allocated; `largest` is the (max_h, max_w) of its rectangles."""
        frames = np.asarray(roi.frames)
        extent, m = fmt.frames_extent_of(frames)
        table, largest = fmt.checked_rois(roi.rois, extent, m)
        staged = self._staging(name, extent, m).copy_in(frames)
        pair = self.slots[name].table('roi')
        if not pair.holds(roi.rois):
            np.copyto(pair.host, table)
        return _Staged(staged, (pair.upload,), None, largest, 'roi')

    @staticmethod
    def _result_of(name, src, output, words, checks):
        """What a feed over `src` reads, nothing waited for and nothing copied: (value -- a DeviceTensor or a host array --, the runner
        whose pass produces it or None, the event behind that pass or None, what `checks` returned or None).  `src`: a DeviceTensor or
        an array; or the InferRequest of another network, in flight -- its device-resident Result -- or waited for -- its host Results,
        like an array.  `output` names the Result when there are several; `words` = (the network, its request, the Result `output`
        names) as the texts say them; `checks(runner, node id, Result name)` runs before the Result is asked for."""
        if not (hasattr(src, 'runner') and hasattr(src, 'start_async')):         # (an InferRequest: inference_engine imports this module)
            return (src if isinstance(src, device.DeviceTensor) else np.asarray(src)), None, None, None
        runner = src.runner
        net = runner.ienet
        results = net.find_node_by_type('Result')
        if output is not None:
            results = [r for r in results if r[1] == output]
            if not results:
                raise ValueError('input {}: the {} has no Result named {!r}'.format(name, words[0], output))
        elif len(results) != 1:
            raise ValueError('input {}: the {} has {} Results: output= names {}'.format(name, words[0], len(results), words[2]))
        nid = results[0][0]
        checked = checks(runner, nid, results[0][1])
        replayed, pending = (src._replayed, runner._pending) if src._in_flight else (None, None)
        value = replayed['results'][results[0][1]] if replayed is not None else net.G.nodes[nid].get('result')
        if value is None:
            raise RuntimeError('input {}: the {} never ran: start_async() or infer() it first'.format(name, words[1]))
        if not isinstance(value, device.DeviceTensor):        # waited for: its host Results, like an array
            return np.asarray(value), runner, None, checked
        return value, runner, (pending[1] if pending is not None else None), checked

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
        buffer) and its options, everything checked before anything is allocated; the launch makes the table of the ROI launch behind
        it, which is sized for whole frames: the host does not know the largest rectangle, the frame bounds it."""
        if sharded:
            raise NotImplementedError('input {}: DetectedRois with a batch sharded over ranks'.format(name))
        frames = np.asarray(det.frames)
        extent, m = fmt.frames_extent_of(frames)
        conf, labels, (min_h, min_w) = det.checked_options(name)

        def is_detection_output(runner, nid, result):
            net = runner.ienet
            if [net.G.nodes[p]['type'] for p in net.G.pred[nid]] != ['DetectionOutput']:
                raise ValueError('input {}: Result {!r} of the detector is no DetectionOutput'.format(name, result))

        records, runner, done, _ = self._result_of(name, det.detections, det.output, ('detector', 'detector request', 'the DetectionOutput one'),
                                                   is_detection_output)
        images, fit = (runner.ienet.batch_size, runner.host_inputs.detector_fit()) if runner is not None else (None, None)
        if det.detector_fit is not None:
            fit = detections_rule.checked_fit(det.detector_fit, 'input {}: detector_fit'.format(name))
        images = det.images if det.images is not None else (images if images is not None else m)
        per_image = det.checked_records(name, records.shape, records.dtype, images, m)
        staged = self._staging(name, extent, m).copy_in(frames)
        slot = self.slots[name]
        table, d = slot.table('roi').block, slot.producer(_Detected)
        uploads = []
        if labels is not None and len(labels):
            d.labels.host[:len(labels)] = labels
            uploads.append(d.labels.upload)
        listed = device.ptr(d.labels.device if labels is not None else None)       # NULL: any label
        if isinstance(records, device.DeviceTensor):
            d.sources = (records,)
        else:
            d.records = _Pair.of_shape(d.records, (images * per_image, 7), np.float32)
            np.copyto(d.records.host, records.reshape(-1, 7))
            d.sources = (d.records.device,)
            uploads.append(d.records.upload)
            runner = None                                     # (waited for: nothing of the detector's is read on the device)
        n = slot.fixed.shape[0]

        def launch():
            if done is not None:
                done.wait()                                   # the detector's pass, on the device
            device.call('pvhip_detections_to_rois' + ('_fit' if fit is not None else ''), device.ptr(d.sources[0]), ctypes.c_void_p(table.ptr),
                        ctypes.c_void_p(table.ptr + 20 * n), ctypes.c_void_p(table.ptr + 24 * n), n, images, per_image, *extent,
                        conf, listed, 0 if labels is None else len(labels), min_h, min_w, *(fit or ()))
            if runner is not None:                            # its next pass may overwrite that Result: not before this launch has read it
                runner._result_readers.append(d.read.record())

        return _Staged(staged, uploads, launch, extent, 'roi')

    def detected_rois(self, name, stream_base) -> DetectedTable:
        """The table the last pass of input `name` used, read back in one copy on stream `stream_base`, which has drained."""
        t, n = self._made_table(name, DetectedRois, stream_base)
        return DetectedTable(int(t[6 * n]), int(t[6 * n + 1]), t[:5 * n].reshape(n, 5).copy(), t[5 * n:6 * n].copy())

    def _made_table(self, name, feed, stream_base):
        """(the block behind the table a launch made for the last pass of input `name`, read back on stream `stream_base`, n)."""
        self._format(name)
        slot = self.slots.get(name)
        if slot is None or feed not in slot.producers or not slot.producers[feed].live:
            raise RuntimeError('input {}: its last pass was not fed a {}'.format(name, feed.__name__))
        device.select_stream(stream_base)
        raw = np.asarray(slot.tables[feed.KIND].block)
        device.select_stream(0)
        return raw, slot.fixed.shape[0]

    def _stage_landmarks(self, name, fmt, lw, sharded):
        """The frames of LandmarkWarps `lw` in this request's page-locked buffers, its template, and its points and regions when they are
        host arrays, everything checked before anything is allocated; the launch fits the table of the warp launch behind it."""
        if sharded:
            raise NotImplementedError('input {}: LandmarkWarps with a batch sharded over ranks'.format(name))
        fmt.resize_declared(WarpInput)
        frames = np.asarray(lw.frames)
        extent, m = fmt.frames_extent_of(frames, LandmarkWarps)
        packed = lw.checked_template(name)
        k = (len(packed) - 3) // 2

        def region_owner(runner, nid, result):
            """The _Slot whose region table the landmark pass was fed, or None: the whole frame."""
            fed = runner.host_inputs
            names = [key for key, f in fed.formats.items() if len(f.dims) == 4]
            owner = fed.slots.get(names[0]) if len(names) == 1 else None
            if len(names) == 1 and fed.formats[names[0]].fitted:
                raise ValueError('input {}: input {!r} of the landmark network declares resize_fit {}: its points are normalised to a fitted '
                                 'rectangle, not to the region'.format(name, names[0], fed.formats[names[0]].fit))
            if owner is not None and owner.last == 'warp':
                raise ValueError('input {}: input {!r} of the landmark network was last fed a WarpInput, a PerspectiveInput or a LandmarkWarps: '
                                 'its rows have no rectangle the points are normalised to'.format(name, names[0]))
            return owner if owner is not None and owner.last == 'table' else None

        points, runner, done, owner = self._result_of(name, lw.landmarks, lw.output,
                                                      ('landmark network', 'landmark request', 'the one that holds the points'), region_owner)
        rows = lw.checked_points(name, points.shape, points.dtype, k)
        regions = lw.checked_regions(name, rows)
        given = owner.tables['roi'].device if owner is not None else None
        if regions is not None:
            owner = given = None
        elif owner is not None and given.shape[0] != rows:
            raise ValueError('input {}: the landmark pass was fed a table of {} regions, its Result holds {} rows of points: regions names '
                             'the rectangle of each row'.format(name, given.shape[0], rows))
        elif owner is None and m != 1 and m != rows:
            raise ValueError('input {}: landmarks over whole frames read frame b for row b (m == N) or frame 0 (m == 1); with {} frames for {} '
                             'rows of points, regions names the frame and the rectangle of each row'.format(name, m, rows))
        staged = self._staging(name, extent, m).copy_in(frames)
        slot = self.slots[name]
        table, lm = slot.table('warp'), slot.producer(_Landmarks)
        uploads = []
        if lm.packed != packed.tobytes():                      # a template is uploaded once
            lm.template.host[:len(packed)] = packed
            lm.packed = packed.tobytes()
            uploads.append(lm.template.upload)
        if isinstance(points, device.DeviceTensor):
            source = points
        else:
            lm.points = _Pair.of_shape(lm.points, (rows, 2 * k), np.float32)
            np.copyto(lm.points.host, points.reshape(rows, 2 * k))
            source, runner = lm.points.device, None           # (waited for: no Result of the landmark request's is read on the device)
            uploads.append(lm.points.upload)
        if regions is not None:
            lm.regions = _Pair.of_shape(lm.regions, (rows, 5), np.int32)
            np.copyto(lm.regions.host, regions)
            given = lm.regions.device
            uploads.append(lm.regions.upload)
        lm.sources = (source, given)                          # (no regions, NULL: the whole frame)
        n = slot.fixed.shape[0]

        def launch():
            if done is not None:
                done.wait()                                   # the landmark pass, on the device
            device.call('pvhip_landmarks_to_warps', device.ptr(source), device.ptr(given), device.ptr(lm.template.device),
                        device.ptr(table.device), ctypes.c_void_p(table.block.ptr + 56 * n), n, rows, k, m, *extent)
            if runner is not None or owner is not None:
                read = lm.read.record()
                if runner is not None:
                    runner._result_readers.append(read)       # its next pass may overwrite that Result: not before this launch has read it
                if owner is not None and read not in owner.table_readers:       # (one event per consumer slot, recorded again each pass)
                    owner.table_readers.append(read)          # nor may its next stage() overwrite that table

        return _Staged(staged, uploads, launch, None, 'warp')

    def landmark_warps(self, name, stream_base) -> LandmarkTable:
        """The table the last pass of input `name` used, read back in one copy on stream `stream_base`, which has drained."""
        raw, n = self._made_table(name, LandmarkWarps, stream_base)
        valid = raw[56 * n:].view(np.int32)
        return LandmarkTable(int(valid[n]), valid[:n] != 0, raw[:56 * n].view(np.int64).reshape(n, 7).copy())

    def _find_or_copy(self, name, fmt, arr):
        """The staging host array `arr` is fed through: the one whose page-locked buffer `arr` is, else -- for a declared format -- the
        one of its extent with `arr` copied into it; None: the input goes the default way."""
        slot = self.slots.get(name)
        if slot is not None:
            # (the frames buffer of a FrameFeed is none of them: handed in without its table it is an array like any other)
            for s in slot.extents.values():
                if s.frames is None and _is_array(arr, s.host):
                    return s
        if not fmt.declared:
            return None
        a = np.asarray(arr)
        return self._staging(name, fmt.extent_of(a)).copy_in(a)

    _STAGERS = {RoiInput: _stage_rois, DetectedRois: _stage_detected, WarpInput: _stage_matrices, PerspectiveInput: _stage_matrices,
                LandmarkWarps: _stage_landmarks}

    def stage(self, inputs: dict, stream_base: int, sharded: bool = False) -> dict:
        """`inputs` with every host input of a declared format, or in one of this request's own buffers, replaced by the request's fixed
        tensor: the caller's array is copied into the page-locked buffer of its extent unless it IS that buffer, the buffer is uploaded on
        the copy stream, stream `stream_base` waits for the copy's event and converts (InputFormat.conversion: one launch at the most).
        A FrameFeed goes the same way through its stager (_STAGERS): its frames, and what it uploads beside them -- the table of a
        RoiInput, a WarpInput or a PerspectiveInput; a DetectedRois' labels, and its records when they are a host array; a LandmarkWarps'
        template, once, and its points and regions when they are host arrays --, all on the copy stream behind the one event.  The
        table of a DetectedRois or a LandmarkWarps is made by the stager's launch on `stream_base` in front of the conversion, behind
        the other request's pass when it reads the Result of one in flight: the host never sees it (`sharded`: the batch is sharded over
        ranks, which both refuse).  A LandmarkWarps' launch may read ANOTHER request's region table: it leaves an event in that slot's
        `table_readers`, and the copy stream and `stream_base` wait for those before this call uploads or makes a table for the slot.
        Every other input is returned unchanged (and goes the default way).  All but the MAX_SOURCE_EXTENTS most recently fed extents
        of an input are released here: the request has no pass in flight, so nothing reads those buffers any more."""
        out = dict(inputs)
        for name, arr in inputs.items():
            fmt = self.formats.get(name)
            stager = self._STAGERS.get(type(arr))
            if stager is None and isinstance(arr, FrameFeed):     # (a subclass of one of the five)
                stager = next(self._STAGERS[cls] for cls in type(arr).__mro__ if cls in self._STAGERS)
            if stager is not None:
                staged = stager(self, name, self._format(name), arr, sharded)
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
                staged = _Staged(staged, (), None, None, None)
            slot, (staging, uploads, launch, largest, kind) = self.slots[name], staged
            slot.fed = staging.extent if kind is None else None
            slot.last = 'images' if kind is None else 'table' if arr.RECTANGLES else 'warp'
            if slot.table_readers:                            # launches of other requests still read the table: nothing overwrites it before them
                readers, slot.table_readers = slot.table_readers, []
                for stream in (device.COPY_STREAM, stream_base):
                    device.select_stream(stream)
                    for event in readers:
                        event.wait()
            slot.extents.move_to_end(staging.key)
            while len(slot.extents) > self.MAX_SOURCE_EXTENTS:
                slot.extents.popitem(last=False)
            device.select_stream(device.COPY_STREAM)
            for dst, host in ((staging.staging, staging.host), *uploads):
                device.call('pvhip_memcpy_h2d_async', device.ptr(dst), ctypes.c_void_p(host.ctypes.data), host.nbytes)
            slot.event.record()
            device.select_stream(stream_base)
            slot.event.wait()
            for feed, producer in slot.producers.items():
                producer.live = isinstance(arr, feed)
                if not producer.live:
                    producer.sources = ()
            if launch is not None:
                launch()
            entry, args = fmt.conversion(staging.extent, staging.frames, largest, kind)
            if entry is not None:
                ptr, table = device.ptr, slot.tables.get(kind)
                operands = {'src': ptr(staging.staging), 'dst': ptr(slot.fixed), 'table': ptr(table and table.device), 'mean': ptr(slot.mean),
                            'std': ptr(slot.std), 'NULL': NULL}
                device.call(entry, *map(operands.get, args, args))      # (every argument that is no operand's name stands for itself)
            device.select_stream(0)
            out[name] = slot.fixed
        return out
