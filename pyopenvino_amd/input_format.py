"""The format a caller hands a network input in: what is declared between ``read_network`` and ``load_network`` (InputInfo, PreProcessInfo,
PreProcessChannel: OpenVINO 2021's ``IENetwork.input_info``) and the fixed value it becomes at load (InputFormat), which owns the shape
arithmetic of that format and the choice of the launch that converts it (``InputFormat.conversion``); and the inputs given as frames
and a rule per batch row instead of images (FrameFeed: RoiInput, DetectedRois, WarpInput, PerspectiveInput, LandmarkWarps), each
stating what the format checks of it.  Host only: nothing here touches the device (host_input.py stages arrays of these formats)."""
import collections
import dataclasses
import functools

import numpy as np

from . import landmarks as landmark_rule

# color formats whose frames are YUV 4:2:0 planes, (n, 3 h / 2, w), and those whose frames are rows of 4-byte units with the `kind` of
# pvhip_input_preprocess_packed_f32: packed YUV 4:2:2 (n, h, w, 2) and four-byte pixels (n, h, w, 4)
YUV420_FORMATS = ('NV12', 'I420')
PACKED_KINDS = {'YUY2': 0, 'UYVY': 1, 'BGRX': 2, 'RGBX': 3}
# how a resized source is placed in the Parameter's extent, with the `fit` of the pvhip_input_preprocess_*_fit_f32 entries
RESIZE_FITS = {'STRETCH': 0, 'LETTERBOX': 1, 'TOP_LEFT': 2}
# the matrix a YUV format's frames were encoded with, with the `matrix` of the pvhip_input_preprocess_*_color_f32 entries, and their range
# (`full_range` 0 / 1); 'BGRX' / 'RGBX' hold nothing to convert
COLOR_STANDARDS = {'BT601': 0, 'BT709': 1, 'BT2020': 2}
COLOR_RANGES = {'LIMITED': 0, 'FULL': 1}
YUV_FORMATS = YUV420_FORMATS + ('YUY2', 'UYVY')


def fit_geometry(src_hw, dst_hw, fit) -> tuple:
    """(dx, dy, iw, ih): the rectangle of a destination (hd, wd) that a source (or ROI rectangle) of (hs, ws) is fitted into -- one scale
    factor for both axes, the short side rounded half up and kept in [1, D]; 'LETTERBOX' centres it (floor), 'TOP_LEFT' does not; 'STRETCH'
    is the whole destination.  Python ints: the rule of include/pvhip.h (pvhip_input_preprocess_fit_f32) word for word."""
    (hs, ws), (hd, wd) = (int(v) for v in src_hw), (int(v) for v in dst_hw)
    if fit == 'STRETCH':
        return 0, 0, wd, hd
    if ws * hd >= hs * wd:
        iw, ih = wd, min(max((2 * hs * wd + ws) // (2 * ws), 1), hd)
    else:
        ih, iw = hd, min(max((2 * ws * hd + hs) // (2 * hs), 1), wd)
    return ((wd - iw) // 2, (hd - ih) // 2, iw, ih) if fit == 'LETTERBOX' else (0, 0, iw, ih)


@dataclasses.dataclass(frozen=True, eq=False)
class InputFormat:
    """One input's format as a fixed value (``InputInfo.frozen()``; load_network makes one per input and every request reads that one):
    ``dims`` the (n, c, h, w) of the fp32 tensor the IR expects, ``supported`` / ``declared`` as InputInfo has them, ``u8`` / ``nhwc`` the
    declared precision and layout, ``resize`` / ``reverse`` / ``mean`` / ``std`` the declared preprocessing (fp32 arrays of c values, or
    None without MEAN_VALUE), ``fit`` / ``pad`` the declared placement of a resized source ('STRETCH', or 'LETTERBOX' / 'TOP_LEFT': one
    scale factor, the rest of the extent filled with ``pad``; ``fit_geometry``), ``color`` the declared colour format: 'RAW', or 'NV12' / 'I420' for YUV 4:2:0 frames, uint8 of shape
    (n, 3 h / 2, w), or 'YUY2' / 'UYVY' for packed YUV 4:2:2 frames, uint8 of shape (n, h, w, 2), or 'BGRX' / 'RGBX' for four-byte
    pixels, uint8 of shape (n, h, w, 4), whatever ``u8`` / ``nhwc`` say; ``standard`` / ``full_range`` the declared matrix ('BT601', 'BT709',
    'BT2020') and range of a YUV format's frames, which ``color_rule`` hands every launch that converts them -- a plain pass, a RoiInput, a
    DetectedRois, a WarpInput, a PerspectiveInput and a fitted input alike: the rule belongs to the format, not to the feed.  An extent is the (h, w) of a caller's image.  A FrameFeed's frames have the same
    shapes with their own count m in place of n (``host_shape(extent, frames=m)``, ``frames_extent_of``); a RoiInput's table is what
    ``checked_rois`` accepts, a WarpInput's or a PerspectiveInput's what ``checked_matrices`` makes (in the request's own buffer:
    ``checked_matrix_table``).  ``conversion`` names the launch and its arguments for an extent and a feed."""
    name: str
    dims: tuple
    supported: bool
    declared: bool
    u8: bool
    nhwc: bool
    resize: bool
    reverse: bool
    mean: np.ndarray
    std: np.ndarray
    color: str = 'RAW'
    fit: str = 'STRETCH'
    pad: float = 0.0
    standard: str = 'BT601'
    full_range: bool = False

    @property
    def color_rule(self) -> tuple:
        """(matrix, full_range) as the pvhip_input_preprocess_*_color_f32 entries take them; (0, 0), BT.601 limited range, is the rule
        of the entries without them (``default_rule``)."""
        return COLOR_STANDARDS[self.standard], int(self.full_range)

    @property
    def default_rule(self) -> bool:
        return self.color_rule == (0, 0)

    @property
    def fitted(self) -> bool:
        """A fit other than the stretch is declared: the pvhip_input_preprocess_*_fit_f32 entries, with ``fit_code`` as their `fit`."""
        return self.fit != 'STRETCH'

    @property
    def fit_code(self) -> int:
        return RESIZE_FITS[self.fit]

    def fit_geometry(self, extent) -> tuple:
        """(dx, dy, iw, ih) of a source of `extent` = (h, w) in the network's extent under the declared fit."""
        return fit_geometry(extent, self.dims[2:], self.fit)

    @property
    def yuv(self) -> bool:
        """YUV 4:2:0 frames (NV12, I420)."""
        return self.color in YUV420_FORMATS

    @property
    def packed(self) -> bool:
        """Frames of 4-byte units (YUY2, UYVY, BGRX, RGBX): ``packed_kind`` is their `kind` for pvhip_input_preprocess_packed_f32 and
        ``packed_bytes`` the trailing axis of their arrays: 2 bytes per pixel of 4:2:2, 4 of an X format."""
        return self.color in PACKED_KINDS

    @property
    def packed_kind(self) -> int:
        return PACKED_KINDS[self.color]

    @property
    def packed_bytes(self) -> int:
        return 2 if self.packed_kind < 2 else 4

    @property
    def host_dtype(self):
        return np.dtype(np.uint8 if self.u8 or self.yuv or self.packed else np.float32)

    def host_shape(self, extent=None, frames=None):
        """The shape of a caller's array of `extent` (default: the network's own) in this layout; `frames` = m: of the m frames of a
        RoiInput (default: one image per batch row)."""
        n, c = self.dims[:2]
        n = n if frames is None else frames
        h, w = extent if extent is not None else self.dims[2:]
        if self.yuv:
            return n, (h // 2 * 3 if isinstance(h, int) else '3h/2'), w
        if self.packed:
            return n, h, w, self.packed_bytes
        return (n, h, w, c) if self.nhwc else (n, c, h, w)

    def checked_extent(self, source_size=None):
        """The (h, w) a caller's image has: `source_size` with RESIZE_BILINEAR declared, else the network's own (even, for YUV 4:2:0; of even width, for
        packed YUV 4:2:2)."""
        n, c, h, w = self.dims
        sh, sw = (int(v) for v in source_size) if source_size is not None else (h, w)
        if self.yuv and (sh % 2 or sw % 2):
            raise ValueError('input {}: {} frames have an even height and width, not {}'.format(self.name, self.color, (sh, sw)))
        if self.packed and self.packed_bytes == 2 and sw % 2:
            raise ValueError('input {}: {} frames have an even width, not {}'.format(self.name, self.color, (sh, sw)))
        if source_size is None:
            return h, w
        if (sh, sw) != (h, w) and not self.resize:
            raise ValueError('input {}: source size {} differs from the network\'s {} and no resize is declared '
                             '(preprocess_info.resize_algorithm = \'RESIZE_BILINEAR\')'.format(self.name, (sh, sw), (h, w)))
        if sh < 1 or sw < 1:
            raise ValueError('input {}: source size {} is empty'.format(self.name, (sh, sw)))
        return sh, sw

    def extent_of(self, a):
        """(h, w) of the caller's array `a`, checked against this format."""
        if self.yuv:
            return self._yuv_extent_of(a)
        if self.packed:
            return self._packed_extent_of(a)
        declared = 'declared {} / {}'.format('U8' if self.u8 else 'FP32', 'NHWC' if self.nhwc else 'NCHW')
        if not self.resize:
            if a.shape != self.host_shape():
                raise ValueError('input {}: {} means shape {}, got {}'.format(self.name, declared, self.host_shape(), a.shape))
            return tuple(self.dims[2:])
        if a.ndim != 4 or (a.shape[0], a.shape[3 if self.nhwc else 1]) != self.dims[:2]:
            raise ValueError('input {}: {} with RESIZE_BILINEAR means shape {} for any h, w; got {}'.format(
                self.name, declared, self.host_shape(('h', 'w')), a.shape))
        return self.checked_extent(a.shape[1:3] if self.nhwc else a.shape[2:4])

    def _yuv_extent_of(self, a):
        declared = 'declared {}'.format(self.color)
        if not self.resize:
            if a.shape != self.host_shape():
                raise ValueError('input {}: {} means shape {}, got {}'.format(self.name, declared, self.host_shape(), a.shape))
            return tuple(self.dims[2:])
        if a.ndim != 3 or a.shape[0] != self.dims[0] or a.shape[1] % 3:
            raise ValueError('input {}: {} with RESIZE_BILINEAR means shape {} for any even h, w; got {}'.format(
                self.name, declared, self.host_shape(('h', 'w')), a.shape))
        return self.checked_extent((a.shape[1] // 3 * 2, a.shape[2]))

    def _packed_any_hw(self):
        return 'any h and even w' if self.packed_bytes == 2 else 'any h, w'

    def _packed_extent_of(self, a):
        declared = 'declared {}'.format(self.color)
        if not self.resize:
            if a.shape != self.host_shape():
                raise ValueError('input {}: {} means shape {}, got {}'.format(self.name, declared, self.host_shape(), a.shape))
            return tuple(self.dims[2:])
        if a.ndim != 4 or a.shape[0] != self.dims[0] or a.shape[3] != self.packed_bytes:
            raise ValueError('input {}: {} with RESIZE_BILINEAR means shape {} for {}; got {}'.format(
                self.name, declared, self.host_shape(('h', 'w')), self._packed_any_hw(), a.shape))
        return self.checked_extent(a.shape[1:3])

    def resize_declared(self, feed=None):
        """ValueError unless a resize is declared: every FrameFeed needs one (`feed`: the class the text names; default: RoiInput)."""
        feed = feed or RoiInput
        if not self.resize:
            raise ValueError('input {}: a {} {} on the device: it needs a declared resize '
                             '(preprocess_info.resize_algorithm = \'RESIZE_BILINEAR\')'.format(self.name, feed.__name__, feed.HOW))

    def checked_frames(self, frames) -> int:
        """The frame count m of a RoiInput as an int >= 1 (any count: it is independent of the batch)."""
        self.resize_declared()
        if isinstance(frames, bool) or not isinstance(frames, (int, np.integer)) or frames < 1:
            raise ValueError('input {}: a RoiInput has m >= 1 frames, not {!r}'.format(self.name, frames))
        return int(frames)

    def frames_extent_of(self, a, feed=None):
        """((h, w), m) of the frames array `a` of a FrameFeed (`feed`: the class the texts name; default: RoiInput), checked against
        this format."""
        self.resize_declared(feed)
        what = (feed or RoiInput).__name__
        if self.yuv:
            ok = a.ndim == 3 and a.shape[0] >= 1 and a.shape[1] % 3 == 0
            declared, any_hw = 'declared {}'.format(self.color), 'any even h, w'
        elif self.packed:
            ok = a.ndim == 4 and a.shape[0] >= 1 and a.shape[3] == self.packed_bytes
            declared, any_hw = 'declared {}'.format(self.color), self._packed_any_hw()
        else:
            ok = a.ndim == 4 and a.shape[0] >= 1 and a.shape[3 if self.nhwc else 1] == self.dims[1]
            declared, any_hw = 'declared {} / {}'.format('U8' if self.u8 else 'FP32', 'NHWC' if self.nhwc else 'NCHW'), 'any h, w'
        if not ok:
            raise ValueError('input {}: {} frames of a {} have shape {} for any m >= 1 and {}; got {}'.format(
                self.name, declared, what, self.host_shape(('h', 'w'), frames='m'), any_hw, a.shape))
        if self.yuv:
            return self.checked_extent((a.shape[1] // 3 * 2, a.shape[2])), a.shape[0]
        return self.checked_extent(a.shape[1:3] if self.nhwc or self.packed else a.shape[2:4]), a.shape[0]

    def checked_rois(self, rois, extent, frames):
        """The table of a RoiInput over `frames` frames of `extent` as a C-contiguous int32 (n, 5) array, and the (max h, max w) of its
        rectangles: row b = (id, x, y, w, h), the order of OpenVINO's ROI struct, is the rectangle [y, y + h) x [x, x + w) of frame id
        that becomes batch row b.  Integers only, 0 <= id < frames, w, h >= 1 and the rectangle inside the frame."""
        self.resize_declared()
        t = np.asarray(rois)
        n, (H, W) = self.dims[0], extent
        if t.shape != (n, 5):
            raise ValueError('input {}: rois is a table of shape {} -- one (id, x, y, w, h) per batch row --, got {}'.format(
                self.name, (n, 5), t.shape))
        if t.dtype.kind not in 'iu':
            raise ValueError('input {}: rois holds integers (id, x, y, w, h), got dtype {}'.format(self.name, t.dtype))
        if t.dtype == np.uint64 and (t > np.iinfo(np.int64).max).any():
            t = np.minimum(t, np.uint64(np.iinfo(np.int64).max))          # (refused below, whichever column)
        t = t.astype(np.int64)
        i, x, y, w, h = t.T
        bad = (i < 0) | (i >= frames) | (x < 0) | (y < 0) | (w < 1) | (h < 1) | (x > W - w) | (y > H - h)
        if bad.any():
            b = int(np.argmax(bad))
            raise ValueError('input {}: rois[{}] = {} is no rectangle (id, x, y, w, h) with w, h >= 1 inside one of {} frames of {}'.format(
                self.name, b, tuple(int(v) for v in t[b]), frames, (H, W)))
        return np.ascontiguousarray(t, np.int32), (int(h.max()), int(w.max()))

    def _checked_ids(self, ids, frames):
        """The frame of every row of a WarpInput or a PerspectiveInput over `frames` frames as n ints in [0, frames): `ids`, or by default
        row b's frame b (frames == n) or frame 0 (frames == 1)."""
        n = self.dims[0]
        if ids is None:
            if frames != n and frames != 1:
                raise ValueError('input {}: a WarpInput without ids reads frame b for row b (m == n) or frame 0 (m == 1); with {} frames '
                                 'for {} rows, ids names the frame of each row'.format(self.name, frames, n))
            return np.arange(n, dtype=np.int64) if frames == n else np.zeros(n, np.int64)
        i = np.asarray(ids)
        if i.shape != (n,) or i.dtype.kind not in 'iu':
            raise ValueError('input {}: ids holds {} integers, the frame of each batch row; got {} {}'.format(self.name, n, i.dtype, i.shape))
        if i.dtype == np.uint64:
            i = np.minimum(i, np.uint64(np.iinfo(np.int64).max))
        i = i.astype(np.int64)
        bad = (i < 0) | (i >= frames)
        if bad.any():
            b = int(np.argmax(bad))
            raise ValueError('input {}: ids[{}] = {} is none of {} frames'.format(self.name, b, int(i[b]), frames))
        return i

    def checked_matrices(self, feed, matrices, ids, frames):
        """The table of a `feed` (WarpInput or PerspectiveInput, the class) over `frames` frames as a C-contiguous int64 (n, feed.COLUMNS)
        array: row b is the frame of the row (`ids`, or its default) in front of ``feed.fixed(matrices, the network's extent)``."""
        self.resize_declared(feed)
        n = self.dims[0]
        try:
            q = feed.fixed(matrices, self.dims[2:])
        except ValueError as e:
            raise ValueError('input {}: {}'.format(self.name, e)) from None
        if q.shape[0] != n:
            raise ValueError('input {}: matrices has shape {} -- one {} x {} matrix per batch row --, got {}'.format(
                self.name, (n,) + feed.MATRIX, *feed.MATRIX, np.shape(matrices)))
        table = np.empty((n, feed.COLUMNS), np.int64)
        table[:, 0] = self._checked_ids(ids, frames)
        table[:, 1:] = q
        return table

    def checked_matrix_table(self, feed, table, frames):
        """`table`, an int64 (n, feed.COLUMNS) array already in the device's form (``InferRequest.warp_buffer`` / ``perspective_buffer``),
        checked by the limits of ``feed.fixed`` over the network's extent and by ``ids``; returned as it is."""
        self.resize_declared(feed)
        bad = feed.beyond_limits(table[:, 1:], self.dims[2:])
        if bad.any():
            b = int(np.argmax(bad))
            raise ValueError('input {}: {}'.format(self.name, feed.limit_text(b, table[b, 1:], self.dims[2:])))
        self._checked_ids(table[:, 0], frames)
        return table

    @functools.lru_cache(maxsize=1024)                         # (a pure function of the format and hashable arguments, asked every pass)
    def conversion(self, extent, frames=None, largest=None, kind=None) -> tuple:
        """(entry, arguments) of the one launch that makes the fp32 NCHW tensor of arrays of `extent`, the operands as the names 'src',
        'dst', 'table', 'mean', 'std' and 'NULL' (host_input.py puts the addresses in); (None, ()) for FP32 NCHW at the network's extent
        with nothing declared besides: the upload is the tensor.  `frames` = m and `kind`: a FrameFeed's frames and FrameFeed.KIND;
        `largest` = (max_h, max_w) of its rectangles for 'roi' (for a DetectedRois the frame: the host does not know them).  The entry is
        pvhip_input_preprocess_<family><form>f32: family 'yuv_' for NV12 / I420 frames, 'packed_' for YUY2 / UYVY / BGRX / RGBX ones, ''
        for the rest; form 'roi_' with a table of rectangles, 'fit_' -- with the table or NULL -- under a declared fit that places
        anything, 'color_' -- the table or NULL, the fit or 0 -- for a colour rule other than BT.601 limited range, '' for whole
        images.  A 'warp' or a 'perspective' is pvhip_input_preprocess_<kind>[_color]_f32 for every format, whatever fit is declared.
        A bare change of precision or layout is pvhip_input_to_nchw_f32."""
        n, c, hd, wd = self.dims
        how = (int(self.color == 'I420'),) if self.yuv else (self.packed_kind,) if self.packed else (int(self.u8), int(self.nhwc))
        pre = (int(self.reverse), 'mean' if self.mean is not None else 'NULL', 'std' if self.std is not None else 'NULL')
        rule = () if self.default_rule else self.color_rule
        if kind in ('warp', 'perspective'):
            form = (1, how[0]) if self.yuv else (2, how[0]) if self.packed else (0, how[0] | how[1] << 1)
            return ('pvhip_input_preprocess_{}{}_f32'.format(kind, '_color' if rule else ''),
                    ('src', 'dst', 'table', n, frames, c, *extent, hd, wd, *form, *pre, self.pad, *rule))
        roi = largest is not None
        family = 'yuv_' if self.yuv else 'packed_' if self.packed else ''
        changed = bool(family) or self.needs_preprocess(extent)
        form = 'color_' if rule else 'fit_' if self.fitted and (roi or changed) else 'roi_' if roi else ''
        if not form and not changed:
            return ('pvhip_input_to_nchw_f32', ('src', 'dst', *self.dims, *how)) if frames is not None or self.needs_convert(extent) else (None, ())
        where = ('src', 'dst', 'table' if roi else 'NULL', n, frames if roi else n) if form else ('src', 'dst', n)
        sizes = (*extent, hd, wd, *((largest if roi else extent) if form else ()))
        fit = (self.fit_code, self.pad) if form in ('fit_', 'color_') else ()
        return 'pvhip_input_preprocess_' + family + form + 'f32', (*where, *(() if family else (c,)), *sizes, *how, *pre, *fit, *rule)

    def needs_preprocess(self, extent) -> bool:
        """Arrays of `extent` go through pvhip_input_preprocess_f32 (YUV 4:2:0 frames: pvhip_input_preprocess_yuv_f32, frames of 4-byte
        units: pvhip_input_preprocess_packed_f32, always): something besides the format change is in effect -- a declared fit that
        leaves padding among it."""
        h, w = self.dims[2:]
        return (tuple(extent) != (h, w) or self.reverse or self.mean is not None or self.yuv or self.packed
                or (self.fitted and self.fit_geometry(extent) != (0, 0, w, h)))

    def needs_convert(self, extent) -> bool:
        """Arrays of `extent` are not the fp32 NCHW tensor itself: they are uploaded into a staging tensor and converted by one launch."""
        return self.needs_preprocess(extent) or self.u8 or self.nhwc


class FrameFeed:
    """A network input given as m >= 1 source frames in the input's declared host format -- the leading count is m, whatever the batch n
    -- and a rule that makes each batch row of them on the device: what RoiInput, DetectedRois, WarpInput, PerspectiveInput and
    LandmarkWarps share.  ``HOW``: what the device does with the frames, as the "needs a declared resize" error says it; ``RECTANGLES``:
    every row is a rectangle (id, x, y, w, h) of a frame, so points in the row can be normalised to it -- no row of a sampled feed has
    one; ``KIND``: the conversion its rows go through and the table of the request they are read from, 'roi', 'warp' or 'perspective'
    (``InputFormat.conversion``)."""
    __slots__ = ()             # (every feed names `frames` first among its own)
    HOW, RECTANGLES, KIND = 'is sampled', False, 'warp'


class RoiInput(FrameFeed):
    """A network input given as regions of interest (OpenVINO 2021's ROI blobs, ``make_shared_blob(frame, ROI{id, posX, posY, sizeX,
    sizeY})``): ``infer({name: RoiInput(frames, rois)})``.  `frames`: m >= 1 source frames in the input's declared host format -- the
    leading count is m, whatever the batch n --; `rois`: an integer (n, 5) table, row b = (id, x, y, w, h): batch row b is the rectangle
    [y, y + h) x [x, x + w) of frame id, cropped and then resized to the network's extent, reversed and scaled as declared, on the
    device in one launch (pvhip_input_preprocess_roi_f32 / _yuv_roi_f32 / _packed_roi_f32).  The frames are uploaded once, however many rows read them, and
    are not modified.  The input needs ``preprocess_info.resize_algorithm = 'RESIZE_BILINEAR'``.  The bilinear taps clamp at the edge
    of the rectangle, not of the frame; a rectangle of exactly the network's extent is copied; an NV12 / I420 rectangle may have an odd
    origin and odd sizes (only the frame's extent is even), and so may a YUY2 / UYVY one (only the frame's width is even).  With `frames` = ``InferRequest.input_buffer(name, (h, w), frames=m)`` and
    `rois` = ``InferRequest.roi_buffer(name)`` nothing is copied on the host."""
    __slots__ = ('frames', 'rois')
    HOW, RECTANGLES, KIND = 'is cropped and resized', True, 'roi'

    def __init__(self, frames, rois):
        self.frames, self.rois = frames, rois

    def __repr__(self):
        return 'RoiInput(frames={}, rois={})'.format(getattr(self.frames, 'shape', None), getattr(self.rois, 'shape', None))


class WarpInput(FrameFeed):
    """A network input given as affine warps of frames (a face aligned by its eye line, a plate cut along its own axis, a rotated box, a
    mirrored copy): ``infer({name: WarpInput(frames, matrices, ids)})``, wherever a RoiInput is accepted.  `frames`: m >= 1 source
    frames in the input's declared host format, exactly as for RoiInput (every format: U8 / FP32, NHWC / NCHW, NV12, I420, YUY2, UYVY,
    BGRX, RGBX); uploaded once and not modified.  `matrices`: real numbers of shape (n, 2, 3); row b maps an OUTPUT pixel index (x, y)
    of the network's extent to a SOURCE position in frame pixels, sx = a00 x + a01 y + c0, sy = a10 x + a11 y + c1, pixel centres at
    the integers: the matrix ``cv2.warpAffine(..., flags=INTER_LINEAR | WARP_INVERSE_MAP)`` takes (pyopenvino_amd.warp has helpers:
    ``invert`` of a forward matrix, ``from_roi``, ``rotated_rect``, ``apply``).  `ids`: (n,) integers in [0, m), the frame each row
    reads; None: row b reads frame b when m == n and frame 0 when m == 1.  The device samples every row bilinearly in one launch
    (pvhip_input_preprocess_warp_f32; the rule in numpy: tests/warp_ref.py): the coefficients are quantised to Q16 on the host
    (``WarpInput.fixed``), coordinates are 64-bit integers, a tap outside the frame has the value ``preprocess_info.pad_value`` in
    every channel (in source units: it goes through mean / scale like a pixel), no antialiasing; then reversal and mean / scale as
    declared.  A zero fraction reads no second tap, so an integer translation is a copy bit for bit and a mirror a reversed copy.  For
    the colour formats a pixel is the converted B, G, R with the chroma of its block of the frame.  The input needs
    ``preprocess_info.resize_algorithm = 'RESIZE_BILINEAR'``.  A declared ``resize_fit`` plays no part in a warp: the matrix places
    the pixels (``infer(..., detections=)`` on such an input refuses a WarpInput as it does a RoiInput).  ``warp.from_roi`` is NOT bit
    for bit a RoiInput at scales other than 1: a RoiInput's taps clamp at the rectangle's edge and its fractions are exact rationals,
    a warp's are Q16 and its border is the pad.  With `frames` = ``InferRequest.input_buffer(name, (h, w), frames=m)`` and `matrices`
    = ``InferRequest.warp_buffer(name)`` -- the (n, 7) int64 table (id, A00, A01, C0, A10, A11, C1) itself, `ids` None -- nothing
    is copied on the host."""
    __slots__ = ('frames', 'matrices', 'ids')
    MATRIX, COLUMNS, BUFFER = (2, 3), 7, 'warp'      # a row's matrix, its row of the table (id, A00 .. C1), InferRequest.warp_buffer
    LINEAR_LIMIT = 1 << 26           # |A| at most: a scale of 1024
    TRANSLATION_LIMIT = 1 << 40      # |C| at most: 2^24 pixels

    def __init__(self, frames, matrices, ids=None):
        self.frames, self.matrices, self.ids = frames, matrices, ids

    def __repr__(self):
        return 'WarpInput(frames={}, matrices={})'.format(getattr(self.frames, 'shape', None), getattr(self.matrices, 'shape', None))

    @classmethod
    def beyond_limits(cls, q, dst_hw=None):
        """Which rows of (n, 6) Q16 coefficients (A00, A01, C0, A10, A11, C1), int64 or float64, break a limit (whatever the extent
        `dst_hw`: PerspectiveInput's three operations take the same arguments and use it)."""
        a, c = q[:, [0, 1, 3, 4]], q[:, [2, 5]]               # (no np.abs: the smallest int64 has none)
        return ((a > cls.LINEAR_LIMIT) | (a < -cls.LINEAR_LIMIT)).any(1) | ((c > cls.TRANSLATION_LIMIT) | (c < -cls.TRANSLATION_LIMIT)).any(1)

    @staticmethod
    def limit_text(b, row, dst_hw=None):
        return ('matrices[{}] is beyond the limits of a warp -- finite, |a| <= 1024 for the four linear terms, |c| <= 2^24 for the '
                'translations --: in Q16 {}'.format(b, [float(v) for v in row]))

    @classmethod
    def fixed(cls, matrices, dst_hw=None) -> np.ndarray:
        """(n, 6) int64: the coefficients (a00, a01, c0, a10, a11, c1) of every row in Q16, ``np.rint(np.float64(v) * 65536)`` (ties to
        even), as the device takes them.  ValueError, naming the row, for a value that is not finite, |A| > 2^26 for a linear term or
        |C| > 2^40 for a translation: with these limits A00 x + A01 y + C0 cannot overflow int64 for any extent a launch admits.  Host
        arithmetic only: no device is needed."""
        t = np.asarray(matrices)
        if t.ndim != 3 or t.shape[1:] != (2, 3):
            raise ValueError('matrices has shape (n, 2, 3) -- one 2 x 3 matrix per batch row --, got {}'.format(t.shape))
        if t.dtype.kind not in 'fiu':
            raise ValueError('matrices holds real numbers, got dtype {}'.format(t.dtype))
        with np.errstate(invalid='ignore', over='ignore'):
            q = np.rint(t.astype(np.float64).reshape(-1, 6) * 65536.0)
        bad = ~np.isfinite(q).all(1)
        bad |= cls.beyond_limits(np.where(np.isfinite(q), q, 0.0))
        if bad.any():
            b = int(np.argmax(bad))
            raise ValueError(cls.limit_text(b, q[b]))
        return q.astype(np.int64)


class PerspectiveInput(FrameFeed):
    """A network input given as homographies of frames (a plate seen from the kerb, a document on a desk, a sign or a screen seen at an
    angle, a road or court plane rectified to a bird's-eye view: four corners in the frame, not a rotated rectangle):
    ``infer({name: PerspectiveInput(frames, matrices, ids)})``, wherever a WarpInput is accepted.  `frames` and `ids`: exactly as for
    WarpInput.  `matrices`: real numbers of shape (n, 3, 3); row b maps an OUTPUT pixel index (x, y) of the network's extent to a SOURCE
    position in frame pixels, sx = (h00 x + h01 y + h02) / (h20 x + h21 y + h22), sy = (h10 x + h11 y + h12) / (the same denominator),
    pixel centres at the integers: the matrix ``cv2.warpPerspective(..., flags=INTER_LINEAR | WARP_INVERSE_MAP)`` takes
    (pyopenvino_amd.perspective has helpers: ``from_quad`` of four frame points, ``from_affine``, ``invert`` of a forward matrix,
    ``apply``).  The device samples every row bilinearly in one launch (pvhip_input_preprocess_perspective_f32; the rule in numpy:
    tests/perspective_ref.py): each matrix is scaled by a power of two of its own and rounded to integers on the host
    (``PerspectiveInput.fixed``: the ratio does not see the scale), the three linear forms are exact 64-bit integers below 2^52, the
    position in Q16 is floor(N / D * 65536) with ONE correctly rounded binary64 division per axis, and from there on the rule is
    WarpInput's word for word: a tap outside the frame has the value ``preprocess_info.pad_value``, a zero fraction reads no second
    tap, colour frames are converted per tap, then reversal and mean / scale as declared.  A pixel whose denominator is 0 (the
    horizon of the map) or whose position is beyond 2^31 pixels is the pad; a negative denominator is a legal one: -H is the same map
    as H.  No antialiasing.  The input needs ``preprocess_info.resize_algorithm = 'RESIZE_BILINEAR'``; a declared ``resize_fit`` plays
    no part, and ``infer(..., detections=)`` refuses a PerspectiveInput wherever it refuses a WarpInput.  With `frames` =
    ``InferRequest.input_buffer(name, (h, w), frames=m)`` and `matrices` = ``InferRequest.perspective_buffer(name)`` -- the (n, 10)
    int64 table (id, Q00, Q01, Q02, Q10, Q11, Q12, Q20, Q21, Q22) itself, `ids` None -- nothing is copied on the host."""
    __slots__ = ('frames', 'matrices', 'ids')
    MATRIX, COLUMNS, BUFFER, KIND = (3, 3), 10, 'perspective', 'perspective'     # (id, Q00 .. Q22), InferRequest.perspective_buffer
    FORM_LIMIT = 1 << 52             # |Q_r0| (wd - 1) + |Q_r1| (hd - 1) + |Q_r2| at most, for each row r of a matrix

    def __init__(self, frames, matrices, ids=None):
        self.frames, self.matrices, self.ids = frames, matrices, ids

    def __repr__(self):
        return 'PerspectiveInput(frames={}, matrices={})'.format(getattr(self.frames, 'shape', None), getattr(self.matrices, 'shape', None))

    @classmethod
    def beyond_limits(cls, q, dst_hw):
        """Which rows of (n, 9) integer coefficients (Q00 .. Q22) break the limit over an extent `dst_hw` = (hd, wd): a bound on one of
        the three linear forms above 2^52.  Python ints: no int64 of a table overflows here."""
        hd, wd = (int(v) for v in dst_hw)
        bad = np.zeros(len(q), bool)
        for b, row in enumerate(np.asarray(q).reshape(-1, 9).tolist()):
            bad[b] = any(abs(row[r]) * (wd - 1) + abs(row[r + 1]) * (hd - 1) + abs(row[r + 2]) > cls.FORM_LIMIT for r in (0, 3, 6))
        return bad

    @staticmethod
    def limit_text(b, row, dst_hw):
        return ('matrices[{}] is beyond the limit of a perspective table -- |Q_r0| (w - 1) + |Q_r1| (h - 1) + |Q_r2| <= 2^52 for each of '
                'its three rows r over the extent {} --: {}'.format(b, tuple(int(v) for v in dst_hw), [int(v) for v in row]))

    @classmethod
    def fixed(cls, matrices, dst_hw) -> np.ndarray:
        """(n, 9) int64: the coefficients (h00 .. h22) of every row as the device takes them over an extent `dst_hw` = (hd, wd), each
        matrix scaled by one power of two of its own: with B_r = |h_r0| (wd - 1) + |h_r1| (hd - 1) + |h_r2| for its three rows and
        B = max B_r in [2^(e-1), 2^e), Q = ``np.rint(np.float64(h) * 2^(51 - e))`` (ties to even).  Each of the three linear forms then
        stays below 2^52 in magnitude over the whole extent -- exact as int64 and as binary64 --, and the scale cancels in the ratio, so
        it is not stored.  ValueError, naming the row, for a matrix with a value that is not finite or with B == 0.  Host arithmetic
        only: no device is needed."""
        t = np.asarray(matrices)
        if t.ndim != 3 or t.shape[1:] != (3, 3):
            raise ValueError('matrices has shape (n, 3, 3) -- one 3 x 3 matrix per batch row --, got {}'.format(t.shape))
        if t.dtype.kind not in 'fiu':
            raise ValueError('matrices holds real numbers, got dtype {}'.format(t.dtype))
        hd, wd = (int(v) for v in dst_hw)
        if hd < 1 or wd < 1:
            raise ValueError('the extent {} is empty'.format((hd, wd)))
        h = t.astype(np.float64)
        with np.errstate(invalid='ignore', over='ignore'):
            bound = (np.abs(h) * np.array([wd - 1, hd - 1, 1], np.float64)).sum(2).max(1)
        bad = ~np.isfinite(bound) | (bound == 0) | ~np.isfinite(h).all((1, 2))
        if bad.any():
            b = int(np.argmax(bad))
            raise ValueError('matrices[{}] is no homography over the extent {} -- every value finite, and the largest of its three bounds '
                             '|h_r0| (w - 1) + |h_r1| (h - 1) + |h_r2| neither zero nor beyond binary64 --: {}'.format(
                                 b, (hd, wd), h[b].tolist()))
        e = np.frexp(bound)[1]
        q = np.rint(np.ldexp(h, (51 - e)[:, None, None])).reshape(-1, 9)
        return q.astype(np.int64)


class DetectedRois(FrameFeed):
    """A network input given as the regions another network detected (a cascade: detector, then classifier, both on this GPU):
    ``start_async({name: DetectedRois(frames, detections)})``, wherever a RoiInput is accepted.  `frames`: as for RoiInput.  `detections`:
    DetectionOutput records [rank, label, score, xmin, ymin, xmax, ymax] with normalised corners, as
      * the ``InferRequest`` of another loaded network whose Result (`output` names it when there are several) is a DetectionOutput: in
        flight, its device-resident Result is read with no host wait -- this request's stream waits for the detector's pass on the device
        --; waited for, its last host Results are taken like an array;
      * a ``device.DeviceTensor``, or a host array (uploaded behind the same event as the frames), float32 of shape (1, 1, R, 7) or (R, 7).
    `images` = N: the images the R records belong to (default: the detector's batch; for an array, the frame count m), R // N records
    each; image b's rectangles are cut from frame b, so N == m.  A record is used when it lies in front of its image's terminator, its
    score is >= `min_confidence`, its corners are finite, its label is one of `labels` (None: any; at most MAX_LABELS ints >= 0) and
    its rectangle -- floor / ceil of the corners scaled to the frame and clamped to it -- is at least `min_size` = (h, w).  The first n
    of them, in the order (image, position), become batch rows 0..count-1; the other rows are quiet NaN.  The table is made on the device
    (pvhip_detections_to_rois; the rule in numpy: tests/detected_rois_ref.py); ``InferRequest.detected_rois(name)`` reads it back.

    A detector whose input declares a fit (``preprocess_info.resize_fit``) saw the frame in a rectangle of its input: its corners are
    mapped back first (pvhip_detections_to_rois_fit).  For a detector request the geometry is that of the pass it was last fed; for
    records given as a tensor or an array it is `detector_fit` = (Hn, Wn, dx, dy, iw, ih), the detector's input extent and
    ``InputFormat.fit_geometry`` of the frames it was fed (None: no fit).

    The detector may be started again as soon as ``start_async`` of this input has returned: its next pass waits, on the device, until
    the table has been made.  ``detector.wait()`` may come before or after that ``start_async``."""
    __slots__ = ('frames', 'detections', 'output', 'images', 'min_confidence', 'labels', 'min_size', 'detector_fit')
    HOW, RECTANGLES, KIND = RoiInput.HOW, True, 'roi'
    MAX_LABELS = 64

    def __init__(self, frames, detections, output=None, images=None, min_confidence=0.5, labels=None, min_size=(1, 1), detector_fit=None):
        self.frames, self.detections, self.output, self.images = frames, detections, output, images
        self.min_confidence, self.labels, self.min_size, self.detector_fit = min_confidence, labels, min_size, detector_fit

    def __repr__(self):
        return 'DetectedRois(frames={}, detections={})'.format(getattr(self.frames, 'shape', None), type(self.detections).__name__)

    def checked_options(self, name):
        """(min_confidence as a float, labels as an int32 array or None, (min_h, min_w)) for input `name`, or ValueError."""
        conf, labels, size = self.min_confidence, self.labels, self.min_size
        if isinstance(conf, bool) or not isinstance(conf, (int, float, np.integer, np.floating)) or conf != conf:
            raise ValueError('input {}: min_confidence {!r} is not a real number'.format(name, conf))
        if labels is not None:
            labels = np.asarray(labels)
            if labels.ndim != 1 or labels.dtype.kind not in 'iu' or len(labels) > self.MAX_LABELS or (labels.astype(np.int64) < 0).any() \
                    or (labels > np.iinfo(np.int32).max).any():
                raise ValueError('input {}: labels is None or at most {} ints >= 0, got {!r}'.format(name, self.MAX_LABELS, self.labels))
            labels = labels.astype(np.int32)
        try:
            ok = len(size) == 2 and all(not isinstance(v, bool) and isinstance(v, (int, np.integer)) and 1 <= v <= np.iinfo(np.int32).max for v in size)
        except TypeError:
            ok = False
        if not ok:
            raise ValueError('input {}: min_size is (h, w) with both >= 1, got {!r}'.format(name, size))
        return float(conf), labels, (int(size[0]), int(size[1]))

    def checked_records(self, name, shape, dtype, images, frames):
        """The records per image P of detections of `shape` and `dtype` over `images` images, cut from `frames` frames; or ValueError."""
        if np.dtype(dtype) != np.float32 or len(shape) not in (2, 4) or shape[-1] != 7 or tuple(shape[:-2]) not in ((), (1, 1)) or shape[-2] < 1:
            raise ValueError('input {}: detections are float32 records of shape (1, 1, R, 7) or (R, 7), got {} {}'.format(
                name, np.dtype(dtype).name, tuple(shape)))
        if isinstance(images, bool) or not isinstance(images, (int, np.integer)) or images < 1:
            raise ValueError('input {}: images is a count >= 1, not {!r}'.format(name, images))
        if images != frames:
            raise ValueError('input {}: image b\'s rectangles are cut from frame b: {} images need {} frames, got {}'.format(
                name, images, images, frames))
        if shape[-2] % images:
            raise ValueError('input {}: {} records do not divide over {} images'.format(name, shape[-2], images))
        if shape[-2] * 7 >= 2 ** 31:
            raise ValueError('input {}: {} records are more than one launch indexes'.format(name, shape[-2]))
        return int(shape[-2]) // int(images)


class LandmarkWarps(FrameFeed):
    """A network input given as crops aligned by the points another network found (a cascade: detector, crops, a landmark regressor on
    the crops, then the aligned crop into a recognition or attribute network, all on this GPU):
    ``start_async({name: LandmarkWarps(frames, landmarks, template)})``, wherever a WarpInput is accepted, for every declared host
    format.  `frames`: as for WarpInput; this request uploads them, as a DetectedRois uploads its own.  `template`: (K, 2) real numbers,
    2 <= K <= 32; point i is the place (x, y) landmark i shall land at, in output pixel indices of this input's extent, pixel centres
    at the integers.  `landmarks`: K points per row, float32 of shape (N, 2 K) or (N, 2 K, 1, 1) as x0, y0, x1, y1, ..., normalised to
    the region the landmark network saw -- 0 its left or top edge, 1 its right or bottom edge --, as
      * the ``InferRequest`` of another loaded network whose Result (`output` names it when there are several) has that shape: in flight,
        its device-resident Result is read with no host wait -- this request's stream waits for the landmark pass on the device --;
        waited for, its last host Results are taken like an array;
      * a ``device.DeviceTensor``, or a host array (uploaded behind the same event as the frames).
    `regions`: the (id, x, y, w, h) each row of points is normalised to.  None: for a request whose single 4-D Parameter was last fed a
    ``RoiInput`` or a ``DetectedRois``, that pass's (N, 5) table, still on the device; for a request last fed whole images, and for
    tensors and arrays, the whole frame -- row b reads frame b (m == N) or frame 0 (m == 1).  Or an integer (N, 5) array, uploaded
    behind the frames' event.
    The (n, 7) table of a WarpInput is fitted on the device (pvhip_landmarks_to_warps; the rule in Python floats:
    pyopenvino_amd/landmarks.py, in numpy: tests/landmark_warps_ref.py): row b is the least-squares similarity, without reflection,
    from the template's points to row b's landmarks in frame pixels, in binary64 with every operation rounded once -- directly the
    inverse map a warp takes.  It is NOT ``warp.invert(cv2.estimateAffinePartial2D(landmarks -> template))``: that call minimises in the
    template's space, this fit in the frame's; the two agree where the fit is exact.  A row is void -- quiet NaN in the input tensor --
    when it lies behind the N rows of points, its region's id is none of the m frames, its region's w or h is outside [1, 2^24] (the
    rows behind a DetectedRois' count), one of its 2 K values is not finite, the fitted matrix breaks a WarpInput's limits, or all its
    points coincide.  ``InferRequest.landmark_warps(name)`` reads the table back.  From there on the pass is a WarpInput's word for word.

    The landmark request may be started again as soon as ``start_async`` of this input has returned: its next pass waits, on the device,
    until the table has been fitted -- of its Result and of its region table alike.  This input keeps that Result tensor alive until its
    own next pass, so the landmark request's next pass writes another one; a request records its pass for replay only when that
    allocates nothing new, so let the landmark request run a few passes on its own before the chain starts (as a DetectedRois'
    detector: scripts/bench_landmark_warps.py does).  ValueError for a landmark request whose 4-D input
    declares a ``resize_fit`` other than STRETCH (the points would need its geometry) or was last fed a WarpInput, a PerspectiveInput or
    a LandmarkWarps (no rectangle to be normalised to)."""
    __slots__ = ('frames', 'landmarks', 'template', 'output', 'regions')

    def __init__(self, frames, landmarks, template, output=None, regions=None):
        self.frames, self.landmarks, self.template, self.output, self.regions = frames, landmarks, template, output, regions

    def __repr__(self):
        return 'LandmarkWarps(frames={}, landmarks={})'.format(getattr(self.frames, 'shape', None), type(self.landmarks).__name__)

    def checked_template(self, name) -> np.ndarray:
        """``landmarks.packed_template(template)`` for input `name`: the 2 K + 3 doubles the device takes; or ValueError."""
        try:
            return landmark_rule.packed_template(self.template)
        except ValueError as e:
            raise ValueError('input {}: {}'.format(name, e)) from None

    @staticmethod
    def checked_points(name, shape, dtype, k) -> int:
        """The row count N of points of `shape` and `dtype` for a template of `k` points; or ValueError."""
        if np.dtype(dtype) != np.float32 or len(shape) not in (2, 4) or shape[0] < 1 or tuple(shape[2:]) not in ((), (1, 1)):
            raise ValueError('input {}: landmarks are float32 points of shape (N, 2 K) or (N, 2 K, 1, 1), got {} {}'.format(
                name, np.dtype(dtype).name, tuple(shape)))
        if shape[1] != 2 * k:
            raise ValueError('input {}: landmarks of shape {} hold {} values per row, the template of {} points needs {}'.format(
                name, tuple(shape), shape[1], k, 2 * k))
        return int(shape[0])

    def checked_regions(self, name, rows):
        """`regions` as a C-contiguous int32 (rows, 5) array, or None when none is given; or ValueError."""
        if self.regions is None:
            return None
        t = np.asarray(self.regions)
        if t.shape != (rows, 5) or t.dtype.kind not in 'iu':
            raise ValueError('input {}: regions is an integer table of shape {} -- one (id, x, y, w, h) per row of landmarks --, got {} {}'.format(
                name, (rows, 5), t.dtype, t.shape))
        lo, hi = np.iinfo(np.int32).min, np.iinfo(np.int32).max
        if t.size and (int(t.min()) < lo or int(t.max()) > hi):
            raise ValueError('input {}: regions holds 32-bit integers, got values in [{}, {}]'.format(name, int(t.min()), int(t.max())))
        return np.ascontiguousarray(t, np.int32)


# what InferRequest.landmark_warps returns: how many rows of the pass were valid, which ones ((n,) bool), and the (n, 7) int64 table
# (id, A00, A01, C0, A10, A11, C1) the pass used, void rows being (-1, 0, 0, 0, 0, 0, 0)
LandmarkTable = collections.namedtuple('LandmarkTable', 'count valid table')


# what InferRequest.detected_rois returns: the (n, 5) int32 table the pass used, the flat row of the detections each batch row came from
# (-1 from row `count` on), how many records passed the screen (`selected`, which may exceed n) and count = min(selected, n)
DetectedTable = collections.namedtuple('DetectedTable', 'count selected rois records')


class InputInfo:
    """The format a caller hands one network input in (OpenVINO 2021's ``IENetwork.input_info[name]``): ``precision`` 'FP32' (default)
    or 'U8', ``layout`` 'NCHW' (default) or 'NHWC'.  A U8 value v means float(v); an NHWC array is ``x.transpose(0, 3, 1, 2)`` of the NCHW
    tensor the IR expects -- a cv2 image as it is, where the reference's callers hand ``img.transpose((2, 0, 1)).astype(np.float32)``.
    Set between ``read_network`` and ``load_network``.  A declared input is uploaded as it is and converted on the device
    (``pvhip_input_to_nchw_f32``); an input whose format is never set goes the default way.  ``preprocess_info`` adds a resize of a source
    of any extent, channel reversal and mean / scale to that launch (``pvhip_input_preprocess_f32``); its ``color_format`` 'NV12' /
    'I420' makes the array a decoder's YUV 4:2:0 frames, uint8 of shape (n, 3 h / 2, w), converted to B, G, R in that launch
    (``pvhip_input_preprocess_yuv_f32``), 'YUY2' / 'UYVY' a camera's packed YUV 4:2:2 frames, uint8 of shape (n, h, w, 2), and 'BGRX' /
    'RGBX' a screen capture's four-byte pixels, uint8 of shape (n, h, w, 4) (``pvhip_input_preprocess_packed_f32``); its
    ``color_standard`` / ``color_range`` say which matrix and range the YUV frames were encoded with (the ``_color_f32`` forms)."""
    PRECISIONS = ('FP32', 'U8')
    LAYOUTS = ('NCHW', 'NHWC')

    def __init__(self, net, nid):
        self._net, self._nid = net, nid
        self._precision, self._layout = 'FP32', 'NCHW'
        self.declared = False           # precision or layout set explicitly (to any value)
        self._precision_set = False     # precision set explicitly: 'FP32' then contradicts a color_format other than 'RAW'
        self._pre = None                # PreProcessInfo, once preprocess_info has been asked for

    @property
    def name(self):
        return self._net.G.nodes[self._nid]['name']

    @property
    def dims(self):
        """The NCHW shape of the tensor the IR expects."""
        return tuple(int(d) for d in self._net.G.nodes[self._nid]['data']['shape'])

    def supported(self):
        """Declared formats exist for 4-D Parameters whose element type is f32 (FP16 IRs read with fp16_as_fp32 are, once promoted)."""
        data = self._net.G.nodes[self._nid]['data']
        return len(tuple(data['shape'])) == 4 and str(data.get('element_type', '')).lower() == 'f32'

    @property
    def precision(self):
        return self._precision

    @precision.setter
    def precision(self, value):
        self._precision = self._checked('precision', value, self.PRECISIONS)
        self._precision_set = True

    @property
    def layout(self):
        return self._layout

    @layout.setter
    def layout(self, value):
        self._layout = self._checked('layout', value, self.LAYOUTS)

    def _checked(self, what, value, allowed):
        self._check_not_loaded(what)
        if not isinstance(value, str) or value.upper() not in allowed:
            raise ValueError('input {}: {} {!r} is not one of {}'.format(self.name, what, value, allowed))
        self._declare(what)
        return value.upper()

    def _check_not_loaded(self, what):
        if self._net._loaded:
            raise ValueError('input {}: set input_info[...].{} between read_network and load_network, not after'.format(self.name, what))

    def _declare(self, what):
        """A valid value of `what` is being set: refused after load_network and for inputs without declared formats; else the input is
        declared from now on."""
        self._check_not_loaded(what)
        if not self.supported():
            self._unsupported(what)
        self.declared = True

    def _unsupported(self, what):
        data = self._net.G.nodes[self._nid]['data']
        raise NotImplementedError('input {}: a declared {} needs a 4-D f32 Parameter; this one is {} {}'.format(
            self.name, what, data.get('element_type'), tuple(data['shape'])))

    @property
    def preprocess_info(self):
        """The preprocessing the device applies to this input (OpenVINO 2021's ``input_info[name].preprocess_info``): PreProcessInfo."""
        if not self.supported():
            self._unsupported('preprocess_info')
        if self._pre is None:
            self._pre = PreProcessInfo(self)
        return self._pre

    def frozen(self) -> InputFormat:
        """The format as declared now, as a fixed value (load_network takes it once the setters refuse)."""
        pre, mean, std = self._pre, None, None
        if pre is not None and pre.mean_variant == 'MEAN_VALUE':
            mean = np.array([ch.mean_value for ch in pre._channels], np.float32)
            std = np.array([ch.std_scale for ch in pre._channels], np.float32)
        color = pre.color_format if pre is not None else 'RAW'
        return InputFormat(self.name, self.dims, self.supported(), self.declared, self._precision == 'U8' or color != 'RAW', self._layout == 'NHWC',
                           pre is not None and pre.resize_algorithm == 'RESIZE_BILINEAR', pre is not None and pre.reverse_channels, mean, std,
                           color, pre.resize_fit if pre is not None else 'STRETCH', pre.pad_value if pre is not None else 0.0,
                           pre.color_standard if pre is not None else 'BT601', pre is not None and pre.color_range == 'FULL')

    def preprocessing(self):
        """(resize, reverse_channels, (mean, std_scale) or None) as declared; (False, False, None) when nothing is."""
        f = self.frozen()
        return f.resize, f.reverse, (f.mean, f.std) if f.mean is not None else None

    def _check_at_load(self):
        pre = self._pre
        if pre is not None and pre.mean_variant == 'MEAN_VALUE' and len(pre._channels) != self.dims[1]:
            raise ValueError('input {}: mean_variant MEAN_VALUE with {} channels (preprocess_info.init), the input has {}'.format(
                self.name, len(pre._channels), self.dims[1]))
        if pre is not None and pre.resize_fit != 'STRETCH' and pre.resize_algorithm != 'RESIZE_BILINEAR':
            raise ValueError('input {}: resize_fit {} places a resized source: it needs preprocess_info.resize_algorithm = '
                             '\'RESIZE_BILINEAR\''.format(self.name, pre.resize_fit))
        if pre is not None and pre.color_format not in YUV_FORMATS and (pre.color_standard, pre.color_range) != ('BT601', 'LIMITED'):
            raise ValueError('input {}: color_standard {} / color_range {} say how YUV frames were encoded; color_format {} holds nothing to '
                             'convert'.format(self.name, pre.color_standard, pre.color_range, pre.color_format))
        if pre is not None and pre.color_format != 'RAW':
            if self.dims[1] != 3:
                raise ValueError('input {}: color_format {} converts to 3 channels (B, G, R), the input has {}'.format(
                    self.name, pre.color_format, self.dims[1]))
            if self._precision_set and self._precision != 'U8':
                raise ValueError('input {}: color_format {} frames are U8, precision {} is declared'.format(
                    self.name, pre.color_format, self._precision))
            if pre.resize_algorithm == 'NO_RESIZE':
                self.frozen().checked_extent()     # the frames have the network's extent: a legal one for the format (even; 4:2:2: even w)

    def source_extent(self, source_size=None):
        """The (h, w) a caller's array has: `source_size` with RESIZE_BILINEAR declared, else the network's own."""
        return self.frozen().checked_extent(source_size)

    def host_format(self, source_size=None, frames=None):
        """(shape, dtype) of the array a caller hands in this format; with RESIZE_BILINEAR declared, `source_size` = (h, w) of the source
        (default: the network's extent) and `frames` = m: of the m frames of a RoiInput."""
        f = self.frozen()
        if frames is not None:
            frames = f.checked_frames(frames)
        return f.host_shape(f.checked_extent(source_size), frames), f.host_dtype


class PreProcessChannel:
    """One channel of PreProcessInfo: ``mean_value`` (default 0) and ``std_scale`` (default 1, never 0)."""

    def __init__(self, owner, index):
        self._owner, self._index = owner, index
        self._mean, self._std = 0.0, 1.0

    @property
    def mean_value(self):
        return self._mean

    @mean_value.setter
    def mean_value(self, value):
        value = self._owner._number('mean_value', value)
        self._owner._info._declare('preprocess_info[c].mean_value')
        self._mean = value

    @property
    def std_scale(self):
        return self._std

    @std_scale.setter
    def std_scale(self, value):
        value = self._owner._number('std_scale', value)
        if value == 0:
            raise ValueError('input {}: std_scale of channel {} is 0 in fp32'.format(self._owner._info.name, self._index))
        self._owner._info._declare('preprocess_info[c].std_scale')
        self._std = value


class PreProcessInfo:
    """What the device does to an input before the network reads it (OpenVINO 2021's PreProcessInfo; pvhip_input_preprocess_f32, in one
    launch with the format change of ``precision`` / ``layout``):
      * ``resize_algorithm``: 'NO_RESIZE' (default) or 'RESIZE_BILINEAR' -- a source of any (h, w) is resized to the Parameter's extent
        (half-pixel centres, clamped at the border, as cv2 INTER_LINEAR; no antialiasing, so large downscales alias); a source at the
        network's own extent is not resized at all;
      * ``resize_fit``: 'STRETCH' (default: the source is stretched onto the whole extent whatever its shape) or 'LETTERBOX' /
        'TOP_LEFT' (OpenVINO Model API's ``fit_to_window_letterbox`` / ``fit_to_window``): the source is scaled by ONE factor into the
        rectangle (dx, dy, iw, ih) of ``InputFormat.fit_geometry`` -- integers only: the long side full, the short side rounded half up,
        centred (floor) for LETTERBOX, at the origin for TOP_LEFT -- by the same bilinear rule onto (ih, iw), and the rest of the extent
        is ``pad_value`` (one finite fp32 number in source units, default 0; it goes through mean / scale like a pixel).  Needs
        RESIZE_BILINEAR.  ``infer(..., detections=)`` and ``DetectedRois`` map a fitted detector's boxes back to the frame;
      * ``reverse_channels``: output channel c takes source channel C-1-c (a BGR frame into an RGB-trained IR);
      * ``mean_variant``: 'NONE' (default) or 'MEAN_VALUE': y = (v - self[c].mean_value) / self[c].std_scale, after ``init(C)``;
      * ``color_format``: 'RAW' (default: the array holds the channels themselves) or 'NV12' / 'I420': the array holds YUV 4:2:0 frames as a
        video decoder writes them and ``cv2.cvtColor(..., COLOR_YUV2BGR_NV12 / _I420)`` takes them -- uint8 of shape (n, 3 h / 2, w), h and
        w even: h rows of Y, then for NV12 h / 2 rows of w / 2 interleaved (U, V) pairs, for I420 the U plane and the V plane of
        h / 2 x w / 2 bytes each.  The device converts them to B, G, R (BT.601 limited range in 20-bit integers unless ``color_standard`` /
        ``color_range`` say otherwise, the chroma of a pixel's 2 x 2 block; pvhip_input_preprocess_yuv_f32) and resizes, reverses (R, G, B) and scales that image as it does a U8 B, G, R one.
        Or 'YUY2' / 'UYVY' / 'BGRX' / 'RGBX': the array holds frames of 4-byte units, converted by pvhip_input_preprocess_packed_f32
        (the same rule in numpy: tests/packed_ref.py):
          - YUY2 / UYVY (packed YUV 4:2:2, a camera's or a capture card's frames): uint8 of shape (n, h, w, 2), the (h, w, 2) array
            ``cv2.cvtColor(..., COLOR_YUV2BGR_YUY2 / _UYVY)`` takes; w even, h any value >= 1.  Each row is w / 2 groups of 4 bytes:
            Y0 U Y1 V for YUY2, U Y0 V Y1 for UYVY.  Pixel (y, x) has luma Y[x & 1] of group x // 2 of row y, and that group's (U, V):
            chroma is not interpolated.  Each pixel goes to B, G, R by exactly the integer rule of NV12 / I420 (BT.601 limited range
            over 2^20, arithmetic shifts, clamp to [0, 255]): the same function, not a second set of constants.
          - BGRX / RGBX (four-byte pixels, a screen capture's or a read-back's frames): uint8 of shape (n, h, w, 4), any h, w >= 1.
            The B, G, R image is ``frames[..., 0:3]`` for BGRX and ``frames[..., 2::-1]`` for RGBX; byte 3 is never read into the
            result, whatever it holds.
        The resulting uint8 B, G, R image is resized, reversed (R, G, B) and scaled bit for bit as a U8 NHWC source is.  The rectangle
        of a RoiInput is the crop of the converted frame: a 4:2:2 pixel keeps the chroma of its absolute column pair, so rectangles
        may start on odd x and have odd w.
      * ``color_standard``: 'BT601' (default), 'BT709' or 'BT2020', and ``color_range``: 'LIMITED' (default: Y in [16, 235], chroma in
        [16, 240]) or 'FULL' (JFIF: all of [0, 255]): the matrix and range the frames of a YUV ``color_format`` were encoded with -- BT.601
        for SD video, BT.709 for HD (a 1080p decoder's frames), BT.2020 for 8-bit HEVC / AV1 streams that say so; FULL for MJPEG webcams
        and JPEG decoders.  One integer rule converts all six (include/pvhip.h has its table, tests/colorimetry_ref.py is the rule in
        numpy): y = max(Y - yoff, 0), t = y CY + 2^19, B = (t + CBU u) >> 20, G = (t - CGV v - CGU u) >> 20, R = (t + CRV v) >> 20, clamped,
        the constants rint(x 2^20) of the standard's matrix; 'BT601' / 'LIMITED' keeps cv2's three-decimal constants bit for bit.  The
        chroma a pixel takes and everything behind the conversion stay as they are, for every way of feeding the input (arrays,
        ``input_buffer``, RoiInput, DetectedRois, WarpInput, a declared fit).  Anything but the defaults beside 'RAW', 'BGRX' or 'RGBX'
        is refused at load: there is nothing to convert.
        For every format but 'RAW' the Parameter has 3 channels; ``precision`` is U8 by implication ('FP32' declared beside it is
        refused at load), ``layout`` is not consulted; without a declared resize the network's own extent must be legal for the format.
    Set between ``read_network`` and ``load_network``, like ``precision``; setting anything makes the input declared."""
    RESIZE_ALGORITHMS = ('NO_RESIZE', 'RESIZE_BILINEAR')
    MEAN_VARIANTS = ('NONE', 'MEAN_VALUE')
    COLOR_FORMATS = ('RAW', 'NV12', 'I420', 'YUY2', 'UYVY', 'BGRX', 'RGBX')
    RESIZE_FITS = tuple(RESIZE_FITS)
    COLOR_STANDARDS = tuple(COLOR_STANDARDS)
    COLOR_RANGES = tuple(COLOR_RANGES)

    def __init__(self, info):
        self._info = info
        self._resize, self._mean_variant, self._reverse, self._color = 'NO_RESIZE', 'NONE', False, 'RAW'
        self._standard, self._range = 'BT601', 'LIMITED'
        self._fit, self._pad = 'STRETCH', 0.0
        self._channels = []

    @property
    def resize_algorithm(self):
        return self._resize

    @resize_algorithm.setter
    def resize_algorithm(self, value):
        self._resize = self._info._checked('preprocess_info.resize_algorithm', value, self.RESIZE_ALGORITHMS)

    @property
    def resize_fit(self):
        return self._fit

    @resize_fit.setter
    def resize_fit(self, value):
        self._fit = self._info._checked('preprocess_info.resize_fit', value, self.RESIZE_FITS)

    @property
    def pad_value(self):
        """One finite fp32 number in source units (default 0) that goes through mean / scale like a pixel: what a declared
        ``resize_fit`` fills the extent outside the fitted rectangle with, and the value, in every channel, of a tap of a ``WarpInput`` or a
        ``PerspectiveInput`` outside its frame, and of a pixel a ``PerspectiveInput`` has no position for (there with or without a
        declared fit)."""
        return self._pad

    @pad_value.setter
    def pad_value(self, value):
        value = self._number('pad_value', value)
        self._info._declare('preprocess_info.pad_value')
        self._pad = value

    @property
    def mean_variant(self):
        return self._mean_variant

    @mean_variant.setter
    def mean_variant(self, value):
        self._mean_variant = self._info._checked('preprocess_info.mean_variant', value, self.MEAN_VARIANTS)

    @property
    def color_format(self):
        return self._color

    @color_format.setter
    def color_format(self, value):
        self._color = self._info._checked('preprocess_info.color_format', value, self.COLOR_FORMATS)

    @property
    def color_standard(self):
        return self._standard

    @color_standard.setter
    def color_standard(self, value):
        self._standard = self._info._checked('preprocess_info.color_standard', value, self.COLOR_STANDARDS)

    @property
    def color_range(self):
        return self._range

    @color_range.setter
    def color_range(self, value):
        self._range = self._info._checked('preprocess_info.color_range', value, self.COLOR_RANGES)

    @property
    def reverse_channels(self):
        return self._reverse

    @reverse_channels.setter
    def reverse_channels(self, value):
        if not isinstance(value, (bool, np.bool_)):
            raise ValueError('input {}: preprocess_info.reverse_channels {!r} is not a bool'.format(self._info.name, value))
        self._info._declare('preprocess_info.reverse_channels')
        self._reverse = bool(value)

    def init(self, num_channels: int):
        """num_channels channels of mean 0 and scale 1 (MEAN_VALUE needs as many as the input has)."""
        if isinstance(num_channels, bool) or not isinstance(num_channels, (int, np.integer)) or num_channels < 1:
            raise ValueError('input {}: preprocess_info.init({!r}) needs a channel count >= 1'.format(self._info.name, num_channels))
        self._info._declare('preprocess_info.init')
        self._channels = [PreProcessChannel(self, k) for k in range(int(num_channels))]

    def __len__(self):
        return len(self._channels)

    def __getitem__(self, index):
        if not isinstance(index, (int, np.integer)) or not 0 <= index < len(self._channels):
            raise IndexError('input {}: preprocess_info[{!r}]: {} channels (preprocess_info.init)'.format(self._info.name, index, len(self._channels)))
        return self._channels[index]

    def _number(self, what, value):
        """`value` as the fp32 number the device uses; finite in fp32, or ValueError (nothing is declared here: the setter does that once
        every check has passed)."""
        ok = not isinstance(value, bool) and isinstance(value, (int, float, np.integer, np.floating))
        with np.errstate(over='ignore'):
            if not (ok and np.isfinite(np.float32(value))):
                raise ValueError('input {}: {} {!r} is not a finite fp32 number'.format(self._info.name, what, value))
        return float(np.float32(value))
