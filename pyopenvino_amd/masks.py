"""Instance masks (``infer(..., boxes=..., masks=...)``): the rule, the argument checks and the device launch.
Segmentation heads of the YOLOv8 / v11-seg, YOLOv5 / v7-seg and YOLACT family share one shape: a dense head whose anchors carry T mask
coefficients behind their classes -- (n, 4 + C + 32, 8400) or (n, 25200, 5 + C + 32), asked for with ``boxes=BoxScreen(..., tail=T)`` --
and a second Result of T prototype planes, (n, T, Hp, Wp), e.g. (n, 32, 160, 160), asked for with ``masks=``.  The head answers its
``Detections`` as ever; the prototype Result answers ``Masks``: one packed bit mask per row of those Detections.  Both tensors stay on the
device.

The rule (include/pvhip.h, pvhip_instance_masks_f32; tests/masks_ref.py is the same again in plain loops).  Row j of the head's Detections
is image r and anchor a = records[j] - r * A.  m[t] = e[4 + O + C + t] are the anchor's tail channels, p[t][q] the prototype planes of
image r at the flat pixel q = py * Wp + px.
  bit     L = fmaf(m[T-1], p[T-1][q], ... fmaf(m[0], p[0][q], +0) ...) in float32, t ascending, one rounding per step, subnormals kept
          (gallery.py's fmaf).  The bit is L > 0: sigmoid(L) > 0.5 without the transcendental.  A detection with a coefficient that is
          not finite has an empty mask; a pixel with any of its T prototype values not finite is 0 in every mask.
  crop    with crop=True, the default, the bit is also 0 outside the box.  xa, xb, ya, yb are the float32 corners of rule 2 of boxes.py,
          in network pixels (Hn, Wn), before any frame geometry; pixel (px, py) is inside iff xa * Wp <= px * Wn < xb * Wp and
          ya * Hp <= py * Hn < yb * Hp, the products in binary64, where they are exact (24-bit significands times extents of at most
          2^24).  crop=False skips this.
  layout  W32 = ceil(Hp * Wp / 32) uint32 words per row; pixel q is bit q & 31, least significant first, of word q >> 5; bits at and
          beyond Hp * Wp are 0.
Where this differs from Ultralytics: masks stay at prototype resolution and are thresholded there (Ultralytics upsamples, then
thresholds), and the crop compares exactly where Ultralytics scales float boxes by Wp / Wn.  Out of scope: areas or extents on the
device, FP16 Results, T above 64, YOLACT's own crop, masks behind a TiledScreen or RegionScreen.

MaskScreen(space='FRAME') answers ``FrameMasks`` instead: every kept box's mask in frame pixels over its own rectangle of
``Detections.rois`` -- the logits upsampled bilinearly to the frame the detector was fed, the letterbox removed, thresholded after the
upsampling (Ultralytics' process_mask with upsample, retina_masks).  The geometry (frame_size, fit = (dx, dy, iw, ih)) is the head's, as
boxes.Ask.bound binds it.  The rule (include/pvhip.h, pvhip_frame_masks_f32; tests/frame_masks_ref.py is the same again in plain loops),
for row j: image r, anchor a, rectangle (x, y, w, h), m[t] and p[t][q] as above:
  1. logits    L[q] is the fmaf chain above, t ascending from +0, float32.  A prototype pixel with any of its T values not finite has
     L[q] = NaN.  A detection with a coefficient that is not finite has an all-zero mask; its words are still written, as zeros.
  2. position  for frame column X in [x, x + w), in exact integers: N = (2 dx F + (2 X + 1) iw) Wp - F Wn and D = 2 F Wn with F = frame_w;
     P = floor(65536 N / D), floor toward minus infinity; x0 = P >> 16 (arithmetic), fx = float32(P & 65535) / 65536.  Rows alike with
     (dy, ih, frame_h, Hp, Hn).  This is the pixel centre X + 0.5 taken back through the inverse of the box rule's map t = (p - d) F / i
     and then to prototype coordinates u Wp / Wn - 0.5: align_corners=False, in one step from prototypes to frame.  The taps clamp:
     xa = clamp(x0, 0, Wp - 1), xb = clamp(x0 + 1, 0, Wp - 1); rows alike.
  3. value     t0 = L[ya][xa] + fx * (L[ya][xb] - L[ya][xa]), t1 likewise on row yb, v = t0 + fy * (t1 - t0): every operation float32
     rounded once, no fma; all four taps are always read; no special cases, NaN and inf follow IEEE.  The bit is v > 0.
  4. layout    Wr = ceil(w / 32).  Row j owns h * Wr words from offsets[j], the exclusive prefix sum in int64; pixel (X, Y) is bit
     (X - x) & 31, least significant first, of word offsets[j] + (Y - y) * Wr + ((X - x) >> 5); padding bits are 0.  A row whose
     rectangle is not inside the frame (x < 0, w < 1, x + w > frame_w, y alike) owns no words; the head never writes one.
  5. capacity  made is the largest m with offsets[m] <= max_words, used = offsets[made].  Rows from made on have no mask.
Where this differs from Ultralytics: there is one interpolation, straight through the letterbox geometry (Ultralytics upsamples to the
network's extent, cuts the padding, and resizes again); fractions are Q16; the crop is the integer rectangle of `rois`, not a float box.
Out of scope there: whole-frame masks (crop=False), areas, contours or polygons on the device, bicubic or antialiased resampling."""
import collections
import ctypes

import numpy as np

from . import ask, boxes, device
from .gallery import fmaf

MAX_TAIL = boxes.MAX_TAIL
MAX_PIXELS = 1 << 24
MAX_WORDS = 1 << 26                             # n * max_per_image * W32 at most
STAGE = 128                                     # PVHIP_MASKS_STAGE: tests place the counts around it
SPACES = ('PROTOTYPE', 'FRAME')
MAX_FRAME_WORDS = 1 << 28                       # max_words at most
MAX_FRAME_PLANE = 4096                          # Hp, Wp with space='FRAME'
MAX_FRAME_EXTENT = 16384                        # network and frame extents with space='FRAME': the integers of rule 2 stay below 2^59
MAX_FRAME_ROWS = 1 << 24                        # n * max_per_image with space='FRAME'
LDS_FLOATS, BAND_ROWS = 8192, 1024              # PVHIP_FRAME_MASKS_LDS_FLOATS, PVHIP_FRAME_MASKS_BAND_ROWS
FORM_NONE, FORM_ROW, FORM_PAIR = 0, 1, 2        # PVHIP_FRAME_MASKS_FORM_*

MaskScreen = collections.namedtuple('MaskScreen', 'head crop space max_words', defaults=(None, True, 'PROTOTYPE', 1 << 24))
MaskScreen.__doc__ = ('How to make the masks of a prototype Result: `head` names the Result asked for with boxes= in the same call whose '
                      'kept boxes get masks (None: the only one whose tail equals T); `crop`: bits outside a box are 0; `space`: '
                      '\'PROTOTYPE\' answers Masks at prototype resolution, \'FRAME\' answers FrameMasks in frame pixels, at most '
                      '`max_words` uint32 words of them (it sizes the blocks).')

FrameMasks = collections.namedtuple('FrameMasks', 'words offsets rois made')
FrameMasks.__doc__ = ('What a Result started with masks=MaskScreen(space=\'FRAME\') comes back as: `rois` (total, 5) int32, the head\'s '
                      'Detections.rois (image, x, y, w, h) in frame pixels; `offsets` (total + 1,) int64; `words` (used,) uint32, row j '
                      'owning h * ceil(w / 32) of them from offsets[j]; `made`: the leading rows whose masks are in `words`.  '
                      'unpack_frame() and paste() give the booleans.')

Masks = collections.namedtuple('Masks', 'words shape')
Masks.__doc__ = ('What a Result started with masks= comes back as: `words` (total, W32) uint32, row j the packed mask of row j of the '
                 'head\'s Detections; `shape` = (Hp, Wp).  unpack() gives the booleans.')


def unpack(answer) -> np.ndarray:
    """(total, Hp, Wp) bool of a Masks."""
    hp, wp = answer.shape
    words = np.ascontiguousarray(answer.words, '<u4')
    bits = np.unpackbits(words.view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder='little')
    return bits[:, :hp * wp].reshape(-1, hp, wp).astype(bool)


def unpack_frame(answer, j: int):
    """The (h, w) bool mask of row j of a FrameMasks, None for j >= made."""
    if not 0 <= j < answer.made:
        return None
    w, h = int(answer.rois[j, 3]), int(answer.rois[j, 4])
    words = np.ascontiguousarray(answer.words[int(answer.offsets[j]):int(answer.offsets[j + 1])], '<u4')
    if words.size == 0:                         # (a rectangle that is not inside the frame owns no words)
        return np.zeros((max(h, 0), max(w, 0)), bool)
    return np.unpackbits(words.view(np.uint8).reshape(h, -1), axis=1, bitorder='little')[:, :w].astype(bool)


def paste(answer, j: int, frame_hw):
    """The (H, W) bool frame with the mask of row j of a FrameMasks in place, None for j >= made."""
    mask = unpack_frame(answer, j)
    if mask is None:
        return None
    out = np.zeros((int(frame_hw[0]), int(frame_hw[1])), bool)
    if int(answer.offsets[j + 1]) > int(answer.offsets[j]):
        x, y = int(answer.rois[j, 1]), int(answer.rois[j, 2])
        out[y:y + mask.shape[0], x:x + mask.shape[1]] = mask
    return out


def frame_offsets(rois, frame_size) -> np.ndarray:
    """Rule 4's offsets, (total + 1,) int64, of `rois` (total, 5) over frames of `frame_size` = (H, W)."""
    t = np.asarray(rois, np.int64).reshape(-1, 5)
    x, y, w, h = (t[:, i] for i in range(1, 5))
    inside = (x >= 0) & (w >= 1) & (x + w <= int(frame_size[1])) & (y >= 0) & (h >= 1) & (y + h <= int(frame_size[0]))
    return np.concatenate([[0], np.cumsum(np.where(inside, h * ((w + 31) // 32), 0))]).astype(np.int64)


def taps(first: int, count: int, d: int, i: int, F: int, P: int, N: int):
    """Rule 2 for the frame positions first .. first + count - 1 of one axis: (a, b, f), the clamped taps and the float32 fractions."""
    out = [(((2 * d * F + (2 * X + 1) * i) * P - F * N) * 65536) // (2 * F * N) for X in range(first, first + count)]      # (Python's ints and floor)
    x0 = np.array([p >> 16 for p in out], np.int64).reshape(-1)
    f = np.array([p & 65535 for p in out], np.float32).reshape(-1) / np.float32(65536)
    return np.clip(x0, 0, P - 1), np.clip(x0 + 1, 0, P - 1), f


def make_frame(head, protos, found, screen, net_hw, frame_size, fit=None, max_words=1 << 24) -> FrameMasks:
    """The frame rule in numpy: `head` a host array read by the resolved BoxScreen `screen`, `protos` (n, T, Hp, Wp) float32, `found` the
    head's Detections over frames of `frame_size` = (H, W) that stand in the rectangle `fit` = (dx, dy, iw, ih) of the network's input
    (None: the identity), `net_hw` = (Hn, Wn)."""
    head, protos = np.asarray(head), np.asarray(protos)
    T = int(screen.tail)
    shape = boxes.shape_of(head.shape, screen.layout, screen.objectness, None, T)
    if head.dtype != np.float32 or shape is None or T < 1:
        raise ValueError('masks: the head is float32 of rank 3 with a tail of 1 .. {} channels, got {} {} tail {}'.format(MAX_TAIL, head.dtype, head.shape, T))
    layout, n, A, C = shape
    if protos.dtype != np.float32 or protos.ndim != 4 or protos.shape[:2] != (n, T) or protos.shape[2] * protos.shape[3] < 2:
        raise ValueError('masks: the prototypes are float32 (n, T, Hp, Wp) = ({}, {}, ..) with Hp * Wp >= 2, got {} {}'.format(n, T, protos.dtype, protos.shape))
    hp, wp = int(protos.shape[2]), int(protos.shape[3])
    hn, wn = (int(v) for v in net_hw)
    fh, fw = (int(v) for v in frame_size)
    dx, dy, iw, ih = (0, 0, wn, hn) if fit is None else boxes.checked_fit(fit, 'masks')
    _checked_frame(hp, wp, (hn, wn), (fh, fw), (dx, dy, iw, ih))
    max_words = _checked_max_words(max_words)
    rois = np.asarray(found.rois, np.int32).reshape(-1, 5)
    offsets = frame_offsets(rois, (fh, fw))
    made = int(np.searchsorted(offsets, max_words, side='right')) - 1
    words = np.zeros(int(offsets[made]), np.uint32)
    v = head.transpose(0, 2, 1) if layout == 'NCA' else head                               # (n, A, E)
    at = 4 + int(screen.objectness) + C
    for j in range(made):
        if offsets[j + 1] == offsets[j]:
            continue
        r, x, y, w, h = (int(c) for c in rois[j])
        m = v[r, int(found.records[j]) - r * A, at:at + T]
        if not np.isfinite(m).all():
            continue                                                                       # (zeros)
        xa, xb, fx = taps(x, w, dx, iw, fw, wp, wn)
        ya, yb, fy = taps(y, h, dy, ih, fh, hp, hn)
        x_lo, y_lo = int(xa[0]), int(ya[0])
        window = protos[r, :, y_lo:int(yb[-1]) + 1, x_lo:int(xb[-1]) + 1]                   # the taps ascend: the first and the last bound them
        with np.errstate(invalid='ignore', over='ignore', under='ignore'):
            L = np.zeros(window.shape[1:], np.float32)
            for t in range(T):
                L = fmaf(m[t], window[t], L)
            L = np.where(np.isfinite(window).all(axis=0), L, np.float32(np.nan))
            a, b, c, d = (L[np.ix_(rows - y_lo, cols - x_lo)] for rows in (ya, yb) for cols in (xa, xb))
            t0 = a + fx[None, :] * (b - a)
            t1 = c + fx[None, :] * (d - c)
            bit = (t0 + fy[:, None] * (t1 - t0)) > 0
        padded = np.zeros((h, 32 * ((w + 31) // 32)), np.uint8)
        padded[:, :w] = bit
        words[int(offsets[j]):int(offsets[j + 1])] = np.packbits(padded, axis=1, bitorder='little').view('<u4').reshape(-1)
    return FrameMasks(words, offsets, rois.copy(), made)


def _checked_max_words(value) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= value <= MAX_FRAME_WORDS:
        raise ValueError('masks: max_words is an int in 1 .. 2^28, got {!r}'.format(value))
    return int(value)


def _checked_frame(hp, wp, net_hw=None, frame=None, fit=None):
    """What space='FRAME' asks of the extents it knows; ValueError."""
    if max(hp, wp) > MAX_FRAME_PLANE:
        raise ValueError('masks: space=\'FRAME\' takes prototypes of at most 4096 x 4096, got {} x {}'.format(hp, wp))
    if net_hw is not None and (max(net_hw) > MAX_FRAME_EXTENT or (fit is not None and max(fit) > MAX_FRAME_EXTENT)):
        raise ValueError('masks: space=\'FRAME\' takes a network extent of at most 16384 x 16384, got {} x {}'.format(*net_hw))
    if frame is not None and max(frame) > MAX_FRAME_EXTENT:
        raise ValueError('masks: space=\'FRAME\' takes frames of at most 16384 x 16384, got {} x {}'.format(*frame))


def words_per_row(hp: int, wp: int) -> int:
    return (hp * wp + 31) // 32


def make(head, protos, found, screen, net_hw, crop=True) -> Masks:
    """The rule in numpy: `head` a host array read by the resolved BoxScreen `screen` (its layout, objectness, box and tail), `protos`
    (n, T, Hp, Wp) float32, `found` the head's Detections, `net_hw` = (Hn, Wn)."""
    head, protos = np.asarray(head), np.asarray(protos)
    T = int(screen.tail)
    shape = boxes.shape_of(head.shape, screen.layout, screen.objectness, None, T)
    if head.dtype != np.float32 or shape is None or T < 1:
        raise ValueError('masks: the head is float32 of rank 3 with a tail of 1 .. {} channels, got {} {} tail {}'.format(MAX_TAIL, head.dtype, head.shape, T))
    layout, n, A, C = shape
    if protos.dtype != np.float32 or protos.ndim != 4 or protos.shape[:2] != (n, T) or not 2 <= protos.shape[2] * protos.shape[3] <= MAX_PIXELS:
        raise ValueError('masks: the prototypes are float32 (n, T, Hp, Wp) = ({}, {}, ..) with 2 <= Hp * Wp <= 2^24, got {} {}'.format(n, T, protos.dtype, protos.shape))
    hp, wp = int(protos.shape[2]), int(protos.shape[3])
    hn, wn = (int(v) for v in net_hw)
    hw, w32, at = hp * wp, words_per_row(hp, wp), 4 + int(screen.objectness) + C
    v = head.transpose(0, 2, 1) if layout == 'NCA' else head                               # (n, A, E)
    r = np.asarray(found.rois[:, 0], np.int64)
    e = v[r, np.asarray(found.records, np.int64) - r * A]                                    # (total, E)
    m, planes = e[:, at:at + T], protos.reshape(n, T, hw)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        L = np.zeros((len(r), hw), np.float32)
        for t in range(T):
            L = fmaf(m[:, t:t + 1], planes[r, t], L)
        bit = (L > 0) & np.isfinite(m).all(axis=1)[:, None] & np.isfinite(planes).all(axis=1)[r]
        if crop:
            b = e[:, :4]
            if screen.box == 'CXCYWH':
                half_w, half_h = b[:, 2] * np.float32(0.5), b[:, 3] * np.float32(0.5)
                xa, xb, ya, yb = b[:, 0] - half_w, b[:, 0] + half_w, b[:, 1] - half_h, b[:, 1] + half_h
            else:
                xa, ya, xb, yb = (b[:, i] for i in range(4))
            xa, xb, ya, yb = (c.astype(np.float64)[:, None] for c in (xa, xb, ya, yb))
            q = np.arange(hw, dtype=np.int64)
            px, py = ((q % wp) * wn).astype(np.float64)[None, :], ((q // wp) * hn).astype(np.float64)[None, :]
            bit &= (xa * wp <= px) & (px < xb * wp) & (ya * hp <= py) & (py < yb * hp)
    padded = np.zeros((len(r), 32 * w32), np.uint8)
    padded[:, :hw] = bit
    return Masks(np.packbits(padded, axis=1, bitorder='little').view('<u4').astype(np.uint32).reshape(len(r), w32), (hp, wp))


def resolved(value, what='masks') -> MaskScreen:
    """`value` -- a MaskScreen or True -- checked; ValueError."""
    if value is True:
        value = MaskScreen()
    if not isinstance(value, MaskScreen):
        raise ValueError('{}: a MaskScreen or True, got {!r}'.format(what, value))
    if value.head is not None and not isinstance(value.head, str):
        raise ValueError('{}: head is None or the name of a Result asked for with boxes=, got {!r}'.format(what, value.head))
    if not isinstance(value.crop, (bool, np.bool_)):
        raise ValueError('{}: crop is a bool, got {!r}'.format(what, value.crop))
    if not isinstance(value.space, str) or value.space not in SPACES:
        raise ValueError('{}: space is \'PROTOTYPE\' or \'FRAME\', got {!r}'.format(what, value.space))
    if value.space == 'FRAME' and not value.crop:
        raise ValueError('{}: space=\'FRAME\' answers a box\'s own rectangle, which is the crop: crop=False is not taken'.format(what))
    return MaskScreen(value.head, bool(value.crop), value.space, _checked_max_words(value.max_words))


def shape_of(dims, batch=None):
    """(n, T, Hp, Wp) of a tensor declared as prototype planes -- rank 4, 1 <= T <= 64, 2 <= Hp * Wp <= 2^24, n the batch (when given)
    --, else None."""
    dims = tuple(int(d) for d in dims)
    if len(dims) != 4 or dims[0] < 1 or not 1 <= dims[1] <= MAX_TAIL or min(dims[2:]) < 1 or not 2 <= dims[2] * dims[3] <= MAX_PIXELS \
            or (batch is not None and dims[0] != int(batch)):
        return None
    return dims


SHAPE = 'rank 4 (n, T, Hp, Wp) with the batch n = {} first, 1 <= T <= 64 and 2 <= Hp * Wp <= 2^24'


def _fits(port, screen, batch):
    return port['precision'] == 'FP32' and shape_of(port['dims'], batch) is not None


def _none_fits(ports, screen, batch):
    return 'masks: no FP32 Result of {} (the Results: {})'.format(SHAPE.format(batch), {name: tuple(port['dims']) for name, port in ports.items()})


def checked(ienet, masks, heads: dict, sharded: bool) -> dict:
    """{prototype Result name: (resolved MaskScreen with `head` named, that head's BoxScreen, (T, Hp, Wp))} of the `masks` argument of
    infer() / start_async() -- a MaskScreen or True for every FP32 Result that shape_of takes, or {Result name: either} -- given
    `heads` = {Result name: resolved BoxScreen} of the same call's boxes=.  ValueError ('masks: ...'): no boxes= in the call, an unknown
    name, a sharded batch, a Result of another rank, precision, T or batch, a head not asked for or asked with another tail, several
    candidate heads and no head=, room for more than 2^26 words."""
    if not heads:
        raise ValueError('masks: the boxes whose masks these are come from boxes= in the same call, which names no Result')
    batch = int(ienet.batch_size)
    ports, wanted = ask.named(ienet, 'masks', masks, sharded, _fits, _none_fits, resolved)
    out = {}
    for name, screen in wanted.items():
        n, T, hp, wp = ask.declared('masks', name, ports[name], shape_of(ports[name]['dims'], batch), SHAPE, batch)
        if screen.head is None:
            fitting = sorted(h for h, s in heads.items() if s.tail == T)
            if len(fitting) != 1:
                raise ValueError('masks: Result {!r} has T = {} planes and boxes= asks for {} Results with tail = {} ({}): {}'.format(
                    name, T, len(fitting), T, {h: s.tail for h, s in heads.items()},
                    'head= names the one' if fitting else 'ask for the head with BoxScreen(tail={})'.format(T)))
            head = fitting[0]
        elif screen.head not in heads:
            raise ValueError('masks: Result {!r}: head {!r} is not asked for with boxes= (which asks for {})'.format(name, screen.head, sorted(heads)))
        elif heads[screen.head].tail != T:
            raise ValueError('masks: Result {!r} has T = {} planes and head {!r} is asked for with tail = {}'.format(
                name, T, screen.head, heads[screen.head].tail))
        else:
            head = screen.head
        if head == name:
            raise ValueError('masks: Result {!r} is asked for with boxes as well'.format(name))
        if screen.space == 'FRAME':
            _checked_frame(hp, wp, boxes.extent_of(ienet, heads[head].input), heads[head].frame_size)
            if n * heads[head].max_per_image > MAX_FRAME_ROWS:
                raise ValueError('masks: Result {!r}: {} x {} rows are more than 2^24: lower max_per_image of head {!r}'.format(
                    name, n, heads[head].max_per_image, head))
        words = n * heads[head].max_per_image * words_per_row(hp, wp)
        if screen.space != 'FRAME' and words > MAX_WORDS:
            raise ValueError('masks: Result {!r}: room for {} x {} masks of {} x {} is {} words, more than 2^26: lower max_per_image of head {!r}'.format(
                name, n, heads[head].max_per_image, hp, wp, words, head))
        out[name] = (screen._replace(head=head), heads[head], (T, hp, wp))
    return out


class Blocks:
    """The blocks of one (prototype Result, head's blocks): `words`, room for n * max_per_image rows of W32 words that
    pvhip_instance_masks_f32 writes, and its page-locked twin.  read_back: total from the header the head's own read_back has just
    copied -- wait() reads an ask behind the asks it needs --, then exactly 4 total W32 bytes."""
    __slots__ = ('n', 'per_image', 'shape', 'words', 'words_host', 'head')
    ENTRY = 'pvhip_instance_masks_f32'

    def __init__(self, n: int, per_image: int, shape):
        self.n, self.per_image, self.shape, self.head = n, per_image, shape, None
        w32 = words_per_row(shape[1], shape[2])
        self.words = device.DeviceTensor.empty((n * per_image, w32), np.uint32)
        self.words_host = device.host_empty((n * per_image, w32), np.uint32)

    def launch(self, protos, head_value, head_blocks, screen, net_hw, crop):
        """One launch on the current stream, behind the head's boxes call that has just written `head_blocks` there."""
        T, hp, wp = self.shape
        layout, n, A, C = boxes.shape_of(head_value.shape, screen.layout, screen.objectness, None, T)
        assert n == self.n and tuple(protos.shape) == (n, T, hp, wp) and protos.dtype == np.float32 and head_value.dtype == np.float32
        self.head = head_blocks
        device.call(self.ENTRY, device.ptr(head_value), n, A, 4 + int(screen.objectness) + C + T, boxes.LAYOUTS[layout], 4 + int(screen.objectness) + C, T,
                    boxes.BOXES[screen.box], device.ptr(protos), hp, wp, net_hw[0], net_hw[1], int(crop), self.per_image,
                    ctypes.c_void_p(head_blocks.header.ptr), ctypes.c_void_p(head_blocks.rows.ptr), ctypes.c_void_p(self.words.ptr))

    def read_back(self) -> Masks:
        n, w32 = self.n, self.words_host.shape[1]
        total = int(self.head.header_host[2 * n])
        if not 0 <= total <= self.words_host.shape[0]:
            raise device.PvhipError('{}: the head left total = {} of at most {} rows'.format(self.ENTRY, total, self.words_host.shape[0]))
        if total:
            device.call('pvhip_memcpy_d2h', ctypes.c_void_p(self.words_host.ctypes.data), ctypes.c_void_p(self.words.ptr), 4 * total * w32)
        return Masks(self.words_host[:total].copy(), (self.shape[1], self.shape[2]))


def frame_scratch_bytes(n: int, per_image: int) -> int:
    """PVHIP_FRAME_MASKS_SCRATCH_BYTES: total and the band count, the (rows + 1) int64 offsets, the (rows + 1) int32 band prefix."""
    return (16 + 12 * (n * per_image + 1) + 15) & ~15


class FrameBlocks:
    """The blocks of one (prototype Result, head's blocks, max_words) with space='FRAME': `words`, room for max_words words that
    pvhip_frame_masks_f32 writes, `made`, its 8-byte header (made, used), `scratch`, which stays on the device, and the page-locked
    twins of the first two.  read_back: the 8-byte header, then exactly 4 used bytes; the offsets are made here from the rois the
    head's own read_back has just copied -- wait() reads an ask behind the asks it needs."""
    __slots__ = ('n', 'per_image', 'shape', 'max_words', 'words', 'made', 'scratch', 'words_host', 'made_host', 'head', 'frame_size')
    ENTRY = 'pvhip_frame_masks_f32'

    def __init__(self, n: int, per_image: int, shape, max_words: int):
        self.n, self.per_image, self.shape, self.max_words, self.head, self.frame_size = n, per_image, shape, max_words, None, None
        self.words = device.DeviceTensor.empty((max_words,), np.uint32)
        self.made = device.DeviceTensor.empty((2,), np.int32)
        self.scratch = device.DeviceTensor.empty((frame_scratch_bytes(n, per_image) // 4,), np.int32)
        self.words_host = device.host_empty((max_words,), np.uint32)
        self.made_host = device.host_empty((2,), np.int32)

    def launch(self, protos, head_value, head_blocks, screen, net_hw, frame_size, fit, workgroups=0):
        """One call (two launches) on the current stream, behind the head's boxes call that has just written `head_blocks` there with
        the same `frame_size` and `fit`."""
        T, hp, wp = self.shape
        layout, n, A, C = boxes.shape_of(head_value.shape, screen.layout, screen.objectness, None, T)
        assert n == self.n and tuple(protos.shape) == (n, T, hp, wp) and protos.dtype == np.float32 and head_value.dtype == np.float32
        self.head, self.frame_size = head_blocks, (int(frame_size[0]), int(frame_size[1]))
        at = 4 + int(screen.objectness) + C
        device.call(self.ENTRY, device.ptr(head_value), n, A, at + T, boxes.LAYOUTS[layout], at, T, device.ptr(protos), hp, wp, net_hw[0], net_hw[1],
                    self.frame_size[0], self.frame_size[1], fit[0], fit[1], fit[2], fit[3], self.per_image, self.max_words, workgroups,
                    ctypes.c_void_p(head_blocks.header.ptr), ctypes.c_void_p(head_blocks.rows.ptr), ctypes.c_void_p(self.scratch.ptr),
                    ctypes.c_void_p(self.made.ptr), ctypes.c_void_p(self.words.ptr))

    def read_back(self) -> FrameMasks:
        total = int(self.head.header_host[2 * self.n])
        device.call('pvhip_memcpy_d2h', ctypes.c_void_p(self.made_host.ctypes.data), ctypes.c_void_p(self.made.ptr), 8)
        made, used = int(self.made_host[0]), int(self.made_host[1])
        rois = self.head.rows_host[:total, :5].copy()
        offsets = frame_offsets(rois, self.frame_size)
        if not 0 <= made <= total or used != int(offsets[made]) or used > self.max_words:
            raise device.PvhipError('{} left made = {}, used = {} where the {} rows say offsets[made] = {}'.format(
                self.ENTRY, made, used, total, int(offsets[min(max(made, 0), total)])))
        if used:
            device.call('pvhip_memcpy_d2h', ctypes.c_void_p(self.words_host.ctypes.data), ctypes.c_void_p(self.words.ptr), 4 * used)
        return FrameMasks(self.words_host[:used].copy(), offsets, rois, made)


class Ask(ask.Ask, collections.namedtuple('Ask', 'screen box_screen net_hw shape head_ask', defaults=(None,))):
    """A prototype Result asked for with masks=: `screen` the MaskScreen with its head named, `box_screen` that head's resolved
    BoxScreen, `net_hw` the extent the box numbers stand in, `shape` = (T, Hp, Wp), `head_ask` the head's own ask as checked() made
    it, from which bound() knows the frames a 'FRAME' pass will answer in; the launch takes the geometry from the head's bound ask."""
    __slots__ = ()
    KEYWORD = 'masks'

    @property
    def needs(self):
        return (self.screen.head,)

    @property
    def framed(self):
        return self.screen.space == 'FRAME'

    def bound(self, inputs, slots):
        if self.framed and self.head_ask is not None:       # (nothing is kept: the head's bound ask comes with the launch)
            _checked_frame(self.shape[1], self.shape[2], None, self.head_ask.bound(inputs, slots).frame_size)
        return self

    def key(self, name):
        """(name, the head's key): crop goes with the launch; the head's max_per_image sizes the words.  With space='FRAME' the space
        and max_words, which sizes them, stand behind."""
        key = (name, self.screen.head, self.box_screen._replace(min_score=None, frame_size=None))
        return key + (self.screen.space, self.screen.max_words) if self.framed else key

    def blocks_for(self, value):
        if self.framed:
            return FrameBlocks(int(value.shape[0]), self.box_screen.max_per_image, self.shape, self.screen.max_words)
        return Blocks(int(value.shape[0]), self.box_screen.max_per_image, self.shape)

    def launch(self, blocks, value, *others):
        (head_ask, head_value, head_blocks), = others
        blocks = blocks or self.blocks_for(value)
        if self.framed:
            blocks.launch(value, head_value, head_blocks, self.box_screen, self.net_hw, head_ask.frame_size, head_ask.fit)
        else:
            blocks.launch(value, head_value, head_blocks, self.box_screen, self.net_hw, self.screen.crop)
        return blocks

    def on_host(self, value, *others):
        (head_ask, head_value, _), = others
        head_value = np.asarray(head_value)
        found = head_ask.on_host(head_value)
        if self.framed:
            return make_frame(head_value, value, found, self.box_screen, self.net_hw, head_ask.frame_size, head_ask.fit, self.screen.max_words)
        return make(head_value, value, found, self.box_screen, self.net_hw, self.screen.crop)
