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
thresholds), and the crop compares exactly where Ultralytics scales float boxes by Wp / Wn.  Out of scope: resizing to the frame,
retina_masks, areas or extents on the device, FP16 Results, T above 64, YOLACT's own crop, masks behind a TiledScreen or RegionScreen."""
import collections
import ctypes

import numpy as np

from . import ask, boxes, device
from .gallery import fmaf

MAX_TAIL = boxes.MAX_TAIL
MAX_PIXELS = 1 << 24
MAX_WORDS = 1 << 26                             # n * max_per_image * W32 at most
STAGE = 128                                     # PVHIP_MASKS_STAGE: tests place the counts around it

MaskScreen = collections.namedtuple('MaskScreen', 'head crop', defaults=(None, True))
MaskScreen.__doc__ = ('How to make the masks of a prototype Result: `head` names the Result asked for with boxes= in the same call whose '
                      'kept boxes get masks (None: the only one whose tail equals T); `crop`: bits outside a box are 0.')

Masks = collections.namedtuple('Masks', 'words shape')
Masks.__doc__ = ('What a Result started with masks= comes back as: `words` (total, W32) uint32, row j the packed mask of row j of the '
                 'head\'s Detections; `shape` = (Hp, Wp).  unpack() gives the booleans.')


def unpack(answer) -> np.ndarray:
    """(total, Hp, Wp) bool of a Masks."""
    hp, wp = answer.shape
    words = np.ascontiguousarray(answer.words, '<u4')
    bits = np.unpackbits(words.view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder='little')
    return bits[:, :hp * wp].reshape(-1, hp, wp).astype(bool)


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
    return MaskScreen(value.head, bool(value.crop))


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
        words = n * heads[head].max_per_image * words_per_row(hp, wp)
        if words > MAX_WORDS:
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


class Ask(ask.Ask, collections.namedtuple('Ask', 'screen box_screen net_hw shape')):
    """A prototype Result asked for with masks=: `screen` the MaskScreen with its head named, `box_screen` that head's resolved
    BoxScreen, `net_hw` the extent the box numbers stand in, `shape` = (T, Hp, Wp)."""
    __slots__ = ()
    KEYWORD = 'masks'

    @property
    def needs(self):
        return (self.screen.head,)

    def key(self, name):
        """(name, the head's key): crop goes with the launch; the head's max_per_image sizes the words."""
        return (name, self.screen.head, self.box_screen._replace(min_score=None, frame_size=None))

    def blocks_for(self, value):
        return Blocks(int(value.shape[0]), self.box_screen.max_per_image, self.shape)

    def launch(self, blocks, value, *others):
        (_, head_value, head_blocks), = others
        blocks = blocks or self.blocks_for(value)
        blocks.launch(value, head_value, head_blocks, self.box_screen, self.net_hw, self.screen.crop)
        return blocks

    def on_host(self, value, *others):
        (head_ask, head_value, _), = others
        head_value = np.asarray(head_value)
        return make(head_value, value, head_ask.on_host(head_value), self.box_screen, self.net_hw, self.screen.crop)
