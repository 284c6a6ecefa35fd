"""What the kinds of answer share (top_k.py, detections.py, tiled_detections.py, gallery.py, keypoints.py, segments.py, maxima.py, text.py, boxes.py; answers.py drives them): the
Ask protocol, the flat block pair an answer of fixed size is read back through, the resolver of the Results an argument names, and
the min_score check."""
import ctypes

import numpy as np

from . import device

QUIET_NAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


class Ask:
    """One Result's question in its resolved form, as answers.py drives it: a mixin with no fields in front of the kind's namedtuple, so
    that an ask equals the plain tuple of its fields.  A kind states KEYWORD, the argument of infer() / start_async() it came from;
    `key(name)`, the key of its blocks among the request's; `blocks_for(value)`, new blocks for the value a pass left on the device;
    `launch_with()`, what its blocks' launch takes besides that value; `on_host(value)`, the rule in numpy on a host value; and
    `bound`, when it learns something from the inputs a pass was fed."""
    __slots__ = ()
    KEYWORD = None

    def bound(self, inputs, slots):         # (the ask for the pass whose `inputs`, as they were fed, are staged in `slots`)
        return self

    def launch_with(self) -> tuple:
        return ()

    def launch(self, blocks, value):
        """The launches on the current stream, behind whatever wrote `value` there, into `blocks` -- or into new ones for None --: the
        blocks."""
        blocks = blocks or self.blocks_for(value)
        blocks.launch(value, *self.launch_with())
        return blocks


class FlatBlocks:
    """`dev`, a device block of `words` int32 words that one launch fills, and `host`, its page-locked twin."""
    __slots__ = ('dev', 'host')

    def __init__(self, words: int):
        self.dev = device.DeviceTensor.empty((words,), np.int32)
        self.host = device.host_empty((words,), np.int32)

    def words(self):
        """`host` after one copy of the whole block; what is handed on is copied out of it."""
        device.call('pvhip_memcpy_d2h', ctypes.c_void_p(self.host.ctypes.data), ctypes.c_void_p(self.dev.ptr), self.host.nbytes)
        return self.host


def named(ienet, keyword: str, value, sharded: bool, fits=None, none=None, resolved=None) -> tuple:
    """({Result name: its input port}, {Result name: value}) of the argument `value` of `keyword`: for a dict the Results it names, for
    anything else every Result whose port `fits(port, value, batch)` (None: every Result); ValueError for an unknown name, for
    `none(ports, value, batch)` when no Result fits, for a batch sharded over ranks.  `resolved(value, what)` brings a value into its
    checked form ahead of all that but the unknown name; a kind that passes none resolves its values itself, behind the sharded refusal."""
    ports = {name: next(iter(ienet.G.nodes[nid]['input'].values())) for nid, name in ienet.find_node_by_type('Result')}
    if isinstance(value, dict):
        unknown = [name for name in value if name not in ports]
        if unknown:
            raise ValueError('{}: the network has no Result named {!r} (it has {})'.format(keyword, unknown[0], sorted(ports)))
        wanted = {name: v if resolved is None else resolved(v, '{}: Result {!r}'.format(keyword, name)) for name, v in value.items()}
    else:
        if resolved is not None:
            value = resolved(value, keyword)
        batch = int(ienet.batch_size)
        wanted = {name: value for name, port in ports.items() if fits is None or fits(port, value, batch)}
        if not wanted and none is not None:
            raise ValueError(none(ports, value, batch))
    if wanted and sharded:
        raise ValueError('{}: not with a batch sharded over ranks'.format(keyword))
    return ports, wanted


def declared(keyword: str, name: str, port, shape, expected: str, *batch):
    """`shape`, what the kind made of the dims of Result `name`'s port, when that is not None and the port is FP32; ValueError, which
    says `expected` (with `batch` filled in where it names one)."""
    if shape is None:
        raise ValueError('{}: Result {!r} has shape {}: not {}'.format(keyword, name, tuple(port['dims']), expected.format(*batch)))
    if port['precision'] != 'FP32':
        raise ValueError('{}: Result {!r} is {}: FP32 Results only'.format(keyword, name, port['precision']))
    return shape


def checked_min_score(min_score, what: str):
    """`min_score`, a finite real within float32 (None is the caller's to pass by), as the float of its float32; ValueError."""
    if isinstance(min_score, bool) or not isinstance(min_score, (int, float, np.integer, np.floating)) \
            or not np.isfinite(min_score) or abs(float(min_score)) > float(np.finfo(np.float32).max):
        raise ValueError('{}: min_score is None or a finite real (of float32), got {!r}'.format(what, min_score))
    return float(np.float32(min_score))
