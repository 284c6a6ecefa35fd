"""The greedy CTC decoding of a text recogniser's Result (``infer(..., text=...)``): the rule, the argument checks and the device launch.
Heads that end in per-timestep class scores: CRNN-style licence-plate and scene-text recognisers, handwriting recognisers; the family the
input side cuts its crops for (WarpInput, PerspectiveInput).  A Result (T, n, C) ('TNC'), (n, T, C) ('NTC') or (n, C, T) ('NCT'), also
declared with a fourth axis of extent 1, which is dropped: axis 2 if dims[2] == 1, else axis 3 if dims[3] == 1.

The rule (include/pvhip.h, pvhip_ctc_greedy_f32; tests/text_ref.py is the same again in plain loops), for batch row r with scores
v[t][c]:
  1. winner  w(t) is the first class of timestep t in top_k's total order: NaN of any sign or payload first, then descending with
     +0.0 == -0.0, ties to the lower class.
  2. void    row r is void iff the winning score of any of its timesteps is NaN, that is, iff any of its T * C scores is NaN.
     A void row has length -1 and nothing but filler: the quiet-NaN rows behind `count` of a DetectedRois or LandmarkWarps pass
     are void.  An empty string (length 0) is an answer and not a void row.
  3. emit    timestep t emits iff w(t) != blank and (merge_repeated is false, or t == 0, or w(t) != w(t - 1)).  A repeat across
     a blank therefore emits twice: a, blank, a is aa.
  4. order   the emitting timesteps in ascending t fill slots 0, 1, ...: symbols = w(t), scores = the bits of v[t][w(t)],
     steps = t.
Row r's first lengths[r] slots are its string in time order; the slots behind them -- all of them in a void row -- are
(-1, quiet NaN, -1).  On rows without ties or NaN this is x.argmax(-1) followed by the usual collapse, and OpenVINO's CTCGreedyDecoder
with ctc_merge_repeated and a full sequence mask.  Out of scope: beam search and language models, a sequence mask or per-row lengths,
attention decoders, FP16 Results, T > 4096, confidences aggregated over a string."""
import collections
import ctypes

import numpy as np

from . import ask, device
from .ask import QUIET_NAN

MAX_STEPS = 4096                                # PVHIP_TEXT_MAX_STEPS: T at most
MAX_BLOCKS = 2048                               # PVHIP_TEXT_MAX_BLOCKS: the workgroups (of four rows each) of the rows form's grid at most
LAYOUTS = {'TNC': 0, 'NTC': 1, 'NCT': 2}        # PVHIP_TEXT_LAYOUT_*
FORM_NONE, FORM_ROWS, FORM_PLANES = 0, 1, 2     # PVHIP_TEXT_FORM_*

TextScreen = collections.namedtuple('TextScreen', 'blank merge_repeated layout', defaults=(-1, True, None))
TextScreen.__doc__ = ('How to read a CTC head\'s Result: `blank` is the class that separates, an int in -C .. C - 1, a negative one counted from the end '
                      '(-1, the default: the last class, OpenVINO\'s CTCGreedyDecoder; 0: recognisers with the blank first); `merge_repeated` '
                      'collapses a run of one class into one symbol; `layout` is \'TNC\', \'NTC\', \'NCT\' or None, which infers \'TNC\' or \'NTC\' from '
                      'where the batch stands.')

Text = collections.namedtuple('Text', 'lengths symbols scores steps')
Text.__doc__ = ('What a Result started with text= comes back as: `lengths` (n,) int32, -1 for a void row, `symbols` (n, T) int32 class indices, `scores` '
                '(n, T) float32 the Result\'s own bits of the winning score at the first timestep of each emitted run, `steps` (n, T) int32 that '
                'timestep; in time order, and (-1, NaN, -1) behind the length.')


class AmbiguousLayout(ValueError):
    """Both leading axes equal the batch: 'TNC' and 'NTC' fit alike."""


def resolved(value, what='text') -> TextScreen:
    """`value` -- a TextScreen or True (the default screen) -- as a checked TextScreen (blank may still be negative and layout None:
    they depend on the Result); ValueError."""
    if value is True:
        value = TextScreen()
    if not isinstance(value, TextScreen):
        raise ValueError('{}: a TextScreen or True, got {!r}'.format(what, value))
    blank, merge, layout = value
    if isinstance(blank, (bool, np.bool_)) or not isinstance(blank, (int, np.integer)):
        raise ValueError('{}: blank is an int in -C .. C - 1, got {!r}'.format(what, blank))
    if not isinstance(merge, (bool, np.bool_)):
        raise ValueError('{}: merge_repeated is a bool, got {!r}'.format(what, merge))
    if layout is not None and not (isinstance(layout, str) and layout in LAYOUTS):
        raise ValueError('{}: layout {!r} is not None or one of {}'.format(what, layout, sorted(LAYOUTS)))
    return TextScreen(int(blank), bool(merge), layout)


def steps_of(dims, layout=None, batch=None):
    """(layout, n, T, C) of a tensor declared as per-timestep class scores -- rank 3, or rank 4 with one axis of extent 1 dropped (axis 2
    if dims[2] == 1, else axis 3 if dims[3] == 1); 1 <= T <= 4096, C >= 2, n * T * C < 2^31, n the batch (when given) --, else None.
    `layout` None infers it: 'TNC' when dims[1] is the batch and dims[0] is not, 'NTC' when dims[0] is the batch and dims[1] is not
    ('NCT' is never inferred; without a batch nothing is); AmbiguousLayout, a ValueError, when both are the batch."""
    dims = tuple(int(d) for d in dims)
    if len(dims) == 4:
        dims = dims[:2] + dims[3:] if dims[2] == 1 else dims[:3] if dims[3] == 1 else None
    if dims is None or len(dims) != 3:
        return None
    if layout is None:
        if batch is None or batch not in dims[:2]:
            return None
        if dims[0] == dims[1]:
            raise AmbiguousLayout('shape {} with batch {} reads as \'TNC\' and as \'NTC\': say which with TextScreen(layout=...)'.format(dims, batch))
        layout = 'TNC' if dims[1] == batch else 'NTC'
    n, T, C = {'TNC': (dims[1], dims[0], dims[2]), 'NTC': dims, 'NCT': (dims[0], dims[2], dims[1])}[layout]
    if n < 1 or not 1 <= T <= MAX_STEPS or C < 2 or n * T * C >= 1 << 31 or (batch is not None and n != batch):
        return None
    return layout, n, T, C


def for_steps(screen: TextScreen, layout: str, C: int, what='text') -> TextScreen:
    """`screen`, resolved, for a Result of C classes read as `layout`: blank in 0 .. C - 1, layout filled in; ValueError."""
    if not -C <= screen.blank < C:
        raise ValueError('{}: blank is an int in -C .. C - 1 = {} .. {}, got {}'.format(what, -C, C - 1, screen.blank))
    return TextScreen(screen.blank % C, screen.merge_repeated, layout)


def greedy(x, screen) -> Text:
    """The rule in numpy on a host array read as `screen.layout`, which must be given (there is no batch to infer it from): what a Result
    computed on the host (a foreign plugin set) gets."""
    screen = resolved(screen, 'greedy')
    x = np.asarray(x)
    if screen.layout is None:
        raise ValueError('greedy: layout is one of {} here: there is no batch to infer it from'.format(sorted(LAYOUTS)))
    shape = steps_of(x.shape, screen.layout)
    if x.dtype != np.float32 or shape is None:
        raise ValueError('greedy takes float32 scores of rank 3 (or 4 with an axis of extent 1) with 1 <= T <= 4096, C >= 2 and n * T * C < 2^31, '
                         'got {} {}'.format(x.dtype, x.shape))
    layout, n, T, C = shape
    blank, merge, _ = for_steps(screen, layout, C, 'greedy')
    x = x.reshape({'TNC': (T, n, C), 'NTC': (n, T, C), 'NCT': (n, C, T)}[layout])
    v = x.transpose({'TNC': (1, 0, 2), 'NTC': (0, 1, 2), 'NCT': (0, 2, 1)}[layout])          # (n, T, C)
    nan = np.isnan(v)
    void = nan.any(axis=(1, 2))
    # the first NaN where there is one, else the first of the largest values (argmax takes +0.0 == -0.0 and the lower class)
    w = np.where(nan.any(axis=2), nan.argmax(axis=2), np.where(nan, -np.inf, v).argmax(axis=2))
    emit = w != blank
    if merge:
        emit[:, 1:] &= w[:, 1:] != w[:, :-1]
    emit[void] = False
    out = Text(np.where(void, -1, emit.sum(axis=1)).astype(np.int32), np.full((n, T), -1, np.int32), np.full((n, T), QUIET_NAN, np.float32),
               np.full((n, T), -1, np.int32))
    row, t = np.nonzero(emit)
    slot = (np.cumsum(emit, axis=1) - 1)[row, t]
    out.symbols[row, slot] = w[row, t]
    out.scores[row, slot] = v[row, t, w[row, t]]                 # the score's own bits (no NaN is ever emitted)
    out.steps[row, slot] = t
    return out


def strings(answer: Text, alphabet) -> list:
    """The rows of `answer` as str, one character (or string) of `alphabet` per symbol, the class index its position; None for a void
    row.  ValueError for a symbol outside the alphabet."""
    out = []
    for r, length in enumerate(answer.lengths):
        if length < 0:
            out.append(None)
            continue
        symbols = [int(s) for s in answer.symbols[r, :length]]
        bad = [s for s in symbols if not 0 <= s < len(alphabet)]
        if bad:
            raise ValueError('strings: row {} holds symbol {}, outside the alphabet of {}'.format(r, bad[0], len(alphabet)))
        out.append(''.join(alphabet[s] for s in symbols))
    return out


SHAPE = 'rank 3, or 4 with an axis of extent 1, with the batch n = {}, 1 <= T <= 4096, C >= 2 and n * T * C < 2^31'


def _fits(port, screen, batch):
    try:
        return port['precision'] == 'FP32' and steps_of(port['dims'], screen.layout, batch) is not None
    except AmbiguousLayout:
        return False


def _none_fits(ports, screen, batch):
    return 'text: no FP32 Result of {}{} (the Results: {})'.format(
        SHAPE.format(batch), ' whose layout can be inferred' if screen.layout is None else ' as {!r}'.format(screen.layout),
        {name: tuple(port['dims']) for name, port in ports.items()})


def checked(ienet, text, sharded: bool) -> dict:
    """{Result name: resolved TextScreen, blank in 0 .. C - 1 and layout filled in} of the `text` argument of infer() / start_async() -- a
    TextScreen or True for every FP32 Result that steps_of takes with the screen's layout (None: where it can be inferred), or {Result
    name: either} --, {} for None.  Everything is looked up in the network as it was read: no device is needed, nothing is allocated.
    ValueError ('text: ...'): an unknown name, a value of another type, blank not an int or outside -C .. C - 1, merge_repeated not a
    bool, an unknown layout, no such Result for an unnamed form, a sharded batch, a Result of another rank, shape or precision, T > 4096,
    C < 2, a named Result whose layout is ambiguous."""
    if text is None:
        return {}
    batch = int(ienet.batch_size)
    ports, wanted = ask.named(ienet, 'text', text, sharded, _fits, _none_fits, resolved)
    for name, screen in wanted.items():
        what = 'text: Result {!r}'.format(name)
        try:
            shape = steps_of(ports[name]['dims'], screen.layout, batch)
        except AmbiguousLayout as e:
            raise ValueError('{}: {}'.format(what, e)) from None
        expected = SHAPE + (' as {!r}'.format(screen.layout) if screen.layout is not None else ', the batch on one of the first two axes')
        layout, _, _, C = ask.declared('text', name, ports[name], shape, expected, batch)
        wanted[name] = for_steps(screen, layout, C, what)
    return wanted


class Blocks(ask.FlatBlocks):
    """What a request keeps for one (Result name, layout): the device block pvhip_ctc_greedy_f32 writes -- (n,) int32 lengths, (n, T)
    int32 symbols, (n, T) float32 scores, (n, T) int32 steps -- with the page-locked host block it is read back into in one copy of
    4 n + 12 n T bytes, and `scratch`, the (n, T) 8-byte keys between the entry's two launches, which stay on the device.  None depends
    on blank or merge_repeated, which are arguments of the launch."""
    __slots__ = ('n', 'T', 'scratch')

    def __init__(self, n: int, T: int):
        super().__init__(n + 3 * n * T)
        self.n, self.T = n, T
        self.scratch = device.DeviceTensor.empty((n, T), np.uint64)

    def launch(self, result, layout, blank, merge):
        """One call (two launches) on the current stream, behind whatever wrote `result` there."""
        _, n, T, C = steps_of(result.shape, layout)
        assert (n, T) == (self.n, self.T) and result.dtype == np.float32
        at, row = self.dev.ptr + 4 * n, 4 * n * T
        device.call('pvhip_ctc_greedy_f32', device.ptr(result), n, T, C, LAYOUTS[layout], blank, int(merge), ctypes.c_void_p(self.scratch.ptr),
                    ctypes.c_void_p(self.dev.ptr), ctypes.c_void_p(at), ctypes.c_void_p(at + row), ctypes.c_void_p(at + 2 * row))

    def read_back(self) -> Text:
        """The answer, copied on the current stream, which has drained; the arrays are the caller's own."""
        host, n, T = self.words(), self.n, self.T
        part = lambda i: host[n + i * n * T:n + (i + 1) * n * T].reshape(n, T)
        return Text(host[:n].copy(), part(0).copy(), part(1).view(np.float32).copy(), part(2).copy())


class Ask(ask.Ask, collections.namedtuple('Ask', 'screen')):
    """A Result asked for with text=, in its resolved form."""
    __slots__ = ()
    KEYWORD = 'text'

    def key(self, name):
        """(name, layout).  blank and merge_repeated are no part of it: they go with the launch."""
        return (name, self.screen.layout)

    def blocks_for(self, value):
        _, n, T, _ = steps_of(value.shape, self.screen.layout)
        return Blocks(n, T)

    def launch_with(self):
        return (self.screen.layout, self.screen.blank, self.screen.merge_repeated)

    def on_host(self, value):
        return greedy(value, self.screen)
