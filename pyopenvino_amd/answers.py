"""Answers behind the pass: the Results a start named with ``top_k=``, ``detections=``, ``matches=``, ``keypoints=``, ``segments=``, ``maxima=``, ``text=`` or ``boxes=`` come back from
wait() as a ``TopK``, a ``Detections``, a ``Matches``, a ``Keypoints``, a ``Segments``, a ``Maxima``, a ``Text`` or (a dense head's) a ``Detections`` made on the device instead of as the tensor.  One ``Answers`` per
Executable_Network (one per request), as ``HostInputs`` is on the way in: the request checks the arguments, binds the asks to the staged
inputs, launches behind the pass and reads after it.

An ask is one Result's question in its resolved form, an ``ask.Ask`` (ask.py states the protocol: KEYWORD, `bound`, `key`, `launch`,
`on_host`): top_k.Ask, detections.Ask / FittedAsk, tiled_detections.Ask / RegionAsk, gallery.Ask, keypoints.Ask, segments.Ask, maxima.Ask, text.Ask or boxes.Ask.  Which kind it is
matters only where checked() makes it; the rule of each kind, its argument's forms and its refusals are stated in its module.  A plain
screen over a detector whose input declares a fit (preprocess_info.resize_fit) learns its geometry in bound(), from the extent of the
frames the pass was fed, and so does a BoxScreen over such an input."""
import numpy as np

from . import boxes as boxes_rule, detections as detections_rule, device, gallery as gallery_rule, keypoints as keypoints_rule, maxima as maxima_rule, segments as segments_rule, \
    text as text_rule, tiled_detections as tiled_rule, top_k as top_k_rule
from .input_format import FrameFeed


def _no_clash(keyword: str, names, asks: dict, screens=()):
    """No Result of `names`, which `keyword` asks for, is among the `asks` or the `screens` of the keywords in front of it; ValueError for
    the first that is: the later keyword speaks and names the earlier."""
    for name in names:
        if name in asks or name in screens:
            raise ValueError('{}: Result {!r} is asked for with {} as well'.format(
                keyword, name, asks[name].KEYWORD if name in asks else detections_rule.Ask.KEYWORD))


class Answers:
    """`blocks` = {ask.key(Result name): its Blocks}, this request's own device and page-locked blocks, made on first use: (name, k),
    (name, resolved DetectionScreen), (name, resolved TiledScreen or RegionScreen, m), (name, id of the Gallery, k), (name, refine, space), of a class map (name,), of local maxima (name, max_per_plane, max_per_row, refine, space), of a decoded text (name, layout) or, of a dense head's boxes, (name, the BoxScreen without min_score and frame_size)."""

    def __init__(self, runner):
        self.runner, self.blocks = runner, {}       # runner: the Executable_Network whose base stream and Results these are

    def release(self):
        self.blocks = {}

    def checked(self, inputs, top_k, detections, sharded: bool, matches=None, keypoints=None, segments=None, maxima=None, text=None, boxes=None) -> dict:
        """{Result name: ask} of the `top_k`, `detections`, `matches`, `keypoints`, `segments`, `maxima`, `text` and `boxes` arguments of a start with `inputs`, {} when nothing
        is asked; ValueError.  Everything is looked up in the network as it was read: no device is needed, nothing is staged, allocated or
        launched.  The checks run in this order, which is not the keywords': matches' own, a tiled or region screen for a Result `top_k`
        names, top_k's, detections', a Result under two of the three, what a tiled, region or fitted screen asks of its feed, keypoints',
        a Result under keypoints and another, segments', a Result under segments and another, maxima's, a Result under maxima and another, text's, a Result under text and another, boxes', a Result under boxes and another, what a fitted input asks of its feed."""
        if top_k is detections is matches is keypoints is segments is maxima is text is boxes is None:
            return {}
        ex, ienet, asks = self.runner, self.runner.ienet, {}
        matched = gallery_rule.checked(ienet, matches, sharded) if matches is not None else {}
        if detections is not None:              # (a kind's module is asked only when its keyword is given: a pass pays for what it names)
            tiled_rule.checked_top_k(top_k, detections)
        if top_k is not None:
            asks = {name: top_k_rule.Ask(k) for name, k in top_k_rule.checked(ienet, top_k, sharded).items()}
        screens = detections_rule.checked(ienet, detections, sharded) if detections is not None else {}
        if screens and asks:
            _no_clash('detections', sorted(screens), asks)
        if matched and (asks or screens):
            _no_clash('matches', sorted(matched), asks, screens)
        if screens:
            formats, n = ex.host_inputs.formats, int(ienet.batch_size)
            tiled = {name: s for name, s in screens.items() if isinstance(s, tiled_rule.TiledScreen)}
            for name, s in tiled.items():           # (the geometry would be one per tile)
                if s.input in formats and formats[s.input].fitted:
                    raise ValueError('detections: Result {!r}: a TiledScreen over input {!r}, which declares resize_fit {}'.format(
                        name, s.input, formats[s.input].fit))
            regions = {name: s for name, s in screens.items() if isinstance(s, tiled_rule.RegionScreen)}     # (any declared fit: a geometry per row)
            tiled_rule.checked_feed(inputs, {**tiled, **regions})
            fitted = self._fitted_input() if len(screens) > len(tiled) + len(regions) else None
            if fitted is not None and isinstance(inputs, dict) and isinstance(inputs.get(fitted), FrameFeed):
                raise ValueError('detections: input {!r} declares resize_fit {} and is fed a {}: every row has a geometry of its own'.format(
                    fitted, formats[fitted].fit, type(inputs[fitted]).__name__))
            for name, s in screens.items():
                if name in tiled:
                    asks[name] = tiled_rule.Ask(s, n, None, None)
                elif name in regions:           # the extent and the declared fit of its input, and how the table of a DetectedRois is read
                    fmt = formats[s.input]
                    asks[name] = tiled_rule.RegionAsk(s, n, None, None, (int(fmt.dims[2]), int(fmt.dims[3])), fmt.fit,
                                                      lambda s=s: ex.host_inputs.detected_rois(s.input, ex.stream_base), None)     # (called with no argument: `s` is bound here, not in the loop's last round)
                elif fitted is None:
                    asks[name] = detections_rule.Ask(s, n)
                else:
                    given = detections[name] if isinstance(detections, dict) else detections
                    explicit = isinstance(given, detections_rule.DetectionScreen) and given.frame_size is not None
                    asks[name] = detections_rule.FittedAsk(s, n, fitted, formats[fitted], explicit, None)
        if matched:
            asks.update((name, gallery_rule.Ask(match)) for name, match in matched.items())
        if keypoints is not None:
            peaks = keypoints_rule.checked(ienet, keypoints, sharded)
            if asks:                            # (keypoints speaks of the first Result in its own order)
                _no_clash('keypoints', peaks, asks)
            for name, screen in peaks.items():
                asks[name] = keypoints_rule.Ask(screen)
        if segments is not None:
            maps = segments_rule.checked(ienet, segments, sharded)
            if asks:
                _no_clash('segments', maps, asks)
            for name, screen in maps.items():
                asks[name] = segments_rule.Ask(screen)
        if maxima is not None:
            found = maxima_rule.checked(ienet, maxima, sharded)
            if asks:
                _no_clash('maxima', found, asks)
            for name, screen in found.items():
                asks[name] = maxima_rule.Ask(screen)
        if text is not None:
            read = text_rule.checked(ienet, text, sharded)
            if asks:
                _no_clash('text', read, asks)
            for name, screen in read.items():
                asks[name] = text_rule.Ask(screen)
        if boxes is not None:
            heads = boxes_rule.checked(ienet, boxes, sharded)
            if asks:
                _no_clash('boxes', heads, asks)
            formats = ex.host_inputs.formats
            for name, screen in heads.items():
                fmt = formats.get(screen.input)
                fitted = fmt is not None and fmt.fitted
                if fitted and isinstance(inputs, dict) and isinstance(inputs.get(screen.input), FrameFeed):     # (detections=' refusal: a geometry per row)
                    raise ValueError('boxes: input {!r} declares resize_fit {} and is fed a {}: every row has a geometry of its own'.format(
                        screen.input, fmt.fit, type(inputs[screen.input]).__name__))
                asks[name] = boxes_rule.Ask(screen, boxes_rule.extent_of(ienet, screen.input), fmt if fitted else None, None, None)
        return asks

    def _fitted_input(self):
        """The name of the network's single 4-D Parameter when its format declares a fit, else None."""
        names = [name for name, fmt in self.runner.host_inputs.formats.items() if len(fmt.dims) == 4]
        return names[0] if len(names) == 1 and self.runner.host_inputs.formats[names[0]].fitted else None

    def bound(self, asks: dict, inputs: dict) -> dict:
        """`asks` for the pass whose `inputs`, as they were fed, host_inputs.stage() has just staged: a tiled ask learns its frame count
        and its tile table here, where the frames are known to be m frames."""
        slots = self.runner.host_inputs.slots
        return {name: ask.bound(inputs, slots) for name, ask in asks.items()}

    def launch(self, asks: dict, values: dict):
        """Every ask's launches on the base stream, behind the pass -- replayed or eager, and outside the recording: one recording serves
        every kind -- that left `values` = {Result name: tensor}, and behind the tile table stage() uploaded on that stream; wait_done()
        then waits for one event behind them all.  A Result that is a host array gets the rule in numpy when it is read."""
        ex = self.runner
        on_device = [(name, ask) for name, ask in asks.items() if isinstance(values[name], device.DeviceTensor)]
        if not on_device:
            return
        device.select_stream(ex.stream_base)
        for name, ask in on_device:
            key = ask.key(name)
            self.blocks[key] = ask.launch(self.blocks.get(key), values[name])      # (made on first use)
        ex._pending = (ex._pending[0] if ex._pending is not None else None, ex._order_event().record())
        device.select_stream(0)

    def read(self, name: str, ask, value):
        """The answer of Result `name` after wait_done(): read back from the blocks launch() filled, on the drained base stream; the rule
        in numpy -- a tiled one on the slot's page-locked table -- for a Result that is a host array."""
        if not isinstance(value, device.DeviceTensor):
            return ask.on_host(np.asarray(value))
        device.select_stream(self.runner.stream_base)
        out = self.blocks[ask.key(name)].read_back()
        device.select_stream(0)
        return out
