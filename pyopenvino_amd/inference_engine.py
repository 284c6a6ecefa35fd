"""OpenVINO-IR loader and list scheduler around the op-plugin boundary.

Same public surface as the reference engine (``pyopenvino/inference_engine.py``): ``IECore``
(``read_network`` ``:74-83``, ``load_network`` ``:86-90``), ``IENetwork`` and ``Executable_Network``
(``schedule_tasks`` ``:218-242``, ``run_tasks`` ``:259-292``, ``infer`` ``:295-321``).  The model is a
``networkx.DiGraph`` whose node dicts carry the IR attributes; a static task list is executed by
calling ``plugins[type].compute(node, inputs, kernel_type=..., debug=False)`` per node -- that call is
the drop-in boundary, and what flows through ``inputs`` here are device-resident tensors.

Differences from the reference, all outside the numeric path:
  * constants are decoded with ``np.frombuffer`` (zero copy) instead of ``struct.unpack`` into tuples;
  * ``IENetwork.set_batch`` rewrites the batch dimension of every activation port so that a batch of
    independent images runs through the same graph (the reference IRs are baked at N=1);
  * plugins are discovered as modules of a package (default ``pyopenvino_amd.op_plugins``) instead of a
    CWD-relative glob;
  * ``infer`` can shard the batch across ranks (one process per GPU): every rank runs the unchanged
    scheduler on its slice and the Result plugin all-gathers the Result tensors;
  * the format a caller hands an input in can be declared (``IENetwork.input_info``: input_format.py) and is fixed at ``load_network``;
    host arrays of a declared format, or in a request's own page-locked buffers, are staged by the request's ``HostInputs``
    (host_input.py).
"""
import contextlib
import copy
import ctypes
import importlib
import os
import pickle
import pkgutil
import sys
import time
import xml.etree.ElementTree as et

import networkx as nx
import numpy as np

from . import common_def, device, fusion_plan, stream_plan
from .answers import Answers
from .host_input import HostInputs
from .input_format import DetectedRois, InputInfo, PreProcessChannel, PreProcessInfo  # noqa: F401 -- the classes of IENetwork.input_info
from .stream_plan import CaptureStreamModel

DEFAULT_PLUGIN_PACKAGE = 'pyopenvino_amd.op_plugins'


class Plugins:
    """Registry ``{IR layer type: module}``; a module's file name is the layer type it implements
    (reference inference_engine.py:28-43)."""

    def __init__(self):
        self.plugins = {}

    def import_plugin(self, package: str, module_name: str, plugin_name: str = None):
        module = importlib.import_module(package + '.' + module_name)
        if not hasattr(module, 'compute'):
            return None
        key = plugin_name or module_name
        setattr(self, key, module)
        self.plugins[key] = module
        return module

    def load_plugins(self, plugin_path: str):
        """``plugin_path`` is a dotted package name or a '/'-separated path to one."""
        package = plugin_path.replace(os.sep, '.').replace('/', '.').strip('.')
        pkg = importlib.import_module(package)
        for info in pkgutil.iter_modules(pkg.__path__):
            if not info.name.startswith('_'):
                self.import_plugin(package, info.name)


class IECore:
    def __init__(self, plugin_package: str = DEFAULT_PLUGIN_PACKAGE):
        self.plugins = Plugins()
        self.plugins.load_plugins(plugin_package)

    def construct_node_info(self, net, node_type: str) -> list:
        return [net.G.nodes[node_id] for node_id, _ in net.find_node_by_type(node_type)]

    def check_nodes(self, G: nx.DiGraph):
        missing = {G.nodes[n]['type'] for n in G.nodes} - set(self.plugins.plugins)
        if missing:
            print('Unsupported nodes : {}'.format(sorted(missing)))
        return missing

    def read_network(self, model: str, weights=None, fp16_as_fp32=None):
        """``model``: path of the IR ``.xml``.  ``weights``: path of the ``.bin`` (default: next to the
        xml, as the reference does) or the blob itself (bytes / uint8 ndarray) when the weights were
        synthesised in memory.  ``fp16_as_fp32``: run an FP16 IR with fp32 tensors AND fp32 arithmetic (constants upcast once
        at load, every FP16 port declared FP32); default: what the plugin package asks for (``COMPUTE_FP32``).  False with a
        package that declares ``F16_MFMA`` (this one): Convolution and MatMul round their operands to fp16 and run on the f16
        matrix cores with fp32 accumulation (``net.f16_mfma``), and the tensors between them are fp16 in HBM wherever the plan
        can keep them so (``fusion_plan``: channels blocked by eight, ``device.BlockedHalf`` -- GoogLeNet
        from conv1's output to pool5; ``PVHIP_CONV_F16_C8=0``: fp32 NCHW tensors holding fp16 values); the ports stay declared
        FP32, which is what a reader outside those kernels gets.  With any other package the IR is left as it is (FP16 ports,
        float16 constants: the reference's own mode)."""
        net = IENetwork(self)
        net.read_IR_Model(model, weights)
        net.parse_IR_XML()
        net.build_graph()
        net.set_constants_to_graph()
        if fp16_as_fp32 is None:
            fp16_as_fp32 = all(getattr(sys.modules.get(m.__package__), 'COMPUTE_FP32', False) for m in self.plugins.plugins.values())
        packages = [sys.modules.get(m.__package__) for m in self.plugins.plugins.values()]
        f16_mfma = fp16_as_fp32 is False and all(getattr(pkg, 'F16_MFMA', False) for pkg in packages)
        if fp16_as_fp32 or f16_mfma:
            net.promote_fp16()
            net.f16_mfma = f16_mfma and net.ir_precision == 'FP16'      # an FP32 IR keeps its fp32 kernels
        net.inputs = self.construct_node_info(net, 'Parameter')
        net.outputs = self.construct_node_info(net, 'Result')
        return net

    def load_network(self, network, device_name: str = 'GPU', num_requests: int = 1):
        """`num_requests` (accepted and ignored by the reference, inference_engine.py:86) is the number of infer
        requests that may be in flight at once: `exenet.requests[i].start_async(inputs)` / `.wait()`, each request
        with its own graph state and its own compute streams.  `exenet.infer()` stays the synchronous call."""
        for info in network.input_info.values():
            info._check_at_load()
        # the declared input formats as fixed values: one mapping, shared by every request
        exenet = Executable_Network(network, {name: info.frozen() for name, info in network.input_info.items()})
        self.check_nodes(exenet.ienet.G)
        exenet.schedule_tasks()
        exenet.create_requests(max(1, int(num_requests)))
        network._loaded = True               # input_info is fixed from here on
        return exenet


class IENetwork:
    def __init__(self, iecore: IECore):
        self.ie = iecore
        self.xml = None
        self.bin = None
        self.G = None
        self.layers = None
        self.edges = None
        self.inputs = None
        self.outputs = None
        self.batch_size = 1
        self.f16_mfma = False      # FP16 IR read with fp16_as_fp32=False: Convolution / MatMul on the f16 matrix cores
        self._input_info = None    # {Parameter name: InputInfo}, made when first asked for (the graph is built by then)
        self._loaded = False       # load_network has taken the input formats: their setters refuse from then on

    @property
    def input_info(self) -> dict:
        """{Parameter name: InputInfo}: the format each input is handed in (set before load_network)."""
        if self._input_info is None:
            self._input_info = {self.G.nodes[n]['name']: InputInfo(self, n) for n in self.G.nodes if self.G.nodes[n]['type'] == 'Parameter'}
        return self._input_info

    # ------------------------------------------------------------------ IR reading
    def read_IR_Model(self, model, weights=None):
        stem, _ = os.path.splitext(model)
        xml_file = stem + '.xml'
        if not os.path.isfile(xml_file):
            raise Exception('model {} is not found'.format(model))
        self.xml = et.parse(xml_file)
        if isinstance(weights, (bytes, bytearray, memoryview)):
            self.bin = bytes(weights) if not isinstance(weights, bytes) else weights
        elif isinstance(weights, np.ndarray):
            self.bin = weights.tobytes()
        else:
            bin_file = weights if (isinstance(weights, str) and os.path.isfile(weights)) else stem + '.bin'
            if not os.path.isfile(bin_file):
                raise Exception('model {} is not found'.format(model))
            with open(bin_file, 'rb') as f:
                self.bin = f.read()

    @staticmethod
    def _ports(section):
        ports = {}
        if section is None:
            return None
        for port in section.findall('port'):
            ports[int(port.attrib['id'])] = {
                'precision': port.attrib['precision'],
                'dims': tuple(int(d.text) for d in port.findall('dim')),
            }
        return ports

    def parse_IR_XML(self):
        root = self.xml.getroot()
        if root.tag != 'net':
            raise Exception('Not an OpenVINO IR file')
        layers = {}
        for layer in root.iterfind('./layers/layer'):
            info = {k: v for k, v in layer.attrib.items() if k != 'id'}
            data = layer.find('data')
            if data is not None:
                attrs = dict(data.attrib)
                for key in ('shape', 'stride'):
                    if key in attrs:
                        attrs[key] = common_def.string_to_tuple(attrs[key]) if attrs[key].strip() else ()
                info['data'] = attrs
            for tag in ('input', 'output'):
                ports = self._ports(layer.find(tag))
                if ports is not None:
                    info[tag] = ports
            layers[int(layer.attrib['id'])] = info
        self.layers = layers
        self.edges = [(int(e.attrib['from-layer']), int(e.attrib['from-port']),
                       int(e.attrib['to-layer']), int(e.attrib['to-port']))
                      for e in root.iterfind('./edges/edge')]

    def build_graph(self):
        G = nx.DiGraph()
        for node_id, info in self.layers.items():
            G.add_node(node_id, **info)
        for edge in self.edges:
            G.add_edge(edge[0], edge[2], connection=edge)
        assert nx.is_directed_acyclic_graph(G)
        self.G = G

    def set_constants_to_graph(self):
        """Attach each Const's slice of the ``.bin`` blob (little-endian raw data) to its node."""
        blob = memoryview(self.bin)
        for node_id, _ in self.find_node_by_type('Const'):
            node = self.G.nodes[node_id]
            attrs = node['data']
            offset, size = int(attrs['offset']), int(attrs['size'])
            precision = attrs['element_type'].upper()
            code, width = common_def.format_config[precision]
            if offset + size > len(blob):
                raise Exception('Const {} lies outside the weight blob'.format(node.get('name')))
            values = np.frombuffer(blob[offset:offset + size], dtype=np.dtype('<' + code), count=size // width)
            node['const'] = {'data': values, 'element_info': precision, 'size': size,
                             'decode_info': common_def.format_config[precision]}

    def find_node_by_type(self, type: str) -> list:
        return [(n, self.G.nodes[n]['name']) for n in self.G.nodes if self.G.nodes[n]['type'] == type]

    def promote_fp16(self):
        """SURVEY 8(f)-4, first step: an FP16 IR (ports FP16, f16 constants; the reference runs it in numpy float16,
        common_def.py:13-17) is computed with fp32 tensors -- every FP16 port is declared FP32, f16 constants are upcast
        once here, the Parameter takes fp32.  Results are at least as close to exact arithmetic as the reference's."""
        promoted = False
        for nid in self.G.nodes:
            node = self.G.nodes[nid]
            for tag in ('input', 'output'):
                for port in node.get(tag, {}).values():
                    if port['precision'] == 'FP16':
                        port['precision'] = 'FP32'
                        promoted = True
            attrs = node.get('data')
            if attrs is not None and str(attrs.get('element_type', '')).lower() == 'f16':
                attrs['element_type'] = 'f32'
                promoted = True
                if node['type'] == 'Const':
                    data = np.asarray(node['const']['data'], dtype=np.float16).astype(np.float32)
                    node['const'] = {'data': data, 'element_info': 'F32', 'size': data.nbytes,
                                     'decode_info': common_def.format_config['F32']}
        self.ir_precision = 'FP16' if promoted else 'FP32'

    # ------------------------------------------------------------------ batch
    def set_batch(self, batch: int):
        """Run ``batch`` independent images through the graph: multiply the leading dimension of every
        port that carries activations (anything downstream of a Parameter) by ``batch / current``.
        Constant ports keep their shape; Reshape targets in the shipped IRs use -1 / 0 for the batch
        axis, so they need no edit.  A ShapeOf output is a shape vector, not an activation: nothing that hangs off
        one (the SSD prior-box subgraph) is scaled.  DetectionOutput's records are (1, 1, N * keep, 7)
        (DetectionOutput.py:229-235): its third axis scales."""
        batch = int(batch)
        if batch < 1:
            raise ValueError('batch must be >= 1')
        if batch == self.batch_size:
            return
        if batch % self.batch_size and self.batch_size != 1:
            raise ValueError('set_batch works from the IR batch (call it once, or with a multiple)')
        old = self.batch_size
        G = self.G
        carries = G.copy()
        carries.remove_edges_from([(u, v) for u, v in G.edges if G.nodes[u]['type'] == 'ShapeOf'])
        act_nodes = set()
        for pid, _ in self.find_node_by_type('Parameter'):
            act_nodes.add(pid)
            act_nodes.update(nx.descendants(carries, pid))
        records = set()       # nodes whose tensors are detection records (1, 1, N * keep, 7): DetectionOutput and on
        for did, _ in self.find_node_by_type('DetectionOutput'):
            records.add(did)
            records.update(nx.descendants(G, did))

        def scaled(dims, axis=0):
            if len(dims) <= axis:
                return dims
            return tuple(dims[:axis]) + (dims[axis] // old * batch,) + tuple(dims[axis + 1:])

        for nid in act_nodes:
            node = G.nodes[nid]
            if node['type'] != 'ShapeOf':
                for port in node.get('output', {}).values():
                    port['dims'] = scaled(port['dims'], 2 if nid in records else 0)
            if node['type'] == 'Parameter':
                node['data']['shape'] = scaled(tuple(node['data']['shape']))
            for pred in G.pred[nid]:
                if pred in act_nodes and G.nodes[pred]['type'] != 'ShapeOf':
                    sink_port = G.edges[(pred, nid)]['connection'][3]
                    node['input'][sink_port]['dims'] = scaled(node['input'][sink_port]['dims'], 2 if pred in records else 0)
        self.batch_size = batch


class InferRequest:
    """One inference that can be in flight next to others (the OpenVINO infer-request idea behind the reference's
    unused `num_requests`): it owns a copy of the graph state (node outputs, cached device constants) and a set of
    compute streams, so that the kernels of several requests interleave on the device -- the HBM-bound layers of one
    run beside the matrix-core-bound layers of another, and each fills the other's tails.

    A start may ask for the answer of a Result in the place of the tensor: it is made on the device by launches behind the pass and read
    back by wait() in one or two small copies, while the full Result stays on the device.  Results not named come back whole; the keywords
    may be given together, for different Results; every refusal is a ValueError raised before anything is staged or launched (answers.py):

        keyword        value, for every fitting Result, or {Result name: value}               comes back as   module
        `top_k`        k                                                                       ``TopK``        top_k.py
        `detections`   a ``DetectionScreen`` or a min_confidence                               ``Detections``  detections.py
                       a ``TiledScreen`` / ``RegionScreen`` over a RoiInput / DetectedRois      ``Detections``  tiled_detections.py
        `matches`      a ``Gallery`` or a ``GalleryMatch``                                      ``Matches``     gallery.py
        `keypoints`    a ``PeakScreen``, a min_score or True                                    ``Keypoints``   keypoints.py
        `segments`     a ``SegmentScreen``, a min_score or True                                 ``Segments``    segments.py
        `maxima`       a ``MaximaScreen``, a min_score or True                                  ``Maxima``      maxima.py
        `text`         a ``TextScreen`` or True                                                 ``Text``        text.py
        `boxes`        a ``BoxScreen``, a min_score or True                                     ``Detections``  boxes.py"""

    def __init__(self, owner, runner, index: int):
        self.owner, self.runner, self.index = owner, runner, index      # owner: the network load_network returned
        self._in_flight, self._replayed = False, None
        self._asks = {}                 # {Result name: ask} of the pass in flight (answers.py): what top_k=, detections=, matches=, keypoints=, segments=, maxima=, text= and boxes= named

    def start_async(self, inputs: dict, top_k=None, detections=None, matches=None, keypoints=None, segments=None, maxima=None, text=None, boxes=None):
        self._start(inputs, (top_k, detections, matches, keypoints, segments, maxima, text, boxes), False)

    def _start(self, inputs, asked, verbose):
        """`asked`: (top_k, detections, matches, keypoints, segments, maxima, text, boxes) as the public signatures took them."""
        if self._in_flight:
            raise RuntimeError('request {} is still in flight: wait() first'.format(self.index))
        ex = self.runner
        sharded = ex.sharded or self.owner.sharded
        asks = ex.answers.checked(inputs, asked[0], asked[1], sharded, asked[2], asked[3], asked[4], asked[5], asked[6], asked[7])
        fed, inputs = inputs, ex.host_inputs.stage(inputs, ex.stream_base, sharded)
        self._asks = ex.answers.bound(asks, fed)
        ex.wait_result_readers()
        # The same device-resident tensors as the last calls: the pass is replayed from this request's own recording (one call
        # instead of ~100 dispatches; every request records its own pass on its own stream and keeps its own tensors, so the
        # replays of several requests run side by side like their eager passes do).
        self._replayed = ex._graph_for(inputs, verbose, gathers_later=True)
        if self._replayed is not None:
            ex.launch_graph(self._replayed)
        else:
            ex._bind_inputs(inputs)
            with ex._results_on_device():        # the shards are gathered in wait(): one collective at a time, on stream 0
                ex.run_tasks(verbose)
        if self._asks:                           # behind the pass, replayed or eager, and outside the recording: one recording serves every kind
            ex.answers.launch(self._asks, self._values())
        self._in_flight = True

    def _values(self, results=None) -> dict:
        """{Result name: what the pass in flight, replayed or eager, leaves there}; `results`: the Result nodes, when the caller has them."""
        if self._replayed is not None:
            return self._replayed['results']
        G = self.runner.ienet.G
        return {name: G.nodes[nid]['result'] for nid, name in results or self.runner.ienet.find_node_by_type('Result')}

    def wait(self) -> dict:
        ex = self.runner
        G = ex.ienet.G
        ex.wait_done()
        self._in_flight = False
        out, results = {}, ex.ienet.find_node_by_type('Result')
        values, self._replayed = self._values(results), None
        asks, self._asks = self._asks, {}
        for nid, name in results:
            value = values[name]
            if name in asks:                     # the answer comes back; the Result itself stays where it is, on the device
                G.nodes[nid]['result'], out[name] = value, ex.answers.read(name, asks[name], value)
            else:
                G.nodes[nid]['result'] = out[name] = ex._read_back(value, self.owner.comm)
        return out

    def infer(self, inputs: dict, top_k=None, detections=None, matches=None, keypoints=None, segments=None, maxima=None, text=None, boxes=None) -> dict:
        self.start_async(inputs, top_k, detections, matches, keypoints, segments, maxima, text, boxes)
        return self.wait()

    def input_buffer(self, name: str, source_size=None, frames=None) -> np.ndarray:
        """The host array this request uploads input `name` from: page-locked memory the request owns, allocated on the first call, in
        the declared format (``IENetwork.input_info``; e.g. (256, 224, 224, 3) uint8 for U8 / NHWC).  Handing it to ``start_async({name:
        buf})`` costs no host copy: it is uploaded asynchronously on the copy stream while other requests compute.  With RESIZE_BILINEAR
        declared, `source_size` = (h, w) of the source images (default: the network's extent); the request keeps buffers for its
        Executable_Network.MAX_SOURCE_EXTENTS most recently fed extents and drops older ones when it next starts a pass.  `frames` = m:
        the buffer of the m frames of a ``RoiInput`` instead -- the same shape with m in place of the batch; each (extent, m) counts as
        one of those extents.

        Ownership: the request reads this memory until its pass is done.  Fill it only between ``wait()`` (or before the first
        ``start_async``) and the next ``start_async()``; writing it while the request is in flight changes what the pass may see.  The
        memory is returned when the request's device state is released and the array is no longer referenced."""
        return self.runner.host_inputs.buffer(name, source_size, frames)

    def roi_buffer(self, name: str) -> np.ndarray:
        """The page-locked (n, 5) int32 table this request uploads the rectangles of a ``RoiInput`` of input `name` from, row b =
        (id, x, y, w, h).  ``RoiInput(input_buffer(name, (h, w), frames=m), roi_buffer(name))`` costs no host copy; ownership as for
        ``input_buffer``."""
        return self.runner.host_inputs.roi_buffer(name)

    def warp_buffer(self, name: str) -> np.ndarray:
        """The page-locked (n, 7) int64 table this request uploads the matrices of a ``WarpInput`` of input `name` from, row b =
        (id, A00, A01, C0, A10, A11, C1) with the coefficients in Q16 (``WarpInput.fixed``).  ``WarpInput(input_buffer(name, (h, w),
        frames=m), warp_buffer(name))`` costs no host copy; its values are checked by the limits of ``WarpInput.fixed`` when the pass
        starts; ownership as for ``input_buffer``."""
        return self.runner.host_inputs.warp_buffer(name)

    def perspective_buffer(self, name: str) -> np.ndarray:
        """The page-locked (n, 10) int64 table this request uploads the matrices of a ``PerspectiveInput`` of input `name` from, row b =
        (id, Q00, Q01, Q02, Q10, Q11, Q12, Q20, Q21, Q22), each matrix scaled by a power of two of its own
        (``PerspectiveInput.fixed``).  ``PerspectiveInput(input_buffer(name, (h, w), frames=m), perspective_buffer(name))`` costs no host
        copy; its values are checked by the limit of ``PerspectiveInput.fixed`` when the pass starts; ownership as for ``input_buffer``."""
        return self.runner.host_inputs.perspective_buffer(name)

    def detected_rois(self, name: str):
        """After ``wait()`` of a pass whose input `name` was a ``DetectedRois``: the record (count, selected, rois, records) -- `rois` the
        (n, 5) int32 table that pass used, rows >= count being (-1, 0, 0, 0, 0); `records[k]` the flat row of the detections batch row
        k came from (its label and score stand there), -1 from row count on; `selected` the records that passed the screen, which may
        exceed n; count = min(selected, n).  One small page-locked read-back on this request's drained stream.  RuntimeError when the
        last pass of that input was fed anything else."""
        if self._in_flight:
            raise RuntimeError('request {} is still in flight: wait() first'.format(self.index))
        return self.runner.host_inputs.detected_rois(name, self.runner.stream_base)

    def landmark_warps(self, name: str):
        """After ``wait()`` of a pass whose input `name` was a ``LandmarkWarps``: the record (count, valid, table) -- `table` the (n, 7)
        int64 table that pass used, row b = (id, A00, A01, C0, A10, A11, C1) in Q16, void rows being (-1, 0, 0, 0, 0, 0, 0); `valid` which
        rows are not void, (n,) bool; `count` how many.  ``warp.apply(table[b, 1:].reshape(2, 3) / 65536, xy)`` maps points `xy` of row
        b's network pixels -- what the consumer found in the aligned crop -- back to positions in frame ``table[b, 0]``.  One small
        page-locked read-back on this request's drained stream.  RuntimeError when the last pass of that input was fed anything else."""
        if self._in_flight:
            raise RuntimeError('request {} is still in flight: wait() first'.format(self.index))
        return self.runner.host_inputs.landmark_warps(name, self.runner.stream_base)


@contextlib.contextmanager
def _overridden(obj, **values):
    """Set these attributes of `obj` for the block and restore their old values after it."""
    saved = {name: getattr(obj, name) for name in values}
    for name, value in values.items():
        setattr(obj, name, value)
    try:
        yield
    finally:
        for name, value in saved.items():
            setattr(obj, name, value)


class Executable_Network:
    def __init__(self, ienetwork: IENetwork, input_formats: dict = None):
        """`input_formats`: {input name: InputFormat} as load_network froze them (default: as `ienetwork` declares them now)."""
        self.ienet = ienetwork
        self.kernel_type = 'hip'        # the reference's 'naive' / 'numpy' / 'special' are accepted too
        self.expected_result = None     # {node name: [precision, dims, ndarray]} (the reference's format) or {node name: ndarray}: per-layer compare hook (cf. :284-287)
        self.expected_rtol = 1.0        # the reference compares with np.allclose(rtol=1) (common_def.py:72)
        self.pickle_node_args = []      # node ids whose (node, inputs) run_tasks dumps to node_args_<id>.pickle (cf. :216, :275-278)
        self.pickle_dir = '.'           # where (the reference writes into the working directory)
        self.list_schedule = []         # the static list schedule (schedule_tasks); the plan's task order is this or another legal order of it
        self.plan = fusion_plan.FusionPlan(ienetwork.G, [])     # which nodes fold into which launch (plan_fusion); task_list is its order
        self.last_node_times = []       # [(node id, type, name, host seconds)] of the last run_tasks
        self.comm = None                # shard.BatchShardComm when the batch is sharded over ranks
        self.device_timing = None       # None, 'all', or a set of layer types: bracket those nodes with hipEvents
        self.device_timing_runs = False # True: consecutive bracketed nodes share ONE bracket (a bracket costs ~10-15 us
                                        # of stream time, which a per-node bracket would add to every launch)
        self.fuse_epilogues = True      # run Convolution -> Add(per-channel const) -> ReLU chains as one launch
        self.fuse_siblings = os.environ.get('PVHIP_FUSE_SIBLINGS', '1') != '0'
        self._infer_serial = 0
        self._timed = []                # [(node id, type, name, start Event, stop Event)] of the last run_tasks
        # Independent branches of the graph (the four arms of an inception module) go to separate compute
        # streams, ordered by untimed events; only for plugin sets whose tensors live on the device.
        self.compute_streams = int(os.environ.get('PVHIP_STREAMS', '4'))
        self.stream_base = 0            # first compute stream of this network (several requests in flight use disjoint sets)
        self.defer_sync = False         # True: run_tasks returns after the device-side join; the caller waits
        self.requests = []              # InferRequest per request in flight (create_requests); a request's own runner has none
        self._plan_serial = 0           # counts plan_fusion() calls: a captured pass is a pass of ONE plan
        self._stream_plans = {}         # {(task order, fused-away set, streams): StreamPlan}
        self._recording = False         # a hipGraph capture is open (capture_graph): cross-stream waits go through CaptureStreamModel
        # untimed events that order the streams: spare ones, and those of the pass in flight -- reused only after that pass has been
        # waited for (wait_done, or the start of the next pass, which follows a synchronous one)
        self._order_events, self._events_in_flight = [], []
        self._event_pool = []           # timed events for the device_timing brackets
        self._pending = None            # (allocation epoch or None, event) of a pass issued without a host wait: wait_done() ends it
        # events behind the launches of OTHER requests that read this network's device-resident Result (a DetectedRois fed from this
        # request while in flight): the next pass, eager or replayed, waits for them on the device before it can overwrite that tensor
        self._result_readers = []
        if input_formats is None:
            input_formats = {name: info.frozen() for name, info in ienetwork.input_info.items()}
        self.host_inputs = HostInputs(input_formats)    # host arrays in a declared format or the request's own buffers -> device tensors
        self.answers = Answers(self)    # Results asked for with top_k= / detections=: their blocks, launches and read-backs
        self._graph = None              # the recorded pass (capture_graph): {'handle', 'inputs', 'keep', 'results', 'by_hand'}
        self._auto_graph = {'key': None, 'seen': 0, 'failed': False, 'captured': False}     # infer()'s own recording (_graph_for)
        self._auto_graph_busy = False   # _graph_for is recording
        registry, G = ienetwork.ie.plugins.plugins, ienetwork.G
        # every plugin package of the set keeps its tensors on the device and computes on the current stream: passes fork over streams
        self._device_streams = all(getattr(sys.modules.get(m.__package__), 'DEVICE_STREAMS', False) for m in registry.values())
        # every layer type of the network says its compute() can be recorded (a foreign plugin set does not: its pass stays eager)
        self._graph_safe = all(getattr(registry.get(G.nodes[n]['type']), 'GRAPH_CAPTURE_SAFE', False) for n in G.nodes)

    _stream_ops = None                  # tests: a list that collects the cross-stream waits of a pass as they are issued
    MAX_SOURCE_EXTENTS = HostInputs.MAX_SOURCE_EXTENTS

    def create_requests(self, count: int):
        """Request 0 runs on this network's own graph; the others on copies of it made now, before anything has been
        uploaded (constants are uploaded and weights packed per request: the IRs' weights are tens of MB).  The
        compute streams (`compute_streams`, 4: what the device's hardware queues take without multiplexing -- more
        streams than that serialise behind each other's event waits) are split evenly between the requests."""
        if count > 8:
            raise ValueError('at most 8 requests (one compute stream each)')
        # A graph that has already been loaded or inferred holds device tensors (cached constants, packed weights, node
        # outputs): a deep copy would alias their blocks, and both owners would free them.  Strip that state first: every
        # request uploads and packs its own.
        self.release_device_state()
        per = max(1, int(self.compute_streams) // count)
        self.requests = [InferRequest(self, self, 0)]
        for i in range(1, count):
            twin = IENetwork(self.ienet.ie)
            for key, val in self.ienet.__dict__.items():
                if key not in ('ie', 'G'):
                    twin.__dict__[key] = val
            twin.G = copy.deepcopy(self.ienet.G)
            twin.inputs = self.ienet.ie.construct_node_info(twin, 'Parameter')
            twin.outputs = self.ienet.ie.construct_node_info(twin, 'Result')
            runner = Executable_Network(twin, self.host_inputs.formats)
            runner.fuse_epilogues = self.fuse_epilogues
            runner.schedule_tasks()
            self.requests.append(InferRequest(self, runner, i))
        if count > 1:
            for i, req in enumerate(self.requests):
                req.runner.stream_base = i * per
                req.runner.compute_streams = per

    def release_device_state(self):
        """Drop every device tensor the graph holds (cached constants, packed weights, node outputs, results); the next
        infer uploads and packs again.  A captured hipGraph holds raw addresses of exactly these tensors (packed weights, cached
        constants, Concat buffers): it goes first, or a later infer_graph() would replay kernels over freed or reused pool blocks."""
        self.release_graph()
        self.host_inputs.release()                  # page-locked buffers go back once the caller holds no view of them
        self._result_readers = []
        self.answers.release()
        G = self.ienet.G
        for nid in G.nodes:
            node = G.nodes[nid]
            for key in [k for k in node if isinstance(k, str) and k.startswith('_hip_')]:
                del node[key]
            for port in node.get('output', {}).values():
                port.pop('data', None)
            for key in ('result', 'param', '_sibling_out') + fusion_plan.HINT_KEYS:
                node.pop(key, None)

    sharded = property(lambda self: self.comm is not None and getattr(self.comm, 'world', 1) > 1)

    def wait_result_readers(self):
        """The base stream waits for every launch of another request that still reads the last pass's Result on the device."""
        if self._result_readers:
            readers, self._result_readers = self._result_readers, []
            device.select_stream(self.stream_base)
            for event in readers:
                event.wait()
            device.select_stream(0)

    def start_async(self, request_id: int, inputs: dict, top_k=None, detections=None, matches=None, keypoints=None, segments=None, maxima=None, text=None, boxes=None):
        self.requests[request_id].start_async(inputs, top_k, detections, matches, keypoints, segments, maxima, text, boxes)

    def wait(self, request_id: int) -> dict:
        return self.requests[request_id].wait()

    def schedule_tasks(self):
        """Static list schedule: sources (Const, Parameter) first, then repeated sweeps in node order
        appending every node whose predecessors are all scheduled (same policy as :218-242)."""
        G = self.ienet.G
        order, done = [], set()
        pending = []
        for node_id in G.nodes:
            if G.nodes[node_id]['type'] in ('Const', 'Parameter'):
                order.append(node_id)
                done.add(node_id)
            else:
                pending.append(node_id)
        while pending:
            still = []
            for node_id in pending:
                if all(p in done for p in G.pred[node_id]):
                    order.append(node_id)
                    done.add(node_id)
                else:
                    still.append(node_id)
            if len(still) == len(pending):
                raise RuntimeError('graph has nodes that can never become ready')
            pending = still
        self.list_schedule = order               # the reference's order; the plan may move mutually independent arms (locality order)
        self.plan_fusion()

    def plan_fusion(self):
        """(Re)build the fusion plan of the list schedule for the current flags (fusion_plan.build)."""
        self._plan_serial += 1
        self.plan = fusion_plan.build(self.ienet.G, self.list_schedule, self.ienet.ie.plugins.plugins, self.fuse_epilogues,
                                      self.fuse_siblings, bool(getattr(self.ienet, 'f16_mfma', False)))

    task_list = property(lambda self: self.plan.order, lambda self, order: setattr(self.plan, 'order', order))
    # the plan's fields under their old names, read-only (the live objects: callers look into them, tests edit _c8_entry in place)
    _fusion = property(lambda self: self.plan.fusion)
    _fused_away = property(lambda self: self.plan.fused_away)
    _concat_direct = property(lambda self: self.plan.concat_direct)
    _lrn_pool = property(lambda self: self.plan.lrn_pool)
    _siblings = property(lambda self: self.plan.siblings)
    _pool_conv = property(lambda self: self.plan.pool_conv)
    _pre_add = property(lambda self: self.plan.pre_add)
    _stem_conv = property(lambda self: self.plan.stem_conv)
    _stem_pool = property(lambda self: self.plan.stem_pool)
    _c8_out = property(lambda self: self.plan.c8_out)
    _c8_concat = property(lambda self: self.plan.c8_concat)
    _c8_entry = property(lambda self: self.plan.c8_entry)

    def prepare_inputs_for_task(self, task) -> dict:
        """{sink port: tensor} gathered from the predecessors' output ports, in edge order."""
        G = self.ienet.G
        inputs = {}
        for pred in G.pred[task]:
            src_node, src_port, _, sink_port = G.edges[(pred, task)]['connection']
            inputs[sink_port] = G.nodes[src_node]['output'][src_port]['data']
        return inputs

    def plan_streams(self):
        """The stream plan of the current task list over this network's streams (stream_plan.build): a StreamPlan (stream of task,
        tasks to wait for, tasks that must record an event), or None when not applicable."""
        n = max(1, min(int(self.compute_streams), 8 - self.stream_base))
        if (n <= 1 and self.stream_base == 0 and not self.defer_sync) or not self._device_streams:
            return None                  # one stream and a synchronous pass, or some plugin of the set computes on the host
        key = (tuple(self.task_list), frozenset(self.plan.fused_away), n)
        if key not in self._stream_plans:
            self._stream_plans[key] = stream_plan.build(self.ienet.G, self.plan, n)
        return self._stream_plans[key]

    def recorded_waits(self):
        """stream_plan.recorded_waits of the current plans: what _dispatch_tasks issues while a capture is open."""
        return stream_plan.recorded_waits(self.plan_streams(), self.plan)

    def recording_rings(self) -> bool:
        """True when a recording of the current plan would leave a ring in the runtime's parallel-stream lists."""
        return self.recorded_waits()[1].has_ring()

    def _bind_inputs(self, inputs: dict) -> dict:
        """Hand each input to the Parameter of that name (other names are ignored).  Returns {node name: node id}."""
        G = self.ienet.G
        by_name = {G.nodes[n]['name']: n for n in G.nodes}
        for node_name, val in inputs.items():
            if node_name in by_name:
                G.nodes[by_name[node_name]]['param'] = val
        return by_name

    @contextlib.contextmanager
    def _results_on_device(self):
        """The passes run inside keep their Results on the device, ungathered (the caller reads them back: _read_back), and
        run_tasks returns after the device-side join, without a host wait (wait_done)."""
        G, results = self.ienet.G, self.ienet.find_node_by_type('Result')
        for nid, _ in results:
            G.nodes[nid]['comm'] = None
            G.nodes[nid]['_async'] = True
        self.defer_sync = True
        try:
            yield
        finally:
            self.defer_sync = False
            for nid, _ in results:
                G.nodes[nid].pop('_async', None)

    def _read_back(self, value, comm=None):
        """A Result as infer() returns it: a device tensor is copied to the host, gathered over the ranks first when the batch is sharded.
        The copy synchronises the stream it is issued on: use one that has nothing else queued (this network's own have drained;
        another request's have not).  With sharded batches the gather and the copy go to the copy stream, which no request computes
        on: every rank waits for its requests in the same order, so the collectives of the one communicator are issued in the same
        order everywhere and never overlap each other."""
        gathers = comm is not None and comm.world > 1
        if not (hasattr(value, 'numpy') and not isinstance(value, np.ndarray)):
            return comm.allgather_rows(value) if gathers else value
        device.select_stream(device.COPY_STREAM if gathers else self.stream_base)
        value = np.asarray(comm.allgather_rows(value) if gathers else value)
        device.select_stream(0)
        return value

    def _order_event(self):
        """An untimed event for the pass being issued (it orders the streams); it is recorded again once that pass has been waited for."""
        event = self._order_events.pop() if self._order_events else device.Event(timed=False)
        self._events_in_flight.append(event)
        return event

    def run_tasks(self, verbose: bool = False):
        self._infer_serial += 1
        self._recycle_events()
        plan = self.plan_streams()
        epoch = None
        if plan is not None:
            self._order_events += self._events_in_flight     # the pass that recorded them has been waited for by now
            self._events_in_flight = []
            # blocks allocated during this pass and freed before it has finished on the device (workspaces) are
            # parked until it has; the previous pass's outputs, replaced as we go, are reusable at once
            epoch = device.pool_epoch_begin()
            device.select_stream(self.stream_base)
        try:
            self.last_node_times = self._dispatch_tasks(plan, epoch, verbose)
        except BaseException:
            # a plugin raised in the middle of a pass: leave the device in a defined state -- every stream drained, stream 0
            # current, the allocation epoch closed (its parked blocks back in the pool) -- and let the error travel on
            if plan is not None:
                try:
                    device.select_stream(0)
                    device.synchronize()
                    device.pool_epoch_dispatched()
                    device.pool_epoch_end(epoch)
                except Exception:
                    pass
            raise

    def _dispatch_tasks(self, plan, epoch, verbose):
        """One pass over the task list: `plan` the stream plan (or None), `epoch` the allocation epoch run_tasks opened, the base stream
        current.  Returns [(node id, type, name, host seconds)]."""
        G, registry, fp = self.ienet.G, self.ienet.ie.plugins.plugins, self.plan
        open_run, times = None, []
        if plan is not None:
            stream_of, waits, records = plan
            done_events, current, base = {}, 0, self.stream_base
            cap_model = CaptureStreamModel() if self._recording else None
            ops = self._stream_ops
        for task in fp.order:
            if task in fp.fused_away:
                continue
            node = G.nodes[task]
            node_type = node['type']
            if plan is not None and task in stream_of:
                if stream_of[task] != current:
                    current = stream_of[task]
                    device.select_stream(base + current)
                for dep in waits[task]:
                    how = cap_model.wait(current, stream_of[dep]) if cap_model is not None else 'plain'
                    if ops is not None:
                        ops.append((how, current, stream_of[dep], dep))
                    if how == 'relay':                   # (a recording only: see CaptureStreamModel)
                        device.select_stream(base)
                        done_events[dep].wait()
                        relay = self._order_event().record()
                        device.select_stream(base + current)
                        relay.wait()
                    else:
                        done_events[dep].wait()
            self._set_hints(task, node)
            inputs = self.prepare_inputs_for_task(task) if 'input' in node else {}
            plugin = registry.get(node_type)
            if plugin is None:
                print("ERROR: Operation '{}' (node={}) is not supported.".format(node_type, node['name']))
                sys.exit(-1)
            timed = self.device_timing is not None and (self.device_timing == 'all' or node_type in self.device_timing)
            if timed:
                if open_run is None:
                    open_run = [task, node_type, node['name'], self._event().record(), 0]
                open_run[4] += 1
            elif open_run is not None and node_type not in self.NO_LAUNCH_TYPES:
                open_run = self._close_run(open_run)
            if task in self.pickle_node_args:
                self.dump_node_args(task, node, inputs)
            t0 = time.time()
            res = plugin.compute(node, inputs, kernel_type=self.kernel_type, debug=False)
            dt = time.time() - t0
            if timed and not self.device_timing_runs:
                open_run = self._close_run(open_run)
            if plan is not None and task in records:
                done_events[task] = self._order_event().record()
            times.append((task, node_type, node['name'], dt))
            if verbose:
                print('{}, {}, {}, {}'.format(task, node_type, node['name'], dt))
            if self.expected_result is not None and node['name'] in self.expected_result and len(res) > 0:
                # the reference's hook (inference_engine.py:284-287 -> common_def.py:71-105); entries in its format
                # {name: [precision, dims, ndarray]} or bare arrays; `expected_rtol` = its rtol of 1 unless the caller tightens it
                common_def.compare_results(node['name'], next(iter(res.values())), self.expected_result, disp_results=False,
                                           rtol=self.expected_rtol)
            if len(res) > 0:
                if fp.c8_entry and (task in fp.c8_entry or fp.lrn_pool.get(task) in fp.c8_entry):
                    # the tensor the first blocked module reads: converted once, every reader gets the blocked form
                    res = {port_id: (device.BlockedHalf.from_dense(data) if isinstance(data, device.DeviceTensor) and data.ndim == 4 else data)
                           for port_id, data in res.items()}
                for port_id, data in res.items():
                    node['output'][port_id]['data'] = data
                receivers = fp.receivers.get(task)
                if receivers:                    # the ports of the nodes folded into the launch (a sibling launch: of its members too)
                    outs = [next(iter(res.values()))] + (list(node.pop('_sibling_out')) if task in fp.siblings else [])
                    for k, nid in receivers:
                        self._set_port(nid, outs[k])
        if open_run is not None:
            self._close_run(open_run)
        if plan is not None:
            # join: stream 0 continues after everything the other streams were given, then the host waits
            # (infer() has read the Result back by now, so this costs nothing) and freed blocks become reusable
            joins = []
            for st in sorted(set(stream_of.values()) - {0}):
                device.select_stream(base + st)
                joins.append(self._order_event().record())
            device.select_stream(base)
            for ev in joins:
                ev.wait()
            device.pool_epoch_dispatched()
            if self.defer_sync:          # asynchronous request: wait_done() ends the pass
                self._pending = (epoch, self._order_event().record())
            else:
                device.select_stream(0)
                device.synchronize()
                device.pool_epoch_end(epoch)
        return times

    def _set_port(self, nid, tensor):
        out = self.ienet.G.nodes[nid]['output']
        out[next(iter(out))]['data'] = tensor

    def _set_hints(self, task, node):
        """Clear every hint (HINT_KEYS) on the task's node dict and set the task's own, on every pass (Concat buffers and port tensors change
        from pass to pass).  A MaxPool / Add folded into the task's fetch hands its input on: its port takes that tensor first."""
        G, fp = self.ienet.G, self.plan
        for key in fusion_plan.HINT_KEYS:
            node.pop(key, None)
        pooled_in, pre_add = fp.pool_conv.get(task), fp.pre_add.get(task)
        for folded in (pooled_in, pre_add):
            if folded is not None:
                edge = G.edges[(fp.handed_on[folded[0]], folded[0])]['connection']
                self._set_port(folded[0], G.nodes[edge[0]]['output'][edge[1]]['data'])
        if pooled_in is not None:        # the kernel pools while it builds its tile
            node['_fuse_pool_in'] = G.nodes[pooled_in[0]]
        if pre_add is not None:          # the Add's constant rides in the padding pass
            node['_pre_add'] = G.nodes[pre_add[1]]['output'][0]['data']
        if node['type'] in ('Convolution', 'MatMul'):
            node['_f16_mfma'] = fp.f16
        fusion = fp.fusion.get(task)
        if fusion is not None:
            node['_fuse_bias'] = G.nodes[fusion['bias']]['output'][0]['data']
            node['_fuse_act'] = fusion['act']
            if fusion['into'] is not None:
                node['_out_into'] = (self._concat_buffer(fusion['into'][0]), fusion['into'][1])
        if task in fp.c8_out:
            node['_out_c8'] = True
        for sid in fp.siblings.get(task, ()):
            sf = fp.fusion[sid]
            node.setdefault('_siblings', []).append({'node': G.nodes[sid], 'inputs': self.prepare_inputs_for_task(sid),
                                                     'bias': G.nodes[sf['bias']]['output'][0]['data'], 'c8': sid in fp.c8_out,
                                                     'into': (self._concat_buffer(sf['into'][0]), sf['into'][1]) if sf['into'] is not None else None})
        folded = fp.lrn_pool.get(task)   # the node folded into this one: a MaxPool behind an LRN, or an LRN behind a MaxPool
        if folded is not None:
            node['_fuse_pool' if node['type'] == 'LRN' else '_fuse_lrn'] = G.nodes[folded]
        stem_conv = fp.stem_conv.get(task)   # the 1x1 convolution behind MaxPool + LRN, in the same launch
        if stem_conv is not None:
            sf = fp.fusion[stem_conv]
            wsrc = next(G.edges[(p_, stem_conv)]['connection'] for p_ in G.pred[stem_conv] if G.edges[(p_, stem_conv)]['connection'][3] == 1)
            node['_fuse_conv'] = {'node': G.nodes[stem_conv], 'w': G.nodes[wsrc[0]]['output'][wsrc[1]]['data'],     # c8: FP16 IRs, blocked
                                  'bias': G.nodes[sf['bias']]['output'][0]['data'], 'act': sf['act'], 'c8': fp.f16}
        pooled_by = fp.stem_pool.get(task)   # the stem convolution also writes the tensor of the MaxPool behind it ...
        if pooled_by is not None:
            node['_fuse_pool_out'] = G.nodes[pooled_by]
        for cid, pid in fp.stem_pool.items():    # ... and that MaxPool's launch takes it (a recording holds its address: capture_graph keeps it alive)
            if pid == task:
                node['_pooled_in'] = G.nodes[cid].pop('_pooled_out', None)

    # ---- hipGraph replay of a whole pass (what the reference's run_tasks loop, :259-292, becomes: one launch call)
    def capture_graph(self, inputs: dict, warm: int = 2, streams=1):
        """Record one forward pass into a hipGraph, for inputs that are resident on the device.  `infer_graph()` then replays it with
        ONE call instead of ~100 dispatches.  The graph holds the addresses of every tensor of the pass: they are kept alive with it
        (`release_graph`).  `streams` = 1 (default): the pass is recorded on one compute stream, a linear chain of launches -- with the
        persistent-grid kernels of this build that replays as fast as the forked form (googlenet-v1 batch 256: 44.5 k images/s either
        way, scripts/time_replay.py).  `streams='plan'`: recorded as the stream plan forks it (`compute_streams`).  Until round 4 that
        killed the process for some plans (stack overflow inside hipStreamEndCapture of ROCm 7.2: its walk over the per-stream lists of
        parallel capture streams meets a ring when non-origin streams wait for each other in both directions over time,
        profiles/r04_capture.md); the dispatcher now relays the ring-closing waits through the origin stream (CaptureStreamModel)."""
        if streams != 'plan':
            with _overridden(self, compute_streams=max(1, int(streams))):
                return self.capture_graph(inputs, warm=warm, streams='plan')
        G = self.ienet.G
        if not all(isinstance(v, device.DeviceTensor) for v in inputs.values()):
            raise ValueError('capture_graph needs device-resident inputs (DeviceTensor): their addresses go into the graph')
        self.release_graph()
        for _ in range(max(1, warm)):           # the pool learns every block size of the pass: a capture must not hipMalloc
            self._infer_eager(inputs)         # (which binds the inputs)
        if self.recording_rings():              # (cannot happen with the relays in place: refuse before any HIP call, never crash)
            raise device.PvhipError('capture_graph: this stream plan would close a ring in the runtime\'s parallel-stream lists '
                                    '(hipStreamEndCapture of ROCm 7.2 never returns from it); record on one stream')
        device.select_stream(self.stream_base)
        device.call('pvhip_graph_begin_capture')
        handle = ctypes.c_void_p()
        first_error = None
        try:
            with _overridden(self, device_timing=None, _recording=True), self._results_on_device():    # infer_graph() reads the Results back
                self.run_tasks(False)
        except BaseException as exc:            # noqa: BLE001 -- kept: end_capture below may fail too and must not mask it
            first_error = exc
        try:
            device.select_stream(self.stream_base)
            device.call('pvhip_graph_end_capture', ctypes.byref(handle))       # (also after an error: the capture must be closed)
        except Exception:                       # noqa: BLE001
            if first_error is None:
                raise
        if first_error is not None:
            if handle.value:
                device.call('pvhip_graph_destroy', ctypes.c_void_p(handle.value))
            raise first_error
        if self._pending is not None:           # its event belongs to the graph: nothing to wait for, just close the epoch
            device.pool_epoch_end(self._pending[0])
            self._pending = None
        results = {name: G.nodes[nid]['result'] for nid, name in self.ienet.find_node_by_type('Result')}
        keep = [p['data'] for n in G.nodes for p in G.nodes[n].get('output', {}).values() if 'data' in p] + list(results.values())
        # ... and the pooled tensor the stem convolution handed to the MaxPool behind it: it is on no port, and the next eager pass drops the hint
        keep += [G.nodes[n]['_pooled_in'] for n in G.nodes if G.nodes[n].get('_pooled_in') is not None]
        self._graph = {'handle': handle.value, 'inputs': dict(inputs), 'keep': keep, 'results': results,
                       'by_hand': not self._auto_graph_busy}       # a recording made by hand is never replaced by infer()
        device.select_stream(0)

    def dump_node_args(self, task, node, inputs):
        """The reference's node-replay hook (`pyopenvino/inference_engine.py:216, 275-278`): `(node, inputs)` of a chosen node,
        pickled as `node_args_<id>.pickle`, so that the node can be run on its own (`test_node_sample.py:1-16`; its fixture
        `resources/node_args_6.pickle` was made this way).  What the file holds is what the REFERENCE's plugins can load: device
        tensors are copied to host ndarrays, and the scheduler's private hints (`_fuse_bias`, `_out_into`, device caches: every key
        that starts with an underscore) stay out, so a fused Convolution replays as the plain Convolution it is in the IR."""

        def plain(obj):
            if isinstance(obj, (device.DeviceTensor, device.ChannelSlice)):
                return np.array(obj)
            if isinstance(obj, dict):
                return {k: plain(v) for k, v in obj.items() if not (isinstance(k, str) and (k.startswith('_') or k == 'comm'))}
            if isinstance(obj, (list, tuple)):
                return type(obj)(plain(v) for v in obj)
            return obj

        with open(os.path.join(self.pickle_dir, 'node_args_{}.pickle'.format(task)), 'wb') as f:
            pickle.dump((plain(node), plain(inputs)), file=f)

    def infer_graph(self, inputs: dict = None) -> dict:
        """Replay the captured pass (for new inputs: copied device-to-device into the captured input tensors first) and return
        {Result name: ndarray} like infer()."""
        g = self._graph
        if g is None:
            raise RuntimeError('no captured graph: call capture_graph(inputs) first')
        device.select_stream(self.stream_base)
        for name, val in (inputs or {}).items():
            dst = g['inputs'][name]
            if val is dst:
                continue
            src = device.as_device(val)
            if src.shape != dst.shape:
                raise ValueError('input {} has shape {}, the graph was captured for {}'.format(name, src.shape, dst.shape))
            device.call('pvhip_memcpy_d2d', ctypes.c_void_p(dst.ptr), ctypes.c_void_p(src.ptr), dst.nbytes)
        self.launch_graph(g)
        out = {name: self._read_back(t) for name, t in g['results'].items()}
        self.wait_done()
        device.synchronize()
        return out

    def release_graph(self):
        g, self._graph = self._graph, None
        self._auto_graph.update(captured=False, seen=0)
        if g is not None:
            device.call('pvhip_graph_destroy', ctypes.c_void_p(g['handle']))

    def wait_done(self):
        """Host-side wait for a pass dispatched with defer_sync (its streams have been joined on the base stream) or replayed by
        launch_graph."""
        if self._pending is not None:
            (epoch, done), self._pending = self._pending, None
            done.synchronize()
            if epoch is not None:
                device.pool_epoch_end(epoch)
            self._order_events += self._events_in_flight
            self._events_in_flight = []

    def _concat_buffer(self, cat_id):
        """Output tensor of a Concat whose producers write in place; one fresh tensor per infer."""
        node = self.ienet.G.nodes[cat_id]
        port = next(iter(node['output']))
        if node.get('_buf_serial') != self._infer_serial:
            dims = node['output'][port]['dims']
            # FP16 IRs, module form: the Concat's buffer is fp16 blocked by eight channels and every member writes its range of it
            node['output'][port]['data'] = device.BlockedHalf(dims) if cat_id in self.plan.c8_concat else device.DeviceTensor.empty(dims)
            node['_buf_serial'] = self._infer_serial
        return node['output'][port]['data']

    # ---- device-side per-node timing (hipEvents on the compute stream; cf. the time.time() bracket :279-283)
    def _event(self):
        return self._event_pool.pop() if self._event_pool else device.Event()

    NO_LAUNCH_TYPES = ('Const', 'Parameter', 'Reshape')   # their compute() puts nothing on the stream

    def _close_run(self, run):
        task, node_type, name, e0, count = run
        self._timed.append((task, node_type, name, e0, self._event().record(), count))
        return None

    def _recycle_events(self):
        for _, _, _, e0, e1, _ in self._timed:
            self._event_pool.extend((e0, e1))
        self._timed = []

    def device_times_ms(self, with_counts: bool = False):
        """[(node id, type, name, milliseconds)] for the brackets of the last run_tasks (synchronises).  With
        `device_timing_runs` a bracket spans a run of consecutive bracketed nodes: id / type / name are those of
        its first node and `with_counts=True` appends the number of nodes it covers."""
        out = []
        for task, node_type, name, e0, e1, count in self._timed:
            e1.synchronize()
            row = (task, node_type, name, e0.elapsed_ms(e1))
            out.append(row + (count,) if with_counts else row)
        return out

    def infer_until(self, inputs: dict, node_names) -> dict:
        """Run only what is needed to produce the outputs of the named nodes (e.g. the SSD backbone up to its
        box / class heads, whose host-side PriorBox / DetectionOutput consumers are out of scope) and return
        {node name: tensor of its first output port} -- device tensors are returned as they are."""
        G = self.ienet.G
        by_name = self._bind_inputs(inputs)
        targets = [by_name[name] for name in node_names]
        needed = set(targets)
        for t in targets:
            needed.update(nx.ancestors(G, t))
        with _overridden(self, plan=self.plan.restricted(needed, set(targets))):
            self.run_tasks(False)
        out = {}
        for name, t in zip(node_names, targets):
            ports = G.nodes[t]['output']
            out[name] = ports[next(iter(ports))]['data']
        return out

    # ---- replay instead of dispatch.  A forward pass is ~100 plugin calls = 0.8-0.9 ms of Python + ctypes per pass; with inputs that
    # are resident on the device -- the SAME tensors from call to call -- the pass is the same list of launches on the same addresses
    # every time, so after AUTO_GRAPH_AFTER identical eager passes infer() records it into a hipGraph once (capture_graph) and replays it from then on with one call
    # (infer_graph: bit-identical, tests/test_hip_models.py).  Anything that makes a pass differ -- other input tensors, another stream
    # plan or fusion plan, re-read PVHIP_* settings, hooks that look at single nodes (verbose, expected_result, pickle_node_args,
    # device_timing), a sharded batch -- runs eagerly, and a changed key drops the recording.  PVHIP_AUTO_GRAPH=0 turns it off.
    AUTO_GRAPH_AFTER = 2

    def _auto_graph_key(self, inputs, verbose, gathers_later=False):
        if verbose or os.environ.get('PVHIP_AUTO_GRAPH', '1') == '0' or self._auto_graph_busy:
            return None
        if self.expected_result is not None or self.pickle_node_args or self.device_timing is not None or self.defer_sync:
            return None
        if not gathers_later and self.comm is not None and getattr(self.comm, 'world', 1) > 1:
            return None                             # (a request gathers its shards in wait(), after the recorded pass)
        if not inputs or not all(isinstance(v, device.DeviceTensor) for v in inputs.values()):
            return None
        if not (self._device_streams and self._graph_safe):
            return None
        # (the recording reads the inputs where they lie: another tensor is another recording, never a copy into the caller's tensor)
        return (tuple(sorted((k, tuple(v.shape), v.ptr) for k, v in inputs.items())), self.compute_streams, self.stream_base,
                self._plan_serial, self.fuse_epilogues, device.settings_serial, self.kernel_type)

    def _graph_for(self, inputs, verbose=False, gathers_later=False):
        """The recording that replays this pass, or None: the pass is dispatched eagerly (and counted; the recording is made on the
        call after AUTO_GRAPH_AFTER identical eager ones)."""
        key = self._auto_graph_key(inputs, verbose, gathers_later)
        state, g = self._auto_graph, self._graph
        if key is None or state['failed'] or (g is not None and g['by_hand']):
            return None
        if state['key'] != key:
            if state['captured']:           # (release_graph clears 'captured': it is set exactly while infer()'s own recording exists)
                self.release_graph()
            state.update(key=key, seen=0, captured=False)
        if state['captured']:
            return g
        state['seen'] += 1
        if state['seen'] <= self.AUTO_GRAPH_AFTER:
            return None
        try:
            # (with gathers_later, the warm pass in front of the recording must not gather either: wait() does)
            with _overridden(self, _auto_graph_busy=True, comm=None if gathers_later else self.comm):
                self.capture_graph(inputs, warm=1)
            state['captured'] = True
        except Exception as exc:           # noqa: BLE001 -- replay is an optimisation: say why it is off, keep computing
            state['failed'] = True
            print('pyopenvino_amd: hipGraph replay of infer() disabled for this network ({}: {})'.format(type(exc).__name__, exc), file=sys.stderr)
            return None
        return self._graph

    def infer(self, inputs: dict, verbose: bool = False, top_k=None, detections=None, matches=None, keypoints=None, segments=None, maxima=None, text=None, boxes=None) -> dict:
        """`top_k`, `detections`, `matches`, `keypoints`, `segments`, `maxima`, `text`, `boxes`: the Results they name come back as their answers (InferRequest has the table)."""
        if not (top_k is detections is matches is keypoints is segments is maxima is text is boxes is None):     # something is asked: the pass of request 0 (this network's own graph and streams), waited for at once
            request = self.requests[0] if self.requests else InferRequest(self, self, 0)
            request._start(inputs, (top_k, detections, matches, keypoints, segments, maxima, text, boxes), verbose)
            return request.wait()
        inputs = self.host_inputs.stage(inputs, self.stream_base, self.sharded)
        self.wait_result_readers()
        if self._graph_for(inputs, verbose) is None:
            return self._infer_eager(inputs, verbose)
        return self.infer_graph(inputs)

    def launch_graph(self, g):
        """Asynchronous replay for an infer request: the recorded pass goes to this network's stream with one call; `wait_done()`
        waits for the event behind it."""
        device.select_stream(self.stream_base)
        device.call('pvhip_graph_launch', ctypes.c_void_p(g['handle']))
        self._pending = (None, self._order_event().record())
        device.select_stream(0)
        self.last_node_times = []

    def _infer_eager(self, inputs: dict, verbose: bool = False) -> dict:
        G = self.ienet.G
        self._bind_inputs(inputs)
        for nid, _ in self.ienet.find_node_by_type('Result'):
            G.nodes[nid]['comm'] = self.comm
        if verbose:
            print('# node_id node_name time (sec)')
        t0 = time.time()
        self.run_tasks(verbose)
        if verbose:
            print('@TOTAL_TIME,', time.time() - t0)
        return {name: G.nodes[nid]['result'] for nid, name in self.ienet.find_node_by_type('Result')}
