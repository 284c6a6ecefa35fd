"""The fusion plan of a scheduled graph: which nodes fold into which launch, and the order of the launches.  `build()` runs the peepholes;
each asks the plugin that will run the launch (`*_fusable` / `*_ok`).  A folded node is never dispatched: its port carries the tensor of
the launch it was folded into (a placeholder where its own never exists); `receivers`, `owner` and `writers` say which, once."""
import os

import numpy as np

from . import device        # settings only (parsed from the environment at import / reload_settings(): the SAME values the plugins read)

# every hint the dispatcher may put on a task's node dict for its plugin (cleared before a task's own are set, and by release_device_state)
HINT_KEYS = ('_fuse_pool_in', '_pre_add', '_f16_mfma', '_fuse_bias', '_fuse_act', '_out_into', '_out_c8', '_siblings', '_fuse_pool',
             '_fuse_lrn', '_fuse_conv', '_fuse_pool_out', '_pooled_out', '_pooled_in')


def data_src(G, nid):          # the node that feeds input port 0 of `nid`, or None
    return next((p_ for p_ in G.pred[nid] if G.edges[(p_, nid)]['connection'][3] == 0), None)


class FusionPlan:
    def __init__(self, G, order, f16=False):
        self.G = G
        self.order = list(order)    # the task list: the list schedule, or another legal order of it (_order_for_locality)
        self.f16 = f16              # FP16 IR on the f16 matrix cores (IENetwork.f16_mfma)
        self.fusion = {}            # conv node id -> {'bias': const id, 'add': id, 'relu': id or None, 'act', 'into': (Concat id, channel offset) or None}
        self.fused_away = set()     # node ids whose compute() is folded into another launch
        self.concat_direct = {}     # Concat node id -> total channels, when every input is written in place
        self.lrn_pool = {}          # LRN node id -> id of the MaxPool folded into it, or MaxPool id -> id of the LRN folded into it
        self.siblings = {}          # Convolution node id -> ids of the convolutions of the same input launched with it
        self.pool_conv = {}         # Convolution node id -> (MaxPool node folded into its input tile, id of the MaxPool's data input)
        self.pre_add = {}           # Convolution node id -> (Add node folded into its padding pass, Const id, id of the Add's data input)
        self.stem_conv = {}         # MaxPool (leading MaxPool + LRN) -> the 1x1 convolution behind the LRN that rides in the same launch
        self.stem_pool = {}         # Convolution (the stem) -> the MaxPool behind its chain whose tensor the convolution's launch writes too: that MaxPool's launch is LRN + 1x1 only
        self.c8_out = set()         # FP16 IRs: convolutions whose fused chain hands its output over blocked by eight channels
        self.c8_concat = set()      # ... Concats that get a blocked buffer
        self.c8_entry = set()       # ... the tensor the first blocked module reads, converted once
        self.receivers, self.owner, self.handed_on = {}, {}, {}

    def tail(self, cid):                # the end of a fused convolution chain: its ReLU / Clamp, else its Add
        f = self.fusion[cid]
        return f['relu'] if f['relu'] is not None else f['add']

    def chain(self, cid):               # the convolution, its Add and its activation
        f = self.fusion[cid]
        return [n_ for n_ in (cid, f['add'], f['relu']) if n_ is not None]

    def _derive(self):
        # dispatched task -> [(k, node)]: the node's port takes the launch's k-th returned tensor (0: its own, k > 0: its k-th sibling's)
        self.receivers = {cid: [(0, n_) for n_ in self.chain(cid)[1:]] for cid in self.fusion if cid not in self.fused_away}
        for lead, sibs in self.siblings.items():
            self.receivers.setdefault(lead, []).extend((k, n_) for k, sid in enumerate(sibs, 1) for n_ in self.chain(sid))
        for lead, folded in self.lrn_pool.items():
            self.receivers.setdefault(lead, []).append((0, folded))
        for pid, cid in self.stem_conv.items():      # the pooled and the normalised tensor do not exist: their ports hold the chain's
            self.receivers.setdefault(pid, []).extend((0, n_) for n_ in self.chain(cid))
        self.owner = {n_: task for task, ports in self.receivers.items() for _, n_ in ports}
        # a MaxPool / Add folded into its consumer's fetch -> the node whose tensor it hands on
        self.handed_on = dict(list(self.pool_conv.values()) + [(add_id, src_id) for add_id, _, src_id in self.pre_add.values()])

    def output_of(self, task):          # the graph node whose output port carries the tensor the task's launch writes
        if task in self.stem_conv:
            return self.tail(self.stem_conv[task])
        if task in self.lrn_pool:
            return self.lrn_pool[task]
        return self.tail(task) if task in self.fusion else task

    def writers(self, nid):             # the dispatched tasks whose launches write the tensor of node `nid`
        if nid in self.handed_on:
            return self.writers(self.handed_on[nid])
        if nid in self.concat_direct:
            return [w for pred in self.G.pred[nid] for w in self.writers(pred)]
        if nid in self.owner:
            return [self.owner[nid]]
        return [] if self.G.nodes[nid]['type'] in ('Const', 'Parameter') else [nid]     # (uploads are synchronous, or already resident)

    def restricted(self, needed, targets):
        """The plan of a run of the sub-graph `needed` up to `targets` (infer_until): no siblings, folded pools or Adds, Concat-direct, stem
        convolution or blocked tensors; a fused chain wholly inside it, and an LRN / MaxPool pair led by no target (placeholder port), stay."""
        sub = FusionPlan(self.G, [t for t in self.order if t in needed], self.f16)
        sub.fusion = {c: dict(f, into=None) for c, f in self.fusion.items() if all(n_ in needed for n_ in self.chain(c))}
        sub.lrn_pool = {l_: p_ for l_, p_ in self.lrn_pool.items() if l_ in needed and p_ in needed and l_ not in targets}
        sub.fused_away = {n_ for c in sub.fusion for n_ in sub.chain(c)[1:]} | set(sub.lrn_pool.values())
        sub._derive()
        return sub


def build(G, order, plugins, fuse_epilogues=True, fuse_siblings=True, f16=False):
    """The plan of graph `G` in list-schedule `order` for the plugin registry `plugins` ({layer type: module}).  fuse_epilogues=False:
    nothing is folded.  Reads device.fuse_poolconv, fuse_stem_conv, fuse_stem_pool, conv_f16_c8, conv_f16_dma and PVHIP_SCHEDULE_LOCALITY."""
    p = FusionPlan(G, order, f16)
    if fuse_epilogues:
        _lrn_then_pool(p, plugins)
        _pool_then_lrn(p, plugins)
        conv = plugins.get('Convolution')
        if conv is not None and getattr(conv, 'SUPPORTS_FUSED_EPILOGUE', False):
            _epilogues(p, plugins)
            _concat_direct(p)
            _pool_conv(p, conv)
            _pre_add(p, conv)
            _siblings(p, conv, fuse_siblings)
            _stem_conv(p, plugins)
            _stem_pool(p, plugins)
            _c8_writers(p, conv)
            _c8_stem(p, plugins)
            _c8_stem_conv(p, plugins)
            _c8_modules(p, plugins)
            _order_for_locality(p)
    p._derive()
    return p


def _lrn_then_pool(p, plugins):
    """An LRN whose only consumer is a MaxPool the fused kernel covers: one launch, the LRN tensor is never written."""
    G, lrn = p.G, plugins.get('LRN')
    if lrn is None or not getattr(lrn, 'SUPPORTS_FUSED_POOL', False):
        return
    for lid in G.nodes:
        if G.nodes[lid]['type'] != 'LRN':
            continue
        succ = list(G.successors(lid))
        if len(succ) != 1 or G.nodes[succ[0]]['type'] != 'MaxPool' or G.edges[(lid, succ[0])]['connection'][3] != 0:
            continue
        if lrn.pool_fusable(G.nodes[lid], G.nodes[succ[0]]):
            p.lrn_pool[lid] = succ[0]
            p.fused_away.add(succ[0])


def _pool_then_lrn(p, plugins):
    """The other order: a MaxPool whose only consumer is an LRN the fused kernel covers (GoogLeNet: pool1/3x3_s2 -> pool1/norm1), unless
    that LRN already leads an LRN -> MaxPool launch."""
    G, pool = p.G, plugins.get('MaxPool')
    if pool is None or not getattr(pool, 'SUPPORTS_FUSED_LRN', False):
        return
    for pid in G.nodes:
        if G.nodes[pid]['type'] != 'MaxPool' or pid in p.fused_away:
            continue
        succ = list(G.successors(pid))
        if len(succ) != 1 or G.nodes[succ[0]]['type'] != 'LRN' or G.edges[(pid, succ[0])]['connection'][3] != 0:
            continue
        if succ[0] not in p.lrn_pool and succ[0] not in p.fused_away and pool.lrn_fusable(G.nodes[pid], G.nodes[succ[0]]):
            p.lrn_pool[pid] = succ[0]
            p.fused_away.add(succ[0])


def _epilogues(p, plugins):
    """ Convolution -> Add of a per-output-channel Const (1,K,1,1) -> optional ReLU / Clamp, each the only consumer of the
    one before, is ONE launch: the kernel epilogue adds the bias and applies the activation (same fp32 add, same select: same bits)."""
    G = p.G
    fusable = {t for t in ('Convolution', 'GroupConvolution') if getattr(plugins.get(t), 'SUPPORTS_FUSED_EPILOGUE', False)}
    for cid in G.nodes:
        if G.nodes[cid]['type'] not in fusable:
            continue
        succ = list(G.successors(cid))
        if len(succ) != 1 or G.nodes[succ[0]]['type'] != 'Add' or G.edges[(cid, succ[0])]['connection'][3] != 0:
            continue
        aid = succ[0]
        others = [p_ for p_ in G.pred[aid] if p_ != cid]
        if len(others) != 1 or G.nodes[others[0]]['type'] != 'Const':
            continue
        bid = others[0]
        k_out = next(iter(G.nodes[cid]['output'].values()))['dims'][1]
        if tuple(G.nodes[bid]['data']['shape']) != (1, k_out, 1, 1) or G.nodes[bid]['data']['element_type'] != 'f32':
            continue
        asucc = list(G.successors(aid))
        rid = asucc[0] if len(asucc) == 1 and G.nodes[asucc[0]]['type'] in ('ReLU', 'Clamp') else None
        act = None if rid is None else ('relu',) if G.nodes[rid]['type'] == 'ReLU' else \
            ('clamp', float(G.nodes[rid]['data']['min']), float(G.nodes[rid]['data']['max']))
        p.fusion[cid] = {'bias': bid, 'add': aid, 'relu': rid, 'act': act, 'into': None}
        p.fused_away.update(p.chain(cid)[1:])


def _concat_direct(p):
    """A channel Concat (axis 1, NCHW) whose inputs are all ends of fused convolution chains with no other consumer is not dispatched:
    each convolution writes its channels straight into the Concat's tensor (Concat.py:9-13 as a store pattern)."""
    G = p.G
    tail_of = {p.tail(cid): cid for cid in p.fusion}
    for nid in G.nodes:
        node = G.nodes[nid]
        if node['type'] != 'Concat' or int(node['data']['axis']) != 1:
            continue
        out_dims = next(iter(node['output'].values()))['dims']
        preds = list(G.pred[nid])
        if len(out_dims) != 4 or len(preds) < 2 or len(preds) != len(node['input']):
            continue
        cids = [tail_of.get(pred) for pred in preds]         # edge order == np.concatenate order (Concat.py:11-12)
        if None in cids or any(len(list(G.successors(pred))) != 1 for pred in preds):
            continue
        ks = [next(iter(G.nodes[cid]['output'].values()))['dims'][1] for cid in cids]
        if sum(ks) != out_dims[1]:
            continue
        for i, cid in enumerate(cids):
            p.fusion[cid]['into'] = (nid, sum(ks[:i]))
        p.concat_direct[nid] = sum(ks)
        p.fused_away.add(nid)


def _pool_conv(p, conv):
    """A 3x3 / stride 1 / pad 1 MaxPool whose only consumer is a fused 1x1 convolution (pool -> pool_proj): the convolution reads the
    MaxPool's input and pools while it builds its input tile."""
    G = p.G
    if (p.f16 and not device.conv_f16_dma) or not getattr(conv, 'SUPPORTS_POOLED_INPUT', False) or device.fuse_poolconv == 0:
        return
    for cid in list(p.fusion):
        if G.nodes[cid]['type'] != 'Convolution':
            continue
        src = data_src(G, cid)
        if src is None or G.nodes[src]['type'] != 'MaxPool' or src in p.fused_away or len(list(G.successors(src))) != 1:
            continue
        psrc = data_src(G, src)
        if psrc is not None and conv.pooled_fusable(G.nodes[cid], G.nodes[src]):
            p.pool_conv[cid] = (src, psrc)
            p.fused_away.add(src)


def _pre_add(p, conv):
    """An Add of a per-INPUT-channel Const whose only consumer is a convolution that pads its input in a pass of its own (GoogLeNet:
    data/mean -> conv1): the padding pass adds the constant on the way and the Add is not dispatched (same fp32 add: same bits)."""
    G = p.G
    if not getattr(conv, 'SUPPORTS_PRE_ADD', False):
        return
    for cid in G.nodes:
        if G.nodes[cid]['type'] != 'Convolution' or cid in p.pool_conv:
            continue
        src = data_src(G, cid)
        if src is None or G.nodes[src]['type'] != 'Add' or src in p.fused_away or len(list(G.successors(src))) != 1:
            continue
        preds = list(G.pred[src])
        consts = [p_ for p_ in preds if G.nodes[p_]['type'] == 'Const']
        others = [p_ for p_ in preds if G.nodes[p_]['type'] != 'Const']
        if len(preds) != 2 or len(consts) != 1 or len(others) != 1:
            continue
        if conv.pre_add_fusable(G.nodes[cid], G.nodes[src], G.nodes[consts[0]], f16=p.f16):
            p.pre_add[cid] = (src, consts[0], others[0])
            p.fused_away.add(src)


def _siblings(p, conv, fuse_siblings):
    """Fused chains that read the SAME tensor with the same geometry and activation (an inception module's 1x1, 3x3_reduce, 5x5_reduce)
    are one launch of the first in schedule order, each output with the bits of its own launch (Convolution.launch_siblings)."""
    G = p.G
    if (p.f16 and not device.conv_f16_dma) or not fuse_siblings or not getattr(conv, 'SUPPORTS_SIBLINGS', False):
        return
    position = {t: i for i, t in enumerate(p.order)}
    groups = {}
    for cid, f in p.fusion.items():
        if G.nodes[cid]['type'] != 'Convolution':
            continue
        src = next((G.edges[(p_, cid)]['connection'][:2] for p_ in G.pred[cid] if G.edges[(p_, cid)]['connection'][3] == 0), None)
        if src is None or G.nodes[src[0]]['type'] == 'Const':
            continue
        geometry = tuple(G.nodes[cid]['input'][1]['dims'][2:]) + tuple(G.nodes[cid]['data'].get(k_) for k_ in ('strides', 'pads_begin', 'pads_end', 'auto_pad'))
        groups.setdefault((tuple(src), f['act'], geometry), []).append(cid)
    for members in groups.values():
        members = sorted(members, key=position.get)[:6]
        if len(members) >= 2 and conv.siblings_fusable([G.nodes[m] for m in members]):
            p.siblings[members[0]] = members[1:]
            p.fused_away.update(members[1:])


def _stem_conv(p, plugins):
    """fp32 IRs: MaxPool + LRN whose only reader is a fused chain that stands alone: the convolution rides in that launch too (GoogLeNet:
    pool1/3x3_s2 -> pool1/norm1 -> conv2/3x3_reduce) and the MaxPool task returns the chain's output."""
    G, pool = p.G, plugins.get('MaxPool')
    if p.f16 or device.fuse_stem_conv == 0 or pool is None or not getattr(pool, 'SUPPORTS_FUSED_LRN_CONV', False):
        return
    for pid, lid in p.lrn_pool.items():
        if G.nodes[pid]['type'] != 'MaxPool':
            continue
        readers = list(G.successors(lid))
        if len(readers) != 1 or G.edges[(lid, readers[0])]['connection'][3] != 0:
            continue
        cid = readers[0]
        f = p.fusion.get(cid)
        if f is None or G.nodes[cid]['type'] != 'Convolution' or f['into'] is not None or any(cid in m for m in (p.siblings, p.fused_away, p.pool_conv, p.pre_add)):
            continue
        if pool.lrn_conv_fusable(G.nodes[pid], G.nodes[lid], G.nodes[cid]):
            p.stem_conv[pid] = cid
            p.fused_away.update(p.chain(cid))


def _stem_pool(p, plugins):
    """fp32 IRs: a fused chain that stands alone and is read only by a MaxPool that heads a `stem_conv` launch (GoogLeNet: conv1/7x7_s2 ->
    pool1/3x3_s2): the convolution's launch writes the pooled tensor as a second output and hands it to the MaxPool task, whose launch is
    then LRN + 1x1 convolution only.  Nothing else of the plan changes: the chain's port still gets the convolution's own output.
    PVHIP_FUSE_STEM_POOL: 1 = by the size rule of the native query, 2 = wherever supported, 0 = never."""
    G, conv, pool = p.G, plugins.get('Convolution'), plugins.get('MaxPool')
    if p.f16 or device.fuse_stem_pool == 0 or not getattr(conv, 'SUPPORTS_POOLED_OUTPUT', False) or not getattr(pool, 'SUPPORTS_POOLED_INPUT', False):
        return
    for cid, f in p.fusion.items():
        if G.nodes[cid]['type'] != 'Convolution' or f['into'] is not None or any(cid in m for m in (p.siblings, p.fused_away, p.pool_conv)):
            continue
        readers = list(G.successors(p.tail(cid)))
        if len(readers) != 1 or readers[0] not in p.stem_conv or G.edges[(p.tail(cid), readers[0])]['connection'][3] != 0:
            continue
        pid = readers[0]
        if conv.pooled_output_fusable(G.nodes[cid], G.nodes[pid], by_size=device.fuse_stem_pool != 2, pre_add=cid in p.pre_add) and \
                pool.pooled_input_ok(G.nodes[pid], G.nodes[p.lrn_pool[pid]], G.nodes[p.stem_conv[pid]]):
            p.stem_pool[cid] = pid


def _c8(conv, modules=False):
    """FP16 IRs: fp16 tensors blocked by eight channels (device.BlockedHalf, the reader's MFMA operand as it stands).  PVHIP_CONV_F16_C8=1:
    between a 1x1 convolution and the 3x3 / 5x5 behind it only; =2 (default, `modules`): whole modules and the stem too; =0: never."""
    on = device.conv_f16_c8 != 0 and device.conv_f16_dma and getattr(conv, 'SUPPORTS_C8', False)
    return bool(on) and (not modules or (device.conv_f16_c8 == 2 and getattr(conv, 'SUPPORTS_C8_MODULES', False)))


def _relu_or_none(f):
    return f['act'] is None or f['act'][0] == 'relu'


def _c8_writers(p, conv):
    """A fused chain whose ONLY reader is a 3x3 / 5x5 convolution pvhip_conv2d_f16_c8 covers (3x3_reduce -> 3x3) hands its output over blocked."""
    G = p.G
    if not p.f16 or not _c8(conv):
        return
    for cid, f in p.fusion.items():
        if G.nodes[cid]['type'] != 'Convolution' or f['into'] is not None or cid in p.pool_conv or cid in p.pre_add or not _relu_or_none(f):
            continue
        tail = p.tail(cid)
        readers = list(G.successors(tail))
        if len(readers) != 1 or G.nodes[readers[0]]['type'] != 'Convolution' or G.edges[(tail, readers[0])]['connection'][3] != 0:
            continue
        rid = readers[0]
        if not any(rid in m for m in (p.pool_conv, p.pre_add, p.siblings, p.fused_away)) and \
                conv.c8_writer_ok(G.nodes[cid]) and conv.c8_reader_ok(G.nodes[rid]):
            p.c8_out.add(cid)


def _c8_stem(p, plugins):
    """... and the stem: a chain whose only reader is a 3x3 MaxPool (+ LRN: GoogLeNet's conv1 -> pool1 -> norm1) or LRN + MaxPool whose
    readers all take a blocked input: the MaxPool / LRN plugin works on a blocked tensor as it is."""
    G, conv, pool, lrn = p.G, plugins.get('Convolution'), plugins.get('MaxPool'), plugins.get('LRN')
    if not p.f16 or not _c8(conv, modules=True):
        return
    pool_reader = {pool_id: c_ for c_, (pool_id, _) in p.pool_conv.items()}

    def takes_blocked(r):
        if r in pool_reader:                         # a MaxPool folded into its pool_proj convolution
            return conv.c8_module_member_ok(G.nodes[pool_reader[r]], G.nodes[r])
        return r in p.fusion and G.nodes[r]['type'] == 'Convolution' and conv.c8_module_member_ok(G.nodes[r]) and \
            (r in p.c8_out or r in p.siblings)

    for cid, f in p.fusion.items():
        if G.nodes[cid]['type'] != 'Convolution' or f['into'] is not None or cid in p.pool_conv or cid in p.siblings or cid in p.fused_away \
                or not _relu_or_none(f):
            continue
        readers = list(G.successors(p.tail(cid)))
        if len(readers) != 1 or G.nodes[readers[0]]['type'] not in ('MaxPool', 'LRN') or readers[0] in p.fused_away:
            continue
        pid = readers[0]                                 # a 3x3 MaxPool (alone, or leading MaxPool + LRN), or an LRN leading LRN + MaxPool
        folded = p.lrn_pool.get(pid)
        # the SAME predicates the MaxPool / LRN plugins decide with at run time (blocked_ok): what is planned blocked is blocked
        if not (pool.blocked_ok(G.nodes[pid], G.nodes[folded] if folded is not None else None) if G.nodes[pid]['type'] == 'MaxPool'
                else folded is not None and lrn.blocked_ok(G.nodes[pid], G.nodes[folded])):
            continue
        after = list(G.successors(folded if folded is not None else pid))    # the node folded into the leading one carries the tensor
        if not after or not all(takes_blocked(r) for r in after):
            continue
        # the writer: the f16 1x1 launch, the f16 form of the LDS-DMA kernel (conv1), or -- its own input being blocked -- the module form
        own_blocked = any(data_src(G, cid) == p.tail(c_) for c_ in p.c8_out)
        if conv.c8_writer_ok(G.nodes[cid]) or conv.c8_dma_writer_ok(G.nodes[cid]) or \
                (own_blocked and conv.c8_module_member_ok(G.nodes[cid])):
            p.c8_out.add(cid)


def _c8_stem_conv(p, plugins):
    """... and the 1x1 convolution behind a blocked MaxPool + LRN rides in that launch, as in an fp32 IR (pvhip_maxpool3x3_lrn_conv1x1_c8)."""
    G, pool = p.G, plugins.get('MaxPool')
    if not p.f16 or not _c8(plugins.get('Convolution')) or device.conv_f16_c8 != 2 or device.fuse_stem_conv == 0 or not getattr(pool, 'SUPPORTS_FUSED_LRN_CONV', False):
        return
    tails = {p.tail(c_) for c_ in p.c8_out}
    for pid, lid in p.lrn_pool.items():
        if G.nodes[pid]['type'] != 'MaxPool' or pid in p.stem_conv:
            continue
        readers = list(G.successors(lid))
        if data_src(G, pid) not in tails or len(readers) != 1 or G.edges[(lid, readers[0])]['connection'][3] != 0:
            continue
        cid = readers[0]
        f = p.fusion.get(cid)
        if f is None or cid not in p.c8_out or cid in p.siblings or cid in p.fused_away or cid in p.pool_conv or not _relu_or_none(f):
            continue
        if pool.lrn_conv_fusable(G.nodes[pid], G.nodes[lid], G.nodes[cid], True):
            p.stem_conv[pid] = cid
            p.fused_away.update(p.chain(cid))


def _c8_modules(p, plugins):
    """Whole inception modules: a channel Concat whose members all read a tensor that WILL be blocked (`c8_out`, a blocked Concat or MaxPool
    of one, the entry tensor, converted once: `c8_entry`) and run on pvhip_conv2d_f16_c8_multi gets a blocked buffer (`c8_concat`)."""
    G, conv = p.G, plugins.get('Convolution')
    if not p.f16 or not _c8(conv, modules=True):
        return
    pool, lrn = (plugins.get(t) if hasattr(plugins.get(t), 'blocked_ok') else None for t in ('MaxPool', 'LRN'))
    blocked = {p.tail(cid) for cid in p.c8_out}

    def read_src(cid):                   # the tensor a convolution reads (through a MaxPool folded into its fetch)
        pooled = p.pool_conv.get(cid)
        return data_src(G, pooled[0]) if pooled is not None else data_src(G, cid)

    def member_ok(cid, assume=None):
        f, src, pooled = p.fusion.get(cid), read_src(cid), p.pool_conv.get(cid)
        if f is None or cid in p.pre_add or not _relu_or_none(f) or src is None or not (src in blocked or src == assume):
            return False
        return conv.c8_module_member_ok(G.nodes[cid], G.nodes[pooled[0]] if pooled is not None else None)

    members_of = {}
    for cid, f in p.fusion.items():
        if f['into'] is not None:
            members_of.setdefault(f['into'][0], []).append(cid)
    folded_pools = {p_[0] for p_ in p.pool_conv.values()}
    for nid in p.order:
        node = G.nodes[nid]
        if node['type'] == 'MaxPool':
            folded = G.nodes[p.lrn_pool[nid]] if nid in p.lrn_pool else None
            # MaxPool.blocked_ok / LRN.blocked_ok: the predicates the plugins themselves decide with at run time
            if data_src(G, nid) in blocked and nid not in p.lrn_pool.values() and pool is not None and pool.blocked_ok(node, folded):
                blocked.add(nid)          # the plugin pools a blocked tensor as it is (a folded pool hands its input on)
                if nid in p.lrn_pool:
                    blocked.add(p.lrn_pool[nid])      # MaxPool + LRN on the blocked tensor: the folded LRN carries it
        elif node['type'] == 'LRN' and nid in p.lrn_pool and data_src(G, nid) in blocked and lrn is not None \
                and lrn.blocked_ok(node, G.nodes[p.lrn_pool[nid]]):
            blocked.add(p.lrn_pool[nid])              # LRN + MaxPool on a blocked tensor: the folded MaxPool carries it
        elif node['type'] == 'Concat' and nid in p.concat_direct:
            members = members_of.get(nid, [])
            if not members or int(next(iter(node['output'].values()))['dims'][1]) % 16 != 0:
                continue          # (a blocked tensor holds whole 16-channel stages; its members write whole 8-channel blocks: c8_module_member_ok)
            # the first module: the tensor its 1x1 arms read is not blocked yet -- it is converted if that makes the module blocked
            entry = None
            outside = [s_ for s_ in {read_src(m) for m in members} if s_ not in blocked]
            if len(outside) == 1 and G.nodes[outside[0]]['type'] not in ('Convolution', 'Concat', 'Const', 'Parameter'):
                entry = outside[0]
                if not all(r in p.fusion or r in folded_pools for r in G.successors(entry)):
                    entry = None
            if all(member_ok(m, assume=entry) for m in members):
                p.c8_concat.add(nid)
                blocked.add(nid)
                if entry is not None:
                    p.c8_entry.add(entry)
                    blocked.add(entry)


def _order_for_locality(p):
    """Another legal order of the list schedule (round 4; scripts/exp_hoist.py): behind a sibling launch, MaxPool + pool_proj, which reads
    the SAME module input (still in L2 / the Infinity Cache), then the other arms by ascending output (5x5 before 3x3: the largest output
    is written closest to the next module's reads; one infer() -2 %).  Same launches, same bits; PVHIP_SCHEDULE_LOCALITY=0: the reference's."""
    if os.environ.get('PVHIP_SCHEDULE_LOCALITY', '1') == '0' or not p.siblings:
        return
    G = p.G
    order = list(p.order)
    position = {t: i for i, t in enumerate(order)}
    out_elems = lambda t: int(np.prod(next(iter(G.nodes[t]['output'].values()))['dims']))                # noqa: E731
    for lead in sorted(p.siblings, key=position.get):
        members = [lead] + list(p.siblings[lead])
        tails = {p.tail(m) for m in members}
        arms = [t for t in order if t not in p.fused_away and G.nodes[t]['type'] == 'Convolution' and data_src(G, t) in tails
                and t in p.fusion and t not in p.siblings]
        pooled = [c for c, (_, psrc) in p.pool_conv.items() if psrc == data_src(G, lead)]
        arms.sort(key=lambda t: (out_elems(t), position[t]))
        moved = pooled + arms
        # every moved task depends on the lead's launch (or on the lead's own input) and on constants only: any order behind the lead is legal
        if not all(G.nodes[p_]['type'] == 'Const' or p_ in tails or (t in pooled and p_ == p.pool_conv[t][0]) for t in moved for p_ in G.pred[t]):
            continue
        # a moved unit = the convolution with the nodes folded into it (its MaxPool in front, its Add / ReLU behind), so that the list
        # stays a topological order of the WHOLE graph
        units = [n_ for t in moved for n_ in ([p.pool_conv[t][0]] if t in pooled else []) + p.chain(t)]
        gone = set(units)
        rest = [t for t in order if t not in gone]
        at = max(rest.index(n_) for m in members for n_ in p.chain(m)) + 1
        order = rest[:at] + units + rest[at:]
    p.order = order
