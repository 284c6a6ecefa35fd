"""Which compute stream each launch of a pass goes to, and which cross-stream waits the pass issues.

``build`` is the static stream assignment of a fusion plan's task list; ``recorded_waits`` replays a plan through
``CaptureStreamModel``, the runtime's bookkeeping while a multi-stream hipGraph recording is open.  Both are pure functions of the
graph, the plan and the stream count: no device."""
from typing import NamedTuple


class StreamPlan(NamedTuple):
    stream_of: dict     # dispatched task -> stream, relative to the network's first stream
    waits: dict         # dispatched task -> the tasks on other streams it waits for, in input-port order
    records: set        # tasks that record an event (someone waits for them)


def build(G, fp, n: int) -> StreamPlan:
    """Static stream assignment of ``fp.order`` over ``n`` streams (the reference's list scheduler
    runs the branches of a module one after the other, :259-292).  The consumers of a tensor are ranked by
    the estimated time of the arm each one starts (the chain of single-consumer nodes behind it); the
    heaviest stays on the stream the tensor was produced on, the others go to the next streams, so the arms
    of a fan-out run side by side.  A tensor assembled by several producers (an eliminated Concat) counts as
    produced on the stream of the producer expected to finish last.  Both rules keep the critical path of
    consecutive modules on ONE stream: its kernels follow each other without waiting for a cross-stream event
    (measured 25-40 us per join), which only the lighter arms pay."""
    producers, handed_on = fp.writers, fp.handed_on     # (a MaxPool / Add folded into its consumer's fetch hands its input on)

    def prod(dims):
        out = 1
        for d in dims:
            out *= int(d)
        return out

    def cost(task, alone=False):     # rough device time of a task in microseconds (ranking only)
        if not alone and task in fp.siblings:
            return cost(task, True) + sum(cost(s_, True) for s_ in fp.siblings[task])
        node = G.nodes[task]
        out = prod(next(iter(node['output'].values()))['dims']) if node.get('output') else 0
        if node['type'] == 'Convolution':
            k = node['input'][1]['dims']
            return 2.0 * out * k[1] * k[2] * k[3] / 100e6 + 4.0 * out / 4.5e6
        if node['type'] == 'MatMul':
            return 2.0 * out * node['input'][0]['dims'][-1] / 20e6
        inp = prod(node['input'][0]['dims']) if node.get('input') else 0
        return 4.0 * (inp + out) / 4.5e6

    dispatched = [t for t in fp.order if t not in fp.fused_away and G.nodes[t]['type'] not in ('Const', 'Parameter')]
    position = {t: i for i, t in enumerate(dispatched)}

    def consumers(nid):              # dispatched tasks that read the tensor of graph node nid
        out = []
        for succ in G.successors(nid):
            if succ in fp.concat_direct or succ in handed_on:
                out += [c_ for c_ in consumers(succ) if c_ not in out]     # (a folded Add / MaxPool hands the tensor on)
            elif succ in position and succ not in out:
                out.append(succ)
        return sorted(out, key=position.get)

    def joins(task):                 # the task writes into a tensor that other tasks write too
        f = fp.fusion.get(task)
        return f is not None and f['into'] is not None

    arm_memo = {}

    def arm_cost(task):              # the task plus the chain of sole consumers behind it, up to the next fork / join
        if task not in arm_memo:
            total, cur = 0.0, task
            while True:
                total += cost(cur)
                nxt = consumers(fp.output_of(cur))
                if joins(cur) or len(nxt) != 1:
                    break
                srcs = {p for pred in G.pred[nxt[0]] for p in producers(pred)}
                if srcs != {cur}:
                    break
                cur = nxt[0]
            arm_memo[task] = total
        return arm_memo[task]

    stream_of, waits, records, rank_of, finish, width_of = {}, {}, set(), {}, {}, {}
    for task in dispatched:
        preds = sorted(G.pred[task], key=lambda p: G.edges[(p, task)]['connection'][3])
        primary = next((p for p in preds if producers(p)), None)
        while primary in handed_on:          # read through a folded Add / MaxPool: the arms fork at ITS input
            primary = handed_on[primary]
        if primary is None:
            stream_of[task] = 0
            finish[task] = cost(task)
        else:
            if primary not in rank_of:           # heaviest arm first; schedule order breaks ties
                cons, writers_ = consumers(primary), producers(primary)
                if len(writers_) == 1 and writers_[0] in fp.siblings:
                    # one launch wrote several tensors: the arms behind ALL of them fan out from its stream
                    cons = []
                    for t in [writers_[0]] + list(fp.siblings[writers_[0]]):
                        if not joins(t):         # (a tensor assembled with others is ranked when its last writer is known)
                            cons += [c for c in consumers(fp.output_of(t)) if c not in cons]
                arms = sorted(cons, key=lambda t: (-arm_cost(t), position[t]))
                # the lighter arms behind a sibling launch skip the streams taken by the arms the launch itself forked with
                skip = width_of.get(writers_[0], 1) - 1 if (len(writers_) == 1 and writers_[0] in fp.siblings) else 0
                rank_of[primary] = {t: (j + skip if j else 0) for j, t in enumerate(arms)}
            srcs = producers(primary)
            base = max(srcs, key=lambda p: (finish[p], -position[p]))     # the producer expected to finish last
            stream_of[task] = (stream_of[base] + rank_of[primary].get(task, 0)) % n
            width_of[task] = len(rank_of[primary])
            finish[task] = finish[base] + cost(task)
        deps = []
        for pred in preds:
            for p in producers(pred):
                if stream_of[p] != stream_of[task] and p not in deps:
                    deps.append(p)
        waits[task] = deps
        records.update(deps)
    return StreamPlan(stream_of, waits, records)


class CaptureStreamModel:
    """What ROCm 7.2's runtime keeps per stream while a multi-stream hipGraph recording is open, restated from the disassembly of
    its hipStreamWaitEvent / Stream::EndCapture (libamdhip64.so.7.2.70200 +0x2f63b9 / +0x2df7f0; profiles/r04_capture.md).

    When a stream W that is not the origin of the capture waits for an event recorded on stream E, and E's current parent is not
    W, the runtime sets parent(W) = E and appends W to E's list of parallel streams (once) -- on EVERY such wait, not only on the
    one that makes W join.  hipStreamEndCapture then walks those lists recursively from the origin and clears them on the way
    back.  The parent test stops a 2-cycle only while E's parent still IS W; after E has waited for a third stream in between,
    W <-> E (or a longer ring) closes, the walk never returns and the process dies of stack overflow inside hipStreamEndCapture
    (what LESSONS.md lesson 30 filed as "crashes inside the runtime").  The origin never registers anywhere, so a dependency that
    would close a ring is RELAYED through it: the origin waits for E's event, records a fresh one, W waits for that."""

    def __init__(self):
        self.parent = {}        # non-origin stream -> stream of the event it last registered under
        self.lists = {}         # stream -> streams in its parallel-capture list

    def _reaches(self, src, dst):
        todo, seen = [src], set()
        while todo:
            cur = todo.pop()
            if cur == dst:
                return True
            if cur not in seen:
                seen.add(cur)
                todo.extend(self.lists.get(cur, ()))
        return False

    def wait(self, waiter: int, event_stream: int) -> str:
        """Stream `waiter` is about to wait for an event recorded on `event_stream` (0 = the origin).  'plain': issue the wait;
        'relay': it would close a ring in the runtime's lists -- go through the origin (the bookkeeping of the relay's own two
        waits is applied here)."""
        if waiter == 0 or waiter == event_stream:
            return 'plain'                              # the origin registers nowhere
        if self.parent.get(event_stream) == waiter:
            return 'plain'                              # the runtime's own test: nothing is registered
        if event_stream != 0 and self._reaches(waiter, event_stream):
            self.parent[waiter] = 0                     # relayed: origin waits (registers nothing), waiter waits for the origin's event
            self.lists.setdefault(0, set()).add(waiter)
            return 'relay'
        self.parent[waiter] = event_stream
        self.lists.setdefault(event_stream, set()).add(waiter)
        return 'plain'

    def has_ring(self) -> bool:
        return any(self._reaches(w, s) for s, ws in self.lists.items() for w in ws)


def recorded_waits(sp: StreamPlan, fp):
    """The cross-stream waits a RECORDING of stream plan `sp` (None: no plan) of fusion plan `fp` makes, in dispatch order, as (how,
    waiting stream, event's stream, producer task) with how = 'plain' | 'relay' (CaptureStreamModel), and the model after them --
    what the dispatcher issues while a capture is open, computed from the plans alone."""
    model, out = CaptureStreamModel(), []
    if sp is not None:
        for task in fp.order:
            if task in fp.fused_away or task not in sp.stream_of:
                continue
            for dep in sp.waits[task]:
                out.append((model.wait(sp.stream_of[task], sp.stream_of[dep]), sp.stream_of[task], sp.stream_of[dep], dep))
    return out, model
