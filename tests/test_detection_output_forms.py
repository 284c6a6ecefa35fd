"""Every size regime and attribute of the DetectionOutput launcher (pvhip_detect.hip), one explicit row per regime.

pvhip_detection_output_f32 is three kernels and a workspace: candidates and records run 1024 threads over one image each (compact<1024>
gives a thread ceil(n / 1024) consecutive flags), suppression is tiled by 256 candidates, the dynamic LDS passes 64 KB from 4725 priors
(candidates kernel) and 7678 priors (records kernel) and the launcher refuses from 11499 priors.  ROWS names those sizes directly.

Inputs are constructed so that the number of candidates M and of survivors K of every image is known before anything runs:
  * CORNER with variance_encoded_in_target: a box is prior + loc.  Every prior is a cell of side 2^-7 on a grid with one free cell
    between neighbours, `loc` moves it to its target cell and shifts it by 0 / 1 / 2 quarter cells in x.  All coordinates are multiples
    of 2^-9 below 4, so boxes, areas and intersections are exact in fp32.  Two boxes of a cell shifted by 0 / 1 / 2 quarters against each
    other have IoU 1 / 0.6 / (1/3); boxes of different cells have IoU 0.
  * scores come from LADDER: (4096 + j) 2^(e - 13), neighbours at least 2^-13 = 1.2e-4 apart relatively; LADDER[0] is the confidence
    threshold 0.5 itself.
designed_keep() applies the reference's rule to the DESIGN (which members of a cell overlap is known from their shifts, no IoU is
computed); margins() recomputes every decision quantity from the fp32 inputs in float64.

CPU part (no device): for every row, margins() finds every score / IoU / rank decision either an exact tie the row declares or at least
helpers.REL_TOL away, and the row's promised M and K are what margins() and the oracle find; suppression rows drop at least a quarter of
each image's candidates; per code type the four clip settings give at least three distinct oracle outputs.

GPU part: every row through the plugin against the oracle plugin (itself pinned to the reference by tests/golden/ops/detout_*.npz).
No fp32 implementation can differ on such inputs: rank, class and score columns bit for bit, rows past the terminator zero, CORNER
boxes bit for bit, CENTER_SIZE boxes within 1e-6 (exp is evaluated in double by two libraries; the count of box elements that are not
bit-identical is printed).

NaN rule (include/pvhip.h): a prior with a NaN among its class scores is never a candidate -- the reference's np.argsort puts a NaN last,
so the reversed order picks it and NaN > threshold is false.  One row deliberately has no suppression: 'suppress-nms-1.0' (IoU never
exceeds 1, so identical boxes at nms_threshold 1.0 all stay; the quarter-suppressed rule cannot apply to it).

Edits to pvhip_detect.hip that these rows were seen to catch on an MI355X (each alone, everything else passing): the records kernel's tie
rule `r > q` turned to `r < q` -> records-tied-survivors; the suppress loop's `!(sj < sk)` replaced by `sk < sj` -> suppress-structure;
compact's chunk by floor instead of ceil -> nearly every row; the terminator written when K <= records -> records-keep_top_k; the
candidates loop without the NaN rule -> nan-inf.
"""
import collections
import ctypes
import functools
import importlib

import numpy as np
import pytest

import helpers
from helpers import assert_bit_exact, assert_close, first_out

gpu = pytest.mark.gpu

S = 2.0 ** -7                 # cell side
COLS = 64                     # cells per grid row; cell c sits at (2 (c % COLS) S, 2 (c // COLS) S)
THR, NMS = 0.5, 0.45
CORNER, CENTER = 'caffe.PriorBoxParameter.CORNER', 'caffe.PriorBoxParameter.CENTER_SIZE'
LADDER = np.array([(4096 + t % 4096) * 2.0 ** (t // 4096 - 13) for t in range(3 * 4096)], dtype=np.float32)
LOW = np.float32(0.25)        # best score of a prior that is no candidate
REST = np.float32(0.125)      # every other class score


def hip_plugin():
    return importlib.import_module('pyopenvino_amd.op_plugins.DetectionOutput')


def oracle_plugin():
    return importlib.import_module('oracle.op_plugins.DetectionOutput')


# --------------------------------------------------------------------------------------------------------------- constructed images
def cell_boxes(cell, q):
    """Target boxes (float64, exact): cell `cell` shifted by q quarter cells in x; q < 0: a zero-area box (xmax = xmin)."""
    x0 = 2.0 * (cell % COLS) * S + np.maximum(q, 0) * (S / 4)
    y0 = 2.0 * (cell // COLS) * S
    return np.stack([x0, y0, np.where(q < 0, x0, x0 + S), y0 + S], 1)


class Img:
    """One image over P priors: per prior its target cell, quarter shift, candidacy, class and score; `conf_edits` / `loc_edits`
    (prior, column, value) are written last."""

    def __init__(self, P, C=3, layout='solo', seed=1):
        p = np.arange(P)
        n = (P + 2) // 3
        self.P, self.C = P, C
        self.cell, self.q = {'solo': (p, p * 0), 'near': (p // 3, p % 3), 'far': (p % n, p // n)}[layout]
        self.cand = np.full(P, C > 1)                          # (C == 1: the only class is class 0)
        self.cls = (1 + p % (C - 1)) if C > 1 else p * 0
        self.score = LADDER[1 + np.random.RandomState(seed).permutation(P)]
        self.conf_edits, self.loc_edits = [], []
        self.nms = NMS

    def only(self, m, seed):
        """m candidates, a seeded choice of the priors."""
        self.cand[:] = False
        self.cand[np.random.RandomState(seed).permutation(self.P)[:m]] = True
        return self

    def chains(self):
        """Members A, B, C of a cell (shifts 0, 1, 2) score A > B > C in even cells and C > B > A in odd ones: the reference drops
        B and then the box B beats, greedy NMS would keep it."""
        rank = np.where(self.cell % 2 == 0, 2 - self.q, self.q)
        self.score = LADDER[1 + 3 * self.cell + rank]
        return self

    def first_cells(self, n):
        self.cand = self.cell < n
        return self

    def keep(self):
        return designed_keep(self.cell, self.q, self.cand, self.score, self.nms)

    def loc(self, priors):
        loc = (cell_boxes(self.cell, self.q) - priors).astype(np.float32)
        for p, c, v in self.loc_edits:
            loc[p, c] = v
        return loc.reshape(-1)

    def conf(self):
        conf = np.full((self.P, self.C), REST, dtype=np.float32)
        if self.C == 1:
            conf[:, 0] = self.score
        else:
            conf[np.arange(self.P), self.cls] = np.where(self.cand, self.score, LOW)
        for p, c, v in self.conf_edits:
            conf[p, c] = v
        return conf.reshape(-1)


def designed_keep(cell, q, cand, score, nms):
    """The reference's pair rule on the design: two candidates of a cell overlap by the IoU their shifts give (0 / 1 / 2 quarters: 1 /
    0.6 / 1/3; zero-area boxes: never); of an overlapping pair the lower score goes, the later one on a tie, dropped or not."""
    keep = cand.copy()
    members = collections.defaultdict(list)
    for p in np.nonzero(cand)[0]:
        members[int(cell[p])].append(int(p))
    for group in members.values():
        for i, a in enumerate(group):
            for b in group[i + 1:]:
                if q[a] < 0 or q[b] < 0:
                    continue
                if {0: 1.0, 1: 0.6, 2: 1.0 / 3}[abs(int(q[a]) - int(q[b]))] > nms:
                    keep[a if score[a] < score[b] else b] = False
    return keep


def grid_priors(P):
    return cell_boxes(np.arange(P), np.zeros(P, dtype=int))


# ---- the images of the rows
def pair(P, layout='near'):
    """Every prior a candidate in one image, a seeded third of them in the other."""
    return [Img(P, 3, layout, seed=P), Img(P, 3, layout, seed=P + 1).only((P + 2) // 3, seed=P + 2)]


def ladder_images(P):
    ms = sorted({min(m, P) for m in (0, 1, 255, 256, 257, 512, 513, 1100)})
    return [Img(P, 3, 'far', seed=10 + i).only(m, seed=20 + i) for i, m in enumerate(ms)]


def tie_far(P):
    """Members 0 and 1 of a cell are the same box with the same score, a tile or more apart in candidate order: the later one goes.
    Member 2 (half a cell away) stays."""
    im = Img(P, 3, 'far')
    im.q = np.where(im.q == 1, 0, im.q)
    im.score = LADDER[1 + 2 * im.cell + (im.q == 2)]
    return im


def zero_area(P):
    """Chains, but in every fifth cell members 0 and 1 are the same zero-area box: their IoU is 0 / 0."""
    im = Img(P, 3, 'far').chains()
    im.q = np.where((im.cell % 5 == 0) & (im.q < 2), -1, im.q)
    return im


def identical(P):
    im = Img(P, 3, 'far')
    im.q = im.q * 0
    im.nms = 1.0
    return im


def survivor_ties(P):
    """Nothing overlaps and priors 2i, 2i + 1 share a score: the later one ranks first, also across the last record."""
    im = Img(P, 3, 'solo')
    im.score = LADDER[1 + np.random.RandomState(3).permutation((P + 1) // 2)[np.arange(P) // 2]]
    return im


def threshold_cases(P):
    """By prior % 5: 0 a best score equal to the threshold (out); 1 best class 0 (out); 2 classes 1 and 2 equal (class 2); 3 classes
    0 and 2 equal (class 2); 4 plain."""
    im = Img(P, 3, 'solo')
    for p in range(P):
        kind = p % 5
        if kind == 0:
            im.cand[p] = False
            im.conf_edits.append((p, im.cls[p], LADDER[0]))
        elif kind == 1:
            im.cand[p] = False
            im.conf_edits.append((p, 0, im.score[p]))
        elif kind in (2, 3):
            im.cls[p] = 2
            im.conf_edits.append((p, 1 if kind == 2 else 0, im.score[p]))
    return im


NAN, INF = np.float32(np.nan), np.float32(np.inf)


def nan_scores(P):
    """C = 4, every prior otherwise a candidate.  By prior % 50: 7 NaN at class 0; 17 NaN at a middle class below a finite best at the
    last; 27 NaN at the last class; 37 NaN in two classes.  None of them is a candidate."""
    im = Img(P, 4, 'near', seed=5)
    for p in range(P):
        kind = p % 50
        if kind in (7, 17, 27, 37):
            im.cand[p] = False
            im.cls[p] = 1 if kind == 27 else 3
            im.conf_edits.append((p, im.cls[p], im.score[p]))
            for c in {7: (0,), 17: (1,), 27: (3,), 37: (1, 2)}[kind]:
                im.conf_edits.append((p, c, NAN))
    return im


def infinities(P):
    """Prior 100's best score is +inf (kept, first, the score column holds inf); priors 50 and 200 are -inf in every class (out)."""
    im = Img(P, 4, 'near', seed=6)
    im.score[100] = INF
    for p in (50, 200):
        im.cand[p] = False
        im.conf_edits += [(p, c, -INF) for c in range(4)]
    return im


def nan_loc(P):
    """Priors 31 and 150 have a NaN in loc: their IoU with anything is NaN, they suppress nothing, stay and are stored as they are."""
    im = Img(P, 4, 'near', seed=7)
    for p, c in ((31, 0), (150, 3)):
        im.q[p] = -1                        # (for designed_keep: overlaps nothing)
        im.loc_edits.append((p, c, NAN))
    return im


# ---- seeded inputs of the attribute rows: SSD-like priors, locs large enough that a fifth of the boxes leave [0, 1]
ATTR_P = 300
LOC_SCALE = {(CORNER, True): 0.05, (CORNER, False): 0.5, (CENTER, True): 0.25, (CENTER, False): 2.0}
ATTR_SEED = {(CORNER, True): 44, (CORNER, False): 83, (CENTER, True): 84, (CENTER, False): 45}     # seeds at which every margin holds (test_cpu_row)


def attr_priors():
    c = (np.arange(100) + 0.0)
    cx, cy = (c % 10 + 0.5) / 10, (c // 10 + 0.5) / 10
    boxes = []
    for w, h in ((0.15, 0.15), (0.3, 0.15), (0.15, 0.3)):
        boxes.append(np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1))
    boxes = np.stack(boxes, 1).reshape(ATTR_P, 4)
    var = np.tile(np.array([0.1, 0.1, 0.2, 0.2]), (ATTR_P, 1))
    return np.stack([boxes.reshape(-1), var.reshape(-1)])[None].astype(np.float32)


def attr_inputs(code, enc):
    seed = ATTR_SEED[code, enc]
    loc = (np.random.RandomState(seed).standard_normal((2, ATTR_P * 4)) * LOC_SCALE[code, enc]).astype(np.float32)
    imgs = [Img(ATTR_P, 3, 'solo', seed=seed), Img(ATTR_P, 3, 'solo', seed=seed + 10).only(150, seed=seed + 20)]
    return loc, np.stack([im.conf() for im in imgs]), attr_priors(), [int(im.cand.sum()) for im in imgs]


# K of the two images of the attribute rows by (code type, variance encoded, clip before): seeded locs, so these are recorded, not derived
# (test_cpu_row holds them against margins() and the oracle)
ATTR_K = {(CORNER, True, False): [224, 129], (CORNER, True, True): [210, 126], (CORNER, False, False): [232, 139], (CORNER, False, True): [216, 133],
          (CENTER, True, False): [190, 122], (CENTER, True, True): [158, 106], (CENTER, False, False): [212, 129], (CENTER, False, True): [187, 123]}


# --------------------------------------------------------------------------------------------------------------------- the table
class Row:
    """id, regime (what the row is there for), P, C, the images (a callable -> [Img]), attributes.  `ties`: which exact ties the row
    is built to have ('score': equal scores decide a pair or a rank, 'iou': an IoU equal to the threshold, 'nan': NaN IoUs);
    min_dropped: the share of each image's candidates that must be suppressed."""

    def __init__(self, id_, regime, P, images, C=3, keep_top_k=200, top_k=-1, nms=NMS, code=CORNER, enc=True, clip_before=False,
                 clip_after=False, ties=(), min_dropped=0.0, seeded=False):
        self.id, self.regime, self.P, self.C, self.images = id_, regime, P, C, images
        self.keep_top_k, self.top_k, self.nms, self.code, self.enc = keep_top_k, top_k, nms, code, enc
        self.clip_before, self.clip_after, self.ties, self.min_dropped, self.seeded = clip_before, clip_after, set(ties), min_dropped, seeded

    def __repr__(self):
        return self.id

    @property
    def records(self):
        if self.keep_top_k > 0:
            return self.keep_top_k
        return self.top_k * self.C if self.top_k > 0 else self.C * self.P

    def data(self, **over):
        d = {'num_classes': str(self.C), 'keep_top_k': str(self.keep_top_k), 'top_k': str(self.top_k), 'nms_threshold': repr(self.nms),
             'confidence_threshold': repr(THR), 'code_type': self.code, 'variance_encoded_in_target': str(self.enc).lower(),
             'clip_before_nms': str(self.clip_before).lower(), 'clip_after_nms': str(self.clip_after).lower(),
             'share_location': 'true', 'normalized': 'true', 'background_label_id': '0'}
        d.update(over)
        return d


KR = 80                       # records of the row whose survivor counts straddle it
ROWS = []
for P_ in (1, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 3100):
    ROWS.append(Row('priors-{}'.format(P_), 'compact<1024> chunk {}: M = P and M = P / 3'.format((P_ + 1023) // 1024), P_,
                    functools.partial(pair, P_), ties=()))
ROWS += [
    Row('candidates-1100', 'M = 0, 1, 255, 256, 257, 512, 513, 1100 side by side: suppress tiles, count[img], workspace strides', 1100,
        functools.partial(ladder_images, 1100)),
    Row('candidates-300', 'the same ladder clipped to P = 300', 300, functools.partial(ladder_images, 300)),
    Row('suppress-structure', 'chains inside a tile and across three tiles; an equal-score identical pair across tiles; 0 / 0 IoU', 1100,
        lambda: [Img(1100, 3, 'near').chains(), Img(1100, 3, 'far').chains(), tie_far(1100), zero_area(1100)],
        ties=('score', 'nan'), min_dropped=0.25),
    Row('suppress-nms-1.0', 'identical boxes, IoU == nms_threshold == 1: not above it, all stay', 1100, lambda: [identical(1100)],
        nms=1.0, ties=('iou',)),
    Row('records-keep_top_k', 'K = records + 1, 4 records, records - 1, records, 2', 1100,
        lambda: [Img(1100, 3, 'near').chains().first_cells(k) for k in (KR + 1, 4 * KR, KR - 1, KR, 2)], keep_top_k=KR, min_dropped=0.25),
    Row('records-top_k', 'records = top_k C = 6: K = 5, 6, 7, 100', 300,
        lambda: [Img(300, 3, 'near').chains().first_cells(k) for k in (5, 6, 7, 100)], keep_top_k=-1, top_k=2),
    Row('records-all', 'records = C P = 900: K = 0, 100, 300', 300,
        lambda: [Img(300, 3, 'solo').only(0, 1), Img(300, 3, 'near').chains(), Img(300, 3, 'solo', seed=9)], keep_top_k=-1, top_k=-1),
    Row('records-tied-survivors', 'equal scores among survivors: the later candidate ranks first, also at the last record', 300,
        lambda: [survivor_ties(300)], keep_top_k=21, ties=('score',)),
    Row('threshold', 'score == threshold out, best class 0 out, equal best classes take the later', 300, lambda: [threshold_cases(300)],
        keep_top_k=300),
    Row('classes-1', 'C = 1: the only class is the background, never a candidate', 300, lambda: [Img(300, 1, 'solo')], C=1),
    Row('classes-2', 'C = 2', 300, lambda: [Img(300, 2, 'near')], C=2),
]
for code_ in (CORNER, CENTER):
    for enc_ in (True, False):
        for cb_ in (False, True):
            for ca_ in (False, True):
                ROWS.append(Row('attr-{}-enc{:d}-before{:d}-after{:d}'.format(code_.rsplit('.', 1)[1], enc_, cb_, ca_),
                                'attribute combination', ATTR_P, None, code=code_, enc=enc_, clip_before=cb_, clip_after=ca_, seeded=True))
for P_, why in ((4724, 'below the candidates kernel\'s 64 KB'), (4725, 'first hipFuncSetAttribute (candidates); thousands of records'),
                (7677, 'below the records kernel\'s 64 KB'), (7678, 'second hipFuncSetAttribute (records)'),
                (8732, 'SSD300'), (11498, 'the largest accepted')):
    ROWS.append(Row('lds-{}'.format(P_), why, P_, (lambda P=P_: [Img(P, 3, 'near', seed=P), Img(P, 3, 'near', seed=P + 1).only(300, seed=P + 2)]),
                    keep_top_k=4000 if P_ == 4725 else 200))
ROWS.append(Row('nan-inf', 'NaN class scores (never a candidate), +inf / -inf scores, NaN loc', 300,
                lambda: [nan_scores(300), infinities(300), nan_loc(300)], C=4, keep_top_k=300, ties=('nan',)))
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(row_id):
    """The row's node and inputs, the promised M and K of every image, the oracle's records (computed once, never modified)."""
    row, c = BY_ID[row_id], Case()
    if row.seeded:
        loc, conf, priors, c.M = attr_inputs(row.code, row.enc)
        c.K = ATTR_K[row.code, row.enc, row.clip_before]
    else:
        imgs = row.images()
        assert all(im.P == row.P and im.C == row.C and im.nms == row.nms for im in imgs)
        pri = grid_priors(row.P)
        priors = np.stack([pri.reshape(-1), np.full(row.P * 4, 0.1)])[None].astype(np.float32)
        loc, conf = np.stack([im.loc(pri) for im in imgs]), np.stack([im.conf() for im in imgs])
        c.M, c.K = [int(im.cand.sum()) for im in imgs], [int(im.keep().sum()) for im in imgs]
    c.inputs = {0: loc, 1: conf, 2: priors}
    c.node = node_of(row, c.inputs)
    c.want = first_out(oracle_plugin().compute(c.node, c.inputs))
    for a in (loc, conf, priors, c.want):
        a.setflags(write=False)
    return c


def node_of(row, inputs, **over):
    return {'name': 'DetectionOutput_' + row.id, 'type': 'DetectionOutput', 'version': 'opset1', 'data': row.data(**over),
            'input': {i: {'precision': 'FP32', 'dims': tuple(a.shape)} for i, a in inputs.items()},
            'output': {3: {'precision': 'FP32', 'dims': ()}}}


# ------------------------------------------------------------------------------------------------------------- float64 margins
def rel_gap(a, b):
    """|a - b| relative to the larger magnitude (NaN when one of them is infinite: callers leave those out)."""
    with np.errstate(invalid='ignore'):
        return np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-30)


def decode64(row, loc, pri, var, clip):
    """Boxes of every prior in float64, from the fp32 inputs."""
    if row.code == CORNER:
        box = pri + (loc if row.enc else var * loc)
    else:
        pw, ph = pri[:, 2] - pri[:, 0], pri[:, 3] - pri[:, 1]
        pcx, pcy = (pri[:, 0] + pri[:, 2]) / 2, (pri[:, 1] + pri[:, 3]) / 2
        v = np.ones_like(var) if row.enc else var
        cx, cy = v[:, 0] * loc[:, 0] * pw + pcx, v[:, 1] * loc[:, 1] * ph + pcy
        w, h = np.exp(v[:, 2] * loc[:, 2]) * pw, np.exp(v[:, 3] * loc[:, 3]) * ph
        box = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    return np.clip(box, 0, 1) if clip else box


def margins(row, inputs, img):
    """Every decision of image `img` recomputed in float64.  -> dict: M, K; the smallest relative distance of a best score from the
    threshold / between the scores of an overlapping pair / between rank neighbours among the survivors, and the smallest |IoU -
    nms_threshold| over all candidate pairs -- exact ties left out and counted instead (score_ties, iou_ties, nan_ious); `outside`:
    the share of candidate boxes (before any clip) with a coordinate outside [0, 1]."""
    P, C = row.P, row.C
    loc = inputs[0][img].astype(np.float64).reshape(P, 4)
    conf = inputs[1][img].astype(np.float64).reshape(P, C)
    pri, var = (inputs[2][0, k].astype(np.float64).reshape(P, 4) for k in (0, 1))
    poisoned = np.isnan(conf).any(1)
    cls = C - 1 - np.argmax(np.where(np.isnan(conf), -np.inf, conf)[:, ::-1], axis=1)            # ties: the later class
    score = conf[np.arange(P), cls]
    m = {'score_ties': 0, 'iou_ties': 0, 'nan_ious': 0}
    gap = rel_gap(score[~poisoned], THR)
    m['thr_ties'] = int((gap == 0).sum())
    m['thr'] = float(gap[gap > 0].min()) if (gap > 0).any() else np.inf
    sel = np.nonzero(~poisoned & (score > THR) & (cls != 0))[0]
    M = len(sel)
    box, sc = decode64(row, loc, pri, var, row.clip_before)[sel], score[sel]
    unclipped = decode64(row, loc, pri, var, False)[sel]
    with np.errstate(invalid='ignore'):
        m['outside'] = float(((unclipped < 0) | (unclipped > 1)).any(1).mean()) if M else 0.0
    area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
    keep = np.ones(M, dtype=bool)
    m['iou'], m['pair'] = np.inf, np.inf
    for i0 in range(0, M, 256):                                # pairs (i, j > i), 256 rows of i at a time
        a = box[i0:i0 + 256, None, :]
        with np.errstate(invalid='ignore', divide='ignore'):
            w = np.minimum(a[..., 2], box[None, :, 2]) - np.maximum(a[..., 0], box[None, :, 0])
            h = np.minimum(a[..., 3], box[None, :, 3]) - np.maximum(a[..., 1], box[None, :, 1])
            touch = ~((w < 0) | (h < 0))                       # (NaN extents: neither below 0, as in both implementations)
            touch &= np.arange(M)[None, :] > (i0 + np.arange(a.shape[0]))[:, None]
            ii, jj = np.nonzero(touch)
            inter = w[ii, jj] * h[ii, jj]
            ii += i0
            iou = inter / (area[ii] + area[jj] - inter)
        nan = np.isnan(iou)
        m['nan_ious'] += int(nan.sum())
        d = np.abs(iou[~nan] - row.nms)
        m['iou_ties'] += int((d == 0).sum())
        if (d > 0).any():
            m['iou'] = min(m['iou'], float(d[d > 0].min()))
        with np.errstate(invalid='ignore'):
            over = iou > row.nms
        ii, jj = ii[over], jj[over]
        g = rel_gap(sc[ii], sc[jj])
        m['score_ties'] += int((g == 0).sum())
        if (g > 0).any():
            m['pair'] = min(m['pair'], float(g[g > 0].min()))
        first_loses = sc[ii] < sc[jj]
        keep[ii[first_loses]] = False
        keep[jj[~first_loses]] = False
    m['iou'] = min(m['iou'], row.nms)                          # pairs that do not touch have IoU 0
    kept = np.sort(sc[keep])
    g = rel_gap(kept[1:], kept[:-1])
    g = g[~np.isnan(g)]
    m['score_ties'] += int((g == 0).sum())
    m['rank'] = float(g[g > 0].min()) if (g > 0).any() else np.inf
    m['M'], m['K'] = M, int(keep.sum())
    return m


def oracle_counts(row, c, img):
    """(M, K as far as the records show it) of one image from the oracle: M from a run that suppresses nothing (nms_threshold 1: no
    IoU is above it) and has room for every prior; K from the row's own records: the terminator's place, else `records` (or more)."""
    one = {0: c.inputs[0][img:img + 1], 1: c.inputs[1][img:img + 1], 2: c.inputs[2]}
    full = first_out(oracle_plugin().compute(node_of(row, one, nms_threshold='1.0', keep_top_k='-1', top_k='-1'), one))[0, 0]
    M = int(np.nonzero(full[:, 0] == -1)[0][0])
    rec = c.want[0, 0, img * row.records:(img + 1) * row.records]
    ends = np.nonzero(rec[:, 0] == -1)[0]
    return M, (int(ends[0]) if len(ends) else row.records)


@pytest.mark.parametrize('row', ROWS, ids=repr)
def test_cpu_row(row):
    """Margins, the promised M and K, the suppressed share and (attribute rows) the share of boxes that leave [0, 1]."""
    c = case(row.id)
    assert c.K is not None, 'no K recorded for ' + row.id
    for img in range(len(c.M)):
        m = margins(row, c.inputs, img)
        what = '{} image {}: {}'.format(row.id, img, m)
        for key in ('thr', 'pair', 'rank'):
            assert m[key] >= helpers.REL_TOL, what
        assert m['iou'] >= helpers.REL_TOL, what
        assert m['score_ties'] == 0 or 'score' in row.ties, what
        assert m['iou_ties'] == 0 or 'iou' in row.ties, what
        assert m['nan_ious'] == 0 or 'nan' in row.ties, what
        assert m['thr_ties'] == 0 or row.id == 'threshold', what
        assert (m['M'], m['K']) == (c.M[img], c.K[img]), what
        oM, oK = oracle_counts(row, c, img)
        assert oM == c.M[img] and oK == min(c.K[img], row.records), '{}: the oracle has M = {}, K = {}'.format(what, oM, oK)
        if c.M[img]:
            assert 1.0 - m['K'] / m['M'] >= row.min_dropped, what
        if row.seeded:
            assert m['outside'] >= 0.2, what
    for tie in row.ties:           # a declared tie is really there
        total = sum(margins(row, c.inputs, img)[{'score': 'score_ties', 'iou': 'iou_ties', 'nan': 'nan_ious'}[tie]] for img in range(len(c.M)))
        assert total > 0, '{}: declares {} ties and has none'.format(row.id, tie)


def test_cpu_table_holds_every_regime():
    """The sizes the issue names are in the table, and the candidate / survivor counts it asks for are what the rows promise."""
    assert {r.P for r in ROWS} >= {1, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 3100, 4724, 4725, 7677, 7678, 8732, 11498}
    assert case('candidates-1100').M == [0, 1, 255, 256, 257, 512, 513, 1100]
    assert case('candidates-300').M == [0, 1, 255, 256, 257, 300]
    assert case('records-keep_top_k').K == [KR + 1, 4 * KR, KR - 1, KR, 2] and BY_ID['records-keep_top_k'].records == KR
    assert case('records-top_k').K == [5, 6, 7, 100] and BY_ID['records-top_k'].records == 6
    assert case('records-all').K == [0, 100, 300] and BY_ID['records-all'].records == 900
    assert case('classes-1').M == [0] and case('threshold').M == [180]
    for r in ROWS:
        if r.id.startswith(('priors-', 'lds-')):
            assert case(r.id).M[0] == r.P
    # chains: one survivor per cell, the top of the chain (greedy NMS would keep two)
    c = case('suppress-structure')
    assert c.M[:2] == [1100, 1100] and c.K[:2] == [367, 367]
    # LDS bytes of the launcher: 13 P + 4116 (candidates), 8 P + 4116 (records), refusal above 150 KB
    assert 13 * 4724 + 4116 <= 65536 < 13 * 4725 + 4116 and 8 * 7677 + 4116 <= 65536 < 8 * 7678 + 4116
    assert 13 * 11498 + 4116 <= 153600 < 13 * 11499 + 4116


@pytest.mark.parametrize('code', (CORNER, CENTER), ids=('CORNER', 'CENTER_SIZE'))
def test_cpu_clip_settings_are_told_apart(code):
    """Per code type (and variance setting) the four clip settings give at least three distinct oracle outputs."""
    for enc in (True, False):
        outs = [case(r.id).want.tobytes() for r in ROWS if r.seeded and r.code == code and r.enc == enc]
        assert len(outs) == 4 and len(set(outs)) >= 3, '{} enc={}: {} distinct outputs'.format(code, enc, len(set(outs)))


# ------------------------------------------------------------------------------------------------------------------- GPU part
def check_records(row, c, got, what):
    want = c.want
    assert got.shape == want.shape == (1, 1, len(c.M) * row.records, 7) and got.dtype == np.float32, what
    got, want = got[0, 0], want[0, 0]
    for img in range(len(c.M)):
        rec = got[img * row.records:(img + 1) * row.records]
        K = min(c.K[img], row.records)
        assert np.array_equal(rec[:K, 0], np.arange(K, dtype=np.float32)), '{} image {}: ranks'.format(what, img)
        if K < row.records:
            assert rec[K, 0] == -1 and not rec[K, 1:].any() and not rec[K + 1:].any(), '{} image {}: terminator / zero rows'.format(what, img)
    assert_bit_exact(got[:, :3], want[:, :3], what + ': rank / class / score columns')
    diff = int((~((got[:, 3:].view(np.uint32) == want[:, 3:].view(np.uint32)) | (np.isnan(got[:, 3:]) & np.isnan(want[:, 3:])))).sum())
    print('  {}: M {} K {} records {}; {} of {} box elements not bit-identical'.format(row.id, c.M, c.K, row.records, diff, got[:, 3:].size))
    if row.code == CORNER:
        assert diff == 0, '{}: {} box elements differ bitwise'.format(what, diff)
    else:
        assert_close(got[:, 3:], want[:, 3:], 1e-6, what + ': boxes')


def run_plugin(c):
    return first_out(hip_plugin().compute(c.node, c.inputs))


@gpu
@pytest.mark.parametrize('row', ROWS, ids=repr)
def test_gpu_row(hip, row):
    c = case(row.id)
    check_records(row, c, run_plugin(c), row.id)


@gpu
def test_gpu_too_many_priors_are_refused(hip):
    """13 P + 4116 bytes of LDS pass 150 KB at P = 11499: the plugin raises with the launcher's message and returns nothing."""
    P = 11499
    inputs = {0: np.zeros((1, P * 4), np.float32), 1: np.zeros((1, P * 3), np.float32), 2: np.zeros((1, 2, P * 4), np.float32)}
    result = None
    with pytest.raises(hip.PvhipError, match=r'11499 priors need 153603 bytes of LDS \(limit 150 KB\)'):
        result = hip_plugin().compute(node_of(BY_ID['lds-11498'], inputs), inputs)
    assert result is None
    hip.synchronize()


@gpu
def test_gpu_small_launch_after_large_lds(hip):
    """The attribute set on the kernels by a large launch does not disturb a later small one (same process, in this order)."""
    for row_id in ('lds-11498', 'lds-7678', 'candidates-300', 'priors-257'):
        c = case(row_id)
        check_records(BY_ID[row_id], c, run_plugin(c), row_id + ' in sequence')


@gpu
def test_gpu_large_lds_replays_from_a_graph(hip):
    """P = 8732 (both kernels above 64 KB of LDS) captured with its hipFuncSetAttribute calls and workspace, replayed: the eager bits."""
    row = BY_ID['lds-8732']
    c = case(row.id)
    V = ctypes.c_void_p
    loc, conf, priors = (hip.DeviceTensor.from_numpy(np.ascontiguousarray(c.inputs[i])) for i in range(3))
    out = hip.DeviceTensor.empty(c.want.shape)
    args = (V(loc.ptr), V(conf.ptr), V(priors.ptr), V(out.ptr), len(c.M), row.P, row.C, row.records, THR, row.nms, 0, 1, 0, 0)
    hip.call('pvhip_detection_output_f32', *args)
    hip.synchronize()
    eager = out.numpy().copy()
    check_records(row, c, eager, row.id + ' eager')
    hip.call('pvhip_graph_begin_capture')
    hip.call('pvhip_detection_output_f32', *args)
    handle = ctypes.c_void_p(0)
    hip.call('pvhip_graph_end_capture', ctypes.byref(handle))
    try:
        for turn in range(2):
            junk = np.full(c.want.shape, 7.0, dtype=np.float32)
            hip.call('pvhip_memcpy_h2d', V(out.ptr), junk.ctypes.data_as(V), junk.nbytes)
            hip.call('pvhip_graph_launch', handle)
            assert_bit_exact(out.numpy(), eager, 'replay {}'.format(turn))
    finally:
        hip.call('pvhip_graph_destroy', handle)
