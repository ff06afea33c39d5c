"""References and cases for csrc/nms.hip in numpy + the CPU oracle (oracle.nms, oracle_soft_nms: this project's C, pinned to the
compiled reference by tests/test_oracle_nms.py, ties fixed to "lower index first"), nothing from the GPU.

concatenation() and cut() restate multiclass_nms_kp: per class the candidates with score > score_thr in ascending row order, NMS (or soft-NMS)
on them with the oracle, the results concatenated in class order, and -- if more than max_num remain -- the max_num best by
(decayed) score under a STABLE sort: among ties the earlier in the concatenation comes first.

The inputs sit where the kernels decide: boxes on a grid of 8 (IoU == 0.5 exactly is common), tied and quantized scores, scores equal
to score_thr, negative and subnormal scores, boxes of zero and negative width, thresholds 0 and 1.5, and the sizes at the kernels'
on-chip limits.  tests/test_nms_edge_cases.py holds each case to the edge it claims.
"""
import ctypes
import functools

import numpy as np

import oracle

f32 = np.float32
HARD_LIMIT = 4096        # boxes of a segment that stay on chip (kNmsMaxLen)
SOFT_LIMIT = 4544        # boxes of a soft-NMS problem: 36 bytes each in 160 KiB - 256
KEY_LIMIT = 16384        # keys of the multiclass select: 128 KiB


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def soft_nms(dets, iou_thr, method, sigma, min_score):
    """(new_dets [M, 5] float32, inds [M] int64) of the oracle's soft-NMS; method 0 hard, 1 linear, 2 gaussian"""
    boxes = np.array(dets, f32, copy=True, order='C').reshape(-1, 5)
    n = boxes.shape[0]
    inds = np.empty(n, np.int64)
    m = oracle.lib().oracle_soft_nms(_vp(boxes), ctypes.c_int64(n), ctypes.c_float(iou_thr), ctypes.c_int(method), ctypes.c_float(sigma),
                                     ctypes.c_float(min_score), _vp(inds))
    return boxes[:m].copy(), inds[:m].copy()


def iou(a, b):
    """the float32 expression of the hard kernel and nms_cpu.cpp for boxes a against b"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    one, zero = f32(1), f32(0)
    area = lambda d: (d[..., 2] - d[..., 0] + one) * (d[..., 3] - d[..., 1] + one)
    w = np.maximum(zero, np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]) + one)
    h = np.maximum(zero, np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]) + one)
    inter = w * h
    with np.errstate(all='ignore'):
        return inter / (area(a) + area(b) - inter)


# ---------------------------------------------------------------------------------------------- boxes and scores
def grid_boxes(rng, n):
    """n boxes [n, 4] with corners on a grid of 8 (x2 = x1 + 8 w - 1), clustered: about sqrt(n) / 2 origins per axis, three sizes"""
    span = max(3, int(np.sqrt(n) / 2))
    b = np.empty((n, 4), f32)
    for ax in (0, 1):
        o = 8 * rng.integers(0, span, n)
        b[:, ax], b[:, ax + 2] = o, o + 8 * rng.integers(1, 4, n) - 1
    return b


def apart_boxes(n):
    """n boxes that do not touch"""
    b = np.zeros((n, 4), f32)
    b[:, 0] = 20 * np.arange(n)
    b[:, 2], b[:, 3] = b[:, 0] + 7, 7
    return b


CONTENTS = ('distinct', 'tied', 'signed', 'degenerate')
SEGMENT_LENGTHS = (63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2049)
HARD_THRS = (0.0, 0.5, 1.5)
SUBNORMAL = f32(1e-40)


def segment(n, content, seed=0):
    """dets [n, 5] of one hard-NMS segment"""
    rng = np.random.default_rng([n, CONTENTS.index(content), seed])
    d = np.empty((n, 5), f32)
    d[:, :4] = grid_boxes(rng, n)
    distinct = ((rng.permutation(n) + 1) / f32(n + 1)).astype(f32)
    if content == 'tied':
        d[:, 4] = 0.5
    elif content == 'signed':                  # negatives, and a subnormal of either sign (no zero: -0 and +0 tie on the CPU only)
        d[:, 4] = distinct * 2 - 1
        d[d[:, 4] == 0, 4] = 0.001234
        d[n // 3, 4], d[(2 * n) // 3, 4] = SUBNORMAL, -SUBNORMAL
    else:
        d[:, 4] = distinct
    if content == 'degenerate':                # zero width (x2 = x1 - 1), negative width, the same on y, both
        d[0::5, 2] = d[0::5, 0] - 1
        d[1::7, 2] = d[1::7, 0] - 9
        d[2::9, 3] = d[2::9, 1] - 1
        d[3::11, 3] = d[3::11, 1] - 17
    return d


def hard_reference(dets, offsets, thr):
    """[(keep indices inside the segment, ascending)] per segment"""
    return [oracle.nms(dets[a:b], thr) for a, b in zip(offsets[:-1], offsets[1:])]


@functools.lru_cache(maxsize=None)
def hard_batch(content, lengths=SEGMENT_LENGTHS):
    """(dets [T, 5], offsets [S + 1] int64) of segments of `lengths`, one launch"""
    segs = [segment(n, content) for n in lengths]
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    dets = np.concatenate(segs)
    dets.setflags(write=False)
    return dets, offsets


# ---------------------------------------------------------------------------------------------- multiclass
def concatenation(boxes, scores, C, col0, score_thr, iou_thr, soft=None):
    """(det [T, 5], label [T], src [T]) of ONE image in front of the max_num cut; soft: None or (method, sigma, min_score)"""
    dets, labels, srcs = [np.zeros((0, 5), f32)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for c in range(C):
        s = scores[:, col0 + c]
        cand = np.nonzero(s > f32(score_thr))[0]
        if cand.size == 0:
            continue
        d = np.concatenate([boxes[cand], s[cand, None]], axis=1).astype(f32)
        if soft is None:
            keep = oracle.nms(d, iou_thr)
            out = d[keep]
        else:
            out, keep = soft_nms(d, iou_thr, *soft)
        dets.append(out)
        srcs.append(cand[keep])
        labels.append(np.full(len(keep), c, np.int64))
    return np.concatenate(dets), np.concatenate(labels), np.concatenate(srcs)


def cut(det, label, src, max_num):
    """the outputs of the kernels for one image: det [max_num, 5], label, src [max_num] zero past the count, and the count"""
    if len(det) > max_num:
        order = np.argsort(-det[:, 4], kind='stable')[:max_num]
        det, label, src = det[order], label[order], src[order]
    n = len(det)
    od, ol, os_ = np.zeros((max_num, 5), f32), np.zeros(max_num, np.int64), np.zeros(max_num, np.int64)
    od[:n], ol[:n], os_[:n] = det, label, src
    return od, ol, os_, n


def cut_in_tie(det, max_num):
    """the max_num-th and the (max_num + 1)-th best score are equal"""
    s = np.sort(det[:, 4])[::-1]
    return bool(max_num < len(s) and s[max_num - 1] == s[max_num])


def tie_cuts(det, label):
    """the max_num values at which the cut falls inside a run of equal scores whose two sides of the cut are of different classes"""
    order = np.argsort(-det[:, 4], kind='stable')
    s, l = det[order, 4], label[order]
    r = np.arange(1, len(s))
    return r[(s[r - 1] == s[r]) & (l[r - 1] != l[r])]


# name: B, N, C, S (score_stride), col0, score_thr, iou_thr, max_num (a number; 'T' / 'T-1': image 0's survivor count / one below;
# 'tie': the middle one of tie_cuts(image 0)), levels (scores quantized to k / levels; None: distinct), boxes, and
# special: 'fill' -- the columns outside [col0, col0 + C) hold 0.99; 'edges' -- class 1 of image 0 has no candidate, class 2 all N
MC_CASES = {
    'stride_col':   dict(B=2, N=200, C=5, S=9, col0=3, score_thr=0.05, iou_thr=0.5, max_num=40, levels=None, special='fill'),
    'thr_equal':    dict(B=2, N=300, C=3, S=3, col0=0, score_thr=0.25, iou_thr=0.5, max_num=400, levels=8),     # (no cut: the weakest show)
    'class_edges':  dict(B=2, N=130, C=64, S=66, col0=1, score_thr=0.25, iou_thr=0.5, max_num=100, levels=16, special='edges'),
    'max_num_1':    dict(B=2, N=150, C=4, S=4, col0=0, score_thr=0.05, iou_thr=0.5, max_num=1, levels=None),
    'max_num_gt_N': dict(B=2, N=70, C=3, S=3, col0=0, score_thr=0.05, iou_thr=0.5, max_num=100, levels=None),
    'cut_at_T':     dict(B=2, N=150, C=4, S=4, col0=0, score_thr=0.05, iou_thr=0.5, max_num='T', levels=None),
    'cut_below_T':  dict(B=2, N=150, C=4, S=4, col0=0, score_thr=0.05, iou_thr=0.5, max_num='T-1', levels=None),
    'tie_at_cut':   dict(B=2, N=400, C=6, S=6, col0=0, score_thr=0.125, iou_thr=0.5, max_num='tie', levels=8),
    'all_tied':     dict(B=1, N=300, C=4, S=4, col0=0, score_thr=0.125, iou_thr=0.5, max_num=20, levels=1),
    'thr_zero':     dict(B=1, N=200, C=3, S=3, col0=0, score_thr=0.05, iou_thr=0.0, max_num=10, levels=None),
    'thr_above_1':  dict(B=1, N=200, C=3, S=3, col0=0, score_thr=0.05, iou_thr=1.5, max_num=50, levels=8),
    'rank_runs':    dict(B=1, N=1100, C=3, S=4, col0=1, score_thr=0.125, iou_thr=0.5, max_num=100, levels=8),
    'segment_4096': dict(B=1, N=4096, C=2, S=2, col0=0, score_thr=0.05, iou_thr=0.5, max_num=100, levels=None),
    'keys_16384':   dict(B=1, N=256, C=64, S=64, col0=0, score_thr=0.0, iou_thr=0.5, max_num=256, levels=64, boxes='apart'),
}
# the soft-NMS form: soft = (method, sigma, min_score)
MC_SOFT_CASES = {
    'below_T':      dict(B=2, N=300, C=4, S=6, col0=2, score_thr=0.05, iou_thr=0.3, max_num='T-1', levels=None, soft=(1, 0.5, 0.05), special='fill'),
    'above_T':      dict(B=2, N=300, C=4, S=4, col0=0, score_thr=0.05, iou_thr=0.3, max_num=400, levels=None, soft=(2, 0.5, 0.3)),
    'tie_at_cut':   dict(B=2, N=400, C=6, S=6, col0=0, score_thr=0.125, iou_thr=0.3, max_num='tie', levels=8, soft=(0, 0.5, 0.0)),
    'class_edges':  dict(B=1, N=600, C=64, S=64, col0=0, score_thr=0.25, iou_thr=0.3, max_num=256, levels=16, soft=(1, 0.5, 0.1), special='edges'),
    'thr_equal':    dict(B=2, N=300, C=3, S=3, col0=0, score_thr=0.25, iou_thr=0.3, max_num=400, levels=8, soft=(1, 0.5, 0.05)),
    'limit_4544':   dict(B=1, N=4544, C=1, S=1, col0=0, score_thr=0.0, iou_thr=0.3, max_num=100, levels=None, soft=(1, 0.5, 0.3)),
}


@functools.lru_cache(maxsize=None)
def multiclass_case(name, soft=False):
    """dict(boxes [B, N, 4], scores [B, N, S], the ABI's arguments, max_num resolved, T [B] (survivors in front of the cut) and
    want = [(det, label, src, count)] per image); computed once, shared, read-only"""
    spec = dict((MC_SOFT_CASES if soft else MC_CASES)[name])
    B, N, C, S, col0 = (spec[k] for k in ('B', 'N', 'C', 'S', 'col0'))
    rng = np.random.default_rng([sorted(MC_CASES).index(name) if not soft else 100 + sorted(MC_SOFT_CASES).index(name), 22])
    if spec.get('boxes') == 'apart':
        boxes = np.stack([apart_boxes(N)] * B)
    else:
        boxes = np.stack([grid_boxes(rng, N) for _ in range(B)])
    if spec['levels']:
        scores = (rng.integers(1, spec['levels'] + 1, (B, N, S)) / f32(spec['levels'])).astype(f32)
    else:
        scores = (0.01 + 0.98 * rng.random((B, N, S))).astype(f32)
    special = spec.get('special')
    if special == 'edges':
        scores[0, :, col0 + 1] = np.minimum(scores[0, :, col0 + 1], f32(spec['score_thr']))
        scores[0, :, col0 + 2] = np.maximum(scores[0, :, col0 + 2], f32(spec['score_thr']) * 2)
    if special in ('fill', 'edges'):
        scores[:, :, :col0] = 0.99
        scores[:, :, col0 + C:] = 0.99
    cat = [concatenation(boxes[b], scores[b], C, col0, spec['score_thr'], spec['iou_thr'], spec.get('soft')) for b in range(B)]
    max_num = spec['max_num']
    if max_num == 'T':
        max_num = len(cat[0][0])
    elif max_num == 'T-1':
        max_num = len(cat[0][0]) - 1
    elif max_num == 'tie':
        ties = tie_cuts(cat[0][0], cat[0][1])
        max_num = int(ties[len(ties) // 2])
    boxes.setflags(write=False)
    scores.setflags(write=False)
    spec.update(boxes=boxes, scores=scores, max_num=int(max_num), T=[len(c[0]) for c in cat], cat=cat,
                want=[cut(*c, int(max_num)) for c in cat])
    return spec


# ---------------------------------------------------------------------------------------------- soft-NMS, single problem
SOFT_METHODS = (0, 1, 2)
SOFT_LENGTHS = (1, 2, 511, 512, 513, 1025)
SOFT_IOU, SOFT_SIGMA = 0.3, 0.5
# min_score: 'many' boxes removed (holes and movers across the threads' runs), 'none' (no score is negative), and 'equal': method 0
# decays to exactly 0 = min_score, which stays because the test is a strict <
SOFT_MIN_SCORE = {'many': 0.3, 'none': -1.0, 'equal': 0.0}
SOFT_CASES = [(m, n, r) for m in SOFT_METHODS for n in SOFT_LENGTHS for r in ('many', 'none', 'equal') if r != 'equal' or m == 0]


def soft_dets(n, tied=False):
    rng = np.random.default_rng([n, 23])
    d = np.empty((n, 5), f32)
    d[:, :4] = grid_boxes(rng, n)
    d[:, 4] = 0.5 if tied else (0.05 + 0.9 * rng.random(n)).astype(f32)
    return d
