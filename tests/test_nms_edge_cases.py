"""tests/nms_edge_cases.py held to its own claims on the CPU, before a GPU is involved: the references on hand-worked cases, and every
edge case really containing its edge -- so a mismatch in tests/test_gpu_nms_edges.py is a finding about a kernel."""
import numpy as np
import pytest

import oracle
from tests import nms_edge_cases as E

f32 = np.float32
PAIR = np.array([[0, 0, 9, 9], [0, 0, 9, 4]], f32)          # 100 and 50 pixels, 50 shared: IoU 0.5 exactly


# ---------------------------------------------------------------------------------------------- hand-worked
def test_half_iou_pair_is_suppressed_at_half():
    assert E.iou(PAIR[0], PAIR[1]) == f32(0.5)
    d = np.concatenate([PAIR, [[0.9], [0.8]]], axis=1).astype(f32)
    assert oracle.nms(d, 0.5).tolist() == [0]
    assert oracle.nms(d, float(np.nextafter(f32(0.5), f32(1)))).tolist() == [0, 1]
    assert oracle.nms(d[::-1].copy(), 0.5).tolist() == [1]                      # the better one is kept wherever it stands
    # multiclass: both classes see the pair; class 1 has them in the other order
    boxes, scores = PAIR, np.array([[0.9, 0.3], [0.8, 0.6]], f32)
    det, label, src = E.concatenation(boxes, scores, 2, 0, 0.05, 0.5)
    assert label.tolist() == [0, 1] and src.tolist() == [0, 1] and det[:, 4].tolist() == [f32(0.9), f32(0.6)]
    assert (det[:, :4] == PAIR).all()


def test_threshold_extremes():
    rng = np.random.default_rng(0)
    d = np.concatenate([E.grid_boxes(rng, 50), rng.random((50, 1))], axis=1).astype(f32)
    first = int(np.argmax(d[:, 4]))
    assert oracle.nms(d, 0.0).tolist() == [first]                                # IoU >= 0 holds for every pair: the first visited box alone
    assert oracle.nms(d, 1.5).tolist() == list(range(50))                       # no IoU reaches 1.5
    far = np.array([[0, 0, 7, 7, 0.5], [100, 100, 107, 107, 0.9]], f32)
    assert oracle.nms(far, 0.0).tolist() == [1]                                  # even boxes that do not touch
    # all tied: the lowest index is visited first
    d[:, 4] = 0.5
    assert oracle.nms(d, 0.0).tolist() == [0]


def test_tie_across_two_classes_at_the_cut():
    boxes = E.apart_boxes(3)
    scores = np.array([[0.5, 0.5], [0.9, 0.5], [0.5, 0.2]], f32)
    det, label, src = E.concatenation(boxes, scores, 2, 0, 0.05, 0.5)
    assert label.tolist() == [0, 0, 0, 1, 1, 1] and src.tolist() == [0, 1, 2, 0, 1, 2]
    # 0.9 first, then the four 0.5 in the order of the concatenation: class 0 rows 0, 2, then class 1 rows 0, 1
    for max_num, want in ((2, [(0, 1), (0, 0)]), (3, [(0, 1), (0, 0), (0, 2)]), (4, [(0, 1), (0, 0), (0, 2), (1, 0)])):
        od, ol, os_, n = E.cut(det, label, src, max_num)
        assert n == max_num and list(zip(ol.tolist(), os_.tolist())) == want
    assert E.tie_cuts(det, label).tolist() == [3]
    od, ol, os_, n = E.cut(det, label, src, 8)                                   # no cut: the concatenation as it is, zeros behind
    assert n == 6 and ol[:6].tolist() == label.tolist() and not od[6:].any() and not ol[6:].any() and not os_[6:].any()


def test_soft_nms_methods_by_hand():
    d = np.concatenate([PAIR, [[0.9], [0.8]]], axis=1).astype(f32)
    # method 0 at IoU 0.5 > 0.3: weight 0, the score becomes 0; removed under min_score > 0, kept at min_score = 0 (strict <)
    nd, ni = E.soft_nms(d, 0.3, 0, 0.5, 0.001)
    assert ni.tolist() == [0] and nd[0, 4] == f32(0.9)
    nd, ni = E.soft_nms(d, 0.3, 0, 0.5, 0.0)
    assert ni.tolist() == [0, 1] and nd[1, 4] == 0
    nd, ni = E.soft_nms(d, 0.5, 0, 0.5, 0.001)                                   # ov > thr is strict: 0.5 does not decay at 0.5
    assert ni.tolist() == [0, 1] and nd[1, 4] == f32(0.8)
    nd, ni = E.soft_nms(d, 0.3, 1, 0.5, 0.001)                                   # linear: 0.8 * (1 - 0.5)
    assert ni.tolist() == [0, 1] and nd[1, 4] == f32(0.4)
    nd, ni = E.soft_nms(d, 0.3, 2, 0.5, 0.001)                                   # gaussian: 0.8 * exp(-0.25 / 0.5)
    assert nd[1, 4] == f32(0.8) * f32(np.exp(-0.5))
    for name, code in (('linear', 1), ('gaussian', 2)):                          # the same function the pinned wrapper reaches
        a, b = oracle.soft_nms(E.soft_dets(513), 0.3, name, 0.5, 0.3), E.soft_nms(E.soft_dets(513), 0.3, code, 0.5, 0.3)
        assert (a[0].view(np.int32) == b[0].view(np.int32)).all() and (a[1] == b[1]).all()
    t = E.soft_dets(5, tied=True)                                                # all tied: the first maximum wins
    assert E.soft_nms(t, 0.3, 1, 0.5, -1.0)[1][0] == 0


# ---------------------------------------------------------------------------------------------- the cases contain their edges
@pytest.mark.parametrize('content', E.CONTENTS)
def test_hard_segments_contain_their_edges(content):
    dets, offsets = E.hard_batch(content)
    assert (np.diff(offsets) == E.SEGMENT_LENGTHS).all()
    assert (dets[:, :4] % 8 == np.where(np.arange(4) < 2, 0, 7)).all() or content == 'degenerate'
    s = dets[:, 4]
    assert not (s == 0).any()                                                    # (-0 and +0: equal on the CPU, ordered by the kernel's keys)
    moved = 0
    for a, b in zip(offsets[:-1], offsets[1:]):
        seg = dets[a:b]
        if content == 'tied':
            assert (seg[:, 4] == 0.5).all()
        else:
            assert len(np.unique(seg[:, 4])) == b - a
        if content == 'signed':
            assert (seg[:, 4] < 0).sum() > 10 and (seg[:, 4] == E.SUBNORMAL).sum() == 1 and (seg[:, 4] == -E.SUBNORMAL).sum() == 1
        if content == 'degenerate':
            w, h = seg[:, 2] - seg[:, 0] + 1, seg[:, 3] - seg[:, 1] + 1
            assert (w == 0).any() and (w < 0).any() and (h == 0).any() and (h < 0).any()
        if b - a <= 513:                                                         # IoU == 0.5 exactly is there and decides
            m = E.iou(seg[:, None, :4], seg[None, :, :4])
            assert ((m == f32(0.5)) & ~np.eye(b - a, dtype=bool)).any()
        k0, k1 = oracle.nms(seg, 0.5), oracle.nms(seg, float(np.nextafter(f32(0.5), f32(1))))
        moved += len(k0) != len(k1) or (k0 != k1).any()
        assert 1 < len(k0) < b - a                                               # some kept, some suppressed
        assert len(oracle.nms(seg, 1.5)) == b - a
        assert len(oracle.nms(seg, 0.0)) == 1 or content == 'degenerate'       # (NaN and negative IoU of the degenerate boxes: not >= 0)
    assert moved >= len(E.SEGMENT_LENGTHS) - 2                                   # >= against >: a different result nearly everywhere


def test_limit_segments():
    for n in (E.HARD_LIMIT, E.HARD_LIMIT + 1):
        d = E.segment(n, 'distinct')
        k = oracle.nms(d, 0.5)
        assert d.shape == (n, 5) and 100 < len(k) < n


@pytest.mark.parametrize('name', sorted(E.MC_CASES))
def test_multiclass_cases_contain_their_edges(name):
    c = E.multiclass_case(name)
    B, N, C, S, col0, thr, max_num = (c[k] for k in ('B', 'N', 'C', 'S', 'col0', 'score_thr', 'max_num'))
    used = c['scores'][:, :, col0:col0 + C]
    assert c['boxes'].shape == (B, N, 4) and c['scores'].shape == (B, N, S) and 0 < max_num
    assert not (used == 0).any()
    for b in range(B):
        od, ol, os_, n = c['want'][b]
        assert n == min(c['T'][b], max_num) and not od[n:].any() and not ol[n:].any() and not os_[n:].any()
        assert (used[b][os_[:n], ol[:n]] == od[:n, 4]).all() and (od[:n, 4] > f32(thr)).all()
        assert (c['boxes'][b][os_[:n]] == od[:n, :4]).all()
    T0 = c['T'][0]
    if name == 'stride_col':
        assert S > C and col0 > 0 and col0 + C < S
        assert (c['scores'][:, :, :col0] > used.max()).all() and (c['scores'][:, :, col0 + C:] > used.max()).all()
    if name in ('thr_equal', 'class_edges'):
        assert (used == f32(thr)).any()
    if name == 'thr_equal':          # nothing is cut: a row let in at score == score_thr, the weakest of its class, would show
        assert max(c['T']) <= max_num and (used == f32(thr)).sum() > 50
    if name == 'class_edges':
        assert C == 64 and not (used[0, :, 1] > f32(thr)).any() and (used[0, :, 2] > f32(thr)).all()
        assert 1 not in c['cat'][0][1] and 2 in c['cat'][0][1]
    if name == 'max_num_1':
        assert max_num == 1 and T0 > 1
    if name == 'max_num_gt_N':
        assert max_num > N and T0 < max_num
    if name == 'cut_at_T':
        assert max_num == T0 and c['T'][1] != T0
    if name == 'cut_below_T':
        assert max_num == T0 - 1
    if name == 'tie_at_cut':                                                     # the cut inside a tie that spans classes
        assert max_num in E.tie_cuts(c['cat'][0][0], c['cat'][0][1])
    if name in ('tie_at_cut', 'keys_16384', 'rank_runs', 'all_tied'):           # the cut inside a run of equal scores
        assert E.cut_in_tie(c['cat'][0][0], max_num)
    if name == 'thr_zero':
        assert T0 == C                                                           # one box per class
    if name == 'thr_above_1':
        assert T0 == int((used[0] > f32(thr)).sum()) > max_num                   # every candidate survives
    if name == 'rank_runs':
        assert min(int((used[0, :, k] > f32(thr)).sum()) for k in range(C)) > 512    # runs of the rank scan longer than one
        assert max(int((c['cat'][0][1] == k).sum()) for k in range(C)) > max_num          # a class with more survivors than max_num
    if name == 'segment_4096':
        assert N == E.HARD_LIMIT
    if name == 'keys_16384':
        assert T0 == C * N == E.KEY_LIMIT and C * min(N, max_num) == E.KEY_LIMIT


@pytest.mark.parametrize('name', sorted(E.MC_SOFT_CASES))
def test_multiclass_soft_cases_contain_their_edges(name):
    c = E.multiclass_case(name, soft=True)
    B, N, C, col0, thr, max_num = (c[k] for k in ('B', 'N', 'C', 'col0', 'score_thr', 'max_num'))
    for b in range(B):
        od, ol, os_, n = c['want'][b]
        assert n == min(c['T'][b], max_num) and not od[n:].any() and not ol[n:].any() and not os_[n:].any()
        assert (c['boxes'][b][os_[:n]] == od[:n, :4]).all()
        assert (np.diff(od[:n, 4]) <= 0).all() or c['T'][b] <= max_num
        det, label, src = c['cat'][b]
        for k in range(C):                                                        # what the select relies on: a class leaves in score order
            assert (np.diff(det[label == k, 4]) <= 0).all()
    T0 = c['T'][0]
    if name == 'below_T':
        assert max_num == T0 - 1 and (c['cat'][0][0][:, 4] < c['scores'][0][c['cat'][0][2], col0 + c['cat'][0][1]]).any()    # decayed
    if name == 'above_T':
        assert max(c['T']) < max_num and T0 < int((c['scores'][0][:, col0:col0 + C] > f32(thr)).sum())    # min_score removed some
    if name == 'tie_at_cut':
        assert max_num in E.tie_cuts(c['cat'][0][0], c['cat'][0][1])
        assert (c['cat'][0][0][:, 4] == 0).any()                                  # decayed to min_score exactly, and kept
    if name == 'class_edges':
        assert C == 64 and 1 not in c['cat'][0][1] and 2 in c['cat'][0][1] and C * max_num == E.KEY_LIMIT
    if name == 'thr_equal':
        assert max(c['T']) <= max_num and (c['scores'][:, :, col0:col0 + C] == f32(thr)).sum() > 50
    if name == 'limit_4544':
        assert N == E.SOFT_LIMIT == int((c['scores'][0] > f32(thr)).sum()) and T0 > max_num


@pytest.mark.parametrize('method,n,regime', E.SOFT_CASES)
def test_soft_cases_contain_their_edges(method, n, regime):
    d = E.soft_dets(n)
    assert (d[:, 4] > 0).all()
    nd, ni = E.soft_nms(d, E.SOFT_IOU, method, E.SOFT_SIGMA, E.SOFT_MIN_SCORE[regime])
    assert sorted(set(ni.tolist())) == sorted(ni.tolist())
    if regime == 'many' and n >= 511:
        assert len(ni) < n // 2                                                  # more than half removed ...
        assert (ni[1:] < ni[:-1]).any() and (ni[1:] > ni[:-1]).any()
    if regime == 'none':
        assert len(ni) == n
    if regime == 'equal':
        assert len(ni) == n and (n < 511 or (nd[:, 4] == 0).any())              # ... decayed to min_score exactly, and kept


def test_soft_limit():
    assert E.SOFT_LIMIT * 36 <= 160 * 1024 - 256 < (E.SOFT_LIMIT + 1) * 36
