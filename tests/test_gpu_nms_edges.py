"""csrc/nms.hip through the C ABI against the CPU oracle on the cases of tests/nms_edge_cases.py: hard NMS on chip and on the
large-segment kernel, the multiclass segments with their select, soft-NMS alone and as multiclass segments with their select.
The bar is bit equality of kept indices, detections, labels, source rows and counts; rows past a count are zero where the kernel
promises zeros and untouched where it promises nothing.  Every output and workspace sits in a guarded buffer.

Which kernel serves what (csrc/nms.hip): kgdet_nms_batched / kgdet_nms -- nms_segments while the longest segment has at most 4096
boxes, nms_segments_large for the WHOLE launch beyond; kgdet_multiclass_nms -- multiclass_nms_segments + multiclass_select (at most
16384 keys); kgdet_soft_nms -- soft_nms_kernel (at most 4544 boxes); kgdet_multiclass_soft_nms -- multiclass_soft_nms_segments +
multiclass_soft_select.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import nms_edge_cases as E
from tests.test_gpu_pointwise_kernels import E_SHAPE, E_UNSUPPORTED, Guarded, _L, _ptr, _st, c_f, c_i32, c_i64, c_sz

pytestmark = pytest.mark.gpu

f32 = np.float32
UNTOUCHED = -7


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _ints(n, dtype=torch.int64):
    """n integers of UNTOUCHED inside a guarded buffer"""
    g = Guarded(n * (2 if dtype == torch.int64 else 1))
    g.view().view(dtype).fill_(UNTOUCHED)
    return g


def _floats(n):
    g = Guarded(n)
    g.view().fill_(float('nan'))
    return g


def _get(g, dtype=torch.int64):
    return g.view().view(dtype).cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


# ============================================================================================ hard NMS
def _hard_launch(dets, offsets, thr):
    lib, L = _L()
    T, S = len(dets), len(offsets) - 1
    max_len = int(np.diff(offsets).max())
    keep, num = _ints(T), _ints(S)
    ws, ws_bytes = None, 0
    if max_len > E.HARD_LIMIT:
        ws_bytes = L.kgdet_nms_workspace_bytes(c_i64(T), c_i32(S))
        ws = Guarded((ws_bytes + 3) // 4)
    d_dets, d_offsets = _dev(dets), _dev(np.asarray(offsets, np.int64))
    lib.check(L.kgdet_nms_batched(_ptr(d_dets), _ptr(d_offsets), c_i32(S), c_i64(T), c_i64(max_len), c_f(thr), keep.ptr(),
                                  num.ptr(), ws.ptr() if ws else ctypes.c_void_p(0), c_sz(ws_bytes), _st()), 'kgdet_nms_batched')
    torch.cuda.synchronize()
    assert keep.intact() and num.intact() and (ws is None or ws.intact())
    return _get(keep), _get(num)


def _hard_check(dets, offsets, thr, tag):
    keep, num = _hard_launch(dets, offsets, thr)
    want = E.hard_reference(dets, offsets, thr)
    for s, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        m = len(want[s])
        assert num[s] == m, '%s segment %d (%d boxes): %d kept, oracle %d' % (tag, s, b - a, num[s], m)
        assert (keep[a:a + m] == want[s]).all(), '%s segment %d (%d boxes): kept indices differ' % (tag, s, b - a)
        assert (keep[a + m:b] == UNTOUCHED).all()
    print('NMS-HARD %s: kept %s' % (tag, [len(w) for w in want]))


@pytest.mark.parametrize('thr', E.HARD_THRS)
@pytest.mark.parametrize('content', E.CONTENTS)
def test_hard_segments_either_side_of_every_block_size(content, thr):
    """13 segments of 63 .. 2049 boxes in ONE launch: either side of a chunk of 64, of the 512 threads, of the power-of-two paddings
    of the bitonic sort; IoU == thr decides; tied scores visit the lower index first"""
    dets, offsets = E.hard_batch(content)
    _hard_check(dets, offsets, thr, '%s thr %g' % (content, thr))


@pytest.mark.parametrize('content,thr', [(c, 0.5) for c in E.CONTENTS] + [('tied', 0.0), ('tied', 1.5)])
def test_hard_segment_at_the_on_chip_limit_and_beyond(content, thr):
    """4096 boxes alone: nms_segments at its largest LDS.  The same 4096 next to 4097: the whole launch on nms_segments_large --
    the same boxes through both kernels, the same kept indices"""
    dets, offsets = E.hard_batch(content, (E.HARD_LIMIT,))
    _hard_check(dets, offsets, thr, '%s 4096 on chip' % content)
    dets, offsets = E.hard_batch(content, (E.HARD_LIMIT, E.HARD_LIMIT + 1))
    _hard_check(dets, offsets, thr, '%s 4096 + 4097 large' % content)


@pytest.mark.parametrize('n', [1, 65, 513, E.HARD_LIMIT, E.HARD_LIMIT + 1])
def test_single_problem_entry(n):
    """kgdet_nms: the segment table {0, n} built in the workspace's first 16 bytes"""
    lib, L = _L()
    dets = E.segment(n, 'distinct')
    want = E.hard_reference(dets, [0, n], 0.5)[0]
    ws_bytes = L.kgdet_nms_workspace_bytes(c_i64(n), c_i32(1)) if n > E.HARD_LIMIT else 16
    keep, num, ws = _ints(n), _ints(1), Guarded((ws_bytes + 3) // 4)
    d_dets = _dev(dets)
    lib.check(L.kgdet_nms(_ptr(d_dets), c_i64(n), c_f(0.5), keep.ptr(), num.ptr(), ws.ptr(), c_sz(ws_bytes), _st()), 'kgdet_nms')
    torch.cuda.synchronize()
    assert keep.intact() and num.intact() and ws.intact()
    k, m = _get(keep), int(_get(num)[0])
    assert m == len(want) and (k[:m] == want).all() and (k[m:] == UNTOUCHED).all()


# ============================================================================================ multiclass, hard and soft
def _multiclass_run(c):
    lib, L = _L()
    B, N, C, S, col0, max_num = (c[k] for k in ('B', 'N', 'C', 'S', 'col0', 'max_num'))
    soft = c.get('soft')
    size = L.kgdet_multiclass_soft_nms_workspace_bytes if soft else L.kgdet_multiclass_nms_workspace_bytes
    size.restype = ctypes.c_size_t
    ws_bytes = size(c_i32(B), c_i32(N), c_i32(C))
    ws = Guarded((ws_bytes + 3) // 4)
    det, label, src, count = _floats(B * max_num * 5), _ints(B * max_num), _ints(B * max_num), _ints(B)
    boxes, scores = _dev(c['boxes']), _dev(c['scores'])
    head = (_ptr(boxes), _ptr(scores), c_i32(B), c_i32(N), c_i32(C), c_i32(S), c_i32(col0), c_f(c['score_thr']), c_f(c['iou_thr']))
    tail = (c_i32(max_num), det.ptr(), label.ptr(), src.ptr(), count.ptr(), ws.ptr(), c_sz(ws_bytes), _st())
    if soft:
        rc = L.kgdet_multiclass_soft_nms(*(head + (c_i32(soft[0]), c_f(soft[1]), c_f(soft[2])) + tail))
    else:
        rc = L.kgdet_multiclass_nms(*(head + tail))
    torch.cuda.synchronize()
    assert det.intact() and label.intact() and src.intact() and count.intact() and ws.intact()
    return rc, (det.view().cpu().numpy().reshape(B, max_num, 5), _get(label).reshape(B, max_num), _get(src).reshape(B, max_num), _get(count))


def _multiclass_check(c, tag):
    lib, L = _L()
    rc, (det, label, src, count) = _multiclass_run(c)
    lib.check(rc, tag)
    for b in range(c['B']):
        od, ol, os_, n = c['want'][b]
        print('NMS-MULTI %s image %d: %d in front of the cut, max_num %d, count %d (oracle %d)' % (tag, b, c['T'][b], c['max_num'], count[b], n))
        assert count[b] == n, (tag, b)
        same = (ol == label[b]) & (os_ == src[b]) & (_bits(od) == _bits(det[b])).all(axis=1)
        assert same.all(), '%s image %d: rows %s differ, first (label, src, det) %s, oracle %s' % (
            tag, b, np.nonzero(~same)[0][:8], (label[b][~same][0], src[b][~same][0], det[b][~same][0]), (ol[~same][0], os_[~same][0], od[~same][0]))


@pytest.mark.parametrize('name', sorted(E.MC_CASES))
def test_multiclass_hard(name):
    """kgdet_multiclass_nms: score_stride > C with score_col0 > 0 next to columns of high scores, scores equal to score_thr, a class
    with no and one with all N candidates, C = 64, every relation of max_num to the survivor count, the cut inside ties, rank runs of
    more than one per thread, a segment of 4096 and a select of exactly 16384 keys"""
    _multiclass_check(E.multiclass_case(name), name)


@pytest.mark.parametrize('name', sorted(E.MC_SOFT_CASES))
def test_multiclass_soft(name):
    """kgdet_multiclass_soft_nms: max_num below and above the survivor count, a tie of decayed scores at the cut across classes
    (method 0, min_score 0: scores decayed to exactly min_score stay), empty and full classes at C = 64 with 16384 keys, 4544 rows"""
    _multiclass_check(E.multiclass_case(name, soft=True), 'soft ' + name)


def test_supported_queries_either_side_of_each_limit():
    lib, L = _L()
    hard, soft = L.kgdet_multiclass_nms_supported, L.kgdet_multiclass_soft_nms_supported
    for args, want in (((1, 4096, 4, 100), 1), ((1, 4097, 4, 100), 0), ((1, 256, 64, 256), 1), ((1, 256, 65, 100), 0),
                       ((1, 257, 64, 257), 0), ((1, 256, 64, 1000), 1), ((1, 1000, 64, 256), 1), ((1, 1000, 64, 257), 0),
                       ((1, 100, 4, 0), 0), ((1, 100, 0, 10), 0), ((1, 0, 4, 10), 1)):
        assert hard(*args) == want, ('hard', args)
    for args, want in (((1, 4544, 4, 100), 1), ((1, 4545, 4, 100), 0), ((1, 600, 64, 256), 1), ((1, 600, 64, 257), 0),
                       ((1, 600, 65, 100), 0), ((1, 100, 4, 0), 0), ((1, 100, 0, 10), 0), ((1, 0, 4, 10), 1)):
        assert soft(*args) == want, ('soft', args)


@pytest.mark.parametrize('soft', [None, (1, 0.5, 0.3)])
def test_multiclass_beyond_the_limits_is_refused_untouched(soft):
    rng = np.random.default_rng(5)
    for N, C, max_num in ((E.SOFT_LIMIT + 1 if soft else E.HARD_LIMIT + 1, 1, 10), (300, 64, 257)):
        c = dict(B=1, N=N, C=C, S=C, col0=0, score_thr=0.05, iou_thr=0.5, max_num=max_num, soft=soft,
                 boxes=E.grid_boxes(rng, N)[None], scores=rng.random((1, N, C)).astype(f32))
        rc, (det, label, src, count) = _multiclass_run(c)
        assert rc == E_UNSUPPORTED
        assert np.isnan(det).all() and (label == UNTOUCHED).all() and (src == UNTOUCHED).all() and (count == UNTOUCHED).all()
    c.update(S=C - 1)                                                            # the score columns outside the row
    assert _multiclass_run(c)[0] == E_SHAPE


# ============================================================================================ soft-NMS
def _soft_run(d, method, min_score):
    lib, L = _L()
    n = len(d)
    out, inds, num = _floats(5 * n), _ints(n), _ints(1)
    d_dets = _dev(d)
    rc = L.kgdet_soft_nms(_ptr(d_dets), c_i64(n), c_f(E.SOFT_IOU), c_i32(method), c_f(E.SOFT_SIGMA), c_f(min_score), out.ptr(), inds.ptr(),
                          num.ptr(), _st())
    torch.cuda.synchronize()
    assert out.intact() and inds.intact() and num.intact()
    return rc, out.view().cpu().numpy().reshape(n, 5), _get(inds), int(_get(num)[0])


def _soft_check(d, method, min_score, tag):
    lib, L = _L()
    rc, out, inds, m = _soft_run(d, method, min_score)
    lib.check(rc, tag)
    wd, wi = E.soft_nms(d, E.SOFT_IOU, method, E.SOFT_SIGMA, min_score)
    print('NMS-SOFT %s: %d of %d left (oracle %d)' % (tag, m, len(d), len(wi)))
    assert m == len(wi)
    assert (inds[:m] == wi).all(), '%s: rows differ from position %d' % (tag, int(np.nonzero(inds[:m] != wi)[0][0]))
    assert (_bits(out[:m]) == _bits(wd)).all()
    assert np.isnan(out[m:]).all() and (inds[m:] == UNTOUCHED).all()


@pytest.mark.parametrize('method,n,regime', E.SOFT_CASES)
def test_soft_nms_methods_lengths_and_min_scores(method, n, regime):
    """methods 0, 1, 2 at lengths either side of the 512 threads and of two boxes per thread; min_score removing most boxes (holes
    and movers across the threads' runs), none, and -- method 0, min_score 0 -- equal to the decayed scores, which stay"""
    _soft_check(E.soft_dets(n), method, E.SOFT_MIN_SCORE[regime], 'method %d n %d %s' % (method, n, regime))


@pytest.mark.parametrize('method', E.SOFT_METHODS)
def test_soft_nms_all_tied_takes_the_first_maximum(method):
    for regime in ('many', 'none'):
        _soft_check(E.soft_dets(513, tied=True), method, E.SOFT_MIN_SCORE[regime], 'tied method %d %s' % (method, regime))


def test_soft_nms_at_its_capacity_and_beyond():
    _soft_check(E.soft_dets(E.SOFT_LIMIT), 1, E.SOFT_MIN_SCORE['many'], '4544 boxes')
    rc, out, inds, m = _soft_run(E.soft_dets(E.SOFT_LIMIT + 1), 1, E.SOFT_MIN_SCORE['many'])
    assert rc == E_UNSUPPORTED and np.isnan(out).all() and (inds == UNTOUCHED).all() and m == UNTOUCHED
