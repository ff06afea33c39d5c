"""``kgdet_coco_accumulate`` / ``kgdet_coco_count_gt`` / ``kgdet_coco_pack_landmarks`` (csrc/coco_accumulate.hip), through the
C ABI and through ``DeviceCocoEvaluator``.

The bar is EQUALITY of bits (``np.array_equal`` on float64 arrays without NaN), not a tolerance: the counts are integers, the
two divisions of accumulate and the multiplication / division of the rounding are single correctly rounded float64
operations compiled without contraction, ``rint`` is ties-to-even in numpy and on the device, max / min / comparisons are
exact.  The reference is ``accumulate_restatement`` on the SAME evaluate output (held to ``CocoEvaluator.accumulate`` on the
CPU by tests/test_eval_accumulate_refs.py), and the host packing for the landmark kernel.  Outputs are pre-filled with NaN
between canaries: every element must be written and nothing beside them."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from kgdet_amd import _lib
from kgdet_amd import evaluation as ev
from kgdet_amd import evaluation_device as evd
from tests import eval_accumulate_cases as acc

pytestmark = pytest.mark.gpu
TYPES = ['bbox', 'keypoints']
CASES = ['a', 'b', 'gt', 'live', 'stress', 'replicated']
KEYS = ('precision', 'recall', 'scores')
PAD, CANARY = 64, -12345.5
TILE = acc.header_constant('KGDET_COCO_ACC_TILE')
PACK_ROWS = acc.header_constant('KGDET_COCO_PACK_ROWS')
i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
_cache = {}


def _inputs(case):
    if case not in _cache:
        _cache[case] = acc.case_inputs(case)
    return _cache[case]


def _evaluator(gt, results, typ, edit=None, **kw):
    pg = evd.pack_ground_truth(ev.CocoIndex(copy.deepcopy(gt)))
    e = evd.DeviceCocoEvaluator(pg, evd.pack_results(pg, copy.deepcopy(results)), typ, device='cuda', **kw)
    if edit:
        edit(e.params)
    return e.evaluate()


def _evaluated(case, typ):
    """one device evaluate per (case, type), outputs kept on the device; shared and left unchanged"""
    if (case, typ) not in _cache:
        gt, results = _inputs(case)
        _cache[case, typ] = _evaluator(gt, results[typ], typ, device_accumulate=True)
    return _cache[case, typ]


def _restatement(e, stats=True):
    """accumulate_restatement on e's own evaluate output -> (eval arrays, stats)"""
    e.accumulate_restatement()
    want = {k: e.eval[k].copy() for k in KEYS}
    return want, (np.array(e.summarize(verbose=False)) if stats else None)


def _up(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype, copy=False))).cuda()


def _guarded(sizes, dtype, fill, canary):
    """one device buffer: canary | block | canary | block ... | canary -> (buffer, [views], check())"""
    total = PAD + sum(n + PAD for n in sizes)
    buf = torch.full((total,), canary, dtype=dtype, device='cuda')
    views, spans, at = [], [], PAD
    for n in sizes:
        buf[at:at + n] = fill
        views.append(buf[at:at + n])
        spans.append((at, at + n))
        at += n + PAD

    def check():
        host = buf.cpu().numpy()
        keep = np.ones(total, bool)
        for lo, hi in spans:
            keep[lo:hi] = False
        assert (host[keep] == canary).all(), 'a canary was overwritten'
    return buf, views, check


def _accumulate_args(e):
    """the arguments of kgdet_coco_accumulate for an evaluated (device_accumulate) evaluator, outputs NaN-filled in canaries"""
    p, d, g = e.params, e.dt, e.gt
    T, R, K, A, M = len(p.iou_thrs), len(p.rec_thrs), len(p.cat_ids), len(p.area_rng), len(p.max_dets)
    nd, ng = len(d.score), len(g.id)
    order, cat_cut = evd.category_order(d, K)
    rank = (np.arange(nd) - d.start[d.cell]) if nd else np.zeros(0, np.int64)
    d_match, d_ignore, g_ignore = e._out.dev
    assert d_match.is_cuda and d_match.shape == (nd, A, T) and g_ignore.shape == (ng, A)
    L = _lib.lib()
    _, (n_gt,), check_n = _guarded([K * A], torch.int32, -9, -7)
    g_cat = _up(g.cat_idx, np.int32)
    rc = L.kgdet_coco_count_gt(_lib.ptr(g_ignore), _lib.ptr(g_cat), i64(ng), i32(K), i32(A), _lib.ptr(n_gt), _lib.current_stream())
    assert rc == 0, L.kgdet_last_error()
    check_n()
    gi = g_ignore.cpu().numpy()
    want_n = np.array([[np.count_nonzero(gi[g.cat_idx == k, a] == 0) for a in range(A)] for k in range(K)], np.int32)
    assert np.array_equal(n_gt.cpu().numpy().reshape(K, A), want_n)
    tp_cap = int(np.minimum(np.diff(cat_cut), np.bincount(g.cat_idx, minlength=K)[:K]).max())
    nP, nR = T * R * K * A * M, T * K * A * M
    _, (prec, rec, sco), check = _guarded([nP, nR, nP], torch.float64, float('nan'), CANARY)
    work = torch.full((max(2 * tp_cap * K * A * M * T, 1),), float('nan'), dtype=torch.float64, device='cuda')
    keep = [_up(d.score, np.float64), _up(rank, np.int32), _up(order, np.int64), _up(cat_cut, np.int64), n_gt,
            _up(p.max_dets, np.int32), _up(p.rec_thrs, np.float64), work, g_cat]
    a = dict(d_match=_lib.ptr(d_match), d_ignore=_lib.ptr(d_ignore), score=_lib.ptr(keep[0]), rank=_lib.ptr(keep[1]),
             order=_lib.ptr(keep[2]), cat_cut=_lib.ptr(keep[3]), n_gt=_lib.ptr(n_gt), max_dets=_lib.ptr(keep[5]),
             rec_thrs=_lib.ptr(keep[6]), ND=i64(nd), K=i32(K), A=i32(A), T=i32(T), M=i32(M), R=i32(R), tp_cap=i64(tp_cap),
             precision=_lib.ptr(prec), recall=_lib.ptr(rec), scores=_lib.ptr(sco), workspace=_lib.ptr(work),
             workspace_bytes=ctypes.c_size_t(2 * tp_cap * K * A * M * T * 8), stream=_lib.current_stream())
    out = dict(precision=(prec, (T, R, K, A, M)), recall=(rec, (T, K, A, M)), scores=(sco, (T, R, K, A, M)))
    return a, out, check, keep, want_n, cat_cut


def _call(a):
    return _lib.lib().kgdet_coco_accumulate(*[a[k] for k in (
        'd_match', 'd_ignore', 'score', 'rank', 'order', 'cat_cut', 'n_gt', 'max_dets', 'rec_thrs', 'ND', 'K', 'A', 'T', 'M', 'R',
        'tp_cap', 'precision', 'recall', 'scores', 'workspace', 'workspace_bytes', 'stream')])


def _kernel(e):
    """kgdet_coco_accumulate through the C ABI on e's device outputs -> {precision, recall, scores} as numpy"""
    a, out, check, keep, _, _ = _accumulate_args(e)
    rc = _call(a)
    assert rc == 0, _lib.lib().kgdet_last_error()
    torch.cuda.synchronize()
    check()
    got = {k: t.cpu().numpy().reshape(shape) for k, (t, shape) in out.items()}
    for k in KEYS:
        assert not np.isnan(got[k]).any(), '%s: an element was not written' % k
    return got


def _assert_equal(got, want, what):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype == np.float64 and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('typ', TYPES)
def test_kernel_equals_the_restatement_on_the_same_evaluate_output(case, typ):
    e = _evaluated(case, typ)
    assert isinstance(e._out, evd._DeviceOutputs)
    got = _kernel(e)
    e.accumulate()                                              # the class: kernel route
    by_class = {k: e.eval[k].copy() for k in KEYS}
    stats = np.array(e.summarize(verbose=False))
    want, want_stats = _restatement(e)
    _assert_equal(got, want, 'C ABI')
    _assert_equal(by_class, want, 'class')
    assert stats.tobytes() == want_stats.tobytes()
    assert (want['precision'] > 0).sum() > 100                  # (not a trivial comparison)


def _edge(name):
    """(ground truth, results, params edit) of one hand-made edge"""
    if name == 'long':                                          # one category: two scan tiles and a ragged tail
        n_images = (2 * TILE + TILE // 4 + 9) // 10 + 1
        return acc.edge_dataset(n_images, seed=3, only_first=True) + (None,)
    gt, dets = acc.edge_dataset()
    if name == 'empty':
        return gt, [], None
    edits = dict(
        default=None,
        single=lambda p: (setattr(p, 'iou_thrs', np.array([0.5])), setattr(p, 'rec_thrs', np.array([0.3])),
                          setattr(p, 'area_rng', [[0, 1e10]]), setattr(p, 'area_lbl', ['all'])),
        at64=lambda p: (setattr(p, 'iou_thrs', np.linspace(0.3, 0.9, 8)),
                        setattr(p, 'area_rng', [[0, 1e10], [0, 500], [500, 1024], [1024, 2000], [2000, 3000], [3000, 9216],
                                                [9216, 20000], [20000, 1e10]]),
                        setattr(p, 'area_lbl', ['r%d' % i for i in range(8)])),
        rec01=lambda p: setattr(p, 'rec_thrs', np.array([0.0, 1.0, 0.5, 0.0, 1.0])))
    return gt, dets, edits[name]


@pytest.mark.parametrize('name', ['default', 'single', 'at64', 'rec01', 'long', 'empty'])
def test_hand_made_edges(name):
    gt, dets, edit = _edge(name)
    e = _evaluator(gt, dets, 'bbox', edit, device_accumulate=True)
    p = e.params
    assert list(p.max_dets) == [1, 10, 100]
    a, _, _, _, n_gt, cat_cut = _accumulate_args(e)
    got = _kernel(e)
    e.accumulate()
    by_class = {k: e.eval[k].copy() for k in KEYS}
    want, _ = _restatement(e, stats=False)
    _assert_equal(got, want, name)
    _assert_equal(by_class, want, name)
    T, R, K, A, M = e.eval['counts']
    if name == 'default':                                       # the edges are really there (categories of edge_dataset)
        assert 0.0 in p.rec_thrs and 1.0 in p.rec_thrs
        assert cat_cut[2] == cat_cut[1] and (n_gt[1] > 0).any()                        # ground truth, no detection
        assert (want['recall'][:, 1][:, n_gt[1] > 0] == 0).all() and (want['precision'][:, :, 1][:, :, n_gt[1] > 0] == 0).all()
        assert list(n_gt[2] == 0) == [False, False, False, True] and cat_cut[3] > cat_cut[2]   # n_gt == 0 for 'large' alone
        assert (want['precision'][:, :, 2, 3] == -1).all() and (want['recall'][:, 2, 3] == -1).all()
        assert want['recall'][0, 2, 0, 2] == 1.0 and (want['precision'][0, :, 2, 0, 2] > 0).all()   # recall reaches 1.0
        sel = e.dt.cat_idx == 3
        assert sel.sum() >= 18 and e._out.d_ignore[sel].all() and not e._out.d_match[sel].any()   # every detection ignored
        assert (want['recall'][:, 3, 0] == 0).all() and (want['precision'][:, :, 3, 0] == 0).all()
        assert 0 < want['recall'][0, 4, 0, 2] < 0.1 and (want['precision'][0, 50:, 4, 0, 2] == 0).all()   # low recall
        per_cell = np.diff(e.dt.start)
        assert (per_cell > 10).any() and ((per_cell > 0) & (per_cell < 10)).any()
        first = e.dt.score[e.dt.cat_idx == 0]
        assert len(np.unique(first)) <= 4 < len(first)                                 # equal scores, in and across cells
        assert not np.array_equal(want['precision'][..., 0], want['precision'][..., 2])   # max_dets matters
    elif name == 'single':
        assert (T, R, A) == (1, 1, 1)
    elif name == 'at64':
        assert A * T == 64 and (want['precision'] > 0).any() and (want['precision'] == -1).any()
    elif name == 'rec01':
        assert np.array_equal(want['precision'][:, 0], want['precision'][:, 3]) and (want['precision'][:, 0] > 0).any()
    elif name == 'long':
        n = int(cat_cut[1] - cat_cut[0])
        assert n >= 2 * TILE + 1 and n % TILE != 0 and a['K'].value == 1
    elif name == 'empty':
        assert len(e.dt.score) == 0 and set(np.unique(want['precision'])) <= {0.0, -1.0} and (want['recall'] == 0).any()


@pytest.mark.parametrize('typ', TYPES)
def test_two_runs_give_the_same_bits(typ):
    e = _evaluated('stress', typ)
    a, b = _kernel(e), _kernel(e)
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes()


@pytest.mark.parametrize('typ', TYPES)
def test_chunked_evaluate_then_device_accumulate_equals_one_chunk(typ, monkeypatch):
    gt, results = _inputs('stress')
    whole = _evaluated('stress', typ)
    whole.accumulate()
    want = {k: whole.eval[k].copy() for k in KEYS}
    monkeypatch.setitem(evd.CHUNK_DETS, typ, len(whole.dt.score) // 4)
    parts = _evaluator(gt, results[typ], typ, device_accumulate=True)
    assert len(list(parts._chunks(evd.CHUNK_DETS[typ]))) >= 3
    for x, y in zip(whole._out.dev, parts._out.dev):
        assert torch.equal(x, y)
    parts.accumulate()
    _assert_equal({k: parts.eval[k] for k in KEYS}, want, 'chunked')
    _assert_equal(_kernel(parts), want, 'chunked, C ABI')


# --- kgdet_coco_pack_landmarks ---------------------------------------------------------------------------------------------
def _pack_kernel(src, num_digits=4):
    n, K = src.shape[0], src.shape[1] // 3
    _, (kxy, bbox, area), check = _guarded([n * K * 2, n * 4, n], torch.float64, float('nan'), CANARY)
    d_src = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    L = _lib.lib()
    rc = L.kgdet_coco_pack_landmarks(_lib.ptr(d_src), i64(n), i32(K), i32(num_digits), _lib.ptr(kxy), _lib.ptr(bbox),
                                     _lib.ptr(area), _lib.current_stream())
    assert rc == 0, L.kgdet_last_error()
    torch.cuda.synchronize()
    check()
    return kxy.cpu().numpy().reshape(n, K, 2), bbox.cpu().numpy().reshape(n, 4), area.cpu().numpy()


def _landmark_rows(case):
    if case == 'ties':
        return acc.rounding_rows()
    data, res = acc.detector_results(*_inputs(case))
    return np.concatenate([blk for r in res for blk in r[2] if len(blk)])


@pytest.mark.parametrize('case', ['live', 'stress', 'ties'])
def test_pack_kernel_is_bit_equal_to_the_host_packing(case):
    src = _landmark_rows(case)
    assert src.dtype == np.float32 and src.shape[1] == 882 and len(src) >= 20
    bbox, area, kxy = evd._landmarks_in_order([src], len(src), np.arange(len(src)), 294, 4)     # the host packing
    got_kxy, got_bbox, got_area = _pack_kernel(src)
    for name, g, w in (('kxy', got_kxy, kxy), ('bbox', got_bbox, bbox), ('area', got_area, area)):
        assert not np.isnan(g).any() and g.shape == w.shape and np.array_equal(g, w), (case, name)
    assert got_kxy.tobytes() == kxy.tobytes()                  # (the rounded values to the bit, signed zeros included)
    for n in (1, PACK_ROWS - 1, PACK_ROWS, PACK_ROWS + 1):      # any row count, nothing written beside the rows
        part = _pack_kernel(src[:n])
        assert np.array_equal(part[0], kxy[:n]) and np.array_equal(part[1], bbox[:n]) and np.array_equal(part[2], area[:n])


@pytest.mark.parametrize('case', ['live', 'stress'])
def test_lazy_route_with_device_accumulate_equals_todays_route(case):
    data, res = acc.detector_results(*_inputs(case))
    pg = evd.pack_ground_truth(data.coco)
    today = evd.evaluate_results(data, res, TYPES, device='cuda', packed_gt=pg, device_accumulate=False)
    new = evd.evaluate_results(data, res, TYPES, device='cuda', packed_gt=pg, lazy_landmarks=True, device_accumulate=True)
    for typ in TYPES:
        assert np.array_equal(new[typ], today[typ]) and (today[typ][:2] > 0).all()
    eager = evd.pack_test_results(pg, data, res)
    lazy = evd.pack_test_results(pg, data, res, lazy_landmarks=True)
    for typ in TYPES:
        old = evd.DeviceCocoEvaluator(pg, eager[typ], typ, device='cuda', device_accumulate=False).evaluate().accumulate()
        e = evd.DeviceCocoEvaluator(pg, lazy[typ], typ, device='cuda', device_accumulate=True).evaluate().accumulate()
        assert isinstance(e._out, evd._DeviceOutputs) and 'd_match' not in e._out.__dict__      # nothing downloaded so far
        _assert_equal({k: e.eval[k] for k in KEYS}, {k: old.eval[k] for k in KEYS}, typ)
        K, A, I = len(pg.cat_ids), len(e.params.area_rng), len(pg.img_ids)
        n = 0
        for k in range(K):
            for a in range(A):
                for i in range(I):
                    w, g = old.eval_imgs_of(k, a, i), e.eval_imgs_of(k, a, i)
                    assert (w is None) == (g is None)
                    if w is not None:
                        n += 1
                        for key in w:
                            assert np.array_equal(w[key], g[key]), (typ, key, k, a, i)
        assert n > 20
    lk, ek = lazy['keypoints'], eager['keypoints']
    assert lk.kxy is None                                       # the float64 copy never existed on the host
    for key in ('cell', 'start', 'img_idx', 'cat_idx', 'score', 'id', 'bbox', 'area'):
        x, y = getattr(lk, key), getattr(ek, key)
        assert x.dtype == y.dtype and np.array_equal(x, y), key


def test_lazy_chunks_write_their_bbox_and_area_slices(monkeypatch):
    data, res = acc.detector_results(*_inputs('stress'))
    pg = evd.pack_ground_truth(data.coco)
    eager = evd.pack_test_results(pg, data, res)['keypoints']
    lazy = evd.pack_test_results(pg, data, res, lazy_landmarks=True)['keypoints']
    monkeypatch.setitem(evd.CHUNK_DETS, 'keypoints', len(lazy.score) // 4)
    for dev_acc in (True, False):
        lazy.bbox = lazy.area = None
        e = evd.DeviceCocoEvaluator(pg, lazy, 'keypoints', device='cuda', device_accumulate=dev_acc).evaluate().accumulate()
        assert len(list(e._chunks(evd.CHUNK_DETS['keypoints']))) >= 3
        assert np.array_equal(lazy.bbox, eager.bbox) and np.array_equal(lazy.area, eager.area)
        old = evd.DeviceCocoEvaluator(pg, eager, 'keypoints', device='cuda', device_accumulate=False).evaluate().accumulate()
        _assert_equal({k: e.eval[k] for k in KEYS}, {k: old.eval[k] for k in KEYS}, dev_acc)


# --- argument checks ---------------------------------------------------------------------------------------------------------
def test_argument_checks_refuse_before_any_launch():
    L = _lib.lib()
    e = _evaluated('a', 'bbox')
    a, out, check, keep, _, _ = _accumulate_args(e)
    null = vp(0)
    bad = [(dict(A=i32(7), T=i32(10)), _lib.KGDET_E_SHAPE, b'at most 64'),
           (dict(A=i32(0)), _lib.KGDET_E_SHAPE, b'area ranges'),
           (dict(K=i32(0)), _lib.KGDET_E_SHAPE, b'categories'),
           (dict(M=i32(-1)), _lib.KGDET_E_SHAPE, b'max_dets'),
           (dict(R=i32(0)), _lib.KGDET_E_SHAPE, b'recall thresholds'),
           (dict(K=i32(2 ** 30)), _lib.KGDET_E_SHAPE, b'lines'),
           (dict(ND=i64(-1)), _lib.KGDET_E_SHAPE, b'detections'),
           (dict(ND=i64(2 ** 31)), _lib.KGDET_E_SHAPE, b'detections'),
           (dict(tp_cap=i64(-1)), _lib.KGDET_E_SHAPE, b'tp_cap'),
           (dict(rec_thrs=null), _lib.KGDET_E_SHAPE, b'null'),
           (dict(precision=null), _lib.KGDET_E_SHAPE, b'null'),
           (dict(d_match=null), _lib.KGDET_E_SHAPE, b'null detection'),
           (dict(order=null), _lib.KGDET_E_SHAPE, b'null detection'),
           (dict(workspace=null), _lib.KGDET_E_WORKSPACE, b'workspace'),
           (dict(workspace_bytes=ctypes.c_size_t(a['workspace_bytes'].value - 1)), _lib.KGDET_E_WORKSPACE, b'workspace')]
    assert a['workspace_bytes'].value > 0
    for change, code, text in bad:
        args = dict(a)
        args.update(change)
        assert _call(args) == code, change
        assert text in L.kgdet_last_error(), (change, L.kgdet_last_error())
    torch.cuda.synchronize()
    check()
    for t, _ in out.values():                                   # nothing was launched: the outputs are still all NaN
        assert torch.isnan(t).all()
    z = null
    assert L.kgdet_coco_count_gt(z, z, i64(5), i32(3), i32(4), a['n_gt'], z) == _lib.KGDET_E_SHAPE and b'null' in L.kgdet_last_error()
    assert L.kgdet_coco_count_gt(z, z, i64(0), i32(3), i32(65), a['n_gt'], z) == _lib.KGDET_E_SHAPE
    assert L.kgdet_coco_count_gt(z, z, i64(-1), i32(3), i32(4), a['n_gt'], z) == _lib.KGDET_E_SHAPE
    one = vp(8)                                                 # (never dereferenced: every call below is refused)
    assert L.kgdet_coco_pack_landmarks(one, i64(1), i32(0), i32(4), one, one, one, z) == _lib.KGDET_E_SHAPE
    assert L.kgdet_coco_pack_landmarks(one, i64(-1), i32(294), i32(4), one, one, one, z) == _lib.KGDET_E_SHAPE
    assert L.kgdet_coco_pack_landmarks(one, i64(1), i32(294), i32(16), one, one, one, z) == _lib.KGDET_E_SHAPE
    assert L.kgdet_coco_pack_landmarks(one, i64(1), i32(294), i32(-1), one, one, one, z) == _lib.KGDET_E_SHAPE
    assert L.kgdet_coco_pack_landmarks(z, i64(1), i32(294), i32(4), one, one, one, z) == _lib.KGDET_E_SHAPE
    assert b'null' in L.kgdet_last_error()
    assert L.kgdet_coco_pack_landmarks(z, i64(0), i32(294), i32(4), z, z, z, z) == 0      # no rows: a no-op
    assert _call(a) == 0                                        # and the unchanged arguments are accepted
    torch.cuda.synchronize()
    check()


# --- the validation hook (the set-up of tests/test_gpu_eval.py) --------------------------------------------------------------
DEMO_LR = dict(policy='step', warmup='linear', warmup_iters=500, warmup_ratio=1.0 / 3, step=[8, 11])


def _loader(n_batches):
    from kgdet_amd import datasets as ds
    from tests.golden import demo_cases
    data = demo_cases.demo_dataset(test_mode=False, flip_ratio=0.5, with_label=True, with_crowd=False)
    np.random.seed(0)
    order = list(ds.GroupSampler(data, samples_per_gpu=2))[:2 * n_batches]
    batches = [ds.collate([data[i] for i in order[k:k + 2]]) for k in range(0, 2 * n_batches, 2)]
    for b in batches:
        b['img_metas'] = b.pop('img_meta')
    return batches


def _to_device(batch):
    out = dict(batch)
    out['img'] = batch['img'].cuda()
    for k in ('gt_bboxes', 'gt_labels', 'gt_keypoints'):
        out[k] = [t.cuda() for t in batch[k]]
    return out


def _process(model, batch, train_mode=True):
    from kgdet_amd import runner as rn
    losses = model.forward_train(batch['img'], batch['img_metas'], batch['gt_bboxes'], batch['gt_labels'],
                                 batch['gt_keypoints'])
    loss, log = rn.parse_losses(losses)
    return dict(loss=loss, log_vars=log, num_samples=len(batch['img']))


def test_runner_validate_logs_the_same_record_with_both_keys(tmp_path, monkeypatch):
    from kgdet_amd import runner as rn
    from tests.golden import demo_cases
    val = demo_cases.demo_dataset(test_mode=True)
    cfg, model = demo_cases.demo_detector()
    model = model.cuda()
    opt = rn.build_optimizer(model, dict(type='Adam', lr=1e-4))

    def runner(**keys):
        return rn.Runner(model, opt, work_dir=str(tmp_path), lr_config=DEMO_LR,
                         optimizer_config=dict(grad_clip=dict(max_norm=35, norm_type=2)), checkpoint_config=dict(interval=0),
                         log_interval=1, logger=lambda s: None, batch_processor=_process,
                         eval_config=dict(dataset=val, interval=1, imgs_per_gpu=4, to_device=lambda t: t.cuda(non_blocking=True),
                                          **keys))

    seen, calls = [], []
    real_test, real_eval = rn.single_gpu_test, evd.evaluate_results

    def once(*args, **kw):                                      # both runners evaluate the SAME detections
        if not seen:
            seen.append(real_test(*args, **kw))
        return seen[0]

    def recording(*args, **kw):
        calls.append((kw.get('lazy_landmarks'), kw.get('device_accumulate')))
        return real_eval(*args, **kw)
    monkeypatch.setattr(rn, 'single_gpu_test', once)
    monkeypatch.setattr(evd, 'evaluate_results', recording)
    r = runner(lazy_landmarks=True, device_accumulate=True)
    r.run(_loader(1), max_epochs=1, to_device=_to_device)
    new = [rec for rec in r.log_history if 'bbox_mAP' in rec]
    plain = runner()
    plain.epoch = r.epoch
    old = plain.validate()
    assert calls == [(True, True), (None, None)]
    assert len(new) == 1 and dict(new[0]) == dict(old) and list(new[0]) == list(old)
    assert 'keypoints_mAP_copypaste' in old and model.training
