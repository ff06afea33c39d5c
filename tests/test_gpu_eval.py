"""The HIP evaluator kernels (csrc/coco_eval.hip through evaluation_device.DeviceCocoEvaluator) against evaluation.CocoEvaluator,
and the validation hook of runner.Runner on the demo pipeline.

Similarities: box IoU bit-equal; OKS within a relative 1e-12 (bit-identical exponent argument; each library's float64 exp
good to a few ulp; at most 294 non-negative terms summed in another order: under 7e-14 together).  Matching, eval arrays and
stats are compared for EQUALITY, which is sound only where no decision sits inside that tolerance: ``_decision_margin`` checks
every input of this file on the CPU first -- every similarity at least 1e-9 away from every threshold and from 1 - 1e-10, any
two candidates of one detection exactly equal or 1e-9 apart.  One kind of value is exempt from the first check, by reasoning
on the INPUTS and not by measurement: a similarity of 1.0 that is provably exact (``_provably_one``) -- a box identical to the
ground truth's (intersection = union = the one area), or landmarks whose every exponent argument is exactly 0 (ground truth
fed back as detections; every landmark inside the doubled box of a ground truth without labelled landmarks): exp(-0) = 1 in
any library, a sum of at most 294 ones is exact in any order, n / n = 1, so the device gives the same bits.  Such a value is
1e-10 from the cap and cannot be moved away from it; the issue's own ground-truth-as-detections case consists of them.  A 1.0
that is not provably exact is checked like any other value."""
import copy
import os

import numpy as np
import pytest
import torch

from kgdet_amd import evaluation as ev
from kgdet_amd import evaluation_device as evd
from tests import eval_cases as cases

pytestmark = pytest.mark.gpu
TYPES = ['bbox', 'keypoints']
CASES = ['a', 'b', 'gt', 'live', 'stress', 'replicated']
_cache = {}


def _inputs(case):
    if case not in _cache:
        if case == 'stress':
            _cache[case] = cases.stress_case()
        elif case == 'replicated':
            _cache[case] = cases.replicated_case(8)         # 256 images
        else:
            _cache[case] = cases.golden_case(case)
    return _cache[case]


def _pair(case, typ):
    key = (case, typ)
    if key not in _cache:
        gt, results = _inputs(case)
        _cache[key] = (cases.packed_evaluator(gt, results[typ], typ, 'cuda'), cases.host_evaluator(gt, results[typ], typ))
    return _cache[key]


def _provably_one(want, img_id, cat_id):
    """[D, G] mask (rows in the order of ``_similarity``): the inputs alone make this similarity exactly 1.0 (module docstring)"""
    gts, dts = want._pair(img_id, cat_id)
    order = np.argsort([-d['score'] for d in dts], kind='mergesort')[:want.params.max_dets[-1]]
    dts = [dts[i] for i in order]
    mask = np.zeros((len(dts), len(gts)), bool)
    for j, g in enumerate(gts):
        for i, d in enumerate(dts):
            if want.params.iou_type == 'bbox':
                mask[i, j] = [float(v) for v in d['bbox']] == [float(v) for v in g['bbox']] and d['bbox'][2] * d['bbox'][3] > 0
                continue
            k, q = np.asarray(g['keypoints'], dtype=np.float64), np.asarray(d['keypoints'], dtype=np.float64)
            vis = k[2::3] > 0
            if vis.any():
                dx, dy = (q[0::3] - k[0::3])[vis], (q[1::3] - k[1::3])[vis]
            else:
                bx, by, bw, bh = g['bbox']
                dx = np.maximum(0, (bx - bw) - q[0::3]) + np.maximum(0, q[0::3] - (bx + bw * 2))
                dy = np.maximum(0, (by - bh) - q[1::3]) + np.maximum(0, q[1::3] - (by + bh * 2))
            mask[i, j] = bool(np.all(dx == 0) and np.all(dy == 0))
    return mask


def _decision_margin(want):
    """(closest approach of a similarity to a threshold / to 1 - 1e-10, closest two unequal candidates of one detection) over
    all cells of a CocoEvaluator; provably exact values of 1.0 left out of the first (module docstring)"""
    borders = np.concatenate([want.params.iou_thrs, [1 - 1e-10]])
    to_border, to_rival = np.inf, np.inf
    for i in want.params.img_ids:
        for c in want.params.cat_ids:
            s = want._similarity(i, c)
            if not s.size:
                continue
            exact = _provably_one(want, i, c)
            assert (s[exact] == 1.0).all()
            v = s[~exact]
            if v.size:
                to_border = min(to_border, float(np.abs(v[:, None] - borders[None, :]).min()))
            gaps = np.diff(np.sort(s, axis=1), axis=1)
            gaps = gaps[gaps != 0]
            if gaps.size:
                to_rival = min(to_rival, float(gaps.min()))
    return to_border, to_rival


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('typ', TYPES)
def test_similarities(case, typ):
    got, want = _pair(case, typ)
    assert str(got.device) == 'cuda'
    worst, n = 0.0, 0
    for i, c, mine, theirs in cases.similarities(got, want):
        assert mine.shape == theirs.shape, (i, c)
        if not mine.size:
            continue
        n += mine.size
        if typ == 'bbox':
            assert np.array_equal(mine, theirs), (i, c)
        else:
            with np.errstate(divide='ignore', invalid='ignore'):
                rel = np.where(theirs != 0, np.abs(mine - theirs) / np.abs(theirs), np.abs(mine))
            worst = max(worst, float(rel.max()))
    print('similarity %s %s: %d values, worst relative difference %.3e' % (case, typ, n, worst))
    assert n > 50
    assert worst <= 1e-12


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('typ', TYPES)
def test_matching_eval_arrays_and_stats_equal(case, typ):
    got, want = _pair(case, typ)
    to_border, to_rival = _decision_margin(want)
    print('margin %s %s: %.3e to a threshold, %.3e between unequal candidates' % (case, typ, to_border, to_rival))
    assert to_border >= 1e-9 and to_rival >= 1e-9, 'the INPUT is unfit for an equality test: re-draw it with another seed'
    cases.assert_same_matching(got, want)


@pytest.mark.parametrize('typ', TYPES)
def test_two_evaluations_give_the_same_bits(typ):
    gt, results = _inputs('stress')
    a = cases.packed_evaluator(gt, results[typ], typ, 'cuda')
    b = cases.packed_evaluator(gt, results[typ], typ, 'cuda')
    for key in ('sim', 'd_match', 'd_ignore', 'g_ignore'):
        x, y = getattr(a._out, key), getattr(b._out, key)
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), key
    for key in ('precision', 'recall', 'scores'):
        assert a.eval[key].tobytes() == b.eval[key].tobytes()
    assert a.stats.tobytes() == b.stats.tobytes()


def test_chunked_launches_equal_one_launch(monkeypatch):
    gt, results = _inputs('stress')
    whole = cases.packed_evaluator(gt, results['keypoints'], 'keypoints', 'cuda')
    monkeypatch.setitem(evd.CHUNK_DETS, 'keypoints', 23)
    parts = cases.packed_evaluator(gt, results['keypoints'], 'keypoints', 'cuda')
    for key in ('sim', 'd_match', 'd_ignore', 'g_ignore'):
        assert getattr(whole._out, key).tobytes() == getattr(parts._out, key).tobytes(), key


def test_kernel_argument_checks():
    import ctypes
    from kgdet_amd import _lib
    L = _lib.lib()
    z, i32, i64 = ctypes.c_void_p(0), ctypes.c_int32, ctypes.c_int64
    rc = L.kgdet_coco_match(z, z, i32(1), i64(0), i64(0), i64(0), z, z, z, z, z, z, i32(7), z, i32(10), z, z, z, z, z)
    assert rc == _lib.KGDET_E_SHAPE and b'lanes' in L.kgdet_last_error()
    rc = L.kgdet_coco_similarity(i32(2), z, z, i32(1), i64(0), i64(0), i64(1), z, z, z, z, z, z, z, z, i32(294), z, z)
    assert rc == _lib.KGDET_E_SHAPE and b'iou_type' in L.kgdet_last_error()
    rc = L.kgdet_coco_similarity(i32(0), z, z, i32(1), i64(1), i64(1), i64(1), z, z, z, z, z, z, z, z, i32(294), z, z)
    assert rc == _lib.KGDET_E_SHAPE and b'null' in L.kgdet_last_error()


# --- the validation hook (the set-up of tests/test_gpu_runner.py) ------------------------------------------------------------
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


def test_runner_validates_after_every_epoch(tmp_path, monkeypatch):
    from kgdet_amd import runner as rn
    from tests.golden import demo_cases
    loader = _loader(2)
    val = demo_cases.demo_dataset(test_mode=True)

    def make():
        cfg, model = demo_cases.demo_detector()
        model = model.cuda()
        return model, rn.build_optimizer(model, dict(type='Adam', lr=1e-4))

    def runner(model, opt, work, **kw):
        return rn.Runner(model, opt, work_dir=str(work), lr_config=DEMO_LR,
                         optimizer_config=dict(grad_clip=dict(max_norm=35, norm_type=2)),
                         checkpoint_config=dict(interval=1), log_interval=1, logger=lambda s: None,
                         batch_processor=_process, **kw)

    seen = []
    real = rn.single_gpu_test

    def recording(*args, **kw):
        seen.append(real(*args, **kw))
        return seen[-1]
    monkeypatch.setattr(rn, 'single_gpu_test', recording)

    model, opt = make()
    r = runner(model, opt, tmp_path / 'val', eval_config=dict(dataset=val, interval=1, imgs_per_gpu=4,
                                                             to_device=lambda t: t.cuda(non_blocking=True)))
    r.run(loader, max_epochs=3, to_device=_to_device)
    assert model.training and r.epoch == 3 and len(seen) == 3
    records = [rec for rec in r.log_history if 'bbox_mAP' in rec]
    assert len(records) == 3 and [rec['epoch'] for rec in records] == [1, 2, 3]
    assert len([rec for rec in r.log_history if 'loss' in rec]) == 6
    names = ['mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l']
    for n, (rec, results) in enumerate(zip(records, seen)):
        files = ev.results2json(val, results, str(tmp_path / ('epoch%d' % n)))
        want = ev.coco_eval(files, TYPES, val.coco, verbose=False)
        for t in TYPES:
            for i, name in enumerate(names):
                assert rec['%s_%s' % (t, name)] == float('{:.3f}'.format(want[t][i])), (n, t, name)
            assert rec['%s_mAP_copypaste' % t] == ('{ap[0]:.3f} {ap[1]:.3f} {ap[2]:.3f} {ap[3]:.3f} '
                                                   '{ap[4]:.3f} {ap[5]:.3f}').format(ap=want[t][:6])
        assert set(rec) == {'epoch'} | {'%s_%s' % (t, k) for t in TYPES for k in names + ['mAP_copypaste']}
        print('epoch %d: %s | %s' % (n + 1, rec['bbox_mAP_copypaste'], rec['keypoints_mAP_copypaste']))
    assert r._packed_gt is not None and os.path.isfile(str(tmp_path / 'val' / 'epoch_3.pth'))

    monkeypatch.setattr(rn, 'single_gpu_test', real)
    plain_model, plain_opt = make()
    plain = runner(plain_model, plain_opt, tmp_path / 'plain').run(loader, max_epochs=3, to_device=_to_device)
    assert not [rec for rec in plain.log_history if 'bbox_mAP' in rec]
    bad = [k for (k, a), b in zip(model.state_dict().items(), plain_model.state_dict().values()) if not torch.equal(a, b)]
    assert not bad, 'validation changed the training: %s' % bad[:8]
