"""The numpy side of the device accumulate / landmark packing (evaluation_device.py), on the CPU: ``accumulate_restatement`` is
``CocoEvaluator.accumulate``; the one stable sort per evaluation selects what the per-``max_dets`` sorts select; a lazy
landmark Packed materialised on the host is the eager one; and the kernel's rounding, ``rint(v * 1e4) / 1e4`` on widened
float32 values, is ``np.round(float64, 4)`` bit for bit -- at and beside the ties too."""
import copy

import numpy as np
import pytest

from kgdet_amd import evaluation as ev
from kgdet_amd import evaluation_device as evd
from tests import eval_accumulate_cases as acc
from tests import eval_cases as cases

TYPES = ['bbox', 'keypoints']


@pytest.mark.parametrize('case', ['a', 'b', 'gt', 'live', 'stress'])
def test_accumulate_restatement_equals_coco_evaluator(case):
    gt, results = acc.case_inputs(case)
    for typ in TYPES:
        want = cases.host_evaluator(gt, results[typ], typ)
        got = cases.packed_evaluator(gt, results[typ], typ, 'cpu')
        got.eval = {}
        assert got.accumulate_restatement() is got
        assert got.eval['counts'] == want.eval['counts']
        for key in ('precision', 'recall', 'scores'):
            assert got.eval[key].dtype == np.float64 and np.array_equal(got.eval[key], want.eval[key]), (typ, key)
        again = cases.packed_evaluator(gt, results[typ], typ, 'cpu')          # accumulate() off the device IS the restatement
        for key in ('precision', 'recall', 'scores'):
            assert again.eval[key].tobytes() == got.eval[key].tobytes()


def test_one_stable_sort_serves_every_max_dets():
    gt, results = cases.stress_case()
    for typ in TYPES:
        pg = evd.pack_ground_truth(ev.CocoIndex(copy.deepcopy(gt)))
        d = evd.pack_results(pg, copy.deepcopy(results[typ]))
        K = len(pg.cat_ids)
        order, cat_cut = evd.category_order(d, K)
        assert order.dtype == np.int64 and cat_cut.dtype == np.int64 and cat_cut[0] == 0 and cat_cut[-1] == len(d.score)
        assert np.array_equal(np.sort(order), np.arange(len(d.score)))
        rank = np.arange(len(d.score)) - d.start[d.cell]
        d_by_cat = np.argsort(d.cat_idx, kind='mergesort')                  # (the current code's route, per m)
        d_cut = np.searchsorted(d.cat_idx[d_by_cat], np.arange(K + 1))
        n_ties = 0
        for k in range(K):
            seq = order[cat_cut[k]:cat_cut[k + 1]]
            assert (d.cat_idx[seq] == k).all()
            dk = d_by_cat[d_cut[k]:d_cut[k + 1]]
            n_ties += len(dk) - len(np.unique(d.score[dk]))
            for max_det in ev.EvalParams(typ).max_dets:
                sel = np.nonzero(rank[dk] < max_det)[0]
                want = dk[sel[np.argsort(-d.score[dk][sel], kind='mergesort')]]
                assert np.array_equal(seq[rank[seq] < max_det], want), (typ, k, max_det)
        assert n_ties > 10                                                  # (equal scores are what the claim is about)


@pytest.mark.parametrize('case', ['live', 'stress'])
def test_lazy_packed_materialised_on_the_cpu_equals_the_eager_one(case):
    gt, results = acc.case_inputs(case)
    data, res = acc.detector_results(gt, results)
    pg = evd.pack_ground_truth(data.coco)
    eager = evd.pack_test_results(pg, data, res)
    lazy = evd.pack_test_results(pg, data, res, lazy_landmarks=True)
    lk = lazy['keypoints']
    assert lk.kxy is None and lk.bbox is None and lk.area is None
    assert lk.kxy32.dtype == np.float32 and lk.kxy32.shape == (len(lk.score), 882) and len(lk.score) > 50
    for key in ('cell', 'start', 'img_idx', 'cat_idx', 'score', 'id'):
        assert np.array_equal(getattr(lk, key), getattr(eager['keypoints'], key)), key
    for key in ('cell', 'start', 'img_idx', 'cat_idx', 'score', 'id', 'bbox', 'area'):
        assert np.array_equal(getattr(lazy['bbox'], key), getattr(eager['bbox'], key)), key
    # through the evaluator's CPU path (which materialises) ...
    a = evd.DeviceCocoEvaluator(pg, lk, 'keypoints', device='cpu').evaluate().accumulate()
    b = evd.DeviceCocoEvaluator(pg, eager['keypoints'], 'keypoints', device='cpu').evaluate().accumulate()
    for key in ('kxy', 'bbox', 'area'):
        x, y = getattr(lk, key), getattr(eager['keypoints'], key)
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), key
    for key in ('precision', 'recall', 'scores'):
        assert np.array_equal(a.eval[key], b.eval[key])
    # ... and through the public helper
    again = evd.materialize(evd.pack_test_results(pg, data, res, lazy_landmarks=True)['keypoints'])
    for key in ('kxy', 'bbox', 'area'):
        assert np.array_equal(getattr(again, key), getattr(eager['keypoints'], key)), key
    assert evd.materialize(eager['keypoints']) is eager['keypoints']
    got = evd.evaluate_results(data, res, TYPES, device='cpu', lazy_landmarks=True)
    want = evd.evaluate_results(data, res, TYPES, device='cpu')
    for typ in TYPES:
        assert np.array_equal(got[typ], want[typ])


def test_device_accumulate_is_refused_off_the_device():
    gt, results = cases.golden_case('a')
    pg = evd.pack_ground_truth(ev.CocoIndex(copy.deepcopy(gt)))
    e = evd.DeviceCocoEvaluator(pg, evd.pack_results(pg, copy.deepcopy(results['bbox'])), 'bbox', device='cpu',
                                device_accumulate=True)
    with pytest.raises(ValueError):
        e.evaluate()


def test_the_kernels_rounding_is_np_round_at_and_beside_the_ties():
    v = acc.rounding_values()
    assert v.dtype == np.float32 and len(v) > 30000
    wide = v.astype(np.float64)
    want = np.round(wide, 4)
    got = evd.round_landmarks_restatement(v, 4)
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
    frac = np.abs(wide) * 1e4 - np.floor(np.abs(wide) * 1e4)
    assert (frac == 0.5).sum() > 1000 and ((np.abs(frac - 0.5) < 1e-3) & (frac != 0.5)).sum() > 1000
    up = want[(frac == 0.5) & (wide > 0)] * 1e4
    assert (np.rint(up) % 2 == 0).all()                                     # (ties went to even)
    for digits in (0, 1, 3, 6):
        assert evd.round_landmarks_restatement(v, digits).tobytes() == np.round(wide, digits).tobytes(), digits
    rows = acc.rounding_rows()
    assert rows.shape[1] == 882 and len(rows) >= 20
