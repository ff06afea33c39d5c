"""Inputs and comparisons shared by tests/test_eval_packed.py (numpy restatement) and tests/test_gpu_eval.py (HIP kernels):
the golden detection sets of tests/test_evaluation.py, a stress set built from the demo annotations, and the comparison
of a ``DeviceCocoEvaluator`` with ``CocoEvaluator`` at every level (similarities, per-cell matches, eval arrays, stats)."""
import copy
import importlib.util
import json
import os

import numpy as np

from kgdet_amd import evaluation as ev
from kgdet_amd import evaluation_device as evd

HERE = os.path.dirname(os.path.abspath(__file__))
GT = os.path.join(HERE, 'golden', 'demo_dataset-32.json')
GOLD = np.load(os.path.join(HERE, 'golden', 'eval_golden.npz'))
LIVE = np.load(os.path.join(HERE, 'golden', 'eval_live_golden.npz'))
STRESS_SEED = 2024          # (a stress input that breaks the decision-margin check of the GPU test is re-drawn by changing this)


def generator():
    spec = importlib.util.spec_from_file_location('make_eval_golden', os.path.join(HERE, 'golden', 'make_eval_golden.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def demo_gt():
    with open(GT) as f:
        return json.load(f)


def golden_case(case):
    """(ground truth dict, {'bbox': results, 'keypoints': results}, golden arrays prefix or None) for 'a', 'b', 'gt', 'live'"""
    gt, gen = demo_gt(), generator()
    if case in ('a', 'b'):
        b, k = gen.as_results(GOLD[case + '_boxes'], GOLD[case + '_kpts'], GOLD[case + '_cats'], GOLD[case + '_imgs'],
                              GOLD[case + '_scores'])
    elif case == 'live':
        b, k = gen.as_results(*gen.synth_detections(gt, seed=gen.LIVE_SEED))
    else:
        b = [dict(image_id=a['image_id'], bbox=a['bbox'], score=1.0, category_id=a['category_id']) for a in gt['annotations']]
        k = [dict(image_id=a['image_id'], keypoints=a['keypoints'], score=1.0, category_id=a['category_id'])
             for a in gt['annotations']]
    return gt, dict(bbox=b, keypoints=k)


def golden_arrays(case, typ):
    """(stats, precision, recall) of the reference evaluator; precision / recall None for the known-answer case"""
    if case == 'live':
        return LIVE['%s_stats' % typ], LIVE['%s_precision' % typ], LIVE['%s_recall' % typ]
    if case == 'gt':
        return GOLD['gt_%s_stats' % typ], None, None
    return GOLD['%s_%s_stats' % (case, typ)], GOLD['%s_%s_precision' % (case, typ)], GOLD['%s_%s_recall' % (case, typ)]


def _square_landmarks(k, x, y, side):
    """landmark triplets whose extent is exactly side x side at (x, y): every coordinate inside, two corners pinned"""
    k = np.asarray(k, dtype=np.float64).reshape(-1, 3).copy()
    k[:, 0] = x + (k[:, 0] % side)
    k[:, 1] = y + (k[:, 1] % side)
    k[0, :2], k[1, :2] = (x, y), (x + side, y + side)
    return k.reshape(-1)


def stress_case(seed=STRESS_SEED):
    """The demo annotations bent into every rule of the evaluator (see the issue's list): crowd ground truths, ground truths
    with num_keypoints == 0 (with and without labelled landmarks), one with no labelled landmark but num_keypoints > 0 (the
    doubled-box rule decides matches), a duplicated ground truth (equal similarities: the tie rule), images without ground
    truth and without detections, a cell with 130 detections, scores on a 0.01 grid (ties inside cells and across
    images), every eighth detection twice, areas exactly on and on both sides of 32^2 and 96^2."""
    gt, gen = demo_gt(), generator()
    rng = np.random.default_rng(seed)
    anns = gt['annotations']
    next_id = max(a['id'] for a in anns) + 1
    for n, a in enumerate(anns):
        if n % 7 == 1:
            a['iscrowd'] = 1
        if n % 9 == 2:
            a['num_keypoints'] = 0                      # ignored for landmarks, its labelled landmarks still define the OKS
        if n % 11 == 3:
            k = np.asarray(a['keypoints'], dtype=np.float64).reshape(-1, 3)
            k[:, 2] = 0
            a['keypoints'] = k.reshape(-1).tolist()
            a['num_keypoints'] = 0 if n % 2 else 5      # no labelled landmark at all: the doubled-box distance rule
        a['area'] = [1024.0, 9216.0, 1023.999, 1024.001, 9215.999, 9216.001, a['area'], a['area']][n % 8]
    twin = copy.deepcopy(anns[4])
    twin['id'] = next_id
    anns.append(twin)
    last = max(im['id'] for im in gt['images'])
    for extra in (1, 2, 3):                              # images without ground truth (two of them get detections)
        im = copy.deepcopy(gt['images'][0])
        im['id'] = last + extra
        gt['images'].append(im)
    boxes, kpts, cats, imgs, scores = [np.asarray(v) for v in gen.synth_detections(gt, seed)]
    boxes, kpts, cats, imgs, scores = list(boxes), list(kpts), list(cats), list(imgs), list(scores)
    silent = {gt['images'][1]['id'], gt['images'][2]['id'], last + 3}       # images without detections
    keep = [i for i in range(len(imgs)) if int(imgs[i]) not in silent]
    boxes, kpts, cats, imgs, scores = ([v[i] for i in keep] for v in (boxes, kpts, cats, imgs, scores))
    crowded = anns[0]                                    # one cell with 130 jittered copies of its ground truth
    x, y, w, h = crowded['bbox']
    g = np.asarray(crowded['keypoints'], dtype=np.float64)
    for _ in range(130):
        boxes.append(np.array([x, y, w, h]) + rng.normal(0, 0.08, 4) * np.array([w, h, w, h]))
        k = g.copy()
        k[0::3] += rng.normal(0, 0.02 * np.sqrt(crowded['area']), 294)
        k[1::3] += rng.normal(0, 0.02 * np.sqrt(crowded['area']), 294)
        kpts.append(k); cats.append(crowded['category_id']); imgs.append(crowded['image_id']); scores.append(rng.random())
    # detections whose own area sits on / beside the range borders (not inside a crowd region: intersection / own area would be
    # 1 give or take an ulp, within 1e-9 of the 1 - 1e-10 cap, and the GPU test wants every decision clear of its borders)
    for n, a in enumerate([a for a in anns if not a['iscrowd']][:16]):
        side = [32.0, 96.0][n % 2] + [0.0, 0.0, -0.001, 0.001][n % 4]
        boxes.append(np.array([a['bbox'][0], a['bbox'][1], side, side]))
        kpts.append(_square_landmarks(a['keypoints'], a['bbox'][0], a['bbox'][1], side))
        cats.append(a['category_id']); imgs.append(a['image_id']); scores.append(rng.random())
    for extra in (1, 2):
        for _ in range(3):
            boxes.append(np.array([10.0, 20.0, 50.0, 60.0]) + rng.random(4))
            kpts.append(np.round(rng.random(882) * 200, 4)); cats.append(int(rng.choice(cats[:20]))); imgs.append(last + extra)
            scores.append(rng.random())
    for i in range(0, len(boxes), 8):                    # the same detection twice
        boxes.append(boxes[i]); kpts.append(kpts[i]); cats.append(cats[i]); imgs.append(imgs[i]); scores.append(scores[i])
    scores = np.round(np.asarray(scores, dtype=np.float64), 2)
    b, k = gen.as_results(np.round(np.asarray(boxes), 4), np.round(np.asarray(kpts), 4), np.asarray(cats), np.asarray(imgs),
                          scores)
    return gt, dict(bbox=b, keypoints=k)


def replicated_case(copies, seed=5):
    """the demo set ``copies`` times under fresh image / annotation ids, detections drawn per copy"""
    base, gen = demo_gt(), generator()
    gt = dict(images=[], annotations=[], categories=base['categories'])
    b_all, k_all = [], []
    step_i = max(im['id'] for im in base['images']) + 1
    step_a = max(a['id'] for a in base['annotations']) + 1
    for c in range(copies):
        part = copy.deepcopy(base)
        for im in part['images']:
            im['id'] += c * step_i
        for a in part['annotations']:
            a['id'] += c * step_a
            a['image_id'] += c * step_i
        gt['images'] += part['images']
        gt['annotations'] += part['annotations']
        b, k = gen.as_results(*gen.synth_detections(part, seed=seed + c))
        b_all += b
        k_all += k
    return gt, dict(bbox=b_all, keypoints=k_all)


def host_evaluator(gt, results, typ):
    index = ev.CocoIndex(copy.deepcopy(gt))
    e = ev.CocoEvaluator(index, index.load_results(copy.deepcopy(results)), typ)
    e.params.img_ids = index.get_img_ids()
    e.evaluate().accumulate()
    e.summarize(verbose=False)
    return e


def packed_evaluator(gt, results, typ, device):
    pg = evd.pack_ground_truth(ev.CocoIndex(copy.deepcopy(gt)))
    e = evd.DeviceCocoEvaluator(pg, evd.pack_results(pg, copy.deepcopy(results)), typ, device=device, keep_similarity=True)
    e.evaluate().accumulate()
    e.summarize(verbose=False)
    return e


def assert_same_matching(got, want):
    """entry by entry against CocoEvaluator.eval_imgs, then the eval arrays and the stats: all EQUAL"""
    p = want.params
    K, A, I = len(p.cat_ids), len(p.area_rng), len(p.img_ids)
    assert list(got.params.img_ids) == list(p.img_ids) and list(got.params.cat_ids) == list(p.cat_ids)
    assert len(want.eval_imgs) == K * A * I
    n_entries = 0
    for k in range(K):
        for a in range(A):
            for i in range(I):
                w, g = want.eval_imgs[(k * A + a) * I + i], got.eval_imgs_of(k, a, i)
                assert (w is None) == (g is None), (k, a, i)
                if w is None:
                    continue
                n_entries += 1
                for key in ('d_match', 'd_scores', 'g_ignore', 'd_ignore'):
                    assert w[key].shape == g[key].shape and np.array_equal(w[key], g[key]), (key, k, a, i)
    assert n_entries > 0
    assert got.eval['counts'] == want.eval['counts']
    for key in ('precision', 'recall', 'scores'):
        assert np.array_equal(got.eval[key], want.eval[key]), key
    assert np.array_equal(got.stats, want.stats)


def similarities(got, want):
    """[(img_id, cat_id, packed evaluator's matrix, CocoEvaluator's matrix)] for every cell"""
    out = []
    for i in want.params.img_ids:
        for c in want.params.cat_ids:
            out.append((i, c, got.similarity(i, c), want._similarity(i, c)))
    return out
