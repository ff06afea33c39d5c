"""Inputs shared by tests/test_eval_pack_refs.py (numpy) and tests/test_gpu_eval_pack.py (HIP kernels): ground truth sets plus
the detections of a test run as ``runner.DeviceResults.rows`` holds them -- float32 [N, M, 7 + 3K]: box, score, label, count,
landmarks -- with the list ``single_gpu_test`` would have returned for the same detections.  Seeds are fixed.

Every case: image ids out of ascending order; four labels of which the second maps to a category the ground truth does not
know (it lies between known ones and must still count in the ids); NaN in every row at or beyond an image's count."""
from fractions import Fraction

import numpy as np

from kgdet_amd import evaluation as ev
from tests import eval_accumulate_cases as acc

IMG_IDS = [30, 10, 20, 50, 40, 70, 60]          # dataset order
GT_CATS = [2, 5, 9]
LABEL_CATS = [2, 7, 5, 9]                       # label -> category id; 7 is unknown to the ground truth
NAMES = ['mixed', 'cuts', 'ties', 'single', 'empty', 'rounding']


class Dataset(object):
    """what the packing reads of a dataset: the ground truth index, the samples' image ids, the labels' category ids"""

    def __init__(self, coco, img_ids, cat_ids):
        self.coco, self.img_ids, self.cat_ids = coco, list(img_ids), list(cat_ids)

    def __len__(self):
        return len(self.img_ids)


class Case(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def ground_truth(img_ids, seed, K=294):
    """two or three annotations per image with all K landmarks labelled, categories of GT_CATS"""
    rng = np.random.default_rng(seed)
    images = [dict(id=int(i), width=640, height=480, file_name='%d.jpg' % i) for i in img_ids]
    anns = []
    for i in img_ids:
        for _ in range(int(rng.integers(2, 4))):
            x, y, w, h = rng.uniform(0, 300), rng.uniform(0, 200), rng.uniform(40, 300), rng.uniform(40, 250)
            kp = np.stack([rng.uniform(x, x + w, K), rng.uniform(y, y + h, K), np.full(K, 2.0)], axis=1)
            anns.append(dict(id=len(anns) + 1, image_id=int(i), category_id=int(rng.choice(GT_CATS)),
                             bbox=[float(np.round(v, 2)) for v in (x, y, w, h)], area=float(np.round(w * h * 0.6, 2)), iscrowd=0,
                             keypoints=[float(v) for v in np.round(kp, 2).reshape(-1)], num_keypoints=K))
    return dict(images=images, annotations=anns, categories=[dict(id=c, name='c%d' % c) for c in GT_CATS])


def as_rows(dets, M, K):
    """per image (det [n, 5], labels [n], kpts [n, 3K]) -> rows float32 [N, M, 7 + 3K], NaN wherever nothing is to be read"""
    rows = np.full((len(dets), M, 7 + 3 * K), np.nan, np.float32)
    for n, (det, labels, kpts) in enumerate(dets):
        c = len(det)
        assert c <= M
        rows[n, :c, :5], rows[n, :c, 5], rows[n, :c, 7:] = det, labels, kpts
        rows[n, :max(c, 1), 6] = c
    return rows


def as_list(dets, n_labels):
    """the same detections as ``single_gpu_test`` returns them: per image (boxes per class, scores, landmarks per class), or a
    1-tuple of empty box arrays for an image without detections"""
    out = []
    for det, labels, kpts in dets:
        if len(det) == 0:
            out.append(([np.zeros((0, 5), np.float32) for _ in range(n_labels)],))
            continue
        out.append(([det[labels == l] for l in range(n_labels)], det[:, 4], [kpts[labels == l] for l in range(n_labels)]))
    return out


def _boxes(rng, n):
    x1, y1 = rng.uniform(0, 400, n), rng.uniform(0, 300, n)
    return np.stack([x1, y1, x1 + rng.uniform(5, 200, n), y1 + rng.uniform(5, 150, n)], axis=1)


def _random_dets(rng, n, K, labels=None, scores=None):
    det = np.concatenate([_boxes(rng, n), (rng.random((n, 1)) if scores is None else np.asarray(scores).reshape(n, 1))],
                         axis=1).astype(np.float32)
    labels = rng.integers(0, len(LABEL_CATS), n) if labels is None else np.asarray(labels)
    kpts = rng.uniform(0, 600, (n, 3 * K)).astype(np.float32)
    return det, labels.astype(np.int64), kpts


def _mixed(rng, gt, img_ids, M, K):
    """jittered ground truths (right and wrong labels) and false positives; one image at the full M rows, one empty"""
    by_img = {}
    for a in gt['annotations']:
        by_img.setdefault(a['image_id'], []).append(a)
    dets = []
    for n, i in enumerate(img_ids):
        c = [17, M, 5, 0, 40, 1, 63][n % 7]
        det, labels, kpts = _random_dets(rng, c, K)
        for r in range(min(c, 12)):
            a = by_img[i][r % len(by_img[i])]
            x, y, w, h = a['bbox']
            jit = rng.normal(0, 0.05, 4) * [w, h, w, h]
            det[r, :4] = [x + jit[0], y + jit[1], x + w - 1 + jit[2], y + h - 1 + jit[3]]
            kp = np.asarray(a['keypoints'], np.float64).reshape(K, 3)
            kp[:, :2] += rng.normal(0, 2.0, (K, 2))
            kpts[r] = kp.reshape(-1)
            if rng.random() < 0.8:
                labels[r] = LABEL_CATS.index(a['category_id'])
        det[:, 4] = np.round(det[:, 4], 2) if n % 2 else det[:, 4]      # (a coarse grid on every other image: equal scores)
        dets.append((det, labels, kpts))
    return dets


def _cuts(rng, K):
    """image 0: one cell of 130 rows (over both cuts); image 1: cells of exactly 100 and exactly 20 rows, 10 rows of the
    unknown label between them in row order"""
    a = _random_dets(rng, 130, K, labels=np.full(130, 2), scores=np.round(rng.random(130), 3))
    lab = np.concatenate([np.full(100, 0), np.full(10, 1), np.full(20, 3)])
    b = _random_dets(rng, 130, K, labels=lab[rng.permutation(130)])
    return [a, b]


def _ties(rng, K):
    """image 0: raw scores ASCENDING in row order that round to one 4-digit value -- the tie goes to the row order (k), where the
    raw scores would have it reversed.  Image 1: rows 0 and 2 share a label and a rounded score, the raw order of the pair is
    the reverse of its packed order; the row between them belongs to another cell."""
    a = _random_dets(rng, 3, K, labels=[2, 2, 2], scores=np.array([0.50001, 0.50002, 0.50003], np.float32))
    b = _random_dets(rng, 3, K, labels=[0, 3, 0], scores=np.array([0.12341, 0.9, 0.12344], np.float32))
    return [a, b]


def rounding_specials():
    """exact decimal ties with a representable half and their negatives, signed zeros, the float32 neighbours of
    (k + 0.5) / 1e4"""
    ties = np.array([0.03125, 0.09375, 0.15625, 0.28125, 2.5 / 1e1, 0.5, 1.5, 2.5, 1024.03125], np.float32)
    k = np.arange(0, 400, dtype=np.float64)
    half = ((k + 0.5) / 1e4).astype(np.float32)
    near = np.concatenate([half, np.nextafter(half, np.float32(1)), np.nextafter(half, np.float32(-1))])
    v = np.concatenate([ties, near, np.zeros(1, np.float32)])
    return np.concatenate([v, -v]).astype(np.float32)


def rounding_pool():
    """float32 values for the rounding: ``rounding_values()`` of eval_accumulate_cases and the specials above"""
    return np.concatenate([rounding_specials(), acc.rounding_values()]).astype(np.float32)


def rounding_inputs(d):
    """the rounding pool plus 200 000 seeded random values inside the rounding's domain |v| * 10**d < 2**40"""
    from kgdet_amd import evaluation_device as evd
    rng = np.random.default_rng(2024)
    lim = min(2000.0, 0.9 * evd.ROUND_LIMIT / 10.0 ** d)
    pool = rounding_pool().astype(np.float64)
    coords = rng.uniform(-lim, lim, 60000).astype(np.float32).astype(np.float64)
    scores = rng.random(60000).astype(np.float32).astype(np.float64)
    a = rng.uniform(0, min(1e5, lim - 1), 40000).astype(np.float32).astype(np.float64)
    b = rng.uniform(0, 2 ** -10, 40000).astype(np.float32).astype(np.float64)
    doubles = rng.uniform(-lim, lim, 40000)                           # (full 53-bit values: the residual is a real product)
    return np.concatenate([pool, coords, scores, a - b + 1, doubles])


def _rounding(rng, K, N, M):
    """x1, y1 and the score of every row come from the rounding pool (the specials first, the rest sampled); x2 - x1 + 1 and
    y2 - y1 + 1 are differences of a large and a tiny float32 whose float64 subtraction has to round"""
    pool, special = rounding_pool(), rounding_specials()
    need = 3 * N * M
    rest = pool[len(special):]
    v = np.concatenate([special, rest[rng.choice(len(rest), need - len(special), replace=False)]])
    v = v[rng.permutation(need)].reshape(N, M, 3)
    dets = []
    for n in range(N):
        det, labels, kpts = _random_dets(rng, M, K)
        det[:, 0], det[:, 1], det[:, 4] = v[n, :, 0], v[n, :, 1], v[n, :, 2]
        det[:, 2] = rng.uniform(1e4, 1e5, M).astype(np.float32)
        det[:, 3] = rng.uniform(1e3, 1e4, M).astype(np.float32)
        tiny = (rng.uniform(1, 2, M) * 2.0 ** -20).astype(np.float32)
        det[::3, 0] = tiny[::3]                                     # (24 bits from 2^-20 down against 24 bits from 2^16 down)
        inexact = [Fraction(float(b)) - Fraction(float(a)) != Fraction(float(b) - float(a)) for a, b in det[:30:3, [0, 2]]]
        assert sum(inexact) >= 5                                    # (the float64 difference is not the exact one)
        dets.append((det, labels, kpts))
    return dets


_cache = {}


def case(name):
    """-> Case(name, gt dict, dataset, rows [N, M, 7 + 3K] float32, results list, K, M, n_labels); built once, leave unchanged"""
    if name in _cache:
        return _cache[name]
    seed = NAMES.index(name)
    rng = np.random.default_rng(100 + seed)
    N, M, K = dict(mixed=(7, 100, 294), cuts=(2, 130, 1), ties=(2, 3, 1), single=(1, 1, 294), empty=(3, 3, 1),
                   rounding=(40, 130, 1))[name]
    img_ids = (IMG_IDS * ((N + 6) // 7))[:N] if N <= 7 else [1000 - 3 * n if n % 2 else 3 * n + 1 for n in range(N)]
    gt = ground_truth(img_ids, seed)
    if name == 'mixed':
        dets = _mixed(rng, gt, img_ids, M, K)
    elif name == 'cuts':
        dets = _cuts(rng, K)
    elif name == 'ties':
        dets = _ties(rng, K)
    elif name == 'single':
        dets = [_random_dets(rng, 1, K, labels=[3])]
    elif name == 'empty':
        dets = [_random_dets(rng, 0, K) for _ in range(N)]
    else:
        dets = _rounding(rng, K, N, M)
    index = ev.CocoIndex(gt)
    _cache[name] = Case(name=name, gt=gt, dataset=Dataset(index, img_ids, LABEL_CATS), rows=as_rows(dets, M, K),
                        results=as_list(dets, len(LABEL_CATS)), K=K, M=M, n_labels=len(LABEL_CATS))
    return _cache[name]


def packed_gt(c):
    """the case's packed ground truth, telling the packing the case's landmark count"""
    from kgdet_amd import evaluation_device as evd
    pg = evd.pack_ground_truth(c.dataset.coco)
    pg.num_landmarks_gt, pg.num_landmarks = pg.num_landmarks, c.K
    return pg
