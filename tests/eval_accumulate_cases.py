"""Inputs shared by tests/test_eval_accumulate_refs.py (numpy) and tests/test_gpu_eval_accumulate.py (HIP kernels): the cases
of tests/eval_cases.py in the form a detector returns them, float32 values at and beside the rounding ties of
``np.round(float64, 4)``, and small hand-made datasets for the edges of ``accumulate``."""
import re
import os

import numpy as np

from kgdet_amd import evaluation as ev
from tests import eval_cases as cases

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'kgdet_hip.h')


def header_constant(name):
    with open(HEADER) as f:
        return int(re.search(r'#define\s+%s\s+(\d+)' % name, f.read()).group(1))


class Dataset(object):
    def __init__(self, coco):
        self.coco, self.img_ids, self.cat_ids = coco, coco.get_img_ids(), coco.get_cat_ids()

    def __len__(self):
        return len(self.img_ids)


def detector_results(gt, results):
    """(dataset, results as ``single_gpu_test`` returns them) for a case of eval_cases: per image (boxes per class [n, 5] xyxy +
    score, scores per class, landmarks per class [n, 882]), float32; box and landmark results pair up by position"""
    index = ev.CocoIndex(gt)
    data = Dataset(index)
    img_pos = {i: n for n, i in enumerate(data.img_ids)}
    cat_pos = {c: n for n, c in enumerate(data.cat_ids)}
    n_cls = len(data.cat_ids)
    det = [[[] for _ in range(n_cls)] for _ in data.img_ids]
    kpt = [[[] for _ in range(n_cls)] for _ in data.img_ids]
    for b, k in zip(results['bbox'], results['keypoints']):
        if b['category_id'] not in cat_pos:
            continue
        i, c = img_pos[b['image_id']], cat_pos[b['category_id']]
        x, y, w, h = b['bbox']
        det[i][c].append([x, y, x + w - 1, y + h - 1, b['score']])
        kpt[i][c].append(k['keypoints'])
    out = []
    for i in range(len(data.img_ids)):
        d = [np.asarray(v, dtype=np.float32).reshape(-1, 5) for v in det[i]]
        out.append((d, [v[:, 4] for v in d], [np.asarray(v, dtype=np.float32).reshape(-1, 882) for v in kpt[i]]))
    return data, out


def case_inputs(case):
    if case == 'stress':
        return cases.stress_case()
    if case == 'replicated':
        return cases.replicated_case(8)
    return cases.golden_case(case)


def rounding_values():
    """float32 values where ``rint(v * 1e4)`` decides closely: k * 1e-4 and (k + 0.5) * 1e-4 rounded to float32 and moved by
    0, 1 and 2 ulps either way (the scaled fraction is at or beside 0 / one half), exact ties m / 32 with odd m
    (m / 32 * 1e4 = 312.5 m exactly), both signs, zeros"""
    rng = np.random.default_rng(17)
    # (below k = 2000 a float32 ulp is under 1.5e-4 of the scaled value: "beside" the tie; the large k are image coordinates)
    k = np.concatenate([np.arange(0, 2000), rng.integers(0, 6 * 10 ** 6, 1500)]).astype(np.float64)
    base = np.concatenate([k * 1e-4, (k + 0.5) * 1e-4]).astype(np.float32)
    out = [base]
    for _ in range(2):
        out.append(np.nextafter(out[-1], np.float32(np.inf)))
    out.append(np.nextafter(base, np.float32(-np.inf)))
    out.append(np.nextafter(out[-1], np.float32(-np.inf)))
    m = (2 * np.concatenate([np.arange(0, 200), rng.integers(0, 2 ** 14, 800)]) + 1).astype(np.float32)
    ties = m / np.float32(32)
    scaled = ties.astype(np.float64) * 1e4
    assert np.all(scaled - np.floor(scaled) == 0.5)
    v = np.concatenate(out + [ties, np.zeros(2, np.float32)])
    return np.concatenate([v, -v]).astype(np.float32)


def rounding_rows(K=294):
    """the values above as landmark rows [n, 3K] float32 (cut to whole rows)"""
    v = rounding_values()
    n = len(v) // (3 * K)
    return np.ascontiguousarray(v[:n * 3 * K].reshape(n, 3 * K))


def edge_dataset(n_images=6, seed=0, only_first=False):
    """(ground truth dict, bbox results) bent into the edges of accumulate.  Category 1: small / medium / large ground truths in
    every image, 15 detections in the first two images and 3 in the others (cells over and under max_dets = 10), scores on a
    grid of four values (ties across images and inside a cell).  Category 2: ground truth, no detection.  Category 3: small and
    medium ground truths only (n_gt == 0 for 'large' alone), every one of them detected exactly (recall reaches 1.0) plus a
    false positive.  Category 4: a ground truth and only detections of area 1e12, outside every range and unmatched: all
    ignored.  Category 5: five ground truths per image, one detected in the first image: recall stays at 1 / (5 n_images).
    ``only_first``: category 1 alone with 10 detections per image (the long sequence)."""
    rng = np.random.default_rng(seed)
    images = [dict(id=i + 1, width=640, height=480, file_name='%d.jpg' % i) for i in range(n_images)]
    anns, dets = [], []

    def gt(img, cat, box, crowd=0):
        anns.append(dict(id=len(anns) + 1, image_id=img, category_id=cat, bbox=[float(v) for v in box],
                         area=float(box[2] * box[3]), iscrowd=crowd))

    def det(img, cat, box, score):
        dets.append(dict(image_id=img, category_id=cat, bbox=[float(v) for v in box], score=float(score)))

    grid = [0.3, 0.5, 0.7, 0.9]
    for n, im in enumerate(images):
        i = im['id']
        mine = [(10, 10, 20, 20), (100, 10, 50, 50), (200, 10, 120, 120), (400, 10, 60, 40)]
        for b in mine:
            gt(i, 1, b)
        gt(i, 1, (300, 200, 200, 150), crowd=1)
        for j in range(10 if only_first else (15 if n < 2 else 3)):
            b = np.asarray(mine[j % 4], dtype=np.float64)
            jitter = rng.choice([0.0, 0.02, 0.1, 0.5]) * rng.normal(0, 1, 4) * b[[2, 3, 2, 3]]
            det(i, 1, np.round(np.concatenate([b[:2] + jitter[:2], np.maximum(b[2:] + jitter[2:], 1.0)]), 4), rng.choice(grid))
        if only_first:
            continue
        gt(i, 2, (50, 300, 40, 40))
        for b in [(10, 200, 25, 25), (60, 200, 70, 70)]:
            gt(i, 3, b)
            det(i, 3, b, rng.choice(grid))
        det(i, 3, (500, 400, 30, 30), 0.2)
        gt(i, 4, (10, 300, 30, 30))
        for j in range(3):
            det(i, 4, (0, 0, 1e6, 1e6 + j), rng.choice(grid))
        for j in range(5):
            gt(i, 5, (10 + 60 * j, 400, 40, 40))
        if n == 0:
            det(i, 5, (10, 400, 40, 40), 0.8)
            det(i, 5, (300, 100, 40, 40), 0.9)
    cats = [dict(id=c, name='c%d' % c) for c in ([1] if only_first else [1, 2, 3, 4, 5])]
    return dict(images=images, annotations=anns, categories=cats), dets
