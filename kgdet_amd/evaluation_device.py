"""The bbox / landmark (OKS) evaluator on packed arrays, with its two hot steps on the GPU.

``evaluation.CocoEvaluator`` restates pycocotools: dictionaries per annotation, a Python loop per ground truth for the
similarities and four nested Python loops for the matching.  This module keeps its semantics -- it is held to
``CocoEvaluator`` value for value by tests/test_eval_packed.py and tests/test_gpu_eval.py -- on a layout a kernel can walk:

* ``pack_ground_truth(coco)``: once per dataset.  Annotations sorted (stably) by cell = (image index, category index) in
  the sorted id order ``CocoEvaluator`` uses, one float64 / integer array per field, a CSR table ``start`` over all cells.
* ``pack_results`` (the list-of-dicts form ``CocoIndex.load_results`` takes) / ``pack_test_results`` (what
  ``single_gpu_test`` returns, no files: ``kpt2json``'s rounding applied to the arrays): detections sorted by cell, inside a
  cell by descending score (stable), cut to the type's ``max_dets[-1]``.
* ``DeviceCocoEvaluator``: ``evaluate()`` runs similarity + matching for every cell in one launch each
  (csrc/coco_eval.hip) or, with ``device='cpu'``, their numpy restatement below; ``accumulate()`` is one more launch over
  the outputs where they lie on the device (csrc/coco_accumulate.hip) or ``accumulate_restatement()``, numpy over the packed
  outputs, vectorised per (category, area range, max_dets); ``summarize()`` is ``CocoEvaluator``'s.
* ``pack_test_results(..., lazy_landmarks=True)``: the landmark rows stay float32 on the host and are rounded, with their
  extents, by ``kgdet_coco_pack_landmarks`` chunk by chunk (``materialize`` is the numpy route).
* ``pack_device_results``: the packing of a ``runner.DeviceResults`` -- detections that never left the device -- by
  ``kgdet_coco_order_dets`` / ``kgdet_coco_scatter_dets`` (csrc/coco_pack_dets.hip): order, exact decimal rounding, cut and
  the landmark gather as kernels, ``kxy32`` a device tensor; ``pack_rows_restatement`` is their numpy restatement.
* ``write_device_results_json`` / ``results2json_any``: ``results2json`` for a ``runner.DeviceResults`` -- the two result files,
  byte for byte, formatted by ``kgdet_coco_json_measure`` / ``kgdet_coco_json_write`` (csrc/coco_json.hip) from the rows where
  they lie; ``json_restatement`` is their numpy restatement.
* What those two routes and their restatements share is written once: ``_row_block`` (what a rows block is, with every check
  of it and of ``num_digits``), ``_image_rows`` (the restatements' walk over an image), ``_order_rows_on_device`` (the order
  kernel's launch) with ``_refuse_flags``, and ``_round_half_even``, the one rounding rule (``round_like_python`` adds ``round``).

What the device computes differently from numpy is stated in DESIGN.md: box IoU is bit-identical; for OKS the exponent
argument is bit-identical, ``exp`` and the order of the sum over the landmarks are the device's.
"""
import ctypes
import functools
import json
import os

import numpy as np

from .evaluation import CocoEvaluator, CocoIndex, EvalParams, landmark_meta

MAX_DETS = dict(bbox=100, keypoints=20)       # EvalParams.max_dets[-1] per type
# detections per launch: bounds the device (and pinned staging) memory of one chunk -- a landmark detection is 4.7 kB
CHUNK_DETS = dict(bbox=1 << 22, keypoints=1 << 18)


class Packed(object):
    """a bag of arrays (attributes)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _index_of(sorted_ids, ids):
    """(position of every id in sorted_ids, whether it is there)"""
    ids = np.asarray(ids)
    if len(sorted_ids) == 0:
        return np.zeros(len(ids), np.int64), np.zeros(len(ids), bool)
    pos = np.minimum(np.searchsorted(sorted_ids, ids), len(sorted_ids) - 1)
    return pos.astype(np.int64), sorted_ids[pos] == ids


def _csr(cell_sorted, n_cells):
    return np.searchsorted(cell_sorted, np.arange(n_cells + 1)).astype(np.int64)


def pack_ground_truth(coco):
    """Annotations of a ``CocoIndex`` (or an annotation file / dict) as arrays, in cell order.  Built once per dataset.
    An annotation id of 0 is refused (``ValueError``): ``CocoEvaluator``, like pycocotools, stores the matched ground truth's id
    and reads 0 as "unmatched", so a match to such an annotation counts as a miss there; the packed path tells matched from
    unmatched by index and does not reproduce that -- renumber the annotations, or use ``CocoEvaluator``."""
    if not isinstance(coco, CocoIndex):
        coco = CocoIndex(coco)
    K = len(landmark_meta()['oks_sigmas'])
    img_ids = np.unique(np.asarray(coco.get_img_ids(), dtype=np.int64))
    cat_ids = np.unique(np.asarray(coco.get_cat_ids(), dtype=np.int64))
    anns = list(coco.dataset.get('annotations', ()))
    ii, ok_i = _index_of(img_ids, np.asarray([a['image_id'] for a in anns], dtype=np.int64))
    ci, ok_c = _index_of(cat_ids, np.asarray([a['category_id'] for a in anns], dtype=np.int64))
    keep = np.nonzero(ok_i & ok_c)[0]           # (what get_ann_ids(img_ids, cat_ids) selects)
    cell = ii[keep] * len(cat_ids) + ci[keep]
    order = keep[np.argsort(cell, kind='mergesort')]
    anns = [anns[i] for i in order]
    n = len(anns)
    if any(a['id'] == 0 for a in anns):
        raise ValueError('annotation id 0 reads as "unmatched" in CocoEvaluator; the packed evaluator refuses it')
    kpt = np.zeros((n, K * 3), np.float64)
    for r, a in enumerate(anns):
        if a.get('keypoints'):
            kpt[r] = a['keypoints']
    n_vis = np.count_nonzero(kpt[:, 2::3] > 0, axis=1).astype(np.int32)
    cell = ii[order] * len(cat_ids) + ci[order]
    return Packed(
        img_ids=img_ids, cat_ids=cat_ids, num_landmarks=K, img_idx=ii[order], cat_idx=ci[order], cell=cell,
        start=_csr(cell, len(img_ids) * len(cat_ids)),
        bbox=np.asarray([a['bbox'] for a in anns], dtype=np.float64).reshape(n, 4),
        area=np.asarray([a['area'] for a in anns], dtype=np.float64),
        iscrowd=np.asarray([int(a.get('iscrowd', 0)) for a in anns], dtype=np.int32),
        num_keypoints=np.asarray([a['num_keypoints'] if 'num_keypoints' in a else v for a, v in zip(anns, n_vis)],
                                 dtype=np.int64),
        id=np.asarray([a['id'] for a in anns], dtype=np.int64), keypoints=kpt, num_visible=n_vis)


def _order_dets(pg, kind, image_id, category_id, score):
    """(source rows kept, in packed order; image index; category index) -- by cell, inside a cell by descending score with the
    input order for equal scores, cut to the type's max_dets[-1]; a category the ground truth does not know is never loaded"""
    image_id = np.asarray(image_id, dtype=np.int64)
    ii, ok_i = _index_of(pg.img_ids, image_id)
    if not ok_i.all():
        raise ValueError('Results do not correspond to current coco set')
    ci, ok_c = _index_of(pg.cat_ids, np.asarray(category_id, dtype=np.int64))
    cell = np.where(ok_c, ii * len(pg.cat_ids) + ci, -1)
    order = np.lexsort((-score, cell))                             # stable
    order = order[cell[order] >= 0]
    first = _csr(cell[order], len(pg.img_ids) * len(pg.cat_ids))
    rank = np.arange(len(order)) - first[cell[order]]
    return order[rank < MAX_DETS[kind]], ii, ci


def _pack_dets(pg, kind, image_id, category_id, score, bbox, area, kxy, order=None):
    """``kxy``: [n, K, 2] in input order, or already in packed order when ``order`` (from ``_order_dets``) is passed"""
    score = np.asarray(score, dtype=np.float64)
    if order is None:
        order, ii, ci = _order_dets(pg, kind, image_id, category_id, score)
        if kxy is not None:
            kxy = np.ascontiguousarray(kxy[order])
    else:
        order, ii, ci = order
    cell = ii[order] * len(pg.cat_ids) + ci[order]
    if bbox is not None:                                            # (None: a lazy landmark Packed, see pack_test_results)
        bbox, area = np.ascontiguousarray(bbox[order]), area[order]
    return Packed(kind=kind, cell=cell, start=_csr(cell, len(pg.img_ids) * len(pg.cat_ids)), img_idx=ii[order],
                  cat_idx=ci[order], score=score[order], bbox=bbox, area=area,
                  id=order.astype(np.int64) + 1, kxy=kxy)          # load_results: id = k + 1


def _result_kind(first):
    if 'bbox' in first and first['bbox'] != []:
        return 'bbox'
    if 'keypoints' in first:
        return 'keypoints'
    raise ValueError('only bbox and keypoints results are supported')


def _derive_from_landmarks(kpt):
    """load_results for a landmark result: bbox / area from the extent of ALL coordinates.  kpt [n, 3K] -> bbox, area, kxy"""
    n = len(kpt)
    xy = kpt.reshape(n, -1, 3)[:, :, :2]
    if n == 0:
        return np.zeros((0, 4)), np.zeros(0), np.ascontiguousarray(xy)
    x0, x1, y0, y1 = xy[:, :, 0].min(1), xy[:, :, 0].max(1), xy[:, :, 1].min(1), xy[:, :, 1].max(1)
    return np.stack([x0, y0, x1 - x0, y1 - y0], axis=1), (x1 - x0) * (y1 - y0), np.ascontiguousarray(xy)


def pack_results(packed_gt, results):
    """Detections in the form ``CocoIndex.load_results`` takes (a list of dicts, or a json file of them) -> packed arrays.
    The type is the first result's, as there: 'bbox' results get ``area = w * h``, landmark results ``bbox`` / ``area`` from
    the extent of all 294 coordinates; ids are ``k + 1``.  The dicts are not modified."""
    if isinstance(results, (str, bytes, os.PathLike)):
        with open(results) as f:
            results = json.load(f)
    if not isinstance(results, list):
        raise TypeError('results must be a list of objects')
    K = packed_gt.num_landmarks
    img = [r['image_id'] for r in results]
    _, known = _index_of(packed_gt.img_ids, np.asarray(img, dtype=np.int64))
    if not known.all():
        raise ValueError('Results do not correspond to current coco set')
    if not results:
        return _pack_dets(packed_gt, 'bbox', [], [], [], np.zeros((0, 4)), np.zeros(0), None)
    kind = _result_kind(results[0])
    cat = [r['category_id'] for r in results]
    score = [r['score'] for r in results]
    if kind == 'bbox':
        bbox = np.asarray([r['bbox'] for r in results], dtype=np.float64).reshape(len(results), 4)
        return _pack_dets(packed_gt, kind, img, cat, score, bbox, bbox[:, 2] * bbox[:, 3], None)
    kpt = np.asarray([r['keypoints'] for r in results], dtype=np.float64).reshape(len(results), K * 3)
    bbox, area, kxy = _derive_from_landmarks(kpt)
    return _pack_dets(packed_gt, kind, img, cat, score, bbox, area, kxy)


ROUND_LIMIT = 2.0 ** 40          # |v * 10**d| the exact rounding holds below (here and in csrc/coco_pack_dets.hip)


def _round_half_even_masked(values, num_digits, block=1 << 15):
    """(rounded float64 array, bool array: the values outside the rounding's domain -- those are returned as they are)"""
    v = np.asarray(values, dtype=np.float64)
    S = np.float64(10.0 ** num_digits)                              # (exact up to 10**22)

    def split(x):                                                   # Veltkamp: x = hi + lo, 26 bits each
        t = 134217729.0 * x
        hi = t - (t - x)
        return hi, x - hi

    sh, sl = split(S)
    flat = v.reshape(-1)
    out, bad = np.empty(flat.shape), np.empty(flat.shape, bool)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(0, len(flat), block):                        # (blocks whose two dozen temporaries stay in the cache)
            x = flat[i:i + block]
            a = np.abs(x)
            p = a * S
            bad[i:i + block] = ~(p < ROUND_LIMIT)                   # (a NaN is "bad" too)
            ah, al = split(a)
            e = ((ah * sh - p) + ah * sl + al * sh) + al * sl       # Dekker: a * S - p exactly (what fma(a, S, -p) returns)
            f = np.floor(p)
            r = p - f
            odd = np.floor(f * 0.5) * 2.0 != f                      # (exact for an integer f; np.fmod takes 100 ns per element)
            up = (r > 0.5) | ((r == 0.5) & ((e > 0) | ((e == 0) & odd)))
            out[i:i + block] = np.where(bad[i:i + block], x, np.copysign((f + up) / S, x))
    return out.reshape(v.shape), bad.reshape(v.shape)


def _round_half_even(values, num_digits):
    """(rounded float64 array, number of values outside the rounding's domain -- those are returned as they are)"""
    out, bad = _round_half_even_masked(values, num_digits)
    return out, int(np.count_nonzero(bad))


def round_half_even_restatement(values, num_digits):
    """``kgdet_coco_order_dets``'s rounding in numpy: bit-equal to ``[round(float(v), num_digits) for v in values]`` for
    ``1 <= num_digits <= 9`` and finite ``|v * 10**d| < 2**40`` (other values come back unchanged; the packing counts them and
    raises).  With S = 10**d: p = fl(|v| * S) and the exact residual e = |v| * S - p -- an FMA on the device, a Veltkamp /
    Dekker product here -- place the exact decimal value against the half: n = floor(p) + 1 where p - floor(p) > 1/2, or
    == 1/2 with e > 0, or e == 0 and floor(p) odd; else floor(p).  The result is copysign(n / S, v), one correctly rounded
    division: the double nearest to the decimal Python's ``round`` arrives at, with its sign of zero."""
    return _round_half_even(values, num_digits)[0]


def round_like_python(values, num_digits):
    """``[round(float(v), num_digits) for v in values]`` as an array: ``round_half_even_restatement`` where that is exact
    (``1 <= num_digits <= 9``, finite ``|v * 10**d| < 2**40``); the elements outside that domain, and every element for any
    other ``num_digits``, take Python's ``round`` one by one."""
    v = np.asarray(values, dtype=np.float64)
    if 1 <= num_digits <= 9:
        out, rest = _round_half_even_masked(v, num_digits)
    else:
        out, rest = v.copy(), np.ones(v.shape, bool)
    flat, src = out.reshape(-1), v.reshape(-1)
    for i in np.nonzero(rest.reshape(-1))[0]:
        flat[i] = round(float(src[i]), num_digits)
    return flat.reshape(v.shape)


def _landmarks_in_order(blocks, n, order, K, num_digits, batch=4096):
    """kpt2json + load_results for the landmark rows of ``blocks`` (arrays [m, 3K] in result order, n rows together):
    ``np.round(float64, num_digits)``, bbox / area from the extent of all coordinates (for every row, in input order), and the
    x, y of the rows ``order`` keeps written straight into their packed place -- in batches of rows on a few threads (numpy
    drops the interpreter lock), so the float64 copy of all 882 values per row never exists at once."""
    from concurrent.futures import ThreadPoolExecutor
    pos = np.full(n, -1, np.int64)
    pos[order] = np.arange(len(order))
    bbox, area, kxy = np.zeros((n, 4)), np.zeros(n), np.zeros((len(order), K, 2))

    def work(job):
        r0, parts = job
        a = np.concatenate(parts).astype(np.float64) if len(parts) > 1 else parts[0].astype(np.float64)
        np.round(a, num_digits, out=a)
        v = a.reshape(len(a), K, 3)
        x0, x1, y0, y1 = v[:, :, 0].min(1), v[:, :, 0].max(1), v[:, :, 1].min(1), v[:, :, 1].max(1)
        bbox[r0:r0 + len(a)] = np.stack([x0, y0, x1 - x0, y1 - y0], axis=1)
        area[r0:r0 + len(a)] = (x1 - x0) * (y1 - y0)
        to = pos[r0:r0 + len(a)]
        keep = to >= 0
        kxy[to[keep]] = v[keep, :, :2]

    def jobs():
        r0, rows, parts = 0, 0, []
        for blk in blocks:
            parts.append(blk)
            rows += len(blk)
            if rows >= batch:
                yield r0, parts
                r0, rows, parts = r0 + rows, 0, []
        if parts:
            yield r0, parts

    workers = max(1, min(16, int(os.environ.get('OMP_NUM_THREADS') or 4)))
    with ThreadPoolExecutor(workers) as pool:
        pending = []
        for job in jobs():                       # (a bounded queue: the batches' float64 copies are the memory in flight)
            pending.append(pool.submit(work, job))
            if len(pending) >= 2 * workers:
                pending.pop(0).result()
        for f in pending:
            f.result()
    return bbox, area, kxy


def _landmark_rows_in_order(blocks, n, order, K):
    """the float32 landmark rows ``order`` keeps, copied straight into their packed place [len(order), 3K]: a gather, no
    arithmetic and no float64 copy"""
    pos = np.full(n, -1, np.int64)
    pos[order] = np.arange(len(order))
    out = np.zeros((len(order), 3 * K), np.float32)
    r0 = 0
    for blk in blocks:
        if blk.dtype != np.float32:
            raise TypeError('lazy_landmarks takes float32 landmark rows (what single_gpu_test returns), not %s' % blk.dtype)
        to = pos[r0:r0 + len(blk)]
        keep = to >= 0
        out[to[keep]] = blk[keep]
        r0 += len(blk)
    return out


def round_landmarks_restatement(values, num_digits):
    """``kgdet_coco_pack_landmarks``'s rounding of float32 values: widen, ``rint(v * 10**d) / 10**d`` (ties to even, two
    float64 operations).  Held to ``np.round(float64, d)`` bit for bit by tests/test_eval_accumulate_refs.py."""
    v = np.asarray(values, dtype=np.float32).astype(np.float64)
    scale = np.float64(10.0 ** num_digits)
    return np.rint(v * scale) / scale


def materialize(packed, num_digits=None):
    """Fill ``kxy``, ``bbox`` and ``area`` of a lazy landmark Packed (``pack_test_results(..., lazy_landmarks=True)``) on the
    host, by the numpy route of the eager packing: ``np.round(float64, num_digits)`` of the float32 rows, extents over all
    coordinates.  A Packed that already holds them is returned as it is.  -> packed"""
    if getattr(packed, 'kxy32', None) is None or (packed.kxy is not None and packed.bbox is not None):
        return packed
    if not isinstance(packed.kxy32, np.ndarray):                    # (a device tensor: pack_device_results)
        packed.kxy32 = packed.kxy32.cpu().numpy()
    a = np.round(packed.kxy32.astype(np.float64), packed.num_digits if num_digits is None else num_digits)
    packed.bbox, packed.area, packed.kxy = _derive_from_landmarks(a)
    return packed


def pack_test_results(packed_gt, dataset, results, num_digits=4, lazy_landmarks=False):
    """{'bbox': packed[, 'keypoints': packed]} straight from what ``single_gpu_test`` / ``multi_gpu_test`` return, with the very
    numbers ``results2json`` + ``json.dump`` + ``load_results`` yield (a float's json text reads back as the same float):
    ``det2json`` for per-class box lists (no rounding), ``kpt2json`` for (boxes, scores, landmarks) tuples --
    ``np.round(float64, num_digits)`` for the landmarks, Python's ``round`` for xywh and the score (``round_like_python``).
    ``lazy_landmarks``: the 'keypoints' Packed carries ``kxy32`` -- the float32 rows [n, 3K] in packed order -- and
    ``num_digits`` instead of ``kxy`` / ``bbox`` / ``area`` (None): ``DeviceCocoEvaluator.evaluate`` rounds them and takes the
    extents on the GPU (``kgdet_coco_pack_landmarks``) and stores ``bbox`` / ``area``; ``materialize`` does it on the host."""
    if not isinstance(results[0], (list, tuple)):
        raise TypeError('invalid type of results')
    with_kpt = isinstance(results[0], tuple)
    K = packed_gt.num_landmarks
    rows, kpts, img, cat = [], [], [], []
    for idx in range(len(dataset)):
        res = results[idx]
        if with_kpt:
            if len(res) != 3:
                continue
            det, kpt = res[0], res[2]
        else:
            det, kpt = res, None
        for label in range(len(det)):
            boxes = np.asarray(det[label]).reshape(-1, 5)
            if kpt is not None:
                pts = np.asarray(kpt[label]).reshape(len(kpt[label]), K * 3)
                if len(pts) != len(boxes):
                    raise ValueError('image %d, class %d: %d boxes but %d landmark rows' % (idx, label, len(boxes), len(pts)))
                if len(pts):
                    kpts.append(pts)
            if len(boxes):
                rows.append(boxes.astype(np.float64))
                img.append(np.full(len(boxes), dataset.img_ids[idx], dtype=np.int64))
                cat.append(np.full(len(boxes), dataset.cat_ids[label], dtype=np.int64))
    rows = np.concatenate(rows) if rows else np.zeros((0, 5))
    img = np.concatenate(img) if img else np.zeros(0, np.int64)
    cat = np.concatenate(cat) if cat else np.zeros(0, np.int64)
    xywh = np.stack([rows[:, 0], rows[:, 1], rows[:, 2] - rows[:, 0] + 1, rows[:, 3] - rows[:, 1] + 1], axis=1)
    score = rows[:, 4]
    if with_kpt:
        xywh, score = round_like_python(xywh, num_digits), round_like_python(score, num_digits)
    out = dict(bbox=_pack_dets(packed_gt, 'bbox', img, cat, score, xywh, xywh[:, 2] * xywh[:, 3], None))
    if with_kpt:
        order = _order_dets(packed_gt, 'keypoints', img, cat, score)
        if lazy_landmarks:
            out['keypoints'] = _pack_dets(packed_gt, 'keypoints', img, cat, score, None, None, None, order=order)
            out['keypoints'].kxy32 = _landmark_rows_in_order(kpts, len(rows), order[0], K)
            out['keypoints'].num_digits = num_digits
            return out
        bbox, area, kxy = _landmarks_in_order(kpts, len(rows), order[0], K, num_digits)
        out['keypoints'] = _pack_dets(packed_gt, 'keypoints', img, cat, score, bbox, area, kxy, order=order)
    return out


# ------------------------------------------------------------------------------------------------
# pack_test_results for results that stayed on the device (runner.DeviceResults; csrc/coco_pack_dets.hip)
# ------------------------------------------------------------------------------------------------
def _row_block(rows, dataset, num_labels, num_digits, max_digits):
    """THE description of a ``runner.DeviceResults.rows`` block (numpy or tensor) -> N, M, W, K, L: float32 [N, M, W = 7 + 3K]
    -- box, score, label, count, K landmarks -- for a dataset of N samples; image n's count sits in ``rows[n, 0, 6]``, a row is
    valid when its label lies in [0, L), and L (``num_labels``; None: the dataset's categories) is 1 .. what the dataset names
    and the order kernel takes.  ``num_digits`` is an int in 1 .. ``max_digits``, the route's ceiling: 9 for the packing (the
    exact rounding's), ``JSON_MAX_DIGITS`` for the files.  Anything else is a ``ValueError``."""
    from . import _lib
    if isinstance(num_digits, bool) or not isinstance(num_digits, (int, np.integer)) or not 1 <= num_digits <= max_digits:
        raise ValueError('num_digits %r (1 .. %d)' % (num_digits, max_digits))
    N, M, W = rows.shape
    K = (W - 7) // 3
    if W != 7 + 3 * K or K < 1:
        raise ValueError('rows of %d floats (7 + 3K)' % W)
    if N != len(dataset):
        raise ValueError('%d result blocks for a dataset of %d samples' % (N, len(dataset)))
    L = len(dataset.cat_ids) if num_labels is None else int(num_labels)
    if not 1 <= L <= min(len(dataset.cat_ids), _lib.COCO_ORDER_MAX_LABELS):
        raise ValueError('%d labels: the dataset names %d categories, the kernels take up to %d'
                         % (L, len(dataset.cat_ids), _lib.COCO_ORDER_MAX_LABELS))
    return N, M, W, K, L


def _rows_and_labels(dev_results, device):
    """(a ``runner.DeviceResults``' rows, on ``device`` when one other than 'cpu' is named; its label count L)"""
    if dev_results.rows is None:
        raise ValueError('the device results were released')
    move = device is not None and str(device) != 'cpu'
    return (dev_results.rows.to(device) if move else dev_results.rows), int(dev_results.num_classes) - 1


def _image_rows(rows, n, L, num_digits):
    """THE walk over image ``n`` of a host block, for both numpy restatements: of the first ``count`` rows the valid ones ->
    (their row indices, their labels, k = a row's place in (label, row) order, float64 [x, y, x2 - x + 1, y2 - y + 1, score] per
    row, rounded like Python's ``round``, how many of those values lie outside the rounding's domain).  ``ValueError``: a count
    outside [0, M]."""
    M, cf = rows.shape[1], rows[n, 0, 6]
    if not (cf >= 0 and cf < M + 1):
        raise ValueError('sample %d: count %r outside [0, %d]' % (n, cf, M))
    r = rows[n, :int(cf)]
    with np.errstate(invalid='ignore'):
        src = np.nonzero((r[:, 5] > -1) & (r[:, 5] < L))[0]
    r = r[src]
    label = r[:, 5].astype(np.int64)
    k = np.empty(len(r), np.int64)
    k[np.argsort(label, kind='mergesort')] = np.arange(len(r))
    b = r[:, :5].astype(np.float64)
    xywhs, bad = _round_half_even(np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0] + 1, b[:, 3] - b[:, 1] + 1, b[:, 4]], axis=1),
                                  num_digits)
    return src, label, k, xywhs, bad


def _refuse_flags(bad_value, bad_layout, M, num_digits, values, layout):
    """the order kernel's two flag words as ``ValueError``s, in the route's words for what they count"""
    if bad_value:
        raise ValueError('%d %s are not finite or reach 2**40 / 10**%d' % (bad_value, values, num_digits))
    if bad_layout:
        raise ValueError('%d samples with a count outside [0, %d] %s' % (bad_layout, M, layout))


def _pack_tables(packed_gt, dataset, N, L):
    """(img_slot int32 [N]: sample -> index into packed_gt.img_ids, -1 unknown; cat_of_label int32 [L]: label -> index into
    packed_gt.cat_ids, -1 unknown); N and L are ``_row_block``'s"""
    ii, ok_i = _index_of(packed_gt.img_ids, np.asarray(dataset.img_ids[:N], dtype=np.int64).reshape(-1))
    ci, ok_c = _index_of(packed_gt.cat_ids, np.asarray(dataset.cat_ids[:L], dtype=np.int64))
    slot = np.where(ok_i, ii, -1).astype(np.int32)
    if len(np.unique(slot[slot >= 0])) != np.count_nonzero(slot >= 0):
        raise ValueError('two samples share an image id: their detections share cells, which only the host packing handles')
    return slot, np.where(ok_c, ci, -1).astype(np.int32)


def _packed_pair(outs, start, kxy32, num_digits):
    """the two Packed objects from per-kind dicts of arrays"""
    b, k = outs
    return dict(
        bbox=Packed(kind='bbox', cell=b['cell'], start=start[0], img_idx=b['img_idx'], cat_idx=b['cat_idx'], score=b['score'],
                    bbox=b['bbox'], area=b['area'], id=b['id'], kxy=None),
        keypoints=Packed(kind='keypoints', cell=k['cell'], start=start[1], img_idx=k['img_idx'], cat_idx=k['cat_idx'],
                         score=k['score'], bbox=None, area=None, id=k['id'], kxy=None, kxy32=kxy32, num_digits=num_digits))


def pack_rows_restatement(packed_gt, dataset, rows, num_digits=4, num_labels=None):
    """``kgdet_coco_order_dets`` + the two scans + ``kgdet_coco_scatter_dets`` in numpy on a host copy of ``rows`` float32
    [N, M, 7 + 3K] (``runner.DeviceResults.rows``) -> {'bbox': Packed, 'keypoints': Packed}, field for field what
    ``pack_test_results(packed_gt, dataset, dev.to_host(), num_digits, lazy_landmarks=True)`` returns.  Per image: the first
    ``count`` rows; a row's k = its place in (label, row) order; its rank = its place among the rows of its category in
    (descending rounded score, k) order; a row with rank < 100 / 20 goes to ``start[cell] + rank`` of the bbox / keypoints kind.
    ``num_labels``: how many labels the detector has (None: the dataset's categories).  ``ValueError``: a value outside the
    rounding's domain, a count outside [0, M], detections of an image the ground truth does not hold."""
    if not isinstance(rows, np.ndarray):
        rows = rows.cpu().numpy()
    N, M, W, K, L = _row_block(rows, dataset, num_labels, num_digits, 9)
    pg = packed_gt
    slot, cat_of_label = _pack_tables(pg, dataset, N, L)
    C = len(pg.cat_ids)
    n_cells = len(pg.img_ids) * C
    cuts = (MAX_DETS['bbox'], MAX_DETS['keypoints'])
    cnt = np.zeros((2, n_cells), np.int64)
    per_image, img_rows, n_bad = [], np.zeros(N, np.int64), 0
    for n in range(N):
        src, label, k, xywhs, bad = _image_rows(rows, n, L, num_digits)
        cat = cat_of_label[label].astype(np.int64)
        img_rows[n] = len(src)
        if len(src) and slot[n] < 0:
            raise ValueError('Results do not correspond to current coco set')
        n_bad += bad
        rank = np.full(len(src), -1, np.int64)
        for c in np.unique(cat[cat >= 0]):
            sel = np.nonzero(cat == c)[0]
            rank[sel[np.lexsort((k[sel], -xywhs[sel, 4]))]] = np.arange(len(sel))
            cnt[:, slot[n] * C + c] = np.minimum(len(sel), cuts)
        per_image.append((src, cat, k, rank, xywhs))
    _refuse_flags(n_bad, 0, M, num_digits, 'box / score values', '')
    start = np.zeros((2, n_cells + 1), np.int64)
    np.cumsum(cnt, axis=1, out=start[:, 1:])
    img_base = np.cumsum(img_rows) - img_rows
    outs = []
    for kind in range(2):
        nk = int(start[kind, -1])
        outs.append(dict(cell=np.full(nk, -1, np.int64), img_idx=np.full(nk, -1, np.int64), cat_idx=np.full(nk, -1, np.int64),
                         id=np.full(nk, -1, np.int64), score=np.full(nk, np.nan), bbox=np.full((nk, 4), np.nan),
                         area=np.full(nk, np.nan)))
    kxy32 = np.zeros((int(start[1, -1]), 3 * K), np.float32)
    for n, (src, cat, k, rank, xywhs) in enumerate(per_image):
        for kind, o in enumerate(outs):
            keep = (cat >= 0) & (rank >= 0) & (rank < cuts[kind])
            cell = slot[n] * C + cat[keep]
            pos = start[kind][cell] + rank[keep]
            o['cell'][pos], o['img_idx'][pos], o['cat_idx'][pos], o['id'][pos] = cell, slot[n], cat[keep], img_base[n] + k[keep] + 1
            o['score'][pos], o['bbox'][pos] = xywhs[keep, 4], xywhs[keep, :4]
            o['area'][pos] = xywhs[keep, 2] * xywhs[keep, 3]
            if kind == 1:
                kxy32[pos] = rows[n, src[keep], 7:]
    return _packed_pair(outs, start, kxy32, num_digits)


def pack_device_results(packed_gt, dataset, dev_results, num_digits=4, device=None):
    """``pack_test_results(packed_gt, dataset, dev_results.to_host(), num_digits, lazy_landmarks=True)`` without the host list:
    ``kgdet_coco_order_dets``, two ``torch.cumsum``, ``kgdet_coco_scatter_dets`` on ``dev_results.rows`` where it lies.  The small
    arrays of both Packed come back as numpy (``category_order``, ``accumulate`` and ``summarize`` work on them unchanged);
    the landmark rows ``kxy32`` of the 'keypoints' Packed are a float32 tensor on the device, which ``_run_device`` slices in
    place of an upload.  ``device``: None = where the rows are.  Rows on the CPU take ``pack_rows_restatement``.
    ``ValueError`` as the restatement's -- ``evaluate_results`` then packs ``to_host()`` on the host."""
    rows, L = _rows_and_labels(dev_results, device)
    if not rows.is_cuda or rows.shape[0] == 0:
        return pack_rows_restatement(packed_gt, dataset, rows, num_digits, num_labels=L)
    N, M, W, K, L = _row_block(rows, dataset, L, num_digits, 9)
    slot, cat_of_label = _pack_tables(packed_gt, dataset, N, L)
    C = len(packed_gt.cat_ids)
    outs, start = _pack_rows_on_device(rows.contiguous(), slot, cat_of_label, C, len(packed_gt.img_ids) * C, num_digits)
    kxy32 = outs[1].pop('kxy32')
    host = [{f: (t.cpu().numpy() if t is not None else None) for f, t in o.items() if f != 'kxy32'} for o in outs]
    return _packed_pair(host, start.cpu().numpy(), kxy32, num_digits)


def _empty_on(dev):
    import torch
    return lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)


def _order_rows_on_device(rows, slot_t, col_t, C, n_cells, num_digits, alloc):
    """THE launch of ``kgdet_coco_order_dets``, for the packing and for the result files: contiguous CUDA ``rows`` [N, M, W],
    the tables sample -> image slot [N] and label -> column [L] as int32 device tensors, ``C`` columns per image, ``n_cells``
    cells -> (vals float64 [N, M, 6], info int32 [N, M, 3], img_rows int32 [N], all three from ``alloc(shape, dtype)``; img_base
    int64 [N], the exclusive scan of img_rows; cnt int32 [2, n_cells], a cell's kept rows under either cut; flags int32 [2]).
    ``cnt`` and ``flags`` are zeroed here: the kernel writes only the cells of images it knows and adds to the flags.  Nothing
    is read back.  ``ValueError``: more rows per image than the kernel ranks."""
    import torch
    from . import _lib
    N, M, W = rows.shape
    if M > _lib.COCO_ORDER_MAX_ROWS:
        raise ValueError('%d detections per image: the order kernel ranks up to %d' % (M, _lib.COCO_ORDER_MAX_ROWS))
    dev = rows.device
    i32, i64, p = ctypes.c_int32, ctypes.c_int64, _lib.ptr
    with torch.cuda.device(dev):
        vals, info, img_rows = alloc((N, M, 6), torch.float64), alloc((N, M, 3), torch.int32), alloc((N,), torch.int32)
        cnt = torch.zeros((2, n_cells), dtype=torch.int32, device=dev)
        flags = torch.zeros(2, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().kgdet_coco_order_dets(
            p(rows), i64(N), i32(M), i32(W), p(slot_t), p(col_t), i32(len(col_t)), i32(C), i64(n_cells), i32(num_digits),
            i32(MAX_DETS['bbox']), i32(MAX_DETS['keypoints']), p(vals), p(info), p(img_rows), p(cnt[0]), p(cnt[1]), p(flags),
            _lib.current_stream()), 'kgdet_coco_order_dets')
        img_base = torch.cumsum(img_rows, dim=0, dtype=torch.int64) - img_rows
    return vals, info, img_rows, img_base, cnt, flags


def _pack_rows_on_device(rows, slot, cat_of_label, C, n_cells, num_digits, alloc=None):
    """the launches of ``pack_device_results`` on a CUDA tensor ``rows`` [N, M, W] and the two host tables ->
    ([bbox arrays, keypoints arrays] as dicts of device tensors, start int64 [2, n_cells + 1] on the device).  ``alloc(shape,
    dtype)``: where the kernels' outputs and intermediates come from (None: ``torch.empty`` on the rows' device)."""
    import torch
    from . import _lib
    N, M, W = rows.shape
    dev = rows.device
    alloc = _empty_on(dev) if alloc is None else alloc
    i32, i64, p = ctypes.c_int32, ctypes.c_int64, _lib.ptr
    with torch.cuda.device(dev):
        slot_t, col_t = torch.from_numpy(slot).to(dev), torch.from_numpy(cat_of_label).to(dev)
        vals, info, img_rows, img_base, cnt, flags = _order_rows_on_device(rows, slot_t, col_t, C, n_cells, num_digits, alloc)
        start = torch.zeros((2, n_cells + 1), dtype=torch.int64, device=dev)
        start[:, 1:] = torch.cumsum(cnt, dim=1, dtype=torch.int64)
        n_b, n_k, bad_value, bad_layout = torch.cat([start[:, -1], flags.to(torch.int64)]).tolist()     # (the one read-back)
        _refuse_flags(bad_value, bad_layout, M, num_digits, 'box / score values',
                      'or with detections of an image the ground truth does not hold')
        outs, structs = [], []
        for n, lazy in ((n_b, False), (n_k, True)):
            o = dict(cell=alloc((n,), torch.int64), img_idx=alloc((n,), torch.int64), cat_idx=alloc((n,), torch.int64),
                     id=alloc((n,), torch.int64), score=alloc((n,), torch.float64),
                     bbox=None if lazy else alloc((n, 4), torch.float64), area=None if lazy else alloc((n,), torch.float64),
                     kxy32=alloc((n, W - 7), torch.float32) if lazy else None)
            outs.append(o)
            structs.append(_lib.CocoPackedDets(n=n, **{f: (o[f].data_ptr() if o[f] is not None else None) for f in o}))
        _lib.check(_lib.lib().kgdet_coco_scatter_dets(
            p(rows), i64(N), i32(M), i32(W), p(slot_t), i32(C), i64(n_cells), p(vals), p(info), p(img_base), p(start[0]), p(start[1]),
            i32(MAX_DETS['bbox']), i32(MAX_DETS['keypoints']), ctypes.byref(structs[0]), ctypes.byref(structs[1]), p(flags),
            _lib.current_stream()), 'kgdet_coco_scatter_dets')
        if int(flags[1]):
            raise RuntimeError('kgdet_coco_scatter_dets: rows fell outside the packed arrays (counts and scans disagree)')
        return outs, start


def _is_device_results(results):
    return hasattr(results, 'rows') and hasattr(results, 'to_host') and hasattr(results, 'release')


# ------------------------------------------------------------------------------------------------
# the two kernels restated in numpy on the packed layout (csrc/coco_eval.hip)
# ------------------------------------------------------------------------------------------------
def similarity_restatement(c):
    """``kgdet_coco_similarity`` for one chunk ``c`` (see ``DeviceCocoEvaluator._chunks``): evaluation.box_iou_xywh /
    evaluation.oks, operation by operation, on the arrays."""
    sim = np.zeros(c.sim_size, np.float64)
    for (d0, D, g0, G), off in zip(c.cells, c.sim_off):
        if D == 0 or G == 0:
            continue
        if c.iou_type == 'bbox':
            d, g = c.d_box[d0:d0 + D], c.g_box[g0:g0 + G]
            iw = np.minimum(d[:, None, 0] + d[:, None, 2], g[None, :, 0] + g[None, :, 2]) - np.maximum(d[:, None, 0], g[None, :, 0])
            ih = np.minimum(d[:, None, 1] + d[:, None, 3], g[None, :, 1] + g[None, :, 3]) - np.maximum(d[:, None, 1], g[None, :, 1])
            inter = np.where((iw > 0) & (ih > 0), iw * ih, 0.0)
            da, ga = (d[:, 2] * d[:, 3])[:, None], (g[:, 2] * g[:, 3])[None, :]
            union = np.where(c.g_crowd[g0:g0 + G].astype(bool)[None, :], da, da + ga - inter)
            with np.errstate(divide='ignore', invalid='ignore'):
                block = np.where(inter > 0, inter / union, 0.0)
        else:
            xd, yd = c.d_kxy[d0:d0 + D, :, 0], c.d_kxy[d0:d0 + D, :, 1]
            block = np.zeros((D, G))
            for j in range(G):
                k = c.g_kpt[g0 + j]
                xg, yg, vis = k[0::3], k[1::3], k[2::3] > 0
                if c.g_nvis[g0 + j] > 0:
                    dx, dy = xd - xg, yd - yg
                else:
                    bx, by, bw, bh = c.g_box[g0 + j]
                    x0, x1, y0, y1 = bx - bw, bx + bw * 2, by - bh, by + bh * 2
                    dx = np.maximum(0, x0 - xd) + np.maximum(0, xd - x1)
                    dy = np.maximum(0, y0 - yd) + np.maximum(0, yd - y1)
                e = (dx ** 2 + dy ** 2) / c.var / (c.g_area[g0 + j] + np.spacing(1)) / 2
                if c.g_nvis[g0 + j] > 0:
                    e = e[:, vis]
                block[:, j] = np.exp(-e).sum(axis=1) / e.shape[1]
        sim[off:off + D * G] = block.reshape(-1)
    return sim


def match_restatement(c, sim):
    """``kgdet_coco_match`` for one chunk: every (area range, threshold) pair is a lane ([A, T] arrays), a detection sweeps the
    regular ground truths in order and then, in the lanes where none matched, the ignored ones."""
    A, T = len(c.area_rng), len(c.best0)
    lo, hi = c.area_rng[:, 0], c.area_rng[:, 1]
    d_match = np.zeros((c.nd, A, T), np.int32)
    d_ignore = np.zeros((c.nd, A, T), np.uint8)
    g_ignore = np.zeros((c.ng, A), np.uint8)
    aa, tt = np.meshgrid(np.arange(A), np.arange(T), indexing='ij')
    for (d0, D, g0, G), off in zip(c.cells, c.sim_off):
        ga = c.g_area[g0:g0 + G]
        ign = c.g_ign[g0:g0 + G, None].astype(bool) | (ga[:, None] < lo[None]) | (ga[:, None] > hi[None])     # [G, A]
        g_ignore[g0:g0 + G] = ign
        ign = np.repeat(ign[:, :, None], T, axis=2)
        taken = np.zeros((G, A, T), bool)
        crowd = c.g_crowd[g0:g0 + G] != 0
        block = sim[off:off + D * G].reshape(D, G) if D and G else None
        for di in range(D):
            best = np.broadcast_to(c.best0[None, :], (A, T)).copy()
            m = np.full((A, T), -1)
            if block is not None:
                for sweep in (False, True):
                    live = (m < 0) if sweep else np.ones((A, T), bool)
                    for gi in range(G):
                        cand = live & (ign[gi] == sweep) & ~(taken[gi] & ~crowd[gi]) & ~(block[di, gi] < best)
                        best = np.where(cand, block[di, gi], best)
                        m = np.where(cand, gi, m)
            hit = m >= 0
            da = c.d_area[d0 + di]
            outside = np.broadcast_to(((da < lo) | (da > hi))[:, None], (A, T))
            d_ignore[d0 + di] = np.where(hit, ign[np.maximum(m, 0), aa, tt] if G else False, outside)
            d_match[d0 + di] = np.where(hit, g0 + m + 1, 0)
            taken[m[hit], aa[hit], tt[hit]] = True
    return d_match, d_ignore, g_ignore


def _run_host(c, want_sim=True):
    sim = similarity_restatement(c)
    return (sim if want_sim else None,) + match_restatement(c, sim)


def _is_lazy(packed):
    """a landmark Packed that carries the float32 rows ``kxy32`` in place of ``kxy`` / ``bbox`` / ``area``"""
    return packed.kxy is None and getattr(packed, 'kxy32', None) is not None


def _upload(dev, a, dtype=None):
    """an array (cast to ``dtype`` first) or a tensor, contiguous on ``dev``; None stays None"""
    import torch
    if a is None:
        return None
    if torch.is_tensor(a):                                          # (rows that never left the device: pack_device_results)
        return a.to(dev).contiguous()
    a = np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype, copy=False))).to(dev)


def _run_device(c, device, want_sim=True, on_device=None):
    """the two launches of csrc/coco_eval.hip for one chunk; the similarity matrix stays on the device between them.  A lazy
    landmark chunk (``c.kxy32``) first runs ``kgdet_coco_pack_landmarks`` on its float32 rows: the two kernels read its
    ``d_kxy`` / ``d_area`` in device memory, ``bbox`` / ``area`` come back as ``c.out_bbox`` / ``c.out_area``.  ``on_device``:
    (d_match, d_ignore, g_ignore) dataset-sized device tensors -- the chunk writes its slices there, ``g0`` is added on the
    device and the three are not downloaded (None in their place)."""
    import torch
    from . import _lib
    L = _lib.lib()
    dev = torch.device(device)
    up = functools.partial(_upload, dev)
    A, T = len(c.area_rng), len(c.best0)
    kp = c.iou_type == 'keypoints'
    with torch.cuda.device(dev):
        cells, sim_off = up(c.cells, np.int32), up(c.sim_off, np.int64)
        d_box, g_box = (None if kp else up(c.d_box)), up(c.g_box)
        stream, p = _lib.current_stream(), _lib.ptr
        i32, i64 = ctypes.c_int32, ctypes.c_int64
        if kp and getattr(c, 'kxy32', None) is not None:
            K = c.kxy32.shape[1] // 3
            src = up(c.kxy32)
            d_kxy = torch.empty((c.nd, K, 2), dtype=torch.float64, device=dev)
            d_bbox = torch.empty((c.nd, 4), dtype=torch.float64, device=dev)
            d_area = torch.empty((c.nd,), dtype=torch.float64, device=dev)
            _lib.check(L.kgdet_coco_pack_landmarks(p(src), i64(c.nd), i32(K), i32(c.num_digits), p(d_kxy), p(d_bbox), p(d_area),
                                                   stream), 'kgdet_coco_pack_landmarks')
            c.out_bbox, c.out_area = d_bbox.cpu().numpy(), d_area.cpu().numpy()
            del src
            g_kpt = up(c.g_kpt)
        else:
            d_kxy, g_kpt = (up(c.d_kxy), up(c.g_kpt)) if kp else (None, None)
            d_area = up(c.d_area)
        g_area = up(c.g_area)
        g_crowd, g_nvis, g_ign = up(c.g_crowd, np.int32), up(c.g_nvis, np.int32), up(c.g_ign, np.uint8)
        var, rng, best0 = up(c.var), up(c.area_rng), up(c.best0)
        sim = torch.zeros(max(c.sim_size, 1), dtype=torch.float64, device=dev)
        if on_device is None:
            d_match = torch.zeros((c.nd, A, T), dtype=torch.int32, device=dev)
            d_ignore = torch.zeros((c.nd, A, T), dtype=torch.uint8, device=dev)
            g_ignore = torch.zeros((c.ng, A), dtype=torch.uint8, device=dev)
        else:
            d_match, d_ignore, g_ignore = on_device[0][c.d0:c.d1], on_device[1][c.d0:c.d1], on_device[2][c.g0:c.g1]
        g_taken = torch.empty((c.ng, A, T), dtype=torch.uint8, device=dev)
        C = len(c.cells)
        _lib.check(L.kgdet_coco_similarity(i32(1 if kp else 0), p(cells), p(sim_off), i32(C), i64(c.nd), i64(c.ng),
                                           i64(c.sim_size), p(d_box), p(d_kxy), p(g_box), p(g_kpt), p(g_area), p(g_crowd),
                                           p(g_nvis), p(var), i32(len(c.var)), p(sim), stream), 'kgdet_coco_similarity')
        _lib.check(L.kgdet_coco_match(p(cells), p(sim_off), i32(C), i64(c.nd), i64(c.ng), i64(c.sim_size), p(sim), p(d_area),
                                      p(g_area), p(g_ign), p(g_crowd), p(rng), i32(A), p(best0), i32(T), p(d_match),
                                      p(d_ignore), p(g_ignore), p(g_taken), stream), 'kgdet_coco_match')
        if on_device is not None:
            if c.g0:
                d_match.add_((d_match > 0).to(torch.int32), alpha=c.g0)       # chunk-local -> packed index
            return sim[:c.sim_size].cpu().numpy() if want_sim else None, None, None, None
        return (sim[:c.sim_size].cpu().numpy() if want_sim else None, d_match.cpu().numpy(), d_ignore.cpu().numpy(),
                g_ignore.cpu().numpy())


def _default_device():
    from . import _lib
    try:
        import torch
        if torch.cuda.is_available() and os.path.exists(_lib.LIB_PATH):
            return 'cuda'
    except ImportError:
        pass
    return 'cpu'


def category_order(packed_dt, K):
    """(order int64 [ND], cat_cut int64 [K + 1]): the detections grouped by category, inside a category in descending score,
    equal scores in packed = (image, rank) order -- ONE stable sort per evaluation.  Restricted to ``rank < max_det`` it is the
    stable score sort of that subset, i.e. the per-``max_dets`` argsort of ``accumulate_restatement``."""
    d = packed_dt
    order = np.lexsort((-d.score, d.cat_idx)).astype(np.int64)          # (stable: ties keep the packed order)
    return order, np.searchsorted(d.cat_idx[order], np.arange(K + 1)).astype(np.int64)


def _has_device_accumulate():
    from . import _lib
    return hasattr(_lib.lib(), 'kgdet_coco_accumulate')


class _DeviceOutputs(object):
    """``evaluate()``'s outputs while they stay in device memory (``dev`` = d_match, d_ignore, g_ignore tensors): the host
    arrays of the same names are downloaded when first asked for, and kept"""

    def __init__(self, dev, **kw):
        self.dev = dev
        self.__dict__.update(kw)

    def __getattr__(self, name):                  # (only reached for what is not there yet)
        if name not in ('d_match', 'd_ignore', 'g_ignore'):
            raise AttributeError(name)
        self.d_match, self.g_ignore = self.dev[0].cpu().numpy(), self.dev[2].cpu().numpy()
        self.d_ignore = self.dev[1].cpu().numpy().view(bool)
        return self.__dict__[name]


class DeviceCocoEvaluator(CocoEvaluator):
    """``CocoEvaluator`` on packed arrays.  ``device``: a CUDA device (the HIP kernels), ``'cpu'`` (their numpy restatement)
    or None = the GPU when there is one and the library is built, else the restatement.  ``params`` as ``CocoEvaluator``'s;
    what packing has already fixed cannot be edited there: ``evaluate`` raises ``ValueError`` when ``img_ids`` / ``cat_ids`` are
    not the packed ground truth's (pack a subset instead), when ``max_dets[-1]`` is not the cut the detections were packed
    with, and for ``use_cats = 0``.  ``iou_thrs``, ``rec_thrs``, ``area_rng`` (at most 64 (range, threshold) pairs) and the
    smaller ``max_dets`` entries are honoured.  ``keep_similarity``: also download the similarity matrices (``similarity``);
    the stats do not need them.  ``device_accumulate``: keep the matching outputs in device memory and run ``accumulate`` as
    ``kgdet_coco_accumulate`` (bit-equal to ``accumulate_restatement``); None = on for a CUDA device when the library has the
    kernel, else off; True on the CPU path, or without the kernel, is an error.  A lazy landmark Packed
    (``pack_test_results(..., lazy_landmarks=True)``) is rounded on the GPU chunk by chunk, or on the host for ``'cpu'``;
    ``evaluate`` stores its ``bbox`` / ``area``."""

    def __init__(self, packed_gt, packed_dt, iou_type, device=None, keep_similarity=False, device_accumulate=None):
        self.keep_similarity = keep_similarity
        self.device_accumulate = device_accumulate
        self.params = EvalParams(iou_type)
        if len(packed_dt.score) and packed_dt.kind != iou_type:
            raise ValueError('the detections were packed as %r results (sorted and cut for that type), not %r'
                             % (packed_dt.kind, iou_type))
        self.gt, self.dt = packed_gt, packed_dt
        self.params.img_ids, self.params.cat_ids = list(packed_gt.img_ids), list(packed_gt.cat_ids)
        self.device = _default_device() if device is None else device
        self.eval_imgs, self.eval, self.stats = None, {}, None
        self._out = None

    # --- evaluate ---------------------------------------------------------------------------------
    def _chunks(self, limit):
        """the cell table (cells with a detection or a ground truth), cut where a chunk would pass ``limit`` detections.
        Detections and ground truths are both in cell order, so a run of cells owns one slice of each."""
        p, g, d = self.params, self.gt, self.dt
        kp = p.iou_type == 'keypoints'
        dn, gn = np.diff(d.start), np.diff(g.start)
        live = np.nonzero((dn > 0) | (gn > 0))[0]
        cells = np.stack([d.start[live], dn[live], g.start[live], gn[live]], axis=1)
        base = ((g.iscrowd != 0) | (g.num_keypoints == 0)) if kp else (g.iscrowd != 0)
        common = dict(iou_type=p.iou_type, var=(landmark_meta()['oks_sigmas'] * 2) ** 2,
                      area_rng=np.asarray(p.area_rng, dtype=np.float64).reshape(-1, 2),
                      best0=np.minimum(np.asarray(p.iou_thrs, dtype=np.float64), 1 - 1e-10))
        lazy = kp and _is_lazy(d)                                   # (rounded by the chunk on the device)
        if lazy:
            common['num_digits'] = d.num_digits
        lo = 0
        while lo < len(cells):
            hi = int(np.searchsorted(cells[:, 0] + cells[:, 1], cells[lo, 0] + limit, side='right'))
            hi = max(hi, lo + 1)
            d0, d1 = int(cells[lo, 0]), int(cells[hi - 1, 0] + cells[hi - 1, 1])
            g0, g1 = int(cells[lo, 2]), int(cells[hi - 1, 2] + cells[hi - 1, 3])
            local = cells[lo:hi] - np.array([d0, 0, g0, 0])
            size = local[:, 1] * local[:, 3]
            yield Packed(d0=d0, d1=d1, g0=g0, g1=g1, nd=d1 - d0, ng=g1 - g0, cells=local,
                         sim_off=np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64), sim_size=int(size.sum()),
                         kxy32=d.kxy32[d0:d1] if lazy else None,
                         d_box=None if lazy else d.bbox[d0:d1], d_area=None if lazy else d.area[d0:d1],
                         d_kxy=(d.kxy[d0:d1] if d.kxy is not None else np.zeros((0, g.num_landmarks, 2))) if kp and not lazy else None,
                         g_box=g.bbox[g0:g1], g_area=g.area[g0:g1], g_kpt=g.keypoints[g0:g1] if kp else None,
                         g_crowd=g.iscrowd[g0:g1], g_nvis=g.num_visible[g0:g1], g_ign=base[g0:g1].astype(np.uint8), **common)
            lo = hi

    def evaluate(self):
        p = self.params
        if not p.use_cats:
            raise ValueError('use_cats = 0 is not offered on the packed path: use evaluation.CocoEvaluator')
        on_cpu = str(self.device) == 'cpu'
        if on_cpu and p.iou_type == 'keypoints':
            materialize(self.dt)                                    # (a lazy Packed: the numpy route)
        if p.iou_type == 'keypoints' and len(self.dt.score) and self.dt.kxy is None and not _is_lazy(self.dt):
            raise ValueError('landmark evaluation needs landmark detections')
        dev_acc = self.device_accumulate
        if dev_acc is None:
            dev_acc = not on_cpu and _has_device_accumulate()
        elif dev_acc and (on_cpu or not _has_device_accumulate()):
            raise ValueError('device_accumulate needs a CUDA device and a library with kgdet_coco_accumulate')
        if (not np.array_equal(np.unique(p.img_ids), self.gt.img_ids) or not np.array_equal(np.unique(p.cat_ids), self.gt.cat_ids)):
            raise ValueError('params.img_ids / cat_ids differ from the packed ground truth: the cells are fixed by packing '
                             '(pack the subset, or use evaluation.CocoEvaluator)')
        p.max_dets = sorted(p.max_dets)
        if p.max_dets[-1] != MAX_DETS[p.iou_type]:
            raise ValueError('params.max_dets[-1] = %r, but the detections were cut to %d per cell when they were packed'
                             % (p.max_dets[-1], MAX_DETS[p.iou_type]))
        A, T = len(p.area_rng), len(p.iou_thrs)
        nd, ng = len(self.dt.score), len(self.gt.id)
        lazy = p.iou_type == 'keypoints' and _is_lazy(self.dt)
        if lazy:
            self.dt.bbox, self.dt.area = np.zeros((nd, 4)), np.zeros(nd)
        size = np.diff(self.dt.start) * np.diff(self.gt.start)
        sim_start = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
        # d_match, d_ignore, g_ignore of the whole dataset, where the chunks' outputs go (np.zeros touches no page by itself)
        if dev_acc:
            import torch
            out = (torch.zeros((nd, A, T), dtype=torch.int32, device=self.device),
                   torch.zeros((nd, A, T), dtype=torch.uint8, device=self.device),
                   torch.zeros((ng, A), dtype=torch.uint8, device=self.device))
        else:
            out = np.zeros((nd, A, T), np.int32), np.zeros((nd, A, T), np.uint8), np.zeros((ng, A), np.uint8)
        run = _run_host if on_cpu else functools.partial(_run_device, device=self.device, on_device=out if dev_acc else None)
        sims = []
        for c in self._chunks(CHUNK_DETS[p.iou_type]):
            sim, dm, di, gi = run(c, want_sim=self.keep_similarity)
            sims.append(sim)
            if lazy:
                self.dt.bbox[c.d0:c.d1], self.dt.area[c.d0:c.d1] = c.out_bbox, c.out_area
            if dev_acc:
                continue                                            # (the chunk wrote its slices itself)
            if c.g0:
                np.add(dm, c.g0, out=dm, where=dm > 0)             # chunk-local -> packed index, in place
            if c.nd == nd and c.ng == ng:
                out = dm, di, gi                                    # one chunk: the downloaded arrays as they are
            else:
                out[0][c.d0:c.d1], out[1][c.d0:c.d1], out[2][c.g0:c.g1] = dm, di, gi
        sim = (np.concatenate(sims) if sims else np.zeros(0)) if self.keep_similarity else None
        if dev_acc:
            self._out = _DeviceOutputs(out, sim_start=sim_start, sim=sim)
        else:
            self._out = Packed(d_match=out[0], d_ignore=out[1].view(bool), g_ignore=out[2], sim=sim, sim_start=sim_start)
        return self

    # --- accessors at the level of CocoEvaluator's intermediate results -----------------------------
    def _cell(self, img_id, cat_id):
        (i,), (oki,) = _index_of(self.gt.img_ids, [img_id])
        (k,), (okk,) = _index_of(self.gt.cat_ids, [cat_id])
        if not (oki and okk):
            raise KeyError((img_id, cat_id))
        return int(i) * len(self.gt.cat_ids) + int(k)

    def similarity(self, img_id, cat_id):
        """the [D, G] matrix of one (image, category), rows in descending-score order; [0, 0] when either side is empty"""
        c = self._cell(img_id, cat_id)
        D, G = int(self.dt.start[c + 1] - self.dt.start[c]), int(self.gt.start[c + 1] - self.gt.start[c])
        if D == 0 or G == 0:
            return np.zeros((0, 0))
        if self._out.sim is None:
            raise RuntimeError('the similarities were not downloaded: construct with keep_similarity=True')
        s = self._out.sim_start[c]
        return self._out.sim[s:s + D * G].reshape(D, G).copy()

    def eval_imgs_of(self, k, a, i):
        """what ``CocoEvaluator.eval_imgs[(k * A + a) * I + i]`` holds: None, or d_match [T, D] (ground-truth ids, 0 = none),
        d_scores [D], g_ignore [G] (regular first, as the reference orders the ground truths), d_ignore [T, D]"""
        c = i * len(self.gt.cat_ids) + k
        d0, d1, g0, g1 = self.dt.start[c], self.dt.start[c + 1], self.gt.start[c], self.gt.start[c + 1]
        if d0 == d1 and g0 == g1:
            return None
        m = self._out.d_match[d0:d1, a, :].T
        ids = self.gt.id[np.maximum(m, 1) - 1] if len(self.gt.id) else np.zeros(m.shape, np.int64)
        return dict(d_match=np.where(m > 0, ids, 0).astype(np.float64), d_scores=self.dt.score[d0:d1].copy(),
                    g_ignore=np.sort(self._out.g_ignore[g0:g1, a].astype(np.int64)),
                    d_ignore=self._out.d_ignore[d0:d1, a, :].T.copy())

    # --- accumulate ---------------------------------------------------------------------------------
    def accumulate(self):
        """``CocoEvaluator.accumulate``.  When ``evaluate()`` kept its outputs on the device (``device_accumulate``):
        ``kgdet_coco_accumulate`` -- ``order`` / ``cat_cut`` are built on the host by ONE numpy lexsort (``category_order``;
        the sort is not the hot path), ``n_gt`` by ``kgdet_coco_count_gt``, and only precision, recall and scores are
        downloaded, bit-equal to ``accumulate_restatement``.  Otherwise ``accumulate_restatement`` itself."""
        if self._out is None:
            raise RuntimeError('Please run evaluate() first')
        if not isinstance(self._out, _DeviceOutputs):
            return self.accumulate_restatement()
        import torch
        from . import _lib
        L = _lib.lib()
        p, d, g = self.params, self.dt, self.gt
        T, R, K, A, M = len(p.iou_thrs), len(p.rec_thrs), len(p.cat_ids), len(p.area_rng), len(p.max_dets)
        nd, ng = len(d.score), len(g.id)
        if min(T, R, K, A, M) == 0:
            return self.accumulate_restatement()                    # (empty result arrays: nothing to launch)
        dev = self._out.dev[0].device
        order, cat_cut = category_order(d, K)
        rank = (np.arange(nd) - d.start[d.cell]) if nd else np.zeros(0, np.int64)
        tp_cap = int(np.minimum(np.diff(cat_cut), np.bincount(g.cat_idx, minlength=K)[:K]).max())
        up = functools.partial(_upload, dev)
        with torch.cuda.device(dev):
            d_match, d_ignore, g_ignore = self._out.dev
            stream, ptr = _lib.current_stream(), _lib.ptr
            i32, i64 = ctypes.c_int32, ctypes.c_int64
            n_gt = torch.empty((K, A), dtype=torch.int32, device=dev)
            _lib.check(L.kgdet_coco_count_gt(ptr(g_ignore), ptr(up(g.cat_idx, np.int32)), i64(ng), i32(K), i32(A), ptr(n_gt),
                                             stream), 'kgdet_coco_count_gt')
            precision = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
            scores = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
            recall = torch.empty((T, K, A, M), dtype=torch.float64, device=dev)
            work = torch.empty(2 * tp_cap * K * A * M * T, dtype=torch.float64, device=dev)
            args = [up(d.score, np.float64), up(rank, np.int32), up(order, np.int64), up(cat_cut, np.int64), n_gt,
                    up(p.max_dets, np.int32), up(p.rec_thrs, np.float64)]
            _lib.check(L.kgdet_coco_accumulate(ptr(d_match), ptr(d_ignore), *[ptr(a) for a in args], i64(nd), i32(K), i32(A),
                                               i32(T), i32(M), i32(R), i64(tp_cap), ptr(precision), ptr(recall), ptr(scores),
                                               ptr(work), ctypes.c_size_t(work.numel() * 8), stream), 'kgdet_coco_accumulate')
            self.eval = dict(counts=[T, R, K, A, M], precision=precision.cpu().numpy(), recall=recall.cpu().numpy(),
                             scores=scores.cpu().numpy())
        return self

    def accumulate_restatement(self):
        """``CocoEvaluator.accumulate`` on the packed outputs: per (category, area range, max_dets) one stable score sort, integer
        cumulative sums over all thresholds at once, the precision envelope and ``searchsorted(side='left')`` per threshold."""
        if self._out is None:
            raise RuntimeError('Please run evaluate() first')
        p, d, g, o = self.params, self.dt, self.gt, self._out
        T, R, K, A, M = len(p.iou_thrs), len(p.rec_thrs), len(p.cat_ids), len(p.area_rng), len(p.max_dets)
        precision, recall, scores = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), -np.ones((T, R, K, A, M))
        eps = np.spacing(1)
        rec_thrs = np.asarray(p.rec_thrs)
        rank = np.arange(len(d.score)) - d.start[d.cell] if len(d.score) else np.zeros(0, np.int64)
        d_by_cat = np.argsort(d.cat_idx, kind='mergesort')          # (inside a category: image order, then rank)
        d_cut = np.searchsorted(d.cat_idx[d_by_cat], np.arange(K + 1))
        g_by_cat = np.argsort(g.cat_idx, kind='mergesort')
        g_cut = np.searchsorted(g.cat_idx[g_by_cat], np.arange(K + 1))
        for k in range(K):
            dk, gk = d_by_cat[d_cut[k]:d_cut[k + 1]], g_by_cat[g_cut[k]:g_cut[k + 1]]
            rank_k, score_k = rank[dk], d.score[dk]
            matched_k, ignored_k = o.d_match[dk] != 0, o.d_ignore[dk]          # [n, A, T], gathered once per category
            for a in range(A):
                n_gt = int(np.count_nonzero(o.g_ignore[gk, a] == 0))
                if n_gt == 0:
                    continue
                for m, max_det in enumerate(p.max_dets):
                    sel = np.nonzero(rank_k < max_det)[0]
                    sc = score_k[sel]
                    order = np.argsort(-sc, kind='mergesort')
                    sc, sel = sc[order], sel[order]
                    matched = np.ascontiguousarray(matched_k[sel, a, :].T)
                    ignored = np.ascontiguousarray(ignored_k[sel, a, :].T)
                    tp = np.cumsum(matched & ~ignored, axis=1).astype(np.float64)
                    fp = np.cumsum(~matched & ~ignored, axis=1).astype(np.float64)
                    rc = tp / n_gt
                    pr = tp / (fp + tp + eps)
                    recall[:, k, a, m] = rc[:, -1] if len(sel) else 0
                    pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]
                    for t in range(T):
                        pos = np.searchsorted(rc[t], rec_thrs, side='left')
                        ok = pos < len(sel)
                        q, s = np.zeros(R), np.zeros(R)
                        q[ok], s[ok] = pr[t, pos[ok]], sc[pos[ok]]
                        precision[t, :, k, a, m], scores[t, :, k, a, m] = q, s
        self.eval = dict(counts=[T, R, K, A, M], precision=precision, recall=recall, scores=scores)
        return self


def evaluate_packed(packed_gt, packed_dt, iou_type, device=None, verbose=False, device_accumulate=None):
    return DeviceCocoEvaluator(packed_gt, packed_dt, iou_type, device,
                               device_accumulate=device_accumulate).evaluate().accumulate().summarize(verbose)


def evaluate_results(dataset, results, result_types=('bbox', 'keypoints'), device=None, packed_gt=None, verbose=False,
                     lazy_landmarks=None, device_accumulate=None):
    """{type: stats} for what ``single_gpu_test`` / ``multi_gpu_test`` returned for ``dataset``, without result files: the
    numbers of ``coco_eval(results2json(dataset, results, ...), result_types, dataset.coco)``.  ``packed_gt``: the dataset's
    ``pack_ground_truth(dataset.coco)`` when the caller keeps it between calls (a validation hook does).  ``lazy_landmarks``
    (None = off): the landmark rows stay float32 on the host and are rounded on the device (``pack_test_results``);
    ``device_accumulate``: ``DeviceCocoEvaluator``'s.  ``results`` may be a ``runner.DeviceResults``
    (``single_gpu_test(..., device_results=True)``): it is packed where it lies (``pack_device_results``, always with lazy
    landmarks) and released once packed; a ``ValueError`` of that packing sends its ``to_host()`` list down the host route."""
    for t in result_types:
        if t not in ('bbox', 'keypoints'):
            raise ValueError('unsupported result type {!r}'.format(t))
    if packed_gt is None:
        packed_gt = pack_ground_truth(dataset.coco)
    packed = None
    if _is_device_results(results):
        try:
            packed = pack_device_results(packed_gt, dataset, results)
        except ValueError as e:                  # (outside the device packing's domain: the host packing of the same detections)
            import warnings
            warnings.warn('device results are packed on the host instead (the slow route): %s' % e, RuntimeWarning)
            dev_results, results = results, results.to_host()
            dev_results.release()
        else:
            results.release()
    if packed is None:
        packed = pack_test_results(packed_gt, dataset, results, lazy_landmarks=bool(lazy_landmarks))
    out = {}
    for t in result_types:
        if t not in packed:
            raise ValueError('the results hold no {!r} detections'.format(t))
        out[t] = evaluate_packed(packed_gt, packed[t], t, device, verbose, device_accumulate)
    return out


# ------------------------------------------------------------------------------------------------
# results2json for results that stayed on the device (runner.DeviceResults; csrc/coco_json.hip)
# ------------------------------------------------------------------------------------------------
JSON_MAX_DIGITS = 4              # with 5 digits a non-zero value can fall below 1e-4, where repr switches to exponent form
# bytes of text per launch, copy and f.write: two device and two page-locked host buffers of this size are held.  Chosen from
# the sizes involved, not from a sweep: a landmark record is about 8.7 kB, so 64 MiB is some 7 700 records = 7 700 workgroups
# per launch (30 per CU), a copy of a few milliseconds over the host link, and a file write long enough for the page cache
# to take it in one piece; 4 x 64 MiB is small beside the rows themselves (11 GB at 32 000 x 100).
JSON_CHUNK_BYTES = 64 << 20


def format_decimals(q, negative, num_digits):
    """``repr`` of the doubles ``(-1)**negative * q / 10**num_digits`` as a list of str, from the integers alone: an optional
    ``-``, the integer part's digits, ``.``, the ``num_digits`` fractional digits without their trailing zeros but at least
    one.  For ``q < 2**40 + 1`` and ``1 <= num_digits <= 4`` the digits are at most 15 significant and the value is 0 or at
    least 1e-4, so this positional text is the shortest one that reads back as the same double -- what ``float.__repr__``
    prints (held to it by tests/test_json_refs.py)."""
    P = 10 ** num_digits
    out = []
    for v, neg in zip(np.asarray(q, dtype=np.int64).reshape(-1).tolist(), np.asarray(negative, dtype=bool).reshape(-1).tolist()):
        ip, fr = divmod(v, P)
        out.append('%s%d.%s' % ('-' if neg else '', ip, ('%0*d' % (num_digits, fr)).rstrip('0') or '0'))
    return out


def decimals_of_rounded(values, num_digits):
    """(q int64, negative bool) of doubles that are already n / 10**d (``round_half_even_restatement``'s): n = rint(|x| * 10**d),
    the sign is the double's sign bit -- a negative value that rounded to zero stays ``-0.0``"""
    x = np.asarray(values, dtype=np.float64)
    return np.rint(np.abs(x) * np.float64(10.0 ** num_digits)).astype(np.int64), np.signbit(x)


def decimals_of_landmarks(values, num_digits):
    """(q int64, negative bool, values outside the domain) for float32 landmark values: ``np.round(float64(v), d)`` is
    ``rint(v * 10**d) / 10**d`` and the float32 x 10**d product is exact in float64, so q = rint(|v| * 10**d) and the sign is
    v's sign bit.  A value that is not finite or with ``|v| * 10**d >= 2**40`` is counted and stands as 0."""
    v = np.asarray(values, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        p = np.abs(v) * np.float64(10.0 ** num_digits)
        bad = ~(p < ROUND_LIMIT)
    q = np.rint(np.where(bad, 0.0, p)).astype(np.int64)
    return q, np.signbit(v) & ~bad, int(np.count_nonzero(bad))


def _json_tables(dataset, N, L):
    """(image ids int64 [N], category ids int64 [L]) as the records print them; ``ValueError`` for what the kernels do not take"""
    tables = []
    for what, ids in (('image', list(dataset.img_ids)[:N]), ('category', list(dataset.cat_ids)[:L])):
        for v in ids:
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < 2 ** 63:
                raise ValueError('%s id %r: the device route prints non-negative integers below 2**63' % (what, v))
        tables.append(np.asarray([int(v) for v in ids], dtype=np.int64).reshape(-1))
    return tables


def _json_records(dataset, rows, num_digits=4, num_labels=None):
    """([bbox record bytes], [keypoints record bytes]) in id order: what ``json_restatement`` joins"""
    if not isinstance(rows, np.ndarray):
        rows = rows.cpu().numpy()
    N, M, W, K, L = _row_block(rows, dataset, num_labels, num_digits, JSON_MAX_DIGITS)
    img_ids, cat_ids = _json_tables(dataset, N, L)
    box_out, kpt_out, n_bad = [], [], 0
    for n in range(N):
        src, label, k, xywhs, bad = _image_rows(rows, n, L, num_digits)
        by_k = np.argsort(k)                                        # the records' order: label ascending, then row order
        src, label, xywhs = src[by_k], label[by_k], xywhs[by_k]
        q, neg, bad_k = decimals_of_landmarks(rows[n, src, 7:], num_digits)
        n_bad += bad + bad_k
        if bad or bad_k:
            continue
        box_text = format_decimals(*decimals_of_rounded(xywhs, num_digits), num_digits)
        kpt_text = format_decimals(q, neg, num_digits)
        for i in range(len(src)):
            x, y, w, h, s = box_text[5 * i:5 * i + 5]
            tail = '], "score": %s, "category_id": %d}' % (s, cat_ids[label[i]])
            box_out.append(('{"image_id": %d, "bbox": [%s, %s, %s, %s' % (img_ids[n], x, y, w, h) + tail).encode('ascii'))
            kpt_out.append(('{"image_id": %d, "keypoints": [%s' % (img_ids[n], ', '.join(kpt_text[3 * K * i:3 * K * (i + 1)]))
                            + tail).encode('ascii'))
    _refuse_flags(n_bad, 0, M, num_digits, 'values', '')
    return box_out, kpt_out


def json_restatement(dataset, rows, num_digits=4, num_labels=None):
    """(contents of P.bbox.json, contents of P.keypoints.json) as bytes: what ``evaluation.results2json(dataset, dev.to_host(),
    P)`` writes for ``rows`` float32 [N, M, 7 + 3K] (``runner.DeviceResults.rows``, a host copy), computed from the rows with
    the formatter rule written out (``format_decimals``) -- no ``json`` and no ``repr`` of a float.  Per image the first
    ``count`` rows with a label in [0, L), label ascending and in row order inside a label; xywh and score rounded like
    Python's ``round`` (``round_half_even_restatement``), landmark values like ``np.round``.  The reference of
    ``kgdet_coco_json_measure`` / ``kgdet_coco_json_write``; held to ``results2json`` by tests/test_json_refs.py.
    ``ValueError``: ``num_digits`` outside 1 .. 4, a value outside the domain, a count outside [0, M], more labels than
    ``dataset.cat_ids`` (``num_labels``: the detector's, None = the dataset's), ids that are not non-negative ints."""
    box, kpt = _json_records(dataset, rows, num_digits, num_labels)
    return b'[' + b', '.join(box) + b']', b'[' + b', '.join(kpt) + b']'


def _json_files(out_file):
    files = {'bbox': '{}.bbox.json'.format(out_file), 'keypoints': '{}.keypoints.json'.format(out_file)}
    files['proposal'] = files['bbox']
    return files


class _TempFiles(object):
    """the two result files under temporary names beside their targets: renamed by ``commit()``, removed on any exit
    without it"""

    def __init__(self, files):
        self.final = {k: files[k] for k in ('bbox', 'keypoints')}
        self.temp = {k: '%s.tmp-%d' % (p, os.getpid()) for k, p in self.final.items()}
        self.done = False

    def __enter__(self):
        return self

    def commit(self):
        for k in ('bbox', 'keypoints'):
            os.replace(self.temp[k], self.final[k])
        self.done = True

    def __exit__(self, *exc):
        if not self.done:
            for p in self.temp.values():
                if os.path.exists(p):
                    os.remove(p)
        return False


def _json_chunks(off, n_records, chunk_bytes):
    """record ranges [r0, r1) of at most ``chunk_bytes`` each, greedily, from the records' offsets (int64 [>= n_records + 1])"""
    bounds, r = [], 0
    while r < n_records:
        nxt = min(int(np.searchsorted(off[:n_records + 1], off[r] + chunk_bytes, side='right')) - 1, n_records)
        assert nxt > r
        bounds.append((r, nxt))
        r = nxt
    return bounds


def write_device_results_json(dataset, dev_results, out_file, num_digits=4, chunk_bytes=JSON_CHUNK_BYTES, device=None,
                              timings=None):
    """``evaluation.results2json(dataset, dev_results.to_host(), out_file)`` -- the same two files, byte for byte, and the
    same dict of their names -- without the host list: ``kgdet_coco_order_dets`` (identity tables, so no row is dropped
    for lack of ground truth) and ``kgdet_coco_json_measure`` on ``dev_results.rows`` where it lies, one ``torch.cumsum``
    per kind, ONE read-back (flags, record count and the records' byte offsets: 16 bytes per detection against 8.8 kB of
    text), then per kind a loop over chunks of whole records of at most ``chunk_bytes``: ``kgdet_coco_json_write`` into one of
    two device buffers, a non-blocking copy into one of two page-locked host buffers with an event behind it, and ``f.write``
    of that buffer while the next chunk's kernel and copy run; the write kernel's own flag word (records that disagree with
    their offsets) is read once more before the rename.  Only the calling thread touches HIP.  ``chunk_bytes``
    defaults to ``JSON_CHUNK_BYTES`` (see there for what it was chosen from).  The files are written under temporary names
    and renamed when both are complete.  ``dataset`` needs ``img_ids``, ``cat_ids`` and ``__len__`` only; the results are not
    released.  ``device``: None = where the rows are; rows on the CPU (or none) take ``json_restatement``.  ``timings``: a dict
    that receives seconds per stage (``order_measure_s``, ``kernel_s`` and ``copy_s`` from events, ``file_s``) and ``bytes``.
    ``ValueError``, with no file under a final name: released results, ``num_digits`` outside 1 .. 4, a value outside the
    domain (finite, ``|v| * 10**d < 2**40``), a count outside [0, M], more labels than ``dataset.cat_ids`` or than the order
    kernel's 64, more than its 1024 rows per image or more landmarks than a record's LDS image holds, ids that are not
    non-negative ints below 2**63, a record longer than ``chunk_bytes``."""
    import time
    import torch
    from . import _lib
    rows, L = _rows_and_labels(dev_results, device)
    chunk_bytes = int(chunk_bytes)
    if chunk_bytes < 1:
        raise ValueError('chunk_bytes %r' % (chunk_bytes,))
    files = _json_files(out_file)
    if timings is None:
        timings = {}
    timings.update(order_measure_s=0.0, kernel_s=0.0, copy_s=0.0, file_s=0.0, bytes=0)
    if not rows.is_cuda or rows.shape[0] == 0:
        box, kpt = _json_records(dataset, rows, num_digits, num_labels=L)
        longest = max([len(r) + 2 for r in box[1:] + kpt[1:]] + [len(r) for r in box[:1] + kpt[:1]] + [0])
        if longest > chunk_bytes:
            raise ValueError('a record of %d bytes does not fit chunk_bytes = %d' % (longest, chunk_bytes))
        with _TempFiles(files) as tmp:
            for kind, recs in (('bbox', box), ('keypoints', kpt)):
                with open(tmp.temp[kind], 'wb') as f:
                    f.write(b'[' + b', '.join(recs) + b']')
                timings['bytes'] += os.path.getsize(tmp.temp[kind])
            tmp.commit()
        return files
    rows = rows.contiguous()
    N, M, W, K, L = _row_block(rows, dataset, L, num_digits, JSON_MAX_DIGITS)
    if K > _lib.COCO_JSON_MAX_K:
        raise ValueError('%d landmarks: a record of the json kernels holds up to %d' % (K, _lib.COCO_JSON_MAX_K))
    img_ids, cat_ids = _json_tables(dataset, N, L)
    lib, dev, cap, clock = _lib.lib(), rows.device, N * M, time.perf_counter
    i32, i64, p = ctypes.c_int32, ctypes.c_int64, _lib.ptr
    with torch.cuda.device(dev):
        stream = _lib.current_stream()
        t0 = clock()
        img_t, cat_t = torch.from_numpy(img_ids).to(dev), torch.from_numpy(cat_ids).to(dev)
        # identity tables: a sample is its own image slot, a label its own column, so no row is dropped for lack of ground truth
        vals, info, img_rows, img_base, _, flags = _order_rows_on_device(
            rows, torch.arange(N, dtype=torch.int32, device=dev), torch.arange(L, dtype=torch.int32, device=dev), L, N * L,
            num_digits, _empty_on(dev))
        lens = torch.zeros((2, cap), dtype=torch.int32, device=dev)
        rec_src = torch.full((cap,), -1, dtype=torch.int64, device=dev)
        _lib.check(lib.kgdet_coco_json_measure(p(rows), i64(N), i32(M), i32(W), p(vals), p(info), p(img_base), p(img_t), p(cat_t),
                                               i32(L), i32(num_digits), p(lens[0]), p(lens[1]), p(rec_src), i64(cap), p(flags),
                                               stream), 'kgdet_coco_json_measure')
        # where record r begins, with the ", " in front of every record but the first: the exclusive scan of len + (r > 0) * 2
        offset = torch.zeros((2, cap + 1), dtype=torch.int64, device=dev)
        offset[:, 1:] = torch.cumsum(lens, dim=1, dtype=torch.int64) + 2 * torch.arange(cap, dtype=torch.int64, device=dev)
        del lens, info
        # the one read-back: both flag words, the number of records, their offsets
        host = torch.cat([flags.to(torch.int64), img_base[-1:] + img_rows[-1:], offset.reshape(-1)]).cpu().numpy()
        bad_value, bad_layout, R = (int(v) for v in host[:3])
        off = host[3:].reshape(2, cap + 1)
        timings['order_measure_s'] = clock() - t0
        _refuse_flags(bad_value, bad_layout, M, num_digits, 'values', '(or rows outside the record table)')
        longest = int(np.diff(off[:, :R + 1], axis=1).max()) if R else 0
        if longest > chunk_bytes:
            raise ValueError('a record of %d bytes does not fit chunk_bytes = %d' % (longest, chunk_bytes))
        size = min(chunk_bytes, max(int(off[:, R].max()), 1))
        d_buf = [torch.empty(size, dtype=torch.uint8, device=dev) for _ in range(2)]
        h_buf = [torch.empty(size, dtype=torch.uint8).pin_memory() for _ in range(2)]
        h_view = [memoryview(b.numpy()) for b in h_buf]
        events = []                                                 # (before kernel, after kernel, after copy) per chunk
        with _TempFiles(files) as tmp:
            for kind, name in enumerate(('bbox', 'keypoints')):
                chunks = _json_chunks(off[kind], R, chunk_bytes)

                def issue(c):
                    r0, r1 = chunks[c]
                    nbytes = int(off[kind, r1] - off[kind, r0])
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                    ev[0].record()
                    _lib.check(lib.kgdet_coco_json_write(i32(kind), p(rows), i64(N), i32(M), i32(W), p(vals), p(rec_src),
                                                         p(offset[kind]), p(img_t), p(cat_t), i32(L), i32(num_digits), i64(r0),
                                                         i64(r1), i64(nbytes), p(d_buf[c % 2]), i64(size), p(flags), stream),
                               'kgdet_coco_json_write')
                    ev[1].record()
                    h_buf[c % 2][:nbytes].copy_(d_buf[c % 2][:nbytes], non_blocking=True)
                    ev[2].record()
                    events.append(ev)
                    return ev[2], nbytes

                with open(tmp.temp[name], 'wb') as f:
                    f.write(b'[')
                    pending = issue(0) if chunks else None
                    for c in range(len(chunks)):
                        done, nbytes = pending
                        pending = issue(c + 1) if c + 1 < len(chunks) else None
                        done.synchronize()
                        t0 = clock()
                        f.write(h_view[c % 2][:nbytes])
                        timings['file_s'] += clock() - t0
                        timings['bytes'] += nbytes
                    f.write(b']')
                    timings['bytes'] += 2
            if int(flags[1]):
                raise RuntimeError('kgdet_coco_json_write: records disagree with their offsets (measure and write differ)')
            tmp.commit()
        for ev in events:
            timings['kernel_s'] += ev[0].elapsed_time(ev[1]) * 1e-3
            timings['copy_s'] += ev[1].elapsed_time(ev[2]) * 1e-3
    return files


def results2json_any(dataset, results, out_file):
    """``evaluation.results2json`` for whatever ``single_gpu_test`` returned: a ``runner.DeviceResults`` takes the device
    route (``write_device_results_json``) and, on its ``ValueError``, ``results2json`` of its ``to_host()`` list with one warning
    that names the reason; a list takes ``results2json`` as it is.  -> the dict of file names"""
    from .evaluation import results2json
    if not _is_device_results(results):
        return results2json(dataset, results, out_file)
    try:
        return write_device_results_json(dataset, results, out_file)
    except ValueError as e:
        import warnings
        warnings.warn('the result files are written on the host instead (the slow route): %s' % e, RuntimeWarning)
        return results2json(dataset, results.to_host(), out_file)
