"""Time the packed (device) evaluator against evaluation.CocoEvaluator on the same detections.

    python tools/time_eval.py [--images N] [--dets P] [--device cuda|cpu] [--types bbox,keypoints] [--no-host]
                              [--lazy-landmarks] [--device-accumulate] [--device-results]

A validation set of N images is built from the committed demo annotations (tests/golden/demo_dataset-32.json replicated
under fresh image / annotation ids); every image gets P detections in the form ``single_gpu_test`` returns them (per class
float32 boxes [n, 5], scores, landmarks [n, 882]): jittered copies of its ground truths and false positives with random
categories and scores (seeded).  Device route, as the validation hook runs it: ``pack_test_results`` (both types at once),
then per type ``evaluate`` (upload, similarity + matching, download) and ``accumulate``.  Host route, as ``coco_eval`` runs it
minus the file: ``kpt2json``, then per type ``load_results``, ``CocoEvaluator.evaluate``, ``accumulate``.  The ``stats`` must
be equal.  ``--no-host`` leaves the host route out (it holds every detection as a dict of Python floats: about 30 kB per
landmark detection).  ``--lazy-landmarks`` / ``--device-accumulate`` (a CUDA device): the device route is run a second time
with the landmark rounding (``kgdet_coco_pack_landmarks``) and / or ``accumulate`` (``kgdet_coco_accumulate``) on the GPU and
reported as ``device_route``; the first run, with both off, becomes ``old_route``, and the ``stats`` of the two must be equal.
``--device-results`` (a CUDA device): the same detections are also built directly as the ``[N, M, 7 + 3K]`` device tensor a
``single_gpu_test(..., device_results=True)`` run leaves behind and packed where they lie (``pack_device_results``:
``kgdet_coco_order_dets`` / ``kgdet_coco_scatter_dets``), with lazy landmarks and ``--device-accumulate`` as given; reported as
``device_results_route`` with the same phases and the peak device memory, ``stats`` equal to the other routes'.
Prints one JSON line with seconds per stage, totals, milliseconds per image and host / device ratios."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgdet_amd import evaluation as ev  # noqa: E402
from kgdet_amd import evaluation_device as evd  # noqa: E402

GT = os.path.join(ROOT, 'tests', 'golden', 'demo_dataset-32.json')


class Dataset(object):
    def __init__(self, coco):
        self.coco, self.img_ids, self.cat_ids = coco, coco.get_img_ids(), coco.get_cat_ids()

    def __len__(self):
        return len(self.img_ids)


def build(n_images, n_dets, seed=0, rows_out=None):
    """(annotation dict, results): results[i] = (boxes per class, scores per class, landmarks per class), float32.
    ``rows_out(n, det, label, kpt)``: also handed every image's detections before they are split by class, in row order"""
    with open(GT) as f:
        base = json.load(f)
    rng = np.random.default_rng(seed)
    by_img = {}
    for a in base['annotations']:
        by_img.setdefault(a['image_id'], []).append(a)
    cat_ids = [c['id'] for c in base['categories']]
    label_of = {c: i for i, c in enumerate(cat_ids)}
    n_cls = len(cat_ids)
    gt = dict(images=[], annotations=[], categories=base['categories'])
    proto = {}
    for img_id, anns in by_img.items():
        proto[img_id] = (np.array([a['bbox'] for a in anns], np.float64), np.array([a['keypoints'] for a in anns], np.float64),
                         np.array([a['area'] for a in anns], np.float64), np.array([label_of[a['category_id']] for a in anns]))
    results = []
    n_jit = (2 * n_dets) // 3
    for n in range(n_images):
        im = dict(base['images'][n % len(base['images'])])
        anns = by_img.get(im['id'], [])
        src = im['id']
        im['id'] = n + 1
        gt['images'].append(im)
        for a in anns:
            a = dict(a)
            a['id'], a['image_id'] = len(gt['annotations']) + 1, n + 1
            gt['annotations'].append(a)
        W, H = im['width'], im['height']
        box = np.stack([rng.uniform(0, W / 2, n_dets), rng.uniform(0, H / 2, n_dets), rng.uniform(10, W / 2, n_dets),
                        rng.uniform(10, H / 2, n_dets)], axis=1)                       # false positives, xywh
        kpt = np.zeros((n_dets, 294, 3), np.float32)
        sel = rng.integers(0, 294, (n_dets, 20))
        rows = np.arange(n_dets)[:, None]
        kpt[rows, sel, 0], kpt[rows, sel, 1], kpt[rows, sel, 2] = rng.uniform(0, W, (n_dets, 20)), rng.uniform(0, H, (n_dets, 20)), 1.0
        label = rng.integers(0, n_cls, n_dets)
        if anns and n_jit:                                                           # jittered ground truths, some under a wrong category
            gb, gk, ga, gl = proto[src]
            pick = np.arange(n_jit) % len(anns)
            noise = rng.choice([0.01, 0.05, 0.15, 0.4], n_jit)
            b = gb[pick] + rng.normal(0, 1, (n_jit, 4)) * noise[:, None] * gb[pick][:, [2, 3, 2, 3]]
            b[:, 2:] = np.maximum(b[:, 2:], 1.0)
            box[:n_jit] = b
            k = gk[pick].reshape(n_jit, 294, 3).astype(np.float32)
            jitter = rng.standard_normal((n_jit, 294, 2), dtype=np.float32) * (noise * 0.3 * np.sqrt(ga[pick]))[:, None, None].astype(np.float32)
            k[:, :, :2] += jitter * (k[:, :, 2:3] > 0)
            kpt[:n_jit] = k
            keep_cat = rng.random(n_jit) > 0.15
            label[:n_jit] = np.where(keep_cat, gl[pick], label[:n_jit])
        det = np.concatenate([box[:, :2], box[:, :2] + box[:, 2:] - 1, rng.random((n_dets, 1))], axis=1).astype(np.float32)
        kpt = kpt.reshape(n_dets, 882)
        if rows_out is not None:
            rows_out(n, det, label, kpt)
        order = np.argsort(label, kind='mergesort')
        cut = np.searchsorted(label[order], np.arange(n_cls + 1))
        dets = [det[order[cut[c]:cut[c + 1]]] for c in range(n_cls)]
        results.append((dets, [d[:, 4] for d in dets], [kpt[order[cut[c]:cut[c + 1]]] for c in range(n_cls)]))
    return gt, results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=256)
    ap.add_argument('--dets', type=int, default=100)
    ap.add_argument('--device', default=None)
    ap.add_argument('--types', default='bbox,keypoints')
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--lazy-landmarks', action='store_true')
    ap.add_argument('--device-accumulate', action='store_true')
    ap.add_argument('--device-results', action='store_true')
    args = ap.parse_args()
    device = args.device or evd._default_device()
    types = args.types.split(',')
    clock = time.perf_counter
    t0 = clock()
    rows_out = rows = None
    if args.device_results:
        import torch
        rows = torch.empty((args.images, args.dets, 7 + 882), dtype=torch.float32, device=device)
        stage = torch.empty((256,) + tuple(rows.shape[1:]), dtype=torch.float32)

        def rows_out(n, det, label, kpt):                         # (staged 256 images at a time: no second host copy of the set)
            block = stage[n % 256].numpy()
            block[:, :5], block[:, 5], block[:, 6], block[:, 7:] = det, label, len(det), kpt
            if n % 256 == 255 or n == args.images - 1:
                rows[n - n % 256:n + 1].copy_(stage[:n % 256 + 1])
    gt, results = build(args.images, args.dets, rows_out=rows_out)
    index = ev.CocoIndex(gt)
    data = Dataset(index)
    out = dict(images=args.images, dets_per_image=args.dets, device=str(device), build_s=round(clock() - t0, 3))
    t0 = clock()
    packed_gt = evd.pack_ground_truth(index)
    out['pack_ground_truth_s'] = round(clock() - t0, 4)
    evd.evaluate_packed(packed_gt, evd.pack_results(packed_gt, []), 'bbox', device)     # context, library load, first launches

    def device_route(lazy, dev_acc, dev_results=None):
        if dev_acc or dev_results is not None:
            import torch
        dev = dict()
        t0 = clock()
        if dev_results is not None:
            on_gpu = dev_results.rows.is_cuda                                    # (CPU rows: the numpy restatement, for checks)
            if on_gpu:
                torch.cuda.reset_peak_memory_stats()
            packed = evd.pack_device_results(packed_gt, data, dev_results)       # (its downloads wait for the kernels)
            dev_results.release()
        else:
            packed = evd.pack_test_results(packed_gt, data, results, lazy_landmarks=lazy)
        dev['pack_s'] = clock() - t0
        got = {}
        for typ in types:
            t0 = clock()
            e = evd.DeviceCocoEvaluator(packed_gt, packed[typ], typ, device=device, device_accumulate=dev_acc).evaluate()
            if dev_acc:
                torch.cuda.synchronize()                            # (nothing is downloaded here: wait for the launches)
            t1 = clock()
            e.accumulate()
            t2 = clock()
            got[typ] = e.summarize(verbose=False)
            dev[typ] = dict(kept_detections=int(len(packed[typ].score)), match_s=t1 - t0, accumulate_s=t2 - t1)
        dev['total_s'] = dev['pack_s'] + sum(dev[t]['match_s'] + dev[t]['accumulate_s'] for t in types)
        dev['ms_per_image'] = 1e3 * dev['total_s'] / args.images
        if dev_results is not None and on_gpu:
            dev['peak_device_gb'] = torch.cuda.max_memory_allocated() / 1e9
        return dev, got

    dev, got = device_route(False, False)                      # the route with packing and accumulate on the host
    if args.lazy_landmarks or args.device_accumulate:
        out['old_route'] = dev
        dev, new = device_route(args.lazy_landmarks, args.device_accumulate)
        dev['lazy_landmarks'], dev['device_accumulate'] = args.lazy_landmarks, args.device_accumulate
        for typ in types:
            assert np.array_equal(new[typ], got[typ]), (typ, new[typ], got[typ])
        out['ratio_old_new'] = out['old_route']['total_s'] / dev['total_s']
    out['device_route'] = dev
    if args.device_results:
        from kgdet_amd.runner import DeviceResults
        held, rows = DeviceResults(rows, len(data.cat_ids) + 1), None          # (released once packed, as evaluate_results does)
        dres, new = device_route(True, args.device_accumulate, held)
        dres['device_accumulate'] = args.device_accumulate
        for typ in types:
            assert np.array_equal(new[typ], got[typ]), (typ, new[typ], got[typ])
        out['device_results_route'] = dres
        out['ratio_pack'] = dev['pack_s'] / dres['pack_s']
    if not args.no_host:
        host = dict()
        t0 = clock()
        boxes, kpts = ev.kpt2json(data, results)
        host['kpt2json_s'] = clock() - t0
        for typ, res in (('bbox', boxes), ('keypoints', kpts)):
            if typ not in types:
                continue
            t0 = clock()
            dt = index.load_results(res)
            t1 = clock()
            h = ev.CocoEvaluator(index, dt, typ)
            h.params.img_ids = index.get_img_ids()
            h.evaluate()
            t2 = clock()
            h.accumulate()
            t3 = clock()
            want = h.summarize(verbose=False)
            assert np.array_equal(got[typ], want), (typ, got[typ], want)
            host[typ] = dict(load_results_s=t1 - t0, match_s=t2 - t1, accumulate_s=t3 - t2)
        host['total_s'] = host['kpt2json_s'] + sum(sum(host[t].values()) for t in types)
        host['ms_per_image'] = 1e3 * host['total_s'] / args.images
        out['host_route'] = host
        out['ratio_total'] = host['total_s'] / dev['total_s']
        out['ratio_match'] = {t: host[t]['match_s'] / dev[t]['match_s'] for t in types}
    out['mAP'] = {t: float(got[t][0]) for t in types}

    def tidy(v):
        if isinstance(v, dict):
            return {k: tidy(x) for k, x in v.items()}
        return round(v, 4) if isinstance(v, float) else v
    print(json.dumps(tidy(out)))


if __name__ == '__main__':
    main()
