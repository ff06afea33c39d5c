"""Does the feed keep up?  Training and test throughput from a directory of JPEGs, against a resident batch.

    python tools/time_loader.py [--images 256] [--iters 200] [--warmup 20] [--workers 2,4,8,16] [--test-workers 0,4,8,16]
                                [--rounds 2] [--skip-train] [--skip-test] [--legs a,d,e] [--out FILE]

Image set: the records of tests/golden/demo_dataset-32.json, rendered with tests/golden/demo_cases.render_image, repeated
under fresh ids to ``--images`` and saved as JPEG into a temporary directory (sorted by size, so the test loop finds groups).

Training legs -- KGDet config, eager step (``Runner``'s: forward, nine losses, backward, clip, Adam), batch 2, ``--iters``
iterations per leg after ``--warmup``, all in this process, the whole list repeated ``--rounds`` times in the same order:

    a       one resident synthetic batch (bench.py's situation): the ceiling for that shape
    a_real  16 resident batches of the image set, cycled: the ceiling for the set's own shapes
    b       the serial loop: ``collate([dataset[i] ...])`` and ``.cuda()`` between steps
    c<N>    ``build_dataloader(..., device='cuda')``, host route (pixels on the host, uploaded from page-locked memory), N threads
    d<N>    the same with ``device_preprocess=True`` (raw pixels up, one preprocess launch per batch)
    e<N>    the same with ``device_decode=True`` as well (the files' bytes up, one decode call and one preprocess launch per
            batch); it runs right behind d<N>, so the two alternate over the rounds

each with ``data_time``, the mean seconds per iteration spent in the feed's ``next()``.  ``--legs``: only the legs whose name
begins with one of these prefixes.  Test legs -- bf16 autocast, ``imgs_per_gpu=8``, ``device_preprocess`` and
``device_results`` on: ``single_gpu_test`` at each ``--test-workers``, images per second; at ``workers`` 0 and 4 also with
``device_decode=True`` (``w<N>_decode``), right behind the leg without.  ``single_gpu_test`` reports no feed time, so the
tool clocks it from outside: a test leg's ``data_time`` is the seconds per IMAGE its loop's thread spent getting samples
(``prepare_test_raw`` inline or the wait for a prefetched one) and inside the decode route's call.

MIOpen's find mode is off (``cudnn.benchmark = False``) for every leg: the image set has many padded shapes, and a find per
new shape would be timed as feed.  Prints one JSON line (also written to ``--out``): per leg the img/s of every round, their
mean and spread, ``data_time``, and the ratios to ``a`` and ``a_real``; the CPUs this process may use."""
import argparse
import itertools
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def render_image_dir(root, count):
    from PIL import Image
    from tests.golden import demo_cases
    with open(demo_cases.ANN) as f:
        base = json.load(f)
    anns_of = {}
    for a in base['annotations']:
        anns_of.setdefault(a['image_id'], []).append(a)
    os.makedirs(os.path.join(root, 'image'), exist_ok=True)
    rendered = {}
    for k, im in enumerate(base['images']):
        path = os.path.join(root, 'image', 'src_%02d.jpg' % k)
        Image.fromarray(demo_cases.render_image(im, anns_of.get(im['id'], []), seed=1000 + k)).save(path, quality=90)
        rendered[im['id']] = path
    images, anns, next_ann = [], [], 1
    for n in range(count):
        src = base['images'][n % len(base['images'])]
        name = '%06d.jpg' % (n + 1)
        shutil.copyfile(rendered[src['id']], os.path.join(root, 'image', name))
        images.append(dict(src, id=n + 1, file_name=name))
        for a in anns_of.get(src['id'], []):
            anns.append(dict(a, id=next_ann, image_id=n + 1))
            next_ann += 1
    images.sort(key=lambda im: (im['height'], im['width'], im['id']))
    ann_file = os.path.join(root, 'set.json')
    with open(ann_file, 'w') as f:
        json.dump(dict(images=images, annotations=anns, categories=base['categories']), f)
    return ann_file, os.path.join(root, 'image') + os.sep


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=256)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--workers', default='2,4,8,16')
    ap.add_argument('--test-workers', default='0,4,8,16')
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--skip-train', action='store_true')
    ap.add_argument('--skip-test', action='store_true')
    ap.add_argument('--legs', default=None, help='only the training legs whose names begin with one of these prefixes')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), 'tools/time_loader.py needs a GPU'
    from kgdet_amd import configs, synthetic
    from kgdet_amd import datasets as ds
    from kgdet_amd import runner as rn
    from kgdet_amd.dist import DistOptimizerHook
    from kgdet_amd.loader import build_dataloader
    from kgdet_amd.registry import build_detector
    from tests.golden import demo_cases

    device = torch.device('cuda', 0)
    torch.backends.cudnn.benchmark = False
    tmp = tempfile.mkdtemp(prefix='kgdet_feed_')
    try:
        t0 = time.time()
        ann_file, prefix = render_image_dir(tmp, args.images)
        common = dict(ann_file=ann_file, img_prefix=prefix, img_scale=demo_cases.IMG_SCALE, img_norm_cfg=demo_cases.IMG_NORM,
                      size_divisor=32, with_mask=False, with_crowd=False, with_keypoint=True)
        train_set = ds.DeepFashion2Dataset(flip_ratio=0.5, with_label=True, **common)
        test_set = ds.DeepFashion2Dataset(flip_ratio=0, with_label=False, test_mode=True, **common)
        out = dict(images=args.images, iters=args.iters, warmup=args.warmup, rounds=args.rounds, batch=2,
                   cpus_usable=len(os.sched_getaffinity(0)), cpus_machine=os.cpu_count(), miopen_find=False,
                   side_stream='the device_decode route only', render_s=round(time.time() - t0, 1))

        cfg = configs.kgdet_r50_fpn()
        torch.manual_seed(0)
        model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).to(device)
        workers = [int(w) for w in args.workers.split(',') if w]

        if not args.skip_train:
            model.train()
            optimizer = rn.build_optimizer(model, cfg.optimizer)
            hook = DistOptimizerHook(**cfg.optimizer_config)

            def step(data):
                res = rn.batch_processor(model, data, train_mode=True)
                hook.step(model, optimizer, res['loss'])

            def epochs(loader):
                while True:
                    for batch in loader:
                        yield batch

            def serial():
                while True:
                    order = list(ds.GroupSampler(train_set, 2))
                    for k in range(0, len(order), 2):
                        batch = ds.collate([train_set[i] for i in order[k:k + 2]])
                        batch['img'] = batch['img'].cuda()
                        for key in ('gt_bboxes', 'gt_labels', 'gt_keypoints'):
                            batch[key] = [t.cuda() for t in batch[key]]
                        yield batch

            def timed(feed):
                for _ in range(args.warmup):
                    step(next(feed))
                torch.cuda.synchronize()
                start, waited = time.time(), 0.0
                for _ in range(args.iters):
                    t = time.time()
                    data = next(feed)
                    waited += time.time() - t
                    step(data)
                torch.cuda.synchronize()
                return 2 * args.iters / (time.time() - start), waited / args.iters

            synth = synthetic.make_batch(2, device, seed=0)
            synth = dict(img=synth['img'], img_meta=synth['img_meta'], gt_bboxes=synth['gt_bboxes'],
                         gt_labels=synth['gt_labels'], gt_keypoints=synth['gt_keypoints'])
            np.random.seed(0)
            resident = list(itertools.islice(iter(build_dataloader(train_set, 2, 4, device=device, device_preprocess=True)), 16))
            legs = [('a', lambda: itertools.repeat(synth)), ('a_real', lambda: itertools.cycle(resident)), ('b', serial)]
            for w in workers:
                legs.append(('c%d' % w, lambda w=w: epochs(build_dataloader(train_set, 2, w, device=device))))
            for w in workers:
                legs.append(('d%d' % w, lambda w=w: epochs(build_dataloader(train_set, 2, w, device=device,
                                                                            device_preprocess=True))))
                legs.append(('e%d' % w, lambda w=w: epochs(build_dataloader(train_set, 2, w, device=device,
                                                                            device_preprocess=True, device_decode=True))))
            if args.legs:
                wanted = tuple(p for p in args.legs.split(',') if p)
                legs = [leg for leg in legs if leg[0] == 'a' or leg[0].startswith(wanted)]
            train = {name: dict(img_s=[], data_time=[]) for name, _ in legs}
            for _ in range(args.rounds):
                for name, make in legs:
                    feed = make()
                    rate, waited = timed(feed)
                    if hasattr(feed, 'close'):
                        feed.close()              # (a generator: leaving it ends the loader's threads)
                    del feed
                    train[name]['img_s'].append(round(rate, 1))
                    train[name]['data_time'].append(round(waited, 5))
                    print('train %s: %.1f img/s, data_time %.2f ms' % (name, rate, waited * 1e3), file=sys.stderr, flush=True)
            for name, rec in train.items():
                rec['mean'] = round(float(np.mean(rec['img_s'])), 1)
                rec['spread'] = round((max(rec['img_s']) - min(rec['img_s'])) / rec['mean'], 4)
            for name, rec in train.items():
                rec['vs_a'] = round(rec['mean'] / train['a']['mean'], 3)
                if 'a_real' in train:
                    rec['vs_a_real'] = round(rec['mean'] / train['a_real']['mean'], 3)
            out['train'] = train
            del optimizer, hook, resident, synth

        if not args.skip_test:
            model.eval()
            test_workers = [int(w) for w in args.test_workers.split(',') if w]
            test_legs = [(w, decode) for w in test_workers for decode in ((False, True) if w in (0, 4) else (False,))]
            test = {'w%d%s' % (w, '_decode' if decode else ''): dict(img_s=[], data_time=[]) for w, decode in test_legs}

            # ``single_gpu_test`` reports no feed time of its own, so the tool clocks the calls its loop makes for samples ON THE
            # LOOP'S THREAD: ``prepare_test_raw`` / ``load_image_file`` inline (workers 0), the wait for a prefetched sample, and
            # the decode route's call (upload, decode, status read-back, PIL for a refused file)
            import threading
            from kgdet_amd import jpeg
            loop_thread, fed = threading.get_ident(), [0.0]

            def clocked(fn):
                def inner(*a, **kw):
                    if threading.get_ident() != loop_thread:
                        return fn(*a, **kw)
                    t = time.time()
                    try:
                        return fn(*a, **kw)
                    finally:
                        fed[0] += time.time() - t
                return inner

            test_set.prepare_test_raw = clocked(test_set.prepare_test_raw)
            test_set.load_image_file = clocked(test_set.load_image_file)
            rn._Prefetched.__call__ = clocked(rn._Prefetched.__call__)
            jpeg.DeviceDecodeRoute.__call__ = clocked(jpeg.DeviceDecodeRoute.__call__)

            def test_run(w, dataset, decode=False):
                with torch.autocast('cuda', dtype=torch.bfloat16):
                    res = rn.single_gpu_test(model, dataset, imgs_per_gpu=8, device_preprocess=True, device_results=True,
                                             workers=w, device_decode=decode)
                torch.cuda.synchronize()
                return res

            test_run(4, test_set)                         # warm-up: every shape of the set once
            test_run(4, test_set, True).release()
            for _ in range(args.rounds):
                for w, decode in test_legs:
                    torch.cuda.synchronize()
                    start, fed[0] = time.time(), 0.0
                    test_run(w, test_set, decode).release()
                    rate = len(test_set) / (time.time() - start)
                    rec = test['w%d%s' % (w, '_decode' if decode else '')]
                    rec['img_s'].append(round(rate, 1))
                    rec['data_time'].append(round(fed[0] / len(test_set), 6))
                    print('test workers=%d%s: %.1f img/s, data_time %.3f ms per image'
                          % (w, ' device_decode' if decode else '', rate, fed[0] / len(test_set) * 1e3), file=sys.stderr, flush=True)
            for name, rec in test.items():
                rec['mean'] = round(float(np.mean(rec['img_s'])), 1)
                rec['spread'] = round((max(rec['img_s']) - min(rec['img_s'])) / rec['mean'], 4)
            if 'w0' in test:
                for name, rec in test.items():
                    rec['vs_w0'] = round(rec['mean'] / test['w0']['mean'], 3)
            out['test'] = test
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return out


if __name__ == '__main__':
    main()
