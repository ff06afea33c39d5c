"""Cost of the input transform under ``extra_aug``, on the workload of tools/time_preprocess.py: 624 x 468 demo images to
1088 x 800 at img_scale (1333, 800), batch 8, 16 host threads.  Prints one JSON line.

One child process under its own ``timeout`` (a failure ends the run, no retries) measures, alternating per repetition in ONE
process from one tree:

* ``aug`` -- ``kgdet_image_preprocess_aug`` with all three augmentations on: every colour stage drawn, an expand to a
  936 x 702 canvas and a 624 x 468 crop that cuts the raw image, so the slot written is the plain launch's 1088 x 800;
  the distortion staged in LDS once per source row (the kernel's default);
* ``aug_per_tap`` -- the same launch with ``KGDET_PREPROC_AUG_STAGE=0``: the distortion computed at every tap;
* ``aug_window_only`` -- the same window without ``photo_metric_distortion`` (what the distortion itself costs);
* ``plain`` -- ``kgdet_image_preprocess`` on the same sources;
* ``host`` -- ``preprocess.image_transform_restatement_aug`` per image with the same plan (the host route of a dataset with
  ``extra_aug``), and ``datasets.ImageTransform`` (the plain host route) beside it.

Kernel times are device events over ``--inner`` back-to-back launches of a prebuilt job table on device-resident sources; the
whole calls (upload included) and the host routes are host clocks, the device ones ending in a synchronise.

python tools/time_augment.py [--reps 10] [--inner 50]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALE = (1333, 800)


def _median(xs):
    import numpy as np
    return float(np.median(xs))


def workload_plan(h, w, colour=True):
    """all three augmentations on, deterministic: the virtual image keeps the raw size"""
    from kgdet_amd import augment
    p = augment.AugPlan(h, w, 0)
    if colour:
        p.colour, p.delta, p.alpha, p.contrast_first, p.sat, p.hue, p.perm = True, -17.25, 1.37, True, 0.81, 11.5, (1, 2, 0)
    p.canvas, p.top, p.left = (h * 3 // 2, w * 3 // 2), h // 6, w // 6
    p.patch = (w // 12, h // 12, w // 12 + w, h // 12 + h)
    return p


def step_measure(a):
    import torch
    from kgdet_amd import datasets, preprocess
    from tests.golden import demo_cases
    assert torch.cuda.is_available(), 'time_augment.py measures the GPU'
    data = demo_cases.demo_dataset(test_mode=True)
    idx = [i for i, info in enumerate(data.img_infos) if (info['height'], info['width']) == (624, 468)]
    raws = [torch.from_numpy(data.load_image(idx[k % len(idx)]).copy()) for k in range(8)]
    B, (h, w) = len(raws), raws[0].shape[:2]
    T = data.device_transform()
    norm = data.img_norm_cfg
    plans = {'aug': [workload_plan(h, w) for _ in raws], 'aug_window_only': [workload_plan(h, w, colour=False) for _ in raws]}
    scales, flips = [SCALE] * B, [False] * B
    size = T.plan(raws[0], SCALE)
    H, W = size[3][:2]
    assert plans['aug'][0].virtual_hw == (h, w)
    dst = torch.empty((B, 3, H, W), dtype=torch.float32, device='cuda')
    dev = [r.cuda() for r in raws]
    dsts = [dst[b] for b in range(B)]
    tables = {k: T.aug_job_tables(dev, [size] * B, flips, dsts, p) for k, p in plans.items()}
    tables['plain'] = T.job_tables(dev, [size] * B, flips, dsts)
    tables['aug_per_tap'], plans['aug_per_tap'] = tables['aug'], plans['aug']
    launch = {k: (T.launch_tables if k == 'plain' else T.launch_aug_tables) for k in tables}

    def variant(k):
        """the library reads the switch at every call"""
        os.environ['KGDET_PREPROC_AUG_STAGE'] = '0' if k == 'aug_per_tap' else '1'

    def kernel(k):
        variant(k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        launch[k](tables[k])
        e0.record()
        for _ in range(a.inner):
            launch[k](tables[k])
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner

    def whole(k):
        variant(k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        T(raws, scales, flips, out=dst, aug_plans=plans.get(k))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    arrays = [r.numpy() for r in raws]
    host_plain = datasets.ImageTransform(size_divisor=data.size_divisor, **norm)
    torch.set_num_threads(16)

    def host(aug):
        t0 = time.perf_counter()
        for arr, p in zip(arrays[:a.host_images], plans['aug']):
            if aug:
                preprocess.image_transform_restatement_aug(arr, p, SCALE, False, True, size_divisor=data.size_divisor, **norm)
            else:
                host_plain(arr, SCALE)
        return (time.perf_counter() - t0) * 1e3 / a.host_images

    acc = {}
    for rep in range(a.warmup + a.reps):
        row = {}
        for k in ('aug', 'plain', 'aug_per_tap', 'aug_window_only'):
            row[k + '_kernel'] = kernel(k)
            row[k + '_whole'] = whole(k)
        row['host_aug'], row['host_plain'] = host(True), host(False)
        if rep >= a.warmup:
            for k, v in row.items():
                acc.setdefault(k, []).append(v)
    os.environ.pop('KGDET_PREPROC_AUG_STAGE')
    out = {'source_hw': [h, w], 'out_hw': [H, W], 'batch': B}
    for k in ('aug', 'aug_per_tap', 'aug_window_only', 'plain'):
        out[k] = {'kernel_us_per_image': round(_median(acc[k + '_kernel']) * 1e3 / B, 2),
                  'kernel_us_per_launch': round(_median(acc[k + '_kernel']) * 1e3, 2),
                  'kernel_us_per_launch_min': round(min(acc[k + '_kernel']) * 1e3, 2),
                  'whole_call_ms_per_image': round(_median(acc[k + '_whole']) / B, 4)}
    out['host_ms_per_image_16_threads'] = {'restatement_aug': round(_median(acc['host_aug']), 2),
                                           'restatement_aug_min': round(min(acc['host_aug']), 2),
                                           'image_transform_plain': round(_median(acc['host_plain']), 2)}
    # the launch computes what the host route computes (one image, bit for bit)
    want = preprocess.image_transform_restatement_aug(arrays[0], plans['aug'][0], SCALE, False, True,
                                                      size_divisor=data.size_divisor, **norm)[0]
    T(raws[:1], scales[:1], flips[:1], out=dst[:1], aug_plans=plans['aug'][:1])
    out['device_equals_host_bits'] = bool(torch.equal(dst[0].cpu().view(torch.int32), torch.from_numpy(want).view(torch.int32)))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--host-images', type=int, default=2)
    ap.add_argument('--step', default=None, choices=['measure'])
    a = ap.parse_args()
    if a.step == 'measure':
        return step_measure(a)
    me = [sys.executable, os.path.abspath(__file__), '--reps', str(a.reps), '--warmup', str(a.warmup), '--inner', str(a.inner),
          '--host-images', str(a.host_images), '--step', 'measure']
    p = subprocess.run(['timeout', '-k', '10', '300'] + me, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        print(json.dumps({'failed_step': {'name': 'measure', 'returncode': p.returncode}}))
        sys.exit(1)
    print(p.stdout.strip().splitlines()[-1])


if __name__ == '__main__':
    main()
